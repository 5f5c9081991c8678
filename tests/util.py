"""Shared helpers for the parity tests (seeded synthetic inputs, score-from-CIGAR recomputation)."""
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
AA = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)


def golden(name):
    """Path of a stored fixture under tests/golden/, whatever the working directory."""
    return os.path.join(GOLDEN, name)


def random_seqs(rng, n, lo, hi, alphabet=DNA):
    lens = rng.integers(lo, hi + 1, size=n)
    return [alphabet[rng.integers(0, len(alphabet), size=int(l))].tobytes() for l in lens]


def mutate(rng, seq, sub=0.10, indel=0.02, alphabet=DNA):
    """related-pair generator: substitutions and single-base indels."""
    out = bytearray()
    for c in seq:
        u = rng.random()
        if u < indel / 2:
            continue                                   # deletion
        if u < indel:
            out.append(int(alphabet[rng.integers(0, len(alphabet))]))   # insertion
        if rng.random() < sub:
            out.append(int(alphabet[rng.integers(0, len(alphabet))]))
        else:
            out.append(c)
    return bytes(out) if out else bytes(seq[:1])


def cigar_ops(text):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", text)]


def score_from_cigar(text, q, r, bq, br, scores, mapper, open_, ext):
    """Re-derive the alignment score from a CIGAR (I consumes the query, D the reference)."""
    i, j, s = bq, br, 0
    for n, op in cigar_ops(text):
        if op in "=X":
            for _ in range(n):
                s += int(scores[mapper[q[i]], mapper[r[j]]])
                i += 1; j += 1
        else:
            s -= open_ + (n - 1) * ext
            if op == "I":
                i += n
            else:
                j += n
    return s, i, j


B62_LETTERS = b"ARNDCQEGHILKMFPSTWYVBZX*"


def consensus_pssm(rng, L, top, bottom, lo=-6, hi=9, by_letter=None):
    """A 24-letter PSSM (BLOSUM62's alphabet) whose every row holds `top` in its consensus column (one of the 20 amino acids) and
    `bottom` under '*'; the rest is random in lo .. hi.  by_letter (a query of L letters): rows of equal query letters are equal --
    the PSSM of a square matrix, which the square oracle scores at any length (the byte-encoded PSSM checker ends at 200 rows).
    Returns (int32 [L, 24], the consensus sequence, the square matrix or None)."""
    if by_letter is None:
        vals = rng.integers(lo, hi + 1, size=(L, 24)).astype(np.int32)
        cons = rng.integers(0, 20, size=L)
        square = None
    else:
        square = rng.integers(lo, hi + 1, size=(24, 24)).astype(np.int32)
        perm = rng.permutation(20)                                   # letter a's consensus column (need not be a)
        idx = np.array([B62_LETTERS.index(bytes([c])) for c in by_letter])
        square[np.arange(20), perm] = top
        square[:, 23] = bottom
        vals, cons = square[idx].copy(), perm[idx]
    vals[np.arange(L), cons] = top
    vals[:, 23] = bottom
    return vals, bytes(B62_LETTERS[c] for c in cons), square


# ---- the edges of a packed kernel's host-side proof, found by launching (tests/test_gpu_nwsg_proof_edges.py, test_gpu_stats_window_edges.py) ----
def window_hint(pkg, qlen, msize, smin, smax, open_, ext, rowx=1, rows=0):
    """the longest reference the window hook (pmx_window_nwsgv) admits: where the search by launching looks first"""
    import ctypes as C
    pkg.lib.pmx_window_nwsgv.restype = C.c_int
    lo, hi = 0, 30000
    while hi - lo > 0:
        mid = (lo + hi + 1) // 2
        ok = pkg.lib.pmx_window_nwsgv(int(qlen), int(mid), int(msize), int(smin), int(smax), int(open_), int(ext), int(rowx), int(rows))
        lo, hi = (mid, hi) if ok else (lo, mid - 1)
    return lo


def longest_by_launch(fast, hint=0):
    """The longest reference for which fast(rlen) holds -- a launch, pmx_last_kernel() tells whether the packed kernel ran.  The
    hint is tried first (two launches when it is right: taken at `hint`, not taken one beyond); bisection otherwise.
    A kernel that is never taken is a failure, not a skip."""
    assert fast(1), "the packed kernel did not take a reference of one letter"
    if hint >= 1 and fast(hint) and not fast(hint + 1):
        return hint
    lo, hi = 1, 30001                                                # (no packed kernel takes more than 30 000 columns)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fast(mid) else (lo, mid)
    return lo


def families(rng, q, rlen, alphabet=AA, hot=b"W", cold=b"*"):
    """the references that stretch the value range for query q: the hottest letter throughout (poly-W against poly-W when q is),
    q repeated, q behind a long unrelated prefix, q in front of a long suffix, the coldest letter throughout, random"""
    far = random_seqs(rng, 1, rlen, rlen, alphabet)[0]
    return [hot * rlen, (q * (rlen // len(q) + 1))[:rlen], far[:rlen - len(q)] + q if rlen > len(q) else far,
            q + far[:rlen - len(q)] if rlen > len(q) else far, cold * rlen, far]


def tile(seqs, n):
    return [seqs[i % len(seqs)] for i in range(n)]


def edge_lengths(longest):
    """the longest reference a kernel takes, one short of it, half of it"""
    return [longest, max(1, longest - 1), max(1, longest // 2)]
