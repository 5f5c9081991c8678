"""Exact PSSM checker on the square-matrix oracle (no change to oracle/).

The oracle takes any size x size matrix and a 256-entry mapper.  A PSSM of L rows over a reference alphabet of A symbols becomes
a square matrix of size L + A: query position i gets a byte code of its own (mapped to row i), reference symbol c maps to column
L + c, and M[i][L + c] = pssm[i][c].  The oracle then runs the exact PSSM recurrence: scores, end cells, `similar`, `length` and
the path.  Only `matches` and the = / X letters differ (the encoded query bytes never equal a reference letter); they are
recomputed along the oracle's path from the mapped symbols of the real letters, as the library counts them."""
import re

import numpy as np

MAX_ROWS = 200


def _query_codes(L, ref_bytes):
    """L distinct byte codes that are neither 0 nor any byte a reference may hold."""
    taken = set(int(b) for b in ref_bytes) | {0}
    codes = [c for c in range(1, 256) if c not in taken]
    assert len(codes) >= L, "PSSM too long for the byte encoding"
    return np.array(codes[:L], dtype=np.uint8)


def encode(orc, pssm, ref_mapper, ref_bytes):
    """pssm: int [L, A]; ref_mapper: the real matrix's 256-entry mapper (reference byte -> column c < A).  Returns (oracle
    Matrix, encoded query bytes)."""
    pssm = np.asarray(pssm, dtype=np.int32)
    L, A = pssm.shape
    assert L <= MAX_ROWS
    codes = _query_codes(L, ref_bytes)
    M = np.zeros((L + A, L + A), dtype=np.int32)
    M[:L, L:] = pssm
    mp = np.full(256, L + A - 1, dtype=np.int32)
    for b in ref_bytes:
        mp[int(b)] = L + int(ref_mapper[int(b)])
    for i, c in enumerate(codes):
        mp[int(c)] = i
    return orc.Matrix(M, mp), codes.tobytes()


def _fix_cigar(text, bq, br, q, r, mapper):
    """The oracle's path with = / X from the mapped real letters; returns (text, matches)."""
    runs, i, j, matches = [], bq, br, 0
    for n, op in re.findall(r"(\d+)([=XID])", text):
        n = int(n)
        if op in "=X":
            for _ in range(n):
                eq = mapper[q[i]] == mapper[r[j]]
                matches += int(eq)
                letter = "=" if eq else "X"
                if runs and runs[-1][1] == letter and runs[-1][2]:
                    runs[-1][0] += 1
                else:
                    runs.append([1, letter, True])
                i += 1; j += 1
        else:
            runs.append([n, op, False])
            if op == "I":
                i += n
            else:
                j += n
    return "".join("%d%s" % (n, op) for n, op, _ in runs), matches


def check(orc, mode, sg_flags, pssm, ref_mapper, alphabet_bytes, queries, refs, open_, ext, with_cigar=True):
    """Every pair (queries[k] of the PSSM's length, refs[k]) through the encoded oracle.  Returns int32 [n, 6] (score,
    end_query, end_ref, matches, similar, length) and, with_cigar, the CIGAR texts with begin cells."""
    om, qcode = encode(orc, pssm, ref_mapper, alphabet_bytes)
    n = len(refs)
    qb, qo = orc.pack([qcode] * n)
    rb, ro = orc.pack(refs)
    idx = np.arange(n)
    st = orc.align_stats_sample(mode, idx, qb, qo, rb, ro, open_, ext, om, sg_flags=sg_flags, bits=32)
    out = st[:, :6].copy()
    texts = None
    if with_cigar:
        raw, rec = orc.cigar_sample(mode, idx, qb, qo, rb, ro, open_, ext, om, sg_flags=sg_flags)
        texts = []
        for k in range(n):
            t, m = _fix_cigar(raw[k], int(rec[k, 3]), int(rec[k, 4]), queries[k], refs[k], ref_mapper)
            texts.append(t)
    # matches along the statistics path (the same path as the traceback's: the coupled tables follow its decisions)
    if with_cigar:
        for k in range(n):
            out[k, 3] = sum(int(a) for a, op in re.findall(r"(\d+)([=XID])", texts[k]) if op == "=")
    else:
        raw, rec = orc.cigar_sample(mode, idx, qb, qo, rb, ro, open_, ext, om, sg_flags=sg_flags)
        for k in range(n):
            out[k, 3] = _fix_cigar(raw[k], int(rec[k, 3]), int(rec[k, 4]), queries[k], refs[k], ref_mapper)[1]
    return out, texts


def random_pssm(rng, L, A, lo=-6, hi=9):
    return rng.integers(lo, hi + 1, size=(L, A)).astype(np.int32)
