"""Reference model of protein seeding (include/parasail_amd.h "Protein seeding") in plain Python: the alphabets, keys from a
table, the index as a sorted list, the orientations and matches of every query mode, both diagonal rules, both window rules and the
order -- and, beside it, a brute-force matcher that compares group letters position by position and never forms a key.  Sequences
are bytes.  Clusters are seed_ref's, the translation is translate_ref's."""
import numpy as np

from seed_ref import PAIR_DTYPE, SEED_HIT_DTYPE, clusters
from translate_ref import CODE_STD, FRAMES_ALL, FRAMES_FORWARD, FRAMES_REVERSE, frames_of, tlen, translate

QUERY_LETTERS, CODONS_FORWARD, CODONS_REVERSE, CODONS_BOTH = -1, 9, 10, 11
MODES = (QUERY_LETTERS, 0, 1, 2, 3, 4, 5, FRAMES_FORWARD, FRAMES_REVERSE, FRAMES_ALL, CODONS_FORWARD, CODONS_REVERSE, CODONS_BOTH)
AA20 = ["A", "C", "D", "E", "F", "G", "H", "I", "K", "L", "M", "N", "P", "Q", "R", "S", "T", "V", "W", "Y"]
AA11 = ["KREDQN", "C", "G", "H", "ILV", "M", "F", "Y", "W", "P", "STA"]


def table_of(groups):
    """groups of letters -> the 256-byte table: group number per byte in either case, 255 = invalid"""
    t = np.full(256, 255, dtype=np.uint8)
    for g, letters in enumerate(groups):
        for c in letters:
            t[ord(c.upper())] = t[ord(c.lower())] = g
    return t


def bits_of(table):
    """bits per letter: ceil(log2 G), G = the largest group + 1"""
    groups = int(max(int(v) for v in table if v != 255)) + 1
    bits = 1
    while (1 << bits) < groups:
        bits += 1
    return bits


def kmers(seq, k, table):
    """[(pos, key)] of the k-mers of seq: all k letters valid, `bits` bits per letter, first letter most significant"""
    bits = bits_of(table)
    out = []
    seq = bytes(seq)
    for j in range(len(seq) - k + 1):
        key = 0
        for c in seq[j:j + k]:
            g = int(table[c])
            if g == 255:
                break
            key = (key << bits) | g
        else:
            out.append((j, key))
    return out


def empty_key(k, table):
    return 1 << (k * bits_of(table))


def index_entries(refs, k, table):
    """the index: (kmer, seq, pos) of every k-mer of the set, ascending"""
    return sorted((key, r, j) for r, s in enumerate(refs) for j, key in kmers(s, k, table))


def index_dict(refs, k, table):
    d = {}
    for key, r, j in index_entries(refs, k, table):
        d.setdefault(key, []).append((r, j))
    return d


def orientations(mode):
    """[(byte, [frames])] of a query mode; the letters mode's one orientation has the frame None"""
    if mode == QUERY_LETTERS:
        return [(0, [None])]
    if mode in (CODONS_FORWARD, CODONS_REVERSE, CODONS_BOTH):
        strands = {CODONS_FORWARD: (0,), CODONS_REVERSE: (1,), CODONS_BOTH: (0, 1)}[mode]
        return [(s, [3 * s, 3 * s + 1, 3 * s + 2]) for s in strands]
    return [(f, [f]) for f in frames_of(mode)]


def is_codon_mode(mode):
    return mode in (CODONS_FORWARD, CODONS_REVERSE, CODONS_BOTH)


def letters_of(query, frame, code=CODE_STD):
    """the letters of an orientation: the row itself, or its translation in the frame"""
    return bytes(query) if frame is None else translate(bytes(query), frame, code)


def key_matches(idx, k, table, max_occ):
    """a matcher from the index: letters -> [(p, r, j)], k-mers above max_occ entries ignored"""
    def fn(letters):
        out = []
        for p, key in kmers(letters, k, table):
            occ = idx.get(key, ())
            if len(occ) <= max_occ:
                out += [(p, r, j) for r, j in occ]
        return out
    return fn


def brute_matches(refs, k, table, max_occ):
    """a matcher that compares group letters position by position; the occurrences are counted the same way over the whole set"""
    refs = [bytes(s) for s in refs]

    def same(a, p, b, j):
        if p + k > len(a) or j + k > len(b):
            return False
        for x in range(k):
            u, v = int(table[a[p + x]]), int(table[b[j + x]])
            if u == 255 or v == 255 or u != v:
                return False
        return True

    def fn(letters):
        out = []
        for p in range(len(letters) - k + 1):
            found = [(r, j) for r, s in enumerate(refs) for j in range(len(s) - k + 1) if same(letters, p, s, j)]
            if len(found) <= max_occ:
                out += [(p, r, j) for r, j in found]
        return out
    return fn


def floor3(a):
    return a // 3                       # Python's // rounds towards minus infinity


def row_candidates(query, q, mode, matcher, rlens, min_seeds, band, pad, code=CODE_STD):
    """[(descriptor, byte, seed record)] of one row in the order of the entry: (byte, r, diag_min)"""
    W = len(query)
    out = []
    for byte, frames in orientations(mode):
        per_ref = {}
        for f in frames:
            off = 0 if f is None else f % 3
            for p, r, j in matcher(letters_of(query, f, code)):
                per_ref.setdefault(r, []).append(3 * j - (off + 3 * p) if is_codon_mode(mode) else j - p)
        for r in sorted(per_ref):
            for n, dmin, dmax in clusters(per_ref[r], band):
                if n < min_seeds:
                    continue
                if is_codon_mode(mode):
                    beg = max(0, floor3(dmin) - pad)
                    end = min(rlens[r], floor3(dmax + W - 1) + 1 + pad)
                else:
                    L = W if frames[0] is None else tlen(W, frames[0])
                    beg = max(0, dmin - pad)
                    end = min(rlens[r], dmax + L + pad)
                out.append(((q, r, 0, -1, beg, end - beg), byte, (n, dmin, dmax, 0)))
    return out


def seed(queries, refs, k, table, mode, min_seeds=2, band=8, pad=16, max_occ=64, q_first=0, nq=None, max_qlen=None, code=CODE_STD,
         matcher=None):
    """what pmx_seed_pairs_letters_device writes with a capacity that holds everything: row_off (nq + 1), pairs, byte, seeds"""
    nq = len(queries) - q_first if nq is None else nq
    if matcher is None:
        matcher = key_matches(index_dict(refs, k, table), k, table, max_occ)
    rlens = [len(s) for s in refs]
    row_off, rows = [0], []
    for q in range(q_first, q_first + nq):
        query = bytes(queries[q])
        size = len(query) if mode == QUERY_LETTERS else len(query) // 3
        if max_qlen is None or size <= max_qlen:
            rows += row_candidates(query, q, mode, matcher, rlens, min_seeds, band, pad, code)
        row_off.append(len(rows))
    return {"row_off": np.array(row_off, dtype=np.int64),
            "pairs": np.array([c[0] for c in rows], dtype=PAIR_DTYPE),
            "byte": np.array([c[1] for c in rows], dtype=np.uint8),
            "seeds": np.array([c[2] for c in rows], dtype=SEED_HIT_DTYPE)}


# ---- inputs shared by the tests: proteins, and reads back-translated from pieces of them ------------------------------------------------
_BACK = {}
for _i, _aa in enumerate(CODE_STD):
    _BACK.setdefault(_aa, []).append("TCAG"[_i >> 4] + "TCAG"[(_i >> 2) & 3] + "TCAG"[_i & 3])


def back_translate(protein, rng):
    """a nucleotide sequence whose frame-0 translation is `protein` (letters of AA20 only), codons chosen by rng"""
    return "".join(_BACK[c][int(rng.integers(len(_BACK[c])))] for c in bytes(protein)).encode()


def revcomp(seq):
    from pairs_ex_ref import revcomp as rc
    return rc(bytes(seq))


def random_protein(rng, n):
    return bytes(ord(AA20[int(x)]) for x in rng.integers(0, 20, size=n))
