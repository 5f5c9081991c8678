"""Reference model of k-mer seeding (include/parasail_amd.h), in plain Python / numpy: the index as a sorted list and a
dictionary of k-mers, matches, diagonal clusters, windows and their order -- and, beside it, a brute-force cross-check that compares
every (i, j) letter by letter and never forms a key.  Sequences are bytes."""
import numpy as np

PAIR_DTYPE = np.dtype([("q", "<i8"), ("r", "<i8"), ("q_beg", "<i4"), ("q_len", "<i4"), ("r_beg", "<i4"), ("r_len", "<i4")])
SEED_HIT_DTYPE = np.dtype([("n_seeds", "<i4"), ("diag_min", "<i4"), ("diag_max", "<i4"), ("reserved", "<i4")])
FORWARD, REVERSE, BOTH = 0, 1, 2

CODE = {ord(c): v for c, v in zip("ACGTUacgtu", (0, 1, 2, 3, 3, 0, 1, 2, 3, 3))}


_LUT = np.full(256, 255, dtype=np.uint8)
for _c, _v in CODE.items():
    _LUT[_c] = _v


def complement_table():
    t = list(range(256))
    for a, b in zip("ACGTUMRWSYKVHDBN", "TGCAAKYWSRMBDHVN"):
        t[ord(a)] = ord(b)
        t[ord(a.lower())] = ord(b.lower())
    return bytes(t)


COMP = complement_table()


def orient(seq, strand):
    """the oriented query: as stored, or w'[x] = comp[w[L - 1 - x]]"""
    return bytes(seq) if strand == 0 else bytes(seq)[::-1].translate(COMP)


def kmers(seq, k):
    """[(pos, key)] of the k-mers of seq: all k letters valid, first letter most significant"""
    a = np.frombuffer(bytes(seq), dtype=np.uint8)
    n = len(a) - k + 1
    if n <= 0:
        return []
    c = _LUT[a]
    bad = np.concatenate(([0], np.cumsum(c == 255)))
    key = np.zeros(n, dtype=np.uint64)
    for x in range(k):
        key = (key << np.uint64(2)) | (c[x:x + n] & 3).astype(np.uint64)
    pos = np.nonzero(bad[k:] == bad[:-k])[0]
    return list(zip(pos.tolist(), key[pos].tolist()))


def index_entries(refs, k):
    """the index: (kmer, seq, pos) of every k-mer of the set, ascending"""
    return sorted((key, r, j) for r, s in enumerate(refs) for j, key in kmers(s, k))


def index_dict(refs, k):
    d = {}
    for key, r, j in index_entries(refs, k):
        d.setdefault(key, []).append((r, j))
    return d


def strands_of(mode):
    return {FORWARD: (0,), REVERSE: (1,), BOTH: (0, 1)}[mode]


def matches(query, strand, idx, k, max_occ):
    """{r: [d, ...]} of one oriented query: d = j - i for every (i, j) with the same k-mer, k-mers above max_occ entries ignored"""
    out = {}
    for i, key in kmers(orient(query, strand), k):
        occ = idx.get(key, ())
        if len(occ) > max_occ:
            continue
        for r, j in occ:
            out.setdefault(r, []).append(j - i)
    return out


def clusters(diags, band):
    """sorted diagonals -> [(n, dmin, dmax)]: maximal runs whose consecutive diagonals differ by at most band"""
    out = []
    ds = sorted(diags)
    a = 0
    for x in range(1, len(ds) + 1):
        if x == len(ds) or ds[x] - ds[x - 1] > band:
            out.append((x - a, ds[a], ds[x - 1]))
            a = x
    return out


def candidates_from(per_ref, qlen, rlens, q, strand, min_seeds, band, pad):
    out = []
    for r in sorted(per_ref):
        for n, dmin, dmax in clusters(per_ref[r], band):
            if n >= min_seeds:
                beg = max(0, dmin - pad)
                end = min(rlens[r], dmax + qlen + pad)
                out.append(((q, r, 0, -1, beg, end - beg), strand, (n, dmin, dmax, 0)))
    return out


def seed(queries, refs, k, strand=BOTH, min_seeds=2, band=8, pad=16, max_occ=64, q_first=0, nq=None, max_qlen=None, match_fn=None):
    """what pmx_seed_pairs_device writes with a capacity that holds everything: row_off (nq + 1), pairs, strand, seeds"""
    nq = len(queries) - q_first if nq is None else nq
    idx = index_dict(refs, k) if match_fn is None else None
    rlens = [len(s) for s in refs]
    row_off, rows = [0], []
    for q in range(q_first, q_first + nq):
        query = bytes(queries[q])
        if max_qlen is None or len(query) <= max_qlen:
            for s in strands_of(strand):
                per_ref = matches(query, s, idx, k, max_occ) if match_fn is None else match_fn(query, s)
                rows += candidates_from(per_ref, len(query), rlens, q, s, min_seeds, band, pad)
        row_off.append(len(rows))
    return {"row_off": np.array(row_off, dtype=np.int64),
            "pairs": np.array([c[0] for c in rows], dtype=PAIR_DTYPE),
            "strand": np.array([c[1] for c in rows], dtype=np.uint8),
            "seeds": np.array([c[2] for c in rows], dtype=SEED_HIT_DTYPE)}


# ---- brute force: no keys, letters only ------------------------------------------------------------------------------------------------
def _letter(c):
    return CODE.get(c)


def _same_kmer(a, i, b, j, k):
    """both have a k-mer there and the letters agree (T and U are one letter)"""
    if i + k > len(a) or j + k > len(b):
        return False
    for x in range(k):
        u, v = _letter(a[i + x]), _letter(b[j + x])
        if u is None or v is None or u != v:
            return False
    return True


def brute_matches(refs, k, max_occ):
    """a match function for seed(): every (i, j) compared letter by letter; the occurrences of the query's k-mer are counted the
    same way over the whole set"""
    refs = [bytes(s) for s in refs]

    def fn(query, strand):
        w = orient(query, strand)
        out = {}
        for i in range(len(w) - k + 1):
            found = [(r, j) for r, s in enumerate(refs) for j in range(len(s) - k + 1) if _same_kmer(w, i, s, j, k)]
            if len(found) > max_occ:
                continue
            for r, j in found:
                out.setdefault(r, []).append(j - i)
        return out
    return fn


def longest_clean_run(length, error_positions):
    """the longest stretch of [0, length) without a position of error_positions"""
    best, last = 0, -1
    for p in sorted(set(error_positions)) + [length]:
        best = max(best, p - last - 1)
        last = p
    return best
