"""Reference model of seed chaining (include/parasail_amd.h, "Seed chaining"), written from the definitions on top of
tests/seed_ref.py and tests/seed_minimizer_ref.py: the anchors (j, i) of a (row, strand, reference), the link rule and its cost, f,
pred, child, the chains, the candidates and what pmx_seed_chains_device writes.  Sequences are bytes."""
import numpy as np

import seed_minimizer_ref as mref
import seed_ref as ref

CHAIN_DTYPE = np.dtype([("score", "<i4"), ("n_anchors", "<i4"), ("q_beg", "<i4"), ("q_end", "<i4"), ("r_beg", "<i4"), ("r_end", "<i4"),
                        ("diag_min", "<i4"), ("diag_max", "<i4")])
DEFAULTS = dict(min_seeds=2, min_score=0, band=500, max_gap=5000, lookback=64, gap_scale=38, pad=16, max_occ=64)


def cost(g, gap_scale):
    """cost(0) = 0; for g >= 1: (g * gap_scale >> 8) + ((32 - clz(g)) >> 1) -- 32 - clz(g) is g's bit length"""
    return 0 if g == 0 else ((g * gap_scale) >> 8) + (int(g).bit_length() >> 1)


def admissible(b, a, anchors, band, max_gap, lookback):
    """may position b precede position a (anchors: (j, i) in anchor order)"""
    dj, di = anchors[a][0] - anchors[b][0], anchors[a][1] - anchors[b][1]
    return b < a and dj >= 1 and di >= 1 and dj <= max_gap and di <= max_gap and abs(dj - di) <= band and a - b <= lookback


def link_value(fb, b, a, anchors, k, gap_scale):
    dj, di = anchors[a][0] - anchors[b][0], anchors[a][1] - anchors[b][1]
    return fb + min(di, dj, k) - cost(abs(dj - di), gap_scale)


def scores(anchors, k, band, max_gap, lookback, gap_scale):
    """f and pred of anchors sorted by (j, i), one predecessor at a time, as the definition reads"""
    f, pred = [], []
    for a in range(len(anchors)):
        best, bb = k, -1
        for b in range(a - 1, max(-1, a - 1 - lookback), -1):          # nearest first: a farther one has to be strictly better
            if admissible(b, a, anchors, band, max_gap, lookback):
                v = link_value(f[b], b, a, anchors, k, gap_scale)
                if v > best:
                    best, bb = v, b
        f.append(best)
        pred.append(bb)
    return f, pred


def scores_fast(anchors, k, band, max_gap, lookback, gap_scale):
    """the same f and pred with the window of a evaluated at once (numpy); tests compare it with scores() before they rely on it"""
    n = len(anchors)
    J = np.array([x[0] for x in anchors], dtype=np.int64)
    I = np.array([x[1] for x in anchors], dtype=np.int64)
    F = np.zeros(n, dtype=np.int64)
    pred = [-1] * n
    for a in range(n):
        lo = max(0, a - lookback)
        best, bb = k, -1
        if a > lo:
            dj, di = J[a] - J[lo:a], I[a] - I[lo:a]
            g = np.abs(dj - di)
            ok = (dj >= 1) & (di >= 1) & (dj <= max_gap) & (di <= max_gap) & (g <= band)
            if ok.any():
                c = ((g * gap_scale) >> 8) + (np.frexp(g.astype(np.float64))[1] >> 1)        # frexp's exponent of g >= 1 is its bit length
                v = np.where(ok, F[lo:a] + np.minimum(np.minimum(di, dj), k) - np.where(g > 0, c, 0), -(1 << 62))
                m = int(v.max())
                if m > k:
                    best, bb = m, lo + (a - lo - 1 - int(np.argmax(v[::-1])))                # the last index that attains it: the nearest
        F[a] = best
        pred[a] = bb
    return F.tolist(), pred


def children(f, pred):
    """child(b): among the a with pred(a) = b the one with the largest f(a), the smallest a among equals; -1: none"""
    child = [-1] * len(f)
    for a in range(len(f)):
        b = pred[a]
        if b >= 0 and (child[b] < 0 or f[a] > f[child[b]]):
            child[b] = a
    return child


def chains(f, pred, child):
    """[(members head .. tail, score)] ascending by tail: the maximal paths of kept links (a -> pred(a) kept iff child(pred(a)) == a)"""
    out = []
    for t in range(len(f)):
        if child[t] >= 0:
            continue
        members, x = [t], t
        while pred[x] >= 0 and child[pred[x]] == x:
            x = pred[x]
            members.append(x)
        score = f[t] - (f[pred[x]] if pred[x] >= 0 else 0)
        out.append((members[::-1], score))
    return out


def anchors_of(query, strand, idx, k, max_occ, w=1):
    """{r: [(j, i)] ascending} of one oriented query; idx: the index dictionary (of the minimizers where w > 1)"""
    o = ref.orient(query, strand)
    keys = dict(ref.kmers(o, k))
    positions = sorted(keys) if w == 1 else mref.minimizers(o, k, w)
    out = {}
    for i in positions:
        occ = idx.get(keys[i], ())
        if len(occ) > max_occ:
            continue
        for r, j in occ:
            out.setdefault(r, []).append((j, i))
    return {r: sorted(v) for r, v in out.items()}


def candidates_of(anchors, k, qlen, rlen, q, r, strand, min_seeds, min_score, band, max_gap, lookback, gap_scale, pad, fast=True):
    f, pred = (scores_fast if fast else scores)(anchors, k, band, max_gap, lookback, gap_scale)
    out = []
    for members, score in chains(f, pred, children(f, pred)):
        if score < min_score or len(members) < min_seeds:
            continue
        d = [anchors[x][0] - anchors[x][1] for x in members]
        dmin, dmax = min(d), max(d)
        beg, end = max(0, dmin - pad), min(rlen, dmax + qlen + pad)
        (jh, ih), (jt, it) = anchors[members[0]], anchors[members[-1]]
        out.append(((q, r, 0, -1, beg, end - beg), strand, (len(members), dmin, dmax, 0),
                    (score, len(members), ih, it + k, jh, jt + k, dmin, dmax)))
    return out


def seed_chains(queries, refs, k, w=1, strand=ref.BOTH, q_first=0, nq=None, max_qlen=None, fast=True, **opts):
    """what pmx_seed_chains_device writes with a capacity that holds everything: row_off (nq + 1), pairs, strand, seeds, chains"""
    o = dict(DEFAULTS)
    o.update(opts)
    nq = len(queries) - q_first if nq is None else nq
    idx = ref.index_dict(refs, k) if w == 1 else mref.index_dict(refs, k, w)
    row_off, rows = [0], []
    for q in range(q_first, q_first + nq):
        query = bytes(queries[q])
        if max_qlen is None or len(query) <= max_qlen:
            for s in ref.strands_of(strand):
                per_ref = anchors_of(query, s, idx, k, o["max_occ"], w)
                for r in sorted(per_ref):
                    rows += candidates_of(per_ref[r], k, len(query), len(refs[r]), q, r, s, o["min_seeds"], o["min_score"], o["band"], o["max_gap"],
                                          o["lookback"], o["gap_scale"], o["pad"], fast)
        row_off.append(len(rows))
    return {"row_off": np.array(row_off, dtype=np.int64),
            "pairs": np.array([c[0] for c in rows], dtype=ref.PAIR_DTYPE),
            "strand": np.array([c[1] for c in rows], dtype=np.uint8),
            "seeds": np.array([c[2] for c in rows], dtype=ref.SEED_HIT_DTYPE),
            "chains": np.array([c[3] for c in rows], dtype=CHAIN_DTYPE)}


def brute_best(anchors, k, band, max_gap, lookback, gap_scale):
    """f by exhaustion: for every a the best of k + the sum of (gain - cost) over every subsequence that ends at a and whose
    consecutive members are admissible links; the sequence of a alone scores k"""
    n = len(anchors)
    best = [k] * n

    def grow(last, value):
        for a in range(last + 1, n):
            if admissible(last, a, anchors, band, max_gap, lookback):
                v = link_value(value, last, a, anchors, k, gap_scale)
                best[a] = max(best[a], v)
                grow(a, v)
    for s in range(n):
        grow(s, k)
    return best


# ---- planted anchor sets (anchors are (j, i)): the link rule one step either side of every bound, and the ties -----------------------
# name: (anchors, options, pred); k = 12, and where nothing is said band 100, max_gap 1000, lookback 64, gap_scale 38
PLANT_K = 12
PLANT_OPTS = dict(band=100, max_gap=1000, lookback=64, gap_scale=38)
BOUNDARIES = {
    # name: (anchors, options, pred)
    "dj = max_gap":       ([(0, 0), (50, 45)], dict(max_gap=50), [-1, 0]),
    "dj = max_gap + 1":   ([(0, 0), (51, 45)], dict(max_gap=50), [-1, -1]),
    "di = max_gap":       ([(0, 0), (45, 50)], dict(max_gap=50), [-1, 0]),
    "di = max_gap + 1":   ([(0, 0), (45, 51)], dict(max_gap=50), [-1, -1]),
    "g = band":           ([(0, 0), (60, 30)], dict(band=30), [-1, 0]),
    "g = band + 1":       ([(0, 0), (61, 30)], dict(band=30), [-1, -1]),
    "g = band, i ahead":  ([(0, 0), (30, 60)], dict(band=30), [-1, 0]),
    "g = band + 1, i ahead": ([(0, 0), (30, 61)], dict(band=30), [-1, -1]),
    # two anchors between that link to nothing: j rises by 1 while i falls, and i is far beyond the band
    "a - b = lookback":     ([(0, 0), (1, 950), (2, 900), (100, 100)], dict(lookback=3), [-1, -1, -1, 0]),
    "a - b = lookback + 1": ([(0, 0), (1, 950), (2, 900), (100, 100)], dict(lookback=2), [-1, -1, -1, -1]),
    # a k-mer repeated in the read: through (20, 20) the last anchor would reach k + 12 + 0 - cost(20), what it reaches from (0, 0) --
    # were dj = 0 a link, the nearer one would win the tie
    "dj = 0, di > 0":     ([(0, 0), (20, 20), (20, 40)], dict(), [-1, 0, 0]),
    "dj = 1, di > 0":     ([(0, 0), (20, 20), (21, 40)], dict(), [-1, 0, 1]),
    # ... and one repeated in the reference
    "di = 0, dj > 0":     ([(0, 0), (20, 20), (40, 20)], dict(), [-1, 0, 0]),
    "di = 1, dj > 0":     ([(0, 0), (20, 20), (40, 21)], dict(), [-1, 0, 1]),
}
TIE_NEAREST = [(0, 20), (20, 0), (60, 60)]            # both reach (60, 60) with g = 20 and a full gain: equal values
TIE_CHILD = [(0, 0), (30, 50), (50, 30)]              # both choose (0, 0) with g = 20: equal f
TIE_AT_K = [(0, 0), (84, 20)]                         # g = 64: cost 9 + 3 = the gain of 12, the value is k


def plant(rng, anchors, k=PLANT_K, tries=50):
    """(read, reference): random letters but for the equalities the anchors ask for -- read[i + x] == reference[j + x] for x < k, whatever
    that makes equal inside the read or the reference (a k-mer repeated on one side, overlapping k-mers) -- such that the matches of the
    pair are exactly `anchors`.  Chance matches are drawn again."""
    qlen = max(i for _, i in anchors) + k + 5
    rlen = max(j for j, _ in anchors) + k + 5
    parent = list(range(qlen + rlen))                     # letters of the read, then of the reference

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for j, i in anchors:
        for x in range(k):
            parent[find(i + x)] = find(qlen + j + x)
    for _ in range(tries):
        letters = rng.integers(0, 4, size=qlen + rlen)
        both = bytes(b"ACGT"[letters[find(x)]] for x in range(qlen + rlen))
        q, r = both[:qlen], both[qlen:]
        if anchors_of(q, 0, ref.index_dict([r], k), k, 1 << 20) == {0: sorted(anchors)}:
            return q, r
    raise AssertionError("no pair with exactly these anchors: %r" % (anchors,))
