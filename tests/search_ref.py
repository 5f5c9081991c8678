"""numpy reference of the search's hit selection (include/parasail_amd.h: pmx_select_hits_device) and the helpers the search tests
share.  No GPU, no library."""
import numpy as np

BY_INDEX, BY_SCORE = 0, 1


def select(scores, min_score, max_hits, order):
    """-> (int64 indices of the selected records in output order, number passing the threshold)"""
    scores = np.asarray(scores, dtype=np.int64)
    passing = np.nonzero(scores >= min_score)[0]
    # (score descending, index ascending): a stable sort of the negated scores over ascending indices
    ranked = passing[np.argsort(-scores[passing], kind="stable")]
    if max_hits > 0:
        ranked = ranked[:max_hits]
    out = ranked if order == BY_SCORE else np.sort(ranked)
    return out.astype(np.int64), int(len(passing))


def select_sorted(scores, min_score, max_hits, order):
    """the same through plain sorted(): the formulation select() is tested against"""
    passing = [k for k, s in enumerate(scores) if s >= min_score]
    ranked = sorted(passing, key=lambda k: (-int(scores[k]), k))
    if max_hits > 0:
        ranked = ranked[:max_hits]
    return (ranked if order == BY_SCORE else sorted(ranked)), len(passing)


def tied_scores(rng, n, distinct=20, lo=-300, hi=300):
    """n scores drawn from `distinct` values, negative ones included: every rank sits in a long tie run"""
    values = np.unique(np.concatenate([rng.integers(lo, hi, size=distinct - 2), [lo - 7, hi + 5]]))
    return values[rng.integers(0, len(values), size=n)].astype(np.int32)


INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
# The selection's radix digits of the biased score (score ^ 0x80000000), from the top: (shift, bits)
DIGITS = ((21, 11), (10, 11), (0, 10))


def _draw(rng, values, n):
    values = np.unique(np.asarray(values, dtype=np.int64))
    return values[rng.integers(0, len(values), size=n)].astype(np.int32)


def full_range_scores(rng, n):
    """uniform over all of int32: nearly every record alone in its bins"""
    return rng.integers(INT32_MIN, INT32_MAX + 1, size=n, dtype=np.int64).astype(np.int32)


def top_digit_scores(rng, n, distinct=40):
    """multiples of 2^21 -- values that differ in the top digit only -- drawn from `distinct` of the 2048, both ends among them: the
    first pass chooses among many bins (bin 0 is INT32_MIN), the later passes see one bin"""
    d = np.concatenate([rng.integers(0, 2048, size=distinct - 2), [0, 2047]])
    return _draw(rng, (d - 1024) << 21, n)


def middle_digit_scores(rng, n, distinct=40):
    """multiples of 2^10 inside one top bin (a negative one), bins 0 and 2047 of the middle digit among them: one bin in the first
    pass, the choice in the second"""
    m = np.concatenate([rng.integers(0, 2048, size=distinct - 2), [0, 2047]])
    return _draw(rng, ((300 - 1024) << 21) + (m << 10), n)


def low_digit_scores(rng, n, distinct=40):
    """values that differ in the low 10 bits only, on top of non-zero upper digits"""
    l = np.concatenate([rng.integers(0, 1024, size=distinct - 2), [0, 1023]])
    return _draw(rng, ((1500 - 1024) << 21) + (77 << 10) + l, n)


def cluster_scores(rng, n):
    """the values next to the digit borders -- +-2^10 +- 1, +-2^21 +- 1 and the borders themselves, 0, -1 -- and both ends of int32:
    20 values, so every one is a tie run of n / 20 records, and neighbours differ in the low digit, the middle one or the sign"""
    v = [0, -1, INT32_MIN, INT32_MAX]
    for b in (1 << 10, 1 << 21):
        v += [b - 1, b, b + 1, -b - 1, -b, -b + 1]
    return _draw(rng, v, n)


def bin0_scores(which, n=3000, seed=5300):
    """n scores of which the 600 highest lie in higher bins and the others in bin 0 of the `which` ("top" / "middle") digit, spread over
    the digits below it in short tie runs: with 600 < max_hits < n the K-th score lies in that bin 0, which the pick loop never tests.
    top: biased keys below 2^21, scores next to INT32_MIN.  middle: one top bin, 600 records in middle bins 1 .. 2047, the others in 0."""
    rng = np.random.default_rng(seed)
    if which == "top":
        low = INT32_MIN + (rng.integers(0, 1 << 21, size=300)[rng.integers(0, 300, size=n)])
        high = ((rng.integers(1, 2048, size=600) - 1024) << 21) + rng.integers(0, 1 << 21, size=600)
    else:
        base = (1234 - 1024) << 21
        low = base + rng.integers(0, 1 << 10, size=300)[rng.integers(0, 300, size=n)]
        high = base + (rng.integers(1, 2048, size=600) << 10) + rng.integers(0, 1 << 10, size=600)
    scores = low.astype(np.int64)
    scores[rng.choice(n, size=600, replace=False)] = high
    return scores.astype(np.int32)


WIDE_SCORES = {"full-range": full_range_scores, "top-digit": top_digit_scores, "middle-digit": middle_digit_scores,
               "low-digit": low_digit_scores, "clusters": cluster_scores}


def radix_select_model(scores, min_score, max_hits):
    """The three passes of the device's radix select (csrc/pmx_select.hip), restated: per pass the histogram of one digit over the
    passing records whose upper digits equal the prefix so far (pmx_select_hist_kernel), then the pick (pmx_select_pick_kernel) --
    from the top bin down the first bin at which the running count reaches the rank krem still looked for; the records of the bins
    above it are `gt`, krem shrinks by them, the bin's digit joins the prefix; bin 0 is taken when no bin above it holds the rank.
    After the last digit the prefix is the K-th score Tu and krem the number E kept of its tie run (eq_take).
    -> (T, above, E): the records with score > T (`above` of them) and the first E with score == T in index order are the selection.
    (None, |P|, 0) when nothing is cut: max_hits <= 0 or |P| <= max_hits."""
    u = (np.asarray(scores).astype(np.int64) & 0xFFFFFFFF) ^ 0x80000000
    min_u = (int(min_score) & 0xFFFFFFFF) ^ 0x80000000
    n_pass = krem = gt = eq_take = prefix = mask = Tu = 0
    cut = False
    for ps, (shift, bits) in enumerate(DIGITS):
        first = ps == 0
        if not first and (max_hits <= 0 or not cut):
            break
        live = (u >= min_u) & ((u & mask) == prefix)
        hist = np.bincount((u[live] >> shift) & ((1 << bits) - 1), minlength=1 << bits)
        if first:
            n_pass = int(hist.sum())
            cut = max_hits > 0 and n_pass > max_hits
            krem = max_hits
        if cut:
            acc, d = 0, (1 << bits) - 1
            while d > 0:
                if acc + int(hist[d]) >= krem:
                    break
                acc += int(hist[d])
                d -= 1
            gt += acc
            krem -= acc
            prefix |= d << shift
            mask |= ((1 << bits) - 1) << shift
            if shift == 0:
                Tu, eq_take = prefix, krem
    if not cut:
        return None, n_pass, 0
    return _signed(Tu ^ 0x80000000), gt, eq_take


def _signed(v):
    return v - (1 << 32) if v >= 1 << 31 else v


def model_selection(scores, min_score, max_hits):
    """the indices radix_select_model()'s answer selects, ascending: what the count / scan / scatter kernels make of (T, above, E)"""
    scores = np.asarray(scores, dtype=np.int64)
    T, above, E = radix_select_model(scores, min_score, max_hits)
    if T is None:
        return np.nonzero(scores >= min_score)[0]
    return np.sort(np.concatenate([np.nonzero(scores > T)[0], np.nonzero(scores == T)[0][:E]]))


def records(scores, rng=None):
    """[n, 4] int32 records with these scores; the other fields are noise the selection must not look at"""
    n = len(scores)
    rec = np.zeros((n, 4), dtype=np.int32)
    rec[:, 0] = scores
    if rng is not None:
        rec[:, 1:] = rng.integers(-5, 1 << 20, size=(n, 3))
    return rec


NEG = -(1 << 30)


def oracle_banded(orc, mode, flags, q, r, open_, ext, om, band, diag):
    """orc_align_ex inside the band with a trace table, then the oracle's walk:
    (score, end_query, end_ref, cigar, matches, similar, length, beg_query, beg_ref); no path: score NEG, "", zeros, begins -1"""
    import ctypes as C
    qa, ra = np.frombuffer(q, dtype=np.uint8), np.frombuffer(r, dtype=np.uint8)
    res, out = orc._Result(), orc._Outputs()
    trace = np.zeros((len(q), len(r)), dtype=np.int8)
    out.trace_table = trace.ctypes.data
    rc = orc.lib().orc_align_ex(mode, flags, orc._ptr(qa), len(q), orc._ptr(ra), len(r), int(open_), int(ext), orc._ptr(om.scores),
                                om.size, orc._ptr(om.mapper), 32, 1, int(band), int(diag), C.byref(res), C.byref(out))
    assert rc == 0
    if res.score == NEG:
        return res.score, res.end_query, res.end_ref, "", 0, 0, 0, -1, -1
    o = orc.Result()
    o.mode, o.trace_table, o.query, o.ref, o.matrix, o.end_query, o.end_ref = mode, trace, q, r, om, res.end_query, res.end_ref
    _, bq, br = orc.walk(o)
    return res.score, res.end_query, res.end_ref, orc.cigar(o), res.matches, res.similar, res.length, bq, br


def hit_tuple(hits, k):
    """what oracle_banded returns, out of a SearchHits (recs, cigars, stats, begins)"""
    return (int(hits.recs["score"][k]), int(hits.recs["end_query"][k]), int(hits.recs["end_ref"][k]), hits.cigars[k],
            int(hits.stats["matches"][k]), int(hits.stats["similar"][k]), int(hits.stats["length"][k]),
            int(hits.beg_query[k]), int(hits.beg_ref[k]))
