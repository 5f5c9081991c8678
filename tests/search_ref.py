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
