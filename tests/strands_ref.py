"""Plain numpy restatement of the strand modes of the set entries (include/parasail_amd.h, PMX_STRAND_*): the fold of the two
records a pair has -- rec0 with strand byte 0, rec1 with strand byte 1, as pmx_align_pairs_ex_device writes them -- and the two
reference pipelines over the folded records: set search (set_search_ref.hits) and per-query top-K (topk_ref.topk), each with the
strand byte of every hit."""
import numpy as np

import set_search_ref
import topk_ref

STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = 0, 1, 2


def fold(rec0, rec1, stats0=None, stats1=None, mode=STRAND_BOTH):
    """rec0 / rec1: int32 [n, 4].  -> (records, stats or None, strand uint8).  BOTH: rec1 where rec1.score > rec0.score, else rec0
    -- only the score is compared, a tie goes to the forward strand; the record and the statistics are the winner's, whole.  A bad
    descriptor is bad on both strands (two equal records, a tie), so its strand is 0 -- in REVERSE too."""
    rec0, rec1 = np.asarray(rec0), np.asarray(rec1)
    if mode == STRAND_FORWARD:
        won = np.zeros(len(rec0), dtype=bool)
    elif mode == STRAND_REVERSE:
        won = (rec1[:, 3] & 8) == 0
    else:
        won = rec1[:, 0].astype(np.int64) > rec0[:, 0].astype(np.int64)
    rec = np.where(won[:, None], rec1, rec0)
    stats = np.where(won[:, None], stats1, stats0) if stats0 is not None else None
    return np.ascontiguousarray(rec), (np.ascontiguousarray(stats) if stats is not None else None), won.astype(np.uint8)


def search(rec0, rec1, min_score, first=0, descs=None, stats0=None, stats1=None, capacity=None, mode=STRAND_BOTH):
    """set_search_ref.hits over the folded records, plus "strand": the strand byte of every hit written."""
    rec, stats, strand = fold(rec0, rec1, stats0, stats1, mode)
    h = set_search_ref.hits(rec, min_score, first, descs, stats, capacity)
    h["strand"] = strand[h["index"] - first]
    return h


def topk(rec0, rec1, nr, q_first, nq, k, min_score=topk_ref.INT32_MIN, skip_self=False, stats0=None, stats1=None, capacity=None,
         mode=STRAND_BOTH):
    """topk_ref.topk over the folded records (a pair is one candidate; the strand is not part of the order), plus "strand"."""
    rec, stats, strand = fold(rec0, rec1, stats0, stats1, mode)
    t = topk_ref.topk(rec, nr, q_first, nq, k, min_score, skip_self, stats, capacity)
    t["strand"] = strand[t["index"] - q_first * nr]
    return t
