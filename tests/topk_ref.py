"""Plain numpy restatement of the per-query top-K set search (include/parasail_amd.h, pmx_search_topk[_device]): from the records of
the full entry on the rows' pairs, the per-row cut under (score descending, j ascending), the CSR offsets, descriptors, indices,
counts and the capacity rule -- and a chunked model of the running merge, which looks at the row-major record stream chunk by chunk
the way the device does and relies on the two chunk-order facts of DESIGN 2.5g."""
import numpy as np

import pairs_ref

INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)
TOPK_MAX = 1024


def row_cut(scores, k, min_score=INT32_MIN, skip=None):
    """One row.  scores: the row's scores by j.  -> (kept j in (score descending, j ascending) order, |P_i|)."""
    s = np.asarray(scores, dtype=np.int64)
    ok = s >= int(min_score)
    if skip is not None and 0 <= skip < len(s):
        ok[skip] = False
    j = np.nonzero(ok)[0]
    order = np.lexsort((j, -s[j]))                     # (last key first: score descending, then j ascending)
    return j[order][:k], len(j)


def topk(records, nr, q_first, nq, k, min_score=INT32_MIN, skip_self=False, stats=None, capacity=None):
    """records: int32 [nq * nr, 4] of the full entry on pairs [q_first * nr, (q_first + nq) * nr) of the rectangle.  -> dict: row_off
    (nq + 1, in full), row_passing, counts [kept, written, passing] and index (absolute p), pairs, records, stats of the hits written
    (the first `capacity` in CSR order).  row_cut() on every row at once: one sort of the passing records by (row, score descending, j
    ascending), then the first k of every row (tests/test_topk_records_args.py holds the two against each other)."""
    records = np.asarray(records).reshape(nq * nr, 4)
    s = records[:, 0].astype(np.int64)
    ok = s >= int(min_score)
    if skip_self:
        rows = np.arange(nq, dtype=np.int64)
        own = rows[(q_first + rows >= 0) & (q_first + rows < nr)]
        ok[own * nr + q_first + own] = False
    p = np.nonzero(ok)[0]                                               # local positions li * nr + j of the candidates
    li, j = p // max(nr, 1), p % max(nr, 1)
    p = p[np.lexsort((j, -s[p], li))]                                   # (last key first)
    row_passing = np.bincount(li, minlength=nq).astype(np.int64)[:nq]
    start = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum(row_passing, out=start[1:])
    rank = np.arange(len(p), dtype=np.int64) - np.repeat(start[:-1], row_passing)
    keep = p[rank < k]
    row_off = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum(np.minimum(row_passing, k), out=row_off[1:])
    kept = len(keep)
    if capacity is not None:
        keep = keep[:capacity]
    index = keep + q_first * nr
    pairs = np.zeros(len(keep), dtype=pairs_ref.PAIR_DTYPE)
    pairs["q"], pairs["r"] = index // max(nr, 1), index % max(nr, 1)
    pairs["q_len"] = -1
    pairs["r_len"] = -1
    return {"row_off": row_off, "row_passing": row_passing,
            "counts": [kept, len(keep), int(row_passing.sum())], "index": index, "pairs": pairs, "records": records[keep],
            "stats": stats[keep] if stats is not None else None}


def topk_by_rows(records, nr, q_first, nq, k, min_score=INT32_MIN, skip_self=False):
    """topk() row by row through row_cut(): -> (local positions kept, row_off, row_passing)"""
    records = np.asarray(records).reshape(nq * nr, 4)
    keep, row_off, row_passing = [], [0], []
    for li in range(nq):
        j, passing = row_cut(records[li * nr:(li + 1) * nr, 0], k, min_score, q_first + li if skip_self else None)
        keep.extend((li * nr + j).tolist())
        row_off.append(len(keep))
        row_passing.append(passing)
    return keep, row_off, row_passing


def chunked_rows(scores, nr, k, chunk, min_score=INT32_MIN, skip_self=False, q_first=0):
    """The running merge as the device runs it.  scores: the row-major stream of nq * nr scores, cut into chunks of `chunk` whatever
    the rows.  Per row a list of at most k (score, j) in final order.  Per row segment of a chunk:
      prefilter -- score >= min_score, not the self pair, and, ONCE THE LIST IS FULL with k-th score T, score > T strictly: every j
                   of the segment is larger than every j the row has seen, so a record equal to T loses to every kept one;
      merge     -- stable by score descending with THE LIST'S MEMBERS FIRST inside a tie run, then the segment's in ascending j,
                   cut at k.
    -> (lists of kept j per row, passing per row)."""
    scores = np.asarray(scores, dtype=np.int64)
    nq = len(scores) // nr
    lists = [[] for _ in range(nq)]
    passing = [0] * nq
    for c0 in range(0, len(scores), chunk):
        c1 = min(c0 + chunk, len(scores))
        for li in range(c0 // nr, (c1 - 1) // nr + 1):
            j0, j1 = max(c0, li * nr) - li * nr, min(c1, (li + 1) * nr) - li * nr
            lst = lists[li]
            full = len(lst) == k
            t = lst[-1][0] if full else None
            seg = []
            for j in range(j0, j1):
                s = int(scores[li * nr + j])
                if s < min_score or (skip_self and j == q_first + li):
                    continue
                passing[li] += 1
                if full and not s > t:
                    continue
                seg.append((s, j))
            merged = sorted(lst + seg, key=lambda e: -e[0])            # (stable: the list's members first, then ascending j)
            lists[li] = merged[:k]
    return [[j for _, j in lst] for lst in lists], passing
