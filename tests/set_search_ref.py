"""Plain Python / numpy restatement of set search (include/parasail_amd.h): the two enumerations in exact integers, the descriptors
a shape generates, and the hit list -- the records of the full entry on the same pairs, filtered by score, in enumeration order."""
import numpy as np

import pairs_ref

PAIRS_LIST, PAIRS_TRIANGLE, PAIRS_RECT = 0, 1, 2
INT64_MAX = (1 << 63) - 1
INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)


def rect_pairs_count(nq, nr):
    """nq * nr, -1 if negative or beyond INT64_MAX."""
    if nq < 0 or nr < 0 or nq * nr > INT64_MAX:
        return -1
    return nq * nr


def rect_pairs_index(nr, p):
    """(i, j) of pair p = i * nr + j of the row-major rectangle."""
    return p // nr, p % nr


def shape_count(shape, nq, nr):
    return pairs_ref.all_pairs_count(nq) if shape == PAIRS_TRIANGLE else rect_pairs_count(nq, nr)


def rect_pairs_descriptors(nr, first, count):
    a = np.zeros(count, dtype=pairs_ref.PAIR_DTYPE)
    a["q_len"] = -1
    a["r_len"] = -1
    for k in range(count):
        a[k]["q"], a[k]["r"] = rect_pairs_index(nr, first + k)
    return a


def descriptors(shape, nq, nr, first, count, pairs=None):
    """The descriptors of pairs [first, first + count) of the enumeration, in its order."""
    if shape == PAIRS_LIST:
        assert first == 0
        return np.ascontiguousarray(pairs[:count])
    if shape == PAIRS_TRIANGLE:
        return pairs_ref.all_pairs_descriptors(nq, first, count)
    return rect_pairs_descriptors(nr, first, count)


def hits(records, min_score, first=0, descs=None, stats=None, capacity=None):
    """records: int32 [n, 4] of the full entry on the enumeration's pairs.  -> dict: passing (the full count), written, index
    (absolute), records, pairs and stats of the hits written -- { k : score_k >= min_score } in ascending k, cut at `capacity`."""
    keep = np.nonzero(records[:, 0].astype(np.int64) >= int(min_score))[0]
    passing = len(keep)
    if capacity is not None:
        keep = keep[:capacity]
    return {"passing": passing, "written": len(keep), "index": keep.astype(np.int64) + first, "records": records[keep],
            "pairs": descs[keep] if descs is not None else None, "stats": stats[keep] if stats is not None else None}


def first_empty_pair(shape, qlens, rlens, first, count):
    """Brute force over pairs [first, first + count) of an enumerated shape (TRIANGLE: rlens is qlens): (x, i, j, side) of the first
    pair whose query -- checked first -- or reference is an empty sequence, x counted from the window's first pair; None without one."""
    for p in range(first, first + count):
        i, j = pairs_ref.all_pairs_index(len(qlens), p) if shape == PAIRS_TRIANGLE else rect_pairs_index(len(rlens), p)
        if qlens[i] < 1 or rlens[j] < 1:
            return p - first, i, j, "query" if qlens[i] < 1 else "reference"
    return None
