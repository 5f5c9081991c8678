"""Plain Python / numpy restatement of the sequence-set batches (include/parasail_amd.h): descriptors resolved to byte strings, the
row-major numbering of the strict upper triangle in exact integers, and the record a bad descriptor gets."""
from math import isqrt

import numpy as np

PAIR_DTYPE = np.dtype([("q", "<i8"), ("r", "<i8"), ("q_beg", "<i4"), ("q_len", "<i4"), ("r_beg", "<i4"), ("r_len", "<i4")])
FLAG_BAD_PAIR = 8
BAD_RECORD = (0, -1, -1, FLAG_BAD_PAIR)
INT32_MAX = (1 << 31) - 1


def pairs_array(rows):
    """(q, r) or (q, r, q_beg, q_len, r_beg, r_len) tuples -> PAIR_DTYPE array (missing windows: whole sequences)."""
    a = np.zeros(len(rows), dtype=PAIR_DTYPE)
    for k, t in enumerate(rows):
        a[k] = tuple(t) if len(t) == 6 else (t[0], t[1], 0, -1, 0, -1)
    return a


def resolve_side(seqs, idx, beg, length, max_len=INT32_MAX):
    """The window's bytes, or None for a bad descriptor side."""
    idx, beg, length = int(idx), int(beg), int(length)
    if idx < 0 or idx >= len(seqs) or beg < 0 or length < -1:
        return None
    s = seqs[idx]
    l = len(s) - beg if length < 0 else length
    if l < 1 or beg + l > len(s) or l > max_len:
        return None
    return bytes(s[beg:beg + l])


def resolve(qseqs, rseqs, pairs, max_qlen=INT32_MAX, max_rlen=INT32_MAX):
    """[(query bytes, reference bytes) or None for a bad pair] for a PAIR_DTYPE array."""
    out = []
    for p in pairs:
        q = resolve_side(qseqs, p["q"], p["q_beg"], p["q_len"], max_qlen)
        r = resolve_side(rseqs, p["r"], p["r_beg"], p["r_len"], max_rlen)
        out.append((q, r) if q is not None and r is not None else None)
    return out


def all_pairs_count(n):
    return n * (n - 1) // 2


def row_start(n, i):
    return i * (2 * n - i - 1) // 2


def all_pairs_index(n, p):
    """(i, j), i < j, of pair p = i (2 n - i - 1) / 2 + (j - i - 1): i is the largest row whose first pair is <= p."""
    assert n >= 2 and 0 <= p < all_pairs_count(n)
    b = 2 * n - 1
    d = b * b - 8 * p
    root = isqrt(d)
    if root * root < d:
        root += 1                                   # ceil(sqrt(d)): i = floor((b - sqrt(d)) / 2)
    i = (b - root) // 2
    assert row_start(n, i) <= p < row_start(n, i + 1)
    return i, i + 1 + (p - row_start(n, i))


def all_pairs_descriptors(n, first, count):
    a = np.zeros(count, dtype=PAIR_DTYPE)
    a["q_len"] = -1
    a["r_len"] = -1
    for k in range(count):
        a[k]["q"], a[k]["r"] = all_pairs_index(n, first + k)
    return a


def edge_positions(n, rng, rows=64, width=4096):
    """Where a rounded square root is off by one: the first and last `width` pairs and `width` pairs around `rows` random row starts."""
    total = all_pairs_count(n)
    ps = set(range(min(width, total))) | set(range(max(0, total - width), total))
    for i in rng.integers(1, n - 1, size=rows):
        s = row_start(n, int(i))
        ps |= set(range(max(0, s - width // 2), min(total, s + width // 2)))
    return sorted(ps)
