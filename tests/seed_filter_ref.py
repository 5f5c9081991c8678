"""Plain Python / numpy restatement of the ungapped diagonal filter (include/parasail_amd.h, pmx_seed_ungapped / pmx_seed_filter): the
oriented windows of a candidate -- strands through pairs_ex_ref (the restatement of the _ex entries' strand rule that strands_ref
builds on), frames through translate_ref --, the recurrence h(d, i) = max(0, h(d, i - 1) + w) along the seeded diagonals, the tie
rule (lowest d, then lowest i), the record of a bad candidate, and the selection: threshold, top_n per row by (score descending,
position ascending), output in input order.  Written from the specification; nothing here reads the library."""
import numpy as np

import pairs_ex_ref
import pairs_ref
import translate_ref

INT32_MAX = pairs_ref.INT32_MAX
PAIR_DTYPE = pairs_ref.PAIR_DTYPE
SEED_HIT_DTYPE = np.dtype([("n_seeds", "<i4"), ("diag_min", "<i4"), ("diag_max", "<i4"), ("reserved", "<i4")])
UNGAPPED_DTYPE = np.dtype([("score", "<i4"), ("diag", "<i4"), ("end_query", "<i4"), ("end_ref", "<i4")])
BAD = (-1, 0, -1, -1)


def symbols(seq, mapper, size):
    """The matrix row / column of every byte: mapper[b], and the last symbol for a byte the mapper does not place inside the matrix."""
    m = np.asarray(mapper, dtype=np.int64)[np.frombuffer(bytes(seq), dtype=np.uint8)]
    return np.where((m < 0) | (m >= size), size - 1, m)


def windows(qseqs, rseqs, pairs, byte, kind, code=translate_ref.CODE_STD, max_qlen=INT32_MAX, max_rlen=INT32_MAX):
    """[(oriented query window, reference window) or None for a bad candidate]: kind "strand" -- the byte is a strand (None: all
    forward), 2 and above is bad; kind "frame" -- a frame 0 .. 5 of the query (None: all 0), translated with `code`, max_qlen in
    letters; a frame that holds no codon is bad."""
    if kind == "strand":
        return pairs_ex_ref.resolve(qseqs, rseqs, pairs, byte, max_qlen, max_rlen)
    assert kind == "frame"
    frames = np.zeros(len(pairs), dtype=np.uint8) if byte is None else byte
    return translate_ref.resolve(qseqs, rseqs, pairs, [int(f) for f in frames], max_qlen, max_rlen, code)


def ungapped_window(x, y, r_beg, diag_min, diag_max, scores, mapper):
    """One candidate whose windows are good.  x: the oriented query, y: the reference window that starts at r_beg of its sequence;
    diagonals d = j - i with j in the WHOLE reference.  -> (score, diag, end_query, end_ref)."""
    if diag_min > diag_max:
        return BAD
    scores = np.asarray(scores, dtype=np.int64)
    size = scores.shape[0]
    sx, sy = symbols(x, mapper, size), symbols(y, mapper, size)
    L, rl = len(sx), len(sy)
    best = (0, int(diag_min), -1, -1)
    lo, hi = max(int(diag_min), r_beg - (L - 1)), min(int(diag_max), r_beg + rl - 1)       # the diagonals that have a cell
    for d in range(lo, hi + 1):
        i0, i1 = max(0, r_beg - d), min(L, r_beg + rl - d)                                   # r_beg <= i + d < r_beg + rl
        w = scores[sx[i0:i1], sy[i0 + d - r_beg:i1 + d - r_beg]].tolist()
        h = 0
        for t, v in enumerate(w):
            h = max(0, h + v)
            if h > best[0]:                                                                  # ascending d, ascending i: the first wins
                best = (h, d, i0 + t, i0 + t + d)
    return best


def ungapped(qseqs, rseqs, pairs, byte, seeds, scores, mapper, kind="strand", code=translate_ref.CODE_STD, max_qlen=INT32_MAX,
             max_rlen=INT32_MAX):
    """UNGAPPED_DTYPE array, one record per candidate."""
    out = np.zeros(len(pairs), dtype=UNGAPPED_DTYPE)
    win = windows(qseqs, rseqs, pairs, byte, kind, code, max_qlen, max_rlen)
    for k, xy in enumerate(win):
        if xy is None:
            out[k] = BAD
        else:
            out[k] = ungapped_window(xy[0], xy[1], int(pairs[k]["r_beg"]), int(seeds[k]["diag_min"]), int(seeds[k]["diag_max"]), scores, mapper)
    return out


def select(score, row_off, min_score=0, top_n=0):
    """-> (kept: ascending indices into the list, new row_off).  A candidate passes iff score >= max(min_score, 0); with top_n > 0 a
    row keeps its top_n best passing candidates by (score descending, position ascending); kept candidates stay in input order."""
    score = np.asarray(score, dtype=np.int64)
    floor = max(int(min_score), 0)
    kept = []
    off = [0]
    for a, z in zip(row_off[:-1], row_off[1:]):
        row = [x for x in range(int(a), int(z)) if score[x] >= floor]
        if top_n > 0:
            row = sorted(sorted(row, key=lambda x: (-score[x], x))[:top_n])
        kept += row
        off.append(len(kept))
    return np.array(kept, dtype=np.int64), np.array(off, dtype=np.int64)


def filter_hits(qseqs, rseqs, row_off, pairs, byte, seeds, scores, mapper, kind="strand", min_score=0, top_n=0, code=translate_ref.CODE_STD,
                max_qlen=INT32_MAX, max_rlen=INT32_MAX, capacity=None):
    """The filter's outputs: row_off and counts in full, the columns of the kept candidates below `capacity` (None: all)."""
    ung = ungapped(qseqs, rseqs, pairs, byte, seeds, scores, mapper, kind, code, max_qlen, max_rlen)
    kept, off = select(ung["score"], row_off, min_score, top_n)
    w = len(kept) if capacity is None else min(len(kept), capacity)
    src = kept[:w]
    b = np.zeros(len(pairs), dtype=np.uint8) if byte is None else np.asarray(byte, dtype=np.uint8)
    return {"row_off": off, "counts": [len(kept), w], "pairs": np.ascontiguousarray(pairs[src]), "byte": np.ascontiguousarray(b[src]),
            "seeds": np.ascontiguousarray(seeds[src]), "ungapped": np.ascontiguousarray(ung[src]), "source": src, "all_ungapped": ung}
