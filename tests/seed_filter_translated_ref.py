"""Plain Python restatement of the ungapped diagonal filter for the codon and translated-index lists (include/parasail_amd.h,
pmx_seed_ungapped_translated / pmx_seed_filter_translated): which cells a seed record's diagonals mean per list kind, the walk
order, the record and the bad candidates.  The windows come from the helpers that already restate the three gathers --
frameshift_ref.codon_stream, frameshift_ref_side.stream, translate_ref_side.resolve --, the selection is seed_filter_ref.select.
Written from the specification; nothing here reads the library."""
import numpy as np

import frameshift_ref
import frameshift_ref_side
import pairs_ref
import seed_filter_ref
import translate_ref
import translate_ref_side
from seed_filter_ref import BAD, SEED_HIT_DTYPE, UNGAPPED_DTYPE, symbols          # noqa: F401

INT32_MAX = pairs_ref.INT32_MAX
LIST_CODONS, LIST_REF_FRAMES, LIST_REF_CODONS = 1, 2, 3
KINDS = {"codons": LIST_CODONS, "ref_frames": LIST_REF_FRAMES, "ref_codons": LIST_REF_CODONS}


def _walk(best, D, cells, scores, sa, sb, record):
    """One diagonal: cells [(a, b)] in walking order, a / b indices into the symbol arrays; record(a, b) -> (end_query, end_ref).
    -> the best so far, replaced only by a higher h (ascending D, ascending cell: the first wins)."""
    h = 0
    for a, b in cells:
        h = max(0, h + int(scores[sa[a], sb[b]]))
        if h > best[0]:
            best = (h, D) + record(a, b)
    return best


def codons_window(T, y, r_beg, diag_min, diag_max, scores, mapper):
    """LIST_CODONS, a good candidate.  T: the codon stream of the oriented query window, y: the reference window that starts at r_beg.
    Cell (n, j): n = 3 j - D.  -> (U, D, n + 2, j)."""
    if diag_min > diag_max:
        return BAD
    scores = np.asarray(scores, dtype=np.int64)
    sT, sy = symbols(T, mapper, scores.shape[0]), symbols(y, mapper, scores.shape[0])
    best = (0, int(diag_min), -1, -1)
    lo, hi = max(int(diag_min), 3 * r_beg - (len(T) - 1)), min(int(diag_max), 3 * (r_beg + len(y) - 1))
    for D in range(lo, hi + 1):
        cells = [(3 * j - D, j - r_beg) for j in range(r_beg, r_beg + len(y)) if 0 <= 3 * j - D < len(T)]
        best = _walk(best, D, cells, scores, sT, sy, lambda n, jr: (n + 2, jr + r_beg))
    return best


def ref_codons_window(x, T, lo, diag_min, diag_max, scores, mapper):
    """LIST_REF_CODONS, a good candidate.  x: the query window, T: the codon stream of the oriented reference window that starts at
    oriented position lo of the whole sequence.  Cell (p, X): X = D + 3 p.  -> (U, D, p, X + 2)."""
    if diag_min > diag_max:
        return BAD
    scores = np.asarray(scores, dtype=np.int64)
    sx, sT = symbols(x, mapper, scores.shape[0]), symbols(T, mapper, scores.shape[0])
    best = (0, int(diag_min), -1, -1)
    a, z = max(int(diag_min), lo - 3 * (len(x) - 1)), min(int(diag_max), lo + len(T) - 1)
    for D in range(a, z + 1):
        cells = [(p, D + 3 * p - lo) for p in range(len(x)) if 0 <= D + 3 * p - lo < len(T)]
        best = _walk(best, D, cells, scores, sx, sT, lambda p, t: (p, t + lo + 2))
    return best


def frame_origin(N, r_beg, r_len, byte, g):
    """LIST_REF_FRAMES: the letter lb of sequence frame g's whole translation at which the window's translation starts, or None for
    a byte other than 0 or 3, g outside 0 .. 5 or on the other strand, and a window that is not codon-aligned for g."""
    if byte not in (0, 3) or not 0 <= g <= 5 or g // 3 != byte // 3:
        return None
    off = g % 3
    lead = r_beg - off if byte == 0 else N - off - (r_beg + r_len)
    return lead // 3 if lead % 3 == 0 else None


def ungapped(qseqs, rseqs, pairs, byte, seeds, scores, mapper, kind, code=translate_ref.CODE_STD, max_qlen=INT32_MAX, max_rlen=INT32_MAX):
    """UNGAPPED_DTYPE array, one record per candidate.  kind: "codons", "ref_frames" or "ref_codons"; byte None: all 0."""
    assert kind in KINDS
    out = np.zeros(len(pairs), dtype=UNGAPPED_DTYPE)
    b = np.zeros(len(pairs), dtype=np.uint8) if byte is None else np.asarray(byte, dtype=np.uint8)
    if kind == "ref_frames":
        win = translate_ref_side.resolve(qseqs, rseqs, pairs, [int(f) for f in b], max_qlen, max_rlen, code)
    for k, p in enumerate(pairs):
        dmin, dmax = int(seeds[k]["diag_min"]), int(seeds[k]["diag_max"])
        s = int(b[k])
        rec = BAD
        if kind == "codons":
            q = pairs_ref.resolve_side(qseqs, p["q"], p["q_beg"], p["q_len"])
            r = pairs_ref.resolve_side(rseqs, p["r"], p["r_beg"], p["r_len"], max_rlen)
            if q is not None and r is not None and s <= 1 and len(q) >= 3 and len(q) - 2 <= max_qlen:
                rec = codons_window(frameshift_ref.codon_stream(q, s, code), r, int(p["r_beg"]), dmin, dmax, scores, mapper)
        elif kind == "ref_codons":
            q = pairs_ref.resolve_side(qseqs, p["q"], p["q_beg"], p["q_len"], max_qlen)
            r = pairs_ref.resolve_side(rseqs, p["r"], p["r_beg"], p["r_len"])
            if q is not None and r is not None and s <= 1 and len(r) >= 3 and len(r) - 2 <= max_rlen:
                N = len(rseqs[int(p["r"])])
                lo = int(p["r_beg"]) if s == 0 else N - (int(p["r_beg"]) + len(r))
                rec = ref_codons_window(q, frameshift_ref_side.stream(r, s, code), lo, dmin, dmax, scores, mapper)
        elif win[k] is not None:
            N = len(rseqs[int(p["r"])])
            r_len = len(pairs_ref.resolve_side(rseqs, p["r"], p["r_beg"], p["r_len"]))
            lb = frame_origin(N, int(p["r_beg"]), r_len, s, int(seeds[k]["reserved"]))
            if lb is not None:
                rec = seed_filter_ref.ungapped_window(win[k][0], win[k][1], lb, dmin, dmax, scores, mapper)
        out[k] = rec
    return out


def filter_hits(qseqs, rseqs, row_off, pairs, byte, seeds, scores, mapper, kind, min_score=0, top_n=0, code=translate_ref.CODE_STD,
                max_qlen=INT32_MAX, max_rlen=INT32_MAX, capacity=None, ung=None):
    """The filter's outputs: row_off and counts in full, the columns of the kept candidates below `capacity` (None: all).  ung: the
    list's records where the caller has them already (the "all_ungapped" of an earlier call with the same list and maxima)."""
    if ung is None:
        ung = ungapped(qseqs, rseqs, pairs, byte, seeds, scores, mapper, kind, code, max_qlen, max_rlen)
    kept, off = seed_filter_ref.select(ung["score"], row_off, min_score, top_n)
    w = len(kept) if capacity is None else min(len(kept), capacity)
    src = kept[:w]
    b = np.zeros(len(pairs), dtype=np.uint8) if byte is None else np.asarray(byte, dtype=np.uint8)
    return {"row_off": off, "counts": [len(kept), w], "pairs": np.ascontiguousarray(pairs[src]), "byte": np.ascontiguousarray(b[src]),
            "seeds": np.ascontiguousarray(seeds[src]), "ungapped": np.ascontiguousarray(ung[src]), "source": src, "all_ungapped": ung}
