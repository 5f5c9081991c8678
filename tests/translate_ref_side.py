"""The reference-side translated set entries (include/parasail_amd.h, pmx_*_translated_ref[_device]) in plain Python: everything but
the side is translate_ref.py's -- the code, translate(), tlen(), stored_bytes() (with r_beg for q_beg), fold(), search() and topk()
-- so this module adds only the resolve step with the sides exchanged: Q holds proteins, R nucleotides, max_rlen bounds the
translated length."""
import pairs_ref
import set_search_ref                                   # noqa: F401  (what search() and topk() of translate_ref rest on)
import topk_ref                                         # noqa: F401
import translate_ref
from translate_ref import (FRAMES_FORWARD, FRAMES_REVERSE, FRAMES_ALL, CODE_STD, BASES, frames_of, tlen, translate,      # noqa: F401
                           stored_bytes, fold, search, topk)


def resolve(qseqs, rseqs, pairs, frames, max_qlen=pairs_ref.INT32_MAX, max_rlen=pairs_ref.INT32_MAX, code=CODE_STD):
    """[(query window, translated reference) or None] per pair and its frame byte: None for a bad descriptor, a frame byte above 5,
    a frame that does not exist and a translation longer than max_rlen."""
    out = []
    for p, f in zip(pairs, frames):
        q = pairs_ref.resolve_side(qseqs, p["q"], p["q_beg"], p["q_len"], max_qlen)
        r = pairs_ref.resolve_side(rseqs, p["r"], p["r_beg"], p["r_len"])
        if q is None or r is None or f > 5 or not 1 <= tlen(len(r), f) <= max_rlen:
            out.append(None)
        else:
            out.append((q, translate_ref.translate(r, int(f), code)))
    return out
