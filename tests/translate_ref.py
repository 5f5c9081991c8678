"""Plain Python / numpy restatement of the translated set entries (include/parasail_amd.h, pmx_*_translated[_device]): the genetic
code, the translation of a nucleotide window per frame, which frames exist, the fold over frames, the map from a letter of the
translated query back to stored bytes, and search / top-K on folded records (set_search_ref.py and topk_ref.py do what is unchanged)."""
import numpy as np

import pairs_ref
import set_search_ref
import topk_ref
from pairs_ex_ref import revcomp

FRAMES_FORWARD, FRAMES_REVERSE, FRAMES_ALL = 6, 7, 8
BASES = "TCAG"                                          # NCBI order: index = 16 b0 + 4 b1 + b2
CODE_STD = b"FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
_CLASS = {ord(c): i for i, c in enumerate(BASES)}
_CLASS.update({ord(c.lower()): i for i, c in enumerate(BASES)})
_CLASS[ord("U")] = _CLASS[ord("u")] = 0                 # U reads as T


def frames_of(mode):
    """The frames a frame mode looks at, in ascending order."""
    if 0 <= mode <= 5:
        return [mode]
    return {FRAMES_FORWARD: [0, 1, 2], FRAMES_REVERSE: [3, 4, 5], FRAMES_ALL: [0, 1, 2, 3, 4, 5]}[mode]


def tlen(w, frame):
    """Letters of a window of w nucleotides in a frame (0: the frame does not exist)."""
    return max(w - frame % 3, 0) // 3


def translate(window, frame, code=CODE_STD):
    """The translated query of a nucleotide window (bytes) in frame 0 .. 5; b"" when the frame does not exist."""
    assert 0 <= frame <= 5
    s = revcomp(window) if frame >= 3 else bytes(window)
    off = frame % 3
    out = bytearray()
    for p in range(tlen(len(s), frame)):
        c = [_CLASS.get(b) for b in s[off + 3 * p: off + 3 * p + 3]]
        out.append(ord("X") if None in c else code[16 * c[0] + 4 * c[1] + c[2]])
    return bytes(out)


def stored_bytes(q_beg, w, frame, p):
    """The three sequence byte positions letter p of the translated window (q_beg, w) was read from, in reading order."""
    off = frame % 3
    if frame < 3:
        return [q_beg + off + 3 * p + x for x in range(3)]
    return [q_beg + w - 1 - (off + 3 * p) - x for x in range(3)]


def resolve(qseqs, rseqs, pairs, frames, max_qlen=pairs_ref.INT32_MAX, max_rlen=pairs_ref.INT32_MAX, code=CODE_STD):
    """[(translated query, reference window) or None] per pair and its frame byte: None for a bad descriptor, a frame byte above 5,
    a frame that does not exist and a translation longer than max_qlen."""
    out = []
    for p, f in zip(pairs, frames):
        q = pairs_ref.resolve_side(qseqs, p["q"], p["q_beg"], p["q_len"])
        r = pairs_ref.resolve_side(rseqs, p["r"], p["r_beg"], p["r_len"], max_rlen)
        if q is None or r is None or f > 5 or not 1 <= tlen(len(q), f) <= max_qlen:
            out.append(None)
        else:
            out.append((translate(q, int(f), code), r))
    return out


def fold(recs, exists, stats=None, frames=(0, 1, 2, 3, 4, 5)):
    """recs: int32 [len(frames), n, 4] of the single-frame runs; exists: bool [len(frames), n].  -> (records [n, 4], statistics or
    None, frame bytes): the highest score among the frames that exist, the lowest frame on a tie; no frame: the bad record, frame 0."""
    recs = np.asarray(recs)
    n = recs.shape[1]
    out = np.tile(np.array(pairs_ref.BAD_RECORD, dtype=np.int32), (n, 1))
    st = np.zeros((n, 3), dtype=np.int32) if stats is not None else None
    won = np.zeros(n, dtype=np.uint8)
    for k in range(n):
        best = None
        for x, f in enumerate(frames):
            if exists[x][k] and (best is None or int(recs[x, k, 0]) > int(recs[best, k, 0])):
                best = x
        if best is not None:
            out[k] = recs[best, k]
            won[k] = frames[best]
            if stats is not None:
                st[k] = stats[best][k]
    return out, st, won


def search(rec, won, min_score, first=0, descs=None, stats=None, capacity=None):
    """set_search_ref.hits on folded records, with the hits' frames."""
    h = set_search_ref.hits(rec, min_score, first, descs, stats, capacity)
    h["frame"] = won[h["index"] - first]
    return h


def topk(rec, won, nr, q_first, nq, k, min_score=topk_ref.INT32_MIN, stats=None, capacity=None):
    """topk_ref.topk on folded records (rows q_first .. of the rectangle), with the hits' frames."""
    t = topk_ref.topk(rec, nr, q_first, nq, k, min_score, False, stats, capacity)
    t["frame"] = won[t["index"] - q_first * nr]
    return t
