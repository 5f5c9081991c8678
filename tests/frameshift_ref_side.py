"""The CPU model of the reference-side frameshift-aware entries (include/parasail_amd.h, "Frameshift-aware translated search, reference
side") for the tests: tests/swfsc_model.c compiled on first use, and what the tests need around it -- records of a pair list with
the bad-pair rule, search and top-K results built from those records, and a path enumerator without dynamic programming."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import pairs_ref
import translate_ref

HERE = os.path.dirname(os.path.abspath(__file__))
STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = 0, 1, 2
BAD = list(pairs_ref.BAD_RECORD)
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tempfile.mkdtemp(prefix="swfsc_model"), "swfsc_model.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "swfsc_model.c")], check=True)
        _lib = C.CDLL(so)
        _lib.swfsc_stream.restype = C.c_int
        _lib.swfsc_align.restype = None
        _lib.swfsc_pair.restype = None
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _ll(x):
    return C.c_longlong(int(x))


def stream(window, strand=0, code=translate_ref.CODE_STD):
    w = np.frombuffer(bytes(window), dtype=np.uint8)
    out = np.zeros(max(len(w), 1), dtype=np.uint8)
    cd = np.frombuffer(bytes(code), dtype=np.uint8)
    n = lib().swfsc_stream(_p(w), len(w), int(strand), _p(cd), _p(out))
    return out[:n].tobytes()


def align(q, T, om, open_, ext, fs, no_shift=False):
    """the recurrence over a protein q (rows) and a codon stream T (columns) -> [score, end_query, end_ref, flags]; om: an oracle Matrix"""
    qq = np.frombuffer(bytes(q), dtype=np.uint8); t = np.frombuffer(bytes(T), dtype=np.uint8)
    rec = np.zeros(4, dtype=np.int32)
    lib().swfsc_align(_p(qq), len(qq), _p(t), len(t), _p(om.scores), _p(om.mapper), om.size, _ll(open_), _ll(ext), _ll(fs),
                      1 if no_shift else 0, _p(rec))
    return rec.tolist()


def pair(q, window, mode, om, open_, ext, fs, code=translate_ref.CODE_STD, no_shift=False):
    qq = np.frombuffer(bytes(q), dtype=np.uint8); w = np.frombuffer(bytes(window), dtype=np.uint8)
    cd = np.frombuffer(bytes(code), dtype=np.uint8)
    rec = np.zeros(4, dtype=np.int32); strand = np.zeros(1, dtype=np.uint8)
    lib().swfsc_pair(_p(qq), len(qq), _p(w), len(w), int(mode), _p(cd), _p(om.scores), _p(om.mapper), om.size, _ll(open_), _ll(ext),
                     _ll(fs), 1 if no_shift else 0, _p(rec), _p(strand))
    return rec.tolist(), int(strand[0])


def records(qseqs, rseqs, pairs, mode, om, open_, ext, fs, strands=None, max_qlen=pairs_ref.INT32_MAX, max_rlen=pairs_ref.INT32_MAX,
            code=translate_ref.CODE_STD):
    """the device entries' records and strand bytes of a pair list: mode for all pairs, or (mode 0) one strand byte per pair; a bad
    descriptor, a query beyond max_qlen, a strand byte above 1, W < 3 and W - 2 > max_rlen give the bad record and strand 0"""
    rec = np.zeros((len(pairs), 4), dtype=np.int32); won = np.zeros(len(pairs), dtype=np.uint8)
    for k, d in enumerate(pairs):
        q = pairs_ref.resolve_side(qseqs, d["q"], d["q_beg"], d["q_len"], max_qlen)
        r = pairs_ref.resolve_side(rseqs, d["r"], d["r_beg"], d["r_len"])
        m = mode if strands is None else int(strands[k])
        if q is None or r is None or len(r) < 3 or len(r) - 2 > max_rlen or (strands is not None and m > 1):
            rec[k] = BAD
            continue
        rec[k], won[k] = pair(q, r, m, om, open_, ext, fs, code)
    return rec, won


def rect_records(qseqs, rseqs, mode, om, open_, ext, fs):
    """records [nq, nr, 4] and strands [nq, nr] of the whole rectangle, whole sequences"""
    rec = np.zeros((len(qseqs), len(rseqs), 4), dtype=np.int32); won = np.zeros((len(qseqs), len(rseqs)), dtype=np.uint8)
    for i, q in enumerate(qseqs):
        for j, r in enumerate(rseqs):
            rec[i, j], won[i, j] = pair(q, r, mode, om, open_, ext, fs)
    return rec, won


def search(rec, won, min_score):
    """the hits of a rectangle's records in row-major order -> (index, records, strands)"""
    nq, nr = won.shape
    idx = [i * nr + j for i in range(nq) for j in range(nr) if rec[i, j, 0] >= min_score]
    return (np.array(idx, dtype=np.int64), np.array([rec[p // nr, p % nr] for p in idx], dtype=np.int32).reshape(-1, 4),
            np.array([won[p // nr, p % nr] for p in idx], dtype=np.uint8))


def topk(rec, won, k, min_score):
    """per row the best k references at or above min_score in (score descending, reference index ascending) order
    -> (row_off, reference indices, records, strands)"""
    nq, nr = won.shape
    off, refs = [0], []
    for i in range(nq):
        cand = sorted((j for j in range(nr) if rec[i, j, 0] >= min_score), key=lambda j: (-int(rec[i, j, 0]), j))[:k]
        refs += [(i, j) for j in cand]
        off.append(len(refs))
    return (np.array(off, dtype=np.int64), np.array([j for _, j in refs], dtype=np.int64),
            np.array([rec[i, j] for i, j in refs], dtype=np.int32).reshape(-1, 4), np.array([won[i, j] for i, j in refs], dtype=np.uint8))


def brute(q, T, score, open_, ext, fs):
    """the best local path by enumeration, no table.  A path starts with a match at any cell and goes on step by step: a match that
    advances the query by one row and the stream by 3 (free), 2 or 4 (fs each) columns; one query letter against a gap (one row down,
    the column stays); one whole reference codon against a gap (three columns on, the row stays).  Gap runs are affine: a gap step
    costs open, or ext when it continues a run of its own kind.  The best running sum over all paths and prefixes, at least 0.
    score(query letter, reference letter).  A prefix that is not positive is dropped: the path that starts behind it is enumerated too
    and is no worse."""
    m, N = len(q), len(T)
    best = 0

    def walk(i, j, total, last):
        nonlocal best
        if total > best:
            best = total
        if total <= 0:
            return
        for dj, cost in ((3, 0), (2, fs), (4, fs)):
            if i + 1 < m and j + dj < N:
                walk(i + 1, j + dj, total - cost + score(q[i + 1], T[j + dj]), "M")
        if i + 1 < m:
            walk(i + 1, j, total - (min(open_, ext) if last == "F" else open_), "F")
        if j + 3 < N:
            walk(i, j + 3, total - (min(open_, ext) if last == "E" else open_), "E")

    for i in range(m):
        for j in range(N):
            walk(i, j, score(q[i], T[j]), "M")
    return best
