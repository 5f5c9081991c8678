"""The CPU model of the frameshift-aware entries (include/parasail_amd.h, "Frameshift-aware translated search") for the tests:
tests/swfs_model.c compiled on first use, and what the tests need around it -- records of a pair list with the bad-pair rule, and a
path enumerator without dynamic programming that the model is held against."""
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
        so = os.path.join(tempfile.mkdtemp(prefix="swfs_model"), "swfs_model.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "swfs_model.c")], check=True)
        _lib = C.CDLL(so)
        _lib.swfs_codon_stream.restype = C.c_int
        _lib.swfs_model_align.restype = None
        _lib.swfs_model_pair.restype = None
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def codon_stream(window, strand=0, code=translate_ref.CODE_STD):
    w = np.frombuffer(bytes(window), dtype=np.uint8)
    out = np.zeros(max(len(w), 1), dtype=np.uint8)
    cd = np.frombuffer(bytes(code), dtype=np.uint8)
    n = lib().swfs_codon_stream(_p(w), len(w), int(strand), _p(cd), _p(out))
    return out[:n].tobytes()


def align(T, r, om, open_, ext, fs, no_shift=False):
    """the recurrence over a codon stream T and a protein r -> [score, end_query, end_ref, flags]; om: an oracle Matrix"""
    t = np.frombuffer(bytes(T), dtype=np.uint8); rr = np.frombuffer(bytes(r), dtype=np.uint8)
    rec = np.zeros(4, dtype=np.int32)
    lib().swfs_model_align(_p(t), len(t), _p(rr), len(rr), _p(om.scores), _p(om.mapper), om.size, int(open_), int(ext), C.c_longlong(int(fs)),
                           1 if no_shift else 0, _p(rec))
    return rec.tolist()


def pair(window, r, mode, om, open_, ext, fs, code=translate_ref.CODE_STD):
    w = np.frombuffer(bytes(window), dtype=np.uint8); rr = np.frombuffer(bytes(r), dtype=np.uint8)
    cd = np.frombuffer(bytes(code), dtype=np.uint8)
    rec = np.zeros(4, dtype=np.int32); strand = np.zeros(1, dtype=np.uint8)
    lib().swfs_model_pair(_p(w), len(w), _p(rr), len(rr), int(mode), _p(cd), _p(om.scores), _p(om.mapper), om.size, int(open_), int(ext),
                          C.c_longlong(int(fs)), _p(rec), _p(strand))
    return rec.tolist(), int(strand[0])


def records(qseqs, rseqs, pairs, mode, om, open_, ext, fs, strands=None, max_qlen=pairs_ref.INT32_MAX, max_rlen=pairs_ref.INT32_MAX,
            code=translate_ref.CODE_STD):
    """the device entries' records and strand bytes of a pair list: mode for all pairs, or (mode 0) one strand byte per pair; a bad
    descriptor, a strand byte above 1, W < 3 and W - 2 > max_qlen give the bad record and strand 0"""
    rec = np.zeros((len(pairs), 4), dtype=np.int32); won = np.zeros(len(pairs), dtype=np.uint8)
    for k, d in enumerate(pairs):
        q = pairs_ref.resolve_side(qseqs, d["q"], d["q_beg"], d["q_len"])
        r = pairs_ref.resolve_side(rseqs, d["r"], d["r_beg"], d["r_len"], max_rlen)
        m = mode if strands is None else int(strands[k])
        if q is None or r is None or len(q) < 3 or len(q) - 2 > max_qlen or (strands is not None and m > 1):
            rec[k] = BAD
            continue
        rec[k], won[k] = pair(q, r, m, om, open_, ext, fs, code)
    return rec, won


def brute(T, r, score, open_, ext, fs):
    """the best local path by enumeration, no table.  A path starts with a match at any cell and goes on step by step: a match that
    advances the stream by 3 (free), 2 or 4 (fs each) rows and the reference by one column; one reference letter against a gap (the
    row stays); one whole codon against a gap (three rows down, the column stays).  Gap runs are affine: a gap step costs open, or
    ext when it continues a run of its own kind.  The best running sum over all paths and prefixes, at least 0.  score(a, b).  A
    prefix that is not positive is dropped: the path that starts behind it is enumerated too and is no worse."""
    N, m = len(T), len(r)
    best = 0

    def walk(i, j, total, last):
        # (i, j): the cell the path has just used; last: 'M', 'E' (a reference letter against a gap) or 'F' (a codon against a gap)
        nonlocal best
        if total > best:
            best = total
        if total <= 0:
            return
        for di, cost in ((3, 0), (2, fs), (4, fs)):
            if i + di < N and j + 1 < m:
                walk(i + di, j + 1, total - cost + score(T[i + di], r[j + 1]), "M")
        if j + 1 < m:
            walk(i, j + 1, total - (min(open_, ext) if last == "E" else open_), "E")
        if i + 3 < N:
            walk(i + 3, j, total - (min(open_, ext) if last == "F" else open_), "F")

    for i in range(N):
        for j in range(m):
            walk(i, j, score(T[i], r[j]), "M")
    return best
