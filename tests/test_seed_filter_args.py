"""CPU tier of the ungapped diagonal filter: exported symbols, header declarations and struct layouts, every refusal of
pmx_seed_ungapped[_device] and pmx_seed_filter[_device] that needs no GPU -- wrapped sets whose pointers are never followed --, each
with a pmx_last_error() text that names the reason, and the Python mirror's refusals.  Every call with n > 0 below ends before the
device is asked for, so it also ends before any pointer is followed on a machine that has one; the accepted edges are asked with
n == 0.  Not here: the refusal of a set of another device than the current one, which needs two devices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import seed_filter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_seed_ungapped_device", "pmx_seed_ungapped", "pmx_seed_filter_device", "pmx_seed_filter", "pmx_seed_filtered_free",
           "pmx_seed_ungapped_shape")
P = 256                                                                                      # a pointer that is never followed


def _header():
    return open(os.path.join(ROOT, "include", "parasail_amd.h")).read()


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_symbols_constants_and_layouts(pkg):
    text = _header()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name, value in (("PMX_SEED_BYTE_STRAND", 0), ("PMX_SEED_BYTE_FRAME", 1)):
        m = re.search(r"#define %s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == value and getattr(pkg, name[4:]) == value
    for name in ("seed_ungapped", "seed_ungapped_device", "seed_filter", "seed_filter_device", "UNGAPPED_DTYPE", "pmx_ungapped_t",
                 "pmx_seed_filter_opts_t", "pmx_seed_filtered_t", "ungapped_shape"):
        assert hasattr(pkg, name), name
    assert "csrc/pmx_ungap.hip" in open(os.path.join(ROOT, "parasail-rs_amd", "Makefile")).read()
    assert re.search(r"typedef struct pmx_ungapped \{ int32_t score, diag, end_query, end_ref; \} pmx_ungapped_t;", text)
    assert re.search(r"typedef struct pmx_seed_filter_opts \{ int32_t min_score, top_n, reserved\[2\]; \} pmx_seed_filter_opts_t;", text)
    assert re.search(r"typedef struct pmx_seed_filtered \{ pmx_seed_hits_t hits; pmx_ungapped_t \*ungapped; int64_t \*source; \} pmx_seed_filtered_t;", text)
    U, F, B = pkg.pmx_ungapped_t, pkg.pmx_seed_filter_opts_t, pkg.pmx_seed_filtered_t
    assert C.sizeof(U) == 16 and [(f, getattr(U, f).offset) for f in ("score", "diag", "end_query", "end_ref")] == \
        [("score", 0), ("diag", 4), ("end_query", 8), ("end_ref", 12)]
    assert C.sizeof(F) == 16 and (F.min_score.offset, F.top_n.offset, F.reserved.offset, F.reserved.size) == (0, 4, 8, 8)
    assert C.sizeof(B) == 72 and (B.hits.offset, B.ungapped.offset, B.source.offset) == (0, 56, 64)
    assert pkg.UNGAPPED_DTYPE == ref.UNGAPPED_DTYPE and pkg.UNGAPPED_DTYPE.itemsize == 16
    g, s = pkg.ungapped_shape()
    assert g == 16 and s == 4


@pytest.fixture(scope="module")
def world(pkg):
    class W:
        pass
    w = W()
    w.Q = pkg.SeqSet.wrap_device(P, P, 10, 1000)
    w.R = pkg.SeqSet.wrap_device(P, P, 5, 5000)
    w.dna = pkg.Matrix.create(b"ACGT", 2, -3)
    w.big = pkg.Matrix.create(b"ACGT", 30000, -30000)
    w.pssm = pkg.Matrix.create_pssm("ACGT", [1, -1, 0, 2] * 6, 6)
    w.cfg = lambda m=None: pkg.pmx_config_t(2, 0, 0, 0, 0, 0, (m or w.dna).inner)
    return w


def _shared_refusals(pkg, w, entry):
    """what the four entries refuse about the list, the configuration and the byte's kind: entry(**changes) -> rc"""
    assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
    assert entry(r=None) == -1 and "null sequence set" in _err(pkg)
    assert entry(n=-1) == -1 and "negative n" in _err(pkg)
    assert entry(pairs=None) == -1 and "null pairs or records" in _err(pkg)
    assert entry(seeds=None) == -1 and "null seed records" in _err(pkg)
    assert entry(chunk=-1) == -1 and "chunk_pairs must not be negative" in _err(pkg)
    assert entry(cfg=None) == -1 and "null config or matrix" in _err(pkg)
    nomat = pkg.pmx_config_t(2, 0, 0, 0, 0, 0, None)
    assert entry(cfg=nomat) == -1 and "null config or matrix" in _err(pkg)
    assert entry(cfg=w.cfg(w.pssm)) == -1 and "no PSSM" in _err(pkg)
    for bad in (2, -1, 7):
        assert entry(kind=bad) == -1 and "unknown byte_kind %d" % bad in _err(pkg) and "PMX_SEED_BYTE_FRAME" in _err(pkg)


def test_ungapped_refusals_without_gpu(pkg, world):
    w, L = world, pkg.lib

    def dev(q=w.Q.inner, r=w.R.inner, n=4, pairs=P, byte=P, kind=0, seeds=P, mq=150, mr=400, out=P, cfg=w.cfg(), chunk=0):
        o = pkg.pmx_pairs_opts_t(chunk)
        return L.pmx_seed_ungapped_device(C.byref(cfg) if cfg is not None else None, q, r, n, pairs, byte, kind, None, seeds, mq, mr, out, None, C.byref(o))

    def host(q=w.Q.inner, r=w.R.inner, n=4, pairs=P, byte=P, kind=0, seeds=P, out=P, cfg=w.cfg(), chunk=0, **unused):
        o = pkg.pmx_pairs_opts_t(chunk)
        return L.pmx_seed_ungapped(C.byref(cfg) if cfg is not None else None, q, r, n, pairs, byte, kind, None, seeds, out, C.byref(o))

    for entry in (dev, host):
        _shared_refusals(pkg, w, entry)
        assert entry(out=None) == -1 and "null pairs or records" in _err(pkg)
        for kind in (0, 1):
            assert entry(n=0, kind=kind, pairs=None, byte=None, seeds=None, out=None) == 0
    for mq, mr in ((0, 10), (10, 0), (-4, 10)):
        assert dev(mq=mq, mr=mr) == -1 and "max_qlen / max_rlen must be positive" in _err(pkg)
    # max |w| x max_qlen >= 2^31: 30000 x 71583 = 2 147 490 000 is refused, 30000 x 71582 = 2 147 460 000 fits
    assert dev(cfg=w.cfg(w.big), mq=71583) == -1 and "does not fit int32" in _err(pkg) and "30000 x 71583" in _err(pkg)
    assert dev(cfg=w.cfg(w.big), mq=71582, n=0) == 0
    assert dev(mq=(1 << 31) // 3 + 1) == -1 and "does not fit int32" in _err(pkg)            # |w| = 3
    assert dev(mq=(1 << 31) // 3, n=0) == 0


def test_filter_refusals_without_gpu(pkg, world):
    w, L = world, pkg.lib
    FO = pkg.pmx_seed_filter_opts_t

    def dev(q=w.Q.inner, r=w.R.inner, n=4, pairs=P, byte=P, kind=0, seeds=P, mq=150, mr=400, cfg=w.cfg(), chunk=0, nq=2, off=P, f=FO(0, 0),
            cap=8, ooff=P, cnt=P):
        o = pkg.pmx_pairs_opts_t(chunk)
        return L.pmx_seed_filter_device(C.byref(cfg) if cfg is not None else None, q, r, n, pairs, byte, kind, None, seeds, mq, mr, nq, off,
                                        C.byref(f) if f is not None else None, P, P, P, P, P, cap, ooff, cnt, None, C.byref(o))

    _shared_refusals(pkg, w, dev)
    for mq, mr in ((0, 10), (10, 0)):
        assert dev(mq=mq, mr=mr) == -1 and "max_qlen / max_rlen must be positive" in _err(pkg)
    assert dev(cfg=w.cfg(w.big), mq=71583) == -1 and "does not fit int32" in _err(pkg)
    assert dev(f=None) == -1 and "null filter opts" in _err(pkg)
    assert dev(f=FO(0, -1)) == -1 and "top_n -1 is negative" in _err(pkg)
    assert dev(f=FO(-1, 0)) == -1 and "min_score -1 is negative" in _err(pkg)
    for res in ((1, 0), (0, 5)):
        assert dev(f=FO(0, 0, res)) == -1 and "reserved must be 0" in _err(pkg)
    assert dev(nq=-1) == -1 and "negative nq or capacity" in _err(pkg)
    assert dev(cap=-1) == -1 and "negative nq or capacity" in _err(pkg)
    assert dev(off=None) == -1 and "null row offsets" in _err(pkg)
    assert dev(ooff=None) == -1 and "null row offsets" in _err(pkg)
    assert dev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert dev(nq=0) == -1 and "4 candidates in no row" in _err(pkg)
    assert dev(n=1 << 31) == -1 and "beyond 2^31 - 1" in _err(pkg)

    # the host entry: its own refusals, the shared ones through a pmx_seed_hits_t, and the empty list, which needs no GPU
    off = np.zeros(4, dtype=np.int64)

    def host(q=w.Q.inner, r=w.R.inner, n=4, pairs=P, byte=P, kind=0, seeds=P, cfg=w.cfg(), chunk=0, f=FO(0, 0), hits=True, passing=None,
             rows=3, row_off=off.ctypes.data, res=True, **unused):
        h = pkg.pmx_seed_hits_t(rows, n, n if passing is None else passing, row_off, pairs, byte, seeds)
        o = pkg.pmx_pairs_opts_t(chunk)
        out = C.POINTER(pkg.pmx_seed_filtered_t)()
        rc = L.pmx_seed_filter(C.byref(cfg) if cfg is not None else None, q, r, C.byref(h) if hits else None, kind, None,
                               C.byref(f) if f is not None else None, C.byref(o), C.byref(out) if res else None)
        if rc == 0:
            b = out.contents
            assert b.hits.n_rows == rows and b.hits.n_hits == 0 and b.hits.n_passing == 0
            assert [C.cast(b.hits.row_off, C.POINTER(C.c_int64))[x] for x in range(rows + 1)] == [0] * (rows + 1)
            L.pmx_seed_filtered_free(out)
        else:
            assert not out
        return rc

    _shared_refusals(pkg, w, host)
    assert host(res=False) == -1 and "null result pointer" in _err(pkg)
    assert host(hits=False) == -1 and "null hits" in _err(pkg)
    assert host(n=4, passing=9) == -1 and "max_hits cut" in _err(pkg) and "4 of 9" in _err(pkg)
    assert host(rows=-1) == -1 and "negative n_hits or n_rows" in _err(pkg)
    assert host(f=None) == -1 and "null filter opts" in _err(pkg)
    assert host(f=FO(0, -3)) == -1 and "top_n -3 is negative" in _err(pkg)
    assert host(f=FO(-2, 0)) == -1 and "min_score -2 is negative" in _err(pkg)
    assert host(f=FO(0, 0, (0, 1))) == -1 and "reserved must be 0" in _err(pkg)
    assert host(row_off=None) == -1 and "null row offsets" in _err(pkg)
    assert host(rows=0) == -1 and "4 candidates in no row" in _err(pkg)
    for kind in (0, 1):
        for f in (FO(0, 0), FO(40, 3)):
            assert host(n=0, pairs=None, byte=None, seeds=None, kind=kind, f=f) == 0
    assert host(n=0, pairs=None, byte=None, seeds=None, rows=0) == 0


def test_python_mirror_refusals_and_kinds(pkg, world):
    w = world
    S = pkg.SeqSet.wrap_device(P, P, 3, 12)
    empty = pkg.SeqSet.wrap_device(P, P, 0, 0)
    dna = pkg.SeedIndex.build(empty, 12)
    let = pkg.SeedIndex.build(empty, 4, alphabet="aa11")
    tra = pkg.SeedIndex.build(empty, 4, alphabet="aa11", translated="both")
    kinds = [(dna, {}, "strand"), (dna, {"strand": 1}, "strand"), (let, {"frames": "letters"}, "letters"), (let, {"frames": 4}, "frame"),
             (let, {"frames": "all"}, "frame"), (let, {"frames": "forward"}, "frame"), (let, {"frames": "codons"}, "codons"),
             (let, {"frames": "codons-both"}, "codons"), (tra, {"ref_frames": "frames"}, "ref_frames"), (tra, {"ref_frames": "codons"}, "ref_codons")]
    for ix, kw, kind in kinds:
        h = pkg.seed_pairs(S, ix, rows=0, **kw)
        assert h.kind == kind, kw
        if kind in ("codons", "ref_frames", "ref_codons"):
            with pytest.raises(pkg.BatchError, match="kind \"%s\"" % kind):
                pkg.seed_filter(S, S, h, w.dna)
        else:                                                                                # an empty list: no GPU work
            f = pkg.seed_filter(S, S, h, w.dna, min_score=10, top_n=2)
            assert isinstance(f, pkg.SeedHits) and f.kind == kind and len(f) == 0 and f.row_off.tolist() == [0]
            assert f.ungapped.dtype == pkg.UNGAPPED_DTYPE and len(f.ungapped) == 0 and f.source.dtype == np.int64 and len(f.source) == 0
            assert (f.frame is not None) == (kind == "frame")
    h = pkg.seed_pairs(S, dna, rows=0)
    with pytest.raises(pkg.BatchError, match="top_n -1 is negative"):
        pkg.seed_filter(S, S, h, w.dna, top_n=-1)
    with pytest.raises(pkg.BatchError, match="min_score -1 is negative"):
        pkg.seed_filter(S, S, h, w.dna, min_score=-1)
    with pytest.raises(pkg.BatchError, match="no PSSM"):
        pkg.seed_filter(S, S, h, w.pssm)
    with pytest.raises(pkg.BatchError, match="a Matrix"):
        pkg.seed_filter(S, S, h, None)
    with pytest.raises(pkg.BatchError, match="64 letters"):
        pkg.seed_filter(S, S, h, w.dna, code=b"FF")
    h.n_passing = 5
    with pytest.raises(pkg.BatchError, match="max_hits cut"):
        pkg.seed_filter(S, S, h, w.dna)
    none = np.zeros(0, dtype=pkg.PAIR_DTYPE)
    seeds = np.zeros(0, dtype=pkg.SEED_HIT_DTYPE)
    assert len(pkg.seed_ungapped(S, S, none, None, seeds, w.dna)) == 0
    assert pkg.seed_ungapped(S, S, none, None, seeds, w.dna, kind="frame", code=b"F" * 64).dtype == pkg.UNGAPPED_DTYPE
    with pytest.raises(pkg.BatchError, match="\"strand\" or \"frame\""):
        pkg.seed_ungapped(S, S, none, None, seeds, w.dna, kind="codons")
    with pytest.raises(pkg.BatchError, match="seeds and pairs differ"):
        pkg.seed_ungapped(S, S, none, None, np.zeros(2, dtype=pkg.SEED_HIT_DTYPE), w.dna)
    with pytest.raises(pkg.BatchError, match="byte and pairs differ"):
        pkg.seed_ungapped(S, S, none, np.zeros(1, dtype=np.uint8), seeds, w.dna)
    with pytest.raises(pkg.BatchError, match="no PSSM"):
        pkg.seed_ungapped(S, S, pkg.as_pairs([(0, 0)]), None, np.zeros(1, dtype=pkg.SEED_HIT_DTYPE), w.pssm)
    with pytest.raises(pkg.BatchError, match="max_qlen / max_rlen must be positive"):
        pkg.seed_ungapped_device(S, S, 1, P, None, P, 0, 5, w.dna, P)
    with pytest.raises(pkg.BatchError, match="top_n -2 is negative"):
        pkg.seed_filter_device(S, S, 1, P, None, P, 5, 5, w.dna, 1, P, None, None, None, None, None, 0, P, P, top_n=-2)
