"""CPU tier of the strand modes (PMX_STRAND_*): exported symbols, constants and struct layouts, every refusal that needs no GPU
(wrapped sets whose pointers are never followed), each with a pmx_last_error() text that names the reason, and the fold rule of
tests/strands_ref.py against a brute-force maximum."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import strands_ref as ref
from test_set_search_args import _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_align_pairs_both_device", "pmx_align_pairs_both", "pmx_search_pairs_stranded_device", "pmx_search_pairs_stranded",
           "pmx_strand_hits_free", "pmx_search_topk_stranded_device", "pmx_search_topk_stranded", "pmx_topk_strand_hits_free")


def _header():
    return open(os.path.join(ROOT, "include", "parasail_amd.h")).read()


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_symbols_are_exported_and_declared(pkg):
    text = _header()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name, value in (("FORWARD", 0), ("REVERSE", 1), ("BOTH", 2)):
        assert re.search(r"#define PMX_STRAND_%s\s+%d\b" % (name, value), text)
        assert getattr(pkg, "STRAND_" + name) == getattr(ref, "STRAND_" + name) == value
    for name in ("align_pairs_both_device", "search_pairs_stranded_device", "search_topk_stranded_device"):
        assert hasattr(pkg, name), name


def test_struct_layouts_match_the_header(pkg):
    text = _header()
    for struct, ctype, old, old_size, names in (
            ("pmx_strand_hits", pkg.pmx_strand_hits_t, "pmx_pair_hits", 48, ["n_hits", "n_passing", "pairs", "index", "recs", "stats", "strand"]),
            ("pmx_topk_strand_hits", pkg.pmx_topk_strand_hits_t, "pmx_topk_hits", 72,
             ["n_rows", "n_hits", "n_passing", "row_off", "row_passing", "pairs", "index", "recs", "stats", "strand"])):
        fields, size = _layout(text, struct, struct + "_t")
        assert size == old_size + 8 == C.sizeof(ctype)
        assert [f[0] for f in fields] == names
        for name, o, sz in fields:
            assert getattr(ctype, name).offset == o and getattr(ctype, name).size == sz, name
        before, bsize = _layout(text, old, old + "_t")                      # the existing result is a prefix, unchanged
        assert bsize == old_size == C.sizeof(getattr(pkg, old + "_t")) and before == fields[:-1]
    # the existing option structs keep their sizes
    assert _layout(text, "pmx_pair_search_opts", "pmx_pair_search_opts_t")[1] == 32 == C.sizeof(pkg.pmx_pair_search_opts_t)
    assert _layout(text, "pmx_topk_opts", "pmx_topk_opts_t")[1] == 32 == C.sizeof(pkg.pmx_topk_opts_t)


def _cfg(pkg, pm, want=0):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, want, pm.inner)


def test_refusals_without_gpu(pkg):
    """wrapped sets over addresses that are never followed: every case ends before any GPU work"""
    L = pkg.lib
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    pssm = pkg.Matrix.create_pssm(b"ACGT", [1, -1, -1, -1] * 8, 8)
    cfg = _cfg(pkg, pm)
    S = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    T = pkg.SeqSet.wrap_device(256, 256, 7, 700)
    s, t = S.inner, T.inner
    O = pkg.pmx_pairs_opts_t
    TRI, RECT, LIST = pkg.PAIRS_TRIANGLE, pkg.PAIRS_RECT, pkg.PAIRS_LIST
    FWD, REV, BOTH = pkg.STRAND_FORWARD, pkg.STRAND_REVERSE, pkg.STRAND_BOTH
    pairs = np.zeros(4, dtype=pkg.PAIR_DTYPE)
    out = np.zeros((4, 4), dtype=np.int32)
    won = np.zeros(4, dtype=np.uint8)

    # ---- listed pairs on both strands
    def both_dev(c=cfg, q=s, r=t, n=4, p=256, mq=8, mr=8, o=256, st=None, so=256, opts=None):
        return L.pmx_align_pairs_both_device(C.byref(c), q, r, n, p, mq, mr, o, st, so, None, C.byref(opts) if opts is not None else None)

    def both_host(c=cfg, q=s, r=t, n=4, p=pairs.ctypes.data, o=out.ctypes.data, st=None, so=won.ctypes.data, opts=None, **_):
        return L.pmx_align_pairs_both(C.byref(c), q, r, n, p, o, st, so, C.byref(opts) if opts is not None else None)

    for entry in (both_dev, both_host):
        assert entry(so=None) == -1 and "null strand output" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR)) == -1 and "CIGAR" in _err(pkg) and "pmx_align_pairs_ex" in _err(pkg) and "strand bytes" in _err(pkg)
        assert entry(c=_cfg(pkg, pssm)) == -1 and "PSSM" in _err(pkg) and "reversed query" in _err(pkg)
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(n=-1) == -1 and "negative n" in _err(pkg)
        assert entry(p=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(o=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(7, 0, 5, 2, 0, 0, pm.inner)) == -1 and "mode" in _err(pkg)
        assert entry(n=0, so=None) == 0                                                    # n == 0 touches nothing
    assert both_dev(c=_cfg(pkg, pm, pkg.WANT_STATS)) == -1 and "stats requested without a stats buffer" in _err(pkg)
    assert both_dev(mq=0) == -1 and "max_qlen" in _err(pkg)

    # ---- set search with a strand mode
    def sdev(c=cfg, q=s, r=None, shape=TRI, first=0, n=4, p=None, mq=8, mr=8, ms=0, hp=256, hi=256, hr=256, hs=None, cap=16, cnt=256, opts=None,
             mode=BOTH, hb=256):
        return L.pmx_search_pairs_stranded_device(C.byref(c), q, r, shape, first, n, p, mq, mr, ms, hp, hi, hr, hs, cap, cnt, None,
                                                  C.byref(opts) if opts is not None else None, mode, hb)

    def shost(c=cfg, q=s, r=None, shape=TRI, first=0, n=4, p=None, max_hits=0, chunk=0, sl=0, mode=BOTH, **_):
        res = C.POINTER(pkg.pmx_strand_hits_t)()
        o = pkg.pmx_pair_search_opts_t(0, shape, max_hits, chunk, sl)
        rc = L.pmx_search_pairs_stranded(C.byref(c), q, r, first, n, p, C.byref(o), mode, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_passing == 0 and res.contents.strand
            L.pmx_strand_hits_free(res)
        else:
            assert not res
        return rc

    for entry in (sdev, shost):
        for mode in (-1, 3, 255):
            assert entry(mode=mode) == -1 and "strand mode %d is outside 0 .. 2" % mode in _err(pkg)
        for mode in (REV, BOTH):
            assert entry(c=_cfg(pkg, pssm), mode=mode) == -1 and "PSSM" in _err(pkg) and "reversed query" in _err(pkg)
        for mode in (FWD, REV, BOTH):
            assert entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR), mode=mode) == -1 and "CIGAR" in _err(pkg) and "pmx_align_pairs_ex" in _err(pkg)
            assert entry(shape=3, mode=mode) == -1 and "unknown pair shape 3" in _err(pkg)
            assert entry(shape=TRI, r=t, mode=mode) == -1 and "R must be NULL or Q" in _err(pkg)
            assert entry(shape=RECT, r=None, mode=mode) == -1 and "null sequence set" in _err(pkg)
            assert entry(shape=LIST, r=t, p=None, mode=mode) == -1 and "null pairs" in _err(pkg)
            assert entry(shape=RECT, r=t, first=67, n=4, mode=mode) == -1 and "beyond the 70 pairs of 10 x 7" in _err(pkg)
            assert entry(n=-1, mode=mode) == -1 and "negative" in _err(pkg)
            kw = {"cnt": None} if entry is sdev else {}
            assert entry(n=0, mode=mode, **kw) == 0
    assert sdev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    assert sdev(hr=None) == -1 and "null hit records" in _err(pkg)
    assert sdev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert sdev(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
    assert sdev(hs=256) == -1 and "stats buffer without PMX_WANT_STATS" in _err(pkg)
    assert sdev(mq=0) == -1 and "max_qlen" in _err(pkg)
    assert sdev(hb=None, hp=None, hi=None, n=0, cnt=None) == 0                              # (optional outputs)
    assert shost(max_hits=-1) == -1 and "max_hits" in _err(pkg)
    assert shost(sl=-1) == -1 and "slice_pairs" in _err(pkg)
    o = pkg.pmx_pair_search_opts_t(0, TRI, 0, 0, 0)
    assert L.pmx_search_pairs_stranded(C.byref(cfg), s, None, 0, 4, None, C.byref(o), BOTH, None) == -1 and "null result" in _err(pkg)
    L.pmx_strand_hits_free(None)

    # ---- top-K with a strand mode
    def tdev(c=cfg, q=s, r=t, qf=0, nq=4, mq=8, mr=8, ms=0, k=3, skip=0, hp=256, hi=256, hr=256, hs=None, cap=16, off=256, rp=256, cnt=256, opts=None,
             mode=BOTH, hb=256):
        return L.pmx_search_topk_stranded_device(C.byref(c), q, r, qf, nq, mq, mr, ms, k, skip, hp, hi, hr, hs, cap, off, rp, cnt, None,
                                                 C.byref(opts) if opts is not None else None, mode, hb)

    def thost(c=cfg, q=s, r=t, qf=0, nq=4, k=3, skip=0, chunk=0, sl=0, mode=BOTH, **_):
        res = C.POINTER(pkg.pmx_topk_strand_hits_t)()
        o = pkg.pmx_topk_opts_t(0, k, skip, chunk, sl)
        rc = L.pmx_search_topk_stranded(C.byref(c), q, r, qf, nq, C.byref(o), mode, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_rows == 0 and res.contents.strand
            L.pmx_topk_strand_hits_free(res)
        else:
            assert not res
        return rc

    for entry in (tdev, thost):
        for mode in (-1, 3):
            assert entry(mode=mode) == -1 and "strand mode %d is outside 0 .. 2" % mode in _err(pkg)
        for mode in (REV, BOTH):
            assert entry(c=_cfg(pkg, pssm), mode=mode) == -1 and "PSSM" in _err(pkg) and "reversed query" in _err(pkg)
        for mode in (FWD, REV, BOTH):
            assert entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR), mode=mode) == -1 and "CIGAR" in _err(pkg) and "pmx_align_pairs_ex" in _err(pkg)
            assert entry(k=0, mode=mode) == -1 and "k 0 is outside 1 .. 1024" in _err(pkg)
            assert entry(k=1025, mode=mode) == -1 and "k 1025 is outside" in _err(pkg)
            assert entry(skip=1, mode=mode) == -1 and "skip_self needs R to be Q" in _err(pkg)
            assert entry(qf=8, nq=3, mode=mode) == -1 and "beyond the 10 sequences" in _err(pkg)
            assert entry(nq=-1, mode=mode) == -1 and "negative" in _err(pkg)
            kw = {"cnt": None, "off": None} if entry is tdev else {}
            assert entry(nq=0, mode=mode, **kw) == 0
    assert tdev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    assert tdev(hr=None) == -1 and "null hit records" in _err(pkg)
    assert tdev(off=None) == -1 and "null row offsets" in _err(pkg)
    assert tdev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert tdev(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
    assert thost(sl=-1) == -1 and "slice_rows" in _err(pkg)
    L.pmx_topk_strand_hits_free(None)


def test_python_mirror_defaults_and_refusals(pkg):
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    for strand in (0, "both", pkg.STRAND_REVERSE):
        h = al.search_pairs(S, min_score=5, count=0, strand=strand)
        assert isinstance(h, pkg.PairHits) and len(h) == 0 and h.strand.dtype == np.uint8 and len(h.strand) == 0
        t = al.search_topk(S, k=2, rows=0, strand=strand)
        assert isinstance(t, pkg.TopKHits) and len(t) == 0 and t.strand.dtype == np.uint8 and len(t.strand) == 0
    with pytest.raises(pkg.BatchError, match="strand mode 5"):
        al.search_pairs(S, strand=5)
    with pytest.raises(pkg.BatchError, match="strand mode 7"):
        al.search_topk(S, strand=7)
    with pytest.raises(pkg.BatchError, match="both"):
        al.search_pairs(S, strand="sideways")
    with pytest.raises(pkg.BatchError, match="both"):
        al.align_pairs(S, S, [(0, 1)], strand="sideways")
    rec, won = al.align_pairs(S, S, [], strand="both")
    assert len(rec) == 0 and won.dtype == np.uint8 and len(won) == 0


def test_fold_is_the_brute_force_maximum(pkg):
    rng = np.random.default_rng(12000)
    n = 4000
    rec0 = rng.integers(-5, 6, size=(n, 4)).astype(np.int32)                                # few distinct scores: many ties
    rec1 = rng.integers(-5, 6, size=(n, 4)).astype(np.int32)
    rec0[:, 3] = rng.integers(0, 2, size=n); rec1[:, 3] = rng.integers(0, 2, size=n)
    rec0[::50] = rec1[::50] = (0, -1, -1, 8)                                                # bad descriptors: bad on both strands
    rec0[7], rec1[7] = (-(1 << 31), 0, 0, 0), ((1 << 31) - 1, 1, 1, 1)                      # no 32-bit wrap in the comparison
    rec0[8], rec1[8] = ((1 << 31) - 1, 0, 0, 0), (-(1 << 31), 1, 1, 1)
    st0 = rng.integers(0, 100, size=(n, 3)).astype(np.int32)
    st1 = rng.integers(0, 100, size=(n, 3)).astype(np.int32)
    rec, st, strand = ref.fold(rec0, rec1, st0, st1, mode=pkg.STRAND_BOTH)
    ties = 0
    for k in range(n):
        a, b = int(rec0[k, 0]), int(rec1[k, 0])
        w = 1 if b > a else 0                                                              # the higher score; a tie goes to the forward strand
        ties += a == b
        assert int(rec[k, 0]) == max(a, b) and strand[k] == w
        assert rec[k].tolist() == (rec1 if w else rec0)[k].tolist() and st[k].tolist() == (st1 if w else st0)[k].tolist()
    assert ties > n // 20 and 0 < strand.sum() < n and strand[7] == 1 and strand[8] == 0 and (strand[::50] == 0).all()
    f = ref.fold(rec0, rec1, mode=pkg.STRAND_FORWARD)                                       # (the package's constants are the reference's)
    assert f[0].tobytes() == rec0.tobytes() and f[1] is None and not f[2].any()
    r = ref.fold(rec0, rec1, mode=pkg.STRAND_REVERSE)
    assert r[0].tobytes() == rec1.tobytes() and (r[2][::50] == 0).all() and r[2].sum() == n - len(r[2][::50])
    h = ref.search(rec0, rec1, 3, first=10)
    keep = np.nonzero(rec[:, 0] >= 3)[0]
    assert h["index"].tolist() == (keep + 10).tolist() and h["strand"].tolist() == strand[keep].tolist() and h["records"].tobytes() == rec[keep].tobytes()
    t = ref.topk(rec0[:3900], rec1[:3900], 130, 2, 30, 4)
    assert t["strand"].tolist() == strand[:3900][t["index"] - 2 * 130].tolist() and len(t["index"]) == 120
