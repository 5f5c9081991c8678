"""CPU tier of the reference-side frameshift-aware entries (pmx_*_frameshift_ref[_device], pmx_gather_pairs_codons_ref_device): symbols,
constants and test hooks, every refusal that needs no GPU (wrapped sets whose pointers are never followed) with its pmx_last_error()
text, and the Python keywords' exclusions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_frameshift_ref_max_query", "pmx_gather_pairs_codons_ref_device", "pmx_align_pairs_frameshift_ref_device",
           "pmx_align_pairs_frameshift_ref", "pmx_search_pairs_frameshift_ref_device", "pmx_search_pairs_frameshift_ref",
           "pmx_search_topk_frameshift_ref_device", "pmx_search_topk_frameshift_ref",
           "pmx_swfsc_strip_rows", "pmx_swfsc_lane_rows", "pmx_swfsc_bound_bytes_per_slot", "pmx_swfsc_max_msize")


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_symbols_constants_and_hooks(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    cap = int(re.search(r"#define PMX_FRAMESHIFT_REF_MAX_QUERY\s+(\d+)\b", text).group(1))
    assert cap == 4096 == pkg.lib.pmx_frameshift_ref_max_query() == pkg.frameshift_ref_max_query()
    assert cap * 32767 < 1 << 28                          # the contract's reason why nothing wraps
    for name in ("gather_pairs_codons_ref_device", "align_pairs_frameshift_ref_device", "frameshift_ref_max_query", "codon_stream"):
        assert hasattr(pkg, name), name
    assert "Frameshift-aware translated search, reference side" in text and "NO CAP OF THEIR OWN" in text
    L = pkg.lib
    lane, strip = L.pmx_swfsc_lane_rows(), L.pmx_swfsc_strip_rows()
    assert lane >= 1 and strip % lane == 0 and strip // lane in (16, 64)
    assert L.pmx_swfsc_max_msize() == 128
    # two buffers of 8 bytes per column, and 256 MiB of them hold at least one workgroup's slots of a 1 Mbp window
    assert L.pmx_swfsc_bound_bytes_per_slot(1) == 16 and L.pmx_swfsc_bound_bytes_per_slot(20000) == 320000
    assert 4 * L.pmx_swfsc_bound_bytes_per_slot(1 << 20) <= 256 << 20


def _cfg(pkg, pm, mode=None, width=0, want=0):
    return pkg.pmx_config_t(pkg.MODE_SW if mode is None else mode, 0, 11, 1, width, want, pm.inner)


def test_refusals_without_gpu(pkg):
    """wrapped sets over addresses that are never followed: every case ends before any GPU work"""
    L = pkg.lib
    pm = pkg.Matrix.from_name("blosum62")
    pssm = pkg.Matrix.create_pssm(b"ACGT", [1, -1, -1, -1] * 8, 8)
    wide = pkg.Matrix.create(bytes(range(33, 33 + 128)), 2, -1)                 # 129 symbols with the wildcard
    cfg = _cfg(pkg, pm)
    S = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    T = pkg.SeqSet.wrap_device(256, 256, 7, 700)
    s, t = S.inner, T.inner
    O = pkg.pmx_pairs_opts_t
    RECT, TRI, LIST = pkg.PAIRS_RECT, pkg.PAIRS_TRIANGLE, pkg.PAIRS_LIST
    BOTH = pkg.STRAND_BOTH
    cap = L.pmx_frameshift_ref_max_query()
    pairs = np.zeros(4, dtype=pkg.PAIR_DTYPE)
    out = np.zeros((4, 4), dtype=np.int32)
    won = np.zeros(4, dtype=np.uint8)

    def adev(c=cfg, q=s, r=t, n=4, p=256, sb=None, mode=BOTH, f=15, mq=8, mr=8, o=256, so=256, opts=None):
        return L.pmx_align_pairs_frameshift_ref_device(C.byref(c), q, r, n, p, sb, mode, f, None, mq, mr, o, so, None,
                                                       C.byref(opts) if opts is not None else None)

    def ahost(c=cfg, q=s, r=t, n=4, p=pairs.ctypes.data, sb=None, mode=BOTH, f=15, o=out.ctypes.data, so=won.ctypes.data, opts=None, **_):
        return L.pmx_align_pairs_frameshift_ref(C.byref(c), q, r, n, p, sb, mode, f, None, o, so, C.byref(opts) if opts is not None else None)

    def sdev(c=cfg, q=s, r=t, shape=RECT, first=0, n=4, p=None, mq=8, mr=8, ms=0, hp=256, hi=256, hr=256, hs=None, cap=16, cnt=256, opts=None,
             mode=BOTH, hb=256, f=15):
        return L.pmx_search_pairs_frameshift_ref_device(C.byref(c), q, r, shape, first, n, p, mq, mr, ms, hp, hi, hr, hs, cap, cnt, None,
                                                        C.byref(opts) if opts is not None else None, mode, hb, f, None)

    def shost(c=cfg, q=s, r=t, shape=RECT, first=0, n=4, p=None, max_hits=0, chunk=0, sl=0, mode=BOTH, f=15, **_):
        res = C.POINTER(pkg.pmx_strand_hits_t)()
        o = pkg.pmx_pair_search_opts_t(0, shape, max_hits, chunk, sl)
        rc = L.pmx_search_pairs_frameshift_ref(C.byref(c), q, r, first, n, p, C.byref(o), mode, f, None, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_passing == 0 and res.contents.strand
            L.pmx_strand_hits_free(res)
        else:
            assert not res
        return rc

    def tdev(c=cfg, q=s, r=t, qf=0, nq=4, mq=8, mr=8, ms=0, k=3, skip=0, hp=256, hi=256, hr=256, hs=None, cap=16, off=256, rp=256, cnt=256, opts=None,
             mode=BOTH, hb=256, f=15):
        return L.pmx_search_topk_frameshift_ref_device(C.byref(c), q, r, qf, nq, mq, mr, ms, k, skip, hp, hi, hr, hs, cap, off, rp, cnt, None,
                                                       C.byref(opts) if opts is not None else None, mode, hb, f, None)

    def thost(c=cfg, q=s, r=t, qf=0, nq=4, k=3, skip=0, chunk=0, sl=0, mode=BOTH, f=15, **_):
        res = C.POINTER(pkg.pmx_topk_strand_hits_t)()
        o = pkg.pmx_topk_opts_t(0, k, skip, chunk, sl)
        rc = L.pmx_search_topk_frameshift_ref(C.byref(c), q, r, qf, nq, C.byref(o), mode, f, None, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_rows == 0 and res.contents.strand
            L.pmx_topk_strand_hits_free(res)
        else:
            assert not res
        return rc

    # the Limits of the contract, at every entry
    for entry in (adev, ahost, sdev, shost, tdev, thost):
        for mode in (pkg.MODE_NW, pkg.MODE_SG):
            assert entry(c=_cfg(pkg, pm, mode=mode)) == -1 and "PMX_MODE_SW" in _err(pkg)
        for width in (8, 16, 64):
            assert entry(c=_cfg(pkg, pm, width=width)) == -1 and "width %d is neither 0 nor 32" % width in _err(pkg)
        assert entry(c=_cfg(pkg, pm, width=3)) == -1 and "bad width" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, want=pkg.WANT_STATS)) == -1 and "PMX_WANT_STATS" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, want=pkg.WANT_CIGAR)) == -1 and "PMX_WANT_CIGAR" in _err(pkg) and "reference-side" in _err(pkg)
        assert entry(c=_cfg(pkg, pssm)) == -1 and "PSSM" in _err(pkg) and "reference-side" in _err(pkg)
        assert entry(c=_cfg(pkg, wide)) == -1 and "129 symbols exceed 128" in _err(pkg)
        assert entry(f=-1) == -1 and "frameshift penalty" in _err(pkg)
        for mode in (-1, 3, 255):
            assert entry(mode=mode) == -1 and "strand mode %d is outside 0 .. 2" % mode in _err(pkg)
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(7, 0, 11, 1, 0, 0, pm.inner)) == -1 and "mode" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(pkg.MODE_SW, 0, -1, 1, 0, 0, pm.inner)) == -1 and "gap penalties" in _err(pkg)
    for entry in (adev, sdev, tdev):                                           # max_qlen bounds the protein, max_rlen has no cap
        assert entry(mq=cap + 1) == -1 and "PMX_FRAMESHIFT_REF_MAX_QUERY" in _err(pkg)
        assert entry(mq=0) == -1 and "max_qlen" in _err(pkg)
        assert entry(mr=0) == -1 and "max_rlen" in _err(pkg)
        assert entry(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
    # listed pairs
    for entry in (adev, ahost):
        assert entry(sb=256 if entry is adev else won.ctypes.data, mode=BOTH) == -1 and "strand byte per pair takes strand mode PMX_STRAND_FORWARD" in _err(pkg)
        assert entry(so=None) == -1 and "null strand output" in _err(pkg)
        assert entry(so=None, mode=1, n=0) == 0                                # (optional with one strand)
        assert entry(n=-1) == -1 and "negative n" in _err(pkg)
        assert entry(p=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(o=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(n=0, so=None) == 0
    bad = np.array([0, 1, 2, 1], dtype=np.uint8)
    assert ahost(sb=bad.ctypes.data, mode=0) == -1 and "pair 2: strand byte 2 is neither 0 nor 1" in _err(pkg)
    # the gather hook
    def gdev(q=s, r=t, n=4, p=256, mq=8, mr=8, qo=256, qc=64, qf=256, ro=256, rc=64, rf=256):
        return L.pmx_gather_pairs_codons_ref_device(q, r, n, p, None, None, mq, mr, qo, qc, qf, ro, rc, rf, None, None)
    assert gdev(q=None) == -1 and "null sequence set" in _err(pkg)
    assert gdev(n=-1) == -1 and "negative n or capacity" in _err(pkg)
    assert gdev(qf=None) == -1 and "null buffer" in _err(pkg)
    assert gdev(mr=0) == -1 and "max_rlen" in _err(pkg)
    assert gdev(n=0, p=None, qo=None, ro=None) == 0
    # set search and top-K: what the stranded entries refuse, with their texts
    for entry in (sdev, shost):
        assert entry(shape=3) == -1 and "unknown pair shape 3" in _err(pkg)
        assert entry(shape=TRI, r=t) == -1 and "R must be NULL or Q" in _err(pkg)
        assert entry(shape=LIST, r=t, p=None) == -1 and "null pairs" in _err(pkg)
        assert entry(shape=RECT, r=t, first=67, n=4) == -1 and "beyond the 70 pairs of 10 x 7" in _err(pkg)
        assert entry(n=0, **({"cnt": None} if entry is sdev else {})) == 0
    assert sdev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    assert sdev(hr=None) == -1 and "null hit records" in _err(pkg)
    assert sdev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert sdev(hs=256) == -1 and "stats buffer without PMX_WANT_STATS" in _err(pkg)
    assert shost(max_hits=-1) == -1 and "max_hits" in _err(pkg)
    for entry in (sdev, tdev):                                                 # both strands, room for hits, nowhere to say which strand
        assert entry(hb=None) == -1 and "null strand output" in _err(pkg)
    for entry in (tdev, thost):
        assert entry(k=0) == -1 and "k 0 is outside 1 .. 1024" in _err(pkg)
        assert entry(skip=1) == -1 and "skip_self needs R to be Q" in _err(pkg)
        assert entry(qf=8, nq=3) == -1 and "beyond the 10 sequences" in _err(pkg)
        assert entry(nq=0, **({"cnt": None, "off": None} if entry is tdev else {})) == 0
    assert tdev(off=None) == -1 and "null row offsets" in _err(pkg)
    assert thost(sl=-1) == -1 and "slice_rows" in _err(pkg)


def test_python_keywords(pkg):
    pm = pkg.Matrix.from_name("blosum62")
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    for strand in (None, 0, 1, "both"):
        h = al.search_pairs(S, S, min_score=5, count=0, ref_frameshift=15, ref_strand=strand)
        assert isinstance(h, pkg.PairHits) and len(h) == 0 and h.strand.dtype == np.uint8
        t = al.search_topk(S, S, k=2, rows=0, ref_frameshift=15, ref_strand=strand)
        assert isinstance(t, pkg.TopKHits) and len(t) == 0
    rec, won = al.align_pairs(S, S, [], ref_frameshift=15, ref_strand="both")
    assert len(rec) == 0 and won.dtype == np.uint8
    for kw, text in (({"frame": 0}, "ref_frameshift excludes frame and ref_frame"), ({"ref_frame": "all"}, "ref_frameshift excludes frame and ref_frame"),
                     ({"frameshift": 15}, "ref_frameshift and frameshift exclude each other"),
                     ({"strand": "both"}, "ref_frameshift and strand exclude each other")):
        for call in (lambda: al.align_pairs(S, S, [], ref_frameshift=15, **kw), lambda: al.search_pairs(S, S, ref_frameshift=15, **kw),
                     lambda: al.search_topk(S, S, ref_frameshift=15, **kw)):
            with pytest.raises(pkg.BatchError, match=text):
                call()
    with pytest.raises(pkg.BatchError, match="ref_frameshift and strand exclude each other"):
        al.align_pairs(S, S, [], ref_frameshift=15, strand=[])
    with pytest.raises(pkg.BatchError, match="ref_frameshift excludes cigar"):
        al.align_pairs(S, S, [], ref_frameshift=15, cigar=True)
    for call in (lambda: al.align_pairs(S, S, [], ref_strand=1), lambda: al.search_pairs(S, S, ref_strand="both"), lambda: al.search_topk(S, S, ref_strand=0)):
        with pytest.raises(pkg.BatchError, match="ref_strand belongs to ref_frameshift"):
            call()
    with pytest.raises(pkg.BatchError, match="frameshift penalty"):
        al.search_pairs(S, S, ref_frameshift=-2)
    with pytest.raises(pkg.BatchError, match="differ in count"):
        al.align_pairs(S, S, [(0, 1)], ref_frameshift=3, ref_strand=[0, 1])
