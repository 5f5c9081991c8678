"""CPU tier of the reference-side translated set entries (pmx_*_translated_ref[_device]): symbols, header, Python wrappers, struct
layouts, every refusal that needs no GPU (wrapped sets whose pointers are never followed) with its pmx_last_error() text, the
ref_frame= keyword's exclusions, and the model (tests/translate_ref_side.py) on hand-written reference windows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_ref
import translate_ref_side as ref
from test_set_search_args import _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_gather_pairs_translated_ref_device", "pmx_align_pairs_translated_ref_device", "pmx_align_pairs_translated_ref",
           "pmx_search_pairs_translated_ref_device", "pmx_search_pairs_translated_ref",
           "pmx_search_topk_translated_ref_device", "pmx_search_topk_translated_ref")


def _header():
    return open(os.path.join(ROOT, "include", "parasail_amd.h")).read()


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_symbols_wrappers_and_layouts(pkg):
    text = _header()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name in ("gather_pairs_translated_ref_device", "align_pairs_translated_ref_device", "search_pairs_translated_ref_device",
                 "search_topk_translated_ref_device"):
        assert callable(getattr(pkg, name)), name
    import inspect
    for method in (pkg.Aligner.align_pairs, pkg.Aligner.search_pairs, pkg.Aligner.search_topk):
        p = inspect.signature(method).parameters
        assert p["ref_frame"].default is None and p["frame"].default is None and "code" in p
    # no entry takes two frame arguments, and the frame modes are the existing ones
    for name in SYMBOLS:
        decl = re.search(r"\b%s\(([^;]*?)\);" % name, text, re.S).group(1)
        assert len(re.findall(r"\bint frame_mode\b", decl)) == (0 if "gather" in name else 1), name
    for name, value in (("FORWARD", 6), ("REVERSE", 7), ("ALL", 8)):
        assert len(re.findall(r"#define PMX_FRAMES_%s\s+%d\b" % (name, value), text)) == 1
    # the result blocks are reused, the option and result struct layouts are what they were
    assert len(re.findall(r"typedef struct pmx_frame_hits\b", text)) == 1 and len(re.findall(r"typedef struct pmx_topk_frame_hits\b", text)) == 1
    for struct, ctype, size in (("pmx_frame_hits", pkg.pmx_frame_hits_t, 56), ("pmx_topk_frame_hits", pkg.pmx_topk_frame_hits_t, 80),
                                ("pmx_pair_hits", pkg.pmx_pair_hits_t, 48), ("pmx_topk_hits", pkg.pmx_topk_hits_t, 72)):
        fields, hsize = _layout(text, struct, struct + "_t")
        assert hsize == size == C.sizeof(ctype), struct
        for name, o, sz in fields:
            assert getattr(ctype, name).offset == o and getattr(ctype, name).size == sz, name
    assert _layout(text, "pmx_pairs_opts", "pmx_pairs_opts_t")[1] == 8 == C.sizeof(pkg.pmx_pairs_opts_t)
    assert _layout(text, "pmx_pair_search_opts", "pmx_pair_search_opts_t")[1] == 32 == C.sizeof(pkg.pmx_pair_search_opts_t)
    assert _layout(text, "pmx_topk_opts", "pmx_topk_opts_t")[1] == 32 == C.sizeof(pkg.pmx_topk_opts_t)


# ------------------------------------------------------------------------------------------------------------ the model, by hand
TEN = b"ATGGCCTAAN"          # reverse complement: NTTAGGCCAT
PROTS = [b"MKV", b"W", b"ACDEFGHIK"]
NUCS = [TEN, b"AT", b"ATG", b"ATGG", b"ATGGC", b"ccATGGCCTAANgg", b"A"]


def _one(row, f, mq=pairs_ref.INT32_MAX, mr=pairs_ref.INT32_MAX):
    return ref.resolve(PROTS, NUCS, pairs_ref.pairs_array([row]), [f], mq, mr)[0]


def test_model_on_hand_written_reference_windows():
    # both strands, a stop, an N: the whole ten-letter reference in every frame; the query is a plain copy
    for f, want in enumerate((b"MA*", b"WPX", b"GL", b"XRP", b"LGH", b"*A")):
        assert _one((0, 0), f) == (b"MKV", want)
        assert _one((2, 5, 2, 4, 2, 10), f) == (b"DEFG", want)                              # the same ten letters as a window, a query window beside
        assert _one((2, 5, 2, 4, 2, 10), f)[1] == ref.translate(NUCS[5][2:12], f)
    # W < 3: no frame;  W = 3: frames 0 and 3;  W = 4: 0 1 3 4;  W = 5: all six
    exist = {1: [], 2: [0, 3], 3: [0, 1, 3, 4], 4: [0, 1, 2, 3, 4, 5], 6: []}
    for j, frames in exist.items():
        for f in range(6):
            got = _one((1, j), f)
            assert (got is not None) == (f in frames), (j, f)
            if got is not None:
                assert got == (b"W", ref.translate(NUCS[j], f)) and len(got[1]) == ref.tlen(len(NUCS[j]), f) == 1
    assert [_one((1, 4), f)[1] for f in range(6)] == [b"M", b"W", b"G", b"A", b"P", b"H"]
    assert [_one((1, 3), f) and _one((1, 3), f)[1] for f in range(6)] == [b"M", b"W", None, b"P", b"H", None]
    # every W mod 3 through a window of the ten letters, from both ends
    for w in range(3, 11):
        for f in range(6):
            for beg, win in ((10 - w, TEN[10 - w:]), (0, TEN[:w])):
                got = _one((0, 0, 0, -1, beg, -1 if beg and w % 2 else w), f)
                if (w - f % 3) // 3 == 0:
                    assert got is None and ref.translate(win, f) == b""
                else:
                    assert got[1] == ref.translate(win, f) and len(got[1]) == (w - f % 3) // 3
    # max_rlen bounds the letters, not the nucleotides; max_qlen bounds the query window as it stands
    assert _one((0, 0), 0, mr=3) is not None and _one((0, 0), 0, mr=2) is None and _one((0, 0), 2, mr=2) is not None
    assert _one((2, 0), 0, mq=9) is not None and _one((2, 0), 0, mq=8) is None and _one((2, 0, 1, 8, 0, -1), 0, mq=8) is not None
    # bad descriptors and frame bytes
    for row, f in (((3, 0), 0), ((0, 7), 0), ((0, 0, 0, -1, 8, 3), 0), ((0, 0, 0, -1, -1, -1), 0), ((0, 0), 6), ((0, 0), 255)):
        assert _one(row, f) is None
    # letter p back to stored bytes: stored_bytes with r_beg where the query side has q_beg
    comp = {ord(a): ord(b) for a, b in zip("ACGTNacgtn", "TGCANtgcan")}
    seq = NUCS[5]
    for r_beg, w in ((0, 14), (2, 10), (3, 8)):
        for f in range(6):
            t = ref.translate(seq[r_beg:r_beg + w], f)
            for p in range(len(t)):
                at = ref.stored_bytes(r_beg, w, f, p)
                codon = bytes(seq[x] if f < 3 else comp[seq[x]] for x in at)
                assert ref.translate(codon, 0) == t[p:p + 1] and all(r_beg <= x < r_beg + w for x in at)


def _cfg(pkg, pm, want=0):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, want, pm.inner)


def test_refusals_without_gpu(pkg):
    """wrapped sets over addresses that are never followed: every case ends before any GPU work"""
    L = pkg.lib
    pm = pkg.Matrix.from_name("blosum62")
    pssm = pkg.Matrix.create_pssm(b"ACGT", [1, -1, -1, -1] * 8, 8)
    cfg = _cfg(pkg, pm)
    S = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    T = pkg.SeqSet.wrap_device(256, 256, 7, 700)
    s, t = S.inner, T.inner
    O = pkg.pmx_pairs_opts_t
    TRI, RECT, LIST = pkg.PAIRS_TRIANGLE, pkg.PAIRS_RECT, pkg.PAIRS_LIST
    ALL = pkg.FRAMES_ALL
    pairs = np.zeros(4, dtype=pkg.PAIR_DTYPE)
    out = np.zeros((4, 4), dtype=np.int32)
    won = np.zeros(4, dtype=np.uint8)
    route = ("CIGAR", "pmx_gather_pairs_translated_ref_device", "pmx_align_batch_cigar_device")

    def refuses_cigar(rc):
        return rc == -1 and all(word in _err(pkg) for word in route)

    def refuses_pssm(rc):
        return rc == -1 and "PSSM" in _err(pkg) and "translated reference" in _err(pkg) and "not wired" in _err(pkg)

    # ---- listed pairs
    def adev(c=cfg, q=s, r=t, n=4, p=256, fr=None, mode=ALL, mq=8, mr=8, o=256, st=None, fo=256, opts=None):
        return L.pmx_align_pairs_translated_ref_device(C.byref(c), q, r, n, p, fr, mode, None, mq, mr, o, st, fo, None,
                                                       C.byref(opts) if opts is not None else None)

    def ahost(c=cfg, q=s, r=t, n=4, p=pairs.ctypes.data, fr=None, mode=ALL, o=out.ctypes.data, st=None, fo=won.ctypes.data, opts=None, **_):
        return L.pmx_align_pairs_translated_ref(C.byref(c), q, r, n, p, fr, mode, None, o, st, fo, C.byref(opts) if opts is not None else None)

    for entry in (adev, ahost):
        for mode in (-1, 9, 255):
            assert entry(mode=mode) == -1 and "frame mode %d is outside 0 .. 8" % mode in _err(pkg)
        assert entry(fr=256 if entry is adev else won.ctypes.data, mode=2) == -1 and "frame byte per pair takes frame mode 0" in _err(pkg)
        for mode in (pkg.FRAMES_FORWARD, pkg.FRAMES_REVERSE, ALL):
            assert entry(fo=None, mode=mode) == -1 and "null frame output" in _err(pkg)
        assert entry(fo=None, mode=4, n=0) == 0                                             # (optional in a single-frame mode)
        assert refuses_cigar(entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR)))
        assert refuses_pssm(entry(c=_cfg(pkg, pssm)))
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(r=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(n=-1) == -1 and "negative n" in _err(pkg)
        assert entry(p=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(o=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(7, 0, 11, 1, 0, 0, pm.inner)) == -1 and "mode" in _err(pkg)
        assert entry(n=0, fo=None) == 0                                                     # n == 0 touches nothing
    assert adev(c=_cfg(pkg, pm, pkg.WANT_STATS)) == -1 and "stats requested without a stats buffer" in _err(pkg)
    assert adev(mq=0) == -1 and "max_qlen" in _err(pkg)
    assert adev(mr=0) == -1 and "max_rlen" in _err(pkg)
    bad = np.array([0, 5, 6, 1], dtype=np.uint8)
    assert ahost(fr=bad.ctypes.data, mode=0) == -1 and "pair 2: frame byte 6 is outside 0 .. 5" in _err(pkg)

    # ---- the gather hook
    def gdev(q=s, r=t, n=4, p=256, mq=8, mr=8, qo=256, qc=64, qf=256, ro=256, rc=64, rf=256):
        return L.pmx_gather_pairs_translated_ref_device(q, r, n, p, None, None, mq, mr, qo, qc, qf, ro, rc, rf, None, None)
    assert gdev(r=None) == -1 and "null sequence set" in _err(pkg)
    assert gdev(n=-1) == -1 and "negative n or capacity" in _err(pkg)
    assert gdev(rc=-1) == -1 and "negative n or capacity" in _err(pkg)
    assert gdev(rf=None) == -1 and "null buffer" in _err(pkg)
    assert gdev(p=None) == -1 and "null buffer" in _err(pkg)
    assert gdev(ro=None) == -1 and "null buffer" in _err(pkg)
    assert gdev(mr=0) == -1 and "max_rlen" in _err(pkg)
    assert gdev(n=0, p=None, qo=None, ro=None) == 0

    # ---- set search
    def sdev(c=cfg, q=s, r=t, shape=RECT, first=0, n=4, p=None, mq=8, mr=8, ms=0, hp=256, hi=256, hr=256, hs=None, cap=16, cnt=256, opts=None,
             mode=ALL, hb=256):
        return L.pmx_search_pairs_translated_ref_device(C.byref(c), q, r, shape, first, n, p, mq, mr, ms, hp, hi, hr, hs, cap, cnt, None,
                                                        C.byref(opts) if opts is not None else None, mode, None, hb)

    def shost(c=cfg, q=s, r=t, shape=RECT, first=0, n=4, p=None, max_hits=0, chunk=0, sl=0, mode=ALL, **_):
        res = C.POINTER(pkg.pmx_frame_hits_t)()
        o = pkg.pmx_pair_search_opts_t(0, shape, max_hits, chunk, sl)
        rc = L.pmx_search_pairs_translated_ref(C.byref(c), q, r, first, n, p, C.byref(o), mode, None, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_passing == 0 and res.contents.frame
            L.pmx_frame_hits_free(res)
        else:
            assert not res
        return rc

    for entry in (sdev, shost):
        for mode in (-1, 9):
            assert entry(mode=mode) == -1 and "frame mode %d is outside 0 .. 8" % mode in _err(pkg)
        for mode in (0, 4, pkg.FRAMES_FORWARD, pkg.FRAMES_REVERSE, ALL):
            assert refuses_pssm(entry(c=_cfg(pkg, pssm), mode=mode))
            assert refuses_cigar(entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR), mode=mode))
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
    assert sdev(mr=0) == -1 and "max_rlen" in _err(pkg)
    for mode in (pkg.FRAMES_FORWARD, pkg.FRAMES_REVERSE, ALL):                              # a multi-frame mode without a frame output
        assert sdev(hb=None, mode=mode) == -1 and "null frame output" in _err(pkg)
    assert sdev(hb=None, hp=None, hi=None, n=0, cnt=None, mode=3) == 0                      # (optional in a single-frame mode ...
    assert sdev(hb=None, hr=None, cap=0, n=0, cnt=None) == 0                                # ... and where no hit is written)
    assert shost(max_hits=-1) == -1 and "max_hits" in _err(pkg)
    assert shost(sl=-1) == -1 and "slice_pairs" in _err(pkg)
    o = pkg.pmx_pair_search_opts_t(0, RECT, 0, 0, 0)
    assert L.pmx_search_pairs_translated_ref(C.byref(cfg), s, t, 0, 4, None, C.byref(o), ALL, None, None) == -1 and "null result" in _err(pkg)

    # ---- top-K
    def tdev(c=cfg, q=s, r=t, qf=0, nq=4, mq=8, mr=8, ms=0, k=3, skip=0, hp=256, hi=256, hr=256, hs=None, cap=16, off=256, rp=256, cnt=256, opts=None,
             mode=ALL, hb=256):
        return L.pmx_search_topk_translated_ref_device(C.byref(c), q, r, qf, nq, mq, mr, ms, k, skip, hp, hi, hr, hs, cap, off, rp, cnt, None,
                                                       C.byref(opts) if opts is not None else None, mode, None, hb)

    def thost(c=cfg, q=s, r=t, qf=0, nq=4, k=3, skip=0, chunk=0, sl=0, mode=ALL, **_):
        res = C.POINTER(pkg.pmx_topk_frame_hits_t)()
        o = pkg.pmx_topk_opts_t(0, k, skip, chunk, sl)
        rc = L.pmx_search_topk_translated_ref(C.byref(c), q, r, qf, nq, C.byref(o), mode, None, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_rows == 0 and res.contents.frame
            L.pmx_topk_frame_hits_free(res)
        else:
            assert not res
        return rc

    for entry in (tdev, thost):
        for mode in (-1, 9):
            assert entry(mode=mode) == -1 and "frame mode %d is outside 0 .. 8" % mode in _err(pkg)
        for mode in (3, ALL):
            assert refuses_pssm(entry(c=_cfg(pkg, pssm), mode=mode))
            assert refuses_cigar(entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR), mode=mode))
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
    assert tdev(hb=None) == -1 and "null frame output" in _err(pkg)
    assert tdev(hb=None, mode=1, nq=0, cnt=None, off=None) == 0
    assert thost(sl=-1) == -1 and "slice_rows" in _err(pkg)

    # the query-side entries keep their own texts
    assert L.pmx_align_pairs_translated_device(C.byref(_cfg(pkg, pssm)), s, t, 4, 256, None, ALL, None, 8, 8, 256, None, 256, None, None) == -1
    assert "translated query" in _err(pkg)
    assert L.pmx_align_pairs_translated_device(C.byref(_cfg(pkg, pm, pkg.WANT_CIGAR)), s, t, 4, 256, None, ALL, None, 8, 8, 256, None, 256, None, None) == -1
    assert "pmx_gather_pairs_translated_device" in _err(pkg)


def test_python_mirror_defaults_and_refusals(pkg):
    pm = pkg.Matrix.from_name("blosum62")
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    for frame in (0, 5, "forward", "reverse", "all", pkg.FRAMES_ALL):
        h = al.search_pairs(S, S, min_score=5, count=0, ref_frame=frame)
        assert isinstance(h, pkg.PairHits) and len(h) == 0 and h.frame.dtype == np.uint8 and len(h.frame) == 0
        t = al.search_topk(S, S, k=2, rows=0, ref_frame=frame)
        assert isinstance(t, pkg.TopKHits) and len(t) == 0 and t.frame.dtype == np.uint8 and len(t.frame) == 0
    rec, won = al.align_pairs(S, S, [], ref_frame="all")
    assert len(rec) == 0 and won.dtype == np.uint8 and len(won) == 0
    with pytest.raises(pkg.BatchError, match="frame mode 11"):
        al.search_pairs(S, S, ref_frame=11)
    with pytest.raises(pkg.BatchError, match="frame mode 9"):
        al.search_topk(S, S, ref_frame=9)
    with pytest.raises(pkg.BatchError, match="all"):
        al.search_pairs(S, S, ref_frame="sideways")
    for call in (lambda: al.search_pairs(S, S, ref_frame=0, frame=0), lambda: al.search_topk(S, S, ref_frame="all", frame="all"),
                 lambda: al.align_pairs(S, S, [(0, 1)], ref_frame=2, frame=[0]), lambda: al.align_pairs(S, S, [], ref_frame=0, frame=3)):
        with pytest.raises(pkg.BatchError, match="frame and ref_frame exclude each other"):
            call()
    for call in (lambda: al.search_pairs(S, S, ref_frame=0, strand="both"), lambda: al.search_topk(S, S, ref_frame="all", strand=1),
                 lambda: al.align_pairs(S, S, [(0, 1)], ref_frame=2, strand=[0]), lambda: al.align_pairs(S, S, [(0, 1)], ref_frame="all", strand="both")):
        with pytest.raises(pkg.BatchError, match="ref_frame and strand exclude each other"):
            call()
    with pytest.raises(pkg.BatchError, match="differ in count"):
        al.align_pairs(S, S, [(0, 1)], ref_frame=[0, 1])
    with pytest.raises(pkg.BatchError, match="one frame mode"):
        al.search_pairs(S, S, ref_frame=[0, 1])
    with pytest.raises(pkg.BatchError, match="pmx_gather_pairs_translated_ref_device"):
        al.align_pairs(S, S, [], ref_frame=0, cigar=True)
    pssm_al = pkg.Aligner.new().local().matrix(pkg.Matrix.create_pssm(b"ACGT", [1, -1, -1, -1] * 8, 8)).gap_open(11).gap_extend(1).build()
    with pytest.raises(pkg.BatchError, match="translated reference takes no PSSM"):
        pssm_al.search_pairs(S, S, ref_frame="all", count=0)
    h = al.search_pairs(S, S, min_score=5, count=0)                                      # ref_frame=None: today's path, no frames
    assert len(h.frame) == 0 and len(h.strand) == 0
