"""CPU tier of the windowed reference-side frameshift traceback entries (pmx_align_pairs_frameshift_ref_cigar_long[_device]): symbols,
the refusals shared with pmx_align_pairs_frameshift_ref_cigar[_device] with their pmx_last_error() texts -- on wrapped sets whose
pointers are never followed, every case ends before any GPU work --, the one refusal that is NOT shared (the bound on four slots of the
un-narrowed shape), the window bound's hook on hand-computed inputs, and the Python mirror."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_align_pairs_frameshift_ref_cigar_long_device", "pmx_align_pairs_frameshift_ref_cigar_long", "pmx_swfsc_window_cols",
           "pmx_frameshift_ref_cigar_long_parts")
ALL = (1 << 63) - 1


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_symbols(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    assert hasattr(pkg, "align_pairs_frameshift_ref_cigar_long_device") and hasattr(pkg.Aligner, "align_pairs_frameshift_ref_cigar_long")
    assert "Windowed frameshift traceback, reference side" in text and "BYTE-IDENTICAL" in text
    assert "SYNCHRONISES THE CALLER'S STREAM ONCE PER CHUNK" in text
    assert pkg.lib.pmx_frameshift_ref_cigar_long_parts() >= 0           # the parts of the thread's last call; 0 before any


def test_window_bound_by_hand(pkg):
    """W = 3 rows + 3 floor(slack / gmin) + min(rows - 1, floor(slack / fs)), slack = P - S, gmin = min(open, extend)"""
    W = pkg.lib.pmx_swfsc_window_cols
    # (P, S, rows, open, extend, fs) -> W
    assert W(100, 80, 10, 11, 1, 15) == 30 + 3 * 20 + 1                 # slack 20: twenty codon gaps at most, one frameshift
    assert W(100, 80, 10, 11, 1, 0) == 30 + 3 * 20 + 9                  # fs = 0: every match column but the first may shift
    assert W(50, 50, 4, 3, 3, 7) == 12                                  # no slack: the path is rows codons at most
    assert W(200, 100, 20, 2, 5, 4) == 60 + 3 * 50 + 19                 # extend above open: gmin is open; 25 shifts would fit, 19 rows allow
    assert W(200, 100, 20, 5, 2, 40) == 60 + 3 * 50 + 2
    assert W(4, 0, 1, 11, 1, 15) == 3 + 3 * 4                           # a zero-score record: one row
    assert W(1000, 10, 7, 1 << 30, 1 << 30, 1 << 30) == 21              # penalties above 2^28 are read as 2^28, as the kernel reads them
    assert W(100, 99, 10, 11, 2, 1) == 30 + 0 + 1
    for open_, ext in ((4, 0), (0, 4), (0, 0)):
        assert W(100, 80, 10, open_, ext, 15) == ALL                    # a free gap bounds nothing
    # the column shift the kernel derives from it: a = max(0, end_ref + 1 - W)
    assert max(0, 5000 + 1 - W(100, 80, 10, 11, 1, 15)) == 4910 and max(0, 60 + 1 - W(100, 80, 10, 11, 1, 15)) == 0


def _cfg(pkg, pm, mode=None, width=0, want=None):
    return pkg.pmx_config_t(pkg.MODE_SW if mode is None else mode, 0, 11, 1, width, pkg.WANT_CIGAR if want is None else want, pm.inner)


def test_refusals_without_gpu(pkg, monkeypatch):
    """wrapped sets over addresses that are never followed: every case ends before any GPU work"""
    L = pkg.lib
    pm = pkg.Matrix.from_name("blosum62")
    pssm = pkg.Matrix.create_pssm(b"ACGT", [1, -1, -1, -1] * 8, 8)
    cfg = _cfg(pkg, pm)
    S = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    T = pkg.SeqSet.wrap_device(256, 256, 7, 700)
    s, t = S.inner, T.inner
    O = pkg.pmx_pairs_opts_t
    BOTH = pkg.STRAND_BOTH
    cap = L.pmx_frameshift_ref_max_query()
    pairs = np.zeros(4, dtype=pkg.PAIR_DTYPE)
    out = np.zeros((4, 4), dtype=np.int32)
    won = np.zeros(4, dtype=np.uint8)
    st = np.zeros((4, 3), dtype=np.int32)
    beg = np.zeros((4, 2), dtype=np.int32)
    off = np.zeros(5, dtype=np.int64)
    buf = C.c_void_p()

    def dev(fn):
        def call(c=cfg, q=s, r=t, n=4, p=256, sb=None, mode=BOTH, f=15, mq=8, mr=8, o=256, so=256, ds=None, db=256, tx=256, tc=64, to=256, opts=None):
            return fn(C.byref(c), q, r, n, p, sb, mode, f, None, mq, mr, o, so, ds, db, tx, tc, to, None, C.byref(opts) if opts is not None else None)
        return call

    adev, old = dev(L.pmx_align_pairs_frameshift_ref_cigar_long_device), dev(L.pmx_align_pairs_frameshift_ref_cigar_device)

    def ahost(c=cfg, q=s, r=t, n=4, p=pairs.ctypes.data, sb=None, mode=BOTH, f=15, o=out.ctypes.data, so=won.ctypes.data, ds=None,
              db=beg.ctypes.data, tx=C.byref(buf), to=off.ctypes.data, opts=None, **_):
        if ds == 256:
            ds = st.ctypes.data
        return L.pmx_align_pairs_frameshift_ref_cigar_long(C.byref(c), q, r, n, p, sb, mode, f, None, o, so, ds, db, tx, to,
                                                           C.byref(opts) if opts is not None else None)

    for entry in (adev, ahost):
        # what the score entries of this side refuse, with their texts
        for mode in (pkg.MODE_NW, pkg.MODE_SG):
            assert entry(c=_cfg(pkg, pm, mode=mode)) == -1 and "PMX_MODE_SW" in _err(pkg)
        for width in (8, 16, 64):
            assert entry(c=_cfg(pkg, pm, width=width)) == -1 and "width %d is neither 0 nor 32" % width in _err(pkg)
        assert entry(c=_cfg(pkg, pm, width=3)) == -1 and "bad width" in _err(pkg)
        assert entry(c=_cfg(pkg, pssm)) == -1 and "reference-side frameshift entries take no PSSM matrix" in _err(pkg)
        assert entry(f=-1) == -1 and "frameshift penalty" in _err(pkg)
        for mode in (-1, 3, 255):
            assert entry(mode=mode) == -1 and "strand mode %d is outside 0 .. 2" % mode in _err(pkg)
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(r=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(7, 0, 11, 1, 0, pkg.WANT_CIGAR, pm.inner)) == -1 and "mode" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(pkg.MODE_SW, 0, -1, 1, 0, pkg.WANT_CIGAR, pm.inner)) == -1 and "gap penalties" in _err(pkg)
        assert entry(sb=256 if entry is adev else won.ctypes.data, mode=BOTH) == -1 and "strand byte per pair takes strand mode PMX_STRAND_FORWARD" in _err(pkg)
        assert entry(so=None) == -1 and "null strand output" in _err(pkg)
        assert entry(n=-1) == -1 and "negative n" in _err(pkg)
        assert entry(p=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(o=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
        # what the traceback entries refuse about their outputs
        assert entry(c=_cfg(pkg, pm, want=0)) == -1 and "PMX_WANT_CIGAR" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, want=pkg.WANT_STATS)) == -1 and "PMX_WANT_CIGAR" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, want=pkg.WANT_CIGAR | pkg.WANT_STATS)) == -1 and "stats requested without a stats buffer" in _err(pkg)
        assert entry(ds=256) == -1 and "stats buffer without PMX_WANT_STATS" in _err(pkg)
        assert entry(tx=None) == -1 and "null cigar output" in _err(pkg)
        assert entry(to=None) == -1 and "null cigar output" in _err(pkg)
        assert entry(n=0, so=None, db=None) == 0
        assert entry(n=0, so=None, mode=1, c=_cfg(pkg, pm, want=pkg.WANT_CIGAR | pkg.WANT_STATS), ds=256) == 0
    assert adev(tc=-1) == -1 and "negative cigar_capacity" in _err(pkg)
    assert adev(mq=cap + 1) == -1 and "PMX_FRAMESHIFT_REF_MAX_QUERY" in _err(pkg)
    assert adev(mq=0) == -1 and "max_qlen" in _err(pkg)
    bad = np.array([0, 1, 2, 1], dtype=np.uint8)
    assert ahost(sb=bad.ctypes.data, mode=0) == -1 and "pair 2: strand byte 2 is neither 0 nor 1" in _err(pkg)
    # the one refusal that is not shared: four slots of the UN-NARROWED shape against the bound.  Where the old entry speaks of the
    # bound, the new one goes on to the next check (max_rlen 0 is refused behind it, so nothing reaches the GPU)
    four0 = 4 * L.pmx_swfsc_trace_bytes_per_slot(8, 0)
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(four0 - 1))
    assert old(mr=0) == -1 and "PMX_CIGAR_CHUNK_BYTES" in _err(pkg)
    assert adev(mr=0) == -1 and "max_qlen / max_rlen must be positive" in _err(pkg)
    monkeypatch.delenv("PMX_CIGAR_CHUNK_BYTES")
    assert old(mq=4096, mr=100000) == -1 and "exceed the bound" in _err(pkg)
    assert adev(mq=4096, mr=0) == -1 and "max_qlen / max_rlen must be positive" in _err(pkg)


def test_python_mirror(pkg):
    pm = pkg.Matrix.from_name("blosum62")
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    for strand in (0, 1, "both", "forward", "reverse", None):
        rec, cig, beg, won = al.align_pairs_frameshift_ref_cigar_long(S, S, [], 15, ref_strand=strand)
        assert len(rec) == 0 and cig == [] and beg.shape == (0, 2) and won.dtype == np.uint8
    rec, cig, beg, won, st = al.align_pairs_frameshift_ref_cigar_long(S, S, [], 15, stats=True)
    assert len(st) == 0
    with pytest.raises(pkg.BatchError, match="frameshift penalty"):
        al.align_pairs_frameshift_ref_cigar_long(S, S, [], -1)
    with pytest.raises(pkg.BatchError, match="differ in count"):
        al.align_pairs_frameshift_ref_cigar_long(S, S, [(0, 1)], 3, ref_strand=[0, 1])
    with pytest.raises(TypeError):
        al.align_pairs_frameshift_ref_cigar_long(S, S, [], 3, ref_frame=0)
    prof = pkg.Aligner.new().local().matrix(pm).profile(pkg.Profile.new(b"ACDEF", False, pm)).build()
    with pytest.raises(pkg.BatchError, match="takes no profile"):
        prof.align_pairs_frameshift_ref_cigar_long(S, S, [], 15)
    import inspect
    assert inspect.signature(pkg.Aligner.align_pairs_frameshift_ref_cigar_long) == inspect.signature(pkg.Aligner.align_pairs_frameshift_ref_cigar)
