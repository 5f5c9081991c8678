"""Banded traceback without a GPU: the one bound of the trace scratch (pmx_bandtr_geometry, the C ABI test hook of
parasail-rs_amd/csrc/pmx_banded.hip) against a brute-force count of every admitted pair's band, and the refusals of the two new
entries (pmx_align_batch_banded_cigar / _device), which return -1 with a message before any GPU work."""
import ctypes as C

import numpy as np
import pytest

LENGTHS = (1, 2, 3, 5, 17, 64, 100, 127, 300)
BANDS = (0, 1, 2, 7, 15, 16, 31, 32, 48, 63)


def _geometry(lib, max_qlen, max_rlen, band, q_shared):
    lib.pmx_bandtr_geometry.restype = C.c_int
    lp, rows, stride = C.c_int(0), C.c_int(0), C.c_longlong(0)
    ok = lib.pmx_bandtr_geometry(max_qlen, max_rlen, band, q_shared, C.byref(lp), C.byref(rows), C.byref(stride))
    assert ok == 1, (max_qlen, max_rlen, band, q_shared)
    return lp.value, rows.value, stride.value


def _band_steps(ql, rl, band, d0s):
    """brute force over the cells of the band, row by row, for every centre in d0s: (s_first, s_last), s_last = -1 if no cell"""
    i = np.arange(ql)[None, :]
    d = np.asarray(d0s)[:, None]
    jlo = np.maximum(0, i + d - band)
    jhi = np.minimum(rl - 1, i + d + band)
    has = jlo <= jhi
    big = 1 << 30
    s_first = np.where(has, i + jlo, big).min(axis=1)
    s_last = np.where(has, i + jhi, -1).max(axis=1)
    return s_first, s_last


def _pair_rows(ql, rl, band):
    """every centre from "the band misses the matrix" through both corners: (step pairs of the layout, true steps) per centre"""
    d0s = np.arange(-(ql - 1) - band - 3, rl - 1 + band + 4)
    s_first, s_last = _band_steps(ql, rl, band, d0s)
    hit = s_last >= 0
    s0 = s_first - ((s_first + band - d0s) & 1)                 # the layout's even origin
    rows = np.where(hit, (s_last - s0) // 2 + 1, 0)
    steps = np.where(hit, s_last - s_first + 1, 0)
    return rows, steps, hit


@pytest.mark.parametrize("q_shared", [0, 1])
def test_bandtr_geometry_bounds_every_pair(pkg, q_shared):
    """No admitted pair (queries <= max_qlen, or exactly max_qlen for one shared query; references <= max_rlen; any centre) needs
    more step pairs than the bound, and the bound exceeds the longest true step count by at most the one step pair of padding."""
    lib = pkg.lib
    checked = 0
    for band in BANDS:
        lp_want = 16 if band <= 15 else 32 if band <= 31 else 64
        for Q in LENGTHS:
            for R in LENGTHS:
                lp, rows, stride = _geometry(lib, Q, R, band, q_shared)
                assert lp == lp_want and stride == rows * lp, (Q, R, band, lp, rows, stride)
                most_steps = 0
                for ql in ([Q] if q_shared else [x for x in LENGTHS if x <= Q]):
                    for rl in [x for x in LENGTHS if x <= R]:
                        pr, steps, hit = _pair_rows(ql, rl, band)
                        over = np.nonzero(pr > rows)[0]
                        assert len(over) == 0, (Q, R, band, ql, rl, pr.max(), rows)
                        most_steps = max(most_steps, int(steps.max()))
                        checked += len(pr)
                # the bound is reached by the longest pair (the sweep runs that many steps): 2 rows <= steps + 2
                assert 2 * rows <= most_steps + 2, (Q, R, band, rows, most_steps)
                assert 2 * rows >= most_steps, (Q, R, band, rows, most_steps)
    assert checked > 100000


def test_bandtr_geometry_every_length(pkg):
    """lengths 1-300 on both sides at every band edge width: the bound holds for the pair of the maximal lengths at every centre"""
    lib = pkg.lib
    rng = np.random.default_rng(9100)
    for band in (0, 1, 15, 16, 31, 32, 63):
        for ql in range(1, 301, 7):
            for rl in sorted(set([1, 2, ql, max(1, ql - 2 * band), ql + 2 * band, int(rng.integers(1, 301))])):
                if rl > 300 + 2 * band:
                    continue
                lp, rows, stride = _geometry(lib, ql, rl, band, 0)
                pr, steps, _ = _pair_rows(ql, rl, band)
                assert pr.max() <= rows and 2 * rows <= steps.max() + 2, (ql, rl, band, pr.max(), steps.max(), rows)


def test_bandtr_geometry_rejects_out_of_range(pkg):
    lib = pkg.lib
    lib.pmx_bandtr_geometry.restype = C.c_int
    lp, rows, stride = C.c_int(0), C.c_int(0), C.c_longlong(0)
    for args in ((0, 5, 3), (5, 0, 3), (5, 5, -1), (5, 5, 64)):
        assert lib.pmx_bandtr_geometry(*args, 0, C.byref(lp), C.byref(rows), C.byref(stride)) == 0, args


def _call_host(pkg, cfg, band, profile=None, null_ref=False, n=2):
    qbuf, qoff = pkg.pack([b"ACGT", b"ACGTA"][:n])
    rbuf, roff = pkg.pack([b"ACGT", b"ACCT"][:n])
    out = np.zeros(n, dtype=pkg.RECORD_DTYPE)
    st = np.zeros(n, dtype=pkg.STATS_DTYPE)
    coff = np.zeros(n + 1, dtype=np.int64)
    cbuf = C.c_void_p()
    return pkg.lib.pmx_align_batch_banded_cigar(C.byref(cfg), profile, n, qbuf.ctypes.data, qoff.ctypes.data,
                                                None if null_ref else rbuf.ctypes.data, roff.ctypes.data, band, None,
                                                out.ctypes.data, st.ctypes.data, C.byref(cbuf), coff.ctypes.data)


def _call_device(pkg, cfg, band):
    # (host addresses stand in for device pointers: a refused call must not touch them)
    dummy = np.zeros(64, dtype=np.int64)
    p = dummy.ctypes.data
    return pkg.lib.pmx_align_batch_banded_cigar_device(C.byref(cfg), None, 2, p, p, p, p, 8, 8, band, None, p, p, p, 64, p, None)


def test_banded_cigar_refusals(pkg):
    """band 64, a 33-letter matrix, PSSM, want == 0, null buffers: -1 and a message, no kernel launched"""
    lib = pkg.lib
    before = lib.pmx_last_kernel()
    dna = pkg.Matrix.create(b"ACGT", 2, -3)
    big = pkg.Matrix.create(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456", 2, -3)                 # 33 letters + the wildcard
    pssm = pkg.Matrix.from_name("blosum62").to_pssm(b"ACGT")
    want = pkg.WANT_CIGAR | pkg.WANT_STATS
    cases = [
        ("band 64", pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 32, want, dna.inner), 64, b"bands 0 .. 63"),
        ("negative band", pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 32, want, dna.inner), -1, b"bands 0 .. 63"),
        ("33 letters", pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 32, want, big.inner), 8, b"alphabets"),
        ("PSSM", pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 32, want, pssm.inner), 8, b"PSSM"),
        ("want 0", pkg.pmx_config_t(pkg.MODE_SG, pkg.SG_ALL, 5, 2, 32, 0, dna.inner), 8, b"PMX_WANT_CIGAR"),
        ("want sorted only", pkg.pmx_config_t(pkg.MODE_SG, pkg.SG_ALL, 5, 2, 32, pkg.WANT_SORTED, dna.inner), 8, b"PMX_WANT_CIGAR"),
        ("unknown want bit", pkg.pmx_config_t(pkg.MODE_SG, pkg.SG_ALL, 5, 2, 32, pkg.WANT_CIGAR | 64, dna.inner), 8, b"want"),
        ("bad mode", pkg.pmx_config_t(7, 0, 5, 2, 32, want, dna.inner), 8, b"bad mode"),
    ]
    for what, cfg, band, msg in cases:
        assert _call_host(pkg, cfg, band) == -1, what
        assert msg in lib.pmx_last_error(), (what, lib.pmx_last_error())
        assert _call_device(pkg, cfg, band) == -1, what
        assert msg in lib.pmx_last_error(), (what, lib.pmx_last_error())
    cfg = pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 32, want, dna.inner)
    assert _call_host(pkg, cfg, 8, null_ref=True) == -1 and b"null buffer" in lib.pmx_last_error()
    # the requested outputs need their buffers
    qbuf, qoff = pkg.pack([b"ACGT"])
    out = np.zeros(1, dtype=pkg.RECORD_DTYPE)
    cbuf = C.c_void_p()
    coff = np.zeros(2, dtype=np.int64)
    rc = lib.pmx_align_batch_banded_cigar(C.byref(cfg), None, 1, qbuf.ctypes.data, qoff.ctypes.data, qbuf.ctypes.data,
                                          qoff.ctypes.data, 8, None, out.ctypes.data, None, C.byref(cbuf), coff.ctypes.data)
    assert rc == -1 and b"stats" in lib.pmx_last_error()
    cfg.want = pkg.WANT_CIGAR
    rc = lib.pmx_align_batch_banded_cigar(C.byref(cfg), None, 1, qbuf.ctypes.data, qoff.ctypes.data, qbuf.ctypes.data,
                                          qoff.ctypes.data, 8, None, out.ctypes.data, None, None, None)
    assert rc == -1 and b"null cigar output" in lib.pmx_last_error()
    # a refused call launched nothing
    assert lib.pmx_last_kernel() == before
    # the Python mirror raises with the message
    al = pkg.Aligner.new().matrix(dna).gap_open(5).gap_extend(2).build()
    with pytest.raises(pkg.BatchError, match="bands 0 .. 63"):
        al.align_batch_banded_cigar([b"ACGT"], [b"ACGT"], 64)
