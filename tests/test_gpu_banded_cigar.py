"""Banded traceback (`-m gpu`): pmx_align_batch_banded_cigar / _device -- the trace form of the 32-bit anti-diagonal banded kernels
(pmx_banded.hip) and its walk (pmx_walkb.hip) -- against the banded oracle: records equal pmx_align_batch_banded's and the oracle's,
CIGAR text equals the oracle's banded walk byte for byte, statistics equal the oracle's, and every path re-scores to the record's
score inside the band."""
import ctypes as C

import numpy as np
import pytest

import workloads as wl
from util import random_seqs, mutate, AA, golden, cigar_ops

pytestmark = pytest.mark.gpu

BANDS = (0, 1, 7, 15, 16, 31, 32, 48, 63)
NEG = -(1 << 30)


def _oracle(orc, mode, flags, q, r, open_, ext, om, band, diag):
    """orc_align_ex with the band and a trace table, then the oracle's walk: (score, end_query, end_ref, cigar, m, s, l)"""
    lib = orc.lib()
    qa, ra = np.frombuffer(q, dtype=np.uint8), np.frombuffer(r, dtype=np.uint8)
    res, out = orc._Result(), orc._Outputs()
    trace = np.zeros((len(q), len(r)), dtype=np.int8)
    out.trace_table = trace.ctypes.data
    rc = lib.orc_align_ex(mode, flags, orc._ptr(qa), len(q), orc._ptr(ra), len(r), int(open_), int(ext), orc._ptr(om.scores), om.size,
                          orc._ptr(om.mapper), 32, 1, int(band), int(diag), C.byref(res), C.byref(out))
    assert rc == 0
    if res.score == NEG:
        return res.score, res.end_query, res.end_ref, "", 0, 0, 0
    o = orc.Result()
    o.mode, o.trace_table, o.query, o.ref, o.matrix, o.end_query, o.end_ref = mode, trace, q, r, om, res.end_query, res.end_ref
    return res.score, res.end_query, res.end_ref, orc.cigar(o), res.matches, res.similar, res.length


def _in_band_and_rescore(orc, cig, rec, qs, rs, band, diag, open_, ext, om, free_mask):
    """every aligned cell of each path lies inside the band; the text re-scores to the record's score"""
    n = len(cig)
    text = np.frombuffer("".join(cig).encode() or b"\0", dtype=np.uint8)
    toff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cig], out=toff[1:])
    beg = np.zeros((n, 2), dtype=np.int32)
    for k, c in enumerate(cig):
        if not c:
            continue
        ops = cigar_ops(c)
        cq = sum(l for l, op in ops if op in "=XI")
        cr = sum(l for l, op in ops if op in "=XD")
        bq, br = (rec["end_query"][k] + 1 - cq, rec["end_ref"][k] + 1 - cr) if free_mask is None else (0, 0)
        if free_mask is None:
            beg[k] = (bq, br)
        # band test: walk the runs; a cell is aligned where it is entered by a = / X / I / D move inside the matrix
        i, j, d0 = bq, br, 0 if diag is None else int(diag[k])
        for l, op in ops:
            di, dj = (1, 1) if op in "=X" else (1, 0) if op == "I" else (0, 1)
            i1, j1 = i + di * l, j + dj * l
            lo_i, lo_j = i + di - 1, j + dj - 1                       # first cell of the run, 0-based
            for (ci, cj) in ((lo_i, lo_j), (i1 - 1, j1 - 1)):
                # (cells of row / column -1 are boundary gaps; cells beyond the end cell are a semi-global unaligned tail)
                if 0 <= ci <= rec["end_query"][k] and 0 <= cj <= rec["end_ref"][k]:
                    assert abs((cj - ci) - d0) <= band, (k, c, ci, cj, d0, band)
            i, j = i1, j1
    qb, qo = orc.pack(qs)
    rb, ro = orc.pack(rs)
    got, bad = orc.rescore_cigars(text, toff, qb, qo, rb, ro, open_, ext, om, beg=beg.reshape(-1),
                                  free_mask=0 if free_mask is None else free_mask)
    assert bad == 0
    has = np.array([bool(c) for c in cig])
    if open_ >= ext:                                               # (open < extend: a run may be two gaps, the text cannot tell)
        assert (got[has, 0] == rec["score"][has]).all(), np.nonzero(got[has, 0] != rec["score"][has])
    assert (got[has, 3] == 0).all()                                # = / X labelled by the alphabet


def _check(pkg, orc, al, mode, flags, qs, rs, band, diag, open_, ext, om, kernel=None, profile_query=None, oracle_idx=None):
    rec, cig, st = al.align_batch_banded_cigar(qs, rs, band, diag, stats=True)
    name = pkg.lib.pmx_last_kernel().decode()
    assert name.endswith(" + pmx_walkb_kernel") and name.split(" + ")[0] in ("pmx_banded_staged_kernel/trace", "pmx_banded_kernel/trace"), name
    if kernel:
        assert name == kernel + " + pmx_walkb_kernel", name
    ref = al.align_batch_banded(qs, rs, band, diag)
    assert (rec == ref).all(), np.nonzero(rec != ref)
    rec2, cig2 = al.align_batch_banded_cigar(qs, rs, band, diag)
    assert (rec2 == rec).all() and cig2 == cig
    idx = range(len(rs)) if oracle_idx is None else oracle_idx
    for k in idx:
        q = profile_query if profile_query is not None else qs[k]
        want = _oracle(orc, mode, flags, q, rs[k], open_, ext, om, band, 0 if diag is None else diag[k])
        got = (int(rec["score"][k]), int(rec["end_query"][k]), int(rec["end_ref"][k]), cig[k],
               int(st["matches"][k]), int(st["similar"][k]), int(st["length"][k]))
        if want[0] == NEG:
            assert got[0] == NEG and got[3] == "" and got[4:] == (0, 0, 0), (k, got)
        else:
            assert got == want, (mode, flags, band, k, len(q), len(rs[k]), None if diag is None else diag[k], got, want)
    fm = None if mode == orc.SW else (flags if mode == orc.SG else 0)
    _in_band_and_rescore(orc, cig, rec, [profile_query] * len(rs) if profile_query is not None else qs, rs, band, diag, open_, ext, om, fm)
    return rec, cig, st


def _pairs(rng, n, lo, hi, band, alphabet=None):
    kw = {} if alphabet is None else {"alphabet": alphabet}
    qs = random_seqs(rng, n, lo, hi, **kw)
    rs, diag = [], np.zeros(n, dtype=np.int32)
    for t, q in enumerate(qs):
        pre = random_seqs(rng, 1, 0, 30, **kw)[0] if t % 3 == 1 else b""
        body = mutate(rng, q, 0.08, 0.04, **kw) if t % 7 else random_seqs(rng, 1, 1, hi, **kw)[0]
        rs.append(pre + body + (random_seqs(rng, 1, 0, 20, **kw)[0] if t % 4 == 0 else b""))
        diag[t] = len(pre) + int(rng.integers(-3, 4))
        if t % 11 == 5:                                      # a centre whose band misses the end cell, or the matrix
            diag[t] = int(rng.choice([len(rs[-1]) + band + 5, -len(q) - band - 5, len(rs[-1]) - len(q) + 2 * band + 3]))
    return qs, rs, diag


def _aligner(pkg, mode, flags, pm, open_, ext):
    """global / semi-global (every end free) / local; _FlagAligner sets other free-end sets"""
    b = pkg.Aligner.new().matrix(pm).gap_open(open_).gap_extend(ext)
    if mode == 0:
        b.global_()
    elif mode == 2:
        b.local()
    else:
        b.semi_global()
    return b.build()


class _FlagAligner:
    """an aligner whose batch config carries an explicit free-end set (every one of the 16)"""

    def __init__(self, pkg, al, flags):
        self.pkg, self.al, self.flags = pkg, al, flags

    def _cfg(self, want):
        cfg = self.al._config()
        cfg.sg_flags = self.flags
        cfg.want = want
        return cfg

    def align_batch_banded_cigar(self, qs, rs, band, diag=None, stats=False):
        pkg = self.pkg
        qb, qo = pkg.pack(qs); rb, ro = pkg.pack(rs)
        n = len(rs)
        cfg = self._cfg(pkg.WANT_CIGAR | (pkg.WANT_STATS if stats else 0))
        out = np.zeros(n, dtype=pkg.RECORD_DTYPE); st = np.zeros(n, dtype=pkg.STATS_DTYPE); coff = np.zeros(n + 1, dtype=np.int64)
        d = None if diag is None else np.ascontiguousarray(diag, dtype=np.int32)
        cbuf = C.c_void_p()
        rc = pkg.lib.pmx_align_batch_banded_cigar(C.byref(cfg), None, n, qb.ctypes.data, qo.ctypes.data, rb.ctypes.data, ro.ctypes.data,
                                                  band, None if d is None else d.ctypes.data, out.ctypes.data, st.ctypes.data,
                                                  C.byref(cbuf), coff.ctypes.data)
        assert rc == 0, pkg.lib.pmx_last_error()
        raw = C.string_at(cbuf.value, int(coff[n])) if coff[n] else b""
        pkg.lib.pmx_free(cbuf)
        cig = [raw[coff[k]:coff[k + 1]].decode() for k in range(n)]
        return (out, cig, st) if stats else (out, cig)

    def align_batch_banded(self, qs, rs, band, diag=None):
        pkg = self.pkg
        qb, qo = pkg.pack(qs); rb, ro = pkg.pack(rs)
        n = len(rs)
        cfg = self._cfg(0)
        out = np.zeros(n, dtype=pkg.RECORD_DTYPE)
        d = None if diag is None else np.ascontiguousarray(diag, dtype=np.int32)
        rc = pkg.lib.pmx_align_batch_banded(C.byref(cfg), None, n, qb.ctypes.data, qo.ctypes.data, rb.ctypes.data, ro.ctypes.data,
                                            band, None if d is None else d.ctypes.data, out.ctypes.data)
        assert rc == 0, pkg.lib.pmx_last_error()
        return out


@pytest.mark.parametrize("mf", [(0, 0), (2, 0)] + [(1, f) for f in range(16)])
def test_banded_cigar_every_mode_and_free_end_set(pkg, orc, mf):
    mode, flags = mf
    band = BANDS[(mode * 16 + flags) % len(BANDS)]
    rng = np.random.default_rng(9300 + 17 * mode + flags)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    al = _FlagAligner(pkg, _aligner(pkg, mode, flags, pm, 5, 2), flags)
    qs, rs, diag = _pairs(rng, 90, 1, 160, band)
    _check(pkg, orc, al, mode, flags, qs, rs, band, diag, 5, 2, om, kernel="pmx_banded_staged_kernel/trace")
    if mode == 0:
        _check(pkg, orc, al, mode, flags, qs, rs, band, None, 5, 2, om)


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_banded_cigar_every_band(pkg, orc, mode, band):
    rng = np.random.default_rng(9400 + 3 * band + mode)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    al = _aligner(pkg, mode, orc.SG_ALL, pm, 5, 2)
    qs, rs, diag = _pairs(rng, 70, 1, 220, band)
    _check(pkg, orc, al, mode, orc.SG_ALL, qs, rs, band, diag, 5, 2, om, kernel="pmx_banded_staged_kernel/trace")


@pytest.mark.parametrize("which", ["default", "blosum62", "open_lt_extend"])
def test_banded_cigar_matrices(pkg, orc, which):
    rng = np.random.default_rng(9500 + len(which))
    if which == "default":
        pm, om, o, e, alpha = pkg.Matrix.default(), orc.Matrix.create("ACGTA", 1, -1), 5, 2, None
    elif which == "blosum62":
        pm, om, o, e, alpha = pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt")), 11, 1, AA
    else:
        pm, om, o, e, alpha = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3), 2, 3, None
    for mode, band in ((0, 16), (1, 7), (2, 31)):
        al = _aligner(pkg, mode, orc.SG_ALL, pm, o, e)
        qs, rs, diag = _pairs(rng, 60, 1, 150, band, alpha)
        _check(pkg, orc, al, mode, orc.SG_ALL, qs, rs, band, diag, o, e, om)


def test_banded_cigar_checked_kernel_long_pair(pkg, orc):
    """a pair beyond the LDS staging limit sends the launch to the checked kernel"""
    rng = np.random.default_rng(9600)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    for mode, band in ((0, 15), (2, 15), (1, 40)):
        al = _aligner(pkg, mode, orc.SG_ALL, pm, 5, 2)
        qs, rs, diag = _pairs(rng, 30, 1, 200, band)
        long_q = random_seqs(rng, 1, 21000, 21000)[0]
        qs.append(long_q)
        rs.append(mutate(rng, long_q, 0.05, 0.0))
        diag = np.append(diag, 0).astype(np.int32)
        _check(pkg, orc, al, mode, orc.SG_ALL, qs, rs, band, diag, 5, 2, om, kernel="pmx_banded_kernel/trace")


def test_banded_cigar_profile_arm_cfg5_shape(pkg, orc):
    """the profile arm at a scaled-down config-5 shape: 1 kbp query, 0.5-5 kbp references, band 48, SW, centres from a first pass"""
    n = 160
    q, rbuf, roff, planted = wl.make_cfg5(n * 50, rank=3)
    rs = [rbuf[roff[k]:roff[k + 1]].tobytes() for k in list(planted[:40]) + list(range(n - 40))]
    rb, ro = orc.pack(rs)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    al = pkg.Aligner.new().local().profile(pkg.Profile.new(q, False, pm)).matrix(pm).gap_open(5).gap_extend(2).build()
    full = al.align_batch_packed(None, None, rb, ro)
    diag = (full["end_ref"] - full["end_query"]).astype(np.int32)
    rec, cig, st = _check(pkg, orc, al, orc.SW, 0, [], rs, 48, diag, 5, 2, om, profile_query=q, oracle_idx=range(0, len(rs), 3))
    assert (rec["score"][:40] == full["score"][:40]).all()         # the planted copies stay inside the band


def test_banded_cigar_several_chunks(pkg, orc, monkeypatch):
    rng = np.random.default_rng(9700)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    al = _aligner(pkg, 1, orc.SG_ALL, pm, 5, 2)
    qs, rs, diag = _pairs(rng, 2000, 50, 200, 15)
    one = al.align_batch_banded_cigar(qs, rs, 15, diag, stats=True)
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", "300000")          # ~60 pairs a chunk: many chunks, two trace buffers
    rec, cig, st = _check(pkg, orc, al, 1, orc.SG_ALL, qs, rs, 15, diag, 5, 2, om, oracle_idx=range(0, 2000, 13))
    assert (rec == one[0]).all() and cig == one[1] and (st == one[2]).all()


def test_banded_cigar_device_capacity(pkg, orc):
    """pmx_align_batch_banded_cigar_device: a text buffer that is too small is reported and not overrun, then a sufficient one"""
    import torch
    rng = np.random.default_rng(9800)
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    al = _aligner(pkg, 1, orc.SG_ALL, pm, 5, 2)
    qs, rs, diag = _pairs(rng, 500, 100, 250, 31)
    want_rec, want_cig = al.align_batch_banded_cigar(qs, rs, 31, diag)
    qb, qo = pkg.pack(qs); rb, ro = pkg.pack(rs)
    n = len(rs)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(x).to(dev) for x in (qb, qo, rb, ro, diag)]
    out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    toff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    cfg = al._config()
    cfg.want = pkg.WANT_CIGAR
    stream = torch.cuda.current_stream(dev).cuda_stream
    mq, mr = max(len(x) for x in qs), max(len(x) for x in rs)
    small = torch.full((2048 + 64,), 0x55, dtype=torch.uint8, device=dev)
    rc = pkg.lib.pmx_align_batch_banded_cigar_device(C.byref(cfg), None, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                     d[3].data_ptr(), mq, mr, 31, d[4].data_ptr(), out.data_ptr(), None,
                                                     small.data_ptr(), 2048, toff.data_ptr(), stream)
    assert rc == 0, pkg.lib.pmx_last_error()
    torch.cuda.synchronize()
    need = int(toff[n].item())
    assert need > 2048 and (small[2048:] == 0x55).all()
    text = torch.zeros(need, dtype=torch.uint8, device=dev)
    rc = pkg.lib.pmx_align_batch_banded_cigar_device(C.byref(cfg), None, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                     d[3].data_ptr(), mq, mr, 31, d[4].data_ptr(), out.data_ptr(), None,
                                                     text.data_ptr(), need, toff.data_ptr(), stream)
    assert rc == 0, pkg.lib.pmx_last_error()
    torch.cuda.synchronize()
    raw = text.cpu().numpy().tobytes()
    o = toff.cpu().numpy()
    assert [raw[o[k]:o[k + 1]].decode() for k in range(n)] == want_cig
    assert (out.cpu().numpy().view(pkg.RECORD_DTYPE).reshape(-1) == want_rec).all()


@pytest.mark.parametrize("mismatch", (-3, -1))
def test_banded_cigar_text_beyond_the_estimate(pkg, orc, mismatch):
    """the host entry's second pass: alternating match / mismatch pairs ("1=1X..." is two bytes of text per symbol) push the text past
    the first capacity, (query bytes + reference bytes) / 2 + 16 n + 256, and the batch runs again with the exact size"""
    import torch
    rng = np.random.default_rng(9850 - mismatch)
    pm, om = pkg.Matrix.create(b"ACGT", 2, mismatch), orc.Matrix.create("ACGT", 2, mismatch)
    al = _aligner(pkg, 0, 0, pm, 5, 2)
    qs = random_seqs(rng, 6, 100, 300)
    rs = [mutate(rng, q, 0.08, 0.01) for q in qs]
    for at, L in ((0, 600), (2, 2000), (5, 600), (9, 2000)):          # among ordinary related pairs: per-pair offsets and the total
        qs.insert(at, (b"AC" * L)[:L]); rs.insert(at, (b"AG" * L)[:L])
    n = len(rs)
    rec, cig, st = _check(pkg, orc, al, 0, 0, qs, rs, 31, None, 5, 2, om)
    estimate = (sum(len(x) for x in qs) + sum(len(x) for x in rs)) // 2 + 16 * n + 256
    assert sum(len(c) for c in cig) > estimate                     # = cigar_off[n]: the first pass cannot have held it
    for at, L in ((0, 600), (2, 2000), (5, 600), (9, 2000)):
        assert cig[at] == "1=1X" * (L // 2) and rec["score"][at] == (2 + mismatch) * (L // 2)
    # the device entry into an exact-size buffer
    qb, qo = pkg.pack(qs); rb, ro = pkg.pack(rs)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(x).to(dev) for x in (qb, qo, rb, ro)]
    out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    dst = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    toff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    need = sum(len(c) for c in cig)
    text = torch.zeros(need, dtype=torch.uint8, device=dev)
    cfg = al._config()
    cfg.want = pkg.WANT_CIGAR | pkg.WANT_STATS
    rc = pkg.lib.pmx_align_batch_banded_cigar_device(C.byref(cfg), None, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                     d[3].data_ptr(), max(len(x) for x in qs), max(len(x) for x in rs), 31, None,
                                                     out.data_ptr(), dst.data_ptr(), text.data_ptr(), need, toff.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, pkg.lib.pmx_last_error()
    torch.cuda.synchronize()
    raw, o = text.cpu().numpy().tobytes(), toff.cpu().numpy()
    assert o[n] == need and [raw[o[k]:o[k + 1]].decode() for k in range(n)] == cig
    assert (out.cpu().numpy().view(pkg.RECORD_DTYPE).reshape(-1) == rec).all()
    assert (dst.cpu().numpy().view(pkg.STATS_DTYPE).reshape(-1) == st).all()


def test_banded_cigar_300kbp_pair(pkg, orc):
    """one 300 kbp x 300 kbp global pair at band 32: re-scored and band-checked (the oracle is too slow here)"""
    rng = np.random.default_rng(9900)
    L = 300000
    q = random_seqs(rng, 1, L, L)[0]
    r = mutate(rng, q, 0.05, 0.004)
    r = (r + random_seqs(rng, 1, L, L)[0])[:L]
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    al = _aligner(pkg, 0, 0, pm, 5, 2)
    rec, cig, st = al.align_batch_banded_cigar([q], [r], 32, None, stats=True)
    assert pkg.lib.pmx_last_kernel().decode() == "pmx_banded_kernel/trace + pmx_walkb_kernel"
    assert rec["score"][0] > NEG and (rec["end_query"][0], rec["end_ref"][0]) == (L - 1, L - 1)
    assert (rec == al.align_batch_banded([q], [r], 32)).all()
    _in_band_and_rescore(orc, cig, rec, [q], [r], 32, None, 5, 2, om, 0)
    ops = cigar_ops(cig[0])
    assert st["length"][0] == sum(l for l, _ in ops) and st["matches"][0] == sum(l for l, op in ops if op == "=")
