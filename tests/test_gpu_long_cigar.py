"""Tiled traceback of long pairs (`-m gpu`): pmx_align_batch_cigar_long / _device -- the checkpoint form of the long-pair sweep
(pmx_long.hip) and the tile re-derive + walk kernel (pmx_walkt.hip) -- through the C ABI against the oracle: records equal
orc.align_batch, CIGAR text equals orc.cigar_sample, statistics equal orc.align_stats_sample.  Beyond the oracle's table
(100 kbp x 100 kbp) the text is re-scored independently and the record compared with pmx_align_batch's.

Oracle cells of this file: fuzz 18 x 6 pairs of 300 .. 3 000 (~0.3e9, three passes), shaped cases ~0.1e9, ragged sample ~0.1e9,
two 20 kbp x 20 kbp pairs (0.8e9)."""
import ctypes as C

import numpy as np
import pytest

from util import random_seqs, mutate, AA, DNA, golden, cigar_ops

pytestmark = pytest.mark.gpu

GAPS = ((5, 2), (10, 1), (1, 1))
KERNEL_TAIL = "/checkpoint sweep + pmx_walkt_kernel"


def _matrix(pkg, orc, which):
    if which == 0:
        return pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3), DNA
    if which == 1:
        return pkg.Matrix.default(), orc.Matrix.default(), DNA
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt")), AA


def _run(pkg, mode, flags, pm, o, e, qs, rs, tile_cols=0, band_rows=0, want=None):
    """the host entry through the C ABI -> (records, list of CIGAR text, stats, text offsets, raw text)"""
    want = (pkg.WANT_CIGAR | pkg.WANT_STATS) if want is None else want
    cfg = pkg.pmx_config_t(mode, flags, o, e, 32, want, pm.inner)
    qb, qo = pkg.pack(qs); rb, ro = pkg.pack(rs)
    n = len(rs)
    out = np.zeros(n, dtype=pkg.RECORD_DTYPE); st = np.zeros(n, dtype=pkg.STATS_DTYPE); coff = np.zeros(n + 1, dtype=np.int64)
    cbuf = C.c_void_p()
    opts = pkg.pmx_long_cigar_opts_t(tile_cols, band_rows)
    rc = pkg.lib.pmx_align_batch_cigar_long(C.byref(cfg), n, qb.ctypes.data, qo.ctypes.data, rb.ctypes.data, ro.ctypes.data,
                                            out.ctypes.data, st.ctypes.data if want & pkg.WANT_STATS else None,
                                            C.byref(cbuf) if want & pkg.WANT_CIGAR else None,
                                            coff.ctypes.data if want & pkg.WANT_CIGAR else None, C.byref(opts))
    assert rc == 0, pkg.lib.pmx_last_error()
    name = pkg.lib.pmx_last_kernel().decode()
    assert name.startswith("pmx_long32_kernel") and name.endswith(KERNEL_TAIL), name
    raw = b""
    if want & pkg.WANT_CIGAR:
        raw = C.string_at(cbuf.value, int(coff[n])) if cbuf.value and coff[n] else b""
        if cbuf.value:
            pkg.lib.pmx_free(cbuf)
    return out, [raw[coff[k]:coff[k + 1]].decode() for k in range(n)], st, coff, raw


def _against_oracle(pkg, orc, mode, flags, om, o, e, qs, rs, got, idx=None, stats=True):
    rec, cig, st = got[:3]
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    idx = np.arange(len(rs)) if idx is None else np.asarray(idx)
    want_cig, want_rec = orc.cigar_sample(mode, idx, qb, qo, rb, ro, o, e, om, sg_flags=flags)
    for t, k in enumerate(idx):
        ctx = (mode, flags, o, e, int(k), len(qs[k]), len(rs[k]))
        assert (int(rec["score"][k]), int(rec["end_query"][k]), int(rec["end_ref"][k])) == tuple(int(x) for x in want_rec[t][:3]), ctx
        assert rec["flags"][k] == 0, ctx
        assert cig[k] == want_cig[t], ctx + (cig[k][:200], want_cig[t][:200])
    if stats:
        want_st = orc.align_stats_sample(mode, idx, qb, qo, rb, ro, o, e, om, sg_flags=flags)
        for t, k in enumerate(idx):
            assert (int(st["matches"][k]), int(st["similar"][k]), int(st["length"][k])) == tuple(int(x) for x in want_st[t][3:6]), (mode, flags, int(k))


def _related(rng, n, lo, hi, alphabet):
    qs = random_seqs(rng, n, lo, hi, alphabet=alphabet)
    rs = []
    for t, q in enumerate(qs):
        if t % 5 == 4:
            rs.append(random_seqs(rng, 1, lo, hi, alphabet=alphabet)[0])            # unrelated
        else:
            pre = random_seqs(rng, 1, 0, 200, alphabet=alphabet)[0] if t % 2 else b""
            rs.append((pre + mutate(rng, q, 0.08, 0.04, alphabet=alphabet))[:hi])
    return qs, rs


@pytest.mark.parametrize("case", range(18))
def test_geometry_fuzz(pkg, orc, case):
    """the smallest tile width, both common band heights: paths cross several bands and many column tiles"""
    mode, flags = ((0, 0), (2, 0))[case] if case < 2 else (1, case - 2)
    pm, om, alphabet = _matrix(pkg, orc, case % 3)
    o, e = GAPS[(case // 3) % 3]
    rng = np.random.default_rng(4100 + case)
    qs, rs = _related(rng, 6, 300, 3000, alphabet)
    first = None
    for rows in (128, 256):
        got = _run(pkg, mode, flags, pm, o, e, qs, rs, 64, rows)
        if first is None:
            _against_oracle(pkg, orc, mode, flags, om, o, e, qs, rs, got)
            first = got
        else:
            assert (got[0] == first[0]).all() and got[1] == first[1] and (got[2] == first[2]).all()


@pytest.mark.parametrize("gaps", GAPS)
def test_every_matrix_and_gap_set_local_and_global(pkg, orc, gaps):
    o, e = gaps
    rng = np.random.default_rng(4200 + o)
    for which in range(3):
        pm, om, alphabet = _matrix(pkg, orc, which)
        qs, rs = _related(rng, 4, 300, 1500, alphabet)
        for mode, flags in ((0, 0), (2, 0), (1, 15)):
            _against_oracle(pkg, orc, mode, flags, om, o, e, qs, rs, _run(pkg, mode, flags, pm, o, e, qs, rs, 64, 128))


def test_long_gap_runs_cross_tiles_and_bands(pkg, orc):
    """a 700-symbol deletion and insertion: an E run across >= 3 column tiles, an F run across >= 3 bands (carried states)"""
    rng = np.random.default_rng(4300)
    pm, om, _ = _matrix(pkg, orc, 0)
    q = random_seqs(rng, 1, 2400, 2400)[0]
    cut = q[:850] + q[1550:]
    qs, rs = [q, cut, mutate(rng, q, 0.03, 0.0), q[:850] + q[1550:]], [cut, q, q[:400] + q[1100:], mutate(rng, q, 0.03, 0.0)]
    for mode, flags in ((0, 0), (2, 0), (1, 15), (1, 0)):
        for o, e in ((5, 2), (10, 1), (1, 1)):
            got = _run(pkg, mode, flags, pm, o, e, qs, rs, 64, 128)
            _against_oracle(pkg, orc, mode, flags, om, o, e, qs, rs, got)
            if mode == 0:
                assert any(l >= 700 and op in "ID" for l, op in cigar_ops(got[1][0]))
                assert any(l >= 700 and op in "ID" for l, op in cigar_ops(got[1][1]))


def test_lengths_at_tile_and_band_borders(pkg, orc):
    """k 256 + {-1, 0, 1} rows and k C + {-1, 0, 1} columns: in NW the end cell sits in every corner of a tile"""
    rng = np.random.default_rng(4400)
    pm, om, _ = _matrix(pkg, orc, 0)
    qs, rs = [], []
    for dq in (-1, 0, 1):
        for dr in (-1, 0, 1):
            q = random_seqs(rng, 1, 2 * 256 + dq, 2 * 256 + dq)[0]
            r = mutate(rng, q, 0.06, 0.03)
            r = (r + random_seqs(rng, 1, 400, 400)[0])[:5 * 64 + dr] if dr >= 0 else r[:5 * 64 + dr]
            qs.append(q); rs.append(r)
            qs.append(r); rs.append(q)
    for tile, rows in ((64, 256), (64, 128), (128, 256)):
        for mode, flags in ((0, 0), (2, 0), (1, 15), (1, 6), (1, 9)):
            _against_oracle(pkg, orc, mode, flags, om, 5, 2, qs, rs, _run(pkg, mode, flags, pm, 5, 2, qs, rs, tile, rows))


def test_degenerate_shapes(pkg, orc):
    """qlen = 1, rlen = 1, a query shorter than one band against a 50 kbp reference and the transpose"""
    rng = np.random.default_rng(4500)
    pm, om, _ = _matrix(pkg, orc, 0)
    long_r = random_seqs(rng, 1, 50000, 50000)[0]
    short = long_r[31000:31100]
    qs = [b"A", b"C", random_seqs(rng, 1, 700, 700)[0], b"G", short, long_r, mutate(rng, short, 0.1, 0.05)]
    rs = [b"A", random_seqs(rng, 1, 700, 700)[0], b"T", b"A", long_r, short, long_r]
    for mode, flags in ((0, 0), (2, 0), (1, 15), (1, 0), (1, 3), (1, 12)):
        _against_oracle(pkg, orc, mode, flags, om, 5, 2, qs, rs, _run(pkg, mode, flags, pm, 5, 2, qs, rs, 64, 0))
    _against_oracle(pkg, orc, 2, 0, om, 5, 2, qs, rs, _run(pkg, 2, 0, pm, 5, 2, qs, rs, 0, 0))


def test_local_paths_short_or_inside_one_tile(pkg, orc):
    """a local alignment that starts and ends inside one tile of a large pair; unrelated sequences (short paths)"""
    rng = np.random.default_rng(4600)
    pm, om, _ = _matrix(pkg, orc, 0)
    q = bytearray(random_seqs(rng, 1, 3000, 3000)[0]); r = bytearray(random_seqs(rng, 1, 3000, 3000)[0])
    core = random_seqs(rng, 1, 40, 40)[0]
    q[1290:1330] = core; r[1670:1710] = core                  # rows 1280 .. 1535, columns 1664 .. 1727: one 256 x 64 tile
    qs = [bytes(q)] + random_seqs(rng, 5, 1500, 2500)
    rs = [bytes(r)] + random_seqs(rng, 5, 1500, 2500)
    got = _run(pkg, 2, 0, pm, 5, 2, qs, rs, 64, 256)
    _against_oracle(pkg, orc, 2, 0, om, 5, 2, qs, rs, got)
    assert 1290 <= got[0]["end_query"][0] - 39 and got[0]["end_query"][0] < 1536 and sum(l for l, _ in cigar_ops(got[1][0])) < 64


def _rescore(orc, mode, om, o, e, qs, rs, rec, cig, st, flags=0):
    """independent check of texts the oracle's table cannot reach (semi-global: the text spans both sequences, gap runs at the
    free ends cost nothing, and the statistics stop at the end cell, so they are not read off the text)"""
    n = len(rs)
    text = np.frombuffer("".join(cig).encode() or b"\0", dtype=np.uint8)
    toff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cig], out=toff[1:])
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    beg = None
    cons = []
    for k, c in enumerate(cig):
        ops = cigar_ops(c)
        cons.append((sum(l for l, op in ops if op in "=XI"), sum(l for l, op in ops if op in "=XD"),
                     sum(l for l, op in ops if op == "="), sum(l for l, _ in ops)))
    if mode == orc.SW:
        beg = np.array([[rec["end_query"][k] + 1 - cons[k][0], rec["end_ref"][k] + 1 - cons[k][1]] for k in range(n)], dtype=np.int32).reshape(-1)
        assert (beg >= 0).all()
    got, bad = orc.rescore_cigars(text, toff, qb, qo, rb, ro, o, e, om, beg=beg, free_mask=flags if mode == orc.SG else 0)
    assert bad == 0
    for k in range(n):
        assert got[k, 0] == rec["score"][k] and got[k, 3] == 0, (k, got[k], rec[k])
        assert (got[k, 1], got[k, 2]) == cons[k][:2]
        if mode != orc.SW:
            assert cons[k][:2] == (len(qs[k]), len(rs[k]))
        if mode != orc.SG:
            assert (int(st["matches"][k]), int(st["length"][k])) == cons[k][2:], (k, st[k], cons[k])


def test_ragged_batch_and_chunks(pkg, orc, monkeypatch):
    """64 pairs from 200 to 12 000 symbols in one call; the same batch in several chunks: identical bytes"""
    rng = np.random.default_rng(4700)
    pm, om, _ = _matrix(pkg, orc, 0)
    lens = (200 + 11800 * rng.random(64) ** 3).astype(int)
    lens[7] = 12000; lens[40] = 200
    qs = [random_seqs(rng, 1, int(l), int(l))[0] for l in lens]
    rs = [mutate(rng, q, 0.07, 0.03) if k % 6 else random_seqs(rng, 1, 200, 3000)[0] for k, q in enumerate(qs)]
    small = [int(k) for k in np.argsort(lens)[:40:5]] + [40]
    for mode, flags in ((1, 15), (2, 0)):
        got = _run(pkg, mode, flags, pm, 5, 2, qs, rs)
        ref = pkg.Aligner.new().matrix(pm).gap_open(5).gap_extend(2)
        ref = (ref.semi_global() if mode == 1 else ref.local()).solution_width(32).build().align_batch(qs, rs)
        for f in ("score", "end_query", "end_ref"):
            assert (got[0][f] == ref[f]).all(), f
        _against_oracle(pkg, orc, mode, flags, om, 5, 2, qs, rs, got, idx=small)
        _rescore(orc, mode, om, 5, 2, qs, rs, *got[:3], flags=flags)
        one = pkg.long_cigar_scratch_bytes(1, max(len(x) for x in qs), max(len(x) for x in rs))
        monkeypatch.setenv("PMX_LONG_CHUNK_BYTES", str(5 * one))
        again = _run(pkg, mode, flags, pm, 5, 2, qs, rs)
        monkeypatch.delenv("PMX_LONG_CHUNK_BYTES")
        assert (again[0] == got[0]).all() and (again[2] == got[2]).all() and (again[3] == got[3]).all() and again[4] == got[4]


@pytest.mark.parametrize("mode", (0, 2))
def test_20kbp_default_tile_against_oracle(pkg, orc, mode):
    rng = np.random.default_rng(4800 + mode)
    pm, om, _ = _matrix(pkg, orc, 0)
    q = random_seqs(rng, 1, 20000, 20000)[0]
    r = mutate(rng, q, 0.08, 0.03)
    if mode == 2:
        r = random_seqs(rng, 1, 900, 900)[0] + r[2000:17000] + random_seqs(rng, 1, 700, 700)[0]
    got = _run(pkg, mode, 0, pm, 5, 2, [q], [r])
    _against_oracle(pkg, orc, mode, 0, om, 5, 2, [q], [r], got, stats=False)
    _rescore(orc, mode, om, 5, 2, [q], [r], *got[:3])


@pytest.mark.parametrize("mode", (0, 2))
def test_100kbp_pair_in_linear_memory(pkg, orc, mode):
    """beyond the oracle's table (and 10 GB of byte trace): record = pmx_align_batch's, text re-scored, statistics read off the text"""
    rng = np.random.default_rng(4900 + mode)
    pm, om, _ = _matrix(pkg, orc, 0)
    L = 100000
    q = random_seqs(rng, 1, L, L)[0]
    r = mutate(rng, q, 0.10 if mode == 2 else 0.05, 0.01)
    r = (r + random_seqs(rng, 1, L, L)[0])[:L]
    need = pkg.long_cigar_scratch_bytes(1, L, L)
    assert need <= L * L // 8 + 64 * 2 * L + (1 << 20)
    got = _run(pkg, mode, 0, pm, 5, 2, [q], [r])
    b = pkg.Aligner.new().matrix(pm).gap_open(5).gap_extend(2)
    ref = (b.global_() if mode == 0 else b.local()).solution_width(32).build().align_batch([q], [r])
    assert (got[0] == ref).all(), (got[0], ref)
    _rescore(orc, mode, om, 5, 2, [q], [r], *got[:3])


def test_device_entry_and_capacity(pkg, orc):
    import torch
    rng = np.random.default_rng(5000)
    pm, om, _ = _matrix(pkg, orc, 0)
    qs, rs = _related(rng, 12, 500, 4000, DNA)
    want = _run(pkg, 1, 15, pm, 5, 2, qs, rs)
    qb, qo = pkg.pack(qs); rb, ro = pkg.pack(rs)
    n = len(rs)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(x).to(dev) for x in (qb, qo, rb, ro)]
    out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    st = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    toff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    cfg = pkg.pmx_config_t(1, 15, 5, 2, 32, pkg.WANT_CIGAR | pkg.WANT_STATS, pm.inner)
    stream = torch.cuda.current_stream(dev).cuda_stream
    mq, mr = max(len(x) for x in qs), max(len(x) for x in rs)
    cap = int(want[3][5]) + 3                                   # room for the first five texts and a little
    small = torch.full((cap + 64,), 0x55, dtype=torch.uint8, device=dev)
    pkg.align_batch_cigar_long_device(cfg, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), mq, mr,
                                      out.data_ptr(), st.data_ptr(), small.data_ptr(), cap, toff.data_ptr(), stream)
    torch.cuda.synchronize()
    o = toff.cpu().numpy()
    assert (o == want[3]).all() and (small[cap:] == 0x55).all()
    raw = small.cpu().numpy().tobytes()
    assert o[5] + 3 < o[6]                                       # (pair 5 does not fit: nothing of it may be written)
    assert raw[:o[5]] == want[4][:o[5]] and raw[o[5]:cap] == b"\x55" * (cap - int(o[5]))     # texts that fit are written, the others not
    text = torch.zeros(int(o[n]), dtype=torch.uint8, device=dev)
    pkg.align_batch_cigar_long_device(cfg, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), mq, mr,
                                      out.data_ptr(), st.data_ptr(), text.data_ptr(), int(o[n]), toff.data_ptr(), stream, 64, 128)
    torch.cuda.synchronize()
    assert text.cpu().numpy().tobytes() == want[4] and (toff.cpu().numpy() == want[3]).all()
    assert (out.cpu().numpy().view(pkg.RECORD_DTYPE).reshape(-1) == want[0]).all()
    assert (st.cpu().numpy().view(pkg.STATS_DTYPE).reshape(-1) == want[2]).all()


@pytest.mark.parametrize("mismatch", (-3, -1))
def test_text_beyond_the_estimate(pkg, orc, mismatch):
    """the host entry's second pass: alternating match / mismatch pairs ("1=1X..." is two bytes of text per symbol) push the text past
    the first capacity, (query bytes + reference bytes) / 2 + 16 n + 256, and the batch runs again with the exact size"""
    import torch
    rng = np.random.default_rng(5025 - mismatch)
    pm, om = pkg.Matrix.create(b"ACGT", 2, mismatch), orc.Matrix.create("ACGT", 2, mismatch)
    qs, rs = _related(rng, 6, 300, 900, DNA)
    for at, L in ((0, 600), (2, 2000), (5, 600), (9, 2000)):          # among ordinary related pairs: per-pair offsets and the total
        qs.insert(at, (b"AC" * L)[:L]); rs.insert(at, (b"AG" * L)[:L])
    n = len(rs)
    got = _run(pkg, 0, 0, pm, 5, 2, qs, rs)
    rec, cig, st, coff, raw = got
    estimate = (sum(len(x) for x in qs) + sum(len(x) for x in rs)) // 2 + 16 * n + 256
    assert coff[n] > estimate and coff[n] == len(raw)              # the first pass cannot have held it
    for at, L in ((0, 600), (2, 2000), (5, 600), (9, 2000)):
        assert cig[at] == "1=1X" * (L // 2) and rec["score"][at] == (2 + mismatch) * (L // 2)
    _against_oracle(pkg, orc, 0, 0, om, 5, 2, qs, rs, got)
    # the device entry into an exact-size buffer
    qb, qo = pkg.pack(qs); rb, ro = pkg.pack(rs)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(x).to(dev) for x in (qb, qo, rb, ro)]
    out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    dst = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    toff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    text = torch.zeros(int(coff[n]), dtype=torch.uint8, device=dev)
    cfg = pkg.pmx_config_t(0, 0, 5, 2, 32, pkg.WANT_CIGAR | pkg.WANT_STATS, pm.inner)
    pkg.align_batch_cigar_long_device(cfg, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                      max(len(x) for x in qs), max(len(x) for x in rs), out.data_ptr(), dst.data_ptr(),
                                      text.data_ptr(), int(coff[n]), toff.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert text.cpu().numpy().tobytes() == raw and (toff.cpu().numpy() == coff).all()
    assert (out.cpu().numpy().view(pkg.RECORD_DTYPE).reshape(-1) == rec).all()
    assert (dst.cpu().numpy().view(pkg.STATS_DTYPE).reshape(-1) == st).all()


def test_device_entry_returns_before_the_work_is_done(pkg, orc):
    """the header's promise: a call whose scratch is already large enough does not synchronise with the host.  One 20 kbp pair is
    tens of milliseconds of device work; right after the (second, warmed-up) call returns the stream must still be busy."""
    import torch
    rng = np.random.default_rng(5050)
    pm, om, _ = _matrix(pkg, orc, 0)
    q = random_seqs(rng, 1, 20000, 20000)[0]
    r = mutate(rng, q, 0.08, 0.03)
    want = _run(pkg, 0, 0, pm, 5, 2, [q], [r])
    qb, qo = pkg.pack([q]); rb, ro = pkg.pack([r])
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(x).to(dev) for x in (qb, qo, rb, ro)]
    out = torch.zeros((1, 4), dtype=torch.int32, device=dev); st = torch.zeros((1, 3), dtype=torch.int32, device=dev)
    toff = torch.zeros(2, dtype=torch.int64, device=dev)
    cap = len(q) + len(r) + 64
    text = torch.zeros(cap, dtype=torch.uint8, device=dev)
    cfg = pkg.pmx_config_t(0, 0, 5, 2, 32, pkg.WANT_CIGAR | pkg.WANT_STATS, pm.inner)
    stream = torch.cuda.current_stream(dev)

    def call():
        pkg.align_batch_cigar_long_device(cfg, 1, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(q), len(r),
                                          out.data_ptr(), st.data_ptr(), text.data_ptr(), cap, toff.data_ptr(), stream.cuda_stream)

    call()                                                       # (allocates the scratch: may synchronise)
    torch.cuda.synchronize()
    out.zero_(); text.zero_(); toff.zero_()
    torch.cuda.synchronize()
    call()
    busy = not stream.query()                                    # asked before anything waits
    torch.cuda.synchronize()
    assert busy, "the device entry returned only after its work was done"
    o = toff.cpu().numpy()
    assert (o == want[3]).all() and text.cpu().numpy().tobytes()[:o[1]] == want[4]
    assert (out.cpu().numpy().view(pkg.RECORD_DTYPE).reshape(-1) == want[0]).all()
    assert (st.cpu().numpy().view(pkg.STATS_DTYPE).reshape(-1) == want[2]).all()


def test_options_are_result_neutral(pkg, orc):
    rng = np.random.default_rng(5100)
    pm, om, _ = _matrix(pkg, orc, 0)
    qs, rs = _related(rng, 8, 3000, 3000, DNA)
    for mode, flags in ((0, 0), (2, 0), (1, 15)):
        first = None
        for tile in (0, 64, 128, 256):
            for rows in (0, 128, 256, 1024):
                got = _run(pkg, mode, flags, pm, 5, 2, qs, rs, tile, rows)
                if first is None:
                    first = got
                    _against_oracle(pkg, orc, mode, flags, om, 5, 2, qs, rs, got, idx=[0, 4])
                assert (got[0] == first[0]).all() and (got[2] == first[2]).all() and (got[3] == first[3]).all() and got[4] == first[4], (tile, rows)
        only_stats = _run(pkg, mode, flags, pm, 5, 2, qs, rs, want=pkg.WANT_STATS)
        assert (only_stats[0] == first[0]).all() and (only_stats[2] == first[2]).all()
        only_cigar = _run(pkg, mode, flags, pm, 5, 2, qs, rs, want=pkg.WANT_CIGAR)
        assert only_cigar[4] == first[4]
