"""CPU tier: the tiled traceback of long pairs (pmx_align_batch_cigar_long).

1. tests/tilewalk_model.c -- the stored form of the checkpoint sweep (row granules (H, F), column checkpoints (H, E), with the
   sweep's skew), the re-derivation of one tile from its two boundaries, the four decision bits and the state carried over a tile
   border -- against the oracle: CIGAR text, begin cell and statistics identical for tiles as small as 4 x 4 and 8 x 3.
2. the planner pmx_long_cigar_scratch_bytes and the refusals of the host entry, none of which needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from util import random_seqs, mutate, AA, DNA, golden

HERE = os.path.dirname(os.path.abspath(__file__))
TILES = ((4, 4), (8, 3), (16, 8), (64, 16))                 # (band rows, tile columns)
GAPS = ((5, 2), (10, 1), (1, 1))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tilewalk_model") / "tilewalk_model.so")
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "tilewalk_model.c")], check=True)
    lib = C.CDLL(so)
    lib.tilewalk_model.restype = C.c_int
    return lib


def _runs(ops):
    out, k = [], 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append("%d%s" % (e - k, ops[k]))
        k = e
    return "".join(out)


def _model_pair(model, mode, flags, q, r, o, e, om, br, c, rec):
    qa, ra = np.frombuffer(q, dtype=np.uint8), np.frombuffer(r, dtype=np.uint8)
    ops = C.create_string_buffer(len(q) + len(r) + 2)
    beg, st, cells = (C.c_int * 2)(), (C.c_int * 3)(), C.c_long()
    n = model.tilewalk_model(mode, flags, qa.ctypes.data_as(C.c_void_p), len(q), ra.ctypes.data_as(C.c_void_p), len(r), o, e,
                             om.scores.ctypes.data_as(C.c_void_p), om.size, om.mapper.ctypes.data_as(C.c_void_p), br, c,
                             int(rec[0]), int(rec[1]), int(rec[2]), ops, beg, st, C.byref(cells))
    assert n >= 0
    return _runs(ops.value.decode()), (beg[0], beg[1]), (st[0], st[1], st[2]), cells.value


def _pairs(rng, n, alphabet, hi=80):
    qs = random_seqs(rng, n, 1, hi, alphabet=alphabet)
    rs = []
    for t, q in enumerate(qs):
        if t % 3 == 0:
            rs.append(random_seqs(rng, 1, 1, hi, alphabet=alphabet)[0])
        elif t % 3 == 1:
            rs.append(mutate(rng, q, 0.10, 0.08, alphabet=alphabet)[:hi])
        else:                                                  # a long gap on one side
            cut = int(rng.integers(0, len(q) + 1)); ln = int(rng.integers(0, 30))
            rs.append((q[:cut] + q[cut + ln:]) or q[:1])
            if t % 2:
                qs[t], rs[t] = rs[t], qs[t]
    return qs, rs


def _check(model, orc, mode, flags, qs, rs, o, e, om, tiles=TILES):
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    idx = np.arange(len(qs))
    cig, rec = orc.cigar_sample(mode, idx, qb, qo, rb, ro, o, e, om, sg_flags=flags)
    st = orc.align_stats_sample(mode, idx, qb, qo, rb, ro, o, e, om, sg_flags=flags)
    for k in range(len(qs)):
        for br, c in tiles:
            text, beg, stats, _ = _model_pair(model, mode, flags, qs[k], rs[k], o, e, om, br, c, rec[k])
            ctx = (mode, flags, o, e, br, c, qs[k], rs[k])
            assert text == cig[k], ctx + (text, cig[k])
            assert beg == (rec[k][3], rec[k][4]), ctx + (beg, rec[k])
            assert stats == tuple(int(x) for x in st[k][3:6]), ctx + (stats, st[k])


def _matrices(orc):
    return (("acgt", orc.Matrix.create("ACGT", 2, -3), DNA), ("default", orc.Matrix.default(), DNA),
            ("blosum62", orc.Matrix.from_file(golden("blosum62.txt")), AA))


@pytest.mark.parametrize("mode,flags", [(0, 0), (2, 0)] + [(1, f) for f in range(16)])
def test_model_equals_oracle(model, orc, mode, flags):
    rng = np.random.default_rng(1000 + 16 * mode + flags)
    for name, om, alphabet in _matrices(orc):
        for o, e in GAPS:
            qs, rs = _pairs(rng, 30, alphabet)                 # 18 x 3 x 3 x 30 = 4 860 pairs, each under every tile size
            _check(model, orc, mode, flags, qs, rs, o, e, om)


@pytest.mark.parametrize("mode,flags", [(0, 0), (2, 0), (1, 15), (1, 0), (1, 5), (1, 10)])
def test_model_tie_heavy(model, orc, mode, flags):
    """homopolymers and two-letter sequences: every tie-break of the oracle is exercised many times over"""
    rng = np.random.default_rng(77 + mode + flags)
    two = np.frombuffer(b"AC", dtype=np.uint8)
    qs = [b"A" * int(n) for n in rng.integers(1, 70, size=12)] + random_seqs(rng, 40, 1, 70, alphabet=two) + [b"AC" * 20, b"A" * 30 + b"C" * 30]
    rs = [b"A" * int(n) for n in rng.integers(1, 70, size=12)] + random_seqs(rng, 40, 1, 70, alphabet=two) + [b"CA" * 25, b"C" * 30 + b"A" * 30]
    for name, om, _ in _matrices(orc)[:2]:
        for o, e in GAPS + ((0, 0), (2, 5)):
            _check(model, orc, mode, flags, qs, rs, o, e, om, tiles=((4, 4), (8, 3)))


def test_model_rederives_a_small_share(model, orc):
    """related pairs: the tiles the path enters are a small share of the table (the reason for the scheme)"""
    rng = np.random.default_rng(5)
    q = random_seqs(rng, 1, 2000, 2000)[0]
    r = mutate(rng, q, 0.05, 0.02)
    om = orc.Matrix.create("ACGT", 2, -3)
    qb, qo = orc.pack([q]); rb, ro = orc.pack([r])
    cig, rec = orc.cigar_sample(0, [0], qb, qo, rb, ro, 5, 2, om)
    text, beg, stats, cells = _model_pair(model, 0, 0, q, r, 5, 2, om, 128, 64, rec[0])
    assert text == cig[0]
    assert cells <= (len(q) // 128 + len(r) // 64 + 2) * 128 * 64 and cells < 0.15 * len(q) * len(r)


# ---- planner and refusals (no GPU) ----------------------------------------------------------------------------------------------
SHAPES = ((20_000, 20_000), (100_000, 100_000), (300_000, 300_000), (1_000, 1_000_000), (1_000_000, 1_000))


@pytest.mark.parametrize("band_rows", (0, 128, 256, 1024))
@pytest.mark.parametrize("tile_cols", (0, 128, 256))
def test_planner_is_linear(pkg, band_rows, tile_cols):
    """an 8-byte granule per 128th row is m n / 16, one per 128th column the same again; coarser tiles only lower it"""
    for m, n in SHAPES:
        got = pkg.long_cigar_scratch_bytes(1, m, n, tile_cols, band_rows)
        bound = m * n // 8 + 64 * (m + n) + (1 << 20)
        print(band_rows, tile_cols, m, n, got, bound)
        assert 0 < got <= bound, (band_rows, tile_cols, m, n, got, bound)


def test_planner_grows_linearly_up_to_the_chunk_budget(pkg, monkeypatch):
    one = pkg.long_cigar_scratch_bytes(1, 5000, 5000)
    for k in (2, 8, 64):
        got = pkg.long_cigar_scratch_bytes(k, 5000, 5000)
        assert k * (one - 512) <= got <= k * one, (k, one, got)
    monkeypatch.setenv("PMX_LONG_CHUNK_BYTES", str(3 * one))
    assert pkg.long_cigar_scratch_bytes(64, 5000, 5000) <= 3 * one      # a chunk, not the batch
    monkeypatch.setenv("PMX_LONG_CHUNK_BYTES", "1")
    assert pkg.long_cigar_scratch_bytes(64, 5000, 5000) == one           # a single pair always gets what it needs


def test_planner_and_entry_refusals_without_gpu(pkg):
    lib = pkg.lib
    for tile, rows in ((32, 0), (100, 0), (512, 0), (0, 64), (0, 512), (-1, 0)):
        opts = pkg.pmx_long_cigar_opts_t(tile, rows)
        assert lib.pmx_long_cigar_scratch_bytes(1, 1000, 1000, C.byref(opts)) == -1
        assert b"not offered" in lib.pmx_last_error()
    assert lib.pmx_long_cigar_scratch_bytes(0, 1000, 1000, None) == -1
    assert lib.pmx_long_cigar_scratch_bytes(1, 1000, 1000, None) > 0

    al = pkg.Aligner.new().build()
    qb, qo = pkg.pack([b"ACGT"]); rb, ro = pkg.pack([b"ACGA"])
    out = np.zeros(1, dtype=pkg.RECORD_DTYPE); st = np.zeros(1, dtype=pkg.STATS_DTYPE); coff = np.zeros(2, dtype=np.int64)
    cbuf = C.c_void_p()

    def call(cfg, qoff=qo, opts=None):
        return lib.pmx_align_batch_cigar_long(C.byref(cfg), 1, qb.ctypes.data, qoff.ctypes.data, rb.ctypes.data, ro.ctypes.data,
                                              out.ctypes.data, st.ctypes.data, C.byref(cbuf), coff.ctypes.data, opts)

    cfg = pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 32, 0, al.matrix.inner)                   # a want without CIGAR and STATS
    assert call(cfg) == -1 and b"PMX_WANT_CIGAR" in lib.pmx_last_error()
    cfg = pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 32, pkg.WANT_SORTED, al.matrix.inner)
    assert call(cfg) == -1 and b"PMX_WANT_CIGAR" in lib.pmx_last_error()
    pssm = pkg.Matrix.create_pssm(b"ACGT", [1, 0, 0, 0, 0] * 4, 4)
    cfg = pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 32, pkg.WANT_CIGAR, pssm.inner)
    assert call(cfg) == -1 and b"PSSM" in lib.pmx_last_error()
    cfg = pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 32, pkg.WANT_CIGAR, al.matrix.inner)
    bad = np.array([0, 0], dtype=np.int64)                                                 # an empty query
    assert call(cfg, qoff=bad) == -1 and b"bad offsets" in lib.pmx_last_error()
    bad = np.array([1, 4], dtype=np.int64)                                                 # offsets that do not start at 0
    assert call(cfg, qoff=bad) == -1 and b"bad offsets" in lib.pmx_last_error()
    assert call(cfg, opts=C.byref(pkg.pmx_long_cigar_opts_t(48, 0))) == -1 and b"not offered" in lib.pmx_last_error()
    cfg = pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 32, pkg.WANT_CIGAR | 64, al.matrix.inner)
    assert call(cfg) == -1 and b"unknown want" in lib.pmx_last_error()
