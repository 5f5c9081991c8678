"""Every launchable form of the long-pair sweep (`-m gpu`): the nine (rows per lane, columns per step, steps per boundary chunk)
shapes of pmx_long.hip's shape list, scores through pmx_align_batch and checkpoints through pmx_align_batch_cigar_long, each forced by
the PMX_LONG_* switches, in all three modes, against the oracle -- and pmx_last_kernel() names the instance that was asked for.
Four pairs per call: queries of BR + 1, 2 BR, 2 BR + 1 and 512 rows (BR = 64 R; at least 512, the road's threshold), references at
the chunk edges (63, 64, 65, 129 columns for one column per step, 127, 128, 129, 257 for two)."""
import numpy as np
import pytest

from util import random_seqs, mutate
from test_gpu_long_cigar import _run, _against_oracle

pytestmark = pytest.mark.gpu

FORMS = [(2, 1, 16), (2, 1, 64), (4, 1, 16), (4, 1, 64), (16, 1, 64), (2, 2, 32), (2, 2, 64), (4, 2, 32), (4, 2, 64)]


def _pairs(rng, R, cols):
    BR = 64 * R
    qlens = [max(L, 512) for L in (BR + 1, 2 * BR, 2 * BR + 1, 512)]
    rlens = (63, 64, 65, 129) if cols == 1 else (127, 128, 129, 257)
    qs = [random_seqs(rng, 1, L, L)[0] for L in qlens]
    rs = [(mutate(rng, q[100:100 + L], 0.08, 0.04) + random_seqs(rng, 1, L, L)[0])[:L] for q, L in zip(qs, rlens)]
    return qs, rs


def _force(monkeypatch, R, cols, steps, rows_switch):
    monkeypatch.setenv("PMX_LONG_MIN_CELLS", "0")
    monkeypatch.setenv("PMX_LONG_TWO_COLUMNS" if cols == 2 else "PMX_LONG_ONE_COLUMN", "1")
    monkeypatch.setenv("PMX_LONG_CHUNK_COLS", "64" if steps == 64 else "16")
    if rows_switch:
        monkeypatch.setenv("PMX_LONG_ROWS_PER_LANE", str(R))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("form", FORMS, ids=lambda f: "R%d-c%d-s%d" % f)
def test_score_forms(pkg, orc, monkeypatch, form, mode):
    R, cols, steps = form
    _force(monkeypatch, R, cols, steps, True)
    rng = np.random.default_rng(7300 + 10 * FORMS.index(form) + mode)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    qs, rs = _pairs(rng, R, cols)
    b = pkg.Aligner.new().matrix(pm).gap_open(5).gap_extend(2)
    [b.global_, b.semi_global, b.local][mode]()
    got = b.build().align_batch(qs, rs)
    name = pkg.lib.pmx_last_kernel().decode()
    assert name.startswith("pmx_long32_kernel%s<%d>/" % ("_c2" if cols == 2 else "", R)), name
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    want = orc.align_batch(mode, qb, qo, rb, ro, 5, 2, om)
    assert (np.stack([got["score"], got["end_query"], got["end_ref"]], axis=1) == want).all(), (form, mode, got, want)
    assert (got["flags"] == 0).all()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("form", FORMS, ids=lambda f: "R%d-c%d-s%d" % f)
def test_checkpoint_forms(pkg, orc, monkeypatch, form, mode):
    R, cols, steps = form
    _force(monkeypatch, R, cols, steps, False)          # (this road takes its rows from band_rows)
    rng = np.random.default_rng(7400 + 10 * FORMS.index(form) + mode)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    qs, rs = _pairs(rng, R, cols)
    flags = 15 if mode == 1 else 0
    got = _run(pkg, mode, flags, pm, 5, 2, qs, rs, 64, 64 * R)
    name = pkg.lib.pmx_last_kernel().decode()
    assert name.startswith("pmx_long32_kernel%s<%d,ck>/" % ("_c2" if cols == 2 else "", R)), name
    _against_oracle(pkg, orc, mode, flags, om, 5, 2, qs, rs, got)
