"""CPU tier: the encoded PSSM checker (tests/pssm_oracle.py) against the plain square-matrix oracle, and the refusals of the
PSSM batch contract (include/parasail_amd.h), which happen before any GPU work."""
import ctypes as C

import numpy as np
import pytest

from tests.pssm_oracle import check
from tests.util import AA, golden, mutate, random_seqs

SG_SETS = None


def _sg_sets(orc):
    return [orc.SG_ALL, 0, orc.S1_BEG, orc.S1_END, orc.S2_BEG, orc.S2_END, orc.S1_BEG | orc.S2_END, orc.S2_BEG | orc.S1_END,
            orc.S1_BEG | orc.S1_END, orc.S2_BEG | orc.S2_END]


def test_checker_equals_square_oracle_on_derived_pssms(orc):
    """to_pssm(q) of BLOSUM62 through the encoding == BLOSUM62 on q: records, matches / similar / length, CIGAR text"""
    om = orc.Matrix.from_file(golden("blosum62.txt"))
    alpha = np.frombuffer(om.alphabet.encode(), dtype=np.uint8)
    rng = np.random.default_rng(9100)
    cases = [(0, 0)] + [(1, f) for f in _sg_sets(orc)] + [(2, 0)]
    total = 0
    for ci, (mode, sg) in enumerate(cases):
        for _ in range(2):
            L = int(rng.integers(8, 120))
            q = random_seqs(rng, 1, L, L, AA)[0]
            n = 90
            rs = [mutate(rng, q, 0.3, 0.06, AA) if k % 2 else random_seqs(rng, 1, 5, 160, AA)[0] for k in range(n)]
            pssm = om.scores[om.mapper[np.frombuffer(q, dtype=np.uint8)]][:, :om.size]
            got, texts = check(orc, mode, sg, pssm, om.mapper, alpha, [q] * n, rs, 11, 1)
            qb, qo = orc.pack([q] * n); rb, ro = orc.pack(rs)
            want = orc.align_stats_sample(mode, np.arange(n), qb, qo, rb, ro, 11, 1, om, sg_flags=sg, bits=32)
            assert (got == want[:, :6]).all(), (mode, sg, np.nonzero((got != want[:, :6]).any(axis=1))[0][:5])
            wt, _ = orc.cigar_sample(mode, np.arange(n), qb, qo, rb, ro, 11, 1, om, sg_flags=sg)
            assert texts == wt, (mode, sg)
            total += n
    assert total >= 2000


def _cfg(pkg, mode, m, want=0, width=16):
    return pkg.pmx_config_t(mode, pkg.SG_ALL if mode == pkg.MODE_SG else 0, 11, 1, width, want, m.inner)


def test_pssm_batch_refusals(pkg):
    """length mismatch (per-pair, profile, CIGAR), banded and table batches with a PSSM: -1 and a message, no kernel launched"""
    lib = pkg.lib
    before = lib.pmx_last_kernel()
    pm = pkg.Matrix.from_name("blosum62")
    ps = pm.to_pssm(b"MKVLAAGIVG")                       # 10 rows
    rbuf, roff = pkg.pack([b"MKVLAAGIVGL", b"MKV"])
    out = np.zeros(2, dtype=pkg.RECORD_DTYPE)
    # per-pair: one query of another length
    qbuf, qoff = pkg.pack([b"MKVLAAGIVG", b"MKVLAAGIV"])
    for mode in (pkg.MODE_NW, pkg.MODE_SG, pkg.MODE_SW):
        cfg = _cfg(pkg, mode, ps)
        rc = lib.pmx_align_batch(C.byref(cfg), 2, qbuf.ctypes.data, qoff.ctypes.data, rbuf.ctypes.data, roff.ctypes.data,
                                 out.ctypes.data, None)
        assert rc == -1 and b"PSSM length 10 differs" in lib.pmx_last_error(), lib.pmx_last_error()
        cb = C.c_void_p(); co = np.zeros(3, dtype=np.int64)
        rc = lib.pmx_align_batch_cigar(C.byref(cfg), 2, qbuf.ctypes.data, qoff.ctypes.data, rbuf.ctypes.data, roff.ctypes.data,
                                       out.ctypes.data, C.byref(cb), co.ctypes.data)
        assert rc == -1 and b"PSSM length 10 differs" in lib.pmx_last_error(), lib.pmx_last_error()
    # profile of another length
    prof = pkg.Profile.new(b"MKVLAAGIV", False, ps)
    cfg = _cfg(pkg, pkg.MODE_SW, ps)
    rc = lib.pmx_align_profile_batch(C.byref(cfg), prof.inner, 2, rbuf.ctypes.data, roff.ctypes.data, out.ctypes.data, None)
    assert rc == -1 and b"PSSM length 10 differs" in lib.pmx_last_error()
    dummy = np.zeros(64, dtype=np.int64); p = dummy.ctypes.data
    rc = lib.pmx_align_profile_batch_device(C.byref(cfg), prof.inner, 2, p, p, 16, p, None, None)
    assert rc == -1 and b"PSSM length 10 differs" in lib.pmx_last_error()
    rc = lib.pmx_align_batch_device(C.byref(cfg), 2, p, p, p, p, 9, 16, p, None, None)
    assert rc == -1 and b"PSSM length 10 differs" in lib.pmx_last_error()
    # banded and table batches stay out of scope
    qbuf, qoff = pkg.pack([b"MKVLAAGIVG", b"MKVLAAGIVG"])
    rc = lib.pmx_align_batch_banded(C.byref(cfg), None, 2, qbuf.ctypes.data, qoff.ctypes.data, rbuf.ctypes.data, roff.ctypes.data,
                                    8, None, out.ctypes.data)
    assert rc == -1 and b"PSSM" in lib.pmx_last_error() and b"single-pair only" not in lib.pmx_last_error()
    rc = lib.pmx_align_batch_banded_device(C.byref(cfg), 2, p, p, p, p, 10, 16, 8, None, p, None)
    assert rc == -1 and b"PSSM" in lib.pmx_last_error() and b"banded" in lib.pmx_last_error()
    rc = lib.pmx_align_batch_table_device(C.byref(cfg), 2, p, p, p, p, 10, 16, p, p, None, None, p, None)
    assert rc == -1 and b"PSSM" in lib.pmx_last_error() and b"table" in lib.pmx_last_error()
    assert lib.pmx_last_kernel() == before
