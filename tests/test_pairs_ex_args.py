"""CPU tier of strands and CIGAR output for the sequence-set batches: exported symbols, pmx_complement_table against the Python
restatement on all 256 bytes, the restatement against itself, and every refusal of pmx_align_pairs_ex[_device] and
pmx_gather_pairs_device that needs no GPU (wrapped sets whose pointers are never followed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_ex_ref
import pairs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_complement_table", "pmx_align_pairs_ex", "pmx_align_pairs_ex_device", "pmx_gather_pairs_device")


def test_symbols_are_exported_and_declared(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name in ("align_pairs_ex_device", "gather_pairs_device", "complement_table"):
        assert callable(getattr(pkg, name)), name


def test_complement_table_equals_the_restatement(pkg):
    got = np.full(256, 0xEE, dtype=np.uint8)
    pkg.lib.pmx_complement_table(got.ctypes.data)
    want = pairs_ex_ref.complement_table()
    assert got.tobytes() == want
    assert pkg.complement_table().tobytes() == want
    pkg.lib.pmx_complement_table(None)                                  # (nothing to write to: nothing happens)


def test_restatement_is_the_documented_table():
    t = pairs_ex_ref.complement_table()
    assert len(t) == 256
    assert bytes(t[c] for c in b"ACGTUMRWSYKVHDBN") == b"TGCAAKYWSRMBDHVN"
    assert bytes(t[c] for c in b"acgtumrwsykvhdbn") == b"tgcaakywsrmbdhvn"
    letters = set(b"ACGTUMRWSYKVHDBNacgtumrwsykvhdbn")
    assert all(t[c] == c for c in range(256) if c not in letters)
    # an involution on everything but U / u (which pair with A like T)
    assert all(t[t[c]] == c for c in range(256) if c not in b"Uu")
    assert pairs_ex_ref.revcomp(b"AACGN-x") == b"x-NCGTT"
    pairs = pairs_ref.pairs_array([(0, 0, 1, 3, 0, -1), (0, 0), (0, 0), (1, 0)])
    got = pairs_ex_ref.resolve([b"AACGT"], [b"TTT"], pairs, [1, 0, 2, 1])
    assert got == [(b"CGT", b"TTT"), (b"AACGT", b"TTT"), None, None]
    assert pairs_ex_ref.resolve([b"AACGT"], [b"TTT"], pairs[:2]) == [(b"ACG", b"TTT"), (b"AACGT", b"TTT")]


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def _cfg(pkg, pm, want=0):
    return pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, want, pm.inner)


def test_refusals_without_gpu(pkg):
    """wrapped sets over addresses that are never followed: every case ends before any GPU work"""
    L = pkg.lib
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    plain, cig = _cfg(pkg, pm), _cfg(pkg, pm, pkg.WANT_CIGAR)
    S = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    h = S.inner
    O = pkg.pmx_pairs_opts_t
    pairs = np.zeros(4, dtype=pkg.PAIR_DTYPE)
    out = np.zeros(64, dtype=pkg.RECORD_DTYPE)
    coff = np.full(5, -7, dtype=np.int64)
    beg = np.zeros(8, dtype=np.int32)
    strand = np.zeros(4, dtype=np.uint8)
    cbuf = C.c_void_p(77)

    def dev(c=plain, q=h, r=h, n=4, p=256, s=None, o=256, st=None, b=None, t=None, cap=0, to=None, opts=None, mq=8, mr=8):
        return L.pmx_align_pairs_ex_device(C.byref(c), q, r, n, p, s, mq, mr, o, st, b, t, cap, to, None,
                                           C.byref(opts) if opts is not None else None)

    def host(c=plain, q=h, r=h, n=4, p=pairs.ctypes.data, s=None, o=out.ctypes.data, st=None, b=None, t=None, to=None, opts=None):
        return L.pmx_align_pairs_ex(C.byref(c), q, r, n, p, s, o, st, b, t, to, C.byref(opts) if opts is not None else None)

    def gather(q=h, r=h, n=4, p=256, s=None, qo=256, qc=100, qf=256, ro=256, rc=100, rf=256, mq=8, mr=8):
        return L.pmx_gather_pairs_device(q, r, n, p, s, mq, mr, qo, qc, qf, ro, rc, rf, None, None)

    for entry in (dev, host):
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(r=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(n=-1) == -1 and "negative n" in _err(pkg)
        assert entry(p=None) == -1 and "null pairs" in _err(pkg)
        assert entry(o=None) == -1 and "null" in _err(pkg)
        assert entry(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, pkg.WANT_STATS)) == -1 and "stats" in _err(pkg)
        assert entry(n=0) == 0
        assert entry(n=0, p=None, o=None) == 0
    # PMX_WANT_CIGAR without text or offset buffers
    assert dev(c=cig) == -1 and "null cigar output" in _err(pkg)
    assert dev(c=cig, t=256) == -1 and "null cigar output" in _err(pkg)
    assert dev(c=cig, to=256) == -1 and "null cigar output" in _err(pkg)
    assert dev(c=cig, t=256, to=256, cap=-1) == -1 and "negative cigar_capacity" in _err(pkg)
    assert host(c=cig) == -1 and "null cigar output" in _err(pkg)
    assert host(c=cig, t=C.byref(cbuf)) == -1 and "null cigar output" in _err(pkg)
    assert host(c=cig, to=coff.ctypes.data) == -1 and "null cigar output" in _err(pkg)
    assert cbuf.value == 77 and (coff == -7).all()                        # nothing was written
    # begins or text buffers without PMX_WANT_CIGAR
    assert dev(b=256) == -1 and "need PMX_WANT_CIGAR" in _err(pkg)
    assert dev(t=256) == -1 and "need PMX_WANT_CIGAR" in _err(pkg)
    assert dev(to=256) == -1 and "need PMX_WANT_CIGAR" in _err(pkg)
    assert host(b=beg.ctypes.data) == -1 and "need PMX_WANT_CIGAR" in _err(pkg)
    assert host(t=C.byref(cbuf)) == -1 and "need PMX_WANT_CIGAR" in _err(pkg)
    assert host(to=coff.ctypes.data) == -1 and "need PMX_WANT_CIGAR" in _err(pkg)
    # CIGAR together with statistics
    both = _cfg(pkg, pm, pkg.WANT_CIGAR | pkg.WANT_STATS)
    st = np.zeros(4, dtype=pkg.STATS_DTYPE)
    assert dev(c=both, st=256, t=256, to=256, cap=10) == -1 and "PMX_WANT_STATS" in _err(pkg)
    assert host(c=both, st=st.ctypes.data, t=C.byref(cbuf), to=coff.ctypes.data) == -1 and "PMX_WANT_STATS" in _err(pkg)
    # a host strand byte of 2: the message names the pair
    strand[2] = 2
    assert host(s=strand.ctypes.data) == -1 and re.search(r"pair 2: strand byte 2\b", _err(pkg))
    strand[1] = 255
    assert host(c=cig, s=strand.ctypes.data, t=C.byref(cbuf), to=coff.ctypes.data) == -1 and re.search(r"pair 1: strand byte 255\b", _err(pkg))
    assert cbuf.value is None and coff[0] == 0                            # (a failed CIGAR call leaves no block behind)
    # the gather
    assert gather(q=None) == -1 and "null sequence set" in _err(pkg)
    assert gather(r=None) == -1 and "null sequence set" in _err(pkg)
    assert gather(n=-1) == -1 and "negative" in _err(pkg)
    assert gather(qc=-1) == -1 and "negative" in _err(pkg)
    assert gather(rc=-5) == -1 and "negative" in _err(pkg)
    assert gather(p=None) == -1 and "null buffer" in _err(pkg)
    assert gather(qo=None) == -1 and "null buffer" in _err(pkg)
    assert gather(rf=None) == -1 and "null buffer" in _err(pkg)
    assert gather(n=0, qf=None) == -1 and "null buffer" in _err(pkg)
    assert gather(mq=0) == -1 and "max_qlen" in _err(pkg)
    assert gather(n=0) == 0
    # the existing entries still have no CIGAR output
    assert L.pmx_align_pairs(C.byref(cig), h, h, 4, pairs.ctypes.data, out.ctypes.data, None, None) == -1 and "CIGAR" in _err(pkg)


def test_python_mirror_checks_its_arguments(pkg):
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    al = pkg.Aligner.new().semi_global().matrix(pm).gap_open(5).gap_extend(2).build()
    with pytest.raises(pkg.BatchError, match="differ in count"):
        al.align_pairs(S, S, [(0, 1), (1, 2)], strand=[1])
    with pytest.raises(pkg.BatchError, match=r"pair 1: strand byte 3\b"):
        al.align_pairs(S, S, [(0, 1), (1, 2)], strand=[1, 3])
    with pytest.raises(pkg.BatchError, match=r"pair 0: strand byte 9\b"):
        al.align_pairs(S, S, [(0, 1), (1, 2)], strand=[9, 0], cigar=True)
    prof = pkg.Aligner.new().local().matrix(pm).profile(pkg.Profile.new(b"ACGT", False, pm)).build()
    with pytest.raises(pkg.BatchError):
        prof.align_pairs(S, S, [(0, 1)], strand=[0], cigar=True)
