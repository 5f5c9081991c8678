"""CPU tier of the reference-side frameshift traceback entries (pmx_align_pairs_frameshift_ref_cigar[_device]): symbols, the unit rule,
every refusal that needs no GPU (wrapped sets whose pointers are never followed) with its pmx_last_error() text, the Python mirror, and
the model the GPU tests compare against (tests/swfsc_trace_model.c) held against the score model, the invariants of the contract, and
a path enumerator without DP."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frameshift_ref_side as fr
import frameshift_trace_ref_side as ft
from util import golden, AA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_align_pairs_frameshift_ref_cigar_device", "pmx_align_pairs_frameshift_ref_cigar", "pmx_swfsc_trace_bytes_per_slot")


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_symbols_and_unit_rule(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    assert hasattr(pkg, "align_pairs_frameshift_ref_cigar_device") and hasattr(pkg.Aligner, "align_pairs_frameshift_ref_cigar")
    assert "Frameshift traceback, reference side" in text
    assert "CONSUME THREE REFERENCE NUCLEOTIDES" in text  # the unit rule, said in capitals
    assert "CONSUME ONE QUERY LETTER" in text
    # the hook is the layout's arithmetic: strips x (columns + 15 steps of skew) x 192 bytes
    S = pkg.lib.pmx_swfsc_strip_rows()
    for mq, mr in ((1, 1), (S, 8), (S + 1, 8), (2 * S + 1, 301), (4096, 100000)):
        assert pkg.lib.pmx_swfsc_trace_bytes_per_slot(mq, mr) == -(-mq // S) * (mr + 15) * 192


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

    def adev(c=cfg, q=s, r=t, n=4, p=256, sb=None, mode=BOTH, f=15, mq=8, mr=8, o=256, so=256, ds=None, db=256, tx=256, tc=64, to=256, opts=None):
        return L.pmx_align_pairs_frameshift_ref_cigar_device(C.byref(c), q, r, n, p, sb, mode, f, None, mq, mr, o, so, ds, db, tx, tc, to, None,
                                                             C.byref(opts) if opts is not None else None)

    def ahost(c=cfg, q=s, r=t, n=4, p=pairs.ctypes.data, sb=None, mode=BOTH, f=15, o=out.ctypes.data, so=won.ctypes.data, ds=None,
              db=beg.ctypes.data, tx=C.byref(buf), to=off.ctypes.data, opts=None, **_):
        if ds == 256:
            ds = st.ctypes.data
        return L.pmx_align_pairs_frameshift_ref_cigar(C.byref(c), q, r, n, p, sb, mode, f, None, o, so, ds, db, tx, to,
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
    # the score entry of this side keeps refusing the traceback's outputs
    assert L.pmx_align_pairs_frameshift_ref_device(C.byref(cfg), s, t, 4, 256, None, BOTH, 15, None, 8, 8, 256, 256, None, None) == -1
    assert "PMX_WANT_CIGAR" in _err(pkg)
    # four slots of trace against the bound, from the hook: one byte under refuses, naming the switch and both figures
    four = 4 * L.pmx_swfsc_trace_bytes_per_slot(8, 8)
    assert four == 4 * (8 + 15) * 192
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(four - 1))
    assert adev() == -1 and "PMX_CIGAR_CHUNK_BYTES" in _err(pkg) and str(four - 1) in _err(pkg) and str(four) in _err(pkg)
    # exactly four slots pass the bound: the next check speaks (max_rlen 0 is refused behind the bound, and nothing reaches the GPU)
    four0 = 4 * L.pmx_swfsc_trace_bytes_per_slot(8, 0)
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(four0 - 1))
    assert adev(mr=0) == -1 and "PMX_CIGAR_CHUNK_BYTES" in _err(pkg)
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(four0))
    assert adev(mr=0) == -1 and "max_qlen / max_rlen must be positive" in _err(pkg)
    # a long reference traces every cell: 4 096 letters x 100 kb is refused by the default bound
    monkeypatch.delenv("PMX_CIGAR_CHUNK_BYTES")
    assert adev(mq=4096, mr=100000) == -1 and "exceed the bound" in _err(pkg)


def test_python_mirror(pkg):
    pm = pkg.Matrix.from_name("blosum62")
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    for strand in (0, 1, "both", "forward", "reverse", None):
        rec, cig, beg, won = al.align_pairs_frameshift_ref_cigar(S, S, [], 15, ref_strand=strand)
        assert len(rec) == 0 and cig == [] and beg.shape == (0, 2) and won.dtype == np.uint8
    rec, cig, beg, won = al.align_pairs_frameshift_ref_cigar(S, S, [], 15, ref_strand=np.zeros(0, dtype=np.uint8))
    assert len(rec) == 0 and cig == []
    rec, cig, beg, won, st = al.align_pairs_frameshift_ref_cigar(S, S, [], 15, stats=True)
    assert len(st) == 0
    with pytest.raises(pkg.BatchError, match="frameshift penalty"):
        al.align_pairs_frameshift_ref_cigar(S, S, [], -1)
    with pytest.raises(pkg.BatchError, match="differ in count"):
        al.align_pairs_frameshift_ref_cigar(S, S, [(0, 1)], 3, ref_strand=[0, 1])
    with pytest.raises(TypeError):
        al.align_pairs_frameshift_ref_cigar(S, S, [], 3, ref_frame=0)    # no frame argument: the strands are the frames' carriers
    with pytest.raises(pkg.BatchError, match="ref_frameshift excludes cigar"):      # align_pairs keeps refusing
        al.align_pairs(S, S, [], ref_frameshift=3, cigar=True)
    prof = pkg.Aligner.new().local().matrix(pm).profile(pkg.Profile.new(b"ACDEF", False, pm)).build()
    with pytest.raises(pkg.BatchError, match="takes no profile"):
        prof.align_pairs_frameshift_ref_cigar(S, S, [], 15)


# ------------------------------------------------------------------------------------------------------------------- the model
def _check_invariants(q, T, rec, text, beg, stats, score, open_, ext, f):
    """the invariants of the contract, from the text alone"""
    if rec[0] == 0:
        assert text == "" and beg == [rec[1] + 1, rec[2] + 1] == [1, 3] and stats == [0, 0, 0]
        return None
    runs = ft.parse(text)
    assert runs[0][1] in "=X" and runs[-1][1] in "=X"
    for (c0, o0), (c1, o1) in zip(runs, runs[1:]):
        assert o0 != o1
        if o0 in "/\\":
            assert c0 == 1 and o1 in "=X"
    c = ft.counts(text)
    assert rec[1] - beg[0] + 1 == c["m"] + c[ft.QUERY_GAP]
    assert rec[2] - beg[1] + 1 == 3 * (c["m"] + c[ft.CODON_GAP]) - c[ft.SHORT] + c[ft.LONG]
    assert list(ft.rescore(text, beg, q, T, score, open_, ext, f)) == rec[:3]
    similar = sum(score(q[row], T[col]) > 0 for op, _, row, col, _ in ft.steps(text, beg) if op in "=X")
    assert stats == [sum(n for n, o in runs if o == "="), similar, c["m"] + c[ft.QUERY_GAP] + c[ft.CODON_GAP]]
    assert len(runs) <= len(q) + len(T)
    return c


def _b62_score(orc):
    b62 = orc.Matrix.from_file(golden("blosum62.txt"))
    score = lambda a, b: int(b62.scores[b62.mapper[a], b62.mapper[b]])
    score.same = lambda a, b: b62.mapper[a] == b62.mapper[b]
    return b62, score


def test_model_against_score_model_and_invariants(orc):
    """a random lattice: every record equals tests/swfsc_model.c's byte for byte, every text holds the invariants, and each of the
    five op kinds is seen at least 100 times"""
    b62, score = _b62_score(orc)
    rng = np.random.default_rng(19000)
    seen = {"m": 0, ft.QUERY_GAP: 0, ft.CODON_GAP: 0, ft.SHORT: 0, ft.LONG: 0}
    positive = 0
    small = AA[:5]                                         # few letters: many ties, many positive scores
    for k in range(1500):
        m, N = int(rng.integers(1, 13)), int(rng.integers(1, 39))
        open_, ext = ((11, 1), (2, 1), (1, 1), (3, 3))[k % 4]
        f = (0, 1, 3, 15)[(k // 4) % 4]
        alpha = small if k % 3 else AA
        q = alpha[rng.integers(0, len(alpha), m)].tobytes(); T = alpha[rng.integers(0, len(alpha), N)].tobytes()
        rec, text, beg, stats = ft.align(q, T, b62, open_, ext, f)
        assert rec == fr.align(q, T, b62, open_, ext, f)
        c = _check_invariants(q, T, rec, text, beg, stats, score, open_, ext, f)
        if c:
            positive += 1
            for key in seen:
                seen[key] += c[key]
    assert positive > 1200 and all(v >= 100 for v in seen.values()), seen


def test_model_pairs_and_strands(orc):
    """the pair form, all three strand modes: the strand fold of the score model, byte for byte, and the winner's text on the winner's
    stream"""
    b62, score = _b62_score(orc)
    rng = np.random.default_rng(19100)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    won = set()
    for k in range(300):
        w = dna[rng.integers(0, 4, int(rng.integers(1, 60)))].tobytes()
        q = AA[rng.integers(0, len(AA), int(rng.integers(1, 12)))].tobytes()
        for mode in (0, 1, 2):
            rec, strand, text, beg, stats = ft.pair(q, w, mode, b62, 2, 1, 3)
            want = fr.pair(q, w, mode, b62, 2, 1, 3)
            assert (rec, strand) == want
            if len(w) < 3:
                assert rec == ft.BAD and text == "" and beg == [-1, -1] and stats == [0, 0, 0] and strand == 0
                continue
            _check_invariants(q, fr.stream(w, strand), rec, text, beg, stats, score, 2, 1, 3)
            if mode == 2:
                won.add(strand)
    assert won == {0, 1}


def test_model_against_brute_force(orc):
    """every m <= 4 and N <= 8: the re-scored text equals the best path found by enumeration"""
    om = orc.Matrix.create("ACDE", 3, -2)
    letters = np.frombuffer(b"ACDE", dtype=np.uint8)
    score = lambda a, b: int(om.scores[om.mapper[a], om.mapper[b]])
    rng = np.random.default_rng(19200)
    shifted = gapped = 0
    for m in range(1, 5):
        for N in range(1, 9):
            for open_, ext, f in ((3, 1, 2), (1, 1, 0), (1, 3, 1), (5, 2, 7)):
                for _ in range(8):
                    q = letters[rng.integers(0, 4, m)].tobytes(); T = letters[rng.integers(0, 4, N)].tobytes()
                    rec, text, beg, stats = ft.align(q, T, om, open_, ext, f)
                    assert ft.rescore(text, beg, q, T, score, open_, ext, f)[0] == rec[0] == fr.brute(q, T, score, open_, ext, f), (q, T, open_, ext, f)
                    _check_invariants(q, T, rec, text, beg, stats, score, open_, ext, f)
                    shifted += "/" in text or "\\" in text
                    gapped += "I" in text or "D" in text
    assert shifted >= 20 and gapped >= 20


def test_model_without_frameshifts(orc):
    """fs = 2^20: no text contains a frameshift op, and begin and end lie in one frame"""
    b62, _ = _b62_score(orc)
    rng = np.random.default_rng(19300)
    small = AA[:6]
    texts = 0
    for k in range(300):
        q = small[rng.integers(0, 6, int(rng.integers(1, 15)))].tobytes(); T = small[rng.integers(0, 6, int(rng.integers(1, 60)))].tobytes()
        rec, text, beg, stats = ft.align(q, T, b62, 2, 1, 1 << 20)
        assert "/" not in text and "\\" not in text
        if text:
            texts += 1
            assert (rec[2] - 2 - beg[1]) % 3 == 0
    assert texts > 250
