"""CPU tier of the frameshift-aware entries (pmx_*_frameshift[_device], pmx_gather_pairs_codons_device): symbols and constants, every
refusal that needs no GPU (wrapped sets whose pointers are never followed) with its pmx_last_error() text, and the model the GPU
tests compare against (tests/swfs_model.c) held against a path enumerator without DP, against the oracle's plain local score over the
three host-translated frames, and against translate()."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frameshift_ref as fs
import translate_ref
from util import golden, AA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_frameshift_max_window", "pmx_gather_pairs_codons_device", "pmx_align_pairs_frameshift_device", "pmx_align_pairs_frameshift",
           "pmx_search_pairs_frameshift_device", "pmx_search_pairs_frameshift", "pmx_search_topk_frameshift_device", "pmx_search_topk_frameshift")


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_symbols_and_constants(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    cap = int(re.search(r"#define PMX_FRAMESHIFT_MAX_WINDOW\s+(\d+)\b", text).group(1))
    assert cap >= 2048 and pkg.lib.pmx_frameshift_max_window() == cap == pkg.frameshift_max_window()
    for name in ("codon_stream", "gather_pairs_codons_device", "align_pairs_frameshift_device", "search_pairs_frameshift_device",
                 "search_topk_frameshift_device"):
        assert hasattr(pkg, name), name
    assert "IN NUCLEOTIDES" in text                       # the record's unit, said in capitals


def _cfg(pkg, pm, mode=None, width=0, want=0):
    return pkg.pmx_config_t(pkg.MODE_SW if mode is None else mode, 0, 11, 1, width, want, pm.inner)


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
    RECT, TRI, LIST = pkg.PAIRS_RECT, pkg.PAIRS_TRIANGLE, pkg.PAIRS_LIST
    BOTH = pkg.STRAND_BOTH
    cap = L.pmx_frameshift_max_window()
    pairs = np.zeros(4, dtype=pkg.PAIR_DTYPE)
    out = np.zeros((4, 4), dtype=np.int32)
    won = np.zeros(4, dtype=np.uint8)

    def adev(c=cfg, q=s, r=t, n=4, p=256, sb=None, mode=BOTH, f=15, mq=8, mr=8, o=256, so=256, opts=None):
        return L.pmx_align_pairs_frameshift_device(C.byref(c), q, r, n, p, sb, mode, f, None, mq, mr, o, so, None,
                                                   C.byref(opts) if opts is not None else None)

    def ahost(c=cfg, q=s, r=t, n=4, p=pairs.ctypes.data, sb=None, mode=BOTH, f=15, o=out.ctypes.data, so=won.ctypes.data, opts=None, **_):
        return L.pmx_align_pairs_frameshift(C.byref(c), q, r, n, p, sb, mode, f, None, o, so, C.byref(opts) if opts is not None else None)

    def sdev(c=cfg, q=s, r=t, shape=RECT, first=0, n=4, p=None, mq=8, mr=8, ms=0, hp=256, hi=256, hr=256, hs=None, cap=16, cnt=256, opts=None,
             mode=BOTH, hb=256, f=15):
        return L.pmx_search_pairs_frameshift_device(C.byref(c), q, r, shape, first, n, p, mq, mr, ms, hp, hi, hr, hs, cap, cnt, None,
                                                    C.byref(opts) if opts is not None else None, mode, hb, f, None)

    def shost(c=cfg, q=s, r=t, shape=RECT, first=0, n=4, p=None, max_hits=0, chunk=0, sl=0, mode=BOTH, f=15, **_):
        res = C.POINTER(pkg.pmx_strand_hits_t)()
        o = pkg.pmx_pair_search_opts_t(0, shape, max_hits, chunk, sl)
        rc = L.pmx_search_pairs_frameshift(C.byref(c), q, r, first, n, p, C.byref(o), mode, f, None, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_passing == 0 and res.contents.strand
            L.pmx_strand_hits_free(res)
        else:
            assert not res
        return rc

    def tdev(c=cfg, q=s, r=t, qf=0, nq=4, mq=8, mr=8, ms=0, k=3, skip=0, hp=256, hi=256, hr=256, hs=None, cap=16, off=256, rp=256, cnt=256, opts=None,
             mode=BOTH, hb=256, f=15):
        return L.pmx_search_topk_frameshift_device(C.byref(c), q, r, qf, nq, mq, mr, ms, k, skip, hp, hi, hr, hs, cap, off, rp, cnt, None,
                                                   C.byref(opts) if opts is not None else None, mode, hb, f, None)

    def thost(c=cfg, q=s, r=t, qf=0, nq=4, k=3, skip=0, chunk=0, sl=0, mode=BOTH, f=15, **_):
        res = C.POINTER(pkg.pmx_topk_strand_hits_t)()
        o = pkg.pmx_topk_opts_t(0, k, skip, chunk, sl)
        rc = L.pmx_search_topk_frameshift(C.byref(c), q, r, qf, nq, C.byref(o), mode, f, None, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_rows == 0 and res.contents.strand
            L.pmx_topk_strand_hits_free(res)
        else:
            assert not res
        return rc

    # what section 1 of the contract refuses, at every entry
    for entry in (adev, ahost, sdev, shost, tdev, thost):
        for mode in (pkg.MODE_NW, pkg.MODE_SG):
            assert entry(c=_cfg(pkg, pm, mode=mode)) == -1 and "PMX_MODE_SW" in _err(pkg)
        for width in (8, 16, 64):
            assert entry(c=_cfg(pkg, pm, width=width)) == -1 and "width %d is neither 0 nor 32" % width in _err(pkg)
        assert entry(c=_cfg(pkg, pm, width=3)) == -1 and "bad width" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, want=pkg.WANT_STATS)) == -1 and "PMX_WANT_STATS" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, want=pkg.WANT_CIGAR)) == -1 and "PMX_WANT_CIGAR" in _err(pkg)
        assert entry(c=_cfg(pkg, pssm)) == -1 and "PSSM" in _err(pkg)
        assert entry(f=-1) == -1 and "frameshift penalty" in _err(pkg)
        for mode in (-1, 3, 255):
            assert entry(mode=mode) == -1 and "strand mode %d is outside 0 .. 2" % mode in _err(pkg)
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(7, 0, 11, 1, 0, 0, pm.inner)) == -1 and "mode" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(pkg.MODE_SW, 0, -1, 1, 0, 0, pm.inner)) == -1 and "gap penalties" in _err(pkg)
    for entry in (adev, sdev, tdev):                                           # max_qlen bounds N = W - 2
        assert entry(mq=cap - 1) == -1 and "PMX_FRAMESHIFT_MAX_WINDOW" in _err(pkg)
        assert entry(mq=0) == -1 and "max_qlen" in _err(pkg)
        assert entry(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
    # listed pairs
    for entry in (adev, ahost):
        assert entry(sb=256 if entry is adev else won.ctypes.data, mode=BOTH) == -1 and "strand byte per pair takes strand mode PMX_STRAND_FORWARD" in _err(pkg)
        assert entry(so=None) == -1 and "null strand output" in _err(pkg)
        assert entry(so=None, mode=1, n=0) == 0                                # (optional with one strand)
        assert entry(n=-1) == -1 and "negative n" in _err(pkg)
        assert entry(p=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(o=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(n=0, so=None) == 0
    bad = np.array([0, 1, 2, 1], dtype=np.uint8)
    assert ahost(sb=bad.ctypes.data, mode=0) == -1 and "pair 2: strand byte 2 is neither 0 nor 1" in _err(pkg)
    # the gather hook
    def gdev(q=s, r=t, n=4, p=256, mq=8, mr=8, qo=256, qc=64, qf=256, ro=256, rc=64, rf=256):
        return L.pmx_gather_pairs_codons_device(q, r, n, p, None, None, mq, mr, qo, qc, qf, ro, rc, rf, None, None)
    assert gdev(q=None) == -1 and "null sequence set" in _err(pkg)
    assert gdev(n=-1) == -1 and "negative n or capacity" in _err(pkg)
    assert gdev(qf=None) == -1 and "null buffer" in _err(pkg)
    assert gdev(mq=0) == -1 and "max_qlen" in _err(pkg)
    assert gdev(n=0, p=None, qo=None, ro=None) == 0
    # set search and top-K: what the stranded entries refuse, with their texts
    for entry in (sdev, shost):
        assert entry(shape=3) == -1 and "unknown pair shape 3" in _err(pkg)
        assert entry(shape=TRI, r=t) == -1 and "R must be NULL or Q" in _err(pkg)
        assert entry(shape=LIST, r=t, p=None) == -1 and "null pairs" in _err(pkg)
        assert entry(shape=RECT, r=t, first=67, n=4) == -1 and "beyond the 70 pairs of 10 x 7" in _err(pkg)
        assert entry(n=0, **({"cnt": None} if entry is sdev else {})) == 0
    assert sdev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    assert sdev(hr=None) == -1 and "null hit records" in _err(pkg)
    assert sdev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert sdev(hs=256) == -1 and "stats buffer without PMX_WANT_STATS" in _err(pkg)
    assert shost(max_hits=-1) == -1 and "max_hits" in _err(pkg)
    for entry in (tdev, thost):
        assert entry(k=0) == -1 and "k 0 is outside 1 .. 1024" in _err(pkg)
        assert entry(skip=1) == -1 and "skip_self needs R to be Q" in _err(pkg)
        assert entry(qf=8, nq=3) == -1 and "beyond the 10 sequences" in _err(pkg)
        assert entry(nq=0, **({"cnt": None, "off": None} if entry is tdev else {})) == 0
    assert tdev(off=None) == -1 and "null row offsets" in _err(pkg)
    assert thost(sl=-1) == -1 and "slice_rows" in _err(pkg)


def test_python_mirror(pkg):
    pm = pkg.Matrix.from_name("blosum62")
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    for strand in (0, 1, "both"):
        h = al.search_pairs(S, S, min_score=5, count=0, frameshift=15, strand=strand)
        assert isinstance(h, pkg.PairHits) and len(h) == 0 and h.strand.dtype == np.uint8
        t = al.search_topk(S, S, k=2, rows=0, frameshift=15, strand=strand)
        assert isinstance(t, pkg.TopKHits) and len(t) == 0
    rec, won = al.align_pairs(S, S, [], frameshift=15, strand="both")
    assert len(rec) == 0 and won.dtype == np.uint8
    for call in (lambda: al.align_pairs(S, S, [], frameshift=15, frame=0), lambda: al.align_pairs(S, S, [], frameshift=15, ref_frame="all"),
                 lambda: al.search_pairs(S, S, frameshift=15, frame="all"), lambda: al.search_pairs(S, S, frameshift=15, ref_frame=1),
                 lambda: al.search_topk(S, S, frameshift=15, frame=2), lambda: al.search_topk(S, S, frameshift=15, ref_frame="forward")):
        with pytest.raises(pkg.BatchError, match="frameshift excludes frame and ref_frame"):
            call()
    with pytest.raises(pkg.BatchError, match="frameshift penalty"):
        al.search_pairs(S, S, frameshift=-2)
    with pytest.raises(pkg.BatchError, match="differ in count"):
        al.align_pairs(S, S, [(0, 1)], frameshift=3, strand=[0, 1])
    with pytest.raises(pkg.BatchError, match="PMX_WANT_CIGAR"):
        al.align_pairs(S, S, [], frameshift=3, cigar=True)
    with pytest.raises(pkg.BatchError, match="neither 0 nor 1"):
        pkg.codon_stream(b"ACGT", 2)


def test_model_against_brute_force(orc):
    """every N <= 8 and m <= 4, random letters of a 4-letter alphabet, four (open, extend, fs) triples: the recurrence equals the
    enumeration of all paths.  Match 3 / mismatch -2 with penalties from 0 up, so that gaps and frameshifts are on best paths."""
    om = orc.Matrix.create("ACDE", 3, -2)
    letters = np.frombuffer(b"ACDE", dtype=np.uint8)
    score = lambda a, b: int(om.scores[om.mapper[a], om.mapper[b]])
    rng = np.random.default_rng(15000)
    used_shift = used_gap = 0
    for N in range(1, 9):
        for m in range(1, 5):
            for open_, ext, f in ((3, 1, 2), (1, 1, 0), (1, 3, 1), (5, 2, 7)):
                for _ in range(8):
                    T = letters[rng.integers(0, 4, N)].tobytes(); r = letters[rng.integers(0, 4, m)].tobytes()
                    got = fs.align(T, r, om, open_, ext, f)
                    assert got[0] == fs.brute(T, r, score, open_, ext, f), (T, r, open_, ext, f)
                    assert got[3] == 0 and 2 <= got[1] < N + 2 and 0 <= got[2] < m
                    used_shift += got[0] > fs.align(T, r, om, open_, ext, 1 << 20)[0]
                    used_gap += got[0] > fs.align(T, r, om, 1 << 20, 1 << 20, f)[0]
    assert used_shift >= 5 and used_gap >= 5               # no vacuous pass: frameshifts and gaps lie on best paths
    # the tie rule: the first maximum in column-major order; a zero maximum ends at (2, 0)
    assert fs.align(b"EEEE", b"AA", om, 3, 1, 2) == [0, 2, 0, 0]
    assert fs.align(b"CACA", b"A", om, 3, 1, 2) == [3, 3, 0, 0]           # rows 1 and 3 of column 0 tie: the smaller row
    assert fs.align(b"AEEE", b"EA", om, 3, 1, 2) == [3, 3, 0, 0]          # (1, 0), (2, 0), (3, 0) and (0, 1) tie: the smaller column first


def test_model_against_the_oracle_and_translate(pkg, orc):
    """frameshift 2^20: no path changes frame, and the score is the best plain local score over the three host-translated frames
    of the strand; the stream's rows f, f + 3, .. are translate()'s frame"""
    b62 = orc.Matrix.from_file(golden("blosum62.txt"))
    rng = np.random.default_rng(15100)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    for k in range(120):
        w = dna[rng.integers(0, 4, int(rng.integers(3, 201)))].tobytes()
        r = AA[rng.integers(0, len(AA), int(rng.integers(1, 80)))].tobytes()
        for strand in (0, 1):
            T = fs.codon_stream(w, strand)
            assert T == pkg.codon_stream(w, strand) and len(T) == len(w) - 2
            frames = [x for x in (T[f::3] for f in range(3)) if x]
            qb, qo = orc.pack(frames); rb, ro = orc.pack([r] * len(frames))
            want = int(orc.align_batch(orc.SW, qb, qo, rb, ro, 11, 1, b62)[:, 0].max())
            assert fs.align(T, r, b62, 11, 1, 1 << 20)[0] == want == fs.align(T, r, b62, 11, 1, 0, no_shift=True)[0]
    mixed = np.frombuffer(b"ACGTacgtUuNn-RY", dtype=np.uint8)
    for k in range(200):
        w = mixed[rng.integers(0, len(mixed), int(rng.integers(0, 40)))].tobytes()
        for f in range(6):
            assert pkg.codon_stream(w, f // 3)[f % 3::3] == pkg.translate(w, f) == translate_ref.translate(w, f)
            assert fs.codon_stream(w, f // 3)[f % 3::3] == translate_ref.translate(w, f)
    other = bytes(translate_ref.CODE_STD[:14]) + b"W" + bytes(translate_ref.CODE_STD[15:])
    assert pkg.codon_stream(b"ATGTGATAA", 0, code=other)[0::3] == b"MW*" == fs.codon_stream(b"ATGTGATAA", 0, other)[0::3]
    assert pkg.codon_stream(b"AT") == b"" == fs.codon_stream(b"AT") and pkg.codon_stream(b"atg", 1) == b"H"
