"""CPU tier of the translated set entries (pmx_*_translated[_device]): the exported genetic code against a codon dictionary written
out amino acid by amino acid, translate() on hand-written cases, the host model against it, constants and struct layouts, and every
refusal that needs no GPU (wrapped sets whose pointers are never followed), each with its pmx_last_error() text."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import translate_ref as ref
from test_set_search_args import _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_genetic_code_table", "pmx_gather_pairs_translated_device", "pmx_align_pairs_translated_device", "pmx_align_pairs_translated",
           "pmx_search_pairs_translated_device", "pmx_search_pairs_translated", "pmx_frame_hits_free",
           "pmx_search_topk_translated_device", "pmx_search_topk_translated", "pmx_topk_frame_hits_free")

# the standard code, amino acid by amino acid (NCBI table 1)
CODONS = {
    "A": "GCT GCC GCA GCG", "R": "CGT CGC CGA CGG AGA AGG", "N": "AAT AAC", "D": "GAT GAC", "C": "TGT TGC", "Q": "CAA CAG",
    "E": "GAA GAG", "G": "GGT GGC GGA GGG", "H": "CAT CAC", "I": "ATT ATC ATA", "L": "TTA TTG CTT CTC CTA CTG", "K": "AAA AAG",
    "M": "ATG", "F": "TTT TTC", "P": "CCT CCC CCA CCG", "S": "TCT TCC TCA TCG AGT AGC", "T": "ACT ACC ACA ACG", "W": "TGG",
    "Y": "TAT TAC", "V": "GTT GTC GTA GTG", "*": "TAA TAG TGA"}


def _header():
    return open(os.path.join(ROOT, "include", "parasail_amd.h")).read()


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_symbols_constants_and_layouts(pkg):
    text = _header()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name, value in (("FORWARD", 6), ("REVERSE", 7), ("ALL", 8)):
        assert re.search(r"#define PMX_FRAMES_%s\s+%d\b" % (name, value), text)
        assert getattr(pkg, "FRAMES_" + name) == getattr(ref, "FRAMES_" + name) == value
    for name in ("gather_pairs_translated_device", "align_pairs_translated_device", "search_pairs_translated_device",
                 "search_topk_translated_device", "genetic_code_table", "translate"):
        assert hasattr(pkg, name), name
    for struct, ctype, like in (("pmx_frame_hits", pkg.pmx_frame_hits_t, "pmx_strand_hits"),
                                ("pmx_topk_frame_hits", pkg.pmx_topk_frame_hits_t, "pmx_topk_strand_hits")):
        fields, size = _layout(text, struct, struct + "_t")
        lfields, lsize = _layout(text, like, like + "_t")                    # laid out like the stranded blocks, `frame` for `strand`
        assert size == lsize == C.sizeof(ctype) and fields[:-1] == lfields[:-1]
        assert fields[-1][0] == "frame" and fields[-1][1:] == lfields[-1][1:]
        for name, o, sz in fields:
            assert getattr(ctype, name).offset == o and getattr(ctype, name).size == sz, name
    assert _layout(text, "pmx_pairs_opts", "pmx_pairs_opts_t")[1] == 8 == C.sizeof(pkg.pmx_pairs_opts_t)      # the option structs are untouched
    assert _layout(text, "pmx_pair_search_opts", "pmx_pair_search_opts_t")[1] == 32
    assert _layout(text, "pmx_topk_opts", "pmx_topk_opts_t")[1] == 32


def test_code_table_is_the_standard_code(pkg):
    table = pkg.genetic_code_table()
    assert table == ref.CODE_STD == b"FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
    index = {c: i for i, c in enumerate("TCAG")}
    seen = {}
    for aa, codons in CODONS.items():
        for codon in codons.split():
            assert codon not in seen
            seen[codon] = aa
            assert chr(table[16 * index[codon[0]] + 4 * index[codon[1]] + index[codon[2]]]) == aa, codon
    assert len(seen) == 64
    count = {aa: len(c.split()) for aa, c in CODONS.items()}
    assert count["L"] == count["S"] == count["R"] == 6 and count["*"] == 3 and count["M"] == count["W"] == 1
    assert [table.count(aa.encode()) for aa in "LSR*MW"] == [6, 6, 6, 3, 1, 1]
    pkg.lib.pmx_genetic_code_table(None)                                     # (NULL is ignored)


TEN = b"ATGGCCTAAN"          # reverse complement: NTTAGGCCAT
HAND = [
    (TEN, 0, b"MA*"), (TEN, 1, b"WPX"), (TEN, 2, b"GL"), (TEN, 3, b"XRP"), (TEN, 4, b"LGH"), (TEN, 5, b"*A"),
    (b"atggcctaan", 0, b"MA*"), (b"atggcctaan", 4, b"LGH"),                 # lower case, upper-case letters out
    (b"AUGUUUuaa", 0, b"MF*"), (b"UUUCAU", 3, b"MK"),                       # U reads as T; its complement is A
    (b"ATNGCC", 0, b"XA"), (b"AT-GCC", 0, b"XA"), (b"GGCNAT", 3, b"XA"),    # a byte that is no base: X, on either strand
    (b"AT", 0, b""), (b"AT", 1, b""), (b"AT", 3, b""), (b"AT", 5, b""),     # W = 2: no frame
    (b"ATG", 0, b"M"), (b"ATG", 1, b""), (b"ATG", 2, b""), (b"ATG", 3, b"H"), (b"ATG", 4, b""),
    (b"ATGG", 0, b"M"), (b"ATGG", 1, b"W"), (b"ATGG", 2, b""), (b"ATGG", 3, b"P"), (b"ATGG", 4, b"H"), (b"ATGG", 5, b""),
    (b"ATGGC", 0, b"M"), (b"ATGGC", 1, b"W"), (b"ATGGC", 2, b"G"), (b"ATGGC", 3, b"A"), (b"ATGGC", 4, b"P"), (b"ATGGC", 5, b"H"),
]


def test_translate_hand_written_cases(pkg):
    for seq, frame, want in HAND:
        assert pkg.translate(seq, frame) == want, (seq, frame)
        assert ref.translate(seq, frame) == want, (seq, frame)
        assert ref.tlen(len(seq), frame) == len(want)
    with pytest.raises(pkg.BatchError, match="outside 0 .. 5"):
        pkg.translate(TEN, 6)
    other = bytes(ref.CODE_STD[:14]) + b"W" + bytes(ref.CODE_STD[15:])      # a caller's code: TGA reads W
    assert pkg.translate(b"ATGTGATAA", 0, code=other) == b"MW*" == ref.translate(b"ATGTGATAA", 0, other)
    with pytest.raises(pkg.BatchError, match="64 letters"):
        pkg.translate(TEN, 0, code=b"ACGT")


def test_model_and_helper_agree_on_random_windows(pkg):
    rng = np.random.default_rng(13000)
    letters = np.frombuffer(b"ACGTacgtUuNn-RY", dtype=np.uint8)
    for _ in range(300):
        w = letters[rng.integers(0, len(letters), size=int(rng.integers(0, 40)))].tobytes()
        for f in range(6):
            assert pkg.translate(w, f) == ref.translate(w, f)
    # the positions map: a letter read back from the stored bytes it names
    seq = letters[rng.integers(0, 8, size=50)].tobytes()
    comp = pkg.complement_table()
    for q_beg, w in ((0, 50), (3, 40), (7, 11)):
        for f in range(6):
            t = ref.translate(seq[q_beg:q_beg + w], f)
            for p in range(len(t)):
                at = ref.stored_bytes(q_beg, w, f, p)
                codon = bytes(seq[x] if f < 3 else int(comp[seq[x]]) for x in at)
                assert ref.translate(codon, 0) == t[p:p + 1] and all(q_beg <= x < q_beg + w for x in at)


def test_fold_rule_of_the_model():
    rng = np.random.default_rng(13100)
    n = 2000
    recs = rng.integers(-3, 4, size=(6, n, 4)).astype(np.int32)
    stats = rng.integers(0, 50, size=(6, n, 3)).astype(np.int32)
    exists = rng.random((6, n)) < 0.7
    exists[:, :20] = False
    rec, st, won = ref.fold(recs, exists, stats)
    assert (rec[:20] == (0, -1, -1, 8)).all() and not won[:20].any() and not st[:20].any()
    for k in range(20, n):
        cand = [f for f in range(6) if exists[f, k]]
        if not cand:
            assert rec[k].tolist() == [0, -1, -1, 8] and won[k] == 0
            continue
        top = max(int(recs[f, k, 0]) for f in cand)
        first = min(f for f in cand if int(recs[f, k, 0]) == top)             # a tie: the lowest frame
        assert won[k] == first and rec[k].tolist() == recs[first, k].tolist() and st[k].tolist() == stats[first, k].tolist()
    r3, _, w3 = ref.fold(recs[3:], exists[3:], frames=(3, 4, 5))
    assert set(w3[exists[3:].any(axis=0)].tolist()) <= {3, 4, 5}


def _cfg(pkg, pm, want=0):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, want, pm.inner)


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
    TRI, RECT, LIST = pkg.PAIRS_TRIANGLE, pkg.PAIRS_RECT, pkg.PAIRS_LIST
    ALL = pkg.FRAMES_ALL
    pairs = np.zeros(4, dtype=pkg.PAIR_DTYPE)
    out = np.zeros((4, 4), dtype=np.int32)
    won = np.zeros(4, dtype=np.uint8)
    route = ("CIGAR", "pmx_gather_pairs_translated_device", "pmx_align_batch_cigar_device")

    def refuses_cigar(rc):
        return rc == -1 and all(word in _err(pkg) for word in route)

    # ---- listed pairs
    def adev(c=cfg, q=s, r=t, n=4, p=256, fr=None, mode=ALL, mq=8, mr=8, o=256, st=None, fo=256, opts=None):
        return L.pmx_align_pairs_translated_device(C.byref(c), q, r, n, p, fr, mode, None, mq, mr, o, st, fo, None,
                                                   C.byref(opts) if opts is not None else None)

    def ahost(c=cfg, q=s, r=t, n=4, p=pairs.ctypes.data, fr=None, mode=ALL, o=out.ctypes.data, st=None, fo=won.ctypes.data, opts=None, **_):
        return L.pmx_align_pairs_translated(C.byref(c), q, r, n, p, fr, mode, None, o, st, fo, C.byref(opts) if opts is not None else None)

    for entry in (adev, ahost):
        for mode in (-1, 9, 255):
            assert entry(mode=mode) == -1 and "frame mode %d is outside 0 .. 8" % mode in _err(pkg)
        assert entry(fr=256 if entry is adev else won.ctypes.data, mode=2) == -1 and "frame byte per pair takes frame mode 0" in _err(pkg)
        assert entry(fo=None) == -1 and "null frame output" in _err(pkg)
        assert entry(fo=None, mode=4, n=0) == 0                                             # (optional in a single-frame mode)
        assert refuses_cigar(entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR)))
        assert entry(c=_cfg(pkg, pssm)) == -1 and "PSSM" in _err(pkg) and "translated query" in _err(pkg)
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(n=-1) == -1 and "negative n" in _err(pkg)
        assert entry(p=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(o=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(7, 0, 11, 1, 0, 0, pm.inner)) == -1 and "mode" in _err(pkg)
        assert entry(n=0, fo=None) == 0                                                     # n == 0 touches nothing
    assert adev(c=_cfg(pkg, pm, pkg.WANT_STATS)) == -1 and "stats requested without a stats buffer" in _err(pkg)
    assert adev(mq=0) == -1 and "max_qlen" in _err(pkg)
    bad = np.array([0, 5, 6, 1], dtype=np.uint8)
    assert ahost(fr=bad.ctypes.data, mode=0) == -1 and "pair 2: frame byte 6 is outside 0 .. 5" in _err(pkg)

    # ---- the gather hook
    def gdev(q=s, r=t, n=4, p=256, mq=8, mr=8, qo=256, qc=64, qf=256, ro=256, rc=64, rf=256):
        return L.pmx_gather_pairs_translated_device(q, r, n, p, None, None, mq, mr, qo, qc, qf, ro, rc, rf, None, None)
    assert gdev(q=None) == -1 and "null sequence set" in _err(pkg)
    assert gdev(n=-1) == -1 and "negative n or capacity" in _err(pkg)
    assert gdev(qc=-1) == -1 and "negative n or capacity" in _err(pkg)
    assert gdev(qf=None) == -1 and "null buffer" in _err(pkg)
    assert gdev(p=None) == -1 and "null buffer" in _err(pkg)
    assert gdev(mq=0) == -1 and "max_qlen" in _err(pkg)
    assert gdev(n=0, p=None, qo=None, ro=None) == 0

    # ---- set search
    def sdev(c=cfg, q=s, r=t, shape=RECT, first=0, n=4, p=None, mq=8, mr=8, ms=0, hp=256, hi=256, hr=256, hs=None, cap=16, cnt=256, opts=None,
             mode=ALL, hb=256):
        return L.pmx_search_pairs_translated_device(C.byref(c), q, r, shape, first, n, p, mq, mr, ms, hp, hi, hr, hs, cap, cnt, None,
                                                    C.byref(opts) if opts is not None else None, mode, None, hb)

    def shost(c=cfg, q=s, r=t, shape=RECT, first=0, n=4, p=None, max_hits=0, chunk=0, sl=0, mode=ALL, **_):
        res = C.POINTER(pkg.pmx_frame_hits_t)()
        o = pkg.pmx_pair_search_opts_t(0, shape, max_hits, chunk, sl)
        rc = L.pmx_search_pairs_translated(C.byref(c), q, r, first, n, p, C.byref(o), mode, None, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_passing == 0 and res.contents.frame
            L.pmx_frame_hits_free(res)
        else:
            assert not res
        return rc

    for entry in (sdev, shost):
        for mode in (-1, 9):
            assert entry(mode=mode) == -1 and "frame mode %d is outside 0 .. 8" % mode in _err(pkg)
        for mode in (0, 4, pkg.FRAMES_FORWARD, pkg.FRAMES_REVERSE, ALL):
            assert entry(c=_cfg(pkg, pssm), mode=mode) == -1 and "PSSM" in _err(pkg) and "translated query" in _err(pkg)
            assert refuses_cigar(entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR), mode=mode))
            assert entry(shape=3, mode=mode) == -1 and "unknown pair shape 3" in _err(pkg)
            assert entry(shape=TRI, r=t, mode=mode) == -1 and "R must be NULL or Q" in _err(pkg)
            assert entry(shape=RECT, r=None, mode=mode) == -1 and "null sequence set" in _err(pkg)
            assert entry(shape=LIST, r=t, p=None, mode=mode) == -1 and "null pairs" in _err(pkg)
            assert entry(shape=RECT, r=t, first=67, n=4, mode=mode) == -1 and "beyond the 70 pairs of 10 x 7" in _err(pkg)
            assert entry(n=-1, mode=mode) == -1 and "negative" in _err(pkg)
            kw = {"cnt": None} if entry is sdev else {}
            assert entry(n=0, mode=mode, **kw) == 0
    assert sdev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    assert sdev(hr=None) == -1 and "null hit records" in _err(pkg)
    assert sdev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert sdev(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
    assert sdev(hs=256) == -1 and "stats buffer without PMX_WANT_STATS" in _err(pkg)
    assert sdev(mq=0) == -1 and "max_qlen" in _err(pkg)
    assert sdev(hb=None, hp=None, hi=None, n=0, cnt=None) == 0                              # (optional outputs)
    assert shost(max_hits=-1) == -1 and "max_hits" in _err(pkg)
    assert shost(sl=-1) == -1 and "slice_pairs" in _err(pkg)
    o = pkg.pmx_pair_search_opts_t(0, RECT, 0, 0, 0)
    assert L.pmx_search_pairs_translated(C.byref(cfg), s, t, 0, 4, None, C.byref(o), ALL, None, None) == -1 and "null result" in _err(pkg)
    L.pmx_frame_hits_free(None)

    # ---- top-K
    def tdev(c=cfg, q=s, r=t, qf=0, nq=4, mq=8, mr=8, ms=0, k=3, skip=0, hp=256, hi=256, hr=256, hs=None, cap=16, off=256, rp=256, cnt=256, opts=None,
             mode=ALL, hb=256):
        return L.pmx_search_topk_translated_device(C.byref(c), q, r, qf, nq, mq, mr, ms, k, skip, hp, hi, hr, hs, cap, off, rp, cnt, None,
                                                   C.byref(opts) if opts is not None else None, mode, None, hb)

    def thost(c=cfg, q=s, r=t, qf=0, nq=4, k=3, skip=0, chunk=0, sl=0, mode=ALL, **_):
        res = C.POINTER(pkg.pmx_topk_frame_hits_t)()
        o = pkg.pmx_topk_opts_t(0, k, skip, chunk, sl)
        rc = L.pmx_search_topk_translated(C.byref(c), q, r, qf, nq, C.byref(o), mode, None, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_rows == 0 and res.contents.frame
            L.pmx_topk_frame_hits_free(res)
        else:
            assert not res
        return rc

    for entry in (tdev, thost):
        for mode in (-1, 9):
            assert entry(mode=mode) == -1 and "frame mode %d is outside 0 .. 8" % mode in _err(pkg)
        for mode in (3, ALL):
            assert entry(c=_cfg(pkg, pssm), mode=mode) == -1 and "PSSM" in _err(pkg) and "translated query" in _err(pkg)
            assert refuses_cigar(entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR), mode=mode))
            assert entry(k=0, mode=mode) == -1 and "k 0 is outside 1 .. 1024" in _err(pkg)
            assert entry(k=1025, mode=mode) == -1 and "k 1025 is outside" in _err(pkg)
            assert entry(skip=1, mode=mode) == -1 and "skip_self needs R to be Q" in _err(pkg)
            assert entry(qf=8, nq=3, mode=mode) == -1 and "beyond the 10 sequences" in _err(pkg)
            assert entry(nq=-1, mode=mode) == -1 and "negative" in _err(pkg)
            kw = {"cnt": None, "off": None} if entry is tdev else {}
            assert entry(nq=0, mode=mode, **kw) == 0
    assert tdev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    assert tdev(hr=None) == -1 and "null hit records" in _err(pkg)
    assert tdev(off=None) == -1 and "null row offsets" in _err(pkg)
    assert tdev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert tdev(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
    assert thost(sl=-1) == -1 and "slice_rows" in _err(pkg)
    L.pmx_topk_frame_hits_free(None)


def test_python_mirror_defaults_and_refusals(pkg):
    pm = pkg.Matrix.from_name("blosum62")
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    for frame in (0, 5, "forward", "reverse", "all", pkg.FRAMES_ALL):
        h = al.search_pairs(S, S, min_score=5, count=0, frame=frame)
        assert isinstance(h, pkg.PairHits) and len(h) == 0 and h.frame.dtype == np.uint8 and len(h.frame) == 0
        t = al.search_topk(S, S, k=2, rows=0, frame=frame)
        assert isinstance(t, pkg.TopKHits) and len(t) == 0 and t.frame.dtype == np.uint8 and len(t.frame) == 0
    rec, won = al.align_pairs(S, S, [], frame="all")
    assert len(rec) == 0 and won.dtype == np.uint8 and len(won) == 0
    with pytest.raises(pkg.BatchError, match="frame mode 11"):
        al.search_pairs(S, S, frame=11)
    with pytest.raises(pkg.BatchError, match="frame mode 9"):
        al.search_topk(S, S, frame=9)
    with pytest.raises(pkg.BatchError, match="all"):
        al.search_pairs(S, S, frame="sideways")
    for call in (lambda: al.search_pairs(S, S, frame=0, strand="both"), lambda: al.search_topk(S, S, frame="all", strand=1),
                 lambda: al.align_pairs(S, S, [(0, 1)], frame=2, strand=[0]), lambda: al.align_pairs(S, S, [(0, 1)], frame="all", strand="both")):
        with pytest.raises(pkg.BatchError, match="frame and strand exclude each other"):
            call()
    with pytest.raises(pkg.BatchError, match="differ in count"):
        al.align_pairs(S, S, [(0, 1)], frame=[0, 1])
    with pytest.raises(pkg.BatchError, match="one frame mode"):
        al.search_pairs(S, S, frame=[0, 1])
    with pytest.raises(pkg.BatchError, match="pmx_gather_pairs_translated_device"):
        al.align_pairs(S, S, [], frame=0, cigar=True)
    h = al.search_pairs(S, S, min_score=5, count=0)                                      # frame=None: today's path, no frames
    assert len(h.frame) == 0 and len(h.strand) == 0
