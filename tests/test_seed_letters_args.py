"""CPU tier of protein seeding: exported symbols and constants, the built-in alphabets, every refusal that needs no GPU -- wrapped sets
whose pointers are never followed, and the letters index of an empty wrapped set, which is built without GPU work --, each with a
pmx_last_error() text that names the reason, and the Python mirror's argument rules.  Not here: the refusal of a set or index of
another device than the current one, which needs two devices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import seed_letters_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_seed_alphabet", "pmx_seed_index_build_letters", "pmx_seed_index_bits", "pmx_seed_pairs_letters_device",
           "pmx_seed_pairs_letters")
CONSTANTS = {"PMX_SEED_ALPHABET_AA20": 0, "PMX_SEED_ALPHABET_AA11": 1, "PMX_SEED_QUERY_LETTERS": -1, "PMX_SEED_CODONS_FORWARD": 9,
             "PMX_SEED_CODONS_REVERSE": 10, "PMX_SEED_CODONS_BOTH": 11}


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def _ptr(table):
    return table.ctypes.data_as(C.c_void_p)


def test_symbols_and_constants(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name, value in CONSTANTS.items():
        m = re.search(r"#define %s\s+\(?(-?\d+)\)?" % name, text)
        assert m and int(m.group(1)) == value, name
    for name, value in (("SEED_ALPHABET_AA20", 0), ("SEED_ALPHABET_AA11", 1), ("SEED_QUERY_LETTERS", -1), ("SEED_CODONS_FORWARD", 9),
                        ("SEED_CODONS_REVERSE", 10), ("SEED_CODONS_BOTH", 11)):
        assert getattr(pkg, name) == value
    assert hasattr(pkg, "seed_alphabet")


def test_builtin_alphabets(pkg):
    for which, name, groups in ((0, "aa20", ref.AA20), (1, "aa11", ref.AA11)):
        t = np.zeros(256, dtype=np.uint8)
        assert pkg.lib.pmx_seed_alphabet(which, _ptr(t)) == 0
        assert t.tobytes() == ref.table_of(groups).tobytes()
        assert pkg.seed_alphabet(name).tobytes() == t.tobytes() == pkg.seed_alphabet(which).tobytes()
        assert all(t[ord(c)] == 255 for c in "*XBZxbz")
    t = np.zeros(256, dtype=np.uint8)
    assert pkg.lib.pmx_seed_alphabet(2, _ptr(t)) == -1 and "alphabet 2" in _err(pkg)
    assert pkg.lib.pmx_seed_alphabet(0, None) == -1 and "null table" in _err(pkg)
    with pytest.raises(pkg.BatchError, match="aa20"):
        pkg.seed_alphabet("dna")


def test_index_refusals_bits_and_the_empty_index(pkg):
    L = pkg.lib
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    big = pkg.SeqSet.wrap_device(256, 256, 3, 1 << 29)
    fits = pkg.SeqSet.wrap_device(256, 256, 0, (1 << 29) - 1)
    many = pkg.SeqSet.wrap_device(256, 256, 1 << 31, 1000)
    t11, t20 = ref.table_of(ref.AA11), ref.table_of(ref.AA20)
    build = L.pmx_seed_index_build_letters
    assert not build(None, 4, _ptr(t11), None) and "null sequence set" in _err(pkg)
    assert not build(empty.inner, 4, None, None) and "null alphabet table" in _err(pkg)
    none = np.full(256, 255, dtype=np.uint8)
    assert not build(empty.inner, 4, _ptr(none), None) and "0 group(s)" in _err(pkg) and "2 .. 32" in _err(pkg)
    one = none.copy()
    one[65] = 0
    assert not build(empty.inner, 4, _ptr(one), None) and "1 group(s)" in _err(pkg)
    high = t11.copy()
    high[66] = 32
    assert not build(empty.inner, 4, _ptr(high), None) and "byte 66 to group 32" in _err(pkg)
    for k, table, bits in ((1, t11, 4), (0, t11, 4), (-3, t20, 5), (16, t11, 4), (13, t20, 5), (63, ref.table_of(["A", "C"]), 1)):
        assert not build(empty.inner, k, _ptr(table), None)
        assert "k %d with %d bits per letter is outside k >= 2 and k x bits <= 62" % (k, bits) in _err(pkg)
    assert not build(big.inner, 4, _ptr(t11), None) and "2^29 - 1 bytes" in _err(pkg) and "parts" in _err(pkg)
    assert not build(many.inner, 4, _ptr(t11), None) and "2^31 - 1 sequences" in _err(pkg)
    assert L.pmx_seed_index_bits(None) == -1
    cases = ((2, t11, 4), (15, t11, 4), (12, t20, 5), (62, ref.table_of(["A", "C"]), 1), (31, ref.table_of(["AC", "DE"]), 1),
             (20, ref.table_of(list("ACDEFGHI")), 3))
    for k, table, bits in cases:
        for S in (empty, fits):                                                             # no sequence: nothing to index, no GPU work
            ix = build(S.inner, k, _ptr(table), None)
            assert ix and L.pmx_seed_index_count(ix) == 0 and L.pmx_seed_index_bits(ix) == bits
            assert L.pmx_seed_index_entries_device(ix, 0, 0, None, None, None, None) == 0
            assert L.pmx_seed_index_entries_device(ix, 0, 1, 256, 256, 256, None) == -1 and "beyond the 0 entries" in _err(pkg)
            L.pmx_seed_index_free(ix)
    dna = L.pmx_seed_index_build(empty.inner, 12, None)
    assert L.pmx_seed_index_bits(dna) == 2
    L.pmx_seed_index_free(dna)


def test_seeding_refusals_without_gpu(pkg):
    """wrapped sets over addresses that are never followed and empty indexes: every case ends before any GPU work"""
    L = pkg.lib
    Q = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    t11 = ref.table_of(ref.AA11)
    ix = L.pmx_seed_index_build_letters(empty.inner, 4, _ptr(t11), None)
    dna = L.pmx_seed_index_build(empty.inner, 12, None)
    assert ix and dna
    SO = pkg.pmx_seed_opts_t

    def opts(strand=0, min_seeds=2, band=8, pad=16, max_occ=64, reserved=0, max_hits=0, slice_rows=0):
        return SO(strand, min_seeds, band, pad, max_occ, reserved, max_hits, slice_rows)

    def dev(q=Q.inner, index=ix, first=0, nq=4, mq=50, o=opts(), mode=8, hp=256, hs=256, hd=256, cap=16, off=256, cnt=256):
        return L.pmx_seed_pairs_letters_device(q, index, first, nq, mq, C.byref(o) if o is not None else None, mode, None, hp, hs, hd, cap,
                                               off, cnt, None)

    def host(q=Q.inner, index=ix, first=0, nq=4, o=opts(), mode=8, **unused):
        res = C.POINTER(pkg.pmx_seed_hits_t)()
        rc = L.pmx_seed_pairs_letters(q, index, first, nq, C.byref(o) if o is not None else None, mode, None, C.byref(res))
        if rc == 0:
            r = res.contents
            assert r.n_rows == 0 and r.n_hits == 0 and r.n_passing == 0 and C.cast(r.row_off, C.POINTER(C.c_int64))[0] == 0
            L.pmx_seed_hits_free(res)
        else:
            assert not res
        return rc

    for entry in (dev, host):
        # what pmx_seed_pairs[_device] refuses, with its texts
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(index=None) == -1 and "null seed index" in _err(pkg)
        assert entry(o=None) == -1 and "null opts" in _err(pkg)
        assert entry(first=-1) == -1 and "negative q_first or nq" in _err(pkg)
        assert entry(nq=-1) == -1 and "negative q_first or nq" in _err(pkg)
        assert entry(o=opts(max_hits=-1)) == -1 and "max_hits" in _err(pkg)
        assert entry(o=opts(slice_rows=-1)) == -1 and "slice_rows" in _err(pkg)
        assert entry(first=8, nq=3) == -1 and "beyond the 10 sequences" in _err(pkg)
        assert entry(first=11, nq=0) == -1 and "beyond" in _err(pkg)
        assert entry(o=opts(min_seeds=0)) == -1 and "min_seeds 0 is below 1" in _err(pkg)
        for bad in (-1, (1 << 20) + 1):
            assert entry(o=opts(band=bad)) == -1 and "band %d is outside 0 .. 2^20" % bad in _err(pkg)
            assert entry(o=opts(pad=bad)) == -1 and "pad %d is outside 0 .. 2^20" % bad in _err(pkg)
        for bad in (0, -5, 65536):
            assert entry(o=opts(max_occ=bad)) == -1 and "max_occ %d is outside 1 .. 65535" % bad in _err(pkg)
        assert entry(o=opts(reserved=1)) == -1 and "reserved must be 0" in _err(pkg)
        # its own
        for s in (1, 2, -1):
            assert entry(o=opts(strand=s)) == -1 and "opts->strand %d must be 0" % s in _err(pkg)
        for mode in (-2, 12, 100, -(1 << 31)):
            assert entry(mode=mode) == -1 and "query mode" in _err(pkg) and "PMX_SEED_CODONS_FORWARD" in _err(pkg)
        assert entry(index=dna) == -1 and "pmx_seed_pairs[_device]" in _err(pkg) and "DNA index" in _err(pkg)
        kw = {"cnt": None, "off": None} if entry is dev else {}
        for mode in (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11):
            assert entry(nq=0, mode=mode, **kw) == 0
        assert entry(first=10, nq=0, **kw) == 0
    # the device entry's own
    assert dev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    for mq in (0, -3):
        assert dev(mq=mq) == -1 and "max_qlen must be positive" in _err(pkg)
    assert dev(hp=None) == -1 and "null hit pairs or strand bytes" in _err(pkg)
    assert dev(hs=None) == -1 and "null hit pairs or strand bytes" in _err(pkg)
    assert dev(off=None) == -1 and "null row offsets" in _err(pkg)
    assert dev(cnt=None) == -1 and "null counts" in _err(pkg)
    # the per-row budget: max_qlen x orientations x max_occ x 24 bytes against 256 MiB, with 1 / 3 / 6 orientations
    edge = (1 << 28) // (64 * 24)                                                           # 174762 positions of one orientation fit
    for mode, orients in ((-1, 1), (4, 1), (6, 3), (7, 3), (9, 3), (10, 3), (8, 6), (11, 6)):
        assert dev(mq=edge // orients + 1, mode=mode) == -1 and "worst case" in _err(pkg) and "match buffer" in _err(pkg)
        assert "x %d orientation(s)" % orients in _err(pkg)
        assert dev(mq=edge // orients, mode=mode, nq=0, off=None, cnt=None) == 0
    was = L.pmx_seed_match_budget(1 << 16)
    try:
        assert dev(mq=8, mode=8) == -1 and "worst case" in _err(pkg) and "65536 bytes" in _err(pkg)          # 8 x 6 x 64 x 24 = 73 728
        assert dev(mq=7, mode=8, nq=0, off=None, cnt=None) == 0
    finally:
        L.pmx_seed_match_budget(0)
    # the one new refusal of the DNA entries: a letters index, with a text that names the new entry
    o = opts(strand=2)
    assert L.pmx_seed_pairs_device(Q.inner, ix, 0, 4, 150, C.byref(o), 256, 256, 256, 16, 256, 256, None) == -1
    assert "pmx_seed_pairs_letters" in _err(pkg)
    res = C.POINTER(pkg.pmx_seed_hits_t)()
    assert L.pmx_seed_pairs(Q.inner, ix, 0, 4, C.byref(o), C.byref(res)) == -1 and "pmx_seed_pairs_letters" in _err(pkg) and not res
    o = opts()
    assert L.pmx_seed_pairs_letters(Q.inner, ix, 0, 4, C.byref(o), 8, None, None) == -1 and "null result" in _err(pkg)
    L.pmx_seed_index_free(ix)
    L.pmx_seed_index_free(dna)


def test_python_mirror_argument_rules(pkg):
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    dna = pkg.SeedIndex.build(empty, 12)
    assert not dna.letters and dna.bits == 2
    old = pkg.SeedIndex.build(empty, 12, 0)                                                  # (R, k, stream): the call from before alphabets
    assert not old.letters and old.bits == 2 and len(old) == 0
    for alphabet, bits in (("aa20", 5), ("aa11", 4), (ref.table_of(["AC", "DE", "FG"]), 2), (ref.table_of(["A", "C"]).tobytes(), 1)):
        ix = pkg.SeedIndex.build(empty, 6, alphabet=alphabet)
        assert ix.letters and ix.bits == bits and len(ix) == 0 and ix.k == 6
        ix.close()
    ix = pkg.SeedIndex.build(empty, 4, alphabet="aa11")
    frame_modes = (0, 5, "forward", "reverse", "all")
    for frames in ("letters",) + frame_modes + ("codons", "codons-reverse", "codons-both"):
        h = pkg.seed_pairs(S, ix, rows=0, frames=frames)
        assert isinstance(h, pkg.SeedHits) and len(h) == 0 and h.n_rows == 0 and h.row_off.tolist() == [0]
        assert h.strand.dtype == np.uint8 and len(h.strand) == 0
        if frames in frame_modes:
            assert h.frame is not None and h.frame.dtype == np.uint8 and len(h.frame) == 0
        else:
            assert h.frame is None
    assert pkg.seed_pairs(S, dna, rows=0).frame is None
    with pytest.raises(pkg.BatchError, match="needs frames="):
        pkg.seed_pairs(S, ix, rows=0)
    with pytest.raises(pkg.BatchError, match="frames= is for a letters index"):
        pkg.seed_pairs(S, dna, rows=0, frames="all")
    with pytest.raises(pkg.BatchError, match="strand= is for a DNA index"):
        pkg.seed_pairs(S, ix, rows=0, frames="all", strand="both")
    with pytest.raises(pkg.BatchError, match="code= is for a letters index"):
        pkg.seed_pairs(S, dna, rows=0, code=b"F" * 64)
    for bad in ("sideways", 6, -1, 9):
        with pytest.raises(pkg.BatchError, match="frames is"):
            pkg.seed_pairs(S, ix, rows=0, frames=bad)
    with pytest.raises(pkg.BatchError, match="64 letters"):
        pkg.seed_pairs(S, ix, rows=0, frames=0, code=b"FF")
    pkg.seed_pairs(S, ix, rows=0, frames=0, code=b"F" * 64)
    with pytest.raises(pkg.BatchError, match="beyond the 3 sequences"):
        pkg.seed_pairs(S, ix, first_row=2, rows=2, frames="codons")
    with pytest.raises(pkg.BatchError, match="max_qlen must be positive"):
        pkg.seed_pairs_device(S, ix, 0, 1, 0, 256, 256, None, 4, 256, 256, frames="all")
    with pytest.raises(pkg.BatchError, match="needs frames="):
        pkg.seed_pairs_device(S, ix, 0, 1, 50, 256, 256, None, 4, 256, 256)
    with pytest.raises(pkg.BatchError, match="256 bytes"):
        pkg.SeedIndex.build(empty, 4, alphabet=np.zeros(20, dtype=np.uint8))
    with pytest.raises(pkg.BatchError, match="aa20"):
        pkg.SeedIndex.build(empty, 4, alphabet="blosum")
    with pytest.raises(pkg.BatchError, match="k x bits <= 62"):
        pkg.SeedIndex.build(empty, 16, alphabet="aa11")
    ix.close()
    with pytest.raises(pkg.BatchError, match="closed"):
        ix.bits
