"""CPU tier of seeding translated references: exported symbols and constants and every refusal that needs no GPU -- wrapped sets whose
pointers are never followed, and the translated index of an empty wrapped set, which is built without GPU work --, each with a
pmx_last_error() text that names the reason; the three index kinds refusing one another's seeding entries by name; and the Python
mirror's argument rules.  Not here: the refusal of a set or index of another device than the current one, which needs two devices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import seed_translated_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_seed_index_build_translated", "pmx_seed_index_strands", "pmx_seed_pairs_translated_ref_device", "pmx_seed_pairs_translated_ref")
CONSTANTS = {"PMX_SEED_REF_FRAMES": 0, "PMX_SEED_REF_CODONS": 1}
T11, T20 = ref.table_of(ref.AA11), ref.table_of(ref.AA20)


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
    assert pkg.SEED_REF_FRAMES == 0 and pkg.SEED_REF_CODONS == 1


def test_index_refusals_and_the_empty_index(pkg):
    L = pkg.lib
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    big = pkg.SeqSet.wrap_device(256, 256, 3, 1 << 30)
    fits = pkg.SeqSet.wrap_device(256, 256, 0, (1 << 30) - 1)
    many = pkg.SeqSet.wrap_device(256, 256, (1 << 29) + 1, 1000)
    build = L.pmx_seed_index_build_translated
    assert not build(None, 4, _ptr(T11), None, 2, None) and "null sequence set" in _err(pkg)
    assert not build(empty.inner, 4, None, None, 2, None) and "null alphabet table" in _err(pkg)
    none = np.full(256, 255, dtype=np.uint8)
    assert not build(empty.inner, 4, _ptr(none), None, 2, None) and "0 group(s)" in _err(pkg) and "2 .. 32" in _err(pkg)
    one = none.copy()
    one[65] = 0
    assert not build(empty.inner, 4, _ptr(one), None, 2, None) and "1 group(s)" in _err(pkg)
    high = T11.copy()
    high[66] = 32
    assert not build(empty.inner, 4, _ptr(high), None, 2, None) and "byte 66 to group 32" in _err(pkg)
    for k, table, bits in ((1, T11, 4), (0, T11, 4), (-3, T20, 5), (16, T11, 4), (13, T20, 5), (63, ref.table_of(["A", "C"]), 1)):
        assert not build(empty.inner, k, _ptr(table), None, 2, None)
        assert "k %d with %d bits per letter is outside k >= 2 and k x bits <= 62" % (k, bits) in _err(pkg)
    for mode in (-1, 3, 100):
        assert not build(empty.inner, 4, _ptr(T11), None, mode, None) and "strand mode %d is outside 0 .. 2" % mode in _err(pkg)
    assert not build(big.inner, 4, _ptr(T11), None, 0, None) and "2^30 - 1 bytes" in _err(pkg) and "parts" in _err(pkg)
    assert not build(many.inner, 4, _ptr(T11), None, 2, None) and "2^29 sequences" in _err(pkg)
    assert L.pmx_seed_index_strands(None) == -1
    code = np.frombuffer(b"F" * 64, dtype=np.uint8).copy()
    for k, table, bits in ((2, T11, 4), (15, T11, 4), (12, T20, 5), (62, ref.table_of(["A", "C"]), 1)):
        for S in (empty, fits):                                                             # no sequence: nothing to index, no GPU work
            for mode in (0, 1, 2):
                ix = build(S.inner, k, _ptr(table), _ptr(code) if mode == 1 else None, mode, None)
                assert ix and L.pmx_seed_index_count(ix) == 0 and L.pmx_seed_index_bits(ix) == bits and L.pmx_seed_index_strands(ix) == mode
                assert L.pmx_seed_index_entries_device(ix, 0, 0, None, None, None, None) == 0
                assert L.pmx_seed_index_entries_device(ix, 0, 1, 256, 256, 256, None) == -1 and "beyond the 0 entries" in _err(pkg)
                L.pmx_seed_index_free(ix)
    for other in (L.pmx_seed_index_build(empty.inner, 12, None), L.pmx_seed_index_build_letters(empty.inner, 4, _ptr(T11), None)):
        assert other and L.pmx_seed_index_strands(other) == -2
        L.pmx_seed_index_free(other)


def test_seeding_refusals_without_gpu(pkg):
    """wrapped sets over addresses that are never followed and empty indexes: every case ends before any GPU work"""
    L = pkg.lib
    Q = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    ix = L.pmx_seed_index_build_translated(empty.inner, 4, _ptr(T11), None, 2, None)
    letters = L.pmx_seed_index_build_letters(empty.inner, 4, _ptr(T11), None)
    dna = L.pmx_seed_index_build(empty.inner, 12, None)
    assert ix and letters and dna
    SO = pkg.pmx_seed_opts_t

    def opts(strand=0, min_seeds=2, band=8, pad=16, max_occ=64, reserved=0, max_hits=0, slice_rows=0):
        return SO(strand, min_seeds, band, pad, max_occ, reserved, max_hits, slice_rows)

    def dev(q=Q.inner, index=ix, first=0, nq=4, mq=50, o=opts(), mode=0, hp=256, hs=256, hd=256, cap=16, off=256, cnt=256):
        return L.pmx_seed_pairs_translated_ref_device(q, index, first, nq, mq, C.byref(o) if o is not None else None, mode, hp, hs, hd, cap,
                                                      off, cnt, None)

    def host(q=Q.inner, index=ix, first=0, nq=4, o=opts(), mode=0, **unused):
        res = C.POINTER(pkg.pmx_seed_hits_t)()
        rc = L.pmx_seed_pairs_translated_ref(q, index, first, nq, C.byref(o) if o is not None else None, mode, C.byref(res))
        if rc == 0:
            r = res.contents
            assert r.n_rows == 0 and r.n_hits == 0 and r.n_passing == 0 and C.cast(r.row_off, C.POINTER(C.c_int64))[0] == 0
            L.pmx_seed_hits_free(res)
        else:
            assert not res
        return rc

    for entry in (dev, host):
        # what pmx_seed_pairs_letters[_device] refuses about the shared arguments, with its texts
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
            assert entry(o=opts(strand=s)) == -1 and "opts->strand %d must be 0 with a translated index" % s in _err(pkg)
        for mode in (-1, 2, 8, 100, -(1 << 31), -(1 << 31) + 2):
            assert entry(mode=mode) == -1 and "ref_mode" in _err(pkg) and "PMX_SEED_REF_CODONS" in _err(pkg)
        assert entry(index=dna) == -1 and "pmx_seed_pairs[_device]" in _err(pkg) and "DNA index" in _err(pkg)
        assert entry(index=letters) == -1 and "pmx_seed_pairs_letters[_device]" in _err(pkg) and "letters index" in _err(pkg)
        kw = {"cnt": None, "off": None} if entry is dev else {}
        for mode in (0, 1):
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
    # the per-row budget: max_qlen x 1 orientation x max_occ x 24 bytes against 256 MiB
    edge = (1 << 28) // (64 * 24)
    for mode in (0, 1):
        assert dev(mq=edge + 1, mode=mode) == -1 and "worst case" in _err(pkg) and "match buffer" in _err(pkg) and "x 1 orientation(s)" in _err(pkg)
        assert dev(mq=edge, mode=mode, nq=0, off=None, cnt=None) == 0
    L.pmx_seed_match_budget(1 << 16)
    try:
        assert dev(mq=43, mode=1) == -1 and "worst case" in _err(pkg) and "65536 bytes" in _err(pkg)          # 43 x 64 x 24 = 66 048
        assert dev(mq=42, mode=1, nq=0, off=None, cnt=None) == 0
    finally:
        L.pmx_seed_match_budget(0)
    # the DNA and letters entries refuse a translated index, with a text that names the new entry
    o = opts(strand=2)
    assert L.pmx_seed_pairs_device(Q.inner, ix, 0, 4, 150, C.byref(o), 256, 256, 256, 16, 256, 256, None) == -1
    assert "pmx_seed_pairs_translated_ref[_device]" in _err(pkg) and "translated index" in _err(pkg)
    res = C.POINTER(pkg.pmx_seed_hits_t)()
    assert L.pmx_seed_pairs(Q.inner, ix, 0, 4, C.byref(o), C.byref(res)) == -1 and "pmx_seed_pairs_translated_ref" in _err(pkg) and not res
    o = opts()
    for mode in (-1, 0, 8, 11):
        assert L.pmx_seed_pairs_letters_device(Q.inner, ix, 0, 4, 50, C.byref(o), mode, None, 256, 256, 256, 16, 256, 256, None) == -1
        assert "pmx_seed_pairs_translated_ref[_device]" in _err(pkg)
        assert L.pmx_seed_pairs_letters(Q.inner, ix, 0, 4, C.byref(o), mode, None, C.byref(res)) == -1 and "pmx_seed_pairs_translated_ref" in _err(pkg)
    assert L.pmx_seed_pairs_translated_ref(Q.inner, ix, 0, 4, C.byref(o), 0, None) == -1 and "null result" in _err(pkg)
    for index in (ix, letters, dna):
        L.pmx_seed_index_free(index)


def test_python_mirror_argument_rules(pkg):
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    dna = pkg.SeedIndex.build(empty, 12)
    letters = pkg.SeedIndex.build(empty, 4, alphabet="aa11")
    assert not dna.translated and dna.strands is None and not letters.translated and letters.strands is None and letters.letters
    for translated in ("forward", "reverse", "both"):
        for alphabet, bits in (("aa20", 5), ("aa11", 4), (ref.table_of(["AC", "DE", "FG"]), 2)):
            ix = pkg.SeedIndex.build(empty, 6, alphabet=alphabet, translated=translated, code=b"F" * 64 if translated == "reverse" else None)
            assert ix.translated and ix.strands == translated and not ix.letters and ix.bits == bits and len(ix) == 0 and ix.k == 6
            assert pkg.lib.pmx_seed_index_strands(ix._handle()) == ("forward", "reverse", "both").index(translated)
            ix.close()
    ix = pkg.SeedIndex.build(empty, 4, alphabet="aa11", translated="both")
    for ref_frames in ("frames", "codons"):
        h = pkg.seed_pairs(S, ix, rows=0, ref_frames=ref_frames)
        assert isinstance(h, pkg.SeedHits) and len(h) == 0 and h.n_rows == 0 and h.row_off.tolist() == [0]
        assert h.strand.dtype == np.uint8 and len(h.strand) == 0 and "reserved" in h.seeds.dtype.names
        if ref_frames == "frames":
            assert h.frame is not None and h.frame.dtype == np.uint8 and len(h.frame) == 0
        else:
            assert h.frame is None
    with pytest.raises(pkg.BatchError, match="translated= needs alphabet="):
        pkg.SeedIndex.build(empty, 12, translated="both")
    with pytest.raises(pkg.BatchError, match="translated is"):
        pkg.SeedIndex.build(empty, 4, alphabet="aa11", translated="all")
    with pytest.raises(pkg.BatchError, match="code= is for a translated index"):
        pkg.SeedIndex.build(empty, 4, alphabet="aa11", code=b"F" * 64)
    with pytest.raises(pkg.BatchError, match="64 letters"):
        pkg.SeedIndex.build(empty, 4, alphabet="aa11", translated="both", code=b"FF")
    with pytest.raises(pkg.BatchError, match="k x bits <= 62"):
        pkg.SeedIndex.build(empty, 16, alphabet="aa11", translated="both")
    with pytest.raises(pkg.BatchError, match="needs ref_frames="):
        pkg.seed_pairs(S, ix, rows=0)
    for bad in ("letters", "all", 0, 3):
        with pytest.raises(pkg.BatchError, match="needs ref_frames="):
            pkg.seed_pairs(S, ix, rows=0, ref_frames=bad)
    for kw in (dict(strand="both"), dict(frames="all"), dict(frames="letters"), dict(strand=0)):
        with pytest.raises(pkg.BatchError, match="ref_frames="):
            pkg.seed_pairs(S, ix, rows=0, ref_frames="frames", **kw)
        with pytest.raises(pkg.BatchError, match="ref_frames="):
            pkg.seed_pairs_device(S, ix, 0, 1, 50, 256, 256, None, 4, 256, 256, **kw)
    with pytest.raises(pkg.BatchError, match="code= belongs to the build"):
        pkg.seed_pairs(S, ix, rows=0, ref_frames="frames", code=b"F" * 64)
    for other, kw in ((dna, {}), (letters, dict(frames="letters"))):
        with pytest.raises(pkg.BatchError, match="ref_frames= is for a translated index"):
            pkg.seed_pairs(S, other, rows=0, ref_frames="frames", **kw)
    with pytest.raises(pkg.BatchError, match="beyond the 3 sequences"):
        pkg.seed_pairs(S, ix, first_row=2, rows=2, ref_frames="codons")
    with pytest.raises(pkg.BatchError, match="max_qlen must be positive"):
        pkg.seed_pairs_device(S, ix, 0, 1, 0, 256, 256, None, 4, 256, 256, ref_frames="frames")
    ix.close()
    with pytest.raises(pkg.BatchError, match="closed"):
        ix.bits
