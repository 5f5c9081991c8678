"""CPU tier of minimizer seeding: exported symbols, every refusal of pmx_seed_index_build_minimizers and pmx_seed_sketch[_device] with
its pmx_last_error() text -- over wrapped sets whose pointers are never followed, so every call ends before any GPU work --, NULL
handles, the empty set's index, the Python mirror's refusals, and the plan: with w = 1 every number of the probe is what
pmx_seed_plan_probe says, with w > 1 a position slot costs one byte more and the slice shrinks with it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_seed_index_build_minimizers", "pmx_seed_index_window", "pmx_seed_index_bytes", "pmx_seed_sketch", "pmx_seed_sketch_device",
           "pmx_seed_sketch_shape", "pmx_seed_mix", "pmx_seed_rows_max_len", "pmx_seed_plan_probe_w")


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_symbols_are_exported_and_declared(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name in ("seed_minimizers", "seed_minimizers_device", "seed_sketch_shape", "seed_mix"):
        assert hasattr(pkg, name), name
    row_tile, set_tile = pkg.seed_sketch_shape()
    assert row_tile >= 64 and set_tile >= 64 and row_tile % 64 == 0 and set_tile % 64 == 0


def test_build_refusals_null_handles_and_the_empty_set(pkg):
    L = pkg.lib
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    big = pkg.SeqSet.wrap_device(256, 256, 3, 1 << 31)
    many = pkg.SeqSet.wrap_device(256, 256, 1 << 31, 1000)
    assert not L.pmx_seed_index_build_minimizers(None, 12, 5, None) and "null sequence set" in _err(pkg)
    for k in (7, 32, 0, -1):
        assert not L.pmx_seed_index_build_minimizers(empty.inner, k, 5, None) and "k %d is outside 8 .. 31" % k in _err(pkg)
    for w in (0, 65, -1, 1 << 20):
        assert not L.pmx_seed_index_build_minimizers(empty.inner, 12, w, None) and "w %d is outside 1 .. 64" % w in _err(pkg)
    assert not L.pmx_seed_index_build_minimizers(big.inner, 12, 5, None) and "2^31 - 1 bytes" in _err(pkg)
    assert not L.pmx_seed_index_build_minimizers(many.inner, 12, 5, None) and "2^31 - 1 bytes and sequences" in _err(pkg)
    assert L.pmx_seed_index_window(None) == -1 and L.pmx_seed_index_bytes(None) == -1
    for k, w in ((8, 1), (31, 64), (15, 10)):
        ix = L.pmx_seed_index_build_minimizers(empty.inner, k, w, None)                      # nothing to index: no GPU work
        assert ix and L.pmx_seed_index_count(ix) == 0 and L.pmx_seed_index_window(ix) == w and L.pmx_seed_index_bytes(ix) == 0
        assert L.pmx_seed_index_bits(ix) == 2 and L.pmx_seed_index_strands(ix) == -2
        assert L.pmx_seed_index_entries_device(ix, 0, 0, None, None, None, None) == 0
        L.pmx_seed_index_free(ix)
    ix = L.pmx_seed_index_build(empty.inner, 12, None)                                       # every other build: w = 1
    assert L.pmx_seed_index_window(ix) == 1 and L.pmx_seed_index_bytes(ix) == 0
    L.pmx_seed_index_free(ix)
    table = pkg.seed_alphabet("aa11")
    ix = L.pmx_seed_index_build_letters(empty.inner, 5, table.ctypes.data, None)
    assert L.pmx_seed_index_window(ix) == 1 and L.pmx_seed_index_bytes(ix) == 0
    L.pmx_seed_index_free(ix)


def test_seeding_with_an_empty_minimizer_index_needs_no_gpu(pkg):
    """the entries take a minimizer index as it is: their refusals are unchanged, and no rows is a success"""
    L = pkg.lib
    Q = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    ix = L.pmx_seed_index_build_minimizers(empty.inner, 12, 10, None)
    o = pkg.pmx_seed_opts_t(2, 2, 8, 16, 64, 0, 0, 0)
    assert L.pmx_seed_pairs_device(Q.inner, ix, 0, 0, 150, C.byref(o), None, None, None, 0, None, None, None) == 0
    assert L.pmx_seed_pairs_device(Q.inner, ix, 0, 4, 0, C.byref(o), 256, 256, 256, 4, 256, 256, None) == -1 and "max_qlen must be positive" in _err(pkg)
    assert L.pmx_seed_pairs_device(Q.inner, ix, 0, 4, (1 << 28) // (2 * 64 * 24) + 1, C.byref(o), 256, 256, 256, 4, 256, 256, None) == -1
    assert "worst case" in _err(pkg) and "x 24 bytes per match" in _err(pkg)               # the row budget rule is the plain index's
    assert L.pmx_seed_pairs_letters_device(Q.inner, ix, 0, 0, 150, C.byref(o), -1, None, None, None, None, 0, None, None, None) == -1
    assert "a DNA index" in _err(pkg)
    L.pmx_seed_index_free(ix)


def test_sketch_refusals_without_gpu(pkg):
    L = pkg.lib
    Q = pkg.SeqSet.wrap_device(256, 256, 10, 1000)

    def dev(q=Q.inner, first=0, nq=4, mq=150, k=15, w=10, mode=2, flags=256):
        return L.pmx_seed_sketch_device(q, first, nq, mq, k, w, mode, flags, None)

    def host(q=Q.inner, first=0, nq=4, mq=150, k=15, w=10, mode=2, flags=256):
        return L.pmx_seed_sketch(q, first, nq, mq, k, w, mode, flags, None)

    for entry in (dev, host):
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        for k in (7, 32, -1):
            assert entry(k=k) == -1 and "k %d is outside 8 .. 31" % k in _err(pkg)
        for w in (0, 65, -3):
            assert entry(w=w) == -1 and "w %d is outside 1 .. 64" % w in _err(pkg)
        assert entry(first=-1) == -1 and "negative q_first or nq" in _err(pkg)
        assert entry(nq=-1) == -1 and "negative q_first or nq" in _err(pkg)
        assert entry(first=8, nq=3) == -1 and "beyond the 10 sequences" in _err(pkg)
        for mode in (-1, 3):
            assert entry(mode=mode) == -1 and "strand mode %d is outside 0 .. 2" % mode in _err(pkg)
        for mq in (0, -2):
            assert entry(mq=mq) == -1 and "max_qlen must be positive" in _err(pkg)
        assert entry(nq=10, mq=(1 << 31) - 1) == -1 and "2^31 - 1 position slots" in _err(pkg)
        assert entry(flags=None) == -1 and "null flags with nq > 0" in _err(pkg)
        assert entry(nq=0, flags=None) == 0 and entry(first=10, nq=0, flags=None) == 0         # no rows: success, nothing written
    assert L.pmx_seed_rows_max_len(None, 0, 0) == -1 and "null sequence set" in _err(pkg)
    assert L.pmx_seed_rows_max_len(Q.inner, 8, 3) == -1 and "beyond the 10 sequences" in _err(pkg)
    assert L.pmx_seed_rows_max_len(Q.inner, 3, 0) == 0


def test_python_mirror_refusals(pkg):
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    ix = pkg.SeedIndex.build(empty, 12, w=10)
    assert len(ix) == 0 and ix.k == 12 and ix.w == 10 and ix.nbytes == 0 and ix.bits == 2 and not ix.letters and not ix.translated
    h = pkg.seed_pairs(S, ix, rows=0)
    assert isinstance(h, pkg.SeedHits) and len(h) == 0 and h.kind == "strand"
    plain = pkg.SeedIndex.build(empty, 12)
    assert plain.w == 1 and pkg.SeedIndex.build(empty, 12, 0).w == 1                           # (the stream in alphabet's place, as before)
    with pytest.raises(pkg.BatchError, match="w= is for a DNA index"):
        pkg.SeedIndex.build(empty, 5, alphabet="aa11", w=5)
    with pytest.raises(pkg.BatchError, match="w= is for a DNA index"):
        pkg.SeedIndex.build(empty, 5, alphabet="aa11", translated="both", w=2)
    assert pkg.SeedIndex.build(empty, 5, alphabet="aa11", w=1).w == 1
    with pytest.raises(pkg.BatchError, match="w 65 is outside 1 .. 64"):
        pkg.SeedIndex.build(empty, 12, w=65)
    with pytest.raises(pkg.BatchError, match="w 0 is outside 1 .. 64"):
        pkg.SeedIndex.build(empty, 12, w=0)
    with pytest.raises(pkg.BatchError, match="outside 8 .. 31"):
        pkg.SeedIndex.build(empty, 32, w=5)
    f = pkg.seed_minimizers(S, 15, 10, rows=0, max_qlen=7)
    assert f.shape == (0, 2, 7) and f.dtype == np.uint8
    assert pkg.seed_minimizers(S, 15, 10, strand="forward", rows=0, max_qlen=7).shape == (0, 1, 7)
    with pytest.raises(pkg.BatchError, match="beyond the 3 sequences"):
        pkg.seed_minimizers(S, 15, 10, first_row=2, rows=2, max_qlen=7)
    with pytest.raises(pkg.BatchError, match="w 0 is outside"):
        pkg.seed_minimizers(S, 15, 0, rows=1, max_qlen=7)
    with pytest.raises(pkg.BatchError, match="strand"):
        pkg.seed_minimizers(S, 15, 10, strand="sideways", rows=0, max_qlen=7)
    with pytest.raises(pkg.BatchError, match="null flags"):
        pkg.seed_minimizers_device(S, 0, 1, 7, 15, 10, None)
    with pytest.raises(pkg.BatchError, match="max_qlen must be positive"):
        pkg.seed_minimizers_device(S, 0, 1, 0, 15, 10, 256)
    ix.close()
    with pytest.raises(pkg.BatchError, match="closed"):
        ix.w


PROBES = [(0, s, nq, mq, occ, sl, bud, 1000) for s in (0, 1, 2) for nq, mq in ((1, 1), (2, 150), (1000, 151), (10 ** 6, 150), (7, 10000), (3, 1 << 20))
          for occ, sl, bud in ((64, 0, 0), (1, 0, 0), (65535, 0, 0), (64, 1, 0), (64, 7, 4096), (64, 0, 1 << 34))]


def test_the_plan_is_unchanged_for_w_1_and_costs_a_byte_per_slot_above(pkg):
    L = pkg.lib
    a, b, c = (C.c_longlong * 11)(), (C.c_longlong * 11)(), (C.c_longlong * 11)()
    planned = 0
    for args in PROBES:
        rc = L.pmx_seed_plan_probe(*args, a)
        assert L.pmx_seed_plan_probe_w(*args, 1, b) == rc and list(a) == list(b), args
        assert L.pmx_seed_plan_probe_w(*args, 10, c) == rc, args                             # the refusal (the row budget rule) knows no w
        if rc:
            continue
        planned += 1
        old, new = list(a), list(c)
        assert old[5] == 16 and new[5] == 17
        assert new[:5] == old[:5] and new[10] == old[10]
        nq, mq, sl = args[2], args[3], args[5]
        want = max(1, (1 << 28) // (old[4] * 17))
        want = min(want, nq) if sl == 0 else min(want, sl, nq)
        assert new[6] == want <= old[6] and new[8] == want * old[4] and new[9] == want * old[0]
    assert planned > 60
    # the letters and translated kinds plan as before with w = 1 and take no other w
    for kind, mode in ((1, -1), (1, 8), (1, 11), (2, 0), (2, 1)):
        args = (kind, mode, 1000, 150, 64, 0, 0, 1000)
        assert L.pmx_seed_plan_probe(*args, a) == 0 and L.pmx_seed_plan_probe_w(*args, 1, b) == 0 and list(a) == list(b)
        assert L.pmx_seed_plan_probe_w(*args, 2, b) == -1
    for w in (0, 65, -1):
        assert L.pmx_seed_plan_probe_w(0, 2, 10, 150, 64, 0, 0, 1000, w, b) == -1
