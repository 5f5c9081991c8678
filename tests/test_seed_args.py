"""CPU tier of k-mer seeding: exported symbols and struct layouts, every refusal that needs no GPU -- wrapped sets whose pointers are
never followed, and the index of an empty wrapped set, which is built without GPU work --, each with a pmx_last_error() text that names
the reason, and the Python mirror's shapes and refusals.  Not here: the refusal of a set or index of another device than the current
one, which needs two devices -- every call below ends before the device is asked for, so it also ends before any pointer is
followed on a machine that has one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import seed_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_seed_index_build", "pmx_seed_index_free", "pmx_seed_index_count", "pmx_seed_index_entries_device",
           "pmx_seed_pairs_device", "pmx_seed_pairs", "pmx_seed_hits_free", "pmx_seed_match_budget")


def _header():
    return open(os.path.join(ROOT, "include", "parasail_amd.h")).read()


def test_symbols_are_exported_and_declared(pkg):
    text = _header()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name in ("SeedIndex", "SeedHits", "seed_pairs", "seed_pairs_device", "seed_index_entries_device", "pmx_seed_hit_t",
                 "pmx_seed_opts_t", "pmx_seed_hits_t", "SEED_HIT_DTYPE"):
        assert hasattr(pkg, name), name
    assert "csrc/pmx_seed.hip" in open(os.path.join(ROOT, "parasail-rs_amd", "Makefile")).read()


def _layout(text, struct, typedef):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, typedef), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int32_t": 4, "int64_t": 8, "uint8_t": 1, "pmx_pair_t": 32, "pmx_seed_hit_t": 16}
    off, fields = 0, []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        typ, names = decl.split(None, 1)
        for name in names.split(","):
            name = name.strip()
            size = 8 if name.startswith("*") else sizes[typ]
            off = (off + size - 1) // size * size
            fields.append((name.lstrip("*"), off, size))
            off += size
    return fields, off


def test_struct_layouts_match_the_header(pkg):
    text = _header()
    for struct, cls, size, names in (
            ("pmx_seed_hit", pkg.pmx_seed_hit_t, 16, ["n_seeds", "diag_min", "diag_max", "reserved"]),
            ("pmx_seed_opts", pkg.pmx_seed_opts_t, 40, ["strand", "min_seeds", "band", "pad", "max_occ", "reserved", "max_hits", "slice_rows"]),
            ("pmx_seed_hits", pkg.pmx_seed_hits_t, 56, ["n_rows", "n_hits", "n_passing", "row_off", "pairs", "strand", "seeds"])):
        fields, total = _layout(text, struct, struct + "_t")
        assert total == size == C.sizeof(cls), struct
        assert [f[0] for f in fields] == names
        for name, o, sz in fields:
            assert getattr(cls, name).offset == o and getattr(cls, name).size == sz, (struct, name)
    assert pkg.SEED_HIT_DTYPE.itemsize == 16 and pkg.SEED_HIT_DTYPE == ref.SEED_HIT_DTYPE and pkg.PAIR_DTYPE == ref.PAIR_DTYPE


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_index_refusals_and_the_empty_index(pkg):
    L = pkg.lib
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    big = pkg.SeqSet.wrap_device(256, 256, 3, 1 << 31)
    many = pkg.SeqSet.wrap_device(256, 256, 1 << 31, 1000)
    assert not L.pmx_seed_index_build(None, 12, None) and "null sequence set" in _err(pkg)
    for k in (7, 32, 0, -1):
        assert not L.pmx_seed_index_build(empty.inner, k, None) and "k %d is outside 8 .. 31" % k in _err(pkg)
    assert not L.pmx_seed_index_build(big.inner, 12, None) and "2^31 - 1 bytes" in _err(pkg)
    assert not L.pmx_seed_index_build(many.inner, 12, None) and "2^31 - 1 bytes and sequences" in _err(pkg)
    assert L.pmx_seed_index_count(None) == -1
    L.pmx_seed_index_free(None)
    for k in (8, 31):
        ix = L.pmx_seed_index_build(empty.inner, k, None)                                  # nothing to index: no GPU work
        assert ix and L.pmx_seed_index_count(ix) == 0
        assert L.pmx_seed_index_entries_device(ix, 0, 0, None, None, None, None) == 0
        assert L.pmx_seed_index_entries_device(ix, 0, 1, 256, 256, 256, None) == -1 and "beyond the 0 entries" in _err(pkg)
        assert L.pmx_seed_index_entries_device(ix, -1, 0, 256, 256, 256, None) == -1 and "negative" in _err(pkg)
        L.pmx_seed_index_free(ix)
    assert L.pmx_seed_index_entries_device(None, 0, 0, None, None, None, None) == -1 and "null seed index" in _err(pkg)


def test_seeding_refusals_without_gpu(pkg):
    """wrapped sets over addresses that are never followed and an empty index: every case ends before any GPU work"""
    L = pkg.lib
    Q = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    ix = L.pmx_seed_index_build(empty.inner, 12, None)
    assert ix
    SO = pkg.pmx_seed_opts_t

    def opts(strand=2, min_seeds=2, band=8, pad=16, max_occ=64, reserved=0, max_hits=0, slice_rows=0):
        return SO(strand, min_seeds, band, pad, max_occ, reserved, max_hits, slice_rows)

    def dev(q=Q.inner, index=ix, first=0, nq=4, mq=150, o=opts(), hp=256, hs=256, hd=256, cap=16, off=256, cnt=256):
        return L.pmx_seed_pairs_device(q, index, first, nq, mq, C.byref(o) if o is not None else None, hp, hs, hd, cap, off, cnt, None)

    def host(q=Q.inner, index=ix, first=0, nq=4, o=opts(), **unused):
        res = C.POINTER(pkg.pmx_seed_hits_t)()
        rc = L.pmx_seed_pairs(q, index, first, nq, C.byref(o) if o is not None else None, C.byref(res))
        if rc == 0:
            r = res.contents
            assert r.n_rows == 0 and r.n_hits == 0 and r.n_passing == 0 and C.cast(r.row_off, C.POINTER(C.c_int64))[0] == 0
            L.pmx_seed_hits_free(res)
        else:
            assert not res
        return rc

    for entry in (dev, host):
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(index=None) == -1 and "null seed index" in _err(pkg)
        assert entry(o=None) == -1 and "null opts" in _err(pkg)
        assert entry(first=-1) == -1 and "negative q_first or nq" in _err(pkg)
        assert entry(nq=-1) == -1 and "negative q_first or nq" in _err(pkg)
        assert entry(o=opts(max_hits=-1)) == -1 and "max_hits" in _err(pkg)
        assert entry(o=opts(slice_rows=-1)) == -1 and "slice_rows" in _err(pkg)
        assert entry(first=8, nq=3) == -1 and "beyond the 10 sequences" in _err(pkg)
        assert entry(first=11, nq=0) == -1 and "beyond" in _err(pkg)
        for mode in (-1, 3):
            assert entry(o=opts(strand=mode)) == -1 and "strand mode %d is outside 0 .. 2" % mode in _err(pkg)
        assert entry(o=opts(min_seeds=0)) == -1 and "min_seeds 0 is below 1" in _err(pkg)
        for bad in (-1, (1 << 20) + 1):
            assert entry(o=opts(band=bad)) == -1 and "band %d is outside 0 .. 2^20" % bad in _err(pkg)
            assert entry(o=opts(pad=bad)) == -1 and "pad %d is outside 0 .. 2^20" % bad in _err(pkg)
        for bad in (0, -5, 65536):
            assert entry(o=opts(max_occ=bad)) == -1 and "max_occ %d is outside 1 .. 65535" % bad in _err(pkg)
        assert entry(o=opts(reserved=1)) == -1 and "reserved must be 0" in _err(pkg)
        # no rows: success, nothing touched (the device entry: NULL outputs, as no device is there to write them)
        kw = {"cnt": None, "off": None} if entry is dev else {}
        assert entry(nq=0, **kw) == 0
        assert entry(first=10, nq=0, **kw) == 0
        assert entry(nq=0, o=opts(band=1 << 20, pad=1 << 20, max_occ=65535, strand=0), **kw) == 0
    # the device entry's own
    assert dev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    for mq in (0, -3):
        assert dev(mq=mq) == -1 and "max_qlen must be positive" in _err(pkg)
    assert dev(hp=None) == -1 and "null hit pairs or strand bytes" in _err(pkg)
    assert dev(hs=None) == -1 and "null hit pairs or strand bytes" in _err(pkg)
    assert dev(off=None) == -1 and "null row offsets" in _err(pkg)
    assert dev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert dev(hp=None, hs=None, hd=None, cap=0, nq=0, off=None, cnt=None) == 0
    # the per-row budget: max_qlen x strands x max_occ x 24 bytes against 256 MiB
    assert dev(mq=100000, o=opts(max_occ=65535)) == -1 and "worst case" in _err(pkg) and "match buffer" in _err(pkg)
    assert dev(mq=(1 << 28) // (2 * 64 * 24) + 1) == -1 and "worst case" in _err(pkg)
    was = L.pmx_seed_match_budget(1 << 16)
    try:
        assert was == 1 << 28 and L.pmx_seed_match_budget(1 << 16) == 1 << 16
        assert dev(mq=22) == -1 and "worst case" in _err(pkg) and "65536 bytes" in _err(pkg)      # 22 x 2 x 64 x 24 = 67 584
        assert dev(mq=21, nq=0, off=None, cnt=None) == 0
    finally:
        L.pmx_seed_match_budget(0)
    assert L.pmx_seed_match_budget(0) == 1 << 28
    # the host entry's own
    o = opts()
    assert L.pmx_seed_pairs(Q.inner, ix, 0, 4, C.byref(o), None) == -1 and "null result" in _err(pkg)
    L.pmx_seed_hits_free(None)
    L.pmx_seed_index_free(ix)


def test_python_mirror_shapes_and_refusals(pkg):
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    ix = pkg.SeedIndex.build(empty, 12)
    assert len(ix) == 0 and ix.k == 12
    for kw in ({"rows": 0}, {"first_row": 3}, {"rows": 0, "strand": "forward", "max_hits": 5, "slice_rows": 2}, {"rows": 0, "strand": 1}):
        h = pkg.seed_pairs(S, ix, **kw)
        assert isinstance(h, pkg.SeedHits) and len(h) == 0 and h.n_rows == 0 and h.n_passing == 0
        assert h.row_off.tolist() == [0] and h.row_off.dtype == np.int64
        assert h.pairs.dtype == pkg.PAIR_DTYPE and h.strand.dtype == np.uint8 and h.seeds.dtype == pkg.SEED_HIT_DTYPE
        assert len(h.pairs) == len(h.strand) == len(h.seeds) == 0
    with pytest.raises(pkg.BatchError, match="beyond the 3 sequences"):
        pkg.seed_pairs(S, ix, first_row=2, rows=2)
    with pytest.raises(pkg.BatchError, match="min_seeds 0 is below 1"):
        pkg.seed_pairs(S, ix, min_seeds=0, rows=0)
    with pytest.raises(pkg.BatchError, match="strand"):
        pkg.seed_pairs(S, ix, strand="sideways", rows=0)
    with pytest.raises(pkg.BatchError, match="outside 8 .. 31"):
        pkg.SeedIndex.build(empty, 32)
    with pytest.raises(pkg.BatchError, match="max_qlen must be positive"):
        pkg.seed_pairs_device(S, ix, 0, 1, 0, 256, 256, None, 4, 256, 256)
    with pytest.raises(pkg.BatchError, match="beyond the 0 entries"):
        pkg.seed_index_entries_device(ix, 0, 1, 256, 256, 256)
    ix.close()
    with pytest.raises(pkg.BatchError, match="closed"):
        len(ix)
