"""CPU tier of seed chaining: exported symbols and struct sizes, every refusal of pmx_seed_chains[_device] with its pmx_last_error()
text -- over wrapped sets whose pointers are never followed and indexes of an empty set, so every call ends before any GPU work --,
nq == 0, the Python mirror's refusals, and the plan of the cluster road, which costs what it cost: pmx_seed_plan_probe against a sample
of tests/golden/seed_plans.json and against its own arithmetic at 24 bytes per match."""
import ctypes as C
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_seed_chains", "pmx_seed_chains_device", "pmx_seed_chained_free", "pmx_seed_chain_shape")


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def _opts(pkg, strand=2, min_seeds=2, band=500, pad=16, max_occ=64, reserved=0, max_hits=0, slice_rows=0):
    return pkg.pmx_seed_opts_t(strand, min_seeds, band, pad, max_occ, reserved, max_hits, slice_rows)


def _copts(pkg, max_gap=5000, lookback=64, gap_scale=38, min_score=0, reserved=(0, 0, 0, 0)):
    return pkg.pmx_seed_chain_opts_t(max_gap, lookback, gap_scale, min_score, (C.c_int32 * 4)(*reserved))


def test_symbols_structs_and_shape(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name in ("seed_chains", "seed_chains_device", "seed_chain_shape", "SEED_CHAIN_DTYPE"):
        assert hasattr(pkg, name), name
    assert C.sizeof(pkg.pmx_seed_chain_opts_t) == 32 and C.sizeof(pkg.pmx_seed_chain_t) == 32
    assert pkg.SEED_CHAIN_DTYPE.itemsize == 32
    assert pkg.SEED_CHAIN_DTYPE.names == ("score", "n_anchors", "q_beg", "q_end", "r_beg", "r_end", "diag_min", "diag_max")
    assert [f[0] for f in pkg.pmx_seed_chain_t._fields_] == list(pkg.SEED_CHAIN_DTYPE.names)
    assert C.sizeof(pkg.pmx_seed_chained_t) == C.sizeof(pkg.pmx_seed_hits_t) + 8
    assert "typedef struct pmx_seed_chain_opts { int32_t max_gap, lookback, gap_scale, min_score, reserved[4]; } pmx_seed_chain_opts_t;" in text
    lanes, ring = pkg.seed_chain_shape()
    assert lanes == 64 and ring == 1024                                                       # a wave; the largest lookback


@pytest.fixture()
def sets(pkg):
    L = pkg.lib
    Q = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    ix = L.pmx_seed_index_build(empty.inner, 12, None)
    mz = L.pmx_seed_index_build_minimizers(empty.inner, 15, 10, None)
    table = pkg.seed_alphabet("aa11")
    letters = L.pmx_seed_index_build_letters(empty.inner, 5, table.ctypes.data, None)
    translated = L.pmx_seed_index_build_translated(empty.inner, 5, table.ctypes.data, None, 2, None)
    assert ix and mz and letters and translated
    yield Q, ix, mz, letters, translated
    for x in (ix, mz, letters, translated):
        L.pmx_seed_index_free(x)


def test_device_entry_refusals(pkg, sets):
    L = pkg.lib
    Q, ix, mz, letters, translated = sets

    def dev(q=Q.inner, index=ix, first=0, nq=4, mq=150, o="default", co="default", pairs=256, strand=256, seeds=256, chains=256, cap=4, off=256, cnt=256):
        o = _opts(pkg) if o == "default" else o
        co = _copts(pkg) if co == "default" else co
        return L.pmx_seed_chains_device(q, index, first, nq, mq, C.byref(o) if o is not None else None, C.byref(co) if co is not None else None,
                                        pairs, strand, seeds, chains, cap, off, cnt, None)

    # what pmx_seed_pairs_device refuses, with its texts
    assert dev(q=None) == -1 and "null sequence set" in _err(pkg)
    assert dev(index=None) == -1 and "null seed index" in _err(pkg)
    assert dev(o=None) == -1 and "null opts" in _err(pkg)
    assert dev(first=-1) == -1 and "negative q_first or nq" in _err(pkg)
    assert dev(nq=-1) == -1 and "negative q_first or nq" in _err(pkg)
    assert dev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    assert dev(o=_opts(pkg, max_hits=-1)) == -1 and "max_hits must not be negative" in _err(pkg)
    assert dev(o=_opts(pkg, slice_rows=-1)) == -1 and "slice_rows must not be negative" in _err(pkg)
    assert dev(first=8, nq=3) == -1 and "beyond the 10 sequences" in _err(pkg)
    for mq in (0, -5):
        assert dev(mq=mq) == -1 and "max_qlen must be positive" in _err(pkg)
    for s in (-1, 3):
        assert dev(o=_opts(pkg, strand=s)) == -1 and "strand mode %d is outside 0 .. 2" % s in _err(pkg)
    assert dev(o=_opts(pkg, min_seeds=0)) == -1 and "min_seeds 0 is below 1" in _err(pkg)
    for band in (-1, (1 << 20) + 1):
        assert dev(o=_opts(pkg, band=band)) == -1 and "band %d is outside 0 .. 2^20" % band in _err(pkg)
    for pad in (-1, (1 << 20) + 1):
        assert dev(o=_opts(pkg, pad=pad)) == -1 and "pad %d is outside 0 .. 2^20" % pad in _err(pkg)
    for occ in (0, 65536):
        assert dev(o=_opts(pkg, max_occ=occ)) == -1 and "max_occ %d is outside 1 .. 65535" % occ in _err(pkg)
    assert dev(o=_opts(pkg, reserved=1)) == -1 and "reserved must be 0" in _err(pkg)
    assert dev(pairs=None) == -1 and "null hit pairs or strand bytes with capacity > 0" in _err(pkg)
    assert dev(strand=None) == -1 and "null hit pairs or strand bytes with capacity > 0" in _err(pkg)
    assert dev(off=None) == -1 and "null row offsets" in _err(pkg)
    assert dev(cnt=None) == -1 and "null counts" in _err(pkg)
    # its own
    assert dev(co=None) == -1 and "null chain opts" in _err(pkg)
    for gap in (0, -1, (1 << 20) + 1):
        assert dev(co=_copts(pkg, max_gap=gap)) == -1 and "max_gap %d is outside 1 .. 2^20" % gap in _err(pkg)
    for lb in (0, -1, 1025):
        assert dev(co=_copts(pkg, lookback=lb)) == -1 and "lookback %d is outside 1 .. 1024" % lb in _err(pkg)
    for sc in (-1, 65536):
        assert dev(co=_copts(pkg, gap_scale=sc)) == -1 and "gap_scale %d is outside 0 .. 65535" % sc in _err(pkg)
    assert dev(co=_copts(pkg, min_score=-1)) == -1 and "min_score -1 is negative" in _err(pkg)
    for x in range(4):
        res = [0, 0, 0, 0]
        res[x] = 1
        assert dev(co=_copts(pkg, reserved=res)) == -1 and "chain opts: reserved must be 0" in _err(pkg)
    assert dev(index=letters) == -1 and "chaining takes a DNA index" in _err(pkg) and "letters" in _err(pkg)
    assert dev(index=translated) == -1 and "chaining takes a DNA index" in _err(pkg) and "translated" in _err(pkg)
    assert dev(index=letters, nq=0) == -1 and "chaining takes a DNA index" in _err(pkg)     # (whatever the rows)
    # the per-row budget at 40 bytes per match: 2^28 / (2 strands x 64 x 40) positions fit, one more does not
    fit = (1 << 28) // (2 * 64 * 40)
    assert dev(mq=fit + 1) == -1 and "worst case" in _err(pkg) and "x 40 bytes per match" in _err(pkg)
    assert dev(mq=fit + 1, o=_opts(pkg, strand=0), co=None) == -1 and "null chain opts" in _err(pkg)
    old = L.pmx_seed_match_budget(1 << 34)
    try:
        assert dev(mq=(1 << 26) + 1, o=_opts(pkg, strand=0, max_occ=1)) == -1 and "above 2^26" in _err(pkg)
    finally:
        L.pmx_seed_match_budget(0)
    assert old == 1 << 28
    # the cluster road's rule still counts 24 bytes: a row that chaining refuses is planned there (its nq == 0 path needs no GPU)
    assert L.pmx_seed_pairs_device(Q.inner, ix, 0, 0, fit + 1, C.byref(_opts(pkg, band=8)), None, None, None, 0, None, None, None) == 0
    # no rows: success before any GPU work, with every valid index of the DNA road, outputs NULL
    for index in (ix, mz):
        assert dev(index=index, nq=0, pairs=None, strand=None, seeds=None, chains=None, cap=0, off=None, cnt=None) == 0
        assert dev(index=index, first=10, nq=0, pairs=None, strand=None, seeds=None, chains=None, cap=0, off=None, cnt=None) == 0
    # the extremes of every range are taken
    assert dev(nq=0, off=None, cnt=None, o=_opts(pkg, band=1 << 20), co=_copts(pkg, max_gap=1 << 20, lookback=1024, gap_scale=65535, min_score=(1 << 31) - 1)) == 0
    assert dev(nq=0, off=None, cnt=None, o=_opts(pkg, band=0), co=_copts(pkg, max_gap=1, lookback=1, gap_scale=0, min_score=0)) == 0


def test_host_entry_refusals_and_no_rows(pkg, sets):
    L = pkg.lib
    Q, ix, mz, letters, translated = sets
    res = C.POINTER(pkg.pmx_seed_chained_t)()
    o, co = _opts(pkg), _copts(pkg)
    assert L.pmx_seed_chains(Q.inner, ix, 0, 0, C.byref(o), C.byref(co), None) == -1 and "null result pointer" in _err(pkg)
    assert L.pmx_seed_chains(None, ix, 0, 0, C.byref(o), C.byref(co), C.byref(res)) == -1 and "null sequence set" in _err(pkg) and not res
    assert L.pmx_seed_chains(Q.inner, ix, 0, 0, C.byref(o), None, C.byref(res)) == -1 and "null chain opts" in _err(pkg)
    assert L.pmx_seed_chains(Q.inner, letters, 0, 0, C.byref(o), C.byref(co), C.byref(res)) == -1 and "chaining takes a DNA index" in _err(pkg)
    assert L.pmx_seed_chains(Q.inner, ix, 0, 11, C.byref(o), C.byref(co), C.byref(res)) == -1 and "beyond the 10 sequences" in _err(pkg)
    bad = _copts(pkg, lookback=2000)
    assert L.pmx_seed_chains(Q.inner, ix, 0, 0, C.byref(o), C.byref(bad), C.byref(res)) == -1 and "lookback 2000 is outside 1 .. 1024" in _err(pkg)
    assert L.pmx_seed_chains(Q.inner, mz, 3, 0, C.byref(o), C.byref(co), C.byref(res)) == 0 and res
    r = res.contents
    assert (r.hits.n_rows, r.hits.n_hits, r.hits.n_passing) == (0, 0, 0)
    assert C.cast(r.hits.row_off, C.POINTER(C.c_int64))[0] == 0
    L.pmx_seed_chained_free(res)
    L.pmx_seed_chained_free(None)


def test_python_mirror(pkg):
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    empty = pkg.SeqSet.wrap_device(256, 256, 0, 0)
    ix = pkg.SeedIndex.build(empty, 12, w=10)
    h = pkg.seed_chains(S, ix, rows=0)
    assert isinstance(h, pkg.SeedHits) and len(h) == 0 and h.kind == "strand" and h.row_off.tolist() == [0]
    assert h.chains.dtype == pkg.SEED_CHAIN_DTYPE and h.chains.shape == (0,)
    with pytest.raises(pkg.BatchError, match="chaining takes a DNA index"):
        pkg.seed_chains(S, pkg.SeedIndex.build(empty, 5, alphabet="aa11"), rows=0)
    with pytest.raises(pkg.BatchError, match="chaining takes a DNA index"):
        pkg.seed_chains(S, pkg.SeedIndex.build(empty, 5, alphabet="aa11", translated="both"), rows=0)
    with pytest.raises(pkg.BatchError, match="lookback 0 is outside"):
        pkg.seed_chains(S, ix, rows=0, lookback=0)
    with pytest.raises(pkg.BatchError, match="max_gap 0 is outside"):
        pkg.seed_chains(S, ix, rows=0, max_gap=0)
    with pytest.raises(pkg.BatchError, match="min_score -3 is negative"):
        pkg.seed_chains(S, ix, rows=0, min_score=-3)
    with pytest.raises(pkg.BatchError, match="beyond the 3 sequences"):
        pkg.seed_chains(S, ix, first_row=2, rows=2)
    with pytest.raises(pkg.BatchError, match="null row offsets"):
        pkg.seed_chains_device(S, ix, 0, 1, 150, None, None, None, None, 0, None, None)
    with pytest.raises(pkg.BatchError, match="gap_scale 70000"):
        pkg.seed_chains_device(S, ix, 0, 1, 150, None, None, None, None, 0, 256, 256, gap_scale=70000)
    pkg.seed_chains_device(S, ix, 0, 0, 150, None, None, None, None, 0, None, None)           # no rows: nothing to do


def test_the_cluster_road_plans_what_it_planned(pkg):
    """chaining has a match size of its own; every existing mode still plans with 24 bytes per match"""
    L = pkg.lib
    with open(os.path.join(ROOT, "tests", "golden", "seed_plans.json")) as f:
        table = json.load(f)
    out = (C.c_longlong * 11)()
    checked = 0
    for ctx in table["contexts"][::7]:
        kind, mode, max_occ, slice_rows, budget, ref_count = ctx[:6]
        for want in ctx[6][::5]:
            rc = L.pmx_seed_plan_probe(kind, mode, want[0], want[1], max_occ, slice_rows, budget, ref_count, out)
            assert want[:2] + (list(out) if rc == 0 else []) == want
            checked += 1
    assert checked > 40
    for mode, nq, mq in ((2, 1000, 150), (0, 7, 10000), (1, 10 ** 6, 151)):
        assert L.pmx_seed_plan_probe(0, mode, nq, mq, 64, 0, 0, 1000, out) == 0
        orients = 2 if mode == 2 else 1
        rows = min(nq, max(1, (1 << 28) // (orients * mq * 16)))
        assert out[6] == rows and out[7] == min((1 << 28) // 24, rows * orients * mq * 64)
