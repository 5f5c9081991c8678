"""CPU tier of the per-query top-K set search: exported symbols and struct layouts, every refusal that needs no GPU (wrapped sets
whose pointers are never followed), each with a pmx_last_error() text that names the reason, the Python mirror's shapes and refusals,
and the model test: the chunked running merge of tests/topk_ref.py -- strict prefilter once a list is full, the list's members first
inside a tie run -- equals the brute-force per-row cut for every chunk size and K."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import topk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_search_topk_device", "pmx_search_topk", "pmx_topk_hits_free")
NMAX = (1 << 31) - 1


def _header():
    return open(os.path.join(ROOT, "include", "parasail_amd.h")).read()


def test_symbols_are_exported_and_declared(pkg):
    text = _header()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    assert re.search(r"#define PMX_TOPK_MAX\s+1024\b", text) and pkg.TOPK_MAX == ref.TOPK_MAX == 1024
    for name in ("search_topk_device", "TopKHits", "pmx_topk_opts_t", "pmx_topk_hits_t"):
        assert hasattr(pkg, name), name
    assert hasattr(pkg.Aligner, "search_topk")


def _layout(text, struct, typedef):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, typedef), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, fields = 0, []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        typ, names = decl.split(None, 1)
        for name in names.split(","):
            name = name.strip()
            size = 8 if name.startswith("*") else {"int32_t": 4, "int64_t": 8}[typ]
            off = (off + size - 1) // size * size
            fields.append((name.lstrip("*"), off, size))
            off += size
    return fields, off


def test_struct_layouts_match_the_header(pkg):
    text = _header()
    fields, size = _layout(text, "pmx_topk_opts", "pmx_topk_opts_t")
    assert size == 32 == C.sizeof(pkg.pmx_topk_opts_t)
    assert [f[0] for f in fields] == ["min_score", "k", "skip_self", "chunk_pairs", "slice_rows"]
    for name, o, sz in fields:
        assert getattr(pkg.pmx_topk_opts_t, name).offset == o and getattr(pkg.pmx_topk_opts_t, name).size == sz, name
    fields, size = _layout(text, "pmx_topk_hits", "pmx_topk_hits_t")
    assert size == 72 == C.sizeof(pkg.pmx_topk_hits_t)
    assert [f[0] for f in fields] == ["n_rows", "n_hits", "n_passing", "row_off", "row_passing", "pairs", "index", "recs", "stats"]
    for name, o, sz in fields:
        assert getattr(pkg.pmx_topk_hits_t, name).offset == o and getattr(pkg.pmx_topk_hits_t, name).size == sz, name


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def _cfg(pkg, pm, want=0):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, want, pm.inner)


def test_topk_refusals_without_gpu(pkg):
    """wrapped sets over addresses that are never followed: every case ends before any GPU work"""
    L = pkg.lib
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = _cfg(pkg, pm)
    S = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    T = pkg.SeqSet.wrap_device(256, 256, 7, 700)
    huge = pkg.SeqSet.wrap_device(256, 256, 4 * 10 ** 9, 1000)
    toomany = pkg.SeqSet.wrap_device(256, 256, NMAX + 1, 1000)
    s, t = S.inner, T.inner
    O, TO = pkg.pmx_pairs_opts_t, pkg.pmx_topk_opts_t

    def dev(c=cfg, q=s, r=t, first=0, nq=4, mq=8, mr=8, ms=0, k=5, skip=0, hp=256, hi=256, hr=256, hs=None, cap=16, off=256, rp=256,
            cnt=256, opts=None):
        return L.pmx_search_topk_device(C.byref(c), q, r, first, nq, mq, mr, ms, k, skip, hp, hi, hr, hs, cap, off, rp, cnt, None,
                                        C.byref(opts) if opts is not None else None)

    def host(c=cfg, q=s, r=t, first=0, nq=4, ms=0, k=5, skip=0, chunk=0, sl=0, opts=True, **unused):
        res = C.POINTER(pkg.pmx_topk_hits_t)()
        o = TO(ms, k, skip, chunk, sl)
        rc = L.pmx_search_topk(C.byref(c), q, r, first, nq, C.byref(o) if opts else None, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_rows == 0 and res.contents.n_hits == 0 and res.contents.n_passing == 0
            L.pmx_topk_hits_free(res)
        else:
            assert not res
        return rc

    for entry in (dev, host):
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(nq=-1) == -1 and "negative" in _err(pkg)
        assert entry(first=-1) == -1 and "negative" in _err(pkg)
        assert entry(first=8, nq=3) == -1 and "beyond the 10 sequences" in _err(pkg)
        assert entry(first=11, nq=0) == -1 and "beyond" in _err(pkg)
        assert entry(k=0) == -1 and "k 0 is outside 1 .. 1024" in _err(pkg)
        assert entry(k=-3) == -1 and "outside 1 .. 1024" in _err(pkg)
        assert entry(k=1025) == -1 and "pmx_search_pairs" in _err(pkg) and "pmx_select_hits_device" in _err(pkg)
        assert entry(skip=1) == -1 and "skip_self" in _err(pkg)                              # R is another set
        assert entry(r=toomany.inner) == -1 and "2^31 - 1" in _err(pkg)
        assert entry(q=huge.inner, r=huge.inner) == -1 and ("2^31 - 1" in _err(pkg) or "overflow" in _err(pkg))
        assert entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR)) == -1 and "CIGAR" in _err(pkg) and "pmx_align_pairs_ex" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(7, 0, 5, 2, 0, 0, pm.inner)) == -1 and "mode" in _err(pkg)
        # no rows: success, nothing touched (the device entry: NULL outputs, as no device is there to write them)
        kw = {"cnt": None, "off": None} if entry is dev else {}
        assert entry(nq=0, **kw) == 0
        assert entry(first=10, nq=0, **kw) == 0
        assert entry(r=None, nq=0, skip=1, **kw) == 0                                         # R NULL means Q: the flag is allowed
        assert entry(r=s, nq=0, skip=1, **kw) == 0
    # the device entry's own
    assert dev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    assert dev(hr=None) == -1 and "null hit records" in _err(pkg)
    assert dev(off=None) == -1 and "null row offsets" in _err(pkg)
    assert dev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert dev(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
    assert dev(c=_cfg(pkg, pm, pkg.WANT_STATS)) == -1 and "stats requested without a stats buffer" in _err(pkg)
    assert dev(hs=256) == -1 and "stats buffer without PMX_WANT_STATS" in _err(pkg)
    assert dev(mq=0) == -1 and "max_qlen" in _err(pkg)
    assert dev(mr=-5) == -1 and "max_qlen" in _err(pkg)
    assert dev(hp=None, hi=None, hr=None, rp=None, cap=0, nq=0, cnt=None, off=None) == 0   # (optional outputs, counting only)
    # the host entry's own
    assert host(opts=False) == -1 and "null opts" in _err(pkg)
    assert host(sl=-1) == -1 and "slice_rows" in _err(pkg)
    assert host(chunk=-1) == -1 and "chunk_pairs" in _err(pkg)
    o = TO(0, 5, 0, 0, 0)
    assert L.pmx_search_topk(C.byref(cfg), s, t, 0, 4, C.byref(o), None) == -1 and "null result" in _err(pkg)
    L.pmx_topk_hits_free(None)


def test_python_mirror_shapes_and_refusals(pkg):
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    T = pkg.SeqSet.wrap_device(256, 256, 4, 12)
    for kw in ({"rows": 0}, {"R": T, "rows": 0}, {"first_row": 3}, {"R": T, "first_row": 3}, {"rows": 0, "skip_self": True}):
        h = al.search_topk(S, k=3, **kw)
        assert isinstance(h, pkg.TopKHits) and len(h) == 0 and h.n_rows == 0 and h.n_passing == 0
        assert h.row_off.tolist() == [0] and h.row_off.dtype == np.int64 and h.row_passing.dtype == np.int64 and len(h.row_passing) == 0
        assert h.pairs.dtype == pkg.PAIR_DTYPE and h.index.dtype == np.int64 and h.records.dtype == pkg.RECORD_DTYPE and h.stats is None
    assert al.search_topk(S, k=3, rows=0, stats=True).stats.dtype == pkg.STATS_DTYPE
    with pytest.raises(pkg.BatchError, match="beyond the 3 sequences"):
        al.search_topk(S, k=3, first_row=2, rows=2)
    with pytest.raises(pkg.BatchError, match="outside 1 .. 1024"):
        al.search_topk(S, k=0)
    with pytest.raises(pkg.BatchError, match="skip_self"):
        al.search_topk(S, T, k=2, skip_self=True)
    prof = pkg.Aligner.new().local().matrix(pm).profile(pkg.Profile.new(b"ACGT", False, pm)).build()
    with pytest.raises(pkg.BatchError, match="no profile"):
        prof.search_topk(S, k=3)


def test_reference_cut_and_capacity():
    recs = np.zeros((6, 4), dtype=np.int32)
    recs[:, 0] = [5, 9, 5, 5, -2, 9]                                                        # two rows of three
    recs[:, 1] = np.arange(6)
    w = ref.topk(recs, 3, 4, 2, 2)
    assert w["row_off"].tolist() == [0, 2, 4] and w["index"].tolist() == [13, 12, 17, 15] and w["counts"] == [4, 4, 6]
    assert [(int(p["q"]), int(p["r"])) for p in w["pairs"]] == [(4, 1), (4, 0), (5, 2), (5, 0)]
    assert w["records"][:, 1].tolist() == [1, 0, 5, 3]
    w = ref.topk(recs, 3, 4, 2, 2, min_score=5, capacity=3)
    assert w["row_off"].tolist() == [0, 2, 4] and w["counts"] == [4, 3, 5] and w["row_passing"].tolist() == [3, 2]
    assert w["index"].tolist() == [13, 12, 17]
    w = ref.topk(recs, 3, 1, 2, 3, skip_self=True)                                          # rows 1 and 2: (1, 1) and (2, 2) are left out
    assert w["index"].tolist() == [3, 5, 6, 7] and w["row_passing"].tolist() == [2, 2]
    assert ref.topk(recs, 3, 0, 2, 5, min_score=ref.INT32_MAX)["row_off"].tolist() == [0, 0, 0]


def test_chunked_merge_equals_the_brute_force_cut():
    """the two chunk-order facts: a full list admits only score > T, and the list's members come first inside a tie run"""
    rng = np.random.default_rng(1100)
    nq = 3
    for nr in (1, 9, 70):
        rows = []
        for levels in (3, 4, 5):
            rows.append(rng.choice(rng.integers(-50, 50, size=levels), size=(nq, nr)))      # heavy ties
        rows.append(np.full((nq, nr), 7))                                                   # all equal
        rows.append(np.tile(np.arange(nr), (nq, 1)) - 5)                                    # strictly increasing with j
        rows.append(20 - np.tile(np.arange(nr), (nq, 1)))                                   # strictly decreasing with j
        rows.append(np.where(np.arange(nq * nr).reshape(nq, nr) % 2 == 0, 12, 11))          # two levels interleaved
        for scores in rows:
            flat = scores.reshape(-1).astype(np.int64)
            for k in sorted({1, 2, 5, nr, nr + 3}):
                for ms, skip in ((ref.INT32_MIN, False), (int(np.median(flat)), False), (ref.INT32_MIN, True)):
                    want = [ref.row_cut(scores[li], k, ms, li if skip else None) for li in range(nq)]
                    for chunk in sorted({1, 7, 64, nr, nr + 1, 3 * nr - 1} - {0}):
                        got, passing = ref.chunked_rows(flat, nr, k, chunk, ms, skip)
                        assert [g for g in got] == [w[0].tolist() for w in want], (nr, k, chunk, ms, skip)
                        assert passing == [w[1] for w in want]
