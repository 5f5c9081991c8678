"""CPU tier of set search: exported symbols and struct layouts, pmx_rect_pairs_count against exact Python integers, the Python
restatement of both enumerations against brute force, and every refusal that needs no GPU (wrapped sets whose pointers are never
followed), each with a pmx_last_error() text that names the reason."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_ref
import set_search_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_rect_pairs_count", "pmx_rect_pairs_enumerate_device", "pmx_search_pairs_device", "pmx_search_pairs", "pmx_pair_hits_free")
NMAX = (1 << 31) - 1


def _header():
    return open(os.path.join(ROOT, "include", "parasail_amd.h")).read()


def test_symbols_are_exported_and_declared(pkg):
    text = _header()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name, value in (("LIST", 0), ("TRIANGLE", 1), ("RECT", 2)):
        assert re.search(r"#define PMX_PAIRS_%s\s+%d\b" % (name, value), text)
        assert getattr(pkg, "PAIRS_" + name) == getattr(ref, "PAIRS_" + name) == value
    for name in ("search_pairs_device", "rect_pairs_count", "rect_pairs_enumerate_device", "PairHits"):
        assert hasattr(pkg, name), name
    assert hasattr(pkg.Aligner, "search_pairs")


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
    fields, size = _layout(text, "pmx_pair_search_opts", "pmx_pair_search_opts_t")
    assert size == 32 == C.sizeof(pkg.pmx_pair_search_opts_t)
    assert [f[0] for f in fields] == ["min_score", "shape", "max_hits", "chunk_pairs", "slice_pairs"]
    for name, o, sz in fields:
        assert getattr(pkg.pmx_pair_search_opts_t, name).offset == o and getattr(pkg.pmx_pair_search_opts_t, name).size == sz, name
    fields, size = _layout(text, "pmx_pair_hits", "pmx_pair_hits_t")
    assert size == 48 == C.sizeof(pkg.pmx_pair_hits_t)
    assert [f[0] for f in fields] == ["n_hits", "n_passing", "pairs", "index", "recs", "stats"]
    for name, o, sz in fields:
        assert getattr(pkg.pmx_pair_hits_t, name).offset == o and getattr(pkg.pmx_pair_hits_t, name).size == sz, name


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_rect_pairs_count_against_python_integers(pkg):
    L = pkg.lib
    big = 3 * 10 ** 9
    cases = [(0, 0), (0, 5), (5, 0), (1, 1), (7, 300), (NMAX, NMAX), (NMAX + 1, 3), (big, big), (1 << 62, 1), (1 << 62, 2), ((1 << 63) - 1, 1),
             (4 * 10 ** 9, 4 * 10 ** 9), (3037000499, 3037000499), (3037000500, 3037000500), (-1, 3), (3, -1)]
    for nq, nr in cases:
        want = ref.rect_pairs_count(nq, nr)
        assert L.pmx_rect_pairs_count(nq, nr) == want, (nq, nr)
        if want < 0:
            assert ("negative" if min(nq, nr) < 0 else "overflow") in _err(pkg)
            with pytest.raises(pkg.BatchError):
                pkg.rect_pairs_count(nq, nr)
        else:
            assert pkg.rect_pairs_count(nq, nr) == nq * nr
    assert ref.rect_pairs_count(big, big) == 9 * 10 ** 18 and ref.rect_pairs_count(4 * 10 ** 9, 4 * 10 ** 9) == -1


def test_reference_enumerations_equal_brute_force():
    for nq, nr in ((1, 1), (1, 5), (5, 1), (3, 4), (7, 13)):
        want = [(i, j) for i in range(nq) for j in range(nr)]
        assert len(want) == ref.rect_pairs_count(nq, nr) == ref.shape_count(ref.PAIRS_RECT, nq, nr)
        assert [ref.rect_pairs_index(nr, p) for p in range(len(want))] == want
        cut = 2 if len(want) > 4 else 0                                                     # a window that starts and ends mid-row
        d = ref.descriptors(ref.PAIRS_RECT, nq, nr, cut, len(want) - 2 * cut)
        assert [(int(x["q"]), int(x["r"])) for x in d] == want[cut:len(want) - cut]
        assert (d["q_beg"] == 0).all() and (d["q_len"] == -1).all() and (d["r_beg"] == 0).all() and (d["r_len"] == -1).all()
    for n in (2, 3, 5, 17):
        want = [(i, j) for i in range(n) for j in range(i + 1, n)]
        assert len(want) == ref.shape_count(ref.PAIRS_TRIANGLE, n, n)
        d = ref.descriptors(ref.PAIRS_TRIANGLE, n, n, 0, len(want))
        assert [(int(x["q"]), int(x["r"])) for x in d] == want
    recs = np.array([[5, 0, 0, 0], [-3, 1, 1, 0], [0, -1, -1, 8], [9, 2, 2, 0], [5, 3, 3, 0]], dtype=np.int32)
    h = ref.hits(recs, 5, first=100)
    assert h["passing"] == 3 and h["index"].tolist() == [100, 103, 104] and h["records"][:, 0].tolist() == [5, 9, 5]
    h = ref.hits(recs, 0, capacity=2)
    assert h["passing"] == 4 and h["written"] == 2 and h["index"].tolist() == [0, 2]                # (a bad pair's record passes at 0)
    assert ref.hits(recs, ref.INT32_MAX)["passing"] == 0 and ref.hits(recs, ref.INT32_MIN)["passing"] == 5


def _cfg(pkg, pm, want=0):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, want, pm.inner)


def test_search_refusals_without_gpu(pkg):
    """wrapped sets over addresses that are never followed: every case ends before any GPU work"""
    L = pkg.lib
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = _cfg(pkg, pm)
    S = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    T = pkg.SeqSet.wrap_device(256, 256, 7, 700)
    huge = pkg.SeqSet.wrap_device(256, 256, 4 * 10 ** 9, 1000)
    toomany = pkg.SeqSet.wrap_device(256, 256, NMAX + 1, 1000)
    s, t = S.inner, T.inner
    O, SO = pkg.pmx_pairs_opts_t, pkg.pmx_pair_search_opts_t
    LIST, TRI, RECT = pkg.PAIRS_LIST, pkg.PAIRS_TRIANGLE, pkg.PAIRS_RECT
    pairs = np.zeros(4, dtype=pkg.PAIR_DTYPE)
    tri_total, rect_total = pairs_ref.all_pairs_count(10), 70

    def dev(c=cfg, q=s, r=None, shape=TRI, first=0, n=4, p=None, mq=8, mr=8, ms=0, hp=256, hi=256, hr=256, hs=None, cap=16, cnt=256, opts=None):
        return L.pmx_search_pairs_device(C.byref(c), q, r, shape, first, n, p, mq, mr, ms, hp, hi, hr, hs, cap, cnt, None,
                                         C.byref(opts) if opts is not None else None)

    def host(c=cfg, q=s, r=None, shape=TRI, first=0, n=4, p=None, max_hits=0, chunk=0, sl=0, opts=True):
        res = C.POINTER(pkg.pmx_pair_hits_t)()
        o = SO(0, shape, max_hits, chunk, sl)
        rc = L.pmx_search_pairs(C.byref(c), q, r, first, n, p, C.byref(o) if opts else None, C.byref(res))
        if rc == 0:
            assert res and res.contents.n_hits == 0 and res.contents.n_passing == 0
            L.pmx_pair_hits_free(res)
        else:
            assert not res
        return rc

    pp = pairs.ctypes.data
    for entry, lp in ((dev, 256), (host, pp)):
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(shape=3) == -1 and "unknown pair shape 3" in _err(pkg)
        assert entry(shape=-1) == -1 and "unknown pair shape" in _err(pkg)
        assert entry(shape=TRI, r=t) == -1 and "R must be NULL or Q" in _err(pkg)
        assert entry(shape=RECT, r=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(shape=LIST, r=None, p=lp) == -1 and "null sequence set" in _err(pkg)
        assert entry(shape=LIST, r=t, p=lp, first=1) == -1 and "first must be 0" in _err(pkg)
        assert entry(shape=LIST, r=t, p=None) == -1 and "null pairs" in _err(pkg)
        assert entry(shape=TRI, p=lp) == -1 and "pairs must be NULL" in _err(pkg)
        assert entry(shape=RECT, r=t, p=lp) == -1 and "pairs must be NULL" in _err(pkg)
        assert entry(n=-1) == -1 and "negative" in _err(pkg)
        assert entry(first=-1) == -1 and "negative" in _err(pkg)
        assert entry(shape=TRI, first=tri_total - 3, n=4) == -1 and "beyond" in _err(pkg)
        assert entry(shape=TRI, first=tri_total + 1, n=0) == -1 and "beyond" in _err(pkg)
        assert entry(shape=TRI, q=toomany.inner) == -1 and "nseq" in _err(pkg)
        assert entry(shape=RECT, r=t, first=rect_total - 3, n=4) == -1 and "beyond the 70 pairs of 10 x 7" in _err(pkg)
        assert entry(shape=RECT, r=t, first=rect_total + 1, n=0) == -1 and "beyond" in _err(pkg)
        assert entry(shape=RECT, q=huge.inner, r=huge.inner) == -1 and "overflow" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR)) == -1 and "CIGAR" in _err(pkg) and "pmx_align_pairs_ex" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(7, 0, 5, 2, 0, 0, pm.inner)) == -1 and "mode" in _err(pkg)
        # an empty window touches nothing, whatever the shape (the device entry: d_counts NULL, as no device is there to write it)
        kw = {"cnt": None} if entry is dev else {}
        assert entry(n=0, **kw) == 0
        assert entry(shape=TRI, r=s, first=tri_total, n=0, **kw) == 0
        assert entry(shape=RECT, r=t, first=rect_total, n=0, **kw) == 0
        assert entry(shape=RECT, r=s, n=0, **kw) == 0
        assert entry(shape=LIST, r=t, n=0, p=None, **kw) == 0
    # the device entry's own
    assert dev(cap=-1) == -1 and "negative capacity" in _err(pkg)
    assert dev(hr=None) == -1 and "null hit records" in _err(pkg)
    assert dev(hr=None, cap=0, n=0, cnt=None) == 0                                         # (counting only needs no records)
    assert dev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert dev(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
    assert dev(c=_cfg(pkg, pm, pkg.WANT_STATS)) == -1 and "stats requested without a stats buffer" in _err(pkg)
    assert dev(hs=256) == -1 and "stats buffer without PMX_WANT_STATS" in _err(pkg)
    assert dev(mq=0) == -1 and "max_qlen" in _err(pkg)
    assert dev(mr=-5) == -1 and "max_qlen" in _err(pkg)
    assert dev(hp=None, hi=None, n=0, cnt=None) == 0                                       # (optional outputs)
    # the host entry's own
    assert host(opts=False) == -1 and "null opts" in _err(pkg)
    assert host(max_hits=-1) == -1 and "max_hits" in _err(pkg)
    assert host(sl=-1) == -1 and "slice_pairs" in _err(pkg)
    assert host(chunk=-1) == -1 and "chunk_pairs" in _err(pkg)
    o = SO(0, TRI, 0, 0, 0)
    assert L.pmx_search_pairs(C.byref(cfg), s, None, 0, 4, None, C.byref(o), None) == -1 and "null result" in _err(pkg)
    L.pmx_pair_hits_free(None)
    # the enumerator hook
    assert L.pmx_rect_pairs_enumerate_device(10, 7, 68, 3, 256, None) == -1 and "beyond" in _err(pkg)
    assert L.pmx_rect_pairs_enumerate_device(10, 7, -1, 3, 256, None) == -1 and "negative" in _err(pkg)
    assert L.pmx_rect_pairs_enumerate_device(-10, 7, 0, 3, 256, None) == -1 and "negative" in _err(pkg)
    assert L.pmx_rect_pairs_enumerate_device(4 * 10 ** 9, 4 * 10 ** 9, 0, 3, 256, None) == -1 and "overflow" in _err(pkg)
    assert L.pmx_rect_pairs_enumerate_device(10, 7, 0, 3, None, None) == -1 and "null" in _err(pkg)
    assert L.pmx_rect_pairs_enumerate_device(10, 7, 70, 0, None, None) == 0


def test_python_mirror_shapes_and_refusals(pkg):
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    T = pkg.SeqSet.wrap_device(256, 256, 4, 12)
    for kw in ({"count": 0}, {"R": T, "count": 0}, {"R": T, "first": 12}, {"first": 3}, {"pairs": []}, {"R": T, "pairs": np.zeros(0, dtype=pkg.PAIR_DTYPE)}):
        h = al.search_pairs(S, min_score=5, **kw)
        assert isinstance(h, pkg.PairHits) and len(h) == 0 and h.n_passing == 0
        assert h.pairs.dtype == pkg.PAIR_DTYPE and h.index.dtype == np.int64 and h.records.dtype == pkg.RECORD_DTYPE and h.stats is None
    assert al.search_pairs(S, count=0, stats=True).stats.dtype == pkg.STATS_DTYPE
    with pytest.raises(pkg.BatchError, match="beyond"):
        al.search_pairs(S, first=2, count=2)
    with pytest.raises(pkg.BatchError, match="beyond the 12 pairs of 3 x 4"):
        al.search_pairs(S, T, first=10, count=3)
    with pytest.raises(pkg.BatchError, match="max_hits"):
        al.search_pairs(S, max_hits=-1)
    prof = pkg.Aligner.new().local().matrix(pm).profile(pkg.Profile.new(b"ACGT", False, pm)).build()
    with pytest.raises(pkg.BatchError, match="no profile"):
        prof.search_pairs(S)
