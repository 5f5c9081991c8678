"""CPU tier of the profile search: the numpy reference of the selection against a plain sorted() formulation, every refusal of the
search entries (before any GPU work: no device is needed), and the layout of the two new structs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import search_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", range(6))
def test_reference_select_equals_sorted_formulation(seed):
    rng = np.random.default_rng(4100 + seed)
    for n in (1, 2, 63, 64, 65, 500, 3000):
        scores = search_ref.tied_scores(rng, n, distinct=3 + seed * 4)
        values = np.unique(scores)
        for min_score in (-(1 << 31), int(values[len(values) // 2]), int(values[-1]) + 1):
            npass = int((scores >= min_score).sum())
            for max_hits in sorted({0, 1, max(1, npass // 3), max(1, npass), npass + 1}):
                for order in (search_ref.BY_INDEX, search_ref.BY_SCORE):
                    got, gp = search_ref.select(scores, min_score, max_hits, order)
                    want, wp = search_ref.select_sorted(scores, min_score, max_hits, order)
                    assert gp == wp == npass
                    assert got.tolist() == want, (n, min_score, max_hits, order)
                    assert len(want) == (min(npass, max_hits) if max_hits else npass)


def test_reference_select_cuts_inside_the_tie_run():
    scores = np.array([5, 9, 5, 5, 9, 1, 5, 5], dtype=np.int32)
    assert search_ref.select(scores, 2, 4, search_ref.BY_INDEX)[0].tolist() == [0, 1, 2, 4]
    assert search_ref.select(scores, 2, 4, search_ref.BY_SCORE)[0].tolist() == [1, 4, 0, 2]
    assert search_ref.select(scores, 2, 0, search_ref.BY_SCORE)[0].tolist() == [1, 4, 0, 2, 3, 6, 7]


def _wide_thresholds(scores):
    """the minimum, a median value, and one above the maximum (the maximum itself where that is INT32_MAX: no threshold lies above)"""
    values = np.unique(scores)
    return (int(values[0]), int(values[len(values) // 2]), min(int(values[-1]) + 1, search_ref.INT32_MAX))


@pytest.mark.parametrize("name", sorted(search_ref.WIDE_SCORES))
def test_radix_select_model_equals_the_reference(name):
    """the three narrowing passes of the device's select, restated in numpy, choose what select() chooses on every generator of wide
    scores -- and the generators spread over the digits they are named for"""
    rng = np.random.default_rng(4200)
    for n in (1, 2, 257, 2049, 20011):
        scores = search_ref.WIDE_SCORES[name](rng, n)
        assert scores.dtype == np.int32
        u = (scores.astype(np.int64) & 0xFFFFFFFF) ^ 0x80000000
        bins = [len(np.unique((u >> shift) & ((1 << bits) - 1))) for shift, bits in search_ref.DIGITS]
        if n >= 2049:
            spread = {"full-range": (1000, 1000, 500), "top-digit": (30, 1, 1), "middle-digit": (1, 30, 1), "low-digit": (1, 1, 30),
                      "clusters": (6, 4, 3)}[name]
            assert all(b >= w for b, w in zip(bins, spread)) and (name in ("full-range", "clusters") or sorted(bins)[:2] == [1, 1])
        for min_score in _wide_thresholds(scores):
            npass = int((scores >= min_score).sum())
            s = np.sort(scores[scores >= min_score])[::-1]
            inside = int((s > s[len(s) // 2]).sum()) + int((s == s[len(s) // 2]).sum()) // 2 if npass else 0
            for max_hits in sorted({0, 1, inside, max(npass - 1, 0), npass, npass + 1}):
                want, wp = search_ref.select(scores, min_score, max_hits, search_ref.BY_INDEX)
                T, above, E = search_ref.radix_select_model(scores, min_score, max_hits)
                ctx = (name, n, min_score, max_hits)
                assert search_ref.model_selection(scores, min_score, max_hits).tolist() == want.tolist(), ctx
                if T is None:
                    assert (max_hits == 0 or npass <= max_hits) and above == npass == wp and E == 0, ctx
                else:
                    assert npass > max_hits and T == s[max_hits - 1] and above == int((scores > T).sum()) and above + E == max_hits, ctx
                    assert 1 <= E <= int((scores == T).sum()), ctx


def test_radix_select_model_takes_bin_0():
    """the K-th score in bin 0 of the first pass (a biased key below 2^21) and in bin 0 of the second: the pick loop falls through"""
    for scores, k in ((search_ref.bin0_scores("top"), 900), (search_ref.bin0_scores("middle"), 900)):
        T, above, E = search_ref.radix_select_model(scores, search_ref.INT32_MIN, k)
        want, _ = search_ref.select(scores, search_ref.INT32_MIN, k, search_ref.BY_INDEX)
        assert search_ref.model_selection(scores, search_ref.INT32_MIN, k).tolist() == want.tolist() and above + E == k


def _header_struct(name):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    m = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (name, name), text, flags=re.S)
    assert m, name
    return m.group(1)


def _c_layout(body, known):
    """size of a C struct of int32_t / int64_t / known-struct members under natural alignment"""
    off, align = 0, 1
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        typ, names = decl.split(None, 1)
        size, al = {"int32_t": (4, 4), "int64_t": (8, 8)}.get(typ) or known[typ]
        for _ in names.split(","):
            off = (off + al - 1) // al * al + size
            align = max(align, al)
    return (off + align - 1) // align * align


def test_struct_layouts_match_the_header(pkg):
    known = {"pmx_record_t": (16, 4)}
    assert C.sizeof(pkg.pmx_record_t) == 16
    assert C.sizeof(pkg.pmx_search_opts_t) == _c_layout(_header_struct("pmx_search_opts"), known) == 24
    assert C.sizeof(pkg.pmx_hit_t) == _c_layout(_header_struct("pmx_hit"), known) == 40
    assert pkg.HIT_DTYPE.itemsize == 40
    for f in ("index", "first", "diag", "beg_query", "beg_ref", "reserved"):
        assert pkg.HIT_DTYPE.fields[f][1] == getattr(pkg.pmx_hit_t, f).offset
    assert [pkg.pmx_search_opts_t.min_score.offset, pkg.pmx_search_opts_t.max_hits.offset, pkg.pmx_search_opts_t.order.offset,
            pkg.pmx_search_opts_t.band.offset] == [0, 8, 16, 20]
    assert (pkg.HITS_BY_INDEX, pkg.HITS_BY_SCORE) == (0, 1)


def _search(pkg, cfg, prof, opts, n=1):
    rb = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    ro = np.array([0, 8], dtype=np.int64)
    res = C.POINTER(pkg.pmx_search_result_t)()
    rc = pkg.lib.pmx_search_profile(C.byref(cfg), prof, n, rb.ctypes.data, ro.ctypes.data, C.byref(opts) if opts is not None else None,
                                    C.byref(res))
    assert not res                                             # nothing is handed out on a refusal
    return rc, pkg.lib.pmx_last_error().decode()


def _search_device(pkg, cfg, prof, opts, capacity=4, cigar_capacity=64):
    # (the pointers are never followed: every case is refused before any GPU work)
    rc = pkg.lib.pmx_search_profile_device(C.byref(cfg), prof, 1, 256, 256, 8, C.byref(opts), None, 256, 256, 256, capacity,
                                           256, cigar_capacity, 256, 256, None)
    return rc, pkg.lib.pmx_last_error().decode()


def test_search_refusals_without_gpu(pkg):
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    prof = pkg.Profile.new(b"ACGTTGCA", False, pm)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_CIGAR, pm.inner)
    O = pkg.pmx_search_opts_t
    for entry in (_search, _search_device):
        rc, msg = entry(pkg, cfg, prof.inner, O(10, 0, 2, 48))
        assert rc == -1 and "order" in msg
        rc, msg = entry(pkg, cfg, prof.inner, O(10, 0, -1, 48))
        assert rc == -1 and "order" in msg
        rc, msg = entry(pkg, cfg, prof.inner, O(10, -1, 0, 48))
        assert rc == -1 and "max_hits" in msg
        rc, msg = entry(pkg, cfg, prof.inner, O(10, 0, 0, 64))
        assert rc == -1 and "63" in msg
        rc, msg = entry(pkg, cfg, None, O(10, 0, 0, 48))
        assert rc == -1 and "profile" in msg
        nowant = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_SORTED, pm.inner)
        rc, msg = entry(pkg, nowant, prof.inner, O(10, 0, 0, 48))
        assert rc == -1 and "PMX_WANT_CIGAR" in msg
        other = pkg.Matrix.create(b"ACGT", 1, -1)
        rc, msg = entry(pkg, pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_CIGAR, other.inner), prof.inner, O(10, 0, 0, 48))
        assert rc == -1 and "different matrix" in msg
    rc, msg = _search_device(pkg, cfg, prof.inner, O(10, 0, 0, 48), capacity=-1)
    assert rc == -1 and "capacity" in msg
    rc, msg = _search_device(pkg, cfg, prof.inner, O(10, 0, 0, 48), cigar_capacity=-1)
    assert rc == -1 and "capacity" in msg
    rc = pkg.lib.pmx_search_profile(C.byref(cfg), prof.inner, 1, None, None, None, None)
    assert rc == -1
    rc, msg = _search(pkg, cfg, prof.inner, None)
    assert rc == -1 and "options" in msg


def test_search_refuses_a_pssm_second_pass_without_gpu(pkg):
    values = np.arange(8 * 5, dtype=np.int32) % 7 - 3
    pssm = pkg.Matrix.create_pssm(b"ACGT", values.tolist(), 8)
    prof = pkg.Profile.new(b"ACGTTGCA", False, pssm)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_CIGAR, pssm.inner)
    for entry in (_search, _search_device):
        rc, msg = entry(pkg, cfg, prof.inner, pkg.pmx_search_opts_t(10, 0, 0, 0))
        assert rc == -1 and "PSSM" in msg


def test_select_and_gather_refusals_without_gpu(pkg):
    L = pkg.lib
    assert L.pmx_select_hits_device(256, 4, 0, 0, 2, 256, 4, 256, None) == -1 and b"order" in L.pmx_last_error()
    assert L.pmx_select_hits_device(256, 4, 0, -1, 0, 256, 4, 256, None) == -1
    assert L.pmx_select_hits_device(256, 4, 0, 0, 0, 256, -1, 256, None) == -1
    assert L.pmx_select_hits_device(256, 4, 0, 0, 0, 256, 4, None, None) == -1 and b"null" in L.pmx_last_error()
    assert L.pmx_select_hits_device(None, 4, 0, 0, 0, 256, 4, 256, None) == -1
    assert L.pmx_gather_refs_device(256, 256, 4, 256, -1, 256, 16, 256, None) == -1
    assert L.pmx_gather_refs_device(256, 256, 4, 256, 2, 256, 16, None, None) == -1 and b"null" in L.pmx_last_error()


def test_python_mirror_needs_a_profile(pkg):
    al = pkg.Aligner.new().local().build()
    with pytest.raises(pkg.NullProfile):
        al.search_profile([b"ACGT"], 5)
