"""CPU tier of the record-level top-K hook (pmx_topk_records_device): the symbol, its declaration and Python mirror, every refusal (none
follows a pointer), and the models: topk_ref.topk's one-sort form against the row-by-row cut, and the chunked running merge against both
on small versions of the score patterns tests/test_gpu_topk_records.py feeds the kernels."""
import re
import os

import numpy as np

import topk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX, INT32_MIN = ref.INT32_MAX, ref.INT32_MIN
EDGE_SCORES = np.array([INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX], dtype=np.int64)


def test_symbol_is_exported_and_declared_as_a_test_hook(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    assert hasattr(pkg.lib, "pmx_topk_records_device") and hasattr(pkg, "topk_records_device")
    decl = text.index("int pmx_topk_records_device(")
    comment = text.rindex("/*", 0, decl)
    assert text[comment:].startswith("/* Test hook")
    m = re.search(r"#define PMX_TOPK_RECORDS_CHUNK \(\(int64_t\)1 << (\d+)\)", text)
    assert m and int(m.group(1)) <= 26


def test_refusals_without_gpu(pkg):
    L = pkg.lib
    err = lambda: L.pmx_last_error().decode()

    def hook(rec=256, st=None, first=0, nq=4, nr=10, ms=0, k=5, skip=0, chunk=0, marked=0, sb=None, hp=256, hi=256, hr=256, hs=None, cap=16,
             off=256, rp=256, cnt=256):
        return L.pmx_topk_records_device(rec, st, first, nq, nr, ms, k, skip, chunk, marked, sb, hp, hi, hr, hs, cap, off, rp, cnt, None)

    assert hook(k=0) == -1 and "k 0 is outside 1 .. 1024" in err()
    assert hook(k=-3) == -1 and "outside 1 .. 1024" in err()
    assert hook(k=1025) == -1 and "outside 1 .. 1024" in err()
    assert hook(nq=-1) == -1 and "negative" in err()
    assert hook(nr=-1) == -1 and "negative" in err()
    assert hook(first=-1) == -1 and "negative" in err()
    assert hook(nr=1 << 31) == -1 and "2^31 - 1" in err()
    assert hook(nq=1 << 40, nr=1 << 30) == -1 and "overflow" in err()
    assert hook(first=1 << 40, nq=1, nr=1 << 30) == -1 and "overflow" in err()               # the absolute index of the last pair
    assert hook(first=(1 << 63) - 1, nq=2, nr=1) == -1 and "overflow" in err()
    assert hook(rec=None) == -1 and "null records" in err()
    assert hook(off=None) == -1 and "null row offsets" in err()
    assert hook(cnt=None) == -1 and "null counts" in err()
    assert hook(cap=-1) == -1 and "negative capacity" in err()
    assert hook(chunk=-1) == -1 and "chunk_pairs" in err()
    assert hook(hr=None) == -1 and "null hit records" in err()
    assert hook(hs=256) == -1 and "hit statistics without statistics" in err()
    for bad in (dict(rec=None), dict(off=None), dict(cnt=None), dict(k=0)):                   # ... with no rows or no columns too
        assert hook(nq=0, **bad) == -1 and hook(nr=0, **bad) == -1


def patterns(rng, nq, nr):
    """small versions of the GPU tests' scores, [nq, nr] int64"""
    j = np.tile(np.arange(nr, dtype=np.int64), (nq, 1))
    step = (1 << 32) // max(nr, 1) - 1
    runs = rng.integers(1, 6, size=nq * nr)
    yield "uniform", rng.integers(INT32_MIN, INT32_MAX + 1, size=(nq, nr), dtype=np.int64)
    yield "ascending", INT32_MIN + step * j
    yield "descending", INT32_MAX - step * j
    yield "equal", np.full((nq, nr), INT32_MAX, dtype=np.int64)
    yield "lowest", np.full((nq, nr), INT32_MIN, dtype=np.int64)
    yield "saw-tooth", (j % 9) * 1000 + j // 9
    yield "edges", np.repeat(EDGE_SCORES[rng.integers(0, 7, size=nq * nr)], runs)[:nq * nr].reshape(nq, nr)


def test_one_sort_reference_equals_the_row_by_row_cut():
    rng = np.random.default_rng(1200)
    for nq, nr, q_first in ((3, 1, 0), (5, 3, 1), (4, 70, 68), (3, 257, 0), (0, 5, 0), (3, 0, 0)):
        for name, scores in patterns(rng, nq, nr):
            rec = np.zeros((nq * nr, 4), dtype=np.int32)
            rec[:, 0] = scores.reshape(-1)
            rec[:, 1] = np.arange(nq * nr)
            st = rng.integers(0, 100, size=(nq * nr, 3)).astype(np.int32)
            for k in sorted({1, 2, max(nr, 1), nr + 3, 1024}):
                for ms in (INT32_MIN, 0, INT32_MAX):
                    for skip in (False, True):
                        w = ref.topk(rec, nr, q_first, nq, k, ms, skip, stats=st)
                        keep, row_off, row_passing = ref.topk_by_rows(rec, nr, q_first, nq, k, ms, skip)
                        ctx = (name, nq, nr, q_first, k, ms, skip)
                        assert w["row_off"].tolist() == row_off and w["row_passing"].tolist() == row_passing, ctx
                        assert (w["index"] - q_first * nr).tolist() == keep and w["records"][:, 1].tolist() == keep, ctx
                        assert w["stats"].tobytes() == st[keep].tobytes() and w["counts"] == [len(keep), len(keep), sum(row_passing)], ctx
                        assert w["pairs"]["q"].tolist() == [q_first + p // nr for p in keep] and w["pairs"]["r"].tolist() == [p % nr for p in keep]
                        cut = ref.topk(rec, nr, q_first, nq, k, ms, skip, stats=st, capacity=len(keep) // 2)
                        assert cut["index"].tolist() == w["index"][:len(keep) // 2].tolist() and cut["counts"][:2] == [len(keep), len(keep) // 2]
                        assert cut["row_off"].tolist() == row_off


def test_chunked_merge_equals_the_cut_on_the_record_patterns():
    """the running merge's two chunk-order facts hold at the ends of int32 as they do for alignment scores"""
    rng = np.random.default_rng(1210)
    for nq, nr, q_first in ((3, 1, 0), (3, 3, 1), (3, 70, 67)):
        for name, scores in patterns(rng, nq, nr):
            flat = scores.reshape(-1)
            rec = np.zeros((nq * nr, 4), dtype=np.int32)
            rec[:, 0] = flat
            for k in sorted({1, 2, 5, max(nr, 1), nr + 3}):
                for ms, skip in ((INT32_MIN, False), (0, False), (INT32_MAX, False), (INT32_MIN, True)):
                    w = ref.topk(rec, nr, q_first, nq, k, ms, skip)
                    rows = [(w["index"][w["row_off"][li]:w["row_off"][li + 1]] - (q_first + li) * nr).tolist() for li in range(nq)]
                    for chunk in sorted({1, 7, 64, max(nr, 1), nr + 1, 3 * nr - 1} - {0}):
                        got, passing = ref.chunked_rows(flat, nr, k, chunk, ms, skip, q_first)
                        assert got == rows and passing == w["row_passing"].tolist(), (name, nq, nr, q_first, k, ms, skip, chunk)
