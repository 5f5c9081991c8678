"""The first bad pair of an enumerated window (`-m gpu`: SeqSet.new uploads): every host entry that enumerates -- pmx_align_all_pairs,
pmx_search_pairs[_stranded] with TRIANGLE and RECT, pmx_search_topk[_stranded] -- over sets with an empty sequence, against the brute
force of tests/set_search_ref.py.  They share one row-by-row walk, so for the same set and window they name the same pair in the same
words: "pair P (i, j): side: empty window", P counted from the window's first pair, the query checked before the reference, the row's
first empty column reported.  A window that meets no empty sequence runs, and gives what the set without holes gives."""
import ctypes as C

import pytest

import set_search_ref as ref

pytestmark = pytest.mark.gpu

TRI, RECT = ref.PAIRS_TRIANGLE, ref.PAIRS_RECT
N = 12
BASE = [bytes(b"ACGT"[(7 * k + 3 * x + x * x // 5) % 4] for x in range(8 + (3 * k) % 13)) for k in range(N)]       # 8 .. 20 bases
# (first, count) per set of holes.  Triangle -- sequence 0 is only ever a query, sequence 11 only ever a reference: a window from a row
# start; from mid-row before the empty column; from mid-row behind it, so that a later row reports; of one pair; one that ends a pair
# before the first bad pair (it runs).  Rows start at 0, 11, 21, 30, 38, 45, 51, 56, 60, 63, 65.
TRI_WINDOWS = {
    (0,): [(0, 66), (4, 20), (10, 1), (11, 55)],
    (5,): [(11, 30), (22, 20), (24, 20), (31, 1), (24, 7), (39, 20)],
    (11,): [(0, 66), (13, 30), (65, 1), (11, 9)],
    (5, 9): [(21, 40), (24, 30), (28, 30), (60, 1), (24, 3), (61, 5)],
}
# Rectangle 12 x 12, pair p = 12 i + j, the holed set as Q, as R and as both: the same kinds of window around the empty column (R) and
# the empty row (Q).
RECT_WINDOWS = {
    (0,): [(12, 30), (13, 30), (24, 1), (13, 11), (0, 20), (5, 3), (12, 132), (11, 2)],
    (5,): [(12, 60), (14, 40), (19, 40), (29, 1), (19, 10), (48, 40), (50, 40), (63, 5), (60, 1), (48, 12), (72, 72), (54, 30), (65, 1), (54, 6)],
    (11,): [(12, 30), (20, 30), (23, 1), (12, 11), (120, 24), (125, 10), (135, 2), (120, 12), (132, 3)],
    (5, 9): [(12, 60), (18, 40), (22, 40), (21, 1), (18, 3), (22, 7), (48, 40), (72, 60), (72, 36), (110, 1), (54, 30), (58, 10)],
}
ROWS = [(0, 12), (1, 3), (4, 2), (6, 3), (10, 2)]                # whole rows: the rectangle's window and the top-K entry's rows
# worked by hand from the numbering, so that the reference is not the only witness
ANCHORS = {
    (TRI, (5,), "both", 24, 20): "pair 7 (3, 5): reference: empty window",
    (TRI, (5,), "both", 39, 20): "pair 6 (5, 6): query: empty window",
    (TRI, (11,), "both", 0, 66): "pair 10 (0, 11): reference: empty window",
    (RECT, (5, 9), "R", 18, 40): "pair 3 (1, 9): reference: empty window",
    (RECT, (5, 9), "both", 58, 10): "pair 2 (5, 0): query: empty window",
    (RECT, (0,), "Q", 11, 2): "pair 0 (0, 11): query: empty window",
    (RECT, (0,), "R", 11, 2): "pair 1 (1, 0): reference: empty window",
}


def _expected(shape, qseqs, rseqs, first, count):
    bad = ref.first_empty_pair(shape, [len(s) for s in qseqs], [len(s) for s in rseqs], first, count)
    return None if bad is None else "pair %d (%d, %d): %s: empty window" % bad


def _outcome(pkg, call):
    """(result, None), or (None, the BatchError's text)"""
    try:
        return call(), None
    except pkg.BatchError as e:
        return None, str(e)


def _pairs_entries(pkg, al, cfg, Q, R, shape, first, count):
    """{entry: outcome} of pmx_search_pairs through the Python mirror and of pmx_search_pairs_stranded itself in the three modes (the
    mirror sends mode 0 to the plain entry)"""
    out = {"plain": _outcome(pkg, lambda: al.search_pairs(Q, R, min_score=0, first=first, count=count))}
    o = pkg.pmx_pair_search_opts_t(0, shape, 0, 0, 0)
    for mode in (0, 1, 2):
        args = (C.byref(cfg), Q.inner, R.inner if R is not None else None, first, count, None, C.byref(o), mode)
        out[mode] = _outcome(pkg, lambda: pkg._hits_call(pkg.lib.pmx_search_pairs_stranded, args, pkg.pmx_strand_hits_t, pkg.PairHits,
                                                         pkg.lib.pmx_strand_hits_free))
    return out


def _topk_entries(pkg, al, cfg, Q, R, row, rows):
    out = {"plain": _outcome(pkg, lambda: al.search_topk(Q, R, k=3, min_score=0, first_row=row, rows=rows))}
    o = pkg.pmx_topk_opts_t(0, 3, 0, 0, 0)
    for mode in (0, 1, 2):
        args = (C.byref(cfg), Q.inner, R.inner, row, rows, C.byref(o), mode)
        out[mode] = _outcome(pkg, lambda: pkg._hits_call(pkg.lib.pmx_search_topk_stranded, args, pkg.pmx_topk_strand_hits_t, pkg.TopKHits,
                                                         pkg.lib.pmx_topk_strand_hits_free))
    return out


def _same_hits(a, b):
    assert a.n_hits == b.n_hits and a.n_passing == b.n_passing
    assert a.index.tolist() == b.index.tolist() and a.records.tobytes() == b.records.tobytes() and a.pairs.tobytes() == b.pairs.tobytes()
    assert a.strand.tolist() == b.strand.tolist()
    if hasattr(a, "row_off"):
        assert a.row_off.tolist() == b.row_off.tolist() and a.row_passing.tolist() == b.row_passing.tolist()


def test_first_bad_pair_of_enumerated_windows(pkg):
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    assert sorted({len(s) for s in BASE})[0] == 8 and max(len(s) for s in BASE) == 20
    S = pkg.SeqSet.new(BASE)
    whole = {}                                                   # what the set without holes gives, per call

    def against_whole(key, outcomes, base_call):
        """a window that runs: every entry's hits equal those of the same call over the set without holes"""
        if key not in whole:
            whole[key] = base_call()
        for entry, (got, text) in outcomes.items():
            assert text is None, (key, entry, text)
            _same_hits(got, whole[key][entry][0])

    seen = set()
    for holes in TRI_WINDOWS:
        seqs = [b"" if k in holes else s for k, s in enumerate(BASE)]
        H = pkg.SeqSet.new(seqs)
        ran = 0
        for first, count in TRI_WINDOWS[holes]:
            want = _expected(TRI, seqs, seqs, first, count)
            assert want == ANCHORS.get((TRI, holes, "both", first, count), want)
            seen.add((TRI, holes, "both", first, count))
            rec, text = _outcome(pkg, lambda: al.align_all_pairs(H, first, count))
            assert text == want, (holes, first, count, text, want)
            outcomes = _pairs_entries(pkg, al, cfg, H, None, TRI, first, count)
            if want is None:
                ran += 1
                assert rec.tobytes() == al.align_all_pairs(S, first, count).tobytes()
                against_whole((TRI, first, count), outcomes, lambda: _pairs_entries(pkg, al, cfg, S, None, TRI, first, count))
            else:
                assert {e: t for e, (_, t) in outcomes.items()} == dict.fromkeys(outcomes, want), (holes, first, count, want)
        assert ran >= 1
        for side, Q, R, qs, rs in (("Q", H, S, seqs, BASE), ("R", S, H, BASE, seqs), ("both", H, H, seqs, seqs)):
            ran = 0
            for first, count in RECT_WINDOWS[holes]:
                want = _expected(RECT, qs, rs, first, count)
                assert want == ANCHORS.get((RECT, holes, side, first, count), want)
                seen.add((RECT, holes, side, first, count))
                outcomes = _pairs_entries(pkg, al, cfg, Q, R, RECT, first, count)
                if want is None:
                    ran += 1
                    against_whole((RECT, first, count), outcomes, lambda: _pairs_entries(pkg, al, cfg, S, S, RECT, first, count))
                else:
                    assert {e: t for e, (_, t) in outcomes.items()} == dict.fromkeys(outcomes, want), (holes, side, first, count, want)
            assert ran >= 1
            for row, rows in ROWS:                                # whole rows: the rectangle's text is the top-K entry's
                want = _expected(RECT, qs, rs, row * N, rows * N)
                pairs_out = _pairs_entries(pkg, al, cfg, Q, R, RECT, row * N, rows * N)
                topk_out = _topk_entries(pkg, al, cfg, Q, R, row, rows)
                assert {e: t for e, (_, t) in pairs_out.items()} == dict.fromkeys(pairs_out, want), (holes, side, row, rows, want)
                assert {e: t for e, (_, t) in topk_out.items()} == dict.fromkeys(topk_out, want), (holes, side, row, rows, want)
                if want is None:
                    against_whole(("topk", row, rows), topk_out, lambda: _topk_entries(pkg, al, cfg, S, S, row, rows))
    assert set(ANCHORS) <= seen
