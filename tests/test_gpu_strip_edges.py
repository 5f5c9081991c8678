"""What the strip kernels share around the recurrence (parasail-rs_amd/csrc/pmx_strip.h), at the smallest shapes
where it can go wrong, every case against the CPU oracle:

  A. the pair table's clamp and -1 index: a ragged last block.  n = 1, NP - 1, NP, NP + 1 pairs, NP the pairs per block of the
     family's 16-lane shape (32 lanes for the first-generation trace kernel).  Up to 64 pairs sw16, nwsg16v and stats16 run their
     64-lane latency shapes instead (2, 2 and 1 pairs per block: the same sizes are then several full blocks, or full blocks and
     one ragged one), so for these the sizes 64 + NP - 1, 64 + NP, 64 + NP + 1 follow, which the 16-lane shape takes; sw16m and
     nwsg16m run from 2 049 pairs on, so theirs are 2 048 + NP - 1, + NP, + NP + 1 only.  Ragged lengths 1 .. 40 with a query
     and a reference of one letter, in the given order and with lengths descending;
  B. the end rule and its ties: nw and all 16 free-end sets of sg over a corpus in which, by the oracle's last row and column,
     the last-row best ties the last-column best at another cell, the last column holds two equal maxima and so does the last row;
  C. what a boundary means in local alignment: a best alignment that starts in row 0 and one that starts in column 0, through the
     two kernels whose launchers once patched the flags for sw.

Each case asserts through pmx_last_kernel() that the intended family ran and skips, with the kernel that ran as the reason, otherwise."""
import numpy as np
import pytest

from util import random_seqs

pytestmark = pytest.mark.gpu

AA20 = b"ARNDCQEGHILKMFPSTWYV"          # (holds A, C, G, T: the DNA corpora score alike under both match / mismatch matrices)
OPEN, EXT = 5, 2

# family -> (environment switches, alphabet of the matrix, what is compared, NP: pairs per block of the 16-lane shape,
#            the batch size beyond which that shape (or the family at all) runs, kernel name prefix)
FAMILIES = {
    "sw16":     ({}, b"ACGT", "score", 8, 64, "pmx_sw16_kernel"),
    "sw16m":    ({"PMX_SW16_MATRIX_LOOKUP": "1"}, AA20, "score", 8, 2048, "pmx_sw16m_kernel"),
    "nwsg16":   ({"PMX_NWSG16_GEN1": "1"}, b"ACGT", "score", 8, 0, "pmx_nwsg16_kernel"),
    "nwsg16v":  ({}, b"ACGT", "score", 8, 64, "pmx_nwsg16v_kernel"),
    "nwsg16m":  ({}, AA20, "score", 8, 2048, "pmx_nwsg16m_kernel"),
    "stats16":  ({"PMX_STATS16_GEN1": "1", "PMX_NO_STATS_BY_TRACE": "1"}, b"ACGT", "stats", 4, 64, "pmx_stats16_kernel"),
    "stats16p": ({"PMX_STATS16P_ALWAYS": "1", "PMX_NO_STATS_BY_TRACE": "1"}, b"ACGT", "stats", 8, 0, "pmx_stats16p_kernel"),
    "trace1":   ({"PMX_TRACE16_GEN1": "1"}, b"ACGT", "cigar", 2, 0, "pmx_trace16_kernel"),      # (its smallest shape has 32 lanes per pair)
}
LOCAL = ("sw16", "sw16m")
GLOBAL = tuple(f for f in FAMILIES if f not in LOCAL)

_want = {}          # (mode, sg, q, r, what) -> the oracle's answer, computed once per distinct pair


def _oracle(orc, om, mode, sg, q, r, what):
    key = (mode, sg, q, r, what, om.size)
    if key not in _want:
        w = orc.align(mode, q, r, OPEN, EXT, om, sg_flags=orc.SG_ALL if sg is None else sg, stats=what == "stats", trace=what == "cigar")
        ans = (w.score, w.end_query, w.end_ref)
        if what == "stats":
            ans += (w.matches, w.similar, w.length)
        if what == "cigar":
            ans += (orc.cigar(w),)
        _want[key] = ans
    return _want[key]


def _run(pkg, orc, monkeypatch, family, mode, sg, qs, rs):
    """the batch through `family`, every pair against the oracle; skips when another kernel took it"""
    envs, alphabet, what, _, _, prefix = FAMILIES[family]
    for k, v in envs.items():
        monkeypatch.setenv(k, v)
    pm, om = pkg.Matrix.create(alphabet, 2, -3), orc.Matrix.create(alphabet.decode(), 2, -3)
    b = pkg.Aligner.new().matrix(pm).gap_open(OPEN).gap_extend(EXT).solution_width(16)
    [b.global_, b.semi_global, b.local][mode]()
    if what == "stats":
        b.use_stats()
    if what == "cigar":
        b.use_trace()
    al = b.build()
    if mode == 1 and sg is not None:
        al.sg_flags = sg        # (the builder's names cannot say "sg with no free end", and the kernels take all 16 sets)
    if what == "score":
        rec = al.align_batch(qs, rs)
        got = list(zip(rec["score"].tolist(), rec["end_query"].tolist(), rec["end_ref"].tolist()))
    elif what == "stats":
        rec, st = al.align_batch(qs, rs)
        got = list(zip(rec["score"].tolist(), rec["end_query"].tolist(), rec["end_ref"].tolist(),
                       st["matches"].tolist(), st["similar"].tolist(), st["length"].tolist()))
    else:
        rec, cig = al.align_batch_cigar(qs, rs)
        got = list(zip(rec["score"].tolist(), rec["end_query"].tolist(), rec["end_ref"].tolist(), list(cig)))
    kernel = pkg.lib.pmx_last_kernel().decode()
    if not kernel.startswith(prefix):
        pytest.skip("%s: %d pairs went to %s" % (family, len(qs), kernel))
    assert (rec["flags"] == 0).all()
    for k in range(len(qs)):
        want = _oracle(orc, om, mode, sg, qs[k], rs[k], what)
        assert got[k] == want, (family, kernel, mode, sg, len(qs), k, got[k], want, qs[k], rs[k])


def _sizes(family):
    _, _, _, NP, beyond, _ = FAMILIES[family]
    small = [] if beyond > 64 else [1, max(1, NP - 1), NP, NP + 1]           # (sw16m, nwsg16m: no batch this small reaches them)
    return sorted(set(small + ([beyond + NP - 1, beyond + NP, beyond + NP + 1] if beyond else [])))


def _ragged(n):
    """n pairs of 1 .. 40 letters; the second query and the third reference have one letter"""
    rng = np.random.default_rng(7100 + n)
    qs, rs = random_seqs(rng, n, 1, 40), random_seqs(rng, n, 1, 40)
    qs[1 % n] = qs[1 % n][:1]
    rs[2 % n] = rs[2 % n][:1]
    return qs, rs


@pytest.mark.parametrize("family", list(FAMILIES))
def test_ragged_last_block(pkg, orc, monkeypatch, family):
    for n in _sizes(family):
        qs, rs = _ragged(n)
        order = sorted(range(n), key=lambda k: -(len(qs[k]) + len(rs[k])))
        for idx in (range(n), order):                    # as given; lengths descending (a length-sorted order is then no identity)
            q2, r2 = [qs[k] for k in idx], [rs[k] for k in idx]
            _run(pkg, orc, monkeypatch, family, 2 if family in LOCAL else 1, None, q2, r2)
            if family not in LOCAL:
                _run(pkg, orc, monkeypatch, family, 0, None, q2, r2)


def tie_corpus(orc):
    """(queries, references, kinds): pairs of 4 .. 24 letters in which, by the oracle's last row and column under all free ends,
    (a) the last-row best equals the last-column best at another cell, (b) the last column holds two equal maxima,
    (c) the last row holds two equal maxima.  Every kind occurs, or the generator fails."""
    om = orc.Matrix.create("ACGT", 2, -3)
    rng = np.random.default_rng(7200)
    cand = [(b"A" * a, b"A" * b) for a, b in ((5, 8), (8, 5), (4, 24), (24, 4), (7, 9), (12, 11))]
    cand += [(b"ACGT" * 2, b"ACGT" * 4), (b"ACGT" * 5, b"ACGT" * 2), (b"GATTACA", b"GATTACAGATTACA"), (b"CCGGCCGG", b"GGCC")]
    cand += list(zip(random_seqs(rng, 6, 4, 24), random_seqs(rng, 6, 4, 24)))
    kinds = set()
    for q, r in cand:
        w = orc.align(orc.SG, q, r, OPEN, EXT, om, sg_flags=orc.SG_ALL, rowcol=True)
        row, col = w.score_row, w.score_col
        if row.max() == col.max() and (int(row.argmax()) != len(r) - 1 or int(col.argmax()) != len(q) - 1):
            kinds.add("a")
        if int((col == col.max()).sum()) >= 2:
            kinds.add("b")
        if int((row == row.max()).sum()) >= 2:
            kinds.add("c")
    assert kinds == {"a", "b", "c"}, kinds
    return [q for q, _ in cand], [r for _, r in cand], kinds


@pytest.mark.parametrize("family", GLOBAL)
def test_end_rule_and_ties(pkg, orc, monkeypatch, family):
    qs, rs, _ = tie_corpus(orc)
    _, _, _, NP, beyond, _ = FAMILIES[family]
    n = max(len(qs), beyond + NP + 1)                    # (tiled up to the batch size at which the family runs)
    qs, rs = [qs[k % len(qs)] for k in range(n)], [rs[k % len(rs)] for k in range(n)]
    _run(pkg, orc, monkeypatch, family, 0, None, qs, rs)
    for sg in range(16):
        _run(pkg, orc, monkeypatch, family, 1, sg, qs, rs)


@pytest.mark.parametrize("family", ["stats16", "trace1"])
def test_local_boundaries_are_free(pkg, orc, monkeypatch, family):
    """sw: neither H(i, -1) nor H(-1, j) is penalised -- an alignment that starts in row 0 or in column 0 scores its full length"""
    x = b"ACGTTGCAACGTAGGCTAAC"
    qs, rs = [x, b"TTTT" + x, x], [b"GGGG" + x, x, x]   # starts at row 0; at column 0; at both
    n = FAMILIES[family][4] + 3
    qs, rs = [qs[k % 3] for k in range(n)], [rs[k % 3] for k in range(n)]
    om = orc.Matrix.create("ACGT", 2, -3)
    for k in range(3):
        assert _oracle(orc, om, 2, None, qs[k], rs[k], "score")[0] == 2 * len(x)
    _run(pkg, orc, monkeypatch, family, 2, None, qs, rs)
