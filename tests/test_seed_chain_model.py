"""The chaining model (tests/seed_chain_ref.py) against its definitions, no GPU: f against exhaustion over every admissible
subsequence, the link rule one step either side of each bound, the three tie rules, the cost's values, the partition of the anchors
into chains, and the two planted properties that motivate chaining -- a long indel does not split a locus, two distant matches on one
diagonal do not merge."""
import numpy as np
import pytest

import seed_chain_ref as cref
import seed_ref as ref

K = 12
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rand(rng, n):
    return DNA[rng.integers(0, 4, size=n)].tobytes()


def _dp(anchors, k=K, band=100, max_gap=1000, lookback=64, gap_scale=38):
    f, pred = cref.scores(anchors, k, band, max_gap, lookback, gap_scale)
    assert (f, pred) == cref.scores_fast(anchors, k, band, max_gap, lookback, gap_scale)
    return f, pred


def test_f_is_the_best_over_every_admissible_subsequence():
    rng = np.random.default_rng(4100)
    linked = 0
    for trial in range(300):
        n = int(rng.integers(1, 10))
        cells = set()
        while len(cells) < n:
            cells.add((int(rng.integers(40)), int(rng.integers(40))))
        anchors = sorted(cells)
        k = int(rng.integers(3, 13))
        band, max_gap, scale = int(rng.integers(0, 30)), int(rng.integers(1, 45)), int(rng.choice([0, 38, 300, 3000]))
        f, pred = _dp(anchors, k, band, max_gap, n + int(rng.integers(0, 3)), scale)
        assert f == cref.brute_best(anchors, k, band, max_gap, n + 2, scale), (trial, anchors)
        linked += sum(p >= 0 for p in pred)
        for a, b in enumerate(pred):                                                         # pred attains f, strictly above k
            if b >= 0:
                assert cref.admissible(b, a, anchors, band, max_gap, n + 2) and f[a] == cref.link_value(f[b], b, a, anchors, k, scale) > k
            else:
                assert f[a] == k
    assert linked > 200                                                                      # (the sets are not trivial)


def test_lookback_1_links_only_the_adjacent_anchor():
    rng = np.random.default_rng(4101)
    diag = [(10 * x, 10 * x) for x in range(8)]                                             # one diagonal: every anchor links to the one before
    f, pred = _dp(diag, lookback=1)
    assert pred == [-1, 0, 1, 2, 3, 4, 5, 6] and f == [K + 10 * x for x in range(8)]
    # an anchor between two collinear ones (it links to neither) hides the first from the last
    gapped = [(0, 0), (5, 400), (10, 10)]
    assert _dp(gapped, lookback=1)[1] == [-1, -1, -1] and _dp(gapped, lookback=2)[1] == [-1, -1, 0]
    for trial in range(50):
        cells = sorted({(int(rng.integers(60)), int(rng.integers(60))) for _ in range(12)})
        _, pred = _dp(cells, lookback=1)
        assert all(p in (-1, a - 1) for a, p in enumerate(pred))


def test_chains_partition_the_anchors():
    rng = np.random.default_rng(4102)
    for trial in range(100):
        cells = sorted({(int(rng.integers(80)), int(rng.integers(80))) for _ in range(int(rng.integers(1, 40)))})
        f, pred = _dp(cells, k=int(rng.integers(3, 13)), band=int(rng.integers(0, 40)), max_gap=int(rng.integers(1, 60)), lookback=int(rng.integers(1, 12)))
        child = cref.children(f, pred)
        got = cref.chains(f, pred, child)
        members = sorted(x for m, _ in got for x in m)
        assert members == list(range(len(cells)))                                            # every anchor in exactly one chain
        assert [m[-1] for m, _ in got] == sorted(m[-1] for m, _ in got)
        for m, score in got:
            assert all(pred[y] == x and child[x] == y for x, y in zip(m, m[1:]))
            assert child[m[-1]] == -1 and (pred[m[0]] < 0 or child[pred[m[0]]] != m[0])
            assert score == f[m[-1]] - (f[pred[m[0]]] if pred[m[0]] >= 0 else 0)


# ---- the link rule, one step either side of every bound (anchors are (j, i)) ---------------------------------------------------------
BOUNDARIES = cref.BOUNDARIES


@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_link_rule_boundaries(name):
    anchors, opts, want = BOUNDARIES[name]
    assert anchors == sorted(anchors)
    f, pred = _dp(anchors, **opts)
    assert pred == want, (name, pred)
    assert [v > K for v in f] == [p >= 0 for p in want]


def test_a_repeat_would_tie_if_it_were_a_link():
    """the two repeat cases above decide something: the forbidden link's value equals the taken one's"""
    for anchors in (BOUNDARIES["dj = 0, di > 0"][0], BOUNDARIES["di = 0, dj > 0"][0]):
        f, _ = _dp(anchors)
        assert cref.link_value(f[1], 1, 2, anchors, K, 38) == f[2] == cref.link_value(f[0], 0, 2, anchors, K, 38)


# ---- ties ------------------------------------------------------------------------------------------------------------------------------
TIE_NEAREST, TIE_CHILD, TIE_AT_K = cref.TIE_NEAREST, cref.TIE_CHILD, cref.TIE_AT_K


def test_tie_rules():
    f, pred = _dp(TIE_NEAREST)
    assert pred == [-1, -1, 1] and f == [K, K, 2 * K - cref.cost(20, 38)]
    assert cref.link_value(f[0], 0, 2, TIE_NEAREST, K, 38) == cref.link_value(f[1], 1, 2, TIE_NEAREST, K, 38)
    f, pred = _dp(TIE_CHILD)
    assert pred == [-1, 0, 0] and f[1] == f[2] > K
    child = cref.children(f, pred)
    assert child == [1, -1, -1]
    assert cref.chains(f, pred, child) == [([0, 1], f[1]), ([2], f[2] - f[0])]
    f, pred = _dp(TIE_AT_K)
    assert cref.cost(64, 38) == K and pred == [-1, -1] and f == [K, K]
    assert _dp([(0, 0), (80, 20)])[1] == [-1, 0]                                              # g = 60 costs 11: one above k, linked


def test_cost_values():
    assert cref.cost(0, 38) == 0 and cref.cost(0, 65535) == 0
    assert [cref.cost(g, 38) for g in (1, 2, 3, 4)] == [0, 1, 1, 1]                           # 38 g >> 8 = 0; bit lengths 1, 2, 2, 3
    assert [cref.cost(g, 0) for g in (1, 2, 3, 4, 1 << 20)] == [0, 1, 1, 1, 10]
    assert cref.cost(1 << 20, 38) == (38 << 12) + 10
    assert [cref.cost(g, 65535) for g in (1, 2, 3, 4)] == [255, 512, 768, 1024]              # 255 + 0, 511 + 1, 767 + 1, 1023 + 1
    assert cref.cost(1 << 20, 65535) == ((65535 << 20) >> 8) + 10 < 1 << 28
    assert cref.cost((1 << 20) - 1, 65535) < 1 << 28


# ---- the planted properties ------------------------------------------------------------------------------------------------------------
def _only(res):
    return [(int(c["n_anchors"]), int(c["score"])) for c in res["chains"]]


def test_a_long_indel_is_one_chain_and_two_clusters():
    rng = np.random.default_rng(4204)           # (a seed whose insert does not prolong A or B by a letter: no k-mer across the junctions)
    A, B, ins = _rand(rng, 152), _rand(rng, 150), _rand(rng, 60)
    genome = _rand(rng, 300) + A + ins + B + _rand(rng, 300)
    read = A + B
    na, nb = len(A) - K + 1, len(B) - K + 1
    res = cref.seed_chains([read], [genome], K, strand=ref.FORWARD, band=100, fast=False)
    assert res["row_off"].tolist() == [0, 1]                                                  # ONE chain ...
    c = res["chains"][0]
    assert c["n_anchors"] == na + nb == 280                                                  # ... of both halves' anchors
    assert (c["q_beg"], c["q_end"], c["r_beg"], c["r_end"]) == (0, len(read), 300, 300 + len(read) + 60)
    assert (c["diag_min"], c["diag_max"]) == (300, 360)
    assert c["score"] == K + (na - 1) + K - cref.cost(60, 38) + (nb - 1)
    assert res["pairs"][0].tolist() == (0, 0, 0, -1, 300 - 16, 360 + len(read) + 16 - (300 - 16))
    two = ref.seed([read], [genome], K, ref.FORWARD, 2, 8, 16, 64)                            # the cluster road at band 8: two candidates
    assert [tuple(s) for s in two["seeds"].tolist()] == [(na, 300, 300, 0), (nb, 360, 360, 0)]
    # a band below the indel's length splits the chain as well: the bound is the link's
    assert sorted(n for n, _ in _only(cref.seed_chains([read], [genome], K, strand=ref.FORWARD, band=59))) == [nb, na]


def test_two_distant_matches_on_one_diagonal_are_one_cluster_and_two_chains():
    rng = np.random.default_rng(4201)
    A, B = _rand(rng, 152), _rand(rng, 150)
    genome = _rand(rng, 300) + A + _rand(rng, 2000) + B + _rand(rng, 300)
    read = A + _rand(rng, 2000) + B
    na, nb = len(A) - K + 1, len(B) - K + 1
    one = ref.seed([read], [genome], K, ref.FORWARD, 2, 8, 16, 64)
    assert [tuple(s) for s in one["seeds"].tolist()] == [(na + nb, 300, 300, 0)]              # ONE cluster of 280 seeds
    near = cref.seed_chains([read], [genome], K, strand=ref.FORWARD, band=100, max_gap=1000)
    assert _only(near) == [(na, K + na - 1), (nb, K + nb - 1)]                                # two chains at max_gap 1 000
    assert [(c["q_beg"], c["q_end"]) for c in near["chains"]] == [(0, 152), (2152, 2302)]
    far = cref.seed_chains([read], [genome], K, strand=ref.FORWARD, band=100, max_gap=5000)
    assert _only(far) == [(na + nb, K + na - 1 + K + nb - 1)]                                 # one at 5 000: the step of 2 012 costs nothing on the diagonal
