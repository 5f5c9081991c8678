"""Seed chaining (`-m gpu`): pmx_seed_chains[_device] byte for byte against tests/seed_chain_ref.py -- at the segment sizes and
lookbacks where the chain kernel's rounds of 64, its ring and its look-ahead change shape, across reference changes inside a window,
on the planted boundary and tie cases of the model test, on repeats, under slices, tiny match buffers and capacities -- and the two
planted properties end to end through the ungapped filter and the extension.  Every output buffer starts as a sentinel."""
import numpy as np
import pytest

import seed_chain_ref as cref
import seed_ref as ref
from util import random_seqs, mutate

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
KEYS = ("pairs", "strand", "seeds", "chains")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device=_dev())


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize()


def _rand(rng, n):
    return DNA[rng.integers(0, 4, size=n)].tobytes()


class Got:
    pass


def _chain(pkg, Q, ix, nq, mq, capacity, q_first=0, seeds=True, chains=True, **kw):
    import torch
    slots = capacity + 3
    hp = _full((slots * 32,), FILL, torch.uint8)
    hs = _full((slots,), FILL, torch.uint8)
    hd = _full((slots, 4), SENTINEL, torch.int32)
    hc = _full((slots, 8), SENTINEL, torch.int32)
    off = _full((nq + 1 + 2,), SENTINEL, torch.int64)
    cnt = _full((2 + 2,), SENTINEL, torch.int64)
    pkg.seed_chains_device(Q, ix, q_first, nq, mq, hp.data_ptr(), hs.data_ptr(), hd.data_ptr() if seeds else None, hc.data_ptr() if chains else None,
                           capacity, off.data_ptr(), cnt.data_ptr(), stream=_stream(), **kw)
    _sync()
    g = Got()
    g.pairs, g.strand, g.off, g.counts = hp.cpu().numpy().view(ref.PAIR_DTYPE), hs.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy()
    g.seeds = hd.cpu().numpy().reshape(-1).view(ref.SEED_HIT_DTYPE)
    g.chains = hc.cpu().numpy().reshape(-1).view(cref.CHAIN_DTYPE)
    return g


def _same(g, want, capacity, nq, seeds=True, chains=True):
    """row_off and counts in full and uncapped, the first min(candidates, capacity) entries the model's bytes, every entry at or behind
    `capacity` -- and an optional output that was not given -- the sentinel"""
    total = int(want["row_off"][-1])
    w = min(total, capacity)
    assert g.off[:nq + 1].tolist() == want["row_off"].tolist() and (g.off[nq + 1:] == SENTINEL).all()
    assert g.counts[:2].tolist() == [total, w] and (g.counts[2:] == SENTINEL).all()
    assert g.pairs[:w].tobytes() == want["pairs"][:w].tobytes() and (g.pairs[w:].view(np.uint8) == FILL).all()
    assert g.strand[:w].tobytes() == want["strand"][:w].tobytes() and (g.strand[w:] == FILL).all()
    ws, wc = (w if seeds else 0), (w if chains else 0)
    assert g.seeds[:ws].tobytes() == want["seeds"][:ws].tobytes() and (g.seeds[ws:].view(np.int32) == SENTINEL).all()
    if g.chains[:wc].tobytes() != want["chains"][:wc].tobytes():
        bad = [x for x in range(wc) if g.chains[x] != want["chains"][x]]
        raise AssertionError((len(bad), bad[:3], g.chains[bad[0]], want["chains"][bad[0]], want["pairs"][bad[0]]))
    assert (g.chains[wc:].view(np.int32) == SENTINEL).all()


def _check(pkg, queries, refs, k, mq=None, w=1, strand=ref.BOTH, **opts):
    """one run with room for everything against the model; returns the model's result"""
    mq = max(1, max(len(s) for s in queries)) if mq is None else mq
    want = cref.seed_chains(queries, refs, k, w=w, strand=strand, max_qlen=mq, **opts)
    Q, R = pkg.SeqSet.new(queries), pkg.SeqSet.new(refs)
    ix = pkg.SeedIndex.build(R, k, stream=_stream(), w=w)
    total = int(want["row_off"][-1])
    _same(_chain(pkg, Q, ix, len(queries), mq, total + 2, strand=strand, **opts), want, total + 2, len(queries))
    return want


# ---- segment sizes and lookbacks -------------------------------------------------------------------------------------------------------
def test_segment_sizes_around_the_rounds_of_64(pkg):
    """a read of n + k - 1 letters cut from the reference has n anchors on one diagonal: n = 0, 1, 2, 63, 64, 65, 129"""
    rng = np.random.default_rng(5000)
    k = 12
    genome = _rand(rng, 3000)
    sizes = (0, 1, 2, 63, 64, 65, 129)
    rows = []
    for x, n in enumerate(sizes):
        s = genome[200 * x + 7:200 * x + 7 + n + k - 1] if n else _rand(rng, 40)
        rows.append(ref.orient(s, x & 1))
    idx = ref.index_dict([genome], k)
    for x, n in enumerate(sizes):
        got = cref.anchors_of(rows[x], x & 1, idx, k, 64)
        assert sum(len(v) for v in got.values()) == n and not cref.anchors_of(rows[x], 1 - (x & 1), idx, k, 64)
    for min_seeds in (1, 2):
        want = _check(pkg, rows, [genome], k, min_seeds=min_seeds, band=20, max_gap=100, lookback=64)
        assert np.diff(want["row_off"]).tolist() == [0, 1 if min_seeds == 1 else 0, 1, 1, 1, 1, 1]
        assert want["chains"]["n_anchors"].tolist()[-5:] == [2, 63, 64, 65, 129]
        assert want["chains"]["score"].tolist()[-5:] == [k + n - 1 for n in (2, 63, 64, 65, 129)]


@pytest.mark.parametrize("lookback", [64, 1024])
def test_a_5_kb_row_against_itself(pkg, lookback):
    """about 5 000 anchors in one segment: the row itself and a copy with substitutions and indels, against the row as a reference"""
    rng = np.random.default_rng(5001)
    k = 12
    row = _rand(rng, 5011)
    other = mutate(rng, row, sub=0.04, indel=0.01)[:5011]
    want = _check(pkg, [row, other], [row, _rand(rng, 500)], k, min_seeds=3, band=50, max_gap=500, lookback=lookback, max_occ=8)
    best = want["chains"][np.argmax(want["chains"]["n_anchors"])]
    assert best["n_anchors"] == 5000 and best["score"] == k + 4999 and (best["q_beg"], best["q_end"]) == (0, 5011)
    a, b = int(want["row_off"][1]), int(want["row_off"][2])
    assert b - a >= 1 and want["chains"]["n_anchors"][a:b].max() > 1000                        # the copy chains across its indels


@pytest.fixture(scope="module")
def dense():
    """reads over a tandem repeat (unit 7, k 12: seven k-mers with some forty entries each): thousands of anchors per segment, many
    with equal j or equal i inside one window"""
    rng = np.random.default_rng(5002)
    unit = _rand(rng, 7)
    refs = [_rand(rng, 200) + unit * 40 + _rand(rng, 200), _rand(rng, 300), _rand(rng, 150) + unit * 6 + _rand(rng, 100)]
    reads = [refs[0][130:330], ref.orient(refs[0][380:560], 1), refs[2][100:260]]
    return refs, reads


@pytest.mark.parametrize("lookback", [1, 2, 63, 64, 65, 200, 1024])
def test_lookbacks(pkg, dense, lookback):
    refs, reads = dense
    want = _check(pkg, reads, refs, 12, min_seeds=2, band=60, max_gap=300, lookback=lookback, max_occ=64)
    assert len(want["pairs"]) >= (100 if lookback >= 63 else 1)                                # (at 1 and 2 the repeat's anchors reach nothing)
    n = sum(len(v) for q in reads for s in (0, 1) for v in cref.anchors_of(q, s, ref.index_dict(refs, 12), 12, 64).values())
    assert n > 5000


def test_a_reference_change_inside_the_window_empties_it(pkg):
    """short references that continue one another along the read: were the window not emptied at a change of r, the first anchor of
    reference x + 1 (j = i = 40 (x + 1)) would link to the last of reference x (j = i = 40 x + 28) and carry its score on"""
    rng = np.random.default_rng(5003)
    k = 12
    read = _rand(rng, 250)
    other = bytes.maketrans(b"ACGT", b"CGTA")
    refs = [read[:40]]                                                                       # 29 anchors each, fewer than the lookback
    refs += [_rand(rng, 40 * x - 1) + read[40 * x - 1:40 * x].translate(other) + read[40 * x:40 * x + 40] for x in range(1, 6)]
    idx = ref.index_dict(refs, k)
    got = cref.anchors_of(read, 0, idx, k, 64)
    assert sorted(got) == list(range(6)) and all(got[x] == [(40 * x + y, 40 * x + y) for y in range(29)] for x in range(6))
    for lookback in (64, 200):
        want = _check(pkg, [read, ref.orient(read, 1)], refs, k, min_seeds=1, band=20, max_gap=100, lookback=lookback)
        assert want["chains"]["score"].tolist() == [k + 28] * 12 and want["chains"]["n_anchors"].tolist() == [29] * 12
        assert want["pairs"]["r"].tolist() == list(range(6)) * 2 and want["strand"].tolist() == [0] * 6 + [1] * 6


# ---- the planted boundary and tie cases ------------------------------------------------------------------------------------------------
def test_link_rule_boundaries_and_ties_as_sequences(pkg):
    rng = np.random.default_rng(5004)
    k = cref.PLANT_K
    cases = [(name, a, o) for name, (a, o, _) in sorted(cref.BOUNDARIES.items())]
    cases += [("nearest", cref.TIE_NEAREST, {}), ("child", cref.TIE_CHILD, {}), ("at k", cref.TIE_AT_K, {})]
    reads, refs = zip(*(cref.plant(rng, a, k) for _, a, _ in cases))
    Q, R = pkg.SeqSet.new(list(reads)), pkg.SeqSet.new(list(refs))
    ix = pkg.SeedIndex.build(R, k, stream=_stream())
    mq = max(len(s) for s in reads)
    for x, (name, anchors, o) in enumerate(cases):
        opts = dict(cref.PLANT_OPTS, min_seeds=1, pad=3, max_occ=64)
        opts.update(o)
        want = cref.seed_chains(list(reads), list(refs), k, strand=ref.FORWARD, q_first=x, nq=1, fast=False, **opts)
        total = int(want["row_off"][-1])
        _same(_chain(pkg, Q, ix, 1, mq, total + 1, q_first=x, strand=ref.FORWARD, **opts), want, total + 1, 1)
        mine = [c for c, p in zip(want["chains"], want["pairs"]) if p["r"] == x]
        f, pred = cref.scores(sorted(anchors), k, opts["band"], opts["max_gap"], opts["lookback"], opts["gap_scale"])
        assert sorted(c["n_anchors"] for c in mine) == sorted(len(m) for m, _ in cref.chains(f, pred, cref.children(f, pred))), name
    # what the three tie cases look like in the output
    x = len(cases) - 3
    opts = dict(cref.PLANT_OPTS, min_seeds=1, pad=3, max_occ=64)
    near = _chain(pkg, Q, ix, 1, mq, 8, q_first=x, strand=ref.FORWARD, **opts)
    mine = [c for c, p in zip(near.chains[:int(near.counts[1])], near.pairs) if p["r"] == x]
    assert [(c["n_anchors"], c["r_beg"], c["q_beg"]) for c in mine] == [(1, 0, 20), (2, 20, 0)]   # (20, 0) -- the nearer -- carries (60, 60)
    child = _chain(pkg, Q, ix, 1, mq, 8, q_first=x + 1, strand=ref.FORWARD, **opts)
    mine = [c for c, p in zip(child.chains[:int(child.counts[1])], child.pairs) if p["r"] == x + 1]
    assert [(c["n_anchors"], c["r_end"], c["score"]) for c in mine] == [(2, 30 + k, 2 * k - cref.cost(20, 38)), (1, 50 + k, k - cref.cost(20, 38))]
    at_k = _chain(pkg, Q, ix, 1, mq, 8, q_first=x + 2, strand=ref.FORWARD, **opts)
    mine = [c for c, p in zip(at_k.chains[:int(at_k.counts[1])], at_k.pairs) if p["r"] == x + 2]
    assert [(c["n_anchors"], c["score"]) for c in mine] == [(1, k), (1, k)]


def test_repeats_on_both_strands_and_max_occ(pkg):
    """homopolymer and dinucleotide rows: every anchor shares its j or its i with many others.  A12 has 89 entries: max_occ 89 keeps
    them, 88 drops them all"""
    rng = np.random.default_rng(5005)
    k = 12
    refs = [_rand(rng, 50) + b"A" * 100 + _rand(rng, 50), b"CA" * 60, _rand(rng, 30) + b"ACG" * 40 + _rand(rng, 20)]
    rows = [b"A" * 80, b"AC" * 40, b"T" * 50, b"ACG" * 30, b"GT" * 33 + b"G"]
    seen = []
    for max_occ, lookback in ((89, 64), (89, 200), (88, 200)):
        want = _check(pkg, rows, refs, k, min_seeds=2, band=30, max_gap=200, lookback=lookback, max_occ=max_occ)
        seen.append(np.diff(want["row_off"]).tolist())
    # the A-row has 69 k-mers: between (j, i) and any (j - 1, i' < i) lie 69 + i - i' > 64 anchors, so a lookback of 64 links nothing
    # there and one of 200 does; the T-row (strand 1) has 39 and chains at 64
    assert seen[0][0] == 0 and seen[1][0] > 0 and seen[0][2] > 0 and seen[2][0] == 0 and seen[2][2] == 0
    assert seen[2][1] == seen[1][1] > 0 and seen[0][4] > 0


# ---- a medium set: letters, lengths, strands, slices, budgets, capacity ----------------------------------------------------------------
K_MED, OPTS_MED = 13, dict(min_seeds=2, min_score=20, band=40, max_gap=200, lookback=64, gap_scale=38, pad=12, max_occ=24)


@pytest.fixture(scope="module")
def medium():
    rng = np.random.default_rng(5100)
    refs = random_seqs(rng, 24, 1500, 3000)
    unit = _rand(rng, 9)
    refs[7] = refs[7][:800] + unit * 60 + refs[7][800:]                                     # a tandem repeat
    reads = []
    for x in range(300):
        r = int(rng.integers(24)) if x % 25 else 7
        a = int(rng.integers(0, len(refs[r]) - 170)) if x % 25 else int(rng.integers(700, 1300))
        piece = refs[r][a:a + 170]
        if x % 3 == 0:
            piece = piece[:70] + piece[70 + 15:]                                             # a deletion of 15: two diagonals, one chain
        s = mutate(rng, piece, sub=0.02, indel=0.005)[:150]
        reads.append(ref.orient(s, x & 1))
    reads[5] = reads[5][:40] + b"N" + reads[5][41:]                                          # an invalid letter
    reads[6] = b""
    reads[8] = reads[8][:75] + b"nnnn" + reads[8][79:]
    reads[9] = reads[9].lower().replace(b"t", b"u")
    reads[11] = refs[3][100:260]                                                             # longer than max_qlen 150: no candidates
    want = cref.seed_chains(reads, refs, K_MED, max_qlen=150, **OPTS_MED)
    full = cref.seed_chains(reads, refs, K_MED, **OPTS_MED)                                  # the host entry: max_qlen is the longest row
    for a in list(want.values()) + list(full.values()):
        a.setflags(write=False)
    return refs, reads, want, full


@pytest.fixture(scope="module")
def medium_dev(pkg, medium):
    refs, reads, _, _ = medium
    R, Q = pkg.SeqSet.new(refs), pkg.SeqSet.new(reads)
    return Q, R, pkg.SeedIndex.build(R, K_MED, stream=_stream())


def test_medium_equals_the_model_twice_and_per_strand(pkg, medium, medium_dev):
    refs, reads, want, _ = medium
    Q, R, ix = medium_dev
    total, nq = int(want["row_off"][-1]), len(reads)
    assert total >= 250 and want["row_off"][12] == want["row_off"][11] and want["row_off"][7] == want["row_off"][6]
    assert (want["seeds"]["diag_max"] - want["seeds"]["diag_min"] >= 10).sum() > 50           # chains over the deletion
    a = _chain(pkg, Q, ix, nq, 150, total + 5, **OPTS_MED)
    _same(a, want, total + 5, nq)
    b = _chain(pkg, Q, ix, nq, 150, total + 5, **OPTS_MED)
    for x, y in ((a.pairs, b.pairs), (a.strand, b.strand), (a.seeds, b.seeds), (a.chains, b.chains), (a.off, b.off), (a.counts, b.counts)):
        assert x.tobytes() == y.tobytes()
    both = []
    for mode in (ref.FORWARD, ref.REVERSE):                                                  # both strands are the two, listed separately
        one = cref.seed_chains(reads, refs, K_MED, strand=mode, max_qlen=150, **OPTS_MED)
        n = int(one["row_off"][-1])
        _same(_chain(pkg, Q, ix, nq, 150, n + 1, strand=mode, **OPTS_MED), one, n + 1, nq)
        assert (one["strand"] == mode).all()
        both.append(n)
    assert sum(both) == total and min(both) > 100


def test_host_entry_max_hits_and_subranges(pkg, medium, medium_dev):
    refs, reads, short, want = medium
    Q, R, ix = medium_dev
    total = int(want["row_off"][-1])
    assert total == int(short["row_off"][-1]) + 1                                            # row 11, 160 letters long, has its candidate here
    h = pkg.seed_chains(Q, ix, **OPTS_MED)
    assert h.kind == "strand" and h.n_rows == len(reads) and h.n_passing == h.n_hits == len(h) == total
    for key in KEYS:
        assert getattr(h, key).tobytes() == want[key].tobytes(), key
    assert h.row_off.tobytes() == want["row_off"].tobytes() and h.chains.dtype == pkg.SEED_CHAIN_DTYPE
    for max_hits in (1, 37, total, total + 9):
        c = pkg.seed_chains(Q, ix, max_hits=max_hits, **OPTS_MED)
        n = min(max_hits, total)
        assert c.n_passing == total and c.n_hits == n and c.row_off.tobytes() == want["row_off"].tobytes()
        for key in KEYS:
            assert getattr(c, key).tobytes() == want[key][:n].tobytes(), key
    for first, n in ((0, 1), (1, 199), (299, 1), (300, 0)):
        a, b = int(want["row_off"][first]), int(want["row_off"][first + n])
        sub = pkg.seed_chains(Q, ix, first_row=first, rows=n, slice_rows=77, **OPTS_MED)
        assert sub.row_off.tolist() == (want["row_off"][first:first + n + 1] - a).tolist()
        for key in KEYS:
            assert getattr(sub, key).tobytes() == want[key][a:b].tobytes(), key


@pytest.mark.parametrize("slice_rows,budget", [(1, 0), (3, 0), (0, 0), (0, 300000), (0, 1 << 20)])
def test_slices_and_match_budgets_never_change_a_byte(pkg, medium, medium_dev, slice_rows, budget):
    """budget: the match buffer (test hook) -- one row's worst case is 150 x 2 x 24 x 40 = 288 000 bytes; 300 000 bytes hold 7 500
    matches and 1 MiB 26 214, so the cut falls inside the rows either way"""
    refs, reads, want, _ = medium
    Q, R, ix = medium_dev
    nq = 120 if slice_rows in (1, 3) else len(reads)                                        # (a slice costs a synchronisation)
    sub = {key: want[key][:int(want["row_off"][nq])] for key in KEYS}
    sub["row_off"] = want["row_off"][:nq + 1]
    total = int(sub["row_off"][-1])
    pkg.lib.pmx_seed_match_budget(budget)
    try:
        _same(_chain(pkg, Q, ix, nq, 150, total, slice_rows=slice_rows, **OPTS_MED), sub, total, nq)
    finally:
        pkg.lib.pmx_seed_match_budget(0)


def test_capacity_and_optional_outputs(pkg, medium, medium_dev):
    refs, reads, want, _ = medium
    Q, R, ix = medium_dev
    nq, total = len(reads), int(want["row_off"][-1])
    for cap in (0, total // 2, total):                                                       # counts only; entries behind it untouched; exact
        _same(_chain(pkg, Q, ix, nq, 150, cap, **OPTS_MED), want, cap, nq)
    for seeds, chains in ((False, True), (True, False), (False, False)):
        _same(_chain(pkg, Q, ix, nq, 150, total, seeds=seeds, chains=chains, **OPTS_MED), want, total, nq, seeds=seeds, chains=chains)


def test_thresholds_of_min_score_and_min_seeds(pkg, medium, medium_dev):
    refs, reads, _, _ = medium
    Q, R, ix = medium_dev
    nq = 60
    base = dict(OPTS_MED, min_score=0, min_seeds=1)
    every = cref.seed_chains(reads, refs, K_MED, nq=nq, max_qlen=150, **base)
    s = int(np.median(every["chains"]["score"][every["chains"]["n_anchors"] > 1]))
    n = int(np.median(every["chains"]["n_anchors"][every["chains"]["n_anchors"] > 1]))
    assert (every["chains"]["score"] == s).any() and (every["chains"]["n_anchors"] == n).any()
    counts = []
    for o in (dict(base), dict(base, min_score=s), dict(base, min_score=s + 1), dict(base, min_seeds=n), dict(base, min_seeds=n + 1)):
        want = cref.seed_chains(reads, refs, K_MED, nq=nq, max_qlen=150, **o)
        total = int(want["row_off"][-1])
        _same(_chain(pkg, Q, ix, nq, 150, total, **o), want, total, nq)
        counts.append(total)
    assert counts[0] > counts[1] > counts[2] and counts[0] > counts[3] > counts[4]


@pytest.mark.parametrize("k,w", [(8, 1), (15, 1), (31, 1), (15, 5), (15, 10)])
def test_index_parameters(pkg, k, w):
    rng = np.random.default_rng(5200 + 40 * k + w)
    refs = random_seqs(rng, 6, 800, 1200)
    reads = []
    for x in range(40):
        r = int(rng.integers(6))
        a = int(rng.integers(0, len(refs[r]) - 330))
        piece = refs[r][a:a + 330]
        if x % 2:
            piece = piece[:150] + piece[180:]                                                # a deletion of 30
        reads.append(ref.orient(mutate(rng, piece, sub=0.01, indel=0.003), x % 3 == 0))
    want = _check(pkg, reads, refs, k, w=w, min_seeds=2, min_score=k + 5, band=60, max_gap=300, lookback=64, max_occ=16)
    assert int(want["row_off"][-1]) >= 30
    assert (want["seeds"]["diag_max"] - want["seeds"]["diag_min"] >= 25).sum() >= 5           # one chain over the deletion


def test_pad_clips_at_both_reference_ends(pkg):
    rng = np.random.default_rng(5300)
    k = 12
    refs = [_rand(rng, 400), _rand(rng, 300)]
    rows = [refs[0][:100], refs[0][-100:], ref.orient(refs[1][3:90], 1), ref.orient(refs[1][-95:-2], 1), refs[0][150:250]]
    want = _check(pkg, rows, refs, k, min_seeds=2, band=20, max_gap=100, lookback=64, pad=16)
    p = want["pairs"]
    assert len(p) == 5 and p["r"].tolist() == [0, 0, 1, 1, 0]
    assert p["r_beg"].tolist() == [0, 300 - 16, 0, 300 - 95 - 16, 150 - 16]
    assert (p["r_beg"] + p["r_len"]).tolist() == [100 + 16, 400, 3 + 87 + 16, 300, 250 + 16]


# ---- the planted properties, end to end ------------------------------------------------------------------------------------------------
def test_planted_properties_through_filter_and_extension(pkg):
    """reads A + B whose locus is A + 60 nt + B, and reads A + 2 kb noise + B on one diagonal, on both strands: chaining lists the
    first as ONE window, the cluster road as two; the chain's window scores at least what either cluster window scores in the gapped
    extension; and top_n = 1 of the ungapped filter keeps the planted locus of every row.  The letters next to a junction are chosen
    so that no k-mer crosses it; chance matches elsewhere make chains of a few anchors, so "the locus' candidates" are those of at
    least 50 anchors"""
    rng = np.random.default_rng(5400)
    k = 12
    genome, reads, truth = bytearray(_rand(rng, 40000)), [], []
    for x in range(8):
        A, B = _rand(rng, 152), _rand(rng, 150)
        pos = 1000 + 4500 * x
        other = bytes.maketrans(b"ACGT", b"CGTA")
        if x < 5:
            mid = _rand(rng, 58)
            mid = B[:1].translate(other) + mid + A[-1:].translate(other)                     # the insert prolongs neither half
            read = A + B
        else:
            mid, noise = _rand(rng, 2000), _rand(rng, 1998)
            read = A + mid[:1].translate(other) + noise + mid[-1:].translate(other) + B      # ... nor does the read's own noise
        locus = A + mid + B
        genome[pos:pos + len(locus)] = locus
        truth.append((pos, len(locus), x & 1))
        reads.append(ref.orient(read, x & 1))
    genome = bytes(genome)
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new([genome])
    ix = pkg.SeedIndex.build(R, k, stream=_stream())
    opts = dict(min_seeds=2, band=100, max_gap=5000, lookback=64, pad=16, max_occ=64)
    chained = pkg.seed_chains(Q, ix, **opts)
    want = cref.seed_chains(reads, [genome], k, **opts)
    for key in KEYS:
        assert getattr(chained, key).tobytes() == want[key].tobytes(), key
    clustered = pkg.seed_pairs(Q, ix, min_seeds=2, band=8, pad=16, max_occ=64)
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()

    def scores(hits):
        rec = al.align_pairs(Q, R, hits.pairs, strand=hits.strand)
        rec = rec[0] if isinstance(rec, tuple) else rec
        assert (rec["flags"] == 0).all()
        return rec["score"]
    cs, ks = scores(chained), scores(clustered)
    for q, (pos, span, strand) in enumerate(truth):
        a, b = int(chained.row_off[q]), int(chained.row_off[q + 1])
        mine = [x for x in range(a, b) if chained.strand[x] == strand and pos <= chained.chains[x]["r_beg"] < pos + span and
                chained.chains[x]["n_anchors"] >= 50]
        assert len(mine) == 1, (q, chained.chains[a:b])                                       # ONE candidate at the locus ...
        c = chained.chains[mine[0]]
        assert c["n_anchors"] == 280 and (c["r_beg"], c["r_end"]) == (pos, pos + span)       # ... spanning all of it
        ka, kb = int(clustered.row_off[q]), int(clustered.row_off[q + 1])
        theirs = [x for x in range(ka, kb) if clustered.strand[x] == strand and clustered.seeds[x]["n_seeds"] >= 50]
        assert len(theirs) == (2 if q < 5 else 1)                                            # the indel splits the cluster; the diagonal merges it
        assert cs[mine[0]] >= max(ks[x] for x in theirs)
        if q < 5:                                                                            # a cluster's window ends qlen + pad behind its diagonal: A's
            assert cs[mine[0]] > max(ks[x] for x in theirs)                                  # lacks the last 44 letters of B, B's the first 44 of A
    kept = pkg.seed_filter(Q, R, chained, pm, min_score=0, top_n=1)
    assert kept.kind == "strand" and np.diff(kept.row_off).tolist() == [1] * len(reads)
    for q, (pos, span, strand) in enumerate(truth):
        x = int(kept.row_off[q])
        assert kept.strand[x] == strand and kept.pairs[x]["r_beg"] <= pos and kept.pairs[x]["r_beg"] + kept.pairs[x]["r_len"] >= pos + span
    # two chains at max_gap 1 000 for the reads with 2 kb between the halves
    near = pkg.seed_chains(Q, ix, first_row=5, rows=3, **dict(opts, max_gap=1000))
    assert near.chains["n_anchors"][near.chains["n_anchors"] >= 50].tolist() == [141, 139] * 3
