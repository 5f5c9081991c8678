"""K-mer seeding (`-m gpu`): pmx_seed_index_build and pmx_seed_pairs[_device] against the model tests/seed_ref.py -- index entries at
the key-width boundaries and the sequence ends, matches, max_occ, diagonal clusters, windows and their order on small crafted sets and
on 2 000 noisy reads, slices, a tiny match buffer, capacity, sub-ranges, the host entry -- and, end to end, the candidates of planted
reads through Aligner.align_pairs with CIGARs.  Every comparison is exact; every output buffer starts as a sentinel."""
import numpy as np
import pytest

import pairs_ex_ref
import seed_ref as ref
from util import random_seqs, mutate

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


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


# ---- the index -------------------------------------------------------------------------------------------------------------------------
def _entries(pkg, ix, first, count, slack=3):
    import torch
    km = _full((count + slack,), SENTINEL, torch.int64)
    sq = _full((count + slack,), SENTINEL, torch.int64)
    ps = _full((count + slack,), SENTINEL, torch.int32)
    pkg.seed_index_entries_device(ix, first, count, km.data_ptr(), sq.data_ptr(), ps.data_ptr(), _stream())
    _sync()
    km, sq, ps = km.cpu().numpy(), sq.cpu().numpy(), ps.cpu().numpy()
    assert (km[count:] == SENTINEL).all() and (sq[count:] == SENTINEL).all() and (ps[count:] == SENTINEL).all()
    return list(zip(km[:count].view(np.uint64).tolist(), sq[:count].tolist(), ps[:count].tolist()))


def _edge_set(rng, k):
    """empty sequences, lengths k - 1, k and k + 1, invalid letters at the first and last position of a k-mer, the lowest and the
    highest key, lower case and U, and enough random sequence for more than one block of the extraction"""
    body = _rand(rng, 3 * k)
    return [b"", _rand(rng, k - 1), _rand(rng, k), _rand(rng, k + 1), b"", b"N" + body[:k], body[:k - 1] + b"N", body[:k] + b"N" + body[k:2 * k],
            b"A" * (k + 2), b"T" * k + b"U", b"acgu" * k, _rand(rng, 9000), b"N" * 40, _rand(rng, 700) + b"n" + _rand(rng, 2 * k), b""]


@pytest.mark.parametrize("k", [8, 16, 17, 31])
def test_index_entries_equal_the_model(pkg, k):
    rng = np.random.default_rng(5000 + k)
    refs = _edge_set(rng, k)
    want = ref.index_entries(refs, k)
    assert want[0][0] == 0 and want[-1][0] == 4 ** k - 1                                    # all-A and all-T are there
    R = pkg.SeqSet.new(refs)
    ix = pkg.SeedIndex.build(R, k, _stream())
    assert len(ix) == len(want)
    assert _entries(pkg, ix, 0, len(want)) == want
    for first, count in ((0, 1), (len(want) - 1, 1), (17, 300), (len(want), 0)):             # windows of the hook
        assert _entries(pkg, ix, first, count) == want[first:first + count]
    with pytest.raises(pkg.BatchError, match="beyond"):
        pkg.seed_index_entries_device(ix, len(want), 1, None, None, None)
    ix.close()


def test_index_of_empty_and_wrapped_sets(pkg):
    rng = np.random.default_rng(5100)
    for refs in ([], [b""], [b"ACGT"], [b"N" * 50]):
        R = pkg.SeqSet.new(refs)
        ix = pkg.SeedIndex.build(R, 8)
        assert len(ix) == 0
        Q = pkg.SeqSet.new([b"ACGTACGTACGT", b""])
        h = pkg.seed_pairs(Q, ix, min_seeds=1)
        assert h.row_off.tolist() == [0, 0, 0] and len(h) == 0 and h.n_passing == 0
    # a wrapped set: offsets that start behind a prefix, bytes behind the last sequence, nothing outside `bytes` is read
    refs = [_rand(rng, 300), b"", _rand(rng, 5), _rand(rng, 4100)]
    buf = np.frombuffer(b"ACGTACGTACGTACGT" + b"".join(refs) + b"ACGTACGTACGTACGTACGT", dtype=np.uint8).copy()
    off = 16 + np.concatenate(([0], np.cumsum([len(s) for s in refs]))).astype(np.int64)
    d_buf, d_off = _up(buf), _up(off)
    R = pkg.SeqSet.wrap_device(d_buf.data_ptr(), d_off.data_ptr(), len(refs), len(buf), keep=(d_buf, d_off))
    ix = pkg.SeedIndex.build(R, 11, _stream())
    want = ref.index_entries(refs, 11)
    assert len(ix) == len(want) and _entries(pkg, ix, 0, len(want)) == want
    qs = [refs[0][20:80], ref.orient(refs[3][4000:4060], 1)]
    d_qb, d_qo = _up(np.frombuffer(b"".join(qs), dtype=np.uint8).copy()), _up(np.array([0, 60, 120], dtype=np.int64))
    Q = pkg.SeqSet.wrap_device(d_qb.data_ptr(), d_qo.data_ptr(), 2, 120, keep=(d_qb, d_qo))
    h = pkg.seed_pairs(Q, ix, min_seeds=3, band=0, pad=4)                                   # (the host entry finds max_qlen on the device)
    _same_host(h, ref.seed(qs, refs, 11, ref.BOTH, 3, 0, 4, 64))
    assert len(h) >= 2


# ---- seeding ---------------------------------------------------------------------------------------------------------------------------
class Got:
    pass


def _seed(pkg, Q, ix, nq, mq, capacity, q_first=0, with_seeds=True, **kw):
    import torch
    slots = capacity + 3
    hp = _full((slots * 32,), FILL, torch.uint8)
    hs = _full((slots,), FILL, torch.uint8)
    hd = _full((slots, 4), SENTINEL, torch.int32) if with_seeds else None
    off = _full((nq + 1 + 2,), SENTINEL, torch.int64)
    cnt = _full((2 + 2,), SENTINEL, torch.int64)
    pkg.seed_pairs_device(Q, ix, q_first, nq, mq, hp.data_ptr(), hs.data_ptr(), hd.data_ptr() if with_seeds else None, capacity,
                          off.data_ptr(), cnt.data_ptr(), stream=_stream(), **kw)
    _sync()
    g = Got()
    g.pairs, g.strand, g.off, g.counts = hp.cpu().numpy().view(ref.PAIR_DTYPE), hs.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy()
    g.seeds = hd.cpu().numpy().reshape(-1).view(ref.SEED_HIT_DTYPE) if with_seeds else None
    return g


def _same(g, want, capacity, nq):
    """row_off and counts in full and uncapped, the first min(candidates, capacity) entries equal to the model's, every entry behind
    them the sentinel"""
    total = int(want["row_off"][-1])
    w = min(total, capacity)
    assert g.off[:nq + 1].tolist() == want["row_off"].tolist() and (g.off[nq + 1:] == SENTINEL).all()
    assert g.counts[:2].tolist() == [total, w] and (g.counts[2:] == SENTINEL).all()
    assert g.pairs[:w].tobytes() == want["pairs"][:w].tobytes() and (g.pairs[w:].view(np.uint8) == FILL).all()
    assert g.strand[:w].tobytes() == want["strand"][:w].tobytes() and (g.strand[w:] == FILL).all()
    if g.seeds is not None:
        assert g.seeds[:w].tobytes() == want["seeds"][:w].tobytes() and (g.seeds[w:].view(np.int32) == SENTINEL).all()


def _same_host(h, want, stored=None):
    total = int(want["row_off"][-1])
    stored = total if stored is None else stored
    assert h.n_rows == len(want["row_off"]) - 1 and h.n_passing == total and h.n_hits == len(h) == stored
    assert h.row_off.tobytes() == want["row_off"].tobytes()
    assert h.pairs.tobytes() == want["pairs"][:stored].tobytes() and h.strand.tobytes() == want["strand"][:stored].tobytes()
    assert h.seeds.tobytes() == want["seeds"][:stored].tobytes()


def _check(pkg, qs, refs, k, mq=None, expect=None, **kw):
    """device entry == model for the options kw, in every strand mode unless kw names one; returns the model's result of the last"""
    Q, R = pkg.SeqSet.new(qs), pkg.SeqSet.new(refs)
    ix = pkg.SeedIndex.build(R, k, _stream())
    mq = max(1, max(len(s) for s in qs)) if mq is None else mq
    modes = (kw.pop("strand"),) if "strand" in kw else (ref.FORWARD, ref.REVERSE, ref.BOTH)
    o = dict(min_seeds=2, band=8, pad=16, max_occ=64)
    o.update(kw)
    for mode in modes:
        want = ref.seed(qs, refs, k, mode, o["min_seeds"], o["band"], o["pad"], o["max_occ"], max_qlen=mq)
        total = int(want["row_off"][-1])
        _same(_seed(pkg, Q, ix, len(qs), mq, total + 2, strand=mode, **o), want, total + 2, len(qs))
    if expect is not None:
        assert [tuple(int(v) for v in s)[:3] for s in want["seeds"]] == expect, want["seeds"]
    return want


@pytest.mark.parametrize("seed", range(4))
def test_small_random_sets(pkg, seed):
    rng = np.random.default_rng(5200 + seed)
    refs = random_seqs(rng, int(rng.integers(1, 6)), 0, 300)
    refs[0] = refs[0] + _rand(rng, 120)
    qs = []
    for _ in range(int(rng.integers(1, 9))):
        r = refs[int(rng.integers(len(refs)))]
        L = int(rng.integers(20, 61))
        if len(r) >= L and rng.random() < 0.8:
            a = int(rng.integers(0, len(r) - L + 1))
            s = mutate(rng, r[a:a + L], sub=0.04, indel=0.02)
            qs.append(ref.orient(s, int(rng.integers(2))))
        else:
            qs.append(_rand(rng, L))
    want = _check(pkg, qs, refs, 8, min_seeds=int(rng.integers(1, 4)), band=int(rng.integers(0, 6)), pad=int(rng.integers(0, 20)))
    assert len(want["pairs"]) > 0


@pytest.mark.parametrize("k", [16, 17, 27, 31])
def test_long_kmers_through_the_lookup(pkg, k):
    """keys at and beyond 32 bits through the count kernel's key, bucket and binary search (the bucket's shift is 2k - 22)"""
    rng = np.random.default_rng(5250 + k)
    refs = [_rand(rng, 400), _rand(rng, 37), _rand(rng, 900)]
    refs[2] = refs[2][:500] + refs[0][100:180] + refs[2][500:]                              # a repeat across references
    qs = [mutate(rng, refs[0][90:190], sub=0.01, indel=0.0), ref.orient(refs[2][300:420], 1), refs[1], b"A" * (k - 1) + b"N" + b"T" * k,
          refs[0][100:100 + k], b"T" * k]
    want = _check(pkg, qs, refs, k, min_seeds=1, band=2, pad=7)
    assert len(want["pairs"]) >= 5 and want["row_off"][-1] > want["row_off"][4] == want["row_off"][3]


def test_palindromic_kmer_matches_on_both_strands(pkg):
    pal = b"ACGTACGT"                                                                       # its own reverse complement
    refs = [b"GGGGG" + pal + b"CCCCC"]
    want = _check(pkg, [b"TT" + pal + b"TT"], refs, 8, strand=ref.BOTH, min_seeds=1, band=0, pad=0)
    assert want["strand"].tolist() == [0, 1] and [tuple(p)[4:] for p in want["pairs"]] == [(3, 12), (3, 12)]


def test_max_occ_keeps_exactly_and_drops_one_more(pkg):
    rng = np.random.default_rng(5300)
    unit, other = _rand(rng, 12), _rand(rng, 12)
    spacers = [_rand(rng, 30) for _ in range(8)]
    three = spacers[0] + unit + spacers[1] + unit + spacers[2] + unit + spacers[3]          # `unit` three times, `other` four times
    four = other + spacers[4] + other + spacers[5] + other + spacers[6] + other
    refs, qs = [three, four], [unit, other]
    assert len(ref.index_dict(refs, 12)[ref.kmers(unit, 12)[0][1]]) == 3 and len(ref.index_dict(refs, 12)[ref.kmers(other, 12)[0][1]]) == 4
    kept = _check(pkg, qs, refs, 12, strand=ref.FORWARD, min_seeds=1, band=0, pad=0, max_occ=3)
    assert kept["row_off"].tolist() == [0, 3, 3]                                            # exactly max_occ: kept; max_occ + 1: dropped
    assert _check(pkg, qs, refs, 12, strand=ref.FORWARD, min_seeds=1, band=0, pad=0, max_occ=4)["row_off"].tolist() == [0, 3, 7]
    assert _check(pkg, qs, refs, 12, strand=ref.FORWARD, min_seeds=1, band=0, pad=0, max_occ=2)["row_off"].tolist() == [0, 0, 0]
    assert _check(pkg, qs, refs, 12, strand=ref.FORWARD, min_seeds=1, band=0, pad=0, max_occ=1)["row_off"].tolist() == [0, 0, 0]


def _two_blocks(rng, gap_q, gap_r, n=10, k=8):
    """a query of two blocks of n letters that a reference holds gap_r - gap_q further apart: two diagonals, n - k + 1 matches each"""
    a, b = _rand(rng, n), _rand(rng, n)
    q = a + b"C" * gap_q + b
    r = b"G" * 7 + a + b"T" * gap_r + b + b"G" * 5
    return q, r


def test_band_joins_at_band_and_splits_one_beyond(pkg):
    rng = np.random.default_rng(5400)
    q, r = _two_blocks(rng, 3, 7)                                                           # diagonals 7 and 11
    both = ref.seed([q], [r], 8, ref.FORWARD, 1, 4, 0, 64)
    assert [tuple(s)[:3] for s in both["seeds"]] == [(6, 7, 11)]
    _check(pkg, [q], [r], 8, strand=ref.FORWARD, min_seeds=1, band=4, pad=0, expect=[(6, 7, 11)])          # exactly band apart: one cluster
    _check(pkg, [q], [r], 8, strand=ref.FORWARD, min_seeds=1, band=3, pad=0, expect=[(3, 7, 7), (3, 11, 11)])
    _check(pkg, [q], [r], 8, strand=ref.FORWARD, min_seeds=1, band=0, pad=0, expect=[(3, 7, 7), (3, 11, 11)])
    _check(pkg, [q], [r], 8, strand=ref.FORWARD, min_seeds=1, band=1 << 20, pad=1 << 20, expect=[(6, 7, 11)])


def test_min_seeds_at_and_below_the_cluster_size(pkg):
    rng = np.random.default_rng(5500)
    q, r = _two_blocks(rng, 3, 9, n=12)                                                     # two clusters of 5 matches
    _check(pkg, [q], [r], 8, strand=ref.FORWARD, min_seeds=5, band=0, pad=2, expect=[(5, 7, 7), (5, 13, 13)])
    _check(pkg, [q], [r], 8, strand=ref.FORWARD, min_seeds=6, band=0, pad=2, expect=[])
    _check(pkg, [q], [r], 8, strand=ref.FORWARD, min_seeds=10, band=6, pad=2, expect=[(10, 7, 13)])
    _check(pkg, [q], [r], 8, strand=ref.FORWARD, min_seeds=11, band=6, pad=2, expect=[])


def test_equal_diagonals_in_adjacent_references_do_not_merge(pkg):
    rng = np.random.default_rng(5600)
    core = _rand(rng, 14)
    refs = [b"GGG" + core + b"G", b"TTT" + core + b"TT", b"", b"CCC" + core]                 # diagonal 3 in three references
    want = _check(pkg, [core], refs, 8, strand=ref.FORWARD, min_seeds=7, band=50, pad=1)
    assert [int(p["r"]) for p in want["pairs"]] == [0, 1, 3] and [tuple(s)[:3] for s in want["seeds"]] == [(7, 3, 3)] * 3
    assert [tuple(p)[4:] for p in want["pairs"]] == [(2, 16), (2, 16), (2, 15)]             # the last one clamped at len(r)


def test_negative_diagonals_and_the_reference_ends(pkg):
    rng = np.random.default_rng(5700)
    r = _rand(rng, 60)
    qs = [_rand(rng, 9) + r[:25],                                                           # hangs over the reference's start: d = -9
          r[40:] + _rand(rng, 12),                                                          # hangs over its end: d = 40
          r]                                                                                # the whole reference: d = 0
    for pad in (0, 5, 100):
        want = _check(pkg, qs, [r], 8, strand=ref.FORWARD, min_seeds=3, band=0, pad=pad)
        assert [tuple(s)[1:3] for s in want["seeds"]] == [(-9, -9), (40, 40), (0, 0)]
        assert [tuple(p)[4:] for p in want["pairs"]] == [(0, min(60, 25 + pad)), (max(0, 40 - pad), 60 - max(0, 40 - pad)), (0, 60)]


def test_rows_without_kmers_long_rows_and_q_equal_r(pkg):
    rng = np.random.default_rng(5800)
    r = _rand(rng, 200)
    qs = [b"ACGTACG", b"", b"N" * 30, r[10:50], r[5:95], r[100:140]]                        # no k-mer: short, empty, invalid; longer than max_qlen
    want = _check(pkg, qs, [r], 8, mq=60, min_seeds=2, band=2, pad=3)
    assert want["row_off"].tolist() == [0, 0, 0, 0, 1, 1, 2]
    S = [r[20:90], _rand(rng, 40), r[50:120], b""]                                          # Q the same set as R: every sequence finds itself
    Q = pkg.SeqSet.new(S)
    ix = pkg.SeedIndex.build(Q, 10, _stream())
    want = ref.seed(S, S, 10, ref.BOTH, 4, 0, 8, 64)
    _same(_seed(pkg, Q, ix, 4, 70, 64, min_seeds=4, band=0, pad=8), want, 64, 4)
    assert (0, 0) in [(int(p["q"]), int(p["r"])) for p in want["pairs"]] and (0, 2) in [(int(p["q"]), int(p["r"])) for p in want["pairs"]]


# ---- medium: noisy reads of many references, slices, capacity, sub-ranges, the host entry ----------------------------------------------
K_MED, OPTS_MED = 13, dict(min_seeds=3, band=6, pad=12, max_occ=24)


@pytest.fixture(scope="module")
def medium():
    rng = np.random.default_rng(6000)
    refs = random_seqs(rng, 64, 1500, 4700)                                                 # about 200 kb
    unit = _rand(rng, 9)
    refs[7] = refs[7][:800] + unit * 60 + refs[7][800:]                                     # a tandem repeat: 9 keys of ~59 entries each, above max_occ
    reads, truth = [], []
    for x in range(2000):
        r = int(rng.integers(64)) if x % 50 else 7
        a = int(rng.integers(0, len(refs[r]) - 150)) if x % 50 else int(rng.integers(700, 1300))
        s = mutate(rng, refs[r][a:a + 150], sub=0.02, indel=0.005)[:150]
        strand = x & 1
        reads.append(ref.orient(s, strand))
        truth.append((r, a, strand))
    idx = ref.index_dict(refs, K_MED)
    assert max(len(v) for v in idx.values()) > OPTS_MED["max_occ"]                          # the repeat is above max_occ
    want = ref.seed(reads, refs, K_MED, ref.BOTH, OPTS_MED["min_seeds"], OPTS_MED["band"], OPTS_MED["pad"], OPTS_MED["max_occ"])
    for a in want.values():
        a.setflags(write=False)
    return refs, reads, truth, want


@pytest.fixture(scope="module")
def medium_dev(pkg, medium):
    refs, reads, _, _ = medium
    R, Q = pkg.SeqSet.new(refs), pkg.SeqSet.new(reads)
    return Q, R, pkg.SeedIndex.build(R, K_MED, _stream())


def test_medium_equals_the_model_and_repeats(pkg, medium, medium_dev):
    refs, reads, truth, want = medium
    Q, R, ix = medium_dev
    assert len(ix) == len(ref.index_entries(refs, K_MED))
    total = int(want["row_off"][-1])
    assert total >= 1800                                                                    # (nearly every read finds its locus)
    a = _seed(pkg, Q, ix, len(reads), 150, total + 5, **OPTS_MED)
    _same(a, want, total + 5, len(reads))
    b = _seed(pkg, Q, ix, len(reads), 150, total + 5, **OPTS_MED)
    for x, y in ((a.pairs, b.pairs), (a.strand, b.strand), (a.seeds, b.seeds), (a.off, b.off), (a.counts, b.counts)):
        assert x.tobytes() == y.tobytes()
    found = 0
    for q, (r, pos, strand) in enumerate(truth):
        lo, hi = int(want["row_off"][q]), int(want["row_off"][q + 1])
        found += any(int(want["pairs"][x]["r"]) == r and want["strand"][x] == strand and
                     want["seeds"][x]["diag_min"] - 8 <= pos <= want["seeds"][x]["diag_max"] + 8 for x in range(lo, hi))
    assert found >= 1800


@pytest.mark.parametrize("slice_rows,budget", [(1, 0), (3, 0), (0, 0), (0, 1 << 20), (700, 300000)])
def test_slices_and_a_tiny_match_buffer_never_change_a_byte(pkg, medium, medium_dev, slice_rows, budget):
    """budget: the match buffer (test hook) -- 2^20 bytes hold 43 690 matches, a few hundred reads; 300 000 bytes a few dozen, and no
    fewer than one row's worst case of 150 x 2 x 24 x 24 = 172 800"""
    refs, reads, _, want = medium
    Q, R, ix = medium_dev
    nq = 300 if slice_rows in (1, 3) else len(reads)                                        # (a slice costs a synchronisation)
    sub = {key: want[key][:int(want["row_off"][nq])] for key in ("pairs", "strand", "seeds")}
    sub["row_off"] = want["row_off"][:nq + 1]
    total = int(sub["row_off"][-1])
    pkg.lib.pmx_seed_match_budget(budget)
    try:
        _same(_seed(pkg, Q, ix, nq, 150, total, slice_rows=slice_rows, **OPTS_MED), sub, total, nq)
    finally:
        pkg.lib.pmx_seed_match_budget(0)


def test_capacity_subranges_and_the_host_entry(pkg, medium, medium_dev):
    refs, reads, _, want = medium
    Q, R, ix = medium_dev
    nq = len(reads)
    total = int(want["row_off"][-1])
    for cap in (0, 1, total // 2, total, total + 9):
        _same(_seed(pkg, Q, ix, nq, 150, cap, with_seeds=cap != 1, **OPTS_MED), want, cap, nq)
    for first, n in ((0, 1), (1, 999), (1500, 500), (1999, 1), (2000, 0), (700, 0)):        # sub-ranges: the rows of the full run
        a, b = int(want["row_off"][first]), int(want["row_off"][first + n])
        sub = {"row_off": want["row_off"][first:first + n + 1] - a, "pairs": want["pairs"][a:b], "strand": want["strand"][a:b], "seeds": want["seeds"][a:b]}
        _same(_seed(pkg, Q, ix, n, 150, b - a + 1, q_first=first, slice_rows=333, **OPTS_MED), sub, b - a + 1, n)
    _same_host(pkg.seed_pairs(Q, ix, **OPTS_MED), want)
    _same_host(pkg.seed_pairs(Q, ix, max_hits=total // 3, slice_rows=512, **OPTS_MED), want, stored=total // 3)
    _same_host(pkg.seed_pairs(Q, ix, max_hits=total + 7, **OPTS_MED), want)
    # far more than two candidates per row (reads 0 and 50 lie in the tandem repeat, whose k-mers max_occ 64 keeps: every copy is
    # a diagonal of its own at band 0): the host entry's second, exact-size run
    many = ref.seed(reads, refs, K_MED, ref.BOTH, 1, 0, 0, 64, nq=51)
    n_many = int(many["row_off"][-1])
    assert n_many > 2 * (2 * 51 + 16)                                                       # twice the first run's room
    _same_host(pkg.seed_pairs(Q, ix, rows=51, min_seeds=1, band=0, pad=0, max_occ=64), many)
    _same_host(pkg.seed_pairs(Q, ix, rows=51, min_seeds=1, band=0, pad=0, max_occ=64, max_hits=n_many - 3), many, stored=n_many - 3)
    _same_host(pkg.seed_pairs(Q, ix, rows=51, min_seeds=1, band=0, pad=0, max_occ=64, max_hits=7), many, stored=7)
    h = pkg.seed_pairs(Q, ix, first_row=40, rows=25, **OPTS_MED)
    a, b = int(want["row_off"][40]), int(want["row_off"][65])
    assert h.row_off.tolist() == (want["row_off"][40:66] - a).tolist() and h.pairs.tobytes() == want["pairs"][a:b].tobytes()
    p, s, d = h.row(3)
    x, y = int(want["row_off"][43]), int(want["row_off"][44])
    assert p.tobytes() == want["pairs"][x:y].tobytes() and s.tobytes() == want["strand"][x:y].tobytes() and d.tobytes() == want["seeds"][x:y].tobytes()
    with pytest.raises(pkg.BatchError, match="worst case"):                                  # refused before any GPU work
        pkg.seed_pairs(Q, ix, max_occ=65535, min_seeds=3)


# ---- end to end: planted reads -> candidates -> alignments with CIGARs -----------------------------------------------------------------
def test_planted_reads_end_to_end(pkg, orc):
    rng = np.random.default_rng(7000)
    genome = _rand(rng, 200000)
    n, L, k = 400, 100, 12
    reads, truth = [], []
    for x in range(n):
        pos = int(rng.integers(0, len(genome) - L))
        s = bytearray(genome[pos:pos + L])
        errs = sorted(rng.choice(L, size=int(rng.integers(0, 4)), replace=False).tolist()) if x else [24, 49, 74]
        for e in errs:
            s[e] = b"ACGT"[(b"ACGT".index(s[e]) + 1 + int(rng.integers(3))) % 4]
        strand = x & 1
        reads.append(ref.orient(bytes(s), strand))
        truth.append((pos, strand, errs))
        assert ref.longest_clean_run(L, errs) >= 24                                         # the pigeonhole condition: (100 - 3) / 4 > 24
    idx = ref.index_dict([genome], k)
    assert max(len(v) for v in idx.values()) <= 64                                          # no reference 12-mer above max_occ
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new([genome])
    ix = pkg.SeedIndex.build(R, k, _stream())
    hits = pkg.seed_pairs(Q, ix, strand="both", min_seeds=13, band=0, pad=0, max_occ=64)
    _same_host(hits, ref.seed(reads, [genome], k, ref.BOTH, 13, 0, 0, 64))
    planted = []
    for q, (pos, strand, errs) in enumerate(truth):
        a, b = int(hits.row_off[q]), int(hits.row_off[q + 1])
        ok = [x for x in range(a, b) if hits.pairs[x]["r"] == 0 and hits.strand[x] == strand and
              hits.seeds[x]["diag_min"] <= pos <= hits.seeds[x]["diag_max"]]
        assert len(ok) == 1, (q, pos, strand)
        planted.append(ok[0])
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    rec, cigars, begins = al.align_pairs(Q, R, hits.pairs, strand=hits.strand, cigar=True)
    assert (rec["flags"] == 0).all()
    for q, x in enumerate(planted):
        s = len(truth[q][2])
        assert rec["score"][x] >= 2 * (L - s) - 3 * s, (q, int(rec["score"][x]), s)
    # every CIGAR re-scores to its score on the oriented read against the window (the oracle on the resolved strings)
    strings = pairs_ex_ref.resolve(reads, [genome], hits.pairs, hits.strand)
    assert all(s is not None for s in strings)
    qb, qo = orc.pack([s[0] for s in strings])
    rb, ro = orc.pack([s[1] for s in strings])
    text = np.frombuffer("".join(cigars).encode(), dtype=np.uint8)
    toff = np.concatenate(([0], np.cumsum([len(c) for c in cigars]))).astype(np.int64)
    res, malformed = orc.rescore_cigars(text if len(text) else np.zeros(1, dtype=np.uint8), toff, qb, qo, rb, ro, 5, 2, om,
                                        beg=np.ascontiguousarray(begins, dtype=np.int32).reshape(-1))
    assert malformed == 0 and (res[:, 0] == rec["score"]).all() and (res[:, 3] == 0).all()
