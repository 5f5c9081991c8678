"""Minimizer seeding (`-m gpu`): the sketch kernel's row form (pmx_seed_sketch_device) and set form (the entries of
pmx_seed_index_build_minimizers) against the window enumeration of tests/seed_minimizer_ref.py, at the lengths where the kernel's tile,
halo and sequence ends meet; seeding end to end against the same model under slices and a tiny match buffer; the guarantee, the
filter and the extension behind it.  Every comparison is exact; every output buffer starts as a sentinel."""
import numpy as np
import pytest

import seed_minimizer_ref as mref
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


# ---- the sketch: the row form against the model ----------------------------------------------------------------------------------------
def _sketch(pkg, Q, first, nq, mq, k, w, strand):
    """the device entry's bytes as [[bytes per orientation] per row]; nothing is written behind the last slot"""
    import torch
    orients = 2 if strand == ref.BOTH else 1
    total = nq * orients * mq
    d = _full((total + 64,), FILL, torch.uint8)
    pkg.seed_minimizers_device(Q, first, nq, mq, k, w, d.data_ptr(), strand=strand, stream=_stream())
    _sync()
    h = d.cpu().numpy()
    assert (h[total:] == FILL).all()
    h = h[:total].reshape(nq, orients, mq)
    return [[h[r, s].tobytes() for s in range(orients)] for r in range(nq)]


def _sketch_rows(rng, k, w, tile):
    """every length 0 .. 2 (w + k) + 2; the tile's size - 1, + 0, + 1; two tiles plus the halo; invalid letters at the first and the last
    letter, as a window's only k-mer and over a whole window; lower case and U; homopolymers and period-2 / period-3 repeats (ties)"""
    rows = [_rand(rng, n) for n in range(2 * (w + k) + 3)]
    rows += [_rand(rng, n) for n in (tile - 1, tile, tile + 1, tile + k - 2, tile + k - 1, tile + k, 2 * tile + w - 1 + k - 1)]
    body = _rand(rng, 3 * (w + k))
    rows += [b"N" + body[1:], body[:-1] + b"N", b"N" + body[1:-1] + b"n",
             b"N" * (w + 3) + _rand(rng, k) + b"N" * (w + 3),                                # one k-mer, alone in every window that holds it
             _rand(rng, w + k) + b"N" * (w + k + 2) + _rand(rng, k) + b"N" + _rand(rng, w + k + 5),      # whole windows without a k-mer
             body.lower(), body.replace(b"T", b"U"), body.lower().replace(b"t", b"u"),
             b"A" * (2 * w + k + 7), b"T" * (w + k), b"C" * (tile + w + k), b"AC" * (w + k), b"GT" * (w + k) + b"G", b"ACG" * (w + k),
             b"TTA" * ((tile + w + k) // 3), b"A" * (w + k) + b"N" + b"A" * (w + k), _rand(rng, 10) + b"AG" * (w + k) + _rand(rng, 10)]
    return rows


@pytest.mark.parametrize("w", [1, 2, 3, 10, 19, 64])
@pytest.mark.parametrize("k", [8, 15, 31])
def test_sketch_equals_the_window_enumeration(pkg, k, w):
    rng = np.random.default_rng(9000 + 100 * k + w)
    tile, _ = pkg.seed_sketch_shape()
    rows = _sketch_rows(rng, k, w, tile)
    mq = max(len(s) for s in rows)
    assert mq == 2 * tile + w - 1 + k - 1                                                   # three tiles: the third holds only the halo's rest
    rows.append(_rand(rng, mq + 1))                                                         # longer than max_qlen: no minimizer
    Q = pkg.SeqSet.new(rows)
    got = _sketch(pkg, Q, 0, len(rows), mq, k, w, ref.BOTH)
    want = mref.flags(rows, k, w, ref.BOTH, mq)
    bad = [(r, s) for r in range(len(rows)) for s in (0, 1) if got[r][s] != want[r][s]]
    assert not bad, (bad[:5], rows[bad[0][0]])
    assert not any(want[-1][0]) and not any(want[-1][1]) and any(want[-2][0])
    if w > 1:                                                                               # ties: leftmost in ORIENTED order on both strands
        homo = rows.index(b"A" * (2 * w + k + 7))
        nk = len(rows[homo]) - k + 1
        for s in (0, 1):
            assert got[homo][s][:nk] == bytes([1] * (nk - w + 1) + [0] * (w - 1))
    # the single strands and a sub-range are the same bytes
    for strand in (ref.FORWARD, ref.REVERSE):
        sub = _sketch(pkg, Q, 5, 40, mq, k, w, strand)
        assert [x[0] for x in sub] == [want[r][strand] for r in range(5, 45)]
    # a smaller max_qlen: the rows above it go blank, the others keep their bytes
    small = 2 * (w + k)
    got = _sketch(pkg, Q, 0, len(rows), small, k, w, ref.BOTH)
    assert got == mref.flags(rows, k, w, ref.BOTH, small)


def test_sketch_host_entry_and_w_1(pkg):
    rng = np.random.default_rng(9100)
    rows = [_rand(rng, 150), b"", _rand(rng, 30), b"ACGTN" * 20, _rand(rng, 149)]
    Q = pkg.SeqSet.new(rows)
    f = pkg.seed_minimizers(Q, 15, 10)
    assert f.shape == (5, 2, 150) and f.dtype == np.uint8
    want = mref.flags(rows, 15, 10, ref.BOTH, 150)
    assert [[f[r, s].tobytes() for s in (0, 1)] for r in range(5)] == want
    one = pkg.seed_minimizers(Q, 15, 1, strand="reverse", first_row=2, rows=3)
    assert one.shape == (3, 1, 149)
    for x, r in enumerate((2, 3, 4)):
        assert np.nonzero(one[x, 0])[0].tolist() == [p for p, _ in ref.kmers(ref.orient(rows[r], 1), 15)]
    # about 2 / (w + 1) of the positions of random sequence
    dens = f[0].sum() / (2 * 136)
    assert 0.10 < dens < 0.30


# ---- the index: the set form against the model -----------------------------------------------------------------------------------------
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


def _short_set(rng, k, w, tile):
    """many short sequences whose ends fall inside tiles and halos -- lengths 0, 1, k - 1, k, k + w - 2, k + w - 1, k + w, some with an
    N or a repeat -- and sequence ends ON the boundaries of the first three tiles and one position either side of them"""
    lens = [0, 1, k - 1, k, k + w - 2, k + w - 1, k + w]
    refs, total = [], 0

    def add(s):
        nonlocal total
        refs.append(s)
        total += len(s)

    for boundary, shift in ((tile, -1), (2 * tile, 0), (3 * tile, 1)):
        while total + 3 * (k + w) < boundary + shift:
            n = lens[int(rng.integers(len(lens)))]
            s = bytearray(_rand(rng, n))
            if n and rng.integers(0, 6) == 0:
                s[int(rng.integers(n))] = ord("N")
            if n > 3 and rng.integers(0, 6) == 0:
                s[:] = (b"AC" * n)[:n]
            add(bytes(s))
        add(_rand(rng, boundary + shift - total))                                           # this sequence ends at the boundary + shift
        assert total == boundary + shift
    add(_rand(rng, k + w))
    add(b"A" * (2 * w + k))                                                                 # ties across the last sequences
    add(_rand(rng, 2 * tile + 17))                                                          # a sequence over whole tiles
    add(b"")
    return refs


@pytest.mark.parametrize("k,w", [(8, 1), (8, 3), (11, 19), (15, 10), (31, 64), (16, 2)])
def test_index_entries_equal_the_model(pkg, k, w):
    rng = np.random.default_rng(9200 + 100 * k + w)
    _, tile = pkg.seed_sketch_shape()
    refs = _short_set(rng, k, w, tile)
    want = mref.index_entries(refs, k, w)
    R = pkg.SeqSet.new(refs)
    ix = pkg.SeedIndex.build(R, k, stream=_stream(), w=w)
    assert ix.w == w and len(ix) == len(want) > 0
    assert _entries(pkg, ix, 0, len(want)) == want
    nb = 4 ** min(k, 11)
    if w > 1:                                                                               # (the mirror's w = 1 is pmx_seed_index_build itself)
        assert ix.nbytes == 16 * len(want) + 4 * (nb + 1)
    plain = pkg.SeedIndex.build(R, k, _stream())
    every = _entries(pkg, plain, 0, len(plain))
    assert plain.w == 1 and plain.nbytes == 16 * sum(len(s) for s in refs) + 4 * (nb + 1)
    if w == 1:
        one = pkg.lib.pmx_seed_index_build_minimizers(R._handle(), k, 1, _stream())            # w = 1 through the new build: every k-mer
        assert one
        ix1 = pkg.SeedIndex(one, R, k)
        assert len(ix1) == len(plain) and _entries(pkg, ix1, 0, len(ix1)) == every == want
        assert ix1.w == 1 and ix1.nbytes == 16 * len(want) + 4 * (nb + 1) < plain.nbytes
        ix1.close()
    else:
        assert set(want) < set(every) and len(want) < len(every)
    ix.close()
    plain.close()


def test_index_of_sets_without_minimizers_and_a_wrapped_set(pkg):
    rng = np.random.default_rng(9300)
    Q = pkg.SeqSet.new([b"ACGTACGTACGTACGTACGT", b""])
    for refs in ([b""], [b"ACGT"], [b"N" * 50], [b"ACGTACG", b"ACGTACG"]):
        R = pkg.SeqSet.new(refs)
        ix = pkg.SeedIndex.build(R, 8, w=5)
        assert len(ix) == 0 and ix.nbytes in (0, 4 * (4 ** 8 + 1))
        h = pkg.seed_pairs(Q, ix, min_seeds=1)
        assert h.row_off.tolist() == [0, 0, 0] and len(h) == 0
    refs = [_rand(rng, 300), b"", _rand(rng, 5), _rand(rng, 2100)]
    buf = np.frombuffer(b"ACGTACGTACGTACGT" + b"".join(refs) + b"ACGTACGTACGTACGTACGT", dtype=np.uint8).copy()
    off = 16 + np.concatenate(([0], np.cumsum([len(s) for s in refs]))).astype(np.int64)
    d_buf, d_off = _up(buf), _up(off)
    R = pkg.SeqSet.wrap_device(d_buf.data_ptr(), d_off.data_ptr(), len(refs), len(buf), keep=(d_buf, d_off))
    ix = pkg.SeedIndex.build(R, 11, stream=_stream(), w=7)
    want = mref.index_entries(refs, 11, 7)                                                  # the bytes around the sequences are in no window
    assert len(ix) == len(want) and _entries(pkg, ix, 0, len(want)) == want


# ---- seeding end to end against the model ----------------------------------------------------------------------------------------------
class Got:
    pass


def _seed(pkg, Q, ix, nq, mq, capacity, q_first=0, **kw):
    import torch
    slots = capacity + 3
    hp = _full((slots * 32,), FILL, torch.uint8)
    hs = _full((slots,), FILL, torch.uint8)
    hd = _full((slots, 4), SENTINEL, torch.int32)
    off = _full((nq + 1 + 2,), SENTINEL, torch.int64)
    cnt = _full((2 + 2,), SENTINEL, torch.int64)
    pkg.seed_pairs_device(Q, ix, q_first, nq, mq, hp.data_ptr(), hs.data_ptr(), hd.data_ptr(), capacity, off.data_ptr(), cnt.data_ptr(),
                          stream=_stream(), **kw)
    _sync()
    g = Got()
    g.pairs, g.strand, g.off, g.counts = hp.cpu().numpy().view(ref.PAIR_DTYPE), hs.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy()
    g.seeds = hd.cpu().numpy().reshape(-1).view(ref.SEED_HIT_DTYPE)
    return g


def _same(g, want, capacity, nq):
    """row_off and counts in full and uncapped, the first min(candidates, capacity) entries the model's bytes, every entry at or behind
    `capacity` the sentinel"""
    total = int(want["row_off"][-1])
    w = min(total, capacity)
    assert g.off[:nq + 1].tolist() == want["row_off"].tolist() and (g.off[nq + 1:] == SENTINEL).all()
    assert g.counts[:2].tolist() == [total, w] and (g.counts[2:] == SENTINEL).all()
    assert g.pairs[:w].tobytes() == want["pairs"][:w].tobytes() and (g.pairs[w:].view(np.uint8) == FILL).all()
    assert g.strand[:w].tobytes() == want["strand"][:w].tobytes() and (g.strand[w:] == FILL).all()
    assert g.seeds[:w].tobytes() == want["seeds"][:w].tobytes() and (g.seeds[w:].view(np.int32) == SENTINEL).all()


def _same_host(h, want):
    total = int(want["row_off"][-1])
    assert h.n_rows == len(want["row_off"]) - 1 and h.n_passing == total and h.n_hits == len(h) == total
    assert h.row_off.tobytes() == want["row_off"].tobytes()
    assert h.pairs.tobytes() == want["pairs"].tobytes() and h.strand.tobytes() == want["strand"].tobytes()
    assert h.seeds.tobytes() == want["seeds"].tobytes()


K_MED, W_MED, OPTS_MED = 13, 5, dict(min_seeds=2, band=6, pad=12, max_occ=24)


@pytest.fixture(scope="module")
def medium():
    rng = np.random.default_rng(9400)
    refs = random_seqs(rng, 24, 1500, 3000)
    unit = _rand(rng, 9)
    refs[7] = refs[7][:800] + unit * 60 + refs[7][800:]                                     # a tandem repeat
    reads, truth = [], []
    for x in range(300):
        r = int(rng.integers(24)) if x % 25 else 7
        a = int(rng.integers(0, len(refs[r]) - 150)) if x % 25 else int(rng.integers(700, 1300))
        s = mutate(rng, refs[r][a:a + 150], sub=0.02, indel=0.005)[:150]
        strand = x & 1
        reads.append(ref.orient(s, strand))
        truth.append((r, a, strand))
    reads[5] = reads[5][:40] + b"N" + reads[5][41:]
    reads[6] = b""
    want = mref.seed(reads, refs, K_MED, W_MED, ref.BOTH, **OPTS_MED)
    for a in want.values():
        a.setflags(write=False)
    return refs, reads, truth, want


@pytest.fixture(scope="module")
def medium_dev(pkg, medium):
    refs, reads, _, _ = medium
    R, Q = pkg.SeqSet.new(refs), pkg.SeqSet.new(reads)
    return Q, R, pkg.SeedIndex.build(R, K_MED, stream=_stream(), w=W_MED)


def test_medium_equals_the_model_and_repeats(pkg, medium, medium_dev):
    refs, reads, truth, want = medium
    Q, R, ix = medium_dev
    assert len(ix) == len(mref.index_entries(refs, K_MED, W_MED)) < len(ref.index_entries(refs, K_MED)) // 2
    total = int(want["row_off"][-1])
    assert total >= 250                                                                     # (most reads find their locus)
    a = _seed(pkg, Q, ix, len(reads), 150, total + 5, **OPTS_MED)
    _same(a, want, total + 5, len(reads))
    b = _seed(pkg, Q, ix, len(reads), 150, total + 5, **OPTS_MED)
    for x, y in ((a.pairs, b.pairs), (a.strand, b.strand), (a.seeds, b.seeds), (a.off, b.off), (a.counts, b.counts)):
        assert x.tobytes() == y.tobytes()
    for mode in (ref.FORWARD, ref.REVERSE):
        one = mref.seed(reads, refs, K_MED, W_MED, mode, **OPTS_MED)
        n = int(one["row_off"][-1])
        _same(_seed(pkg, Q, ix, len(reads), 150, n + 1, strand=mode, **OPTS_MED), one, n + 1, len(reads))
    _same_host(pkg.seed_pairs(Q, ix, **OPTS_MED), want)
    # fewer seeds than the plain index finds, never other loci: every minimizer match is a k-mer match
    every = ref.seed(reads, refs, K_MED, ref.BOTH, 1, OPTS_MED["band"], OPTS_MED["pad"], 64)
    assert int(every["row_off"][-1]) >= total


@pytest.mark.parametrize("slice_rows,budget", [(1, 0), (3, 0), (0, 0), (0, 200000), (100, 180000)])
def test_slices_and_a_tiny_match_buffer_never_change_a_byte(pkg, medium, medium_dev, slice_rows, budget):
    """budget: the match buffer (test hook) -- no less than one row's worst case of 150 x 2 x 24 x 24 = 172 800 bytes, and small enough
    for the cut to fall inside the rows (they carry some 9 800 matches together, the buffer holds 8 333 or 7 500)"""
    refs, reads, _, want = medium
    Q, R, ix = medium_dev
    nq = 120 if slice_rows in (1, 3) else len(reads)                                        # (a slice costs a synchronisation)
    sub = {key: want[key][:int(want["row_off"][nq])] for key in ("pairs", "strand", "seeds")}
    sub["row_off"] = want["row_off"][:nq + 1]
    total = int(sub["row_off"][-1])
    pkg.lib.pmx_seed_match_budget(budget)
    try:
        _same(_seed(pkg, Q, ix, nq, 150, total, slice_rows=slice_rows, **OPTS_MED), sub, total, nq)
    finally:
        pkg.lib.pmx_seed_match_budget(0)


def test_capacity_is_respected_and_subranges_are_the_rows_of_the_full_run(pkg, medium, medium_dev):
    refs, reads, _, want = medium
    Q, R, ix = medium_dev
    nq, total = len(reads), int(want["row_off"][-1])
    for cap in (0, 1, total // 2, total):                                                   # nothing at or behind `capacity` is written
        _same(_seed(pkg, Q, ix, nq, 150, cap, **OPTS_MED), want, cap, nq)
    for first, n in ((0, 1), (1, 199), (299, 1), (300, 0)):
        a, b = int(want["row_off"][first]), int(want["row_off"][first + n])
        sub = {"row_off": want["row_off"][first:first + n + 1] - a, "pairs": want["pairs"][a:b], "strand": want["strand"][a:b], "seeds": want["seeds"][a:b]}
        _same(_seed(pkg, Q, ix, n, 150, b - a + 1, q_first=first, slice_rows=77, **OPTS_MED), sub, b - a + 1, n)


def test_max_occ_counts_the_entries_of_the_minimizer_index(pkg):
    rng = np.random.default_rng(9500)
    k, w = 12, 4
    unit, other = _rand(rng, k + w - 1), _rand(rng, k + w - 1)                              # one whole window each: at least one minimizer inside
    sp = [_rand(rng, 40) for _ in range(9)]
    refs = [sp[0] + unit + sp[1] + unit + sp[2] + unit + sp[3], other + sp[4] + other + sp[5] + other + sp[6] + other]
    qs = [sp[7][:20] + unit + sp[7][20:], sp[8][:20] + other + sp[8][20:]]
    idx = mref.index_dict(refs, k, w)
    occ = sorted({len(v) for v in idx.values()})
    assert occ[-1] >= 4 and 3 in occ                                                        # minimizers of `unit` 3 times, of `other` 4 times
    Q, R = pkg.SeqSet.new(qs), pkg.SeqSet.new(refs)
    ix = pkg.SeedIndex.build(R, k, stream=_stream(), w=w)
    seen = []
    for max_occ in (4, 3, 2):
        want = mref.seed(qs, refs, k, w, ref.FORWARD, min_seeds=1, band=0, pad=0, max_occ=max_occ)
        n = int(want["row_off"][-1])
        _same(_seed(pkg, Q, ix, 2, max(len(s) for s in qs), n + 2, strand=ref.FORWARD, min_seeds=1, band=0, pad=0, max_occ=max_occ), want, n + 2, 2)
        seen.append(want["row_off"].tolist())
    assert seen[0][1] >= 3 and seen[0][2] - seen[0][1] >= 4                                 # max_occ 4 keeps both
    assert seen[1][1] >= 3 and seen[1][2] == seen[1][1]                                     # 3 drops `other`'s, which have 4 entries
    assert seen[2] == [0, 0, 0]


def test_w_1_hits_equal_the_plain_index(pkg, medium):
    refs, reads, _, _ = medium
    Q, R = pkg.SeqSet.new(reads[:100]), pkg.SeqSet.new(refs)
    plain = pkg.SeedIndex.build(R, K_MED, _stream())
    inner = pkg.lib.pmx_seed_index_build_minimizers(R._handle(), K_MED, 1, _stream())
    assert inner
    one = pkg.SeedIndex(inner, R, K_MED)
    a, b = pkg.seed_pairs(Q, plain, **OPTS_MED), pkg.seed_pairs(Q, one, **OPTS_MED)
    assert len(a) > 80 and a.row_off.tobytes() == b.row_off.tobytes() and a.pairs.tobytes() == b.pairs.tobytes()
    assert a.strand.tobytes() == b.strand.tobytes() and a.seeds.tobytes() == b.seeds.tobytes()
    _same_host(a, ref.seed(reads[:100], refs, K_MED, ref.BOTH, **OPTS_MED))


# ---- the guarantee, the filter and the extension ---------------------------------------------------------------------------------------
def test_one_clean_stretch_of_w_plus_k_minus_1_letters_finds_the_locus(pkg, orc):
    """reads with one clean stretch of exactly w + k - 1 letters and a substitution at every 7th letter or closer elsewhere (no other
    k-mer survives): with min_seeds 1 each has a candidate over its planted locus, the list goes through seed_filter and align_pairs as
    it is, and the planted locus scores best"""
    rng = np.random.default_rng(9600)
    k, w, L = 15, 10, 120
    genome = _rand(rng, 60000)
    reads, truth = [], []
    for x in range(60):
        pos = int(rng.integers(0, len(genome) - L))
        a = int(rng.integers(1, L - (w + k - 1) - 1))                                       # the clean stretch [a, a + w + k - 1)
        s = bytearray(genome[pos:pos + L])
        errs = list(range(a - 1, -1, -7)) + list(range(a + w + k - 1, L, 7))
        for e in errs:
            s[e] = b"ACGT"[(b"ACGT".index(s[e]) + 1 + int(rng.integers(3))) % 4]
        assert ref.longest_clean_run(L, errs) == w + k - 1
        strand = x & 1
        reads.append(ref.orient(bytes(s), strand))
        truth.append((pos, strand))
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new([genome])
    ix = pkg.SeedIndex.build(R, k, stream=_stream(), w=w)
    hits = pkg.seed_pairs(Q, ix, strand="both", min_seeds=1, band=4, pad=20, max_occ=64)
    _same_host(hits, mref.seed(reads, [genome], k, w, ref.BOTH, min_seeds=1, band=4, pad=20, max_occ=64))
    assert hits.kind == "strand"
    planted = []
    for q, (pos, strand) in enumerate(truth):
        a, b = int(hits.row_off[q]), int(hits.row_off[q + 1])
        ok = [x for x in range(a, b) if hits.pairs[x]["r"] == 0 and hits.strand[x] == strand and
              hits.seeds[x]["diag_min"] <= pos <= hits.seeds[x]["diag_max"]]
        assert len(ok) == 1, (q, pos, strand)                                               # the guarantee
        planted.append(ok[0])
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    kept = pkg.seed_filter(Q, R, hits, pm, min_score=0)
    assert kept.kind == "strand" and set(planted) <= set(kept.source.tolist())
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    rec, cigars, begins = al.align_pairs(Q, R, hits.pairs, strand=hits.strand, cigar=True)
    assert (rec["flags"] == 0).all() and len(cigars) == len(hits)
    for q, x in enumerate(planted):
        a, b = int(hits.row_off[q]), int(hits.row_off[q + 1])
        assert rec["score"][x] == rec["score"][a:b].max() >= 2 * (w + k - 1)
