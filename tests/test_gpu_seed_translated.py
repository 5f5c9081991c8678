"""Seeding translated references (`-m gpu`): pmx_seed_index_build_translated and pmx_seed_pairs_translated_ref[_device] against the
model tests/seed_translated_ref.py -- index entries for the three strand modes at small and large keys, with sequence ends, an N and a
stop codon at every offset around a thread's tile edge and a block's first and last slot on both strands (strand 1's blocks where
they begin with one strand held and with both), and a wrapped set with
bytes in front of and behind its sequences; both modes byte for byte (row offsets, descriptors, bytes, seed records with `reserved`,
counts) under every slicing, with a tiny match buffer and a capped capacity; the frame mode against the letters road over the
host-translated six-frame set; and the candidates through the reference-side aligner roads with nothing in between.  Every comparison
is exact; every output buffer starts as a sentinel."""
import numpy as np
import pytest

import seed_letters_ref as lref
import seed_translated_ref as ref
import translate_ref_side as trs
from util import golden

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
T20, T11 = ref.table_of(ref.AA20), ref.table_of(ref.AA11)
STRANDS = {ref.FORWARD: "forward", ref.REVERSE: "reverse", ref.BOTH: "both"}
TILE, BLOCK = 48, 256 * 48                                                                   # entry slots per thread and per block of the extraction


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


def _random_nt(rng, n):
    return bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, size=n))


def _mutate_nt(rng, nt, rate):
    s = bytearray(nt)
    for x in np.nonzero(rng.random(len(s)) < rate)[0]:
        s[x] = b"ACGT"[(b"ACGT".index(s[x]) + 1 + int(rng.integers(3))) % 4]
    return bytes(s)


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


def _index_set(rng, k):
    """40 contigs of 0 .. 2 000 nt (most below 400, so that nearly every tile of 48 slots near them holds a sequence end): lengths
    0 .. 3 and 3 k - 1 .. 3 k + 2, an N at the first and last byte and inside, lower case with U, stop codons wherever random
    nucleotides put them (one codon in 21)"""
    seqs = [b"", b"A", b"AC", b"ACG"] + [_random_nt(rng, n) for n in (3 * k - 1, 3 * k, 3 * k + 1, 3 * k + 2)]
    body = _random_nt(rng, 300)
    seqs += [b"N" + body, body + b"N", body[:150] + b"N" + body[151:], body.lower().replace(b"t", b"u"), b"N" * 70, b""]
    while len(seqs) < 39:
        n = int(rng.integers(0, 2001)) if len(seqs) % 5 == 0 else int(rng.integers(0, 401))
        s = bytearray(_random_nt(rng, n))
        if n and rng.random() < 0.3:
            s[int(rng.integers(n))] = ord("NnRY-"[int(rng.integers(5))])
        seqs.append(bytes(s))
    return seqs + [_random_nt(rng, 3 * k)]


@pytest.mark.parametrize("name,table,k,strand_mode", [("aa11", T11, 3, ref.BOTH), ("aa11", T11, 15, ref.BOTH), ("aa20", T20, 12, ref.FORWARD),
                                                      ("aa20", T20, 4, ref.REVERSE), ("aa11", T11, 9, ref.REVERSE), ("aa20", T20, 6, ref.BOTH)])
def test_index_entries_equal_the_model(pkg, name, table, k, strand_mode):
    """key bits 12, 60, 60, 20, 36, 30"""
    rng = np.random.default_rng(9000 + k)
    refs = _index_set(rng, k)
    want = ref.index_entries(refs, k, table, strand_mode)
    assert len(want) > 1000
    R = pkg.SeqSet.new(refs)
    ix = pkg.SeedIndex.build(R, k, alphabet=name, translated=STRANDS[strand_mode], stream=_stream())
    assert ix.bits == ref.bits_of(table) and len(ix) == len(want) and ix.strands == STRANDS[strand_mode]
    assert _entries(pkg, ix, 0, len(want)) == want
    for first, count in ((0, 1), (len(want) - 1, 1), (17, 300), (len(want), 0)):
        assert _entries(pkg, ix, first, count) == want[first:first + count]
    ix.close()


EDGE_BYTES = 4 * BLOCK + 100
EDGE_TILES = -(-EDGE_BYTES // TILE)                                                          # threads per strand of the extraction: 1027


def _block_edges(strand_mode, strand):
    """the slots at which a block of the extraction begins on `strand`.  A thread is (strand_local, tile): with one strand held the
    thread number is the tile, so blocks begin at multiples of BLOCK; with both, strand 1's threads are EDGE_TILES + tile, so its
    blocks begin at tiles 256 j - EDGE_TILES: 253, 509, 765, 1021"""
    first = EDGE_TILES if strand_mode == ref.BOTH and strand == 1 else 0
    return [(256 * j - first) * TILE for j in range(1, 9) if 0 < (256 * j - first) * TILE < EDGE_BYTES]


def _edge_set(rng, d):
    """(sequences, features) -- four blocks and a little of random nucleotides in five sequences, the last one ending at `bytes`
    exactly, with a sequence end, an N and a stop codon at offset d from a tile edge and from a block's first slot (d < 0: the slots
    before it, the previous block's last ones) -- on strand 0 at the multiples of BLOCK, on strand 1 both at the multiples of BLOCK
    (where its blocks begin when the index holds the reverse strand alone) and at tiles 253, 509, 765, 1021 (where they begin when it
    holds both).  A feature for slot p of strand 1 is written at the stored byte b + e - 1 - p of the sequence [b, e) that holds p,
    which is what strand 1 reads there; a sequence end is an end of both strands' slots.  features: (kind, strand, slot)."""
    T = TILE
    e1 = _block_edges(ref.BOTH, 1)
    assert e1 == [253 * T, 509 * T, 765 * T, 1021 * T] and _block_edges(ref.REVERSE, 1) == _block_edges(ref.BOTH, 0) == [BLOCK, 2 * BLOCK, 3 * BLOCK, 4 * BLOCK]
    ends = [5 * T + d, e1[0] + d, BLOCK + d, 700 * T + d, EDGE_BYTES]
    begs = [0] + ends[:-1]
    buf = bytearray(_random_nt(rng, EDGE_BYTES))
    features = [("end", s, e) for e in ends[:-1] for s in (0, 1)]

    def stored(strand, p, n):
        """the stored bytes, ascending, of slots p .. p + n - 1 of `strand`, all inside one sequence"""
        x = next(x for x in range(len(ends)) if begs[x] <= p < ends[x])
        assert p + n <= ends[x], (p, n)
        lo = p if strand == 0 else begs[x] + ends[x] - 1 - (p + n - 1)
        assert begs[x] <= lo and lo + n <= ends[x]
        return lo

    for strand, p in ((0, 20 * T + d), (0, 2 * BLOCK + d), (1, 29 * T + d), (1, 2 * BLOCK + d), (1, e1[1] + d), (1, e1[3] + d)):
        buf[stored(strand, p, 1)] = ord("N")
        features.append(("N", strand, p))
    for strand, p in ((0, 40 * T + d), (0, 3 * BLOCK + d), (1, 45 * T + d), (1, 3 * BLOCK + 9 * T + d), (1, 3 * BLOCK + d), (1, e1[2] + d)):
        lo = stored(strand, p, 3)
        buf[lo:lo + 3] = b"TTA" if strand else b"TAA"                                         # strand 1 reads it downwards, complemented: TAA
        features.append(("stop", strand, p))
    return [bytes(buf[a:b]) for a, b in zip(begs, ends)], features


@pytest.mark.parametrize("d", [-3, -2, -1, 0, 1, 2, 3])
def test_the_edge_set_holds_what_it_says(d):
    """on the CPU, by the definitions alone: every feature is where (kind, strand, slot) says -- the oriented sequence of the strand
    has the N, or the stop codon's three letters, at that slot -- and every kind sits at offset d from a block's first slot of strand 0,
    of strand 1 held alone and of strand 1 held with strand 0, and from a tile edge that is no block edge"""
    refs, features = _edge_set(np.random.default_rng(9100 + d), d)
    off = np.cumsum([0] + [len(s) for s in refs])
    assert off[-1] == EDGE_BYTES
    for kind, strand, p in features:
        x = int(np.searchsorted(off, p, side="right")) - 1
        o = lref.revcomp(refs[x]) if strand else refs[x]
        at = p - int(off[x])
        if kind == "end":
            assert at == 0
        elif kind == "N":
            assert o[at:at + 1] == b"N"
        else:
            assert o[at:at + 3] == b"TAA"
    for kind in ("end", "N", "stop"):
        where = {(s, p - d) for k, s, p in features if k == kind}
        assert any(s == 0 and p in _block_edges(ref.FORWARD, 0) for s, p in where), kind
        assert any(s == 1 and p in _block_edges(ref.REVERSE, 1) for s, p in where), kind
        assert any(s == 1 and p in _block_edges(ref.BOTH, 1) for s, p in where), kind
        for strand in (0, 1):
            assert any(s == strand and p % TILE == 0 and p % BLOCK and p not in _block_edges(ref.BOTH, 1) for s, p in where), (kind, strand)


@pytest.mark.parametrize("strand_mode", [ref.BOTH, ref.FORWARD, ref.REVERSE])
@pytest.mark.parametrize("d", [-3, -2, -1, 0, 1, 2, 3])
def test_index_entries_at_tile_and_block_edges(pkg, d, strand_mode):
    refs, _ = _edge_set(np.random.default_rng(9100 + d), d)
    want = ref.index_entries(refs, 4, T11, strand_mode)
    R = pkg.SeqSet.new(refs)
    ix = pkg.SeedIndex.build(R, 4, alphabet="aa11", translated=STRANDS[strand_mode], stream=_stream())
    assert len(ix) == len(want) and _entries(pkg, ix, 0, len(want)) == want
    ix.close()


def test_wrapped_set_with_bytes_around_its_sequences(pkg):
    """offsets that start at 50 and end 70 bytes before `bytes`: the bytes in front and behind are good nucleotides that no entry may
    come from, on either strand"""
    import torch
    rng = np.random.default_rng(9200)
    refs = [_random_nt(rng, n) for n in (130, 0, 47, 96, 11, 200)]
    raw = _random_nt(rng, 50) + b"".join(refs) + _random_nt(rng, 70)
    off = np.cumsum([50] + [len(s) for s in refs]).astype(np.int64)
    d_buf = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(_dev())
    d_off = torch.from_numpy(off).to(_dev())
    R = pkg.SeqSet.wrap_device(d_buf.data_ptr(), d_off.data_ptr(), len(refs), len(raw), keep=(d_buf, d_off))
    for strand_mode in (ref.FORWARD, ref.REVERSE, ref.BOTH):
        want = ref.index_entries(refs, 4, T20, strand_mode)
        ix = pkg.SeedIndex.build(R, 4, alphabet="aa20", translated=STRANDS[strand_mode], stream=_stream())
        assert len(want) > 300 and len(ix) == len(want) and _entries(pkg, ix, 0, len(want)) == want
        ix.close()


# ---- seeding ---------------------------------------------------------------------------------------------------------------------------
K_MED, MQ_MED = 4, 120
OPTS = {ref.REF_FRAMES: dict(min_seeds=2, band=4, pad=8, max_occ=3), ref.REF_CODONS: dict(min_seeds=2, band=12, pad=20, max_occ=3)}
REF_ARG = {ref.REF_FRAMES: "frames", ref.REF_CODONS: "codons"}


class Got:
    pass


def _seed(pkg, Q, ix, nq, mq, capacity, mode, q_first=0, with_seeds=True, **kw):
    import torch
    slots = capacity + 3
    hp = _full((slots * 32,), FILL, torch.uint8)
    hs = _full((slots,), FILL, torch.uint8)
    hd = _full((slots, 4), SENTINEL, torch.int32) if with_seeds else None
    off = _full((nq + 1 + 2,), SENTINEL, torch.int64)
    cnt = _full((2 + 2,), SENTINEL, torch.int64)
    pkg.seed_pairs_device(Q, ix, q_first, nq, mq, hp.data_ptr(), hs.data_ptr(), hd.data_ptr() if with_seeds else None, capacity,
                          off.data_ptr(), cnt.data_ptr(), stream=_stream(), ref_frames=REF_ARG[mode], **kw)
    _sync()
    g = Got()
    g.pairs, g.byte, g.off, g.counts = hp.cpu().numpy().view(ref.PAIR_DTYPE), hs.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy()
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
    assert g.byte[:w].tobytes() == want["byte"][:w].tobytes() and (g.byte[w:] == FILL).all()
    if g.seeds is not None:
        assert g.seeds[:w].tobytes() == want["seeds"][:w].tobytes() and (g.seeds[w:].view(np.int32) == SENTINEL).all()


def _same_host(h, want, mode, stored=None):
    total = int(want["row_off"][-1])
    stored = total if stored is None else stored
    assert h.n_rows == len(want["row_off"]) - 1 and h.n_passing == total and h.n_hits == len(h) == stored
    assert h.row_off.tobytes() == want["row_off"].tobytes()
    assert h.pairs.tobytes() == want["pairs"][:stored].tobytes() and h.seeds.tobytes() == want["seeds"][:stored].tobytes()
    if mode == ref.REF_FRAMES:
        assert h.frame.tobytes() == want["byte"][:stored].tobytes() and not h.strand.any() and len(h.strand) == stored
    else:
        assert h.frame is None and h.strand.tobytes() == want["byte"][:stored].tobytes()


@pytest.fixture(scope="module")
def medium():
    """60 proteins of 0 .. 130 letters (one above max_qlen) and 40 contigs of 0 .. 700 nt that carry back-translated pieces of them at
    every frame offset on both strands, some with substitutions, some at a contig's very ends (clipped windows), some with one
    nucleotide deleted or inserted; a motif at max_occ = 3 entries and one above it; computed once, never changed"""
    rng = np.random.default_rng(9300)
    prots = [lref.random_protein(rng, int(rng.integers(30, 111))) for _ in range(54)]
    at, above = b"MKWFPHCYG", b"GYCHPFWKM"
    for x in range(3):
        prots[10 + x] = prots[10 + x][:20] + at + prots[10 + x][20:]
    for x in range(4):
        prots[20 + x] = prots[20 + x][:15] + above + prots[20 + x][15:]
    prots += [b"", b"MK", prots[0][:12] + b"X" + prots[1][:20], b"*" + prots[2][:25], prots[3].lower(), prots[4] + prots[5][:60]]
    assert len(prots) == 60 and len(prots[-1]) > MQ_MED

    def piece(i, a, n, rate=0.0):
        return _mutate_nt(rng, lref.back_translate(prots[i][a:a + n], rng), rate)

    contigs = []
    for x in range(26):
        i = int(rng.integers(54))
        n = int(rng.integers(10, min(60, len(prots[i])) + 1))
        a = int(rng.integers(0, len(prots[i]) - n + 1))
        gene = piece(i, a, n, 0.03 if x % 3 == 0 else 0.0)
        if x % 4 == 1:
            gene = gene[:len(gene) // 2] + gene[len(gene) // 2 + 1:]                          # one nucleotide deleted
        if x % 4 == 3:
            gene = gene[:len(gene) // 2] + b"G" + gene[len(gene) // 2:]                       # one inserted
        lead = 0 if x % 6 == 0 else int(rng.integers(0, 200))                                 # (0: the gene at the contig's first byte)
        tail = 0 if x % 6 == 3 else int(rng.integers(0, 200))
        c = _random_nt(rng, lead) + gene + _random_nt(rng, tail)
        contigs.append(lref.revcomp(c) if x % 2 else c)
    for x, i in enumerate((10, 11, 12, 20, 21, 22, 23)):                                      # the motifs, one copy each, alternating strands
        a = 14 if i < 20 else 9
        c = _random_nt(rng, 30 + x) + piece(i, a, 22) + _random_nt(rng, 40)
        contigs.append(lref.revcomp(c) if x % 2 else c)
    s = piece(40, 5, 40)
    contigs += [s[:30] + b"TAA" + s[33:], s[:31] + b"N" + s[32:], s.lower().replace(b"t", b"u"), b"", b"ACGTACGTACG",
                piece(41, 0, 30) + piece(42, 3, 25), _random_nt(rng, 3 * K_MED - 1)]
    assert len(contigs) == 40
    idx = ref.index_dict(ref.index_entries(contigs, K_MED, T11, ref.BOTH))
    occ = {key: len(v) for key, v in idx.items()}
    key_of = lambda m: ref.kmers(m, K_MED, T11)[0][1]
    assert occ[key_of(at)] == 3 and occ[key_of(above)] == 4
    matcher = ref.key_matches(idx, K_MED, T11, 3)
    cache = {}

    def model(mode, **kw):
        o = dict(OPTS[mode])
        o.update(kw)
        key = (mode, tuple(sorted(o.items())))
        if key not in cache:
            cache[key] = ref.seed(prots, contigs, K_MED, T11, mode, ref.BOTH, o["min_seeds"], o["band"], o["pad"], o["max_occ"],
                                  max_qlen=o.get("max_qlen", MQ_MED), matcher=matcher)
        return cache[key]
    return prots, contigs, model


@pytest.fixture(scope="module")
def medium_dev(pkg, medium):
    prots, contigs, _ = medium
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(contigs)
    return Q, R, pkg.SeedIndex.build(R, K_MED, alphabet="aa11", translated="both", stream=_stream())


def test_the_inputs_are_not_empty(medium):
    """on the CPU: the model's own result has candidates for most rows, in every sequence frame and on both strands, windows clipped at
    both contig ends, and the row above max_qlen has none"""
    prots, contigs, model = medium
    fr, co = model(ref.REF_FRAMES), model(ref.REF_CODONS)
    assert (np.diff(fr["row_off"]) > 0).sum() >= 20 and (np.diff(co["row_off"]) > 0).sum() >= 20
    assert sorted(set(fr["seeds"]["reserved"].tolist())) == [0, 1, 2, 3, 4, 5] and sorted(set(fr["byte"].tolist())) == [0, 3]
    assert sorted(set(co["byte"].tolist())) == [0, 1] and not co["seeds"]["reserved"].any()
    rlens = np.array([len(c) for c in contigs])
    for w in (fr, co):
        assert (w["pairs"]["r_beg"] == 0).any() and (w["pairs"]["r_beg"] + w["pairs"]["r_len"] == rlens[w["pairs"]["r"]]).any()
        assert (w["pairs"]["r_len"] > 0).all() and (w["pairs"]["r_beg"] >= 0).all()
        assert (w["pairs"]["r_beg"] + w["pairs"]["r_len"] <= rlens[w["pairs"]["r"]]).all()
    assert (fr["pairs"]["r_len"] % 3 == 0).all()
    assert fr["row_off"][-1] == fr["row_off"][-2] and np.diff(model(ref.REF_FRAMES, max_qlen=None)["row_off"])[-1] > 0


@pytest.mark.parametrize("mode", [ref.REF_FRAMES, ref.REF_CODONS])
def test_both_modes_equal_the_model(pkg, medium, medium_dev, mode):
    prots, contigs, model = medium
    Q, R, ix = medium_dev
    want = model(mode)
    total = int(want["row_off"][-1])
    assert total > 0
    _same(_seed(pkg, Q, ix, len(prots), MQ_MED, total + 2, mode, **OPTS[mode]), want, total + 2, len(prots))
    _same_host(pkg.seed_pairs(Q, ix, ref_frames=REF_ARG[mode], **OPTS[mode]), model(mode, max_qlen=None), mode)    # max_qlen from the rows


@pytest.mark.parametrize("strand_mode", [ref.FORWARD, ref.REVERSE, ref.BOTH])
def test_frame_mode_equals_the_letters_road_over_the_six_frame_set(pkg, medium, strand_mode):
    """the defining equivalence on the device: a letters index of the host-translated R6, seed_pairs(frames="letters"), the mapping"""
    prots, contigs, _ = medium
    o = dict(min_seeds=2, band=4, pad=8, max_occ=3)
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(contigs)
    ix = pkg.SeedIndex.build(R, K_MED, alphabet="aa11", translated=STRANDS[strand_mode], stream=_stream())
    R6 = pkg.SeqSet.new(ref.r6(contigs, strand_mode))
    ix6 = pkg.SeedIndex.build(R6, K_MED, alphabet="aa11", stream=_stream())
    assert len(ix) == len(ix6) > 0
    mine = pkg.seed_pairs(Q, ix, ref_frames="frames", **o)
    theirs = pkg.seed_pairs(Q, ix6, frames="letters", **o)
    mapped = ref.from_letters({"row_off": theirs.row_off, "pairs": theirs.pairs, "seeds": theirs.seeds}, contigs)
    assert len(mine) > 0
    _same_host(mine, mapped, ref.REF_FRAMES)
    count = len(contigs)
    a, b = _entries(pkg, ix, 0, len(ix)), _entries(pkg, ix6, 0, len(ix6))
    assert sorted((key, (3 * (sr // count) + x % 3) * count + sr % count, x // 3) for key, sr, x in a) == b


@pytest.mark.parametrize("mode", [ref.REF_FRAMES, ref.REF_CODONS])
@pytest.mark.parametrize("slice_rows", [1, 3, 700])
@pytest.mark.parametrize("budget", [1 << 20, 300000])
def test_slices_and_a_tiny_match_buffer_never_change_a_byte(pkg, medium, medium_dev, mode, slice_rows, budget):
    """budget: the match buffer (test hook) -- one row's worst case is 120 x 3 x 24 = 8 640 bytes"""
    prots, contigs, model = medium
    Q, R, ix = medium_dev
    want = model(mode)
    total = int(want["row_off"][-1])
    pkg.lib.pmx_seed_match_budget(budget)
    try:
        _same(_seed(pkg, Q, ix, len(prots), MQ_MED, total, mode, slice_rows=slice_rows, **OPTS[mode]), want, total, len(prots))
    finally:
        pkg.lib.pmx_seed_match_budget(0)


def test_capacity_subranges_and_the_host_entry(pkg, medium, medium_dev):
    prots, contigs, model = medium
    Q, R, ix = medium_dev
    nq = len(prots)
    for mode in (ref.REF_FRAMES, ref.REF_CODONS):
        want = model(mode)
        total = int(want["row_off"][-1])
        for cap in (0, 1, total // 2, total + 9):
            _same(_seed(pkg, Q, ix, nq, MQ_MED, cap, mode, with_seeds=cap != 1, **OPTS[mode]), want, cap, nq)
        for first, n in ((0, 1), (1, 40), (50, 10), (59, 1), (60, 0), (7, 0)):
            a, b = int(want["row_off"][first]), int(want["row_off"][first + n])
            sub = {"row_off": want["row_off"][first:first + n + 1] - a, "pairs": want["pairs"][a:b], "byte": want["byte"][a:b], "seeds": want["seeds"][a:b]}
            _same(_seed(pkg, Q, ix, n, MQ_MED, b - a + 1, mode, q_first=first, slice_rows=7, **OPTS[mode]), sub, b - a + 1, n)
        # far more than two candidates per row: every match a candidate of its own -- the host entry's second, exact-size run
        many = model(mode, min_seeds=1, band=0, pad=0, max_qlen=None)
        n_many = int(many["row_off"][-1])
        assert n_many > 2 * (2 * nq + 16)
        o = dict(min_seeds=1, band=0, pad=0, max_occ=3, ref_frames=REF_ARG[mode])
        _same_host(pkg.seed_pairs(Q, ix, **o), many, mode)
        _same_host(pkg.seed_pairs(Q, ix, max_hits=n_many - 3, slice_rows=16, **o), many, mode, stored=n_many - 3)
        _same_host(pkg.seed_pairs(Q, ix, max_hits=7, **o), many, mode, stored=7)
    with pytest.raises(pkg.BatchError, match="worst case"):                                  # refused before any GPU work
        pkg.lib.pmx_seed_match_budget(1 << 16)
        try:
            pkg.seed_pairs(Q, ix, max_occ=65535, ref_frames="frames")
        finally:
            pkg.lib.pmx_seed_match_budget(0)


def test_nothing_to_find(pkg):
    """proteins longer than a contig and contigs shorter than 3 k: no candidate, offsets all equal, nothing written"""
    import torch
    rng = np.random.default_rng(9400)
    k = 5
    contigs = [_random_nt(rng, n) for n in (0, 1, 3 * k - 1, 14, 7)] + [lref.back_translate(lref.random_protein(rng, 8), rng)]
    prots = [lref.random_protein(rng, 40), lref.random_protein(rng, 9), b"", tr_protein(contigs[-1])]
    R, Q = pkg.SeqSet.new(contigs), pkg.SeqSet.new(prots)
    ix = pkg.SeedIndex.build(R, k, alphabet="aa20", translated="both", stream=_stream())
    assert len(ix) == len(ref.index_entries(contigs, k, T20, ref.BOTH)) > 0                   # the 24-nt contig has k-mers
    for mode in (ref.REF_FRAMES, ref.REF_CODONS):
        want = ref.seed(prots, contigs, k, T20, mode, ref.BOTH, 2, 8, 16, 64, max_qlen=40)
        g = _seed(pkg, Q, ix, 4, 40, 8, mode, min_seeds=2, band=8, pad=16, max_occ=64)
        _same(g, want, 8, 4)
        # rows 0 .. 2 have nothing; row 3, the contig's own 8 letters, is the one candidate: longer proteins find nothing in it
        assert want["row_off"].tolist() == [0, 0, 0, 0, 1]
    short = pkg.SeqSet.new(contigs[:5])
    ix2 = pkg.SeedIndex.build(short, k, alphabet="aa20", translated="both", stream=_stream())
    assert len(ix2) == 0
    for mode in ("frames", "codons"):
        off = _full((4 + 1 + 2,), SENTINEL, torch.int64)
        cnt = _full((2 + 2,), SENTINEL, torch.int64)
        pkg.seed_pairs_device(Q, ix2, 0, 4, 40, None, None, None, 0, off.data_ptr(), cnt.data_ptr(), min_seeds=1, stream=_stream(), ref_frames=mode)
        _sync()
        assert off.cpu().tolist() == [0, 0, 0, 0, 0, SENTINEL, SENTINEL] and cnt.cpu().tolist() == [0, 0, SENTINEL, SENTINEL]
        h = pkg.seed_pairs(Q, ix2, min_seeds=1, ref_frames=mode)
        assert h.row_off.tolist() == [0, 0, 0, 0, 0] and len(h) == 0 and h.n_passing == 0


def tr_protein(nt):
    return trs.translate(nt, 0)


# ---- into the aligners -----------------------------------------------------------------------------------------------------------------
K_AL, OPEN, EXT, SHIFT = 6, 11, 1, 15
N_PLANTED = 20
PLANTED_SEED = 9500


def planted_inputs(seed):
    """N_PLANTED contigs of 1 .. 3 kb, contig i carrying the back-translation of protein i (80 .. 150 letters) with 5 % nucleotide
    substitutions, odd ones on the reverse strand; `cut`: the same contigs with the gene's middle nucleotide deleted.  g0: the gene's
    first nucleotide in oriented coordinates of its strand."""
    rng = np.random.default_rng(seed)
    prots = [lref.random_protein(rng, int(rng.integers(80, 151))) for _ in range(N_PLANTED)]
    whole, cut, g0 = [], [], []
    for i, p in enumerate(prots):
        gene = _mutate_nt(rng, lref.back_translate(p, rng), 0.05)
        total = int(rng.integers(1000, 3001))
        lead = int(rng.integers(0, total - len(gene) + 1))
        a, b = _random_nt(rng, lead), _random_nt(rng, total - len(gene) - lead)
        mid = len(gene) // 2
        w, c = a + gene + b, a + gene[:mid] + gene[mid + 1:] + b
        whole.append(lref.revcomp(w) if i % 2 else w)
        cut.append(lref.revcomp(c) if i % 2 else c)
        g0.append(lead)
    return prots, whole, cut, g0


def planted_model(seed):
    prots, whole, cut, g0 = planted_inputs(seed)
    o = dict(min_seeds=2, pad=8, max_occ=64)
    m_cut = ref.key_matches(ref.index_dict(ref.index_entries(cut, K_AL, T11, ref.BOTH)), K_AL, T11, 64)
    frames = ref.seed(prots, whole, K_AL, T11, ref.REF_FRAMES, ref.BOTH, band=4, **o)
    cut_frames = ref.seed(prots, cut, K_AL, T11, ref.REF_FRAMES, ref.BOTH, band=4, matcher=m_cut, **o)
    cut_codons = ref.seed(prots, cut, K_AL, T11, ref.REF_CODONS, ref.BOTH, min_seeds=2, band=12, pad=24, max_occ=64, matcher=m_cut)
    return prots, whole, cut, g0, frames, cut_frames, cut_codons


def _rows(w, q):
    return range(int(w["row_off"][q]), int(w["row_off"][q + 1]))


def planted_codon_candidate(co, fr, q, g0):
    """(the codon candidate of planted pair q, the seed counts of the frame candidates inside its diagonals): the candidate of (q, r = q)
    on the planted strand whose nucleotide diagonals hold D = g0 (in front of the deleted nucleotide) and g0 - 1 (behind it); a frame
    candidate of sequence frame g lies inside it when 3 d + g % 3 does for its d_min and d_max"""
    s = q % 2
    mine = [x for x in _rows(co, q) if co["pairs"][x]["r"] == q and co["byte"][x] == s and
            co["seeds"][x]["diag_min"] <= g0[q] - 1 and co["seeds"][x]["diag_max"] >= g0[q]]
    if len(mine) != 1:
        return None, []
    lo, hi = int(co["seeds"][mine[0]]["diag_min"]), int(co["seeds"][mine[0]]["diag_max"])
    inside = []
    for x in _rows(fr, q):
        g = int(fr["seeds"][x]["reserved"])
        if fr["pairs"][x]["r"] == q and g // 3 == s and lo <= 3 * int(fr["seeds"][x]["diag_min"]) + g % 3 and \
                3 * int(fr["seeds"][x]["diag_max"]) + g % 3 <= hi:
            inside.append(int(fr["seeds"][x]["n_seeds"]))
    return mine[0], inside


@pytest.fixture(scope="module")
def planted():
    """PLANTED_SEED: the codon road's seed-count comparison needs every planted pair to keep at least min_seeds 6-mers on both sides of
    the deleted nucleotide (two frame candidates inside the one codon candidate); protein seeding found about one input in a hundred
    of its recipe (halves of 25 codons) without them.  Here a half has 40 .. 75 codons: generator seeds 9500 .. 9519 were run on the
    CPU through planted_model() and all twenty keep both halves (at 9503 and 9512 a chance match adds a third, two-seed frame
    candidate inside one codon candidate, which the comparison allows).  9500 is the first of them; the test asserts the condition
    on the model before it looks at the device."""
    return planted_model(PLANTED_SEED)


def _b62(pkg, orc):
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))


def test_frame_road_into_align_pairs(pkg, orc, planted):
    prots, whole, cut, g0, want, _, _ = planted
    for q in range(N_PLANTED):                                                               # on the model: the planted gene is a candidate
        g = 3 * (q % 2) + g0[q] % 3
        assert any(want["pairs"][x]["r"] == q and want["seeds"][x]["reserved"] == g and
                   want["seeds"][x]["diag_min"] <= g0[q] // 3 <= want["seeds"][x]["diag_max"] for x in _rows(want, q)), q
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(whole)
    ix = pkg.SeedIndex.build(R, K_AL, alphabet="aa11", translated="both", stream=_stream())
    hits = pkg.seed_pairs(Q, ix, min_seeds=2, band=4, pad=8, max_occ=64, ref_frames="frames")
    _same_host(hits, want, ref.REF_FRAMES)
    pm, om = _b62(pkg, orc)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(OPEN).gap_extend(EXT).build()
    rec, frames = al.align_pairs(Q, R, hits.pairs, ref_frame=hits.frame)
    assert frames.tobytes() == hits.frame.tobytes() and (rec["flags"] == 0).all()
    strings = trs.resolve(prots, whole, hits.pairs, hits.frame.tolist())                              # the protein, the host-translated window
    assert all(s is not None for s in strings)
    qb, qo = orc.pack([s[0] for s in strings])
    rb, ro = orc.pack([s[1] for s in strings])
    full = orc.align_batch(orc.SW, qb, qo, rb, ro, OPEN, EXT, om)
    assert (rec["score"] == full[:, 0]).all() and (rec["end_query"] == full[:, 1]).all() and (rec["end_ref"] == full[:, 2]).all()
    assert rec["score"].max() > 300


def test_codon_road_into_the_frameshift_ref_entries(pkg, planted):
    prots, whole, cut, g0, _, fr, co = planted
    found = []
    for q in range(N_PLANTED):                                                               # on the model first
        x, inside = planted_codon_candidate(co, fr, q, g0)
        assert x is not None, q
        n = int(co["seeds"][x]["n_seeds"])
        assert len(inside) >= 2 and all(n > v for v in inside) and n >= sum(inside), (q, n, inside)   # both halves kept seeds: strictly more
        # the candidate covers the whole gene: its oriented window against [g0, g0 + 3 L - 1)
        N, p = len(cut[q]), co["pairs"][x]
        lo = int(p["r_beg"]) if q % 2 == 0 else N - int(p["r_beg"]) - int(p["r_len"])
        assert lo <= g0[q] and g0[q] + 3 * len(prots[q]) - 1 <= lo + int(p["r_len"]), q
        found.append((q, x, lo))
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(cut)
    ix = pkg.SeedIndex.build(R, K_AL, alphabet="aa11", translated="both", stream=_stream())
    hits = pkg.seed_pairs(Q, ix, min_seeds=2, band=12, pad=24, max_occ=64, ref_frames="codons")
    _same_host(hits, co, ref.REF_CODONS)
    _same_host(pkg.seed_pairs(Q, ix, min_seeds=2, band=4, pad=8, max_occ=64, ref_frames="frames"), fr, ref.REF_FRAMES)
    al = pkg.Aligner.new().local().matrix(pkg.Matrix.from_name("blosum62")).gap_open(OPEN).gap_extend(EXT).build()
    rec, strand = al.align_pairs(Q, R, hits.pairs, ref_frameshift=SHIFT, ref_strand=hits.strand)
    rec2, cigars, begins, strand2 = al.align_pairs_frameshift_ref_cigar(Q, R, hits.pairs, SHIFT, ref_strand=hits.strand)
    assert rec.tobytes() == rec2.tobytes() and strand.tobytes() == strand2.tobytes() == hits.strand.tobytes() and (rec["flags"] == 0).all()
    for q, x, lo in found:
        # the path crosses the deleted nucleotide, so it has a '/', begins in front of it and ends behind it; a local path may run a
        # few chance letters past the gene: 10 letters are allowed on either side
        L, gap = len(prots[q]), g0[q] + (3 * len(prots[q])) // 2
        beg, end = lo + int(begins[x][1]), lo + int(rec["end_ref"][x])
        print("pair %d: codon candidate %d seeds, cigar %s, nucleotides %d .. %d of gene %d .. %d" %
              (q, int(co["seeds"][x]["n_seeds"]), cigars[x], beg, end, g0[q], g0[q] + 3 * L - 2))
        assert "/" in cigars[x], (q, cigars[x])
        assert g0[q] - 30 <= beg < gap < end <= g0[q] + 3 * L - 2 + 30, (q, beg, end)
        assert 0 <= int(begins[x][0]) < L // 2 < int(rec["end_query"][x]) < L
