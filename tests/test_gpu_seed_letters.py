"""Protein seeding (`-m gpu`): pmx_seed_index_build_letters and pmx_seed_pairs_letters[_device] against the model
tests/seed_letters_ref.py -- index entries at the key-width boundaries and the sequence ends, and the candidates of every query mode
byte for byte: row offsets, descriptors, frame / strand bytes, seed records and counts, under every slicing, with a tiny match buffer
and a capped capacity -- and the candidates through the two aligner roads with nothing in between.  Every comparison is exact; every
output buffer starts as a sentinel."""
import numpy as np
import pytest

import seed_letters_ref as ref
import translate_ref as tr
from util import golden

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
T20, T11 = ref.table_of(ref.AA20), ref.table_of(ref.AA11)
T1 = ref.table_of(["ACDEFGHIKL", "MNPQRSTVWY"])                                             # two groups: one bit per letter
CUSTOM_CODE = bytearray(tr.CODE_STD)
CUSTOM_CODE[16 * 0 + 4 * 3 + 2] = ord("W")                                                  # TGA reads as W, as in NCBI table 4
CUSTOM_CODE[16 * 2 + 4 * 3 + 0] = ord("*")                                                  # AGT is a stop here
CUSTOM_CODE = bytes(CUSTOM_CODE)


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
    """about 200 sequences of 0 .. 120 letters: empty ones, lengths k - 1, k and k + 1, invalid letters at the first and last position
    of a sequence and beside its ends, lower case, the lowest and the highest key; with these lengths nearly every thread's tile of 16
    positions holds a sequence boundary"""
    body = ref.random_protein(rng, 3 * k)
    seqs = [b"", ref.random_protein(rng, k - 1), ref.random_protein(rng, k), ref.random_protein(rng, k + 1), b"", b"X" + body[:k],
            body[:k - 1] + b"*", body[:k] + b"X" + body[k:2 * k], b"*" + body[:k] + b"B", b"K" * (k + 2), b"A" * k + b"a", body.lower(),
            b"X" * 40, b"", b"Z"]
    while len(seqs) < 200:
        s = bytearray(ref.random_protein(rng, int(rng.integers(0, 121))))
        if len(s) and rng.random() < 0.3:
            s[int(rng.integers(len(s)))] = ord("X*BZ-"[int(rng.integers(5))])
        if len(s) and rng.random() < 0.1:
            s[-1] = ord("*")
        seqs.append(bytes(s))
    return seqs + [ref.random_protein(rng, k), b""]


@pytest.mark.parametrize("name,table,k", [("aa11", T11, 3), ("aa11", T11, 15), ("aa20", T20, 12), ("bit", T1, 31), ("aa20", T20, 4)])
def test_index_entries_equal_the_model(pkg, name, table, k):
    rng = np.random.default_rng(8000 + k)
    refs = _index_set(rng, k)
    want = ref.index_entries(refs, k, table)
    assert len(want) > 1000 and want[0][0] == 0                                             # K K K .. / A A A ..: the lowest key
    R = pkg.SeqSet.new(refs)
    ix = pkg.SeedIndex.build(R, k, alphabet=name if name != "bit" else table, stream=_stream())
    assert ix.bits == ref.bits_of(table) and len(ix) == len(want)
    assert _entries(pkg, ix, 0, len(want)) == want
    for first, count in ((0, 1), (len(want) - 1, 1), (17, 300), (len(want), 0)):
        assert _entries(pkg, ix, first, count) == want[first:first + count]
    ix.close()


def test_all_invalid_set_and_zero_offsets(pkg):
    import torch
    R = pkg.SeqSet.new([b"X" * 30, b"", b"**BZ", b"-" * 100])
    ix = pkg.SeedIndex.build(R, 3, alphabet="aa11", stream=_stream())
    assert len(ix) == 0
    Q = pkg.SeqSet.new([b"ATGAAATGGTTTCCACATTGT", b"", b"ACG"])
    for frames in ("letters", "all", "codons-both"):
        off = _full((4 + 2,), SENTINEL, torch.int64)
        cnt = _full((2 + 2,), SENTINEL, torch.int64)
        pkg.seed_pairs_device(Q, ix, 0, 3, 30, None, None, None, 0, off.data_ptr(), cnt.data_ptr(), min_seeds=1, stream=_stream(), frames=frames)
        _sync()
        assert off.cpu().tolist() == [0, 0, 0, 0, SENTINEL, SENTINEL] and cnt.cpu().tolist() == [0, 0, SENTINEL, SENTINEL]
        h = pkg.seed_pairs(Q, ix, min_seeds=1, frames=frames)
        assert h.row_off.tolist() == [0, 0, 0, 0] and len(h) == 0 and h.n_passing == 0
    with pytest.raises(pkg.BatchError, match="pmx_seed_pairs_letters"):
        _dna_entry_on_letters_index(pkg, Q, ix)


def _dna_entry_on_letters_index(pkg, Q, ix):
    import ctypes as C
    o = pkg.pmx_seed_opts_t(2, 2, 8, 16, 64, 0, 0, 0)
    if pkg.lib.pmx_seed_pairs_device(Q._handle(), ix._handle(), 0, 3, 30, C.byref(o), None, None, None, 0, None, None, None):
        raise pkg.BatchError(pkg.lib.pmx_last_error().decode())


# ---- seeding ---------------------------------------------------------------------------------------------------------------------------
K_MED, MQ_MED = 4, 53
OPTS_LETTERS = dict(min_seeds=2, band=4, pad=8, max_occ=3)
OPTS_CODONS = dict(min_seeds=2, band=12, pad=8, max_occ=3)


def _opts(mode):
    return OPTS_CODONS if ref.is_codon_mode(mode) else OPTS_LETTERS


FRAMES_ARG = {ref.QUERY_LETTERS: "letters", tr.FRAMES_FORWARD: "forward", tr.FRAMES_REVERSE: "reverse", tr.FRAMES_ALL: "all",
              ref.CODONS_FORWARD: "codons", ref.CODONS_REVERSE: "codons-reverse", ref.CODONS_BOTH: "codons-both"}


def _frames_arg(mode):
    return FRAMES_ARG.get(mode, mode)


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
                          off.data_ptr(), cnt.data_ptr(), stream=_stream(), frames=_frames_arg(mode), **kw)
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
    if 0 <= mode <= tr.FRAMES_ALL:
        assert h.frame.tobytes() == want["byte"][:stored].tobytes() and not h.strand.any() and len(h.strand) == stored
    else:
        assert h.frame is None and h.strand.tobytes() == want["byte"][:stored].tobytes()


def _mutate_nt(rng, nt, rate):
    s = bytearray(nt)
    for x in np.nonzero(rng.random(len(s)) < rate)[0]:
        s[x] = b"ACGT"[(b"ACGT".index(s[x]) + 1 + int(rng.integers(3))) % 4]
    return bytes(s)


@pytest.fixture(scope="module")
def medium():
    """about 150 proteins and 300 reads of 0 .. 160 nt (one above max_qlen) that are back-translated pieces of them, in every frame
    and on both strands; computed once, never changed"""
    rng = np.random.default_rng(8100)
    prots = [ref.random_protein(rng, int(rng.integers(30, 121))) for _ in range(146)]
    at, above = b"MKWFPHCYG", b"GYCHPFWKM"                                                   # motifs at and just above max_occ = 3
    for x in range(3):
        prots[10 + x] = prots[10 + x][:20] + at + prots[10 + x][20:]
    for x in range(4):
        prots[20 + x] = prots[20 + x][:15] + above + prots[20 + x][15:]
    prots += [b"", b"MK", ref.random_protein(rng, 30)[:12] + b"X" + ref.random_protein(rng, 20), b"*" + ref.random_protein(rng, 25)]
    reads = []

    def piece(i, a, n, lead=None, strand=None, rate=0.0):
        nt = ref.back_translate(prots[i][a:a + n], rng)
        lead = int(rng.integers(3)) if lead is None else lead
        nt = _mutate_nt(rng, b"ACGT"[:lead] + nt + b"ACGT"[:int(rng.integers(3))], rate)
        return ref.revcomp(nt) if (int(rng.integers(2)) if strand is None else strand) else nt

    for x in range(250):
        i = int(rng.integers(146))
        n = int(rng.integers(8, min(50, len(prots[i])) + 1))
        a = int(rng.integers(0, len(prots[i]) - n + 1))
        reads.append(piece(i, a, n, rate=0.03 if x % 3 == 0 else 0.0))
    k = K_MED
    for off in (0, 1, 2):                                                                    # W = 3 k + off exactly, and one less
        exact = piece(5, 7, k, lead=off, strand=0)[:3 * k + off]
        reads += [exact, exact[:-1], ref.revcomp(exact)]
    reads += [b"", b"A", b"AC", b"ACG"]
    reads.append(piece(30, 0, 30, strand=0) + piece(31, 0, 30, strand=0)[:110])              # 200 nt: above max_qlen = 53 letters
    assert len(reads[-1]) // 3 > MQ_MED
    s = piece(40, 5, 40, lead=0, strand=0)
    reads += [s[:30] + b"TAA" + s[33:], s[:31] + b"N" + s[32:], s.lower().replace(b"t", b"u"), ref.revcomp(s).lower()]
    reads += [piece(10, 14, 22, strand=0), piece(11, 12, 25, strand=1), piece(20, 9, 22, strand=0), piece(22, 10, 24, strand=1)]   # the motifs
    for i in (50, 51, 52):                                                                   # overhang at both reference ends: clipped windows
        n = len(prots[i])
        reads.append(b"GGCCGGCCGG" + piece(i, 0, 14, lead=0, strand=0))                      # a negative diagonal
        reads.append(piece(i, n - 14, 14, lead=1, strand=0)[:44] + b"GGCCGGCCGGCCGG")
        reads.append(ref.revcomp(b"CCGGCCG" + piece(i, 0, 12, lead=0, strand=0)))
    reads.append(ref.back_translate(prots[60][3:30], rng).replace(b"TGG", b"TGA"))          # for the custom code: TGA = W
    while len(reads) < 300:
        reads.append(bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, size=int(rng.integers(30, 161)))))
    assert max(len(r) for r in reads[:-1]) <= 200 and len(reads) == 300
    idx = ref.index_dict(prots, K_MED, T11)
    occ = {key: len(v) for key, v in idx.items()}
    key_of = lambda m: ref.kmers(m, K_MED, T11)[0][1]
    assert occ[key_of(at)] == 3 and occ[key_of(above)] == 4
    matcher = ref.key_matches(idx, K_MED, T11, 3)
    cache = {}

    def model(mode, code=tr.CODE_STD, queries=None, **kw):
        o = dict(_opts(mode))
        o.update(kw)
        key = (mode, code, queries is None, tuple(sorted(o.items())))
        if key not in cache:
            cache[key] = ref.seed(reads if queries is None else queries, prots, K_MED, T11, mode, o["min_seeds"], o["band"], o["pad"],
                                  o["max_occ"], max_qlen=o.get("max_qlen", MQ_MED), code=code, matcher=matcher)
        return cache[key]
    return prots, reads, model


@pytest.fixture(scope="module")
def medium_dev(pkg, medium):
    prots, reads, _ = medium
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    return Q, R, pkg.SeedIndex.build(R, K_MED, alphabet="aa11", stream=_stream())


def test_the_inputs_are_not_empty(medium):
    """on the CPU: the model's own result has candidates for at least half of the rows, in every frame and on both strands, windows
    clipped at both reference ends, a negative nucleotide diagonal, and the motif above max_occ gives no seed"""
    prots, reads, model = medium
    want = model(tr.FRAMES_ALL)
    per_row = np.diff(want["row_off"])
    assert (per_row > 0).sum() >= len(reads) // 2
    assert sorted(set(want["byte"].tolist())) == [0, 1, 2, 3, 4, 5]
    co = model(ref.CODONS_BOTH)
    assert sorted(set(co["byte"].tolist())) == [0, 1] and (np.diff(co["row_off"]) > 0).sum() >= len(reads) // 2
    assert (co["seeds"]["diag_min"] < 0).any() and (want["seeds"]["diag_min"] < 0).any()
    rlens = np.array([len(p) for p in prots])
    for w in (want, co):
        assert (w["pairs"]["r_beg"] == 0).any() and (w["pairs"]["r_beg"] + w["pairs"]["r_len"] == rlens[w["pairs"]["r"]]).any()
        assert (w["pairs"]["r_len"] > 0).all()
    long_row = next(q for q, r in enumerate(reads) if len(r) // 3 > MQ_MED)
    assert per_row[long_row] == 0 and np.diff(model(tr.FRAMES_ALL, max_qlen=None)["row_off"])[long_row] > 0
    assert len(model(tr.FRAMES_ALL, code=CUSTOM_CODE)["pairs"]) != len(want["pairs"]) or \
        model(tr.FRAMES_ALL, code=CUSTOM_CODE)["seeds"].tobytes() != want["seeds"].tobytes()


@pytest.mark.parametrize("mode", [m for m in ref.MODES if m != ref.QUERY_LETTERS])
def test_every_query_mode_equals_the_model(pkg, medium, medium_dev, mode):
    prots, reads, model = medium
    Q, R, ix = medium_dev
    want = model(mode)
    total = int(want["row_off"][-1])
    assert total > 0
    _same(_seed(pkg, Q, ix, len(reads), MQ_MED, total + 2, mode, **_opts(mode)), want, total + 2, len(reads))
    _same_host(pkg.seed_pairs(Q, ix, frames=_frames_arg(mode), **_opts(mode)), model(mode, max_qlen=66), mode)   # max_qlen from the rows: 200 / 3


def test_custom_genetic_code_and_letters_mode(pkg, medium, medium_dev):
    prots, reads, model = medium
    Q, R, ix = medium_dev
    for mode in (tr.FRAMES_ALL, ref.CODONS_BOTH):
        want = model(mode, code=CUSTOM_CODE)
        total = int(want["row_off"][-1])
        _same(_seed(pkg, Q, ix, len(reads), MQ_MED, total + 2, mode, code=CUSTOM_CODE, **_opts(mode)), want, total + 2, len(reads))
    # letters mode: pieces of the proteins as queries, W bounded by max_qlen itself
    rng = np.random.default_rng(8150)
    qs = [prots[i][a:a + 40] for i, a in zip(rng.integers(0, 146, size=60).tolist(), rng.integers(0, 20, size=60).tolist())]
    qs += [b"", b"MKW", b"MKWF", prots[10][10:40].lower(), prots[12], prots[21][5:45], b"X" * 30, prots[3] + prots[4]]
    P = pkg.SeqSet.new(qs)
    want = model(ref.QUERY_LETTERS, queries=qs, max_qlen=120)
    total = int(want["row_off"][-1])
    assert total >= 60 and len(qs[-1]) > 120 and want["row_off"][-1] == want["row_off"][-2]
    _same(_seed(pkg, P, ix, len(qs), 120, total + 2, ref.QUERY_LETTERS, **OPTS_LETTERS), want, total + 2, len(qs))


@pytest.mark.parametrize("mode", [tr.FRAMES_ALL, ref.CODONS_BOTH])
@pytest.mark.parametrize("slice_rows", [1, 3, 700])
@pytest.mark.parametrize("budget", [1 << 20, 300000])
def test_slices_and_a_tiny_match_buffer_never_change_a_byte(pkg, medium, medium_dev, mode, slice_rows, budget):
    """budget: the match buffer (test hook) -- one row's worst case is 53 x 6 x 3 x 24 = 22 896 bytes"""
    prots, reads, model = medium
    Q, R, ix = medium_dev
    want = model(mode)
    total = int(want["row_off"][-1])
    pkg.lib.pmx_seed_match_budget(budget)
    try:
        _same(_seed(pkg, Q, ix, len(reads), MQ_MED, total, mode, slice_rows=slice_rows, **_opts(mode)), want, total, len(reads))
    finally:
        pkg.lib.pmx_seed_match_budget(0)


def test_capacity_subranges_and_the_host_entry(pkg, medium, medium_dev):
    prots, reads, model = medium
    Q, R, ix = medium_dev
    nq = len(reads)
    for mode in (tr.FRAMES_ALL, ref.CODONS_BOTH):
        want = model(mode)
        total = int(want["row_off"][-1])
        for cap in (0, 1, total // 2, total + 9):
            _same(_seed(pkg, Q, ix, nq, MQ_MED, cap, mode, with_seeds=cap != 1, **_opts(mode)), want, cap, nq)
        for first, n in ((0, 1), (1, 200), (250, 50), (299, 1), (300, 0), (70, 0)):
            a, b = int(want["row_off"][first]), int(want["row_off"][first + n])
            sub = {"row_off": want["row_off"][first:first + n + 1] - a, "pairs": want["pairs"][a:b], "byte": want["byte"][a:b], "seeds": want["seeds"][a:b]}
            _same(_seed(pkg, Q, ix, n, MQ_MED, b - a + 1, mode, q_first=first, slice_rows=33, **_opts(mode)), sub, b - a + 1, n)
        # far more than two candidates per row: every match a candidate of its own -- the host entry's second, exact-size run
        many = model(mode, min_seeds=1, band=0, pad=0, max_qlen=66)
        n_many = int(many["row_off"][-1])
        assert n_many > 2 * (2 * nq + 16)
        o = dict(min_seeds=1, band=0, pad=0, max_occ=3, frames=_frames_arg(mode))
        _same_host(pkg.seed_pairs(Q, ix, **o), many, mode)                                   # (max_qlen from the rows: 200 / 3 = 66)
        _same_host(pkg.seed_pairs(Q, ix, max_hits=n_many - 3, slice_rows=64, **o), many, mode, stored=n_many - 3)
        _same_host(pkg.seed_pairs(Q, ix, max_hits=7, **o), many, mode, stored=7)
    with pytest.raises(pkg.BatchError, match="worst case"):                                  # refused before any GPU work
        pkg.seed_pairs(Q, ix, max_occ=65535, min_seeds=3, frames="all")


# ---- into the aligners -----------------------------------------------------------------------------------------------------------------
K_AL, OPEN, EXT, SHIFT = 6, 11, 1, 15


@pytest.fixture(scope="module")
def planted():
    """200 reads of 150 nt, each the back-translation of 50 letters of its own protein (200 of 300 letters) with 5 % nucleotide
    substitutions; `cut`: the same reads with the nucleotide at mid-read deleted.  In this recipe about one read in a hundred
    loses every 6-mer of one of its halves to the substitutions, and its codon-mode candidate then has as many seeds as its one
    frame-mode candidate, not more (generator seeds 8200 .. 8229: 0 .. 7 such reads of 200); the seed below is one at which every
    read keeps seeds in both halves, which the codon road's test asserts on the model before it looks at the device."""
    rng = np.random.default_rng(8209)
    prots = [ref.random_protein(rng, 300) for _ in range(200)]
    at = [int(a) for a in rng.integers(0, 251, size=200)]
    reads = [_mutate_nt(rng, ref.back_translate(prots[i][at[i]:at[i] + 50], rng), 0.05) for i in range(200)]
    cut = [r[:75] + r[76:] for r in reads]
    idx = ref.index_dict(prots, K_AL, T11)
    matcher = ref.key_matches(idx, K_AL, T11, 64)
    o = dict(min_seeds=2, pad=8, max_occ=64, matcher=matcher)
    frames_all = ref.seed(reads, prots, K_AL, T11, tr.FRAMES_ALL, band=4, **o)
    cut_frames = ref.seed(cut, prots, K_AL, T11, tr.FRAMES_FORWARD, band=4, **o)
    cut_codons = ref.seed(cut, prots, K_AL, T11, ref.CODONS_FORWARD, band=12, **o)
    return prots, at, reads, cut, frames_all, cut_frames, cut_codons


def _rows(w, q):
    return range(int(w["row_off"][q]), int(w["row_off"][q + 1]))


def _b62(pkg, orc):
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))


def test_frame_road_into_align_pairs(pkg, orc, planted):
    prots, at, reads, cut, want, _, _ = planted
    found = sum(any(want["pairs"][x]["r"] == q and want["byte"][x] == 0 and want["seeds"][x]["diag_min"] <= at[q] <= want["seeds"][x]["diag_max"]
                    for x in _rows(want, q)) for q in range(len(reads)))
    print("reads whose planted protein in frame 0 is among the model's candidates: %d of %d" % (found, len(reads)))
    assert found >= 0.9 * len(reads)                                                         # the recall condition, on the model
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    ix = pkg.SeedIndex.build(R, K_AL, alphabet="aa11", stream=_stream())
    hits = pkg.seed_pairs(Q, ix, min_seeds=2, band=4, pad=8, max_occ=64, frames="all")
    _same_host(hits, want, tr.FRAMES_ALL)
    pm, om = _b62(pkg, orc)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(OPEN).gap_extend(EXT).build()
    rec, frames = al.align_pairs(Q, R, hits.pairs, frame=hits.frame)
    assert frames.tobytes() == hits.frame.tobytes() and (rec["flags"] == 0).all()
    strings = tr.resolve(reads, prots, hits.pairs, hits.frame)                               # the host-translated frame, the window
    assert all(s is not None for s in strings)
    qb, qo = orc.pack([s[0] for s in strings])
    rb, ro = orc.pack([s[1] for s in strings])
    full = orc.align_batch(orc.SW, qb, qo, rb, ro, OPEN, EXT, om)
    assert (rec["score"] == full[:, 0]).all() and (rec["end_query"] == full[:, 1]).all() and (rec["end_ref"] == full[:, 2]).all()
    assert rec["score"].max() > 100


def test_codon_road_into_the_frameshift_entries(pkg, planted):
    prots, at, reads, cut, _, fr, co = planted
    Q, R = pkg.SeqSet.new(cut), pkg.SeqSet.new(prots)
    ix = pkg.SeedIndex.build(R, K_AL, alphabet="aa11", stream=_stream())
    hits = pkg.seed_pairs(Q, ix, min_seeds=2, band=12, pad=8, max_occ=64, frames="codons")
    _same_host(hits, co, ref.CODONS_FORWARD)
    _same_host(pkg.seed_pairs(Q, ix, min_seeds=2, band=4, pad=8, max_occ=64, frames="forward"), fr, tr.FRAMES_FORWARD)
    al = pkg.Aligner.new().local().matrix(pkg.Matrix.from_name("blosum62")).gap_open(OPEN).gap_extend(EXT).build()
    rec, strand = al.align_pairs(Q, R, hits.pairs, frameshift=SHIFT, strand=hits.strand)
    rec2, cigars, begins, strand2 = al.align_pairs_frameshift_cigar(Q, R, hits.pairs, SHIFT, strand=hits.strand)
    assert rec.tobytes() == rec2.tobytes() and strand.tobytes() == strand2.tobytes() == hits.strand.tobytes() and (rec["flags"] == 0).all()
    over = 0
    for q in range(len(cut)):
        # the planted locus: D = 3 at before the deleted nucleotide, 3 at + 1 behind it
        mine = [x for x in _rows(co, q) if co["pairs"][x]["r"] == q and co["seeds"][x]["diag_min"] <= 3 * at[q] + 1 and
                co["seeds"][x]["diag_max"] >= 3 * at[q]]
        if not mine:
            continue
        assert len(mine) == 1
        over += 1
        there = [int(fr["seeds"][x]["n_seeds"]) for x in _rows(fr, q) if fr["pairs"][x]["r"] == q and
                 fr["seeds"][x]["diag_min"] <= at[q] + 1 and fr["seeds"][x]["diag_max"] >= at[q]]
        print("read %d: codon candidate %d seeds, frame candidates %s, cigar %s" % (q, int(co["seeds"][mine[0]]["n_seeds"]), there, cigars[mine[0]]))
        assert all(int(co["seeds"][mine[0]]["n_seeds"]) > n for n in there), q
        assert "/" in cigars[mine[0]], (q, cigars[mine[0]])
    assert over >= 0.9 * len(cut)


def test_letters_road_proteins_against_themselves(pkg, orc, planted):
    """band 0: a cluster is one diagonal, so the protein's own diagonal stands alone (with a band, a chance 6-mer match a letter or
    two beside it joins the cluster of a few proteins in a hundred and widens d_min .. d_max)"""
    prots = planted[0]
    P = pkg.SeqSet.new(prots)
    ix = pkg.SeedIndex.build(P, K_AL, alphabet="aa11", stream=_stream())
    hits = pkg.seed_pairs(P, ix, min_seeds=2, band=0, pad=8, max_occ=64, frames="letters")
    _same_host(hits, ref.seed(prots, prots, K_AL, T11, ref.QUERY_LETTERS, 2, 0, 8, 64), ref.QUERY_LETTERS)
    mine = []
    for i in range(len(prots)):
        p, s, d = hits.row(i)
        ok = [x for x in range(len(p)) if p[x]["r"] == i and d[x]["diag_min"] == 0 and d[x]["diag_max"] == 0]
        assert len(ok) == 1 and d[ok[0]]["n_seeds"] == 300 - K_AL + 1 and tuple(p[ok[0]]) == (i, i, 0, -1, 0, 300)
        mine.append(int(hits.row_off[i]) + ok[0])
    pm, om = _b62(pkg, orc)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(OPEN).gap_extend(EXT).build()
    rec = al.align_pairs(P, P, hits.pairs)
    qb, qo = orc.pack(prots)
    full = orc.align_batch(orc.SW, qb, qo, qb, qo, OPEN, EXT, om)
    assert (rec["score"][mine] == full[:, 0]).all() and (rec["end_query"][mine] == 299).all() and (rec["flags"] == 0).all()
