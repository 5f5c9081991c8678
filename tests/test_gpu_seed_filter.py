"""The ungapped diagonal filter (`-m gpu`): pmx_seed_ungapped[_device] and pmx_seed_filter[_device] against the model
tests/seed_filter_ref.py.  Every comparison is exact; every output buffer starts as a sentinel and is checked behind `capacity`.

The kernel's shape (pmx_seed_ungapped_shape): G = 16 lanes per candidate, s = 4 cells per lane step.  The G lanes divide
themselves by the span -- 16, 8, 4, 2, 1 lanes per diagonal for spans of 1, 2, <= 4, <= 8, more -- and a diagonal's cells are cut into
pieces of whole steps, ceil(cells / (lanes x s)) steps each.  A candidate is always ONE pass, whatever its length: what changes with the
length is the piece, which grows by a step at every multiple of G x s = 64 cells.  So the lengths here are 1 .. 9 (dword heads and
tails), G s - 1, G s, G s + 1 = 63, 64, 65, the next two piece boundaries 127 .. 129 and 255 .. 257, and the longest query the call
allows with its neighbours (398, 399, 400 = max_qlen); the spans are 1, 2, G - 1, G, G + 1, every span at which the lanes per diagonal
change (3, 4, 5, 8, 9) and one of 300."""
import numpy as np
import pytest

import seed_filter_ref as ref
import translate_ref as tr
from pairs_ex_ref import revcomp
from seed_letters_ref import back_translate, random_protein
from util import golden

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
G, S = 16, 4
LENGTHS = list(range(1, 10)) + [G * S - 1, G * S, G * S + 1, 127, 128, 129, 255, 256, 257, 398, 399, 400]
SPANS = [1, 2, 3, 4, 5, 8, 9, G - 1, G, G + 1, 300]
MAX_QLEN = 400
CUSTOM_CODE = bytearray(tr.CODE_STD)
CUSTOM_CODE[16 * 0 + 4 * 3 + 2] = ord("W")                                                  # TGA reads as W, as in NCBI table 4
CUSTOM_CODE[16 * 2 + 4 * 3 + 0] = ord("*")                                                  # AGT is a stop here
CUSTOM_CODE = bytes(CUSTOM_CODE)                                                            # (the code of test_gpu_seed_letters.py)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device=_dev())


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev())


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize()


def _mutate(rng, s, rate, letters=b"ACGT"):
    s = bytearray(s)
    for x in np.nonzero(rng.random(len(s)) < rate)[0]:
        s[x] = letters[(letters.index(s[x]) + 1 + int(rng.integers(len(letters) - 1))) % len(letters)] if s[x] in letters else letters[0]
    return bytes(s)


def _dna(rng, n):
    return bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, size=n))


def _seeds(rows):
    a = np.zeros(len(rows), dtype=ref.SEED_HIT_DTYPE)
    for k, (lo, hi) in enumerate(rows):
        a[k] = (2, lo, hi, 0)
    return a


# ---- hand-built lists --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dna_list():
    """About 420 candidates over both strands: a mutated copy of every query (forward in reference 0, reverse-complemented in reference
    1) under every span, with windows clipped at both reference ends and pad 0, diagonals that leave the window on either side or
    have no cell at all, all-negative candidates, equal maxima on two diagonals and twice on one, lower-case and invalid letters, and
    bad candidates between good ones.  Computed once, never changed."""
    rng = np.random.default_rng(9200)
    qs = [_dna(rng, n) for n in LENGTHS]
    period = b"ACGTTGCA" * 12                                                                # 96: equal maxima 8 diagonals apart
    s1 = _dna(rng, 30)
    qs += [period, s1 + b"T" * 20 + s1, b"A" * 70, _dna(rng, 90).lower(), _mutate(rng, _dna(rng, 120), 0.1, b"ACGTN*"), b"AC", b"ACTTAC"]
    I_PERIOD, I_TWICE, I_NEG, I_LOWER, I_INVALID, I_AC, I_ACTTAC = range(len(LENGTHS), len(LENGTHS) + 7)
    pos, parts, at = {}, [], 0
    for i, q in enumerate(qs):
        lead = _dna(rng, int(rng.integers(0, 7)))
        body = _mutate(rng, q.upper(), 0.08) if i < len(LENGTHS) or i in (I_LOWER, I_INVALID) else q
        if i == I_TWICE:
            body = s1 + b"G" * 20 + s1
        if i == I_NEG:
            body = b"C" * 70
        if i == I_AC:
            body = b"ACTTAC"
        if i == I_ACTTAC:
            body = b"ACGGAC"
        pos[i] = at + len(lead)
        parts += [lead, body]
        at += len(lead) + len(body)
    fwd = b"".join(parts)
    rev_pos, parts, at = {}, [], 0
    for i, q in enumerate(qs[:len(LENGTHS)]):
        lead = _dna(rng, int(rng.integers(0, 7)))
        rev_pos[i] = at + len(lead)
        parts += [lead, _mutate(rng, revcomp(q), 0.08)]
        at += len(lead) + len(parts[-1])
    refs = [fwd, b"".join(parts), period * 3, _dna(rng, 5)]
    rows, byte, sd = [], [], []

    def add(q, r, strand, r_beg, r_len, lo, hi):
        rows.append((q, r, 0, -1, r_beg, r_len))
        byte.append(strand)
        sd.append((lo, hi))

    def window(r, L, lo, hi, pad):
        """the seeding entries' window: clipped at both reference ends"""
        b, e = max(0, lo - pad), min(len(refs[r]), hi + L + pad)
        return b, max(1, e - b)

    for i in range(len(LENGTHS)):
        L = len(qs[i])
        for strand, r, p in ((0, 0, pos[i]), (1, 1, rev_pos[i])):
            for span in SPANS:
                lo = p - int(rng.integers(0, span))                                          # the planted diagonal lies inside lo .. lo + span - 1
                add(i, r, strand, *window(r, L, lo, lo + span - 1, 0 if span % 2 else 5), lo, lo + span - 1)
        add(i, 0, 0, pos[i] + L // 2, max(1, L // 3), pos[i] - 2, pos[i] + 2)                # a window that cuts the diagonal on both sides
        add(i, 0, 0, 0, len(refs[0]), pos[i], pos[i])                                        # the whole reference as the window
    # diagonals outside the window: on the left, on the right, partly, and with no cell at all
    add(12, 0, 0, 100, 50, 100 - 300, 100 - 250)
    add(12, 0, 0, 100, 50, 100 - len(qs[12]) + 1, 100 - len(qs[12]) + 1)                     # one cell: the query's last letter on the window's first
    add(12, 0, 0, 100, 50, 149, 149)                                                         # one cell: the query's first letter on the window's last
    add(12, 0, 0, 100, 50, 150, 190)                                                         # behind the window: no cell
    add(12, 0, 0, 100, 50, -500, -400)                                                       # in front of it: no cell
    add(12, 0, 0, 100, 50, 140, 160)                                                         # 140 .. 149 have cells, 150 .. 160 none
    add(12, 0, 0, 100, 50, -(1 << 31), (1 << 31) - 1)                                        # every diagonal there is
    add(I_NEG, 0, 0, *window(0, 70, pos[I_NEG], pos[I_NEG] + 3, 0), pos[I_NEG], pos[I_NEG] + 3)      # all negative
    add(I_PERIOD, 2, 0, 0, len(refs[2]), 0, 40)                                              # equal maxima on d = 0, 8, 16, ..
    add(I_PERIOD, 2, 0, 0, len(refs[2]), 3, 40)                                              # ... on 8, 16, ..
    add(I_PERIOD, 2, 0, 40, 150, -20, 100)
    add(I_TWICE, 0, 0, *window(0, 80, pos[I_TWICE], pos[I_TWICE], 0), pos[I_TWICE], pos[I_TWICE])    # 60 twice on one diagonal: i = 29 and 79
    add(I_AC, 0, 0, pos[I_AC], 6, pos[I_AC], pos[I_AC] + 4)
    add(I_ACTTAC, 0, 0, pos[I_ACTTAC], 6, pos[I_ACTTAC], pos[I_ACTTAC])
    for i in (I_LOWER, I_INVALID):
        add(i, 0, 0, *window(0, len(qs[i]), pos[i] - 1, pos[i] + 1, 4), pos[i] - 1, pos[i] + 1)
        add(i, 0, 1, *window(0, len(qs[i]), pos[i] - 1, pos[i] + 1, 4), pos[i] - 1, pos[i] + 1)
    # bad candidates, each between good neighbours
    good = (14, 0, 0, pos[14], len(qs[14]), pos[14], pos[14])
    for bad in ((len(qs), 0, 0, 0, 10, 0, 0), (-1, 0, 0, 0, 10, 0, 0), (14, 4, 0, 0, 10, 0, 0), (14, 0, 0, 0, len(refs[0]) + 1, 0, 0),
                (14, 0, 0, -1, 10, 0, 0), (14, 0, 0, 5, 0, 0, 0), (14, 0, 2, pos[14], 65, pos[14], pos[14]), (14, 0, 255, pos[14], 65, pos[14], pos[14]),
                (14, 0, 0, pos[14], 65, pos[14] + 1, pos[14])):
        add(*good)
        add(*bad)
    add(*good)
    return qs, refs, ref.pairs_ref.pairs_array(rows), np.array(byte, dtype=np.uint8), _seeds(sd)


@pytest.fixture(scope="module")
def dna_matrix(pkg):
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    return m, m.to_numpy(), m.mapper()


@pytest.fixture(scope="module")
def dna_want(dna_list, dna_matrix):
    qs, refs, pairs, byte, seeds = dna_list
    _, scores, mapper = dna_matrix
    return ref.ungapped(qs, refs, pairs, byte, seeds, scores, mapper, max_qlen=MAX_QLEN, max_rlen=max(len(r) for r in refs))


def _ungapped_device(pkg, Q, R, pairs, byte, seeds, mq, mr, matrix, kind="strand", code=None, chunk_pairs=0):
    import torch
    n = len(pairs)
    out = _full((n + 3, 4), SENTINEL, torch.int32)
    dp, ds = _up(pairs), _up(seeds)
    db = _up(byte) if byte is not None else None
    pkg.seed_ungapped_device(Q, R, n, dp.data_ptr(), db.data_ptr() if db is not None else None, ds.data_ptr(), mq, mr, matrix, out.data_ptr(),
                             kind=kind, code=code, stream=_stream(), chunk_pairs=chunk_pairs)
    _sync()
    got = out.cpu().numpy()
    assert (got[n:] == SENTINEL).all()
    return got[:n].reshape(-1).view(ref.UNGAPPED_DTYPE)


def _explain(got, want, k):
    return "candidate %d: got %s, want %s" % (k, tuple(got[k]), tuple(want[k]))


def _assert_same(got, want):
    diff = np.nonzero(got.view(np.int32).reshape(-1, 4) != want.view(np.int32).reshape(-1, 4))[0]
    assert len(diff) == 0, _explain(got, want, int(diff[0]))


def test_the_dna_list_covers_what_it_claims(dna_list, dna_want):
    """on the CPU, on the model's own result: every kind of record is there"""
    qs, refs, pairs, byte, seeds = dna_list
    w = dna_want
    assert (w["score"] == -1).sum() == 9 and ((w["score"] == 0) & (w["end_query"] == -1)).sum() >= 4
    assert (w["score"] > 100).sum() > 100 and set(byte.tolist()) >= {0, 1, 2}
    assert sorted(set((seeds["diag_max"].astype(np.int64) - seeds["diag_min"] + 1).tolist()) & set(SPANS)) == sorted(SPANS)
    assert (pairs["r_beg"] == 0).any() and (pairs["r_beg"] + pairs["r_len"] == len(refs[0])).any()
    twice = [k for k in range(len(pairs)) if pairs[k]["q"] == len(LENGTHS) + 1]
    assert len(twice) == 1 and w[twice[0]]["score"] == 60 and w[twice[0]]["end_query"] == 29
    bad = np.nonzero(w["score"] == -1)[0]
    assert all(tuple(w[k - 1]) == tuple(w[k + 1]) and w[k - 1]["score"] > 50 for k in bad)


@pytest.mark.parametrize("chunk_pairs", [0, 1, 7])
def test_dna_scores_equal_the_model_under_any_chunking(pkg, dna_list, dna_matrix, dna_want, chunk_pairs):
    qs, refs, pairs, byte, seeds = dna_list
    Q, R = pkg.SeqSet.new(qs), pkg.SeqSet.new(refs)
    mr = max(len(r) for r in refs)
    got = _ungapped_device(pkg, Q, R, pairs, byte, seeds, MAX_QLEN, mr, dna_matrix[0], chunk_pairs=chunk_pairs)
    _assert_same(got, dna_want)
    if chunk_pairs == 0:                                                                     # determinism: a second run, the same bytes
        again = _ungapped_device(pkg, Q, R, pairs, byte, seeds, MAX_QLEN, mr, dna_matrix[0])
        assert again.tobytes() == got.tobytes()
        assert pkg.lib.pmx_last_kernel().decode() == "pmx_ungapped_kernel"
        _assert_same(pkg.seed_ungapped(Q, R, pairs, byte, seeds, dna_matrix[0]), dna_want)   # the host entry finds the maxima itself
        assert pkg.ungapped_shape() == (G, S)


def test_forward_list_without_bytes_and_a_short_max_qlen(pkg, dna_list, dna_matrix):
    """d_byte NULL is all forward; a query longer than max_qlen is a bad candidate under the gather's rule"""
    qs, refs, pairs, byte, seeds = dna_list
    _, scores, mapper = dna_matrix
    keep = np.nonzero(byte == 0)[0][::3]
    Q, R = pkg.SeqSet.new(qs), pkg.SeqSet.new(refs)
    mr = max(len(r) for r in refs)
    want = ref.ungapped(qs, refs, pairs[keep], None, seeds[keep], scores, mapper, max_qlen=128, max_rlen=mr)
    assert (want["score"] == -1).sum() > 5 and (want["score"] > 0).sum() > 50
    _assert_same(_ungapped_device(pkg, Q, R, pairs[keep], None, seeds[keep], 128, mr, dna_matrix[0]), want)


@pytest.fixture(scope="module")
def protein_list():
    """proteins under BLOSUM62: mutated pieces of the references as queries, lower case, X, * and bytes outside the alphabet"""
    rng = np.random.default_rng(9201)
    prots = [random_protein(rng, int(rng.integers(80, 400))) for _ in range(30)]
    qs, rows, sd = [], [], []
    for n in LENGTHS[:18] + [300]:
        i = int(rng.integers(30))
        n = min(n, len(prots[i]))
        a = int(rng.integers(0, len(prots[i]) - n + 1))
        q = bytearray(_mutate(rng, prots[i][a:a + n], 0.15, b"ACDEFGHIKLMNPQRSTVWY"))
        if n > 20:
            q[3], q[7], q[11] = ord("X"), ord("*"), ord("#")
            q[12:16] = bytes(q[12:16]).lower()
        qs.append(bytes(q))
        for span in (1, 2, 5, 9, G + 1):
            lo = a - int(rng.integers(0, span))
            b, e = max(0, lo - 8), min(len(prots[i]), lo + span - 1 + n + 8)
            rows.append((len(qs) - 1, i, 0, -1, b, e - b))
            sd.append((lo, lo + span - 1))
    return qs, prots, ref.pairs_ref.pairs_array(rows), _seeds(sd)


def test_protein_scores_equal_the_model(pkg, protein_list):
    qs, prots, pairs, seeds = protein_list
    m = pkg.Matrix.from_name("blosum62")
    assert m.size <= 32                                                                      # the table staged as bytes
    mr = max(len(p) for p in prots)
    want = ref.ungapped(qs, prots, pairs, None, seeds, m.to_numpy(), m.mapper())
    assert want["score"].max() > 300 and (want["score"] >= 0).all() and (want["score"] > 0).sum() > 80
    Q, R = pkg.SeqSet.new(qs), pkg.SeqSet.new(prots)
    for byte in (None, np.zeros(len(pairs), dtype=np.uint8)):
        _assert_same(_ungapped_device(pkg, Q, R, pairs, byte, seeds, 300, mr, m, chunk_pairs=13), want)
    # a table that is not staged as bytes (scores beyond a byte): the same model, the general form of the kernel
    wide = pkg.Matrix.create(b"ACDEFGHIKLMNPQRSTVWY", 300, -200)
    want = ref.ungapped(qs, prots, pairs, None, seeds, wide.to_numpy(), wide.mapper())
    _assert_same(_ungapped_device(pkg, Q, R, pairs, None, seeds, 300, mr, wide), want)


# ---- lists of the seeding entries ----------------------------------------------------------------------------------------------------------
K_AA = 4


@pytest.fixture(scope="module")
def translated_world(pkg):
    """60 proteins of 300 letters and 90 reads of 150 nt (some 149, 151): back-translated pieces with 5 % substitutions, on either strand
    and in any frame"""
    rng = np.random.default_rng(9202)
    prots = [random_protein(rng, 300) for _ in range(60)]
    reads = []
    for x in range(90):
        i, a = int(rng.integers(60)), int(rng.integers(0, 251))
        nt = _mutate(rng, b"ACGT"[:x % 3] + back_translate(prots[i][a:a + 50], rng), 0.05)[:149 + x % 3]
        reads.append(revcomp(nt) if x % 2 else nt)
    reads += [b"", b"AC", b"ACGTAC"]
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    ix = pkg.SeedIndex.build(R, K_AA, alphabet="aa11", stream=_stream())
    return prots, reads, Q, R, ix


def _model_filter(qseqs, rseqs, hits, matrix, kind, **kw):
    byte = hits.frame if kind == "frame" else hits.strand
    return ref.filter_hits(qseqs, rseqs, hits.row_off, hits.pairs, byte, hits.seeds, matrix.to_numpy(), matrix.mapper(), kind=kind, **kw)


def _same_hits(f, want, kind, n_rows):
    assert f.n_rows == n_rows and f.n_hits == len(f) == want["counts"][0] == f.n_passing
    assert f.row_off.tobytes() == want["row_off"].tobytes()
    assert f.pairs.tobytes() == want["pairs"].tobytes() and f.seeds.tobytes() == want["seeds"].tobytes()
    assert f.ungapped.tobytes() == want["ungapped"].tobytes() and f.source.tobytes() == want["source"].tobytes()
    if kind == "frame":
        assert f.frame.tobytes() == want["byte"].tobytes() and not f.strand.any()
    else:
        assert f.frame is None and f.strand.tobytes() == want["byte"].tobytes()


@pytest.mark.parametrize("frames,code", [("all", None), (4, CUSTOM_CODE), ("all", CUSTOM_CODE)])
def test_frame_lists_scores_and_filter(pkg, translated_world, frames, code):
    prots, reads, Q, R, ix = translated_world
    m = pkg.Matrix.from_name("blosum62")
    hits = pkg.seed_pairs(Q, ix, min_seeds=2, band=4, pad=8, max_occ=64, frames=frames, code=code)
    assert hits.kind == "frame" and len(hits) > 150 and hits.n_passing == len(hits)
    if frames == "all":
        assert sorted(set(hits.frame.tolist())) == [0, 1, 2, 3, 4, 5]
    kw = {"code": code} if code is not None else {}
    want = _model_filter(reads, prots, hits, m, "frame", **kw)
    got = pkg.seed_ungapped(Q, R, hits.pairs, hits.frame, hits.seeds, m, kind="frame", code=code)
    _assert_same(got, want["all_ungapped"])
    assert (got["score"] >= 0).all() and got["score"].max() > 150
    _same_hits(pkg.seed_filter(Q, R, hits, m, code=code), want, "frame", len(reads))
    for min_score, top_n in ((40, 0), (0, 1), (30, 2)):
        w = _model_filter(reads, prots, hits, m, "frame", min_score=min_score, top_n=top_n, **kw)
        f = pkg.seed_filter(Q, R, hits, m, min_score=min_score, top_n=top_n, code=code, chunk_pairs=37)
        _same_hits(f, w, "frame", len(reads))
        assert 0 < len(f) < len(hits)


@pytest.fixture(scope="module")
def dna_world(pkg):
    """40 references of 1 500 nt and 120 reads of 100 .. 150 nt, on both strands, 4 % substitutions; a repeat shared by all references
    gives every read several candidates, a few reads are random"""
    rng = np.random.default_rng(9203)
    repeat = _dna(rng, 60)
    refs = []
    for _ in range(40):
        s = _dna(rng, 1500)
        a = int(rng.integers(100, 1300))
        refs.append(s[:a] + _mutate(rng, repeat, 0.03) + s[a + 60:])
    reads = []
    for x in range(110):
        i, n = int(rng.integers(40)), int(rng.integers(100, 151))
        a = int(rng.integers(0, 1500 - n + 1))
        piece = refs[i][a:a + n]
        if x % 4 == 0:
            piece = piece[:40] + repeat + piece[100:]
        piece = _mutate(rng, piece, 0.04)
        reads.append(revcomp(piece) if x % 2 else piece)
    reads += [_dna(rng, 120) for _ in range(8)] + [b"", b"ACGT"]
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new(refs)
    ix = pkg.SeedIndex.build(R, 11, stream=_stream())
    hits = pkg.seed_pairs(Q, ix, min_seeds=2, band=8, pad=16, max_occ=64)
    return refs, reads, Q, R, hits


def test_dna_road_end_to_end(pkg, dna_world, dna_matrix):
    refs, reads, Q, R, hits = dna_world
    m = dna_matrix[0]
    assert hits.kind == "strand" and len(hits) > 200 and set(hits.strand.tolist()) == {0, 1}
    per_row = np.diff(hits.row_off)
    assert (per_row == 0).sum() >= 2 and (per_row >= 3).sum() > 10                           # empty rows, rows with several candidates
    for min_score, top_n in ((0, 0), (0, 1), (0, 2), (60, 0), (100, 3), (10 ** 6, 0), (10 ** 6, 2)):
        want = _model_filter(reads, refs, hits, m, "strand", min_score=min_score, top_n=top_n)
        f = pkg.seed_filter(Q, R, hits, m, min_score=min_score, top_n=top_n)
        _same_hits(f, want, "strand", len(reads))
        assert (np.diff(f.source) > 0).all()
        if min_score == 10 ** 6:                                                             # above every score: nothing is kept
            assert len(f) == 0 and not f.row_off.any()
    # top_n = 1 with ties: a read made of one repeated unit has equal scores at several loci, and the earlier position stays
    f1 = pkg.seed_filter(Q, R, hits, m, top_n=1)
    assert len(f1) == (per_row > 0).sum()
    # the filtered list goes into align_pairs as the unfiltered one does, and gives the records of the same pairs there
    al = pkg.Aligner.new().local().matrix(m).gap_open(5).gap_extend(2).build()
    rec_all = al.align_pairs(Q, R, hits.pairs, strand=hits.strand)
    f = pkg.seed_filter(Q, R, hits, m, min_score=40, top_n=2)
    rec = al.align_pairs(Q, R, f.pairs, strand=f.strand)
    assert 0 < len(f) < len(hits) and rec.tobytes() == rec_all[f.source].tobytes() and (rec["flags"] == 0).all()
    assert (rec["score"] >= f.ungapped["score"]).all()                                       # a gapped local score is at least the ungapped one


def test_top_n_ties_keep_the_earlier_position(pkg, dna_matrix):
    """four equal candidates and one better in a row, hand-built: top_n 1, 2 and 3"""
    m = dna_matrix[0]
    unit = b"ACGTTGCAGGATCCATTGAC"
    refs = [unit + b"TTTT" + unit + b"TTTT" + unit[:-1] + b"A" + b"TTTT" + unit, b"GG" + unit]
    qs = [unit, unit[:10]]
    Q, R = pkg.SeqSet.new(qs), pkg.SeqSet.new(refs)
    rows = [(0, 0, 0, -1, 0, 92), (0, 0, 0, -1, 20, 30), (0, 0, 0, -1, 48, 20), (0, 1, 0, -1, 0, 22), (1, 0, 0, -1, 0, 92), (1, 1, 0, -1, 0, 22)]
    seeds = _seeds([(0, 0), (24, 24), (48, 48), (2, 2), (0, 80), (2, 2)])
    hits = pkg.SeedHits.__new__(pkg.SeedHits)
    hits.kind, hits.n_rows, hits.n_hits, hits.n_passing = "strand", 3, 6, 6
    hits.row_off = np.array([0, 4, 4, 6], dtype=np.int64)
    hits.pairs, hits.seeds, hits.strand, hits.frame = ref.pairs_ref.pairs_array(rows), seeds, np.zeros(6, dtype=np.uint8), None
    full = pkg.seed_filter(Q, R, hits, m)
    assert full.ungapped["score"].tolist() == [40, 40, 38, 40, 20, 20] and full.source.tolist() == [0, 1, 2, 3, 4, 5]
    for top_n, kept in ((1, [0, 4]), (2, [0, 1, 4, 5]), (3, [0, 1, 3, 4, 5]), (4, [0, 1, 2, 3, 4, 5])):
        f = pkg.seed_filter(Q, R, hits, m, top_n=top_n)
        assert f.source.tolist() == kept and f.row_off.tolist() == [0, min(top_n, 4), min(top_n, 4), min(top_n, 4) + min(top_n, 2)]
        _same_hits(f, _model_filter(qs, refs, hits, m, "strand", top_n=top_n), "strand", 3)


def test_letters_road_end_to_end(pkg, translated_world):
    prots = translated_world[0]
    rng = np.random.default_rng(9204)
    qs = [_mutate(rng, prots[i][a:a + 60], 0.1, b"ACDEFGHIKLMNPQRSTVWY") for i, a in zip(rng.integers(0, 60, size=50).tolist(), rng.integers(0, 240, size=50).tolist())]
    qs += [b"", b"MKW", random_protein(rng, 60)]
    P, R, ix = pkg.SeqSet.new(qs), translated_world[3], translated_world[4]
    hits = pkg.seed_pairs(P, ix, min_seeds=2, band=4, pad=8, max_occ=64, frames="letters")
    m = pkg.Matrix.from_name("blosum62")
    assert hits.kind == "letters" and len(hits) >= 50 and hits.frame is None and not hits.strand.any()
    for min_score, top_n in ((0, 0), (50, 0), (0, 1)):
        f = pkg.seed_filter(P, R, hits, m, min_score=min_score, top_n=top_n)
        assert f.kind == "letters"
        _same_hits(f, _model_filter(qs, prots, hits, m, "strand", min_score=min_score, top_n=top_n), "strand", len(qs))
    al = pkg.Aligner.new().local().matrix(m).gap_open(11).gap_extend(1).build()
    f = pkg.seed_filter(P, R, hits, m, min_score=50, top_n=1)
    assert 40 <= len(f) <= 52
    assert al.align_pairs(P, R, f.pairs).tobytes() == al.align_pairs(P, R, hits.pairs)[f.source].tobytes()


def test_frame_list_into_align_pairs(pkg, translated_world):
    prots, reads, Q, R, ix = translated_world
    m = pkg.Matrix.from_name("blosum62")
    hits = pkg.seed_pairs(Q, ix, min_seeds=2, band=4, pad=8, max_occ=64, frames="all")
    f = pkg.seed_filter(Q, R, hits, m, min_score=40, top_n=2)
    al = pkg.Aligner.new().local().matrix(m).gap_open(11).gap_extend(1).build()
    rec, frames = al.align_pairs(Q, R, f.pairs, frame=f.frame)
    rec_all, frames_all = al.align_pairs(Q, R, hits.pairs, frame=hits.frame)
    assert 0 < len(f) < len(hits) and rec.tobytes() == rec_all[f.source].tobytes() and frames.tobytes() == f.frame.tobytes() == frames_all[f.source].tobytes()


# ---- the device entry: capacity, sentinels, empty lists, determinism -------------------------------------------------------------------
def _filter_device(pkg, Q, R, hits, matrix, mq, mr, capacity, kind="strand", skip=(), **kw):
    import torch
    n, nq = len(hits.pairs), hits.n_rows
    slots = capacity + 3
    op = _full((slots * 32,), FILL, torch.uint8)
    ob = _full((slots,), FILL, torch.uint8)
    os_ = _full((slots, 4), SENTINEL, torch.int32)
    ou = _full((slots, 4), SENTINEL, torch.int32)
    osrc = _full((slots,), SENTINEL, torch.int64)
    off = _full((nq + 1 + 2,), SENTINEL, torch.int64)
    cnt = _full((2 + 2,), SENTINEL, torch.int64)
    byte = hits.frame if kind == "frame" else hits.strand
    dp, db, ds, dro = _up(hits.pairs), _up(byte), _up(hits.seeds), _up(hits.row_off)
    ptr = lambda name, t: None if name in skip else t.data_ptr()
    pkg.seed_filter_device(Q, R, n, dp.data_ptr() if n else None, db.data_ptr() if n else None, ds.data_ptr() if n else None, mq, mr, matrix, nq,
                           dro.data_ptr(), ptr("pairs", op), ptr("byte", ob), ptr("seeds", os_), ptr("ungapped", ou), ptr("source", osrc), capacity,
                           off.data_ptr(), cnt.data_ptr(), kind=kind, stream=_stream(), **kw)
    _sync()
    return {"pairs": op.cpu().numpy().view(ref.PAIR_DTYPE), "byte": ob.cpu().numpy(), "seeds": os_.cpu().numpy().reshape(-1).view(ref.SEED_HIT_DTYPE),
            "ungapped": ou.cpu().numpy().reshape(-1).view(ref.UNGAPPED_DTYPE), "source": osrc.cpu().numpy(), "row_off": off.cpu().numpy(),
            "counts": cnt.cpu().numpy()}


def _same_device(g, want, capacity, nq, skip=()):
    kept = want["counts"][0]
    w = min(kept, capacity)
    assert g["row_off"][:nq + 1].tolist() == want["row_off"].tolist() and (g["row_off"][nq + 1:] == SENTINEL).all()
    assert g["counts"][:2].tolist() == [kept, w] and (g["counts"][2:] == SENTINEL).all()
    for name, fill in (("pairs", FILL), ("byte", FILL), ("seeds", SENTINEL), ("ungapped", SENTINEL), ("source", SENTINEL)):
        a = g[name]
        raw = a.view(np.uint8 if fill == FILL else np.int64 if name == "source" else np.int32)
        per = len(raw) // len(a)
        if name in skip:
            assert (raw == fill).all(), name
            continue
        assert a[:w].tobytes() == np.ascontiguousarray(want[name][:w]).tobytes(), name
        assert (raw[w * per:] == fill).all(), name                                           # behind the written positions: untouched


def test_device_entry_capacity_sentinels_and_determinism(pkg, dna_world, dna_matrix):
    refs, reads, Q, R, hits = dna_world
    m = dna_matrix[0]
    nq, mr = len(reads), 1500
    for min_score, top_n in ((0, 0), (50, 2)):
        full = _model_filter(reads, refs, hits, m, "strand", min_score=min_score, top_n=top_n)
        kept = full["counts"][0]
        assert kept > 20
        runs = []
        for cap, chunk in ((kept + 2, 0), (kept, 7), (kept // 2, 0), (1, 0), (0, 0), (kept + 2, 1 if top_n else 0)):
            want = _model_filter(reads, refs, hits, m, "strand", min_score=min_score, top_n=top_n, capacity=cap)
            g = _filter_device(pkg, Q, R, hits, m, 150, mr, cap, min_score=min_score, top_n=top_n, chunk_pairs=chunk)
            _same_device(g, want, cap, nq)
            if cap == kept + 2:
                runs.append(b"".join(g[k].tobytes() for k in sorted(g)))
        assert runs[0] == runs[1]                                                            # run to run, and under another chunking
    want = _model_filter(reads, refs, hits, m, "strand", top_n=1, capacity=5)
    skip = ("pairs", "seeds", "source")                                                      # every output column is optional
    _same_device(_filter_device(pkg, Q, R, hits, m, 150, mr, 5, top_n=1, skip=skip), want, 5, nq, skip)


def test_device_entry_empty_lists(pkg, dna_world, dna_matrix):
    refs, reads, Q, R, hits = dna_world
    m = dna_matrix[0]

    class Empty:
        pass
    for nq in (0, 5):
        e = Empty()
        e.n_rows, e.pairs, e.strand, e.seeds, e.frame = nq, hits.pairs[:0], hits.strand[:0], hits.seeds[:0], None
        e.row_off = np.zeros(nq + 1, dtype=np.int64)
        want = {"row_off": e.row_off, "counts": [0, 0], "pairs": e.pairs, "byte": e.strand, "seeds": e.seeds,
                "ungapped": np.zeros(0, dtype=ref.UNGAPPED_DTYPE), "source": np.zeros(0, dtype=np.int64)}
        _same_device(_filter_device(pkg, Q, R, e, m, 150, 1500, 4, top_n=2), want, 4, nq)
    # rows without candidates between rows that have some: row offsets repeat
    per_row = np.diff(hits.row_off)
    f = pkg.seed_filter(Q, R, hits, m, top_n=1)
    assert (np.diff(f.row_off) == (per_row > 0)).all()
