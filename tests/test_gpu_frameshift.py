"""The frameshift-aware entries (`-m gpu`): pmx_swfs_kernel behind pmx_align_pairs_frameshift[_device], the searches and the gather
hook, against the CPU model tests/swfs_model.c (tests/frameshift_ref.py).  Records are compared byte for byte unless said otherwise;
every output buffer starts as a sentinel."""
import numpy as np
import pytest

import frameshift_ref as fs
import pairs_ref
import set_search_ref
import topk_ref
import strands_ref
from pairs_ex_ref import revcomp
from test_gpu_translate import _up, _full, _stream, _sync, _ptr, _pairs_up, back_translate, SENTINEL, FILL
from util import random_seqs, AA, golden

pytestmark = pytest.mark.gpu

FWD, REV, BOTH = 0, 1, 2
LIST, TRI, RECT = 0, 1, 2
G, R = 16, 10                   # the shipped instantiation: a strip is G * R rows
INT32_MIN = -(1 << 31)
BAD = fs.BAD


def _b62(pkg, orc):
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))


def _cfg(pkg, pm, open_=11, ext=1, width=0):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, open_, ext, width, 0, pm.inner)


def _align(pkg, cfg, Q, Rs, pairs, mode, f, mq, mr, chunk=0, strands=None):
    """pmx_align_pairs_frameshift_device -> records, strand bytes, kernel"""
    import torch
    n = len(pairs)
    rec = _full((n + 2, 4), SENTINEL, torch.int32)
    won = _full((n + 2,), FILL, torch.uint8)
    d_pairs = _pairs_up(pairs)
    d_strand = _up(np.asarray(strands, dtype=np.uint8)) if strands is not None else None
    pkg.align_pairs_frameshift_device(cfg, Q, Rs, n, d_pairs.data_ptr(), _ptr(d_strand), mode, f, mq, mr, rec.data_ptr(), won.data_ptr(),
                                      _stream(), chunk)
    kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    rec, won = rec.cpu().numpy(), won.cpu().numpy()
    assert (rec[n:] == SENTINEL).all() and (won[n:] == FILL).all()
    return rec[:n], won[:n], kernel


def _same(got, want):
    assert got[1].tolist() == want[1].tolist()
    assert got[0].tobytes() == want[0].tobytes()


def _dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


# --------------------------------------------------------------------------------------------------------------- 1. top-row edges
def test_top_row_edges(pkg, orc):
    """every window W = 3 .. 12 against every m = 1 .. 5: rows 0 .. 3 have missing predecessors"""
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(15200)
    prots = [p for m in range(1, 6) for p in random_seqs(rng, 4, m, m, AA)]
    reads = []
    for W in range(3, 13):
        for rep in range(4):
            p = prots[int(rng.integers(0, len(prots)))]
            s = (back_translate(rng, p) + _dna(rng, 12))[:W]                       # the start of a read that codes for a reference
            reads.append(_dna(rng, rep % 3) + s[:W - rep % 3] if rep else s)
    assert sorted({len(s) for s in reads}) == list(range(3, 13))
    Q, Rs = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    pairs = pairs_ref.pairs_array([(i, j) for i in range(len(reads)) for j in range(len(prots))])
    positive = 0
    for open_, ext in ((11, 1), (2, 1)):
        cfg = _cfg(pkg, pm, open_, ext)
        for f in (0, 1, 15):
            want = fs.records(reads, prots, pairs, BOTH, om, open_, ext, f)
            got = _align(pkg, cfg, Q, Rs, pairs, BOTH, f, 10, 5)
            _same(got, want)
            assert got[2] == "pmx_swfs_kernel<16,10>"
            positive += int((want[0][:, 0] > 0).sum())
    assert positive > 1000


# ------------------------------------------------------------------------------------------------- 2. hand-off and strip edges
def _noisy_read(rng, prot, W):
    """W nucleotides that code for `prot` over and over, with a single-nucleotide deletion or insertion every 25 - 45 nt and now and
    then a whole codon dropped or added"""
    out = bytearray()
    nxt = int(rng.integers(10, 30))
    while len(out) < W + 8:
        for b in back_translate(rng, prot):
            out.append(b)
            nxt -= 1
            if nxt <= 0:
                kind = int(rng.integers(0, 6))
                if kind in (0, 1):
                    out.pop()                                                       # one nucleotide missing
                elif kind in (2, 3):
                    out += _dna(rng, 1)                                             # one nucleotide too many
                elif kind == 4:
                    del out[-3:]                                                    # a codon missing
                else:
                    out += _dna(rng, 3)                                             # a codon too many
                nxt = int(rng.integers(25, 46))
    return bytes(out[:W])


def _anchored_read(rng, prot, W):
    """W nucleotides that END in a noisy coding of `prot` behind a random flank: the alignment's last rows are the stream's last"""
    tail = _noisy_read(rng, prot, min(W, 3 * len(prot) + 2))
    return _dna(rng, W - len(tail)) + tail


def test_handoff_and_strip_edges(pkg, orc):
    """one batch with every N from 1 to 2 G R + 5 against m = 40: every lane boundary and the seams of the first and second strip.
    Even N: the coding piece sits at the read's end, so its 120 rows cross whatever boundary lies above row N; odd N: the read codes
    for its reference over and over from row 0."""
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(15300)
    prots = random_seqs(rng, 12, 40, 40, AA)
    top = 2 * G * R + 5
    reads = [(_noisy_read if N % 2 else _anchored_read)(rng, prots[N % 12], N + 2) for N in range(1, top + 1)]
    Q, Rs = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    pairs = pairs_ref.pairs_array([(N - 1, N % 12) for N in range(1, top + 1)])
    cfg = _cfg(pkg, pm)
    for f in (15, 1):
        want = fs.records(reads, prots, pairs, BOTH, om, 11, 1, f)
        got = _align(pkg, cfg, Q, Rs, pairs, BOTH, f, top, 40)
        _same(got, want)
        assert got[2] == "pmx_swfs_kernel<16,10>/strips"
    ends = want[0][:, 1] - 2                                                        # the best cell's row: in every lane, beyond both seams
    assert {int(e) % (G * R) // R for e in ends} == set(range(G)) and (ends >= 2 * G * R).any() and (ends[:G * R] < G * R).all()
    noshift = fs.records(reads, prots, pairs, BOTH, om, 11, 1, 1 << 20)
    assert (want[0][:, 0] > noshift[0][:, 0]).sum() > top // 2                      # the frameshift terms decide most of these scores
    # one strip alone takes the kernel without scratch, and the same records
    short = pairs[:G * R]
    got = _align(pkg, cfg, Q, Rs, short, BOTH, 1, G * R, 40, chunk=7)
    assert got[2] == "pmx_swfs_kernel<16,10>" and got[0].tobytes() == want[0][:G * R].tobytes()
    # N beyond max_qlen: the bad record, the neighbours unaffected
    got = _align(pkg, cfg, Q, Rs, pairs, BOTH, 1, 200, 40)
    assert got[0][:200].tobytes() == want[0][:200].tobytes() and all(r.tolist() == BAD for r in got[0][200:]) and not got[1][200:].any()


def test_window_cap(pkg, orc):
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(15400)
    cap = pkg.frameshift_max_window()
    prots = random_seqs(rng, 1, 40, 40, AA)
    reads = [_noisy_read(rng, prots[0], cap), _noisy_read(rng, prots[0], cap + 1)]
    Q, Rs = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    cfg = _cfg(pkg, pm)
    pairs = pairs_ref.pairs_array([(0, 0), (1, 0)])
    want = fs.records(reads, prots, pairs, BOTH, om, 11, 1, 15, max_qlen=cap - 2)
    assert want[0][1].tolist() == BAD and want[0][0][0] > 100
    _same(_align(pkg, cfg, Q, Rs, pairs, BOTH, 15, cap - 2, 40), want)              # the window at the cap runs; cap + 1 exceeds max_qlen
    with pytest.raises(pkg.BatchError, match="PMX_FRAMESHIFT_MAX_WINDOW"):
        _align(pkg, cfg, Q, Rs, pairs, BOTH, 15, cap - 1, 40)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    rec, won = al.align_pairs(Q, Rs, pairs[:1], frameshift=15, strand="both")
    assert rec.view(np.int32).reshape(-1, 4).tobytes() == want[0][:1].tobytes() and won.tolist() == want[1][:1].tolist()
    with pytest.raises(pkg.BatchError, match="PMX_FRAMESHIFT_MAX_WINDOW"):
        al.align_pairs(Q, Rs, pairs, frameshift=15, strand="both")
    with pytest.raises(pkg.BatchError, match="PMX_FRAMESHIFT_MAX_WINDOW"):
        al.search_pairs(Q, Rs, frameshift=15)


# ------------------------------------------------------------------------------------------------------- 3. a planted frameshift
def test_planted_frameshift(pkg, orc):
    """120-nt reads that code for 40 aa of their reference, nucleotide 60 deleted: the six-frame fold keeps half of the alignment, the
    three-frame DP the whole of it; with an unpayable penalty the two roads agree"""
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(15500)
    prots = random_seqs(rng, 24, 60, 90, AA)
    reads = []
    for p in prots:
        a = int(rng.integers(0, len(p) - 40))
        s = back_translate(rng, p[a:a + 40])
        reads.append(s[:60] + s[61:])
    Q, Rs = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    pairs = pairs_ref.pairs_array([(i, i) for i in range(24)])
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    fwd3 = al.align_pairs(Q, Rs, pairs, frame="forward")[0]["score"]
    rec15, won = al.align_pairs(Q, Rs, pairs, frameshift=15, strand=0)
    want = fs.records(reads, prots, pairs, FWD, om, 11, 1, 15)
    assert rec15.view(np.int32).reshape(-1, 4).tobytes() == want[0].tobytes() and not won.any()
    assert (rec15["score"] > fwd3).all()
    assert (rec15["score"] >= fwd3 + 40).all()                                       # the other half of the read, less the penalty
    big = al.align_pairs(Q, Rs, pairs, frameshift=1 << 20, strand=0)[0]
    assert big["score"].tolist() == fwd3.tolist()
    huge = al.align_pairs(Q, Rs, pairs, frameshift=(1 << 31) - 1, strand=0)[0]      # clamped, not wrapped
    assert huge.tobytes() == big.tobytes()
    assert big.view(np.int32).reshape(-1, 4).tobytes() == fs.records(reads, prots, pairs, FWD, om, 11, 1, 1 << 20)[0].tobytes()


# ------------------------------------------------------------------------------------------------------------------- 4. the width
@pytest.mark.parametrize("width", [0, 32])
def test_scores_beyond_int16(pkg, orc, width):
    """match 127 on N = 600 x m = 300: a poly-K protein against a poly-A read, whose every codon reads K.  With a free frameshift
    the best path takes every second row, 300 matches: 38 100 exceeds int16 and comes back exact."""
    letters = "ARNDCQEGHILKMFPSTWYV"
    pm, om = pkg.Matrix.create(letters.encode(), 127, -127), orc.Matrix.create(letters, 127, -127)
    reads, prots = [b"A" * 602], [b"K" * 300]
    Q, Rs = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    pairs = pairs_ref.pairs_array([(0, 0)] * 6)
    want = fs.records(reads, prots, pairs, FWD, om, 11, 1, 0)
    assert want[0][0].tolist() == [300 * 127, 598 + 2, 299, 0] and 300 * 127 > 32767      # the last column, the first row that 300 steps of two reach
    got = _align(pkg, _cfg(pkg, pm, width=width), Q, Rs, pairs, FWD, 0, 600, 300)
    _same(got, want)
    assert "pmx_swfs_kernel" in got[2]


# ---------------------------------------------------------------------------------------------------------------- 5. the strands
def test_strands(pkg, orc):
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(15600)
    prots = random_seqs(rng, 10, 20, 50, AA)
    reads = []
    for i in range(30):
        p = prots[i % 10]
        s = _noisy_read(rng, p[int(rng.integers(0, 8)):], int(rng.integers(20, 140)))
        reads.append(revcomp(s) if i % 2 else s)
    half = back_translate(rng, prots[0][2:14])
    pal = half + revcomp(half)                                                      # equals its reverse complement: the strands tie
    assert pal == revcomp(pal)
    reads.append(pal)
    Q, Rs = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    Qrc = pkg.SeqSet.new([revcomp(s) for s in reads])
    rows = [(i, j) for i in range(len(reads)) for j in range(len(prots))]
    rows += [(3, 2, 5, 40, 1, -1), (4, 1, 2, -1, 0, 12), (30, 0, 3, 60, 0, -1)]     # windows: the reverse strand is the window's
    pairs = pairs_ref.pairs_array(rows)
    cfg = _cfg(pkg, pm)
    mq, mr = 140, 50
    fwd = _align(pkg, cfg, Q, Rs, pairs[:310], FWD, 15, mq, mr)
    rev = _align(pkg, cfg, Q, Rs, pairs[:310], REV, 15, mq, mr)
    fwd_rc = _align(pkg, cfg, Qrc, Rs, pairs[:310], FWD, 15, mq, mr)
    assert rev[0].tobytes() == fwd_rc[0].tobytes() and (rev[1] == 1).all() and not fwd[1].any()
    for mode in (FWD, REV, BOTH):
        want = fs.records(reads, prots, pairs, mode, om, 11, 1, 15)
        for chunk in (0, 7, 1):
            _same(_align(pkg, cfg, Q, Rs, pairs, mode, 15, mq, mr, chunk), want)
    both = _align(pkg, cfg, Q, Rs, pairs, BOTH, 15, mq, mr)
    f2, r2 = _align(pkg, cfg, Q, Rs, pairs, FWD, 15, mq, mr), _align(pkg, cfg, Q, Rs, pairs, REV, 15, mq, mr)
    folded = strands_ref.fold(f2[0], r2[0])
    assert both[0].tobytes() == folded[0].tobytes() and both[1].tolist() == folded[2].tolist()
    assert 20 < int(both[1].sum()) < len(pairs) - 20                                # both strands win somewhere
    k = rows.index((30, 0))
    assert f2[0][k].tolist() == r2[0][k].tolist() and f2[0][k][0] > 40 and both[1][k] == 0      # the tie goes to forward
    # a strand byte per pair
    sb = rng.integers(0, 2, len(pairs)).astype(np.uint8)
    want = fs.records(reads, prots, pairs, FWD, om, 11, 1, 15, strands=sb)
    _same(_align(pkg, cfg, Q, Rs, pairs, FWD, 15, mq, mr, 7, strands=sb), want)
    assert want[1].tolist() == sb.tolist()


# ------------------------------------------------------------------------------------------------------------------ 6. bad pairs
def test_bad_pairs(pkg, orc):
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(15700)
    prots = random_seqs(rng, 4, 10, 30, AA)
    reads = [_noisy_read(rng, prots[0], 60), b"AT", b"A", b"ATG", _noisy_read(rng, prots[1], 33)]
    Q, Rs = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    rows = [(0, 0), (4, 1), (1, 0), (3, 2), (2, 1), (0, 4), (5, 0), (0, 1, 59, -1, 0, -1), (0, 1, 58, 2, 0, -1), (0, 1, 57, 3, 0, -1),
            (4, 0, 0, -1, 40, 2), (4, 3)]
    pairs = pairs_ref.pairs_array(rows)
    cfg = _cfg(pkg, pm)
    bad_at = [2, 4, 5, 6, 7, 8, 10]
    for mode in (FWD, REV, BOTH):
        want = fs.records(reads, prots, pairs, mode, om, 11, 1, 15)
        assert [k for k in range(len(rows)) if want[0][k].tolist() == BAD] == bad_at
        for chunk in (0, 1, 5):
            _same(_align(pkg, cfg, Q, Rs, pairs, mode, 15, 60, 30, chunk), want)
    sb = np.array([0, 1, 0, 2, 1, 0, 0, 1, 1, 255, 0, 1], dtype=np.uint8)              # strand bytes outside {0, 1}: pairs 3 and 9
    want = fs.records(reads, prots, pairs, FWD, om, 11, 1, 15, strands=sb)
    assert [k for k in range(len(rows)) if want[0][k].tolist() == BAD] == sorted(bad_at + [3, 9])
    _same(_align(pkg, cfg, Q, Rs, pairs, FWD, 15, 60, 30, 5, strands=sb), want)
    # the host entries name the first bad pair
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    with pytest.raises(pkg.BatchError, match="pair 2: "):
        al.align_pairs(Q, Rs, pairs, frameshift=15, strand="both")
    with pytest.raises(pkg.BatchError, match="pair 3: strand byte 2"):
        al.align_pairs(Q, Rs, pairs[:4], frameshift=15, strand=sb[:4])
    with pytest.raises(pkg.BatchError, match="pair 5: "):
        al.align_pairs(Q, Rs, pairs[[0, 1, 3, 9, 11, 5]], frameshift=15, strand=1)
    with pytest.raises(pkg.BatchError, match="pair 2"):
        al.search_pairs(Q, Rs, pairs=pairs, frameshift=15, strand="both")
    with pytest.raises(pkg.BatchError, match="pair 4 "):                             # rectangle 5 x 4: read 1 (W = 2) against protein 0
        al.search_topk(Q, Rs, k=2, frameshift=15, strand="both")
    rec, won = al.align_pairs(Q, Rs, pairs[[0, 1, 3, 9, 11]], frameshift=15, strand="both")
    want = fs.records(reads, prots, pairs[[0, 1, 3, 9, 11]], BOTH, om, 11, 1, 15)
    assert rec.view(np.int32).reshape(-1, 4).tobytes() == want[0].tobytes() and won.tolist() == want[1].tolist()


# ------------------------------------------------------------------------------------------------------------ 7. search and top-K
NQ, NR = 40, 30


class Sets:
    pass


@pytest.fixture(scope="module")
def sets(pkg, orc):
    """40 reads x 30 proteins and the model's records of the rectangle per strand mode -- computed once, shared, left unchanged"""
    p = Sets()
    p.pm, p.om = _b62(pkg, orc)
    rng = np.random.default_rng(15800)
    p.prots = random_seqs(rng, NR, 25, 60, AA)
    p.reads = []
    for i in range(NQ):
        s = _noisy_read(rng, p.prots[(i * 7) % NR][int(rng.integers(0, 6)):], int(rng.integers(40, 151)))
        p.reads.append(revcomp(s) if i % 3 == 1 else s)
    p.Q, p.R = pkg.SeqSet.new(p.reads), pkg.SeqSet.new(p.prots)
    p.rect = set_search_ref.rect_pairs_descriptors(NR, 0, NQ * NR)
    p.model = {mode: fs.records(p.reads, p.prots, p.rect, mode, p.om, 11, 1, 15) for mode in (FWD, REV, BOTH)}
    p.al = pkg.Aligner.new().local().matrix(p.pm).gap_open(11).gap_extend(1).build()
    return p


def _search_dev(pkg, cfg, p, first, n, min_score, capacity, mode, f, chunk=0, pairs=None):
    import torch
    slots = capacity + 3
    hp = _full((slots * 32,), FILL, torch.uint8); hi = _full((slots,), SENTINEL, torch.int64)
    hr = _full((slots, 4), SENTINEL, torch.int32); hb = _full((slots,), FILL, torch.uint8)
    cnt = _full((2,), SENTINEL, torch.int64)
    d_pairs = _pairs_up(pairs) if pairs is not None else None
    pkg.search_pairs_frameshift_device(cfg, p.Q, p.R, LIST if pairs is not None else RECT, first, n, _ptr(d_pairs), 150, 60, min_score,
                                       hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), capacity, cnt.data_ptr(), mode, f, hb.data_ptr(), _stream(), chunk)
    _sync()
    return [hp.cpu().numpy().view(pairs_ref.PAIR_DTYPE), hi.cpu().numpy(), hr.cpu().numpy(), hb.cpu().numpy(), cnt.cpu().numpy()]


def _check_search(g, want, strand, first, capacity):
    pairs, index, recs, sb, cnt = g
    w = min(want["passing"], capacity)
    assert cnt.tolist() == [want["passing"], w]
    assert recs[:w].tobytes() == want["records"][:w].tobytes() and (recs[w:] == SENTINEL).all()
    assert index[:w].tolist() == want["index"][:w].tolist() and (index[w:] == SENTINEL).all()
    assert pairs[:w].tobytes() == want["pairs"][:w].tobytes() and (pairs[w:].view(np.uint8) == FILL).all()
    assert sb[:w].tolist() == strand[want["index"][:w] - first].tolist() and (sb[w:] == FILL).all()


def test_search_on_folded_records(pkg, sets):
    p = sets
    cfg = _cfg(pkg, p.pm)
    first, n = 7, NQ * NR - 19                                                        # a window that starts and ends inside a row
    for mode in (BOTH, REV):
        rec, won = p.model[mode]
        ms = int(np.sort(rec[:, 0])[-NQ * NR // 12])
        want = set_search_ref.hits(rec[first:first + n], ms, first, p.rect[first:first + n])
        assert 60 <= want["passing"] <= 200
        if mode == BOTH:
            assert len(set(won[want["index"]].tolist())) == 2
        runs = [_search_dev(pkg, cfg, p, first, n, ms, n, mode, 15, chunk) for chunk in (7, 0, 1, 7)]
        for g in runs:
            _check_search(g, want, won[first:first + n], first, n)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(g, runs[0]))       # bit-identical, whatever the chunk, run after run
        assert (runs[0][2][:want["passing"], 3] == 0).all()                          # the strand mark does not reach the caller
        for cap in (0, 1, want["passing"] - 1, want["passing"] + 5):
            cut = set_search_ref.hits(rec[first:first + n], ms, first, p.rect[first:first + n], capacity=cap)
            _check_search(_search_dev(pkg, cfg, p, first, n, ms, cap, mode, 15, 7), cut, won[first:first + n], first, cap)
    # a listed window of the rectangle
    rec, won = p.model[BOTH]
    sel = np.arange(3, NQ * NR, 11)
    want = set_search_ref.hits(rec[sel], 30, 0, p.rect[sel])
    _check_search(_search_dev(pkg, cfg, p, 0, len(sel), 30, len(sel), BOTH, 15, 7, pairs=p.rect[sel]), want, won[sel], 0, len(sel))
    # the host entry: slices of 1, 7 and the default
    ms = int(np.sort(rec[:, 0])[-NQ * NR // 12])
    want = set_search_ref.hits(rec, ms, 0, p.rect)
    for chunk, sl in ((0, 0), (7, 7), (1, 0), (0, 1), (7, 0)):
        h = p.al.search_pairs(p.Q, p.R, min_score=ms, frameshift=15, strand="both", chunk_pairs=chunk, slice_pairs=sl)
        assert h.n_hits == h.n_passing == want["passing"] and h.index.tolist() == want["index"].tolist()
        assert h.records.view(np.int32).reshape(-1, 4).tobytes() == want["records"].tobytes() and h.pairs.tobytes() == want["pairs"].tobytes()
        assert h.strand.tolist() == won[want["index"]].tolist()
    h = p.al.search_pairs(p.Q, p.R, min_score=ms, frameshift=15, strand="both", max_hits=9, slice_pairs=100)
    assert h.n_hits == 9 and h.n_passing == want["passing"] and h.index.tolist() == want["index"][:9].tolist()
    # the hit descriptors stay a valid pair list
    rec2, won2 = p.al.align_pairs(p.Q, p.R, h.pairs, frameshift=15, strand=h.strand)
    assert rec2.tobytes() == h.records.tobytes() and won2.tolist() == h.strand.tolist()


def _topk_dev(pkg, cfg, p, q_first, nq, min_score, k, capacity, mode, f, chunk=0):
    import torch
    slots = capacity + 3
    hp = _full((slots * 32,), FILL, torch.uint8); hi = _full((slots,), SENTINEL, torch.int64)
    hr = _full((slots, 4), SENTINEL, torch.int32); hb = _full((slots,), FILL, torch.uint8)
    off = _full((nq + 3,), SENTINEL, torch.int64); rp = _full((nq + 2,), SENTINEL, torch.int64); cnt = _full((5,), SENTINEL, torch.int64)
    pkg.search_topk_frameshift_device(cfg, p.Q, p.R, q_first, nq, 150, 60, min_score, k, False, hp.data_ptr(), hi.data_ptr(), hr.data_ptr(),
                                      capacity, off.data_ptr(), rp.data_ptr(), cnt.data_ptr(), mode, f, hb.data_ptr(), _stream(), chunk)
    _sync()
    return [hp.cpu().numpy().view(pairs_ref.PAIR_DTYPE), hi.cpu().numpy(), hr.cpu().numpy(), hb.cpu().numpy(), off.cpu().numpy(), rp.cpu().numpy(),
            cnt.cpu().numpy()]


def test_topk_on_folded_records(pkg, sets):
    p = sets
    cfg = _cfg(pkg, p.pm)
    q_first, nq = 3, NQ - 5
    for mode, k, ms in ((BOTH, 4, INT32_MIN), (BOTH, 50, 25), (REV, 3, 20)):
        rec, won = p.model[mode]
        part = rec[q_first * NR:(q_first + nq) * NR]
        want = topk_ref.topk(part, NR, q_first, nq, k, ms)
        kept = int(want["row_off"][-1])
        cap = nq * min(k, NR)
        runs = [_topk_dev(pkg, cfg, p, q_first, nq, ms, k, cap, mode, 15, chunk) for chunk in (7, 0, 1, 7)]
        for g in runs:
            pairs, index, recs, sb, off, rp, cnt = g
            assert off[:nq + 1].tolist() == want["row_off"].tolist() and (off[nq + 1:] == SENTINEL).all()
            assert cnt[:3].tolist() == [kept, kept, int(want["row_passing"].sum())] and (cnt[3:] == SENTINEL).all()
            assert rp[:nq].tolist() == want["row_passing"].tolist() and (rp[nq:] == SENTINEL).all()
            assert recs[:kept].tobytes() == want["records"].tobytes() and (recs[kept:] == SENTINEL).all()
            assert index[:kept].tolist() == want["index"].tolist() and pairs[:kept].tobytes() == want["pairs"].tobytes()
            assert sb[:kept].tolist() == won[want["index"]].tolist() and (sb[kept:] == FILL).all()
            assert (recs[:kept, 3] == 0).all()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(g, runs[0]))
    rec, won = p.model[BOTH]
    want = topk_ref.topk(rec, NR, 0, NQ, 5, 20)
    for chunk, sl in ((0, 0), (7, 7), (1, 0), (0, 1)):
        t = p.al.search_topk(p.Q, p.R, k=5, min_score=20, frameshift=15, strand="both", chunk_pairs=chunk, slice_rows=sl)
        assert t.row_off.tolist() == want["row_off"].tolist() and t.row_passing.tolist() == want["row_passing"].tolist()
        assert t.records.view(np.int32).reshape(-1, 4).tobytes() == want["records"].tobytes() and t.index.tolist() == want["index"].tolist()
        assert t.pairs.tobytes() == want["pairs"].tobytes() and t.strand.tolist() == won[want["index"]].tolist()
    assert len(set(t.strand.tolist())) == 2


# ------------------------------------------------------------------------------------------------------------- 8. the gather hook
def test_gather_codons_at_the_sets_edges(pkg):
    """windows that begin at a set's first byte and end at its last, both strands, over sets wrapped around exactly their bytes"""
    import torch
    rng = np.random.default_rng(15900)
    letters = np.frombuffer(b"ACGTACGTACGTacgtUuN-", dtype=np.uint8)
    qseqs = [letters[rng.integers(0, len(letters), size=l)].tobytes() for l in (31, 2, 3, 4, 5, 6, 7, 8, 9, 17, 64, 1, 29)]
    rseqs = random_seqs(rng, 5, 1, 9, AA)
    rows, strands = [], []
    for i in range(len(qseqs)):
        for s in (0, 1):
            rows.append((i, (i + s) % 5)); strands.append(s)
    for i, b, l in ((0, 0, 3), (0, 0, 12), (0, 1, -1), (0, 28, 3), (12, 0, -1), (12, 26, 3), (12, 20, -1), (12, 1, 28), (10, 5, 40), (10, 0, 2)):
        for s in (0, 1):
            rows.append((i, 0, b, l, 0, -1)); strands.append(s)
    rows += [(13, 0), (0, 5), (0, 0)]; strands += [0, 1, 2]                                       # bad descriptors, a bad strand byte
    pairs = pairs_ref.pairs_array(rows)
    n = len(pairs)
    want = []
    for d, s in zip(pairs, strands):
        q = pairs_ref.resolve_side(qseqs, d["q"], d["q_beg"], d["q_len"]); r = pairs_ref.resolve_side(rseqs, d["r"], d["r_beg"], d["r_len"], 9)
        want.append(None if q is None or r is None or len(q) < 3 or s > 1 else (pkg.codon_stream(q, s), r))
        if want[-1]:
            assert want[-1][0] == fs.codon_stream(q, s)
    assert sum(w is None for w in want) == 2 * 2 + 2 + 3 and any(w and b"X" in w[0] for w in want)
    qwant = b"".join(w[0] if w else b"\0" for w in want); rwant = b"".join(w[1] if w else b"\0" for w in want)
    qoffw = np.concatenate([[0], np.cumsum([len(w[0]) if w else 1 for w in want])]); roffw = np.concatenate([[0], np.cumsum([len(w[1]) if w else 1 for w in want])])
    assert {int(o) % 4 for o, w in zip(qoffw, want) if w} == {0, 1, 2, 3}
    qb, qo = pkg.pack(qseqs); rb, ro = pkg.pack(rseqs)
    keep = (_up(qb), _up(qo), _up(rb), _up(ro))
    WQ = pkg.SeqSet.wrap_device(keep[0].data_ptr(), keep[1].data_ptr(), len(qseqs), len(qb), keep=keep[:2])
    WR = pkg.SeqSet.wrap_device(keep[2].data_ptr(), keep[3].data_ptr(), len(rseqs), len(rb), keep=keep[2:])
    for SQ, SR in ((pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)), (WQ, WR)):
        qout = _full((len(qwant) + 32,), FILL, torch.uint8); rout = _full((len(rwant) + 32,), FILL, torch.uint8)
        qoff = _full((n + 3,), SENTINEL, torch.int64); roff = _full((n + 3,), SENTINEL, torch.int64)
        ok = _full((n + 2,), FILL, torch.uint8)
        d_pairs = _pairs_up(pairs); d_strand = _up(np.asarray(strands, dtype=np.uint8))
        pkg.gather_pairs_codons_device(SQ, SR, n, d_pairs.data_ptr(), d_strand.data_ptr(), 62, 9, qout.data_ptr() + 16, len(qwant), qoff.data_ptr(),
                                       rout.data_ptr() + 16, len(rwant), roff.data_ptr(), ok.data_ptr(), _stream())
        _sync()
        qout, qoff, rout, roff, ok = [t.cpu().numpy() for t in (qout, qoff, rout, roff, ok)]
        assert qoff[:n + 1].tolist() == qoffw.tolist() and roff[:n + 1].tolist() == roffw.tolist()
        assert ok[:n].tolist() == [1 if w else 0 for w in want] and (ok[n:] == FILL).all()
        assert qout[16:16 + len(qwant)].tobytes() == qwant and rout[16:16 + len(rwant)].tobytes() == rwant
        assert (qout[:16] == FILL).all() and (qout[16 + len(qwant):] == FILL).all()
        assert (rout[:16] == FILL).all() and (rout[16 + len(rwant):] == FILL).all()
