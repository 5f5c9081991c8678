"""The reference-side frameshift-aware entries (`-m gpu`): pmx_swfsc_kernel behind pmx_align_pairs_frameshift_ref[_device], the
searches and the gather hook, against the CPU model tests/swfsc_model.c (tests/frameshift_ref_side.py).  Everything is compared byte
for byte; every output buffer starts as a sentinel."""
import numpy as np
import pytest

import frameshift_ref_side as fr
import pairs_ref
import set_search_ref
import translate_ref
from pairs_ex_ref import revcomp
from test_gpu_translate import _up, _full, _stream, _sync, _ptr, _pairs_up, back_translate, SENTINEL, FILL
from util import random_seqs, AA, golden

pytestmark = pytest.mark.gpu

FWD, REV, BOTH = 0, 1, 2
LIST, TRI, RECT = 0, 1, 2
BAD = fr.BAD
BIG = 1 << 30


def _b62(pkg, orc):
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))


def _cfg(pkg, pm, open_=11, ext=1, width=0):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, open_, ext, width, 0, pm.inner)


def _shape(pkg):
    """(R^, S^): rows per lane and per strip of the shipped instantiation"""
    return pkg.lib.pmx_swfsc_lane_rows(), pkg.lib.pmx_swfsc_strip_rows()


def _align(pkg, cfg, Q, Rs, pairs, mode, f, mq, mr, chunk=0, strands=None):
    """pmx_align_pairs_frameshift_ref_device -> records, strand bytes, kernel"""
    import torch
    n = len(pairs)
    rec = _full((n + 2, 4), SENTINEL, torch.int32)
    won = _full((n + 2,), FILL, torch.uint8)
    d_pairs = _pairs_up(pairs)
    d_strand = _up(np.asarray(strands, dtype=np.uint8)) if strands is not None else None
    pkg.align_pairs_frameshift_ref_device(cfg, Q, Rs, n, d_pairs.data_ptr(), _ptr(d_strand), mode, f, mq, mr, rec.data_ptr(), won.data_ptr(),
                                          _stream(), chunk)
    kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    rec, won = rec.cpu().numpy(), won.cpu().numpy()
    assert (rec[n:] == SENTINEL).all() and (won[n:] == FILL).all()
    return rec[:n], won[:n], kernel


def _same(got, want):
    assert got[1].tolist() == want[1].tolist()
    bad = np.nonzero((got[0] != want[0]).any(axis=1))[0]
    assert got[0].tobytes() == want[0].tobytes(), (bad[:5], got[0][bad[:5]], want[0][bad[:5]])


def _dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _gene(rng, prot, shifts=()):
    """a nucleotide string whose frame 0 reads `prot`; shifts: (letter, kind) -- behind the codon of that letter one base is dropped
    from the NEXT codon (kind 0: the path's next match steps two columns) or one is inserted (kind 1: four columns)"""
    out = bytearray()
    at = dict(shifts)
    for i, a in enumerate(prot):
        c = back_translate(rng, bytes([a]))
        if at.get(i - 1) == 0:
            c = c[1:]
        elif at.get(i - 1) == 1:
            c = _dna(rng, 1) + c
        out += c
    return bytes(out)


def _noisy_gene(rng, prot, W):
    """W nucleotides that code for `prot` over and over with a single-base deletion or insertion every 25 - 45 nt"""
    out = bytearray()
    nxt = int(rng.integers(10, 30))
    while len(out) < W + 8:
        for b in back_translate(rng, prot):
            out.append(b)
            nxt -= 1
            if nxt <= 0:
                if int(rng.integers(0, 2)):
                    out.pop()
                else:
                    out += _dna(rng, 1)
                nxt = int(rng.integers(25, 46))
    return bytes(out[:W])


# ------------------------------------------------------------------------------------------------------- 1. column-history edges
def test_column_history_edges(pkg, orc):
    """every N = 1 .. 30 against m in {1, 2, 3, R^ - 1, R^, R^ + 1, 2 R^}: the columns where j - 2 .. j - 4 do not exist and every
    residue of the ring and unroll period; fs 0, 3, 15 and 2^30, gaps 11 / 1 and 2^30 / 2^30"""
    pm, om = _b62(pkg, orc)
    R, S = _shape(pkg)
    rng = np.random.default_rng(17400)
    ms = [1, 2, 3, R - 1, R, R + 1, 2 * R]
    prots = [p for m in ms for p in random_seqs(rng, 2, m, m, AA)]
    refs = []
    for W in range(3, 33):
        for rep in range(3):
            p = prots[int(rng.integers(0, len(prots)))]
            g = _gene(rng, p, [(int(rng.integers(0, len(p))), rep % 2)] if rep else ())
            refs.append((_dna(rng, rep) + g + _dna(rng, 32))[:W])
    assert sorted({len(s) - 2 for s in refs}) == list(range(1, 31))
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    pairs = pairs_ref.pairs_array([(i, j) for i in range(len(prots)) for j in range(len(refs))])
    positive = shifted = 0
    for open_, ext in ((11, 1), (BIG, BIG)):
        cfg = _cfg(pkg, pm, open_, ext)
        for f in (0, 3, 15, BIG):
            want = fr.records(prots, refs, pairs, BOTH, om, open_, ext, f)
            got = _align(pkg, cfg, Q, Rs, pairs, BOTH, f, 2 * R, 30)
            _same(got, want)
            assert got[2] == "pmx_swfsc_kernel<16,%d>" % R
            positive += int((want[0][:, 0] > 0).sum())
            if f == 3:
                shifted += int((want[0][:, 0] > fr.records(prots, refs, pairs, BOTH, om, open_, ext, BIG)[0][:, 0]).sum())
    assert positive > 4000 and shifted > 50


# --------------------------------------------------------------------------------------------------------- 2. lane and strip edges
def test_lane_and_strip_edges(pkg, orc):
    """m in {S^ - 1, S^, S^ + 1, 2 S^, 2 S^ + 1} x N in {7, 100, 301}, the references coding for their query with single-base shifts"""
    pm, om = _b62(pkg, orc)
    R, S = _shape(pkg)
    rng = np.random.default_rng(17500)
    ms = [S - 1, S, S + 1, 2 * S, 2 * S + 1]
    prots = [random_seqs(rng, 1, m, m, AA)[0] for m in ms]
    refs, rows = [], []
    for i, p in enumerate(prots):
        for N in (7, 100, 301):
            a = int(rng.integers(0, len(p) - 110))
            refs.append(_noisy_gene(rng, p[a:a + 110], N + 2)); rows.append((i, len(refs) - 1))
            tail = _noisy_gene(rng, p[len(p) - 30:], min(N + 2, 92))                 # the alignment's last rows are the query's last
            refs.append(_dna(rng, N + 2 - len(tail)) + tail); rows.append((i, len(refs) - 1))
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    pairs = pairs_ref.pairs_array(rows)
    cfg = _cfg(pkg, pm)
    for f in (15, 1):
        want = fr.records(prots, refs, pairs, BOTH, om, 11, 1, f)
        got = _align(pkg, cfg, Q, Rs, pairs, BOTH, f, 2 * S + 1, 301)
        _same(got, want)
        assert got[2] == "pmx_swfsc_kernel<16,%d>/strips" % R
    ends = want[0][:, 1]
    assert (ends >= 2 * S).any() and ((ends >= S) & (ends < 2 * S)).any() and (ends < S).any()
    # one strip alone takes the kernel without scratch, and the same records
    got = _align(pkg, cfg, Q, Rs, pairs[:12], BOTH, 1, S, 301, chunk=5)
    assert got[2] == "pmx_swfsc_kernel<16,%d>" % R and got[0].tobytes() == want[0][:12].tobytes()


def test_shift_on_a_lanes_and_a_strips_first_row(pkg, orc):
    """planted shifts whose frameshift step lands exactly on row i = k R^ (the D terms come from the H handed down by the lane above)
    and on row i = S^ (from the boundary scratch): deletions and insertions, scored with a cheap and a dear penalty"""
    pm, om = _b62(pkg, orc)
    R, S = _shape(pkg)
    rng = np.random.default_rng(17600)
    p = random_seqs(rng, 1, S + 3 * R, S + 3 * R, AA)[0]
    refs, rows, at = [], [], []
    for i in [k * R for k in range(2, 7)] + [S - R, S, S + R]:
        for kind in (0, 1):
            lo = i - 12
            refs.append(_dna(rng, int(rng.integers(0, 7))) + _gene(rng, p[lo:i + 12], [(i - 1 - lo, kind)]) + _dna(rng, 5))
            rows.append((0, len(refs) - 1)); at.append(i)
    Q, Rs = pkg.SeqSet.new([p]), pkg.SeqSet.new(refs)
    pairs = pairs_ref.pairs_array(rows)
    for f in (3, 15):
        want = fr.records([p], refs, pairs, FWD, om, 11, 1, f)
        plain = fr.records([p], refs, pairs, FWD, om, 11, 1, BIG)
        assert (want[0][:, 0] >= plain[0][:, 0] + 20).all()                         # the path crosses the shift: both halves count
        assert all(i + 8 <= int(e) <= i + 12 for e, i in zip(want[0][:, 1], at))    # and ends at the piece's end, beyond the shifted row
        got = _align(pkg, _cfg(pkg, pm), Q, Rs, pairs, FWD, f, len(p), 90)
        _same(got, want)
        assert got[2].endswith("/strips")


def test_equal_maxima_across_lanes_and_strips(pkg, orc):
    """low complexity: a poly-K query of 2 S^ + 7 letters against poly-A (every codon reads K) and against K-coding repeats that are
    shorter than the query, so the maximum is reached in many rows of many lanes of every strip: the first in column-major order"""
    pm, om = _b62(pkg, orc)
    R, S = _shape(pkg)
    prots = [b"K" * (2 * S + 7), b"K" * (S + 1), b"KR" * S, b"K" * 5]
    refs = [b"A" * 50, b"A" * 17, b"AAG" * 20 + b"C", b"AAAAGG" * 9, b"T" * 40, b"A" * 3]
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    pairs = pairs_ref.pairs_array([(i, j) for i in range(len(prots)) for j in range(len(refs))])
    for f in (0, 15):
        want = fr.records(prots, refs, pairs, BOTH, om, 11, 1, f)
        _same(_align(pkg, _cfg(pkg, pm), Q, Rs, pairs, BOTH, f, 2 * S + 7, 60), want)
    k = int(om.scores[om.mapper[ord("K")], om.mapper[ord("K")]])
    assert want[0][0].tolist() == [16 * k, 15, 47, 0] and want[1][0] == 0           # 48 columns: 16 in-frame matches, first reached in row 15


# ------------------------------------------------------------------------------------------------- 3. unequal slots in one wave
def test_unequal_slots_in_a_wave(pkg, orc):
    """(m, N) = (1, 1), (S^ + 1, 7), (5, 300), (R^, 3) in one launch of one wave: the trip counts are the wave's; then 4 k + 1 slots"""
    pm, om = _b62(pkg, orc)
    R, S = _shape(pkg)
    rng = np.random.default_rng(17700)
    prots = [random_seqs(rng, 1, m, m, AA)[0] for m in (1, S + 1, 5, R)]
    refs = [_gene(rng, prots[0]), _gene(rng, prots[1][S - 2:S + 1]), _noisy_gene(rng, prots[2], 302), _gene(rng, prots[3][:1])]
    refs[1] = (refs[1] + _dna(rng, 9))[:9]; refs[3] = (refs[3] + _dna(rng, 5))[:5]
    assert [len(r) - 2 for r in refs] == [1, 7, 300, 3]
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    cfg = _cfg(pkg, pm)
    four = pairs_ref.pairs_array([(i, i) for i in range(4)])
    want = fr.records(prots, refs, four, FWD, om, 11, 1, 15)
    assert (want[0][:, 0] > 0).all()
    _same(_align(pkg, cfg, Q, Rs, four, FWD, 15, S + 1, 300), want)
    many = pairs_ref.pairs_array([((3 * k) % 4, (5 * k + 1) % 4) for k in range(4 * 9 + 1)])
    want = fr.records(prots, refs, many, FWD, om, 11, 1, 15)
    _same(_align(pkg, cfg, Q, Rs, many, FWD, 15, S + 1, 300), want)
    want = fr.records(prots, refs, many, BOTH, om, 11, 1, 15)
    _same(_align(pkg, cfg, Q, Rs, many, BOTH, 15, S + 1, 300, chunk=5), want)


# --------------------------------------------------------------------------------------------------- 4. past the query side's cap
def test_references_past_the_query_sides_cap(pkg, orc):
    """W = 4 099 and W = 20 000 -- beyond PMX_FRAMESHIFT_MAX_WINDOW -- against m = 35 and m = S^ + 5, a frameshifted gene near the far
    end: the stream has no cap of its own"""
    pm, om = _b62(pkg, orc)
    R, S = _shape(pkg)
    rng = np.random.default_rng(17800)
    assert pkg.frameshift_max_window() < 4099
    prots = [random_seqs(rng, 1, m, m, AA)[0] for m in (35, S + 5)]
    refs = []
    for W in (4099, 20000):
        for p in prots:
            g = _gene(rng, p, [(len(p) // 2, 0), (len(p) - 9, 1)])
            refs.append(_dna(rng, W - len(g) - 40) + g + _dna(rng, 40))
    assert [len(r) for r in refs] == [4099, 4099, 20000, 20000]
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    cfg = _cfg(pkg, pm)
    short = pairs_ref.pairs_array([(0, 0), (0, 2)])
    want = fr.records(prots, refs, short, FWD, om, 11, 1, 15)
    got = _align(pkg, cfg, Q, Rs, short, FWD, 15, 35, 19998)
    _same(got, want)
    assert got[2] == "pmx_swfsc_kernel<16,%d>" % R and (want[0][:, 2] > [4000, 19900]).all() and (want[0][:, 0] > 120).all()
    long_ = pairs_ref.pairs_array([(1, 1), (1, 3), (0, 2), (1, 2, 10000, -1, 10000, -1)])                  # (the last: a bad window)
    want = fr.records(prots, refs, long_, FWD, om, 11, 1, 15)
    got = _align(pkg, cfg, Q, Rs, long_, FWD, 15, S + 5, 19998)
    _same(got, want)
    assert got[2].endswith("/strips") and want[0][1][0] > 600 and want[0][3].tolist() == BAD
    # the reverse strand of the long window, through the host entry, which sizes max_rlen itself
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    RC = pkg.SeqSet.new([revcomp(r) for r in refs])
    rec, won = al.align_pairs(Q, RC, long_[:2], ref_frameshift=15, ref_strand="both")
    assert won.tolist() == [1, 1] and rec.view(np.int32).reshape(-1, 4).tobytes() == want[0][:2].tobytes()


# ------------------------------------------------------------------------------------------------------- 5. an asymmetric matrix
def test_asymmetric_matrix(pkg, orc):
    """entries that differ above and below the diagonal: the records equal the model's, which pins s(query letter, reference letter)"""
    letters = "ARNDCQEGHILKMFPSTWYV"
    pm, om0 = pkg.Matrix.create(letters.encode(), 5, -4), orc.Matrix.create(letters, 5, -4)
    s = om0.scores.copy()
    rng = np.random.default_rng(17900)
    for _ in range(60):
        a, b = (int(x) for x in rng.integers(0, 20, 2))
        if a != b:
            v = int(rng.integers(-6, 5))
            s[a, b] = v; pm.set_value(a, b, v)
    assert (s != s.T).sum() > 60
    om, omT = orc.Matrix(s, om0.mapper, letters), orc.Matrix(np.ascontiguousarray(s.T), om0.mapper, letters)
    prots = random_seqs(rng, 12, 8, 60, AA)
    refs = [_noisy_gene(rng, prots[i % 12][int(rng.integers(0, 4)):], int(rng.integers(30, 200))) for i in range(24)]
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    pairs = pairs_ref.pairs_array([(i, j) for i in range(12) for j in range(24)])
    want = fr.records(prots, refs, pairs, BOTH, om, 7, 2, 6)
    _same(_align(pkg, _cfg(pkg, pm, 7, 2), Q, Rs, pairs, BOTH, 6, 60, 198), want)
    wrong = fr.records(prots, refs, pairs, BOTH, omT, 7, 2, 6)
    assert (want[0][:, 0] != wrong[0][:, 0]).sum() > 50                              # the transposed matrix would not pass


# ---------------------------------------------------------------------------------------------------------------- 6. the strands
def test_strands(pkg, orc):
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(18000)
    prots = random_seqs(rng, 10, 20, 50, AA)
    refs, where = [], []
    for i in range(30):
        p = prots[i % 10]
        g = _gene(rng, p[3:19], [(7, i % 2)])
        left = _dna(rng, int(rng.integers(0, 40)))
        s = left + g + _dna(rng, int(rng.integers(0, 40)))
        where.append((len(left), len(left) + len(g) - 1))                            # the gene's first and last stored byte
        if i % 3 == 1:
            s = revcomp(s); where[-1] = (len(s) - 1 - where[-1][1], len(s) - 1 - where[-1][0])
        refs.append(s)
    half = back_translate(rng, prots[0][2:14])
    pal = half + revcomp(half)                                                       # equals its reverse complement: the strands tie
    refs.append(pal)
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    Rrc = pkg.SeqSet.new([revcomp(s) for s in refs])
    rows = [(i, j) for i in range(len(prots)) for j in range(len(refs))]
    rows += [(2, 3, 1, -1, 5, 60), (1, 4, 0, 12, 2, -1), (0, 30, 0, -1, 3, 60)]      # windows: the reverse strand is the window's
    pairs = pairs_ref.pairs_array(rows)
    cfg = _cfg(pkg, pm)
    mq, mr = 50, 140
    fwd = _align(pkg, cfg, Q, Rs, pairs[:310], FWD, 15, mq, mr)
    rev = _align(pkg, cfg, Q, Rs, pairs[:310], REV, 15, mq, mr)
    fwd_rc = _align(pkg, cfg, Q, Rrc, pairs[:310], FWD, 15, mq, mr)
    assert rev[0].tobytes() == fwd_rc[0].tobytes() and (rev[1] == 1).all() and not fwd[1].any()
    for mode in (FWD, REV, BOTH):
        want = fr.records(prots, refs, pairs, mode, om, 11, 1, 15)
        for chunk in (0, 7, 1):
            _same(_align(pkg, cfg, Q, Rs, pairs, mode, 15, mq, mr, chunk), want)
    both = want
    assert 20 < int(both[1].sum()) < len(pairs) - 20                                # both strands win somewhere
    k = rows.index((0, 30))
    f1, r1 = fr.records(prots, refs, pairs[k:k + 1], FWD, om, 11, 1, 15), fr.records(prots, refs, pairs[k:k + 1], REV, om, 11, 1, 15)
    assert f1[0][0].tolist() == r1[0][0].tolist() and f1[0][0][0] > 40 and both[1][k] == 0       # the tie goes to forward
    # end_ref maps back to the planted stored bytes: where the path ends on the gene's last letter (query letter 18; chance may carry
    # it on into the flank), the last base of the gene's last codon, on the strand that carries it
    mapped = 0
    for j in range(30):
        rec, strand = both[0][(j % 10) * len(refs) + j], int(both[1][(j % 10) * len(refs) + j])
        assert strand == (1 if j % 3 == 1 else 0) and rec[0] > 40
        if rec[1] == 18:
            stored = rec[2] if strand == 0 else len(refs[j]) - 1 - rec[2]
            assert stored == (where[j][1] if strand == 0 else where[j][0])
            mapped += 1
    assert mapped >= 20
    # a strand byte per pair
    sb = rng.integers(0, 2, len(pairs)).astype(np.uint8)
    want = fr.records(prots, refs, pairs, FWD, om, 11, 1, 15, strands=sb)
    _same(_align(pkg, cfg, Q, Rs, pairs, FWD, 15, mq, mr, 7, strands=sb), want)
    assert want[1].tolist() == sb.tolist()


# ------------------------------------------------------------------------------------------------------------------ 7. bad pairs
def test_bad_pairs(pkg, orc):
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(18100)
    prots = random_seqs(rng, 4, 10, 30, AA) + [random_seqs(rng, 1, 31, 31, AA)[0]]
    refs = [_noisy_gene(rng, prots[0], 60), b"AT", b"A", b"ATG", _noisy_gene(rng, prots[1], 33), _noisy_gene(rng, prots[2], 63)]
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    rows = [(0, 0), (1, 4), (0, 1), (2, 3), (1, 2), (5, 0), (0, 6), (1, 0, 0, -1, 59, -1), (1, 0, 0, -1, 58, 2), (1, 0, 0, -1, 57, 3),
            (0, 4, 40, 2, 0, -1), (3, 4), (4, 0), (0, 5), (2, 0)]
    pairs = pairs_ref.pairs_array(rows)
    cfg = _cfg(pkg, pm)
    # W < 3: 2, 4, 7, 8; descriptors: 5, 6, 10; m = 31 > max_qlen: 12; N = 61 > max_rlen: 13
    bad_at = [2, 4, 5, 6, 7, 8, 10, 12, 13]
    for mode in (FWD, REV, BOTH):
        want = fr.records(prots, refs, pairs, mode, om, 11, 1, 15, max_qlen=30, max_rlen=60)
        assert [k for k in range(len(rows)) if want[0][k].tolist() == BAD] == bad_at and not want[1][bad_at].any()
        for chunk in (0, 1, 5):
            _same(_align(pkg, cfg, Q, Rs, pairs, mode, 15, 30, 60, chunk), want)
    sb = np.array([0, 1, 0, 2, 1, 0, 0, 1, 1, 255, 0, 1, 0, 1, 1], dtype=np.uint8)         # strand bytes outside {0, 1}: pairs 3 and 9
    want = fr.records(prots, refs, pairs, FWD, om, 11, 1, 15, strands=sb, max_qlen=30, max_rlen=60)
    assert [k for k in range(len(rows)) if want[0][k].tolist() == BAD] == sorted(bad_at + [3, 9])
    _same(_align(pkg, cfg, Q, Rs, pairs, FWD, 15, 30, 60, 5, strands=sb), want)
    # the host entries name the first bad pair
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    with pytest.raises(pkg.BatchError, match="pair 2: "):
        al.align_pairs(Q, Rs, pairs, ref_frameshift=15, ref_strand="both")
    with pytest.raises(pkg.BatchError, match="pair 3: strand byte 2"):
        al.align_pairs(Q, Rs, pairs[:4], ref_frameshift=15, ref_strand=sb[:4])
    with pytest.raises(pkg.BatchError, match="pair 1 "):                             # rectangle 5 x 6: protein 0 against reference 1 (W = 2)
        al.search_topk(Q, Rs, k=2, ref_frameshift=15, ref_strand="both")
    good = [0, 1, 3, 9, 11, 14]
    rec, won = al.align_pairs(Q, Rs, pairs[good], ref_frameshift=15, ref_strand="both")
    want = fr.records(prots, refs, pairs[good], BOTH, om, 11, 1, 15)
    assert rec.view(np.int32).reshape(-1, 4).tobytes() == want[0].tobytes() and won.tolist() == want[1].tolist()


# ------------------------------------------------------------------------------------------------------------- 8. the gather hook
def test_gather_codons_ref_at_the_sets_edges(pkg):
    """reference windows of 3, 4, 66, 67 and 1 000 nt -- one, and several, trips of the 16-lane loop over destination dwords -- that
    begin at a set's first byte and end at its last, both strands, over sets wrapped around exactly their bytes"""
    import torch
    rng = np.random.default_rng(18200)
    letters = np.frombuffer(b"ACGTACGTACGTacgtUuN-", dtype=np.uint8)
    rseqs = [letters[rng.integers(0, len(letters), size=l)].tobytes() for l in (1000, 2, 3, 4, 66, 67, 5, 9, 1, 1003)]
    qseqs = random_seqs(rng, 5, 1, 9, AA)
    rows, strands = [], []
    for j in range(len(rseqs)):
        for s in (0, 1):
            rows.append(((j + s) % 5, j)); strands.append(s)
    for j, b, l in ((0, 0, 3), (0, 0, 66), (0, 1, -1), (0, 997, 3), (9, 0, -1), (9, 1000, 3), (9, 936, -1), (9, 3, 1000), (9, 1, 67), (0, 0, 2),
                    (0, 0, 4), (9, 999, 4)):
        for s in (0, 1):
            rows.append((0, j, 0, -1, b, l)); strands.append(s)
    rows += [(0, 10), (5, 0), (0, 0)]; strands += [0, 1, 2]                                       # bad descriptors, a bad strand byte
    pairs = pairs_ref.pairs_array(rows)
    n = len(pairs)
    want = []
    for d, s in zip(pairs, strands):
        q = pairs_ref.resolve_side(qseqs, d["q"], d["q_beg"], d["q_len"], 9); r = pairs_ref.resolve_side(rseqs, d["r"], d["r_beg"], d["r_len"])
        want.append(None if q is None or r is None or len(r) < 3 or s > 1 else (q, pkg.codon_stream(r, s)))
        if want[-1]:
            assert want[-1][1] == fr.stream(r, s)
    assert sum(w is None for w in want) == 2 * 2 + 2 + 3 and any(w and b"X" in w[1] for w in want)
    assert {len(w[1]) + 2 for w in want if w} >= {3, 4, 66, 67, 1000}
    qwant = b"".join(w[0] if w else b"\0" for w in want); rwant = b"".join(w[1] if w else b"\0" for w in want)
    qoffw = np.concatenate([[0], np.cumsum([len(w[0]) if w else 1 for w in want])]); roffw = np.concatenate([[0], np.cumsum([len(w[1]) if w else 1 for w in want])])
    assert {int(o) % 4 for o, w in zip(roffw, want) if w} == {0, 1, 2, 3}
    qb, qo = pkg.pack(qseqs); rb, ro = pkg.pack(rseqs)
    keep = (_up(qb), _up(qo), _up(rb), _up(ro))
    WQ = pkg.SeqSet.wrap_device(keep[0].data_ptr(), keep[1].data_ptr(), len(qseqs), len(qb), keep=keep[:2])
    WR = pkg.SeqSet.wrap_device(keep[2].data_ptr(), keep[3].data_ptr(), len(rseqs), len(rb), keep=keep[2:])
    for SQ, SR in ((pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)), (WQ, WR)):
        qout = _full((len(qwant) + 32,), FILL, torch.uint8); rout = _full((len(rwant) + 32,), FILL, torch.uint8)
        qoff = _full((n + 3,), SENTINEL, torch.int64); roff = _full((n + 3,), SENTINEL, torch.int64)
        ok = _full((n + 2,), FILL, torch.uint8)
        d_pairs = _pairs_up(pairs); d_strand = _up(np.asarray(strands, dtype=np.uint8))
        pkg.gather_pairs_codons_ref_device(SQ, SR, n, d_pairs.data_ptr(), d_strand.data_ptr(), 9, 1001, qout.data_ptr() + 16, len(qwant), qoff.data_ptr(),
                                           rout.data_ptr() + 16, len(rwant), roff.data_ptr(), ok.data_ptr(), _stream())
        _sync()
        qout, qoff, rout, roff, ok = [t.cpu().numpy() for t in (qout, qoff, rout, roff, ok)]
        assert qoff[:n + 1].tolist() == qoffw.tolist() and roff[:n + 1].tolist() == roffw.tolist()
        assert ok[:n].tolist() == [1 if w else 0 for w in want] and (ok[n:] == FILL).all()
        assert qout[16:16 + len(qwant)].tobytes() == qwant and rout[16:16 + len(rwant)].tobytes() == rwant
        assert (qout[:16] == FILL).all() and (qout[16 + len(qwant):] == FILL).all()
        assert (rout[:16] == FILL).all() and (rout[16 + len(rwant):] == FILL).all()


# ------------------------------------------------------------------------------------------------------------ 9. search and top-K
NQ, NR = 6, 40


class Sets:
    pass


@pytest.fixture(scope="module")
def sets(pkg, orc):
    """6 proteins x 40 references with planted hits and the model's records of the rectangle per strand mode -- computed once, shared,
    left unchanged"""
    p = Sets()
    p.pm, p.om = _b62(pkg, orc)
    rng = np.random.default_rng(18300)
    p.prots = random_seqs(rng, NQ, 30, 70, AA)
    p.refs = []
    for j in range(NR):
        q = p.prots[(j * 5) % NQ]
        a = int(rng.integers(0, len(q) - 25))
        s = _dna(rng, int(rng.integers(0, 60))) + _noisy_gene(rng, q[a:], int(rng.integers(40, 150))) + _dna(rng, int(rng.integers(0, 60)))
        p.refs.append(revcomp(s) if j % 3 == 1 else s)
    p.Q, p.R = pkg.SeqSet.new(p.prots), pkg.SeqSet.new(p.refs)
    p.rect = set_search_ref.rect_pairs_descriptors(NR, 0, NQ * NR)
    p.model = {mode: fr.rect_records(p.prots, p.refs, mode, p.om, 11, 1, 15) for mode in (FWD, REV, BOTH)}
    p.al = pkg.Aligner.new().local().matrix(p.pm).gap_open(11).gap_extend(1).build()
    return p


def test_search_and_topk(pkg, sets):
    p = sets
    rec, won = p.model[BOTH]
    ms = int(np.sort(rec[:, :, 0].ravel())[-NR - 5])
    idx, recs, sb = fr.search(rec, won, ms)
    assert NR <= len(idx) <= NR + 12 and len(set(sb.tolist())) == 2
    runs = []
    for chunk in (0, 7, 64):
        h = p.al.search_pairs(p.Q, p.R, min_score=ms, ref_frameshift=15, ref_strand="both", chunk_pairs=chunk)
        assert h.n_hits == h.n_passing == len(idx) and h.index.tolist() == idx.tolist()
        assert h.records.view(np.int32).reshape(-1, 4).tobytes() == recs.tobytes() and h.strand.tolist() == sb.tolist()
        assert h.pairs.tobytes() == p.rect[idx].tobytes()
        runs.append(h)
    for mode, name in ((FWD, 0), (REV, 1)):
        i1, r1, s1 = fr.search(*p.model[mode], ms)
        h1 = p.al.search_pairs(p.Q, p.R, min_score=ms, ref_frameshift=15, ref_strand=name, chunk_pairs=7)
        assert h1.index.tolist() == i1.tolist() and h1.records.view(np.int32).reshape(-1, 4).tobytes() == r1.tobytes() and h1.strand.tolist() == s1.tolist()
    h9 = p.al.search_pairs(p.Q, p.R, min_score=ms, ref_frameshift=15, ref_strand="both", max_hits=9, slice_pairs=100)
    assert h9.n_hits == 9 and h9.n_passing == len(idx) and h9.index.tolist() == idx[:9].tolist()
    # the hit descriptors and strand bytes are valid input to the listed entry, and reproduce the hit records
    h = runs[0]
    rec2, won2 = p.al.align_pairs(p.Q, p.R, h.pairs, ref_frameshift=15, ref_strand=h.strand)
    assert rec2.tobytes() == h.records.tobytes() and won2.tolist() == h.strand.tolist()
    # top-K: (score descending, reference index ascending) per protein, K = 1, 3 and beyond the row's length
    for k, floor in ((1, ms), (3, 25), (NR + 10, 20)):
        off, refs, recs, sb = fr.topk(rec, won, k, floor)
        for chunk in (0, 7, 64):
            t = p.al.search_topk(p.Q, p.R, k=k, min_score=floor, ref_frameshift=15, ref_strand="both", chunk_pairs=chunk)
            assert t.row_off.tolist() == off.tolist()
            assert t.pairs["r"].tolist() == refs.tolist() and t.pairs["q"].tolist() == np.repeat(np.arange(NQ), np.diff(off)).tolist()
            assert t.records.view(np.int32).reshape(-1, 4).tobytes() == recs.tobytes() and t.strand.tolist() == sb.tolist()
        assert (np.diff(off) > 0).all()
    assert (np.diff(off) > 3).all() and len(set(sb.tolist())) == 2
    rec2, won2 = p.al.align_pairs(p.Q, p.R, t.pairs, ref_frameshift=15, ref_strand=t.strand)
    assert rec2.tobytes() == t.records.tobytes() and won2.tolist() == t.strand.tolist()


def test_search_device_entry(pkg, sets):
    """pmx_search_pairs_frameshift_ref_device over a window of the rectangle: hits, order, counts and strand bytes, and a capacity
    below the passing count"""
    import torch
    p = sets
    rec, won = p.model[BOTH]
    first, n = 7, NQ * NR - 19
    flat, fwon = rec.reshape(-1, 4)[first:first + n], won.ravel()[first:first + n]
    ms = int(np.sort(flat[:, 0])[-30])
    hit = np.nonzero(flat[:, 0] >= ms)[0]
    cfg = _cfg(pkg, p.pm)
    opts = pkg.pmx_pairs_opts_t(7)
    import ctypes as C
    for cap in (n, 5):
        slots = cap + 3
        hp = _full((slots * 32,), FILL, torch.uint8); hi = _full((slots,), SENTINEL, torch.int64)
        hr = _full((slots, 4), SENTINEL, torch.int32); hb = _full((slots,), FILL, torch.uint8)
        cnt = _full((2,), SENTINEL, torch.int64)
        rc = pkg.lib.pmx_search_pairs_frameshift_ref_device(C.byref(cfg), p.Q._handle(), p.R._handle(), RECT, first, n, None, 70, 270, ms,
                                                            hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), None, cap, cnt.data_ptr(), _stream(),
                                                            C.byref(opts), BOTH, hb.data_ptr(), 15, None)
        assert rc == 0, pkg.lib.pmx_last_error()
        _sync()
        w = min(len(hit), cap)
        assert cnt.cpu().tolist() == [len(hit), w]
        assert hi.cpu().numpy()[:w].tolist() == (hit[:w] + first).tolist() and (hi.cpu().numpy()[w:] == SENTINEL).all()
        assert hr.cpu().numpy()[:w].tobytes() == flat[hit[:w]].tobytes() and (hr.cpu().numpy()[w:] == SENTINEL).all()
        assert hb.cpu().numpy()[:w].tolist() == fwon[hit[:w]].tolist() and (hb.cpu().numpy()[w:] == FILL).all()
        assert hp.cpu().numpy().view(pairs_ref.PAIR_DTYPE)[:w].tobytes() == p.rect[first:first + n][hit[:w]].tobytes()


# ------------------------------------------------------------------------------------------ 10. a planted frameshift, end to end
def test_planted_frameshift_end_to_end(pkg, orc):
    """64 proteins x 64 references, reference j carrying a back-translated piece of 30 - 50 letters of protein j with one base deleted
    somewhere inside (every third one reverse-complemented).  At the lowest score the model gives a planted pair, the new search returns all
    64; search_pairs(ref_frame="all") at the same threshold returns what the six-frame model predicts -- fewer."""
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(18400)
    n = 64
    prots = random_seqs(rng, n, 50, 70, AA)
    refs = []
    for j, q in enumerate(prots):
        L = int(rng.integers(30, 51)); a = int(rng.integers(0, len(q) - L + 1)); d = int(rng.integers(12, 3 * L - 12))
        g = back_translate(rng, q[a:a + L])
        s = _dna(rng, int(rng.integers(5, 40))) + g[:d] + g[d + 1:] + _dna(rng, int(rng.integers(5, 40)))
        refs.append(revcomp(s) if j % 3 == 2 else s)
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    rec, won = fr.rect_records(prots, refs, BOTH, om, 11, 1, 15)
    ms = int(min(rec[j, j, 0] for j in range(n)))
    idx, recs, sb = fr.search(rec, won, ms)
    assert {j * n + j for j in range(n)} <= set(idx.tolist()) and len(idx) < n + 8 and ms > 100
    h = al.search_pairs(Q, Rs, min_score=ms, ref_frameshift=15, ref_strand="both")
    assert h.index.tolist() == idx.tolist() and h.records.view(np.int32).reshape(-1, 4).tobytes() == recs.tobytes() and h.strand.tolist() == sb.tolist()
    assert [int(s) for s in won.diagonal()] == [1 if j % 3 == 2 else 0 for j in range(n)]
    # the road without frameshifts: the oracle's plain local score of every protein against the six host-translated frames
    six = np.zeros((n, n), dtype=np.int64)
    for j, r in enumerate(refs):
        frames = [f for f in (translate_ref.translate(r, k) for k in range(6)) if f]
        for i, q in enumerate(prots):
            qb, qo = orc.pack([q] * len(frames)); rb, ro = orc.pack(frames)
            six[i, j] = int(orc.align_batch(orc.SW, qb, qo, rb, ro, 11, 1, om)[:, 0].max())
    expect = [i * n + j for i in range(n) for j in range(n) if six[i, j] >= ms]
    plain = al.search_pairs(Q, Rs, min_score=ms, ref_frame="all")
    assert plain.index.tolist() == expect and plain.records["score"].tolist() == [int(six[p // n, p % n]) for p in expect]
    assert 0 < len(expect) < n - 16 and all(p // n == p % n for p in expect)          # the shorter halves fall under the threshold
