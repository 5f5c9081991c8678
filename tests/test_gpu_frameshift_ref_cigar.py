"""The reference-side frameshift traceback entries (`-m gpu`): the trace form of pmx_swfsc_kernel and pmx_walkfs_kernel<true> behind
pmx_align_pairs_frameshift_ref_cigar[_device], against the CPU model tests/swfsc_trace_model.c (tests/frameshift_trace_ref_side.py).
Records, strand bytes, text, offsets, begins and statistics are compared byte for byte, for every pair of every batch; every output
buffer starts as a sentinel and is checked beyond n."""
import numpy as np
import pytest

import frameshift_ref_side as fr
import frameshift_trace_ref_side as ft
import pairs_ref
from pairs_ex_ref import revcomp
from test_gpu_translate import _up, _full, _stream, _sync, _ptr, _pairs_up, back_translate, SENTINEL, FILL
from test_gpu_frameshift_ref import _b62, _dna, _gene, _noisy_gene, _align
from util import random_seqs, AA

pytestmark = pytest.mark.gpu

FWD, REV, BOTH = 0, 1, 2
G, R = 16, 10                   # the shipped instantiation: a strip is G * R query letters, a lane's rows change every R
S = G * R
BAD = ft.BAD
SCORE = "pmx_swfsc_kernel<16,10>"
TRACE = "pmx_swfsc_kernel<16,10,trace>"
SLACK = 32                      # text bytes behind the capacity, to stay sentinel


def _cfg(pkg, pm, open_=11, ext=1, stats=True):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, open_, ext, 0, pkg.WANT_CIGAR | (pkg.WANT_STATS if stats else 0), pm.inner)


class Got:
    pass


def _run(pkg, cfg, Q, Rs, pairs, mode, f, mq, mr, capacity, chunk=0, strands=None, stats=True, beg=True):
    """pmx_align_pairs_frameshift_ref_cigar_device -> every output as it lies in its buffer, sentinels beyond n checked"""
    import torch
    n = len(pairs)
    rec = _full((n + 2, 4), SENTINEL, torch.int32); won = _full((n + 2,), FILL, torch.uint8)
    st = _full((n + 2, 3), SENTINEL, torch.int32) if stats else None
    bg = _full((n + 2, 2), SENTINEL, torch.int32) if beg else None
    text = _full((capacity + SLACK,), FILL, torch.uint8); off = _full((n + 3,), SENTINEL, torch.int64)
    d_pairs = _pairs_up(pairs)
    d_strand = _up(np.asarray(strands, dtype=np.uint8)) if strands is not None else None
    pkg.align_pairs_frameshift_ref_cigar_device(cfg, Q, Rs, n, d_pairs.data_ptr(), _ptr(d_strand), mode, f, mq, mr, rec.data_ptr(), won.data_ptr(),
                                                _ptr(st), _ptr(bg), text.data_ptr(), capacity, off.data_ptr(), _stream(), chunk)
    g = Got()
    g.kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    g.rec, g.won, g.text, g.off = rec.cpu().numpy(), won.cpu().numpy(), text.cpu().numpy(), off.cpu().numpy()
    g.stats = st.cpu().numpy() if stats else None
    g.beg = bg.cpu().numpy() if beg else None
    assert (g.rec[n:] == SENTINEL).all() and (g.won[n:] == FILL).all() and (g.off[n + 1:] == SENTINEL).all()
    assert not stats or (g.stats[n:] == SENTINEL).all()
    assert not beg or (g.beg[n:] == SENTINEL).all()
    assert (g.text[capacity:] == FILL).all()
    return g


def _same(g, want, capacity=None):
    """every pair of the batch, byte for byte; capacity: the texts that fit are written, the bytes beyond stay sentinel"""
    n = len(want.texts)
    assert g.won[:n].tolist() == want.strand.tolist()
    bad = np.nonzero((g.rec[:n] != want.records).any(axis=1))[0]
    assert g.rec[:n].tobytes() == want.records.tobytes(), (bad[:5], g.rec[bad[:5]], want.records[bad[:5]])
    assert g.off[:n + 1].tolist() == want.off.tolist()
    if g.beg is not None:
        assert g.beg[:n].tobytes() == want.beg.tobytes()
    if g.stats is not None:
        assert g.stats[:n].tobytes() == want.stats.tobytes()
    total = int(want.off[n])
    if capacity is None or capacity >= total:
        assert g.text[:total].tobytes() == want.text_bytes() and (g.text[total:] == FILL).all()
        return
    fits = int((want.off[1:] <= capacity).sum())          # offsets ascend: the pairs whose text ends inside the capacity
    end = int(want.off[fits])
    assert g.text[:end].tobytes() == want.text_bytes()[:end] and (g.text[end:] == FILL).all()


def _bytes_equal(a, b):
    for name in ("rec", "won", "text", "off", "stats", "beg"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name


class Batch:
    pass


# ------------------------------------------------------------------------------------------------------- 1. column-history edges
def _lattice_batch(pkg, orc):
    """every N = 1 .. 30 against m in {1, 2, 3, R - 1, R, R + 1, 2 R}, as test_gpu_frameshift_ref.test_column_history_edges builds it;
    the model's results for three gap models x three penalties, both strands -- computed once, shared, left unchanged"""
    p = Batch()
    p.pm, p.om = _b62(pkg, orc)
    rng = np.random.default_rng(19400)
    ms = [1, 2, 3, R - 1, R, R + 1, 2 * R]
    p.prots = [q for m in ms for q in random_seqs(rng, 2, m, m, AA)]
    p.refs = []
    for W in range(3, 33):
        for rep in range(3):
            q = p.prots[int(rng.integers(0, len(p.prots)))]
            g = _gene(rng, q, [(int(rng.integers(0, len(q))), rep % 2)] if rep else ())
            p.refs.append((_dna(rng, rep) + g + _dna(rng, 32))[:W])
    assert sorted({len(s) - 2 for s in p.refs}) == list(range(1, 31))
    p.Q, p.R = pkg.SeqSet.new(p.prots), pkg.SeqSet.new(p.refs)
    p.pairs = pairs_ref.pairs_array([(i, j) for i in range(len(p.prots)) for j in range(len(p.refs))])
    p.cases = [(o, e, f) for o, e in ((11, 1), (2, 1), (1, 1)) for f in (0, 1, 15)]
    p.want = {c: ft.results(p.prots, p.refs, p.pairs, BOTH, p.om, c[0], c[1], c[2]) for c in p.cases}
    return p


@pytest.fixture(scope="module")
def lattice(pkg, orc):
    return _lattice_batch(pkg, orc)


def test_column_history_edges(pkg, lattice):
    """the columns where j - 2 .. j - 4 do not exist, every residue of the ring and unroll period; cheap, equal penalties make ties,
    which is where the precedence shows"""
    p = lattice
    nonempty = 0
    seen = {"m": 0, ft.QUERY_GAP: 0, ft.CODON_GAP: 0, ft.SHORT: 0, ft.LONG: 0}
    for case in p.cases:
        want = p.want[case]
        total = int(want.off[-1])
        g = _run(pkg, _cfg(pkg, p.pm, case[0], case[1]), p.Q, p.R, p.pairs, BOTH, case[2], 2 * R, 30, total)
        _same(g, want)
        assert g.kernel == TRACE
        nonempty += sum(1 for t in want.texts if t)
        for t in want.texts:
            for key, v in ft.counts(t).items():
                seen[key] += v
    assert nonempty > 4000 and all(v > 0 for v in seen.values()), (nonempty, seen)
    assert set(np.concatenate([w.strand for w in p.want.values()]).tolist()) == {0, 1}


# --------------------------------------------------------------------------------------------------------- 2. lane and strip seams
BOUNDARIES = (4 * R, S, 2 * S)          # a lane boundary inside the first strip, and the two strip seams
EVENTS = ("plain", "base deleted", "base inserted", "query letter inserted", "two codons inserted")
ONE_STRIP = 24                          # the batch's first pairs: queries of at most one strip


def _planted_ref(rng, p, row, kind):
    """a reference that codes for the 12 letters before and the 12 from `row` of p, with one event whose step lands on `row`"""
    lo, hi = row - 12, row + 12
    if kind == "plain":
        g = _gene(rng, p[lo:hi])
    elif kind == "base deleted":
        g = _gene(rng, p[lo:hi], [(row - 1 - lo, 0)])
    elif kind == "base inserted":
        g = _gene(rng, p[lo:hi], [(row - 1 - lo, 1)])
    elif kind == "query letter inserted":                       # the reference has no codon for letter `row`
        g = _gene(rng, p[lo:row]) + _gene(rng, p[row + 1:hi])
    else:                                                       # two codons the query does not have, behind letter `row`
        g = _gene(rng, p[lo:row + 1]) + _dna(rng, 6) + _gene(rng, p[row + 1:hi])
    return _dna(rng, int(rng.integers(0, 7))) + g + _dna(rng, 5)


def _seams_batch(pkg, orc):
    """queries of S - 1, S, S + 1, 2 S and 2 S + 1 letters against references that code for their last 2, 28 and 44 letters, the longer ones
    with one single-base deletion or insertion, and two queries of 2 S + 15 letters -- a step INTO row 2 S that is a query gap needs rows
    behind it -- against references with one planted event whose step lands on rows b - 2 .. b + 2 of every boundary b; the model's
    results with gaps 11 / 1, fs 15, both strands -- computed once, shared, left unchanged.  The first ONE_STRIP pairs have queries of
    at most one strip."""
    p = Batch()
    p.pm, p.om = _b62(pkg, orc)
    rng = np.random.default_rng(19500)
    ms = [S - 1, S, S + 1, 2 * S, 2 * S + 1]
    p.prots = [random_seqs(rng, 1, m, m, AA)[0] for m in ms] + random_seqs(rng, 2, 2 * S + 15, 2 * S + 15, AA)
    p.refs, rows = [], []

    def add(i, ref):
        p.refs.append(ref if len(rows) % 3 else revcomp(ref))          # every third reference carries its gene on the reverse strand
        rows.append((i, len(p.refs) - 1))

    for rep in range(ONE_STRIP // 2):                                   # one strip: m = S - 1 and m = S
        for i in (0, 1):
            q = p.prots[i]
            add(i, _noisy_gene(rng, q[len(q) - 30 - rep:], 92) if rep % 2 else _planted_ref(rng, q, BOUNDARIES[0] + rep - 4, EVENTS[rep // 2 % 5]))
    assert len(rows) == ONE_STRIP
    for i in (2, 3, 4):
        q = p.prots[i]
        for k in (2, 28, 44):                                           # the alignment's last rows are the query's last k
            g = _gene(rng, q[len(q) - k:], [(k // 2, k % 8 == 4)] if k > 2 else ())
            add(i, _dna(rng, int(rng.integers(0, 9))) + g + _dna(rng, 3))
    for i in (5, 6):
        for b in BOUNDARIES:
            for kind in EVENTS:
                for d in range(-2, 3):
                    add(i, _planted_ref(rng, p.prots[i], b + d, kind))
    p.Q, p.R = pkg.SeqSet.new(p.prots), pkg.SeqSet.new(p.refs)
    p.pairs = pairs_ref.pairs_array(rows)
    p.mq = 2 * S + 15
    p.mr = max(len(s) for s in p.refs) - 2
    p.want = ft.results(p.prots, p.refs, p.pairs, BOTH, p.om, 11, 1, 15)
    p.capacity = int(p.want.off[-1])
    return p


@pytest.fixture(scope="module")
def seams(pkg, orc):
    return _seams_batch(pkg, orc)


def test_lane_and_strip_seams(pkg, seams):
    p = seams
    # from the model's paths, not from the construction: every row-crossing step kind lands on the first row behind every boundary
    # (source row b - 1, row b), and a codon-gap run of at least two lies in a lane's and in a strip's first row
    crossing = {(b, how): 0 for b in BOUNDARIES for how in ("3", ft.SHORT, ft.LONG, ft.QUERY_GAP)}
    runs_in_lane_first = runs_in_strip_first = 0
    for text, beg in zip(p.want.texts, p.want.beg):
        st = ft.steps(text, beg.tolist())
        for op, src, row, col, how in st:
            if src is not None and (row, how) in crossing and src == row - 1:
                crossing[(row, how)] += 1
        for a, b in zip(st, st[1:]):
            if a[4] == ft.CODON_GAP and b[4] == ft.CODON_GAP and a[2] == b[2]:
                runs_in_lane_first += a[2] % R == 0 and a[2] % S != 0
                runs_in_strip_first += a[2] % S == 0 and a[2] > 0
    assert all(v > 0 for v in crossing.values()), crossing
    assert runs_in_lane_first > 0 and runs_in_strip_first > 0
    assert set(p.want.strand.tolist()) == {0, 1}
    ends = p.want.records[:, 1]
    assert {int(e) for e in ends} >= {S - 2, S - 1, S, 2 * S - 1, 2 * S}          # the last letters of the five queries
    g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, p.mr, p.capacity)
    _same(g, p.want)
    assert g.kernel == TRACE + "/strips"
    p.got = g                                                  # (the unswitched run, for test_parts)


def test_one_strip_without_scratch(pkg, seams):
    """the first pairs alone: one strip, no boundary scratch, chunks of seven -- the bytes of the long batch's prefix"""
    p = seams
    n = ONE_STRIP
    want = ft.results(p.prots, p.refs, p.pairs[:n], BOTH, p.om, 11, 1, 15)
    assert want.records.tobytes() == p.want.records[:n].tobytes() and want.texts == p.want.texts[:n] and sum(1 for t in want.texts if t) == n
    g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs[:n], BOTH, 15, S, p.mr, int(want.off[-1]), chunk=7)
    _same(g, want)
    assert g.kernel == TRACE


def test_parts(pkg, seams, monkeypatch):
    """a bound on the trace scratch that cuts the batch into at least three parts changes no byte"""
    p = seams
    base = getattr(p, "got", None) or _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, p.mr, p.capacity)
    per_slot = -(-p.mq // S) * (p.mr + G - 1) * 192            # strips x steps x 192 bytes
    assert per_slot == pkg.lib.pmx_swfsc_trace_bytes_per_slot(p.mq, p.mr)
    slots = 2 * len(p.pairs)
    bound = per_slot * 102                                     # (not a multiple of four slots: a part is whole workgroups)
    assert -(-slots // (bound // per_slot // 4 * 4)) >= 3 and len(p.pairs) > 97
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(bound))
    g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, p.mr, p.capacity)
    monkeypatch.undo()
    _bytes_equal(g, base)
    _same(g, p.want)
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(bound))
    g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, p.mr, p.capacity, chunk=97)      # parts inside chunks
    monkeypatch.undo()
    _bytes_equal(g, base)
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(4 * per_slot))                                   # exactly one workgroup per part
    g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs[:9], BOTH, 15, p.mq, p.mr, p.capacity)
    monkeypatch.undo()
    assert g.rec[:9].tobytes() == base.rec[:9].tobytes() and g.text[:int(g.off[9])].tobytes() == base.text[:int(base.off[9])].tobytes()
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(4 * per_slot - 1))
    with pytest.raises(pkg.BatchError, match="PMX_CIGAR_CHUNK_BYTES"):
        _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, p.mr, p.capacity)


def test_text_capacity(pkg, seams):
    """a capacity below the need: the offsets still give the full need, the texts that fit are written, the rest stays sentinel"""
    p = seams
    total = p.capacity
    for cap in (total - 1, total // 2):
        g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, p.mr, cap, chunk=101)
        _same(g, p.want, capacity=cap)
        assert int(g.off[len(p.pairs)]) == total


# ------------------------------------------------------------------------------------------------- 3. unequal slots in one wave
def test_unequal_slots_in_a_wave(pkg, orc):
    """(m, N) = (1, 1), (S + 1, 7), (5, 300), (R, 3) in one launch of one wave: the trip counts are the wave's, the trace's steps are
    the slot's own (the skew padding), and the slot with N = max_rlen is followed by another (the slot stride); then 4 k + 1 slots"""
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(19600)
    prots = [random_seqs(rng, 1, m, m, AA)[0] for m in (1, S + 1, 5, R)]
    refs = [_gene(rng, prots[0]), _gene(rng, prots[1][S - 2:S + 1]), _noisy_gene(rng, prots[2], 302), _gene(rng, prots[3][:1])]
    refs[1] = (refs[1] + _dna(rng, 9))[:9]; refs[3] = (refs[3] + _dna(rng, 5))[:5]
    assert [len(r) - 2 for r in refs] == [1, 7, 300, 3]
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    cfg = _cfg(pkg, pm)
    four = pairs_ref.pairs_array([(i, i) for i in range(4)])
    want = ft.results(prots, refs, four, FWD, om, 11, 1, 15)
    assert (want.records[:, 0] > 0).all() and all(want.texts)
    g = _run(pkg, cfg, Q, Rs, four, FWD, 15, S + 1, 300, int(want.off[-1]))
    _same(g, want)
    assert g.kernel == TRACE + "/strips"
    many = pairs_ref.pairs_array([((3 * k) % 4, (5 * k + 1) % 4) for k in range(4 * 9 + 1)])
    want = ft.results(prots, refs, many, FWD, om, 11, 1, 15)
    _same(_run(pkg, cfg, Q, Rs, many, FWD, 15, S + 1, 300, int(want.off[-1])), want)
    want = ft.results(prots, refs, many, BOTH, om, 11, 1, 15)
    _same(_run(pkg, cfg, Q, Rs, many, BOTH, 15, S + 1, 300, int(want.off[-1]), chunk=5), want)
    # the longest stream last in its workgroup and first in the next
    edge = pairs_ref.pairs_array([(0, 0), (3, 3), (1, 1), (2, 2), (2, 2), (3, 3)])
    want = ft.results(prots, refs, edge, FWD, om, 11, 1, 15)
    _same(_run(pkg, cfg, Q, Rs, edge, FWD, 15, S + 1, 300, int(want.off[-1])), want)


# ------------------------------------------------------------------------------------------------------ 4. strands and bad pairs
def test_strands_and_bad_pairs(pkg, orc):
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(19700)
    prots = random_seqs(rng, 4, 10, 30, AA) + [random_seqs(rng, 1, 31, 31, AA)[0], b"WWWW"]
    refs = [_noisy_gene(rng, prots[0], 60), b"AT", b"A", b"ATG", _noisy_gene(rng, prots[1], 33), _noisy_gene(rng, prots[2], 63),
            revcomp(_noisy_gene(rng, prots[3], 57)), revcomp(_noisy_gene(rng, prots[1], 48)), b"TGA"]
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    rows = [(0, 0), (1, 4), (0, 1), (2, 3), (1, 2), (6, 0), (0, 9), (1, 0, 0, -1, 59, -1), (1, 0, 0, -1, 58, 2), (1, 0, 0, -1, 57, 3),
            (0, 4, 40, 2, 0, -1), (3, 4), (4, 0), (0, 5), (2, 0), (3, 6), (1, 7), (2, 6, 2, 5, 3, 50), (5, 8), (1, 0)]
    pairs = pairs_ref.pairs_array(rows)
    cfg = _cfg(pkg, pm)
    # W < 3: 2, 4, 7, 8; descriptors: 5, 6, 10; m = 31 > max_qlen: 12; N = 61 > max_rlen: 13
    bad_at = [2, 4, 5, 6, 7, 8, 10, 12, 13]
    both = None
    for mode in (FWD, REV, BOTH):
        want = ft.results(prots, refs, pairs, mode, om, 11, 1, 15, max_qlen=30, max_rlen=60)
        assert [k for k in range(len(rows)) if want.records[k].tolist() == BAD] == bad_at
        for k in bad_at:
            assert want.texts[k] == "" and want.beg[k].tolist() == [-1, -1] and want.stats[k].tolist() == [0, 0, 0] and want.strand[k] == 0
        for chunk in (0, 1, 5):
            _same(_run(pkg, cfg, Q, Rs, pairs, mode, 15, 30, 60, int(want.off[-1]), chunk), want)
        both = want if mode == BOTH else both
    assert set(both.strand.tolist()) == {0, 1}
    # a stop codon (its reverse strand reads S) against WWWW scores nothing: the empty path
    k = rows.index((5, 8))
    assert both.records[k].tolist() == [0, 0, 2, 0] and both.texts[k] == "" and both.beg[k].tolist() == [1, 3]
    # a strand byte per pair; bytes outside {0, 1} make pairs 3 and 9 bad
    sb = rng.integers(0, 2, len(rows)).astype(np.uint8)
    sb[3], sb[9] = 2, 255
    want = ft.results(prots, refs, pairs, FWD, om, 11, 1, 15, strands=sb, max_qlen=30, max_rlen=60)
    assert [k for k in range(len(rows)) if want.records[k].tolist() == BAD] == sorted(bad_at + [3, 9])
    _same(_run(pkg, cfg, Q, Rs, pairs, FWD, 15, 30, 60, int(want.off[-1]), 5, strands=sb), want)
    # optional outputs left out change nothing else
    g = _run(pkg, _cfg(pkg, pm, stats=False), Q, Rs, pairs, BOTH, 15, 30, 60, int(both.off[-1]), stats=False, beg=False)
    _same(g, both)
    # the host entry: the same through Aligner (it sizes the maxima itself), bad pairs refused by name
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    good = [k for k in range(len(rows)) if k not in (2, 4, 5, 6, 7, 8, 10)]
    want = ft.results(prots, refs, pairs[good], BOTH, om, 11, 1, 15)
    rec, cig, beg, won, st = al.align_pairs_frameshift_ref_cigar(Q, Rs, pairs[good], 15, ref_strand="both", stats=True, chunk_pairs=3)
    assert rec.view(np.int32).reshape(-1, 4).tobytes() == want.records.tobytes() and cig == want.texts and beg.tobytes() == want.beg.tobytes()
    assert won.tolist() == want.strand.tolist() and st.view(np.int32).reshape(-1, 3).tobytes() == want.stats.tobytes()
    rec2, cig2, beg2, won2 = al.align_pairs_frameshift_ref_cigar(Q, Rs, pairs[good], 15, ref_strand=won)
    assert rec2.tobytes() == rec.tobytes() and cig2 == cig and beg2.tobytes() == beg.tobytes() and won2.tolist() == won.tolist()
    with pytest.raises(pkg.BatchError, match="pair 2: "):
        al.align_pairs_frameshift_ref_cigar(Q, Rs, pairs, 15, ref_strand="both")


# ------------------------------------------------------------------------------------------------------- 5. an asymmetric matrix
def test_asymmetric_matrix(pkg, orc):
    """entries that differ above and below the diagonal: `similar` and '=' / 'X' pin s(query letter, stream letter)"""
    letters = "ARNDCQEGHILKMFPSTWYV"
    pm, om0 = pkg.Matrix.create(letters.encode(), 5, -4), orc.Matrix.create(letters, 5, -4)
    s = om0.scores.copy()
    rng = np.random.default_rng(19800)
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
    want = ft.results(prots, refs, pairs, BOTH, om, 7, 2, 6)
    _same(_run(pkg, _cfg(pkg, pm, 7, 2), Q, Rs, pairs, BOTH, 6, 60, 198, int(want.off[-1])), want)
    wrong = ft.results(prots, refs, pairs, BOTH, omT, 7, 2, 6)
    assert (want.records[:, 0] != wrong.records[:, 0]).sum() > 50                    # the transposed matrix would not pass
    assert (want.stats[:, 1] != wrong.stats[:, 1]).sum() > 50 and sum(a != b for a, b in zip(want.texts, wrong.texts)) > 50


# --------------------------------------------------------------------------------------------------- 6. past the query side's cap
def test_references_past_the_query_sides_cap(pkg, orc):
    """W = 4 099 and W = 20 000 -- beyond PMX_FRAMESHIFT_MAX_WINDOW -- against m = 35 and m = S + 5, a frameshifted gene near the far
    end: the text holds the '/' and the begins lie near the far end"""
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(19900)
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
    want = ft.results(prots, refs, short, FWD, om, 11, 1, 15)
    g = _run(pkg, cfg, Q, Rs, short, FWD, 15, 35, 19998, int(want.off[-1]))
    _same(g, want)
    assert g.kernel == TRACE and (want.beg[:, 1] > [3900, 19800]).all() and (want.records[:, 0] > 120).all()
    assert all(t.count("/") == 1 and t.count("\\") == 1 for t in want.texts)
    long_ = pairs_ref.pairs_array([(1, 1), (1, 3), (0, 2), (1, 2, 10000, -1, 10000, -1)])                  # (the last: a bad window)
    want = ft.results(prots, refs, long_, FWD, om, 11, 1, 15)
    g = _run(pkg, cfg, Q, Rs, long_, FWD, 15, S + 5, 19998, int(want.off[-1]), chunk=3)
    _same(g, want)
    assert g.kernel == TRACE + "/strips" and want.records[1][0] > 600 and want.records[3].tolist() == BAD
    assert all(t.count("/") == 1 for t in want.texts[:3]) and want.beg[1][1] > 19000


# ------------------------------------------------------------------------------------------------------- 7. search round trip
def test_search_round_trip(pkg, orc):
    """12 proteins x 36 references, every third reference a gene with one planted single-base deletion or insertion, on either strand:
    the search's hit pairs and strand bytes, as they are, give the hits' records back, and every planted deletion's text holds
    exactly one '/'"""
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(20000)
    prots = random_seqs(rng, 12, 40, 60, AA)
    refs, planted = [], {}
    for j in range(36):
        if j % 3:
            refs.append(_dna(rng, int(rng.integers(60, 161))))
            continue
        i = (j // 3) % 12
        kind = (j // 3) % 2
        g = _gene(rng, prots[i][3:35], [(15, kind)])
        s = _dna(rng, int(rng.integers(0, 30))) + g + _dna(rng, int(rng.integers(0, 30)))
        refs.append(revcomp(s) if j % 2 else s)
        planted[j] = (i, ft.LONG if kind else ft.SHORT)
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    h = al.search_pairs(Q, Rs, min_score=60, ref_frameshift=15, ref_strand="both")
    hits = len(h.pairs)
    assert 12 <= hits < 40 and set(h.strand.tolist()) == {0, 1}
    index = {(int(d["q"]), int(d["r"])): k for k, d in enumerate(h.pairs)}
    assert set(index) >= {(i, j) for j, (i, _) in planted.items()}
    want = ft.results(prots, refs, h.pairs, FWD, om, 11, 1, 15, strands=h.strand)
    rec, cig, beg, won, st = al.align_pairs_frameshift_ref_cigar(Q, Rs, h.pairs, 15, ref_strand=h.strand, stats=True)
    assert rec.tobytes() == h.records.tobytes() == want.records.tobytes() and won.tolist() == h.strand.tolist()
    assert cig == want.texts and beg.tobytes() == want.beg.tobytes() and st.view(np.int32).reshape(-1, 3).tobytes() == want.stats.tobytes()
    deletions = 0
    for j, (i, op) in planted.items():
        t = cig[index[(i, j)]]
        assert t.count(op) == 1, (i, j, t)
        deletions += op == ft.SHORT
    assert deletions >= 5
    # and as they lie on the device: the descriptors and strand bytes uploaded, every output in a sentinel buffer
    g = _run(pkg, _cfg(pkg, pm), Q, Rs, h.pairs, FWD, 15, 60, 218, int(want.off[-1]), strands=h.strand)
    _same(g, want)


# ----------------------------------------------------------------------------------------------------- 8. score kernel untouched
def test_score_kernel_untouched(pkg, lattice):
    """the score-only entry on the lattice: the records and strand bytes of the score model, and the kernel name it had"""
    p = lattice
    for case in p.cases:
        cfg0 = pkg.pmx_config_t(pkg.MODE_SW, 0, case[0], case[1], 0, 0, p.pm.inner)
        rec, won, kernel = _align(pkg, cfg0, p.Q, p.R, p.pairs, BOTH, case[2], 2 * R, 30)
        want = fr.records(p.prots, p.refs, p.pairs, BOTH, p.om, case[0], case[1], case[2])
        assert rec.tobytes() == want[0].tobytes() == p.want[case].records.tobytes() and won.tolist() == want[1].tolist()
        assert kernel == SCORE
