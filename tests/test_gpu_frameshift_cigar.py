"""The frameshift traceback entries (`-m gpu`): the trace form of pmx_swfs_kernel and pmx_walkfs_kernel behind
pmx_align_pairs_frameshift_cigar[_device], against the CPU model tests/swfs_trace_model.c (tests/frameshift_trace_ref.py).  Records,
strand bytes, text, offsets, begins and statistics are compared byte for byte, for every pair of every batch; every output buffer
starts as a sentinel and is checked beyond n."""
import numpy as np
import pytest

import frameshift_ref as fs
import frameshift_trace_ref as ft
import pairs_ref
import set_search_ref
from pairs_ex_ref import revcomp
from test_gpu_translate import _up, _full, _stream, _sync, _ptr, _pairs_up, back_translate, SENTINEL, FILL
from test_gpu_frameshift import _noisy_read, _anchored_read, _dna, _b62, _align
from util import random_seqs, AA

pytestmark = pytest.mark.gpu

FWD, REV, BOTH = 0, 1, 2
RECT = 2
G, R = 16, 10                   # the shipped instantiation: a strip is G * R rows, a lane's rows change every R
BAD = ft.BAD
TRACE = "pmx_swfs_kernel<16,10,trace>"
SLACK = 32                      # text bytes behind the capacity, to stay sentinel


def _cfg(pkg, pm, open_=11, ext=1, stats=True):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, open_, ext, 0, pkg.WANT_CIGAR | (pkg.WANT_STATS if stats else 0), pm.inner)


class Got:
    pass


def _run(pkg, cfg, Q, Rs, pairs, mode, f, mq, mr, capacity, chunk=0, strands=None, stats=True, beg=True):
    """pmx_align_pairs_frameshift_cigar_device -> every output as it lies in its buffer, sentinels beyond n checked"""
    import torch
    n = len(pairs)
    rec = _full((n + 2, 4), SENTINEL, torch.int32); won = _full((n + 2,), FILL, torch.uint8)
    st = _full((n + 2, 3), SENTINEL, torch.int32) if stats else None
    bg = _full((n + 2, 2), SENTINEL, torch.int32) if beg else None
    text = _full((capacity + SLACK,), FILL, torch.uint8); off = _full((n + 3,), SENTINEL, torch.int64)
    d_pairs = _pairs_up(pairs)
    d_strand = _up(np.asarray(strands, dtype=np.uint8)) if strands is not None else None
    pkg.align_pairs_frameshift_cigar_device(cfg, Q, Rs, n, d_pairs.data_ptr(), _ptr(d_strand), mode, f, mq, mr, rec.data_ptr(), won.data_ptr(),
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
    assert g.rec[:n].tobytes() == want.records.tobytes()
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


# --------------------------------------------------------------------------------------------------------------- 1. top-row edges
def _lattice_batch(pkg, orc):
    """every window W = 3 .. 12 against every m = 1 .. 5, as test_gpu_frameshift.test_top_row_edges builds it; the model's results for
    three gap models x three penalties -- computed once, shared, left unchanged"""
    p = Batch()
    p.pm, p.om = _b62(pkg, orc)
    rng = np.random.default_rng(15200)
    p.prots = [q for m in range(1, 6) for q in random_seqs(rng, 4, m, m, AA)]
    p.reads = []
    for W in range(3, 13):
        for rep in range(4):
            q = p.prots[int(rng.integers(0, len(p.prots)))]
            s = (back_translate(rng, q) + _dna(rng, 12))[:W]
            p.reads.append(_dna(rng, rep % 3) + s[:W - rep % 3] if rep else s)
    assert sorted({len(s) for s in p.reads}) == list(range(3, 13))
    p.Q, p.R = pkg.SeqSet.new(p.reads), pkg.SeqSet.new(p.prots)
    p.pairs = pairs_ref.pairs_array([(i, j) for i in range(len(p.reads)) for j in range(len(p.prots))])
    p.cases = [(o, e, f) for o, e in ((11, 1), (2, 1), (1, 1)) for f in (0, 1, 15)]
    p.want = {c: ft.results(p.reads, p.prots, p.pairs, BOTH, p.om, c[0], c[1], c[2]) for c in p.cases}
    return p


@pytest.fixture(scope="module")
def lattice(pkg, orc):
    return _lattice_batch(pkg, orc)


def test_top_row_edges(pkg, lattice):
    """rows 0 .. 3 have missing predecessors; cheap, equal penalties make ties, which is where the precedence shows"""
    p = lattice
    nonempty = 0
    seen = {"m": 0, ft.CODON_GAP: 0, ft.REF_GAP: 0, ft.SHORT: 0, ft.LONG: 0}
    for case in p.cases:
        want = p.want[case]
        total = int(want.off[-1])
        g = _run(pkg, _cfg(pkg, p.pm, case[0], case[1]), p.Q, p.R, p.pairs, BOTH, case[2], 10, 5, total)
        _same(g, want)
        assert g.kernel == TRACE
        nonempty += sum(1 for t in want.texts if t)
        for t in want.texts:
            for key, v in ft.counts(t).items():
                seen[key] += v
    assert nonempty > 1000 and all(v > 0 for v in seen.values()), (nonempty, seen)


# ----------------------------------------------------------------------------------------- 2. lane hand-offs and strip seams
BOUNDARIES = (40, 160, 320)             # a lane boundary inside the first strip, and the two strip seams
EVENTS = ("base deleted", "base inserted", "codon inserted")


def _planted_read(rng, prot, pos, kind):
    """a read that codes for the 27 letters of `prot` behind a random flank, with one event at nucleotide `pos` of the read"""
    e = min(39, pos // 3 * 3)                                # the event's offset in the coding piece, a codon boundary
    s = bytearray(back_translate(rng, prot))
    if kind == "base deleted":
        del s[e]
    elif kind == "base inserted":
        s[e:e] = _dna(rng, 1)
    else:
        s[e:e] = _dna(rng, 3)
    return _dna(rng, pos - e) + bytes(s) + _dna(rng, 4)


def _seams_batch(pkg, orc):
    """test_gpu_frameshift.test_handoff_and_strip_edges' batch -- every N from 1 to 2 G R + 5 against m = 40 -- and behind it, for each
    boundary and event kind, 13 planted reads whose event sits at nucleotide b - 6 .. b + 6; the model's results with gaps 11 / 1,
    fs 15, both strands -- computed once, shared, left unchanged"""
    p = Batch()
    p.pm, p.om = _b62(pkg, orc)
    rng = np.random.default_rng(15300)
    prots = random_seqs(rng, 12, 40, 40, AA)
    p.top = 2 * G * R + 5
    p.reads = [(_noisy_read if N % 2 else _anchored_read)(rng, prots[N % 12], N + 2) for N in range(1, p.top + 1)]
    rows = [(N - 1, N % 12) for N in range(1, p.top + 1)]
    rng2 = np.random.default_rng(16400)
    planted = random_seqs(rng2, 12, 27, 27, AA)
    for b in BOUNDARIES:
        for kind in EVENTS:
            for d in range(-6, 7):
                j = len(rows) % 12
                p.reads.append(_planted_read(rng2, planted[j], b + d, kind))
                rows.append((len(p.reads) - 1, 12 + j))
    p.prots = prots + planted
    p.Q, p.R = pkg.SeqSet.new(p.reads), pkg.SeqSet.new(p.prots)
    p.pairs = pairs_ref.pairs_array(rows)
    p.mq = max(len(s) for s in p.reads) - 2
    p.want = ft.results(p.reads, p.prots, p.pairs, BOTH, p.om, 11, 1, 15)
    p.capacity = int(p.want.off[-1])
    return p


@pytest.fixture(scope="module")
def seams(pkg, orc):
    return _seams_batch(pkg, orc)


def test_handoff_and_strip_edges(pkg, seams):
    p = seams
    # from the model's paths, not from the construction: every step kind crosses every boundary (source row < b <= target row)
    crossing = {(b, how): 0 for b in BOUNDARIES for how in ("3", ft.SHORT, ft.LONG, ft.CODON_GAP)}
    for text, beg in zip(p.want.texts, p.want.beg):
        for op, src, row, col, how in ft.steps(text, beg.tolist()):
            for b in BOUNDARIES:
                if src is not None and (b, how) in crossing and src < b <= row:
                    crossing[(b, how)] += 1
    assert all(v > 0 for v in crossing.values()), crossing
    g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, 40, p.capacity)
    _same(g, p.want)
    assert g.kernel == TRACE + "/strips"
    p.got = g                                                  # (the unswitched run, for test_parts)


def test_one_strip_without_scratch(pkg, seams):
    """the first G R pairs alone: one strip, no boundary scratch, chunks of seven -- the bytes of the long batch's prefix"""
    p = seams
    n = G * R
    want = ft.results(p.reads, p.prots, p.pairs[:n], BOTH, p.om, 11, 1, 15)
    assert want.records.tobytes() == p.want.records[:n].tobytes() and want.texts == p.want.texts[:n]
    g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs[:n], BOTH, 15, n, 40, int(want.off[-1]), chunk=7)
    _same(g, want)
    assert g.kernel == TRACE


def test_parts(pkg, seams, monkeypatch):
    """a bound on the trace scratch that cuts the batch into at least three parts changes no byte"""
    p = seams
    base = getattr(p, "got", None) or _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, 40, p.capacity)
    per_slot = -(-p.mq // (G * R)) * 40 * 192                  # strips x columns x 192 bytes
    slots = 2 * len(p.pairs)
    bound = per_slot * 150
    assert -(-slots // (bound // per_slot // 4 * 4)) >= 3
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(bound))
    g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, 40, p.capacity)
    monkeypatch.undo()
    _bytes_equal(g, base)
    _same(g, p.want)
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(bound))
    g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, 40, p.capacity, chunk=97)      # parts inside chunks
    monkeypatch.undo()
    _bytes_equal(g, base)
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(4 * per_slot - 1))
    with pytest.raises(pkg.BatchError, match="PMX_CIGAR_CHUNK_BYTES"):
        _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, 40, p.capacity)


def test_text_capacity(pkg, seams):
    """a capacity below the need: the offsets still give the full need, the texts that fit are written, the rest stays sentinel"""
    p = seams
    total = p.capacity
    for cap in (total - 1, total // 2):
        g = _run(pkg, _cfg(pkg, p.pm), p.Q, p.R, p.pairs, BOTH, 15, p.mq, 40, cap, chunk=101)
        _same(g, p.want, capacity=cap)
        assert int(g.off[len(p.pairs)]) == total


# ------------------------------------------------------------------------------------------------------ 6. strands and bad pairs
def test_strands_and_bad_pairs(pkg, orc):
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(16500)
    prots = random_seqs(rng, 4, 10, 30, AA) + [b"WWWW"]
    reads = [_noisy_read(rng, prots[0], 60), b"AT", b"A", b"ATG", _noisy_read(rng, prots[1], 33), revcomp(_noisy_read(rng, prots[2], 57)),
             revcomp(_noisy_read(rng, prots[3], 48)), _noisy_read(rng, prots[3], 70), b"TGA"]
    Q, Rs = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    rows = [(0, 0), (4, 1), (1, 0), (3, 2), (2, 1), (0, 5), (9, 0), (0, 1, 59, -1, 0, -1), (0, 1, 58, 2, 0, -1), (0, 1, 57, 3, 0, -1),
            (4, 0, 0, -1, 40, 2), (4, 3), (5, 2), (6, 3), (7, 3), (5, 0), (6, 1, 3, 40, 2, -1), (8, 4), (0, 2)]
    pairs = pairs_ref.pairs_array(rows)
    cfg = _cfg(pkg, pm)
    bad_at = [2, 4, 5, 6, 7, 8, 10, 14]                        # W < 3, bad descriptors, and read 7: N = 68 > max_qlen = 60
    both = None
    for mode in (FWD, REV, BOTH):
        want = ft.results(reads, prots, pairs, mode, om, 11, 1, 15, max_qlen=60)
        assert [k for k in range(len(rows)) if want.records[k].tolist() == BAD] == bad_at
        for k in bad_at:
            assert want.texts[k] == "" and want.beg[k].tolist() == [-1, -1] and want.stats[k].tolist() == [0, 0, 0] and want.strand[k] == 0
        for chunk in (0, 1, 5):
            _same(_run(pkg, cfg, Q, Rs, pairs, mode, 15, 60, 30, int(want.off[-1]), chunk), want)
        both = want if mode == BOTH else both
    assert set(both.strand.tolist()) == {0, 1}
    # a stop codon (its reverse strand reads S) against WWWW scores nothing: the empty path
    k = rows.index((8, 4))
    assert both.records[k].tolist() == [0, 2, 0, 0] and both.texts[k] == "" and both.beg[k].tolist() == [3, 1]
    # a strand byte per pair; bytes outside {0, 1} make pairs 3 and 9 bad
    sb = rng.integers(0, 2, len(rows)).astype(np.uint8)
    sb[3], sb[9] = 2, 255
    want = ft.results(reads, prots, pairs, FWD, om, 11, 1, 15, strands=sb, max_qlen=60)
    assert [k for k in range(len(rows)) if want.records[k].tolist() == BAD] == sorted(bad_at + [3, 9])
    _same(_run(pkg, cfg, Q, Rs, pairs, FWD, 15, 60, 30, int(want.off[-1]), 5, strands=sb), want)
    # optional outputs left out change nothing else
    g = _run(pkg, _cfg(pkg, pm, stats=False), Q, Rs, pairs, BOTH, 15, 60, 30, int(both.off[-1]), stats=False, beg=False)
    _same(g, both)
    # the host entry: the same through Aligner, bad pairs refused by name
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    good = [k for k in range(len(rows)) if k not in bad_at]
    want = ft.results(reads, prots, pairs[good], BOTH, om, 11, 1, 15)
    rec, cig, beg, won, st = al.align_pairs_frameshift_cigar(Q, Rs, pairs[good], 15, strand="both", stats=True, chunk_pairs=3)
    assert rec.view(np.int32).reshape(-1, 4).tobytes() == want.records.tobytes() and cig == want.texts and beg.tobytes() == want.beg.tobytes()
    assert won.tolist() == want.strand.tolist() and st.view(np.int32).reshape(-1, 3).tobytes() == want.stats.tobytes()
    rec2, cig2, beg2, won2 = al.align_pairs_frameshift_cigar(Q, Rs, pairs[good], 15, strand=won)
    assert rec2.tobytes() == rec.tobytes() and cig2 == cig and beg2.tobytes() == beg.tobytes() and won2.tolist() == won.tolist()
    with pytest.raises(pkg.BatchError, match="pair 2: "):
        al.align_pairs_frameshift_cigar(Q, Rs, pairs, 15, strand="both")


# ------------------------------------------------------------------------------------------------------- 7. search round trip
def test_search_round_trip(pkg, orc):
    """40 reads x 12 proteins, every fourth read coding with one planted frameshift: the search's hit pairs and strand bytes, as they
    are, give the hits' records back and texts that hold the planted op"""
    import torch
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(16600)
    prots = random_seqs(rng, 12, 40, 60, AA)
    reads, planted = [], {}
    for i in range(40):
        if i % 4:
            reads.append(_dna(rng, int(rng.integers(60, 121))))
            continue
        j = (i // 4) % 12
        s = bytearray(back_translate(rng, prots[j][3:35]))
        if i % 8:
            s[48:48] = _dna(rng, 1); planted[i] = (j, ft.LONG)
        else:
            del s[48]; planted[i] = (j, ft.SHORT)
        s = _dna(rng, 5) + bytes(s) + _dna(rng, 7)
        reads.append(revcomp(s) if i % 3 == 1 else s)
    Q, Rs = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    n = 40 * 12
    cfg0 = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, pm.inner)
    cap = n
    hp = _full((cap * 32,), FILL, torch.uint8); hi = _full((cap,), SENTINEL, torch.int64)
    hr = _full((cap, 4), SENTINEL, torch.int32); hb = _full((cap,), FILL, torch.uint8); cnt = _full((2,), SENTINEL, torch.int64)
    pkg.search_pairs_frameshift_device(cfg0, Q, Rs, RECT, 0, n, None, 130, 60, 60, hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), cap, cnt.data_ptr(),
                                       BOTH, 15, hb.data_ptr(), _stream(), 0)
    _sync()
    hits = int(cnt.cpu().numpy()[1])
    assert 10 <= hits < 40
    index = hi.cpu().numpy()[:hits]
    assert {int(x) for x in index} >= {i * 12 + j for i, (j, _) in planted.items()}
    hit_pairs = hp.cpu().numpy().view(pairs_ref.PAIR_DTYPE)[:hits]; hit_strand = hb.cpu().numpy()[:hits]
    want = ft.results(reads, prots, hit_pairs, FWD, om, 11, 1, 15, strands=hit_strand)
    # fed as they lie on the device
    rec = _full((hits + 2, 4), SENTINEL, torch.int32); won = _full((hits + 2,), FILL, torch.uint8)
    total = int(want.off[-1])
    text = _full((total + SLACK,), FILL, torch.uint8); off = _full((hits + 3,), SENTINEL, torch.int64)
    pkg.align_pairs_frameshift_cigar_device(_cfg(pkg, pm, stats=False), Q, Rs, hits, hp.data_ptr(), hb.data_ptr(), FWD, 15, 130, 60, rec.data_ptr(),
                                            won.data_ptr(), None, None, text.data_ptr(), total, off.data_ptr(), _stream(), 0)
    _sync()
    assert rec.cpu().numpy()[:hits].tobytes() == hr.cpu().numpy()[:hits].tobytes() == want.records.tobytes()
    assert won.cpu().numpy()[:hits].tolist() == hit_strand.tolist() and off.cpu().numpy()[:hits + 1].tolist() == want.off.tolist()
    raw = text.cpu().numpy()
    assert raw[:total].tobytes() == want.text_bytes() and (raw[total:] == FILL).all()
    texts = {int(x): t for x, t in zip(index, want.texts)}
    for i, (j, op) in planted.items():
        assert op in texts[i * 12 + j], (i, j, texts[i * 12 + j])
    # the same through Aligner: PairHits.pairs / .strand accepted as they are
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    h = al.search_pairs(Q, Rs, min_score=60, frameshift=15, strand="both")
    rec2, cig, beg, won2 = al.align_pairs_frameshift_cigar(Q, Rs, h.pairs, 15, strand=h.strand)
    assert rec2.tobytes() == h.records.tobytes() and cig == want.texts and won2.tolist() == h.strand.tolist() and beg.tobytes() == want.beg.tobytes()


# ----------------------------------------------------------------------------------------------------- 8. score kernel untouched
def test_score_kernel_untouched(pkg, lattice):
    """the score-only entry on the lattice: the records and strand bytes of the score model, and the kernel name it had"""
    p = lattice
    for case in p.cases:
        cfg0 = pkg.pmx_config_t(pkg.MODE_SW, 0, case[0], case[1], 0, 0, p.pm.inner)
        rec, won, kernel = _align(pkg, cfg0, p.Q, p.R, p.pairs, BOTH, case[2], 10, 5)
        want = fs.records(p.reads, p.prots, p.pairs, BOTH, p.om, case[0], case[1], case[2])
        assert rec.tobytes() == want[0].tobytes() == p.want[case].records.tobytes() and won.tolist() == want[1].tolist()
        assert kernel == "pmx_swfs_kernel<16,10>"
