"""The strand modes of the set entries (`-m gpu`): pmx_align_pairs_both[_device], pmx_search_pairs_stranded[_device] and
pmx_search_topk_stranded[_device] against two runs of the entry that existed before -- pmx_align_pairs_ex_device with strand bytes 0 and
1 -- folded and selected by tests/strands_ref.py, and a sample of the winners against the CPU oracle on the reverse-complemented
windows.  Every comparison is exact; every output buffer starts as a sentinel."""
import numpy as np
import pytest

import pairs_ref
import set_search_ref
import strands_ref as ref
from pairs_ex_ref import revcomp, resolve
from util import random_seqs, AA, golden

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)
LIST, TRI, RECT = 0, 1, 2
FWD, REV, BOTH = ref.STRAND_FORWARD, ref.STRAND_REVERSE, ref.STRAND_BOTH


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


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _dna(pkg, orc):
    return pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)


def _cfg(pkg, pm, mode="sw", want=0, open_=5, extend=2):
    m = {"sw": (pkg.MODE_SW, 0), "nw": (pkg.MODE_NW, 0), "sg": (pkg.MODE_SG, pkg.SG_ALL)}[mode]
    return pkg.pmx_config_t(m[0], m[1], open_, extend, 0, want, pm.inner)


def _ex(pkg, cfg, Q, R, pairs, strand, mq, mr):
    """the yardstick: pmx_align_pairs_ex_device over the descriptors with one strand byte for all -> records, statistics"""
    import torch
    n = len(pairs)
    stats = bool(cfg.want & pkg.WANT_STATS)
    rec = _full((n, 4), SENTINEL, torch.int32)
    st = _full((n, 3), SENTINEL, torch.int32) if stats else None
    d_pairs = _up(np.ascontiguousarray(pairs).view(np.uint8))
    d_strand = _full((n,), strand, torch.uint8)
    pkg.align_pairs_ex_device(cfg, Q, R, n, d_pairs.data_ptr(), d_strand.data_ptr(), mq, mr, rec.data_ptr(), _ptr(st), None, None, 0, None, _stream())
    _sync()
    recs = rec.cpu().numpy()
    recs.setflags(write=False)
    return recs, (st.cpu().numpy() if stats else None)


def _two(pkg, cfg, Q, R, pairs, mq, mr):
    rec0, st0 = _ex(pkg, cfg, Q, R, pairs, 0, mq, mr)
    rec1, st1 = _ex(pkg, cfg, Q, R, pairs, 1, mq, mr)
    return rec0, rec1, st0, st1


def _both(pkg, cfg, Q, R, pairs, mq, mr, chunk=0):
    """pmx_align_pairs_both_device -> records, statistics, strand bytes"""
    import torch
    n = len(pairs)
    stats = bool(cfg.want & pkg.WANT_STATS)
    rec = _full((n + 2, 4), SENTINEL, torch.int32)
    st = _full((n + 2, 3), SENTINEL, torch.int32) if stats else None
    won = _full((n + 2,), FILL, torch.uint8)
    d_pairs = _up(np.ascontiguousarray(pairs).view(np.uint8))
    pkg.align_pairs_both_device(cfg, Q, R, n, d_pairs.data_ptr(), mq, mr, rec.data_ptr(), _ptr(st), won.data_ptr(), _stream(), chunk)
    kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    rec, won = rec.cpu().numpy(), won.cpu().numpy()
    assert (rec[n:] == SENTINEL).all() and (won[n:] == FILL).all()
    if stats:
        st = st.cpu().numpy()
        assert (st[n:] == SENTINEL).all()
        st = st[:n]
    return rec[:n], st, won[:n], kernel


def _same_fold(got, want):
    rec, st, won = got[:3]
    wrec, wst, wwon = want
    assert won.tolist() == wwon.tolist()
    assert rec.tobytes() == wrec.tobytes()
    if wst is not None:
        assert st.tobytes() == wst.tobytes()


def _oracle_sample(pkg, orc, cfg, om, qseqs, rseqs, pairs, strand, recs, sample):
    """the folded records of `sample` against the CPU oracle on the windows, reverse-complemented where the strand says so"""
    strings = resolve(qseqs, rseqs, pairs[sample], strand[sample])
    assert all(s is not None for s in strings)
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    sg = cfg.sg_flags if cfg.mode == 1 else orc.SG_ALL
    want = orc.align_batch(cfg.mode, qb, qo, rb, ro, cfg.open, cfg.extend, om, sg_flags=sg, bits=cfg.width)
    assert (recs[sample][:, :3] == want[:, :3]).all() and (recs[sample][:, 3] == 0).all()


# ------------------------------------------------------------------------------------------------ the sets of cases 1, 6, 8 and 9
NQ, NR = 37, 23
PALINDROME = 36                                    # this read equals its reverse complement: a tie with every reference


def planted_sets():
    """37 reads of 20 - 70 bp; 23 references of 60 - 200 bp built from unmutated copies of reads -- as stored for even reads,
    reverse-complemented for odd ones -- between random spacers; reference 0 holds read 0 twice, once per strand."""
    rng = np.random.default_rng(12100)
    reads = random_seqs(rng, NQ, 20, 70)
    half = random_seqs(rng, 1, 17, 17)[0]
    reads[PALINDROME] = half + revcomp(half)
    assert reads[PALINDROME] == revcomp(reads[PALINDROME])
    refs = []
    for j in range(NR):
        parts, total = [], 0
        picks = [0, 0] if j == 0 else [int(x) for x in rng.choice(NQ - 1, size=4, replace=False)]
        for x, i in enumerate(picks):
            copy = reads[i] if (i % 2 == 0 and not (j == 0 and x == 1)) else revcomp(reads[i])
            spacer = random_seqs(rng, 1, 3, 12)[0]
            if total + len(spacer) + len(copy) > 200:
                break
            parts += [spacer, copy]
            total += len(spacer) + len(copy)
        ref_ = b"".join(parts)
        if len(ref_) < 60:
            ref_ += random_seqs(rng, 1, 60 - len(ref_), 60 - len(ref_))[0]
        refs.append(ref_)
    assert all(20 <= len(s) <= 70 for s in reads) and all(60 <= len(s) <= 200 for s in refs)
    return reads, refs


def planted_pairs(reads, refs):
    """all 851 pairs, every fifth with windows on both sides"""
    rows = []
    for i in range(NQ):
        for j in range(NR):
            k = i * NR + j
            rows.append((i, j, 2, len(reads[i]) - 5, 3, len(refs[j]) - 7) if k % 5 == 2 else (i, j))
    return pairs_ref.pairs_array(rows)


class Planted:
    pass


@pytest.fixture(scope="module")
def planted(pkg, orc):
    """the sets, the list and, per mode, the two yardstick runs with statistics: computed once, shared, left unchanged"""
    p = Planted()
    p.pm, p.om = _dna(pkg, orc)
    p.reads, p.refs = planted_sets()
    p.pairs = planted_pairs(p.reads, p.refs)
    p.Q, p.R = pkg.SeqSet.new(p.reads), pkg.SeqSet.new(p.refs)
    p.two = {}
    for mode in ("sw", "nw", "sg"):
        p.two[mode] = _two(pkg, _cfg(pkg, p.pm, mode, pkg.WANT_STATS), p.Q, p.R, p.pairs, 70, 200)
    return p


# ------------------------------------------------------------------------------------------------------- 1. fold against two _ex runs
@pytest.mark.parametrize("mode", ["sw", "nw", "sg"])
def test_fold_equals_two_ex_runs(pkg, orc, planted, mode):
    p = planted
    n = len(p.pairs)
    assert n == 851
    rec0, rec1, st0, st1 = p.two[mode]
    want = ref.fold(rec0, rec1, st0, st1)
    won = want[2]
    ties = int((rec0[:, 0] == rec1[:, 0]).sum())
    assert won.sum() * 4 >= n and (n - won.sum()) * 4 >= n and ties >= 1                     # no vacuous pass: both strands win, some tie
    cfg_s = _cfg(pkg, p.pm, mode, pkg.WANT_STATS)
    cfg = _cfg(pkg, p.pm, mode)
    runs = []
    for chunk in (0, 1, 7, 64, n - 1, n):                                                   # one, two, many chunks; a ragged last chunk
        got = _both(pkg, cfg_s, p.Q, p.R, p.pairs, 70, 200, chunk)
        _same_fold(got, want)
        runs.append(got)
    assert len({g[3] for g in runs if g[3]}) >= 1 and all(g[3] for g in runs)              # pmx_last_kernel names the alignment
    _same_fold(_both(pkg, cfg, p.Q, p.R, p.pairs, 70, 200, 64), (want[0], None, won))      # without statistics
    sample = np.concatenate([np.nonzero(won == 1)[0][:40], np.nonzero(won == 0)[0][:40], np.nonzero(rec0[:, 0] == rec1[:, 0])[0][:10]])
    _oracle_sample(pkg, orc, cfg, p.om, p.reads, p.refs, p.pairs, won, want[0], sample)


# -------------------------------------------------------------------------------------------------------------------------- 2. ties
def test_ties_go_to_the_forward_strand(pkg, orc):
    rng = np.random.default_rng(12200)
    pm, om = _dna(pkg, orc)
    halves = random_seqs(rng, 6, 10, 25)
    pals = [h + revcomp(h) for h in halves]                                                 # q == revcomp(q): rec0 == rec1
    q = random_seqs(rng, 1, 40, 40)[0]
    assert q != revcomp(q)
    spacer = random_seqs(rng, 1, 15, 15)[0]
    queries = pals + [q, q[1:]]
    refs = random_seqs(rng, 5, 60, 120) + [q + spacer + revcomp(q),                        # equal scores, different end_ref
                                           revcomp(q) + spacer + q,
                                           q[1:] + spacer + revcomp(q)]                     # the reverse copy better by exactly one match
    Q, R = pkg.SeqSet.new(queries), pkg.SeqSet.new(refs)
    pairs = pairs_ref.pairs_array([(i, j) for i in range(len(queries)) for j in range(len(refs))])
    for mode in ("sw", "sg", "nw"):
        cfg = _cfg(pkg, pm, mode, pkg.WANT_STATS)
        rec0, rec1, st0, st1 = _two(pkg, cfg, Q, R, pairs, 50, 120)
        want = ref.fold(rec0, rec1, st0, st1)
        for chunk in (0, 5):
            got = _both(pkg, cfg, Q, R, pairs, 50, 120, chunk)
            _same_fold(got, want)
        rec, _, won, _ = got
        pal = pairs["q"] < len(pals)
        assert rec0[pal].tobytes() == rec1[pal].tobytes() and (won[pal] == 0).all()
        if mode == "sw":
            at = lambda i, j: i * len(refs) + j
            for j in (5, 6):                                                                # both copies are there: 80 on either strand
                k = at(6, j)
                assert rec0[k][0] == rec1[k][0] == 80 and rec0[k][2] != rec1[k][2]
                assert won[k] == 0 and rec[k].tolist() == rec0[k].tolist()                  # strand 0 and rec0's ends
            k = at(6, 7)
            assert rec0[k][0] == 78 and rec1[k][0] == 80 and won[k] == 1 and rec[k].tolist() == rec1[k].tolist()
            k = at(7, 7)                                                                    # and seen from the shorter query: forward by one
            assert rec0[k][0] == 78 and rec1[k][0] == 78 and won[k] == 0


# ------------------------------------------------------------------------------------------------------------------ 3. PMX_WANT_SORTED
def test_sorted_keeps_the_slots_paired(pkg, orc):
    rng = np.random.default_rng(12300)
    pm, om = _dna(pkg, orc)
    seqs = random_seqs(rng, 60, 8, 250)
    for k in range(0, 60, 3):                                                               # relatives on either strand
        src = seqs[(k + 11) % 60]
        seqs[k] = src if k % 2 else revcomp(src)
    S = pkg.SeqSet.new(seqs)
    pairs = pairs_ref.all_pairs_descriptors(60, 0, pairs_ref.all_pairs_count(60))
    plain = _cfg(pkg, pm, "sw", pkg.WANT_STATS)
    srt = _cfg(pkg, pm, "sw", pkg.WANT_STATS | pkg.WANT_SORTED)
    want = ref.fold(*_two(pkg, plain, S, S, pairs, 250, 250))
    assert 0 < want[2].sum() < len(pairs)
    for chunk in (0, 100, 1000):
        _same_fold(_both(pkg, srt, S, S, pairs, 250, 250, chunk), want)
    _same_fold(_both(pkg, plain, S, S, pairs, 250, 250, 100), want)
    sample = np.concatenate([np.nonzero(want[2] == 1)[0][:30], np.nonzero(want[2] == 0)[0][:30]])
    _oracle_sample(pkg, orc, plain, om, seqs, seqs, pairs, want[2], want[0], sample)


# -------------------------------------------------------------------------------------------------------------- 4. a large alphabet
def test_protein_blosum62_in_both_mode(pkg, orc):
    rng = np.random.default_rng(12400)
    pm, om = pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))
    qs, rs = random_seqs(rng, 12, 30, 80, AA), random_seqs(rng, 12, 30, 80, AA)
    for k in range(0, 12, 2):
        rs[k] = revcomp(qs[(k + 1) % 12])                                                   # "reverse-complemented" proteins: the table acts on raw bytes
    assert any(revcomp(s) != s[::-1] for s in qs)                                           # (A, C, G, T, ... are amino acids too)
    Q, R = pkg.SeqSet.new(qs), pkg.SeqSet.new(rs)
    pairs = pairs_ref.pairs_array([(i, j) for i in range(12) for j in range(12)])
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, pkg.WANT_STATS, pm.inner)
    want = ref.fold(*_two(pkg, cfg, Q, R, pairs, 80, 80))
    assert 0 < want[2].sum() < 144
    for chunk in (0, 50):
        _same_fold(_both(pkg, cfg, Q, R, pairs, 80, 80, chunk), want)
    plain = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, pm.inner)
    _oracle_sample(pkg, orc, plain, om, qs, rs, pairs, want[2], want[0], np.arange(144))


# ------------------------------------------------------------------------------------------------------------- 5. bad descriptors
def test_bad_descriptors(pkg, planted):
    p = planted
    good = p.pairs[:200]
    bad = pairs_ref.pairs_array([(NQ, 0), (0, 1, 0, -1, 50, 500), (1, 2, 5, 0, 0, -1)])      # index out of range, window past the end, length 0
    at = [17, 64, 130]
    pairs = good.copy()
    pairs[at] = bad
    cfg = _cfg(pkg, p.pm, "sw", pkg.WANT_STATS)
    rec0, rec1, st0, st1 = _two(pkg, cfg, p.Q, p.R, pairs, 70, 200)
    assert all(rec0[k].tolist() == list(pairs_ref.BAD_RECORD) == rec1[k].tolist() for k in at)
    want = ref.fold(rec0, rec1, st0, st1)
    ok = np.ones(200, dtype=bool); ok[at] = False
    full = ref.fold(*[a[:200] for a in p.two["sw"]])
    for chunk in (0, 64, 1):
        rec, st, won, _ = got = _both(pkg, cfg, p.Q, p.R, pairs, 70, 200, chunk)
        _same_fold(got, want)
        for k in at:
            assert rec[k].tolist() == list(pairs_ref.BAD_RECORD) and st[k].tolist() == [0, 0, 0] and won[k] == 0
        assert rec[ok].tobytes() == full[0][ok].tobytes() and won[ok].tolist() == full[2][ok].tolist()      # the neighbours are unaffected
    al = pkg.Aligner.new().local().matrix(p.pm).gap_open(5).gap_extend(2).build()
    with pytest.raises(pkg.BatchError, match=r"pair 17: query: index outside"):
        al.align_pairs(p.Q, p.R, pairs, strand="both")
    with pytest.raises(pkg.BatchError, match=r"pair 17: query: index outside"):
        al.search_pairs(p.Q, p.R, pairs=pairs, strand="both")
    for ms in (0, 1):                                                                       # in search: a hit at 0, its flag kept; none at 1
        w = ref.search(rec0, rec1, ms, 0, pairs, st0, st1)
        assert all((k in w["index"]) == (ms <= 0) for k in at)
        for chunk in (0, 64):
            g = _search(pkg, cfg, p.Q, p.R, LIST, 0, 200, pairs, 70, 200, ms, 200, BOTH, chunk)
            _same_search(g, w, 200)
        if ms == 0:
            x = w["index"].tolist().index(64)
            assert g.recs[x].tolist() == list(pairs_ref.BAD_RECORD) and g.strand[x] == 0


# ---------------------------------------------------------------------------------------------- 6. pmx_search_pairs_stranded_device
class Got:
    """outputs of one search call, whole buffers, on the host"""


def _search(pkg, cfg, Q, R, shape, first, n, pairs, mq, mr, min_score, capacity, mode, chunk=0, optional=True, plain=False):
    """pmx_search_pairs_stranded_device, or (plain) pmx_search_pairs_device"""
    import torch
    stats = bool(cfg.want & pkg.WANT_STATS)
    slots = capacity + 3                                                # (sentinel entries behind the capacity)
    hp = _full((slots * 32,), FILL, torch.uint8) if optional else None
    hi = _full((slots,), SENTINEL, torch.int64) if optional else None
    hr = _full((slots, 4), SENTINEL, torch.int32)
    hs = _full((slots, 3), SENTINEL, torch.int32) if stats else None
    hb = _full((slots,), FILL, torch.uint8) if optional and not plain else None
    cnt = _full((2,), SENTINEL, torch.int64)
    d_pairs = _up(np.ascontiguousarray(pairs).view(np.uint8)) if shape == LIST and n else None
    if plain:
        pkg.search_pairs_device(cfg, Q, R, shape, first, n, _ptr(d_pairs), mq, mr, min_score, _ptr(hp), _ptr(hi), hr.data_ptr(), _ptr(hs),
                                capacity, cnt.data_ptr(), _stream(), chunk)
    else:
        pkg.search_pairs_stranded_device(cfg, Q, R, shape, first, n, _ptr(d_pairs), mq, mr, min_score, _ptr(hp), _ptr(hi), hr.data_ptr(), _ptr(hs),
                                         capacity, cnt.data_ptr(), mode, _ptr(hb), _stream(), chunk)
    g = Got()
    g.kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    host = lambda t: t.cpu().numpy() if t is not None else None
    g.pairs, g.index, g.recs, g.stats, g.strand, g.counts = host(hp), host(hi), host(hr), host(hs), host(hb), host(cnt)
    if g.pairs is not None:
        g.pairs = g.pairs.view(pairs_ref.PAIR_DTYPE)
    g.d_pairs, g.d_strand = hp, hb
    g.all = [a for a in (g.pairs, g.index, g.recs, g.stats, g.counts) if a is not None]
    return g


def _same_search(g, want, capacity):
    """counts in full, the first min(passing, capacity) entries equal to the reference's, every entry behind them the sentinel"""
    w = min(want["passing"], capacity)
    assert g.counts.tolist() == [want["passing"], w]
    assert g.recs[:w].tobytes() == want["records"][:w].tobytes() and (g.recs[w:] == SENTINEL).all()
    if g.strand is not None:
        assert g.strand[:w].tolist() == want["strand"][:w].tolist() and (g.strand[w:] == FILL).all()
    if g.index is not None:
        assert g.index[:w].tolist() == want["index"][:w].tolist() and (g.index[w:] == SENTINEL).all()
    if g.pairs is not None and want["pairs"] is not None:
        assert g.pairs[:w].tobytes() == want["pairs"][:w].tobytes() and (g.pairs[w:].view(np.uint8) == FILL).all()
    if g.stats is not None:
        assert g.stats[:w].tobytes() == want["stats"][:w].tobytes() and (g.stats[w:] == SENTINEL).all()


def _identical(a, b, strand=True):
    assert len(a.all) == len(b.all)
    for x, y in zip(a.all, b.all):
        assert x.tobytes() == y.tobytes()
    if strand:
        assert a.strand.tobytes() == b.strand.tobytes()


def _levels(scores):
    """thresholds that leave roughly nothing, 5 % and everything"""
    s = np.sort(scores)
    return (INT32_MAX, int(s[-max(1, len(s) // 20)]), INT32_MIN)


def test_search_list_and_rectangle(pkg, planted):
    p = planted
    n = len(p.pairs)
    cfg = _cfg(pkg, p.pm, "sw", pkg.WANT_STATS)
    rec0, rec1, st0, st1 = p.two["sw"]
    folded = ref.fold(rec0, rec1)
    # LIST: the caller's descriptors with their windows
    for ms in _levels(folded[0][:, 0]):
        want = ref.search(rec0, rec1, ms, 0, p.pairs, st0, st1)
        if ms == INT32_MAX:
            assert want["passing"] == 0
        elif ms == INT32_MIN:
            assert want["passing"] == n
        else:
            assert n // 25 <= want["passing"] <= n // 8 and 0 < want["strand"].sum() < want["passing"]
        runs = [_search(pkg, cfg, p.Q, p.R, LIST, 0, n, p.pairs, 70, 200, ms, n, BOTH, chunk) for chunk in (0, 64, 7, n - 1, 0)]
        for g in runs:
            _same_search(g, want, n)
            _identical(g, runs[0])                                                          # chunking and a second run: not a byte differs
    ms = _levels(folded[0][:, 0])[1]
    passing = ref.search(rec0, rec1, ms)["passing"]
    for cap in (0, 1, passing - 1, passing, passing + 5):                                   # capacity below and above the passing, and none
        for chunk in (0, 64):
            _same_search(_search(pkg, cfg, p.Q, p.R, LIST, 0, n, p.pairs, 70, 200, ms, cap, BOTH, chunk),
                         ref.search(rec0, rec1, ms, 0, p.pairs, st0, st1, capacity=cap), cap)
    g = _search(pkg, cfg, p.Q, p.R, LIST, 0, n, p.pairs, 70, 200, ms, n, BOTH, 64, optional=False)      # optional outputs NULL
    assert g.pairs is None and g.index is None and g.strand is None
    _same_search(g, ref.search(rec0, rec1, ms, 0, p.pairs, st0, st1), n)
    import torch
    cnt = _full((2,), SENTINEL, torch.int64)                                                # capacity 0 with no hit buffer at all: counting
    plain = _cfg(pkg, p.pm, "sw")                                                           # (no statistics: no statistics buffer)
    d_list = _up(p.pairs.view(np.uint8))
    pkg.search_pairs_stranded_device(plain, p.Q, p.R, LIST, 0, n, d_list.data_ptr(), 70, 200, ms, None, None, None, None, 0,
                                     cnt.data_ptr(), BOTH, None, _stream(), 64)
    _sync()
    assert cnt.cpu().tolist() == [passing, 0]
    # RECT: whole sequences, a window that starts and ends inside a row
    first, rn = 5, NQ * NR - 9
    descs = set_search_ref.rect_pairs_descriptors(NR, first, rn)
    r0, r1, _, _ = _two(pkg, plain, p.Q, p.R, descs, 70, 200)
    for mode in (BOTH, REV, FWD):
        for ms in _levels(ref.fold(r0, r1, mode=mode)[0][:, 0]):
            want = ref.search(r0, r1, ms, first, descs, mode=mode)
            runs = [_search(pkg, plain, p.Q, p.R, RECT, first, rn, None, 70, 200, ms, rn, mode, chunk) for chunk in (0, 100, 23)]
            for g in runs:
                _same_search(g, want, rn)
                _identical(g, runs[0])
    # FORWARD is the existing entry, byte for byte; REVERSE is the existing entry over reverse-complemented queries
    ms = _levels(ref.fold(r0, r1)[0][:, 0])[1]
    Qrc = pkg.SeqSet.new([revcomp(s) for s in p.reads])
    for chunk in (0, 100):
        f = _search(pkg, plain, p.Q, p.R, RECT, first, rn, None, 70, 200, ms, rn, FWD, chunk)
        old = _search(pkg, plain, p.Q, p.R, RECT, first, rn, None, 70, 200, ms, rn, FWD, chunk, plain=True)
        _identical(f, old, strand=False)
        assert f.kernel == old.kernel and (f.strand[:int(f.counts[1])] == 0).all()
        r = _search(pkg, plain, p.Q, p.R, RECT, first, rn, None, 70, 200, ms, rn, REV, chunk)
        old = _search(pkg, plain, Qrc, p.R, RECT, first, rn, None, 70, 200, ms, rn, FWD, chunk, plain=True)
        _identical(r, old, strand=False)
        assert int(r.counts[1]) > 0 and (r.strand[:int(r.counts[1])] == 1).all()


def test_search_triangle_on_the_reads(pkg, planted):
    p = planted
    cfg = _cfg(pkg, p.pm, "sw")
    total = pairs_ref.all_pairs_count(NQ)
    first, n = 3, total - 7
    descs = pairs_ref.all_pairs_descriptors(NQ, first, n)
    r0, r1, _, _ = _two(pkg, cfg, p.Q, p.Q, descs, 70, 70)
    for ms in _levels(ref.fold(r0, r1)[0][:, 0]):
        want = ref.search(r0, r1, ms, first, descs)
        runs = [_search(pkg, cfg, p.Q, None, TRI, first, n, None, 70, 70, ms, n, BOTH, chunk) for chunk in (0, 64, 0)]
        for g in runs:
            _same_search(g, want, n)
            _identical(g, runs[0])
    f = _search(pkg, cfg, p.Q, None, TRI, first, n, None, 70, 70, 20, n, FWD, 64)
    _identical(f, _search(pkg, cfg, p.Q, None, TRI, first, n, None, 70, 70, 20, n, FWD, 64, plain=True), strand=False)


# ------------------------------------------------------------------------------------------------ 7. pmx_search_topk_stranded_device
def _topk(pkg, cfg, Q, R, q_first, nq, mq, mr, min_score, k, capacity, mode, chunk=0, skip_self=False, plain=False):
    import torch
    stats = bool(cfg.want & pkg.WANT_STATS)
    slots = capacity + 3
    hp = _full((slots * 32,), FILL, torch.uint8)
    hi = _full((slots,), SENTINEL, torch.int64)
    hr = _full((slots, 4), SENTINEL, torch.int32)
    hs = _full((slots, 3), SENTINEL, torch.int32) if stats else None
    hb = _full((slots,), FILL, torch.uint8) if not plain else None
    off = _full((nq + 1 + 2,), SENTINEL, torch.int64)
    rp = _full((nq + 2,), SENTINEL, torch.int64)
    cnt = _full((3 + 2,), SENTINEL, torch.int64)
    if plain:
        pkg.search_topk_device(cfg, Q, R, q_first, nq, mq, mr, min_score, k, skip_self, hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), _ptr(hs),
                               capacity, off.data_ptr(), rp.data_ptr(), cnt.data_ptr(), _stream(), chunk)
    else:
        pkg.search_topk_stranded_device(cfg, Q, R, q_first, nq, mq, mr, min_score, k, skip_self, hp.data_ptr(), hi.data_ptr(), hr.data_ptr(),
                                        _ptr(hs), capacity, off.data_ptr(), rp.data_ptr(), cnt.data_ptr(), mode, _ptr(hb), _stream(), chunk)
    g = Got()
    g.kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    host = lambda t: t.cpu().numpy() if t is not None else None
    g.pairs, g.index, g.recs, g.stats, g.strand = host(hp).view(pairs_ref.PAIR_DTYPE), host(hi), host(hr), host(hs), host(hb)
    g.off, g.passing, g.counts = host(off), host(rp), host(cnt)
    g.d_pairs, g.d_strand = hp, hb
    g.all = [a for a in (g.pairs, g.index, g.recs, g.stats, g.off, g.passing, g.counts) if a is not None]
    return g


def _same_topk(g, want, capacity, nq):
    kept = int(want["row_off"][-1])
    w = min(kept, capacity)
    assert g.off[:nq + 1].tolist() == want["row_off"].tolist() and (g.off[nq + 1:] == SENTINEL).all()
    assert g.counts[:3].tolist() == [kept, w, int(want["row_passing"].sum())] and (g.counts[3:] == SENTINEL).all()
    assert g.passing[:nq].tolist() == want["row_passing"].tolist() and (g.passing[nq:] == SENTINEL).all()
    assert g.recs[:w].tobytes() == want["records"][:w].tobytes() and (g.recs[w:] == SENTINEL).all()
    assert g.index[:w].tolist() == want["index"][:w].tolist() and (g.index[w:] == SENTINEL).all()
    assert g.pairs[:w].tobytes() == want["pairs"][:w].tobytes() and (g.pairs[w:].view(np.uint8) == FILL).all()
    if g.strand is not None:
        assert g.strand[:w].tolist() == want["strand"][:w].tolist() and (g.strand[w:] == FILL).all()
    if g.stats is not None:
        assert g.stats[:w].tobytes() == want["stats"][:w].tobytes() and (g.stats[w:] == SENTINEL).all()


@pytest.mark.parametrize("nr", [1, 65, 2049])
def test_topk_around_the_wave_and_the_tile(pkg, nr):
    rng = np.random.default_rng(12700 + nr)
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    nq = 5
    qseqs = random_seqs(rng, nq, 12, 24)
    rseqs = random_seqs(rng, nr, 12, 24)
    for j in range(0, nr, 7):                                                               # relatives of the queries on either strand
        src = qseqs[j % nq]
        rseqs[j] = src if (j // 7) % 2 else revcomp(src)
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    cfg = _cfg(pkg, pm, "sw", pkg.WANT_STATS)
    descs = set_search_ref.rect_pairs_descriptors(nr, 0, nq * nr)
    rec0, rec1, st0, st1 = _two(pkg, cfg, Q, R, descs, 24, 24)
    for k in (1, 3, 64, 1024):
        cap = nq * min(k, nr)
        want = ref.topk(rec0, rec1, nr, 0, nq, k, stats0=st0, stats1=st1)
        if nr > 1:
            assert 0 < want["strand"].sum() < len(want["strand"])
        runs = [_topk(pkg, cfg, Q, R, 0, nq, 24, 24, INT32_MIN, k, cap, BOTH, chunk) for chunk in (0, 100, nr + 3, 2500, 0)]      # rows and tiles split
        for g in runs:
            _same_topk(g, want, cap, nq)
            _identical(g, runs[0])
    sub0, sub1 = rec0[nr:4 * nr], rec1[nr:4 * nr]                                           # a sub-range of rows, a threshold, a small capacity
    want = ref.topk(sub0, sub1, nr, 1, 3, 3, min_score=14, stats0=st0[nr:4 * nr], stats1=st1[nr:4 * nr], capacity=4)
    _same_topk(_topk(pkg, cfg, Q, R, 1, 3, 24, 24, 14, 3, 4, BOTH, 77), want, 4, 3)
    plain = _cfg(pkg, pm, "sw")
    for k, chunk in ((3, 0), (64, 100)):                                                    # FORWARD is the existing entry, byte for byte
        f = _topk(pkg, plain, Q, R, 0, nq, 24, 24, INT32_MIN, k, nq * min(k, nr), FWD, chunk)
        old = _topk(pkg, plain, Q, R, 0, nq, 24, 24, INT32_MIN, k, nq * min(k, nr), FWD, chunk, plain=True)
        _identical(f, old, strand=False)
        assert f.kernel == old.kernel and (f.strand[:int(f.counts[1])] == 0).all()
        r = _topk(pkg, plain, Q, R, 0, nq, 24, 24, INT32_MIN, k, nq * min(k, nr), REV, chunk)
        _same_topk(r, ref.topk(rec0, rec1, nr, 0, nq, k, mode=REV), nq * min(k, nr), nq)
        assert (r.strand[:int(r.counts[1])] == 1).all()


def test_topk_tie_run_mixes_strands_and_skip_self(pkg):
    rng = np.random.default_rng(12800)
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    q = random_seqs(rng, 1, 30, 30)[0]
    half = random_seqs(rng, 1, 15, 15)[0]
    pal = half + revcomp(half)
    assert q != revcomp(q) and pal == revcomp(pal)
    # one set: q, then copies of q on alternating strands (all score 60 against q), the palindrome, background
    seqs = [q] + [q if j % 2 else revcomp(q) for j in range(20)] + [pal] + random_seqs(rng, 8, 30, 30)
    n = len(seqs)
    S = pkg.SeqSet.new(seqs)
    cfg = _cfg(pkg, pm, "sw")
    descs = set_search_ref.rect_pairs_descriptors(n, 0, n * n)
    rec0, rec1, _, _ = _two(pkg, cfg, S, S, descs, 30, 30)
    assert (np.maximum(rec0[:21, 0], rec1[:21, 0]) == 60).all()
    for k in (5, 12):
        for skip in (False, True):
            want = ref.topk(rec0, rec1, n, 0, n, k, skip_self=skip)
            row0 = want["index"][:k]
            assert row0.tolist() == list(range(1 if skip else 0, (1 if skip else 0) + k))    # the tie run at 60 is cut by ascending j ...
            s = want["strand"][:k].tolist()
            assert 0 in s and 1 in s                                                        # ... through both strands, not by strand
            for chunk in (0, 7, n + 4, 3 * n - 2):                                          # the run straddles chunks
                g = _topk(pkg, cfg, S, S, 0, n, 30, 30, INT32_MIN, k, n * k, BOTH, chunk, skip_self=skip)
                _same_topk(g, want, n * k, n)
            if skip:                                                                        # (i, i) is no candidate on either strand -- the palindrome's too
                assert all(int(pr["q"]) != int(pr["r"]) for pr in g.pairs[:int(g.counts[1])])
                assert g.passing[:n].tolist() == [n - 1] * n


# ------------------------------------------------------------------------------------------ 8. hits feed the CIGAR entry unchanged
def _cigars_of_hits(pkg, orc, p, g, h, qseqs, rseqs, Q, R, mq, mr):
    import torch
    ccfg = _cfg(pkg, p.pm, "sw", pkg.WANT_CIGAR)
    capacity = 256 * h
    rec = _full((h, 4), SENTINEL, torch.int32)
    beg = _full((h, 2), SENTINEL, torch.int32)
    text = _full((capacity,), FILL, torch.uint8)
    off = _full((h + 1,), -9, torch.int64)
    pkg.align_pairs_ex_device(ccfg, Q, R, h, g.d_pairs.data_ptr(), g.d_strand.data_ptr(), mq, mr, rec.data_ptr(), None, beg.data_ptr(),
                              text.data_ptr(), capacity, off.data_ptr(), _stream(), 50)     # the device hit list itself, nothing in between
    _sync()
    rec, beg, text, off = rec.cpu().numpy(), beg.cpu().numpy(), text.cpu().numpy(), off.cpu().numpy()
    assert rec.tobytes() == g.recs[:h].tobytes()                                            # score and end positions of the hit records
    assert 0 < off[h] <= capacity
    strings = resolve(qseqs, rseqs, g.pairs[:h], g.strand[:h])
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    res, malformed = orc.rescore_cigars(text[:off[h]], off, qb, qo, rb, ro, 5, 2, p.om, beg=beg.reshape(-1), free_mask=0)
    assert malformed == 0 and (res[:, 0] == rec[:, 0]).all() and (res[:, 3] == 0).all()


def test_hits_feed_the_cigar_entry_unchanged(pkg, orc, planted):
    p = planted
    cfg = _cfg(pkg, p.pm, "sw")
    n = len(p.pairs)
    g = _search(pkg, cfg, p.Q, p.R, LIST, 0, n, p.pairs, 70, 200, 30, n, BOTH, 64)
    h = int(g.counts[1])
    assert h > 30 and 0 < g.strand[:h].sum() < h
    _cigars_of_hits(pkg, orc, p, g, h, p.reads, p.refs, p.Q, p.R, 70, 200)
    t = _topk(pkg, cfg, p.Q, p.R, 0, NQ, 70, 200, INT32_MIN, 3, 3 * NQ, BOTH, 100)
    h = int(t.counts[1])
    assert h == 3 * NQ and 0 < t.strand[:h].sum() < h
    _cigars_of_hits(pkg, orc, p, t, h, p.reads, p.refs, p.Q, p.R, 70, 200)


# --------------------------------------------------------------------------------------------------- 9. host entries, Python mirror
def test_host_entries_and_python_mirror(pkg, orc, planted):
    p = planted
    n = len(p.pairs)
    al = pkg.Aligner.new().local().matrix(p.pm).gap_open(5).gap_extend(2).build()
    als = pkg.Aligner.new().local().matrix(p.pm).gap_open(5).gap_extend(2).use_stats().build()
    rec0, rec1, st0, st1 = p.two["sw"]
    want = ref.fold(rec0, rec1, st0, st1)
    for chunk in (0, 100):
        rec, won = al.align_pairs(p.Q, p.R, p.pairs, chunk_pairs=chunk, strand="both")
        assert rec.view(np.int32).reshape(-1, 4).tobytes() == want[0].tobytes() and won.tolist() == want[2].tolist()
    rec, st, won = als.align_pairs(p.Q, p.R, p.pairs, strand="both")
    assert rec.view(np.int32).tobytes() == want[0].tobytes() and st.view(np.int32).tobytes() == want[1].tobytes() and won.tolist() == want[2].tolist()
    rec, cigars, begins, won = al.align_pairs(p.Q, p.R, p.pairs, strand="both", cigar=True)
    assert rec.view(np.int32).tobytes() == want[0].tobytes() and won.tolist() == want[2].tolist() and len(cigars) == n
    again = al.align_pairs(p.Q, p.R, p.pairs, strand=want[2], cigar=True)                   # the fold, then _ex with the chosen strands
    assert list(cigars) == list(again[1]) and begins.tobytes() == again[2].tobytes()
    # wrapped sets: validation and maxima on the device
    qb, qo = pkg.pack(p.reads); rb, ro = pkg.pack(p.refs)
    keep = (_up(qb), _up(qo), _up(rb), _up(ro))
    WQ = pkg.SeqSet.wrap_device(keep[0].data_ptr(), keep[1].data_ptr(), NQ, len(qb), keep=keep[:2])
    WR = pkg.SeqSet.wrap_device(keep[2].data_ptr(), keep[3].data_ptr(), NR, len(rb), keep=keep[2:])
    rec, won = al.align_pairs(WQ, WR, p.pairs, strand="both")
    assert rec.view(np.int32).tobytes() == want[0].tobytes() and won.tolist() == want[2].tolist()
    # search_pairs
    ms = _levels(want[0][:, 0])[1]
    w = ref.search(rec0, rec1, ms, 0, p.pairs, st0, st1)
    for kw in ({}, {"slice_pairs": 100}, {"slice_pairs": 64, "chunk_pairs": 7}, {"max_hits": 5}):
        for Q, R in ((p.Q, p.R), (WQ, WR)):
            h = al.search_pairs(Q, R, min_score=ms, pairs=p.pairs, strand="both", stats=True, **kw)
            cut = ref.search(rec0, rec1, ms, 0, p.pairs, st0, st1, capacity=kw.get("max_hits"))
            assert h.n_passing == w["passing"] and h.n_hits == cut["written"]
            assert h.records.view(np.int32).tobytes() == cut["records"].tobytes() and h.strand.tolist() == cut["strand"].tolist()
            assert h.pairs.tobytes() == cut["pairs"].tobytes() and h.index.tolist() == cut["index"].tolist()
            assert h.stats.view(np.int32).tobytes() == cut["stats"].tobytes()
    plain = al.search_pairs(p.Q, p.R, min_score=ms, pairs=p.pairs)                          # the default: forward, all-zero strands
    assert len(plain.strand) == plain.n_hits > 0 and not plain.strand.any()
    assert plain.records.view(np.int32).tobytes() == set_search_ref.hits(rec0, ms)["records"].tobytes()
    descs = set_search_ref.rect_pairs_descriptors(NR, 0, NQ * NR)
    r0, r1, _, _ = _two(pkg, _cfg(pkg, p.pm, "sw"), p.Q, p.R, descs, 70, 200)
    rms = _levels(ref.fold(r0, r1)[0][:, 0])[1]
    for strand, mode in (("both", BOTH), (1, REV), (pkg.STRAND_FORWARD, FWD)):
        h = al.search_pairs(p.Q, p.R, min_score=rms, strand=strand, slice_pairs=200)
        w = ref.search(r0, r1, rms, 0, descs, mode=mode)
        assert h.n_hits == w["passing"] and h.records.view(np.int32).tobytes() == w["records"].tobytes()
        assert h.strand.tolist() == w["strand"].tolist() and h.index.tolist() == w["index"].tolist()
    # search_topk
    for kw in ({}, {"slice_rows": 5}, {"slice_rows": 1, "chunk_pairs": 30}):
        for Q, R in ((p.Q, p.R), (WQ, WR)):
            t = al.search_topk(Q, R, k=4, strand="both", **kw)
            w = ref.topk(r0, r1, NR, 0, NQ, 4)
            assert t.row_off.tolist() == w["row_off"].tolist() and t.row_passing.tolist() == w["row_passing"].tolist()
            assert t.records.view(np.int32).tobytes() == w["records"].tobytes() and t.strand.tolist() == w["strand"].tolist()
            assert t.index.tolist() == w["index"].tolist() and t.pairs.tobytes() == w["pairs"].tobytes()
    t = al.search_topk(p.Q, p.R, k=4)
    assert len(t.strand) == t.n_hits > 0 and not t.strand.any()
