"""Per-query top-K set search (`-m gpu`): pmx_search_topk[_device] against the full entry (pmx_align_pairs_device on the rectangle's
descriptors) followed by the numpy restatement tests/topk_ref.py, and -- one case per mode -- the full entry itself against the CPU
oracle on the strings.  K and row geometry, chunk geometry, ties, order of arrival, thresholds, skip_self, sub-ranges, capacity,
statistics, kernel families, bad pairs, the CIGAR pass over the hit pairs, the host entry and the Python mirror.  Every comparison is
exact; every output buffer starts as a sentinel with slots behind the capacity."""
import ctypes as C

import numpy as np
import pytest

import pairs_ref
import set_search_ref
import topk_ref as ref
from util import random_seqs, mutate, AA, golden

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
INT32_MAX, INT32_MIN = ref.INT32_MAX, ref.INT32_MIN
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


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


def _full_entry(pkg, cfg, Q, R, q_first, nq, mq, mr):
    """the yardstick: the records (and statistics) of rows [q_first, q_first + nq) of Q x R from pmx_align_pairs_device on the
    descriptors of the rectangle"""
    import torch
    stats = bool(cfg.want & pkg.WANT_STATS)
    nr = len(R)
    n = nq * nr
    descs = set_search_ref.rect_pairs_descriptors(nr, q_first * nr, n)
    rec = _full((max(n, 1), 4), SENTINEL, torch.int32)
    st = _full((max(n, 1), 3), SENTINEL, torch.int32) if stats else None
    d_pairs = _up(descs.view(np.uint8))
    pkg.align_pairs_device(cfg, Q, R, n, d_pairs.data_ptr(), mq, mr, rec.data_ptr(), _ptr(st), _stream())
    kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    recs = rec.cpu().numpy()[:n]
    recs.setflags(write=False)
    return recs, (st.cpu().numpy()[:n] if stats else None), descs, kernel


class Got:
    """outputs of one pmx_search_topk_device call, whole buffers, on the host"""


def _topk(pkg, cfg, Q, R, q_first, nq, mq, mr, min_score, k, capacity, chunk=0, skip_self=False, with_pairs=True, with_index=True,
          with_passing=True):
    import torch
    stats = bool(cfg.want & pkg.WANT_STATS)
    slots = capacity + 3                                                # (sentinel entries behind the capacity)
    hp = _full((slots * 32,), FILL, torch.uint8) if with_pairs else None
    hi = _full((slots,), SENTINEL, torch.int64) if with_index else None
    hr = _full((slots, 4), SENTINEL, torch.int32)
    hs = _full((slots, 3), SENTINEL, torch.int32) if stats else None
    off = _full((nq + 1 + 2,), SENTINEL, torch.int64)
    rp = _full((nq + 2,), SENTINEL, torch.int64) if with_passing else None
    cnt = _full((3 + 2,), SENTINEL, torch.int64)
    pkg.search_topk_device(cfg, Q, R, q_first, nq, mq, mr, min_score, k, skip_self, _ptr(hp), _ptr(hi), hr.data_ptr(), _ptr(hs), capacity,
                           off.data_ptr(), _ptr(rp), cnt.data_ptr(), _stream(), chunk)
    g = Got()
    g.kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    host = lambda t: t.cpu().numpy() if t is not None else None
    g.pairs, g.index, g.recs, g.stats, g.off, g.passing, g.counts = host(hp), host(hi), host(hr), host(hs), host(off), host(rp), host(cnt)
    if g.pairs is not None:
        g.pairs = g.pairs.view(pairs_ref.PAIR_DTYPE)
    g.d_pairs = hp
    g.all = [a for a in (g.pairs, g.index, g.recs, g.stats, g.off, g.passing, g.counts) if a is not None]
    return g


def _same(g, want, capacity, nq):
    """row_off and counts in full, the first min(kept, capacity) entries equal to the reference's, every entry behind them -- and
    behind the offsets, the passing counts and the three counts -- the sentinel"""
    kept = int(want["row_off"][-1])
    w = min(kept, capacity)
    assert g.off[:nq + 1].tolist() == want["row_off"].tolist() and (g.off[nq + 1:] == SENTINEL).all()
    assert g.counts[:3].tolist() == [kept, w, int(want["row_passing"].sum())] and (g.counts[3:] == SENTINEL).all()
    if g.passing is not None:
        assert g.passing[:nq].tolist() == want["row_passing"].tolist() and (g.passing[nq:] == SENTINEL).all()
    assert g.recs[:w].tobytes() == want["records"][:w].tobytes() and (g.recs[w:] == SENTINEL).all()
    if g.index is not None:
        assert g.index[:w].tolist() == want["index"][:w].tolist() and (g.index[w:] == SENTINEL).all()
    if g.pairs is not None:
        assert g.pairs[:w].tobytes() == want["pairs"][:w].tobytes() and (g.pairs[w:].view(np.uint8) == FILL).all()
    if g.stats is not None:
        assert g.stats[:w].tobytes() == want["stats"][:w].tobytes() and (g.stats[w:] == SENTINEL).all()


def _identical(a, b):
    assert len(a.all) == len(b.all)
    for x, y in zip(a.all, b.all):
        assert x.tobytes() == y.tobytes()


def _oracle_check(pkg, orc, cfg, om, qseqs, rseqs, descs, recs, stats=None):
    """the yardstick itself against the CPU oracle on the strings"""
    strings = pairs_ref.resolve(qseqs, rseqs, descs)
    assert all(s is not None for s in strings)
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    sg = cfg.sg_flags if cfg.mode == 1 else orc.SG_ALL
    if stats is not None:
        want = orc.align_stats_sample(cfg.mode, np.arange(len(strings)), qb, qo, rb, ro, cfg.open, cfg.extend, om, sg_flags=sg, bits=cfg.width)
        assert (stats == want[:, 3:6]).all()
    else:
        want = orc.align_batch(cfg.mode, qb, qo, rb, ro, cfg.open, cfg.extend, om, sg_flags=sg, bits=cfg.width)
    assert (recs[:, :3] == want[:, :3]).all() and (recs[:, 3] == 0).all()


# -------------------------------------------------------------------------------- 1. 7 queries x 300 references: chunk geometry, K
NQ7, NR300 = 7, 300
RELATED = {0: 0, 2: 150, 5: 299}                    # query row -> the reference it was derived from; the other rows are unrelated


def sets7x300():
    rng = np.random.default_rng(11400)
    rseqs = random_seqs(rng, NR300, 20, 60)
    for k in RELATED.values():
        rseqs[k] = random_seqs(rng, 1, 60, 60)[0]
    qseqs = random_seqs(rng, NQ7, 20, 60)
    for i, k in RELATED.items():
        qseqs[i] = (mutate(rng, rseqs[k], 0.05, 0.01)[:60] + b"ACGTACGTACGTACGTACGT")[:60]
    return qseqs, rseqs


@pytest.fixture(scope="module")
def case7(pkg, orc):
    """the sets and the yardstick's records of all 2100 pairs (checked against the oracle once), shared and left unchanged"""
    pm, om = _dna(pkg, orc)
    qseqs, rseqs = sets7x300()
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    recs, _, descs, kernel = _full_entry(pkg, cfg, Q, R, 0, NQ7, 60, 60)
    _oracle_check(pkg, orc, cfg, om, qseqs, rseqs, descs, recs)
    return pm, cfg, Q, R, qseqs, rseqs, recs, kernel


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 256, 1024])
def test_chunk_geometry_never_changes_a_byte(pkg, case7, k):
    """|R| = 300: chunks of 64 (a row over five chunks, rows that start and end inside chunks), 192 (a tail, no whole row, a head), 2048
    (a tail plus whole rows plus a head: six rows and 248 records), 300 and 600 (a chunk ends exactly at a row's end), the default"""
    pm, cfg, Q, R, qseqs, rseqs, recs, kernel = case7
    want = ref.topk(recs, NR300, 0, NQ7, k)
    assert want["row_off"].tolist() == [min(k, NR300) * i for i in range(NQ7 + 1)]        # (K above |R|: the whole row, sorted)
    runs = []
    for chunk in (64, 192, 2048, 300, 600, 0, 64):
        g = _topk(pkg, cfg, Q, R, 0, NQ7, 60, 60, INT32_MIN, k, NQ7 * NR300, chunk)
        assert chunk or g.kernel == kernel                                                # (the same chunks: the same alignment kernel)
        _same(g, want, NQ7 * NR300, NQ7)
        runs.append(g)
    for g in runs[1:]:
        _identical(g, runs[0])                                                            # one chunking against another, and a second run


def test_thresholds_and_row_passing(pkg, case7):
    pm, cfg, Q, R, qseqs, rseqs, recs, kernel = case7
    score = recs[:, 0].reshape(NQ7, NR300)
    unrelated = max(int(score[i].max()) for i in range(NQ7) if i not in RELATED)
    ms = unrelated + 1
    want = ref.topk(recs, NR300, 0, NQ7, 10, ms)
    sizes = np.diff(want["row_off"]).tolist()
    assert [s > 0 for s in sizes] == [i in RELATED for i in range(NQ7)]                   # empty rows between non-empty ones
    for i, r in RELATED.items():
        assert int(want["pairs"][want["row_off"][i]]["r"]) == r                           # the planted relative leads its row
    for chunk in (0, 64):
        _same(_topk(pkg, cfg, Q, R, 0, NQ7, 60, 60, ms, 10, 70, chunk), want, 70, NQ7)
    mid = int(np.median(score))                                                           # K above some rows' passing counts, below others'
    pc = (score >= mid).sum(axis=1)
    assert pc.min() < pc.max()
    k = max(1, int(np.sort(pc)[NQ7 // 2]))
    want = ref.topk(recs, NR300, 0, NQ7, k, mid)
    assert (want["row_passing"] == pc).all() and np.diff(want["row_off"]).tolist() == np.minimum(pc, k).tolist()
    for chunk in (0, 192):
        _same(_topk(pkg, cfg, Q, R, 0, NQ7, 60, 60, mid, k, NQ7 * k, chunk), want, NQ7 * k, NQ7)
    g = _topk(pkg, cfg, Q, R, 0, NQ7, 60, 60, INT32_MAX, 10, 70, 64)
    assert g.off[:NQ7 + 1].tolist() == [0] * (NQ7 + 1) and g.counts[:3].tolist() == [0, 0, 0]
    _same(g, ref.topk(recs, NR300, 0, NQ7, 10, INT32_MAX), 70, NQ7)
    g = _topk(pkg, cfg, Q, R, 0, NQ7, 60, 60, INT32_MIN, 10, 70)
    assert g.passing[:NQ7].tolist() == [NR300] * NQ7
    _same(g, ref.topk(recs, NR300, 0, NQ7, 10), 70, NQ7)


def test_sub_range_capacity_and_optional_outputs(pkg, case7):
    import torch
    pm, cfg, Q, R, qseqs, rseqs, recs, kernel = case7
    sub = recs[2 * NR300:6 * NR300]
    want = ref.topk(sub, NR300, 2, 4, 9)
    assert want["index"].min() >= 2 * NR300 and want["pairs"]["q"].min() == 2               # absolute p, absolute row
    for chunk in (0, 64, 500):
        _same(_topk(pkg, cfg, Q, R, 2, 4, 60, 60, INT32_MIN, 9, 36, chunk), want, 36, 4)
    for cap in (0, 13, 36, 40):                                                           # nothing, an end inside row 1, the total, more
        for chunk in (0, 64):
            g = _topk(pkg, cfg, Q, R, 2, 4, 60, 60, INT32_MIN, 9, cap, chunk)
            _same(g, ref.topk(sub, NR300, 2, 4, 9, capacity=cap), cap, 4)
            assert g.off[:5].tolist() == [0, 9, 18, 27, 36]                               # in full whatever the capacity
    for with_pairs, with_index, with_passing in ((False, True, True), (True, False, False), (False, False, False)):
        g = _topk(pkg, cfg, Q, R, 2, 4, 60, 60, INT32_MIN, 9, 13, 64, False, with_pairs, with_index, with_passing)
        _same(g, ref.topk(sub, NR300, 2, 4, 9, capacity=13), 13, 4)
    off, cnt = _full((5,), SENTINEL, torch.int64), _full((3,), SENTINEL, torch.int64)     # capacity 0 with no hit buffer at all: counting
    pkg.search_topk_device(cfg, Q, R, 2, 4, 60, 60, INT32_MIN, 9, False, None, None, None, None, 0, off.data_ptr(), None, cnt.data_ptr(), _stream(), 64)
    _sync()
    assert off.cpu().tolist() == [0, 9, 18, 27, 36] and cnt.cpu().tolist() == [36, 0, 4 * NR300]
    pkg.search_topk_device(cfg, Q, R, 2, 0, 60, 60, INT32_MIN, 9, False, None, None, None, None, 0, off.data_ptr(), None, cnt.data_ptr(), _stream(), 64)
    _sync()
    assert cnt.cpu().tolist() == [0, 0, 0] and off.cpu().tolist()[0] == 0                 # no rows: zero counts


def test_statistics_travel_with_their_hits(pkg, orc, case7):
    pm, cfg, Q, R, qseqs, rseqs, recs, kernel = case7
    cfg_s = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    frec, fst, descs, _ = _full_entry(pkg, cfg_s, Q, R, 0, NQ7, 60, 60)
    ms = int(np.median(frec[:, 0]))
    want = ref.topk(frec, NR300, 0, NQ7, 65, ms, stats=fst)
    assert len(want["stats"]) > NQ7 * 30 and len({tuple(r) for r in want["stats"].tolist()}) > 5
    for chunk in (0, 64, 2048):
        _same(_topk(pkg, cfg_s, Q, R, 0, NQ7, 60, 60, ms, 65, NQ7 * 65, chunk), want, NQ7 * 65, NQ7)


# ------------------------------------------------------------------------------------------- 2. |R| around the tile of 2048 records
@pytest.fixture(scope="module")
def refs2049():
    rng = np.random.default_rng(11500)
    return random_seqs(rng, 6, 30, 60), random_seqs(rng, 2049, 20, 60)


@pytest.mark.parametrize("nr", [1, 63, 65, 2047, 2048, 2049])
def test_row_lengths_around_wave_and_tile(pkg, orc, refs2049, nr):
    pm, om = _dna(pkg, orc)
    qseqs, rall = refs2049
    rseqs = rall[:nr]
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    recs, _, descs, kernel = _full_entry(pkg, cfg, Q, R, 0, 6, 60, 60)
    ks = (1, 2, 64) if nr == 1 else (1, 63, 64, 65, 1024) if nr < 100 else (1, 65, 256, 1024)
    chunks = (0, 64) if nr < 100 else (0, 3000, 2048)                                     # 3000: a row and the head of the next one
    for k in ks:
        want = ref.topk(recs, nr, 0, 6, k)
        runs = [_topk(pkg, cfg, Q, R, 0, 6, 60, 60, INT32_MIN, k, 6 * min(k, nr), chunk) for chunk in chunks]
        for g in runs:
            _same(g, want, 6 * min(k, nr), 6)
        assert runs[0].kernel == kernel
    ms = int(np.sort(recs[:, 0])[len(recs) // 2])                                         # half of the pairs pass
    want = ref.topk(recs, nr, 0, 6, 64, ms)
    for chunk in chunks:
        _same(_topk(pkg, cfg, Q, R, 0, 6, 60, 60, ms, 64, 6 * 64, chunk), want, 6 * 64, 6)


# ------------------------------------------------------------------------------------------------------------------------- 3. ties
def test_all_scores_equal(pkg, orc):
    pm, om = _dna(pkg, orc)
    rng = np.random.default_rng(11600)
    one = random_seqs(rng, 1, 40, 40)[0]
    qseqs, rseqs = random_seqs(rng, 6, 30, 50), [one] * 150
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    recs, _, descs, _ = _full_entry(pkg, cfg, Q, R, 0, 6, 50, 40)
    assert all(len(set(recs[i * 150:(i + 1) * 150, 0].tolist())) == 1 for i in range(6))
    for k in (5, 70):                                                                     # 70: across the edge of the 64-pair chunks
        want = ref.topk(recs, 150, 0, 6, k)
        assert all(want["pairs"]["r"][i * k:(i + 1) * k].tolist() == list(range(k)) for i in range(6))
        for chunk in (64, 192, 2048, 0, 7):
            _same(_topk(pkg, cfg, Q, R, 0, 6, 50, 40, INT32_MIN, k, 6 * k, chunk), want, 6 * k, 6)


def test_the_cut_inside_a_tie_run_that_straddles_a_chunk(pkg, orc):
    pm, om = _dna(pkg, orc)
    rng = np.random.default_rng(11610)
    query = random_seqs(rng, 1, 50, 50)[0]
    high, low = query[:40], query[:25]                                                    # 80 and 50 against the query
    rseqs = [high if j % 2 == 0 else low for j in range(150)]
    qseqs = [query] * 6
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    recs, _, descs, _ = _full_entry(pkg, cfg, Q, R, 0, 6, 50, 40)
    assert recs[:150:2, 0].tolist() == [80] * 75 and recs[1:150:2, 0].tolist() == [50] * 75
    for k, row0 in ((40, list(range(0, 80, 2))), (100, list(range(0, 150, 2)) + list(range(1, 50, 2)))):
        want = ref.topk(recs, 150, 0, 6, k)                                               # 40: the cut at j = 78, behind the chunk edge at 64
        assert want["pairs"]["r"][:k].tolist() == row0
        for chunk in (64, 192, 0, 7):
            _same(_topk(pkg, cfg, Q, R, 0, 6, 50, 40, INT32_MIN, k, 6 * k, chunk), want, 6 * k, 6)


def test_order_of_arrival(pkg, orc):
    """scores that rise with j: every chunk replaces the whole list; scores that fall with j: nothing after the first K survives"""
    pm, om = _dna(pkg, orc)
    rng = np.random.default_rng(11620)
    query = random_seqs(rng, 1, 60, 60)[0]
    rising = [query[:21 + j] for j in range(40)]
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    Q = pkg.SeqSet.new([query] * 6)
    for rseqs, first in ((rising, list(range(39, 34, -1))), (rising[::-1], list(range(5)))):
        R = pkg.SeqSet.new(rseqs)
        recs, _, descs, _ = _full_entry(pkg, cfg, Q, R, 0, 6, 60, 60)
        assert recs[:40, 0].tolist() == [2 * len(r) for r in rseqs]
        want = ref.topk(recs, 40, 0, 6, 5)
        assert want["pairs"]["r"][:5].tolist() == first
        for chunk in (7, 64, 0):
            _same(_topk(pkg, cfg, Q, R, 0, 6, 60, 60, INT32_MIN, 5, 30, chunk), want, 30, 6)


# -------------------------------------------------------------------------------------------------------------------- 4. skip_self
def test_skip_self(pkg, orc):
    pm, om = _dna(pkg, orc)
    seqs = random_seqs(np.random.default_rng(11700), 40, 30, 60)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    S = pkg.SeqSet.new(seqs)
    recs, _, descs, _ = _full_entry(pkg, cfg, S, S, 0, 40, 60, 60)
    score = recs[:, 0].reshape(40, 40)
    assert all(score[i, i] == 2 * len(seqs[i]) and (np.delete(score[i], i) < score[i, i]).all() for i in range(40))
    for R in (S, None):
        for chunk in (0, 64):
            with_self = ref.topk(recs, 40, 0, 40, 5)
            assert (with_self["pairs"]["r"][::5] == np.arange(40)).all()                  # the self pair leads its row
            _same(_topk(pkg, cfg, S, R, 0, 40, 60, 60, INT32_MIN, 5, 200, chunk), with_self, 200, 40)
            without = ref.topk(recs, 40, 0, 40, 5, skip_self=True)
            assert (without["pairs"]["q"] != without["pairs"]["r"]).all() and np.diff(without["row_off"]).tolist() == [5] * 40
            assert without["row_passing"].tolist() == [39] * 40
            _same(_topk(pkg, cfg, S, R, 0, 40, 60, 60, INT32_MIN, 5, 200, chunk, True), without, 200, 40)
    sub = ref.topk(recs[10 * 40:25 * 40], 40, 10, 15, 40, skip_self=True)                  # K = |R| keeps the 39 others of rows 10 .. 24
    _same(_topk(pkg, cfg, S, S, 10, 15, 60, 60, INT32_MIN, 40, 15 * 40, 64, True), sub, 15 * 40, 15)


# ------------------------------------------------------------------------------------------------------------ 5. kernel families
def _related(rng, n, lo, hi, alphabet, sub, indel):
    seqs = random_seqs(rng, n, lo, hi, alphabet)
    for k in range(0, n, 4):
        seqs[k] = mutate(rng, seqs[(k + 7) % n], sub, indel, alphabet)[:hi]
        if len(seqs[k]) < lo:
            seqs[k] = seqs[(k + 7) % n]
    return seqs


def _family(pkg, orc, cfg, om, seqs, kernel, oracle=True):
    S = pkg.SeqSet.new(seqs)
    n = len(seqs)
    recs, st, descs, name = _full_entry(pkg, cfg, S, S, 0, n, 60, 60)
    assert name.startswith(kernel[0]) and kernel[1] in name, name
    if oracle:
        _oracle_check(pkg, orc, cfg, om, seqs, seqs, descs, recs, st)
    ms = int(np.median(recs[:, 0]))                                                       # about half of every row passes: more than K
    want = ref.topk(recs, n, 0, n, 7, ms, skip_self=True, stats=st)
    assert 0 < want["counts"][0] < want["counts"][2]
    for chunk in (0, 500):
        g = _topk(pkg, cfg, S, S, 0, n, 60, 60, ms, 7, 7 * n, chunk, True)
        assert chunk or g.kernel == name                                                  # no other road under the same chunks
        _same(g, want, 7 * n, n)


def test_local_protein_blosum62(pkg, orc):
    pm, om = pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))
    seqs = _related(np.random.default_rng(11800), 70, 20, 60, AA, 0.2, 0.02)              # 4 900 pairs in one chunk: past the 2 048 of pmx_sw16m
    _family(pkg, orc, pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, pm.inner), om, seqs, ("pmx_sw16m_kernel", "matrix lookup"))


def test_global_dna(pkg, orc):
    pm, om = _dna(pkg, orc)
    seqs = _related(np.random.default_rng(11810), 40, 20, 60, ACGT, 0.05, 0.01)
    _family(pkg, orc, pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 0, 0, pm.inner), om, seqs, ("pmx_nwsg16", ""))


def test_semi_global_with_statistics(pkg, orc):
    pm, om = _dna(pkg, orc)
    seqs = _related(np.random.default_rng(11820), 40, 20, 60, ACGT, 0.05, 0.01)
    _family(pkg, orc, pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, pkg.WANT_STATS, pm.inner), om, seqs, ("pmx_stats16", ""))


def test_the_32_bit_road(pkg, orc):
    pm, om = _dna(pkg, orc)
    seqs = _related(np.random.default_rng(11830), 40, 20, 60, ACGT, 0.05, 0.01)
    # open < extend: outside the packed 16-bit kernels' gap model, so a kernel with 32-bit cells runs
    cfg = pkg.pmx_config_t(pkg.MODE_NW, 0, 2, 5, 32, 0, pm.inner)
    name = pkg.lib.pmx_kernel_for(C.byref(cfg), 60, 60).decode()
    assert "32" in name or "general" in name
    _family(pkg, orc, cfg, om, seqs, (name, ""), oracle=False)


# --------------------------------------------------------------------------------------------------------------------- 6. bad pairs
def test_bad_pairs_keep_their_flag(pkg, orc):
    pm, om = _dna(pkg, orc)
    rng = np.random.default_rng(11900)
    qseqs, rseqs = random_seqs(rng, 6, 30, 50), random_seqs(rng, 80, 20, 50)
    rseqs[17] = b""                                                                       # an empty reference
    rseqs[44] = random_seqs(rng, 1, 70, 70)[0]                                            # one longer than max_rlen = 50
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    recs, st, descs, _ = _full_entry(pkg, cfg, Q, R, 0, 6, 50, 50)
    for j in (17, 44):
        assert recs[j].tolist() == list(pairs_ref.BAD_RECORD) and st[j].tolist() == [0, 0, 0]
    for ms, k in ((INT32_MIN, 80), (0, 80), (1, 80), (0, 3)):
        want = ref.topk(recs, 80, 0, 6, k, ms, stats=st)
        bad = [int(p["r"]) in (17, 44) for p in want["pairs"]]
        assert sum(bad) == (12 if ms <= 0 and k == 80 else 0)                             # a candidate at 0 with its flag, absent at 1
        for chunk in (0, 64):
            g = _topk(pkg, cfg, Q, R, 0, 6, 50, 50, ms, k, 6 * k, chunk)
            _same(g, want, 6 * k, 6)
            assert [r[3] == pairs_ref.BAD_RECORD[3] for r in g.recs[:len(bad)].tolist()] == bad
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    with pytest.raises(pkg.BatchError, match=r"pair 17 \(0, 17\): reference: empty window"):
        al.search_topk(Q, R, k=3)
    with pytest.raises(pkg.BatchError, match=r"pair 17 \(2, 17\): reference: empty window"):
        al.search_topk(Q, R, k=3, first_row=2, rows=2)
    holes = list(qseqs); holes[3] = b""
    with pytest.raises(pkg.BatchError, match=r"pair 34 \(3, 0\): query: empty window"):
        al.search_topk(pkg.SeqSet.new(holes), pkg.SeqSet.new(rseqs[:17]), k=3, first_row=1)
    # wrapped sets: the device pass meets the pair
    buf, off = pkg.pack(rseqs)
    d_buf, d_off = _up(buf), _up(off)
    W = pkg.SeqSet.wrap_device(d_buf.data_ptr(), d_off.data_ptr(), len(rseqs), len(buf), keep=(d_buf, d_off))
    with pytest.raises(pkg.BatchError, match=r"pair 17 \(1, 17\)"):
        al.search_topk(Q, W, k=3, first_row=1, min_score=INT32_MAX)


# ------------------------------------------------------------------------------------------------------------------ 7. composition
def test_hit_pairs_feed_the_cigar_entry_unchanged(pkg, orc, case7):
    import torch
    pm, cfg, Q, R, qseqs, rseqs, recs, kernel = case7
    om = _dna(pkg, orc)[1]
    g = _topk(pkg, cfg, Q, R, 0, NQ7, 60, 60, INT32_MIN, 20, NQ7 * 20, 64)
    h = int(g.counts[1])
    assert h == NQ7 * 20
    ccfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_CIGAR, pm.inner)
    capacity = 64 * h
    rec = _full((h, 4), SENTINEL, torch.int32)
    beg = _full((h, 2), SENTINEL, torch.int32)
    text = _full((capacity,), FILL, torch.uint8)
    off = _full((h + 1,), -9, torch.int64)
    pkg.align_pairs_ex_device(ccfg, Q, R, h, g.d_pairs.data_ptr(), None, 60, 60, rec.data_ptr(), None, beg.data_ptr(), text.data_ptr(),
                              capacity, off.data_ptr(), _stream(), 100)                  # the device hit list itself, nothing in between
    _sync()
    rec, beg, text, off = rec.cpu().numpy(), beg.cpu().numpy(), text.cpu().numpy(), off.cpu().numpy()
    assert rec.tobytes() == g.recs[:h].tobytes()                                          # the records equal the hit records
    assert 0 < off[h] <= capacity
    strings = pairs_ref.resolve(qseqs, rseqs, g.pairs[:h])
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    res, malformed = orc.rescore_cigars(text[:off[h]], off, qb, qo, rb, ro, 5, 2, om, beg=beg.reshape(-1), free_mask=0)
    assert malformed == 0 and (res[:, 0] == rec[:, 0]).all() and (res[:, 3] == 0).all()


# --------------------------------------------------------------------------------------------------- 8. host entry, Python mirror
def _host(pkg, cfg, Q, R, q_first, nq, ms, k, skip=0, chunk=0, sl=0):
    res = C.POINTER(pkg.pmx_topk_hits_t)()
    o = pkg.pmx_topk_opts_t(ms, k, skip, chunk, sl)
    rc = pkg.lib.pmx_search_topk(C.byref(cfg), Q.inner, R.inner if R is not None else None, q_first, nq, C.byref(o), C.byref(res))
    assert rc == 0, pkg.lib.pmx_last_error()
    try:
        return pkg.TopKHits(res.contents)
    finally:
        pkg.lib.pmx_topk_hits_free(res)


def _same_host(h, want, nq):
    assert h.n_rows == nq and h.n_hits == want["counts"][0] == len(h) and h.n_passing == want["counts"][2]
    assert h.row_off.tolist() == want["row_off"].tolist() and h.row_passing.tolist() == want["row_passing"].tolist()
    assert h.records.tobytes() == want["records"].tobytes() and h.pairs.tobytes() == want["pairs"].tobytes()
    assert h.index.tolist() == want["index"].tolist()
    if want["stats"] is not None:
        assert h.stats.tobytes() == want["stats"].tobytes()
    else:
        assert h.stats is None


def test_host_entry_and_python_mirror(pkg, case7):
    pm, cfg, Q, R, qseqs, rseqs, recs, kernel = case7
    score = recs[:, 0].reshape(NQ7, NR300)
    ms = max(int(score[i].max()) for i in range(NQ7) if i not in RELATED) - 3              # a few hits in most rows, more in the related ones
    want = ref.topk(recs, NR300, 0, NQ7, 12, ms)
    dev = _topk(pkg, cfg, Q, R, 0, NQ7, 60, 60, ms, 12, NQ7 * 12)
    _same(dev, want, NQ7 * 12, NQ7)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    for sl, chunk in ((1, 0), (3, 64), (0, 0), (3, 0)):
        h = _host(pkg, cfg, Q, R, 0, NQ7, ms, 12, 0, chunk, sl)
        _same_host(h, want, NQ7)
        assert h.records.tobytes() == dev.recs[:h.n_hits].tobytes() and h.row_off.tolist() == dev.off[:NQ7 + 1].tolist()
        _same_host(al.search_topk(Q, R, k=12, min_score=ms, chunk_pairs=chunk, slice_rows=sl), want, NQ7)
    sub = ref.topk(recs[NR300:5 * NR300], NR300, 1, 4, 3)
    for sl in (1, 3, 0):
        h = al.search_topk(Q, R, k=3, first_row=1, rows=4, slice_rows=sl)
        _same_host(h, sub, 4)
        p, x, r, s = h.row(2)
        assert x.tolist() == sub["index"][6:9].tolist() and (p["q"] == 3).all() and s is None and len(r) == 3
    none = al.search_topk(Q, R, k=3, min_score=INT32_MAX, slice_rows=2)
    assert none.n_hits == 0 and none.n_passing == 0 and none.row_off.tolist() == [0] * (NQ7 + 1)
    cfg_s = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    frec, fst, _, _ = _full_entry(pkg, cfg_s, Q, R, 0, NQ7, 60, 60)
    wst = ref.topk(frec, NR300, 0, NQ7, 12, ms, stats=fst)
    _same_host(al.search_topk(Q, R, k=12, min_score=ms, stats=True, slice_rows=3), wst, NQ7)
    # wrapped sets: maxima on the device; Q against itself with the flag
    buf, off = pkg.pack(qseqs)
    d_buf, d_off = _up(np.concatenate([np.zeros(3, dtype=np.uint8), buf])), _up(off)
    W = pkg.SeqSet.wrap_device(d_buf.data_ptr() + 3, d_off.data_ptr(), NQ7, len(buf), keep=(d_buf, d_off))
    _same_host(al.search_topk(W, R, k=12, min_score=ms, slice_rows=3), want, NQ7)
    qrec = _full_entry(pkg, cfg, Q, Q, 0, NQ7, 60, 60)[0]
    _same_host(al.search_topk(W, k=4, skip_self=True, slice_rows=2), ref.topk(qrec, NQ7, 0, NQ7, 4, skip_self=True), NQ7)
