"""The top-K kernels on records of the test's own making (`-m gpu`): pmx_topk_records_device, the record-level hook that runs the
chunk loop, merges and tail of pmx_search_topk_device without the alignments, against the numpy restatement tests/topk_ref.py.  Scores
over all of int32, rows of more than 256 tiles, K and row lengths at the collector's edges, hundreds of thousands of one-record rows,
the self pair in late tiles, the strand bit of the emit.  Every comparison is exact; every output buffer starts as a sentinel with
slots behind the capacity; the fields of a record other than the score are noise that has to come back byte for byte."""
import numpy as np
import pytest

import topk_ref as ref
import test_gpu_topk as entry
from test_gpu_topk import SENTINEL, FILL, INT32_MAX, INT32_MIN, _up, _full, _stream, _sync, _ptr, _same, _identical

pytestmark = pytest.mark.gpu

TILE = 2048
STRAND1 = 0x40000000                                                    # the stranded searches' internal mark (csrc/pmx_common.h)


def records(scores, rng, flag_mask=0xFFFFFFFF):
    """[n, 4] int32: these scores, noise over all 32 bits in the other fields (flags under flag_mask), and [n, 3] statistics"""
    scores = np.asarray(scores).reshape(-1)
    n = len(scores)
    rec = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    rec[:, 3] &= np.uint32(flag_mask)
    rec = rec.view(np.int32)
    rec[:, 0] = scores
    st = rng.integers(0, 1 << 32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.int32)
    rec.setflags(write=False); st.setflags(write=False)
    return rec, st


class Dev:
    """records (and statistics) on the device, uploaded once per case"""
    def __init__(self, rec, st=None):
        self.rec, self.st = _up(rec.copy()), (_up(st.copy()) if st is not None else None)      # (copies: the originals are read-only)


def _hook(pkg, d, q_first, nq, nr, min_score, k, capacity, chunk=0, skip_self=False, marked=0, with_strand=False, with_pairs=True,
          with_index=True, with_passing=True):
    """one pmx_topk_records_device call into sentinel buffers laid out like test_gpu_topk._topk's -> its Got (+ .strand)"""
    import torch
    slots = capacity + 3
    hp = _full((slots * 32,), FILL, torch.uint8) if with_pairs else None
    hi = _full((slots,), SENTINEL, torch.int64) if with_index else None
    hr = _full((slots, 4), SENTINEL, torch.int32)
    hs = _full((slots, 3), SENTINEL, torch.int32) if d.st is not None else None
    sb = _full((slots,), FILL, torch.uint8) if with_strand else None
    off = _full((nq + 1 + 2,), SENTINEL, torch.int64)
    rp = _full((nq + 2,), SENTINEL, torch.int64) if with_passing else None
    cnt = _full((3 + 2,), SENTINEL, torch.int64)
    pkg.topk_records_device(d.rec.data_ptr(), _ptr(d.st), q_first, nq, nr, min_score, k, skip_self, chunk, marked, _ptr(sb), _ptr(hp), _ptr(hi),
                            hr.data_ptr(), _ptr(hs), capacity, off.data_ptr(), _ptr(rp), cnt.data_ptr(), _stream())
    _sync()
    g = entry.Got()
    host = lambda t: t.cpu().numpy() if t is not None else None
    g.pairs, g.index, g.recs, g.stats, g.off, g.passing, g.counts = host(hp), host(hi), host(hr), host(hs), host(off), host(rp), host(cnt)
    g.strand = host(sb)
    if g.pairs is not None:
        g.pairs = g.pairs.view(entry.pairs_ref.PAIR_DTYPE)
    g.all = [a for a in (g.pairs, g.index, g.recs, g.stats, g.off, g.passing, g.counts, g.strand) if a is not None]
    return g


def _check(pkg, d, rec, st, q_first, nq, nr, k, chunks, min_score=INT32_MIN, skip_self=False, capacity=None):
    """the hook at every chunk size against topk_ref.topk, and the runs against each other -> (the reference, the first run)"""
    full = ref.topk(rec, nr, q_first, nq, k, min_score, skip_self, stats=st)
    cap = int(full["row_off"][-1]) if capacity is None else capacity
    want = full if capacity is None else ref.topk(rec, nr, q_first, nq, k, min_score, skip_self, stats=st, capacity=cap)
    runs = [_hook(pkg, d, q_first, nq, nr, min_score, k, cap, chunk, skip_self) for chunk in chunks]
    for g in runs:
        _same(g, want, cap, nq)
    for g in runs[1:]:
        _identical(g, runs[0])
    return want, runs[0]


# ----------------------------------------------------------------------------------------------- 1. the hook runs the entry's kernels
def test_hook_equals_the_entry_on_the_entrys_own_records(pkg, orc):
    """7 x 300 alignments: pmx_search_topk_device, and the hook on the full entry's records of the same pairs under the same chunk
    sizes, byte for byte in every output buffer"""
    pm, om = entry._dna(pkg, orc)
    qseqs, rseqs = entry.sets7x300()
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    nq, nr = entry.NQ7, entry.NR300
    for want_stats in (0, pkg.WANT_STATS):
        cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, want_stats, pm.inner)
        rec, st, _, _ = entry._full_entry(pkg, cfg, Q, R, 0, nq, 60, 60)
        d = Dev(rec, st)
        ms = int(np.median(rec[:, 0]))
        for q_first, rows in ((0, nq), (2, 4)):
            sub = Dev(rec[q_first * nr:(q_first + rows) * nr], st[q_first * nr:(q_first + rows) * nr] if st is not None else None) if q_first else d
            for k, min_score, cap in ((1, INT32_MIN, rows), (65, ms, rows * 65), (65, ms, 40), (1024, INT32_MIN, rows * nr)):
                for chunk in (64, 192, 2048, 0):
                    a = entry._topk(pkg, cfg, Q, R, q_first, rows, 60, 60, min_score, k, cap, chunk)
                    b = _hook(pkg, sub, q_first, rows, nr, min_score, k, cap, chunk)
                    assert int(a.counts[0]) > 0
                    _identical(a, b)


# ------------------------------------------------------------------------------------------------------ 2. rows of more than 256 tiles
NR_BIG = 256 * TILE + 1                                                 # 257 tiles: the row kernel's second round of 256


def _big_scores(pattern):
    rng = np.random.default_rng(12000)
    j = np.arange(NR_BIG, dtype=np.int64)
    if pattern == "uniform":
        return rng.integers(INT32_MIN, INT32_MAX + 1, size=(2, NR_BIG), dtype=np.int64)
    if pattern == "ascending":                                          # every tile hands K survivors on; the last K of the row win
        return np.stack([INT32_MIN + 4095 * j, INT32_MIN + 4095 * j + 1])
    if pattern == "descending":                                         # nothing after the first tile beats the bound
        return np.stack([INT32_MAX - 4095 * j, INT32_MAX - 4095 * j - 1])
    return np.stack([np.full(NR_BIG, -5, dtype=np.int64), np.full(NR_BIG, INT32_MAX, dtype=np.int64)])


@pytest.fixture(scope="module")
def big():
    """per score pattern: records, statistics and their device copies, made once and left unchanged"""
    made = {}

    def get(pattern):
        if pattern not in made:
            rec, st = records(_big_scores(pattern), np.random.default_rng(12001))
            made.clear()                                                # (one pattern's 28 MB at a time)
            made[pattern] = (rec, st, Dev(rec, st))
        return made[pattern]
    return get


@pytest.mark.parametrize("k", [1, 1024])
@pytest.mark.parametrize("pattern", ["uniform", "ascending", "descending", "equal"])
def test_rows_of_more_than_256_tiles(pkg, big, pattern, k):
    """nr = 256 * 2048 + 1, two rows: one chunk per row (row 1 begins where its chunk does, one record past a tile edge of the
    stream) and chunks of 3 * 2048 + 17 (segments that start and end anywhere inside tiles)"""
    rec, st, d = big(pattern)
    want, g = _check(pkg, d, rec, st, 0, 2, NR_BIG, k, (NR_BIG, 3 * TILE + 17))
    assert want["row_off"].tolist() == [0, k, 2 * k] and want["row_passing"].tolist() == [NR_BIG] * 2
    first = want["pairs"]["r"][:k].tolist()
    if pattern == "ascending":
        assert first == list(range(NR_BIG - 1, NR_BIG - 1 - k, -1))     # the row's last K, from tile 256 and the end of tile 255
    if pattern in ("descending", "equal"):
        assert first == list(range(k))


# ------------------------------------------------------------------------------------------------------------- 3. collector sizes
def _kp(k):
    kp = 256
    while kp < k:
        kp <<= 1
    return kp


@pytest.mark.parametrize("k", [255, 256, 257, 511, 512, 513, 1023, 1024])
def test_collector_sizes(pkg, k):
    """2 KP slots, candidates 256 at a time: rows whose length puts `count + 256 > 2 KP` exactly at and one past the edge, and a row of
    eight tiles; ascending scores (every candidate enters, the list is replaced over and over) and a saw-tooth (a tooth of 300 rising
    scores, teeth that rise too: a row settles several times and the bound cuts into every later tooth)"""
    kp = _kp(k)
    rng = np.random.default_rng(12100 + k)
    for nr in (2 * kp - 256, 2 * kp - 255, 2 * kp, 2 * kp + 1, 8 * TILE):
        j = np.arange(nr, dtype=np.int64)
        for scores in (np.stack([j - 7, 3 * j, j // 2]), np.stack([(j % 300) * 1000 + j // 300, (j % 300) * 5 - j // 300, (j % 7) * 100 + j])):
            rec, st = records(scores, rng)
            d = Dev(rec, st)
            want, _ = _check(pkg, d, rec, st, 0, 3, nr, k, (0, nr, TILE + 300))
            assert want["row_off"].tolist() == [i * min(k, nr) for i in range(4)]


# -------------------------------------------------------------------------------------------------------------------- 4. key range
EDGE_SCORES = np.array([INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX], dtype=np.int64)


def edge_scores(rng, n, longest=400):
    """the seven edge values in tie runs of 1 .. `longest` records"""
    runs = rng.integers(1, longest + 1, size=n // 2 + 1)
    values = EDGE_SCORES[rng.integers(0, len(EDGE_SCORES), size=len(runs))]
    return np.repeat(values, runs)[:n]


@pytest.fixture(scope="module")
def edges():
    nq, nr = 3, 5000
    rec, st = records(edge_scores(np.random.default_rng(12200), nq * nr), np.random.default_rng(12201))
    return nq, nr, rec, st, Dev(rec, st)


@pytest.mark.parametrize("min_score", [INT32_MIN, 0, INT32_MAX])
def test_scores_at_the_ends_of_int32(pkg, edges, min_score):
    """keys whose high word is 0 (INT32_MIN) still beat the empty bound; at min_score = INT32_MIN every record passes and is kept up
    to K; at INT32_MAX only the records at INT32_MAX pass"""
    nq, nr, rec, st, d = edges
    score = rec[:, 0].reshape(nq, nr)
    assert all((score == v).any(axis=1).all() for v in EDGE_SCORES)
    for k in (1, 300, 1024):
        want, _ = _check(pkg, d, rec, st, 0, nq, nr, k, (0, 777), min_score)
        assert want["row_passing"].tolist() == (score >= min_score).sum(axis=1).tolist()
        if min_score == INT32_MIN:
            assert want["row_passing"].tolist() == [nr] * nq and np.diff(want["row_off"]).tolist() == [k] * nq
    low, _ = records(np.full(2 * 700, INT32_MIN), np.random.default_rng(12202))      # nothing but the lowest score: every key's high word is 0
    want, _ = _check(pkg, Dev(low), low, None, 0, 2, 700, 300, (0, 64), min_score)
    assert want["row_off"].tolist() == ([0, 300, 600] if min_score == INT32_MIN else [0, 0, 0])


def test_chunking_never_changes_a_byte(pkg, edges):
    nq, nr, rec, st, d = edges
    for k, ms in ((300, INT32_MIN), (1024, 0)):
        _check(pkg, d, rec, st, 0, nq, nr, k, (0, 777, nr, 2 * TILE + 1, 777, 0), ms)
        _check(pkg, d, rec, st, 0, nq, nr, k, (0, 777, 0), ms, capacity=k + 7)           # the capacity ends inside row 1


# -------------------------------------------------------------------------------------------------------------- 5. many short rows
@pytest.mark.parametrize("nr", [1, 2, 3])
def test_a_hundred_thousand_short_rows(pkg, nr):
    """the default chunk holds all of it: 100 000 row workgroups (and as many tile workgroups) in one launch"""
    nq = 100000
    rng = np.random.default_rng(12300 + nr)
    rec, st = records(rng.integers(-3, 4, size=nq * nr), rng)
    d = Dev(rec, st)
    for k, ms in ((1, INT32_MIN), (2, 0), (1024, INT32_MIN)):
        want, _ = _check(pkg, d, rec, st, 0, nq, nr, k, (0, 4099), ms)
        assert ms != INT32_MIN or np.diff(want["row_off"]).tolist() == [min(k, nr)] * nq
    if nr == 1:
        # the self pair of row i is j = i: with one column only row 0 has one, and loses it
        want, _ = _check(pkg, d, rec, st, 0, nq, 1, 5, (0, 4099), skip_self=True)
        assert want["row_off"][:3].tolist() == [0, 0, 1] and want["counts"][0] == nq - 1
        one = Dev(rec[:1], st[:1])
        want, _ = _check(pkg, one, rec[:1], st[:1], 0, 1, 1, 5, (0,), skip_self=True)     # every row is empty
        assert want["row_off"].tolist() == [0, 0] and want["counts"] == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------- 6. skip_self in late tiles
def test_skip_self_in_late_tiles(pkg):
    """nr = 3 * 2048 + 5: self pairs in tile 0, across the edge of tiles 0 and 1, in tiles 2 and 3 and at j = nr - 1, each the best score
    of its row by far"""
    nr = 3 * TILE + 5
    rng = np.random.default_rng(12400)
    for q_first, nq in ((3, 4), (TILE - 2, 4), (3 * TILE - 1, 6)):
        assert q_first + nq <= nr
        scores = rng.integers(-1000, 1000, size=(nq, nr))
        for li in range(nq):
            scores[li, q_first + li] = INT32_MAX
        rec, st = records(scores, rng)
        d = Dev(rec, st)
        for k in (1, 5, 1024):
            with_self, _ = _check(pkg, d, rec, st, q_first, nq, nr, k, (0, TILE, 1000))
            assert (with_self["pairs"]["r"][with_self["row_off"][:-1]] == q_first + np.arange(nq)).all()      # the self pair leads its row
            without, _ = _check(pkg, d, rec, st, q_first, nq, nr, k, (0, TILE, 1000), skip_self=True)
            assert (without["pairs"]["q"] != without["pairs"]["r"]).all() and without["row_passing"].tolist() == [nr - 1] * nq
            assert without["records"][:, 0].max() < 1000


# --------------------------------------------------------------------------------------------------------------- 7. the strand bit
def test_strand_bit_of_the_emit(pkg):
    """records that carry the stranded searches' mark at random: marked = 1 takes it out of the emitted flags and keeps every other
    bit, the strand bytes receive it; marked = 0 hands the flags back unchanged"""
    nq, nr, k = 5, 3000, 70
    rng = np.random.default_rng(12500)
    rec, st = records(rng.integers(-50, 50, size=nq * nr), rng)
    flags = rec[:, 3].view(np.uint32)
    assert 0.3 < (flags & STRAND1 != 0).mean() < 0.7 and len(np.unique(flags & ~np.uint32(STRAND1))) > nq * nr // 2
    d = Dev(rec, st)
    want = ref.topk(rec, nr, 0, nq, k, stats=st)
    h = nq * k
    bit = (want["records"][:, 3].view(np.uint32) & STRAND1 != 0).astype(np.uint8)
    assert 0 < bit.sum() < h
    cleared = dict(want)
    cleared["records"] = want["records"].copy()
    cleared["records"][:, 3] = (want["records"][:, 3].view(np.uint32) & ~np.uint32(STRAND1)).view(np.int32)
    runs = []
    for chunk in (0, 1000, 0):
        g = _hook(pkg, d, 0, nq, nr, INT32_MIN, k, h, chunk, marked=1, with_strand=True)
        _same(g, cleared, h, nq)
        assert g.strand[:h].tobytes() == bit.tobytes() and (g.strand[h:] == FILL).all()
        runs.append(g)
    _identical(runs[1], runs[0]); _identical(runs[2], runs[0])
    g = _hook(pkg, d, 0, nq, nr, INT32_MIN, k, h, 1000, marked=1)                          # no strand bytes asked for
    _same(g, cleared, h, nq)
    g = _hook(pkg, d, 0, nq, nr, INT32_MIN, k, h, 1000, marked=0, with_strand=True)        # unmarked: the flags as they came
    _same(g, want, h, nq)
    assert g.strand[:h].tobytes() == bit.tobytes() and (g.strand[h:] == FILL).all()
    cap = h - 33                                                                           # a capacity inside the last row
    g = _hook(pkg, d, 0, nq, nr, INT32_MIN, k, cap, 0, marked=1, with_strand=True)
    part = ref.topk(rec, nr, 0, nq, k, stats=st, capacity=cap)
    part["records"] = cleared["records"][:cap]
    _same(g, part, cap, nq)
    assert g.strand[:cap].tobytes() == bit[:cap].tobytes() and (g.strand[cap:] == FILL).all()


def test_optional_outputs_and_sub_ranges(pkg, edges):
    nq, nr, rec, st, d = edges
    sub = Dev(rec[nr:3 * nr])                                                             # rows 1 and 2, no statistics
    want = ref.topk(rec[nr:3 * nr], nr, 1, 2, 9, 0)
    assert want["pairs"]["q"].min() == 1 and want["index"].min() >= nr
    for with_pairs, with_index, with_passing in ((True, True, True), (False, True, False), (True, False, True), (False, False, False)):
        g = _hook(pkg, sub, 1, 2, nr, 0, 9, 18, 777, with_pairs=with_pairs, with_index=with_index, with_passing=with_passing)
        _same(g, want, 18, 2)
    g = _hook(pkg, sub, 1, 2, nr, 0, 9, 0, 777)                                            # capacity 0 counts
    _same(g, ref.topk(rec[nr:3 * nr], nr, 1, 2, 9, 0, capacity=0), 0, 2)
