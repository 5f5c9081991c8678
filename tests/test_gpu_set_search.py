"""Set search (`-m gpu`): pmx_search_pairs[_device] against the existing full entry on the same pairs (pmx_align_all_pairs_device, or
pmx_align_pairs_device on the descriptors tests/set_search_ref.py restates) filtered in numpy, and -- one case per shape -- against the
CPU oracle on the resolved strings.  Tile, wave and chunk boundaries of the compaction, capacity, the three shapes, bad descriptors,
kernel families and statistics, the host entry, the CIGAR pass over the hit pairs, the Python mirror.  Every comparison is exact;
every output buffer starts as a sentinel."""
import ctypes as C

import numpy as np
import pytest

import pairs_ref
import set_search_ref as ref
from util import random_seqs, mutate, AA, golden

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
INT32_MAX, INT32_MIN = ref.INT32_MAX, ref.INT32_MIN
LIST, TRI, RECT = ref.PAIRS_LIST, ref.PAIRS_TRIANGLE, ref.PAIRS_RECT


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


def _dna(pkg, orc):
    return pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)


def _b62(pkg, orc):
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _full_entry(pkg, cfg, Q, R, shape, first, n, pairs, mq, mr):
    """the yardstick: every record (and statistics row) of the enumeration's pairs from the entries that existed before, and the
    descriptors the enumeration stands for"""
    import torch
    stats = bool(cfg.want & pkg.WANT_STATS)
    descs = ref.descriptors(shape, len(Q), len(R if R is not None else Q), first, n, pairs)
    rec = _full((max(n, 1), 4), SENTINEL, torch.int32)
    st = _full((max(n, 1), 3), SENTINEL, torch.int32) if stats else None
    if shape == TRI:
        assert mq == mr
        pkg.align_all_pairs_device(cfg, Q, first, n, mq, rec.data_ptr(), _ptr(st), _stream())
    else:
        d_pairs = _up(descs.view(np.uint8))
        pkg.align_pairs_device(cfg, Q, R, n, d_pairs.data_ptr(), mq, mr, rec.data_ptr(), _ptr(st), _stream())
    kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    return rec.cpu().numpy()[:n], (st.cpu().numpy()[:n] if stats else None), descs, kernel


class Got:
    """outputs of one pmx_search_pairs_device call, whole buffers, on the host"""


def _search(pkg, cfg, Q, R, shape, first, n, pairs, mq, mr, min_score, capacity, chunk=0, with_pairs=True, with_index=True):
    import torch
    stats = bool(cfg.want & pkg.WANT_STATS)
    slots = capacity + 3                                                # (sentinel entries behind the capacity)
    hp = _full((slots * 32,), FILL, torch.uint8) if with_pairs else None
    hi = _full((slots,), SENTINEL, torch.int64) if with_index else None
    hr = _full((slots, 4), SENTINEL, torch.int32)
    hs = _full((slots, 3), SENTINEL, torch.int32) if stats else None
    cnt = _full((2,), SENTINEL, torch.int64)
    d_pairs = _up(np.ascontiguousarray(pairs).view(np.uint8)) if shape == LIST and n else None
    pkg.search_pairs_device(cfg, Q, R, shape, first, n, _ptr(d_pairs), mq, mr, min_score, _ptr(hp), _ptr(hi), hr.data_ptr(), _ptr(hs),
                            capacity, cnt.data_ptr(), _stream(), chunk)
    g = Got()
    g.kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    host = lambda t: t.cpu().numpy() if t is not None else None
    g.pairs, g.index, g.recs, g.stats, g.counts = host(hp), host(hi), host(hr), host(hs), host(cnt)
    if g.pairs is not None:
        g.pairs = g.pairs.view(pairs_ref.PAIR_DTYPE)
    g.d_pairs = hp
    return g


def _same(g, want, capacity):
    """counts in full, the first min(passing, capacity) entries equal to the reference's, every entry behind them the sentinel"""
    w = min(want["passing"], capacity)
    assert g.counts.tolist() == [want["passing"], w]
    assert g.recs[:w].tobytes() == want["records"][:w].tobytes() and (g.recs[w:] == SENTINEL).all()
    if g.index is not None:
        assert g.index[:w].tolist() == want["index"][:w].tolist() and (g.index[w:] == SENTINEL).all()
    if g.pairs is not None:
        assert g.pairs[:w].tobytes() == want["pairs"][:w].tobytes() and (g.pairs[w:].view(np.uint8) == FILL).all()
    if g.stats is not None:
        assert g.stats[:w].tobytes() == want["stats"][:w].tobytes() and (g.stats[w:] == SENTINEL).all()


def _oracle_check(pkg, orc, cfg, om, qseqs, rseqs, descs, recs, stats=None):
    """the yardstick itself against the CPU oracle on the resolved strings"""
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


# ------------------------------------------------------------------------------------- the set of cases 1 to 3: 91 sequences, 4095 pairs
N91 = 91
FAMILY = [k for k in range(76) if k != 5]          # row 0 from (0, 6) on: 70 hits in a row; row 5: 79 pairs without one, then its tail
TAIL = [5, 85, 86, 87, 88, 89, 90]                 # hits at the end of row 5 and in the last rows
T_FAMILY = 30                                      # between the best unrelated pair and the worst pair of a family


def set91():
    rng = np.random.default_rng(9100)
    seqs = random_seqs(rng, N91, 20, 60)
    base, tail = random_seqs(rng, 1, 50, 50)[0], random_seqs(rng, 1, 60, 60)[0]
    for k in FAMILY:
        seqs[k] = mutate(rng, base, 0.05, 0.01)
    for k in TAIL:
        seqs[k] = mutate(rng, tail[:56], 0.05, 0.01)                   # (at most 112 against the tail itself)
    seqs[89] = tail
    seqs[90] = tail                                                     # the one identical pair of 60: the single best score
    assert all(20 <= len(s) <= 60 for s in seqs)
    return seqs


@pytest.fixture(scope="module")
def case91(pkg, orc):
    """the set, the yardstick's records of all 4095 pairs (checked against the oracle once), shared and left unchanged"""
    pm, om = _dna(pkg, orc)
    seqs = set91()
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    S = pkg.SeqSet.new(seqs)
    total = pairs_ref.all_pairs_count(N91)
    assert total == 4095
    recs, _, descs, kernel = _full_entry(pkg, cfg, S, None, TRI, 0, total, None, 60, 60)
    _oracle_check(pkg, orc, cfg, om, seqs, seqs, descs, recs)
    recs.setflags(write=False)
    return pm, cfg, S, seqs, recs, descs, kernel


def test_triangle_across_tile_and_wave_boundaries(pkg, case91):
    pm, cfg, S, seqs, recs, descs, kernel = case91
    total, score = len(recs), np.sort(recs[:, 0])
    assert score[-1] == 120 and score[-2] < 120                                         # one best pair
    fam = np.array([int(d["q"]) in FAMILY and int(d["r"]) in FAMILY for d in descs])
    assert recs[fam, 0].min() >= T_FAMILY > recs[~fam & (recs[:, 0] < 60), 0].max()
    levels = {"none": INT32_MAX, "one": 120, "1%": int(score[-41]), "50%": int(score[total // 2]), "all": INT32_MIN}
    for name, ms in levels.items():
        want = ref.hits(recs, ms, 0, descs)
        if name == "none":
            assert want["passing"] == 0
        if name == "one":
            assert want["passing"] == 1 and want["index"].tolist() == [total - 1]
        if name == "1%":
            assert 41 <= want["passing"] <= 200                                         # (the ties at the 41st best score pass too)
        if name == "50%":
            assert total // 2 <= want["passing"] <= total * 6 // 10
            k = want["index"]                                                           # hits on both sides of the 2048-record tile,
            assert (k < 2048).any() and (k >= 2048).any()                               # of a 256-thread step and of a wave
            assert len(set(k // 256)) >= 12 and len(set(k // 64)) >= 40
        g = _search(pkg, cfg, S, None, TRI, 0, total, None, 60, 60, ms, total)
        assert g.kernel == kernel
        _same(g, want, total)
        if name == "all":
            assert g.recs[:total].tobytes() == recs.tobytes() and g.pairs[:total].tobytes() == descs.tobytes()
            assert g.index[:total].tolist() == list(range(total))
    g = _search(pkg, cfg, S, S, TRI, 0, total, None, 60, 60, levels["1%"], total)       # R == Q is the same triangle
    _same(g, ref.hits(recs, levels["1%"], 0, descs), total)


# the window of the chunking and capacity cases: from (0, 6) -- 64 family pairs, the whole first chunk of 64 -- to the middle of row 9
W_FIRST, W_N = 5, 64 * 13 + 1


def test_chunking_never_changes_a_byte(pkg, case91):
    pm, cfg, S, seqs, recs, descs, kernel = case91
    assert pairs_ref.row_start(N91, 9) < W_FIRST + W_N < pairs_ref.row_start(N91, 10)    # the window ends inside a row
    win, wdesc = recs[W_FIRST:W_FIRST + W_N], descs[W_FIRST:W_FIRST + W_N]
    want = ref.hits(win, T_FAMILY, W_FIRST, wdesc)
    per_chunk = [int((win[c:c + 64, 0] >= T_FAMILY).sum()) for c in range(0, W_N, 64)]
    assert per_chunk[0] == 64 and per_chunk[7] == 0 and per_chunk[6] > 0 and per_chunk[8] > 0 and per_chunk[-1] == 1
    runs = []
    for chunk in (64, 192, 2048, 0, 64):
        g = _search(pkg, cfg, S, None, TRI, W_FIRST, W_N, None, 60, 60, T_FAMILY, W_N, chunk)
        _same(g, want, W_N)
        runs.append(g)
    for g in runs[1:]:
        for a, b in ((g.recs, runs[0].recs), (g.pairs, runs[0].pairs), (g.index, runs[0].index), (g.counts, runs[0].counts)):
            assert a.tobytes() == b.tobytes()
    cfg_s = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)                                 # statistics travel with their hits
    frec, fst, _, _ = _full_entry(pkg, cfg_s, S, None, TRI, W_FIRST, W_N, None, 60, 60)
    for chunk in (64, 0):
        _same(_search(pkg, cfg_s, S, None, TRI, W_FIRST, W_N, None, 60, 60, T_FAMILY, W_N, chunk), ref.hits(frec, T_FAMILY, W_FIRST, wdesc, fst), W_N)


def test_capacity(pkg, case91):
    pm, cfg, S, seqs, recs, descs, kernel = case91
    win, wdesc = recs[W_FIRST:W_FIRST + W_N], descs[W_FIRST:W_FIRST + W_N]
    passing = ref.hits(win, T_FAMILY)["passing"]
    assert passing > 200
    # 64: the running total reaches it exactly at the end of the first chunk of 64; 70: it crosses it inside the second
    for cap in (0, 1, passing - 1, passing, passing + 5, 64, 70):
        for chunk in (64, 0):
            g = _search(pkg, cfg, S, None, TRI, W_FIRST, W_N, None, 60, 60, T_FAMILY, cap, chunk)
            _same(g, ref.hits(win, T_FAMILY, W_FIRST, wdesc, capacity=cap), cap)
    for with_pairs, with_index in ((False, True), (True, False), (False, False)):
        g = _search(pkg, cfg, S, None, TRI, W_FIRST, W_N, None, 60, 60, T_FAMILY, 70, 64, with_pairs, with_index)
        assert (g.pairs is None) == (not with_pairs) and (g.index is None) == (not with_index)
        _same(g, ref.hits(win, T_FAMILY, W_FIRST, wdesc, capacity=70), 70)
    import torch
    cnt = _full((2,), SENTINEL, torch.int64)                                              # capacity 0 with no hit buffer at all: counting
    pkg.search_pairs_device(cfg, S, None, TRI, W_FIRST, W_N, None, 60, 60, T_FAMILY, None, None, None, None, 0, cnt.data_ptr(), _stream(), 64)
    _sync()
    assert cnt.cpu().tolist() == [passing, 0]
    pkg.search_pairs_device(cfg, S, None, TRI, W_FIRST, 0, None, 60, 60, T_FAMILY, None, None, None, None, 0, cnt.data_ptr(), _stream(), 64)
    _sync()
    assert cnt.cpu().tolist() == [0, 0]                                                   # n == 0 writes zero counts


# ------------------------------------------------------------------------------------------------------------------ 4. rectangle
@pytest.fixture(scope="module")
def rect_sets():
    rng = np.random.default_rng(9400)
    rseqs = random_seqs(rng, 300, 20, 60)
    for k in (0, 150, 299):
        rseqs[k] = random_seqs(rng, 1, 60, 60)[0]
    qseqs = [mutate(rng, rseqs[k], 0.05, 0.01)[:60] for k in (0, 150, 299)] + random_seqs(rng, 4, 20, 60)
    qseqs = [s if len(s) >= 20 else s + b"ACGT" * 5 for s in qseqs]
    return qseqs, rseqs


@pytest.mark.parametrize("shape", ["1x1", "1x300", "300x1", "7x300", "QxQ"])
def test_rectangle(pkg, orc, rect_sets, shape):
    pm, om = _dna(pkg, orc)
    q7, r300 = rect_sets
    qseqs, rseqs, windows = {"1x1": (q7[:1], r300[:1], [(0, 1)]),
                             "1x300": (q7[:1], r300, [(0, 300), (17, 200)]),
                             "300x1": (r300, q7[1:2], [(0, 300), (3, 290)]),
                             "7x300": (q7, r300, [(0, 2100), (150, 1801), (299, 2), (1799, 301)]),
                             "QxQ": (r300[:40], None, [(0, 1600), (35, 1530)])}[shape]
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    Q = pkg.SeqSet.new(qseqs)
    R = pkg.SeqSet.new(rseqs) if rseqs is not None else Q
    rs = rseqs if rseqs is not None else qseqs
    nq, nr = len(qseqs), len(rs)
    assert pkg.rect_pairs_count(nq, nr) == nq * nr
    for first, n in windows:
        recs, _, descs, kernel = _full_entry(pkg, cfg, Q, R, RECT, first, n, None, 60, 60)
        if first == 0:
            _oracle_check(pkg, orc, cfg, om, qseqs, rs, descs, recs)
            if shape == "QxQ":                                                            # the diagonal is there: a sequence against itself
                diag = np.nonzero(descs["q"] == descs["r"])[0]
                assert len(diag) == 40 and (recs[diag, 0] == 2 * np.array([len(s) for s in qseqs])).all()
        for ms in (INT32_MIN, 24, 60, INT32_MAX):
            for chunk in (0, 64):
                g = _search(pkg, cfg, Q, R, RECT, first, n, None, 60, 60, ms, n, chunk)
                assert chunk or g.kernel == kernel                                        # (the same chunks: the same alignment kernel)
                _same(g, ref.hits(recs, ms, first, descs), n)
        if shape == "7x300" and first == 0:
            hit60 = ref.hits(recs, 60, 0, descs)                                          # the planted relatives are found where they are
            assert {(0, 0), (1, 150), (2, 299)} <= {(int(p["q"]), int(p["r"])) for p in hit60["pairs"]}


def test_rect_enumerator_at_three_billion_squared(pkg):
    import torch
    n = 3 * 10 ** 9
    total = pkg.rect_pairs_count(n, n)
    assert total == n * n
    rng = np.random.default_rng(9450)
    row = int(rng.integers(1, n - 1))
    for first in (0, total - 4096, row * n - 2048, (n - 1) * n - 5, (1 << 31) * n - 100):
        d = _full((4096 * 32,), FILL, torch.uint8)
        pkg.rect_pairs_enumerate_device(n, n, first, 4096, d.data_ptr(), _stream())
        _sync()
        got = d.cpu().numpy().view(pairs_ref.PAIR_DTYPE)
        want = np.zeros(4096, dtype=pairs_ref.PAIR_DTYPE)
        want["q"] = [(first + k) // n for k in range(4096)]
        want["r"] = [(first + k) % n for k in range(4096)]
        want["q_len"] = -1
        want["r_len"] = -1
        assert got.tobytes() == want.tobytes(), first
    small = _full((5 * 32,), FILL, torch.uint8)                                           # the hook agrees with the restatement
    pkg.rect_pairs_enumerate_device(7, 3, 4, 5, small.data_ptr(), _stream())
    _sync()
    assert small.cpu().numpy().tobytes() == ref.rect_pairs_descriptors(3, 4, 5).tobytes()


# ------------------------------------------------------------------------------------------------------------------------ 5. list
def test_list_with_windows_reuse_and_a_bad_descriptor(pkg, orc):
    rng = np.random.default_rng(9500)
    pm, om = _dna(pkg, orc)
    refs = random_seqs(rng, 12, 90, 120)
    reads = [mutate(rng, r[20:75], 0.05, 0.01) for r in refs]
    rows = [(k % 12, k % 12, 0, -1, 10, 70) for k in range(60)]                                       # a read against its place, reused
    rows += [(int(rng.integers(12)), int(rng.integers(12)), int(rng.integers(0, 10)), 30, int(rng.integers(0, 40)), 50) for _ in range(150)]
    rows += [(3, 7), (3, 7), (3, 3, 5, 20, 25, 20)]
    good = pairs_ref.pairs_array(rows)
    bad_at = 100
    pairs = np.concatenate([good[:bad_at], pairs_ref.pairs_array([(12, 0)]), good[bad_at:]])          # index outside the set
    n = len(pairs)
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new(refs)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    recs, st, descs, kernel = _full_entry(pkg, cfg, Q, R, LIST, 0, n, pairs, 60, 120)
    assert recs[bad_at].tolist() == list(pairs_ref.BAD_RECORD) and st[bad_at].tolist() == [0, 0, 0]
    keep = np.arange(n) != bad_at
    _oracle_check(pkg, orc, cfg, om, reads, refs, pairs[keep], recs[keep], st[keep])
    for ms in (0, 1, 50, INT32_MIN):
        want = ref.hits(recs, ms, 0, pairs, st)
        assert (bad_at in want["index"]) == (ms <= 0)                                                 # a hit at 0, flag kept; none at 1
        for chunk in (0, 64):
            g = _search(pkg, cfg, Q, R, LIST, 0, n, pairs, 60, 120, ms, n, chunk)
            _same(g, want, n)
            if ms <= 0:
                x = want["index"].tolist().index(bad_at)
                assert g.recs[x].tolist() == list(pairs_ref.BAD_RECORD) and g.pairs[x].tobytes() == pairs[bad_at].tobytes()
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    with pytest.raises(pkg.BatchError, match=r"pair 100: query: index outside"):
        al.search_pairs(Q, R, min_score=50, pairs=pairs)
    h = al.search_pairs(Q, R, min_score=50, pairs=pairs[keep], stats=True)
    want = ref.hits(recs[keep], 50, 0, pairs[keep], st[keep])
    assert h.n_passing == want["passing"] == h.n_hits and h.records.tobytes() == want["records"].tobytes()
    assert h.pairs.tobytes() == want["pairs"].tobytes() and h.index.tolist() == want["index"].tolist() and h.stats.tobytes() == want["stats"].tobytes()


# ------------------------------------------------------------------------------------------- 6. kernel families and statistics
def _family(pkg, orc, cfg, om, seqs, ms_levels, kernel, max_len=60):
    S = pkg.SeqSet.new(seqs)
    total = pairs_ref.all_pairs_count(len(seqs))
    first, n = 3, total - 7
    recs, st, descs, name = _full_entry(pkg, cfg, S, None, TRI, first, n, None, max_len, max_len)
    assert name.startswith(kernel[0]) and kernel[1] in name, name
    _oracle_check(pkg, orc, cfg, om, seqs, seqs, descs, recs, st)
    for ms in ms_levels:
        want = ref.hits(recs, ms, first, descs, st)
        assert 0 < want["passing"] < n
        for chunk in (0, 128):
            g = _search(pkg, cfg, S, None, TRI, first, n, None, max_len, max_len, ms, n, chunk)
            assert chunk or g.kernel == name                                              # (the same chunks: the same alignment kernel)
            _same(g, want, n)
    return S, recs, descs


def _related(rng, n, lo, hi, alphabet, sub, indel):
    seqs = random_seqs(rng, n, lo, hi, alphabet)
    for k in range(0, n, 4):
        seqs[k] = mutate(rng, seqs[(k + 7) % n], sub, indel, alphabet)[:hi]
        if len(seqs[k]) < lo:
            seqs[k] = seqs[(k + 7) % n]
    return seqs


def test_local_dna(pkg, orc):
    pm, om = _dna(pkg, orc)
    # 93 sequences: 4 271 pairs in one chunk, past the 4 096 from which the perm-table form of pmx_sw16_kernel runs
    seqs = _related(np.random.default_rng(9600), 93, 20, 60, np.frombuffer(b"ACGT", dtype=np.uint8), 0.05, 0.01)
    _family(pkg, orc, pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner), om, seqs, (30,), ("pmx_sw16_kernel", "permtable"))


def test_local_protein_blosum62(pkg, orc):
    pm, om = _b62(pkg, orc)
    # 70 sequences: 2 408 pairs in one chunk, past the 2 048 from which per-pair queries over a large alphabet take pmx_sw16m_kernel
    seqs = _related(np.random.default_rng(9610), 70, 20, 60, AA, 0.2, 0.02)
    _family(pkg, orc, pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, pm.inner), om, seqs, (40,), ("pmx_sw16m_kernel", "matrix lookup"))


def test_global_with_a_negative_threshold(pkg, orc):
    pm, om = _dna(pkg, orc)
    seqs = _related(np.random.default_rng(9620), 40, 20, 60, np.frombuffer(b"ACGT", dtype=np.uint8), 0.05, 0.01)
    _family(pkg, orc, pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 0, 0, pm.inner), om, seqs, (-40, 0), ("pmx_nwsg16", ""))


def test_semi_global_with_statistics_and_sorted(pkg, orc):
    pm, om = _dna(pkg, orc)
    seqs = _related(np.random.default_rng(9630), 40, 20, 60, np.frombuffer(b"ACGT", dtype=np.uint8), 0.05, 0.01)
    cfg = pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    S, recs, descs = _family(pkg, orc, cfg, om, seqs, (25,), ("pmx_stats16", ""))
    plain = pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, 0, pm.inner)
    srt = pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, pkg.WANT_SORTED, pm.inner)                                  # passed on: the same hits
    n = len(recs)
    a = _search(pkg, plain, S, None, TRI, 3, n, None, 60, 60, 25, n)
    b = _search(pkg, srt, S, None, TRI, 3, n, None, 60, 60, 25, n, 128)
    _same(a, ref.hits(recs, 25, 3, descs), n)
    _same(b, ref.hits(recs, 25, 3, descs), n)


# ----------------------------------------------------------------------------------------------------------------- 7. host entry
def _host(pkg, cfg, Q, R, shape, first, n, pairs, ms, max_hits=0, chunk=0, sl=0):
    res = C.POINTER(pkg.pmx_pair_hits_t)()
    o = pkg.pmx_pair_search_opts_t(ms, shape, max_hits, chunk, sl)
    rc = pkg.lib.pmx_search_pairs(C.byref(cfg), Q.inner, R.inner if R is not None else None, first, n,
                                  pairs.ctypes.data if pairs is not None else None, C.byref(o), C.byref(res))
    assert rc == 0, pkg.lib.pmx_last_error()
    try:
        return pkg.PairHits(res.contents)
    finally:
        pkg.lib.pmx_pair_hits_free(res)


def _same_host(h, want, passing):
    assert h.n_passing == passing and h.n_hits == want["written"]
    assert h.records.tobytes() == want["records"].tobytes() and h.pairs.tobytes() == want["pairs"].tobytes()
    assert h.index.tolist() == want["index"].tolist()
    if want["stats"] is not None:
        assert h.stats.tobytes() == want["stats"].tobytes()


def test_host_entry(pkg, case91):
    pm, cfg, S, seqs, recs, descs, kernel = case91
    win, wdesc = recs[W_FIRST:W_FIRST + W_N], descs[W_FIRST:W_FIRST + W_N]
    want = ref.hits(win, T_FAMILY, W_FIRST, wdesc)
    for sl, chunk in ((64, 0), (1000, 64), (0, 0), (64, 7)):
        _same_host(_host(pkg, cfg, S, None, TRI, W_FIRST, W_N, None, T_FAMILY, 0, chunk, sl), want, want["passing"])
    for max_hits in (1, 64, 70, want["passing"], want["passing"] + 9):                    # cut in enumeration order, counting goes on
        cut = ref.hits(win, T_FAMILY, W_FIRST, wdesc, capacity=max_hits)
        for sl in (64, 0):
            _same_host(_host(pkg, cfg, S, None, TRI, W_FIRST, W_N, None, T_FAMILY, max_hits, 0, sl), cut, want["passing"])
    none = _host(pkg, cfg, S, None, TRI, W_FIRST, W_N, None, INT32_MAX, 0, 0, 64)
    assert none.n_hits == 0 and none.n_passing == 0 and len(none.records) == 0 and len(none.pairs) == 0
    cfg_s = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    frec, fst, _, _ = _full_entry(pkg, cfg_s, S, None, TRI, W_FIRST, W_N, None, 60, 60)
    wst = ref.hits(frec, T_FAMILY, W_FIRST, wdesc, fst)
    _same_host(_host(pkg, cfg_s, S, None, TRI, W_FIRST, W_N, None, T_FAMILY, 0, 0, 100), wst, wst["passing"])
    # wrapped sets: maxima and validation on the device
    buf, off = pkg.pack(seqs)
    d_buf, d_off = _up(np.concatenate([np.zeros(3, dtype=np.uint8), buf])), _up(off)
    W = pkg.SeqSet.wrap_device(d_buf.data_ptr() + 3, d_off.data_ptr(), len(seqs), len(buf), keep=(d_buf, d_off))
    _same_host(_host(pkg, cfg, W, None, TRI, W_FIRST, W_N, None, T_FAMILY, 0, 0, 64), want, want["passing"])
    rwant = ref.hits(*_full_entry(pkg, cfg, S, S, RECT, 100, 700, None, 60, 60)[:1], T_FAMILY, 100, ref.rect_pairs_descriptors(N91, 100, 700))
    _same_host(_host(pkg, cfg, W, S, RECT, 100, 700, None, T_FAMILY, 0, 0, 256), rwant, rwant["passing"])
    lp = wdesc[::3].copy()
    lwant = ref.hits(win[::3], T_FAMILY, 0, lp)
    _same_host(_host(pkg, cfg, W, W, LIST, 0, len(lp), lp, T_FAMILY, 0, 0, 50), lwant, lwant["passing"])
    broken = lp.copy(); broken[123]["r"] = N91
    o = pkg.pmx_pair_search_opts_t(INT32_MAX, LIST, 0, 0, 50)                             # refused though it could never be a hit
    res = C.POINTER(pkg.pmx_pair_hits_t)()
    assert pkg.lib.pmx_search_pairs(C.byref(cfg), W.inner, W.inner, 0, len(lp), broken.ctypes.data, C.byref(o), C.byref(res)) == -1
    assert "pair 123" in pkg.lib.pmx_last_error().decode() and not res
    holes = list(seqs); holes[7] = b""                                                    # RECT names the first pair like the all-pairs entry
    H = pkg.SeqSet.new(holes)
    o = pkg.pmx_pair_search_opts_t(0, RECT, 0, 0, 0)
    assert pkg.lib.pmx_search_pairs(C.byref(cfg), S.inner, H.inner, 3, 100, None, C.byref(o), C.byref(res)) == -1
    assert "pair 4 (0, 7): reference: empty window" in pkg.lib.pmx_last_error().decode()
    assert pkg.lib.pmx_search_pairs(C.byref(cfg), H.inner, S.inner, 7 * N91 - 2, 100, None, C.byref(o), C.byref(res)) == -1
    assert "pair 2 (7, 0): query: empty window" in pkg.lib.pmx_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- 8. composition
def test_hit_pairs_feed_the_cigar_entry_unchanged(pkg, orc, case91):
    import torch
    pm, cfg, S, seqs, recs, descs, kernel = case91
    om = _dna(pkg, orc)[1]
    g = _search(pkg, cfg, S, None, TRI, W_FIRST, W_N, None, 60, 60, T_FAMILY, W_N, 64)
    h = int(g.counts[1])
    assert h > 200
    ccfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_CIGAR, pm.inner)
    capacity = 64 * h
    rec = _full((h, 4), SENTINEL, torch.int32)
    beg = _full((h, 2), SENTINEL, torch.int32)
    text = _full((capacity,), FILL, torch.uint8)
    off = _full((h + 1,), -9, torch.int64)
    pkg.align_pairs_ex_device(ccfg, S, S, h, g.d_pairs.data_ptr(), None, 60, 60, rec.data_ptr(), None, beg.data_ptr(), text.data_ptr(),
                              capacity, off.data_ptr(), _stream(), 100)                  # the device hit list itself, nothing in between
    _sync()
    rec, beg, text, off = rec.cpu().numpy(), beg.cpu().numpy(), text.cpu().numpy(), off.cpu().numpy()
    assert rec.tobytes() == g.recs[:h].tobytes()                                          # score and end positions of the hit records
    assert 0 < off[h] <= capacity
    strings = pairs_ref.resolve(seqs, seqs, g.pairs[:h])
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    res, malformed = orc.rescore_cigars(text[:off[h]], off, qb, qo, rb, ro, 5, 2, om, beg=beg.reshape(-1), free_mask=0)
    assert malformed == 0 and (res[:, 0] == rec[:, 0]).all() and (res[:, 3] == 0).all()


# --------------------------------------------------------------------------------------------------------------------- 9. Python
def test_python_search_pairs_three_shapes(pkg, case91):
    pm, cfg, S, seqs, recs, descs, kernel = case91
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    total = len(recs)
    h = al.search_pairs(S, min_score=T_FAMILY)
    _same_host(h, ref.hits(recs, T_FAMILY, 0, descs), ref.hits(recs, T_FAMILY)["passing"])
    assert h.stats is None and len(h) == h.n_hits
    h = al.search_pairs(S, min_score=T_FAMILY, first=W_FIRST, count=W_N, max_hits=70, chunk_pairs=64, slice_pairs=200)
    win, wdesc = recs[W_FIRST:W_FIRST + W_N], descs[W_FIRST:W_FIRST + W_N]
    _same_host(h, ref.hits(win, T_FAMILY, W_FIRST, wdesc, capacity=70), ref.hits(win, T_FAMILY)["passing"])
    Q = pkg.SeqSet.new(seqs[85:] + seqs[:3])
    qn = len(seqs[85:]) + 3
    rrec, rst, rdesc, _ = _full_entry(pkg, pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner), Q, S, RECT, 0, qn * N91, None, 60, 60)
    h = al.search_pairs(Q, S, min_score=T_FAMILY, stats=True)
    want = ref.hits(rrec, T_FAMILY, 0, rdesc, rst)
    _same_host(h, want, want["passing"])
    assert (5, 89) in {(int(p["q"]), int(p["r"])) for p in h.pairs}                        # Q[5] is S[90], the copy of S[89]
    h = al.search_pairs(Q, S, min_score=T_FAMILY, first=50, count=300, slice_pairs=128)
    want = ref.hits(_full_entry(pkg, cfg, Q, S, RECT, 50, 300, None, 60, 60)[0], T_FAMILY, 50, rdesc[50:350])
    _same_host(h, want, want["passing"])
    lp = [(int(d["q"]), int(d["r"])) for d in descs[::5]]
    h = al.search_pairs(S, min_score=T_FAMILY, pairs=lp)
    want = ref.hits(recs[::5], T_FAMILY, 0, descs[::5].copy())
    _same_host(h, want, want["passing"])
    assert total == 4095
