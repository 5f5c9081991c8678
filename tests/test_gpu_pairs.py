"""Sequence-set batches (`-m gpu`): pmx_align_pairs / _device and pmx_align_all_pairs / _device against BOTH the CPU oracle on the
strings tests/pairs_ref.py resolves and pmx_align_batch_device on the same pairs packed by numpy (whole records, statistics where
asked).  Gather geometry at every source and destination alignment, one case per kernel family, reuse, chunking, bad descriptors,
all-vs-all windows, the enumerator at 2^31 - 1 sequences, wrapped sets, repeatability.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import pairs_ref
from util import random_seqs, mutate, AA, golden

pytestmark = pytest.mark.gpu

NMAX = (1 << 31) - 1
SENTINEL = -77


def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _up_pairs(pairs):
    return _up(np.ascontiguousarray(pairs).view(np.uint8))


def _outputs(n, stats):
    import torch
    rec = torch.full((max(n, 1), 4), SENTINEL, dtype=torch.int32, device=_dev())
    st = torch.full((max(n, 1), 3), SENTINEL, dtype=torch.int32, device=_dev()) if stats else None
    return rec, st


def _fetch(rec, st, n):
    import torch
    torch.cuda.synchronize()
    return rec.cpu().numpy()[:n], (st.cpu().numpy()[:n] if st is not None else None)


def _pairs_device(pkg, cfg, Q, R, pairs, mq, mr, chunk=0):
    n = len(pairs)
    stats = bool(cfg.want & pkg.WANT_STATS)
    rec, st = _outputs(n, stats)
    d_pairs = _up_pairs(pairs) if n else None
    pkg.align_pairs_device(cfg, Q, R, n, d_pairs.data_ptr() if n else None, mq, mr, rec.data_ptr(), st.data_ptr() if stats else None,
                           _stream(), chunk)
    return _fetch(rec, st, n)


def _batch_device(pkg, cfg, strings, mq=None, mr=None):
    """pmx_align_batch_device on the pairs spelled out back to back -- the path the engine had before"""
    n = len(strings)
    stats = bool(cfg.want & pkg.WANT_STATS)
    qb, qo = pkg.pack([s[0] for s in strings]); rb, ro = pkg.pack([s[1] for s in strings])
    pad = np.zeros(16, dtype=np.uint8)
    dq, dr, dqo, dro = _up(np.concatenate([qb, pad])), _up(np.concatenate([rb, pad])), _up(qo), _up(ro)
    rec, st = _outputs(n, stats)
    mq = mq or int(np.diff(qo).max()); mr = mr or int(np.diff(ro).max())
    pkg.align_batch_device(cfg, n, dq.data_ptr(), dqo.data_ptr(), dr.data_ptr(), dro.data_ptr(), mq, mr, rec.data_ptr(),
                           st.data_ptr() if stats else None, _stream())
    return _fetch(rec, st, n)


def _oracle(orc, cfg, om, strings, stats=False):
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    sg = cfg.sg_flags if cfg.mode == 1 else orc.SG_ALL
    if stats:
        return orc.align_stats_sample(cfg.mode, np.arange(len(strings)), qb, qo, rb, ro, cfg.open, cfg.extend, om, sg_flags=sg, bits=cfg.width)
    return orc.align_batch(cfg.mode, qb, qo, rb, ro, cfg.open, cfg.extend, om, sg_flags=sg, bits=cfg.width)


def _check(pkg, orc, cfg, om, qseqs, rseqs, pairs, got, got_stats=None):
    """records of a set batch == oracle on the resolved strings == pmx_align_batch_device on the packed strings"""
    strings = pairs_ref.resolve(qseqs, rseqs, pairs)
    assert all(s is not None for s in strings)
    stats = bool(cfg.want & pkg.WANT_STATS)
    want = _oracle(orc, cfg, om, strings, stats)
    bad = np.nonzero((got[:, :3] != want[:, :3]).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    direct, direct_stats = _batch_device(pkg, cfg, strings)
    assert got.tobytes() == direct.tobytes()
    if stats:
        assert (got_stats == want[:, 3:6]).all()
        assert got_stats.tobytes() == direct_stats.tobytes()
    return direct


def _dna(pkg, orc):
    return pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)


def _b62(pkg, orc):
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))


# --------------------------------------------------------------------------------------------------------- 1. gather geometry
LENS = list(range(1, 10)) + [15, 16, 17, 63, 64, 65, 255]


def test_gather_geometry_every_alignment(pkg, orc):
    """windows at every source offset mod 4 and every length class, packed at every destination offset mod 4; half of them against
    a copy of the same bytes at another alignment (a wrong byte on either side lowers the score below 2 L)"""
    rng = np.random.default_rng(7100)
    pm, om = _dna(pkg, orc)
    base = random_seqs(rng, 4, 300, 300)
    seqs = [base[0], base[1] + b"A", base[2] + b"AC", base[3] + b"ACG"]                  # offsets 0, 300, 601, 903: residues 0, 0, 1, 3
    seqs += [b"G" * (k + 1) + base[k] for k in range(4)]                                 # the same bytes, shifted by 1 .. 4
    seqs.append(random_seqs(rng, 1, 7, 7)[0])                                            # the last sequence of the set
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    rows = [(0, len(seqs) - 1, 0, 5, 2, 5),                                              # the first bytes of the first sequence,
            (len(seqs) - 1, 0, 3, 4, 100, -1),                                           # the last bytes of the last one, len = -1
            (len(seqs) - 1, len(seqs) - 1, 0, -1, 4, -1)]
    for k in range(4):
        for a in range(4):
            for x, L in enumerate(LENS):
                beg = a + 4 * ((x + k) % 9)
                rows.append((k, k + 4, beg, L, k + 1 + beg, L))                           # identical bytes, another alignment
                rows.append((k + 4, (k + 1) % 4, beg, L, (a + x) % 7, LENS[(x + 5) % len(LENS)]))
    rows = [rows[i] for i in rng.permutation(len(rows))]                                 # (destination offsets of every residue)
    pairs = pairs_ref.pairs_array(rows)
    src = {(int(off[p["q"]] + p["q_beg"]) % 4, int(p["q_len"])) for p in pairs} | {(int(off[p["r"]] + p["r_beg"]) % 4, int(p["r_len"])) for p in pairs}
    assert all((a, L) in src for a in range(4) for L in LENS)
    strings = pairs_ref.resolve(seqs, seqs, pairs)
    dst = {(int(o) % 4, len(s[0])) for o, s in zip(np.cumsum([0] + [len(s[0]) for s in strings]), strings)}
    assert all((a, L) in dst for a in range(4) for L in LENS)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    S = pkg.SeqSet.new(seqs)
    assert len(S) == len(seqs)
    got, _ = _pairs_device(pkg, cfg, S, S, pairs, 300, 300)
    _check(pkg, orc, cfg, om, seqs, seqs, pairs, got)
    same = np.array([r[0] + 4 == r[1] and r[3] == r[5] for r in rows])
    assert same.sum() == 4 * 4 * len(LENS) and (got[same, 0] == 2 * pairs["q_len"][same]).all()
    for chunk in (7, 64):                                                                # destinations restart at every chunk
        again, _ = _pairs_device(pkg, cfg, S, S, pairs, 300, 300, chunk)
        assert again.tobytes() == got.tobytes()
    one = pkg.SeqSet.new([b"A"])                                                         # a set of one 1-byte sequence
    got1, _ = _pairs_device(pkg, cfg, one, one, pairs_ref.pairs_array([(0, 0), (0, 0, 0, 1, 0, -1)]), 1, 1)
    assert got1.tolist() == [[2, 0, 0, 0], [2, 0, 0, 0]]


# --------------------------------------------------------------------------------------------------------- 2. kernel families
def _family_case(pkg, orc, cfg, pm, om, qseqs, rseqs, pairs, kernel=None):
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    strings = pairs_ref.resolve(qseqs, rseqs, pairs)
    mq, mr = max(len(s[0]) for s in strings), max(len(s[1]) for s in strings)
    got, gst = _pairs_device(pkg, cfg, Q, R, pairs, mq, mr)
    name = pkg.lib.pmx_last_kernel().decode()
    _check(pkg, orc, cfg, om, qseqs, rseqs, pairs, got, gst)
    assert name == pkg.lib.pmx_last_kernel().decode()                    # the kernel pmx_align_batch_device picks for these pairs
    if kernel:
        assert kernel in name, name
    al_cfg = pkg.pmx_config_t(cfg.mode, cfg.sg_flags, cfg.open, cfg.extend, cfg.width, cfg.want, cfg.matrix)
    out = np.zeros(len(pairs), dtype=pkg.RECORD_DTYPE)
    st = np.zeros(len(pairs), dtype=pkg.STATS_DTYPE)
    rc = pkg.lib.pmx_align_pairs(C.byref(al_cfg), Q.inner, R.inner, len(pairs), pairs.ctypes.data, out.ctypes.data, st.ctypes.data, None)
    assert rc == 0, pkg.lib.pmx_last_error()
    assert out.tobytes() == got.tobytes()                                # the host entry: the same records
    if gst is not None:
        assert st.tobytes() == gst.tobytes()
    return got


def _read_pairs(rng, nq, nr, n, qlen, rlen):
    """windows of qlen x rlen out of longer sequences: (q, r, q_beg, qlen, r_beg, rlen)"""
    return pairs_ref.pairs_array([(int(rng.integers(nq)), int(rng.integers(nr)), int(rng.integers(0, 40)), qlen, int(rng.integers(0, 40)), rlen)
                                  for _ in range(n)])


def test_local_dna_150(pkg, orc):
    rng = np.random.default_rng(7200)
    pm, om = _dna(pkg, orc)
    refs = random_seqs(rng, 40, 200, 260)
    reads = [mutate(rng, r[10:190]) + b"ACGTACGTACGTAC" * 3 for r in refs]
    pairs = _read_pairs(rng, 40, 40, 600, 150, 150)
    pairs["r"][:300] = pairs["q"][:300]                                  # related pairs too
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    _family_case(pkg, orc, cfg, pm, om, reads, refs, pairs, "pmx_sw16")


def test_local_protein_blosum62(pkg, orc):
    rng = np.random.default_rng(7210)
    pm, om = _b62(pkg, orc)
    prots = random_seqs(rng, 50, 60, 220, AA)
    prots += [mutate(rng, p, 0.3, 0.05, AA) for p in prots[:20]]
    pairs = pairs_ref.pairs_array([(int(rng.integers(70)), int(rng.integers(70))) for _ in range(500)] + [(k, 50 + k) for k in range(20)])
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, pm.inner)
    _family_case(pkg, orc, cfg, pm, om, prots, prots, pairs, "pmx_sw16")


@pytest.mark.parametrize("mode,sg", [(0, 0), (1, 15), (1, 1 | 8)])
def test_global_and_semi_global(pkg, orc, mode, sg):
    rng = np.random.default_rng(7220 + sg)
    pm, om = _dna(pkg, orc)
    refs = random_seqs(rng, 30, 180, 240)
    reads = [mutate(rng, r) for r in refs]
    pairs = _read_pairs(rng, 30, 30, 400, 120, 135)
    pairs["r"][:200] = pairs["q"][:200]
    cfg = pkg.pmx_config_t(mode, sg, 5, 2, 0, 0, pm.inner)
    _family_case(pkg, orc, cfg, pm, om, reads, refs, pairs, "pmx_nwsg16")


def test_semi_global_with_statistics(pkg, orc):
    rng = np.random.default_rng(7230)
    pm, om = _dna(pkg, orc)
    refs = random_seqs(rng, 30, 150, 200)
    reads = [mutate(rng, r) for r in refs]
    pairs = _read_pairs(rng, 30, 30, 300, 90, 110)
    pairs["r"][:150] = pairs["q"][:150]
    cfg = pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    _family_case(pkg, orc, cfg, pm, om, reads, refs, pairs)


def test_one_long_pair(pkg, orc):
    rng = np.random.default_rng(7240)
    pm, om = _dna(pkg, orc)
    ref = random_seqs(rng, 1, 3200, 3200)[0]
    read = mutate(rng, ref)[:3100]
    pairs = pairs_ref.pairs_array([(0, 0, 50, 3000, 100, 3000)])
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    _family_case(pkg, orc, cfg, pm, om, [read], [ref], pairs, "pmx_long")


def test_sorted_with_ragged_lengths(pkg, orc):
    rng = np.random.default_rng(7250)
    pm, om = _dna(pkg, orc)
    seqs = random_seqs(rng, 60, 20, 400)
    pairs = pairs_ref.pairs_array([(int(rng.integers(60)), int(rng.integers(60))) for _ in range(700)])
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_SORTED, pm.inner)
    got = _family_case(pkg, orc, cfg, pm, om, seqs, seqs, pairs)
    plain = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    S = pkg.SeqSet.new(seqs)
    unsorted, _ = _pairs_device(pkg, plain, S, S, pairs, 400, 400, 256)
    assert unsorted.tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------------------------- 3. reuse
def test_reuse_of_sequences_and_windows(pkg, orc):
    rng = np.random.default_rng(7300)
    pm, om = _dna(pkg, orc)
    ref = random_seqs(rng, 1, 10000, 10000)[0]
    starts = [int(x) for x in rng.integers(0, 10000 - 200, size=64)]
    reads = [mutate(rng, ref[s + 20:s + 170])[:150].ljust(150, b"A") for s in starts]
    seqs = [ref] + reads                                                                  # one set holds both: Q is R
    rows = [(1, 0, 0, 150, s, 200) for s in starts]                                       # one read against 64 windows of the reference
    rows += [(1 + k, 0, 0, -1, starts[5], 200) for k in range(64)]                        # 64 reads against the same window
    rows += [(1 + k, 0, 0, 150, starts[k], 200) for k in range(64)]                       # every read at its own place
    rows += [(3, 7), (3, 7), (9, 9), (0, 0, 100, 300, 100, 300), (3, 7)]                  # the same pair again; (i, i)
    pairs = pairs_ref.pairs_array(rows)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    S = pkg.SeqSet.new(seqs)
    got, _ = _pairs_device(pkg, cfg, S, S, pairs, 300, 300)
    _check(pkg, orc, cfg, om, seqs, seqs, pairs, got)
    n = len(rows)
    assert got[n - 5].tobytes() == got[n - 4].tobytes() == got[n - 1].tobytes()
    assert got[n - 3].tolist() == [300, 149, 149, 0] and got[n - 2].tolist() == [600, 299, 299, 0]
    assert (got[128:192, 0] >= 100).all()                                                 # the reads were found where they came from


# ---------------------------------------------------------------------------------------------------------------- 4. chunking
def test_chunking_never_changes_a_byte(pkg, orc):
    rng = np.random.default_rng(7400)
    pm, om = _dna(pkg, orc)
    seqs = random_seqs(rng, 80, 160, 260)
    seqs += [mutate(rng, s) for s in seqs[:40]]
    pairs = _read_pairs(rng, 120, 120, 1000, 90, 100)
    pairs["q_len"][::3] = -1
    pairs["r_beg"][::5] = 0
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    S = pkg.SeqSet.new(seqs)
    base, base_stats = _pairs_device(pkg, cfg, S, S, pairs, 260, 260)
    _check(pkg, orc, cfg, om, seqs, seqs, pairs, base, base_stats)
    for chunk in (1000, 999, 334):
        got, gst = _pairs_device(pkg, cfg, S, S, pairs, 260, 260, chunk)
        assert got.tobytes() == base.tobytes() and gst.tobytes() == base_stats.tobytes(), chunk
    got, gst = _pairs_device(pkg, cfg, S, S, pairs[:40], 260, 260, 1)
    assert got.tobytes() == base[:40].tobytes() and gst.tobytes() == base_stats[:40].tobytes()
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).use_stats().build()
    for chunk, m in ((0, 1000), (1000, 1000), (999, 1000), (334, 1000), (1, 40)):
        out, st = al.align_pairs(S, S, pairs[:m], chunk_pairs=chunk)
        assert out.tobytes() == base[:m].tobytes() and st.tobytes() == base_stats[:m].tobytes(), chunk


# --------------------------------------------------------------------------------------------------------- 5. bad descriptors
def test_bad_descriptors_are_flagged_and_leave_the_rest_alone(pkg, orc):
    rng = np.random.default_rng(7500)
    pm, om = _dna(pkg, orc)
    qseqs, rseqs = random_seqs(rng, 20, 60, 100), random_seqs(rng, 25, 60, 100)
    good = [(int(rng.integers(20)), int(rng.integers(25)), int(rng.integers(0, 10)), 50, int(rng.integers(0, 10)), -1) for _ in range(64)]
    bads = [(-1, 0, 0, -1, 0, -1), (20, 0, 0, -1, 0, -1), (0, 25, 0, -1, 0, -1), (0, -3, 0, -1, 0, -1),      # index outside the set
            (0, 0, -1, 10, 0, -1), (0, 0, 0, 10, -2, 10),                                                     # beg < 0
            (0, 0, 40, 70, 0, -1), (0, 0, 0, -1, 95, 10),                                                     # past the sequence's end
            (0, 0, 0, 0, 0, -1), (0, 0, 0, -1, len(rseqs[0]), -1), (0, 0, 0, -2, 0, -1),                      # resolved length 0; len < -1
            (0, 0, 0, 59, 0, -1), (1 << 40, 0, 0, -1, 0, -1), (0, 0, 1 << 30, 1 << 30, 0, -1)]                # above max_qlen = 58; far out
    at = [0, 15, 16, 31, 32, 40, 47, 48, 55, 60, 63, 70, 76, 77]                                             # first / last of chunks of 16, the last pair
    assert len(at) == len(bads)
    rows, gi = [], iter(good)
    for k in range(len(good) + len(bads)):
        rows.append(bads[at.index(k)] if k in at else next(gi))
    pairs, clean = pairs_ref.pairs_array(rows), pairs_ref.pairs_array(good)
    want_bad = np.array([s is None for s in pairs_ref.resolve(qseqs, rseqs, pairs, 58, 100)])
    assert np.nonzero(want_bad)[0].tolist() == at
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    ref, ref_stats = _pairs_device(pkg, cfg, Q, R, clean, 58, 100)
    _check(pkg, orc, cfg, om, qseqs, rseqs, clean, ref, ref_stats)
    for chunk in (0, 16, 5):
        got, gst = _pairs_device(pkg, cfg, Q, R, pairs, 58, 100, chunk)
        assert (got[want_bad] == np.array(pairs_ref.BAD_RECORD)).all() and (gst[want_bad] == 0).all()
        assert got[~want_bad].tobytes() == ref.tobytes() and gst[~want_bad].tobytes() == ref_stats.tobytes()
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).use_stats().build()
    with pytest.raises(pkg.BatchError, match=r"pair 0: query: index outside"):
        al.align_pairs(Q, R, pairs)
    with pytest.raises(pkg.BatchError, match=r"pair 14: query: index outside"):
        al.align_pairs(Q, R, pairs[1:])
    with pytest.raises(pkg.BatchError, match=r"pair 4: reference: negative window start"):
        al.align_pairs(Q, R, pairs[36:])
    out, st = al.align_pairs(Q, R, clean)
    assert out.tobytes() == ref.tobytes() and st.tobytes() == ref_stats.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 6. all-vs-all
def _all_pairs_device(pkg, cfg, S, first, count, max_len, chunk=0):
    rec, st = _outputs(count, False)
    pkg.align_all_pairs_device(cfg, S, first, count, max_len, rec.data_ptr(), None, _stream(), chunk)
    return _fetch(rec, st, count)[0]


@pytest.mark.parametrize("n", [2, 3, 65])
def test_all_pairs_of_small_sets(pkg, orc, n):
    rng = np.random.default_rng(7600 + n)
    pm, om = _b62(pkg, orc)
    prots = random_seqs(rng, n, 15, 130, AA)
    total = pairs_ref.all_pairs_count(n)
    pairs = pairs_ref.all_pairs_descriptors(n, 0, total)
    assert [(int(p["q"]), int(p["r"])) for p in pairs] == [(i, j) for i in range(n) for j in range(i + 1, n)]
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, pm.inner)
    S = pkg.SeqSet.new(prots)
    got = _all_pairs_device(pkg, cfg, S, 0, total, 130)
    _check(pkg, orc, cfg, om, prots, prots, pairs, got)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    assert al.align_all_pairs(S).tobytes() == got.tobytes()
    assert al.align_all_pairs(S, chunk_pairs=7).tobytes() == got.tobytes()
    listed, _ = _pairs_device(pkg, cfg, S, S, pairs, 130, 130)
    assert listed.tobytes() == got.tobytes()


def test_all_pairs_windows_of_300(pkg, orc):
    rng = np.random.default_rng(7650)
    pm, om = _b62(pkg, orc)
    n = 300
    prots = random_seqs(rng, n, 20, 90, AA)
    total = pairs_ref.all_pairs_count(n)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, pm.inner)
    S = pkg.SeqSet.new(prots)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(11).gap_extend(1).build()
    for first, count in ((0, 500), (pairs_ref.row_start(n, 100) - 150, 400), (total - 450, 450)):
        pairs = pairs_ref.all_pairs_descriptors(n, first, count)
        assert len({int(q) for q in pairs["q"]}) >= 2                    # the window crosses a row boundary
        got = _all_pairs_device(pkg, cfg, S, first, count, 90)
        _check(pkg, orc, cfg, om, prots, prots, pairs, got)
        for chunk in (128, 149):
            assert _all_pairs_device(pkg, cfg, S, first, count, 90, chunk).tobytes() == got.tobytes()
        assert al.align_all_pairs(S, first, count, chunk_pairs=128).tobytes() == got.tobytes()
    assert len(al.align_all_pairs(S, total - 3)) == 3
    with pytest.raises(pkg.BatchError, match="beyond"):
        al.align_all_pairs(S, total - 3, 4)
    holes = list(prots); holes[7] = b""                                  # an empty sequence: the host entry names the first pair that uses it
    with pytest.raises(pkg.BatchError, match=r"pair 5 \(0, 7\): reference: empty window"):
        al.align_all_pairs(pkg.SeqSet.new(holes), 1, 100)


def test_enumerator_at_the_largest_set(pkg):
    import torch
    rng = np.random.default_rng(7700)
    total = pairs_ref.all_pairs_count(NMAX)
    s = pairs_ref.row_start(NMAX, int(rng.integers(1, NMAX - 1)))
    for first in (total - 4096, s - 2048, 0, pairs_ref.row_start(NMAX, NMAX - 200) - 100):
        d = torch.zeros(4096 * 32, dtype=torch.uint8, device=_dev())
        pkg.all_pairs_enumerate_device(NMAX, first, 4096, d.data_ptr(), _stream())
        torch.cuda.synchronize()
        got = d.cpu().numpy().view(pairs_ref.PAIR_DTYPE)
        want = pairs_ref.all_pairs_descriptors(NMAX, first, 4096)
        assert got.tobytes() == want.tobytes(), first


# -------------------------------------------------------------------------------------------- 7. wrapped sets, repeatability
def test_wrapped_sets_equal_uploaded_sets(pkg, orc):
    rng = np.random.default_rng(7800)
    pm, om = _dna(pkg, orc)
    seqs = random_seqs(rng, 50, 80, 180)
    buf, off = pkg.pack(seqs)
    d_buf, d_off = _up(np.concatenate([np.zeros(3, dtype=np.uint8), buf])), _up(off)      # a base address that is not dword-aligned
    W = pkg.SeqSet.wrap_device(d_buf.data_ptr() + 3, d_off.data_ptr(), len(seqs), len(buf), keep=(d_buf, d_off))
    S = pkg.SeqSet.new(seqs)
    assert len(W) == len(S) == 50
    pairs = _read_pairs(rng, 50, 50, 500, 30, -1)
    pairs["r_beg"] = 0
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    got, _ = _pairs_device(pkg, cfg, S, S, pairs, 180, 180)
    _check(pkg, orc, cfg, om, seqs, seqs, pairs, got)
    for Q, R in ((W, W), (W, S), (S, W)):
        again, _ = _pairs_device(pkg, cfg, Q, R, pairs, 180, 180, 200)
        assert again.tobytes() == got.tobytes()
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    assert al.align_pairs(W, W, pairs).tobytes() == got.tobytes()                        # maxima and validation on the device
    assert al.align_pairs(W, S, pairs, chunk_pairs=77).tobytes() == got.tobytes()
    assert al.align_all_pairs(W, 10, 300).tobytes() == al.align_all_pairs(S, 10, 300).tobytes()
    broken = pairs.copy(); broken[123]["q"] = 50
    with pytest.raises(pkg.BatchError, match="pair 123"):
        al.align_pairs(W, W, broken)
    # offsets that point outside the wrapped buffer: flagged, never followed
    lying = off.copy(); lying[50] += 64
    d_lie = _up(lying)
    L = pkg.SeqSet.wrap_device(d_buf.data_ptr() + 3, d_lie.data_ptr(), len(seqs), len(buf), keep=(d_buf, d_lie))
    rows = pairs_ref.pairs_array([(49, 0), (0, 49), (48, 1)])
    flagged, _ = _pairs_device(pkg, cfg, L, L, rows, 300, 300)              # (the lengths pass: only `bytes` tells)
    assert flagged[0].tolist() == list(pairs_ref.BAD_RECORD) and flagged[1].tolist() == list(pairs_ref.BAD_RECORD)
    assert flagged[2].tobytes() == _pairs_device(pkg, cfg, S, S, rows[2:], 180, 180)[0].tobytes()


def test_two_identical_calls_give_identical_bytes(pkg):
    rng = np.random.default_rng(7900)
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    seqs = random_seqs(rng, 200, 100, 200)
    pairs = _read_pairs(rng, 200, 200, 5000, 60, -1)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    S = pkg.SeqSet.new(seqs)
    a, ast = _pairs_device(pkg, cfg, S, S, pairs, 200, 200, 1024)
    b, bst = _pairs_device(pkg, cfg, S, S, pairs, 200, 200, 1024)
    assert a.tobytes() == b.tobytes() and ast.tobytes() == bst.tobytes()
    assert (a[:, 3] == 0).all() and (a != SENTINEL).all()


# ------------------------------------------------------------------------------- 8. the host road's scan on helper threads
def _big_list(rng, n=262144 + 3, nseq=16):
    """n whole-sequence descriptors over a set of nseq sequences: from 262 144 pairs on, the host road scans in four slices"""
    pairs = np.zeros(n, dtype=pairs_ref.PAIR_DTYPE)
    pairs["q"], pairs["r"] = rng.integers(0, nseq, size=n), rng.integers(0, nseq, size=n)
    pairs["q_len"] = pairs["r_len"] = -1
    return pairs


def test_host_entries_equal_device_entries_where_the_scan_is_threaded(pkg):
    import torch
    rng = np.random.default_rng(7950)
    seqs = random_seqs(rng, 16, 8, 8)
    pairs = _big_list(rng)
    n = len(pairs)
    S = pkg.SeqSet.new(seqs)
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    want, _ = _pairs_device(pkg, cfg, S, S, pairs, 8, 8)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    assert al.align_pairs(S, S, pairs).tobytes() == want.tobytes()
    assert len({tuple(r) for r in want[:4096].tolist()}) > 8              # (records that differ: an order mixed up would show)
    # the same list through a frameshift host entry: the nucleotides' eight letters are amino-acid letters too
    b62 = pkg.Matrix.from_name("blosum62")
    fcfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, b62.inner)
    rec = torch.full((n, 4), SENTINEL, dtype=torch.int32, device=_dev())
    won = torch.full((n,), 9, dtype=torch.uint8, device=_dev())
    d_pairs = _up_pairs(pairs)
    pkg.align_pairs_frameshift_device(fcfg, S, S, n, d_pairs.data_ptr(), None, pkg.STRAND_BOTH, 4, 6, 8, rec.data_ptr(), won.data_ptr(), _stream(), 0)
    torch.cuda.synchronize()
    fal = pkg.Aligner.new().local().matrix(b62).gap_open(11).gap_extend(1).build()
    got, gwon = fal.align_pairs(S, S, pairs, frameshift=4, strand="both")
    assert got.tobytes() == rec.cpu().numpy().tobytes() and gwon.tobytes() == won.cpu().numpy().tobytes()
    assert (gwon <= 1).all() and gwon.any() and not gwon.all()
