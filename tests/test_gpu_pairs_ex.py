"""Strands and CIGAR output of the sequence-set batches (`-m gpu`): pmx_gather_pairs_device against the strings
tests/pairs_ex_ref.py resolves (every source and destination alignment, both strands, the first and last bytes of a set);
pmx_align_pairs_ex[_device] against the CPU oracle on those strings AND against pmx_align_batch_device /
pmx_align_batch_cigar_device on the same strings packed by numpy -- records, statistics, CIGAR text, offsets, begins -- under
every chunking; capacity, bad descriptors, the host entry, refusals outside the device CIGAR window, repeatability.  Every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import pairs_ex_ref
import pairs_ref
from util import random_seqs, mutate, AA, golden

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xEE
NO_ROAD = "use pmx_align_batch_cigar"


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


def _maxima(strings):
    good = [s for s in strings if s is not None]
    return max(len(s[0]) for s in good), max(len(s[1]) for s in good)


class Ex:
    """outputs of one pmx_align_pairs_ex_device call, on the host"""


def _ex_device(pkg, cfg, Q, R, pairs, strand, mq, mr, chunk=0, capacity=0, slack=64):
    import torch
    n = len(pairs)
    stats, cigar = bool(cfg.want & pkg.WANT_STATS), bool(cfg.want & pkg.WANT_CIGAR)
    rec = _full((n, 4), SENTINEL, torch.int32)
    st = _full((n, 3), SENTINEL, torch.int32) if stats else None
    beg = _full((n, 2), SENTINEL, torch.int32) if cigar else None
    text = _full((capacity + slack,), FILL, torch.uint8) if cigar else None
    off = _full((n + 1,), -9, torch.int64) if cigar else None
    d_pairs = _up(np.ascontiguousarray(pairs).view(np.uint8))
    d_strand = _up(np.asarray(strand, dtype=np.uint8)) if strand is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    pkg.align_pairs_ex_device(cfg, Q, R, n, d_pairs.data_ptr(), ptr(d_strand), mq, mr, rec.data_ptr(), ptr(st), ptr(beg), ptr(text),
                              capacity, ptr(off), _stream(), chunk)
    e = Ex()
    e.kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    host = lambda t: t.cpu().numpy() if t is not None else None
    e.rec, e.stats, e.beg, e.text, e.off = host(rec), host(st), host(beg), host(text), host(off)
    return e


def _pack16(pkg, seqs):
    buf, off = pkg.pack(seqs)
    return _up(np.concatenate([buf, np.zeros(16, dtype=np.uint8)])), _up(off), off


def _batch_device(pkg, cfg, strings):
    """pmx_align_batch_device on the strings packed back to back"""
    import torch
    n = len(strings)
    stats = bool(cfg.want & pkg.WANT_STATS)
    dq, dqo, qo = _pack16(pkg, [s[0] for s in strings]); dr, dro, ro = _pack16(pkg, [s[1] for s in strings])
    rec = _full((n, 4), SENTINEL, torch.int32)
    st = _full((n, 3), SENTINEL, torch.int32) if stats else None
    pkg.align_batch_device(cfg, n, dq.data_ptr(), dqo.data_ptr(), dr.data_ptr(), dro.data_ptr(), int(np.diff(qo).max()), int(np.diff(ro).max()),
                           rec.data_ptr(), st.data_ptr() if stats else None, _stream())
    _sync()
    return rec.cpu().numpy(), (st.cpu().numpy() if stats else None)


def _cigar_batch_device(pkg, cfg, strings):
    """pmx_align_batch_cigar_device on the strings packed back to back: (records, text bytes, offsets)"""
    import torch
    n = len(strings)
    dq, dqo, qo = _pack16(pkg, [s[0] for s in strings]); dr, dro, ro = _pack16(pkg, [s[1] for s in strings])
    cap = int(2 * (qo[-1] + ro[-1]) + 16 * n)                           # (every op is at most "1X": two bytes per symbol)
    rec = _full((n, 4), SENTINEL, torch.int32)
    text = _full((cap,), FILL, torch.uint8)
    off = _full((n + 1,), -9, torch.int64)
    pkg.align_batch_cigar_device(cfg, n, dq.data_ptr(), dqo.data_ptr(), dr.data_ptr(), dro.data_ptr(), int(np.diff(qo).max()), int(np.diff(ro).max()),
                                 rec.data_ptr(), text.data_ptr(), cap, off.data_ptr(), _stream())
    name = pkg.lib.pmx_last_kernel().decode()
    _sync()
    off = off.cpu().numpy()
    assert 0 < off[n] <= cap
    return rec.cpu().numpy(), text.cpu().numpy()[:off[n]], off, name


def _oracle_records(orc, cfg, om, strings, stats):
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    sg = cfg.sg_flags if cfg.mode == 1 else orc.SG_ALL
    if stats:
        return orc.align_stats_sample(cfg.mode, np.arange(len(strings)), qb, qo, rb, ro, cfg.open, cfg.extend, om, sg_flags=sg, bits=cfg.width)
    return orc.align_batch(cfg.mode, qb, qo, rb, ro, cfg.open, cfg.extend, om, sg_flags=sg, bits=cfg.width)


# --------------------------------------------------------------------------------------------------------- 1. gather geometry
LENS = list(range(1, 10)) + [15, 16, 17, 63, 64, 65, 255]


def _gather(pkg, Q, R, pairs, strand, mq, mr, strings):
    """pmx_gather_pairs_device into buffers of exactly the needed capacity, sentinel bytes behind them"""
    import torch
    n = len(pairs)
    qn, rn = sum(len(s[0]) for s in strings), sum(len(s[1]) for s in strings)
    qout, rout = _full((qn + 64,), FILL, torch.uint8), _full((rn + 64,), FILL, torch.uint8)
    qoff, roff = _full((n + 1,), -9, torch.int64), _full((n + 1,), -9, torch.int64)
    ok = _full((n + 8,), FILL, torch.uint8)
    d_pairs = _up(np.ascontiguousarray(pairs).view(np.uint8))
    d_strand = _up(np.asarray(strand, dtype=np.uint8)) if strand is not None else None
    pkg.gather_pairs_device(Q, R, n, d_pairs.data_ptr(), d_strand.data_ptr() if strand is not None else None, mq, mr,
                            qout.data_ptr(), qn, qoff.data_ptr(), rout.data_ptr(), rn, roff.data_ptr(), ok.data_ptr(), _stream())
    _sync()
    return qout.cpu().numpy(), qoff.cpu().numpy(), rout.cpu().numpy(), roff.cpu().numpy(), ok.cpu().numpy()


def _check_gather(pkg, seqs, pairs, strand, got):
    strings = pairs_ex_ref.resolve(seqs, seqs, pairs, strand)
    assert all(s is not None for s in strings)
    qout, qoff, rout, roff, ok = got
    n = len(pairs)
    want_q, want_r = b"".join(s[0] for s in strings), b"".join(s[1] for s in strings)
    assert qoff.tolist() == np.concatenate([[0], np.cumsum([len(s[0]) for s in strings])]).tolist()
    assert roff.tolist() == np.concatenate([[0], np.cumsum([len(s[1]) for s in strings])]).tolist()
    bad = [k for k in range(n) if qout[qoff[k]:qoff[k + 1]].tobytes() != strings[k][0]]
    assert not bad, (bad[:5], [(int(strand[k]) if strand is not None else 0, pairs[k]) for k in bad[:5]])
    assert qout[:len(want_q)].tobytes() == want_q and rout[:len(want_r)].tobytes() == want_r
    assert (qout[len(want_q):] == FILL).all() and (rout[len(want_r):] == FILL).all()          # the sentinels behind the outputs
    assert (ok[:n] == 1).all() and (ok[n:] == FILL).all()
    return strings


def test_gather_geometry_both_strands(pkg):
    """the lattice of test_gather_geometry_every_alignment -- source offset mod 4 x length class x destination offset mod 4 -- with
    strand 1 on every pair and mixed; windows that hold the first and the last bytes of the set (the bounds fallback of the backward
    walk); a 256-byte sequence of all byte values reversed at four alignments"""
    rng = np.random.default_rng(9100)
    base = random_seqs(rng, 4, 300, 300)
    seqs = [base[0], base[1] + b"A", base[2] + b"AC", base[3] + b"ACG"]                  # offsets 0, 300, 601, 903: residues 0, 0, 1, 3
    seqs += [b"G" * (k + 1) + base[k] for k in range(4)]                                 # the same bytes, shifted by 1 .. 4
    every = bytes(range(256))
    seqs += [b"T" * k + every for k in range(4)]                                         # all byte values, four alignments
    seqs.append(random_seqs(rng, 1, 23, 23)[0])                                          # the last sequence of the set
    last = len(seqs) - 1
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    rows = [(0, last, 0, 5, 2, 5), (0, last, 0, 17, 0, -1), (0, 0, 0, 1, 0, 2), (0, 0, 1, 3, 0, 3),          # the first bytes of the set,
            (last, 0, 19, 4, 100, -1), (last, last, 0, -1, 4, -1), (last, 0, 3, 20, 7, 9), (last, 1, 22, 1, 0, 1),   # the last ones
            (last, 0, 6, -1, 0, 4)]
    rows += [(8 + k, 8 + (k + 1) % 4, k, 256, (k + 1) % 4, 256) for k in range(4)]
    for k in range(4):
        for a in range(4):
            for x, L in enumerate(LENS):
                beg = a + 4 * ((x + k) % 9)
                rows.append((k, k + 4, beg, L, k + 1 + beg, L))
                rows.append((k + 4, (k + 1) % 4, beg, L, (a + x) % 7, LENS[(x + 5) % len(LENS)]))
    rows = [rows[i] for i in rng.permutation(len(rows))]                                 # (destination offsets of every residue)
    pairs = pairs_ref.pairs_array(rows)
    n = len(pairs)
    assert {int(off[p["q"]] + p["q_beg"]) % 4 for p in pairs if p["q"] >= 8 and p["q"] < 12} == {0, 1, 2, 3}
    src = {(int(off[p["q"]] + p["q_beg"]) % 4, int(p["q_len"])) for p in pairs}           # (the query side is the one that reverses)
    assert all((a, L) in src for a in range(4) for L in LENS)
    S = pkg.SeqSet.new(seqs)
    mixed = rng.integers(0, 2, size=n).astype(np.uint8)
    # every pair reversed; then mixed and its inverse: every pair on both strands beside neighbours of the other one; no strands
    for strand in (np.ones(n, dtype=np.uint8), mixed, 1 - mixed, None):
        got = _gather(pkg, S, S, pairs, strand, 300, 300, pairs_ex_ref.resolve(seqs, seqs, pairs, strand))
        strings = _check_gather(pkg, seqs, pairs, strand, got)
        dst = {(int(o) % 4, len(s[0])) for o, s in zip(got[1][:-1], strings)}
        assert all((a, L) in dst for a in range(4) for L in LENS)
    # one window, every destination alignment, both strands: a set of one sequence whose window is the whole set
    one = pkg.SeqSet.new([every])
    for reps in (1, 2, 3, 4):
        rows = [(0, 0, 0, 1, 0, 1)] * reps + [(0, 0)]
        strand = np.array([0] * reps + [1], dtype=np.uint8)
        p1 = pairs_ref.pairs_array(rows)
        got = _gather(pkg, one, one, p1, strand, 256, 256, pairs_ex_ref.resolve([every], [every], p1, strand))
        _check_gather(pkg, [every], p1, strand, got)
        assert got[0][reps:reps + 256].tobytes() == every[::-1].translate(pairs_ex_ref.COMP)


def test_gather_capacity_and_bad_pairs(pkg):
    """a window that would cross its capacity is not written; a bad pair (strand bytes 2 and 255 among them) is one zero byte"""
    import torch
    rng = np.random.default_rng(9150)
    seqs = random_seqs(rng, 6, 40, 90)
    S = pkg.SeqSet.new(seqs)
    rows = [(0, 1), (2, 3, 5, 20, 0, -1), (9, 0), (1, 2), (3, 4, 0, -1, 10, 30), (5, 5), (4, 0, 2, 9, 1, 8)]
    strand = np.array([1, 0, 1, 2, 1, 255, 1], dtype=np.uint8)
    pairs = pairs_ref.pairs_array(rows)
    strings = pairs_ex_ref.resolve(seqs, seqs, pairs, strand)
    assert [s is None for s in strings] == [False, False, True, True, False, True, False]
    filled = [s if s is not None else (b"\0", b"\0") for s in strings]
    full = _gather(pkg, S, S, pairs, strand, 90, 90, filled)
    assert full[0][:full[1][-1]].tobytes() == b"".join(s[0] for s in filled)
    assert full[2][:full[3][-1]].tobytes() == b"".join(s[1] for s in filled)
    assert full[4][:7].tolist() == [1, 1, 0, 0, 1, 0, 1]
    assert (full[0][full[1][-1]:] == FILL).all() and (full[2][full[3][-1]:] == FILL).all()
    n = len(pairs)
    qn, rn = int(full[1][-1]), int(full[3][-1])
    for qc, rc in ((qn - 1, rn), (qn // 2, rn // 3), (0, 0)):
        qout, rout = _full((qn + 8,), FILL, torch.uint8), _full((rn + 8,), FILL, torch.uint8)
        qoff, roff = _full((n + 1,), -9, torch.int64), _full((n + 1,), -9, torch.int64)
        d_pairs, d_strand = _up(pairs.view(np.uint8)), _up(strand)
        pkg.gather_pairs_device(S, S, n, d_pairs.data_ptr(), d_strand.data_ptr(), 90, 90, qout.data_ptr(), qc, qoff.data_ptr(),
                                rout.data_ptr(), rc, roff.data_ptr(), None, _stream())
        _sync()
        assert qoff.cpu().numpy().tolist() == full[1].tolist() and roff.cpu().numpy().tolist() == full[3].tolist()
        for out, offs, cap, ref in ((qout.cpu().numpy(), full[1], qc, full[0]), (rout.cpu().numpy(), full[3], rc, full[2])):
            fit = int(np.searchsorted(offs[1:], cap, side="right"))                       # pairs [0, fit) end inside the capacity
            assert out[:offs[fit]].tobytes() == ref[:offs[fit]].tobytes() and (out[offs[fit]:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------- 2. stranded scores
def _mapper_case(rng, n_reads, lo, hi, ref_len, windows=3, pad=12):
    """reads of lo .. hi bp cut from a reference, half of them stored reverse-complemented; each against `windows` windows of the
    reference: the one it came from (padded) and random ones"""
    ref = random_seqs(rng, 1, ref_len, ref_len)[0]
    reads, rows, strand = [], [], []
    lens = [lo, hi] + [int(x) for x in rng.integers(lo, hi + 1, size=n_reads - 2)]
    for i, L in enumerate(lens):
        s = int(rng.integers(0, ref_len - L))
        read = mutate(rng, ref[s:s + L], 0.06, 0.02 if i >= 2 else 0.0)[:hi]                # (the shortest and the longest keep their lengths)
        rev = i % 2 == 1
        reads.append(pairs_ex_ref.revcomp(read) if rev else read)
        for w in range(windows):
            b = max(0, s - pad) if w == 0 else int(rng.integers(0, ref_len - hi - 2 * pad))
            rl = min(L + 2 * pad, 255, ref_len - b)
            rows.append((i, 0, 0, -1, b, rl))
            strand.append(int(rev) if w < 2 else int(rng.integers(0, 2)))
    return ref, reads, pairs_ref.pairs_array(rows), np.array(strand, dtype=np.uint8)


@pytest.mark.parametrize("mode", [2, 1])
def test_stranded_scores(pkg, orc, mode):
    rng = np.random.default_rng(9200 + mode)
    pm, om = _dna(pkg, orc)
    ref, reads, pairs, strand = _mapper_case(rng, 100, 1, 255, 3000)
    n = len(pairs)
    assert n == 300 and 100 < strand.sum() < 200
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new([ref])
    strings = pairs_ex_ref.resolve(reads, [ref], pairs, strand)
    assert {len(s[0]) for s in strings} >= {1, 255}
    cfg = pkg.pmx_config_t(mode, 15 if mode == 1 else 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    want = _oracle_records(orc, cfg, om, strings, True)
    direct, direct_stats = _batch_device(pkg, cfg, strings)
    assert (direct[:, :3] == want[:, :3]).all() and (direct_stats == want[:, 3:6]).all()
    if mode == 2:                                                                         # the reads were found on their strands
        found = want[0::3, 0] >= np.array([len(r) for r in reads])
        assert found[1::2].sum() > 40 and found[0::2].sum() > 40
        wrong = _oracle_records(orc, cfg, om, pairs_ex_ref.resolve(reads, [ref], pairs, 1 - strand), False)
        assert (wrong[0::3, 0] < want[0::3, 0]).sum() > 80
    for chunk in (0, 64, 100):
        got = _ex_device(pkg, cfg, Q, R, pairs, strand, 255, 255, chunk)
        bad = np.nonzero((got.rec[:, :3] != want[:, :3]).any(axis=1))[0]
        assert len(bad) == 0, (chunk, bad[:5], got.rec[bad[:5]], want[bad[:5]])
        assert (got.stats == want[:, 3:6]).all()
        assert got.rec.tobytes() == direct.tobytes() and got.stats.tobytes() == direct_stats.tobytes(), chunk
    # no strands: the entry is pmx_align_pairs_device, byte for byte
    import torch
    for chunk in (0, 100):
        got = _ex_device(pkg, cfg, Q, R, pairs, None, 255, 255, chunk)
        rec, st = _full((n, 4), SENTINEL, torch.int32), _full((n, 3), SENTINEL, torch.int32)
        d_pairs = _up(pairs.view(np.uint8))
        pkg.align_pairs_device(cfg, Q, R, n, d_pairs.data_ptr(), 255, 255, rec.data_ptr(), st.data_ptr(), _stream(), chunk)
        _sync()
        assert got.rec.tobytes() == rec.cpu().numpy().tobytes() and got.stats.tobytes() == st.cpu().numpy().tobytes()
        zeros = _ex_device(pkg, cfg, Q, R, pairs, np.zeros(n, dtype=np.uint8), 255, 255, chunk)
        assert zeros.rec.tobytes() == got.rec.tobytes() and zeros.stats.tobytes() == got.stats.tobytes()
    al = pkg.Aligner.new()
    al = (al.local() if mode == 2 else al.semi_global()).matrix(pm).gap_open(5).gap_extend(2).use_stats().build()
    out, st = al.align_pairs(Q, R, pairs, strand=strand, chunk_pairs=100)
    assert out.tobytes() == direct.tobytes() and st.tobytes() == direct_stats.tobytes()


# -------------------------------------------------------------------------------------------------------------------- 3. CIGAR
def _texts(e, n):
    return [e.text[e.off[k]:e.off[k + 1]].tobytes().decode() for k in range(n)]


def _cigar_case(pkg, orc, cfg, om, qseqs, rseqs, pairs, strand, chunks=(0, 64, 129)):
    """records, text, offsets and begins of the set batch == pmx_align_batch_cigar_device on the packed strings, for every chunking;
    text and begins == the oracle's; the text re-scores to the record's score from the begins"""
    n = len(pairs)
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    strings = pairs_ex_ref.resolve(qseqs, rseqs, pairs, strand)
    assert all(s is not None for s in strings)
    mq, mr = _maxima(strings)
    drec, dtext, doff, dname = _cigar_batch_device(pkg, cfg, strings)
    assert "pmx_walkp_kernel" in dname, dname
    need = int(doff[n])
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    sg = cfg.sg_flags if cfg.mode == 1 else orc.SG_ALL
    want_text, want = orc.cigar_sample(cfg.mode, np.arange(n), qb, qo, rb, ro, cfg.open, cfg.extend, om, sg_flags=sg)
    first = None
    for chunk in chunks:
        assert chunk == 0 or -(-n // chunk) > 1                                           # more than one chunk runs
        got = _ex_device(pkg, cfg, Q, R, pairs, strand, mq, mr, chunk, need)
        assert "pmx_walkp_kernel" in got.kernel, got.kernel                               # (not a fallback)
        assert got.rec.tobytes() == drec.tobytes(), chunk
        assert got.off.tobytes() == doff.tobytes(), chunk
        assert got.text[:need].tobytes() == dtext.tobytes(), chunk
        assert (got.text[need:] == FILL).all()
        if first is None:
            first = got
            assert (got.rec[:, :3] == want[:, :3]).all() and (got.rec[:, 3] == 0).all()
            texts = _texts(got, n)
            bad = [k for k in range(n) if texts[k] != want_text[k]]
            assert not bad, (bad[:3], [(texts[k], want_text[k]) for k in bad[:3]])
            assert (got.beg == want[:, 3:5]).all(), np.nonzero((got.beg != want[:, 3:5]).any(axis=1))[0][:5]
            res, malformed = orc.rescore_cigars(got.text[:max(need, 1)], got.off, qb, qo, rb, ro, cfg.open, cfg.extend, om,
                                                beg=got.beg.reshape(-1), free_mask=cfg.sg_flags if cfg.mode == 1 else 0)
            assert malformed == 0 and (res[:, 0] == got.rec[:, 0]).all() and (res[:, 3] == 0).all()
        else:
            assert got.beg.tobytes() == first.beg.tobytes(), chunk
    return Q, R, strings, first


def _window_pairs(rng, nq, nr, n, qlen, rlen, slack=40):
    return pairs_ref.pairs_array([(int(rng.integers(nq)), int(rng.integers(nr)), int(rng.integers(0, slack)), qlen, int(rng.integers(0, slack)), rlen)
                                  for _ in range(n)])


def test_cigar_semi_global_dna_150(pkg, orc):
    """(i) DNA 2 / -3, 5 / 2, semi-global, equal lengths: the perm-table form of the sweep"""
    rng = np.random.default_rng(9300)
    pm, om = _dna(pkg, orc)
    refs = random_seqs(rng, 48, 200, 260)
    reads = [mutate(rng, r[10:190], 0.05, 0.02) + b"ACGTACGTACGTAC" * 3 for r in refs]
    reads = [pairs_ex_ref.revcomp(r) if k % 2 else r for k, r in enumerate(reads)]
    pairs = _window_pairs(rng, 48, 48, 384, 150, 150, 30)
    pairs["r"][:256] = pairs["q"][:256]                                                   # related pairs
    strand = (pairs["q"] % 2).astype(np.uint8)
    strand[300:] = rng.integers(0, 2, size=84)
    cfg = pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, pkg.WANT_CIGAR, pm.inner)
    _cigar_case(pkg, orc, cfg, om, reads, refs, pairs, strand)


@pytest.mark.parametrize("mode,sg", [(0, 0), (1, 15)])
def test_cigar_ragged_with_wildcards(pkg, orc, mode, sg):
    """(ii) ragged 20 .. 250 bp, an N in some queries: blocks that fall back to the LDS-profile form"""
    rng = np.random.default_rng(9310 + mode)
    pm, om = _dna(pkg, orc)
    ref, reads, pairs, strand = _mapper_case(rng, 128, 20, 250, 4000)
    for k in range(0, 128, 5):                                                            # an N somewhere in every fifth read
        r = bytearray(reads[k]); r[int(rng.integers(len(r)))] = ord("N"); reads[k] = bytes(r)
    assert len(pairs) == 384
    cfg = pkg.pmx_config_t(mode, sg, 5, 2, 0, pkg.WANT_CIGAR, pm.inner)
    _cigar_case(pkg, orc, cfg, om, reads, [ref], pairs, strand)


def test_cigar_local_blosum62_forward(pkg, orc):
    """(iii) BLOSUM62 11 / 1, local, 30 .. 300 aa, no strands"""
    rng = np.random.default_rng(9320)
    pm, om = _b62(pkg, orc)
    prots = random_seqs(rng, 60, 30, 300, AA)
    prots += [mutate(rng, p, 0.3, 0.05, AA)[:300] for p in prots[:40]]
    rows = [(int(rng.integers(100)), int(rng.integers(100))) for _ in range(304)] + [(k, 60 + k) for k in range(40)] + [(60 + k, k) for k in range(40)]
    pairs = pairs_ref.pairs_array([rows[i] for i in rng.permutation(len(rows))])
    assert len(pairs) == 384
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, pkg.WANT_CIGAR, pm.inner)
    _cigar_case(pkg, orc, cfg, om, prots, prots, pairs, None)


# ----------------------------------------------------------------------------------------------------------------- 4. capacity
def test_cigar_capacity(pkg, orc):
    rng = np.random.default_rng(9400)
    pm, om = _dna(pkg, orc)
    ref, reads, pairs, strand = _mapper_case(rng, 128, 20, 250, 4000)
    n = len(pairs)
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new([ref])
    cfg = pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, pkg.WANT_CIGAR, pm.inner)
    strings = pairs_ex_ref.resolve(reads, [ref], pairs, strand)
    drec, dtext, doff, _ = _cigar_batch_device(pkg, cfg, strings)
    need = int(doff[n])
    for cap in (need - 1, need // 2, 0):
        for chunk in (0, 129):
            got = _ex_device(pkg, cfg, Q, R, pairs, strand, 250, 255, chunk, cap, slack=need + 64)
            assert got.off.tobytes() == doff.tobytes() and got.off[n] == need             # the bytes the batch needs
            assert got.rec.tobytes() == drec.tobytes()
            fit = int(np.searchsorted(doff[1:], cap, side="right"))                       # pairs [0, fit) end inside the capacity
            assert fit < n and (fit > 0) == (cap > 0)
            assert got.text[:doff[fit]].tobytes() == dtext[:doff[fit]].tobytes()
            assert (got.text[doff[fit]:] == FILL).all(), (cap, chunk)                    # from the first pair that does not fit


# ---------------------------------------------------------------------------------------------------------- 5. bad descriptors
def test_bad_descriptors_in_cigar_mode(pkg, orc):
    rng = np.random.default_rng(9500)
    pm, om = _dna(pkg, orc)
    qseqs, rseqs = random_seqs(rng, 20, 60, 100), random_seqs(rng, 25, 60, 100)
    rseqs[:20] = [mutate(rng, q)[:100] for q in qseqs]
    good = [(int(rng.integers(20)), int(rng.integers(25)), int(rng.integers(0, 10)), 50, int(rng.integers(0, 10)), -1) for _ in range(64)]
    good_strand = rng.integers(0, 2, size=64).astype(np.uint8)
    bads = [((-1, 0, 0, -1, 0, -1), 0), ((20, 0, 0, -1, 0, -1), 1), ((0, 25, 0, -1, 0, -1), 0),                # index outside the set
            ((0, 0, -1, 10, 0, -1), 1), ((0, 0, 0, 10, -2, 10), 0),                                            # beg < 0
            ((0, 0, 40, 70, 0, -1), 1), ((0, 24, 0, -1, 95, 10), 0),                                           # past the sequence's end
            ((0, 0, 0, 0, 0, -1), 0), ((0, 0, 0, -2, 0, -1), 1),                                               # resolved length 0; len < -1
            ((0, 0, 0, 59, 0, -1), 1), ((1 << 40, 0, 0, -1, 0, -1), 0),                                        # above max_qlen = 58; far out
            ((1, 1, 0, 50, 0, -1), 2), ((2, 2, 0, 50, 0, -1), 255), ((3, 3), 2)]                               # strand bytes 2 and 255
    at = [0, 14, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 76, 77]                                              # around the borders of chunks of 16; the last pair
    assert len(at) == len(bads)
    rows, strand, gi = [], [], iter(zip(good, good_strand))
    for k in range(len(good) + len(bads)):
        row, s = bads[at.index(k)] if k in at else next(gi)
        rows.append(row); strand.append(int(s))
    pairs, clean, strand = pairs_ref.pairs_array(rows), pairs_ref.pairs_array(good), np.array(strand, dtype=np.uint8)
    n = len(pairs)
    want_bad = np.array([s is None for s in pairs_ex_ref.resolve(qseqs, rseqs, pairs, strand, 58, 100)])
    assert np.nonzero(want_bad)[0].tolist() == at
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_CIGAR, pm.inner)
    _, _, _, ref = _cigar_case(pkg, orc, cfg, om, qseqs, rseqs, clean, good_strand, chunks=(0,))
    ref_texts = _texts(ref, 64)
    for chunk in (0, 16, 5):
        got = _ex_device(pkg, cfg, Q, R, pairs, strand, 58, 100, chunk, int(ref.off[64]))
        assert (got.rec[want_bad] == np.array(pairs_ref.BAD_RECORD)).all()
        assert (got.beg[want_bad] == -1).all()
        assert (np.diff(got.off)[want_bad] == 0).all() and got.off[0] == 0                # an empty text
        assert got.rec[~want_bad].tobytes() == ref.rec.tobytes(), chunk                  # neighbours are unchanged
        assert got.beg[~want_bad].tobytes() == ref.beg.tobytes()
        assert [t for t, b in zip(_texts(got, n), want_bad) if not b] == ref_texts
        assert got.off[n] == ref.off[64] and got.text[:got.off[n]].tobytes() == ref.text[:ref.off[64]].tobytes()
        assert (got.text[got.off[n]:] == FILL).all()
    # score mode: the strand bytes are descriptors like the rest
    plain = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, pkg.WANT_STATS, pm.inner)
    clean_scores = _ex_device(pkg, plain, Q, R, clean, good_strand, 58, 100)
    for chunk in (0, 16):
        got = _ex_device(pkg, plain, Q, R, pairs, strand, 58, 100, chunk)
        assert (got.rec[want_bad] == np.array(pairs_ref.BAD_RECORD)).all() and (got.stats[want_bad] == 0).all()
        assert got.rec[~want_bad].tobytes() == clean_scores.rec.tobytes() and got.stats[~want_bad].tobytes() == clean_scores.stats.tobytes()
    al = pkg.Aligner.new().local().matrix(pm).gap_open(5).gap_extend(2).build()
    with pytest.raises(pkg.BatchError, match=r"pair 0: query: index outside"):
        al.align_pairs(Q, R, pairs, strand=np.minimum(strand, 1), cigar=True)
    with pytest.raises(pkg.BatchError, match=r"pair 64: strand byte 2\b"):
        al.align_pairs(Q, R, pairs, strand=strand, cigar=True)


# --------------------------------------------------------------------------------------------------------------- 6. host entry
def test_host_entry_equals_device_entry(pkg, orc):
    rng = np.random.default_rng(9600)
    pm, om = _dna(pkg, orc)
    ref, reads, pairs, strand = _mapper_case(rng, 128, 20, 250, 4000)
    n = len(pairs)
    cfg = pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, pkg.WANT_CIGAR, pm.inner)
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new([ref])
    strings = pairs_ex_ref.resolve(reads, [ref], pairs, strand)
    mq, mr = _maxima(strings)
    dev = _ex_device(pkg, cfg, Q, R, pairs, strand, mq, mr, 0, 4 * n * 250)
    need = int(dev.off[n])
    out = np.full(n, SENTINEL, dtype=pkg.RECORD_DTYPE)
    beg = np.full((n, 2), SENTINEL, dtype=np.int32)
    coff = np.full(n + 1, -9, dtype=np.int64)
    for chunk in (0, 129):
        cbuf = C.c_void_p()
        opts = pkg.pmx_pairs_opts_t(chunk)
        rc = pkg.lib.pmx_align_pairs_ex(C.byref(cfg), Q.inner, R.inner, n, pairs.ctypes.data, strand.ctypes.data, out.ctypes.data, None,
                                        beg.ctypes.data, C.byref(cbuf), coff.ctypes.data, C.byref(opts))
        assert rc == 0, pkg.lib.pmx_last_error()
        assert "pmx_walkp_kernel" in pkg.lib.pmx_last_kernel().decode()
        assert out.tobytes() == dev.rec.tobytes() and beg.tobytes() == dev.beg.tobytes() and coff.tobytes() == dev.off.tobytes()
        assert C.string_at(cbuf.value, need + 1) == dev.text[:need].tobytes() + b"\0"
        pkg.lib.pmx_free(cbuf)                                                            # the block is the caller's
    # wrapped sets: validation and maxima on the device; no begins asked for
    buf, off = pkg.pack(reads)
    d_buf, d_off = _up(buf), _up(off)
    W = pkg.SeqSet.wrap_device(d_buf.data_ptr(), d_off.data_ptr(), len(reads), len(buf), keep=(d_buf, d_off))
    cbuf = C.c_void_p()
    rc = pkg.lib.pmx_align_pairs_ex(C.byref(cfg), W.inner, R.inner, n, pairs.ctypes.data, strand.ctypes.data, out.ctypes.data, None,
                                    None, C.byref(cbuf), coff.ctypes.data, None)
    assert rc == 0, pkg.lib.pmx_last_error()
    assert out.tobytes() == dev.rec.tobytes() and coff.tobytes() == dev.off.tobytes()
    assert C.string_at(cbuf.value, need) == dev.text[:need].tobytes()
    pkg.lib.pmx_free(cbuf)
    # the Python mirror
    al = pkg.Aligner.new().semi_global().matrix(pm).gap_open(5).gap_extend(2).build()
    rec, cigars, begins = al.align_pairs(Q, R, pairs, strand=strand, cigar=True, chunk_pairs=100)
    assert rec.tobytes() == dev.rec.tobytes() and cigars == _texts(dev, n) and begins.tobytes() == dev.beg.tobytes()
    assert begins.dtype == np.int32 and begins.shape == (n, 2)
    fwd = al.align_pairs(Q, R, pairs)                                                     # the defaults keep today's return value
    assert isinstance(fwd, np.ndarray) and fwd.dtype == pkg.RECORD_DTYPE
    assert al.align_pairs(Q, R, pairs, strand=np.zeros(n, dtype=np.uint8)).tobytes() == fwd.tobytes()
    # a text that does not fit the first estimate (half a byte per symbol + 16 per pair): alternating = and X, two bytes per column
    A, B = pkg.SeqSet.new([b"AC" * 70]), pkg.SeqSet.new([b"A" * 140])
    odd = pairs_ref.pairs_array([(0, 0, int(rng.integers(0, 40)), 100, int(rng.integers(0, 40)), 100) for _ in range(50)])
    ncfg = pkg.pmx_config_t(pkg.MODE_NW, 0, 5, 2, 0, pkg.WANT_CIGAR, pm.inner)
    ndev = _ex_device(pkg, ncfg, A, B, odd, None, 100, 100, 0, 50 * 400)
    assert ndev.off[50] > (50 * 200) // 2 + 16 * 50 + 256
    rec, cigars, begins = pkg.Aligner.new().global_().matrix(pm).gap_open(5).gap_extend(2).build().align_pairs(A, B, odd, cigar=True)
    assert rec.tobytes() == ndev.rec.tobytes() and cigars == _texts(ndev, 50) and (begins == 0).all()


def test_outside_the_device_cigar_window_is_refused(pkg, orc):
    """width 8, open < extend, a PSSM, max_qlen = 1024: both entries refuse before any alignment runs and write nothing"""
    rng = np.random.default_rng(9650)
    pm, om = _dna(pkg, orc)
    b62, _ = _b62(pkg, orc)
    long_read = random_seqs(rng, 1, 1024, 1024)[0]
    seqs = random_seqs(rng, 8, 40, 40) + [long_read]
    prots = random_seqs(rng, 8, 40, 40, AA)
    S, P = pkg.SeqSet.new(seqs), pkg.SeqSet.new(prots)
    short = pairs_ref.pairs_array([(k, (k + 1) % 8) for k in range(8)])
    long_ = pairs_ref.pairs_array([(k, (k + 1) % 8) for k in range(7)] + [(8, 0)])
    pssm = b62.to_pssm(prots[0])
    W = pkg.WANT_CIGAR
    cases = [(pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 8, W, pm.inner), S, short, 40),                          # width 8
             (pkg.pmx_config_t(pkg.MODE_SG, 15, 1, 3, 0, W, pm.inner), S, short, 40),                          # open < extend
             (pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, W, pssm.inner), P, short, 40),                        # a PSSM
             (pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, W, pm.inner), S, long_, 1024)]                        # queries beyond 1023 symbols
    for cfg, X, pairs, mq in cases:
        n = len(pairs)
        with pytest.raises(pkg.BatchError, match=NO_ROAD):
            _ex_device(pkg, cfg, X, X, pairs, None, mq, 40, 0, 4096)
        import torch
        rec, beg = _full((n, 4), SENTINEL, torch.int32), _full((n, 2), SENTINEL, torch.int32)
        text, off = _full((4096,), FILL, torch.uint8), _full((n + 1,), -9, torch.int64)
        d_pairs = _up(pairs.view(np.uint8))
        rc = pkg.lib.pmx_align_pairs_ex_device(C.byref(cfg), X.inner, X.inner, n, d_pairs.data_ptr(), None, mq, 40, rec.data_ptr(), None,
                                               beg.data_ptr(), text.data_ptr(), 4096, off.data_ptr(), _stream(), None)
        _sync()
        assert rc == -1 and NO_ROAD in pkg.lib.pmx_last_error().decode()
        assert (rec.cpu().numpy() == SENTINEL).all() and (beg.cpu().numpy() == SENTINEL).all()
        assert (text.cpu().numpy() == FILL).all() and (off.cpu().numpy() == -9).all()
        out = np.full(n, SENTINEL, dtype=pkg.RECORD_DTYPE)
        coff = np.full(n + 1, -9, dtype=np.int64)
        cbuf = C.c_void_p()
        rc = pkg.lib.pmx_align_pairs_ex(C.byref(cfg), X.inner, X.inner, n, pairs.ctypes.data, None, out.ctypes.data, None, None,
                                        C.byref(cbuf), coff.ctypes.data, None)
        assert rc == -1 and NO_ROAD in pkg.lib.pmx_last_error().decode()
        assert cbuf.value is None and out.tobytes() == np.full(n, SENTINEL, dtype=pkg.RECORD_DTYPE).tobytes() and (coff[1:] == -9).all()
    # the same queries one symbol shorter are inside the window
    ok_pairs = pairs_ref.pairs_array([(8, 0, 0, 1023, 0, -1), (8, 1, 1, 1023, 0, -1)])
    got = _ex_device(pkg, cases[3][0], S, S, ok_pairs, np.array([1, 0], dtype=np.uint8), 1023, 40, 0, 8192)
    assert "pmx_walkp_kernel" in got.kernel and (got.rec[:, 3] == 0).all() and got.off[2] > 0


# ------------------------------------------------------------------------------------------- 7. repeatability, scratch reuse
def test_small_large_small_on_one_thread(pkg, orc):
    rng = np.random.default_rng(9700)
    pm, om = _dna(pkg, orc)
    ref, reads, pairs, strand = _mapper_case(rng, 128, 20, 250, 4000)
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new([ref])
    cfg = pkg.pmx_config_t(pkg.MODE_SG, 15, 5, 2, 0, pkg.WANT_CIGAR, pm.inner)
    big = np.concatenate([pairs] * 8); big_strand = np.concatenate([strand] * 8)

    def run(p, s, chunk):
        e = _ex_device(pkg, cfg, Q, R, p, s, 250, 255, chunk, 2 * len(p) * 250)
        return e.rec.tobytes(), e.off.tobytes(), e.text.tobytes(), e.beg.tobytes()

    small = run(pairs[:40], strand[:40], 0)
    large = run(big, big_strand, 1000)
    assert run(pairs[:40], strand[:40], 0) == small                                       # after the scratch grew
    assert run(pairs[:40], strand[:40], 16) == small
    assert run(big, big_strand, 1000) == large
    assert run(big, big_strand, 0) == large
    n = len(pairs)
    again = _ex_device(pkg, cfg, Q, R, big, big_strand, 250, 255, 0, 2 * len(big) * 250)
    assert again.rec[:n].tobytes() == again.rec[n:2 * n].tobytes() == again.rec[7 * n:].tobytes()    # the same pairs, the same records
