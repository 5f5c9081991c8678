"""The reference-side translated set entries (`-m gpu`): protein queries against nucleotide references translated in six frames,
BLOSUM62 with gaps 11 / 1.  The gather hook byte for byte against tests/translate_ref_side.py; every single-frame mode against the
untranslated entry over a reference set translated on the host; the multi-frame modes against the fold of the single-frame results;
search and top-K on folded records; the query-side entry over the exchanged sets as a check that needs no host translation; the
CIGAR route; the neighbouring entries; the host entries.  Every comparison is exact; every output buffer starts as a sentinel."""
import numpy as np
import pytest

import pairs_ref
import set_search_ref
import translate_ref_side as ref
from pairs_ex_ref import revcomp
from util import random_seqs, AA
from test_gpu_translate import (SENTINEL, FILL, INT32_MAX, INT32_MIN, LIST, RECT, FWD3, REV3, ALL, BAD, _up, _full, _stream, _sync, _ptr, _b62, _cfg,
                                _pairs_up, _plain, _same_fold, _oracle, _same_search, _same_topk, _identical, _level, Got, back_translate, planted_sets)
from test_gpu_translate import _translated as _translated_query, _search as _search_query

pytestmark = pytest.mark.gpu


def _translated(pkg, cfg, Q, R, pairs, mode, mq, mr, chunk=0, frames=None):
    """pmx_align_pairs_translated_ref_device -> records, statistics, frame bytes, kernel"""
    import torch
    n = len(pairs)
    stats = bool(cfg.want & pkg.WANT_STATS)
    rec = _full((n + 2, 4), SENTINEL, torch.int32)
    st = _full((n + 2, 3), SENTINEL, torch.int32) if stats else None
    won = _full((n + 2,), FILL, torch.uint8)
    d_pairs = _pairs_up(pairs)
    d_frame = _up(np.asarray(frames, dtype=np.uint8)) if frames is not None else None
    pkg.align_pairs_translated_ref_device(cfg, Q, R, n, d_pairs.data_ptr(), _ptr(d_frame), mode, mq, mr, rec.data_ptr(), _ptr(st), won.data_ptr(),
                                          _stream(), chunk)
    kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    rec, won = rec.cpu().numpy(), won.cpu().numpy()
    assert (rec[n:] == SENTINEL).all() and (won[n:] == FILL).all()
    if stats:
        st = st.cpu().numpy()
        assert (st[n:] == SENTINEL).all()
        st = st[:n]
    return rec[:n], st, won[:n], kernel


# ------------------------------------------------------------------------------------------------------------ 1. the gather, byte for byte
def _gather(pkg, Q, R, pairs, frames, mq, mr, qcap, rcap, qsize, rsize):
    """pmx_gather_pairs_translated_ref_device into buffers of qsize / rsize bytes with 16 canary bytes on either side"""
    import torch
    n = len(pairs)
    qout = _full((qsize + 32,), FILL, torch.uint8); rout = _full((rsize + 32,), FILL, torch.uint8)
    qoff = _full((n + 3,), SENTINEL, torch.int64); roff = _full((n + 3,), SENTINEL, torch.int64)
    ok = _full((n + 2,), FILL, torch.uint8)
    d_pairs = _pairs_up(pairs)
    d_frame = _up(np.asarray(frames, dtype=np.uint8))
    pkg.gather_pairs_translated_ref_device(Q, R, n, d_pairs.data_ptr(), d_frame.data_ptr(), mq, mr, qout.data_ptr() + 16, qcap, qoff.data_ptr(),
                                           rout.data_ptr() + 16, rcap, roff.data_ptr(), ok.data_ptr(), _stream())
    _sync()
    return [t.cpu().numpy() for t in (qout, qoff, rout, roff, ok)]


LONG = (195, 204, 210, 215)                                                                        # 65 .. 71 letters


def gather_case():
    """the sets, descriptors, frame bytes and maxima of the gather test, and what the model makes of them"""
    rng = np.random.default_rng(14200)
    letters = np.frombuffer(b"ACGTACGTACGTACGTacgtUuN-", dtype=np.uint8)
    rseqs = [letters[rng.integers(0, len(letters), size=l)].tobytes() for l in list(range(1, 46)) + list(LONG)]      # 1 .. 45 nt: every W mod 3, W < 3, W = 3
    rseqs[20] = b"TAAccTAGttTGAggTTActa"                                                           # stops on both strands
    qseqs = random_seqs(rng, 9, 1, 9, AA)
    mq, mr = 9, 70                                                                                 # 215 nt: 71 letters in every frame, too long
    nr = len(rseqs)
    rows, frames = [], []
    for j in range(nr):                                                                            # the first and the last sequence of the set included
        for f in range(6):
            rows.append(((j + f) % 9, j)); frames.append(f)
    for j in (0, 3, 4, 5, 9, 17, 29, 43, 44, 45, 46, 47, 48):                                      # windows at every start 1 .. 3, both ways of giving a length
        for b in (1, 2, 3):
            for f in range(6):
                if b < len(rseqs[j]):
                    rows.append((j % 9, j, 0, -1, b, -1 if f % 2 else len(rseqs[j]) - b)); frames.append(f)
    rows.append((8, 30, 1, 3, 2, -1)); frames.append(4)                                            # a query window beside a reference window
    at = len(rows) // 2
    for row, f in (((9, 0), 0), ((3, nr), 2), ((1, 5, 0, -1, 0, 50), 1), ((1, 7), 6), ((2, 8), 255)):       # bad descriptors and frame bytes between good pairs
        rows.insert(at, row); frames.insert(at, f); at += 7
    rows.append((4, 30)); frames.append(1)                                                         # a last window of several letters, for the capacity cut
    pairs = pairs_ref.pairs_array(rows)
    return qseqs, rseqs, pairs, frames, mq, mr, ref.resolve(qseqs, rseqs, pairs, frames, mq, mr)


def test_gather_byte_for_byte(pkg):
    qseqs, rseqs, pairs, frames, mq, mr, want = gather_case()
    n = len(pairs)
    lens = [len(w[1]) for w in want if w is not None]
    assert set(range(1, 16)) <= set(lens) and max(lens) == mr and sum(w is None for w in want) > 40      # translated lengths 1 .. 15 and the maximum; frames that do not exist
    too_long = [k for k in range(n) if want[k] is None and frames[k] <= 5 and pairs[k]["r"] == 48 and pairs[k]["r_beg"] == 0 and pairs[k]["q"] < 9]
    assert len(too_long) == 6 and all(ref.tlen(215, f) == mr + 1 for f in range(6))                # one length is too long, in every frame
    assert any(w is not None and b"*" in w[1] for w, f in zip(want, frames) if f < 3) and any(w is not None and b"*" in w[1] for w, f in zip(want, frames) if f >= 3)
    assert any(w is not None and b"X" in w[1] for w in want)
    qwant = b"".join(w[0] if w else b"\0" for w in want); rwant = b"".join(w[1] if w else b"\0" for w in want)
    qoffw = np.concatenate([[0], np.cumsum([len(w[0]) if w else 1 for w in want])]); roffw = np.concatenate([[0], np.cumsum([len(w[1]) if w else 1 for w in want])])
    heads = {int(o) % 4 for o, w in zip(roffw, want) if w}; tails = {int(o) % 4 for o, w in zip(roffw[1:], want) if w}
    assert heads == tails == {0, 1, 2, 3}                                                          # the reference side's destinations: every phase at head and tail
    # the lane loop's second trip (16 lanes, so a 17th aligned destination dword), in a forward and in a reverse frame
    dwords = [((len(w[1]) - (-int(o)) % 4) >> 2, f) for o, w, f in zip(roffw, want, frames) if w]
    assert any(d >= 17 and f < 3 for d, f in dwords) and any(d >= 17 and f >= 3 for d, f in dwords)
    assert sum(len(w[1]) >= 65 for w in want if w) >= 8
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    qb, qo = pkg.pack(qseqs); rb, ro = pkg.pack(rseqs)
    keep = (_up(qb), _up(qo), _up(rb), _up(ro))                                                     # wrapped: exactly `bytes` bytes, no slack behind the set
    WQ = pkg.SeqSet.wrap_device(keep[0].data_ptr(), keep[1].data_ptr(), len(qseqs), len(qb), keep=keep[:2])
    WR = pkg.SeqSet.wrap_device(keep[2].data_ptr(), keep[3].data_ptr(), len(rseqs), len(rb), keep=keep[2:])
    for SQ, SR in ((Q, R), (WQ, WR)):
        qout, qoff, rout, roff, ok = _gather(pkg, SQ, SR, pairs, frames, mq, mr, len(qwant), len(rwant), len(qwant), len(rwant))
        assert qoff[:n + 1].tolist() == qoffw.tolist() and roff[:n + 1].tolist() == roffw.tolist()
        assert (qoff[n + 1:] == SENTINEL).all() and (roff[n + 1:] == SENTINEL).all()
        assert ok[:n].tolist() == [1 if w else 0 for w in want] and (ok[n:] == FILL).all()
        assert rout[16:16 + len(rwant)].tobytes() == rwant                                          # the translated side
        assert qout[16:16 + len(qwant)].tobytes() == qwant                                          # the query side: a plain copy
        assert (qout[:16] == FILL).all() and (qout[16 + len(qwant):] == FILL).all()
        assert (rout[:16] == FILL).all() and (rout[16 + len(rwant):] == FILL).all()
    # a capacity that cuts the last window: offsets in full, the window not written, nothing beyond
    assert want[-1] is not None and len(want[-1][0]) > 2 and len(want[-1][1]) > 2
    qcap, rcap = len(qwant) - 1, len(rwant) - 2
    qout, qoff, rout, roff, ok = _gather(pkg, Q, R, pairs, frames, mq, mr, qcap, rcap, len(qwant), len(rwant))
    assert qoff[:n + 1].tolist() == qoffw.tolist() and roff[:n + 1].tolist() == roffw.tolist()
    qcut, rcut = int(qoffw[-2]), int(roffw[-2])
    assert qout[16:16 + qcut].tobytes() == qwant[:qcut] and (qout[16 + qcut:] == FILL).all() and (qout[:16] == FILL).all()
    assert rout[16:16 + rcut].tobytes() == rwant[:rcut] and (rout[16 + rcut:] == FILL).all() and (rout[:16] == FILL).all()


# ------------------------------------------------------------------------------------------------ the sets of cases 2 to 8
NQ, NR = 48, 64                                                                                    # proteins as queries, nucleotide references
MQ, MR = 60, 40


def windowed_pairs(prots, nucs):
    """240 pairs with windows on both sides, every reference window at least 6 nt: all six frames exist"""
    rng = np.random.default_rng(14400)
    rows = []
    for k in range(240):
        i, j = int(rng.integers(0, NQ)), int(rng.integers(0, NR))
        if k % 3 == 0:
            i = j % NQ
        rb = int(rng.integers(0, 8)); rl = int(rng.integers(6, len(nucs[j]) - rb + 1))
        qb = int(rng.integers(0, 4)); ql = int(rng.integers(3, len(prots[i]) - qb + 1))
        rows.append((i, j, qb, ql, rb, rl if k % 2 else (-1 if k % 4 else len(nucs[j]) - rb)))
    return pairs_ref.pairs_array(rows)


class Planted:
    pass


@pytest.fixture(scope="module")
def planted(pkg, orc):
    """planted_sets() of the query-side test with the roles exchanged, the rectangle, the windowed list and, per mode and frame, the
    yardstick: pmx_align_pairs_device over the reference set translated on the host in that frame, with statistics -- computed once,
    shared, left unchanged"""
    p = Planted()
    p.pm, p.om = _b62(pkg, orc)
    p.nucs, p.prots = planted_sets()                                                               # nucleotide j codes for protein j % 48 in frame j % 6
    assert len(p.prots) == NQ and len(p.nucs) == NR
    p.Q, p.R = pkg.SeqSet.new(p.prots), pkg.SeqSet.new(p.nucs)
    p.rect = set_search_ref.rect_pairs_descriptors(NR, 0, NQ * NR)
    p.win = windowed_pairs(p.prots, p.nucs)
    p.Rf = [pkg.SeqSet.new([ref.translate(s, f) for s in p.nucs]) for f in range(6)]
    # the windowed list against sets of translated windows: pair k's reference is sequence k of the set, whole
    wr = [p.nucs[int(d["r"])][int(d["r_beg"]):(int(d["r_beg"]) + int(d["r_len"])) if d["r_len"] >= 0 else None] for d in p.win]
    p.win_strings = wr
    p.Wf = [pkg.SeqSet.new([ref.translate(s, f) for s in wr]) for f in range(6)]
    p.win_t = p.win.copy()
    p.win_t["r"] = np.arange(len(p.win)); p.win_t["r_beg"] = 0; p.win_t["r_len"] = -1
    p.single = {}
    for mode in ("sw", "sg"):
        cfg = _cfg(pkg, p.pm, mode, pkg.WANT_STATS)
        for f in range(6):
            p.single[mode, "rect", f] = _plain(pkg, cfg, p.Q, p.Rf[f], p.rect, MQ, MR)
            p.single[mode, "win", f] = _plain(pkg, cfg, p.Q, p.Wf[f], p.win_t, MQ, MR)
    return p


def _folded(p, mode, which, frames=(0, 1, 2, 3, 4, 5)):
    recs = np.stack([p.single[mode, which, f][0] for f in frames])
    stats = np.stack([p.single[mode, which, f][1] for f in frames])
    return ref.fold(recs, np.ones(recs.shape[:2], dtype=bool), stats, frames)


# ------------------------------------------------------------------------------------------------------ 2. single-frame equivalence
@pytest.mark.parametrize("mode", ["sw", "sg"])
def test_single_frame_equals_host_translated_set(pkg, orc, planted, mode):
    p = planted
    cfg_s = _cfg(pkg, p.pm, mode, pkg.WANT_STATS)
    cfg = _cfg(pkg, p.pm, mode)
    for f in range(6):
        for which, pairs in (("rect", p.rect), ("win", p.win)):
            wrec, wst = p.single[mode, which, f]
            assert (wrec[:, 3] == 0).all()
            for chunk in ((0, 500) if which == "rect" else (0, 37)):                              # 37: seven chunks, both sets of chunk buffers
                rec, st, won, kernel = _translated(pkg, cfg_s, p.Q, p.R, pairs, f, MQ, MR, chunk)
                assert rec.tobytes() == wrec.tobytes() and st.tobytes() == wst.tobytes() and (won == f).all() and kernel
        rec, _, won, _ = _translated(pkg, cfg, p.Q, p.R, p.win, f, MQ, MR, 100)                   # without statistics
        assert rec.tobytes() == p.single[mode, "win", f][0].tobytes()
        rec, _, won, _ = _translated(pkg, cfg, p.Q, p.R, p.win, 0, MQ, MR, 37, frames=[f] * len(p.win))      # the frame as a byte per pair
        assert rec.tobytes() == p.single[mode, "win", f][0].tobytes() and (won == f).all()
        # a sample of the yardstick against the oracle on the translated strings
        sample = np.arange(f, NQ * NR, 53)
        strings = [(p.prots[int(d["q"])], ref.translate(p.nucs[int(d["r"])], f)) for d in p.rect[sample]]
        want = _oracle(orc, cfg, p.om, strings)
        assert (p.single[mode, "rect", f][0][sample][:, :3] == want[:, :3]).all()
        wsample = np.arange(f, len(p.win), 7)
        strings = [(pairs_ref.resolve_side(p.prots, p.win[k]["q"], p.win[k]["q_beg"], p.win[k]["q_len"]), ref.translate(p.win_strings[k], f)) for k in wsample]
        want = _oracle(orc, cfg, p.om, strings)
        assert (p.single[mode, "win", f][0][wsample][:, :3] == want[:, :3]).all()


# --------------------------------------------------------------------------------------------------------------------------- 3. the fold
@pytest.mark.parametrize("mode", ["sw", "sg"])
def test_fold_equals_the_rule_over_single_frames(pkg, planted, mode):
    p = planted
    cfg = _cfg(pkg, p.pm, mode, pkg.WANT_STATS)
    for fm, frames in ((ALL, (0, 1, 2, 3, 4, 5)), (FWD3, (0, 1, 2)), (REV3, (3, 4, 5))):
        for which, pairs in (("rect", p.rect), ("win", p.win)):
            want = _folded(p, mode, which, frames)
            assert set(want[2].tolist()) == set(frames)                                           # no vacuous pass: every frame wins somewhere
            for chunk in ((0, 64, 1000) if which == "rect" else (0, 7)):
                _same_fold(_translated(pkg, cfg, p.Q, p.R, pairs, fm, MQ, MR, chunk), want)
    if mode == "sw":
        rec, _, won = _folded(p, mode, "rect")
        home = np.array([(j % NQ) * NR + j for j in range(NR)])                                   # the protein reference j was built from, against it
        assert (won[home] == np.arange(NR) % 6).sum() >= NR - 2                                   # ALL returns the planted frame ...
        for j in range(NR):
            if won[home[j]] == j % 6:
                assert rec[home[j]].tolist() == p.single[mode, "rect", j % 6][0][home[j]].tolist()      # ... and that frame's record


def test_fold_ties_missing_frames_and_bad_pairs(pkg):
    rng = np.random.default_rng(14500)
    pm = pkg.Matrix.from_name("blosum62")
    prot = random_seqs(rng, 1, 30, 30, AA)[0]
    half = back_translate(rng, prot[5:17])                                                        # 36 nt
    pal = half + revcomp(half)                                                                    # equals its reverse complement: frames f and f + 3 read the same letters
    assert pal == revcomp(pal) and all(ref.translate(pal, f) == ref.translate(pal, f + 3) for f in range(3))
    nucs = [pal, b"ATGG", b"AT", back_translate(rng, prot[:20]), b"G" + back_translate(rng, prot[3:25]), pal[1:], b"ACG", b"A", b"ATGGC"]      # windows of 1 .. 5 nt among them
    prots = [prot] + random_seqs(rng, 3, 10, 40, AA)
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(nucs)
    rows = [(i, j) for j in range(len(nucs)) for i in range(len(prots))]
    rows.insert(9, (0, len(nucs))); rows.insert(14, (1, 0, 50, 5, 0, -1))                         # bad descriptors between good pairs
    pairs = pairs_ref.pairs_array(rows)
    n = len(pairs)
    for mode in ("sw", "sg"):
        cfg = _cfg(pkg, pm, mode, pkg.WANT_STATS)
        single = [_translated(pkg, cfg, Q, R, pairs, f, 40, 30) for f in range(6)]
        w = [len(nucs[int(d["r"])]) if 0 <= d["r"] < len(nucs) and d["q_beg"] == 0 else 0 for d in pairs]
        exists = np.array([[ref.tlen(x, f) >= 1 for x in w] for f in range(6)])
        for f in range(6):                                                                        # a frame that does not exist: the bad record, frame 0
            for k in range(n):
                if not exists[f][k]:
                    assert single[f][0][k].tolist() == BAD and single[f][1][k].tolist() == [0, 0, 0] and single[f][2][k] == 0
                else:
                    assert single[f][0][k][3] == 0 and single[f][2][k] == f
        recs = np.stack([s[0] for s in single]); stats = np.stack([s[1] for s in single])
        for fm, frames in ((ALL, (0, 1, 2, 3, 4, 5)), (FWD3, (0, 1, 2)), (REV3, (3, 4, 5))):
            want = ref.fold(recs[list(frames)], exists[list(frames)], stats[list(frames)], frames)
            for chunk in (0, 5, 1):
                _same_fold(_translated(pkg, cfg, Q, R, pairs, fm, 40, 30, chunk), want)
        rec, st, won, _ = _translated(pkg, cfg, Q, R, pairs, ALL, 40, 30, 4)
        k = rows.index((0, 0))
        assert single[0][0][k].tolist() == single[3][0][k].tolist() and single[0][0][k][0] > 30 and won[k] == 0      # equal scores in two frames: the lowest
        assert _translated(pkg, cfg, Q, R, pairs, REV3, 40, 30)[2][k] == 3
        k = rows.index((0, 1))                                                                    # W = 4: frames 0, 1, 3, 4 exist
        assert exists[:, k].tolist() == [True, True, False, True, True, False] and rec[k][3] == 0 and won[k] in (0, 1, 3, 4)
        k = rows.index((0, 6))                                                                    # W = 3: frames 0 and 3
        assert exists[:, k].tolist() == [True, False, False, True, False, False] and rec[k][3] == 0
        assert _translated(pkg, cfg, Q, R, pairs[k:k + 1], 1, 40, 30)[0][0].tolist() == BAD
        k = rows.index((0, 8))                                                                    # W = 5: all six
        assert exists[:, k].all() and rec[k][3] == 0
        for k in (rows.index((0, 2)), rows.index((0, 7)), 9, 14):                                 # W = 2, W = 1 and the bad descriptors
            assert rec[k].tolist() == BAD and st[k].tolist() == [0, 0, 0] and won[k] == 0
        # a frame longer than max_rlen makes the pair bad, its neighbours are unaffected
        short = _translated(pkg, cfg, Q, R, pairs, ALL, 40, 23)
        long_ = np.array([x // 3 > 23 for x in w])
        assert long_.any() and all(short[0][k].tolist() == BAD for k in np.nonzero(long_)[0])
        assert short[0][~long_].tobytes() == rec[~long_].tobytes() and short[2][~long_].tolist() == won[~long_].tolist()


# ------------------------------------------------------------------------------------------------- 4. search and top-K on folded records
def _search(pkg, cfg, Q, R, shape, first, n, pairs, mq, mr, min_score, capacity, mode, chunk=0, plain=False):
    """pmx_search_pairs_translated_ref_device, or (plain) pmx_search_pairs_device"""
    import torch
    stats = bool(cfg.want & pkg.WANT_STATS)
    slots = capacity + 3
    hp = _full((slots * 32,), FILL, torch.uint8)
    hi = _full((slots,), SENTINEL, torch.int64)
    hr = _full((slots, 4), SENTINEL, torch.int32)
    hs = _full((slots, 3), SENTINEL, torch.int32) if stats else None
    hb = _full((slots,), FILL, torch.uint8) if not plain else None
    cnt = _full((2,), SENTINEL, torch.int64)
    d_pairs = _pairs_up(pairs) if shape == LIST and n else None
    if plain:
        pkg.search_pairs_device(cfg, Q, R, shape, first, n, _ptr(d_pairs), mq, mr, min_score, hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), _ptr(hs),
                                capacity, cnt.data_ptr(), _stream(), chunk)
    else:
        pkg.search_pairs_translated_ref_device(cfg, Q, R, shape, first, n, _ptr(d_pairs), mq, mr, min_score, hp.data_ptr(), hi.data_ptr(), hr.data_ptr(),
                                               _ptr(hs), capacity, cnt.data_ptr(), mode, _ptr(hb), _stream(), chunk)
    g = Got()
    g.kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    host = lambda t: t.cpu().numpy() if t is not None else None
    g.pairs, g.index, g.recs, g.stats, g.frame, g.counts = host(hp).view(pairs_ref.PAIR_DTYPE), host(hi), host(hr), host(hs), host(hb), host(cnt)
    g.d_pairs, g.d_frame = hp, hb
    g.all = [a for a in (g.pairs, g.index, g.recs, g.stats, g.counts) if a is not None]
    return g


def _gathered(pkg, p, d_pairs, d_frame, h):
    """the hits' descriptors and frame bytes, as they lie on the device, through the gather hook: validity bytes and the packed sides"""
    import torch
    qout = _full((h * MQ + 16,), FILL, torch.uint8); rout = _full((h * MR + 16,), FILL, torch.uint8)
    qoff = _full((h + 1,), SENTINEL, torch.int64); roff = _full((h + 1,), SENTINEL, torch.int64)
    ok = _full((h,), FILL, torch.uint8)
    pkg.gather_pairs_translated_ref_device(p.Q, p.R, h, d_pairs.data_ptr(), d_frame.data_ptr(), MQ, MR, qout.data_ptr(), h * MQ, qoff.data_ptr(),
                                           rout.data_ptr(), h * MR, roff.data_ptr(), ok.data_ptr(), _stream())
    return qout, qoff, rout, roff, ok


def _valid_for_the_gather(pkg, p, g, h):
    qout, qoff, rout, roff, ok = _gathered(pkg, p, g.d_pairs, g.d_frame, h)
    _sync()
    strings = ref.resolve(p.prots, p.nucs, g.pairs[:h], g.frame[:h], MQ, MR)
    assert all(s is not None for s in strings) and (ok.cpu().numpy() == 1).all()
    qoff, roff = qoff.cpu().numpy(), roff.cpu().numpy()
    assert qout.cpu().numpy()[:qoff[h]].tobytes() == b"".join(s[0] for s in strings)
    assert rout.cpu().numpy()[:roff[h]].tobytes() == b"".join(s[1] for s in strings)


def test_search_on_folded_records(pkg, planted):
    p = planted
    cfg = _cfg(pkg, p.pm, "sw", pkg.WANT_STATS)
    first, n = 5, NQ * NR - 9                                                                     # a window that starts and ends inside a row
    for fm, frames in ((ALL, (0, 1, 2, 3, 4, 5)), (REV3, (3, 4, 5))):
        rec, st, won = _folded(p, "sw", "rect", frames)
        ms = _level(rec[:, 0])
        want = ref.search(rec[first:first + n], won[first:first + n], ms, first, p.rect[first:first + n], st[first:first + n])
        assert 100 <= want["passing"] <= 200 and len(set(want["frame"].tolist())) == len(frames)
        runs = [_search(pkg, cfg, p.Q, p.R, RECT, first, n, None, MQ, MR, ms, n, fm, chunk) for chunk in (64, 192, 0, 64)]
        for g in runs:
            _same_search(g, want, n)
            _identical(g, runs[0]); assert g.frame.tobytes() == runs[0].frame.tobytes()
        assert (runs[0].recs[:want["passing"], 3] == 0).all()                                     # the frame bits do not reach the caller
        _valid_for_the_gather(pkg, p, runs[0], want["passing"])
        for cap in (0, 1, 7, want["passing"], want["passing"] + 5):                               # a capacity reached inside a chunk
            cut = ref.search(rec[first:first + n], won[first:first + n], ms, first, p.rect[first:first + n], st[first:first + n], capacity=cap)
            _same_search(_search(pkg, cfg, p.Q, p.R, RECT, first, n, None, MQ, MR, ms, cap, fm, 192), cut, cap)
    # the windowed list
    rec, st, won = _folded(p, "sw", "win")
    for ms in (INT32_MAX, _level(rec[:, 0], 8), INT32_MIN):
        want = ref.search(rec, won, ms, 0, p.win, st)
        for chunk in (64, 0):
            _same_search(_search(pkg, cfg, p.Q, p.R, LIST, 0, len(p.win), p.win, MQ, MR, ms, len(p.win), ALL, chunk), want, len(p.win))
    # a single-frame mode is the untranslated entry over the host-translated set, byte for byte
    plain = _cfg(pkg, p.pm, "sw")
    for f in (1, 4):
        ms = _level(p.single["sw", "rect", f][0][:, 0])
        for chunk in (0, 192):
            t = _search(pkg, plain, p.Q, p.R, RECT, first, n, None, MQ, MR, ms, n, f, chunk)
            old = _search(pkg, plain, p.Q, p.Rf[f], RECT, first, n, None, MQ, MR, ms, n, f, chunk, plain=True)
            _identical(t, old)
            h = int(t.counts[1])
            assert h > 50 and (t.frame[:h] == f).all()
    # the host entry: max_hits and two slicings give the same hits
    al = pkg.Aligner.new().local().matrix(p.pm).gap_open(11).gap_extend(1).build()
    rec, st, won = _folded(p, "sw", "rect")
    ms = _level(rec[:, 0])
    for kw in ({}, {"slice_pairs": 1000}, {"slice_pairs": 333, "chunk_pairs": 100}, {"max_hits": 9}):
        w = ref.search(rec, won, ms, 0, p.rect, st, capacity=kw.get("max_hits"))
        h = al.search_pairs(p.Q, p.R, min_score=ms, ref_frame="all", stats=True, **kw)
        assert h.n_passing == w["passing"] and h.n_hits == w["written"]
        assert h.records.view(np.int32).tobytes() == w["records"].tobytes() and h.frame.tolist() == w["frame"].tolist()
        assert h.index.tolist() == w["index"].tolist() and h.stats.view(np.int32).tobytes() == w["stats"].tobytes()


def _topk(pkg, cfg, Q, R, q_first, nq, mq, mr, min_score, k, capacity, mode, chunk=0, plain=False):
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
        pkg.search_topk_device(cfg, Q, R, q_first, nq, mq, mr, min_score, k, False, hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), _ptr(hs),
                               capacity, off.data_ptr(), rp.data_ptr(), cnt.data_ptr(), _stream(), chunk)
    else:
        pkg.search_topk_translated_ref_device(cfg, Q, R, q_first, nq, mq, mr, min_score, k, False, hp.data_ptr(), hi.data_ptr(), hr.data_ptr(),
                                              _ptr(hs), capacity, off.data_ptr(), rp.data_ptr(), cnt.data_ptr(), mode, _ptr(hb), _stream(), chunk)
    g = Got()
    g.kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    host = lambda t: t.cpu().numpy() if t is not None else None
    g.pairs, g.index, g.recs, g.stats, g.frame = host(hp).view(pairs_ref.PAIR_DTYPE), host(hi), host(hr), host(hs), host(hb)
    g.off, g.passing, g.counts = host(off), host(rp), host(cnt)
    g.d_pairs, g.d_frame = hp, hb
    g.all = [a for a in (g.pairs, g.index, g.recs, g.stats, g.off, g.passing, g.counts) if a is not None]
    return g


def test_topk_on_folded_records(pkg, planted):
    p = planted
    cfg = _cfg(pkg, p.pm, "sw", pkg.WANT_STATS)
    rec, st, won = _folded(p, "sw", "rect")
    for k in (1, 3, 70):                                                                          # K > |R|: every reference once
        cap = NQ * min(k, NR)
        want = ref.topk(rec, won, NR, 0, NQ, k, stats=st)
        runs = [_topk(pkg, cfg, p.Q, p.R, 0, NQ, MQ, MR, INT32_MIN, k, cap, ALL, chunk) for chunk in (64, 200, 0)]
        for g in runs:
            _same_topk(g, want, cap, NQ)
            _identical(g, runs[0])
        g = runs[0]
        for i in range(NQ):                                                                       # a reference appears at most once in a row
            row = g.pairs[int(g.off[i]):int(g.off[i + 1])]["r"].tolist()
            assert len(row) == len(set(row)) == min(k, NR)
        assert g.passing[:NQ].tolist() == [NR] * NQ and (g.recs[:cap, 3] == 0).all()             # row_passing counts pairs, not (pair, frame)
        if k == 3:
            _valid_for_the_gather(pkg, p, g, cap)
        if k == 1:                                                                                # the best locus of protein i is one built from it, in its frame
            home = sum(int(g.pairs[i]["r"]) % NQ == i and int(g.frame[i]) == int(g.pairs[i]["r"]) % 6 for i in range(NQ))
            assert home >= NQ - 4
    ms = _level(rec[:, 0])                                                                        # a threshold, a sub-range of rows, a small capacity
    sub = slice(7 * NR, 30 * NR)
    want = ref.topk(rec[sub], won[sub], NR, 7, 23, 3, min_score=ms, stats=st[sub], capacity=11)
    assert 0 < want["row_passing"].sum() < 23 * NR
    _same_topk(_topk(pkg, cfg, p.Q, p.R, 7, 23, MQ, MR, ms, 3, 11, ALL, 100), want, 11, 23)
    plain = _cfg(pkg, p.pm, "sw")
    for f, k, chunk in ((2, 3, 0), (5, 70, 192)):                                                 # single frame: the untranslated entry, byte for byte
        cap = NQ * min(k, NR)
        t = _topk(pkg, plain, p.Q, p.R, 0, NQ, MQ, MR, INT32_MIN, k, cap, f, chunk)
        old = _topk(pkg, plain, p.Q, p.Rf[f], 0, NQ, MQ, MR, INT32_MIN, k, cap, f, chunk, plain=True)
        _identical(t, old)
        assert (t.frame[:cap] == f).all()
    # the host entry: two slicings give the same rows
    al = pkg.Aligner.new().local().matrix(p.pm).gap_open(11).gap_extend(1).build()
    w4 = ref.topk(rec, won, NR, 0, NQ, 4)
    for kw in ({}, {"slice_rows": 5}, {"slice_rows": 1, "chunk_pairs": 30}):
        t = al.search_topk(p.Q, p.R, k=4, ref_frame="all", **kw)
        assert t.row_off.tolist() == w4["row_off"].tolist() and t.row_passing.tolist() == w4["row_passing"].tolist()
        assert t.records.view(np.int32).tobytes() == w4["records"].tobytes() and t.frame.tolist() == w4["frame"].tolist()
        assert t.index.tolist() == w4["index"].tolist() and t.pairs.tobytes() == w4["pairs"].tobytes()


# --------------------------------------------------------------------------------- 5. the query-side entry over the exchanged sets
def test_symmetry_with_the_query_side_entry(pkg, planted):
    """SW with a symmetric matrix scores (P, D) as it scores (D, P): the reference-side entry over (P, D) and the query-side entry
    over (D, P) with every descriptor's sides exchanged agree on score and winning frame -- no host translation between them.  End
    positions transpose and co-optimal ends may differ, so they are not compared."""
    p = planted
    cfg = _cfg(pkg, p.pm, "sw")
    for pairs, chunk in ((p.rect, 0), (p.win, 37)):
        swapped = pairs.copy()
        for a, b in (("q", "r"), ("q_beg", "r_beg"), ("q_len", "r_len")):
            swapped[a], swapped[b] = pairs[b], pairs[a]
        rec, _, won, _ = _translated(pkg, cfg, p.Q, p.R, pairs, ALL, MQ, MR, chunk)
        qrec, _, qwon, _ = _translated_query(pkg, cfg, p.R, p.Q, swapped, ALL, MR, MQ, chunk)
        assert (rec[:, 3] == 0).all() and (qrec[:, 3] == 0).all()
        assert rec[:, 0].tolist() == qrec[:, 0].tolist() and won.tolist() == qwon.tolist()
        assert len(set(won.tolist())) == 6 and rec[:, 0].max() > 40


# ------------------------------------------------------------------------------------------------------------------- 6. the CIGAR route
def test_cigar_route_over_the_hits(pkg, orc, planted):
    import torch
    p = planted
    cfg = _cfg(pkg, p.pm, "sw")
    n = len(p.win)
    rec, _, won = _folded(p, "sw", "win")
    ms = _level(rec[:, 0], 4)
    g = _search(pkg, cfg, p.Q, p.R, LIST, 0, n, p.win, MQ, MR, ms, n, ALL, 64)
    h = int(g.counts[1])
    assert h >= 40 and len(set(g.frame[:h].tolist())) == 6
    # hits -> the gather hook with the hits' frames -> pmx_align_batch_cigar_device over the packed buffers
    qout, qoff, rout, roff, _ = _gathered(pkg, p, g.d_pairs, g.d_frame, h)
    ccfg = _cfg(pkg, p.pm, "sw", pkg.WANT_CIGAR)
    cap = 4 * h * (MQ + MR)
    crec = _full((h, 4), SENTINEL, torch.int32)
    text = _full((cap,), FILL, torch.uint8)
    toff = _full((h + 1,), -9, torch.int64)
    pkg.align_batch_cigar_device(ccfg, h, qout.data_ptr(), qoff.data_ptr(), rout.data_ptr(), roff.data_ptr(), MQ, MR, crec.data_ptr(), text.data_ptr(),
                                 cap, toff.data_ptr(), _stream())
    _sync()
    crec, text, toff = crec.cpu().numpy(), text.cpu().numpy(), toff.cpu().numpy()
    assert crec.tobytes() == g.recs[:h].tobytes()                                                 # score and ends of the hit records
    strings = ref.resolve(p.prots, p.nucs, g.pairs[:h], g.frame[:h], MQ, MR)                      # the host-translated windows
    assert all(s is not None for s in strings)
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    want_text, want = orc.cigar_sample(orc.SW, np.arange(h), qb, qo, rb, ro, 11, 1, p.om)
    assert (crec[:, :3] == want[:, :3]).all() and 0 < toff[h] <= cap
    texts = [text[toff[k]:toff[k + 1]].tobytes().decode() for k in range(h)]
    assert texts == list(want_text)


# --------------------------------------------------------------------------------------------------------- 7. nothing else moved
def test_neighbours_beside_a_reference_side_call(pkg, planted):
    """an untranslated batch and a query-side translated batch and search before and after reference-side calls of the same thread
    (they share its scratch): the same bytes, the same kernels"""
    p = planted
    plain = _cfg(pkg, p.pm, "sw", pkg.WANT_STATS)
    swapped = p.win.copy()
    for a, b in (("q", "r"), ("q_beg", "r_beg"), ("q_len", "r_len")):
        swapped[a], swapped[b] = p.win[b], p.win[a]

    def others():
        out, names = [], []
        rec, st = _plain(pkg, plain, p.Q, p.Rf[2], p.rect, MQ, MR)
        out += [rec, st]; names.append(pkg.lib.pmx_last_kernel().decode())
        got = _translated_query(pkg, plain, p.R, p.Q, swapped, ALL, MR, MQ, 100)
        out += list(got[:3]); names.append(got[3])
        g = _search_query(pkg, plain, p.R, p.Q, RECT, 0, NQ * NR, None, MR, MQ, 45, 200, ALL, 500)
        out += g.all + [g.frame]; names.append(g.kernel)
        return out, names

    before, names = others()
    assert int(before[-2][1]) > 20                                                                # the query-side search has hits
    _translated(pkg, plain, p.Q, p.R, p.rect, ALL, MQ, MR, 500)
    _search(pkg, _cfg(pkg, p.pm, "sw"), p.Q, p.R, RECT, 0, NQ * NR, None, MQ, MR, 40, 100, ALL, 192)
    _topk(pkg, _cfg(pkg, p.pm, "sw"), p.Q, p.R, 0, NQ, MQ, MR, INT32_MIN, 3, 3 * NQ, ALL, 192)
    after, names_after = others()
    assert names_after == names and all(names)
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    assert before[0].tobytes() == p.single["sw", "rect", 2][0].tobytes() and before[1].tobytes() == p.single["sw", "rect", 2][1].tobytes()


# ------------------------------------------------------------------------------------------------- 8. host entries, Python mirror
def test_host_entries_and_python_mirror(pkg, planted):
    p = planted
    al = pkg.Aligner.new().local().matrix(p.pm).gap_open(11).gap_extend(1).build()
    als = pkg.Aligner.new().local().matrix(p.pm).gap_open(11).gap_extend(1).use_stats().build()
    qb, qo = pkg.pack(p.prots); rb, ro = pkg.pack(p.nucs)
    keep = (_up(qb), _up(qo), _up(rb), _up(ro))
    WQ = pkg.SeqSet.wrap_device(keep[0].data_ptr(), keep[1].data_ptr(), NQ, len(qb), keep=keep[:2])
    WR = pkg.SeqSet.wrap_device(keep[2].data_ptr(), keep[3].data_ptr(), NR, len(rb), keep=keep[2:])
    sets = ((p.Q, p.R), (WQ, WR))
    want = _folded(p, "sw", "win")
    dev = _translated(pkg, _cfg(pkg, p.pm, "sw", pkg.WANT_STATS), p.Q, p.R, p.win, ALL, MQ, MR)   # the device entry
    assert dev[0].tobytes() == want[0].tobytes() and dev[1].tobytes() == want[1].tobytes() and dev[2].tolist() == want[2].tolist()
    for Q, R in sets:
        for chunk in (0, 100):
            rec, won = al.align_pairs(Q, R, p.win, chunk_pairs=chunk, ref_frame="all")
            assert rec.view(np.int32).tobytes() == want[0].tobytes() and won.tolist() == want[2].tolist()
        rec, st, won = als.align_pairs(Q, R, p.win, ref_frame=pkg.FRAMES_ALL)
        assert rec.view(np.int32).tobytes() == want[0].tobytes() and st.view(np.int32).tobytes() == want[1].tobytes() and won.tolist() == want[2].tolist()
        rec, won = al.align_pairs(Q, R, p.win, ref_frame=4)
        assert rec.view(np.int32).tobytes() == p.single["sw", "win", 4][0].tobytes() and (won == 4).all()
        rec, won2 = al.align_pairs(Q, R, p.win, ref_frame=want[2])                                # the winners' frames as a byte per pair
        assert rec.view(np.int32).tobytes() == want[0].tobytes() and won2.tolist() == want[2].tolist()
    # search_pairs: the list, then the rectangle
    ms = _level(want[0][:, 0], 8)
    w = ref.search(want[0], want[2], ms, 0, p.win, want[1])
    for kw in ({}, {"slice_pairs": 100}, {"slice_pairs": 64, "chunk_pairs": 7}, {"max_hits": 5}):
        for Q, R in sets:
            h = al.search_pairs(Q, R, min_score=ms, pairs=p.win, ref_frame="all", stats=True, **kw)
            cut = ref.search(want[0], want[2], ms, 0, p.win, want[1], capacity=kw.get("max_hits"))
            assert h.n_passing == w["passing"] and h.n_hits == cut["written"]
            assert h.records.view(np.int32).tobytes() == cut["records"].tobytes() and h.frame.tolist() == cut["frame"].tolist()
            assert h.pairs.tobytes() == cut["pairs"].tobytes() and h.index.tolist() == cut["index"].tolist()
            assert h.stats.view(np.int32).tobytes() == cut["stats"].tobytes() and not h.strand.any()
    for frame, frames in (("all", (0, 1, 2, 3, 4, 5)), ("forward", (0, 1, 2)), (5, (5,))):
        rec, st, won = _folded(p, "sw", "rect", frames)
        rms = _level(rec[:, 0])
        w = ref.search(rec, won, rms, 0, p.rect)
        for Q, R in sets:
            h = al.search_pairs(Q, R, min_score=rms, ref_frame=frame, slice_pairs=1000)
            assert h.n_hits == w["passing"] and h.records.view(np.int32).tobytes() == w["records"].tobytes()
            assert h.frame.tolist() == w["frame"].tolist() and h.index.tolist() == w["index"].tolist()
            t = al.search_topk(Q, R, k=4, ref_frame=frame, slice_rows=7)
            w4 = ref.topk(rec, won, NR, 0, NQ, 4)
            assert t.row_off.tolist() == w4["row_off"].tolist() and t.row_passing.tolist() == w4["row_passing"].tolist()
            assert t.records.view(np.int32).tobytes() == w4["records"].tobytes() and t.frame.tolist() == w4["frame"].tolist()
            assert t.index.tolist() == w4["index"].tolist() and t.pairs.tobytes() == w4["pairs"].tobytes()
    # a bad pair is named, the first one: a descriptor the host sees, and a window without a frame, which only the device sees
    bad = p.win[:20].copy()
    bad[11] = (0, NR, 0, -1, 0, -1)
    bad[15] = (0, NR + 1, 0, -1, 0, -1)
    with pytest.raises(pkg.BatchError, match=r"pair 11: reference: index outside"):
        al.align_pairs(p.Q, p.R, bad, ref_frame="all")
    with pytest.raises(pkg.BatchError, match=r"pair 11: bad descriptor"):
        al.align_pairs(WQ, WR, bad, ref_frame="all")
    bad[11] = (0, 3, 0, -1, 4, 2)                                                                # W = 2: no frame
    bad[15] = (0, 3, 0, -1, 4, 1)
    for Q, R in sets:
        with pytest.raises(pkg.BatchError, match=r"pair 11: bad descriptor"):
            al.align_pairs(Q, R, bad, ref_frame="all")
        with pytest.raises(pkg.BatchError, match=r"pair 11: bad descriptor .* no frame"):
            al.search_pairs(Q, R, pairs=bad, ref_frame="all")
    bad[11] = (0, 3, 0, -1, 4, 4)                                                                # W = 4: frame 2 does not exist, frame 1 does
    bad[15] = p.win[15]
    with pytest.raises(pkg.BatchError, match=r"pair 11: bad descriptor"):
        al.align_pairs(p.Q, p.R, bad, ref_frame=2)
    rec, won = al.align_pairs(p.Q, p.R, bad, ref_frame=1)
    assert rec[11]["flags"] == 0 and won[11] == 1
