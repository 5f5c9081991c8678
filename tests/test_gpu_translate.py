"""The translated set entries (`-m gpu`): nucleotide queries in six frames against proteins, BLOSUM62 with gaps 11 / 1.  The gather
hook byte for byte against tests/translate_ref.py; every single-frame mode against the untranslated entry over a query set translated
on the host; the multi-frame modes against the fold of the single-frame results; search and top-K on folded records; the CIGAR route;
the host entries.  Every comparison is exact; every output buffer starts as a sentinel."""
import numpy as np
import pytest

import pairs_ref
import set_search_ref
import translate_ref as ref
from pairs_ex_ref import revcomp
from util import random_seqs, mutate, AA, golden

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)
LIST, TRI, RECT = 0, 1, 2
FWD3, REV3, ALL = ref.FRAMES_FORWARD, ref.FRAMES_REVERSE, ref.FRAMES_ALL
BAD = list(pairs_ref.BAD_RECORD)


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


def _b62(pkg, orc):
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))


def _cfg(pkg, pm, mode="sw", want=0):
    m = {"sw": (pkg.MODE_SW, 0), "sg": (pkg.MODE_SG, pkg.SG_ALL)}[mode]
    return pkg.pmx_config_t(m[0], m[1], 11, 1, 0, want, pm.inner)


def _pairs_up(pairs):
    return _up(np.ascontiguousarray(pairs).view(np.uint8))


def _plain(pkg, cfg, Q, R, pairs, mq, mr):
    """the yardstick: pmx_align_pairs_device -> records, statistics"""
    import torch
    n = len(pairs)
    stats = bool(cfg.want & pkg.WANT_STATS)
    rec = _full((n, 4), SENTINEL, torch.int32)
    st = _full((n, 3), SENTINEL, torch.int32) if stats else None
    d_pairs = _pairs_up(pairs)
    pkg.align_pairs_device(cfg, Q, R, n, d_pairs.data_ptr(), mq, mr, rec.data_ptr(), _ptr(st), _stream())
    _sync()
    return rec.cpu().numpy(), (st.cpu().numpy() if stats else None)


def _translated(pkg, cfg, Q, R, pairs, mode, mq, mr, chunk=0, frames=None):
    """pmx_align_pairs_translated_device -> records, statistics, frame bytes, kernel"""
    import torch
    n = len(pairs)
    stats = bool(cfg.want & pkg.WANT_STATS)
    rec = _full((n + 2, 4), SENTINEL, torch.int32)
    st = _full((n + 2, 3), SENTINEL, torch.int32) if stats else None
    won = _full((n + 2,), FILL, torch.uint8)
    d_pairs = _pairs_up(pairs)
    d_frame = _up(np.asarray(frames, dtype=np.uint8)) if frames is not None else None
    pkg.align_pairs_translated_device(cfg, Q, R, n, d_pairs.data_ptr(), _ptr(d_frame), mode, mq, mr, rec.data_ptr(), _ptr(st), won.data_ptr(),
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


def _same_fold(got, want):
    rec, st, won = got[:3]
    wrec, wst, wwon = want
    assert won.tolist() == wwon.tolist()
    assert rec.tobytes() == wrec.tobytes()
    if wst is not None:
        assert st.tobytes() == wst.tobytes()


def _oracle(orc, cfg, om, strings):
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    sg = cfg.sg_flags if cfg.mode == 1 else orc.SG_ALL
    return orc.align_batch(cfg.mode, qb, qo, rb, ro, cfg.open, cfg.extend, om, sg_flags=sg, bits=cfg.width)


# ------------------------------------------------------------------------------------------------------------ 1. the gather, byte for byte
def _gather(pkg, Q, R, pairs, frames, mq, mr, qcap, rcap, qsize, rsize):
    """pmx_gather_pairs_translated_device into buffers of qsize / rsize bytes with 16 canary bytes on either side"""
    import torch
    n = len(pairs)
    qout = _full((qsize + 32,), FILL, torch.uint8); rout = _full((rsize + 32,), FILL, torch.uint8)
    qoff = _full((n + 3,), SENTINEL, torch.int64); roff = _full((n + 3,), SENTINEL, torch.int64)
    ok = _full((n + 2,), FILL, torch.uint8)
    d_pairs = _pairs_up(pairs)
    d_frame = _up(np.asarray(frames, dtype=np.uint8))
    pkg.gather_pairs_translated_device(Q, R, n, d_pairs.data_ptr(), d_frame.data_ptr(), mq, mr, qout.data_ptr() + 16, qcap, qoff.data_ptr(),
                                       rout.data_ptr() + 16, rcap, roff.data_ptr(), ok.data_ptr(), _stream())
    _sync()
    return [t.cpu().numpy() for t in (qout, qoff, rout, roff, ok)]


def test_gather_byte_for_byte(pkg):
    rng = np.random.default_rng(13200)
    letters = np.frombuffer(b"ACGTACGTACGTACGTacgtUuN-", dtype=np.uint8)
    qseqs = [letters[rng.integers(0, len(letters), size=l)].tobytes() for l in range(1, 46)]      # 1 .. 45 nt: every W mod 3, W < 3, W = 3
    qseqs[20] = b"TAAccTAGttTGAggTTActa"                                                           # stops on both strands
    qseqs[44] = qseqs[44][:45]
    rseqs = random_seqs(rng, 9, 1, 9, AA)
    mq, mr = 14, 9                                                                                 # 45 nt in frame 0 / 3: 15 letters, too long
    rows, frames = [], []
    for i in range(45):                                                                            # the first and the last sequence of the set included
        for f in range(6):
            rows.append((i, (i + f) % 9)); frames.append(f)
    for i in (0, 3, 4, 5, 9, 17, 29, 43, 44):                                                      # windows at every start 1 .. 3, both ways of giving a length
        for b in (1, 2, 3):
            for f in range(6):
                if b < len(qseqs[i]):
                    rows.append((i, f, b, -1 if f % 2 else len(qseqs[i]) - b, 0, -1)); frames.append(f)
    at = len(rows) // 2
    for row, f in (((45, 0), 0), ((3, 9), 2), ((5, 1, 0, 50, 0, -1), 1), ((7, 1), 6), ((8, 2), 255)):       # bad descriptors and frame bytes between good pairs
        rows.insert(at, row); frames.insert(at, f); at += 7
    rows.append((30, 4)); frames.append(1)                                                         # a last window of several letters, for the capacity cut
    pairs = pairs_ref.pairs_array(rows)
    want = ref.resolve(qseqs, rseqs, pairs, frames, mq, mr)
    n = len(pairs)
    lens = [len(w[0]) for w in want if w is not None]
    assert set(range(1, 15)) <= set(lens) and sum(w is None for w in want) > 40                    # translated lengths 1 .. 14; frames that do not exist
    assert any(w is not None and b"*" in w[0] for w, f in zip(want, frames) if f < 3) and any(w is not None and b"*" in w[0] for w, f in zip(want, frames) if f >= 3)
    assert any(w is not None and b"X" in w[0] for w in want)
    qwant = b"".join(w[0] if w else b"\0" for w in want); rwant = b"".join(w[1] if w else b"\0" for w in want)
    qoffw = np.concatenate([[0], np.cumsum([len(w[0]) if w else 1 for w in want])]); roffw = np.concatenate([[0], np.cumsum([len(w[1]) if w else 1 for w in want])])
    heads = {int(o) % 4 for o, w in zip(qoffw, want) if w}; tails = {int(o) % 4 for o, w in zip(qoffw[1:], want) if w}
    assert heads == tails == {0, 1, 2, 3}
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
        assert qout[16:16 + len(qwant)].tobytes() == qwant and rout[16:16 + len(rwant)].tobytes() == rwant
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


# ------------------------------------------------------------------------------------------------ the sets of cases 2 to 7
NQ, NR = 64, 48
MQ, MR = 40, 60
BACK = {}
for _i, _a in enumerate(ref.CODE_STD):
    BACK.setdefault(_a, []).append("".join(ref.BASES[(_i >> s) & 3] for s in (4, 2, 0)))


def back_translate(rng, protein):
    """a nucleotide string whose frame 0 reads `protein`, codons picked at random"""
    return "".join(BACK[a][int(rng.integers(0, len(BACK[a])))] for a in protein).encode()


def planted_sets():
    """48 proteins of 10 - 60 aa; 64 DNA queries of 30 - 120 nt: query i holds a mutated piece of protein i % 48, back-translated,
    between random flanks so that the piece reads in frame i % 6 (reverse frames: the whole query reverse-complemented)."""
    rng = np.random.default_rng(13300)
    prots = random_seqs(rng, NR, 10, 60, AA)
    queries = []
    for i in range(NQ):
        f = i % 6
        src = prots[i % NR]
        a = int(rng.integers(0, max(1, len(src) - 9)))
        piece = mutate(rng, src[a:a + int(rng.integers(9, 31))], sub=0.08, indel=0.0, alphabet=AA)
        core = back_translate(rng, piece)
        left = random_seqs(rng, 1, 14, 14)[0][:3 * int(rng.integers(2, 5)) + f % 3]               # the piece starts at an offset = f % 3 (mod 3)
        s = left + core + random_seqs(rng, 1, 1, 14)[0]
        queries.append(revcomp(s) if f >= 3 else s)
    assert all(30 <= len(s) <= 120 for s in queries) and all(10 <= len(s) <= 60 for s in prots)
    return queries, prots


def windowed_pairs(queries, prots):
    """240 pairs with windows on both sides, every window at least 6 nt: all six frames exist"""
    rng = np.random.default_rng(13400)
    rows = []
    for k in range(240):
        i, j = int(rng.integers(0, NQ)), int(rng.integers(0, NR))
        if k % 3 == 0:
            j = i % NR
        qb = int(rng.integers(0, 8)); ql = int(rng.integers(6, len(queries[i]) - qb + 1))
        rb = int(rng.integers(0, 4)); rl = int(rng.integers(3, len(prots[j]) - rb + 1))
        rows.append((i, j, qb, ql if k % 2 else (-1 if k % 4 else len(queries[i]) - qb), rb, rl))
    return pairs_ref.pairs_array(rows)


class Planted:
    pass


@pytest.fixture(scope="module")
def planted(pkg, orc):
    """the sets, the rectangle, the windowed list and, per mode and frame, the yardstick: pmx_align_pairs_device over the query set
    translated on the host in that frame, with statistics -- computed once, shared, left unchanged"""
    p = Planted()
    p.pm, p.om = _b62(pkg, orc)
    p.queries, p.prots = planted_sets()
    p.Q, p.R = pkg.SeqSet.new(p.queries), pkg.SeqSet.new(p.prots)
    p.rect = set_search_ref.rect_pairs_descriptors(NR, 0, NQ * NR)
    p.win = windowed_pairs(p.queries, p.prots)
    p.Qf = [pkg.SeqSet.new([ref.translate(s, f) for s in p.queries]) for f in range(6)]
    # the windowed list against sets of translated windows: pair k's query is sequence k of the set, whole
    wq = [p.queries[int(d["q"])][int(d["q_beg"]):(int(d["q_beg"]) + int(d["q_len"])) if d["q_len"] >= 0 else None] for d in p.win]
    p.win_strings = wq
    p.Wf = [pkg.SeqSet.new([ref.translate(s, f) for s in wq]) for f in range(6)]
    p.win_t = p.win.copy()
    p.win_t["q"] = np.arange(len(p.win)); p.win_t["q_beg"] = 0; p.win_t["q_len"] = -1
    p.single = {}
    for mode in ("sw", "sg"):
        cfg = _cfg(pkg, p.pm, mode, pkg.WANT_STATS)
        for f in range(6):
            p.single[mode, "rect", f] = _plain(pkg, cfg, p.Qf[f], p.R, p.rect, MQ, MR)
            p.single[mode, "win", f] = _plain(pkg, cfg, p.Wf[f], p.R, p.win_t, MQ, MR)
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
            for chunk in ((0, 500) if which == "rect" else (0, 64)):
                rec, st, won, kernel = _translated(pkg, cfg_s, p.Q, p.R, pairs, f, MQ, MR, chunk)
                assert rec.tobytes() == wrec.tobytes() and st.tobytes() == wst.tobytes() and (won == f).all() and kernel
        rec, _, won, _ = _translated(pkg, cfg, p.Q, p.R, p.win, f, MQ, MR, 100)              # without statistics
        assert rec.tobytes() == p.single[mode, "win", f][0].tobytes()
        rec, _, won, _ = _translated(pkg, cfg, p.Q, p.R, p.win, 0, MQ, MR, 100, frames=[f] * len(p.win))      # the frame as a byte per pair
        assert rec.tobytes() == p.single[mode, "win", f][0].tobytes() and (won == f).all()
        # a sample against the oracle on the translated strings
        sample = np.arange(f, NQ * NR, 53)
        strings = [(ref.translate(p.queries[int(d["q"])], f), p.prots[int(d["r"])]) for d in p.rect[sample]]
        want = _oracle(orc, cfg, p.om, strings)
        assert (p.single[mode, "rect", f][0][sample][:, :3] == want[:, :3]).all()
        wsample = np.arange(f, len(p.win), 7)
        strings = [(ref.translate(p.win_strings[k], f), pairs_ref.resolve_side(p.prots, p.win[k]["r"], p.win[k]["r_beg"], p.win[k]["r_len"])) for k in wsample]
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
        home = np.array([i * NR + i % NR for i in range(NQ)])                                     # query i against the protein it was built from
        assert (won[home] == np.arange(NQ) % 6).sum() >= NQ - 2                                   # ALL returns the planted frame ...
        for i in range(NQ):
            if won[home[i]] == i % 6:
                assert rec[home[i]].tolist() == p.single[mode, "rect", i % 6][0][home[i]].tolist()      # ... and that frame's record
        stops = [sum(b"*" in ref.translate(p.queries[i], f) for f in range(6) if f != i % 6) for i in range(NQ)]
        assert sum(s >= 1 for s in stops) >= NQ * 3 // 4                                          # stops fall in the other frames


def test_fold_ties_missing_frames_and_bad_pairs(pkg):
    rng = np.random.default_rng(13500)
    pm = pkg.Matrix.from_name("blosum62")
    prot = random_seqs(rng, 1, 30, 30, AA)[0]
    half = back_translate(rng, prot[5:17])                                                        # 36 nt
    pal = half + revcomp(half)                                                                    # equals its reverse complement: frames f and f + 3 read the same letters
    assert pal == revcomp(pal) and all(ref.translate(pal, f) == ref.translate(pal, f + 3) for f in range(3))
    queries = [pal, b"ATGG", b"AT", back_translate(rng, prot[:20]), b"G" + back_translate(rng, prot[3:25]), pal[1:], b"ACG"]
    prots = [prot] + random_seqs(rng, 3, 10, 40, AA)
    Q, R = pkg.SeqSet.new(queries), pkg.SeqSet.new(prots)
    rows = [(i, j) for i in range(len(queries)) for j in range(len(prots))]
    rows.insert(9, (len(queries), 0)); rows.insert(14, (0, 1, 0, -1, 50, 5))                      # bad descriptors between good pairs
    pairs = pairs_ref.pairs_array(rows)
    n = len(pairs)
    for mode in ("sw", "sg"):
        cfg = _cfg(pkg, pm, mode, pkg.WANT_STATS)
        single = [_translated(pkg, cfg, Q, R, pairs, f, 30, 40) for f in range(6)]
        w = [len(queries[int(d["q"])]) if 0 <= d["q"] < len(queries) and d["r_beg"] == 0 else 0 for d in pairs]
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
                got = _translated(pkg, cfg, Q, R, pairs, fm, 30, 40, chunk)
                _same_fold(got, want)
        rec, st, won, _ = _translated(pkg, cfg, Q, R, pairs, ALL, 30, 40, 4)
        k = rows.index((0, 0))
        assert single[0][0][k].tolist() == single[3][0][k].tolist() and single[0][0][k][0] > 30 and won[k] == 0      # the tie: the lowest frame
        assert _translated(pkg, cfg, Q, R, pairs, REV3, 30, 40)[2][k] == 3
        k = rows.index((1, 0))                                                                    # W = 4: frames 0, 1, 3, 4 exist
        assert exists[:, k].tolist() == [True, True, False, True, True, False] and rec[k][3] == 0 and won[k] in (0, 1, 3, 4)
        k = rows.index((6, 0))                                                                    # W = 3: frames 0 and 3
        assert exists[:, k].tolist() == [True, False, False, True, False, False] and rec[k][3] == 0
        assert _translated(pkg, cfg, Q, R, pairs[k:k + 1], 1, 30, 40)[0][0].tolist() == BAD
        for k in (rows.index((2, 0)), 9, 14):                                                     # W = 2 and the bad descriptors
            assert rec[k].tolist() == BAD and st[k].tolist() == [0, 0, 0] and won[k] == 0
        # a frame longer than max_qlen makes the pair bad, its neighbours are unaffected
        short = _translated(pkg, cfg, Q, R, pairs, ALL, 23, 40)
        long_ = np.array([x // 3 > 23 for x in w])
        assert long_.any() and all(short[0][k].tolist() == BAD for k in np.nonzero(long_)[0])
        assert short[0][~long_].tobytes() == rec[~long_].tobytes() and short[2][~long_].tolist() == won[~long_].tolist()


# ------------------------------------------------------------------------------------------------- 4. search and top-K on folded records
class Got:
    """outputs of one search call, whole buffers, on the host"""


def _search(pkg, cfg, Q, R, shape, first, n, pairs, mq, mr, min_score, capacity, mode, chunk=0, plain=False):
    """pmx_search_pairs_translated_device, or (plain) pmx_search_pairs_device"""
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
        pkg.search_pairs_translated_device(cfg, Q, R, shape, first, n, _ptr(d_pairs), mq, mr, min_score, hp.data_ptr(), hi.data_ptr(), hr.data_ptr(),
                                           _ptr(hs), capacity, cnt.data_ptr(), mode, _ptr(hb), _stream(), chunk)
    g = Got()
    g.kernel = pkg.lib.pmx_last_kernel().decode()
    _sync()
    host = lambda t: t.cpu().numpy() if t is not None else None
    g.pairs, g.index, g.recs, g.stats, g.frame, g.counts = host(hp).view(pairs_ref.PAIR_DTYPE), host(hi), host(hr), host(hs), host(hb), host(cnt)
    g.d_pairs, g.d_frame = hp, hb
    g.all = [a for a in (g.pairs, g.index, g.recs, g.stats, g.counts) if a is not None]
    return g


def _same_search(g, want, capacity):
    w = min(want["passing"], capacity)
    assert g.counts.tolist() == [want["passing"], w]
    assert g.recs[:w].tobytes() == want["records"][:w].tobytes() and (g.recs[w:] == SENTINEL).all()
    assert g.frame[:w].tolist() == want["frame"][:w].tolist() and (g.frame[w:] == FILL).all()
    assert g.index[:w].tolist() == want["index"][:w].tolist() and (g.index[w:] == SENTINEL).all()
    assert g.pairs[:w].tobytes() == want["pairs"][:w].tobytes() and (g.pairs[w:].view(np.uint8) == FILL).all()
    if g.stats is not None:
        assert g.stats[:w].tobytes() == want["stats"][:w].tobytes() and (g.stats[w:] == SENTINEL).all()


def _identical(a, b):
    assert len(a.all) == len(b.all)
    for x, y in zip(a.all, b.all):
        assert x.tobytes() == y.tobytes()


def _level(scores, share=20):
    return int(np.sort(scores)[-max(1, len(scores) // share)])


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
            old = _search(pkg, plain, p.Qf[f], p.R, RECT, first, n, None, MQ, MR, ms, n, f, chunk, plain=True)
            _identical(t, old)
            h = int(t.counts[1])
            assert h > 50 and (t.frame[:h] == f).all()


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
        pkg.search_topk_translated_device(cfg, Q, R, q_first, nq, mq, mr, min_score, k, False, hp.data_ptr(), hi.data_ptr(), hr.data_ptr(),
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


def _same_topk(g, want, capacity, nq):
    kept = int(want["row_off"][-1])
    w = min(kept, capacity)
    assert g.off[:nq + 1].tolist() == want["row_off"].tolist() and (g.off[nq + 1:] == SENTINEL).all()
    assert g.counts[:3].tolist() == [kept, w, int(want["row_passing"].sum())] and (g.counts[3:] == SENTINEL).all()
    assert g.passing[:nq].tolist() == want["row_passing"].tolist() and (g.passing[nq:] == SENTINEL).all()
    assert g.recs[:w].tobytes() == want["records"][:w].tobytes() and (g.recs[w:] == SENTINEL).all()
    assert g.index[:w].tolist() == want["index"][:w].tolist() and (g.index[w:] == SENTINEL).all()
    assert g.pairs[:w].tobytes() == want["pairs"][:w].tobytes() and (g.pairs[w:].view(np.uint8) == FILL).all()
    assert g.frame[:w].tolist() == want["frame"][:w].tolist() and (g.frame[w:] == FILL).all()
    if g.stats is not None:
        assert g.stats[:w].tobytes() == want["stats"][:w].tobytes() and (g.stats[w:] == SENTINEL).all()


def test_topk_on_folded_records(pkg, planted):
    p = planted
    cfg = _cfg(pkg, p.pm, "sw", pkg.WANT_STATS)
    rec, st, won = _folded(p, "sw", "rect")
    for k in (1, 3, 60):                                                                          # K > |R|: every reference once
        cap = NQ * min(k, NR)
        want = ref.topk(rec, won, NR, 0, NQ, k, stats=st)
        runs = [_topk(pkg, cfg, p.Q, p.R, 0, NQ, MQ, MR, INT32_MIN, k, cap, ALL, chunk) for chunk in (64, 192, 0)]
        for g in runs:
            _same_topk(g, want, cap, NQ)
            _identical(g, runs[0])
        g = runs[0]
        for i in range(NQ):                                                                       # a reference appears at most once in a row
            row = g.pairs[int(g.off[i]):int(g.off[i + 1])]["r"].tolist()
            assert len(row) == len(set(row)) == min(k, NR)
        assert g.passing[:NQ].tolist() == [NR] * NQ and (g.recs[:cap, 3] == 0).all()             # row_passing counts pairs, not (pair, frame)
        if k == 1:
            home = sum(int(g.pairs[i]["r"]) == i % NR and int(g.frame[i]) == i % 6 for i in range(NQ))
            assert home >= NQ - 4                                                                 # the best reference is the one the query codes for, in its frame
    ms = _level(rec[:, 0])                                                                        # a threshold, a sub-range of rows, a small capacity
    sub = slice(7 * NR, 30 * NR)
    want = ref.topk(rec[sub], won[sub], NR, 7, 23, 3, min_score=ms, stats=st[sub], capacity=11)
    assert 0 < want["row_passing"].sum() < 23 * NR
    _same_topk(_topk(pkg, cfg, p.Q, p.R, 7, 23, MQ, MR, ms, 3, 11, ALL, 100), want, 11, 23)
    plain = _cfg(pkg, p.pm, "sw")
    for f, k, chunk in ((2, 3, 0), (5, 60, 192)):                                                 # single frame: the untranslated entry, byte for byte
        cap = NQ * min(k, NR)
        t = _topk(pkg, plain, p.Q, p.R, 0, NQ, MQ, MR, INT32_MIN, k, cap, f, chunk)
        old = _topk(pkg, plain, p.Qf[f], p.R, 0, NQ, MQ, MR, INT32_MIN, k, cap, f, chunk, plain=True)
        _identical(t, old)
        assert (t.frame[:cap] == f).all()


# ------------------------------------------------------------------------------------------------------------------- 5. the CIGAR route
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
    qout = _full((h * MQ + 16,), FILL, torch.uint8); rout = _full((h * MR + 16,), FILL, torch.uint8)
    qoff = _full((h + 1,), SENTINEL, torch.int64); roff = _full((h + 1,), SENTINEL, torch.int64)
    pkg.gather_pairs_translated_device(p.Q, p.R, h, g.d_pairs.data_ptr(), g.d_frame.data_ptr(), MQ, MR, qout.data_ptr(), h * MQ, qoff.data_ptr(),
                                       rout.data_ptr(), h * MR, roff.data_ptr(), None, _stream())
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
    strings = ref.resolve(p.queries, p.prots, g.pairs[:h], g.frame[:h], MQ, MR)
    assert all(s is not None for s in strings)
    qb, qo = orc.pack([s[0] for s in strings]); rb, ro = orc.pack([s[1] for s in strings])
    want_text, want = orc.cigar_sample(orc.SW, np.arange(h), qb, qo, rb, ro, 11, 1, p.om)
    assert (crec[:, :3] == want[:, :3]).all() and 0 < toff[h] <= cap
    texts = [text[toff[k]:toff[k + 1]].tobytes().decode() for k in range(h)]
    assert texts == list(want_text)


# --------------------------------------------------------------------------------------------------------- 6. nothing else moved
def test_untranslated_entries_beside_a_translated_call(pkg, orc, planted):
    """a forward batch before and after translated calls of the same thread (they share its scratch): the same records, the same kernel"""
    p = planted
    rng = np.random.default_rng(13600)
    dm, dom = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    seqs = random_seqs(rng, 40, 20, 90)
    S = pkg.SeqSet.new(seqs)
    pairs = pairs_ref.all_pairs_descriptors(40, 0, pairs_ref.all_pairs_count(40))
    dcfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, dm.inner)
    n = len(pairs)

    def others():
        """a forward batch, pmx_align_pairs_both_device and a PMX_STRAND_BOTH search: every output, and the kernel each one names"""
        import torch
        out, names = [_plain(pkg, dcfg, S, S, pairs, 90, 90)[0]], [pkg.lib.pmx_last_kernel().decode()]
        rec = _full((n, 4), SENTINEL, torch.int32); won = _full((n,), FILL, torch.uint8)
        d_pairs = _pairs_up(pairs)
        pkg.align_pairs_both_device(dcfg, S, S, n, d_pairs.data_ptr(), 90, 90, rec.data_ptr(), None, won.data_ptr(), _stream(), 300)
        names.append(pkg.lib.pmx_last_kernel().decode())
        hp = _full((n * 32,), FILL, torch.uint8); hi = _full((n,), SENTINEL, torch.int64); hr = _full((n, 4), SENTINEL, torch.int32)
        hb = _full((n,), FILL, torch.uint8); cnt = _full((2,), SENTINEL, torch.int64)
        pkg.search_pairs_stranded_device(dcfg, S, None, TRI, 0, n, None, 90, 90, int(np.sort(out[0][:, 0])[-(n // 4)]), hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), None, n,
                                         cnt.data_ptr(), pkg.STRAND_BOTH, hb.data_ptr(), _stream(), 300)
        names.append(pkg.lib.pmx_last_kernel().decode())
        _sync()
        return out + [t.cpu().numpy() for t in (rec, won, hp, hi, hr, hb, cnt)], names

    before, names = others()
    _translated(pkg, _cfg(pkg, p.pm, "sw", pkg.WANT_STATS), p.Q, p.R, p.rect, ALL, MQ, MR, 500)
    _search(pkg, _cfg(pkg, p.pm, "sw"), p.Q, p.R, RECT, 0, NQ * NR, None, MQ, MR, 40, 100, ALL, 192)
    _topk(pkg, _cfg(pkg, p.pm, "sw"), p.Q, p.R, 0, NQ, MQ, MR, INT32_MIN, 3, 3 * NQ, ALL, 192)
    after, names_after = others()
    assert names_after == names and all(names)
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    rec, won, hits, hit_recs, hit_strand, counts = before[1], before[2], before[4], before[5], before[6], before[7]
    h = int(counts[1])
    assert 0 < h < n and 0 < hit_strand[:h].sum() < h and (hit_recs[:h, 3] == 0).all()              # both strands hit; no private flag bit gets out
    assert hit_recs[:h].tobytes() == rec[hits[:h]].tobytes() and hit_strand[:h].tolist() == won[hits[:h]].tolist()
    strings = pairs_ref.resolve(seqs, seqs, pairs)
    assert (before[0][:, :3] == _oracle(orc, dcfg, dom, strings)[:, :3]).all()
    fwd_better = rec[:, 0] >= before[0][:, 0]
    assert fwd_better.all() and (rec[won == 0].tobytes() == before[0][won == 0].tobytes())          # BOTH never scores below forward; a forward winner is the forward record


# ------------------------------------------------------------------------------------------------- 7. host entries, Python mirror
def test_host_entries_and_python_mirror(pkg, planted):
    p = planted
    al = pkg.Aligner.new().local().matrix(p.pm).gap_open(11).gap_extend(1).build()
    als = pkg.Aligner.new().local().matrix(p.pm).gap_open(11).gap_extend(1).use_stats().build()
    qb, qo = pkg.pack(p.queries); rb, ro = pkg.pack(p.prots)
    keep = (_up(qb), _up(qo), _up(rb), _up(ro))
    WQ = pkg.SeqSet.wrap_device(keep[0].data_ptr(), keep[1].data_ptr(), NQ, len(qb), keep=keep[:2])
    WR = pkg.SeqSet.wrap_device(keep[2].data_ptr(), keep[3].data_ptr(), NR, len(rb), keep=keep[2:])
    sets = ((p.Q, p.R), (WQ, WR))
    want = _folded(p, "sw", "win")
    for Q, R in sets:
        for chunk in (0, 100):
            rec, won = al.align_pairs(Q, R, p.win, chunk_pairs=chunk, frame="all")
            assert rec.view(np.int32).tobytes() == want[0].tobytes() and won.tolist() == want[2].tolist()
        rec, st, won = als.align_pairs(Q, R, p.win, frame=pkg.FRAMES_ALL)
        assert rec.view(np.int32).tobytes() == want[0].tobytes() and st.view(np.int32).tobytes() == want[1].tobytes() and won.tolist() == want[2].tolist()
        rec, won = al.align_pairs(Q, R, p.win, frame=4)
        assert rec.view(np.int32).tobytes() == p.single["sw", "win", 4][0].tobytes() and (won == 4).all()
        rec, won2 = al.align_pairs(Q, R, p.win, frame=want[2])                                    # the winners' frames as a byte per pair
        assert rec.view(np.int32).tobytes() == want[0].tobytes() and won2.tolist() == want[2].tolist()
    # search_pairs: the list, then the rectangle
    ms = _level(want[0][:, 0], 8)
    w = ref.search(want[0], want[2], ms, 0, p.win, want[1])
    for kw in ({}, {"slice_pairs": 100}, {"slice_pairs": 64, "chunk_pairs": 7}, {"max_hits": 5}):
        for Q, R in sets:
            h = al.search_pairs(Q, R, min_score=ms, pairs=p.win, frame="all", stats=True, **kw)
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
            h = al.search_pairs(Q, R, min_score=rms, frame=frame, slice_pairs=1000)
            assert h.n_hits == w["passing"] and h.records.view(np.int32).tobytes() == w["records"].tobytes()
            assert h.frame.tolist() == w["frame"].tolist() and h.index.tolist() == w["index"].tolist()
        for kw in ({}, {"slice_rows": 5}, {"slice_rows": 1, "chunk_pairs": 30}):
            for Q, R in sets:
                t = al.search_topk(Q, R, k=4, frame=frame, **kw)
                w4 = ref.topk(rec, won, NR, 0, NQ, 4)
                assert t.row_off.tolist() == w4["row_off"].tolist() and t.row_passing.tolist() == w4["row_passing"].tolist()
                assert t.records.view(np.int32).tobytes() == w4["records"].tobytes() and t.frame.tolist() == w4["frame"].tolist()
                assert t.index.tolist() == w4["index"].tolist() and t.pairs.tobytes() == w4["pairs"].tobytes()
    # a bad pair is named: a descriptor the host sees, and a window without a frame, which only the device sees
    bad = p.win[:20].copy()
    bad[11] = (NQ, 0, 0, -1, 0, -1)
    with pytest.raises(pkg.BatchError, match=r"pair 11: query: index outside"):
        al.align_pairs(p.Q, p.R, bad, frame="all")
    with pytest.raises(pkg.BatchError, match=r"pair 11: bad descriptor"):
        al.align_pairs(WQ, WR, bad, frame="all")
    bad[11] = (3, 0, 4, 2, 0, -1)                                                                # W = 2: no frame
    for Q, R in sets:
        with pytest.raises(pkg.BatchError, match=r"pair 11: bad descriptor"):
            al.align_pairs(Q, R, bad, frame="all")
        with pytest.raises(pkg.BatchError, match=r"pair 11: bad descriptor .* no frame"):
            al.search_pairs(Q, R, pairs=bad, frame="all")
    bad[11] = (3, 0, 4, 4, 0, -1)                                                                # W = 4: frame 2 does not exist, frame 1 does
    with pytest.raises(pkg.BatchError, match=r"pair 11: bad descriptor"):
        al.align_pairs(p.Q, p.R, bad, frame=2)
    rec, won = al.align_pairs(p.Q, p.R, bad, frame=1)
    assert rec[11]["flags"] == 0 and won[11] == 1
