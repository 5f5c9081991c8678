"""The windowed reference-side frameshift traceback entries (`-m gpu`): pmx_align_pairs_frameshift_ref_cigar_long[_device] -- the score
road, pmx_fsref_window_kernel, the trace road over the narrowed descriptors, pmx_fsref_rebase_kernel -- against
pmx_align_pairs_frameshift_ref_cigar[_device] on the same arguments, byte for byte in every output array, and, where that entry
refuses the trace of the whole matrix, against the CPU model over the full window (tests/frameshift_trace_ref_side.py).  Every output
buffer starts as a sentinel and is checked beyond n."""
import numpy as np
import pytest

import frameshift_ref_side as fr
import frameshift_trace_ref_side as ft
import pairs_ref
from pairs_ex_ref import revcomp
from test_gpu_translate import _up, _full, _stream, _sync, _ptr, _pairs_up, SENTINEL, FILL
from test_gpu_frameshift_ref import _b62, _dna, _gene, _noisy_gene
from test_frameshift_window_model import window_of
from util import random_seqs, AA, golden

pytestmark = pytest.mark.gpu

FWD, REV, BOTH = 0, 1, 2
S = 160                         # a strip of the sweep: queries of 161 and 170 letters need two
TRACE = "pmx_swfsc_kernel<16,10,trace>"
SLACK = 32
OPEN, EXT, FS = 11, 1, 15


def _cfg(pkg, pm, stats=True):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, OPEN, EXT, 0, pkg.WANT_CIGAR | (pkg.WANT_STATS if stats else 0), pm.inner)


class Got:
    pass


def _run(pkg, long_, cfg, Q, Rs, pairs, mode, mq, mr, capacity, chunk=0, strands=None, stats=True, beg=True):
    """the _long device entry (long_) or the entry it must equal -> every output as it lies in its buffer, sentinels beyond n checked"""
    import torch
    entry = pkg.align_pairs_frameshift_ref_cigar_long_device if long_ else pkg.align_pairs_frameshift_ref_cigar_device
    n = len(pairs)
    rec = _full((n + 2, 4), SENTINEL, torch.int32); won = _full((n + 2,), FILL, torch.uint8)
    st = _full((n + 2, 3), SENTINEL, torch.int32) if stats else None
    bg = _full((n + 2, 2), SENTINEL, torch.int32) if beg else None
    text = _full((capacity + SLACK,), FILL, torch.uint8); off = _full((n + 3,), SENTINEL, torch.int64)
    d_pairs = _pairs_up(pairs)
    d_strand = _up(np.asarray(strands, dtype=np.uint8)) if strands is not None else None
    entry(cfg, Q, Rs, n, d_pairs.data_ptr(), _ptr(d_strand), mode, FS, mq, mr, rec.data_ptr(), won.data_ptr(),
          _ptr(st), _ptr(bg), text.data_ptr(), capacity, off.data_ptr(), _stream(), chunk)
    g = Got()
    g.kernel = pkg.lib.pmx_last_kernel().decode()
    g.parts = pkg.lib.pmx_frameshift_ref_cigar_long_parts() if long_ else None
    _sync()
    g.rec, g.won, g.text, g.off = rec.cpu().numpy(), won.cpu().numpy(), text.cpu().numpy(), off.cpu().numpy()
    g.stats = st.cpu().numpy() if stats else None
    g.beg = bg.cpu().numpy() if beg else None
    assert (g.rec[n:] == SENTINEL).all() and (g.won[n:] == FILL).all() and (g.off[n + 1:] == SENTINEL).all()
    assert not stats or (g.stats[n:] == SENTINEL).all()
    assert not beg or (g.beg[n:] == SENTINEL).all()
    assert (g.text[capacity:] == FILL).all()
    return g


def _bytes_equal(a, b):
    for name in ("rec", "won", "off", "text", "stats", "beg"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (name, np.nonzero((x != y).reshape(len(x), -1).any(axis=1))[0][:5])


def _same_as_model(g, want):
    n = len(want.texts)
    assert g.won[:n].tolist() == want.strand.tolist()
    assert g.rec[:n].tobytes() == want.records.tobytes()
    assert g.off[:n + 1].tolist() == want.off.tolist()
    assert g.beg[:n].tobytes() == want.beg.tobytes() and g.stats[:n].tobytes() == want.stats.tobytes()
    total = int(want.off[n])
    assert g.text[:total].tobytes() == want.text_bytes() and (g.text[total:] == FILL).all()


class Batch:
    pass


# ------------------------------------------------------------------------------------------------------------------- the batch
ZERO_Q, ZERO_R = b"WWWW", b"TGA" * 20      # W against *, D, M forward and S, H, I reverse: nothing scores, on either strand


def _batch(pkg, orc):
    """queries of 1, 10, 160, 161 and 170 letters (and three between) against reference windows of 60 - 3 000 nt that hold a piece of
    the query with single-base events -- at the window's first column, ending at its last column, and in the middle of long flanks --,
    as whole sequences (r_len -1), as tails (r_beg > 0, r_len -1) and as inner windows (r_beg > 0, explicit r_len); every third gene on
    the reverse strand; one zero-score pair; one bad pair between good neighbours.  The old entry's outputs and the model's for
    PMX_STRAND_BOTH are computed once, shared and left unchanged."""
    p = Batch()
    p.pm, p.om = _b62(pkg, orc)
    rng = np.random.default_rng(21300)
    lens = (1, 10, S, S + 1, S + 10, 30, 45, 60)
    p.prots = [random_seqs(rng, 1, m, m, AA)[0] for m in lens] + [ZERO_Q]
    p.refs, rows = [], []
    kinds = {"first": 0, "last": 0, "middle": 0}

    def add(i, window, how):
        """the window as a whole sequence, as the tail of one, or inside one"""
        k = len(rows)
        w = window if k % 3 else revcomp(window)
        form = k % 4
        if form == 0:
            p.refs.append(w); rows.append((i, len(p.refs) - 1))
        elif form == 1:
            lead = int(rng.integers(1, 90))
            p.refs.append(_dna(rng, lead) + w); rows.append((i, len(p.refs) - 1, 0, -1, lead, -1))
        else:
            lead, trail = int(rng.integers(1, 90)), int(rng.integers(1, 90))
            p.refs.append(_dna(rng, lead) + w + _dna(rng, trail)); rows.append((i, len(p.refs) - 1, 0, -1, lead, len(w)))
        assert 60 <= len(w) <= 3000
        kinds[how] += 1

    for i, m in enumerate(lens):
        q = p.prots[i]
        for rep in range(4):
            piece = q[int(rng.integers(0, max(1, m // 4))):]
            shifts = [(int(x), int(rng.integers(0, 2))) for x in sorted(set(rng.integers(1, max(2, len(piece) - 2), rep).tolist()))] if len(piece) > 8 else []
            g = _gene(rng, piece, shifts)
            room = 3000 - len(g)
            add(i, g + _dna(rng, max(60 - len(g), int(rng.integers(0, room)))), "first")
            add(i, _dna(rng, max(60 - len(g), int(rng.integers(0, room)))) + g, "last")
            left = int(rng.integers(room // 3, 2 * room // 3))
            add(i, _dna(rng, left) + g + _dna(rng, int(rng.integers(room // 6, room - left))), "middle")
    assert all(v >= 30 for v in kinds.values())
    p.refs.append(ZERO_R)
    p.zero_at = len(rows); rows.append((len(lens), len(p.refs) - 1))
    p.bad_at = 40; rows.insert(p.bad_at, (2, len(p.refs) + 5))                  # a reference index outside the set
    p.zero_at += 1
    p.Q, p.R = pkg.SeqSet.new(p.prots), pkg.SeqSet.new(p.refs)
    p.pairs = pairs_ref.pairs_array(rows)
    p.n = len(rows)
    assert 64 <= p.n <= 200
    p.mq, p.mr = S + 10, 2998
    p.want = ft.results(p.prots, p.refs, p.pairs, BOTH, p.om, OPEN, EXT, FS, max_qlen=p.mq, max_rlen=p.mr)
    p.capacity = int(p.want.off[-1])
    return p


@pytest.fixture(scope="module")
def batch(pkg, orc):
    return _batch(pkg, orc)


def _narrowed_lengths(pkg, p, want):
    """per good pair of a model result: the narrowed query letters, the narrowed stream's letters and the column shift, from the hook"""
    out = []
    for k, d in enumerate(p.pairs):
        rec = want.records[k].tolist()
        if rec == ft.BAD:
            out.append((1, 1, 0))
            continue
        q = pairs_ref.resolve_side(p.prots, d["q"], d["q_beg"], d["q_len"])
        a, W = window_of(pkg, q, rec, p.om, OPEN, EXT, FS)
        out.append((rec[1] + 1, rec[2] + 1 - a - 2, a))
    return out


def test_batch_is_what_it_says(pkg, batch):
    """the edge cases, from the model's results and not from the construction"""
    p = batch
    w = p.want
    assert w.records[p.bad_at].tolist() == ft.BAD and w.records[p.bad_at - 1][0] > 0 and w.records[p.bad_at + 1][0] > 0
    assert w.records[p.zero_at].tolist() == [0, 0, 2, 0] and w.texts[p.zero_at] == "" and w.beg[p.zero_at].tolist() == [1, 3]
    assert set(w.strand.tolist()) == {0, 1}
    nar = _narrowed_lengths(pkg, p, w)
    wins = [len(pairs_ref.resolve_side(p.refs, d["r"], d["r_beg"], d["r_len"]) or b"") for d in p.pairs]
    at_first = sum(1 for k in range(p.n) if w.records[k][0] > 0 and w.beg[k][1] == 0)
    at_last = sum(1 for k in range(p.n) if w.records[k][0] > 0 and w.records[k][2] == wins[k] - 1)
    clipped = sum(1 for k in range(p.n) if w.records[k][0] > 0 and nar[k][2] == 0)
    shifted = sum(1 for k in range(p.n) if nar[k][2] > 0)
    two_strips = sum(1 for k in range(p.n) if w.records[k][1] >= S)
    assert at_first >= 10 and at_last >= 10 and clipped >= 10 and shifted >= 40 and two_strips >= 6, (at_first, at_last, clipped, shifted, two_strips)
    assert {int(d["q_len"]) for d in p.pairs} == {-1} and {len(q) for q in p.prots} >= {1, 10, S, S + 1, S + 10}
    assert sum(1 for d in p.pairs if d["r_beg"] > 0 and d["r_len"] > 0) >= 20 and sum(1 for d in p.pairs if d["r_len"] == -1) >= 20
    assert sum("/" in t for t in w.texts) >= 20 and sum("\\" in t for t in w.texts) >= 20


# ------------------------------------------------------------------------------------------------- 1. equality with the old entry
@pytest.mark.parametrize("mode", ["forward", "reverse", "both", "list"])
def test_equals_the_unwindowed_entry(pkg, batch, mode):
    p = batch
    rng = np.random.default_rng(21400)
    strands = None
    if mode == "list":
        strands = rng.integers(0, 2, p.n).astype(np.uint8)
        strands[7] = 2                                            # a strand byte above 1: one more bad pair
    m = {"forward": FWD, "reverse": REV, "both": BOTH, "list": FWD}[mode]
    for stats, beg in ((True, True), (False, False), (True, False)):
        cfg = _cfg(pkg, p.pm, stats)
        old = _run(pkg, False, cfg, p.Q, p.R, p.pairs, m, p.mq, p.mr, p.capacity, strands=strands, stats=stats, beg=beg)
        new = _run(pkg, True, cfg, p.Q, p.R, p.pairs, m, p.mq, p.mr, p.capacity, strands=strands, stats=stats, beg=beg)
        _bytes_equal(new, old)
        assert new.kernel == old.kernel == TRACE + "/strips"
        assert new.rec[p.bad_at].tolist() == ft.BAD and new.rec[p.zero_at].tolist() == [0, 0, 2, 0]
        if mode == "list":
            assert new.rec[7].tolist() == ft.BAD and new.won[7] == 0
        if mode == "both" and stats and beg:
            _same_as_model(new, p.want)
            p.base = new


# --------------------------------------------------------------------------------------------------- 2. independence from parts
def test_chunks_and_parts_change_no_byte(pkg, batch, monkeypatch):
    p = batch
    cfg = _cfg(pkg, p.pm)
    base = getattr(p, "base", None) or _run(pkg, True, cfg, p.Q, p.R, p.pairs, BOTH, p.mq, p.mr, p.capacity)
    assert base.parts == 1                                        # the default bound: one chunk, one part
    for chunk in (1, 7, p.n):
        g = _run(pkg, True, cfg, p.Q, p.R, p.pairs, BOTH, p.mq, p.mr, p.capacity, chunk=chunk)
        _bytes_equal(g, base)
        assert g.parts == -(-p.n // chunk)
    # the bound in bytes.  A part is whole workgroups of four slots, so the smallest part a bound can force within a chunk is one
    # workgroup: `tight` is four slots of the widest narrowed window, one byte less would refuse that pair
    nar = _narrowed_lengths(pkg, p, p.want)
    per = [pkg.lib.pmx_swfsc_trace_bytes_per_slot(nq, nr) for nq, nr, _ in nar]
    tight = 4 * max(per)
    loose = 3 * tight
    assert 4 * pkg.lib.pmx_swfsc_trace_bytes_per_slot(p.mq, p.mr) > tight      # the unwindowed entry would refuse the tight value
    for bound, chunk in ((loose, 0), (tight, 0), (tight, 1)):      # (tight, 1): chunks of one pair, single-pair parts
        monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(bound))
        g = _run(pkg, True, cfg, p.Q, p.R, p.pairs, BOTH, p.mq, p.mr, p.capacity, chunk=chunk)
        monkeypatch.undo()
        _bytes_equal(g, base)
        assert g.parts == p.n if chunk == 1 else 3 <= g.parts < p.n, (bound, g.parts)
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(tight - 1))
    with pytest.raises(pkg.BatchError, match="PMX_CIGAR_CHUNK_BYTES") as e:
        _run(pkg, True, cfg, p.Q, p.R, p.pairs, BOTH, p.mq, p.mr, p.capacity)
    monkeypatch.undo()
    assert str(tight) in str(e.value) and str(tight - 1) in str(e.value)       # both figures: the pair's four slots, the bound


# ----------------------------------------------------------------------------------------------------------------- 3. new ground
def test_where_the_unwindowed_entry_refuses(pkg, orc, monkeypatch):
    """queries of about 60 letters against references of about 6 000 nt, the bound one byte under four slots of the whole matrix: the
    old entry refuses, the new one runs; every text re-scores to its record, every output equals the model over the FULL window"""
    pm, om = _b62(pkg, orc)
    b62 = orc.Matrix.from_file(golden("blosum62.txt"))
    score = lambda a, b: int(b62.scores[b62.mapper[a], b62.mapper[b]])
    score.same = lambda a, b: b62.mapper[a] == b62.mapper[b]
    rng = np.random.default_rng(21500)
    prots = random_seqs(rng, 8, 52, 64, AA)
    refs, rows, planted = [], [], []
    for j in range(24):
        i = j % 8
        q = prots[i]
        at = [(len(q) // 3 + int(rng.integers(-3, 4)), 0)] + ([(2 * len(q) // 3 + int(rng.integers(-3, 4)), 0)] if j % 2 else [])      # one or two '/'
        g = _gene(rng, q, at)
        W = int(rng.integers(5600, 6001))
        left = int(rng.integers(0, W - len(g)))
        w = _dna(rng, left) + g + _dna(rng, W - len(g) - left)
        refs.append(revcomp(w) if j % 3 == 1 else w)
        rows.append((i, j)); planted.append(len(at))
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    pairs = pairs_ref.pairs_array(rows)
    mq, mr = max(len(q) for q in prots), max(len(r) for r in refs) - 2
    want = ft.results(prots, refs, pairs, BOTH, om, OPEN, EXT, FS)
    cfg = _cfg(pkg, pm)
    four = 4 * pkg.lib.pmx_swfsc_trace_bytes_per_slot(mq, mr)
    monkeypatch.setenv("PMX_CIGAR_CHUNK_BYTES", str(four - 1))
    with pytest.raises(pkg.BatchError, match="exceed the bound") as e:
        _run(pkg, False, cfg, Q, Rs, pairs, BOTH, mq, mr, int(want.off[-1]))
    assert "PMX_CIGAR_CHUNK_BYTES" in str(e.value) and str(four) in str(e.value)
    g = _run(pkg, True, cfg, Q, Rs, pairs, BOTH, mq, mr, int(want.off[-1]))
    monkeypatch.undo()
    _same_as_model(g, want)
    assert g.kernel == TRACE and set(want.strand.tolist()) == {0, 1}
    for k in range(len(rows)):
        text = g.text[int(g.off[k]):int(g.off[k + 1])].tobytes().decode()
        T = fr.stream(refs[k], int(g.won[k]))
        assert list(ft.rescore(text, g.beg[k].tolist(), prots[rows[k][0]], T, score, OPEN, EXT, FS)) == g.rec[k][:3].tolist()
        assert text.count("/") >= planted[k], (k, text)
        assert g.rec[k][0] > 200


# ---------------------------------------------------------------------------------------------------------- 4. the host entries
def test_host_entry_and_python_method(pkg, orc):
    """Aligner.align_pairs_frameshift_ref_cigar_long returns what the C entry writes, and what the unwindowed method returns; texts of
    more than 32 bytes per pair make the host entry run once more at the exact text size"""
    import ctypes as C
    pm, om = _b62(pkg, orc)
    rng = np.random.default_rng(21600)
    prots = random_seqs(rng, 8, 150, 170, AA)
    refs = [_dna(rng, int(rng.integers(100, 900))) + _noisy_gene(rng, q, 3 * len(q) - 20) + _dna(rng, 40) for q in prots]
    refs = [revcomp(r) if j % 2 else r for j, r in enumerate(refs)]
    Q, Rs = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    pairs = pairs_ref.pairs_array([(i, i) for i in range(8)])
    al = pkg.Aligner.new().local().matrix(pm).gap_open(OPEN).gap_extend(EXT).build()
    rec, cig, beg, won, st = al.align_pairs_frameshift_ref_cigar_long(Q, Rs, pairs, FS, ref_strand="both", stats=True, chunk_pairs=3)
    old = al.align_pairs_frameshift_ref_cigar(Q, Rs, pairs, FS, ref_strand="both", stats=True, chunk_pairs=3)
    assert rec.tobytes() == old[0].tobytes() and cig == old[1] and beg.tobytes() == old[2].tobytes()
    assert won.tolist() == old[3].tolist() and st.tobytes() == old[4].tobytes()
    assert sum(len(t) for t in cig) > 32 * len(pairs) + 256 and set(won.tolist()) == {0, 1}      # the estimate was too small: two passes
    # the C entry itself, on the same arguments
    n = len(pairs)
    cfg = _cfg(pkg, pm)
    out = np.zeros(n, dtype=pkg.RECORD_DTYPE); w2 = np.zeros(n, dtype=np.uint8); s2 = np.zeros(n, dtype=pkg.STATS_DTYPE)
    b2 = np.zeros((n, 2), dtype=np.int32); off = np.zeros(n + 1, dtype=np.int64); buf = C.c_void_p()
    opts = pkg.pmx_pairs_opts_t(3)
    rc = pkg.lib.pmx_align_pairs_frameshift_ref_cigar_long(C.byref(cfg), Q._handle(), Rs._handle(), n, pairs.ctypes.data, None, BOTH, FS, None,
                                                           out.ctypes.data, w2.ctypes.data, s2.ctypes.data, b2.ctypes.data, C.byref(buf),
                                                           off.ctypes.data, C.byref(opts))
    assert rc == 0
    text = C.string_at(buf, int(off[n]))
    pkg.lib.pmx_free(buf)
    assert out.tobytes() == rec.tobytes() and w2.tolist() == won.tolist() and s2.tobytes() == st.tobytes() and b2.tobytes() == beg.tobytes()
    assert [text[int(off[k]):int(off[k + 1])].decode() for k in range(n)] == cig
    # one strand byte per pair, as a search returns them
    rec3, cig3, beg3, won3 = al.align_pairs_frameshift_ref_cigar_long(Q, Rs, pairs, FS, ref_strand=won)
    assert rec3.tobytes() == rec.tobytes() and cig3 == cig and beg3.tobytes() == beg.tobytes() and won3.tolist() == won.tolist()
