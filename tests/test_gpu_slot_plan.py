"""Where one resolve kernel, one fold kernel and one gather-hook body serve every entry family (`-m gpu`): the places a merged kernel
could part from the kernel it replaced, each on a handful of pairs.  Every case is compared with the Python references of tests/
(pairs_ref, pairs_ex_ref, translate_ref[_side], frameshift_ref[_side], the CPU oracle for the scores), runs with chunk_pairs 1, 3 and n
and must not differ in a byte between the three; every output buffer starts as a sentinel."""
import ctypes as C

import numpy as np
import pytest

import frameshift_ref as fs
import frameshift_ref_side as fsr
import pairs_ex_ref
import pairs_ref
import translate_ref as tr
import translate_ref_side as trs
from util import golden

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
INT32_MIN = -(1 << 31)
LIST = 0
FWD, REV, BOTH = 0, 1, 2
BAD = list(pairs_ref.BAD_RECORD)
OPEN, EXT, SHIFT = 11, 1, 15                       # protein gaps and the frameshift penalty


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


def _pairs_up(pairs):
    return _up(np.ascontiguousarray(pairs).view(np.uint8))


def _oracle(orc, om, strings, open_, ext):
    """[n, 4] records of resolved (query, reference) strings by the CPU oracle, None -> the bad record"""
    out = np.tile(np.array(BAD, dtype=np.int32), (len(strings), 1))
    good = [k for k, s in enumerate(strings) if s is not None]
    if good:
        qb, qo = orc.pack([strings[k][0] for k in good]); rb, ro = orc.pack([strings[k][1] for k in good])
        want = orc.align_batch(orc.SW, qb, qo, rb, ro, open_, ext, om)
        out[good, :3] = want[:, :3]
        out[good, 3] = 0
    return out


def _three_chunks(n, run):
    """run(chunk) for chunk_pairs 1, 3 and n -> the first run's arrays, all three identical"""
    runs = [run(chunk) for chunk in (1, 3, n)]
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for a, b in zip(runs[0], other):
            assert a.tobytes() == b.tobytes()
    return runs[0]


def _align(call, n, byte_out=True):
    """one align entry: call(d_rec, d_byte or None) -> records [n, 4], bytes [n]; the entries behind the last stay untouched"""
    import torch
    rec = _full((n + 2, 4), SENTINEL, torch.int32)
    won = _full((n + 2,), FILL, torch.uint8) if byte_out else None
    call(rec.data_ptr(), won.data_ptr() if byte_out else None)
    _sync()
    rec = rec.cpu().numpy()
    assert (rec[n:] == SENTINEL).all()
    if not byte_out:
        return (rec[:n],)
    won = won.cpu().numpy()
    assert (won[n:] == FILL).all()
    return rec[:n], won[:n]


def _search(call, n):
    """one search entry at a threshold every pair passes: call(d_hit_index, d_hit_recs, d_hit_byte, capacity, d_counts) -> records, bytes"""
    import torch
    hi = _full((n + 2,), SENTINEL, torch.int64)
    hr = _full((n + 2, 4), SENTINEL, torch.int32)
    hb = _full((n + 2,), FILL, torch.uint8)
    cnt = _full((2,), SENTINEL, torch.int64)
    call(hi.data_ptr(), hr.data_ptr(), hb.data_ptr(), n, cnt.data_ptr())
    _sync()
    assert cnt.cpu().tolist() == [n, n]
    hi, hr, hb = hi.cpu().numpy(), hr.cpu().numpy(), hb.cpu().numpy()
    assert hi[:n].tolist() == list(range(n)) and (hi[n:] == SENTINEL).all() and (hr[n:] == SENTINEL).all() and (hb[n:] == FILL).all()
    return hr[:n], hb[:n]


# ------------------------------------------------------------------------------------------------------------ 1. the merged resolve
def test_one_resolve_kernel_for_plain_strand_bytes_and_chosen_strands(pkg, orc):
    """six pairs over four DNA sequences of 1 - 9 letters, pair 2 with a bad index and pair 4 with a window past its sequence's end,
    through the plain entry, the entry with strand bytes (the byte 2 makes pair 3 bad, and only pair 3), both strands and the stranded
    search on the reverse strand"""
    seqs = [b"G", b"ACGT", b"GATTACAGA", b"TTGCAA"]
    assert [len(s) for s in seqs] == [1, 4, 9, 6]
    pairs = pairs_ref.pairs_array([(0, 1), (2, 3), (7, 1), (1, 2, 1, 3, 2, 5), (3, 0, 4, 5, 0, -1), (2, 2)])
    n = len(pairs)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    S = pkg.SeqSet.new(seqs)
    d_pairs = _pairs_up(pairs)
    bad_desc = [2, 4]
    assert [k for k, s in enumerate(pairs_ref.resolve(seqs, seqs, pairs)) if s is None] == bad_desc
    rec_of = lambda strand: _oracle(orc, om, pairs_ex_ref.resolve(seqs, seqs, pairs, strand), 5, 2)
    # the plain entry
    want = rec_of(None)
    got, = _three_chunks(n, lambda chunk: _align(lambda rec, _: pkg.align_pairs_device(
        cfg, S, S, n, d_pairs.data_ptr(), 9, 9, rec, None, _stream(), chunk), n, byte_out=False))
    assert got.tobytes() == want.tobytes() and [k for k in range(n) if got[k].tolist() == BAD] == bad_desc
    # a strand byte per pair
    strand = np.array([0, 1, 0, 2, 1, 0], dtype=np.uint8)
    d_strand = _up(strand)
    want = rec_of(strand)
    got, = _three_chunks(n, lambda chunk: _align(lambda rec, _: pkg.align_pairs_ex_device(
        cfg, S, S, n, d_pairs.data_ptr(), d_strand.data_ptr(), 9, 9, rec, None, None, None, 0, None, _stream(), chunk), n, byte_out=False))
    assert got.tobytes() == want.tobytes() and [k for k in range(n) if got[k].tolist() == BAD] == [2, 3, 4]
    # both strands: the higher score, the forward strand on a tie; a bad pair reports strand 0
    rec0, rec1 = rec_of(np.zeros(n, dtype=np.uint8)), rec_of(np.ones(n, dtype=np.uint8))
    wwon = (rec1[:, 0] > rec0[:, 0]).astype(np.uint8)
    want = np.where(wwon[:, None] == 1, rec1, rec0)
    got, won = _three_chunks(n, lambda chunk: _align(lambda rec, byte: pkg.align_pairs_both_device(
        cfg, S, S, n, d_pairs.data_ptr(), 9, 9, rec, None, byte, _stream(), chunk), n))
    assert got.tobytes() == want.tobytes() and won.tolist() == wwon.tolist()
    assert all(got[k].tolist() == BAD and won[k] == 0 for k in bad_desc)
    # the stranded search on the reverse strand, every pair a hit: the mark is out of the flags, the byte is the strand
    got, won = _three_chunks(n, lambda chunk: _search(lambda hi, hr, hb, cap, cnt: pkg.search_pairs_stranded_device(
        cfg, S, S, LIST, 0, n, d_pairs.data_ptr(), 9, 9, INT32_MIN, None, hi, hr, None, cap, cnt, REV, hb, _stream(), chunk), n))
    assert got.tobytes() == rec1.tobytes()
    assert won.tolist() == [0 if k in bad_desc else 1 for k in range(n)]


# --------------------------------------------------------------------------------------------- 2. the merged fold: ties, missing slots
def test_palindromic_query_reports_the_forward_strand(pkg, orc):
    seqs = [b"ACGT", b"ACGTT", b"GGACGTAC", b"AACGT"]
    assert pairs_ex_ref.revcomp(seqs[0]) == seqs[0]
    pairs = pairs_ref.pairs_array([(0, 1), (0, 2), (3, 1), (0, 3)])
    n = len(pairs)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, pm.inner)
    S = pkg.SeqSet.new(seqs)
    d_pairs = _pairs_up(pairs)
    rec0 = _oracle(orc, om, pairs_ex_ref.resolve(seqs, seqs, pairs, np.zeros(n, dtype=np.uint8)), 5, 2)
    rec1 = _oracle(orc, om, pairs_ex_ref.resolve(seqs, seqs, pairs, np.ones(n, dtype=np.uint8)), 5, 2)
    wwon = (rec1[:, 0] > rec0[:, 0]).astype(np.uint8)
    want = np.where(wwon[:, None] == 1, rec1, rec0)
    assert rec0[0].tolist() == rec1[0].tolist() and rec0[0][0] == 8 and wwon[2] == 1          # a tie with a score, and a reverse winner beside it
    got, won = _three_chunks(n, lambda chunk: _align(lambda rec, byte: pkg.align_pairs_both_device(
        cfg, S, S, n, d_pairs.data_ptr(), 8, 8, rec, None, byte, _stream(), chunk), n))
    assert got.tobytes() == want.tobytes() and won.tolist() == wwon.tolist() and won[0] == 0 and won[1] == 0 and won[3] == 0
    hrec, hwon = _three_chunks(n, lambda chunk: _search(lambda hi, hr, hb, cap, cnt: pkg.search_pairs_stranded_device(
        cfg, S, S, LIST, 0, n, d_pairs.data_ptr(), 8, 8, INT32_MIN, None, hi, hr, None, cap, cnt, BOTH, hb, _stream(), chunk), n))
    assert hrec.tobytes() == got.tobytes() and hwon.tolist() == won.tolist()                  # (flags 0: PMX_FLAG_STRAND1 is stripped)


def _b62(pkg, orc):
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))


@pytest.mark.parametrize("ref_side", [False, True])
def test_frames_tie_and_frames_that_do_not_exist(pkg, orc, ref_side):
    """AAAA against K in all six frames: frames 0 and 1 both read AAA = K and tie, frame 0 is reported; frames 2 and 5 have no codon
    and are passed over; the reverse frames read TTT = F and lose.  A window of two nucleotides has no frame: a bad pair."""
    nuc = [b"AAAA", b"AA", b"ACGTACGAT"]
    prot = [b"K", b"KF", b"TYD"]
    rows = [(0, 0), (1, 0), (2, 2), (0, 1), (2, 1), (0, 0, 1, 2, 0, -1)]
    if ref_side:
        rows = [(t[1], t[0]) if len(t) == 2 else (t[1], t[0], t[4], t[5], t[2], t[3]) for t in rows]
    pairs = pairs_ref.pairs_array(rows)
    n = len(pairs)
    pm, om = _b62(pkg, orc)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, OPEN, EXT, 0, 0, pm.inner)
    qseqs, rseqs = (prot, nuc) if ref_side else (nuc, prot)
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    mq, mr = 3, 3                                                                             # letters on either side
    resolve = trs.resolve if ref_side else tr.resolve
    per_frame = [resolve(qseqs, rseqs, pairs, [f] * n, mq, mr) for f in range(6)]
    recs = np.stack([_oracle(orc, om, s, OPEN, EXT) for s in per_frame])
    exists = np.array([[x is not None for x in s] for s in per_frame])
    want, _, wwon = tr.fold(recs, exists)
    assert exists[:, 0].tolist() == [True, True, False, True, True, False]
    assert recs[0, 0].tolist() == recs[1, 0].tolist() == [5, 0, 0, 0] and recs[3, 0][0] == 0 and wwon[0] == 0
    assert not exists[:, 1].any() and not exists[:, 5].any() and want[1].tolist() == BAD and wwon[1] == 0
    assert wwon[3] == 3 and recs[3, 3][0] > recs[0, 3][0]                                     # a reverse frame wins beside them
    d_pairs = _pairs_up(pairs)
    align = pkg.align_pairs_translated_ref_device if ref_side else pkg.align_pairs_translated_device
    search = pkg.search_pairs_translated_ref_device if ref_side else pkg.search_pairs_translated_device
    got, won = _three_chunks(n, lambda chunk: _align(lambda rec, byte: align(
        cfg, Q, R, n, d_pairs.data_ptr(), None, pkg.FRAMES_ALL, mq, mr, rec, None, byte, _stream(), chunk), n))
    assert got.tobytes() == want.tobytes() and won.tolist() == wwon.tolist()
    hrec, hwon = _three_chunks(n, lambda chunk: _search(lambda hi, hr, hb, cap, cnt: search(
        cfg, Q, R, LIST, 0, n, d_pairs.data_ptr(), mq, mr, INT32_MIN, None, hi, hr, None, cap, cnt, pkg.FRAMES_ALL, hb, _stream(), chunk), n))
    assert hrec.tobytes() == got.tobytes() and hwon.tolist() == won.tolist()                  # (the frame bits are out of the flags)


@pytest.mark.parametrize("ref_side", [False, True])
def test_palindromic_window_reports_the_forward_strand_in_the_frameshift_entries(pkg, orc, ref_side):
    nuc = [b"AAATTT", b"GATTACAGATTACA", b"AT", b"TGTAATCTGTAATC"]
    prot = [b"KNIF", b"DYR", b"LQIT"]
    assert pairs_ex_ref.revcomp(nuc[0]) == nuc[0] and fs.codon_stream(nuc[0]) == b"KNIF"
    rows = [(0, 0), (1, 1), (2, 0), (3, 1), (1, 2), (0, 2)]
    if ref_side:
        rows = [(t[1], t[0]) for t in rows]
    pairs = pairs_ref.pairs_array(rows)
    n = len(pairs)
    pm, om = _b62(pkg, orc)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, OPEN, EXT, 0, 0, pm.inner)
    qseqs, rseqs = (prot, nuc) if ref_side else (nuc, prot)
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    mq, mr = (4, 12) if ref_side else (12, 4)
    model = fsr if ref_side else fs
    want, wwon = model.records(qseqs, rseqs, pairs, BOTH, om, OPEN, EXT, SHIFT, max_qlen=mq, max_rlen=mr)
    assert want[0][0] > 0 and wwon[0] == 0 and want[2].tolist() == BAD and wwon[2] == 0 and 0 < wwon.sum() < n
    d_pairs = _pairs_up(pairs)
    align = pkg.align_pairs_frameshift_ref_device if ref_side else pkg.align_pairs_frameshift_device
    got, won = _three_chunks(n, lambda chunk: _align(lambda rec, byte: align(
        cfg, Q, R, n, d_pairs.data_ptr(), None, BOTH, SHIFT, mq, mr, rec, byte, _stream(), chunk), n))
    assert got.tobytes() == want.tobytes() and won.tolist() == wwon.tolist()

    def search(hi, hr, hb, cap, cnt, chunk):
        opts = pkg.pmx_pairs_opts_t(chunk)
        entry = pkg.lib.pmx_search_pairs_frameshift_ref_device if ref_side else pkg.lib.pmx_search_pairs_frameshift_device
        rc = entry(C.byref(cfg), Q._handle(), R._handle(), LIST, 0, n, d_pairs.data_ptr(), mq, mr, INT32_MIN, None, hi, hr, None, cap, cnt,
                   _stream(), C.byref(opts), BOTH, hb, SHIFT, None)
        assert rc == 0, pkg.lib.pmx_last_error()
    hrec, hwon = _three_chunks(n, lambda chunk: _search(lambda hi, hr, hb, cap, cnt: search(hi, hr, hb, cap, cnt, chunk), n))
    assert hrec.tobytes() == got.tobytes() and hwon.tolist() == won.tolist()                  # (flags 0: PMX_FLAG_STRAND1 is stripped)


# ------------------------------------------------------------------------------------------------- 3. five gather hooks, one body
NUC = [b"ACGTTGCAAGG", b"GATTACA", b"TTGACCGTAAC"]
PROT = [b"MKVLA", b"WY", b"HEAGAWGHEE"]


def _edge_pairs(qseqs, rseqs, ql, rl):
    """the first ql / rl bytes of the first sequences, the last ql / rl bytes of the last ones"""
    return pairs_ref.pairs_array([(0, 0, 0, ql, 0, rl), (len(qseqs) - 1, len(rseqs) - 1, len(qseqs[-1]) - ql, ql, len(rseqs[-1]) - rl, rl)])


HOOKS = {
    "plain": (NUC, NUC, 7, 5, lambda pkg: pkg.gather_pairs_device,
              lambda q, r, b: (pairs_ex_ref.revcomp(q) if b else q, r)),
    "translated": (NUC, PROT, 10, 4, lambda pkg: pkg.gather_pairs_translated_device,
                   lambda q, r, b: (tr.translate(q, b), r)),
    "translated_ref": (PROT, NUC, 4, 10, lambda pkg: pkg.gather_pairs_translated_ref_device,
                       lambda q, r, b: (q, tr.translate(r, b))),
    "codons": (NUC, PROT, 7, 4, lambda pkg: pkg.gather_pairs_codons_device,
               lambda q, r, b: (fs.codon_stream(q, b), r)),
    "codons_ref": (PROT, NUC, 4, 7, lambda pkg: pkg.gather_pairs_codons_ref_device,
                   lambda q, r, b: (q, fsr.stream(r, b))),
}


@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_gather_hook_stops_at_its_capacity(pkg, hook):
    """two pairs at the two ends of the sets, capacities one byte short of the second window: the first window is written and is the
    reference's, not a byte of the second is, the offsets and the caller's ok column are filled"""
    import torch
    qseqs, rseqs, ql, rl, entry, model = HOOKS[hook]
    pairs = _edge_pairs(qseqs, rseqs, ql, rl)
    byte = np.array([4, 1] if hook.startswith("translated") else [1, 0], dtype=np.uint8)      # a reverse frame / the reverse strand first
    windows = pairs_ref.resolve(qseqs, rseqs, pairs)
    want = [model(q, r, int(b)) for (q, r), b in zip(windows, byte)]
    assert all(len(w[0]) >= 2 and len(w[1]) >= 2 for w in want)
    qoffw = [0, len(want[0][0]), len(want[0][0]) + len(want[1][0])]
    roffw = [0, len(want[0][1]), len(want[0][1]) + len(want[1][1])]
    Q, R = pkg.SeqSet.new(qseqs), pkg.SeqSet.new(rseqs)
    qout = _full((qoffw[2] + 8,), FILL, torch.uint8); rout = _full((roffw[2] + 8,), FILL, torch.uint8)
    qoff = _full((3 + 2,), SENTINEL, torch.int64); roff = _full((3 + 2,), SENTINEL, torch.int64)
    ok = _full((2 + 2,), FILL, torch.uint8)
    d_pairs = _pairs_up(pairs); d_byte = _up(byte)
    entry(pkg)(Q, R, 2, d_pairs.data_ptr(), d_byte.data_ptr(), 16, 16, qout.data_ptr(), qoffw[2] - 1, qoff.data_ptr(),
               rout.data_ptr(), roffw[2] - 1, roff.data_ptr(), ok.data_ptr(), _stream())
    _sync()
    qout, rout, qoff, roff, ok = [t.cpu().numpy() for t in (qout, rout, qoff, roff, ok)]
    assert qoff[:3].tolist() == qoffw and roff[:3].tolist() == roffw and (qoff[3:] == SENTINEL).all() and (roff[3:] == SENTINEL).all()
    assert ok[:2].tolist() == [1, 1] and (ok[2:] == FILL).all()
    assert qout[:qoffw[1]].tobytes() == want[0][0] and (qout[qoffw[1]:] == FILL).all()
    assert rout[:roffw[1]].tobytes() == want[0][1] and (rout[roffw[1]:] == FILL).all()
