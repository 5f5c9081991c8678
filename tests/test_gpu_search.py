"""Profile database search (`-m gpu`): pmx_select_hits_device against the numpy reference (tests/search_ref.py), bit-exact in both
orders; pmx_gather_refs_device against numpy slicing; pmx_search_profile / _device end to end on config 5's own inputs against the CPU
oracle (first-pass records, banded records, CIGAR text, statistics, begins) and against the composition a caller could write before
(pmx_align_profile_batch, a numpy gather, pmx_align_batch_banded_cigar); other modes and matrices; two host threads side by side."""
import ctypes as C
import threading

import numpy as np
import pytest

import search_ref
import workloads as wl
from util import random_seqs, mutate, AA, golden

pytestmark = pytest.mark.gpu

INT32_MIN = -(1 << 31)
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


# ---------------------------------------------------------------------------------------------------------------- 1. selection
def _select(pkg, d_rec, n, min_score, max_hits, order, capacity):
    import torch
    idx = torch.full((max(capacity, 1) + 8,), SENTINEL, dtype=torch.int64, device=_dev())
    counts = torch.full((2,), SENTINEL, dtype=torch.int64, device=_dev())
    pkg.select_hits_device(d_rec.data_ptr(), n, min_score, max_hits, order, idx.data_ptr(), capacity, counts.data_ptr(), _stream())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), counts.cpu().numpy()


def _tie_run_cut(scores, min_score):
    """a max_hits that ends inside a tie run of the passing scores (0 when there is no run of two)"""
    s = np.sort(scores[scores >= min_score])[::-1]
    if len(s) < 2:
        return 0
    v = s[len(s) // 2]
    above, run = int((s > v).sum()), int((s == v).sum())
    return above + run // 2 if run >= 2 else 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 100003, 1250000])
def test_selection_equals_reference(pkg, n):
    rng = np.random.default_rng(5200 + n % 977)
    scores = search_ref.tied_scores(rng, n)
    assert len(np.unique(scores)) <= 20 and (n < 63 or scores.min() < 0)
    d_rec = _up(search_ref.records(scores, rng))
    values = np.unique(scores)
    small_capacity_done = 0
    for min_score in (INT32_MIN, int(values[len(values) // 2]), int(values[-1]) + 1):
        npass = int((scores >= min_score).sum())
        assert (npass == 0) == (min_score > values[-1])
        for max_hits in sorted({0, 1, _tie_run_cut(scores, min_score), npass, npass + 1}):
            for order in (search_ref.BY_INDEX, search_ref.BY_SCORE):
                want, wp = search_ref.select(scores, min_score, max_hits, order)
                got, counts = _select(pkg, d_rec, n, min_score, max_hits, order, n)
                assert counts.tolist() == [len(want), wp], (n, min_score, max_hits, order, counts)
                assert (got[:len(want)] == want).all(), (n, min_score, max_hits, order)
                assert (got[len(want):] == SENTINEL).all()
                again, counts2 = _select(pkg, d_rec, n, min_score, max_hits, order, n)
                assert again.tobytes() == got.tobytes() and counts2.tobytes() == counts.tobytes()
                if len(want) >= 2:                                   # a capacity below the number selected
                    cap = len(want) // 2
                    part, pc = _select(pkg, d_rec, n, min_score, max_hits, order, cap)
                    assert pc.tolist() == [len(want), wp]
                    assert (part[:cap] == want[:cap]).all() and (part[cap:] == SENTINEL).all()
                    small_capacity_done += 1
    assert small_capacity_done or n == 1


def test_selection_looks_at_the_score_only_and_takes_extreme_scores(pkg):
    scores = np.array([INT32_MIN, 2147483647, 0, -1, INT32_MIN, 2147483647, 5], dtype=np.int32)
    d_rec = _up(search_ref.records(scores, np.random.default_rng(1)))
    for min_score in (INT32_MIN, -1, 2147483647):
        for max_hits in (0, 1, 3, 6):
            for order in (0, 1):
                want, wp = search_ref.select(scores, min_score, max_hits, order)
                got, counts = _select(pkg, d_rec, len(scores), min_score, max_hits, order, len(scores))
                assert counts.tolist() == [len(want), wp] and (got[:len(want)] == want).all()


def _tie_run_end(scores, min_score):
    """a max_hits that ends exactly behind a tie run of the passing scores: the rank the pick looks for is the last of its bin in every
    pass (0 when nothing would be cut there)"""
    s = np.sort(scores[scores >= min_score])[::-1]
    if len(s) < 2:
        return 0
    k = int((s >= s[len(s) // 2]).sum())
    return k if k < len(s) else 0


def _selection_cases(pkg, scores, d_rec, thresholds, cuts):
    """test_selection_equals_reference's checks on every (min_score, max_hits, order): exact against search_ref.select, the sentinel
    behind the hits, a second run byte-identical, a capacity below the number selected; max_hits: none, one, a cut inside a tie run, one
    exactly behind a tie run, |P| - 1, |P|, |P| + 1 and `cuts`"""
    n = len(scores)
    small_capacity_done = 0
    for min_score in thresholds:
        npass = int((scores >= min_score).sum())
        for max_hits in sorted({0, 1, _tie_run_cut(scores, min_score), _tie_run_end(scores, min_score), max(npass - 1, 0), npass, npass + 1} | set(cuts)):
            for order in (search_ref.BY_INDEX, search_ref.BY_SCORE):
                want, wp = search_ref.select(scores, min_score, max_hits, order)
                got, counts = _select(pkg, d_rec, n, min_score, max_hits, order, n)
                ctx = (n, min_score, max_hits, order)
                assert counts.tolist() == [len(want), wp], (ctx, counts)
                assert (got[:len(want)] == want).all(), ctx
                assert (got[len(want):] == SENTINEL).all(), ctx
                again, counts2 = _select(pkg, d_rec, n, min_score, max_hits, order, n)
                assert again.tobytes() == got.tobytes() and counts2.tobytes() == counts.tobytes(), ctx
                if len(want) >= 2:
                    cap = len(want) // 2
                    part, pc = _select(pkg, d_rec, n, min_score, max_hits, order, cap)
                    assert pc.tolist() == [len(want), wp], ctx
                    assert (part[:cap] == want[:cap]).all() and (part[cap:] == SENTINEL).all(), ctx
                    small_capacity_done += 1
    return small_capacity_done


@pytest.mark.parametrize("n", [257, 2047, 2048, 2049, 100003])
@pytest.mark.parametrize("name", sorted(search_ref.WIDE_SCORES))
def test_selection_over_the_whole_key_range(pkg, name, n):
    """scores that spread over the radix select's digits -- all of int32, the top digit only, the middle digit only, the low digit
    only, clusters at the digit borders and the ends of int32 -- where tied_scores() fills two bins of the first pass and one per sign
    of the second: the choice among bins and what the passes hand on (krem, gt, prefix, mask) decide the result here"""
    rng = np.random.default_rng(5400 + n % 977)
    scores = search_ref.WIDE_SCORES[name](rng, n)
    values = np.unique(scores)
    top = int(values[-1])
    thresholds = (int(values[0]), int(values[len(values) // 2]), top + 1 if top < search_ref.INT32_MAX else top)
    assert (int((scores >= thresholds[2]).sum()) == 0) == (top < search_ref.INT32_MAX)         # (nothing lies above INT32_MAX)
    T, above, E = search_ref.radix_select_model(scores, thresholds[0], n // 2)
    assert T is not None and above + E == n // 2
    d_rec = _up(search_ref.records(scores, rng))
    assert _selection_cases(pkg, scores, d_rec, thresholds, (n // 2,))


@pytest.mark.parametrize("which", ["top", "middle"])
def test_selection_kth_score_in_bin_0(pkg, which):
    """the K-th score in bin 0 of the first pass / of the second pass: the bin the pick loop takes without looking at it"""
    scores = search_ref.bin0_scores(which)
    n = len(scores)
    shift, bits = search_ref.DIGITS[0 if which == "top" else 1]
    cuts = (601, 900, 1800, n - 1)
    for k in cuts:
        T, above, E = search_ref.radix_select_model(scores, INT32_MIN, k)
        Tu = (T & 0xFFFFFFFF) ^ 0x80000000
        assert (Tu >> shift) & ((1 << bits) - 1) == 0 and above >= 600 and above + E == k
        assert which == "top" or Tu >> 21 != 0
    d_rec = _up(search_ref.records(scores, np.random.default_rng(5500)))
    median = int(np.sort(scores)[n // 2])
    assert _selection_cases(pkg, scores, d_rec, (INT32_MIN, median), cuts)


# ------------------------------------------------------------------------------------------------------------------- 2. gather
def _gather(pkg, d_rbuf_ptr, d_roff, n, index, out_capacity):
    import torch
    h = len(index)
    d_idx = _up(np.asarray(index, dtype=np.int64))
    out = torch.full((out_capacity + 64,), 0x5A, dtype=torch.uint8, device=_dev())
    off = torch.full((h + 1,), SENTINEL, dtype=torch.int64, device=_dev())
    pkg.gather_refs_device(d_rbuf_ptr, d_roff.data_ptr(), n, d_idx.data_ptr(), h, out.data_ptr(), out_capacity, off.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), off.cpu().numpy()


def test_gather_equals_numpy_slicing(pkg):
    rng = np.random.default_rng(5300)
    refs, targets = [], []
    refs.append(random_seqs(rng, 1, 3, 3)[0]); targets.append(0)                 # the first reference of the buffer
    pos = 3
    for a in range(4):                                                           # lengths 1..40 at every source alignment mod 4
        for L in range(1, 41):
            fill = (a - pos) % 4 or 4
            refs.append(random_seqs(rng, 1, fill, fill)[0]); pos += fill
            assert pos % 4 == a
            targets.append(len(refs)); refs.append(random_seqs(rng, 1, L, L)[0]); pos += L
    for L in (5000, 4999, 5003, 5001):                                           # 5 kbp references
        targets.append(len(refs)); refs.append(random_seqs(rng, 1, L, L)[0])
    refs.append(random_seqs(rng, 1, 7, 7)[0]); targets.append(len(refs) - 1)     # the last reference of the buffer
    rbuf, roff = pkg.pack(refs)
    n = len(refs)
    seen = {(int(roff[k]) % 4, len(refs[k])) for k in targets}
    assert all((a, L) in seen for a in range(4) for L in range(1, 41))
    d_roff = _up(roff)
    exact = _up(rbuf)                                                            # exactly roff[n] bytes: no slack behind the last reference
    assert exact.numel() == roff[n]
    shifted = _up(np.concatenate([np.zeros(1, dtype=np.uint8), rbuf]))           # ... and a base address that is not dword-aligned
    for base in (exact.data_ptr(), shifted.data_ptr() + 1):
        for index in (targets, list(rng.permutation(targets)), list(range(n)), [targets[5]] * 3):
            want = b"".join(refs[k] for k in index)
            woff = np.concatenate([[0], np.cumsum([len(refs[k]) for k in index])])
            out, off = _gather(pkg, base, d_roff, n, index, len(want))
            assert (off == woff).all()
            assert out[:len(want)].tobytes() == want
            assert (out[len(want):] == 0x5A).all()
    # a capacity that some references cross: those are not written, the others are
    index = targets
    woff = np.concatenate([[0], np.cumsum([len(refs[k]) for k in index])])
    cap = int(woff[len(index) // 2]) + 1
    out, off = _gather(pkg, exact.data_ptr(), d_roff, n, index, cap)
    assert (off == woff).all()
    fits = int((woff[1:] <= cap).sum())
    assert out[:woff[fits]].tobytes() == b"".join(refs[k] for k in index[:fits]) and (out[woff[fits]:] == 0x5A).all()
    out, off = _gather(pkg, exact.data_ptr(), d_roff, n, [], 0)
    assert off.tolist() == [0]


# --------------------------------------------------------------------------------------------------------------- device entry
class _DeviceSearch:
    """pmx_search_profile_device into fresh sentinel-filled buffers; results as numpy"""

    def __init__(self, pkg, al, rbuf, roff):
        self.pkg, self.al, self.n = pkg, al, len(roff) - 1
        self.d_rbuf, self.d_roff = _up(rbuf), _up(roff)
        self.max_rlen = int(np.max(roff[1:] - roff[:-1]))

    def run(self, min_score, max_hits, order, band, stats=False, capacity=None, cigar_capacity=1 << 22, stream=None, want=None):
        import torch
        pkg, dev = self.pkg, _dev()
        capacity = self.n if capacity is None else capacity
        cfg = self.al._config()
        cfg.want = want if want is not None else ((pkg.WANT_CIGAR | (pkg.WANT_STATS if stats else 0)) if band >= 0 else 0)
        hits = torch.full((capacity + 2, 10), SENTINEL, dtype=torch.int32, device=dev)
        recs = torch.full((capacity + 2, 4), SENTINEL, dtype=torch.int32, device=dev)
        st = torch.full((capacity + 2, 3), SENTINEL, dtype=torch.int32, device=dev)
        text = torch.full((cigar_capacity + 64,), 0x5A, dtype=torch.uint8, device=dev)
        toff = torch.full((capacity + 3,), SENTINEL, dtype=torch.int64, device=dev)
        counts = torch.full((2,), SENTINEL, dtype=torch.int64, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        torch.cuda.current_stream(dev).synchronize()                 # (the sentinel fills ran on this thread's current stream, not on `s`)
        pkg.search_profile_device(cfg, self.al._profile, self.n, self.d_rbuf.data_ptr(), self.d_roff.data_ptr(), self.max_rlen,
                                  min_score, max_hits, order, band, None, hits.data_ptr(), recs.data_ptr(), st.data_ptr(), capacity,
                                  text.data_ptr(), cigar_capacity, toff.data_ptr(), counts.data_ptr(), s.cuda_stream)
        s.synchronize()
        return {"hits": hits.cpu().numpy().view(pkg.HIT_DTYPE).reshape(-1), "recs": recs.cpu().numpy().view(pkg.RECORD_DTYPE).reshape(-1),
                "stats": st.cpu().numpy().view(pkg.STATS_DTYPE).reshape(-1), "text": text.cpu().numpy(), "toff": toff.cpu().numpy(),
                "counts": counts.cpu().numpy()}


def _same_as_host(pkg, dv, host, band, stats):
    """the device entry's outputs equal a SearchHits of the host entry byte for byte; what lies beyond the hits is untouched"""
    h = host.n_hits
    assert dv["counts"].tolist() == [h, host.n_passing]
    assert dv["hits"][:h].tobytes() == host.hits.tobytes()
    assert (dv["hits"][h:].view(np.int32) == SENTINEL).all()
    if band >= 0:
        assert dv["recs"][:h].tobytes() == host.recs.tobytes() and (dv["recs"][h:].view(np.int32) == SENTINEL).all()
        assert (dv["toff"][:h + 1] == host.cigar_off).all()
        assert dv["text"][:host.cigar_off[h]].tobytes() == host.cigar_text.tobytes()
        if stats:
            assert dv["stats"][:h].tobytes() == host.stats.tobytes() and (dv["stats"][h:].view(np.int32) == SENTINEL).all()
    else:
        assert (dv["toff"][:h + 1] == 0).all() and (dv["recs"].view(np.int32) == SENTINEL).all()
    assert (dv["toff"][h + 1:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------- 3. config 5's own inputs
@pytest.fixture(scope="module")
def cfg5(pkg, orc):
    q, rbuf, roff, planted = wl.make_cfg5(4000)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    al = pkg.Aligner.new().local().profile(pkg.Profile.new(q, False, pm)).matrix(pm).gap_open(5).gap_extend(2).build()
    full, _ = orc.cpu_sw_striped16_batch(None, None, rbuf, roff, 5, 2, om, shared_query=q)
    return {"q": q, "rbuf": rbuf, "roff": roff, "planted": planted, "pm": pm, "om": om, "al": al, "oracle": full}


def _first_equals(hits, oracle_rows):
    f = hits.hits["first"]
    assert (f["score"] == oracle_rows[:, 0]).all() and (f["end_query"] == oracle_rows[:, 1]).all() and (f["end_ref"] == oracle_rows[:, 2]).all()
    assert (f["flags"] == 0).all() and (hits.hits["reserved"] == 0).all()
    assert (hits.hits["diag"] == oracle_rows[:, 2] - oracle_rows[:, 1]).all()


def test_search_cfg5_planted_hits_against_the_oracle(pkg, orc, cfg5):
    c = cfg5
    q, rbuf, roff, planted, om = c["q"], c["rbuf"], c["roff"], c["planted"], c["om"]
    # the data as the issue states it
    s = c["oracle"][:, 0]
    assert len(planted) == 40 and s[planted].min() == 889 and s[planted].max() == 1809 and np.delete(s, planted).max() == 35
    hits = c["al"].search_profile_packed(rbuf, roff, 200, band=48, stats=True)
    name = pkg.lib.pmx_last_kernel().decode()
    assert "pmx_select" in name and "pmx_gather_refs_kernel" in name and name.endswith("pmx_walkb_kernel"), name
    assert hits.n_hits == 40 and hits.n_passing == 40 and (hits.index == planted).all()
    _first_equals(hits, c["oracle"][planted])
    rs = [rbuf[roff[k]:roff[k + 1]].tobytes() for k in planted]
    rb, ro = orc.pack(rs)
    qb, qo = orc.pack([q] * len(rs))
    scalar = orc.align_batch(orc.SW, qb, qo, rb, ro, 5, 2, om)
    assert (scalar == c["oracle"][planted]).all()
    diag = hits.hits["diag"]
    banded = orc.align_banded_batch(orc.SW, None, None, rb, ro, 5, 2, om, 48, diag, shared_query=q)
    for f, col in (("score", 0), ("end_query", 1), ("end_ref", 2)):
        assert (hits.recs[f] == banded[:, col]).all() and (hits.recs[f] == hits.hits["first"][f]).all()
    assert (hits.recs["flags"] == 0).all()
    for k in range(len(rs)):
        want = search_ref.oracle_banded(orc, orc.SW, 0, q, rs[k], 5, 2, om, 48, int(diag[k]))
        assert search_ref.hit_tuple(hits, k) == want, (k, search_ref.hit_tuple(hits, k), want)
    beg = np.stack([hits.beg_query, hits.beg_ref], axis=1).astype(np.int32)
    got, bad = orc.rescore_cigars(hits.cigar_text if len(hits.cigar_text) else np.zeros(1, dtype=np.uint8), hits.cigar_off, qb, qo, rb, ro,
                                  5, 2, om, beg=beg.reshape(-1))
    assert bad == 0
    assert (got[:, 0] == hits.recs["score"]).all()
    assert (got[:, 1] == hits.recs["end_query"] - hits.beg_query + 1).all()
    assert (got[:, 2] == hits.recs["end_ref"] - hits.beg_ref + 1).all()
    assert (got[:, 3] == 0).all()


@pytest.mark.parametrize("band", [8, 15, 31, 63])
def test_search_cfg5_other_bands_keep_the_planted_records(pkg, orc, cfg5, band):
    c = cfg5
    hits = c["al"].search_profile_packed(c["rbuf"], c["roff"], 200, band=band)
    assert (hits.index == c["planted"]).all()
    for f in ("score", "end_query", "end_ref"):
        assert (hits.recs[f] == hits.hits["first"][f]).all()
    k = 7
    r = c["rbuf"][c["roff"][c["planted"][k]]:c["roff"][c["planted"][k] + 1]].tobytes()
    want = search_ref.oracle_banded(orc, orc.SW, 0, c["q"], r, 5, 2, c["om"], band, int(hits.hits["diag"][k]))
    assert (hits.cigars[k], int(hits.beg_query[k]), int(hits.beg_ref[k])) == (want[3], want[7], want[8])


@pytest.mark.parametrize("order", [search_ref.BY_INDEX, search_ref.BY_SCORE])
def test_search_cfg5_cut_inside_a_tie_run_host_and_device(pkg, orc, cfg5, order):
    c = cfg5
    s = c["oracle"][:, 0]
    want, wp = search_ref.select(s, 20, 340, order)
    assert wp == 3702 and s[want].min() == 27 and int((s[want] == 27).sum()) == 108 and int((s == 27).sum()) == 120
    assert int((s == 22).sum()) == 678
    host = c["al"].search_profile_packed(c["rbuf"], c["roff"], 20, max_hits=340, order=order, band=48, stats=True)
    assert host.n_hits == 340 and host.n_passing == 3702 and (host.index == want).all()
    _first_equals(host, c["oracle"][want])
    ds = _DeviceSearch(pkg, c["al"], c["rbuf"], c["roff"])
    _same_as_host(pkg, ds.run(20, 340, order, 48, stats=True), host, 48, True)
    # a hit capacity below the number selected: the first ones in output order, the counts in full
    dv = ds.run(20, 340, order, 48, stats=True, capacity=100)
    assert dv["counts"].tolist() == [340, 3702]
    assert dv["hits"][:100].tobytes() == host.hits[:100].tobytes() and (dv["hits"][100:].view(np.int32) == SENTINEL).all()
    assert dv["recs"][:100].tobytes() == host.recs[:100].tobytes() and (dv["toff"][:101] == host.cigar_off[:101]).all()
    assert dv["text"][:host.cigar_off[100]].tobytes() == host.cigar_text[:host.cigar_off[100]].tobytes()
    # no second pass: the same hits, begins -1
    first_only = c["al"].search_profile_packed(c["rbuf"], c["roff"], 20, max_hits=340, order=order, band=-1)
    assert (first_only.index == want).all() and first_only.recs is None and first_only.stats is None
    assert (first_only.beg_query == -1).all() and (first_only.beg_ref == -1).all() and (first_only.cigar_off == 0).all()
    assert first_only.hits["first"].tobytes() == host.hits["first"].tobytes()
    _same_as_host(pkg, ds.run(20, 340, order, -1), first_only, -1, False)


def test_search_cfg5_equals_the_composition_a_caller_could_write(pkg, orc, cfg5):
    c = cfg5
    al, rbuf, roff = c["al"], c["rbuf"], c["roff"]
    for min_score, max_hits, order in ((200, 0, 0), (20, 340, 1)):
        host = al.search_profile_packed(rbuf, roff, min_score, max_hits=max_hits, order=order, band=48, stats=True)
        full = al.align_batch_packed(None, None, rbuf, roff)                       # pmx_align_profile_batch
        index, _ = search_ref.select(full["score"], min_score, max_hits, order)
        sub = [rbuf[roff[k]:roff[k + 1]].tobytes() for k in index]                 # the numpy gather
        diag = (full["end_ref"][index] - full["end_query"][index]).astype(np.int32)
        rec, cig, st = al.align_batch_banded_cigar([], sub, 48, diag, stats=True)  # pmx_align_batch_banded_cigar, profile arm
        assert (host.index == index).all() and host.hits["first"].tobytes() == full[index].tobytes()
        assert host.recs.tobytes() == rec.tobytes() and host.stats.tobytes() == st.tobytes()
        assert host.cigars == cig and host.cigar_text.tobytes() == "".join(cig).encode()


# ----------------------------------------------------------------------------------------------- 4. other modes and matrices
def _related_refs(rng, q, n, alphabet=None):
    kw = {} if alphabet is None else {"alphabet": alphabet}
    rs = []
    for t in range(n):
        if t % 5 == 4:
            rs.append(random_seqs(rng, 1, 20, len(q) + 30, **kw)[0])
        else:
            pre = random_seqs(rng, 1, 0, 12, **kw)[0] if t % 3 == 0 else b""
            rs.append(pre + mutate(rng, q, 0.06, 0.02, **kw) + (random_seqs(rng, 1, 0, 9, **kw)[0] if t % 4 == 1 else b""))
    return rs


@pytest.mark.parametrize("mode", ["nw", "sg"])
def test_search_global_and_semi_global(pkg, orc, mode):
    rng = np.random.default_rng(5400 + len(mode) + (mode == "sg"))
    q = random_seqs(rng, 1, 140, 140)[0]
    rs = _related_refs(rng, q, 300)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    b = pkg.Aligner.new().profile(pkg.Profile.new(q, False, pm)).matrix(pm).gap_open(5).gap_extend(2)
    al = (b.global_() if mode == "nw" else b.semi_global()).build()
    omode, flags = (orc.NW, 0) if mode == "nw" else (orc.SG, orc.SG_ALL)
    rb, ro = orc.pack(rs)
    qb, qo = orc.pack([q] * len(rs))
    full = orc.align_batch(omode, qb, qo, rb, ro, 5, 2, om, sg_flags=flags if mode == "sg" else orc.SG_ALL)
    min_score = int(np.median(full[:, 0]))
    for order in (0, 1):
        want, wp = search_ref.select(full[:, 0], min_score, 120, order)
        hits = al.search_profile(rs, min_score, max_hits=120, order=order, band=31, stats=True)
        assert hits.n_passing == wp and (hits.index == want).all()
        _first_equals(hits, full[want])
        for k, idx in enumerate(want):
            w = search_ref.oracle_banded(orc, omode, flags, q, rs[idx], 5, 2, om, 31, int(hits.hits["diag"][k]))
            assert search_ref.hit_tuple(hits, k) == w, (mode, k, idx, search_ref.hit_tuple(hits, k), w)
        ds = _DeviceSearch(pkg, al, *pkg.pack(rs))
        _same_as_host(pkg, ds.run(min_score, 120, order, 31, stats=True), hits, 31, True)


def test_search_blosum62_local(pkg, orc):
    rng = np.random.default_rng(5500)
    q = random_seqs(rng, 1, 300, 300, alphabet=AA)[0]
    rs = []
    for t in range(160):
        if t % 4 == 0:
            a = int(rng.integers(0, 150))
            rs.append(random_seqs(rng, 1, 5, 200, alphabet=AA)[0] + mutate(rng, q[a:a + 120], 0.15, 0.02, alphabet=AA) +
                      random_seqs(rng, 1, 5, 200, alphabet=AA)[0])
        else:
            rs.append(random_seqs(rng, 1, 50, 600, alphabet=AA)[0])
    pm, om = pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))
    al = pkg.Aligner.new().local().profile(pkg.Profile.new(q, False, pm)).matrix(pm).gap_open(11).gap_extend(1).build()
    rb, ro = orc.pack(rs)
    qb, qo = orc.pack([q] * len(rs))
    full = orc.align_batch(orc.SW, qb, qo, rb, ro, 11, 1, om)
    want, wp = search_ref.select(full[:, 0], 100, 0, 1)
    assert 30 <= wp <= 60
    hits = al.search_profile(rs, 100, order=1, band=31, stats=True)
    assert hits.n_passing == wp and (hits.index == want).all()
    _first_equals(hits, full[want])
    for k, idx in enumerate(want):
        w = search_ref.oracle_banded(orc, orc.SW, 0, q, rs[idx], 11, 1, om, 31, int(hits.hits["diag"][k]))
        assert search_ref.hit_tuple(hits, k) == w, (k, idx)


def test_search_pssm_without_a_second_pass(pkg, orc):
    rng = np.random.default_rng(5600)
    q = random_seqs(rng, 1, 120, 120)[0]
    rs = _related_refs(rng, q, 400)
    pssm = pkg.Matrix.create(b"ACGT", 3, -2).to_pssm(q)
    al = pkg.Aligner.new().local().profile(pkg.Profile.new(q, False, pssm)).matrix(pssm).gap_open(5).gap_extend(2).build()
    rbuf, roff = pkg.pack(rs)
    full = al.align_batch_packed(None, None, rbuf, roff)                            # (the PSSM batch, checked against its oracle elsewhere)
    for order in (0, 1):
        want, wp = search_ref.select(full["score"], 60, 90, order)
        hits = al.search_profile(rs, 60, max_hits=90, order=order, band=-1)
        assert hits.n_passing == wp and (hits.index == want).all() and hits.hits["first"].tobytes() == full[want].tobytes()
        assert (hits.beg_query == -1).all() and hits.recs is None and hits.cigars == [""] * len(want)
    with pytest.raises(pkg.BatchError, match="PSSM"):
        al.search_profile(rs, 60, band=16)


def test_search_zero_hits(pkg, orc, cfg5):
    c = cfg5
    for band in (48, -1):
        hits = c["al"].search_profile_packed(c["rbuf"], c["roff"], 1 << 20, band=band, stats=True)
        assert hits.n_hits == 0 and hits.n_passing == 0 and len(hits.hits) == 0 and hits.cigar_off.tolist() == [0] and hits.cigars == []
        dv = _DeviceSearch(pkg, c["al"], c["rbuf"], c["roff"]).run(1 << 20, 0, 0, band, stats=True)
        assert dv["counts"].tolist() == [0, 0] and dv["toff"][0] == 0 and (dv["hits"].view(np.int32) == SENTINEL).all()
        assert (dv["text"] == 0x5A).all()
    empty = c["al"].search_profile_packed(np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int64), 5)
    assert empty.n_hits == 0 and empty.cigar_off.tolist() == [0]


def test_search_device_cigar_capacity_too_small(pkg, orc, cfg5):
    """the rule of pmx_align_batch_banded_cigar_device: the offsets tell the bytes needed, a hit whose text would cross the capacity is
    not written, nothing is written beyond the capacity"""
    c = cfg5
    host = c["al"].search_profile_packed(c["rbuf"], c["roff"], 200, band=48)
    need = int(host.cigar_off[-1])
    cap = int(host.cigar_off[20]) + 3
    dv = _DeviceSearch(pkg, c["al"], c["rbuf"], c["roff"]).run(200, 0, 0, 48, cigar_capacity=cap)
    assert (dv["toff"][:41] == host.cigar_off).all() and dv["toff"][40] == need > cap
    assert dv["text"][:host.cigar_off[20]].tobytes() == host.cigar_text[:host.cigar_off[20]].tobytes()
    assert (dv["text"][cap:] == 0x5A).all()
    assert dv["recs"][:40].tobytes() == host.recs.tobytes() and dv["hits"][:40].tobytes() == host.hits.tobytes()


def test_search_text_beyond_the_estimate(pkg):
    """the host entry's second text pass: references that alternate match and mismatch against the query ("1=1X..." is two bytes of
    text per column) push the hits' text past the first capacity, (hits x query letters + hit bytes) / 2 + 16 per hit + 256, and the
    second pass runs again at the exact size; texts and records equal the device entry's into a generous buffer"""
    rng = np.random.default_rng(5700)
    q = b"AC" * 50
    rs = [(b"AG" * 60)[:int(L)] for L in rng.integers(94, 107, size=30)]
    pm = pkg.Matrix.create(b"ACGT", 2, -1)
    al = pkg.Aligner.new().global_().profile(pkg.Profile.new(q, False, pm)).matrix(pm).gap_open(5).gap_extend(2).build()
    hits = al.search_profile(rs, -1000, order=1, band=31, stats=True)
    h = hits.n_hits
    assert h == len(rs) and sorted(hits.index.tolist()) == list(range(h))
    assert hits.cigar_off[h] > (h * len(q) + sum(len(r) for r in rs)) // 2 + 16 * h + 256      # the first pass cannot have held it
    assert hits.cigar_off[h] == sum(len(c) for c in hits.cigars) and all(c.count("1=1X") >= 40 for c in hits.cigars)
    ds = _DeviceSearch(pkg, al, *pkg.pack(rs))
    _same_as_host(pkg, ds.run(-1000, 0, 1, 31, stats=True), hits, 31, True)


def test_search_want_sorted_changes_nothing(pkg, orc, cfg5):
    c = cfg5
    host = c["al"].search_profile_packed(c["rbuf"], c["roff"], 200, band=48, stats=True)
    ds = _DeviceSearch(pkg, c["al"], c["rbuf"], c["roff"])
    for want in (pkg.WANT_CIGAR | pkg.WANT_STATS | pkg.WANT_SORTED, pkg.WANT_CIGAR | pkg.WANT_STATS):
        _same_as_host(pkg, ds.run(200, 0, 0, 48, stats=True, want=want), host, 48, True)
    dv = ds.run(200, 0, 0, 48, want=pkg.WANT_STATS)                                   # statistics alone: begins from the statistics walk
    assert dv["hits"][:40].tobytes() == host.hits.tobytes() and dv["stats"][:40].tobytes() == host.stats.tobytes()


# -------------------------------------------------------------------------------------------------------- 5. two host threads
def test_search_two_threads_side_by_side(pkg, orc, cfg5):
    import torch
    c = cfg5
    jobs = [(200, 0, 0, 48), (20, 340, 1, 48)]
    ds = [_DeviceSearch(pkg, c["al"], c["rbuf"], c["roff"]) for _ in jobs]
    single = [d.run(*j, stats=True) for d, j in zip(ds, jobs)]
    streams = [torch.cuda.Stream(device=_dev()) for _ in jobs]
    torch.cuda.synchronize()
    got, errors = [None, None], []

    def work(t):
        try:
            for _ in range(3):
                got[t] = ds[t].run(*jobs[t], stats=True, stream=streams[t])
        except Exception as e:                                                        # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        for key in single[t]:
            assert got[t][key].tobytes() == single[t][key].tobytes(), (t, key)
