"""CPU tier: the band-strip kernel's arithmetic model (tests/bstrip_model.py) against the banded oracle.

The GPU kernel (pmx_bstrip.hip) follows the model cell for cell; what this test pins without a GPU is the DESIGN: boundary
conditions produced by virtual columns / the edge input / the initial state, guarded cells beyond the band, the captures and
their tie rules, and that every intermediate stays inside the int16 window whenever the host predicate admits the batch."""
import numpy as np
import pytest

import bstrip_model as bm
from util import random_seqs, mutate


def _mat5(om):
    return [[int(om.scores[a, b]) for b in range(5)] for a in range(5)]


def _idx(seq):
    return [b"ACGT".index(bytes([c])) for c in seq]


CAPS = [8, 12, 16, 24, 32, 48, 64, 96, 104, 128]


def _cap_for(k):
    for c in CAPS:
        if c >= 2 * k + 1:
            return c
    return 2 * k + 2


def _run_case(orc, rng, mode, sg, match, mis, open_, ext, k, lo, hi, n_pairs, double_skew):
    om = orc.Matrix.create("ACGT", match, mis)
    mat = _mat5(om)
    qs = random_seqs(rng, n_pairs, lo, hi)
    rs, diag = [], np.zeros(n_pairs, dtype=np.int32)
    for t, q in enumerate(qs):
        body = mutate(rng, q, 0.1, 0.05) if rng.random() < 0.8 else random_seqs(rng, 1, lo, hi)[0]
        pre = random_seqs(rng, 1, 0, 30)[0] if rng.random() < 0.5 else b""
        post = random_seqs(rng, 1, 0, 30)[0] if rng.random() < 0.3 else b""
        rs.append((pre + body + post) or b"A")
        diag[t] = len(pre) + int(rng.integers(-6, 7)) if rng.random() < 0.8 else int(rng.integers(-hi - 5, hi + 5))
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    want = orc.align_banded_batch(mode, qb, qo, rb, ro, open_, ext, om, k, diag, sg_flags=sg)
    cap = _cap_for(k)
    n_checked = 0
    for t in range(n_pairs):
        q, r = _idx(qs[t]), _idx(rs[t])
        try:
            got = bm.align(mode, sg, q, r, open_, ext, mat, k, int(diag[t]), cap, double_skew)
        except bm.WindowError as e:
            assert "does not hold" in str(e), (str(e), mode, sg, match, mis, open_, ext, k, len(q), len(r), int(diag[t]))
            continue
        n_checked += 1
        assert tuple(int(x) for x in got) == tuple(int(x) for x in want[t]), \
            (mode, sg, match, mis, open_, ext, k, int(diag[t]), len(q), len(r), got, want[t], double_skew)
    return n_checked


@pytest.mark.parametrize("double_skew", [False, True])
@pytest.mark.parametrize("mode", [bm.NW, bm.SG, bm.SW])
def test_model_matches_the_banded_oracle(orc, mode, double_skew):
    if mode == bm.SW and double_skew:
        pytest.skip("local alignment has one skew only")
    rng = np.random.default_rng(9100 + mode + (7 if double_skew else 0))
    total = 0
    for it in range(60):
        match, mis = [(2, -3), (5, -4), (1, -1), (3, -2)][int(rng.integers(0, 4))]
        open_ = int(rng.choice([1, 2, 3, 5, 11, 20])); ext = int(rng.choice([0, 1, 2, 3]))
        if open_ < ext:
            open_, ext = ext, open_
        k = int(rng.choice([0, 1, 2, 3, 5, 7, 15, 16, 31]))
        lo, hi = [(1, 6), (1, 12), (5, 40), (30, 90)][int(rng.integers(0, 4))]
        sg = int(rng.integers(0, 16)) if mode == bm.SG else 0
        total += _run_case(orc, rng, mode, sg, match, mis, open_, ext, k, lo, hi, 12, double_skew)
    assert total > 300


# every lane shape of pmx_bstrip.hip: bs_shapes (chosen by band) and bs_more (reachable through PMX_BSTRIP_SHAPE only)
BS_SHAPES = [(1, 8), (1, 12), (1, 16), (2, 12), (4, 8), (4, 12), (4, 16), (8, 12), (8, 13), (8, 16), (2, 16), (8, 8)]
_SHAPE_OF_CAP = {8: (1, 8), 32: (4, 8), 104: (8, 13), 128: (8, 16)}


def _geometry(lib, max_qlen, max_rlen, band, G, C, q_shared):
    """pmx_bstrip_geometry (C ABI test hook): (rows, QC, RC, lds) of a launch"""
    import ctypes as C_
    lib.pmx_bstrip_geometry.restype = C_.c_int
    rows, qc, rc, lds = C_.c_int(0), C_.c_int(0), C_.c_int(0), C_.c_longlong(0)
    ok = lib.pmx_bstrip_geometry(max_qlen, max_rlen, band, G, C, q_shared, C_.byref(rows), C_.byref(qc), C_.byref(rc), C_.byref(lds))
    assert ok == 1, (max_qlen, max_rlen, band, G, C, q_shared)
    return rows.value, qc.value, rc.value, lds.value


GEO_LENGTHS = (1, 2, 17, 64, 100, 162, 300, 1000, 5000)


def _pair_lengths(band):
    """the pair lengths the sweep runs through: all of the lattice's maxima, every short length, and the lengths where a band edge
    meets the other sequence's end (x +- band, x +- 2 band, one either side) -- the rows / i_s functions only bend there"""
    s = set(GEO_LENGTHS) | set(range(1, 9))
    for x in GEO_LENGTHS:
        for t in (band, 2 * band):
            for dd in (-1, 0, 1):
                s.update((x + t + dd, x - t + dd))
    return np.array(sorted(v for v in s if 1 <= v <= max(GEO_LENGTHS)), dtype=np.int64)


def _worst_pairs(band):
    """Kernel geometry (pmx_bstrip.hip:164-170; model: bm.plan) of every pair (ql, rl, d0) over the sampled lengths and EVERY band
    centre d0 from one past the miss edge on each side (sampled around the bends when that range is long).  Returns the lengths and,
    per (ql, rl), the most rows a pair runs and the largest first row i_s of a pair that does not miss."""
    L = _pair_lengths(band)
    ql, rl = L[:, None, None], L[None, :, None]
    lo, hi = -(ql - 1) - band - 1, rl - 1 + band + 1                  # one past the miss edge on each side
    span = hi - lo + 1
    # every centre while the range is short (320 from the low miss edge on); beyond that, 7 around every bend and 48 spread over it
    full = lo + np.arange(320)[None, None, :]
    zero = 0 * (ql + rl)
    bends = [zero + b + np.arange(-3, 4)[None, None, :] for b in (lo + 1, -band, 0, band, rl - ql - band, rl - ql, rl - ql + band, hi - 1)]
    spread = lo + (np.arange(48)[None, None, :] * (span - 1)) // 47
    d0 = np.concatenate([zero + x for x in [full] + bends + [spread]], axis=2)
    d0 = np.clip(d0, lo, hi)
    W = 2 * band + 1
    j0 = d0 - band
    miss = (j0 > rl - 1) | (d0 + band < -(ql - 1))
    i_s = np.maximum(0, -j0 - W + 1)
    i_e = np.minimum(ql - 1, rl - 1 - j0)
    rows = i_e - i_s + 1
    live = ~miss & (rows > 0)
    # (spot check: the vectorised geometry is bm.plan's)
    for a, b in ((0, 0), (len(L) - 1, 0), (len(L) // 2, len(L) // 3)):
        for d in (int(d0[a, b, 0]), -band, int(L[b] - L[a])):
            g = bm.plan(bm.NW, int(L[a]), int(L[b]), 0, 0, 0, 0, band, d, 2 * band + 1, False)
            r_ = 0 if g is None else g["i_e"] - g["i_s"] + 1
            j0_, W_ = d - band, 2 * band + 1
            m_ = (j0_ > L[b] - 1) or (d + band < -(L[a] - 1))
            r2 = 0 if m_ else max(0, min(L[a] - 1, L[b] - 1 - j0_) - max(0, -j0_ - W_ + 1) + 1)
            assert r_ == r2, (band, L[a], L[b], d, r_, r2)
    return L, np.where(live, rows, 0).max(axis=2), np.where(live, i_s, 0).max(axis=2)


def test_launch_geometry_covers_every_pair(pkg):
    """The band-strip launcher sizes its LDS streams from the batch's maxima (pmx_bstrip_geometry, the C ABI test hook of the one
    function pmx_launch_bstrip and its window predicate take `rows` from).  For every (max_qlen, max_rlen, band, lane shape, shared
    query) of the lattice, no pair the launch admits may run more rows than `rows` (and some pair runs exactly that many), and the
    highest query-stream / selector-stream index the kernel can read must stay inside its lane group's QC / RC bytes.

    Reads of the kernel (pmx_bstrip.hip), per lane g of a group of G lanes with C offsets each, U = 4:
      * nsteps = max over the wave of rowsLane + G - 1, rounded up to a multiple of U (:258-262);
      * query stream: qs = qs_all + grp * QC + (PADF - g), PADF = G - 1 (:123, :287); it reads qs[0], qs[1] (:329-330) and
        qs[u + 2] for every step u < nsteps (:341): highest index G - 1 + nsteps + 1 (lane 0).  One shared query: qsA = qs_all + i_s +
        (PADF - g) (:288), the same reads on top of the pair's first row i_s;
      * selector stream: rs = rs_all + grp * RC + g * (C - 1) (:286); it reads rs[x] for x < C (:294), rs[C] (:331) and rs[u + C + 1]
        for u < nsteps (:343), whose selectors enter S[C + rho] and shift down every U rows (:342, :496): highest index
        (G - 1)(C - 1) + nsteps + C (lane G - 1)."""
    lib = pkg.lib
    U = 4
    checked = 0
    bad, loose = {"rows": [], "query stream": [], "selector stream": []}, []
    for band in range(64):
        L, worst_rows, worst_is = _worst_pairs(band)
        # the most over ql <= max_qlen, rl <= max_rlen
        cum_rows = np.maximum.accumulate(np.maximum.accumulate(worst_rows, axis=0), axis=1)
        cum_is = np.maximum.accumulate(np.maximum.accumulate(worst_is, axis=0), axis=1)
        shapes = [(G, C) for (G, C) in BS_SHAPES if G * C >= 2 * band + 1]
        import ctypes as C_
        g_, c_ = C_.c_int(0), C_.c_int(0)
        if lib.pmx_bstrip_shape(band, C_.byref(g_), C_.byref(c_)):
            assert (g_.value, c_.value) in shapes, (band, g_.value, c_.value)
        for mq in GEO_LENGTHS:
            a = int(np.searchsorted(L, mq))
            for mr in GEO_LENGTHS:
                b = int(np.searchsorted(L, mr))
                need_rows, need_is = int(cum_rows[a, b]), int(cum_is[a, b])
                for (G, C) in shapes:
                    for q_shared in (0, 1):
                        rows, QC, RC, lds = _geometry(lib, mq, mr, band, G, C, q_shared)
                        tag = (mq, mr, band, (G, C), q_shared, rows, need_rows)
                        nsteps = (need_rows + G - 1 + U - 1) // U * U
                        q_top = (need_is if q_shared else 0) + (G - 1) + nsteps + 1
                        r_top = (G - 1) * (C - 1) + nsteps + C
                        if need_rows > rows:
                            bad["rows"].append(tag)
                        if q_top >= QC:
                            bad["query stream"].append(tag + (q_top, QC))
                        if r_top >= RC:
                            bad["selector stream"].append(tag + (r_top, RC))
                        if need_rows != rows:
                            loose.append(tag)
                        assert lds == (64 // G) * RC + (QC if q_shared else (64 // G) * QC), tag        # the layout of :178
                        checked += 1
    # (max_qlen, max_rlen, band, shape, shared query, rows, rows some pair runs[, highest index read, stream bytes])
    summary = {k: (len(v), v[:3]) for k, v in bad.items() if v}
    assert not summary, summary
    assert not loose, ("the bound is not the most any pair runs", len(loose), loose[:4])
    assert checked > 50000, checked


def test_library_window_predicate_equals_the_model(pkg):
    """the host's admissibility predicate of the band-strip kernel (pmx_bstrip_window, C ABI test hook) against the model's
    `bias_and_low` on a lattice that straddles every edge: score range, gap constants, lengths where the window closes"""
    import ctypes as C
    lib = pkg.lib
    lib.pmx_bstrip_window.restype = C.c_int
    n_ok = n_no = 0
    for mode in (bm.NW, bm.SG, bm.SW):
        for ds in (0, 1):
            if mode == bm.SW and ds:
                continue
            for (smin, smax) in ((-3, 2), (-4, 5), (-1, 1), (-2, 3), (-30, 20), (-4, 11), (0, 250), (-128, 127)):
                for open_ in (0, 1, 2, 3, 5, 11, 20, 60, 121, 122, 130):
                    for ext in (0, 1, 2, 3, 5, 11, 20):
                        for (m, n) in ((1, 1), (150, 150), (250, 250), (1000, 5000), (2000, 2000), (3000, 3000), (5000, 5000), (10000, 300), (12000, 12000), (30000, 30000)):
                            for cap in (8, 32, 104, 128):
                                rows = _geometry(lib, m, n, (cap - 2) // 2, *_SHAPE_OF_CAP[cap], 0)[0]     # what the launcher passes
                                want = bm.bias_and_low(mode, 0, m, n, open_, ext, smin, smax, (cap - 2) // 2, cap, rows, bool(ds))
                                b, l = C.c_int(0), C.c_int(0)
                                ok = lib.pmx_bstrip_window(mode, m, n, open_, ext, smin, smax, cap, rows, ds, C.byref(b), C.byref(l))
                                assert bool(ok) == (want is not None), (mode, ds, smin, smax, open_, ext, m, n, cap)
                                if want is not None:
                                    assert (b.value, l.value) == want, (mode, ds, smin, smax, open_, ext, m, n, cap, b.value, l.value, want)
                                    n_ok += 1
                                else:
                                    n_no += 1
    assert n_ok > 2000 and n_no > 2000, (n_ok, n_no)


@pytest.mark.parametrize("mode", [bm.NW, bm.SG, bm.SW])
def test_model_stays_inside_the_window_at_the_predicates_edge(orc, mode):
    """Scoring schemes the predicate only just admits (the next larger extension penalty or match score is rejected), on the
    inputs that stretch the value range: identical sequences (highest scores), no match at all (lowest), a long sequence against a
    one-letter one and bands far off the diagonal (longest boundary gaps), poly-A (every cell ties).  Every intermediate of the
    model is checked against the window (`check=True`), and the result against the banded oracle."""
    rng = np.random.default_rng(9900 + mode)
    tried = 0
    for L, k in ((120, 31), (90, 15), (200, 48), (60, 3)):
        cap = _cap_for(k)
        for double_skew in ((False,) if mode == bm.SW else (False, True)):
            for open_ in (2, 11, 60, 120):
                for mis in (-1, -4, -30):
                    # the largest match score / extension penalty the predicate admits for this shape
                    ext = 0
                    while ext + 1 <= open_ and bm.window_ok(mode, 15, L, L, open_, ext + 1, mis, 2, k, cap, L, double_skew):
                        ext += 1
                    match = 1
                    while bm.window_ok(mode, 15, L, L, open_, ext, mis, match + 1, k, cap, L, double_skew):
                        match += 1
                    if not bm.window_ok(mode, 15, L, L, open_, ext, mis, match, k, cap, L, double_skew):
                        continue
                    om = orc.Matrix.create("ACGT", match, mis)
                    mat = _mat5(om)
                    a = random_seqs(rng, 1, L, L)[0]
                    pairs = [(a, a, 0), (b"A" * L, b"C" * L, 0), (a, b"G", 0), (b"T", a, 3), (b"A" * L, b"A" * (L - 7), -2),
                             (a, mutate(rng, a, 0.2, 0.1), 1), (a, a[L // 2:], -(L // 2)), (a[L // 2:], a, L // 2), (a, a, k + L // 3)]
                    for sg in ((0, 5, 10, 15) if mode == bm.SG else (0,)):
                        B_LOW = bm.bias_and_low(mode, sg, L, L, open_, ext, mis, match, k, cap, L, double_skew)
                        for q, r, d in pairs:
                            qb, qo = orc.pack([q]); rb, ro = orc.pack([r])
                            want = orc.align_banded_batch(mode, qb, qo, rb, ro, open_, ext, om, k, np.array([d], dtype=np.int32), sg_flags=sg)[0]
                            got = bm.align(mode, sg, _idx(q), _idx(r), open_, ext, mat, k, d, cap, double_skew, B_LOW=B_LOW, check=True)
                            assert tuple(int(x) for x in got) == tuple(int(x) for x in want), (mode, sg, L, k, open_, ext, mis, match, d, got, want)
                            tried += 1
    assert tried > 300, tried


@pytest.mark.parametrize("band", [15, 31, 48])
def test_model_holds_the_window_when_the_query_outgrows_the_reference(pkg, orc, band):
    """Batches whose queries outgrow their references by the band's width or more (ql >= rl + 2 band) with centres in [-band, 0):
    their pairs run rows past the reference's last column, up to min(ql, rl + 2 band).  The model runs each pair with the bias / LOW
    the launcher derives for the whole batch -- bias_and_low at the batch's maxima and the launch-wide `rows` of
    pmx_bstrip_geometry -- every intermediate checked against the int16 window, and must match the banded oracle: global,
    every semi-global free-end set, local; both skews."""
    import ctypes as C_
    lib = pkg.lib
    g_, c_ = C_.c_int(0), C_.c_int(0)
    assert lib.pmx_bstrip_shape(band, C_.byref(g_), C_.byref(c_))
    G, C, cap = g_.value, c_.value, g_.value * c_.value
    rng = np.random.default_rng(9950 + band)
    om = orc.Matrix.create("ACGT", 2, -3)
    mat = _mat5(om)
    tried = 0
    for mode, sgs, skews in ((bm.NW, (0,), (False, True)), (bm.SG, range(1, 16), (False, True)), (bm.SW, (0,), (False,))):
        for sg in sgs:
            for double_skew in skews:
                # ext at the largest value the window admits for this batch (where an undercounted `rows` would matter), or 2
                qs, rs, dg = [], [], []
                for t in range(3):
                    rl = int(rng.integers(1, 40))
                    ql = rl + 2 * band + (0 if t == 0 else int(rng.integers(0, 40)))      # t == 0: the NW corner on the band's edge
                    d = -band if t < 2 else -int(rng.integers(1, band + 1))
                    q = random_seqs(rng, 1, ql, ql)[0]
                    r = mutate(rng, q[-d:-d + rl], 0.1, 0.03)[:rl] if rng.random() < 0.7 else random_seqs(rng, 1, rl, rl)[0]
                    r = (r + random_seqs(rng, 1, rl, rl)[0])[:rl]
                    qs.append(q); rs.append(r); dg.append(d)
                mq, mr = max(len(x) for x in qs), max(len(x) for x in rs)
                rows = _geometry(lib, mq, mr, band, G, C, 0)[0]
                assert rows == min(mq, mr + 2 * band)
                for open_, ext in ((5, 2), (11, None)):
                    if ext is None:
                        ext = 0
                        while ext + 1 <= open_ and bm.window_ok(mode, sg, mq, mr, open_, ext + 1, -3, 2, band, cap, rows, double_skew):
                            ext += 1
                    B_LOW = bm.bias_and_low(mode, sg, mq, mr, open_, ext, -3, 2, band, cap, rows, double_skew)
                    assert B_LOW is not None, (mode, sg, open_, ext, mq, mr, rows)
                    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
                    want = orc.align_banded_batch(mode, qb, qo, rb, ro, open_, ext, om, band, np.array(dg, dtype=np.int32), sg_flags=sg)
                    for t in range(len(qs)):
                        got = bm.align(mode, sg, _idx(qs[t]), _idx(rs[t]), open_, ext, mat, band, dg[t], cap, double_skew, B_LOW=B_LOW, check=True)
                        assert tuple(int(x) for x in got) == tuple(int(x) for x in want[t]), \
                            (mode, sg, double_skew, band, open_, ext, len(qs[t]), len(rs[t]), dg[t], got, want[t])
                        tried += 1
    assert tried >= 3 * 2 * 33, tried
