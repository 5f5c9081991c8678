"""The two statistics kernels at the edges of their host-side windows (`-m gpu`).

pmx_stats16p_kernel (two pairs per lane slot in int16 halves, admitted by pmx_nwsgv_bias without a row offset and by
max_qlen + max_rlen + 2 <= 32767) and pmx_stats16_kernel (u16 lanes biased by 32768, admitted by lo >= -15000, hi <= 15000 and
its LDS need) return six fields per pair as final: no promotion pass stands behind them.  tests/test_stats_window_model.py replays
the packed kernel's stored arithmetic on the CPU; whether the kernels themselves agree with the oracle where their windows end is
decided here:

  A. stats16p, shared profile (4 waves), the production road: shapes <16,10> <32,10> <64,10>, no switch;
  B. the same with free query / reference ends (PMX_STATS16P_ALWAYS): last-row / last-column captures and the combine key;
  C. stats16p, matrix-lookup form: per-pair BLOSUM62 queries, different pairs and lengths in the two halves of a slot;
  D. stats16p, per-pair profile planes: DNA, gap models with open == ext (every E / F tie live), lengths in the thousands;
  E. stats16: hi == 15000, lo == -15000 and one step over each, local with the best cell in the last row / column, every shape
     with its last row filled;
  F. stats16: the LDS fall-through from <16,10> to <32,8>.

References are the LONGEST each kernel (and shape) still takes -- found by launching, pmx_last_kernel() decides --, one short of it
and half of it.  Every case asserts the kernel and shape that ran, compares all six fields of every pair of the batch with the
oracle, exactly, and asserts that no record is flagged."""
import numpy as np
import pytest

from tests.util import AA, DNA, edge_lengths, families, golden, longest_by_launch, random_seqs, tile, window_hint

pytestmark = pytest.mark.gpu

QB, QE, DB, DE = 1, 2, 4, 8                                         # free-end bits (the oracle's S1_BEG, S1_END, S2_BEG, S2_END)
# (mode, free-end set): NW, every end free, the single-end sets and the two pairs of ends
MODES = [(0, 0), (1, 15), (1, 2), (1, 8), (1, 5), (1, 10)]
OPEN, EXT = 11, 1


def _kernel(pkg):
    return pkg.lib.pmx_last_kernel().decode()


def _aligner(pkg, orc, matrix, open_, ext, mode, sg, profile=None):
    """a statistics aligner: per-pair with use_stats(), or on a statistics profile"""
    b = pkg.Aligner.new().matrix(matrix).gap_open(open_).gap_extend(ext).solution_width(16)
    [b.global_, b.semi_global, b.local][mode]()
    if mode == 1:
        b.allow_query_gaps([t for f, t in ((orc.S1_BEG, "prefix"), (orc.S1_END, "suffix")) if sg & f])
        b.allow_ref_gaps([t for f, t in ((orc.S2_BEG, "prefix"), (orc.S2_END, "suffix")) if sg & f])
    if profile is not None:
        b.profile(profile)
    else:
        b.use_stats()
    return b.build()


def _oracle(orc, om, mode, sg, qs, rs, open_, ext, shared=None):
    """int32 [len(rs), 6]: score, end_query, end_ref, matches, similar, length of every distinct pair, in 32 bits"""
    rb, ro = orc.pack(rs)
    qb, qo = (None, None) if shared is not None else orc.pack(qs)
    w = orc.align_stats_sample(mode, np.arange(len(rs)), qb, qo, rb, ro, open_, ext, om, sg_flags=sg or orc.SG_ALL, bits=32, shared_query=shared)
    assert (w[:, 6] == 0).all()                                      # (nothing saturates in 32 bits)
    return w[:, :6]


def _six(rec, st):
    return np.stack([rec["score"], rec["end_query"], rec["end_ref"], st["matches"], st["similar"], st["length"]], axis=1)


def _same_everywhere(res, want, what):
    """all six fields of every pair of the batch (the distinct pairs tiled over it) equal the oracle's, none is flagged"""
    rec, st = res
    n = len(rec)
    full = want[np.arange(n) % len(want)]
    got = _six(rec, st)
    bad = np.nonzero((got != full).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:6], got[bad[:6]], full[bad[:6]])
    assert (rec["flags"] == 0).all(), what


def _b62(pkg, orc):
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))


def _p16_shape(qlen):
    return "pmx_stats16p_kernel<%d,10>" % (16 if qlen <= 160 else 32 if qlen <= 320 else 64)


# --------------------------------------------------------------------------------- A, B: stats16p on a shared profile ----
def _profile_edge(pkg, orc, qlen, modes, floor=0):
    """BLOSUM62 11/1, a statistics profile, 96 references (below the 512 of statistics-by-traceback): a poly-W query and a random
    one, each against the six reference families at the three lengths, every mode of `modes`"""
    rng = np.random.default_rng(7300 + qlen)
    pm, om = _b62(pkg, orc)
    n, name = 96, _p16_shape(qlen)
    for q in (b"W" * qlen, random_seqs(rng, 1, qlen, qlen, AA)[0]):
        prof = pkg.Profile.new(q, True, pm)
        als = {m: _aligner(pkg, orc, pm, OPEN, EXT, m[0], m[1], profile=prof) for m in modes + [(0, 0)]}

        def fast(rlen):
            als[(0, 0)].align_batch([], [b"W" * rlen] * 16)
            return _kernel(pkg) == name
        longest = longest_by_launch(fast, window_hint(pkg, qlen, 24, -4, 11, OPEN, EXT, rowx=0))
        print("stats16p shared profile %s, %d rows, query %s...: longest reference taken %d" % (name, qlen, q[:3].decode(), longest))
        assert longest >= floor, (longest, floor)
        assert longest + qlen + 2 <= 32767                           # (the window proof binds, not the length gate)
        lens = edge_lengths(longest)
        refs = [r for rlen in lens for r in families(rng, q, rlen)]
        for mode, sg in modes:
            want = _oracle(orc, om, mode, sg, None, refs, OPEN, EXT, shared=q)
            for li, rlen in enumerate(lens):
                res = als[(mode, sg)].align_batch([], tile(refs[6 * li:6 * li + 6], n))
                k = _kernel(pkg)
                assert k == name, (k, qlen, rlen, mode, sg)
                _same_everywhere(res, want[6 * li:6 * li + 6], (k, qlen, rlen, longest, mode, sg, q[:4]))


@pytest.mark.parametrize("qlen", [160, 161, 300, 320, 321, 640])
def test_stats16p_shared_profile_at_the_window_edge(pkg, orc, qlen):
    """A: the profile arm with statistics below 512 references, no switch set: NW and the begin-free sets the dispatcher sends to
    the packed kernel.  160 / 320 / 640 rows fill the last row of <16,10> <32,10> <64,10>, 161 / 321 are the first row past a
    shape; 300 rows is the flagship shape (BASELINE config 3: references of up to 5 000 letters must be taken)"""
    _profile_edge(pkg, orc, qlen, [(0, 0), (1, QB), (1, DB), (1, QB | DB)], floor=5000 if qlen == 300 else 1000)


@pytest.mark.parametrize("qlen", [160, 640])
def test_stats16p_shared_profile_free_ends_at_the_window_edge(pkg, orc, monkeypatch, qlen):
    """B: the free-end sets under PMX_STATS16P_ALWAYS -- the last-row and last-column captures (hv = xv - unsk) and the combine key
    (H + 16384, clamped below -16000) are live.  The clamp cannot be reached by an admitted batch: with a free query end the best
    last-column candidate is at least H(0, rlen - 1) >= -(open + rlen ext) + min (a gap along the row above, then one diagonal
    step), and the window proof (span < 31743 with hi >= 0) gives 2 rlen ext < 29695 - 5 open - |min| - (qlen + 134) ext, so
    open + rlen ext + |min| < 14848 + |min| / 2 - 1.5 open < 16000 as long as |min| < 2304 -- and |min| <= open <= 255 (a profile
    byte is score + open).  The coldest family ('*' throughout against a query-end-free set: the whole last column very negative)
    is the closest a batch comes; tests/test_stats_window_model.py counts the candidates below the clamp (none)."""
    monkeypatch.setenv("PMX_STATS16P_ALWAYS", "1")
    _profile_edge(pkg, orc, qlen, [(1, QE), (1, DE), (1, QE | DB), (1, QB | DE), (1, 15)], floor=1000)


# ------------------------------------------------------------------------------------------ C: stats16p, matrix lookup ----
@pytest.mark.parametrize("qlen", [160, 320, 640])
def test_stats16p_matrix_lookup_at_the_window_edge(pkg, orc, qlen):
    """C: per-pair BLOSUM62 queries, 24 distinct pairs per batch, no switch: poly-W and a random query, each against the six
    families, at two DIFFERENT lengths interleaved -- the two halves of a lane slot hold different pairs and different reference
    lengths (the shorter half runs pad columns past its end while the other still counts)"""
    rng = np.random.default_rng(7400 + qlen)
    pm, om = _b62(pkg, orc)
    name = _p16_shape(qlen) + "/matrix lookup"
    qw, q0 = b"W" * qlen, random_seqs(rng, 1, qlen, qlen, AA)[0]
    modes = [(0, 0), (1, DB), (1, QB | DB)]
    als = {m: _aligner(pkg, orc, pm, OPEN, EXT, m[0], m[1]) for m in modes}

    def fast(rlen):
        als[(0, 0)].align_batch([qw] * 24, [b"W" * rlen] * 24)
        return _kernel(pkg) == name
    longest = longest_by_launch(fast, window_hint(pkg, qlen, 24, -4, 11, OPEN, EXT, rowx=0))
    print("stats16p matrix lookup %s, %d rows: longest reference taken %d" % (name, qlen, longest))
    assert longest > 1000 and longest + qlen + 2 <= 32767, longest
    lens = edge_lengths(longest)
    byl = [[(q, r) for q in (qw, q0) for r in families(rng, q, rlen)] for rlen in lens]        # 12 pairs per length
    every = [p for b in byl for p in b]
    batches = [[12 * x + i for i in range(12) for x in (a, b)] for a, b in ((0, 2), (1, 0), (2, 1))]
    for mode, sg in modes:
        want = _oracle(orc, om, mode, sg, [p[0] for p in every], [p[1] for p in every], OPEN, EXT)
        for bi, idx in enumerate(batches):
            res = als[(mode, sg)].align_batch([every[i][0] for i in idx], [every[i][1] for i in idx])
            k = _kernel(pkg)
            assert k == name, (k, qlen, bi, mode, sg)
            _same_everywhere(res, want[idx], (k, qlen, longest, bi, mode, sg))


# --------------------------------------------------------------------------------- D: stats16p, per-pair profile planes ----
@pytest.mark.parametrize("scheme", [(2, -3, 5, 2), (2, -3, 3, 3), (1, -1, 1, 1)])
@pytest.mark.parametrize("qlen", [160, 320])
def test_stats16p_per_pair_planes_at_the_window_edge(pkg, orc, monkeypatch, qlen, scheme):
    """D: DNA, per-pair profile planes (PMX_STATS16P_ALWAYS, statistics by traceback off): open == ext makes every E / F tie live,
    and at the window's edge the lengths along those ties run to thousands.  (1/-1 under 1/1: a profile byte is score + open.)"""
    monkeypatch.setenv("PMX_STATS16P_ALWAYS", "1")
    monkeypatch.setenv("PMX_NO_STATS_BY_TRACE", "1")
    match, mis, open_, ext = scheme
    rng = np.random.default_rng(7500 + qlen + 7 * open_)
    pm, om = pkg.Matrix.create(b"ACGT", match, mis), orc.Matrix.create("ACGT", match, mis)
    n, name = 96, _p16_shape(qlen)
    qa, q0 = b"A" * qlen, random_seqs(rng, 1, qlen, qlen)[0]
    als = {m: _aligner(pkg, orc, pm, open_, ext, m[0], m[1]) for m in MODES}

    def fast(rlen):
        als[(0, 0)].align_batch([qa] * 16, [b"A" * rlen] * 16)
        return _kernel(pkg) == name
    longest = longest_by_launch(fast, window_hint(pkg, qlen, 5, min(mis, 0), match, open_, ext, rowx=0))
    print("stats16p per-pair planes %s, %d rows, %d/%d %d/%d: longest reference taken %d" % (name, qlen, match, mis, open_, ext, longest))
    assert longest > 1000 and longest + qlen + 2 <= 32767, longest
    lens = edge_lengths(longest)
    pairs = [(q, r) for rlen in lens for q in (qa, q0) for r in families(rng, q, rlen, DNA, b"A", b"C")]
    for mode, sg in MODES:
        want = _oracle(orc, om, mode, sg, [p[0] for p in pairs], [p[1] for p in pairs], open_, ext)
        for li, rlen in enumerate(lens):
            sl = slice(12 * li, 12 * li + 12)
            res = als[(mode, sg)].align_batch(tile([p[0] for p in pairs[sl]], n), tile([p[1] for p in pairs[sl]], n))
            k = _kernel(pkg)
            assert k == name, (k, qlen, rlen, mode, sg)
            _same_everywhere(res, want[sl], (k, scheme, qlen, rlen, longest, mode, sg))


# ------------------------------------------------------------------------------------------------ E: stats16's window ----
def _gen1(monkeypatch):
    monkeypatch.setenv("PMX_STATS16_GEN1", "1")
    monkeypatch.setenv("PMX_NO_STATS_BY_TRACE", "1")


def _stats16_window_hint(qlen, smin, open_, ext, local=False):
    """pmx_launch_stats16: max_rlen <= 30000, max_qlen + max_rlen <= 60000, lo = -(3 open + (q + r + 2) ext + |min|) >= -15000"""
    r = min(30000, 60000 - qlen)
    return r if local else min(r, (15000 - 3 * open_ - max(0, -smin)) // ext - qlen - 2)


def _stats16_lds_hint(G, R, shared, msize):
    """the longest reference whose LDS need (launch_stats in pmx_stats16.hip) stays within 160 KB"""
    NP = (64 // G) * (4 if shared else 1)
    fixed = (1 if shared else NP) * (msize + 1) * G * R * 6 + msize * msize * 2 + 256 + 8 + NP * 40
    return ((160 * 1024 - fixed) // NP) // 4 * 4 - 2 * G - 6


def _lo(qlen, rlen, smin, open_, ext):
    return -(3 * open_ + (qlen + rlen + 2) * ext + max(0, -smin))


def _stats16_edge(pkg, orc, monkeypatch, name, qlen, n, shared, match, mis, open_, ext, modes, lens_of=edge_lengths, seed=0):
    """pmx_stats16_kernel instance `name` at the longest reference it takes: a poly-A query and a random one (per pair), or the
    random one alone (shared), against the six families"""
    _gen1(monkeypatch)
    rng = np.random.default_rng(7600 + qlen + seed)
    pm, om = pkg.Matrix.create(b"ACGT", match, mis), orc.Matrix.create("ACGT", match, mis)
    q0 = random_seqs(rng, 1, qlen, qlen)[0]
    queries = [q0] if shared else [b"A" * qlen, q0]
    prof = pkg.Profile.new(q0, True, pm) if shared else None
    als = {m: _aligner(pkg, orc, pm, open_, ext, m[0], m[1], profile=prof) for m in set(modes) | {(0, 0)}}

    def run(al, pairs):
        return al.align_batch([], [p[1] for p in pairs]) if shared else al.align_batch([p[0] for p in pairs], [p[1] for p in pairs])

    def fast(rlen):
        run(als[(0, 0)], tile([(queries[0], b"A" * rlen)], min(n, 65 if n > 64 else n)))
        return _kernel(pkg) == name
    G, R = (int(x) for x in name[name.index("<") + 1:-1].split(","))
    longest = longest_by_launch(fast, min(_stats16_window_hint(qlen, mis, open_, ext), _stats16_lds_hint(G, R, shared, 5)))
    print("stats16 %s (%s, %d pairs), %d rows, %d/%d %d/%d: longest reference taken %d (lo %d, hi %d)"
          % (name, "shared" if shared else "per pair", n, qlen, match, mis, open_, ext, longest, _lo(qlen, longest, mis, open_, ext), min(qlen, longest) * match + match))
    assert longest > 1000, longest
    lens = lens_of(longest)
    per = 6 * len(queries)
    pairs = [(q, r) for rlen in lens for q in queries for r in families(rng, q, rlen, DNA, b"A", b"C")]
    for mode, sg in modes:
        want = _oracle(orc, om, mode, sg, [p[0] for p in pairs], [p[1] for p in pairs], open_, ext, shared=q0 if shared else None)
        for li, rlen in enumerate(lens):
            sl = slice(per * li, per * li + per)
            res = run(als[(mode, sg)], tile(pairs[sl], n))
            k = _kernel(pkg)
            assert k == name, (k, qlen, rlen, mode, sg)
            _same_everywhere(res, want[sl], (k, qlen, rlen, longest, mode, sg))
    return longest


@pytest.mark.parametrize("mode", MODES)
def test_stats16_hi_on_the_edge(pkg, orc, monkeypatch, mode):
    """E: 999 rows, match 15: hi = 999 * 15 + 15 == 15000, and the longest reference taken puts lo on -15000 as well (15/-4, 6/1:
    3 * 6 + (999 + 13977 + 2) + 4 == 15000).  Global and the semi-global sets; 12 pairs: the <64,16> shape of the small-batch arm"""
    longest = _stats16_edge(pkg, orc, monkeypatch, "pmx_stats16_kernel<64,16>", 999, 12, False, 15, -4, 6, 1, [mode])
    assert _lo(999, longest, -4, 6, 1) == -15000 and 999 * 15 + 15 == 15000, longest


def test_stats16_one_step_over_hi_is_not_taken(pkg, orc, monkeypatch):
    """E: 1000 rows, match 15 (hi == 15015) with references long enough to count: the kernel must decline, and what runs instead
    still equals the oracle"""
    _gen1(monkeypatch)
    rng = np.random.default_rng(7700)
    pm, om = pkg.Matrix.create(b"ACGT", 15, -4), orc.Matrix.create("ACGT", 15, -4)
    for qlen, taken in ((999, True), (1000, False)):
        qs = [b"A" * qlen, random_seqs(rng, 1, qlen, qlen)[0]]
        pairs = [(q, r) for q in qs for r in families(rng, q, 1500, DNA, b"A", b"C")]
        for mode, sg in ((0, 0), (1, 15)):
            res = _aligner(pkg, orc, pm, 6, 1, mode, sg).align_batch([p[0] for p in pairs], [p[1] for p in pairs])
            k = _kernel(pkg)
            assert ("pmx_stats16_kernel" in k) == taken, (k, qlen)
            _same_everywhere(res, _oracle(orc, om, mode, sg, [p[0] for p in pairs], [p[1] for p in pairs], 6, 1), (k, qlen, mode, sg))


@pytest.mark.parametrize("mode", MODES)
def test_stats16_lo_on_the_edge(pkg, orc, monkeypatch, mode):
    """E: 160 rows, 2/-3 under 5/2: 3 * 5 + (160 + 7329 + 2) * 2 + 3 == 15000 -- the longest reference taken must be exactly the
    one that puts lo on -15000 (one letter more: declined, which the search by launching has seen).  96 pairs: <16,10>"""
    longest = _stats16_edge(pkg, orc, monkeypatch, "pmx_stats16_kernel<16,10>", 160, 96, False, 2, -3, 5, 2, [mode])
    assert longest == 7329 and _lo(160, longest, -3, 5, 2) == -15000, longest


def test_stats16_local_best_in_the_last_row_and_column(pkg, orc, monkeypatch):
    """E: local, 999 rows, match 15 (hi == 15000), references up to the 30 000 letters the kernel takes: the query's copy ends
    in the last column (best cell in the last row AND the last column: 999 * 15 = 14985 of 15000), in the last row only (a
    suffix follows), in the last column only (the query carries a foreign tail)"""
    _gen1(monkeypatch)
    rng = np.random.default_rng(7800)
    pm, om = pkg.Matrix.create(b"ACGT", 15, -15), orc.Matrix.create("ACGT", 15, -15)
    al = _aligner(pkg, orc, pm, 16, 4, 2, 0)
    name = "pmx_stats16_kernel<64,16>"
    q0 = random_seqs(rng, 1, 999, 999)[0]
    qtail = q0[:900] + bytes(b"ACGT"[(b"ACGT".index(c) + 1) % 4] for c in q0[900:])      # (no letter of the tail matches q0's)

    def fast(rlen):
        al.align_batch([q0] * 3, [b"A" * rlen] * 3)
        return _kernel(pkg) == name
    longest = longest_by_launch(fast, _stats16_window_hint(999, -15, 16, 4, local=True))
    print("stats16 local %s, 999 rows, 15/-15 16/4: longest reference taken %d" % (name, longest))
    assert longest > 1000, longest
    for rlen in edge_lengths(longest):
        far = random_seqs(rng, 1, rlen, rlen)[0]
        pairs = [(q0, far[:rlen - 999] + q0), (q0, far[:rlen - 1499] + q0 + far[-500:]), (qtail, far[:rlen - 900] + q0[:900]), (b"A" * 999, b"A" * rlen)]
        want = _oracle(orc, om, 2, 0, [p[0] for p in pairs], [p[1] for p in pairs], 16, 4)
        assert tuple(want[0, :3]) == (14985, 998, rlen - 1) and want[1, 1] == 998 and want[1, 2] == rlen - 501 and tuple(want[2, 1:3]) == (899, rlen - 1), want[:, :3]
        res = al.align_batch([p[0] for p in pairs], [p[1] for p in pairs])
        k = _kernel(pkg)
        assert k == name, (k, rlen)
        _same_everywhere(res, want, (k, rlen, longest))


# (shape, rows, pairs in the batch, shared query): every instance of the ladder with its last row filled.  Up to 64 per-pair
# queries take the <64,3> / <64,5> arm; a shared query runs the 4-wave instances.
STATS16_SHAPES = [("<64,3>", 192, 12, False), ("<64,5>", 320, 12, False),
                  ("<16,10>", 160, 96, False), ("<32,8>", 256, 96, False), ("<64,5>", 320, 96, False), ("<64,8>", 512, 96, False), ("<64,16>", 1024, 96, False),
                  ("<16,10>", 160, 96, True), ("<32,8>", 256, 96, True), ("<64,5>", 320, 96, True), ("<64,8>", 512, 96, True), ("<64,16>", 1024, 96, True)]


@pytest.mark.parametrize("case", range(len(STATS16_SHAPES)))
def test_stats16_every_shape_with_its_last_row_filled(pkg, orc, monkeypatch, case):
    """E: every <G,R> instance, per pair and on a shared query, G * R rows, the largest match score that keeps hi <= 15000
    (15000 // (rows + 1)), at the longest reference the instance takes (the window, or for the 4-wave <16,10> its LDS) and one
    short of it: NW and two free-end sets, rotating over the cases"""
    shape, qlen, n, shared = STATS16_SHAPES[case]
    match = 15000 // (qlen + 1)
    sets = [(1, 15), (1, 2), (1, 8), (1, 5), (1, 10), (1, 9), (1, 6)]
    modes = [(0, 0), sets[(2 * case) % 7], sets[(2 * case + 1) % 7]]
    _stats16_edge(pkg, orc, monkeypatch, "pmx_stats16_kernel" + shape, qlen, n, shared, match, -4, 6, 1, modes,
                  lens_of=lambda longest: [longest, longest - 1], seed=case)


# --------------------------------------------------------------------------------------- F: stats16's LDS fall-through ----
@pytest.mark.parametrize("form", ["shared", "per pair"])
def test_stats16_lds_fall_through(pkg, orc, monkeypatch, form):
    """F: 150-row queries against references so long that <16,10> no longer fits 160 KB of LDS and <32,8> runs: the last length
    of one shape and the first of the next, NW / SG / SW, the shape name changing between the two.  Shared: a DNA query, the
    4-wave instance (16 pairs' symbols per workgroup); per pair: a 30-letter alphabet (4 profiles of 31 x 160 entries)"""
    _gen1(monkeypatch)
    rng = np.random.default_rng(7900 + len(form))
    shared = form == "shared"
    letters = b"ACGT" if shared else b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123"
    alphabet = np.frombuffer(letters, dtype=np.uint8)
    pm, om = pkg.Matrix.create(letters, 2, -3), orc.Matrix.create(letters.decode(), 2, -3)
    qlen, n = 150, 96
    q0 = random_seqs(rng, 1, qlen, qlen, alphabet)[0]
    queries = [q0] if shared else [letters[:1] * qlen, q0]
    prof = pkg.Profile.new(q0, True, pm) if shared else None
    modes = [(0, 0), (1, 15), (2, 0)]
    als = {m: _aligner(pkg, orc, pm, 5, 1, m[0], m[1], profile=prof) for m in modes}

    def run(al, pairs):
        return al.align_batch([], [p[1] for p in pairs]) if shared else al.align_batch([p[0] for p in pairs], [p[1] for p in pairs])

    for mode, sg in modes:
        def fast(rlen):
            run(als[(mode, sg)], tile([(queries[0], letters[:1] * rlen)], 65))
            return _kernel(pkg) == "pmx_stats16_kernel<16,10>"
        last = longest_by_launch(fast, _stats16_lds_hint(16, 10, shared, len(letters) + 1))
        print("stats16 LDS fall-through (%s, mode %d/%d): <16,10> takes references up to %d" % (form, mode, sg, last))
        assert 5000 < last < _stats16_window_hint(qlen, -3, 5, 1, local=mode == 2), last
        names = []
        for rlen in (last, last + 1):
            pairs = [(q, r) for q in queries for r in families(rng, q, rlen, alphabet, letters[:1], letters[1:2])]
            want = _oracle(orc, om, mode, sg, [p[0] for p in pairs], [p[1] for p in pairs], 5, 1, shared=q0 if shared else None)
            res = run(als[(mode, sg)], tile(pairs, n))
            names.append(_kernel(pkg))
            _same_everywhere(res, want, (names[-1], form, rlen, mode, sg))
        assert names == ["pmx_stats16_kernel<16,10>", "pmx_stats16_kernel<32,8>"], names
