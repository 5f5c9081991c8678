"""The packed global / semi-global kernels at the edges of their two host-side proofs (`-m gpu`).

pmx_nwsg16.hip has no promotion pass: what pmx_nwsgv_bias admits is computed in biased int16 and returned as final, and the
traceback instances that merge a decision with one v_bfi_b32 rely on max(matrix max, 0) + 2 open <= 250.  tests/test_window_models.py
replays the stored arithmetic of pmx_nwsg16v_kernel on the CPU; whether the shared-profile kernel (pmx_nwsg16q_kernel, symbol and
PSSM forms), the matrix-lookup kernel (pmx_nwsg16m_kernel) and every traceback instance agree is decided here:

  A. scores at the LONGEST reference each kernel still takes (found by launching), one short of it and at half of it;
  B. the same edge through the trace-writing instances: CIGAR text and statistics by traceback;
  C. the bounded-difference gate at max + 2 open == 250 (one-instruction merge, byte-identical to the shift form) and at 251.

Every case asserts the kernel that ran (pmx_last_kernel() names the decision form of the trace roads), every pair of every batch
is compared, and every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from tests.pssm_oracle import check, encode
from tests.util import AA, B62_LETTERS, consensus_pssm, edge_lengths, families, golden, longest_by_launch, mutate, random_seqs, tile, window_hint

pytestmark = pytest.mark.gpu

# (mode, free-end set): NW, every end free, the single-end sets and the two pairs of ends
MODES = [(0, 0), (1, 15), (1, 2), (1, 8), (1, 5), (1, 10)]
OPEN, EXT = 11, 1


def _kernel(pkg):
    return pkg.lib.pmx_last_kernel().decode()


def _aligner(pkg, orc, matrix, open_, ext, mode, sg, profile=None, stats=False, trace=False):
    b = pkg.Aligner.new().matrix(matrix).gap_open(open_).gap_extend(ext).solution_width(16)
    [b.global_, b.semi_global][mode]()
    if mode == 1:
        b.allow_query_gaps([t for f, t in ((orc.S1_BEG, "prefix"), (orc.S1_END, "suffix")) if sg & f])
        b.allow_ref_gaps([t for f, t in ((orc.S2_BEG, "prefix"), (orc.S2_END, "suffix")) if sg & f])
    if profile is not None:
        b.profile(profile)
    elif stats:
        b.use_stats()
    if trace:
        b.use_trace()
    return b.build()


def _hook(pkg, qlen, rlen, msize, smin, smax, open_, ext, rows=0):
    pkg.lib.pmx_window_nwsgv.restype = C.c_int
    return pkg.lib.pmx_window_nwsgv(int(qlen), int(rlen), int(msize), int(smin), int(smax), int(open_), int(ext), 1, int(rows))


def _hint(pkg, qlen, msize, smin, smax, open_, ext):
    """the window hook's longest reference (row-offset form): where the search by launching looks first"""
    return window_hint(pkg, qlen, msize, smin, smax, open_, ext, rowx=1)


# (shared with tests/test_gpu_stats_window_edges.py: they live in tests/util.py)
_longest_by_launch, _families, _tile = longest_by_launch, families, tile


def _records(got):
    return np.stack([got["score"], got["end_query"], got["end_ref"]], axis=1)


def _stats(st):
    return np.stack([st["matches"], st["similar"], st["length"]], axis=1)


def _same_everywhere(got, want, n, what):
    """every record of the batch (the distinct pairs tiled n times over) equals the oracle's, none is flagged"""
    full = want[np.arange(n) % len(want)]
    bad = np.nonzero((_records(got) != full[:, :3]).any(axis=1))[0]
    assert len(bad) == 0, (what, bad[:6], _records(got)[bad[:6]], full[bad[:6], :3])
    assert (got["flags"] == 0).all(), what


def _b62(pkg, orc):
    return pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))


_lengths = edge_lengths


# ------------------------------------------------------------------------------------------------------------- A: scores ----
@pytest.mark.parametrize("form", ["symbol", "to_pssm"])
@pytest.mark.parametrize("qlen", [50, 300, 1000, 2048])
def test_profile_scores_at_the_window_edge(pkg, orc, qlen, form):
    """pmx_nwsg16q_kernel (symbol form and the PSSM form on to_pssm of the same query), BLOSUM62 11/1, 520 pairs, shapes <16,10>
    <32,10> <64,16> <64,32>: a poly-W query and a random one, each against the six reference families, every mode"""
    rng = np.random.default_rng(6100 + qlen)
    pm, om = _b62(pkg, orc)
    n = 520
    for q in (b"W" * qlen, random_seqs(rng, 1, qlen, qlen, AA)[0]):
        matrix = pm if form == "symbol" else pm.to_pssm(q)
        vals = matrix.to_numpy()
        prof = pkg.Profile.new(q, False, matrix)
        als = {m: _aligner(pkg, orc, matrix, OPEN, EXT, m[0], m[1], profile=prof) for m in MODES}

        def ran(k):
            return "pmx_nwsg16q_kernel" in k and "shared" in k and (("pssm" in k) == (form == "to_pssm"))

        def fast(rlen):                                              # (the profile road does not look at the number of pairs: a
            als[(0, 0)].align_batch([], [b"W" * rlen] * 16)          #  small probe keeps the one launch beyond the window cheap)
            return ran(_kernel(pkg))
        longest = _longest_by_launch(fast, _hint(pkg, qlen, 24, vals.min(), vals.max(), OPEN, EXT))
        assert longest > 1000, longest                               # (300 rows: about 25.8 k)
        print("nwsg16q scores, %s, %d rows, query %s...: longest reference taken %d" % (form, qlen, q[:3].decode(), longest))
        lens = _lengths(longest)
        refs = [r for rlen in lens for r in _families(rng, q, rlen)]
        qb, qo = orc.pack([q] * len(refs)); rb, ro = orc.pack(refs)
        for mode, sg in MODES:
            want = orc.align_batch(mode, qb, qo, rb, ro, OPEN, EXT, om, sg_flags=sg or orc.SG_ALL, bits=32)
            for li, rlen in enumerate(lens):
                got = als[(mode, sg)].align_batch([], _tile(refs[6 * li:6 * li + 6], n))
                k = _kernel(pkg)
                assert ran(k), (k, qlen, rlen, mode, sg)
                _same_everywhere(got, want[6 * li:6 * li + 6], n, (k, qlen, rlen, longest, mode, sg, q[:4]))


@pytest.mark.parametrize("case", ["A", "B"])
def test_consensus_pssm_scores_at_the_window_edge(pkg, orc, case):
    """the PSSM form of pmx_nwsg16q_kernel on a 200-row PSSM whose every row holds its top value in its consensus column --
    A: top 255 - open - ext and -open under '*' (the byte range of the profile, the steepest climb), B: mild (-6 .. 9), long
    references -- against the byte-encoded PSSM checker's matrix"""
    rng = np.random.default_rng(6200 + ord(case))
    L, n = 200, 520
    top, bottom = (255 - OPEN - EXT, -OPEN) if case == "A" else (9, -6)
    vals, cons, _ = consensus_pssm(rng, L, top, bottom)
    ps = pkg.Matrix.create_pssm(B62_LETTERS.decode(), [int(v) for v in vals.ravel()], L)
    q = random_seqs(rng, 1, L, L, AA)[0]
    om, qcode = encode(orc, vals, np.asarray(ps.mapper()), B62_LETTERS)
    prof = pkg.Profile.new(q, False, ps)
    als = {m: _aligner(pkg, orc, ps, OPEN, EXT, m[0], m[1], profile=prof) for m in MODES}

    def ran(k):
        return "pmx_nwsg16q_kernel" in k and "pssm" in k

    def fast(rlen):
        als[(0, 0)].align_batch([], [cons[:1] * rlen] * 16)
        return ran(_kernel(pkg))
    longest = _longest_by_launch(fast, _hint(pkg, L, 24, vals.min(), vals.max(), OPEN, EXT))
    print("nwsg16q scores, consensus PSSM %s (top %d): longest reference taken %d" % (case, top, longest))
    lens = _lengths(longest)
    refs = [r for rlen in lens for r in _families(rng, cons, rlen)]
    qb, qo = orc.pack([qcode] * len(refs)); rb, ro = orc.pack(refs)
    for mode, sg in MODES:
        want = orc.align_batch(mode, qb, qo, rb, ro, OPEN, EXT, om, sg_flags=sg or orc.SG_ALL, bits=32)
        for li, rlen in enumerate(lens):
            got = als[(mode, sg)].align_batch([], _tile(refs[6 * li:6 * li + 6], n))
            k = _kernel(pkg)
            assert ran(k), (k, rlen, mode, sg)
            _same_everywhere(got, want[6 * li:6 * li + 6], n, (k, case, rlen, longest, mode, sg))


@pytest.mark.parametrize("qlen", [50, 300, 1000])
def test_matrix_lookup_scores_at_the_window_edge(pkg, orc, qlen):
    """pmx_nwsg16m_kernel: per-pair BLOSUM62 batches of more than 2 048 pairs, shapes <16,10> <32,10> <64,16>; poly-W and a
    random query, each against the six reference families, in ONE batch"""
    rng = np.random.default_rng(6300 + qlen)
    pm, om = _b62(pkg, orc)
    n = 2064
    qw, q0 = b"W" * qlen, random_seqs(rng, 1, qlen, qlen, AA)[0]
    als = {m: _aligner(pkg, orc, pm, OPEN, EXT, m[0], m[1]) for m in MODES}

    def fast(rlen):
        als[(0, 0)].align_batch([qw] * n, [b"W" * rlen] * n)
        return "pmx_nwsg16m_kernel" in _kernel(pkg)
    longest = _longest_by_launch(fast, _hint(pkg, qlen, 24, -4, 11, OPEN, EXT))
    assert longest > 1000, longest
    print("nwsg16m scores, %d rows: longest reference taken %d" % (qlen, longest))
    lens = _lengths(longest)
    qs = ([qw] * 6 + [q0] * 6) * len(lens)
    refs = [r for rlen in lens for q in (qw, q0) for r in _families(rng, q, rlen)]
    qb, qo = orc.pack(qs); rb, ro = orc.pack(refs)
    for mode, sg in MODES:
        want = orc.align_batch(mode, qb, qo, rb, ro, OPEN, EXT, om, sg_flags=sg or orc.SG_ALL, bits=32)
        for li, rlen in enumerate(lens):
            sl = slice(12 * li, 12 * li + 12)
            got = als[(mode, sg)].align_batch(_tile(qs[sl], n), _tile(refs[sl], n))
            k = _kernel(pkg)
            assert "pmx_nwsg16m_kernel" in k, (k, qlen, rlen, mode, sg)
            _same_everywhere(got, want[sl], n, (k, qlen, rlen, longest, mode, sg))


# ----------------------------------------------------------------------------------------------------- B: trace instances ----
def _cigar_edge(pkg, orc, pm, om, open_, ext, qs, alphabet, hot, cold, n, name, rng):
    """align_batch_cigar at the longest reference the packed traceback sweep `name` still takes and one short of it: every
    record and every CIGAR text of the batch against the oracle's"""
    als = {m: _aligner(pkg, orc, pm, open_, ext, m[0], m[1], trace=True) for m in MODES}

    def fast(rlen):
        als[(0, 0)].align_batch_cigar(_tile(qs, n), [hot * rlen] * n)
        return name in _kernel(pkg)
    longest = _longest_by_launch(fast)
    assert longest > 1000, longest
    print("%s: longest reference taken %d" % (name, longest))
    for rlen in (longest, longest - 1):
        # one query per family, each family built from the query it is paired with (the ragged lengths stay through the members);
        # the hottest letter throughout meets itself (family 0) and the coldest letter (family 4)
        pq = [qs[i % len(qs)] for i in range(6)]
        pq[0], pq[4] = hot * len(pq[0]), hot * len(pq[4])
        fam = [_families(rng, pq[i], rlen, alphabet, hot, cold)[i] for i in range(6)]
        assert fam[1].startswith(pq[1]) and fam[2].endswith(pq[2]) and fam[3].startswith(pq[3])
        qb, qo = orc.pack(pq); rb, ro = orc.pack(fam)
        for mode, sg in MODES:
            text, want = orc.cigar_sample(mode, np.arange(len(fam)), qb, qo, rb, ro, open_, ext, om, sg_flags=sg or orc.SG_ALL)
            got, cig = als[(mode, sg)].align_batch_cigar(_tile(pq, n), _tile(fam, n))
            k = _kernel(pkg)
            assert name in k and "pmx_walkp_kernel" in k, (k, rlen, mode, sg)
            _same_everywhere(got, want, n, (k, rlen, longest, mode, sg))
            bad = [i for i in range(n) if cig[i] != text[i % len(fam)]]
            assert not bad, (k, rlen, mode, sg, bad[:4], cig[bad[0]][:80], text[bad[0] % len(fam)][:80])
    return longest


@pytest.mark.parametrize("form", ["equal", "ragged"])
def test_dna_cigar_at_the_window_edge(pkg, orc, form):
    """nwsg16v<TR> + pmx_walkp through align_batch_cigar, 2/-3 5/2 (max + 2 open = 12: the one-instruction merge): equal-length
    reads of 200 bp (the perm-table form, top-aligned) and ragged reads of 20 .. 100 bp (LDS profiles, bottom-aligned)"""
    rng = np.random.default_rng(6400)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    qs = random_seqs(rng, 6, 200, 200) if form == "equal" else [random_seqs(rng, 1, L, L)[0] for L in (100, 20, 57, 99, 33, 100)]
    name = "pmx_nwsg16v_kernel/packed trace/bfi" + ("/permtable" if form == "equal" else "")
    _cigar_edge(pkg, orc, pm, om, 5, 2, qs, np.frombuffer(b"ACGT", dtype=np.uint8), b"A", b"C", 96, name, rng)


def test_protein_cigar_at_the_window_edge(pkg, orc):
    """nwsg16m<TR> + pmx_walkp through align_batch_cigar: per-pair BLOSUM62 11/1, ragged queries up to 255 rows"""
    rng = np.random.default_rng(6500)
    pm, om = _b62(pkg, orc)
    qs = [random_seqs(rng, 1, L, L, AA)[0] for L in (255, 40, 131, 255, 200, 77)]
    _cigar_edge(pkg, orc, pm, om, OPEN, EXT, qs, AA, b"W", b"*", 96, "pmx_nwsg16m_kernel/packed trace/shift", rng)


@pytest.mark.parametrize("form", ["symbol", "to_pssm"])
@pytest.mark.parametrize("qlen", [300, 319, 1000])
def test_profile_statistics_at_the_window_edge(pkg, orc, qlen, form):
    """nwsg16q<TR> (symbol and PSSM forms, shapes <16,19> <16,20> <64,16>) + pmx_walkp counting along the path: BLOSUM62 11/1
    profile batches with statistics at the longest reference the traceback sweep takes and one short of it"""
    rng = np.random.default_rng(6600 + qlen)
    pm, om = _b62(pkg, orc)
    n = 520
    q = random_seqs(rng, 1, qlen, qlen, AA)[0]
    matrix = pm if form == "symbol" else pm.to_pssm(q)
    prof = pkg.Profile.new(q, True, matrix)
    als = {m: _aligner(pkg, orc, matrix, OPEN, EXT, m[0], m[1], profile=prof) for m in MODES}

    def ran(k):
        return "pmx_nwsg16q_kernel" in k and "packed trace/bfi" in k and "pmx_walkp_kernel" in k and (("pssm" in k) == (form == "to_pssm"))

    def fast(rlen):
        als[(0, 0)].align_batch([], [b"W" * rlen] * n)
        return ran(_kernel(pkg))
    vals = matrix.to_numpy()
    longest = _longest_by_launch(fast, _hint(pkg, qlen, 24, vals.min(), vals.max(), OPEN, EXT))
    assert longest > 2000, longest
    print("nwsg16q<TR> statistics, %s, %d rows: longest reference taken %d" % (form, qlen, longest))
    lens = [longest, longest - 1]
    refs = [r for rlen in lens for r in _families(rng, q, rlen)]
    rb, ro = orc.pack(refs)
    for mode, sg in MODES:
        want = orc.align_stats_sample(mode, np.arange(len(refs)), None, None, rb, ro, OPEN, EXT, om, sg_flags=sg or orc.SG_ALL, bits=32, shared_query=q)
        for li, rlen in enumerate(lens):
            got, st = als[(mode, sg)].align_batch([], _tile(refs[6 * li:6 * li + 6], n))
            k = _kernel(pkg)
            assert ran(k), (k, qlen, rlen, mode, sg)
            w = want[6 * li:6 * li + 6]
            _same_everywhere(got, w, n, (k, qlen, rlen, longest, mode, sg))
            full = w[np.arange(n) % 6]
            bad = np.nonzero((_stats(st) != full[:, 3:6]).any(axis=1))[0]
            assert len(bad) == 0, (k, qlen, rlen, mode, sg, bad[:6], _stats(st)[bad[:6]], full[bad[:6], 3:6])


@pytest.mark.parametrize("case", ["A", "B"])
def test_consensus_pssm_statistics_at_the_window_edge(pkg, orc, case):
    """the PSSM form of nwsg16q<TR> + pmx_walkp<pssm> on the consensus PSSMs of the score test: records and statistics against
    the byte-encoded PSSM checker"""
    rng = np.random.default_rng(6700 + ord(case))
    L, n = 200, 520
    top, bottom = (250 - 2 * OPEN, -OPEN) if case == "A" else (9, -6)       # (A: the largest top the traceback sweep's gate admits)
    vals, cons, _ = consensus_pssm(rng, L, top, bottom)
    ps = pkg.Matrix.create_pssm(B62_LETTERS.decode(), [int(v) for v in vals.ravel()], L)
    q = random_seqs(rng, 1, L, L, AA)[0]
    prof = pkg.Profile.new(q, True, ps)
    als = {m: _aligner(pkg, orc, ps, OPEN, EXT, m[0], m[1], profile=prof) for m in MODES}

    def ran(k):
        return "pmx_nwsg16q_kernel" in k and "pssm" in k and "packed trace/bfi" in k and "pmx_walkp_kernel<pssm>" in k

    def fast(rlen):
        als[(0, 0)].align_batch([], [cons[:1] * rlen] * n)
        return ran(_kernel(pkg))
    longest = _longest_by_launch(fast, _hint(pkg, L, 24, vals.min(), vals.max(), OPEN, EXT))
    print("nwsg16q<TR> statistics, consensus PSSM %s (top %d): longest reference taken %d" % (case, top, longest))
    for rlen in (longest, max(1, longest - 1)):
        refs = _families(rng, cons, rlen)
        for mode, sg in MODES:
            want, _ = check(orc, mode, sg or orc.SG_ALL, vals, np.asarray(ps.mapper()), B62_LETTERS, [q] * 6, refs, OPEN, EXT, with_cigar=False)
            got, st = als[(mode, sg)].align_batch([], _tile(refs, n))
            k = _kernel(pkg)
            assert ran(k), (k, rlen, mode, sg)
            _same_everywhere(got, want, n, (k, case, rlen, longest, mode, sg))
            full = want[np.arange(n) % 6]
            bad = np.nonzero((_stats(st) != full[:, 3:6]).any(axis=1))[0]
            assert len(bad) == 0, (k, case, rlen, mode, sg, bad[:6], _stats(st)[bad[:6]], full[bad[:6], 3:6])


# ------------------------------------------------------------------------------------------- C: the bounded-difference gate ----
# (match, mismatch, open) with max + 2 open == 250
GATE_SCHEMES = [(110, -70, 70), (40, -105, 105), (248, -1, 1), (228, -11, 11), (250, 0, 0)]
FREE_ENDS = [(1, 15), (1, 5), (1, 10), (1, 2), (1, 8)]


# the ext values (of 0, 1, open / 2, open) the window proof admits for the gate batches below, by open: their pairs are 100 to 200
# letters long, and with open = 70 or 105 the skew growth of ext = open / 2 alone, (rlen + rows + 132) * ext, passes the int16
# window (tests/test_window_models.py runs those ext values on shorter pairs); 11/11 fails the capture bound next to max = 228
GATE_EXTS_ADMITTED = {70: [0, 1], 105: [0, 1], 1: [0, 1], 11: [0, 1, 5], 0: [0]}


def _gate_exts(open_):
    return sorted({0, 1, open_ // 2, open_} & set(range(open_ + 1)))


def _gate_cap(smax):
    """The window proof bounds the highest score, min(qlen, rlen) * max, by the int16 window (31 743 less bias, skew growth and
    capture bias): a scheme with max near 250 is admitted only while the shorter side of a pair stays near 100 letters.  The
    shorter side of every gate batch is capped here; the hook then has to admit ext = 0 and 1."""
    return max(8, min(200, 24000 // max(1, smax)))


def _gate_modes(i):
    """NW and two free-end sets, rotating so that every set comes up across the schemes and ext values"""
    return [(0, 0), FREE_ENDS[(2 * i) % 5], FREE_ENDS[(2 * i + 1) % 5]]


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("scheme", GATE_SCHEMES)
def test_gate_per_pair_cigar(pkg, orc, monkeypatch, scheme, over):
    """pmx_nwsg16v_kernel<TR>: at max + 2 open == 250 the one-instruction merge runs (ragged reads: LDS profiles, bottom-aligned;
    equal-length reads: the perm-table form, top-aligned) and its records and text are the oracle's and byte-identical to the
    three-instruction merge's (PMX_TRACE_NO_BFI); at 251 the launcher reports the shift form, same results"""
    match, mis, open_ = scheme
    match += over
    rng = np.random.default_rng(6800 + match + open_)
    pm, om = pkg.Matrix.create(b"ACGT", match, mis), orc.Matrix.create("ACGT", match, mis)
    smin, smax = int(om.scores[:5, :5].min()), int(om.scores[:5, :5].max())
    cap = _gate_cap(smax)
    for form, rows in (("ragged", 128), ("equal", 256)):
        if form == "ragged":
            qs = random_seqs(rng, 300, 1, min(120, cap))
            rs = [mutate(rng, q, 0.12, 0.06)[:150] if i % 4 else random_seqs(rng, 1, 1, 150)[0] for i, q in enumerate(qs)]
        else:
            qs = random_seqs(rng, 2100, 200, 200)
            rs = [(mutate(rng, q[i % 50:], 0.1, 0.03) + q)[:min(210, cap)] for i, q in enumerate(qs)]
        n = len(qs)
        qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
        mq, mr = max(map(len, qs)), max(map(len, rs))
        exts = [e for e in _gate_exts(open_) if _hook(pkg, mq, mr, 5, smin, smax, open_, e) and _hook(pkg, mq, mr, 5, smin, smax, open_, e, rows)]
        assert exts == GATE_EXTS_ADMITTED[open_], (scheme, form, exts)      # (coverage cannot shrink unnoticed)
        for i, ext in enumerate(exts):
            for mode, sg in _gate_modes(i):
                al = _aligner(pkg, orc, pm, open_, ext, mode, sg, trace=True)
                rec, text, coff = al.align_batch_cigar_packed(qb, qo, rb, ro)
                k = _kernel(pkg)
                if over == 0:
                    assert "pmx_nwsg16v_kernel/packed trace/bfi" in k and (("permtable" in k) == (form == "equal")), (k, scheme, form, ext)
                    monkeypatch.setenv("PMX_TRACE_NO_BFI", "1")
                    rec2, text2, coff2 = al.align_batch_cigar_packed(qb, qo, rb, ro)
                    k2 = _kernel(pkg)
                    monkeypatch.delenv("PMX_TRACE_NO_BFI")
                    assert "pmx_nwsg16v_kernel/packed trace/shift" in k2, k2
                    assert (_records(rec) == _records(rec2)).all() and (rec["flags"] == rec2["flags"]).all() and (coff == coff2).all() and \
                        text.tobytes() == text2.tobytes(), (scheme, form, ext, mode, sg)
                else:
                    assert "pmx_nwsg16v_kernel/packed trace/shift" in k, (k, scheme, form, ext)
                want_text, want = orc.cigar_sample(mode, np.arange(n), qb, qo, rb, ro, open_, ext, om, sg_flags=sg or orc.SG_ALL)
                bad = np.nonzero((_records(rec) != want[:, :3]).any(axis=1))[0]
                assert len(bad) == 0, (k, scheme, over, form, ext, mode, sg, bad[:5], _records(rec)[bad[:5]], want[bad[:5], :3])
                raw = text.tobytes()
                badc = [j for j in range(n) if raw[coff[j]:coff[j + 1]].decode() != want_text[j]]
                assert not badc, (k, scheme, over, form, ext, mode, sg, badc[:4], qs[badc[0]], rs[badc[0]], raw[coff[badc[0]]:coff[badc[0] + 1]], want_text[badc[0]])


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("kind", ["symbol", "pssm"])
@pytest.mark.parametrize("scheme", GATE_SCHEMES)
def test_gate_profile_statistics(pkg, orc, monkeypatch, scheme, kind, over):
    """nwsg16q<TR> + pmx_walkp (every traceback instance of the shared-profile kernel merges with v_bfi_b32): a 4-letter symbol
    matrix and a PSSM with top 250 - 2 open and bottom -open.  At 250 the traceback sweep runs and equals the oracle (and the
    same call under PMX_TRACE_NO_BFI, which this kernel does not read); at 251 it has declined and the results still equal"""
    match, mis, open_ = scheme
    rng = np.random.default_rng(6900 + match + open_)
    L, n = 150, 520
    if kind == "symbol":
        pm, om = pkg.Matrix.create(b"ACGT", match + over, mis), orc.Matrix.create("ACGT", match + over, mis)
        smin, smax, msize = int(om.scores[:5, :5].min()), int(om.scores[:5, :5].max()), 5
        cap = _gate_cap(smax)
        q = random_seqs(rng, 1, L, L)[0]
        rs = [mutate(rng, q[i % 60:], 0.12, 0.06)[:cap] if i % 4 else random_seqs(rng, 1, 1, cap)[0] for i in range(n)]
        rb, ro = orc.pack(rs)
    else:
        vals, cons, _ = consensus_pssm(rng, L, 250 - 2 * open_ + over, -open_, lo=max(-6, -open_), hi=min(9, 250 - 2 * open_))
        pm = pkg.Matrix.create_pssm(B62_LETTERS.decode(), [int(v) for v in vals.ravel()], L)
        smin, smax, msize = int(vals.min()), int(vals.max()), 24
        cap = _gate_cap(smax)
        q = random_seqs(rng, 1, L, L, AA)[0]
        rs = [mutate(rng, cons[i % 60:], 0.2, 0.06, AA)[:cap] if i % 4 else random_seqs(rng, 1, 1, cap, AA)[0] for i in range(n)]
    prof = pkg.Profile.new(q, True, pm)
    mr = max(map(len, rs))
    exts = [e for e in _gate_exts(open_) if _hook(pkg, L, mr, msize, smin, smax, open_, e) and _hook(pkg, L, mr, msize, smin, smax, open_, e, 160)]
    assert exts == GATE_EXTS_ADMITTED[open_], (scheme, kind, exts)          # (coverage cannot shrink unnoticed)
    for i, ext in enumerate(exts):
        for mode, sg in _gate_modes(i):
            al = _aligner(pkg, orc, pm, open_, ext, mode, sg, profile=prof)
            rec, st = al.align_batch([], rs)
            k = _kernel(pkg)
            traced = "pmx_nwsg16q_kernel" in k and "packed trace" in k
            if over == 0:
                assert traced and "packed trace/bfi" in k and "pmx_walkp_kernel" in k and (("pssm" in k) == (kind == "pssm")), (k, scheme, ext)
                monkeypatch.setenv("PMX_TRACE_NO_BFI", "1")
                rec2, st2 = al.align_batch([], rs)
                monkeypatch.delenv("PMX_TRACE_NO_BFI")
                assert (_records(rec) == _records(rec2)).all() and (_stats(st) == _stats(st2)).all() and (rec["flags"] == rec2["flags"]).all()
            else:
                assert not traced, (k, scheme, ext)
            if kind == "symbol":
                want = orc.align_stats_sample(mode, np.arange(n), None, None, rb, ro, open_, ext, om, sg_flags=sg or orc.SG_ALL, bits=32, shared_query=q)
            else:
                want, _ = check(orc, mode, sg or orc.SG_ALL, vals, np.asarray(pm.mapper()), B62_LETTERS, [q] * n, rs, open_, ext, with_cigar=False)
            bad = np.nonzero((_records(rec) != want[:, :3]).any(axis=1) | (_stats(st) != want[:, 3:6]).any(axis=1))[0]
            assert len(bad) == 0, (k, scheme, kind, over, ext, mode, sg, bad[:5], _records(rec)[bad[:5]], _stats(st)[bad[:5]], want[bad[:5], :6])
