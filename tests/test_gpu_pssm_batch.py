"""PSSM scoring in batches (include/parasail_amd.h): profile batches, per-pair batches and CIGAR batches with a position-specific
scoring matrix equal the oracle -- BLOSUM62 itself for PSSMs derived with to_pssm, the encoded PSSM checker (tests/pssm_oracle.py)
for arbitrary ones -- and the one-pair path, pair for pair."""
import numpy as np
import pytest

from tests.pssm_oracle import check
from tests.util import AA, golden, mutate, random_seqs

pytestmark = pytest.mark.gpu

OPEN, EXT = 11, 1
# (mode, oracle sg flags, query gaps, reference gaps)
MODES = [("nw", 0, [], []), ("sg", None, None, None), ("sg", "QB|DE", ["prefix"], ["suffix"]), ("sw", 0, [], [])]


def _sg(orc, spec):
    if spec is None:
        return orc.SG_ALL
    if spec == 0:
        return 0
    return {"QB|DE": orc.S1_BEG | orc.S2_END}[spec]


def _aligner(pkg, matrix, mode, qg, dg, width=16, stats=False, profile=None, trace=False):
    b = pkg.Aligner.new().matrix(matrix).gap_open(OPEN).gap_extend(EXT)
    if width != "sat":
        b.solution_width(width)
    {"nw": b.global_, "sg": b.semi_global, "sw": b.local}[mode]()
    if mode == "sg" and qg is not None:
        b.allow_query_gaps(qg).allow_ref_gaps(dg)
    if profile is not None:
        b.profile(profile)
    if stats:
        b.use_stats()
    if trace:
        b.use_trace()
    return b.build()


def _omode(mode):
    return {"nw": 0, "sg": 1, "sw": 2}[mode]


def _records(got):
    return np.stack([got["score"], got["end_query"], got["end_ref"]], axis=1)


def _stats(st):
    return np.stack([st["matches"], st["similar"], st["length"]], axis=1)


def _kernel(pkg):
    return pkg.lib.pmx_last_kernel().decode()


@pytest.mark.parametrize("qlen", [60, 150, 300, 1000])
def test_derived_pssm_profile_batches(pkg, orc, qlen):
    """to_pssm(q) of BLOSUM62 in profile batches == BLOSUM62 with q, every mode, widths sat / 16 / 32, scores and statistics;
    the PSSM forms of the shared-profile kernels run"""
    rng = np.random.default_rng(8800 + qlen)
    pm, om = pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))
    q = random_seqs(rng, 1, qlen, qlen, AA)[0]
    ps = pm.to_pssm(q)
    n = 520
    rs = [mutate(rng, q[int(a):int(a) + 200], 0.3, 0.05, AA) if k % 2 else random_seqs(rng, 1, 30, 400, AA)[0]
          for k, a in enumerate(rng.integers(0, max(1, qlen - 200), size=n))]
    qb, qo = orc.pack([q] * n); rb, ro = orc.pack(rs)
    idx = np.arange(n)
    for mode, sg, qg, dg in MODES:
        flags = _sg(orc, sg)
        want = orc.align_stats_sample(_omode(mode), idx, qb, qo, rb, ro, OPEN, EXT, om, sg_flags=flags, bits=32, shared_query=q)
        for width in (0, 16, 32):
            al = _aligner(pkg, ps, mode, qg, dg, width=width or "sat", profile=pkg.Profile.new(q, False, ps))
            got = al.align_batch([], rs)
            k = _kernel(pkg)
            assert (("pmx_sw16q_kernel" if mode == "sw" else "pmx_nwsg16q_kernel") in k) and "pssm" in k, k
            bad = np.nonzero((_records(got) != want[:, :3]).any(axis=1))[0]
            assert len(bad) == 0, (mode, sg, width, bad[:5], _records(got)[bad[:5]], want[bad[:5], :3])
            assert (got["flags"] == 0).all()
        for width in (0, 16, 32):
            al = _aligner(pkg, ps, mode, qg, dg, width=width or "sat", stats=True, profile=pkg.Profile.new(q, True, ps))
            got, st = al.align_batch([], rs)
            k = _kernel(pkg)
            if mode != "sw":
                assert "pmx_nwsg16q_kernel" in k and "pssm" in k and "pmx_walkp_kernel" in k, k
            bad = np.nonzero((_records(got) != want[:, :3]).any(axis=1) | (_stats(st) != want[:, 3:6]).any(axis=1))[0]
            assert len(bad) == 0, (mode, sg, width, k, bad[:5], _records(got)[bad[:5]], _stats(st)[bad[:5]], want[bad[:5]])


def _random_case(pkg, rng, L, n, lo=-6, hi=9):
    """A PSSM over BLOSUM62's alphabet whose rows differ for equal query letters, a profile query and per-pair queries of its
    length with other letters, related and unrelated references."""
    A = 24
    vals = rng.integers(lo, hi + 1, size=(L, A)).astype(np.int32)
    ps = pkg.Matrix.create_pssm("ARNDCQEGHILKMFPSTWYVBZX*", [int(v) for v in vals.ravel()], L)
    q0 = random_seqs(rng, 1, L, L, AA)[0]
    qs = [q0 if k % 3 == 0 else random_seqs(rng, 1, L, L, AA)[0] for k in range(n)]
    rs = [mutate(rng, qs[k], 0.3, 0.05, AA) if k % 2 else random_seqs(rng, 1, 10, 2 * L + 40, AA)[0] for k in range(n)]
    return ps, q0, qs, rs


def _check(orc, ps, mode, sg, queries, refs, with_cigar=True):
    return check(orc, _omode(mode), sg, ps.to_numpy().astype(np.int32), np.asarray(ps.mapper()), b"ARNDCQEGHILKMFPSTWYVBZX*",
                 queries, refs, OPEN, EXT, with_cigar=with_cigar)


@pytest.mark.parametrize("seed", [1, 2])
def test_random_pssm_batches(pkg, orc, seed):
    """random PSSMs: profile batches, per-pair batches (the same scores, matches by each pair's own letters) and CIGAR batches
    equal the encoded checker; 200 sampled pairs of each mode equal Aligner.align() with the same PSSM"""
    rng = np.random.default_rng(9900 + seed)
    L = int(rng.integers(40, 201))
    n = 560
    ps, q0, qs, rs = _random_case(pkg, rng, L, n)
    sample = rng.choice(n, size=200, replace=False)
    for mode, sg, qg, dg in MODES:
        flags = _sg(orc, sg)
        want_p, _ = _check(orc, ps, mode, flags, [q0] * n, rs, with_cigar=False)
        want_q, texts = _check(orc, ps, mode, flags, qs, rs)
        # profile batch: scores, then statistics
        got = _aligner(pkg, ps, mode, qg, dg, profile=pkg.Profile.new(q0, False, ps)).align_batch([], rs)
        assert (_records(got) == want_p[:, :3]).all(), (mode, sg, _kernel(pkg))
        got, st = _aligner(pkg, ps, mode, qg, dg, stats=True, profile=pkg.Profile.new(q0, True, ps)).align_batch([], rs)
        bad = np.nonzero((_records(got) != want_p[:, :3]).any(axis=1) | (_stats(st) != want_p[:, 3:6]).any(axis=1))[0]
        assert len(bad) == 0, (mode, sg, _kernel(pkg), bad[:5], _stats(st)[bad[:5]], want_p[bad[:5]])
        # per-pair batch: the same scores as the profile batch; matches follow each pair's letters
        got = _aligner(pkg, ps, mode, qg, dg).align_batch(qs, rs)
        k = _kernel(pkg)
        assert "pssm" in k and ("pmx_sw16q_kernel" in k if mode == "sw" else "pmx_nwsg16q_kernel" in k), k
        assert (_records(got) == want_q[:, :3]).all() and (want_q[:, :3] == want_p[:, :3]).all(), (mode, sg, k)
        al_s = _aligner(pkg, ps, mode, qg, dg, stats=True)
        got, st = al_s.align_batch(qs, rs)
        bad = np.nonzero((_records(got) != want_q[:, :3]).any(axis=1) | (_stats(st) != want_q[:, 3:6]).any(axis=1))[0]
        assert len(bad) == 0, (mode, sg, _kernel(pkg), bad[:5], _stats(st)[bad[:5]], want_q[bad[:5]])
        # CIGAR batch
        al_c = _aligner(pkg, ps, mode, qg, dg)
        got_c, cig = al_c.align_batch_cigar(qs, rs)
        assert (_records(got_c) == want_q[:, :3]).all(), (mode, sg)
        badc = [k for k in range(n) if cig[k] != texts[k]]
        assert not badc, (mode, sg, badc[:3], [cig[k] for k in badc[:3]], [texts[k] for k in badc[:3]])
        # one pair at a time through align(): the same record, statistics and CIGAR
        al_t = _aligner(pkg, ps, mode, qg, dg, trace=True)
        for k in sample:
            one = al_s.align(qs[k], rs[k])
            assert (one.get_score(), one.get_end_query(), one.get_end_ref()) == tuple(want_q[k, :3]), (mode, sg, k)
            assert (one.get_matches(), one.get_similar(), one.get_length()) == tuple(want_q[k, 3:6]), (mode, sg, k)
            assert al_t.align(qs[k], rs[k]).get_cigar(qs[k], rs[k]) == cig[k], (mode, sg, k)


@pytest.mark.parametrize("over", [0, 1])
def test_pssm_profile_byte_edge(pkg, orc, over):
    """PSSM values whose score + open (+ the row offset ext) reach 255 run on the PSSM forms; one more falls back to the general
    kernel; the results match either way"""
    rng = np.random.default_rng(7700 + over)
    L, n = 40, 520
    for mode, sg, qg, dg in MODES:
        top = (255 - OPEN if mode == "sw" else 255 - OPEN - EXT) + over
        vals = rng.integers(-6, 10, size=(L, 24)).astype(np.int32)
        vals[rng.integers(0, L, size=6), rng.integers(0, 20, size=6)] = top
        ps = pkg.Matrix.create_pssm("ARNDCQEGHILKMFPSTWYVBZX*", [int(v) for v in vals.ravel()], L)
        q0 = random_seqs(rng, 1, L, L, AA)[0]
        rs = random_seqs(rng, n, 10, 70, AA)
        want, _ = _check(orc, ps, mode, _sg(orc, sg), [q0] * n, rs, with_cigar=False)
        got = _aligner(pkg, ps, mode, qg, dg, width=32, profile=pkg.Profile.new(q0, False, ps)).align_batch([], rs)
        k = _kernel(pkg)
        if over:
            assert "pmx_general_kernel" in k, (mode, k)
        else:
            assert ("pmx_sw16q_kernel" if mode == "sw" else "pmx_nwsg16q_kernel") in k and "pssm" in k, (mode, k)
        assert (_records(got) == want[:, :3]).all(), (mode, sg, over, k)


def test_pssm_local_beyond_rerun_limit(pkg, orc):
    """a local PSSM batch whose best scores pass the int16 re-run limit (~29.7 k): the 32-bit path, exact results"""
    rng = np.random.default_rng(7600)
    L, n = 200, 64
    vals = rng.integers(-6, 10, size=(L, 24)).astype(np.int32)
    cons = rng.integers(0, 20, size=L)
    vals[np.arange(L), cons] = 160
    ps = pkg.Matrix.create_pssm("ARNDCQEGHILKMFPSTWYVBZX*", [int(v) for v in vals.ravel()], L)
    q0 = random_seqs(rng, 1, L, L, AA)[0]
    letters = b"ARNDCQEGHILKMFPSTWYVBZX*"
    consensus = bytes(letters[c] for c in cons)
    rs = [random_seqs(rng, 1, 0, 40, AA)[0] + (consensus if k % 2 else mutate(rng, consensus, 0.1, 0.02, AA)) +
          random_seqs(rng, 1, 0, 40, AA)[0] for k in range(n)]
    want, _ = _check(orc, ps, "sw", 0, [q0] * n, rs, with_cigar=False)
    assert want[:, 0].max() > 29700
    for width in ("sat", 32):
        got = _aligner(pkg, ps, "sw", [], [], width=width, profile=pkg.Profile.new(q0, False, ps)).align_batch([], rs)
        assert (_records(got) == want[:, :3]).all(), (width, _kernel(pkg))


def test_pssm_2048_rows(pkg, orc):
    """a 2 048-row to_pssm profile batch, score only, all three modes: the largest shapes of the PSSM forms"""
    rng = np.random.default_rng(7500)
    pm, om = pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))
    q = random_seqs(rng, 1, 2048, 2048, AA)[0]
    ps = pm.to_pssm(q)
    n = 40
    rs = [mutate(rng, q[int(a):int(a) + 900], 0.3, 0.05, AA) if k % 2 else random_seqs(rng, 1, 100, 1500, AA)[0]
          for k, a in enumerate(rng.integers(0, 1100, size=n))]
    qb, qo = orc.pack([q] * n); rb, ro = orc.pack(rs)
    for mode in ("nw", "sg", "sw"):
        want = orc.align_batch(_omode(mode), qb, qo, rb, ro, OPEN, EXT, om, bits=32)
        got = _aligner(pkg, ps, mode, None, None, width=32, profile=pkg.Profile.new(q, False, ps)).align_batch([], rs)
        k = _kernel(pkg)
        assert ("pmx_sw16q_kernel" if mode == "sw" else "pmx_nwsg16q_kernel") in k and "pssm" in k, (mode, k)
        assert (_records(got) == want).all(), (mode, k)
