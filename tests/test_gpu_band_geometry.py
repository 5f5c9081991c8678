"""Banded kernels at band-edge geometry (`-m gpu`): every case against the banded oracle, pair by pair, with the kernel's name
asserted so that a fallback cannot pass a case.

The launchers size their LDS streams from the batch's maxima.  Batches built as `pre + mutate(query) + post` never let
max_qlen bind (max_rlen >= max_qlen in every launch); here it does:
  A. queries that outgrow their references by the band's width (ql >= rl + 2 band, centres in [-band, 0)): the band-strip
     kernel's pairs run up to min(ql, rl + 2 band) rows, past the last column -- the NW corner on the band's edge when
     ql == rl + 2 band and d0 == -band;
  B. the same through the profile arm (one shared query);
  C. the mirror shape (rl >= ql + 2 band);
  D. bands that meet the matrix in exactly one corner cell, and one step further, where they miss it;
  E. A, C and D through the other banded kernels (staged, per-cell, packed, general)."""
import numpy as np
import pytest

from util import AA, golden, random_seqs, mutate

pytestmark = pytest.mark.gpu


def _modes(orc):
    sgs = [orc.SG_ALL, orc.S1_BEG, orc.S1_END, orc.S2_BEG, orc.S2_END, orc.S1_END | orc.S2_END]
    return [(0, 0)] + [(1, s) for s in sgs] + [(2, 0)]


def _aligner(pkg, orc, pm, mode, sg, open_, ext, profile_query=None):
    b = pkg.Aligner.new().matrix(pm).gap_open(open_).gap_extend(ext)
    if profile_query is not None:
        b.profile(pkg.Profile.new(profile_query, False, pm))
    [b.global_, b.semi_global, b.local][mode]()
    if mode == 1:
        qg = [t for f, t in ((orc.S1_BEG, "prefix"), (orc.S1_END, "suffix")) if sg & f]
        dg = [t for f, t in ((orc.S2_BEG, "prefix"), (orc.S2_END, "suffix")) if sg & f]
        b.allow_query_gaps(qg).allow_ref_gaps(dg)
    return b.build()


def _piece(rng, src, at, length, alphabet):
    """`length` letters related to src[at:] (a mutated copy, cut or padded to length), or unrelated ones"""
    if rng.random() < 0.75 and 0 <= at < len(src):
        s = mutate(rng, src[at:at + length], 0.1, 0.03, alphabet)
    else:
        s = b""
    return (s + random_seqs(rng, 1, length, length, alphabet)[0])[:length]


def _outgrow(rng, n, k, alphabet, exact_every=4):
    """A: ql >= rl + 2 band; half the centres at -band, the rest in [-band, 0); every `exact_every`-th pair ql == rl + 2 band"""
    qs, rs, dg = [], [], []
    for t in range(n):
        rl = int(rng.integers(1, 121))
        ql = rl + 2 * k + (0 if t % exact_every == 0 else int(rng.integers(0, 60)))
        d = -k if t % 2 == 0 else -int(rng.integers(1, k + 1)) if k else 0
        q = random_seqs(rng, 1, ql, ql, alphabet)[0]
        qs.append(q); rs.append(_piece(rng, q, -d, rl, alphabet) or alphabet[:1].tobytes()); dg.append(d)
    return qs, rs, np.array(dg, dtype=np.int32)


def _mirror(rng, n, k, alphabet):
    """C: rl >= ql + 2 band; centres in (0, band] or at rl - ql +- band"""
    qs, rs, dg = [], [], []
    for t in range(n):
        ql = int(rng.integers(1, 121))
        rl = ql + 2 * k + (0 if t % 4 == 0 else int(rng.integers(0, 60)))
        d = [int(rng.integers(1, k + 1)) if k else 0, k, rl - ql - k, rl - ql + k][t % 4]
        r = random_seqs(rng, 1, rl, rl, alphabet)[0]
        qs.append(_piece(rng, r, d, ql, alphabet) or alphabet[:1].tobytes()); rs.append(r); dg.append(d)
    return qs, rs, np.array(dg, dtype=np.int32)


D_LENGTHS = (1, 2, 3, 17, 64, 65, 200)


def _corners(rng, k, alphabet):
    """D: the band meets the matrix in exactly one corner cell -- (0, rl - 1) at d0 = rl - 1 + band, (ql - 1, 0) at
    d0 = -(ql - 1) - band -- or, one step further, misses it"""
    qs, rs, dg = [], [], []
    for ql in D_LENGTHS:
        for rl in D_LENGTHS:
            for d in (rl - 1 + k, rl + k, -(ql - 1) - k, -ql - k):
                qs.append(random_seqs(rng, 1, ql, ql, alphabet)[0]); rs.append(random_seqs(rng, 1, rl, rl, alphabet)[0]); dg.append(d)
    return qs, rs, np.array(dg, dtype=np.int32)


def _check(pkg, orc, al, om, mode, sg, open_, ext, qs, rs, k, diag, kernel, tag=()):
    got = al.align_batch_banded(qs, rs, k, diag)
    name = pkg.lib.pmx_last_kernel().decode()
    assert (name == kernel) if not kernel.endswith("/") else name.startswith(kernel), (name, kernel, tag)
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    want = orc.align_banded_batch(mode, qb, qo, rb, ro, open_, ext, om, k, diag, sg_flags=sg)
    bad = np.nonzero((got["score"] != want[:, 0]) | (got["end_query"] != want[:, 1]) | (got["end_ref"] != want[:, 2]) | (got["flags"] != 0))[0]
    assert len(bad) == 0, (tag, name, mode, sg, open_, ext, k, len(bad), bad[:5], got[bad[:3]], want[bad[:3]],
                           [(len(qs[x]), len(rs[x]), int(diag[x])) for x in bad[:3]])


def _strip_name(mode, skew):
    return "pmx_bstrip_kernel/local" if mode == 2 else "pmx_bstrip_kernel/%s skew" % skew


A_BANDS = (15, 16, 31, 33, 47, 48, 63)
FORCED = ("4x8", "8x8", "2x16", "4x16", "8x16")


@pytest.mark.parametrize("skew", ["double", "one"])
def test_a_query_outgrows_reference_strip_kernel(pkg, orc, skew, monkeypatch):
    """A on the band-strip kernel: default shapes and every forced shape that holds the band, every mode, both skews; batches of
    64 pairs and single pairs (n = 1: the maxima are the pair's own lengths)"""
    if skew == "one":
        monkeypatch.setenv("PMX_BSTRIP_ONE_SKEW", "1")
    rng = np.random.default_rng(10100 + (skew == "one"))
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    als = {ms: _aligner(pkg, orc, pm, ms[0], ms[1], 5, 2) for ms in _modes(orc)}
    for k in A_BANDS:
        shapes = [None] + [s for s in FORCED if int(s.split("x")[0]) * int(s.split("x")[1]) >= 2 * k + 1]
        for shape in shapes:
            if shape is None:
                monkeypatch.delenv("PMX_BSTRIP_SHAPE", raising=False)
            else:
                monkeypatch.setenv("PMX_BSTRIP_SHAPE", shape)
            for (mode, sg), al in als.items():
                if mode == 2 and skew == "one":
                    continue                          # local alignment has one skew only: the other parametrisation runs it
                qs, rs, dg = _outgrow(rng, 64, k, dna)
                _check(pkg, orc, al, om, mode, sg, 5, 2, qs, rs, k, dg, _strip_name(mode, skew), ("A", k, shape))
                if shape is None:
                    for t in (0, 1, 3):
                        _check(pkg, orc, al, om, mode, sg, 5, 2, qs[t:t + 1], rs[t:t + 1], k, dg[t:t + 1], _strip_name(mode, skew),
                               ("A, n = 1", k, len(qs[t]), len(rs[t]), int(dg[t])))
    monkeypatch.delenv("PMX_BSTRIP_SHAPE", raising=False)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_b_query_outgrows_reference_profile_arm(pkg, orc, mode):
    """B: one shared query of 400 letters, references of at most 120 columns, centres in [-band, 0)"""
    rng = np.random.default_rng(10200 + mode)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    q = random_seqs(rng, 1, 400, 400)[0]
    for sg in ((orc.SG_ALL, orc.S1_END, orc.S2_END) if mode == 1 else (0,)):
        al = _aligner(pkg, orc, pm, mode, sg, 5, 2, profile_query=q)
        for k in (15, 31, 48, 63):
            rs, dg = [], []
            for t in range(200):
                d = -k if t % 2 == 0 else -int(rng.integers(1, k + 1))
                rl = int(rng.integers(1, 121))
                rs.append(_piece(rng, q, -d + (int(rng.integers(0, 400 - rl)) if t % 3 == 2 else 0), rl, dna)); dg.append(d)
            dg = np.array(dg, dtype=np.int32)
            got = al.align_batch_banded([], rs, k, dg)
            name = pkg.lib.pmx_last_kernel().decode()
            assert name.startswith("pmx_bstrip_kernel/"), (name, k)
            rb, ro = orc.pack(rs)
            want = orc.align_banded_batch(mode, None, None, rb, ro, 5, 2, om, k, dg, sg_flags=sg, shared_query=q)
            bad = np.nonzero((got["score"] != want[:, 0]) | (got["end_query"] != want[:, 1]) | (got["end_ref"] != want[:, 2]) | (got["flags"] != 0))[0]
            assert len(bad) == 0, (mode, sg, k, len(bad), got[bad[:3]], want[bad[:3]], [(len(rs[x]), int(dg[x])) for x in bad[:3]])


@pytest.mark.parametrize("skew", ["double", "one"])
def test_c_mirror_and_d_corner_cells_strip_kernel(pkg, orc, skew, monkeypatch):
    """C (rl >= ql + 2 band) and D (one-cell and just-missed bands, batched and one pair at a time) on the band-strip kernel"""
    if skew == "one":
        monkeypatch.setenv("PMX_BSTRIP_ONE_SKEW", "1")
    rng = np.random.default_rng(10300 + (skew == "one"))
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    for (mode, sg) in _modes(orc):
        if mode == 2 and skew == "one":
            continue
        al = _aligner(pkg, orc, pm, mode, sg, 5, 2)
        name = _strip_name(mode, skew)
        for k in (0, 1, 15, 31, 48, 63):
            qs, rs, dg = _mirror(rng, 64, k, dna)
            _check(pkg, orc, al, om, mode, sg, 5, 2, qs, rs, k, dg, name, ("C", k))
            qs, rs, dg = _corners(rng, k, dna)
            _check(pkg, orc, al, om, mode, sg, 5, 2, qs, rs, k, dg, name, ("D", k))
        for t in range(0, len(qs), 13):
            _check(pkg, orc, al, om, mode, sg, 5, 2, qs[t:t + 1], rs[t:t + 1], 63, dg[t:t + 1], name,
                   ("D, n = 1", len(qs[t]), len(rs[t]), int(dg[t])))


def _shapes_acd(rng, k, alphabet):
    for kind, (qs, rs, dg) in (("A", _outgrow(rng, 48, k, alphabet)), ("C", _mirror(rng, 48, k, alphabet)), ("D", _corners(rng, k, alphabet))):
        yield kind, qs, rs, dg


@pytest.mark.parametrize("form", ["no strip", "no staging"])
def test_e_other_band_kernels_dna(pkg, orc, form, monkeypatch):
    """E: A, C and D through the anti-diagonal kernels -- PMX_BANDED_NO_STRIP: the staged kernel (the packed kernel's matrix-rows form
    for local alignment); PMX_BANDED_NO_STAGING: the per-cell kernel"""
    monkeypatch.setenv("PMX_BANDED_NO_STRIP" if form == "no strip" else "PMX_BANDED_NO_STAGING", "1")
    rng = np.random.default_rng(10400 + (form == "no staging"))
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    for (mode, sg) in _modes(orc):
        al = _aligner(pkg, orc, pm, mode, sg, 5, 2)
        if form == "no staging":
            name = "pmx_banded_kernel"
        else:
            name = "pmx_banded_packed_kernel/matrix rows" if mode == 2 else "pmx_banded_staged_kernel"
        for k in (0, 15, 31, 48, 63):
            for kind, qs, rs, dg in _shapes_acd(rng, k, dna):
                _check(pkg, orc, al, om, mode, sg, 5, 2, qs, rs, k, dg, name, (form, kind, k))


def test_e_protein_and_general_kernel(pkg, orc):
    """E: BLOSUM62 protein (the packed kernel's byte-lookup form for local alignment, the staged kernel otherwise) and bands of 64 and
    100 (the general kernel's banded form), shapes A, C and D"""
    rng = np.random.default_rng(10500)
    pb, ob = pkg.Matrix.from_name("blosum62"), orc.Matrix.from_file(golden("blosum62.txt"))
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    for (mode, sg) in _modes(orc):
        al = _aligner(pkg, orc, pb, mode, sg, 11, 1)
        for k in (0, 15, 31, 63):
            for kind, qs, rs, dg in _shapes_acd(rng, k, AA):
                _check(pkg, orc, al, ob, mode, sg, 11, 1, qs, rs, k, dg,
                       "pmx_banded_packed_kernel" if mode == 2 else "pmx_banded_staged_kernel", ("protein", kind, k))
        al = _aligner(pkg, orc, pm, mode, sg, 5, 2)
        for k in (64, 100):
            for kind, qs, rs, dg in _shapes_acd(rng, k, dna):
                _check(pkg, orc, al, om, mode, sg, 5, 2, qs, rs, k, dg, "pmx_general_kernel/banded", ("general", kind, k))


def test_e_local_shared_query_rows(pkg, orc, monkeypatch):
    """E: local alignment against a small-alphabet profile with the strip kernel switched off -- the packed kernel's shared-query-rows
    form -- with references shorter than the query by the band's width or more (A through a profile) and corner-cell bands (D)"""
    monkeypatch.setenv("PMX_BANDED_NO_STRIP", "1")
    rng = np.random.default_rng(10600)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    for ql in (1, 2, 65, 200, 400):
        q = random_seqs(rng, 1, ql, ql)[0]
        al = _aligner(pkg, orc, pm, 2, 0, 5, 2, profile_query=q)
        for k in (0, 15, 31, 48, 63):
            rs, dg = [], []
            for t in range(128):
                if t % 2 == 0:
                    d = -k if t % 4 == 0 else -int(rng.integers(0, k + 1))
                    rl = max(1, min(120, ql - 2 * k - int(rng.integers(0, 8))))
                    rs.append(_piece(rng, q, -d, rl, dna))
                else:
                    rl = D_LENGTHS[(t // 2) % len(D_LENGTHS)]
                    d = [rl - 1 + k, rl + k, -(ql - 1) - k, -ql - k][(t // 2) % 4]
                    rs.append(random_seqs(rng, 1, rl, rl)[0])
                dg.append(d)
            dg = np.array(dg, dtype=np.int32)
            got = al.align_batch_banded([], rs, k, dg)
            name = pkg.lib.pmx_last_kernel().decode()
            assert name == "pmx_banded_packed_kernel/shared query rows", (name, ql, k)
            rb, ro = orc.pack(rs)
            want = orc.align_banded_batch(2, None, None, rb, ro, 5, 2, om, k, dg, shared_query=q)
            bad = np.nonzero((got["score"] != want[:, 0]) | (got["end_query"] != want[:, 1]) | (got["end_ref"] != want[:, 2]) | (got["flags"] != 0))[0]
            assert len(bad) == 0, (ql, k, len(bad), got[bad[:3]], want[bad[:3]], [(len(rs[x]), int(dg[x])) for x in bad[:3]])
