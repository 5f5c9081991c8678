"""The lane hand-off of the sw16 sweep (pmx_sw16.hip): lane g passes its last row's F and H to lane g + 1 once per step.  In the
skewed variants of the shapes whose shift needs no select (interleaved <8,R>, <16,R>, <64,R>) the two moves are DPP VOP2 that
do row 0's first operation on the way, and member 0 of a group -- the lane without a source -- keeps a preloaded value.

Every case here makes the hand-off carry a live value and asks for score, end_query and end_ref exactly as the scalar oracle
gives them:
  * vertical gaps: the query has three letters more than the reference, in rows g R - 1 .. g R + 1, between matching flanks, so
    F crosses the boundary above its floor;
  * diagonals: an exact copy of the query's rows around g R, so H crosses it;
  * member 0: pairs whose best cell lies in query row 0 (the preloaded values are all row 0 of member 0 ever sees);
  * query lengths 1, R - 1, R, R + 1, G R - 1, G R against reference lengths 1, 2, G - 1, G, 150.
The oracle's own CIGARs are walked on the CPU to make sure that every boundary has a pair whose gap run, and one whose
diagonal run, crosses it.

Batch sizes: the perm-table variant (the headline's) takes batches of 4096 pairs and more, <16,10> / <32,10> need more than 64, so
a batch is the smallest number of pairs of the form k NP + 3 (NP = pairs per wave) that reaches its shape and variant: the
last wave is partial, and lengths are mixed inside every wave (the batch is shuffled).  Unswitched, the test also checks
that the intended kernel ran; PMX_SW16_NO_PERMTABLE then runs the same batch through the LDS-profile variant."""
import numpy as np
import pytest

from util import random_seqs, mutate, DNA

pytestmark = pytest.mark.gpu

OPEN, EXT = 5, 2
# name: G, R, fewest pairs that select the shape, shortest random query (the longest is G R, which selects the shape too)
SHAPES = {
    "8x7": (8, 7, 4097, 20),
    "16x10": (16, 10, 65, 130),
    "32x10": (32, 10, 65, 280),
    "8x19": (8, 19, 4097, 135),
}
SWITCHES = [{}, {"PMX_SW16_NO_PERMTABLE": "1"}, {"PMX_SW16_NO_U8": "1"}, {"PMX_SW16_NO_SKEW": "1"}]
SWITCH_IDS = ["unswitched", "no_permtable", "no_u8", "no_skew"]


def _rand(rng, n):
    return DNA[rng.integers(0, 4, size=int(n))].tobytes()


def crafted_pairs(rng, G, R):
    """-> (queries, references, kind) with kind[i] = ("gap" | "diag", boundary row) or None"""
    qs, rs, kind = [], [], []
    for g in range(1, G):
        b = g * R
        for _ in range(2):
            # rows b-1, b, b+1 of the query face a gap
            left, ins, right = _rand(rng, b - 1), _rand(rng, 3), _rand(rng, min(15, G * R - b - 2))
            qs.append(left + ins + right); rs.append(left[-25:] + right); kind.append(("gap", b))
            q = _rand(rng, min(G * R, b + 12))
            qs.append(q); rs.append(q[max(0, b - 12):b + 12]); kind.append(("diag", b))
    for k in (1, 3, R, 2 * R + 1):                      # the best cell in row 0: the first letter matches, nothing else does
        qs.append(b"A" + b"C" * k); rs.append(b"GG" + b"A" + b"G" * k); kind.append(None)
        qs.append(b"A" + b"C" * k); rs.append(b"A"); kind.append(None)
    for ql in (1, R - 1, R, R + 1, G * R - 1, G * R):
        for rl in (1, 2, G - 1, G, 150):
            q = _rand(rng, ql)
            qs.append(q); rs.append((q * (rl // ql + 1))[:rl] if rng.random() < 0.5 else _rand(rng, rl)); kind.append(None)
    return qs, rs, kind


def crossings(orc, om, qs, rs, kind):
    """boundaries whose crafted pair has, by the oracle's own traceback, a gap run resp. a diagonal run across the boundary"""
    idx = np.array([i for i, k in enumerate(kind) if k is not None], dtype=np.int64)
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    texts, rec = orc.cigar_sample(orc.SW, idx, qb, qo, rb, ro, OPEN, EXT, om)
    import re
    found = {"gap": set(), "diag": set()}
    for i, text, (_, _, _, bq, _) in zip(idx, texts, rec):
        what, b = kind[i]
        row = int(bq)
        for n, op in re.findall(r"(\d+)([=XID])", text):
            n = int(n)
            if op == "D":
                continue                                                # consumes the reference only
            crosses = row <= b - 1 and row + n - 1 >= b                 # the run holds rows b - 1 and b
            if crosses and ((op == "I") == (what == "gap")):
                found[what].add(b)
            row += n
    return found


def build_case(orc, name, seed=0):
    G, R, nmin, qlo = SHAPES[name]
    NP = 2 * (64 // G)
    rng = np.random.default_rng(8000 + 100 * G + R + seed)
    qs, rs, kind = crafted_pairs(rng, G, R)
    n = max(nmin, len(qs) + NP)
    n += (3 - n) % NP                                                   # k NP + 3
    assert n <= 2048 or G == 8
    fill = n - len(qs)
    fq = random_seqs(rng, fill, qlo, G * R)
    fr = [mutate(rng, q, 0.08, 0.05) if rng.random() < 0.7 else random_seqs(rng, 1, 1, 200)[0] for q in fq]
    qs, rs, kind = qs + fq, rs + fr, kind + [None] * fill
    order = rng.permutation(n)
    qs, rs, kind = [qs[i] for i in order], [rs[i] for i in order], [kind[i] for i in order]
    om = orc.Matrix.create("ACGT", 2, -3)
    found = crossings(orc, om, qs, rs, kind)
    want_b = {g * R for g in range(1, G)}
    assert found["gap"] == want_b, sorted(want_b - found["gap"])
    assert found["diag"] == want_b, sorted(want_b - found["diag"])
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    want = orc.align_batch(orc.SW, qb, qo, rb, ro, OPEN, EXT, om)
    assert (want[:, 1] == 0).sum() >= 8                                 # best cells in row 0
    return {"qs": qs, "rs": rs, "kind": kind, "want": want, "G": G, "R": R}


def build_shared_case(orc):
    """<64,16>: one 1024-letter query, references of 40 - 300 letters; the crossings are cut out of the query"""
    G, R = 64, 16
    rng = np.random.default_rng(8640)
    q = _rand(rng, 1024)
    qs, rs, kind = [], [], []
    for g in range(1, G):
        b = g * R
        for w in (14, 22):
            rs.append(q[max(0, b - 2 - w):b - 2] + q[b + 3:b + 3 + w]); kind.append(("gap", b))     # rows b-2 .. b+2 face a gap (it may slide)
            rs.append(q[max(0, b - w):b + w]); kind.append(("diag", b))
    rs.append(q[:1]); kind.append(None)                                 # best cell in row 0
    rs.append(b"T" * 40 if q[:1] != b"T" else b"G" * 40); kind.append(None)
    for rl in (1, 2, G - 1, G, 150):
        rs.append(_rand(rng, rl)); kind.append(None)
    fill = 4099 - len(rs)                                               # the perm-table variant; NP = 2: an odd count leaves the last wave partial
    rs += random_seqs(rng, fill, 40, 300); kind += [None] * fill
    order = rng.permutation(len(rs))
    rs, kind = [rs[i] for i in order], [kind[i] for i in order]
    qs = [q] * len(rs)
    om = orc.Matrix.create("ACGT", 2, -3)
    found = crossings(orc, om, qs, rs, kind)
    want_b = {g * R for g in range(1, G)}
    assert found["gap"] == want_b, sorted(want_b - found["gap"])
    assert found["diag"] == want_b, sorted(want_b - found["diag"])
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    want = orc.align_batch(orc.SW, qb, qo, rb, ro, OPEN, EXT, om)
    assert (want[:, 1] == 0).any()
    return {"q": q, "rs": rs, "want": want}


_CASES = {}


def _case(orc, name):
    if name not in _CASES:
        _CASES[name] = build_shared_case(orc) if name == "64x16" else build_case(orc, name)
    return _CASES[name]


def _check(got, want):
    bad = np.nonzero((got["score"] != want[:, 0]) | (got["end_query"] != want[:, 1]) | (got["end_ref"] != want[:, 2]))[0]
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:4]], want[bad[:4]])
    assert (got["flags"] == 0).all()


@pytest.mark.parametrize("env", SWITCHES, ids=SWITCH_IDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_handoff_crossings_per_pair_queries(pkg, orc, monkeypatch, name, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = _case(orc, name)
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(OPEN).gap_extend(EXT).solution_width(16).build()
    got = al.align_batch(c["qs"], c["rs"])
    if not env:
        kernel = pkg.lib.pmx_last_kernel().decode()
        assert "pmx_sw16_kernel<%d,%d>" % (c["G"], c["R"]) in kernel and "skew" in kernel, kernel
        assert ("permtable" in kernel) == (c["G"] == 8), kernel
    _check(got, c["want"])


@pytest.mark.parametrize("env", SWITCHES, ids=SWITCH_IDS)
def test_handoff_crossings_shared_query_64_lanes(pkg, orc, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = _case(orc, "64x16")
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    al = pkg.Aligner.new().local().profile(pkg.Profile.new(c["q"], False, pm)).matrix(pm).gap_open(OPEN).gap_extend(EXT) \
        .solution_width(16).build()
    rb, ro = pkg.pack(c["rs"])
    got = al.align_batch_packed(None, None, rb, ro)
    if not env:
        kernel = pkg.lib.pmx_last_kernel().decode()
        assert "pmx_sw16_kernel<64,16>" in kernel and "permtable" in kernel, kernel
    _check(got, c["want"])


def test_handoff_crossings_in_the_wildcard_retry(pkg, orc):
    """A wildcard in the query sends the pair from the perm-table kernel to the retry launch (the LDS-profile variant, looped),
    which runs the same step.  The wildcard replaces the middle letter of every gap pair's surplus letters -- a row that faces
    the gap, so the alignment (and the crossing) stays -- and a letter of some random pairs."""
    c = _case(orc, "8x19")
    rng = np.random.default_rng(8190)
    qs = list(c["qs"])
    hit = 0
    for i, k in enumerate(c["kind"]):
        if k is not None and k[0] == "gap":
            q = bytearray(qs[i]); q[k[1]] = ord("N"); qs[i] = bytes(q); hit += 1
        elif k is None and i % 50 == 0:
            q = bytearray(qs[i]); q[int(rng.integers(len(q)))] = ord("N"); qs[i] = bytes(q)
    assert hit >= 7
    om = orc.Matrix.create("ACGT", 2, -3)
    qb, qo = orc.pack(qs); rb, ro = orc.pack(c["rs"])
    want = orc.align_batch(orc.SW, qb, qo, rb, ro, OPEN, EXT, om)
    found = crossings(orc, om, qs, c["rs"], [k if (k and k[0] == "gap") else None for k in c["kind"]])
    assert found["gap"] == {g * 19 for g in range(1, 8)}, found
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    al = pkg.Aligner.new().local().matrix(pm).gap_open(OPEN).gap_extend(EXT).solution_width(16).build()
    got = al.align_batch(qs, c["rs"])
    assert "permtable" in pkg.lib.pmx_last_kernel().decode()
    _check(got, want)
