"""End-position ties of the headline local kernel (perm-table variant, 8-lane groups of 19 rows): pairs built so that the
maximum sits in the first or last column, in the first or last row of a lane, appears many times, or is reached by both
pairs of a slot in the same step.  Results must equal the CPU oracle bit for bit (first maximum in column-major order)."""
import numpy as np
import pytest

from util import random_seqs

pytestmark = pytest.mark.gpu

L = 150
MOTIF = b"ACGTAGT"


def _plant(base, motif, end):
    """`base` with `motif` written so that its last letter is at position `end`"""
    s = bytearray(base)
    s[end - len(motif) + 1:end + 1] = motif
    return bytes(s)


def _tie_pairs(rng):
    qs, rs = [], []

    def add(q, r):
        qs.append(q); rs.append(r)

    cq, gr = b"C" * L, b"G" * L                 # C against G scores a mismatch everywhere: only planted motifs score
    # maximum in the first column / the last column; every row ties
    add(b"A" * L, b"A" + b"C" * (L - 1))
    add(b"A" * L, b"C" * (L - 1) + b"A")
    add(_plant(cq, b"A", 70), b"G" * (L - 1) + b"A")
    add(_plant(cq, b"A", 0), b"A" + b"G" * (L - 1))
    # the motif ending in the first / last row of a lane (lane g holds rows 19 g .. 19 g + 18) and in the query's last row
    for end in (6, 18, 19, 37, 38, 132, 133, 149):
        for col in (6, 18, 75, 149):
            add(_plant(cq, MOTIF, end), _plant(gr, MOTIF, col))
    # equal maxima: the same column in two lanes (first row wins), the same row in two columns (first column wins), and a
    # later row in an earlier column against an earlier row in a later column (column-major: the earlier column wins)
    for a, b in ((10, 140), (18, 19), (40, 60)):
        add(_plant(_plant(cq, MOTIF, a), MOTIF, b), _plant(gr, MOTIF, 90))
        add(_plant(cq, MOTIF, 90), _plant(_plant(gr, MOTIF, a), MOTIF, b))
        q = _plant(_plant(cq, MOTIF, a), b"TTGCA", b)
        r = _plant(_plant(gr, MOTIF, b + 20), b"TTGCA", a + 3)
        add(q, r)
    # many equal maxima: periodic sequences
    for period in (b"ACGT", b"AACC", b"ACGTTGCA", b"A"):
        s = (period * L)[:L]
        add(s, s)
        add(s, (period * L)[1:L + 1])
    # random pairs with an exact repeat of the query inside the reference at several offsets
    for k in range(64):
        q = random_seqs(rng, 1, L, L)[0]
        off = int(rng.integers(0, L - 30))
        seg = q[off:off + 30]
        r = bytearray(random_seqs(rng, 1, L, L)[0])
        for at in (int(rng.integers(0, 40)), int(rng.integers(60, L - 30))):
            r[at:at + 30] = seg
        add(q, bytes(r))
    return qs, rs


def test_sw16_permtable_end_position_ties(pkg, orc):
    rng = np.random.default_rng(2606)
    qs, rs = _tie_pairs(rng)
    # each case twice in a row (pairs 2 s and 2 s + 1 share a slot: both halves improve in the same steps), then random
    # pairs up to a batch large enough for the perm-table kernel
    qs = [q for q in qs for _ in range(2)]
    rs = [r for r in rs for _ in range(2)]
    n0 = len(qs)
    qs += random_seqs(rng, 4200 - n0, L, L)
    rs += random_seqs(rng, 4200 - n0, L, L)
    pm, om = pkg.Matrix.create(b"ACGT", 2, -3), orc.Matrix.create("ACGT", 2, -3)
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    for open_, ext in ((5, 2), (3, 3), (4, 1)):         # open >= -mismatch: the perm-table variant
        got = pkg.Aligner.new().local().matrix(pm).gap_open(open_).gap_extend(ext).solution_width(16).build() \
            .align_batch(qs, rs)
        assert "pmx_sw16_kernel<8,19>" in pkg.lib.pmx_last_kernel().decode()
        want = orc.align_batch(orc.SW, qb, qo, rb, ro, open_, ext, om)
        bad = np.nonzero((got["score"] != want[:, 0]) | (got["end_query"] != want[:, 1]) |
                         (got["end_ref"] != want[:, 2]))[0]
        assert len(bad) == 0, (open_, ext, bad[:5], got[bad[:5]], want[bad[:5]])
        assert (got["flags"] == 0).all()
