"""CPU tier of the reference-side frameshift model (tests/swfsc_model.c through tests/frameshift_ref_side.py), the model the GPU tests
compare against: held against a path enumerator without DP, against the query-side model with the roles exchanged and the matrix
transposed (identity 1 of the contract), against the oracle's plain local score over three host-translated frames (identity 2), and
against the tie rule and the planted single-base shifts the feature exists for."""
import numpy as np

import frameshift_ref as fq
import frameshift_ref_side as fr
import translate_ref
from pairs_ex_ref import revcomp
from util import golden, AA


def _dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _asymmetric(orc):
    """match 4 / mismatch -3 over a protein sample, with entries that differ above and below the diagonal"""
    om = orc.Matrix.create("ACDEKLX", 4, -3)
    s = om.scores.copy()
    for a, b, up, low in ((0, 1, 2, -5), (2, 3, -1, 3), (4, 5, 1, -4), (1, 4, 0, -6)):
        s[a, b] = up; s[b, a] = low
    assert (s != s.T).any()
    return orc.Matrix(s, om.mapper, om.alphabet), orc.Matrix(np.ascontiguousarray(s.T), om.mapper, om.alphabet)


def test_model_against_brute_force(orc):
    """every m <= 4 and N <= 8, random letters of a 3-letter alphabet, fs 0, 1 and 3: the recurrence equals the enumeration of all
    paths.  Match 3 / mismatch -2 with small penalties, so that gaps and frameshifts lie on best paths."""
    om = orc.Matrix.create("ACD", 3, -2)
    letters = np.frombuffer(b"ACD", dtype=np.uint8)
    score = lambda a, b: int(om.scores[om.mapper[a], om.mapper[b]])
    rng = np.random.default_rng(17000)
    used_shift = used_gap = 0
    for m in range(1, 5):
        for N in range(1, 9):
            for open_, ext, f in ((3, 1, 0), (1, 1, 1), (2, 2, 3), (1, 3, 1)):
                for _ in range(6):
                    q = letters[rng.integers(0, 3, m)].tobytes(); T = letters[rng.integers(0, 3, N)].tobytes()
                    got = fr.align(q, T, om, open_, ext, f)
                    assert got[0] == fr.brute(q, T, score, open_, ext, f), (q, T, open_, ext, f)
                    assert got[3] == 0 and 0 <= got[1] < m and 2 <= got[2] < N + 2
                    used_shift += got[0] > fr.align(q, T, om, open_, ext, 1 << 20)[0]
                    used_gap += got[0] > fr.align(q, T, om, 1 << 20, 1 << 20, f)[0]
    assert used_shift >= 5 and used_gap >= 5               # no vacuous pass


def test_identity_with_the_query_side_model(orc):
    """identity 1: the score of (q rows, T columns, matrix s) equals the query-side model's score of (T rows, q columns, s transposed),
    with a matrix that is NOT symmetric, so s(query letter, reference letter) is pinned"""
    om, omT = _asymmetric(orc)
    letters = np.frombuffer(b"ACDEKL", dtype=np.uint8)
    rng = np.random.default_rng(17100)
    differ = 0
    for k in range(300):
        q = letters[rng.integers(0, 6, int(rng.integers(1, 30)))].tobytes()
        T = letters[rng.integers(0, 6, int(rng.integers(1, 90)))].tobytes()
        if k % 3 == 0 and len(T) >= 3 * len(q):                                      # a related pair: q spelled out in one frame of T
            T = bytes(b for a in q for b in (a, T[0], T[1]))[:len(T)]
        open_, ext, f = ((5, 1, 3), (3, 2, 0), (11, 1, 15))[k % 3]
        got = fr.align(q, T, om, open_, ext, f)
        assert got[0] == fq.align(T, q, omT, open_, ext, f)[0], (q, T)
        differ += got[0] != fq.align(T, q, om, open_, ext, f)[0]
    assert differ > 20                                     # the transposition matters on this sample


def test_identity_with_three_plain_frames(orc):
    """identity 2: fs = 2^28 is the best plain local score over the three host-translated frames of the strand, the oracle's"""
    b62 = orc.Matrix.from_file(golden("blosum62.txt"))
    rng = np.random.default_rng(17200)
    for k in range(100):
        w = _dna(rng, int(rng.integers(3, 201)))
        q = AA[rng.integers(0, len(AA), int(rng.integers(1, 60)))].tobytes()
        for strand in (0, 1):
            T = fr.stream(w, strand)
            assert T == fq.codon_stream(w, strand) and len(T) == len(w) - 2
            assert all(T[f::3] == translate_ref.translate(w, 3 * strand + f) for f in range(3))
            frames = [x for x in (T[f::3] for f in range(3)) if x]
            qb, qo = orc.pack([q] * len(frames)); rb, ro = orc.pack(frames)
            want = int(orc.align_batch(orc.SW, qb, qo, rb, ro, 11, 1, b62)[:, 0].max())
            assert fr.align(q, T, b62, 11, 1, 1 << 28)[0] == want == fr.align(q, T, b62, 11, 1, 0, no_shift=True)[0]
    assert fr.stream(b"AT") == b"" and fr.stream(b"atg", 1) == b"H" and fr.stream(b"ANGT") == b"XX"


def test_tie_rule_and_the_bad_pair(orc):
    b62 = orc.Matrix.from_file(golden("blosum62.txt"))
    K = int(b62.scores[b62.mapper[ord("K")], b62.mapper[ord("K")]])
    # every codon of poly-A reads K: all cells of a row-0 match tie at K in every column; the first column, then the first row
    assert fr.align(b"K", b"K" * 10, b62, 11, 1, 15) == [K, 0, 2, 0]
    # two rows: the maximum 2 K first appears in column 3 (row 1), whatever lies to its right
    assert fr.align(b"KK", fr.stream(b"A" * 20), b62, 11, 1, 15) == [2 * K, 1, 5, 0]
    assert fr.align(b"WWWW", fr.stream(b"A" * 12), b62, 11, 1, 15) == [0, 0, 2, 0]          # nothing positive: (0, 2)
    assert fr.pair(b"KK", b"A" * 20, 2, b62, 11, 1, 15) == ([2 * K, 1, 5, 0], 0)            # poly-A reversed is poly-T (F): forward
    assert fr.pair(b"FF", b"A" * 20, 2, b62, 11, 1, 15)[1] == 1 and fr.pair(b"FF", b"A" * 20, 0, b62, 11, 1, 15)[0][0] == 0
    pal = b"AAATTT"                                                                          # its own reverse complement: a tie, forward
    assert fr.pair(b"KF", pal, 2, b62, 11, 1, 15) == (fr.pair(b"KF", pal, 0, b62, 11, 1, 15)[0], 0)
    assert fr.pair(b"KF", pal, 1, b62, 11, 1, 15)[0] == fr.pair(b"KF", pal, 0, b62, 11, 1, 15)[0]
    for w in (b"", b"A", b"AT"):
        assert fr.pair(b"KK", w, 2, b62, 11, 1, 15) == (fr.BAD, 0)


def test_planted_single_base_shifts(orc):
    """a reference that codes for the query with one base deleted, or one inserted, at mid-piece: at fs = 15 the model is strictly
    above the best single-frame score, by about the other half of the piece"""
    b62 = orc.Matrix.from_file(golden("blosum62.txt"))
    rng = np.random.default_rng(17300)
    codon = {}
    for i, aa in enumerate(translate_ref.CODE_STD):
        codon.setdefault(aa, "TCAG"[i // 16] + "TCAG"[i // 4 % 4] + "TCAG"[i % 4])
    for k in range(40):
        q = AA[rng.integers(0, 20, 40)].tobytes()
        gene = "".join(codon[a] for a in q).encode()
        cut = 60 + int(rng.integers(-6, 7))
        gene = gene[:cut] + gene[cut + 1:] if k % 2 else gene[:cut] + _dna(rng, 1) + gene[cut:]
        window = _dna(rng, int(rng.integers(0, 30))) + gene + _dna(rng, int(rng.integers(0, 30)))
        for strand in (0, 1):
            w = window if strand == 0 else revcomp(window)
            T = fr.stream(w, strand)
            shifted, plain = fr.align(q, T, b62, 11, 1, 15)[0], fr.align(q, T, b62, 11, 1, 15, no_shift=True)[0]
            assert shifted > plain and shifted >= plain + 30, (k, strand, shifted, plain)
