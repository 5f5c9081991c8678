"""CPU tier of the ungapped diagonal filter: the model tests/seed_filter_ref.py against a brute-force enumeration of every segment
of every diagonal (tiny windows over 2 and 4 letters, where ties are frequent), against the scalar oracle's local alignment with gap
costs no gap can pay (scores only: the oracle's end-cell tie rule is its own), and the selection's rules on hand-made scores."""
import numpy as np

import seed_filter_ref as ref


def _matrix(alphabet, match, mismatch):
    """scores, mapper of a match / mismatch table with a last wildcard symbol that mismatches everything (the layout Matrix.create has)"""
    n = len(alphabet) + 1
    s = np.full((n, n), mismatch, dtype=np.int32)
    for i in range(len(alphabet)):
        s[i, i] = match
    mp = np.full(256, n - 1, dtype=np.int32)
    for i, c in enumerate(alphabet):
        mp[ord(c)] = mp[ord(c.lower())] = i
    return s, mp


def _brute(x, y, r_beg, dmin, dmax, scores, mapper):
    """every segment [a, b] of every diagonal: h(d, b) is the best sum of a segment that ends in b, or 0"""
    if dmin > dmax:
        return ref.BAD
    size = scores.shape[0]
    sx, sy = ref.symbols(x, mapper, size), ref.symbols(y, mapper, size)
    cells = []                                                                               # (h, d, i)
    for d in range(dmin, dmax + 1):
        on = [i for i in range(len(sx)) if r_beg <= i + d < r_beg + len(sy)]
        for bi, b in enumerate(on):
            sums = [sum(int(scores[sx[i], sy[i + d - r_beg]]) for i in on[ai:bi + 1]) for ai in range(bi + 1)]
            cells.append((max(0, max(sums)), d, b))
    top = max((c[0] for c in cells), default=0)
    if top <= 0:
        return (0, dmin, -1, -1)
    h, d, i = min((c for c in cells if c[0] == top), key=lambda c: (c[1], c[2]))
    return (h, d, i, i + d)


def test_model_equals_every_segment_of_every_diagonal():
    rng = np.random.default_rng(9100)
    ties = 0
    for alphabet, match, mismatch in (("AC", 1, -1), ("AC", 2, -3), ("ACGT", 2, -3), ("ACGT", 1, -1)):
        scores, mapper = _matrix(alphabet, match, mismatch)
        letters = alphabet.encode() + b"N"
        for _ in range(150):
            L, rl = int(rng.integers(1, 13)), int(rng.integers(1, 13))
            x = bytes(letters[int(v)] for v in rng.integers(0, len(letters), size=L))
            y = bytes(letters[int(v)] for v in rng.integers(0, len(letters), size=rl))
            r_beg = int(rng.integers(0, 20))
            dmin = r_beg + int(rng.integers(-L - 2, rl + 2))
            dmax = dmin + int(rng.integers(-1, L + rl + 3))
            got = ref.ungapped_window(x, y, r_beg, dmin, dmax, scores, mapper)
            want = _brute(x, y, r_beg, dmin, dmax, scores, mapper)
            assert tuple(got) == tuple(want), (x, y, r_beg, dmin, dmax)
            if want[0] > 0:
                full = [ref.ungapped_window(x, y, r_beg, d, d, scores, mapper)[0] for d in range(dmin, dmax + 1)]
                ties += full.count(want[0]) > 1
    assert ties > 50                                                                         # equal maxima on two diagonals are common here


def test_model_records_of_the_edge_cases():
    scores, mapper = _matrix("ACGT", 2, -3)
    assert ref.ungapped_window(b"ACGT", b"ACGT", 10, 10, 10, scores, mapper) == (8, 10, 3, 13)
    assert ref.ungapped_window(b"ACGT", b"TTTT", 10, 10, 10, scores, mapper) == (2, 10, 3, 13)
    assert ref.ungapped_window(b"AAAA", b"CCCC", 10, 7, 12, scores, mapper) == (0, 7, -1, -1)       # all negative
    assert ref.ungapped_window(b"AAAA", b"AAAA", 10, 20, 25, scores, mapper) == (0, 20, -1, -1)      # no cell at all
    assert ref.ungapped_window(b"AAAA", b"AAAA", 10, 5, 4, scores, mapper) == ref.BAD
    assert ref.ungapped_window(b"ACAC", b"ACAC", 0, -2, 2, scores, mapper) == (8, 0, 3, 3)           # d = -2, 0, 2 reach 4, 8, 4
    assert ref.ungapped_window(b"AC", b"ACTTAC", 0, 0, 4, scores, mapper) == (4, 0, 1, 1)            # equal maxima on d = 0 and 4: the lower d
    assert ref.ungapped_window(b"AC", b"ACTTAC", 0, 1, 4, scores, mapper) == (4, 4, 1, 5)
    assert ref.ungapped_window(b"ACAC", b"ACAC", 0, -2, -1, scores, mapper) == (4, -2, 3, 1)
    assert ref.ungapped_window(b"ACTTAC", b"ACGGAC", 0, 0, 0, scores, mapper) == (4, 0, 1, 1)        # twice on one diagonal: the first
    assert ref.ungapped_window(b"acgn", b"ACGN", 0, 0, 0, scores, mapper) == (6, 0, 2, 2)            # lower case maps, N mismatches itself
    pairs = ref.pairs_ref.pairs_array([(0, 0), (0, 0), (1, 0), (0, 0, 0, -1, 2, 9)])
    seeds = np.zeros(4, dtype=ref.SEED_HIT_DTYPE)
    out = ref.ungapped([b"ACGT"], [b"ACGT"], pairs, np.array([0, 2, 0, 0], dtype=np.uint8), seeds, scores, mapper)
    assert [tuple(r) for r in out] == [(8, 0, 3, 3), ref.BAD, ref.BAD, ref.BAD]
    out = ref.ungapped([b"ACGT"], [b"ACGT"], pairs[:1], np.array([1], dtype=np.uint8), seeds[:1], scores, mapper)
    assert tuple(out[0]) == (8, 0, 3, 3)                                                     # ACGT is its own reverse complement
    out = ref.ungapped([b"ATGAAATGG", b"AT"], [b"MKW"], ref.pairs_ref.pairs_array([(0, 0), (1, 0), (0, 0)]), np.array([0, 0, 6], dtype=np.uint8),
                       seeds[:3], *_matrix("MKW", 3, -1), kind="frame")
    assert [tuple(r) for r in out] == [(9, 0, 2, 2), ref.BAD, ref.BAD]                       # a frame without a codon, a frame byte of 6


def test_model_scores_equal_the_oracle_without_gaps(orc):
    rng = np.random.default_rng(9101)
    om = orc.Matrix.create("ACGT", 2, -3)
    qs, rs = [], []
    for _ in range(200):
        L, rl = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        q = bytes(b"ACGTN"[int(v)] for v in rng.integers(0, 5, size=L))
        r = bytearray(b"ACGTN"[int(v)] for v in rng.integers(0, 5, size=rl))
        if rng.random() < 0.5 and rl > 4:                                                    # a planted run, so that scores are not all tiny
            n = min(L, rl - 2)
            r[1:1 + n] = q[:n]
        qs.append(q)
        rs.append(bytes(r))
    qb, qo = orc.pack(qs)
    rb, ro = orc.pack(rs)
    full = orc.align_batch(orc.SW, qb, qo, rb, ro, 1000, 1000, om)                           # a gap costs more than any run of matches pays
    for k, (q, r) in enumerate(zip(qs, rs)):
        r_beg = 7 * k
        got = ref.ungapped_window(q, r, r_beg, r_beg - (len(q) - 1), r_beg + len(r) - 1, om.scores, om.mapper)
        assert got[0] == full[k, 0], k
    assert full[:, 0].max() > 30


def test_selection_rules():
    score = np.array([5, 9, 9, -1, 0, 9, 3, 3, 3, 7, -1, 0], dtype=np.int32)
    row_off = np.array([0, 6, 6, 9, 12], dtype=np.int64)                                     # rows of 6, 0, 3 and 3 candidates
    kept, off = ref.select(score, row_off)
    assert kept.tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9, 11] and off.tolist() == [0, 5, 5, 8, 10]      # the bad ones (-1) never pass
    kept, off = ref.select(score, row_off, min_score=-5)
    assert kept.tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9, 11]                                  # the floor is max(min_score, 0)
    kept, off = ref.select(score, row_off, top_n=1)
    assert kept.tolist() == [1, 6, 9] and off.tolist() == [0, 1, 1, 2, 3]                    # equal scores: the earlier position
    kept, off = ref.select(score, row_off, top_n=2)
    assert kept.tolist() == [1, 2, 6, 7, 9, 11] and off.tolist() == [0, 2, 2, 4, 6]
    kept, off = ref.select(score, row_off, top_n=4)
    assert kept.tolist() == [0, 1, 2, 5, 6, 7, 8, 9, 11]                                     # in input order, not in score order
    for top_n in (5, 6, 100):                                                                # top_n >= the row's count: all passing
        assert ref.select(score, row_off, top_n=top_n)[0].tolist() == ref.select(score, row_off)[0].tolist()
    kept, off = ref.select(score, row_off, min_score=8, top_n=2)
    assert kept.tolist() == [1, 2] and off.tolist() == [0, 2, 2, 2, 2]
    kept, off = ref.select(score, row_off, min_score=10)
    assert kept.tolist() == [] and off.tolist() == [0, 0, 0, 0, 0]
    rng = np.random.default_rng(9102)
    for _ in range(50):
        counts = rng.integers(0, 9, size=12)
        off_in = np.concatenate([[0], np.cumsum(counts)])
        sc = rng.integers(-1, 4, size=int(off_in[-1]))
        for top_n in (0, 1, 2, 3):
            kept, off = ref.select(sc, off_in, min_score=1, top_n=top_n)
            assert (np.diff(kept) > 0).all()                                                 # `source` strictly ascending
            assert off[-1] == len(kept) and (np.diff(off) >= 0).all()
            for r in range(12):
                mine = kept[off[r]:off[r + 1]]
                assert ((off_in[r] <= mine) & (mine < off_in[r + 1])).all() and (sc[mine] >= 1).all()
                passing = [x for x in range(off_in[r], off_in[r + 1]) if sc[x] >= 1]
                assert len(mine) == (min(top_n, len(passing)) if top_n else len(passing))
                left = sorted(set(passing) - set(mine.tolist()))
                for x in left:                                                               # whatever was dropped loses to everything kept
                    assert all((sc[m], -m) > (sc[x], -x) for m in mine)
