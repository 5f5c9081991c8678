"""CPU tier of the windowed reference-side frameshift traceback (pmx_align_pairs_frameshift_ref_cigar_long[_device]): the
window bound the kernel runs -- the library's hook pmx_swfsc_window_cols, parasail-rs_amd/csrc/pmx_fswin.h -- held against the CPU model
of the traceback (tests/swfsc_trace_model.c through tests/frameshift_trace_ref_side.py).  For every pair the model runs twice: over the
full oriented window, and over query rows [0, end_query] x oriented nucleotides [a, end_ref] with a = max(0, end_ref + 1 - W).  The
second run must give the first run's record (after + a), text, begins (after + a) and statistics, and the path must span at most W
nucleotides.  No case is skipped."""
import numpy as np
import pytest

import frameshift_ref_side as fr
import frameshift_trace_ref_side as ft
from test_gpu_frameshift_ref import _dna, _gene
from util import golden, random_seqs, AA

ALL = (1 << 63) - 1
# open, extend, fs: the usual, cheap ones, open == extend with fs == 0, extend above open, fs == 0 alone, extend == 0 (nothing is bounded)
PENALTIES = ((11, 1, 15), (2, 1, 3), (3, 3, 0), (5, 2, 7), (11, 1, 0), (2, 5, 4), (4, 0, 5), (7, 7, 7))
LETTERS = "ARNDCQEGHILKMFPSTWYV"


def window_of(pkg, q, rec, om, open_, ext, fs):
    """(a, W) of a record, through the library's hook; P from the matrix the model uses"""
    score, eq, er = rec[:3]
    rowmax = np.maximum(om.scores.max(axis=1), 0)
    P = int(sum(int(rowmax[om.mapper[c]]) for c in q[:eq + 1]))
    W = pkg.lib.pmx_swfsc_window_cols(P, score, eq + 1, open_, ext, fs)
    return max(0, er + 1 - W), W


def narrowed(q, T, rec, a):
    """the rows and stream columns of the window [a, end_ref] in nucleotides: stream letter j reads nucleotides j .. j + 2"""
    return q[:rec[1] + 1], T[a:rec[2] - 1]


def _planted(rng, q):
    """a nucleotide string that codes for a piece of q with 0 - 3 single-base events and, in half the cases, a codon gap on either side"""
    lo = int(rng.integers(0, max(1, len(q) // 3)))
    piece = q[lo:lo + int(rng.integers(4, len(q) - lo + 1))]
    events = int(rng.integers(0, 4))
    shifts = []
    if len(piece) > 6:
        at = sorted(set(int(x) for x in rng.integers(1, len(piece) - 2, events)))
        shifts = [(x, int(rng.integers(0, 2))) for x in at]
    g = _gene(rng, piece, shifts)
    if len(piece) > 12 and rng.integers(0, 2):
        cut = 3 * int(rng.integers(4, len(piece) - 4))
        if rng.integers(0, 2):
            g = g[:cut] + _dna(rng, 3 * int(rng.integers(1, 3))) + g[cut:]      # codons the query does not have
        else:
            g = g[:cut] + g[cut + 3:]                                            # a query letter the reference does not have
    return g


def _cases(orc):
    b62 = orc.Matrix.from_file(golden("blosum62.txt"))
    cre = orc.Matrix.create(LETTERS, 5, -4)
    rng = np.random.default_rng(21000)
    for k in range(400):
        om = cre if k % 4 == 3 else b62
        open_, ext, fs = PENALTIES[k % len(PENALTIES)]
        q = random_seqs(rng, 1, 5, 60, AA)[0]
        g = _planted(rng, q) if k % 25 else b""                     # every 25th window is noise alone
        W_nt = int(rng.integers(max(100, len(g) + 10), 3001))
        right = int(rng.integers(0, min(200, W_nt - len(g)) + 1))   # the left flank is the long one: the column shift is what is tested
        window = _dna(rng, W_nt - len(g) - right) + g + _dna(rng, right)
        assert 100 <= len(window) <= 3000
        yield k, om, open_, ext, fs, q, window, k % 3 == 2          # every third window is read on strand 1


def test_window_gives_the_full_matrix_results(pkg, orc):
    removed = total = positive = shifted = gapped = 0
    for k, om, open_, ext, fs, q, window, reverse in _cases(orc):
        T = fr.stream(window, 1 if reverse else 0)
        rec, text, beg, stats = ft.align(q, T, om, open_, ext, fs)
        a, W = window_of(pkg, q, rec, om, open_, ext, fs)
        assert 0 <= a <= rec[2] - 2 and W >= 3 * (rec[1] + 1)
        if min(open_, ext) == 0:
            assert W == ALL and a == 0                             # nothing is bounded
        qn, Tn = narrowed(q, T, rec, a)
        assert len(qn) == rec[1] + 1 and len(Tn) == rec[2] - 1 - a >= 1
        rec2, text2, beg2, stats2 = ft.align(qn, Tn, om, open_, ext, fs)
        assert [rec2[0], rec2[1], rec2[2] + a, rec2[3]] == rec, (k, rec, rec2, a)
        assert text2 == text and [beg2[0], beg2[1] + a] == beg and stats2 == stats, (k, text, text2)
        if rec[0] > 0:
            assert rec[2] - beg[1] + 1 <= W, (k, rec, beg, W)       # the path's span in nucleotides
            positive += 1
            shifted += "/" in text or "\\" in text
            gapped += "I" in text or "D" in text
        else:
            assert rec[:3] == [0, 0, 2] and a == 0 and text2 == "" and beg2 == [1, 3]
        total += 1
        removed += a > 0
    # the share of cases in which narrowing removes at least one column: 282 of 400 with these flanks (an eighth of the cases has
    # extend = 0 and is never narrowed), required above one half
    print("narrowed %d of %d; positive %d, with a frameshift op %d, with a gap %d" % (removed, total, positive, shifted, gapped))
    assert total == 400 and removed > total // 2, (removed, total)
    assert positive >= 380 and shifted >= 100 and gapped >= 50, (positive, shifted, gapped)


def test_extend_zero_is_not_narrowed(pkg, orc):
    """extend = 0 (and open = 0): a gap run is free to grow, W is unbounded and a = 0 whatever the record"""
    b62 = orc.Matrix.from_file(golden("blosum62.txt"))
    rng = np.random.default_rng(21100)
    for k in range(20):
        q = random_seqs(rng, 1, 5, 40, AA)[0]
        window = _dna(rng, int(rng.integers(300, 1500))) + _gene(rng, q) + _dna(rng, 30)
        T = fr.stream(window, 0)
        for open_, ext in ((6, 0), (0, 0), (0, 2)):
            rec, text, beg, stats = ft.align(q, T, b62, open_, ext, 9)
            a, W = window_of(pkg, q, rec, b62, open_, ext, 9)
            assert W == ALL and a == 0 and rec[0] > 0


def test_a_tight_window_is_needed(pkg, orc):
    """the check above is not vacuous: one column fewer than the path spans loses the record"""
    b62 = orc.Matrix.from_file(golden("blosum62.txt"))
    rng = np.random.default_rng(21200)
    lost = 0
    for k in range(40):
        q = random_seqs(rng, 1, 20, 40, AA)[0]
        T = fr.stream(_dna(rng, 400) + _gene(rng, q, [(len(q) // 2, k % 2)]) + _dna(rng, 50), 0)
        rec, text, beg, stats = ft.align(q, T, b62, 11, 1, 15)
        a = beg[1] + 1                                             # the first codon's first nucleotide is cut off
        rec2 = ft.align(q[:rec[1] + 1], T[a:rec[2] - 1], b62, 11, 1, 15)[0]
        lost += [rec2[0], rec2[1], rec2[2] + a] != rec[:3]
    assert lost >= 35
