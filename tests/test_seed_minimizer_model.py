"""CPU tier of minimizer seeding: the model tests/seed_minimizer_ref.py against itself and against tests/seed_ref.py -- window
enumeration equals the per-position rule the kernel uses, w = 1 is every k-mer, the guarantee at w + k - 1 shared letters (and a fixed
counter-example one letter below it), and the order `mix` is injective and is the library's."""
import os

import numpy as np

import seed_minimizer_ref as mref
import seed_ref as ref

DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rand(rng, n):
    return DNA[rng.integers(0, 4, size=n)].tobytes()


def _messy(rng, n):
    """random letters with N's, lower case, U and repeats of period 1 .. 3 pasted in: ties and invalid positions"""
    s = bytearray(_rand(rng, n))
    for _ in range(int(rng.integers(0, 4))):
        if n == 0:
            break
        a = int(rng.integers(0, n))
        unit = _rand(rng, int(rng.integers(1, 4)))
        rep = (unit * (n // len(unit) + 1))[:int(rng.integers(1, 40))]
        s[a:a + len(rep)] = rep[:max(0, n - a)]
    for _ in range(int(rng.integers(0, 3))):
        if n:
            s[int(rng.integers(0, n))] = ord("N")
    if n and rng.integers(0, 4) == 0:
        a = int(rng.integers(0, n))
        s[a:a + 5] = bytes(s[a:a + 5]).lower().replace(b"t", b"u")
    return bytes(s[:n])


def test_window_enumeration_equals_the_per_position_rule():
    rng = np.random.default_rng(8100)
    some = 0
    for case in range(3000):
        k = int(rng.integers(8, 13))
        w = int(rng.choice([1, 2, 3, 5, 10, 19, 64]))
        seq = _messy(rng, int(rng.integers(0, 3 * (w + k))))
        got = mref.minimizers(seq, k, w)
        assert got == mref.minimizers_by_rule(seq, k, w), (seq, k, w)
        some += bool(got)
    assert some > 2000
    # hashes alone, small values: many ties and holes
    for case in range(3000):
        w = int(rng.integers(1, 9))
        h = [None if rng.integers(0, 5) == 0 else int(rng.integers(0, 4)) for _ in range(int(rng.integers(0, 40)))]
        assert mref.minimizers_of_hashes(h, w) == mref.minimizers_by_rule_of_hashes(h, w), (h, w)


def test_w_1_is_every_kmer():
    rng = np.random.default_rng(8101)
    for case in range(200):
        k = int(rng.integers(8, 32))
        seq = _messy(rng, int(rng.integers(0, 200)))
        assert mref.minimizers(seq, k, 1) == [p for p, _ in ref.kmers(seq, k)]
    refs = [_messy(rng, 300) for _ in range(5)]
    assert mref.index_entries(refs, 11, 1) == ref.index_entries(refs, 11)


def test_ties_pick_the_leftmost_in_oriented_order():
    k, w = 8, 5
    seq = b"A" * 30                                         # every k-mer equal: each window selects its first position
    nk = len(seq) - k + 1
    assert mref.minimizers(seq, k, w) == list(range(nk - w + 1))
    # strand 1 of poly-A is poly-T, read in oriented coordinates: again the first positions, not the last
    assert mref.minimizers(ref.orient(seq, 1), k, w) == list(range(nk - w + 1))
    short = b"ACACACACAC"                                   # nk = 3 < w: one window, one minimizer
    assert len(mref.minimizers(short, k, w)) == 1


def _shared(a, i, b, j, k, w, length):
    """a minimizer of a in [i, i + length - k] whose counterpart in b is one too"""
    ma, mb = set(mref.minimizers(a, k, w)), set(mref.minimizers(b, k, w))
    return [p for p in range(i, i + length - k + 1) if p in ma and p - i + j in mb]


def _planted(rng, k, w, length):
    """two sequences that share exactly `length` letters at (i, j) and differ in the letters next to the stretch"""
    core = _rand(rng, length)
    la, lb, ra, rb = (int(rng.integers(w + k, 3 * (w + k))) for _ in range(4))
    a = bytearray(_rand(rng, la) + core + _rand(rng, ra))
    b = bytearray(_rand(rng, lb) + core + _rand(rng, rb))
    for x, y in ((la - 1, lb - 1), (la + length, lb + length)):
        while a[x] == b[y]:
            b[y] = DNA[rng.integers(0, 4)]
    return bytes(a), la, bytes(b), lb


def test_the_guarantee_at_w_plus_k_minus_1_letters():
    rng = np.random.default_rng(8102)
    for case in range(600):
        k = int(rng.integers(8, 16))
        w = int(rng.choice([1, 2, 3, 5, 10, 19]))
        a, i, b, j = _planted(rng, k, w, w + k - 1)
        assert _shared(a, i, b, j, k, w, w + k - 1), (a, i, b, j, k, w)


# found by search over _planted(default_rng(seed), 8, 5, w + k - 2), seed 5: the stretch holds w - 1 k-mers, a window of either sequence takes one
# k-mer from outside it, and the two outside k-mers beat the shared ones on one side only
COUNTER = (b"AAAATAGTACCCTATTTACGCGGTATCGGCTACGGATGTCCTAACGATCAGTTTCA", 22, b"TGTAAGCCTAGCCTACAACGGCATTAAGTATCGGCTACCATGGCGTATACTTAT", 27)


def test_the_guarantee_need_not_hold_one_letter_below():
    k, w = 8, 5
    a, i, b, j = COUNTER
    length = w + k - 2
    assert a[i:i + length] == b[j:j + length] and a[i - 1] != b[j - 1] and a[i + length] != b[j + length]
    assert len(a) - k + 1 >= w and len(b) - k + 1 >= w
    assert not _shared(a, i, b, j, k, w, length)


def test_mix_is_injective_and_the_librarys(pkg):
    rng = np.random.default_rng(8103)
    k = 8
    keys = np.arange(4 ** k, dtype=np.uint64)                                     # all keys of k = 8, vectorised
    m = np.uint64(4 ** k - 1)
    h = (keys ^ np.uint64(mref.MIX_XOR)) & m
    h = (h * np.uint64(mref.MIX_MUL1)) & m
    h ^= h >> np.uint64(k)
    h = (h * np.uint64(mref.MIX_MUL2)) & m
    h ^= h >> np.uint64(k)
    assert len(np.unique(h)) == 4 ** k and int(h.max()) == 4 ** k - 1
    for key in rng.integers(0, 4 ** k, size=200).tolist():
        assert int(h[key]) == mref.mix(key, k)
    for k in (8, 15, 16, 31):
        sample = {int(x) for x in rng.integers(0, 4 ** k, size=20000)} | {0, 4 ** k - 1}
        assert len({mref.mix(key, k) for key in sample}) == len(sample)
        assert all(mref.mix(key, k) < 4 ** k for key in list(sample)[:1000])
        for key in list(sample)[:300]:
            assert pkg.seed_mix(key, k) == mref.mix(key, k)
    assert mref.mix(0, 15) != 0                                                 # poly-A is not the minimum everywhere
    assert pkg.seed_mix(5, 7) == 0 and pkg.seed_mix(5, 32) == 0
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "parasail_amd.h")).read()
    for name, value in (("PMX_SEED_MIX_XOR", mref.MIX_XOR), ("PMX_SEED_MIX_MUL1", mref.MIX_MUL1), ("PMX_SEED_MIX_MUL2", mref.MIX_MUL2)):
        assert "#define %s" % name in text and ("0x%016X" % value) in text
