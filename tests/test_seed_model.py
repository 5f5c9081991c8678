"""CPU tier of k-mer seeding: the model tests/seed_ref.py (a dictionary of k-mer keys) equals its own brute force (every (i, j)
compared letter by letter, no keys) on random tiny sets with Ns, lower case, U, sequences shorter than k and palindromic k-mers; and
the pigeonhole property the end-to-end GPU test relies on holds in the model."""
import numpy as np
import pytest

import seed_ref as ref


def _same(a, b):
    for key in ("row_off", "pairs", "strand", "seeds"):
        assert a[key].tobytes() == b[key].tobytes(), key


def _tiny(rng, n, lo, hi, letters=b"ACGT"):
    al = np.frombuffer(letters, dtype=np.uint8)
    return [al[rng.integers(0, len(al), size=int(rng.integers(lo, hi + 1)))].tobytes() for _ in range(n)]


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_brute_force(seed):
    rng = np.random.default_rng(4000 + seed)
    k = 8
    refs = _tiny(rng, 3, 0, 60, b"ACGTacgtUN") + [b"ACG", b"ACGTACG", b""]                  # (shorter than k, empty)
    pal = b"ACGTACGT"                                                                       # its own reverse complement
    refs.append(b"TT" + pal + b"GG" + pal)
    qs = _tiny(rng, 2, 5, 30, b"ACGTacgtUN")
    qs += [refs[0][3:25], ref.orient(refs[1][0:20], 1), pal, b"ACGTAC", b"", refs[-1][1:14].lower().replace(b"t", b"u")]
    for mode in (ref.FORWARD, ref.REVERSE, ref.BOTH):
        for max_occ, min_seeds, band, pad in ((64, 1, 0, 0), (1, 2, 3, 5), (2, 1, 1, 16)):
            a = ref.seed(qs, refs, k, mode, min_seeds, band, pad, max_occ)
            b = ref.seed(qs, refs, k, mode, min_seeds, band, pad, max_occ, match_fn=ref.brute_matches(refs, k, max_occ))
            _same(a, b)
    assert len(ref.seed(qs, refs, k, ref.BOTH, 1, 0, 0, 64)["pairs"]) > 0


def test_letters_keys_and_order():
    assert ref.kmers(b"ACGTUacgtu", 10) == [(0, int("0123301233", 4))]
    assert ref.kmers(b"ACGNACGT", 4) == [(4, int("0123", 4))]
    assert ref.kmers(b"ACG", 4) == []
    assert ref.orient(b"AACGN", 1) == b"NCGTT" and ref.orient(b"acgu", 1) == b"acgt"
    e = ref.index_entries([b"TTTTACGT", b"ACGTAAAA"], 4)
    assert e == sorted(e) and e[0] == (0, 1, 4) and e[-1] == (255, 0, 0)
    assert [(r, j) for key, r, j in e if key == int("0123", 4)] == [(0, 4), (1, 0)]        # ties in (seq, pos) order
    assert ref.clusters([5, 1, 2, 9, 4], 1) == [(2, 1, 2), (2, 4, 5), (1, 9, 9)]
    assert ref.clusters([3, 3, 3], 0) == [(3, 3, 3)] and ref.clusters([], 4) == []


def test_windows_clamp_and_order():
    refs = [b"G" * 5 + b"ACGTTGCAAT" + b"G" * 5, b"ACGTTGCAAT"]
    q = b"CCACGTTGCAATCC"                                                                   # the core at 2: diagonals 3 and -2
    w = ref.seed([q], refs, 8, ref.FORWARD, 1, 0, 4, 64)
    assert w["row_off"].tolist() == [0, 2]
    assert [tuple(p) for p in w["pairs"]] == [(0, 0, 0, -1, 0, 20), (0, 1, 0, -1, 0, 10)]   # clamped at 0 and at len(r)
    assert [tuple(s) for s in w["seeds"]] == [(3, 3, 3, 0), (3, -2, -2, 0)]
    assert ref.seed([q], refs, 8, ref.FORWARD, 4, 0, 4, 64)["row_off"].tolist() == [0, 0]   # min_seeds above the cluster
    assert ref.seed([q], refs, 8, ref.FORWARD, 1, 0, 4, 64, max_qlen=13)["row_off"].tolist() == [0, 0]


def test_pigeonhole_property_in_the_model():
    """A read of 100 letters with at most 3 substitutions has an error-free run of at least 24 = ceil((100 - 3) / 4) letters, a run
    of n >= 12 letters holds n - 11 consecutive 12-mers on the true diagonal, so with band 0 the true diagonal's cluster has at least
    13 matches -- when no 12-mer of the reference is above max_occ."""
    rng = np.random.default_rng(77)
    al = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = al[rng.integers(0, 4, size=3000)].tobytes()
    idx = ref.index_dict([genome], 12)
    assert max(len(v) for v in idx.values()) <= 64
    for trial in range(40):
        pos = int(rng.integers(0, len(genome) - 100))
        read = bytearray(genome[pos:pos + 100])
        errs = sorted(rng.choice(100, size=int(rng.integers(0, 4)), replace=False).tolist())
        if trial == 0:
            errs = [24, 49, 74]                                                             # the worst case: runs of 24, 24, 24, 25
        for e in errs:
            read[e] = b"ACGT"[(b"ACGT".index(read[e]) + 1) % 4]
        assert ref.longest_clean_run(100, errs) >= 24
        strand = trial & 1
        stored = ref.orient(bytes(read), strand)                                            # strand 1: the read is stored reverse-complemented
        w = ref.seed([stored], [genome], 12, ref.BOTH, 13, 0, 0, 64)
        ok = [x for x in range(len(w["pairs"])) if w["strand"][x] == strand and w["seeds"][x]["diag_min"] <= pos <= w["seeds"][x]["diag_max"]]
        assert ok and w["seeds"][ok[0]]["n_seeds"] >= 13, trial
