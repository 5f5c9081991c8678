"""CPU tier of seeding translated references: the model tests/seed_translated_ref.py (keys from a table, a dictionary of them) equals
its own brute force (letter strings compared at every (p, s, r, x), no keys) in both modes, for the three strand modes and with two
alphabets; the frame mode equals seed_letters_ref over the host-translated six-frame protein set through the mapping; and the window
rules worked by hand: the strand-1 mapping, the codon-aligned window whose frame byte is 0 or 3 also where pad is clipped at either
sequence end, and the one-deleted-base case -- one codon candidate against two frame candidates."""
import numpy as np
import pytest

import seed_letters_ref as lref
import seed_translated_ref as ref
import translate_ref as tr

T20, T11 = ref.table_of(ref.AA20), ref.table_of(ref.AA11)
K = 3
NT = b"ATGAAATGGTTTCCACATTGTTATGGA"                                                          # M K W F P H C Y G
PROT = b"MKWFPHCYG"


def _same(a, b):
    for key in ("row_off", "pairs", "byte", "seeds"):
        assert a[key].tobytes() == b[key].tobytes(), key


def _random_nt(rng, n):
    return bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, size=n))


def _contigs(rng, prots):
    """sequences of length 0, 1, 2, 3, 3 k - 1 .. 3 k + 2, with an N, with stop codons, lower case with U, and contigs that carry a
    back-translated piece of a protein on either strand at every frame offset"""
    refs = [b"", b"A", b"AC", b"ACG"] + [NT[:n] for n in (3 * K - 1, 3 * K, 3 * K + 1, 3 * K + 2)]
    refs += [lref.revcomp(NT[:3 * K + 1]), NT[:10] + b"N" + NT[11:], NT[:9] + b"TAA" + NT[12:], NT.lower().replace(b"t", b"u")]
    for x in range(14):
        p = prots[x % len(prots)]
        a = int(rng.integers(0, len(p) - 14))
        gene = lref.back_translate(p[a:a + int(rng.integers(8, 15))], rng)
        contig = _random_nt(rng, x % 3 + int(rng.integers(0, 12))) + gene + b"TGA" + _random_nt(rng, int(rng.integers(0, 12)))
        refs.append(lref.revcomp(contig) if x % 2 else contig)
    return refs


def test_index_entries_by_hand():
    assert tr.translate(NT, 0) == PROT
    e = ref.index_entries([NT], K, T11, ref.FORWARD)
    assert [x for key, sr, x in e if x % 3 == 0] and sorted(x for key, sr, x in e if x % 3 == 0) == list(range(0, 21, 3))   # 7 3-mers of 9 letters
    assert all(sr == 0 for key, sr, x in e) and max(x for key, sr, x in e) <= len(NT) - 3 * K
    both = ref.index_entries([NT, lref.revcomp(NT)], K, T11, ref.BOTH)
    # sequence 1 on strand 1 reads as sequence 0 on strand 0: the same (key, x) under s * count + r = 3 and 0
    assert sorted((key, x) for key, sr, x in both if sr == 0) == sorted((key, x) for key, sr, x in both if sr == 3)
    assert sorted((key, x) for key, sr, x in both if sr == 1) == sorted((key, x) for key, sr, x in both if sr == 2)
    assert both == sorted(both) and ref.index_entries([NT, lref.revcomp(NT)], K, T11, ref.REVERSE) == [t for t in both if t[1] >= 2]
    # lengths 0 .. 3 k - 1 hold nothing; 3 k one k-mer, 3 k + 1 two (x = 0, 1), 3 k + 2 three
    for n, xs in ((0, []), (1, []), (2, []), (3, []), (3 * K - 1, []), (3 * K, [0]), (3 * K + 1, [0, 1]), (3 * K + 2, [0, 1, 2])):
        got = sorted(x for key, sr, x in ref.index_entries([(b"GCT" * 4)[:n]], K, T20, ref.FORWARD))   # A / L / C in the three frames
        assert got == xs, n
    # an N and a stop codon break exactly the k-mers over them, in the frame that reads them as one codon
    stop = NT[:9] + b"TAA" + NT[12:]
    assert sorted(x for key, sr, x in ref.index_entries([stop], K, T11, ref.FORWARD) if x % 3 == 0) == [0, 12, 15, 18]   # letter 3 is the stop: 3, 6, 9 are gone
    withn = NT[:10] + b"N" + NT[11:]
    assert all(not (x <= 10 < x + 3 * K) for key, sr, x in ref.index_entries([withn], K, T11, ref.FORWARD))
    # 'X' and '*' are invalid even where a table gives them a group
    loose = T11.copy()
    loose[ord("X")] = loose[ord("*")] = 0
    assert ref.index_entries([stop, withn], K, loose) == ref.index_entries([stop, withn], K, T11)


@pytest.mark.parametrize("name,table", [("aa20", T20), ("aa11", T11)])
@pytest.mark.parametrize("strand_mode", [ref.FORWARD, ref.REVERSE, ref.BOTH])
def test_model_equals_brute_force(name, table, strand_mode):
    rng = np.random.default_rng(5200 + len(name))
    prots = [lref.random_protein(rng, int(rng.integers(20, 41))) for _ in range(8)]
    refs = _contigs(rng, prots)
    queries = prots + [b"", b"MK", PROT, PROT.lower(), b"MKWXPHCYG", PROT * 6]
    brute = ref.brute_matches(refs, K, table, 3, strand_mode)
    total = 0
    for ref_mode, band in ((ref.REF_FRAMES, 2), (ref.REF_CODONS, 6)):
        a = ref.seed(queries, refs, K, table, ref_mode, strand_mode, 2, band, 5, 3, max_qlen=50)
        _same(a, ref.seed(queries, refs, K, table, ref_mode, strand_mode, 2, band, 5, 3, max_qlen=50, matcher=brute))
        assert a["row_off"][-1] == a["row_off"][-2]                                          # the row above max_qlen
        total += len(a["pairs"])
        assert set(a["byte"].tolist()) <= ({0, 3} if ref_mode == ref.REF_FRAMES else {0, 1})
    assert total > 0
    a = ref.seed(queries, refs, K, table, ref.REF_FRAMES, strand_mode, 1, 0, 0, 64)
    _same(a, ref.seed(queries, refs, K, table, ref.REF_FRAMES, strand_mode, 1, 0, 0, 64, matcher=ref.brute_matches(refs, K, table, 64, strand_mode)))


@pytest.mark.parametrize("strand_mode", [ref.FORWARD, ref.REVERSE, ref.BOTH])
def test_frame_mode_equals_letters_seeding_of_the_six_frame_set(strand_mode):
    rng = np.random.default_rng(5300)
    prots = [lref.random_protein(rng, int(rng.integers(20, 41))) for _ in range(8)]
    refs = _contigs(rng, prots)
    queries = prots + [b"", PROT, PROT.lower()]
    six = ref.r6(refs, strand_mode)
    assert len(six) == 6 * len(refs)
    # the index entries, by (kmer, then order): r' = g * count + r, j = x / 3
    count = len(refs)
    mine = ref.index_entries(refs, K, T11, strand_mode)
    theirs = lref.index_entries(six, K, T11)
    assert len(mine) == len(theirs) > 100
    assert sorted((key, (3 * (sr // count) + x % 3) * count + sr % count, x // 3) for key, sr, x in mine) == theirs
    for o in (dict(min_seeds=2, band=2, pad=5, max_occ=3), dict(min_seeds=1, band=0, pad=0, max_occ=64), dict(min_seeds=2, band=4, pad=40, max_occ=8)):
        a = ref.seed(queries, refs, K, T11, ref.REF_FRAMES, strand_mode, **o)
        b = lref.seed(queries, six, K, T11, lref.QUERY_LETTERS, **o)
        assert len(a["pairs"]) > 0
        _same(a, ref.from_letters(b, refs))


def test_windows_by_hand():
    """NT carries PROT from stored byte 4 of a 40-nt contig, so on strand 0 the gene lies in sequence frame 1 (x = 4 + 3 j) at letter
    diagonal d = 1, nucleotide diagonal D = 4; the reverse complement of the contig carries it on strand 1 at the same oriented
    coordinates."""
    contig = b"GGCC" + NT + b"CCGGCCGGC"
    N = len(contig)
    assert N == 40
    for s, stored in ((0, contig), (1, lref.revcomp(contig))):
        fr = ref.seed([PROT], [stored], K, T11, ref.REF_FRAMES, ref.BOTH, 2, 0, 2, 64)
        assert [tuple(v) for v in fr["seeds"]] == [(7, 1, 1, 3 * s + 1)] and fr["byte"].tolist() == [3 * s]
        # letters [max(0, 1 - 2), min(13, 1 + 9 + 2)) = [0, 12) of frame offset 1: oriented nucleotides [1, 37)
        assert tuple(fr["pairs"][0]) == ((0, 0, 0, -1, 1, 36) if s == 0 else (0, 0, 0, -1, N - 37, 36))
        beg, n = int(fr["pairs"][0]["r_beg"]), int(fr["pairs"][0]["r_len"])
        assert tr.translate(stored[beg:beg + n], 3 * s)[1:10] == PROT and n % 3 == 0          # byte 0 / 3 reads the window's frame
        co = ref.seed([PROT], [stored], K, T11, ref.REF_CODONS, ref.BOTH, 2, 0, 2, 64)
        assert [tuple(v) for v in co["seeds"]] == [(7, 4, 4, 0)] and co["byte"].tolist() == [s]
        # oriented [4 - 2, 4 + 27 + 2) = [2, 33)
        assert tuple(co["pairs"][0]) == ((0, 0, 0, -1, 2, 31) if s == 0 else (0, 0, 0, -1, N - 33, 31))
    # pad clipped at both sequence ends: the whole frame, still codon-aligned -- frame offset 1 of 40 nt has 13 letters, [1, 40)
    for s, stored in ((0, contig), (1, lref.revcomp(contig))):
        fr = ref.seed([PROT], [stored], K, T11, ref.REF_FRAMES, ref.BOTH, 2, 0, 100, 64)
        assert tuple(fr["pairs"][0]) == ((0, 0, 0, -1, 1, 39) if s == 0 else (0, 0, 0, -1, 0, 39)) and fr["byte"].tolist() == [3 * s]
        beg, n = int(fr["pairs"][0]["r_beg"]), int(fr["pairs"][0]["r_len"])
        assert tr.translate(stored[beg:beg + n], 3 * s) == tr.translate(stored, 3 * s + 1)    # the window's frame 0 / 3 is the sequence frame
        co = ref.seed([PROT], [stored], K, T11, ref.REF_CODONS, ref.BOTH, 2, 0, 100, 64)
        assert tuple(co["pairs"][0]) == (0, 0, 0, -1, 0, 40)
    # clipped at one end only: a lead of 2 (frame offset 2, d = 0) and pad 1 -> letters [0, 10), stored [2, 32); strand 1: [N - 32, N - 2)
    short = b"GG" + NT + b"CCGGC"
    for s, stored in ((0, short), (1, lref.revcomp(short))):
        fr = ref.seed([PROT], [stored], K, T11, ref.REF_FRAMES, ref.BOTH, 2, 0, 1, 64)
        assert [tuple(v) for v in fr["seeds"]] == [(7, 0, 0, 3 * s + 2)]
        assert tuple(fr["pairs"][0]) == ((0, 0, 0, -1, 2, 30) if s == 0 else (0, 0, 0, -1, len(short) - 32, 30))
    # a strand that the index does not hold gives nothing
    assert len(ref.seed([PROT], [contig], K, T11, ref.REF_FRAMES, ref.REVERSE, 1, 0, 0, 64)["pairs"]) == 0
    assert len(ref.seed([PROT], [lref.revcomp(contig)], K, T11, ref.REF_CODONS, ref.FORWARD, 1, 0, 0, 64)["pairs"]) == 0


@pytest.mark.parametrize("s", [0, 1])
def test_one_deleted_base_is_one_codon_candidate(s):
    """30 codons of a gene from oriented byte 6 of the contig, each letter's first codon, the gene's 46th nucleotide deleted -- the T
    that opens codon 15 (TCT) behind codon 14 (CGT), so the codon read across the gap is TCT again: letters 0 .. 14 stay in sequence
    frame 0 on letter diagonal 2 (D = 6, 13 3-mers), letters 15 .. 29 move to frame offset 2 on letter diagonal 1 (D = 5, 13 3-mers)."""
    prot = b"ACDEFGHIKLMNPQRSTVWYADGKNRVCFI"                                                  # no 3-mer twice
    gene = "".join(lref._BACK[c][0] for c in prot).encode()
    assert gene[42:48] == b"CGTTCT" and tr.translate(gene, 0) == prot
    contig = b"GGCCGG" + gene[:45] + gene[46:] + b"CCGGCCGG"
    stored = lref.revcomp(contig) if s else contig
    N = len(stored)
    args = dict(min_seeds=2, band=2, pad=4, max_occ=64)
    fr = ref.seed([prot], [stored], K, T20, ref.REF_FRAMES, ref.BOTH, **args)
    co = ref.seed([prot], [stored], K, T20, ref.REF_CODONS, ref.BOTH, **args)
    assert [tuple(v) for v in fr["seeds"]] == [(13, 2, 2, 3 * s), (13, 1, 1, 3 * s + 2)] and fr["byte"].tolist() == [3 * s, 3 * s]
    assert [tuple(v) for v in co["seeds"]] == [(26, 5, 6, 0)] and co["byte"].tolist() == [s]
    # oriented [5 - 4, 6 + 90 + 4) = [1, 100), clipped to the contig's 103
    lo, hi = 1, 100
    assert N == 103 and tuple(co["pairs"][0]) == ((0, 0, 0, -1, lo, hi - lo) if s == 0 else (0, 0, 0, -1, N - hi, hi - lo))
    beg, n = int(co["pairs"][0]["r_beg"]), int(co["pairs"][0]["r_len"])
    window = stored[beg:beg + n] if s == 0 else lref.revcomp(stored[beg:beg + n])
    assert gene[:45] + gene[46:] in window                                                    # it covers the whole gene
    # the intact gene is one candidate either way, with the same seeds
    whole = b"GGCCGG" + gene + b"CCGGCCGG"
    whole = lref.revcomp(whole) if s else whole
    fr = ref.seed([prot], [whole], K, T20, ref.REF_FRAMES, ref.BOTH, **args)
    co = ref.seed([prot], [whole], K, T20, ref.REF_CODONS, ref.BOTH, **args)
    assert [tuple(v) for v in fr["seeds"]] == [(28, 2, 2, 3 * s)] and [tuple(v) for v in co["seeds"]] == [(28, 6, 6, 0)]
