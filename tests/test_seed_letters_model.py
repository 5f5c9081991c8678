"""CPU tier of protein seeding: the model tests/seed_letters_ref.py (keys from a table, a dictionary of them) equals its own brute force
(group letters compared position by position, no keys) in every query mode and with three alphabets; hand-written cases for the
edges of the translation; and the codon modes' reason worked by hand: a read with one nucleotide deleted is two candidates in the
frame modes and one in the codon modes."""
import numpy as np
import pytest

import seed_letters_ref as ref
import translate_ref as tr

T20, T11 = ref.table_of(ref.AA20), ref.table_of(ref.AA11)
T3 = ref.table_of(["AVLIM", "FWY", "ST", "NQ", "DE", "KRH", "G", "P"])                       # 8 groups: 3 bits; C is invalid


def _same(a, b):
    for key in ("row_off", "pairs", "byte", "seeds"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_alphabets_and_keys():
    assert ref.bits_of(T20) == 5 and ref.bits_of(T11) == 4 and ref.bits_of(T3) == 3 and ref.bits_of(ref.table_of(["A", "C"])) == 1
    for t in (T20, T11):
        assert all(t[ord(c)] == 255 for c in "*XBZJOUxbz-") and (t != 255).sum() == 40
    assert [int(T20[ord(c)]) for c in "ACDEFGHIKLMNPQRSTVWY"] == list(range(20)) and T20[ord("y")] == 19
    assert [int(T11[ord(c)]) for c in "KREDQNCGHILVMFYWPSTA"] == [0] * 6 + [1, 2, 3, 4, 4, 4, 5, 6, 7, 8, 9, 10, 10, 10]
    assert ref.kmers(b"ACD", 3, T20) == [(0, (0 << 10) | (1 << 5) | 2)]
    assert ref.kmers(b"KcXilV", 2, T11) == [(0, 0x01), (3, 0x44), (4, 0x44)]                  # X breaks the k-mers at 1 and 2
    assert ref.kmers(b"AC", 3, T20) == [] and ref.empty_key(3, T11) == 1 << 12
    e = ref.index_entries([b"LLKC", b"IVR"], 2, T11)
    assert e == sorted(e) and [(r, j) for key, r, j in e if key == 0x44] == [(0, 0), (1, 0)]  # L L and I V: one key, (seq, pos) order
    assert e[0] == (0x01, 0, 2)


@pytest.mark.parametrize("name,table", [("aa20", T20), ("aa11", T11), ("custom3", T3)])
def test_model_equals_brute_force(name, table):
    rng = np.random.default_rng(5100 + len(name))
    k = 3
    prots = [ref.random_protein(rng, int(rng.integers(40, 81))) for _ in range(12)]
    prots[3] = prots[3][:20] + b"X*" + prots[3][22:]
    reads = []
    for x in range(30):
        p = prots[int(rng.integers(12))]
        a = int(rng.integers(0, len(p) - 12))
        nt = ref.back_translate(p[a:a + int(rng.integers(8, 20))].replace(b"X", b"A").replace(b"*", b"A"), rng)
        nt = b"ACGTN"[int(rng.integers(5)):][:int(rng.integers(3))] + nt                     # a frame offset of 0 .. 2
        if x % 3 == 1:
            nt = ref.revcomp(nt)
        if x % 5 == 2:
            nt = nt.lower().replace(b"t", b"u")
        if x % 7 == 3:
            nt = nt[:10] + b"N" + nt[11:]
        reads.append(nt)
    reads += [b"", b"AC", b"ACG"]
    brute = ref.brute_matches(prots, k, table, 3)
    total = 0
    for mode in ref.MODES:
        queries = prots[:6] + [b"", b"AC"] if mode == ref.QUERY_LETTERS else reads
        for max_occ, min_seeds, band, pad in ((3, 2, 4, 5),):
            a = ref.seed(queries, prots, k, table, mode, min_seeds, band, pad, max_occ)
            b = ref.seed(queries, prots, k, table, mode, min_seeds, band, pad, max_occ, matcher=brute)
            _same(a, b)
            total += len(a["pairs"])
    assert total > 0
    a = ref.seed(reads, prots, k, table, tr.FRAMES_ALL, 1, 0, 0, 64)
    _same(a, ref.seed(reads, prots, k, table, tr.FRAMES_ALL, 1, 0, 0, 64, matcher=ref.brute_matches(prots, k, table, 64)))


def test_translation_edges():
    k = 3
    prot = b"MKWFPHCYG"                                                                      # one letter per aa11 group, mostly
    refs = [prot]
    nt = b"ATGAAATGGTTTCCACATTGTTATGGA"                                                      # M K W F P H C Y G
    assert tr.translate(nt, 0) == prot
    for off in (0, 1, 2):
        exact = b"C" * off + nt[:3 * k]                                                      # W = 3 k + off: exactly one k-mer in frame off
        w = ref.seed([exact, exact[:-1]], refs, k, T11, off, 1, 0, 0, 64)
        assert w["row_off"].tolist() == [0, 1, 1] and w["byte"].tolist() == [off]            # one nucleotide less: none
        assert tuple(w["seeds"][0]) == (1, 0, 0, 0) and tuple(w["pairs"][0]) == (0, 0, 0, -1, 0, 3)
    assert ref.seed([b"", b"A", b"AT"], refs, k, T11, tr.FRAMES_ALL, 1, 0, 0, 64)["row_off"].tolist() == [0, 0, 0, 0]   # W < 3
    assert ref.seed([b"AT"], refs, k, T11, ref.CODONS_BOTH, 1, 0, 0, 64)["row_off"].tolist() == [0, 0]
    # a stop codon and an N inside a k-mer: the k-mers over them are gone, those beside them stay
    stop = nt[:9] + b"TAA" + nt[12:]
    assert tr.translate(stop, 0) == b"MKW*PHCYG"
    w = ref.seed([stop], refs, k, T11, 0, 1, 0, 0, 64)
    assert [tuple(s) for s in w["seeds"]] == [(4, 0, 0, 0)]                                  # k-mers at 0, 4, 5, 6 of 7
    withn = nt[:10] + b"N" + nt[11:]
    assert tr.translate(withn, 0) == b"MKWXPHCYG"
    assert [tuple(s) for s in ref.seed([withn], refs, k, T11, 0, 1, 0, 0, 64)["seeds"]] == [(4, 0, 0, 0)]
    # lower case and U read as upper case and T
    low = nt.lower().replace(b"t", b"u")
    _same(ref.seed([low], refs, k, T11, tr.FRAMES_ALL, 1, 0, 0, 64), ref.seed([nt], refs, k, T11, tr.FRAMES_ALL, 1, 0, 0, 64))
    # a reverse frame: the stored read is the reverse complement with one byte in front of it once reversed (frame 4)
    stored = ref.revcomp(b"G" + nt)
    w = ref.seed([stored], refs, k, T11, tr.FRAMES_REVERSE, 1, 0, 0, 64)
    assert w["byte"].tolist() == [4] and tuple(w["seeds"][0]) == (7, 0, 0, 0)
    comp = {ord("A"): "T", ord("C"): "G", ord("G"): "C", ord("T"): "A"}
    for p in range(len(prot)):
        codon = "".join(comp[stored[x]] for x in tr.stored_bytes(0, len(stored), 4, p))     # read downwards, complemented
        assert codon.encode() == nt[3 * p:3 * p + 3]
    # max_qlen bounds W / 3 (letters mode: W)
    assert ref.seed([nt], refs, k, T11, 0, 1, 0, 0, 64, max_qlen=9)["row_off"].tolist() == [0, 1]
    assert ref.seed([nt], refs, k, T11, 0, 1, 0, 0, 64, max_qlen=8)["row_off"].tolist() == [0, 0]
    assert ref.seed([nt + b"AC"], refs, k, T11, 0, 1, 0, 0, 64, max_qlen=9)["row_off"].tolist() == [0, 1]      # W = 29: W / 3 = 9
    assert ref.seed([b"C" + nt + b"AC"], refs, k, T11, 1, 1, 0, 0, 64, max_qlen=9)["row_off"].tolist() == [0, 0]  # W / 3 = 10, L_1 = 9
    assert ref.seed([prot], refs, k, T11, ref.QUERY_LETTERS, 1, 0, 0, 64, max_qlen=8)["row_off"].tolist() == [0, 0]
    w = ref.seed([prot], refs, k, T11, ref.QUERY_LETTERS, 1, 0, 0, 64, max_qlen=9)
    assert w["byte"].tolist() == [0] and tuple(w["seeds"][0]) == (7, 0, 0, 0) and tuple(w["pairs"][0]) == (0, 0, 0, -1, 0, 9)
    # a custom genetic code: TGG reads as C instead of W, so the k-mers over letter 2 are gone
    code = bytearray(tr.CODE_STD)
    code[16 * 0 + 4 * 3 + 3] = ord("C")
    assert [tuple(s) for s in ref.seed([nt], refs, k, T11, 0, 1, 0, 0, 64, code=bytes(code))["seeds"]] == [(4, 0, 0, 0)]


def test_one_deleted_nucleotide_is_one_codon_candidate():
    """20 codons of a protein, the 31st nucleotide deleted: letters 0 .. 9 stay in frame 0 on letter diagonal 5, letters 11 .. 19 move
    to frame 2 (offset 2, one letter lost) on letter diagonal 6.  On nucleotide diagonals these are D = 15 and D = 3 * 6 - 2 = 16."""
    rng = np.random.default_rng(9)
    k = 3
    prot = b"ACDEFGHIKLMNPQRSTVWYADGKNRVCFI"                                                  # no 3-mer twice
    refs = [prot, ref.random_protein(rng, 40)]
    nt = ref.back_translate(prot[5:25], rng)
    read = nt[:30] + nt[31:]
    args = dict(min_seeds=2, band=2, pad=4, max_occ=64)
    fr = ref.seed([read], refs, k, T20, tr.FRAMES_FORWARD, **args)
    co = ref.seed([read], refs, k, T20, ref.CODONS_FORWARD, **args)
    assert fr["row_off"].tolist() == [0, 2] and fr["byte"].tolist() == [0, 2]
    assert [tuple(s)[1:3] for s in fr["seeds"]] == [(5, 5), (6, 6)]
    assert co["row_off"].tolist() == [0, 1] and co["byte"].tolist() == [0]
    n, dmin, dmax, _ = (int(v) for v in co["seeds"][0])
    assert n == int(fr["seeds"]["n_seeds"].sum()) and (dmin, dmax) == (15, 16) and dmax - dmin == 1
    # the window: floor(15 / 3) - 4 = 1 .. floor((16 + 59 - 1) / 3) + 1 + 4 = 29, inside the 30 letters
    assert tuple(co["pairs"][0]) == (0, 0, 0, -1, 1, 28)
    # an intact read has one candidate either way, with the same seeds
    fr = ref.seed([nt], refs, k, T20, tr.FRAMES_FORWARD, **args)
    co = ref.seed([nt], refs, k, T20, ref.CODONS_FORWARD, **args)
    assert len(fr["pairs"]) == len(co["pairs"]) == 1 and fr["seeds"]["n_seeds"][0] == co["seeds"]["n_seeds"][0] == 18
    assert tuple(co["seeds"][0])[1:3] == (15, 15)


def test_floor_rule_at_a_negative_diagonal():
    """The read starts 2 codons and 1 nucleotide before the protein does: D = 3 * 0 - (1 + 3 * 2) = -7 for the protein's first letter,
    floor(-7 / 3) = -3 (truncation would give -2); r_beg is clipped to 0 with any pad below 3 and r_end counts from the same D."""
    assert [ref.floor3(a) for a in (-7, -6, -4, -3, -1, 0, 2, 3)] == [-3, -2, -2, -1, -1, 0, 0, 1]
    rng = np.random.default_rng(3)
    prot = b"MKWFPHCYGMFW"
    read = b"G" + b"CCCCCC" + ref.back_translate(prot[:8], rng)                                  # W = 31
    w = ref.seed([read], [prot], 3, T20, ref.CODONS_FORWARD, 1, 0, 0, 64)
    assert [tuple(s) for s in w["seeds"]] == [(6, -7, -7, 0)] and w["byte"].tolist() == [0]
    assert tuple(w["pairs"][0]) == (0, 0, 0, -1, 0, 8)                                           # floor((-7 + 30) / 3) + 1 = 8
    w = ref.seed([read], [prot], 3, T20, 1, 1, 0, 1, 64)                                         # the frame mode: d = -2, L = 10
    assert [tuple(s) for s in w["seeds"]] == [(6, -2, -2, 0)] and tuple(w["pairs"][0]) == (0, 0, 0, -1, 0, 9)
