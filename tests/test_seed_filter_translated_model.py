"""CPU tier of the ungapped filter for the codon and translated-index lists: the model tests/seed_filter_translated_ref.py against
independent restatements -- a codon list's diagonal is a letter diagonal of one query frame (seed_filter_ref, kind "frame"), a
translated index's lists are letter lists over the host-translated six-frame set R6 (kind "strand"), the ungapped score never exceeds
the frameshift models' score and equals it when no gap and no shift can be paid -- and the three roads end to end on the seeding
models' lists, where the planted candidate has to be the survivor before the GPU tier is allowed to rely on it."""
import numpy as np
import pytest

import frameshift_ref
import frameshift_ref_side
import seed_filter_ref as plain
import seed_filter_translated_lists as lists
import seed_filter_translated_ref as ref
import seed_translated_ref
import translate_ref as tr
from pairs_ex_ref import revcomp
from util import golden

AA = b"ACDEFGHIKLMNPQRSTVWY*X"


@pytest.fixture(scope="module")
def b62(orc):
    om = orc.Matrix.from_file(golden("blosum62.txt"))
    return om, np.asarray(om.scores).reshape(om.size, om.size), om.mapper


def _prot(rng, n):
    return bytes(AA[int(v)] for v in rng.integers(0, len(AA), size=n))


def _nt(rng, n):
    return bytes(b"ACGTN"[int(v)] for v in rng.integers(0, 5, size=n)) if rng.random() < 0.2 else lists.dna(rng, n)


def _one(kind, qs, rs, row, byte, lo, hi, scores, mapper, g=0, **kw):
    pairs = ref.pairs_ref.pairs_array([row])
    return tuple(int(v) for v in ref.ungapped(qs, rs, pairs, np.array([byte], dtype=np.uint8), lists.seeds_array([(lo, hi, g)]), scores, mapper, kind, **kw)[0])


def test_codons_diagonal_is_a_letter_diagonal_of_one_frame(b62):
    """every nucleotide diagonal D of small random windows, both strands, clipped reference windows: frame 3 s + off with off = (-D)
    mod 3, letter diagonal (D + off) / 3; and a span's record is the first best of its diagonals"""
    _, scores, mapper = b62
    rng = np.random.default_rng(9500)
    positive = empty = 0
    for _ in range(200):
        W, n = int(rng.integers(3, 24)), int(rng.integers(1, 12))
        read, prot = lists.dna(rng, W), _prot(rng, n)
        if rng.random() < 0.5:                                                               # a read that holds the protein somewhere
            read = (lists.dna(rng, int(rng.integers(0, 3))) + lists.back_translate(bytes(c for c in prot if c in lists.AA), rng) + b"ACGT")[:W + 3]
        r_beg = int(rng.integers(0, n))
        r_len = int(rng.integers(1, n - r_beg + 1))
        s = int(rng.integers(0, 2))
        row = (0, 0, 0, -1, r_beg, r_len)
        per = {}
        for D in range(3 * r_beg - len(read) - 2, 3 * (r_beg + r_len) + 3):
            got = _one("codons", [read], [prot], row, s, D, D, scores, mapper)
            off = (-D) % 3
            d = (D + off) // 3
            want = plain.ungapped([read], [prot], ref.pairs_ref.pairs_array([row]), np.array([3 * s + off], dtype=np.uint8),
                                  lists.seeds_array([(d, d, 0)]), scores, mapper, kind="frame")[0]
            if want["score"] == -1:                                                          # the frame holds no codon: no cell on D
                assert tr.tlen(len(read), off) == 0 and got == (0, D, -1, -1)
                empty += 1
            elif want["score"] == 0:
                assert got == (0, D, -1, -1)
            else:
                assert got == (int(want["score"]), 3 * int(want["diag"]) - off, off + 3 * int(want["end_query"]) + 2, int(want["end_ref"])), (read, prot, row, s, D)
                positive += 1
            per[D] = got
        for _ in range(6):
            lo = int(rng.integers(min(per), max(per) + 1))
            hi = min(max(per), lo + int(rng.integers(0, 12)))
            best = max(per[D][0] for D in range(lo, hi + 1))
            first = next(per[D] for D in range(lo, hi + 1) if per[D][0] == best) if best > 0 else (0, lo, -1, -1)
            assert _one("codons", [read], [prot], row, s, lo, hi, scores, mapper) == first
    assert positive > 500 and empty > 0


def test_ref_frames_records_are_letter_records_over_r6(b62):
    """both strands, every g: r' -> (g, r), the stored window mapped back to the letters [lb, le) of the frame's whole translation"""
    _, scores, mapper = b62
    rng = np.random.default_rng(9501)
    contigs = [_nt(rng, int(rng.integers(30, 70))) for _ in range(4)]
    r6 = seed_translated_ref.r6(contigs)
    seen, positive = set(), 0
    for _ in range(300):
        r, g = int(rng.integers(4)), int(rng.integers(6))
        N, off, s = len(contigs[r]), g % 3, g // 3
        Lg = (N - off) // 3
        lb = int(rng.integers(0, Lg))
        le = int(rng.integers(lb + 1, Lg + 1))
        beg, end = (off + 3 * lb, off + 3 * le) if s == 0 else (N - off - 3 * le, N - off - 3 * lb)
        q = _prot(rng, int(rng.integers(1, 14)))
        if rng.random() < 0.5:
            a = int(rng.integers(lb, le))
            q = r6[g * 4 + r][a:a + len(q)] or q
        lo = int(rng.integers(lb - len(q) - 1, le + 1))
        hi = lo + int(rng.integers(0, 6))
        got = _one("ref_frames", [q], contigs, (0, r, 0, -1, beg, end - beg), 3 * s, lo, hi, scores, mapper, g=g)
        want = plain.ungapped([q], r6, ref.pairs_ref.pairs_array([(0, g * 4 + r, 0, -1, lb, le - lb)]), None, lists.seeds_array([(lo, hi, 0)]), scores, mapper)[0]
        assert got == tuple(int(v) for v in want), (q, r, g, lb, le, lo, hi)
        seen.add(g)
        positive += got[0] > 0
        # a window that is not codon-aligned for g, g of the other strand, a byte that is no window frame
        for shift in (1, 2):
            if beg + shift + (end - beg) <= N:
                assert _one("ref_frames", [q], contigs, (0, r, 0, -1, beg + shift, end - beg), 3 * s, lo, hi, scores, mapper, g=g) == ref.BAD
        assert _one("ref_frames", [q], contigs, (0, r, 0, -1, beg, end - beg), 3 * s, lo, hi, scores, mapper, g=(g + 3) % 6) == ref.BAD
        assert _one("ref_frames", [q], contigs, (0, r, 0, -1, beg, end - beg), 3 * s + 1, lo, hi, scores, mapper, g=g) == ref.BAD
        assert _one("ref_frames", [q], contigs, (0, r, 0, -1, beg, end - beg), 3 * s, hi + 1, hi, scores, mapper, g=g) == ref.BAD
    assert seen == set(range(6)) and positive > 100
    assert ref.frame_origin(30, 4, 9, 0, 1) == 1 and ref.frame_origin(30, 4, 9, 0, 0) is None and ref.frame_origin(30, 4, 9, 0, 6) is None
    assert ref.frame_origin(30, 0, 9, 0, 1) is None                                          # r_beg in front of the frame's first codon
    assert ref.frame_origin(30, 4, 9, 3, 5) == 5 and ref.frame_origin(30, 4, 9, 3, 4) is None and ref.frame_origin(30, 4, 9, 3, 2) is None


def test_ref_codons_diagonal_is_a_letter_diagonal_of_one_sequence_frame(b62):
    """every D: the letters-kind record over frame g = 3 s + D mod 3 of R6, on the letter window the nucleotide window covers; and, the
    matrix being symmetric, the score of the CODONS model with the sides exchanged and D -> -D"""
    _, scores, mapper = b62
    assert (scores == scores.T).all()
    rng = np.random.default_rng(9502)
    contigs = [_nt(rng, int(rng.integers(12, 50))) for _ in range(4)]
    r6 = seed_translated_ref.r6(contigs)
    positive = nowin = 0
    for _ in range(100):
        r, s = int(rng.integers(4)), int(rng.integers(2))
        N = len(contigs[r])
        lo = int(rng.integers(0, N - 2))
        hi = int(rng.integers(lo + 3, N + 1))
        beg = lo if s == 0 else N - hi
        q = _prot(rng, int(rng.integers(1, 10)))
        oriented = contigs[r] if s == 0 else revcomp(contigs[r])
        if rng.random() < 0.5:
            f = int(rng.integers(3))
            q = tr.translate(oriented[lo:hi], f)[:len(q)] or q
        row = (0, r, 0, -1, beg, hi - lo)
        for D in range(lo - 3 * len(q) - 1, hi + 2):
            got = _one("ref_codons", [q], contigs, row, s, D, D, scores, mapper)
            off = D % 3
            g, d = 3 * s + off, (D - off) // 3
            jlo, jhi = -((off - lo) // 3), (hi - 3 - off) // 3                              # the codons x = off + 3 j with lo <= x <= hi - 3
            if jlo > jhi:
                assert got == (0, D, -1, -1)
                nowin += 1
                continue
            want = plain.ungapped([q], r6, ref.pairs_ref.pairs_array([(0, g * 4 + r, 0, -1, jlo, jhi - jlo + 1)]), None, lists.seeds_array([(d, d, 0)]),
                                  scores, mapper)[0]
            if want["score"] <= 0:
                assert want["score"] == 0 and got == (0, D, -1, -1)
            else:
                i, j = int(want["end_query"]), int(want["end_ref"])
                assert got == (int(want["score"]), D, i, off + 3 * j + 2), (q, row, s, D)
                positive += 1
            T = frameshift_ref_side.stream(oriented[lo:hi], 0)
            assert ref.codons_window(T, q, 0, lo - D, lo - D, scores, mapper)[0] == got[0]
    assert positive > 300 and nowin > 0


def test_ungapped_never_exceeds_the_frameshift_score_and_equals_it_without_gaps(b62):
    """U <= the three-frame DP's score under any penalties; with every diagonal of the window seeded and open, extend and frameshift
    that no score can pay, the two are equal"""
    om, scores, mapper = b62
    rng = np.random.default_rng(9503)
    NEVER = 1 << 20
    strict = 0
    for _ in range(120):
        prot = lists.random_protein(rng, int(rng.integers(1, 30)))
        nt = lists.back_translate(lists.mutate(rng, prot, 0.2), rng)
        if len(nt) > 12 and rng.random() < 0.5:
            nt = nt[:len(nt) // 2] + nt[len(nt) // 2 + 1:]                                   # one base deleted: a shift pays
        nt = lists.dna(rng, int(rng.integers(0, 4))) + nt + lists.dna(rng, int(rng.integers(2, 5)))
        s = int(rng.integers(2))
        T = frameshift_ref.codon_stream(nt, s)
        assert T == frameshift_ref_side.stream(nt, s)
        every = (-len(T), 3 * len(prot))
        for lo, hi in (every, (int(rng.integers(-5, 5)), int(rng.integers(5, 12)))):
            u = ref.codons_window(T, prot, 0, lo, hi, scores, mapper)[0]
            v = ref.ref_codons_window(prot, T, 0, -hi, -lo, scores, mapper)[0]
            gapped_q = frameshift_ref.align(T, prot, om, 11, 1, 15)[0]
            gapped_r = frameshift_ref_side.align(prot, T, om, 11, 1, 15)[0]
            assert u == v and u <= gapped_q and v <= gapped_r
            strict += u < gapped_q
            if (lo, hi) == every:
                assert u == frameshift_ref.align(T, prot, om, NEVER, NEVER, NEVER)[0]
                assert v == frameshift_ref_side.align(prot, T, om, NEVER, NEVER, NEVER)[0]
    assert strict > 20


def test_hand_built_lists_cover_what_they_claim(b62):
    """on the model's own result: every kind of record, every span and residue, both strands, clipped windows, ties"""
    _, scores, mapper = b62
    for kind, fn in (("codons", lists.codons_list), ("ref_codons", lists.ref_codons_list), ("ref_frames", lists.ref_frames_list)):
        L = fn()
        w = ref.ungapped(L.qs, L.refs, L.pairs, L.byte, L.seeds, scores, mapper, kind, max_qlen=L.max_qlen, max_rlen=L.max_rlen)
        bad = set(np.nonzero(w["score"] == -1)[0].tolist())
        assert bad == set(L.marks["bad"]) | set(L.marks.get("nostream", [])), kind
        assert all(tuple(w[k - 1]) == tuple(w[k + 1]) and w[k - 1]["score"] > 50 for k in L.marks["bad"]), kind
        spans = (L.seeds["diag_max"].astype(np.int64) - L.seeds["diag_min"] + 1).tolist()
        assert set(spans) >= set(lists.SPANS)
        assert all((w["score"][L.marks["span%d" % sp]] > 0).sum() >= 18 for sp in lists.SPANS), kind     # (a one-letter piece may mismatch)
        assert (w["score"][L.marks["span300"]] > 100).sum() >= 10                            # the planted diagonal is found inside 300
        assert all((w[x]["score"], w[x]["end_query"]) == (0, -1) for x in L.marks["nocell"]), kind
        assert (w["score"][L.marks["clipped"]] > 0).sum() > 10 and (w["score"][L.marks["whole"]] > 0).sum() >= 18
        a, b = L.marks["tie2"]
        assert w[a]["score"] == w[b]["score"] == 288 and w[a]["diag"] < w[b]["diag"]          # equal maxima on two diagonals: the lower one
        per = 24 if kind != "ref_frames" else 8
        assert w[b]["diag"] - w[a]["diag"] == per and L.seeds[a]["diag_min"] <= w[a]["diag"] < L.seeds[b]["diag_min"]
        t = L.marks["twice"][0]
        first = 19 if kind != "codons" else 3 * 19 + 2
        assert w[t]["score"] > 80 and w[t]["end_query"] == first, (kind, tuple(w[t]))          # twice on one diagonal: the first
        assert set(L.byte[np.nonzero(w["score"] > 0)[0]].tolist()) == ({0, 1} if kind != "ref_frames" else {0, 3})
        if kind != "ref_frames":
            lens = {len(L.qs[int(p["q"])]) % 3 for p in L.pairs[L.marks["residue"]]} if kind == "codons" else {int(p["r_len"]) % 3 for p in L.pairs[L.marks["residue"]]}
            assert lens == {0, 1, 2}
        if kind != "codons":                                                                 # strand 1: N != r_beg + r_len, the origin rule works
            s1 = [x for x in range(len(L.pairs)) if L.byte[x] in (1, 3) and w[x]["score"] > 100]
            assert sum(int(L.pairs[x]["r_beg"]) + int(L.pairs[x]["r_len"]) < len(L.refs[int(L.pairs[x]["r"])]) for x in s1) > 50
        else:
            assert tuple(w[L.marks["oneletter"][0]])[0] >= 0


# ---- the roads end to end, on the seeding models' lists ---------------------------------------------------------------------------------
def test_codon_road_on_the_model(b62):
    _, scores, mapper = b62
    prots, reads, planted, hits = lists.codon_world()
    assert len(hits["pairs"]) > 1.2 * lists.N_ROWS                                           # chance candidates beside the planted ones
    f, mine = lists.planted_survivors("codons", reads, prots, hits, planted, scores, mapper)
    # one base deleted: ONE candidate whose diagonals hold D (in front of the deletion) and D + 1 (behind it); its record is the
    # better of its two halves
    for q in list(planted)[:40]:
        x = mine[q]
        r, s, D = planted[q]
        assert hits["seeds"][x]["diag_min"] <= D and D + 1 <= hits["seeds"][x]["diag_max"], q
        halves = [_one("codons", reads, prots, tuple(hits["pairs"][x]), s, d, d, scores, mapper) for d in (D, D + 1)]
        rec = tuple(int(v) for v in f["all_ungapped"][x])
        assert rec == max(halves, key=lambda h: (h[0], -h[1])) and min(h[0] for h in halves) > 40, (q, rec, halves)
    assert (f["all_ungapped"]["score"] >= 0).all() and len(f["source"]) == sum(1 for q in range(len(reads)) if len(lists.rows_of(hits, q)))


def test_tblastn_roads_on_the_model(b62):
    _, scores, mapper = b62
    prots, whole, planted = lists.tblastn_world(cut=False)
    hits = lists.tblastn_hits(prots, whole, seed_translated_ref.REF_FRAMES)
    assert len(hits["pairs"]) > 1.2 * lists.N_ROWS and set(hits["seeds"]["reserved"].tolist()) == set(range(6))
    lists.planted_survivors("ref_frames", prots, whole, hits, planted, scores, mapper)
    prots, cut, planted = lists.tblastn_world(cut=True)
    hits = lists.tblastn_hits(prots, cut, seed_translated_ref.REF_CODONS)
    f, mine = lists.planted_survivors("ref_codons", prots, cut, hits, planted, scores, mapper)
    for q in list(planted)[:40]:                                                             # behind the deleted nucleotide the gene lies on D - 1
        x = mine[q]
        r, s, D = planted[q]
        assert hits["seeds"][x]["diag_min"] <= D - 1 and D <= hits["seeds"][x]["diag_max"], q
        halves = [_one("ref_codons", prots, cut, tuple(hits["pairs"][x]), s, d, d, scores, mapper) for d in (D - 1, D)]
        rec = tuple(int(v) for v in f["all_ungapped"][x])
        assert rec == max(halves, key=lambda h: (h[0], -h[1])) and min(h[0] for h in halves) > 40, (q, rec, halves)
