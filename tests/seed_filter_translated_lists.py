"""Inputs shared by the CPU and the GPU tier of the translated ungapped filter (tests/test_seed_filter_translated_model.py,
tests/test_gpu_seed_filter_translated.py): hand-built candidate lists of the three list kinds that reach every place where the
kernel's shape changes, and three small planted worlds for the roads end to end.  Everything is a pure function of its generator
seed; nothing here reads the library.

The kernel's shape: G = 16 lanes per candidate that divide themselves by the span -- here in NUCLEOTIDE
diagonals for the codon kinds --, pieces of whole s = 4-cell steps, cells counted in codons on a strided side.  So: cells per
diagonal 1 .. 9 (heads and tails of a step, every alignment of the ten bytes a strided step reads), G s - 1 .. G s + 1, the next two
piece boundaries and the longest the lists' maxima allow; W = 3 c + 2 + {0, 1, 2} on a codon side; spans 1, 2, G - 1, G, G + 1,
every span at which the lanes per diagonal change, and one of 300."""
import numpy as np

import pairs_ref
import translate_ref as tr
from pairs_ex_ref import revcomp
from seed_filter_ref import SEED_HIT_DTYPE
from seed_letters_ref import AA11, back_translate, random_protein, table_of
import seed_filter_translated_ref
import seed_letters_ref
import seed_translated_ref

G, S = 16, 4
CELLS = list(range(1, 10)) + [G * S - 1, G * S, G * S + 1, 127, 128, 129, 255, 256, 257, 398, 399, 400]
SPANS = [1, 2, 3, 4, 5, 8, 9, G - 1, G, G + 1, 300]
MAX_LETTERS = 400                                                                           # max_qlen of the protein queries
MAX_STREAM = 3 * 400 + 2                                                                    # max_qlen of the reads' streams: W - 2 with W = 3 c + 2 + 2
AA = b"ACDEFGHIKLMNPQRSTVWY"
CUSTOM_CODE = bytearray(tr.CODE_STD)
CUSTOM_CODE[16 * 0 + 4 * 3 + 2] = ord("W")                                                  # TGA reads as W, as in NCBI table 4
CUSTOM_CODE[16 * 2 + 4 * 3 + 0] = ord("*")                                                  # AGT is a stop here
CUSTOM_CODE = bytes(CUSTOM_CODE)
T11 = table_of(AA11)
K_AA = 4


def dna(rng, n):
    return bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, size=n))


def mutate(rng, s, rate, letters=AA):
    s = bytearray(s)
    for x in np.nonzero(rng.random(len(s)) < rate)[0]:
        s[x] = letters[(letters.index(s[x]) + 1 + int(rng.integers(len(letters) - 1))) % len(letters)] if s[x] in letters else letters[0]
    return bytes(s)


def seeds_array(rows):
    a = np.zeros(len(rows), dtype=SEED_HIT_DTYPE)
    for k, (lo, hi, g) in enumerate(rows):
        a[k] = (2, lo, hi, g)
    return a


class Lists:
    """One hand-built list: qs, refs, pairs, byte, seeds, and `marks`: name -> the list positions of the candidates made for it"""

    def __init__(self, qs, refs):
        self.qs, self.refs, self.rows, self.bytes_, self.sd, self.marks = qs, refs, [], [], [], {}

    def add(self, q, r, byte, r_beg, r_len, lo, hi, g=0, mark=None):
        self.rows.append((q, r, 0, -1, r_beg, r_len))
        self.bytes_.append(byte)
        self.sd.append((lo, hi, g))
        if mark:
            self.marks.setdefault(mark, []).append(len(self.rows) - 1)

    def done(self):
        self.pairs, self.byte, self.seeds = pairs_ref.pairs_array(self.rows), np.array(self.bytes_, dtype=np.uint8), seeds_array(self.sd)
        return self


def _with_oddities(rng, prot):
    """a protein piece with X, a stop, a byte outside the alphabet and lower case where it is long enough"""
    q = bytearray(prot)
    if len(q) > 20:
        q[3], q[7], q[11] = ord("X"), ord("*"), ord("#")
        q[12:16] = bytes(q[12:16]).lower()
    return bytes(q)


# ---- PMX_SEED_LIST_CODONS: nucleotide reads against proteins ------------------------------------------------------------------------------
def codons_list(seed=9300):
    """Reads of W = 3 c + 2 + res nucleotides, stored as read (strand 0) and reverse-complemented (strand 1), whose frame-0 codons are
    a 12 %-mutated piece of the protein reference at letter pos[c]: nucleotide diagonal D = 3 pos.  Every c of CELLS under every span,
    strands and residues rotating, all residues and both strands at span 1; windows by the seeding rule with pad 0 or 5, clipped at
    both ends of the reference; explicit windows with r_beg > 0 and a short r_len; diagonals without a cell; reads with N and lower
    case, proteins with X, *, # and lower case; periodic inputs for equal maxima on two diagonals and a piece planted twice on one;
    bad candidates between good neighbours."""
    rng = np.random.default_rng(seed)
    pieces = [random_protein(rng, c + 1) for c in CELLS]                                    # (+ 1: the letter the residue's last codon may meet)
    unit = b"ACDEFGHI"
    period = unit * 12
    s1 = random_protein(rng, 20)
    twice = s1 + b"W" * 40 + s1
    pos, parts, at = {}, [], 0
    for i, body in enumerate([_with_oddities(rng, p) for p in pieces] + [period * 2, s1 + b"P" * 40 + s1, b"K" * 40]):
        lead = random_protein(rng, int(rng.integers(0, 5)))
        pos[i] = at + len(lead)
        parts += [lead, body]
        at += len(lead) + len(body)
    I_PERIOD, I_TWICE, I_NEG = len(CELLS), len(CELLS) + 1, len(CELLS) + 2
    refs = [b"".join(parts), random_protein(rng, 7)]
    qs, qi = [], {}
    for ci, c in enumerate(CELLS):
        for res in range(3):
            nt = back_translate(mutate(rng, pieces[ci][:c], 0.12), rng) + dna(rng, 2 + res)
            if c > 30:
                nt = nt[:40] + b"N" + nt[41:60] + nt[60:75].lower() + nt[75:]                # a codon with N reads X; lower case reads as upper
            qi[ci, res, 0], qi[ci, res, 1] = len(qs), len(qs) + 1
            qs += [nt, revcomp(nt)]
    q_period = len(qs)
    qs.append(back_translate(unit, np.random.default_rng(seed + 1)) * 6 + b"AC")             # the same codons in every period
    q_twice = len(qs)
    qs.append(back_translate(twice, rng) + b"AC")
    q_neg = len(qs)
    qs.append(b"TGG" * 30 + b"AC")                                                           # W against K: every cell negative
    q_short = len(qs)
    qs += [b"AC", b"ACG", dna(rng, MAX_STREAM + 3)]                                           # no stream; a stream of one letter; one letter above max_qlen
    L = Lists(qs, refs)
    L.max_qlen, L.max_rlen = MAX_STREAM, len(refs[0])

    def window(W, lo, hi, pad):
        b, e = max(0, lo // 3 - pad), min(len(refs[0]), (hi + W - 1) // 3 + 1 + pad)
        return b, max(1, e - b)

    for ci, c in enumerate(CELLS):
        D = 3 * pos[ci]
        for si, span in enumerate(SPANS):
            s, res = (ci + si) % 2, (ci + si) % 3
            W = 3 * c + 2 + res
            lo = D - int(rng.integers(0, span))
            L.add(qi[ci, res, s], 0, s, *window(W, lo, lo + span - 1, 0 if span % 2 else 5), lo, lo + span - 1, mark="span%d" % span)
        for res in range(3):
            for s in range(2):
                W = 3 * c + 2 + res
                L.add(qi[ci, res, s], 0, s, *window(W, D, D, 0), D, D, mark="residue")
        L.add(qi[ci, 0, 0], 0, 0, pos[ci] + c // 2, max(1, c // 3), D - 2, D + 2, mark="clipped")         # r_beg > 0, short r_len
        L.add(qi[ci, 1, 1], 0, 1, 0, len(refs[0]), D, D, mark="whole")
    q12, D12, W12 = qi[12, 0, 0], 3 * pos[12], 3 * CELLS[12] + 2
    b12 = pos[12]
    L.add(q12, 0, 0, b12, 50, 3 * b12 - 900, 3 * b12 - 800, mark="nocell")                   # in front of the window
    L.add(q12, 0, 0, b12, 50, 3 * (b12 + 50), 3 * (b12 + 50) + 40, mark="nocell")            # behind it
    L.add(q12, 0, 0, b12, 50, 3 * b12 - (W12 - 3), 3 * b12 - (W12 - 3), mark="onecell")      # the stream's last letter on the window's first
    L.add(q12, 0, 0, b12, 50, 3 * (b12 + 49), 3 * (b12 + 49), mark="onecell")                # the stream's first letter on the window's last
    L.add(q12, 0, 0, b12, 50, 3 * (b12 + 49) - 6, 3 * (b12 + 49) + 9, mark="partly")
    L.add(q12, 0, 0, b12, 50, -(1 << 31), (1 << 31) - 1, mark="all")
    L.add(q_short + 1, 0, 0, 0, 30, -5, 95, mark="oneletter")                                 # L = 1: two of three diagonals have no cell
    L.add(q_neg, 0, 0, pos[I_NEG], 40, 3 * pos[I_NEG], 3 * pos[I_NEG] + 3, mark="negative")
    L.add(q_period, 0, 0, pos[I_PERIOD], 192, 3 * pos[I_PERIOD], 3 * pos[I_PERIOD] + 60, mark="tie2")      # equal maxima 24 diagonals apart
    L.add(q_period, 0, 0, pos[I_PERIOD], 192, 3 * pos[I_PERIOD] + 3, 3 * pos[I_PERIOD] + 60, mark="tie2")
    L.add(q_twice, 0, 0, pos[I_TWICE], 80, 3 * pos[I_TWICE], 3 * pos[I_TWICE], mark="twice")
    good = (qi[10, 0, 0], 0, 0, pos[10], CELLS[10], 3 * pos[10], 3 * pos[10])
    for bad in ((len(qs), 0, 0, 0, 10, 0, 0), (-1, 0, 0, 0, 10, 0, 0), (good[0], 2, 0, 0, 5, 0, 0), (good[0], 0, 0, 0, len(refs[0]) + 1, 0, 0),
                (good[0], 0, 0, -1, 10, 0, 0), (good[0], 0, 0, 5, 0, 0, 0), (good[0], 0, 2) + good[3:], (good[0], 0, 255) + good[3:],
                good[:5] + (good[5] + 1, good[5]), (q_short, 0, 0, 0, 10, 0, 0), (q_short + 2, 0, 0, 0, 10, 0, 0)):
        L.add(*good)
        L.add(*bad, mark="bad")
    L.add(*good)
    return L.done()


# ---- the reference side: proteins against nucleotide contigs ------------------------------------------------------------------------------
def _contigs(rng, genes, flank):
    """oriented sequences with the genes at pos[i]; stored: as it is (contig 0, strand 0) and reverse-complemented (contig 1, strand 1)"""
    pos, parts, at = {}, [], 0
    for i, gene in enumerate(genes):
        lead = dna(rng, int(rng.integers(*flank)))
        pos[i] = at + len(lead)
        parts += [lead, gene]
        at += len(lead) + len(gene)
    parts.append(dna(rng, int(rng.integers(*flank))))
    o = b"".join(parts)
    return o, pos


def _ref_inputs(seed):
    rng = np.random.default_rng(seed)
    prots = [_with_oddities(rng, random_protein(rng, c)) for c in CELLS]
    unit = b"ACDEFGHI"
    s1 = random_protein(rng, 20)
    prots += [unit * 6, s1 + b"W" * 40 + s1, b"K" * 40, random_protein(rng, MAX_LETTERS + 1)]           # (the last: one letter above max_qlen)
    genes = []
    for ci, c in enumerate(CELLS):
        clean = bytes(p if p in AA else AA[0] for p in prots[ci].upper())                  # (the oddities have no codon of their own)
        nt = back_translate(mutate(rng, clean, 0.12), rng)
        if c > 30:
            nt = nt[:40] + b"N" + nt[41:60] + nt[60:75].lower() + nt[75:]
        genes.append(nt + b"TAAG")                                                           # (a stop behind the gene, and the residues' bases)
    genes += [back_translate(unit, np.random.default_rng(seed + 1)) * 12, back_translate(s1 + b"P" * 40 + s1, rng), b"TGG" * 40]
    o, pos = _contigs(rng, genes, (1, 8))
    return rng, prots, o, pos


def ref_codons_list(seed=9310):
    """Proteins of c letters against a contig read on strand 0 (contig 0) and on strand 1 (contig 1: the same oriented sequence, stored
    reverse-complemented, so N - hi > 0 and the origin is not r_beg); gene i lies at oriented position pos[i], nucleotide diagonal
    D = pos[i].  Windows [D, D + 3 c + 2 + res) at span 1 -- every residue of the stream's length --, the seeding rule with pad 0 or 5
    for the other spans; clipped windows, diagonals without a cell, N, lower case, stops, ties and bad candidates as in codons_list."""
    rng, prots, o, pos = _ref_inputs(seed)
    N = len(o)
    refs = [o, revcomp(o), dna(rng, 2), dna(rng, 3)]
    I_PERIOD, I_TWICE, I_NEG = len(CELLS), len(CELLS) + 1, len(CELLS) + 2
    L = Lists(prots, refs)
    L.max_qlen, L.max_rlen = MAX_LETTERS, N - 2

    def stored(s, lo, hi):
        lo, hi = max(0, lo), min(N, hi)
        return (lo, max(1, hi - lo)) if s == 0 else (N - hi, max(1, hi - lo))

    for ci, c in enumerate(CELLS):
        D = pos[ci]
        for si, span in enumerate(SPANS):
            s, pad = (ci + si) % 2, 0 if span % 2 else 5
            lo = D - int(rng.integers(0, span))
            L.add(ci, s, s, *stored(s, lo - pad, lo + span - 1 + 3 * c + pad), lo, lo + span - 1, mark="span%d" % span)
        for res in range(3):
            for s in range(2):
                L.add(ci, s, s, *stored(s, D, D + 3 * c + 2 + res), D, D, mark="residue")
        L.add(ci, 0, 0, *stored(0, D + c, D + c + max(3, c)), D - 2, D + 2, mark="clipped")
        L.add(ci, 1, 1, *stored(1, D + c, D + c + max(3, c)), D - 2, D + 2, mark="clipped")
        L.add(ci, 1, 1, 0, N, D, D, mark="whole")
    m12, D12 = CELLS[12], pos[12]
    w = stored(1, D12, D12 + 150)
    L.add(12, 1, 1, *w, D12 - 900, D12 - 800, mark="nocell")
    L.add(12, 1, 1, *w, D12 + 150, D12 + 190, mark="nocell")
    L.add(12, 1, 1, *w, D12 - 3 * (m12 - 1), D12 - 3 * (m12 - 1), mark="onecell")            # the query's last letter on the window's first codon
    L.add(12, 1, 1, *w, D12 + 147, D12 + 147, mark="onecell")                                # the query's first letter on the window's last codon
    L.add(12, 1, 1, *w, D12 + 140, D12 + 160, mark="partly")
    L.add(12, 0, 0, *stored(0, D12, D12 + 150), -(1 << 31), (1 << 31) - 1, mark="all")
    L.add(12, 2, 0, 0, 2, -5, 5, mark="nostream")                                            # W = 2: no stream, a bad candidate
    L.add(12, 3, 1, 0, 3, -5, 5, mark="oneletter")                                           # W = 3: a stream of one letter
    L.add(I_NEG, 0, 0, *stored(0, pos[I_NEG], pos[I_NEG] + 120), pos[I_NEG], pos[I_NEG] + 3, mark="negative")
    L.add(I_PERIOD, 1, 1, *stored(1, pos[I_PERIOD], pos[I_PERIOD] + 288), pos[I_PERIOD], pos[I_PERIOD] + 60, mark="tie2")
    L.add(I_PERIOD, 0, 0, *stored(0, pos[I_PERIOD], pos[I_PERIOD] + 288), pos[I_PERIOD] + 3, pos[I_PERIOD] + 60, mark="tie2")
    L.add(I_TWICE, 1, 1, *stored(1, pos[I_TWICE], pos[I_TWICE] + 242), pos[I_TWICE], pos[I_TWICE], mark="twice")
    good = (10, 1, 1) + stored(1, pos[10], pos[10] + 3 * CELLS[10] + 2) + (pos[10], pos[10])
    for bad in ((len(prots), 0, 0, 0, 10, 0, 0), (-1, 0, 0, 0, 10, 0, 0), (10, 4, 0, 0, 5, 0, 0), (10, 0, 0, 0, N + 1, 0, 0), (10, 0, 0, -1, 10, 0, 0),
                (10, 0, 0, 5, 0, 0, 0), (10, 1, 2) + good[3:], (10, 1, 255) + good[3:], good[:5] + (good[5] + 1, good[5]), (len(prots) - 1,) + good[1:]):
        L.add(*good)
        L.add(*bad, mark="bad")
    L.add(*good)
    return L.done()


def ref_frames_list(seed=9320):
    """Proteins of c letters against the translated windows of the same contigs: gene i lies in sequence frame g = 3 s + pos[i] % 3 at
    letter pos[i] // 3, letter diagonal d = pos[i] // 3; the window is the seeding rule's [lb, le) in stored nucleotides, byte 3 s,
    seeds.reserved g.  Besides the shared cases: a window moved by one and by two nucleotides (not codon-aligned for g), g of the other
    strand, g outside 0 .. 5, bytes 1, 2, 4, 5 and 6."""
    rng, prots, o, pos = _ref_inputs(seed)
    N = len(o)
    refs = [o, revcomp(o)]
    I_PERIOD, I_TWICE, I_NEG = len(CELLS), len(CELLS) + 1, len(CELLS) + 2
    L = Lists(prots, refs)
    L.max_qlen, L.max_rlen = MAX_LETTERS, N // 3

    def stored(s, off, lb, le):
        lb, le = max(0, lb), min((N - off) // 3, le)
        le = max(le, lb + 1)
        return (off + 3 * lb, 3 * (le - lb)) if s == 0 else (N - off - 3 * le, 3 * (le - lb))

    def cand(i, s, lo, hi, pad, mark, lb=None, le=None):
        off = pos[i] % 3
        m = len(prots[i])
        w = stored(s, off, lo - pad if lb is None else lb, hi + m + pad if le is None else le)
        L.add(i, s, 3 * s, *w, lo, hi, 3 * s + off, mark=mark)

    for ci, c in enumerate(CELLS):
        d = pos[ci] // 3
        for si, span in enumerate(SPANS):
            lo = d - int(rng.integers(0, span))
            cand(ci, (ci + si) % 2, lo, lo + span - 1, 0 if span % 2 else 5, "span%d" % span)
        cand(ci, 0, d - 2, d + 2, 0, "clipped", d + c // 2, d + c // 2 + max(1, c // 3))
        cand(ci, 1, d - 2, d + 2, 0, "clipped", d + c // 2, d + c // 2 + max(1, c // 3))
        cand(ci, 1, d, d, 0, "whole", 0, N)
    d12 = pos[12] // 3
    cand(12, 1, d12 - 900, d12 - 800, 0, "nocell", d12, d12 + 50)
    cand(12, 1, d12 + 50, d12 + 90, 0, "nocell", d12, d12 + 50)
    cand(12, 1, d12 - (CELLS[12] - 1), d12 - (CELLS[12] - 1), 0, "onecell", d12, d12 + 50)
    cand(12, 1, d12 + 49, d12 + 49, 0, "onecell", d12, d12 + 50)
    cand(12, 1, d12 + 40, d12 + 60, 0, "partly", d12, d12 + 50)
    cand(12, 0, -(1 << 31), (1 << 31) - 1, 0, "all", d12, d12 + 50)
    cand(I_NEG, 0, pos[I_NEG] // 3, pos[I_NEG] // 3 + 3, 0, "negative")
    cand(I_PERIOD, 1, pos[I_PERIOD] // 3, pos[I_PERIOD] // 3 + 20, 0, "tie2", pos[I_PERIOD] // 3, pos[I_PERIOD] // 3 + 96)
    cand(I_PERIOD, 0, pos[I_PERIOD] // 3 + 1, pos[I_PERIOD] // 3 + 20, 0, "tie2", pos[I_PERIOD] // 3, pos[I_PERIOD] // 3 + 96)
    cand(I_TWICE, 1, pos[I_TWICE] // 3, pos[I_TWICE] // 3, 0, "twice")
    for s in (0, 1):
        off = pos[10] % 3
        d = pos[10] // 3
        w = stored(s, off, d, d + CELLS[10])
        good = (10, s, 3 * s) + w + (d, d, 3 * s + off)
        bads = [(len(prots), 0, 0, 0, 9, 0, 0, 0), (-1, 0, 0, 0, 9, 0, 0, 0), (10, 4, 0, 0, 6, 0, 0, 0), (10, 0, 0, 0, N + 1, 0, 0, 0),
                (10, 0, 0, -1, 9, 0, 0, 0), (10, 0, 0, 6, 0, 0, 0, 0), (10, 0, 0, 0, 2, 0, 0, 0),          # (a window without a codon)
                good[:5] + (d + 1, d, good[7]), (len(prots) - 1,) + good[1:],                # diag_min > diag_max; a query above max_qlen
                (10, s, 3 * s, w[0] + 1, w[1], d, d, good[7]), (10, s, 3 * s, w[0] + 2, w[1], d, d, good[7]),      # not codon-aligned for g
                good[:7] + (3 * (1 - s) + off,), good[:7] + (6,), good[:7] + (-1,), good[:7] + (1 << 30,)]          # g against the byte, outside 0 .. 5
        bads += [good[:2] + (b,) + good[3:] for b in (1, 2, 4, 5, 6, 3 * (1 - s), 255)]                           # a byte other than 0 or 3, the other strand's
        for bad in bads:
            L.add(*good)
            L.add(*bad, mark="bad")
        L.add(*good)
    return L.done()


# ---- planted worlds for the three roads ---------------------------------------------------------------------------------------------------
N_ROWS = 200


def codon_world(seed=9400):
    """The blastx road: 30 proteins of 110 letters; read q is the back-translation of 50 letters of protein q % 30 with the middle
    nucleotide deleted (149 nt, 2 % substitutions), reverse-complemented for odd q; a few reads are random, empty or shorter than a
    codon.  -> (prots, reads, planted: q -> (r, strand, D in front of the deletion), the seeding model's list)."""
    rng = np.random.default_rng(seed)
    prots = [random_protein(rng, 110) for _ in range(30)]
    reads, planted = [], {}
    for q in range(N_ROWS):
        r, a = q % 30, int(rng.integers(0, 61))
        nt = mutate(rng, back_translate(prots[r][a:a + 50], rng), 0.02, b"ACGT")
        nt = nt[:75] + nt[76:]
        reads.append(revcomp(nt) if q % 2 else nt)
        planted[q] = (r, q % 2, 3 * a)
    reads += [dna(rng, 149), dna(rng, 150), b"", b"AC"]
    hits = seed_letters_ref.seed(reads, prots, K_AA, T11, seed_letters_ref.CODONS_BOTH, min_seeds=2, band=12, pad=8, max_occ=64)
    return prots, reads, planted, hits


def tblastn_world(seed=9410, cut=True):
    """The tblastn roads: 200 proteins of 60 letters, and for protein q contig q: its gene back-translated (2 % substitutions) between
    random flanks of 60 .. 200 nt, with the middle nucleotide of the gene deleted when `cut`, stored reverse-complemented for odd q;
    three more rows are random, empty and shorter than a k-mer.  -> (prots, contigs, planted: q -> (r, strand, oriented start of the
    gene))."""
    rng = np.random.default_rng(seed)
    prots = [random_protein(rng, 60) for _ in range(N_ROWS)]
    contigs, planted = [], {}
    for q in range(N_ROWS):
        gene = mutate(rng, back_translate(prots[q], rng), 0.02, b"ACGT")
        if cut:
            gene = gene[:90] + gene[91:]
        left, right = dna(rng, int(rng.integers(60, 201))), dna(rng, int(rng.integers(60, 201)))
        o = left + gene + right
        contigs.append(revcomp(o) if q % 2 else o)
        planted[q] = (q, q % 2, len(left))
    prots = prots + [random_protein(rng, 60), b"", b"MKW"]
    return prots, contigs, planted


def tblastn_hits(prots, contigs, ref_mode):
    o = dict(min_seeds=2, max_occ=64)
    if ref_mode == seed_translated_ref.REF_FRAMES:
        return seed_translated_ref.seed(prots, contigs, K_AA, T11, ref_mode, seed_translated_ref.BOTH, band=4, pad=8, **o)
    return seed_translated_ref.seed(prots, contigs, K_AA, T11, ref_mode, seed_translated_ref.BOTH, band=12, pad=24, **o)


def rows_of(h, q):
    return range(int(h["row_off"][q]), int(h["row_off"][q + 1]))


def planted_survivors(kind, qs, rs, hits, planted, scores, mapper, ung=None):
    """the model's filter with top_n = 1 over a seeding model's list, and per planted row the list position of the planted candidate --
    the one of the planted reference and strand whose diagonals hold the planted one; asserts that it is the row's survivor"""
    f = seed_filter_translated_ref.filter_hits(qs, rs, hits["row_off"], hits["pairs"], hits["byte"], hits["seeds"], scores, mapper, kind, top_n=1, ung=ung)
    mine = {}
    for q, (r, s, D) in planted.items():
        if kind == "ref_frames":
            g, D = 3 * s + D % 3, D // 3
        found = [x for x in rows_of(hits, q) if hits["pairs"][x]["r"] == r and hits["byte"][x] == (3 * s if kind == "ref_frames" else s) and
                 hits["seeds"][x]["diag_min"] <= D <= hits["seeds"][x]["diag_max"] and (kind != "ref_frames" or hits["seeds"][x]["reserved"] == g)]
        assert len(found) == 1, (kind, q, found)
        kept = f["source"][int(f["row_off"][q]):int(f["row_off"][q + 1])].tolist()
        assert kept == found, (kind, q, kept, found)
        mine[q] = found[0]
    return f, mine
