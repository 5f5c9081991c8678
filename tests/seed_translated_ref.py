"""Reference model of seeding translated references (include/parasail_amd.h "Seeding translated references") in plain
Python: oriented coordinates, the letter of an oriented codon, the index as a sorted list of (kmer, s * count + r, x), the matches of
a protein row, both diagonal rules, both window rules and the order -- and, beside it, a brute-force matcher that compares letter
strings at every (p, s, r, x) and never forms a key.  Written from the definitions, not from the device code: the letters are
translate_ref's, the alphabets and keys seed_letters_ref's, the clusters seed_ref's.  Sequences are bytes."""
import numpy as np

from seed_letters_ref import AA11, AA20, bits_of, kmers, table_of   # noqa: F401  (re-exported for the tests)
from seed_ref import PAIR_DTYPE, SEED_HIT_DTYPE, clusters
from translate_ref import CODE_STD, translate

FORWARD, REVERSE, BOTH = 0, 1, 2
REF_FRAMES, REF_CODONS = 0, 1


def strands_of(mode):
    return {FORWARD: (0,), REVERSE: (1,), BOTH: (0, 1)}[mode]


def frame_letters(seq, g, table, code=CODE_STD):
    """the letters of sequence frame g = 3 s + off as the index sees them: translate()'s, with 'X' and '*' made invalid whatever the
    table holds for them (returned as a table that maps them to 255 beside the letters)"""
    t = np.array(table, dtype=np.uint8).copy()
    t[ord("X")] = t[ord("*")] = 255
    return translate(bytes(seq), g, code), t


def index_entries(refs, k, table, strand_mode=BOTH, code=CODE_STD):
    """the index: (kmer, s * count + r, x) of every oriented position with a k-mer, ascending -- which is (kmer, s, r, x).  Letter j of
    frame g sits at oriented position x = g % 3 + 3 j."""
    count = len(refs)
    out = []
    for s in strands_of(strand_mode):
        for r, seq in enumerate(refs):
            for off in range(3):
                letters, t = frame_letters(seq, 3 * s + off, table, code)
                out += [(key, s * count + r, off + 3 * j) for j, key in kmers(letters, k, t)]
    return sorted(out)


def index_dict(entries):
    d = {}
    for key, sr, x in entries:
        d.setdefault(key, []).append((sr, x))
    return d


def key_matches(idx, k, table, max_occ):
    """a matcher from the index: protein -> [(p, s * count + r, x)], k-mers above max_occ entries ignored"""
    def fn(protein):
        out = []
        for p, key in kmers(protein, k, table):
            occ = idx.get(key, ())
            if len(occ) <= max_occ:
                out += [(p, sr, x) for sr, x in occ]
        return out
    return fn


def brute_matches(refs, k, table, max_occ, strand_mode=BOTH, code=CODE_STD):
    """a matcher that compares the group letters of the protein at p .. p + k with those of frame g at j .. j + k for every (s, r, x);
    the occurrences are counted the same way over the held strands"""
    count = len(refs)
    frames = [(s, r, off, frame_letters(seq, 3 * s + off, table, code)) for s in strands_of(strand_mode) for r, seq in enumerate(refs)
              for off in range(3)]
    qt = np.array(table, dtype=np.uint8)

    def same(a, p, b, j, t):
        if p + k > len(a) or j + k > len(b):
            return False
        for y in range(k):
            u, v = int(qt[a[p + y]]), int(t[b[j + y]])
            if u == 255 or v == 255 or u != v:
                return False
        return True

    def fn(protein):
        protein = bytes(protein)
        out = []
        for p in range(len(protein) - k + 1):
            found = [(s * count + r, off + 3 * j) for s, r, off, (letters, t) in frames for j in range(len(letters) - k + 1)
                     if same(protein, p, letters, j, t)]
            if len(found) <= max_occ:
                out += [(p, sr, x) for sr, x in sorted(found)]
        return out
    return fn


def row_candidates(protein, q, ref_mode, matcher, rlens, min_seeds, band, pad):
    """[(descriptor, byte, seed record)] of one row in the order of the entry: (g, r, d_min) or (s, r, D_min)"""
    count, m = len(rlens), len(protein)
    groups = {}
    for p, sr, x in matcher(protein):
        s, r = divmod(sr, count)
        if ref_mode == REF_FRAMES:
            groups.setdefault((3 * s + x % 3, r), []).append((x - x % 3) // 3 - p)
        else:
            groups.setdefault((s, r), []).append(x - 3 * p)
    out = []
    for o, r in sorted(groups):
        N = rlens[r]
        for n, dmin, dmax in clusters(groups[(o, r)], band):
            if n < min_seeds:
                continue
            if ref_mode == REF_FRAMES:
                off, s = o % 3, o // 3
                lb, le = max(0, dmin - pad), min((N - off) // 3, dmax + m + pad)
                beg, end = (off + 3 * lb, off + 3 * le) if s == 0 else (N - off - 3 * le, N - off - 3 * lb)
                out.append(((q, r, 0, -1, beg, end - beg), 3 * s, (n, dmin, dmax, o)))
            else:
                lo, hi = max(0, dmin - pad), min(N, dmax + 3 * m + pad)
                beg, end = (lo, hi) if o == 0 else (N - hi, N - lo)
                out.append(((q, r, 0, -1, beg, end - beg), o, (n, dmin, dmax, 0)))
    return out


def seed(queries, refs, k, table, ref_mode, strand_mode=BOTH, min_seeds=2, band=8, pad=16, max_occ=64, q_first=0, nq=None, max_qlen=None,
         code=CODE_STD, matcher=None):
    """what pmx_seed_pairs_translated_ref_device writes with a capacity that holds everything: row_off (nq + 1), pairs, byte, seeds"""
    nq = len(queries) - q_first if nq is None else nq
    if matcher is None:
        matcher = key_matches(index_dict(index_entries(refs, k, table, strand_mode, code)), k, table, max_occ)
    rlens = [len(s) for s in refs]
    row_off, rows = [0], []
    for q in range(q_first, q_first + nq):
        protein = bytes(queries[q])
        if max_qlen is None or len(protein) <= max_qlen:
            rows += row_candidates(protein, q, ref_mode, matcher, rlens, min_seeds, band, pad)
        row_off.append(len(rows))
    return {"row_off": np.array(row_off, dtype=np.int64),
            "pairs": np.array([c[0] for c in rows], dtype=PAIR_DTYPE),
            "byte": np.array([c[1] for c in rows], dtype=np.uint8),
            "seeds": np.array([c[2] for c in rows], dtype=SEED_HIT_DTYPE)}


def r6(refs, strand_mode=BOTH, code=CODE_STD):
    """the protein set of the defining equivalence: sequence g * count + r = translate(R[r], g), b"" for a frame of a strand not held"""
    held = strands_of(strand_mode)
    return [translate(bytes(seq), g, code) if g // 3 in held else b"" for g in range(6) for seq in refs]


def from_letters(want, refs):
    """a seed_letters_ref.seed() result over r6(refs) in letters mode -> what the frame mode gives, through r' -> (g, r) and the window
    mapping"""
    count = len(refs)
    pairs, seeds = want["pairs"].copy(), want["seeds"].copy()
    byte = np.zeros(len(pairs), dtype=np.uint8)
    for x in range(len(pairs)):
        g, r = divmod(int(pairs[x]["r"]), count)
        N, off = len(refs[r]), g % 3
        lb, le = int(pairs[x]["r_beg"]), int(pairs[x]["r_beg"]) + int(pairs[x]["r_len"])
        beg, end = (off + 3 * lb, off + 3 * le) if g < 3 else (N - off - 3 * le, N - off - 3 * lb)
        pairs[x]["r"], pairs[x]["r_beg"], pairs[x]["r_len"] = r, beg, end - beg
        seeds[x]["reserved"] = g
        byte[x] = 3 * (g // 3)
    return {"row_off": want["row_off"], "pairs": pairs, "byte": byte, "seeds": seeds}
