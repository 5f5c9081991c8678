"""Reference model of minimizer seeding (include/parasail_amd.h), in plain Python on top of tests/seed_ref.py: the order
`mix`, the minimizers of a sequence by explicit enumeration of its windows, the same set by the per-position rule the kernel uses, the
index of a set's minimizers, and a match function for seed_ref.seed(...) so that clusters, windows and their order stay that model's."""
import seed_ref as ref

MIX_XOR, MIX_MUL1, MIX_MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def mix(key, k):
    """the order of the k-mers: a bijection on 2 k bits -- xor with a constant, times an odd number, xor with the own upper half, twice"""
    m = (1 << (2 * k)) - 1
    h = (key ^ MIX_XOR) & m
    h = (h * MIX_MUL1) & m
    h ^= h >> k
    h = (h * MIX_MUL2) & m
    h ^= h >> k
    return h


def hashes(seq, k):
    """[h(p) or None] for the nk = len(seq) - k + 1 k-mer positions of seq (empty if nk <= 0)"""
    nk = len(seq) - k + 1
    if nk <= 0:
        return []
    out = [None] * nk
    for p, key in ref.kmers(seq, k):
        out[p] = mix(key, k)
    return out


def windows(nk, w):
    """the windows [a, b) over nk k-mer positions"""
    if nk <= 0:
        return []
    if nk < w:
        return [(0, nk)]
    return [(s, s + w) for s in range(nk - w + 1)]


def minimizers_of_hashes(h, w):
    """sorted positions selected by at least one window: the smallest (hash, position) of the window's k-mers"""
    out = set()
    for a, b in windows(len(h), w):
        have = [(h[p], p) for p in range(a, b) if h[p] is not None]
        if have:
            out.add(min(have)[1])
    return sorted(out)


def minimizers(seq, k, w):
    """the minimizer positions of seq, by explicit window enumeration"""
    return minimizers_of_hashes(hashes(seq, k), w)


def _loses(h, q, p):
    return h[q] is None or (h[q], q) > (h[p], p)


def minimizers_by_rule_of_hashes(h, w):
    """the per-position rule: l consecutive left neighbours that lose to p (at most w - 1, stopping at 0), r the same to the right
    (stopping at nk - 1); p is a minimizer iff it has a k-mer and l + r + 1 >= min(w, nk)"""
    nk, out = len(h), []
    for p in range(nk):
        if h[p] is None:
            continue
        l = 0
        while l < w - 1 and p - l - 1 >= 0 and _loses(h, p - l - 1, p):
            l += 1
        r = 0
        while r < w - 1 and p + r + 1 <= nk - 1 and _loses(h, p + r + 1, p):
            r += 1
        if l + r + 1 >= min(w, nk):
            out.append(p)
    return out


def minimizers_by_rule(seq, k, w):
    return minimizers_by_rule_of_hashes(hashes(seq, k), w)


def flags(queries, k, w, strand, max_qlen, q_first=0, nq=None):
    """what pmx_seed_sketch writes: [[bytes per orientation] per row], a row longer than max_qlen all zeros"""
    nq = len(queries) - q_first if nq is None else nq
    out = []
    for q in range(q_first, q_first + nq):
        row = []
        for s in ref.strands_of(strand):
            f = bytearray(max_qlen)
            if len(queries[q]) <= max_qlen:
                for p in minimizers(ref.orient(queries[q], s), k, w):
                    f[p] = 1
            row.append(bytes(f))
        out.append(row)
    return out


def index_entries(refs, k, w):
    """the minimizer index: (kmer, seq, pos) of the minimizer positions of every sequence of the set, ascending"""
    out = []
    for r, s in enumerate(refs):
        keys = dict(ref.kmers(s, k))
        out += [(keys[p], r, p) for p in minimizers(s, k, w)]
    return sorted(out)


def index_dict(refs, k, w):
    d = {}
    for key, r, j in index_entries(refs, k, w):
        d.setdefault(key, []).append((r, j))
    return d


def match_fn(refs, k, w, max_occ):
    """a match function for seed_ref.seed(): (i, j) where i is a minimizer of the oriented query, j an entry of the minimizer index, the
    keys are equal and the key has at most max_occ entries of THIS index"""
    idx = index_dict(refs, k, w)

    def fn(query, strand):
        o = ref.orient(query, strand)
        keys = dict(ref.kmers(o, k))
        out = {}
        for i in minimizers(o, k, w):
            occ = idx.get(keys[i], ())
            if len(occ) > max_occ:
                continue
            for r, j in occ:
                out.setdefault(r, []).append(j - i)
        return out
    return fn


def seed(queries, refs, k, w, strand=ref.BOTH, min_seeds=2, band=8, pad=16, max_occ=64, q_first=0, nq=None, max_qlen=None):
    return ref.seed(queries, refs, k, strand, min_seeds, band, pad, max_occ, q_first, nq, max_qlen, match_fn=match_fn(refs, k, w, max_occ))
