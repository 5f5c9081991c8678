#!/usr/bin/env python3
"""Seeding translated references (pmx_seed_index_build_translated, pmx_seed_pairs_translated_ref[_device]) on an MI355X.  Not a test;
every input comes from --seed.

  a. index: a synthetic nucleotide set of --nt bases (uniform, 20 sequences), both strands, aa11 at --k: wall-clock time of the build
     (it synchronises), entries, resident bytes (hipMemGetInfo before / after) -- and, in the same process, the letters index of
     --letters uniform protein letters (aa11, the same k) as the yardstick per entry.
  b. end to end on a size the rectangle can run: --prots proteins of 200 .. 400 letters, each back-translated with 5 % nucleotide
     substitutions into one of --prots / 2 contigs (two genes per contig, odd contigs stored reverse-complemented).  Frame road: seed
     (PMX_SEED_REF_FRAMES) + pmx_align_pairs_translated_ref_device over the candidates against
     pmx_search_pairs_translated_ref_device over the rectangle in all six frames.  Codon road (every gene with its middle nucleotide
     deleted): seed (PMX_SEED_REF_CODONS) + pmx_align_pairs_frameshift_ref_device against pmx_search_pairs_frameshift_ref_device on
     both strands.  Times, their ratio, and the share of proteins whose best rectangle hit is also their best-scoring candidate.
  c. one row of long contigs: --long-prots proteins of 400 letters, each planted (one nucleotide deleted) in its own contig of
     --long-nt bases: seed_pairs(ref_frames="codons") + align_pairs_frameshift_ref_cigar_long over the candidate windows, against the
     same traceback entry over the whole contigs on both strands.

One warm-up call per timed leg, then --repeats runs; median / min / max.  One JSON line; --out FILE writes it there as well."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch's HIP runtime first)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_pkg()
lib = pkg.lib
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for a_, b_ in zip(b"ACGT", b"TGCA"):
    COMP[a_] = b_


def codon_table():
    """[20, 6, 3] codons per amino acid (padded by repetition) and their counts, from the library's own genetic code"""
    code = pkg.genetic_code_table()
    tab = np.zeros((20, 6, 3), dtype=np.uint8)
    cnt = np.zeros(20, dtype=np.int64)
    for i, aa in enumerate(code):
        if aa in AA.tobytes():
            a = AA.tobytes().index(aa)
            tab[a, cnt[a]] = [b"TCAG"[i >> 4], b"TCAG"[(i >> 2) & 3], b"TCAG"[i & 3]]
            cnt[a] += 1
    for a in range(20):
        for x in range(cnt[a], 6):
            tab[a, x] = tab[a, x % cnt[a]]
    return tab, cnt


def free_bytes():
    torch.cuda.synchronize(dev)
    return torch.cuda.mem_get_info(dev)[0]


def stats_of(runs, timing):
    return {"median_ms": round(float(np.median(runs)), 3), "min_ms": round(min(runs), 3), "max_ms": round(max(runs), 3), "runs": len(runs),
            "timing": timing}


def wall_ms(fn, repeats):
    fn()
    torch.cuda.synchronize(dev)
    runs = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        runs.append((time.perf_counter() - t) * 1e3)
    return stats_of(runs, "host wall clock around the call and a device synchronisation")


class DevSet:
    def __init__(self, buf, off):
        self.n, self.bytes = len(off) - 1, int(off[-1])
        self.keep = [torch.from_numpy(np.concatenate([buf, np.zeros(16, dtype=np.uint8)])).to(dev), torch.from_numpy(off).to(dev)]
        self.set = pkg.SeqSet.wrap_device(self.keep[0].data_ptr(), self.keep[1].data_ptr(), self.n, self.bytes, keep=self.keep)
        self.max_len = int(np.diff(off).max()) if self.n else 0


def part_index(a, R, k, translated):
    kw = dict(alphabet="aa11", stream=stream.cuda_stream)
    if translated:
        kw["translated"] = "both"
    free0 = free_bytes()
    t = time.perf_counter()
    ix = pkg.SeedIndex.build(R.set, k, **kw)
    first_ms = (time.perf_counter() - t) * 1e3
    resident = free0 - free_bytes()
    runs = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        other = pkg.SeedIndex.build(R.set, k, **kw)
        runs.append((time.perf_counter() - t) * 1e3)
        other.close()
    n = len(ix)
    slots = R.bytes * (2 if translated else 1)
    med = float(np.median(runs))
    out = {"kind": "translated, both strands" if translated else "letters", "alphabet": "aa11", "k": k, "key_bits": ix.bits * k, "bytes": R.bytes,
           "sequences": R.n, "entry_slots": slots, "entries": n, "first_build_ms": round(first_ms, 2),
           "build_ms": stats_of(runs, "host wall clock around the build, which allocates, sorts and synchronises"),
           "ns_per_entry": round(med * 1e6 / max(1, n), 4), "ns_per_entry_slot": round(med * 1e6 / max(1, slots), 4),
           "resident_bytes": resident, "resident_bytes_per_entry_slot": round(resident / max(1, slots), 2),
           "resident_is": "hipMemGetInfo before / after the build: 16 bytes per entry slot, the bucket table and the 256-byte table"}
    ix.close()
    return out


def part_a(a, rng):
    nt = ACGT[rng.integers(0, 4, size=a.nt, dtype=np.uint8)]
    R = DevSet(nt, (np.arange(21, dtype=np.int64) * (a.nt // 20)))
    out = {"translated": part_index(a, R, a.k, True)}
    del R, nt
    torch.cuda.empty_cache()
    n = a.letters // 300
    P = DevSet(AA[rng.integers(0, 20, size=n * 300, dtype=np.uint8)], np.arange(n + 1, dtype=np.int64) * 300)
    out["letters_yardstick"] = part_index(a, P, a.k, False)
    out["ns_per_entry_ratio_translated_over_letters"] = round(out["translated"]["ns_per_entry"] / out["letters_yardstick"]["ns_per_entry"], 3)
    return out


def genes_of(rng, prot_idx, tab, cnt, sub):
    """back-translations with `sub` nucleotide substitutions, one uint8 array per protein"""
    out = []
    for letters in prot_idx:
        pick = (rng.random(len(letters)) * cnt[letters]).astype(np.int64)
        nt = tab[letters, pick].reshape(-1)
        flip = rng.random(len(nt)) < sub
        nt[flip] = ACGT[rng.integers(0, 4, size=int(flip.sum()))]
        out.append(nt)
    return out


def contigs_of(rng, genes, per, lo, hi, delete_mid):
    """`per` genes per contig between spacers of lo .. hi random bases; odd contigs stored reverse-complemented"""
    bufs, off = [], [0]
    for c in range(len(genes) // per):
        parts = [ACGT[rng.integers(0, 4, size=int(rng.integers(lo, hi)))]]
        for gene in genes[c * per:(c + 1) * per]:
            parts += [np.delete(gene, len(gene) // 2) if delete_mid else gene, ACGT[rng.integers(0, 4, size=int(rng.integers(lo, hi)))]]
        s = np.concatenate(parts)
        bufs.append(COMP[s[::-1]] if c % 2 else s)
        off.append(off[-1] + len(s))
    return DevSet(np.concatenate(bufs), np.array(off, dtype=np.int64))


def best_per_row(q, r, score, nq):
    """per protein the reference of its best-scoring entry (the first of equals), -1 without one"""
    best = np.full(nq, -1, dtype=np.int64)
    if len(q):
        order = np.lexsort((r, -score.astype(np.int64), q))
        first = order[np.concatenate(([True], q[order][1:] != q[order][:-1]))]
        best[q[first]] = r[first]
    return best


def part_b(a, rng):
    tab, cnt = codon_table()
    nq = a.prots
    prot_idx = [rng.integers(0, 20, size=int(rng.integers(200, 401)), dtype=np.uint8) for _ in range(nq)]
    off = np.concatenate(([0], np.cumsum([len(p) for p in prot_idx]))).astype(np.int64)
    Q = DevSet(AA[np.concatenate(prot_idx)], off)
    genes = genes_of(rng, prot_idx, tab, cnt, 0.05)
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, m.inner)
    out = {"proteins": nq, "protein_letters": "200 .. 400", "matrix": "blosum62, gaps 11 / 1", "min_score": a.min_score, "frameshift": a.frameshift,
           "options": {"alphabet": "aa11", "k": a.k, "min_seeds": a.min_seeds, "band_letters": a.band, "band_nucleotides": a.band_nt, "pad_letters": a.pad,
                       "pad_nucleotides": 3 * a.pad, "max_occ": a.max_occ}}
    for road in ("frames", "codons"):
        codon = road == "codons"
        R = contigs_of(rng, genes, 2, 100, 400, codon)
        nr = R.n
        ix = pkg.SeedIndex.build(R.set, a.k, alphabet="aa11", translated="both", stream=stream.cuda_stream)
        cap = 64 * nq
        hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        hs = torch.zeros(cap, dtype=torch.uint8, device=dev)
        offs = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        cnts = torch.zeros(2, dtype=torch.int64, device=dev)
        rec = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        won = torch.zeros(cap, dtype=torch.uint8, device=dev)
        state = {}

        def seed_extend():
            pkg.seed_pairs_device(Q.set, ix, 0, nq, Q.max_len, hp.data_ptr(), hs.data_ptr(), None, cap, offs.data_ptr(), cnts.data_ptr(),
                                  min_seeds=a.min_seeds, band=a.band_nt if codon else a.band, pad=3 * a.pad if codon else a.pad, max_occ=a.max_occ,
                                  stream=stream.cuda_stream, ref_frames=road)
            n = int(cnts.cpu()[1])                                     # (the seeding entry has synchronised already)
            state["n"] = n
            if n and codon:
                pkg.align_pairs_frameshift_ref_device(cfg, Q.set, R.set, n, hp.data_ptr(), hs.data_ptr(), pkg.STRAND_FORWARD, a.frameshift,
                                                      Q.max_len, R.max_len, rec.data_ptr(), won.data_ptr(), stream.cuda_stream)
            elif n:
                pkg.align_pairs_translated_ref_device(cfg, Q.set, R.set, n, hp.data_ptr(), hs.data_ptr(), 0, Q.max_len, R.max_len // 3 + 1,
                                                      rec.data_ptr(), None, won.data_ptr(), stream.cuda_stream)
        leg = {"contigs": nr, "contig_bases": R.bytes, "index_entries": len(ix), "seed_extend": wall_ms(seed_extend, a.repeats)}
        n = state["n"]
        leg["candidates"], leg["candidates_passing"] = n, int(cnts.cpu()[0])
        pairs = hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n]
        best_seed = best_per_row(pairs["q"], pairs["r"], rec.cpu().numpy()[:n, 0], nq)
        rp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        rr = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        rb = torch.zeros(cap, dtype=torch.uint8, device=dev)
        rc = torch.zeros(2, dtype=torch.int64, device=dev)

        def rectangle():
            if codon:
                e = lib.pmx_search_pairs_frameshift_ref_device(C.byref(cfg), Q.set.inner, R.set.inner, pkg.PAIRS_RECT, 0, nq * nr, None, Q.max_len,
                                                               R.max_len, a.min_score, rp.data_ptr(), None, rr.data_ptr(), None, cap, rc.data_ptr(),
                                                               stream.cuda_stream, None, pkg.STRAND_BOTH, rb.data_ptr(), a.frameshift, None)
                if e:
                    raise SystemExit(lib.pmx_last_error().decode())
            else:
                pkg.search_pairs_translated_ref_device(cfg, Q.set, R.set, pkg.PAIRS_RECT, 0, nq * nr, None, Q.max_len, R.max_len // 3 + 1, a.min_score,
                                                       rp.data_ptr(), None, rr.data_ptr(), None, cap, rc.data_ptr(), pkg.FRAMES_ALL, rb.data_ptr(),
                                                       stream.cuda_stream)
        leg["rectangle"] = wall_ms(rectangle, a.repeats)
        c = rc.cpu().tolist()
        leg["rectangle_pairs"], leg["rectangle_hits"], leg["rectangle_hits_written"] = nq * nr, c[0], c[1]
        ep = rp.cpu().numpy().view(pkg.PAIR_DTYPE)[:c[1]]
        best_rect = best_per_row(ep["q"], ep["r"], rr.cpu().numpy()[:c[1], 0], nq)
        have = best_rect >= 0
        planted = np.arange(nq) // 2
        leg["proteins_with_a_rectangle_hit"] = round(float(have.sum()) / nq, 5)
        leg["best_rectangle_hit_is_best_candidate"] = round(float((best_seed[have] == best_rect[have]).sum()) / max(1, int(have.sum())), 5)
        leg["best_rectangle_hit_is_the_planted_contig"] = round(float((best_rect[have] == planted[have]).sum()) / max(1, int(have.sum())), 5)
        leg["time_ratio_rectangle_over_seed_extend"] = round(leg["rectangle"]["median_ms"] / leg["seed_extend"]["median_ms"], 2)
        leg["kernel"] = lib.pmx_last_kernel().decode()
        out[road] = leg
        ix.close()
        del R, hp, hs, rec, won, rp, rr, rb
        torch.cuda.empty_cache()
    return out


def part_c(a, rng):
    tab, cnt = codon_table()
    nq = a.long_prots
    prot_idx = [rng.integers(0, 20, size=400, dtype=np.uint8) for _ in range(nq)]
    prots = [AA[p].tobytes() for p in prot_idx]
    genes = genes_of(rng, prot_idx, tab, cnt, 0.05)
    half = (a.long_nt - 1200) // 2
    R = contigs_of(rng, genes, 1, half, half + 1, True)
    Q = pkg.SeqSet.new(prots)
    ix = pkg.SeedIndex.build(R.set, a.k, alphabet="aa11", translated="both", stream=stream.cuda_stream)
    al = pkg.Aligner.new().local().matrix(pkg.Matrix.from_name("blosum62")).gap_open(11).gap_extend(1).build()
    state = {}

    def seeded():
        hits = pkg.seed_pairs(Q, ix, min_seeds=a.min_seeds, band=a.band_nt, pad=3 * a.pad, max_occ=a.max_occ, ref_frames="codons")
        state["hits"] = hits
        state["out"] = al.align_pairs_frameshift_ref_cigar_long(Q, R.set, hits.pairs, a.frameshift, ref_strand=hits.strand)

    def whole():
        state["whole"] = al.align_pairs_frameshift_ref_cigar_long(Q, R.set, [(i, i) for i in range(nq)], a.frameshift, ref_strand="both")
    out = {"proteins": nq, "protein_letters": 400, "contigs": R.n, "contig_bases": R.max_len, "index_entries": len(ix),
           "seed_then_cigar_long": wall_ms(seeded, a.repeats), "cigar_long_over_whole_contigs_both_strands": wall_ms(whole, a.repeats)}
    hits, (rec, cigars, begins, strand) = state["hits"], state["out"]
    wrec = state["whole"][0]
    mine = [[x for x in range(int(hits.row_off[i]), int(hits.row_off[i + 1])) if hits.pairs[x]["r"] == i] for i in range(nq)]
    out["candidates"] = len(hits)
    out["candidate_window_bases_median"] = int(np.median(hits.pairs["r_len"])) if len(hits) else 0
    out["proteins_whose_best_candidate_has_the_whole_contig_score"] = sum(
        1 for i in range(nq) if mine[i] and max(int(rec["score"][x]) for x in mine[i]) == int(wrec["score"][i]))
    out["planted_cigars_with_a_slash"] = sum(1 for i in range(nq) if any("/" in cigars[x] for x in mine[i]))
    out["time_ratio_whole_over_seeded"] = round(out["cigar_long_over_whole_contigs_both_strands"]["median_ms"] / out["seed_then_cigar_long"]["median_ms"], 2)
    ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--nt", type=int, default=100_000_000)
    ap.add_argument("--letters", type=int, default=50_000_000)
    ap.add_argument("--prots", type=int, default=2_000)
    ap.add_argument("--long-prots", type=int, default=16)
    ap.add_argument("--long-nt", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=9)
    ap.add_argument("--min-seeds", type=int, default=2)
    ap.add_argument("--band", type=int, default=4)
    ap.add_argument("--band-nt", type=int, default=12)
    ap.add_argument("--pad", type=int, default=8)
    ap.add_argument("--max-occ", type=int, default=64)
    ap.add_argument("--min-score", type=int, default=100)
    ap.add_argument("--frameshift", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    parts = a.parts.split(",")
    line = {"bench": "seed_translated_ref", "device": torch.cuda.get_device_name(dev), "seed": a.seed}

    def write():
        s = json.dumps(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(s + "\n")
        return s
    if "a" in parts:
        line["index"] = part_a(a, rng)
        write()
    if "b" in parts:
        line["end_to_end"] = part_b(a, rng)
        write()
    if "c" in parts:
        line["long_contigs"] = part_c(a, rng)
    print(write(), flush=True)


if __name__ == "__main__":
    main()
