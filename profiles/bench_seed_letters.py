#!/usr/bin/env python3
"""Protein seeding (pmx_seed_index_build_letters, pmx_seed_pairs_letters_device) on an MI355X.  Not a test; every input comes from --seed.

  a. index: a synthetic protein set of --letters letters (uniform over the twenty amino acids, 300 letters per protein): wall-clock time
     of the build (it synchronises), entries, distinct keys (the mean occupancy per key), resident bytes (hipMemGetInfo before /
     after) -- for aa11 at --k11 and for aa20 at --k20.
  b. seed: --reads reads of 150 nt, each the back-translation of 50 letters of a protein of the set with 5 % nucleotide substitutions,
     every other one stored reverse-complemented, against the aa11 index: pmx_seed_pairs_letters_device in PMX_FRAMES_ALL and in
     PMX_SEED_CODONS_BOTH -- time, slices (by arithmetic on the position scratch), candidates per read, the share of reads with a
     candidate on their protein, scratch bytes.  The per-kernel breakdown comes from a `rocprofv3 --kernel-trace --stats` run of
     `--parts b` alone, whose CSV --kernel-stats names.
  c. end to end on a size the rectangle can run: --e2e-reads reads against --e2e-prots proteins.  Frame road: seed (PMX_FRAMES_ALL) +
     pmx_align_pairs_translated_device over the candidates against pmx_search_pairs_translated_device over the rectangle in all six
     frames.  Codon road (the reads with their middle nucleotide deleted): seed (PMX_SEED_CODONS_BOTH) +
     pmx_align_pairs_frameshift_device against pmx_search_pairs_frameshift_device on both strands.  Times, their ratio, and the share
     of reads whose best rectangle hit (the reference for recall) is also the best-scoring candidate.

One warm-up call per timed leg, then --repeats runs; median / min / max.  One JSON line; --out FILE writes it there as well."""
import argparse
import csv
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
COMP = np.arange(256, dtype=np.uint8)
for a_, b_ in zip(b"ACGT", b"TGCA"):
    COMP[a_] = b_
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
PLEN, RLEN = 300, 50                                                   # letters per protein, letters per read


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


def wall_ms(fn, repeats):
    fn()
    torch.cuda.synchronize(dev)
    runs = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        runs.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(float(np.median(runs)), 3), "min_ms": round(min(runs), 3), "max_ms": round(max(runs), 3), "runs": len(runs),
            "timing": "host wall clock around the call and a device synchronisation"}


class DevSet:
    def __init__(self, buf, off):
        self.n, self.bytes = len(off) - 1, int(off[-1])
        self.keep = [torch.from_numpy(np.concatenate([buf, np.zeros(16, dtype=np.uint8)])).to(dev), torch.from_numpy(off).to(dev)]
        self.set = pkg.SeqSet.wrap_device(self.keep[0].data_ptr(), self.keep[1].data_ptr(), self.n, self.bytes, keep=self.keep)
        self.max_len = int(np.diff(off).max()) if self.n else 0


def proteins(rng, n):
    idx = rng.integers(0, 20, size=(n, PLEN), dtype=np.uint8)
    return idx, DevSet(AA[idx].reshape(-1), np.arange(n + 1, dtype=np.int64) * PLEN)


def planted_reads(rng, idx, n, sub=0.05, delete_mid=False):
    """n reads: 50 letters of a protein back-translated, `sub` nucleotide substitutions, odd reads stored reverse-complemented;
    delete_mid: the nucleotide at position 75 taken out.  -> (DevSet, protein of each read, first letter of each read)"""
    tab, cnt = codon_table()
    bufs, prot, at = [], [], []
    for k in range(0, n, 100_000):
        m = min(100_000, n - k)
        p = rng.integers(0, len(idx), size=m)
        a = rng.integers(0, PLEN - RLEN + 1, size=m)
        letters = idx[p[:, None], a[:, None] + np.arange(RLEN)[None, :]]
        pick = (rng.random(letters.shape) * cnt[letters]).astype(np.int64)
        nt = tab[letters, pick].reshape(m, 3 * RLEN)
        flip = rng.random(nt.shape) < sub
        nt[flip] = ACGT[rng.integers(0, 4, size=int(flip.sum()))]
        if delete_mid:
            nt = np.delete(nt, 75, axis=1)
        nt[1::2] = COMP[nt[1::2, ::-1]]
        bufs.append(nt.reshape(-1))
        prot.append(p)
        at.append(a)
    W = 3 * RLEN - (1 if delete_mid else 0)
    return DevSet(np.concatenate(bufs), np.arange(n + 1, dtype=np.int64) * W), np.concatenate(prot), np.concatenate(at)


def part_index(a, idx, R, alphabet, k):
    free0 = free_bytes()
    t = time.perf_counter()
    ix = pkg.SeedIndex.build(R.set, k, alphabet=alphabet, stream=stream.cuda_stream)
    first_ms = (time.perf_counter() - t) * 1e3
    resident = free0 - free_bytes()
    runs = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        other = pkg.SeedIndex.build(R.set, k, alphabet=alphabet, stream=stream.cuda_stream)
        runs.append((time.perf_counter() - t) * 1e3)
        other.close()
    n = len(ix)
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    pkg.seed_index_entries_device(ix, 0, n, keys.data_ptr(), None, None, stream.cuda_stream)
    distinct = int(torch.unique_consecutive(keys).numel())
    del keys
    out = {"alphabet": alphabet, "k": k, "bits_per_letter": ix.bits, "key_bits": ix.bits * k, "letters": R.bytes, "proteins": R.n, "entries": n,
           "distinct_keys": distinct, "mean_entries_per_key": round(n / max(1, distinct), 3), "first_build_ms": round(first_ms, 2),
           "build_ms": {"median_ms": round(float(np.median(runs)), 2), "min_ms": round(min(runs), 2), "max_ms": round(max(runs), 2), "runs": len(runs),
                        "timing": "host wall clock around pmx_seed_index_build_letters, which allocates, sorts and synchronises"},
           "resident_bytes": resident, "resident_bytes_per_entry": round(resident / max(1, n), 2),
           "resident_is": "hipMemGetInfo before / after the build: 16 bytes per byte of the set, the bucket table and the 256-byte table"}
    return out, ix


class Seeder:
    def __init__(self, Q, ix, cap, a, frames, mq):
        self.Q, self.ix, self.cap, self.a, self.frames, self.mq = Q, ix, cap, a, frames, mq
        self.hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        self.hs = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.hd = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.off = torch.zeros(Q.n + 1, dtype=torch.int64, device=dev)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def run(self):
        a = self.a
        codon = self.frames.startswith("codons")
        pkg.seed_pairs_device(self.Q.set, self.ix, 0, self.Q.n, self.mq, self.hp.data_ptr(), self.hs.data_ptr(), self.hd.data_ptr(), self.cap,
                              self.off.data_ptr(), self.cnt.data_ptr(), min_seeds=a.min_seeds, band=a.band_nt if codon else a.band, pad=a.pad,
                              max_occ=a.max_occ, stream=stream.cuda_stream, frames=self.frames)


def trace_rows(path):
    rows = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name") or r.get("KernelName") or ""
            rows.append({"kernel": name[:160], "calls": int(r.get("Calls", 0)), "total_ms": round(float(r.get("TotalDurationNs", 0)) / 1e6, 4),
                         "percent": float(r.get("Percentage", 0))})
    return sorted(rows, key=lambda r: -r["total_ms"])


def part_seed(a, rng, idx, ix):
    Q, prot, at = planted_reads(rng, idx, a.reads)
    mq = Q.max_len // 3
    out = {"reads": a.reads, "read_letters": "150 nt: 50 letters back-translated, 5 % substitutions; odd reads stored reverse-complemented",
           "max_qlen": mq, "options": {"alphabet": "aa11", "k": a.k11, "min_seeds": a.min_seeds, "band_letters": a.band, "band_nucleotides": a.band_nt,
                                       "pad": a.pad, "max_occ": a.max_occ}}
    for frames in ("all", "codons-both"):
        s = Seeder(Q, ix, 8 * a.reads + 1024, a, frames, mq)
        free0 = free_bytes()
        s.run()
        scratch = free0 - free_bytes()
        cnt = s.cnt.cpu().tolist()
        leg = {"candidates": cnt[0], "written": cnt[1], "candidates_per_read": round(cnt[0] / a.reads, 3), "scratch_bytes_grown": scratch,
               "slices_at_least": -(-a.reads // max(1, (256 << 20) // (6 * mq * 17))),
               "slices_is": "rows / the rows that 256 MiB of position scratch hold (17 bytes x 6 orientations x max_qlen); a cut adds more"}
        leg["seed_pairs_letters_device"] = wall_ms(s.run, a.repeats)
        n = cnt[1]
        pairs = s.hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n]
        byte = s.hs.cpu().numpy()[:n]
        q = pairs["q"]
        want = (q & 1) * 3 if frames == "all" else (q & 1)                  # frame 0 / 3, strand 0 / 1
        near = (pairs["r"] == prot[q]) & (byte == want)
        leg["reads_with_a_candidate_on_their_protein"] = round(len(np.unique(q[near])) / a.reads, 5)
        out[frames] = leg
        del s
        torch.cuda.empty_cache()
    if a.kernel_stats:
        rows = trace_rows(a.kernel_stats)
        out["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats of `--parts b` alone (both index builds, warm-ups and the timed calls of both modes)",
                               "rows": [r for r in rows if "seed" in r["kernel"] or "rocprim" in r["kernel"]][:28]}
    return out


def best_per_read(q, r, score, nq):
    """per read the reference of its best-scoring entry (the first of equals), -1 without one"""
    best = np.full(nq, -1, dtype=np.int64)
    if len(q):
        order = np.lexsort((r, -score.astype(np.int64), q))
        first = order[np.concatenate(([True], q[order][1:] != q[order][:-1]))]
        best[q[first]] = r[first]
    return best


def part_e2e(a, rng):
    idx, R = proteins(rng, a.e2e_prots)
    ix = pkg.SeedIndex.build(R.set, a.k11, alphabet="aa11", stream=stream.cuda_stream)
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, m.inner)
    out = {"proteins": R.n, "reads": a.e2e_reads, "matrix": "blosum62, gaps 11 / 1", "min_score": a.min_score, "frameshift": a.frameshift}
    nq, nr = a.e2e_reads, R.n
    for road in ("frames", "codons"):
        codon = road == "codons"
        Q, prot, at = planted_reads(rng, idx, nq, delete_mid=codon)
        mq = Q.max_len // 3
        s = Seeder(Q, ix, 256 * nq, a, "codons-both" if codon else "all", mq)
        rec = torch.zeros((s.cap, 4), dtype=torch.int32, device=dev)
        won = torch.zeros(s.cap, dtype=torch.uint8, device=dev)
        state = {}

        def seed_extend():
            s.run()
            n = int(s.cnt.cpu()[1])                                    # (the seeding entry has synchronised already)
            state["n"] = n
            if n and codon:
                pkg.align_pairs_frameshift_device(cfg, Q.set, R.set, n, s.hp.data_ptr(), s.hs.data_ptr(), pkg.STRAND_FORWARD, a.frameshift,
                                                  Q.max_len, PLEN, rec.data_ptr(), won.data_ptr(), stream.cuda_stream)
            elif n:
                pkg.align_pairs_translated_device(cfg, Q.set, R.set, n, s.hp.data_ptr(), s.hs.data_ptr(), 0, mq, PLEN, rec.data_ptr(), None,
                                                  won.data_ptr(), stream.cuda_stream)
        leg = {"seed_extend": wall_ms(seed_extend, a.repeats)}
        n = state["n"]
        leg["candidates"] = n
        pairs = s.hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n]
        best_seed = best_per_read(pairs["q"], pairs["r"], rec.cpu().numpy()[:n, 0], nq)
        cap = 64 * nq + 1024
        hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        hr = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        hb = torch.zeros(cap, dtype=torch.uint8, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)

        def rectangle():
            if codon:
                pkg.search_pairs_frameshift_device(cfg, Q.set, R.set, pkg.PAIRS_RECT, 0, nq * nr, None, Q.max_len, PLEN, a.min_score, hp.data_ptr(), None,
                                                   hr.data_ptr(), cap, cnt.data_ptr(), pkg.STRAND_BOTH, a.frameshift, hb.data_ptr(), stream.cuda_stream)
            else:
                pkg.search_pairs_translated_device(cfg, Q.set, R.set, pkg.PAIRS_RECT, 0, nq * nr, None, mq, PLEN, a.min_score, hp.data_ptr(), None,
                                                   hr.data_ptr(), None, cap, cnt.data_ptr(), pkg.FRAMES_ALL, hb.data_ptr(), stream.cuda_stream)
        t = time.perf_counter()                                        # once, without a warm-up: seconds per run
        rectangle()
        torch.cuda.synchronize(dev)
        leg["rectangle"] = {"median_ms": round((time.perf_counter() - t) * 1e3, 3), "runs": 1, "timing": "one cold run, host wall clock and a synchronisation"}
        c = cnt.cpu().tolist()
        leg["rectangle_pairs"], leg["rectangle_hits"], leg["rectangle_hits_written"] = nq * nr, c[0], c[1]
        ep = hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:c[1]]
        best_rect = best_per_read(ep["q"], ep["r"], hr.cpu().numpy()[:c[1], 0], nq)
        have = best_rect >= 0
        leg["reads_with_a_rectangle_hit"] = round(float(have.sum()) / nq, 5)
        leg["best_rectangle_hit_is_best_candidate"] = round(float((best_seed[have] == best_rect[have]).sum()) / max(1, int(have.sum())), 5)
        leg["best_rectangle_hit_is_the_planted_protein"] = round(float((best_rect[have] == prot[have]).sum()) / max(1, int(have.sum())), 5)
        leg["time_ratio_rectangle_over_seed_extend"] = round(leg["rectangle"]["median_ms"] / leg["seed_extend"]["median_ms"], 2)
        leg["kernel"] = lib.pmx_last_kernel().decode()
        out[road] = leg
        del s, rec, won, hp, hr, hb
        torch.cuda.empty_cache()
    ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--letters", type=int, default=50_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--e2e-reads", type=int, default=2_000)
    ap.add_argument("--e2e-prots", type=int, default=20_000)
    ap.add_argument("--k11", type=int, default=9)
    ap.add_argument("--k20", type=int, default=6)
    ap.add_argument("--min-seeds", type=int, default=2)
    ap.add_argument("--band", type=int, default=4)
    ap.add_argument("--band-nt", type=int, default=12)
    ap.add_argument("--pad", type=int, default=8)
    ap.add_argument("--max-occ", type=int, default=64)
    ap.add_argument("--min-score", type=int, default=70)
    ap.add_argument("--frameshift", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats CSV of a rocprofv3 --kernel-trace --stats run of --parts b")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    parts = a.parts.split(",")
    line = {"bench": "seed_letters", "device": torch.cuda.get_device_name(dev), "seed": a.seed}

    def write():
        s = json.dumps(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(s + "\n")
        return s
    if "a" in parts or "b" in parts:
        idx, R = proteins(rng, a.letters // PLEN)
        line["index_aa11"], ix = part_index(a, idx, R, "aa11", a.k11)
        write()
        if "a" in parts:
            line["index_aa20"], other = part_index(a, idx, R, "aa20", a.k20)
            other.close()
            write()
        if "b" in parts:
            line["seed_pairs"] = part_seed(a, rng, idx, ix)
            write()
        ix.close()
        del idx, R
        torch.cuda.empty_cache()
    if "c" in parts:
        line["end_to_end"] = part_e2e(a, rng)
    print(write(), flush=True)


if __name__ == "__main__":
    main()
