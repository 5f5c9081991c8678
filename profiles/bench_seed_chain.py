#!/usr/bin/env python3
"""Seed chaining (pmx_seed_chains_device) against the diagonal-cluster road (pmx_seed_pairs_device) on the same minimizer index in the
same process, on an MI355X.  Not a test and no figure is a pass mark: the ratios are what is reported.

  index  a synthetic reference of --ref-bp letters (20 sequences), pmx_seed_index_build_minimizers with k = --k, w = --w.
  long   --long-reads reads of --long-len letters: 10 % substitutions, 2 % single-base indels and --long-indels indels of 50 .. 200
         letters each; odd reads reverse-complemented; both strands seeded.
         (a) wall-clock time of seed_chains_device against seed_pairs_device; --kernel-stats names the CSV of a
             `rocprofv3 --kernel-trace --stats --output-format csv` run of `--parts long --repeats 1` alone, whose kernels are listed (the chain kernel,
             the segmented sort, the two walks).
         (b) candidates per read, and the share of reads whose planted locus is ONE candidate spanning at least 90 % of the read
             (chains: exactly one candidate inside the locus, its q_end - q_beg at least 0.9 of the read).  A cluster has no extent
             along the read, so for the cluster road the figure is the share of reads with exactly one candidate whose diagonals lie
             in the locus' range -- an upper bound of what spans the read.
         (c) the rank of the planted locus among the read's candidates by chain score, against its rank by n_seeds on the cluster road.
  short  --short-reads reads of 150 letters (the shape of DESIGN 2.5p) at lookback 16 and 64 against the cluster road.

One warm-up call per timed leg, then --repeats runs; median / min / max.  One JSON line; --out FILE writes it there as well;
--merge FILE with --kernel-stats adds the trace rows to an earlier line and runs nothing."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_seed as B  # noqa: E402  (loads torch first, then the package)

torch, pkg, lib, dev, stream = B.torch, B.pkg, B.lib, B.dev, B.stream


def long_reads(rng, genome, n, L, big):
    """n reads of about L letters of `genome`: substitutions, single-base indels, then `big` indels of 50 .. 200 letters each (a
    deletion drops letters of the locus, an insertion adds random ones); odd reads stored reverse-complemented.
    -> (buffer, offsets, planted positions, locus lengths)"""
    pos = rng.integers(0, len(genome) - 2 * L, size=n)
    seqs, spans = [], []
    for x in range(n):
        span = L + int(rng.integers(-200, 200))
        s = genome[pos[x]:pos[x] + span].copy()
        flip = rng.random(span) < 0.10
        s[flip] = B.ACGT[rng.integers(0, 4, size=int(flip.sum()))]
        u = rng.random(span)
        parts, last = [], 0
        cuts = sorted(rng.integers(200, span - 400, size=big).tolist())
        small = np.nonzero(u < 0.02)[0]
        events = sorted([(int(p), 1) for p in small] + [(c, int(rng.integers(50, 201))) for c in cuts])
        for p, size in events:
            if p < last:
                continue
            parts.append(s[last:p])
            if rng.random() < 0.5:
                parts.append(B.ACGT[rng.integers(0, 4, size=size)])                       # an insertion in the read
                last = p
            else:
                last = min(span, p + size)                                                   # a deletion from the read
        parts.append(s[last:])
        r = np.concatenate(parts)
        if x & 1:
            r = B.COMP[r[::-1]]
        seqs.append(r)
        spans.append(span)
    off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64)
    return np.concatenate(seqs), off, pos, np.array(spans)


class Chainer:
    def __init__(self, Q, ix, cap, a, lookback):
        self.Q, self.ix, self.cap, self.a, self.lookback = Q, ix, cap, a, lookback
        self.hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        self.hs = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.hd = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.hc = torch.zeros((cap, 8), dtype=torch.int32, device=dev)
        self.off = torch.zeros(Q.n + 1, dtype=torch.int64, device=dev)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def run(self):
        a = self.a
        pkg.seed_chains_device(self.Q.set, self.ix, 0, self.Q.n, self.Q.max_len, self.hp.data_ptr(), self.hs.data_ptr(), self.hd.data_ptr(),
                               self.hc.data_ptr(), self.cap, self.off.data_ptr(), self.cnt.data_ptr(), strand="both", min_seeds=a.min_seeds,
                               min_score=a.min_score, band=a.chain_band, max_gap=a.max_gap, lookback=self.lookback, gap_scale=a.gap_scale,
                               pad=a.pad, max_occ=a.max_occ, stream=stream.cuda_stream)


def rank_of_planted(q, key, planted, nq):
    """per read the rank (1 = best, ties count against) of its planted candidate by `key`; 0 where it has none"""
    rank = np.zeros(nq, dtype=np.int64)
    best = np.full(nq, -1, dtype=np.int64)
    np.maximum.at(best, q[planted], key[planted])
    have = best >= 0
    better = np.zeros(nq, dtype=np.int64)
    np.add.at(better, q, (key > best[q]).astype(np.int64))
    rank[have] = better[have] + 1
    return rank


def summary(rank, nq):
    return {"reads_with_the_planted_locus": round(float((rank > 0).sum()) / nq, 5), "rank_1": round(float((rank == 1).sum()) / nq, 5),
            "rank_le_3": round(float(((rank > 0) & (rank <= 3)).sum()) / nq, 5),
            "mean_rank_where_found": round(float(rank[rank > 0].mean()), 3) if (rank > 0).any() else None}


def part_long(a, rng, genome, goff, ix):
    buf, off, pos, spans = long_reads(rng, genome, a.long_reads, a.long_len, a.long_indels)
    Q = B.DevSet(buf, off)
    nq, lens = Q.n, np.diff(off)
    seq_len = int(goff[1])
    out = {"reads": nq, "mean_len": round(float(lens.mean()), 1), "max_qlen": Q.max_len, "big_indels_per_read": a.long_indels}
    cap = 64 * nq + 1024
    c = Chainer(Q, ix, cap, a, a.lookback)
    c.run()
    cnt = c.cnt.cpu().tolist()
    out["chains"] = {"candidates": cnt[0], "written": cnt[1], "per_read": round(cnt[0] / nq, 3), "seed_chains_device": B.wall_ms(c.run, a.repeats),
                     "options": {"band": a.chain_band, "max_gap": a.max_gap, "lookback": a.lookback, "gap_scale": a.gap_scale, "min_score": a.min_score}}
    n = cnt[1]
    pairs = c.hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n]
    strand = c.hs.cpu().numpy()[:n]
    ch = c.hc.cpu().numpy().reshape(-1).view(pkg.SEED_CHAIN_DTYPE)[:n]
    q = pairs["q"]
    g = pairs["r"] * seq_len + ch["r_beg"]
    planted = (strand == (q & 1)) & (g >= pos[q] - 300) & (g + (ch["r_end"] - ch["r_beg"]) <= pos[q] + spans[q] + 300)
    per = np.bincount(q[planted], minlength=nq)
    wide = planted & ((ch["q_end"] - ch["q_beg"]) >= 0.9 * lens[q])
    one = (per == 1) & (np.bincount(q[wide], minlength=nq) == 1)
    out["chains"]["planted_locus_is_one_candidate_spanning_90_percent"] = round(float(one.sum()) / nq, 5)
    out["chains"]["candidates_over_the_planted_locus_per_read"] = round(float(per.mean()), 3)
    out["chains"]["rank_by_score"] = summary(rank_of_planted(q, ch["score"].astype(np.int64), planted, nq), nq)
    del c
    s = B.Seeder(Q, ix, cap, a)
    s.run()
    cnt = s.cnt.cpu().tolist()
    out["clusters"] = {"candidates": cnt[0], "written": cnt[1], "per_read": round(cnt[0] / nq, 3), "seed_pairs_device": B.wall_ms(s.run, a.repeats),
                       "options": {"band": a.band}}
    n = cnt[1]
    pairs = s.hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n]
    strand = s.hs.cpu().numpy()[:n]
    sd = s.hd.cpu().numpy().reshape(-1).view(pkg.SEED_HIT_DTYPE)[:n]
    q = pairs["q"]
    d = pairs["r"] * seq_len + (sd["diag_min"] + sd["diag_max"]) // 2
    planted = (strand == (q & 1)) & (d >= pos[q] - 300) & (d <= pos[q] + 300 + np.abs(spans[q] - lens[q]) + 200 * a.long_indels)
    per = np.bincount(q[planted], minlength=nq)
    out["clusters"]["planted_locus_is_one_candidate"] = round(float((per == 1).sum()) / nq, 5)
    out["clusters"]["candidates_over_the_planted_locus_per_read"] = round(float(per.mean()), 3)
    out["clusters"]["rank_by_n_seeds"] = summary(rank_of_planted(q, sd["n_seeds"].astype(np.int64), planted, nq), nq)
    out["chains_over_clusters_time"] = round(out["chains"]["seed_chains_device"]["median_ms"] / out["clusters"]["seed_pairs_device"]["median_ms"], 3)
    return out


def part_short(a, rng, genome, ix):
    buf, off, pos = B.planted_reads(rng, genome, a.short_reads)
    Q = B.DevSet(buf, off)
    cap = 8 * Q.n + 1024
    s = B.Seeder(Q, ix, cap, a)
    s.run()
    out = {"reads": Q.n, "max_qlen": Q.max_len, "clusters": {"candidates": s.cnt.cpu().tolist()[0], "seed_pairs_device": B.wall_ms(s.run, a.repeats)},
           "chains": []}
    del s
    for lookback in (16, 64):
        c = Chainer(Q, ix, cap, a, lookback)
        c.run()
        leg = {"lookback": lookback, "candidates": c.cnt.cpu().tolist()[0], "seed_chains_device": B.wall_ms(c.run, a.repeats)}
        leg["chains_over_clusters_time"] = round(leg["seed_chains_device"]["median_ms"] / out["clusters"]["seed_pairs_device"]["median_ms"], 3)
        out["chains"].append(leg)
        del c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--ref-bp", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--w", type=int, default=10)
    ap.add_argument("--long-reads", type=int, default=2000)
    ap.add_argument("--long-len", type=int, default=10_000)
    ap.add_argument("--long-indels", type=int, default=3)
    ap.add_argument("--short-reads", type=int, default=1_000_000)
    ap.add_argument("--min-seeds", type=int, default=3)
    ap.add_argument("--min-score", type=int, default=40)
    ap.add_argument("--band", type=int, default=8, help="the cluster road's band")
    ap.add_argument("--chain-band", type=int, default=500)
    ap.add_argument("--max-gap", type=int, default=5000)
    ap.add_argument("--lookback", type=int, default=64)
    ap.add_argument("--gap-scale", type=int, default=38)
    ap.add_argument("--pad", type=int, default=16)
    ap.add_argument("--max-occ", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="long,short")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as fh:
            line = json.loads(fh.readline())
        rows = B.trace_rows(a.kernel_stats)
        line["long_kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats of --parts long --repeats 1 alone: the index build, then one warm-up, "
                                               "one counted and one timed call of each road",
                                     "rows": [r for r in rows if "seed" in r["kernel"] or "rocprim" in r["kernel"]][:24]}
    else:
        rng = np.random.default_rng(a.seed)
        parts = a.parts.split(",")
        nseq = 20
        genome = B.ACGT[rng.integers(0, 4, size=a.ref_bp)]
        goff = (np.arange(nseq + 1, dtype=np.int64) * (a.ref_bp // nseq))
        goff[-1] = a.ref_bp
        R = B.DevSet(genome, goff)
        ix = pkg.SeedIndex.build(R.set, a.k, stream=stream.cuda_stream, w=a.w)
        line = {"bench": "seed_chain", "device": torch.cuda.get_device_name(dev), "seed": a.seed, "k": a.k, "w": a.w,
                "index": {"reference_bp": a.ref_bp, "sequences": nseq, "entries": len(ix), "index_bytes": ix.nbytes},
                "options": {"min_seeds": a.min_seeds, "pad": a.pad, "max_occ": a.max_occ, "strand": "both"}}
        if "long" in parts:
            line["long"] = part_long(a, rng, genome, goff, ix)
            torch.cuda.empty_cache()
        if "short" in parts:
            line["short"] = part_short(a, rng, genome, ix)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
