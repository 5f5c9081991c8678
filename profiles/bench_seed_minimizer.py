#!/usr/bin/env python3
"""Minimizer seeding (pmx_seed_index_build_minimizers, pmx_seed_pairs_device over a minimizer index) against the stride-1 index, on an
MI355X, on the inputs of profiles/bench_seed.py (same generators, same --seed).  Not a test and no figure is a pass mark.

  a. build: a synthetic reference of --ref-bp letters (20 sequences), k = --k; pmx_seed_index_build, then per w of --ws
     pmx_seed_index_build_minimizers: wall-clock time (both synchronise), entries, pmx_seed_index_bytes.
  b. seeding: --reads noisy 150-nt reads on both strands; the plain index first (w = 1; with min_seeds 3 the parent's road), then the
     minimizer index per w, each per min_seeds of --min-seeds-list: wall-clock time of pmx_seed_pairs_device, candidates, and the share of reads with a candidate
     over their planted locus.  --kernel-stats names the CSV of a `rocprofv3 --kernel-trace --stats` run of `--parts b --ws W
     --min-seeds-list M --repeats 1` alone, whose seed kernels are listed per launch.
  c. seed + extension: --e2e-reads reads against a --e2e-bp reference in windows of 300 overlapping by 150; per w (1: the plain index)
     seed + pmx_align_pairs_ex_device time, candidates, and the share of reads whose planted locus is the best-scoring candidate.

One warm-up call per timed leg, then --repeats runs; median / min / max.  One JSON line; --out FILE writes it there as well."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_seed as B  # noqa: E402  (loads torch first, then the package)

torch, pkg, lib, dev, stream = B.torch, B.pkg, B.lib, B.dev, B.stream


def build(R, k, w):
    """w None: pmx_seed_index_build; else pmx_seed_index_build_minimizers (w = 1 included)"""
    if w is None:
        return pkg.SeedIndex.build(R.set, k, stream.cuda_stream)
    inner = lib.pmx_seed_index_build_minimizers(R.set._handle(), k, w, stream.cuda_stream)
    if not inner:
        raise RuntimeError(lib.pmx_last_error().decode())
    return pkg.SeedIndex(inner, R.set, k)


def timed_build(R, k, w, repeats):
    t = time.perf_counter()
    ix = build(R, k, w)
    first = (time.perf_counter() - t) * 1e3
    runs = []
    for _ in range(repeats):
        t = time.perf_counter()
        other = build(R, k, w)
        runs.append((time.perf_counter() - t) * 1e3)
        other.close()
    return ix, {"w": w, "entry": "pmx_seed_index_build" if w is None else "pmx_seed_index_build_minimizers", "entries": len(ix),
                "index_bytes": ix.nbytes, "first_build_ms": round(first, 2), "build_median_ms": round(float(np.median(runs)), 2),
                "build_min_ms": round(min(runs), 2), "build_max_ms": round(max(runs), 2), "runs": len(runs)}


def seed_leg(a, Q, ix, pos, min_seeds):
    a2 = argparse.Namespace(**vars(a))
    a2.min_seeds = min_seeds
    s = B.Seeder(Q, ix, 8 * Q.n + 1024, a2)
    s.run()
    cnt = s.cnt.cpu().tolist()
    out = {"min_seeds": min_seeds, "candidates": cnt[0], "written": cnt[1], "seed_pairs_device": B.wall_ms(s.run, a.repeats)}
    n = cnt[1]
    pairs = s.hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n]
    strand = s.hs.cpu().numpy()[:n]
    seeds = s.hd.cpu().numpy().reshape(-1).view(pkg.SEED_HIT_DTYPE)[:n]
    seq_len = a.ref_bp // 20
    g_pos = np.minimum(pairs["r"], 19) * seq_len
    q = pairs["q"]
    near = (np.abs(g_pos + (seeds["diag_min"] + seeds["diag_max"]) // 2 - pos[q]) <= 32) & (strand == (q & 1))
    out["reads_with_a_candidate_on_the_planted_locus"] = round(len(np.unique(q[near])) / Q.n, 5)
    return out


def part_e2e(a, rng, ws):
    genome = B.ACGT[rng.integers(0, 4, size=a.e2e_bp)]
    W, step = 300, 150
    starts = np.arange(0, a.e2e_bp - W + 1, step)
    wbuf = genome[starts[:, None] + np.arange(W)[None, :]].reshape(-1)
    R = B.DevSet(wbuf, np.arange(len(starts) + 1, dtype=np.int64) * W)
    buf, off, pos = B.planted_reads(rng, genome, a.e2e_reads)
    Q = B.DevSet(buf, off)
    nq = Q.n
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 16, 0, m.inner)
    legs = []
    for w in ws:
        ix = build(R, a.k, None if w == 1 else w)
        for min_seeds in a.min_seeds_list:
            a2 = argparse.Namespace(**vars(a))
            a2.min_seeds = min_seeds
            s = B.Seeder(Q, ix, 64 * nq, a2)
            rec = torch.zeros((s.cap, 4), dtype=torch.int32, device=dev)
            state = {}

            def seed_extend():
                s.run()
                n = int(s.cnt.cpu()[1])
                state["n"] = n
                if n:
                    B.check(lib.pmx_align_pairs_ex_device(C.byref(cfg), Q.set.inner, R.set.inner, n, s.hp.data_ptr(), s.hs.data_ptr(), Q.max_len, W,
                                                          rec.data_ptr(), None, None, None, 0, None, stream.cuda_stream, None))
            leg = {"w": w, "min_seeds": min_seeds, "entries": len(ix), "seed_extend": B.wall_ms(seed_extend, a.repeats)}
            n = state["n"]
            leg["candidates"] = n
            pairs = s.hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n]
            strand = s.hs.cpu().numpy()[:n]
            score = rec.cpu().numpy()[:n, 0]
            q = pairs["q"]
            order = np.lexsort((-score, q))
            first = order[np.concatenate(([True], q[order][1:] != q[order][:-1]))] if n else order
            lo = starts[pairs["r"][first]] + pairs["r_beg"][first]
            hi = lo + pairs["r_len"][first]
            ok = (lo < pos[q[first]] + 150) & (hi > pos[q[first]]) & (strand[first] == (q[first] & 1))
            leg["planted_is_best"] = round(float(ok.sum()) / nq, 5)
            legs.append(leg)
            del s, rec
        ix.close()
    return {"reads": nq, "reference_bp": a.e2e_bp, "windows": R.n, "window": W, "overlap": W - step, "legs": legs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--ref-bp", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--e2e-reads", type=int, default=10_000)
    ap.add_argument("--e2e-bp", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--ws", default="1,5,10,19")
    ap.add_argument("--min-seeds-list", default="1,2,3")
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--pad", type=int, default=16)
    ap.add_argument("--max-occ", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ws = [int(x) for x in a.ws.split(",")]
    a.min_seeds_list = [int(x) for x in a.min_seeds_list.split(",")]
    rng = np.random.default_rng(a.seed)
    parts = a.parts.split(",")
    line = {"bench": "seed_minimizer", "device": torch.cuda.get_device_name(dev), "seed": a.seed, "k": a.k,
            "options": {"band": a.band, "pad": a.pad, "max_occ": a.max_occ, "strand": "both"}}
    if "a" in parts or "b" in parts:
        nseq = 20
        genome = B.ACGT[rng.integers(0, 4, size=a.ref_bp)]
        off = (np.arange(nseq + 1, dtype=np.int64) * (a.ref_bp // nseq))
        off[-1] = a.ref_bp
        R = B.DevSet(genome, off)
        Q = pos = None
        if "b" in parts:
            buf, qoff, pos = B.planted_reads(rng, genome, a.reads)
            Q = B.DevSet(buf, qoff)
            line["seeding"] = {"reads": a.reads, "max_qlen": Q.max_len, "legs": []}
        line["build"] = {"reference_bp": a.ref_bp, "sequences": nseq, "legs": []}
        for w in [None] + ws:
            if w is None and "a" not in parts and 1 not in ws:
                continue
            if "a" in parts:
                ix, leg = timed_build(R, a.k, w, a.repeats)
                line["build"]["legs"].append(leg)
            else:
                ix = build(R, a.k, w)
            if "b" in parts and w != 1:                                 # (w = 1 through the new build is the plain index, entry for entry)
                for min_seeds in a.min_seeds_list:
                    leg = seed_leg(a, Q, ix, pos, min_seeds)
                    leg["w"] = 1 if w is None else w
                    leg["index"] = "pmx_seed_index_build" + (" (the parent's road)" if min_seeds == 3 else "") if w is None else "pmx_seed_index_build_minimizers"
                    line["seeding"]["legs"].append(leg)
            ix.close()
            torch.cuda.empty_cache()
        if a.kernel_stats:
            rows = B.trace_rows(a.kernel_stats)
            line["seeding"]["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats of one (w, min_seeds) leg of --parts b alone, --repeats 1: "
                                                         "the index build, one warm-up and two timed calls",
                                               "rows": [r for r in rows if "seed" in r["kernel"] or "rocprim" in r["kernel"]][:24]}
        del genome, R, Q
        torch.cuda.empty_cache()
    if "c" in parts:
        line["seed_extend"] = part_e2e(a, rng, ws)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
