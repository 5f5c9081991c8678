#!/usr/bin/env python3
"""The ungapped diagonal filter (pmx_seed_filter_device) between seeding and extension, on an MI355X.  Not a test; every input comes
from --seed.  Shapes, those of bench_seed_letters.py and bench_seed.py:

  frames   --reads reads of 150 nt seeded in six frames against an aa11 index of --letters protein letters (the list of about 42
           mostly chance candidates per read), BLOSUM62, extension pmx_align_pairs_translated_device
  small    --e2e-reads reads against --e2e-prots proteins, the same road
  dna      --reads DNA reads of 150 nt on both strands against --ref-bp of reference, match 2 / mismatch -3, extension
           pmx_align_pairs_ex_device

Per shape, in one process, the two roads alternating call by call, after the spread of repeats of the same call:
  spread   the filter call over the seeded list, repeated: median / min / max
  a        the filter (scores of every candidate + the selection, top_n 0, min_score 0) against the extension over the same list; the
           share of resolve + gather in the filter comes from a `rocprofv3 --kernel-trace --stats` run of `--legs filter` alone, whose
           CSV --kernel-stats names
  b        seed + filter (top_n 1, 2, 4, 8; min_score 0) + extension of the survivors against seed + extension of all
  c        per top_n the share of reads whose best-scoring candidate ON THE UNFILTERED ROAD (the first of equals) survives the filter

One warm-up per timed leg, then --repeats runs.  One JSON line; --out FILE writes it there as well (default profiles/bench_seed_filter.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bench_seed_letters as bl  # noqa: E402  (torch's HIP runtime first, the package, the planted sets)
import bench_seed as bd  # noqa: E402

torch, pkg, lib, dev, stream = bl.torch, bl.pkg, bl.lib, bl.dev, bl.stream
TOP_N = (1, 2, 4, 8)


def stats(runs):
    return {"median_ms": round(float(np.median(runs)), 3), "min_ms": round(min(runs), 3), "max_ms": round(max(runs), 3), "runs": len(runs)}


def alternate(legs, repeats):
    """legs: {name: fn}.  One warm-up each, then `repeats` rounds in which every leg runs once, in turn; host wall clock around the call
    and a device synchronisation."""
    for fn in legs.values():
        fn()
        torch.cuda.synchronize(dev)
    runs = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            runs[k].append((time.perf_counter() - t) * 1e3)
    return {k: stats(v) for k, v in runs.items()}


class Filter:
    """the filter over a Seeder's list into buffers of its own"""

    def __init__(self, Q, R, s, kind, matrix, mq, mr):
        self.Q, self.R, self.s, self.kind, self.matrix, self.mq, self.mr = Q, R, s, kind, matrix, mq, mr
        cap = self.cap = s.cap
        self.op = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        self.ob = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.ou = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.src = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.off = torch.zeros(Q.n + 1, dtype=torch.int64, device=dev)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def run(self, n, top_n):
        s = self.s
        pkg.seed_filter_device(self.Q.set, self.R.set, n, s.hp.data_ptr(), s.hs.data_ptr(), s.hd.data_ptr(), self.mq, self.mr, self.matrix, self.Q.n,
                               s.off.data_ptr(), self.op.data_ptr(), self.ob.data_ptr(), None, self.ou.data_ptr(), self.src.data_ptr(), self.cap,
                               self.off.data_ptr(), self.cnt.data_ptr(), kind=self.kind, top_n=top_n, stream=stream.cuda_stream)


def best_index_per_row(score, row_off, n):
    """per row the list index of its best-scoring candidate, the first of equals; -1 for an empty row (on the device)"""
    rows = torch.searchsorted(row_off[1:].contiguous(), torch.arange(n, device=dev), right=True)
    order = torch.argsort(score[:n].to(torch.int64), descending=True, stable=True)
    order = order[torch.argsort(rows[order], stable=True)]
    r = rows[order]
    first = torch.ones(n, dtype=torch.bool, device=dev)
    first[1:] = r[1:] != r[:-1]
    best = torch.full((len(row_off) - 1,), -1, dtype=torch.int64, device=dev)
    best[r[first]] = order[first]
    return best


def measure(name, a, Q, R, s, kind, matrix, cfg, mq, mr, extend):
    """extend(n, pairs_ptr, byte_ptr): the shape's extension over a list"""
    s.run()
    n = int(s.cnt.cpu()[1])
    assert int(s.cnt.cpu()[0]) == n, "the candidate buffers are too small for this shape"
    f = Filter(Q, R, s, kind, matrix, mq, mr)
    out = {"shape": name, "reads": Q.n, "candidates": n, "candidates_per_read": round(n / max(1, Q.n), 3), "max_qlen": mq, "max_rlen": mr}
    spans = (s.hd[:n, 2] - s.hd[:n, 1] + 1).to(torch.float64)
    out["mean_span"] = round(float(spans.mean()), 3)
    out["share_span_1"] = round(float((spans == 1).to(torch.float64).mean()), 4)
    if a.legs == "filter":                                               # for the kernel trace: nothing but the filter
        for _ in range(a.repeats + 1):
            f.run(n, 0)
        torch.cuda.synchronize(dev)
        return out
    spread = []
    f.run(n, 0)
    torch.cuda.synchronize(dev)
    for _ in range(a.repeats):
        t = time.perf_counter()
        f.run(n, 0)
        torch.cuda.synchronize(dev)
        spread.append((time.perf_counter() - t) * 1e3)
    out["spread_of_the_same_filter_call"] = stats(spread)
    out["a"] = alternate({"filter": lambda: f.run(n, 0), "extension": lambda: extend(n, s.hp.data_ptr(), s.hs.data_ptr())}, a.repeats)
    out["a"]["extension_over_filter"] = round(out["a"]["extension"]["median_ms"] / out["a"]["filter"]["median_ms"], 2)
    out["kept_at_min_score_0"] = int(f.cnt.cpu()[0])
    # c: the unfiltered road's best candidate per read
    extend(n, s.hp.data_ptr(), s.hs.data_ptr())
    torch.cuda.synchronize(dev)
    best = best_index_per_row(a.rec[:, 0], s.off, n)
    have = best >= 0
    out["reads_with_a_candidate"] = int(have.sum())
    out["b"], out["c"] = {}, {}

    def unfiltered():
        s.run()
        extend(n, s.hp.data_ptr(), s.hs.data_ptr())
    for top_n in TOP_N:
        def filtered():
            s.run()
            f.run(n, top_n)
            kept = int(f.cnt.cpu()[1])
            extend(kept, f.op.data_ptr(), f.ob.data_ptr())
        t = alternate({"seed_filter_extend": filtered, "seed_extend_all": unfiltered}, a.repeats)
        kept = int(f.cnt.cpu()[0])
        t["kept"] = kept
        t["speedup"] = round(t["seed_extend_all"]["median_ms"] / t["seed_filter_extend"]["median_ms"], 3)
        out["b"]["top_%d" % top_n] = t
        mark = torch.zeros(n, dtype=torch.bool, device=dev)
        mark[f.src[:kept]] = True
        out["c"]["top_%d" % top_n] = round(float(mark[best[have]].to(torch.float64).mean()), 5)
    return out


def shape_frames(a, rng, name, nprot, nreads):
    idx, R = bl.proteins(rng, nprot)
    ix = pkg.SeedIndex.build(R.set, a.k11, alphabet="aa11", stream=stream.cuda_stream)
    Q, prot, at = bl.planted_reads(rng, idx, nreads)
    mq = Q.max_len // 3
    opts = SimpleNamespace(min_seeds=2, band=4, band_nt=12, pad=8, max_occ=64)
    s = bl.Seeder(Q, ix, a.cap_per_read * nreads + 1024, opts, "all", mq)
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, m.inner)
    a.rec = torch.zeros((s.cap, 4), dtype=torch.int32, device=dev)
    won = torch.zeros(s.cap, dtype=torch.uint8, device=dev)

    def extend(n, pairs, byte):
        if n:
            pkg.align_pairs_translated_device(cfg, Q.set, R.set, n, pairs, byte, 0, mq, bl.PLEN, a.rec.data_ptr(), None, won.data_ptr(), stream.cuda_stream)
    out = measure(name, a, Q, R, s, "frame", m, cfg, mq, bl.PLEN, extend)
    out["matrix"] = "blosum62, gaps 11 / 1"
    ix.close()
    del s, a.rec, won
    torch.cuda.empty_cache()
    return out


def shape_dna(a, rng):
    nseq = 20
    genome = bd.ACGT[rng.integers(0, 4, size=a.ref_bp)]
    off = (np.arange(nseq + 1, dtype=np.int64) * (a.ref_bp // nseq))
    off[-1] = a.ref_bp
    R = bd.DevSet(genome, off)
    ix = pkg.SeedIndex.build(R.set, a.k, stream.cuda_stream)
    buf, qoff, pos = bd.planted_reads(rng, genome, a.reads)
    Q = bd.DevSet(buf, qoff)
    opts = SimpleNamespace(min_seeds=3, band=8, pad=16, max_occ=64)
    s = bd.Seeder(Q, ix, 8 * a.reads + 1024, opts)
    s.run()
    n = int(s.cnt.cpu()[1])
    mr = int(s.hp.view(torch.int32).view(-1, 8)[:n, 7].max()) if n else 1                  # the longest window of the list
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, 0, m.inner)
    a.rec = torch.zeros((s.cap, 4), dtype=torch.int32, device=dev)

    def extend(n, pairs, byte):
        if n:
            bd.check(lib.pmx_align_pairs_ex_device(C.byref(cfg), Q.set.inner, R.set.inner, n, pairs, byte, Q.max_len, mr, a.rec.data_ptr(),
                                                   None, None, None, 0, None, stream.cuda_stream, None))
    out = measure("dna", a, Q, R, s, "strand", m, cfg, Q.max_len, mr, extend)
    out["matrix"] = "match 2 / mismatch -3, gaps 5 / 2"
    ix.close()
    del s, a.rec
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--letters", type=int, default=50_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--e2e-reads", type=int, default=2_000)
    ap.add_argument("--e2e-prots", type=int, default=20_000)
    ap.add_argument("--ref-bp", type=int, default=100_000_000)
    ap.add_argument("--k11", type=int, default=9)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--cap-per-read", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="frames,small,dna")
    ap.add_argument("--legs", default="all", help="`filter`: nothing but the seeding and the filter calls, for a kernel trace")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats CSV of a rocprofv3 --kernel-trace --stats run of --legs filter --shapes frames")
    ap.add_argument("--out", default=os.path.join(HERE, "bench_seed_filter.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    line = {"bench": "seed_filter", "device": torch.cuda.get_device_name(dev), "seed": a.seed, "legs": a.legs,
            "timing": "host wall clock around the call(s) and a device synchronisation; the roads of a comparison alternate call by call",
            "kernel_shape": dict(zip(("lanes_per_candidate", "cells_per_lane_step"), pkg.ungapped_shape()))}

    def write():
        text = json.dumps(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(text + "\n")
        return text
    for shape in a.shapes.split(","):
        if shape == "frames":
            line["frames"] = shape_frames(a, rng, "frames", a.letters // bl.PLEN, a.reads)
        elif shape == "small":
            line["small"] = shape_frames(a, rng, "small", a.e2e_prots, a.e2e_reads)
        elif shape == "dna":
            line["dna"] = shape_dna(a, rng)
        write()
    if a.kernel_stats:
        rows = bl.trace_rows(a.kernel_stats)
        mine = [r for r in rows if "pmx_ungap" in r["kernel"] or "pmx_pairs_resolve" in r["kernel"] or "pmx_pairs_gather" in r["kernel"]]
        total = sum(r["total_ms"] for r in mine)
        prep = sum(r["total_ms"] for r in mine if "pmx_pairs" in r["kernel"])
        line["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats of `--legs filter --shapes frames` alone (seeding, warm-up and the filter calls)",
                                "rows": rows[:24], "filter_kernels": mine,
                                "share_is": "resolve + gather over resolve + gather + the pmx_ungap kernels; rocPRIM's kernels serve the seeding too and are left out",
                                "resolve_and_gather_share_of_the_filter": round(prep / total, 4) if total else None}
    print(write(), flush=True)


if __name__ == "__main__":
    main()
