#!/usr/bin/env python3
"""K-mer seeding (pmx_seed_index_build, pmx_seed_pairs_device) on an MI355X.  Not a test; every input comes from --seed.

  a. index: a synthetic reference of --ref-bp letters (20 sequences), wall-clock time of pmx_seed_index_build (it synchronises),
     entries, resident bytes (hipMemGetInfo before / after) and the build's peak from the same counter.
  b. seed: --reads reads of 150 nt planted in that reference, every other one stored reverse-complemented, with the error rates of
     BASELINE cfg 4 (10 % substitutions, 2 % single-base indels): wall-clock time of pmx_seed_pairs_device (it synchronises once per
     slice), candidates, the share of reads with a candidate over their planted locus, and a MODEL of the bytes the lookup kernel
     touches (k query bytes, two bucket numbers and one 8-byte key per probe of the binary search, per position) against the time of
     that kernel when --kernel-stats names the CSV of a `rocprofv3 --kernel-trace --stats` run of `--parts b` alone.
  c. end to end: --e2e-reads reads against a --e2e-bp reference cut into windows of 300 that overlap by 150.  (1) seed + extend:
     pmx_seed_pairs_device, then pmx_align_pairs_ex_device over the candidates; (2) exhaustive: pmx_search_pairs_stranded_device,
     PMX_PAIRS_RECT, both strands, min_score 120.  Times, their ratio, and for each road the share of planted reads whose best-scoring
     candidate / hit lies on the planted locus and strand.

One warm-up call per timed leg, then --repeats runs; median / min / max.  One JSON line; --out FILE writes it there as well."""
import argparse
import csv
import ctypes as C
import json
import math
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
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for a_, b_ in zip(b"ACGT", b"TGCA"):
    COMP[a_] = b_
HBM_PEAK = 8.0e12                                                     # bytes / s, the card's specification


def check(rc):
    if rc:
        raise RuntimeError(lib.pmx_last_error().decode())


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


def planted_reads(rng, genome, n, L=150, sub=0.10, indel=0.02):
    """n reads of L letters of `genome` (one array) with substitutions and single-base indels; odd reads reverse-complemented.
    -> (packed buffer, offsets, planted positions)"""
    if n > 100_000:                                                    # in pieces: the index arrays of a million reads are gigabytes
        parts = [planted_reads(rng, genome, min(100_000, n - k), L, sub, indel) for k in range(0, n, 100_000)]
        off = np.concatenate([[0]] + [p[1][1:] + sum(int(q[1][-1]) for q in parts[:i]) for i, p in enumerate(parts)]).astype(np.int64)
        return np.concatenate([p[0] for p in parts]), off, np.concatenate([p[2] for p in parts])
    pos = rng.integers(0, len(genome) - L, size=n)
    base = genome[pos[:, None] + np.arange(L)[None, :]]
    flip = rng.random(base.shape) < sub
    base[flip] = ACGT[rng.integers(0, 4, size=int(flip.sum()))]
    u = rng.random(base.shape)
    two = np.full((n, L, 2), 255, dtype=np.uint8)                      # [inserted letter or none, the letter or none (deleted)]
    two[:, :, 1] = np.where(u < indel / 2, 255, base)
    ins = (u >= indel / 2) & (u < indel)
    two[:, :, 0][ins] = ACGT[rng.integers(0, 4, size=int(ins.sum()))]
    keep = two != 255
    lens = keep.reshape(n, -1).sum(axis=1)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    buf = two[keep]
    for k in range(1, n, 2):                                           # odd reads: stored reverse-complemented
        buf[off[k]:off[k + 1]] = COMP[buf[off[k]:off[k + 1]][::-1]]
    return buf, off, pos


class DevSet:
    def __init__(self, buf, off):
        self.n, self.bytes = len(off) - 1, int(off[-1])
        self.keep = [torch.from_numpy(np.concatenate([buf, np.zeros(16, dtype=np.uint8)])).to(dev), torch.from_numpy(off).to(dev)]
        self.set = pkg.SeqSet.wrap_device(self.keep[0].data_ptr(), self.keep[1].data_ptr(), self.n, self.bytes, keep=self.keep)
        self.max_len = int(np.diff(off).max()) if self.n else 0


class Seeder:
    def __init__(self, Q, ix, cap, a):
        self.Q, self.ix, self.cap, self.a = Q, ix, cap, a
        self.hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        self.hs = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.hd = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.off = torch.zeros(Q.n + 1, dtype=torch.int64, device=dev)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def run(self):
        a = self.a
        pkg.seed_pairs_device(self.Q.set, self.ix, 0, self.Q.n, self.Q.max_len, self.hp.data_ptr(), self.hs.data_ptr(), self.hd.data_ptr(), self.cap,
                              self.off.data_ptr(), self.cnt.data_ptr(), strand="both", min_seeds=a.min_seeds, band=a.band, pad=a.pad,
                              max_occ=a.max_occ, stream=stream.cuda_stream)


def part_index(a, rng):
    nseq = 20
    genome = ACGT[rng.integers(0, 4, size=a.ref_bp)]
    off = (np.arange(nseq + 1, dtype=np.int64) * (a.ref_bp // nseq))
    off[-1] = a.ref_bp
    R = DevSet(genome, off)
    free0 = free_bytes()
    t = time.perf_counter()
    ix = pkg.SeedIndex.build(R.set, a.k, stream.cuda_stream)
    first_ms = (time.perf_counter() - t) * 1e3
    resident = free0 - free_bytes()
    runs = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        other = pkg.SeedIndex.build(R.set, a.k, stream.cuda_stream)
        runs.append((time.perf_counter() - t) * 1e3)
        other.close()
    out = {"reference_bp": a.ref_bp, "sequences": nseq, "k": a.k, "entries": len(ix), "first_build_ms": round(first_ms, 2),
           "build_ms": {"median_ms": round(float(np.median(runs)), 2), "min_ms": round(min(runs), 2), "max_ms": round(max(runs), 2), "runs": len(runs),
                        "timing": "host wall clock around pmx_seed_index_build, which allocates, sorts and synchronises"},
           "resident_bytes": resident, "resident_bytes_per_entry": round(resident / max(1, len(ix)), 2),
           "resident_is": "hipMemGetInfo before / after the build: 16 bytes per byte of the set and the bucket table",
           "transient_bytes_model": 2 * 8 * a.ref_bp, "transient_is": "the unsorted keys and values, freed at the end of the build (plus rocPRIM's scratch)"}
    return out, genome, R, ix


def lookup_model(a, positions, entries):
    nb = 1 << min(2 * a.k, 22)
    probes = max(1.0, math.log2(max(2.0, entries / nb))) + 2
    return positions * (a.k + 8 + 8 * probes), probes


def trace_rows(path):
    rows = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name") or r.get("KernelName") or ""
            rows.append({"kernel": name[:160], "calls": int(r.get("Calls", 0)), "total_ms": round(float(r.get("TotalDurationNs", 0)) / 1e6, 4),
                         "percent": float(r.get("Percentage", 0))})
    return sorted(rows, key=lambda r: -r["total_ms"])


def part_seed(a, rng, genome, ix):
    buf, off, pos = planted_reads(rng, genome, a.reads)
    Q = DevSet(buf, off)
    s = Seeder(Q, ix, 4 * a.reads + 1024, a)
    free0 = free_bytes()
    s.run()
    scratch = free0 - free_bytes()
    cnt = s.cnt.cpu().tolist()
    out = {"reads": a.reads, "read_letters": "150 before indels; 10 % substitutions, 2 % single-base indels; odd reads stored reverse-complemented",
           "max_qlen": Q.max_len, "options": {"k": a.k, "min_seeds": a.min_seeds, "band": a.band, "pad": a.pad, "max_occ": a.max_occ, "strand": "both"},
           "candidates": cnt[0], "written": cnt[1], "scratch_bytes": scratch}
    out["seed_pairs_device"] = wall_ms(s.run, a.repeats)
    # planted locus among the candidates (host check on what was written)
    n = cnt[1]
    pairs = s.hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n]
    strand = s.hs.cpu().numpy()[:n]
    seeds = s.hd.cpu().numpy().reshape(-1).view(pkg.SEED_HIT_DTYPE)[:n]
    seq_len = a.ref_bp // 20
    g_pos = np.minimum(pairs["r"], 19) * seq_len                       # (global start of the candidate's sequence; the last one is longer)
    q = pairs["q"]
    near = (np.abs(g_pos + (seeds["diag_min"] + seeds["diag_max"]) // 2 - pos[q]) <= 32) & (strand == (q & 1))
    out["reads_with_a_candidate_on_the_planted_locus"] = round(len(np.unique(q[near])) / a.reads, 5)
    positions = int(2 * (np.maximum(np.diff(off) - a.k + 1, 0)).sum())
    model, probes = lookup_model(a, positions, len(ix))
    out["lookup_model"] = {"positions": positions, "probes_per_lookup": round(probes, 2), "bytes": int(model),
                           "note": "a model of the count kernel's traffic (query bytes, bucket numbers, 8-byte keys per probe), not a counter"}
    if a.kernel_stats:
        rows = trace_rows(a.kernel_stats)
        out["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats of `--parts b` alone (index build, one warm-up and the timed calls)",
                               "rows": [r for r in rows if "seed" in r["kernel"] or "rocprim" in r["kernel"]][:24]}
        look = [r for r in rows if "pmx_seed_count_kernel" in r["kernel"]]
        if look and look[0]["calls"]:
            per_call_s = look[0]["total_ms"] / 1e3 / look[0]["calls"]
            slices = math.ceil(a.reads / max(1, (256 << 20) // (2 * Q.max_len * 16)))
            rate = model / slices / per_call_s
            out["lookup_model"].update({"count_kernel_ms_per_launch": round(per_call_s * 1e3, 4), "launches_per_call": slices,
                                        "modelled_bytes_per_s": round(rate, 1), "share_of_hbm_peak_8e12": round(rate / HBM_PEAK, 4)})
    return out


def part_e2e(a, rng):
    genome = ACGT[rng.integers(0, 4, size=a.e2e_bp)]
    W, step = 300, 150
    starts = np.arange(0, a.e2e_bp - W + 1, step)
    wbuf = genome[starts[:, None] + np.arange(W)[None, :]].reshape(-1)
    R = DevSet(wbuf, np.arange(len(starts) + 1, dtype=np.int64) * W)
    buf, off, pos = planted_reads(rng, genome, a.e2e_reads)
    Q = DevSet(buf, off)
    nq, nr = Q.n, R.n
    t = time.perf_counter()
    ix = pkg.SeedIndex.build(R.set, a.k, stream.cuda_stream)
    build_ms = (time.perf_counter() - t) * 1e3
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 16, 0, m.inner)
    s = Seeder(Q, ix, 64 * nq, a)
    rec = torch.zeros((s.cap, 4), dtype=torch.int32, device=dev)
    state = {}

    def seed_extend():
        s.run()
        n = int(s.cnt.cpu()[1])                                        # (the seeding entry has synchronised already)
        state["n"] = n
        if n:
            check(lib.pmx_align_pairs_ex_device(C.byref(cfg), Q.set.inner, R.set.inner, n, s.hp.data_ptr(), s.hs.data_ptr(), Q.max_len, W, rec.data_ptr(),
                                                None, None, None, 0, None, stream.cuda_stream, None))
    out = {"reads": nq, "reference_bp": a.e2e_bp, "windows": nr, "window": W, "overlap": W - step, "index_build_ms": round(build_ms, 2),
           "seed_extend": wall_ms(seed_extend, a.repeats)}
    n = state["n"]
    out["candidates"] = n
    pairs = s.hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n]
    strand = s.hs.cpu().numpy()[:n]
    score = rec.cpu().numpy()[:n, 0]

    def planted_is_best(q, r, r_beg, r_len, st, sc):
        """share of reads whose best-scoring entry (first of equals) overlaps the planted locus on the planted strand"""
        order = np.lexsort((-sc, q))
        first = order[np.concatenate(([True], q[order][1:] != q[order][:-1]))]
        lo = starts[r[first]] + r_beg[first]
        hi = lo + r_len[first]
        ok = (lo < pos[q[first]] + 150) & (hi > pos[q[first]]) & (st[first] == (q[first] & 1))
        return round(float(ok.sum()) / nq, 5)
    out["seed_extend_planted_is_best"] = planted_is_best(pairs["q"], pairs["r"], pairs["r_beg"], pairs["r_len"], strand, score)
    # the exhaustive rectangle on both strands
    cap = 8 * nq + 1024
    hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
    hi = torch.zeros(cap, dtype=torch.int64, device=dev)
    hr = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
    hb = torch.zeros(cap, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def exhaustive():
        check(lib.pmx_search_pairs_stranded_device(C.byref(cfg), Q.set.inner, R.set.inner, pkg.PAIRS_RECT, 0, nq * nr, None, Q.max_len, W, a.min_score,
                                                   hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), None, cap, cnt.data_ptr(), stream.cuda_stream, None,
                                                   pkg.STRAND_BOTH, hb.data_ptr()))
    out["exhaustive"] = wall_ms(exhaustive, max(1, a.repeats // 2))
    c = cnt.cpu().tolist()
    out["exhaustive_pairs"], out["exhaustive_hits"], out["exhaustive_min_score"] = nq * nr, c[0], a.min_score
    ep = hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:c[1]]
    out["exhaustive_planted_is_best"] = planted_is_best(ep["q"], ep["r"], np.zeros(c[1], dtype=np.int64), np.full(c[1], W), hb.cpu().numpy()[:c[1]],
                                                        hr.cpu().numpy()[:c[1], 0])
    out["time_ratio_exhaustive_over_seed_extend"] = round(out["exhaustive"]["median_ms"] / out["seed_extend"]["median_ms"], 2)
    out["kernel"] = lib.pmx_last_kernel().decode()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--ref-bp", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--e2e-reads", type=int, default=10_000)
    ap.add_argument("--e2e-bp", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--min-seeds", type=int, default=3)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--pad", type=int, default=16)
    ap.add_argument("--max-occ", type=int, default=64)
    ap.add_argument("--min-score", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats CSV of a rocprofv3 --kernel-trace --stats run of --parts b")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    parts = a.parts.split(",")
    line = {"bench": "seed", "device": torch.cuda.get_device_name(dev), "seed": a.seed}
    if "a" in parts or "b" in parts:
        line["index"], genome, R, ix = part_index(a, rng)
        if "b" in parts:
            line["seed_pairs"] = part_seed(a, rng, genome, ix)
        ix.close()
        del genome, R
        torch.cuda.empty_cache()
    if "c" in parts:
        line["end_to_end"] = part_e2e(a, rng)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
