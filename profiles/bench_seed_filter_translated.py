#!/usr/bin/env python3
"""The ungapped diagonal filter over the codon and translated-index lists (pmx_seed_filter_translated_device) between seeding and
extension, on an MI355X.  Not a test; every input comes from --seed.  Shapes, those of the roads' own benches:

  frameshift      --reads reads of 149 nt (50 letters back-translated, 5 % substitutions, the middle nucleotide deleted, odd reads
                  reverse-complemented) seeded per strand ("codons-both") against an aa11 index of --prots proteins of 300 letters
                  (bench_seed_letters.py, part e2e); extension pmx_align_pairs_frameshift_device; list kind "codons"
  tblastn_frames  --tprots proteins of 200 .. 400 letters against --tprots / 2 contigs of about 2.5 kb that hold two genes each
                  (bench_seed_translated_ref.py, part b), candidates per sequence frame; extension
                  pmx_align_pairs_translated_ref_device; list kind "ref_frames"
  tblastn_codons  the same with the middle nucleotide of every gene deleted, candidates per strand; extension
                  pmx_align_pairs_frameshift_ref_device; list kind "ref_codons"

Per shape, in one process, the two roads alternating call by call, after the spread of repeats of the same call:
  spread   the filter call over the seeded list, repeated: median / min / max
  a        the filter (records of every candidate + the selection, top_n 0, min_score 0) against the extension over the same list
  b        seed + filter (top_n 1, 2, 4, 8; min_score 0) + extension of the survivors against seed + extension of all -- the road as
           it was before the filter took these lists
  c        per top_n the share of rows whose best-scoring candidate ON THE UNFILTERED ROAD (the first of equals) survives
and once:
  d        the strided form against the stride-1 form: pmx_seed_ungapped_translated_device over the frameshift shape's list
           (pmx_ungapped_kernel<codons>) and pmx_seed_ungapped_device over a frame list ("all") of the same reads cut to the same
           number of cells (pmx_ungapped_kernel, the form that existed before), in cells per second of the whole entry (resolve,
           gather and the kernel); the cells are counted on the host by the header's rule.

One warm-up per timed leg, then --repeats runs.  One JSON line; --out FILE writes it there as well (default
profiles/bench_seed_filter_translated.json)."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bench_seed_letters as bl  # noqa: E402  (torch's HIP runtime first, the package, the planted reads)
import bench_seed_translated_ref as bt  # noqa: E402  (genes and contigs)
from bench_seed_filter import TOP_N, alternate, best_index_per_row, stats  # noqa: E402

torch, pkg, lib, dev, stream = bl.torch, bl.pkg, bl.lib, bl.dev, bl.stream


class RefSeeder:
    """pmx_seed_pairs_translated_ref_device into buffers of its own, with the seed records"""

    def __init__(self, Q, ix, cap, a, road):
        self.Q, self.ix, self.cap, self.a, self.road = Q, ix, cap, a, road
        self.hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        self.hs = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.hd = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.off = torch.zeros(Q.n + 1, dtype=torch.int64, device=dev)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def run(self):
        a, codon = self.a, self.road == "codons"
        pkg.seed_pairs_device(self.Q.set, self.ix, 0, self.Q.n, self.Q.max_len, self.hp.data_ptr(), self.hs.data_ptr(), self.hd.data_ptr(), self.cap,
                              self.off.data_ptr(), self.cnt.data_ptr(), min_seeds=a.min_seeds, band=a.band_nt if codon else a.band,
                              pad=3 * a.pad if codon else a.pad, max_occ=a.max_occ, stream=stream.cuda_stream, ref_frames=self.road)


class Filter:
    """the filter over a seeder's list into buffers of its own"""

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
        pkg.seed_filter_translated_device(self.Q.set, self.R.set, n, s.hp.data_ptr(), s.hs.data_ptr(), s.hd.data_ptr(), self.mq, self.mr, self.matrix,
                                          self.Q.n, s.off.data_ptr(), self.op.data_ptr(), self.ob.data_ptr(), None, self.ou.data_ptr(), self.src.data_ptr(),
                                          self.cap, self.off.data_ptr(), self.cnt.data_ptr(), self.kind, top_n=top_n, stream=stream.cuda_stream)


def measure(name, a, Q, R, s, kind, matrix, mq, mr, extend, rec):
    """extend(n, pairs_ptr, byte_ptr): the shape's extension over a list, records into rec"""
    s.run()
    n = int(s.cnt.cpu()[1])
    assert int(s.cnt.cpu()[0]) == n, "the candidate buffers are too small for this shape"
    f = Filter(Q, R, s, kind, matrix, mq, mr)
    out = {"shape": name, "list_kind": kind, "rows": Q.n, "candidates": n, "candidates_per_row": round(n / max(1, Q.n), 3), "max_qlen": mq, "max_rlen": mr}
    spans = (s.hd[:n, 2] - s.hd[:n, 1] + 1).to(torch.float64)
    out["mean_span"] = round(float(spans.mean()), 3)
    out["share_span_1"] = round(float((spans == 1).to(torch.float64).mean()), 4)
    spread = []
    f.run(n, 0)
    torch.cuda.synchronize(dev)
    out["kernel"] = lib.pmx_last_kernel().decode()
    for _ in range(a.repeats):
        t = time.perf_counter()
        f.run(n, 0)
        torch.cuda.synchronize(dev)
        spread.append((time.perf_counter() - t) * 1e3)
    out["spread_of_the_same_filter_call"] = stats(spread)
    out["a"] = alternate({"filter": lambda: f.run(n, 0), "extension": lambda: extend(n, s.hp.data_ptr(), s.hs.data_ptr())}, a.repeats)
    out["a"]["extension_over_filter"] = round(out["a"]["extension"]["median_ms"] / out["a"]["filter"]["median_ms"], 2)
    out["kept_at_min_score_0"] = int(f.cnt.cpu()[0])
    extend(n, s.hp.data_ptr(), s.hs.data_ptr())                              # c: the unfiltered road's best candidate per row
    torch.cuda.synchronize(dev)
    best = best_index_per_row(rec[:, 0], s.off, n)
    have = best >= 0
    out["rows_with_a_candidate"] = int(have.sum())
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


def floor3(x):
    return np.floor_divide(x, 3)


def cells_of(pairs, seeds, qlen, kind):
    """the cells of every candidate by the header's rule, windows as the seeding entries write them (whole queries, r_len given):
    kind "codons": stream letters qlen - 2, cells n = 3 j - D; kind "frame": letters qlen, cells j - i = d"""
    r_beg, r_len = pairs["r_beg"].astype(np.int64), pairs["r_len"].astype(np.int64)
    lo, hi = seeds[:, 1].astype(np.int64), seeds[:, 2].astype(np.int64)
    total = np.zeros(len(pairs), dtype=np.int64)
    for step in range(int((hi - lo).max()) + 1 if len(pairs) else 0):
        D = lo + step
        on = D <= hi
        if kind == "codons":
            d = D - 3 * r_beg
            L = qlen - 2
            i0, i1 = np.maximum(0, floor3(d + 2)), np.minimum(r_len, floor3(L - 1 + d) + 1)
        else:
            d = D - r_beg
            i0, i1 = np.maximum(0, -d), np.minimum(qlen, r_len - d)
        total += np.where(on, np.maximum(i1 - i0, 0), 0)
    return total


def strided_against_plain(a, Q, R, s_codons, n_codons, ix, m, mq_letters):
    """part d, on the frameshift shape's reads"""
    opts = SimpleNamespace(min_seeds=a.min_seeds, band=a.band, band_nt=a.band_nt, pad=a.pad, max_occ=a.max_occ)
    sf = bl.Seeder(Q, ix, s_codons.cap, opts, "all", mq_letters)
    sf.run()
    n_frame = int(sf.cnt.cpu()[1])
    W = Q.max_len                                                            # (every read has this length)
    pc = s_codons.hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n_codons]
    cc = cells_of(pc, s_codons.hd.cpu().numpy()[:n_codons], W, "codons")
    pf = sf.hp.cpu().numpy().view(pkg.PAIR_DTYPE)[:n_frame]
    fb = sf.hs.cpu().numpy()[:n_frame].astype(np.int64)
    cf = cells_of(pf, sf.hd.cpu().numpy()[:n_frame], (W - fb % 3) // 3, "frame")
    target = int(cc.sum())
    cut = int(np.searchsorted(np.cumsum(cf), target, side="left")) + 1
    cut = min(cut, n_frame)
    out_c = torch.zeros((max(n_codons, 1), 4), dtype=torch.int32, device=dev)
    out_f = torch.zeros((max(cut, 1), 4), dtype=torch.int32, device=dev)

    def strided():
        pkg.seed_ungapped_translated_device(Q.set, R.set, n_codons, s_codons.hp.data_ptr(), s_codons.hs.data_ptr(), s_codons.hd.data_ptr(), W - 2, bl.PLEN, m,
                                            out_c.data_ptr(), "codons", stream=stream.cuda_stream)

    def plain():
        pkg.seed_ungapped_device(Q.set, R.set, cut, sf.hp.data_ptr(), sf.hs.data_ptr(), sf.hd.data_ptr(), mq_letters, bl.PLEN, m, out_f.data_ptr(), kind="frame",
                                 stream=stream.cuda_stream)
    strided()
    torch.cuda.synchronize(dev)
    k_strided = lib.pmx_last_kernel().decode()
    plain()
    torch.cuda.synchronize(dev)
    k_plain = lib.pmx_last_kernel().decode()
    t = alternate({"strided": strided, "plain": plain}, a.repeats)
    cells_plain = int(cf[:cut].sum())
    out = {"strided": dict(t["strided"], kernel=k_strided, candidates=n_codons, cells=target,
                           cells_per_second=round(target / (t["strided"]["median_ms"] * 1e-3))),
           "plain": dict(t["plain"], kernel=k_plain, candidates=cut, of_candidates=n_frame, cells=cells_plain,
                         cells_per_second=round(cells_plain / (t["plain"]["median_ms"] * 1e-3))),
           "timed": "the whole entry: resolve, offset scans, gather and the kernel, one chunk"}
    out["strided_over_plain_cells_per_second"] = round(out["strided"]["cells_per_second"] / max(1, out["plain"]["cells_per_second"]), 3)
    return out


def shape_frameshift(a, rng):
    idx, R = bl.proteins(rng, a.prots)
    ix = pkg.SeedIndex.build(R.set, a.k11, alphabet="aa11", stream=stream.cuda_stream)
    Q, prot, at = bl.planted_reads(rng, idx, a.reads, delete_mid=True)
    mq = Q.max_len // 3
    opts = SimpleNamespace(min_seeds=a.min_seeds, band=a.band, band_nt=a.band_nt, pad=a.pad, max_occ=a.max_occ)
    s = bl.Seeder(Q, ix, 256 * a.reads, opts, "codons-both", mq)
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, m.inner)
    rec = torch.zeros((s.cap, 4), dtype=torch.int32, device=dev)
    won = torch.zeros(s.cap, dtype=torch.uint8, device=dev)

    def extend(n, pairs, byte):
        if n:
            pkg.align_pairs_frameshift_device(cfg, Q.set, R.set, n, pairs, byte, pkg.STRAND_FORWARD, a.frameshift, Q.max_len, bl.PLEN, rec.data_ptr(),
                                              won.data_ptr(), stream.cuda_stream)
    out = measure("frameshift", a, Q, R, s, "codons", m, Q.max_len - 2, bl.PLEN, extend, rec)
    out["matrix"], out["proteins"] = "blosum62, gaps 11 / 1, frameshift %d" % a.frameshift, R.n
    d = strided_against_plain(a, Q, R, s, out["candidates"], ix, m, mq)
    ix.close()
    del s, rec, won
    torch.cuda.empty_cache()
    return out, d


def shape_tblastn(a, rng, road):
    tab, cnt = bt.codon_table()
    nq = a.tprots
    prot_idx = [rng.integers(0, 20, size=int(rng.integers(200, 401)), dtype=np.uint8) for _ in range(nq)]
    off = np.concatenate(([0], np.cumsum([len(p) for p in prot_idx]))).astype(np.int64)
    Q = bt.DevSet(bt.AA[np.concatenate(prot_idx)], off)
    genes = bt.genes_of(rng, prot_idx, tab, cnt, 0.05)
    codon = road == "codons"
    R = bt.contigs_of(rng, genes, 2, 100, 400, codon)
    ix = pkg.SeedIndex.build(R.set, a.k11, alphabet="aa11", translated="both", stream=stream.cuda_stream)
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 0, 0, m.inner)
    s = RefSeeder(Q, ix, 64 * nq, a, road)
    rec = torch.zeros((s.cap, 4), dtype=torch.int32, device=dev)
    won = torch.zeros(s.cap, dtype=torch.uint8, device=dev)
    mr = R.max_len if codon else R.max_len // 3 + 1

    def extend(n, pairs, byte):
        if n and codon:
            pkg.align_pairs_frameshift_ref_device(cfg, Q.set, R.set, n, pairs, byte, pkg.STRAND_FORWARD, a.frameshift, Q.max_len, R.max_len, rec.data_ptr(),
                                                  won.data_ptr(), stream.cuda_stream)
        elif n:
            pkg.align_pairs_translated_ref_device(cfg, Q.set, R.set, n, pairs, byte, 0, Q.max_len, R.max_len // 3 + 1, rec.data_ptr(), None, won.data_ptr(),
                                                  stream.cuda_stream)
    out = measure("tblastn_" + road, a, Q, R, s, "ref_codons" if codon else "ref_frames", m, Q.max_len, mr, extend, rec)
    out["matrix"] = "blosum62, gaps 11 / 1" + (", frameshift %d" % a.frameshift if codon else "")
    out["contigs"], out["contig_bases"] = R.n, R.bytes
    ix.close()
    del s, rec, won
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--reads", type=int, default=2_000)
    ap.add_argument("--prots", type=int, default=20_000)
    ap.add_argument("--tprots", type=int, default=2_000)
    ap.add_argument("--k11", type=int, default=9)
    ap.add_argument("--min-seeds", type=int, default=2)
    ap.add_argument("--band", type=int, default=4)
    ap.add_argument("--band-nt", type=int, default=12)
    ap.add_argument("--pad", type=int, default=8)
    ap.add_argument("--max-occ", type=int, default=64)
    ap.add_argument("--frameshift", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default="frameshift,tblastn_frames,tblastn_codons")
    ap.add_argument("--out", default=os.path.join(HERE, "bench_seed_filter_translated.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    line = {"bench": "seed_filter_translated", "device": torch.cuda.get_device_name(dev), "seed": a.seed,
            "timing": "host wall clock around the call(s) and a device synchronisation; the roads of a comparison alternate call by call",
            "options": {"alphabet": "aa11", "k": a.k11, "min_seeds": a.min_seeds, "band_letters": a.band, "band_nucleotides": a.band_nt, "pad": a.pad,
                        "max_occ": a.max_occ},
            "kernel_shape": dict(zip(("lanes_per_candidate", "cells_per_lane_step"), pkg.ungapped_shape()))}

    def write():
        text = json.dumps(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(text + "\n")
        return text
    for shape in a.shapes.split(","):
        if shape == "frameshift":
            line["frameshift"], line["strided_against_plain"] = shape_frameshift(a, rng)
        elif shape in ("tblastn_frames", "tblastn_codons"):
            line[shape] = shape_tblastn(a, rng, shape.split("_")[1])
        write()
    print(write(), flush=True)


if __name__ == "__main__":
    main()
