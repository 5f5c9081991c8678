#!/usr/bin/env python3
"""Frameshift-aware set search (pmx_search_pairs_frameshift_device, PMX_STRAND_BOTH) on an MI355X, beside the six-frame search.

Workload (profiles/bench_translated.py's): `--nq` reads of 150 nt against `--nr` proteins of 200 - 400 aa, PMX_PAIRS_RECT, BLOSUM62,
gaps 11 / 1, local.  Read i codes, in a random one of the six frames, for a 48-letter piece of protein i % nr with 8 % substitutions,
between random flanks.

  (a) pmx_search_pairs_frameshift_device, PMX_STRAND_BOTH, frameshift `--frameshift`: two codon streams of 148 letters per pair through
      pmx_swfs_kernel, folded, only the hits leave;
  (b) pmx_search_pairs_translated_device, PMX_FRAMES_ALL, in the same library: six translations of about 50 letters per pair through
      the protein kernels, folded, only the hits leave.

The two legs fill equally many cells (2 x 148 x m against 6 x about 50 x m), so a / b is the cost of the wider recurrence.  Device
events around each leg, one warm-up each, then `--repeats` rounds that run the legs in turn; the JSON line reports median / min / max
and a / b.  A second table: the same reads with nucleotide 75 deleted (149 nt), the hits of both roads at the same `--min-score` --
all of them, and those of a read against the protein it was built from.  `--legs a` runs one leg alone (for a kernel trace).
`--out FILE` writes the line there as well."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (torch's HIP runtime first)
import bench_translated as bt  # noqa: E402  (the workload, the timing loop and the hit buffers)

pkg, lib, dev, stream = bt.pkg, bt.lib, bt.dev, bt.stream
W = bt.W
MR = bt.MR


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--nr", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-score", type=int, default=120)
    ap.add_argument("--frameshift", type=int, default=15)
    ap.add_argument("--legs", default="", help="letters of the legs to time (default: all), e.g. a")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nq, nr, min_score, fsp = a.nq, a.nr, a.min_score, a.frameshift
    n = nq * nr
    reads, prots, frames = bt.workload(nq, nr, np.random.default_rng(20261019))
    m = pkg.Matrix.from_name("blosum62")
    cfg_a = pkg.pmx_config_t(pkg.MODE_SW, 0, bt.OPEN, bt.EXT, 0, 0, m.inner)
    cfg_b = pkg.pmx_config_t(pkg.MODE_SW, 0, bt.OPEN, bt.EXT, 16, 0, m.inner)
    R = pkg.SeqSet.new(prots)
    cap = 8 * nq + 1024

    def roads(Q, w):
        ha, hb = bt.Hits(cap), bt.Hits(cap)

        def leg_a():
            bt.check(lib.pmx_search_pairs_frameshift_device(C.byref(cfg_a), Q.inner, R.inner, pkg.PAIRS_RECT, 0, n, None, w - 2, MR, min_score, None,
                                                            ha.hi.data_ptr(), ha.hr.data_ptr(), None, ha.cap, ha.cnt.data_ptr(), stream.cuda_stream, None,
                                                            pkg.STRAND_BOTH, ha.hb.data_ptr(), fsp, None))

        def leg_b():
            bt.check(lib.pmx_search_pairs_translated_device(C.byref(cfg_b), Q.inner, R.inner, pkg.PAIRS_RECT, 0, n, None, w // 3, MR, min_score, None,
                                                            hb.hi.data_ptr(), hb.hr.data_ptr(), None, hb.cap, hb.cnt.data_ptr(), stream.cuda_stream, None,
                                                            pkg.FRAMES_ALL, None, hb.hb.data_ptr()))
        return ha, hb, leg_a, leg_b

    def table(ha, hb, leg_a, leg_b):
        """hits of both roads: all, and those of read i against protein i % nr"""
        out = {}
        for name, h, leg in (("a_frameshift", ha, leg_a), ("b_six_frames", hb, leg_b)):
            leg()
            kernel = lib.pmx_last_kernel().decode()
            index, recs, byte = h.take()
            home = (index % nr) == ((index // nr) % nr)
            out[name] = {"hits": int(h.cnt.cpu()[0]), "home_hits": int(home.sum()), "home_median_score": float(np.median(recs[home, 0])) if home.any() else None,
                         "kernel": kernel}
        return out

    Q = pkg.SeqSet.new(reads)
    ha, hb, leg_a, leg_b = roads(Q, W)
    line = {"bench": "frameshift", "device": torch.cuda.get_device_name(dev), "reads": nq, "proteins": nr, "pairs": n,
            "shape": "150 nt reads coding in a random frame for 48-letter pieces (8 %% substitutions) of proteins of 200 - 400 aa, PMX_PAIRS_RECT, "
                     "SW, BLOSUM62, gaps 11/1; a: PMX_STRAND_BOTH, frameshift %d; b: PMX_FRAMES_ALL" % fsp,
            "min_score": min_score, "frameshift": fsp, "intact_reads": table(ha, hb, leg_a, leg_b),
            "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    # the second table: one nucleotide deleted at mid-read
    cut = [s[:75] + s[76:] for s in reads]
    Qc = pkg.SeqSet.new(cut)
    line["reads_with_nucleotide_75_deleted"] = table(*roads(Qc, W - 1))
    legs = {"a_frameshift_both_strands": leg_a, "b_translated_all_frames": leg_b}
    res = bt.alternated({k: v for k, v in legs.items() if not a.legs or k[0] in a.legs}, a.repeats)
    line["legs"] = res
    if len(res) == 2:
        line["a_over_b"] = round(res["a_frameshift_both_strands"]["median_ms"] / res["b_translated_all_frames"]["median_ms"], 4)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
