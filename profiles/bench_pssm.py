"""PSSM batches against the square matrix they came from, in one process.

Shapes: (a) config 3's -- one 300-aa query, 100 k references of 4.5-5 kaa, global with statistics -- with BLOSUM62 and with
blosum62.to_pssm(query); (b) the same query / PSSM, local, score only.  The two matrices alternate and repeat, so the spread shows.
Also the route a PSSM had before batches took one: one Aligner.align() per pair, on a 2 000-pair sample (pairs/s).
Prints one JSON document; --out writes it to a file too.

  python profiles/bench_pssm.py [--n 100000] [--reps 5] [--steps 5] [--out profiles/r07/bench_pssm.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--single", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch                                            # (loaded before the library: torch's HIP runtime comes first)
    import __graft_entry__ as g
    import workloads as wl
    pkg = g.load_pkg()
    dev = torch.device("cuda:0")
    c = wl.CFG3
    q, rbuf, roff = wl.make_cfg3(a.n)
    n = a.n
    d_r = torch.from_numpy(rbuf).to(dev)
    d_roff = torch.from_numpy(roff).to(dev)
    d_out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    d_st = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    max_rlen = int((roff[1:] - roff[:-1]).max())
    cells = c["qlen"] * int(roff[-1])
    square = pkg.Matrix.from_name("blosum62")
    pssm = square.to_pssm(q)
    stream = torch.cuda.current_stream()
    shapes = {"a_nw_stats": (pkg.MODE_NW, 16, pkg.WANT_STATS), "b_sw_score": (pkg.MODE_SW, 0, 0)}
    res = {"workload": "one 300-aa query x %d references of 4.5-5 kaa, BLOSUM62 gaps 11/1" % n, "cells": cells, "shapes": {}}

    def timed(cfg, prof, want_stats):
        st = d_st.data_ptr() if want_stats else None
        for _ in range(2):
            pkg.align_profile_batch_device(cfg, prof, n, d_r.data_ptr(), d_roff.data_ptr(), max_rlen, d_out.data_ptr(), st, stream.cuda_stream)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            pkg.align_profile_batch_device(cfg, prof, n, d_r.data_ptr(), d_roff.data_ptr(), max_rlen, d_out.data_ptr(), st, stream.cuda_stream)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    for name, (mode, width, want) in shapes.items():
        ms = {"square": [], "pssm": []}
        kern = {}
        outs = {}
        for rep in range(a.reps):
            for label, m in (("square", square), ("pssm", pssm)) if rep % 2 == 0 else (("pssm", pssm), ("square", square)):
                cfg = pkg.pmx_config_t(mode, 0, c["open"], c["ext"], width, want, m.inner)
                prof = pkg.Profile.new(q, bool(want), m)
                ms[label].append(timed(cfg, prof, bool(want)))
                kern[label] = pkg.lib.pmx_last_kernel().decode()
                outs[label] = (d_out.cpu().numpy()[:, :3].copy(), d_st.cpu().numpy().copy() if want else None)
        same = bool((outs["square"][0] == outs["pssm"][0]).all() and (not want or (outs["square"][1] == outs["pssm"][1]).all()))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res["shapes"][name] = {"ms": ms, "median_ms": med, "pssm_over_square": med["pssm"] / med["square"],
                               "tcups": {k: cells / (v * 1e-3) / 1e12 for k, v in med.items()},
                               "kernels": kern, "pssm_equals_square": same}
    # the old route: one align() per pair with the PSSM (global, statistics), on a sample
    m = min(a.single, n)
    refs = [rbuf[roff[k]:roff[k + 1]].tobytes() for k in range(m)]
    al = pkg.Aligner.new().global_().matrix(pssm).gap_open(c["open"]).gap_extend(c["ext"]).solution_width(16).use_stats().build()
    al.align(q, refs[0]).get_score()
    t0 = time.perf_counter()
    for r in refs:
        al.align(q, r).get_score()
    t = time.perf_counter() - t0
    single_pps = m / t
    batch_pps = n / (res["shapes"]["a_nw_stats"]["median_ms"]["pssm"] * 1e-3)
    res["one_align_per_pair"] = {"pairs": m, "pairs_per_s": single_pps, "batch_pairs_per_s": batch_pps,
                                 "batch_speedup": batch_pps / single_pps}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
