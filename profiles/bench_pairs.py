#!/usr/bin/env python3
"""Sequence-set batches (pmx_align_pairs / pmx_align_all_pairs) on an MI355X.

  1. materialisation cost -- config 2's shape (1 M pairs of 150 x 150, local, DNA, every sequence used once), device-resident,
     device-event timing: (a) pmx_align_pairs_device over two wrapped sets and 1 M whole-sequence descriptors against
     (b) pmx_align_batch_device on the same pairs already packed (the yardstick);
  2. what the feature buys -- the same shape with 8-fold reuse (125 k reads x 8 windows each of one resident reference set), host
     entries, wall clock: (c) pmx_align_pairs with the sets created beforehand (32 bytes per pair cross the link) against
     (d) pmx_align_batch on the pairs materialised on the host (300 bytes per pair);
  3. all-vs-all of 4 000 synthetic proteins (8 M pairs, BLOSUM62, local), pmx_align_all_pairs_device, as TCUPS.

One warm-up call per leg, then `--repeats` rounds that run the legs of a part once each in turn (alternated); the JSON line reports
median / min / max per leg.  `--out FILE` writes it there as well (profiles/r06/bench_pairs.json)."""
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
import workloads as wl  # noqa: E402

pkg = g.load_pkg()
lib = pkg.lib
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)


def check(rc):
    if rc:
        raise RuntimeError(lib.pmx_last_error().decode())


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternated(legs, repeats, timer):
    """legs: {name: fn}; one warm-up each, then `repeats` rounds over all legs in turn"""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(timer(fn))
    return {k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                "spread_pct": round(100.0 * (max(v) - min(v)) / float(np.median(v)), 2)} for k, v in times.items()}


def whole_pairs(q, r):
    a = np.zeros(len(q), dtype=pkg.PAIR_DTYPE)
    a["q"], a["r"], a["q_len"], a["r_len"] = q, r, -1, -1
    return a


def part_materialisation(n, repeats, chunk_pairs):
    qbuf, qoff, rbuf, roff = wl.make_cfg2(n)
    c = wl.CFG2
    L = c["len"]
    pad = np.zeros(16, dtype=np.uint8)
    d = [torch.from_numpy(x).to(dev) for x in (np.concatenate([qbuf, pad]), qoff, np.concatenate([rbuf, pad]), roff)]
    Q = pkg.SeqSet.wrap_device(d[0].data_ptr(), d[1].data_ptr(), n, len(qbuf), keep=d)
    R = pkg.SeqSet.wrap_device(d[2].data_ptr(), d[3].data_ptr(), n, len(rbuf), keep=d)
    d_pairs = torch.from_numpy(whole_pairs(np.arange(n), np.arange(n)).view(np.uint8)).to(dev)
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, c["open"], c["ext"], 16, 0, m.inner)
    out_a = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    out_b = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    opts = pkg.pmx_pairs_opts_t(chunk_pairs)

    def by_descriptor():
        check(lib.pmx_align_pairs_device(C.byref(cfg), Q.inner, R.inner, n, d_pairs.data_ptr(), L, L, out_a.data_ptr(), None,
                                         stream.cuda_stream, C.byref(opts)))

    def packed():
        check(lib.pmx_align_batch_device(C.byref(cfg), n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), L, L,
                                         out_b.data_ptr(), None, stream.cuda_stream))
    legs = {"a_align_pairs_device": by_descriptor, "b_align_batch_device": packed}
    kernels = {}
    for k, fn in legs.items():
        fn(); torch.cuda.synchronize(dev)
        kernels[k] = lib.pmx_last_kernel().decode()
    res = alternated(legs, repeats, event_ms)
    for k in legs:
        res[k]["kernel"] = kernels[k]
        res[k]["tcups"] = round(n * L * L / (res[k]["median_ms"] * 1e-3) / 1e12, 3)
    return {"pairs": n, "shape": "150 x 150 i.i.d. DNA (config 2 generator), SW, gaps 5/2, every sequence used once",
            "chunk_pairs": chunk_pairs, "records_equal": bool((out_a == out_b).all().item()),
            "a_over_b": round(res["a_align_pairs_device"]["median_ms"] / res["b_align_batch_device"]["median_ms"], 4), "legs": res}


def part_reuse(reads_n, fold, repeats):
    rng = np.random.default_rng(20260601)
    L, ref_len, nref = 150, 10000, 1250
    refs = wl.DNA[rng.integers(0, 4, size=(nref, ref_len))]
    which = rng.integers(0, nref, size=reads_n)
    start = rng.integers(0, ref_len - L - 50, size=reads_n)
    reads = refs[which[:, None], (start[:, None] + 25 + np.arange(L)[None, :])].copy()
    flip = rng.random(reads.shape) < 0.05
    reads[flip] = wl.DNA[rng.integers(0, 4, size=int(flip.sum()))]
    n = reads_n * fold
    pairs = np.zeros(n, dtype=pkg.PAIR_DTYPE)
    pairs["q"] = np.repeat(np.arange(reads_n), fold)
    pairs["q_len"] = -1
    pairs["r"] = rng.integers(0, nref, size=n)
    pairs["r"][::fold] = which                                      # one of the windows is where the read came from
    pairs["r_beg"] = rng.integers(0, ref_len - L - 50, size=n)
    pairs["r_beg"][::fold] = start
    pairs["r_len"] = L
    Q = pkg.SeqSet.packed(reads.reshape(-1), wl.uniform_offsets(reads_n, L))
    R = pkg.SeqSet.packed(refs.reshape(-1), wl.uniform_offsets(nref, ref_len))
    # the host-materialised form of the same pairs
    qbuf = np.ascontiguousarray(reads[pairs["q"]]).reshape(-1)
    rbuf = np.ascontiguousarray(refs[pairs["r"][:, None], pairs["r_beg"][:, None] + np.arange(L)[None, :]]).reshape(-1)
    off = wl.uniform_offsets(n, L)
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 16, 0, m.inner)
    out_c, out_d = np.zeros(n, dtype=pkg.RECORD_DTYPE), np.zeros(n, dtype=pkg.RECORD_DTYPE)

    def by_descriptor():
        check(lib.pmx_align_pairs(C.byref(cfg), Q.inner, R.inner, n, pairs.ctypes.data, out_c.ctypes.data, None, None))

    def materialised():
        check(lib.pmx_align_batch(C.byref(cfg), n, qbuf.ctypes.data, off.ctypes.data, rbuf.ctypes.data, off.ctypes.data, out_d.ctypes.data, None))
    # (c) again over wrapped sets: no offsets on the host, so lengths and validity come from the device and the host scans the flags
    dw = [torch.from_numpy(x).to(dev) for x in (reads.reshape(-1), wl.uniform_offsets(reads_n, L), refs.reshape(-1), wl.uniform_offsets(nref, ref_len))]
    QW = pkg.SeqSet.wrap_device(dw[0].data_ptr(), dw[1].data_ptr(), reads_n, reads.size, keep=dw)
    RW = pkg.SeqSet.wrap_device(dw[2].data_ptr(), dw[3].data_ptr(), nref, refs.size, keep=dw)
    out_w = np.zeros(n, dtype=pkg.RECORD_DTYPE)

    def by_descriptor_wrapped():
        check(lib.pmx_align_pairs(C.byref(cfg), QW.inner, RW.inner, n, pairs.ctypes.data, out_w.ctypes.data, None, None))
    res = alternated({"c_align_pairs_host": by_descriptor, "c_wrapped_sets": by_descriptor_wrapped, "d_align_batch_host": materialised},
                     repeats, wall_ms)
    assert out_w.tobytes() == out_c.tobytes()
    for k in res:
        res[k]["tcups"] = round(n * L * L / (res[k]["median_ms"] * 1e-3) / 1e12, 3)
    return {"pairs": n, "shape": "%d reads of 150 x %d windows of 150 out of %d references of %d bp, SW, gaps 5/2" % (reads_n, fold, nref, ref_len),
            "records_equal": bool(out_c.tobytes() == out_d.tobytes()),
            "link_bytes_per_pair": {"c": 32 + 16, "d": 2 * L + 16 + 16},
            "d_over_c": round(res["d_align_batch_host"]["median_ms"] / res["c_align_pairs_host"]["median_ms"], 3), "legs": res}


def part_all_vs_all(nseq, repeats):
    rng = np.random.default_rng(20260602)
    lens = rng.integers(200, 401, size=nseq)
    seqs = [wl.AA[rng.integers(0, 20, size=int(l))].tobytes() for l in lens]
    S = pkg.SeqSet.new(seqs)
    total = pkg.all_pairs_count(nseq)
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 16, 0, m.inner)
    out = torch.zeros((total, 4), dtype=torch.int32, device=dev)

    def run():
        check(lib.pmx_align_all_pairs_device(C.byref(cfg), S.inner, 0, total, int(lens.max()), out.data_ptr(), None, stream.cuda_stream, None))
    cfg_sorted = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 16, pkg.WANT_SORTED, m.inner)
    out_sorted = torch.zeros((total, 4), dtype=torch.int32, device=dev)

    def run_sorted():                                   # the lengths are ragged: each chunk in length order (the host entry sets this itself)
        check(lib.pmx_align_all_pairs_device(C.byref(cfg_sorted), S.inner, 0, total, int(lens.max()), out_sorted.data_ptr(), None,
                                             stream.cuda_stream, None))
    run(); torch.cuda.synchronize(dev)
    kernel = lib.pmx_last_kernel().decode()
    res = alternated({"all_pairs_device": run, "all_pairs_device_sorted": run_sorted}, repeats, event_ms)
    s = int(lens.sum())
    cells = (s * s - int((lens.astype(np.int64) ** 2).sum())) // 2
    for r in res.values():
        r.update(kernel=kernel, cells=cells, tcups=round(cells / (r["median_ms"] * 1e-3) / 1e12, 3))
    return {"sequences": nseq, "pairs": total, "shape": "synthetic proteins of 200-400 aa, BLOSUM62, SW, gaps 11/1",
            "records_equal": bool((out == out_sorted).all().item()), "legs": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reads", type=int, default=125_000)
    ap.add_argument("--fold", type=int, default=8)
    ap.add_argument("--nseq", type=int, default=4000)
    ap.add_argument("--chunk-pairs", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = {"bench": "pairs", "device": torch.cuda.get_device_name(dev), "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    parts = a.parts.split(",")
    if "1" in parts:
        line["materialisation"] = part_materialisation(a.n, a.repeats, a.chunk_pairs)
    if "2" in parts:
        line["reuse"] = part_reuse(a.reads, a.fold, a.repeats)
    if "3" in parts:
        line["all_vs_all"] = part_all_vs_all(a.nseq, a.repeats)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
