#!/usr/bin/env python3
"""Sequence-set batches with strands and CIGAR output (pmx_align_pairs_ex[_device]) on an MI355X, at config 4's shape:
156 250 reads of 250 bp x 8 windows of 250 bp of a resident reference set (1.25 M pairs), every other read stored on the reverse
strand, semi-global, gaps 5 / 2, records + CIGAR text + begins.

  (a) pmx_align_pairs_ex_device over the two sets, 32-byte descriptors and strand bytes on the device      (device events)
  (b) pmx_align_batch_cigar_device on the same pairs already packed back to back -- the yardstick          (device events)
  (f) (a) without strand bytes (every read as stored): the forward-only resolve and gather kernels, for the kernel trace;
      not in the default set of variants                                                                   (device events)
  (c) pmx_align_pairs_ex, the host entry: 32 + 1 bytes per pair go up, records, begins and text come back  (wall clock)
  (d) pmx_align_batch_cigar on the pairs materialised on the host: 2 x 250 + 16 bytes per pair go up       (wall clock)

The packed form of (b) and (d) comes from pmx_gather_pairs_device, so all four variants align the same bytes; records, offsets and
text of (a) and (b) are compared.  One warm-up call per variant, then `--repeats` rounds over the variants in turn (alternated);
the JSON line reports median / min / max per variant.  `--out FILE` writes it there as well (profiles/r09/bench_pairs_cigar.json)."""
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


def alternated(legs, repeats):
    """legs: {name: (fn, timer)}; one warm-up each, then `repeats` rounds over all legs in turn"""
    for fn, _ in legs.values():
        fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, (fn, timer) in legs.items():
            times[k].append(timer(fn))
    return {k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                "spread_pct": round(100.0 * (max(v) - min(v)) / float(np.median(v)), 2)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=156_250)
    ap.add_argument("--fold", type=int, default=8)
    ap.add_argument("--chunk-pairs", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(20260901)
    c4 = wl.CFG4
    L, ref_len, nref = c4["len"], 10000, 1250
    reads_n, fold = a.reads, a.fold
    n = reads_n * fold
    refs = wl.DNA[rng.integers(0, 4, size=(nref, ref_len))]
    which = rng.integers(0, nref, size=reads_n)
    start = rng.integers(0, ref_len - L, size=reads_n)
    reads = wl.related_fixed(rng, refs[which[:, None], start[:, None] + np.arange(L)[None, :]], c4["sub"], c4["indel"])
    comp = pkg.complement_table()
    rev = (np.arange(reads_n) % 2).astype(bool)                     # every other read is stored reverse-complemented
    reads[rev] = comp[reads[rev][:, ::-1]]
    pairs = np.zeros(n, dtype=pkg.PAIR_DTYPE)
    pairs["q"] = np.repeat(np.arange(reads_n), fold)
    pairs["q_len"] = -1
    pairs["r"] = rng.integers(0, nref, size=n)
    pairs["r"][::fold] = which                                      # one of the windows is where the read came from
    pairs["r_beg"] = rng.integers(0, ref_len - L, size=n)
    pairs["r_beg"][::fold] = start
    pairs["r_len"] = L
    strand = np.repeat(rev, fold).astype(np.uint8)
    Q = pkg.SeqSet.packed(reads.reshape(-1), wl.uniform_offsets(reads_n, L))
    R = pkg.SeqSet.packed(refs.reshape(-1), wl.uniform_offsets(nref, ref_len))
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SG, 15, c4["open"], c4["ext"], 0, pkg.WANT_CIGAR, m.inner)
    opts = pkg.pmx_pairs_opts_t(a.chunk_pairs)
    cap = n * (L + 16)
    d_pairs = torch.from_numpy(pairs.view(np.uint8)).to(dev)
    d_strand = torch.from_numpy(strand).to(dev)
    # the same pairs packed back to back, for (b) and (d)
    d_q, d_r = torch.zeros(n * L + 16, dtype=torch.uint8, device=dev), torch.zeros(n * L + 16, dtype=torch.uint8, device=dev)
    d_qo, d_ro = torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)
    check(lib.pmx_gather_pairs_device(Q.inner, R.inner, n, d_pairs.data_ptr(), d_strand.data_ptr(), L, L, d_q.data_ptr(), n * L, d_qo.data_ptr(),
                                      d_r.data_ptr(), n * L, d_ro.data_ptr(), None, stream.cuda_stream))
    torch.cuda.synchronize(dev)
    qbuf, rbuf = d_q.cpu().numpy()[:n * L].copy(), d_r.cpu().numpy()[:n * L].copy()
    off = wl.uniform_offsets(n, L)
    assert d_qo.cpu().numpy().tobytes() == off.tobytes() and d_ro.cpu().numpy().tobytes() == off.tobytes()
    out = {k: torch.zeros((n, 4), dtype=torch.int32, device=dev) for k in "abf"}
    text = {k: torch.zeros(cap, dtype=torch.uint8, device=dev) for k in "abf"}
    toff = {k: torch.zeros(n + 1, dtype=torch.int64, device=dev) for k in "abf"}
    d_beg = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    h_out = {k: np.zeros(n, dtype=pkg.RECORD_DTYPE) for k in "cd"}
    h_off = {k: np.zeros(n + 1, dtype=np.int64) for k in "cd"}
    h_beg = np.zeros((n, 2), dtype=np.int32)
    h_text = {}

    def leg_a():
        check(lib.pmx_align_pairs_ex_device(C.byref(cfg), Q.inner, R.inner, n, d_pairs.data_ptr(), d_strand.data_ptr(), L, L, out["a"].data_ptr(),
                                            None, d_beg.data_ptr(), text["a"].data_ptr(), cap, toff["a"].data_ptr(), stream.cuda_stream, C.byref(opts)))

    def leg_f():
        check(lib.pmx_align_pairs_ex_device(C.byref(cfg), Q.inner, R.inner, n, d_pairs.data_ptr(), None, L, L, out["f"].data_ptr(),
                                            None, None, text["f"].data_ptr(), cap, toff["f"].data_ptr(), stream.cuda_stream, C.byref(opts)))

    def leg_b():
        check(lib.pmx_align_batch_cigar_device(C.byref(cfg), n, d_q.data_ptr(), d_qo.data_ptr(), d_r.data_ptr(), d_ro.data_ptr(), L, L,
                                               out["b"].data_ptr(), text["b"].data_ptr(), cap, toff["b"].data_ptr(), stream.cuda_stream))

    def host(key, call):
        cbuf = C.c_void_p()
        check(call(cbuf))
        h_text[key] = C.string_at(cbuf.value, int(h_off[key][n])) if key not in h_text else h_text[key]
        lib.pmx_free(cbuf)

    def leg_c():
        host("c", lambda cbuf: lib.pmx_align_pairs_ex(C.byref(cfg), Q.inner, R.inner, n, pairs.ctypes.data, strand.ctypes.data, h_out["c"].ctypes.data,
                                                      None, h_beg.ctypes.data, C.byref(cbuf), h_off["c"].ctypes.data, C.byref(opts)))

    def leg_d():
        host("d", lambda cbuf: lib.pmx_align_batch_cigar(C.byref(cfg), n, qbuf.ctypes.data, off.ctypes.data, rbuf.ctypes.data, off.ctypes.data,
                                                         h_out["d"].ctypes.data, C.byref(cbuf), h_off["d"].ctypes.data))
    all_legs = {"a_align_pairs_ex_device": (leg_a, event_ms), "b_align_batch_cigar_device": (leg_b, event_ms),
                "f_align_pairs_ex_device_no_strands": (leg_f, event_ms), "c_align_pairs_ex_host": (leg_c, wall_ms), "d_align_batch_cigar_host": (leg_d, wall_ms)}
    legs = {k: v for k, v in all_legs.items() if k[0] in a.legs.split(",")}
    kernels = {}
    for k, (fn, _) in legs.items():
        fn(); torch.cuda.synchronize(dev)
        kernels[k] = lib.pmx_last_kernel().decode()
    res = alternated(legs, a.repeats)
    for k in res:
        res[k]["kernel"] = kernels[k]
        res[k]["tcups"] = round(n * L * L / (res[k]["median_ms"] * 1e-3) / 1e12, 3)
    line = {"bench": "pairs_cigar", "device": torch.cuda.get_device_name(dev), "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")},
            "pairs": n, "chunk_pairs": a.chunk_pairs,
            "shape": "%d reads of %d x %d windows of %d out of %d references of %d bp, %d %% substitutions, %d %% indels, every other read on "
                     "the reverse strand, SG, gaps %d/%d, CIGAR" % (reads_n, L, fold, L, nref, ref_len, round(100 * c4["sub"]), round(100 * c4["indel"]),
                                                                  c4["open"], c4["ext"]),
            "link_bytes_per_pair": {"c": 32 + 1, "d": 2 * L + 16}, "legs": res}
    if "a" in a.legs and "b" in a.legs:
        need = int(toff["b"][n].item())
        line["text_bytes"] = need
        line["a_equals_b"] = bool((out["a"] == out["b"]).all().item() and (toff["a"] == toff["b"]).all().item() and
                                  (text["a"][:need] == text["b"][:need]).all().item())
        line["a_over_b"] = round(res["a_align_pairs_ex_device"]["median_ms"] / res["b_align_batch_cigar_device"]["median_ms"], 4)
    if "c" in a.legs and "d" in a.legs:
        line["c_equals_d"] = bool(h_out["c"].tobytes() == h_out["d"].tobytes() and h_off["c"].tobytes() == h_off["d"].tobytes() and
                                  h_text["c"] == h_text["d"])
        line["d_over_c"] = round(res["d_align_batch_cigar_host"]["median_ms"] / res["c_align_pairs_ex_host"]["median_ms"], 3)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
