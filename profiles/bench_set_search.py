#!/usr/bin/env python3
"""Set search (pmx_search_pairs / pmx_search_pairs_device) on an MI355X.

  1. all-vs-all of 4 000 synthetic proteins of 200-400 aa (bench_pairs.py's set and seed, with planted families: 40 families of 64
     mutated copies), BLOSUM62, local; min_score is the score about 1 % of the pairs reach.  Device legs, device-event timing:
       (a) pmx_search_pairs_device, triangle: only the hits leave the chunks;
       (b) pmx_align_all_pairs_device: every record (the yardstick, an entry of the parent commit);
       (c) (b) followed by pmx_select_hits_device over all records.
     Host legs, wall clock: (d) pmx_search_pairs; (e) pmx_align_all_pairs followed by a numpy filter.
     The hits of (a) are compared with (c)'s selection applied to (b)'s records; the device memory (a) takes -- chunk scratch and hit
     buffers -- is read off hipMemGetInfo beside the record array (b) adds.
  2. config 2's shape (1 M pairs of 150 x 150 DNA) through PMX_PAIRS_LIST: (a) pmx_search_pairs_device against (b)
     pmx_align_pairs_device.

One warm-up call per leg, then `--repeats` rounds that run the legs of a part once each in turn (alternated); the JSON line reports
median / min / max per leg.  `--out FILE` writes it there as well (profiles/r10/bench_set_search.json)."""
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
    return {k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in times.items()}


def ratio(res, a, b):
    return {"median": round(res[a]["median_ms"] / res[b]["median_ms"], 4),
            "min": round(res[a]["min_ms"] / res[b]["max_ms"], 4), "max": round(res[a]["max_ms"] / res[b]["min_ms"], 4)}


def free_bytes():
    torch.cuda.synchronize(dev)
    return torch.cuda.mem_get_info(dev)[0]


def protein_set(nseq, families, members):
    rng = np.random.default_rng(20260602)
    lens = rng.integers(200, 401, size=nseq)
    seqs = [wl.AA[rng.integers(0, 20, size=int(l))] for l in lens]
    where = rng.permutation(nseq)[:families * members].reshape(families, members)          # members scattered over the rows
    for fam in where:
        base = seqs[int(fam[0])]
        for k in fam[1:]:
            s = base.copy()
            flip = rng.random(len(s)) < 0.3
            s[flip] = wl.AA[rng.integers(0, 20, size=int(flip.sum()))]
            seqs[int(k)] = s
    return [s.tobytes() for s in seqs]


def part_proteins(nseq, repeats, families, members):
    seqs = protein_set(nseq, families, members)
    max_len = max(len(s) for s in seqs)
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 16, 0, m.inner)
    total = pkg.all_pairs_count(nseq)
    free0 = free_bytes()
    S = pkg.SeqSet.new(seqs)
    cnt_a = torch.zeros(2, dtype=torch.int64, device=dev)
    # the threshold comes from the yardstick's records: the score 1 % of the pairs reach
    out_b = torch.zeros((total, 4), dtype=torch.int32, device=dev)

    def full():
        check(lib.pmx_align_all_pairs_device(C.byref(cfg), S.inner, 0, total, max_len, out_b.data_ptr(), None, stream.cuda_stream, None))
    full(); torch.cuda.synchronize(dev)
    kernel = lib.pmx_last_kernel().decode()
    scores = out_b[:, 0]
    min_score = int(torch.kthvalue(scores, total - total // 100).values.item())
    passing = int((scores >= min_score).sum().item())
    del scores
    cap = passing + 1024
    hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
    hi = torch.zeros(cap, dtype=torch.int64, device=dev)
    hr = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
    sel_idx = torch.zeros(cap, dtype=torch.int64, device=dev)
    cnt_c = torch.zeros(2, dtype=torch.int64, device=dev)
    out_gen = torch.zeros(total * 32, dtype=torch.uint8, device=dev)

    def search():
        check(lib.pmx_search_pairs_device(C.byref(cfg), S.inner, None, pkg.PAIRS_TRIANGLE, 0, total, None, max_len, max_len, min_score,
                                          hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), None, cap, cnt_a.data_ptr(), stream.cuda_stream, None))

    def full_select():
        full()
        check(lib.pmx_select_hits_device(out_b.data_ptr(), total, min_score, 0, pkg.HITS_BY_INDEX, sel_idx.data_ptr(), cap, cnt_c.data_ptr(),
                                         stream.cuda_stream))
    search(); full_select(); torch.cuda.synchronize(dev)
    ca, cc = cnt_a.cpu().tolist(), cnt_c.cpu().tolist()
    idx_c = sel_idx[:passing]
    # the descriptors the enumerator generates
    check(lib.pmx_all_pairs_enumerate_device(nseq, 0, total, out_gen.data_ptr(), stream.cuda_stream))
    want_pairs = out_gen.view(total, 32)[idx_c].reshape(-1)
    equal = (ca == [passing, passing] and cc[0] == passing and bool((hi[:passing] == idx_c).all().item())
             and bool((hr[:passing] == out_b[idx_c]).all().item()) and bool((hp[:passing * 32] == want_pairs).all().item()))
    if not equal:
        raise SystemExit("set search and the selection over the full records differ: counts %s / %s of %d" % (ca, cc, passing))
    del want_pairs
    dev_res = alternated({"a_search_pairs_device": search, "b_align_all_pairs_device": full, "c_all_pairs_then_select": full_select},
                         repeats, event_ms)
    # host entries
    al_cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 16, 0, m.inner)
    host_hits = {}

    def host_search():
        res = C.POINTER(pkg.pmx_pair_hits_t)()
        o = pkg.pmx_pair_search_opts_t(min_score, pkg.PAIRS_TRIANGLE, 0, 0, 0)
        check(lib.pmx_search_pairs(C.byref(al_cfg), S.inner, None, 0, total, None, C.byref(o), C.byref(res)))
        host_hits["d"] = pkg.PairHits(res.contents)
        lib.pmx_pair_hits_free(res)
    out_e = np.zeros(total, dtype=pkg.RECORD_DTYPE)

    def host_full_filter():
        check(lib.pmx_align_all_pairs(C.byref(al_cfg), S.inner, 0, total, out_e.ctypes.data, None, None))
        keep = np.nonzero(out_e["score"] >= min_score)[0]
        host_hits["e"] = (keep, out_e[keep])
    host_res = alternated({"d_search_pairs_host": host_search, "e_all_pairs_host_then_numpy": host_full_filter}, repeats, wall_ms)
    host_equal = (host_hits["d"].index.tolist() == host_hits["e"][0].tolist() and host_hits["d"].records.tobytes() == host_hits["e"][1].tobytes()
                  and host_hits["d"].index.tolist() == hi[:passing].cpu().tolist())
    if not host_equal:
        raise SystemExit("the host entries' hits differ")
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    cells = (int(lens.sum()) ** 2 - int((lens ** 2).sum())) // 2
    for r in list(dev_res.values()) + list(host_res.values()):
        r["tcups"] = round(cells / (r["median_ms"] * 1e-3) / 1e12, 3)
    return {"sequences": nseq, "pairs": total, "shape": "synthetic proteins of 200-400 aa, %d planted families of %d, BLOSUM62, SW, gaps 11/1" % (families, members),
            "kernel": kernel, "min_score": min_score, "passing": passing, "passing_pct": round(100.0 * passing / total, 3),
            "hits_equal_select_over_full_records": equal, "host_hits_equal": host_equal,
            "a_over_b": ratio(dev_res, "a_search_pairs_device", "b_align_all_pairs_device"),
            "a_over_c": ratio(dev_res, "a_search_pairs_device", "c_all_pairs_then_select"),
            "d_over_e": ratio(host_res, "d_search_pairs_host", "e_all_pairs_host_then_numpy"),
            "free_bytes_at_start": free0, "legs_device": dev_res, "legs_host": host_res}


def part_memory(nseq, families, members):
    """device bytes taken by (a) -- set, chunk scratch, hit buffers -- at nseq and at nseq / 2 sequences, read off hipMemGetInfo in a
    process that has run nothing else; then what (b) adds on top (its record array; the chunk buffers are shared)"""
    out = {}
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 16, 0, m.inner)
    seqs_all = protein_set(nseq, families, members)
    max_len = max(len(s) for s in seqs_all)
    warm = torch.zeros(16, device=dev); del warm
    free0 = free_bytes()
    for n in (nseq // 2, nseq):                                     # (scratch only grows: the smaller one first)
        S = pkg.SeqSet.new(seqs_all[:n])
        total = pkg.all_pairs_count(n)
        cap = total // 50
        hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        hi = torch.zeros(cap, dtype=torch.int64, device=dev)
        hr = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        check(lib.pmx_search_pairs_device(C.byref(cfg), S.inner, None, pkg.PAIRS_TRIANGLE, 0, total, None, max_len, max_len, 120,
                                          hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), None, cap, cnt.data_ptr(), stream.cuda_stream, None))
        out["a_bytes_%d_sequences_%d_pairs" % (n, total)] = free0 - free_bytes()
        out["a_hit_buffer_bytes_%d" % n] = cap * 56
        if n == nseq:
            f1 = free_bytes()
            rec = torch.zeros((total, 4), dtype=torch.int32, device=dev)
            check(lib.pmx_align_all_pairs_device(C.byref(cfg), S.inner, 0, total, max_len, rec.data_ptr(), None, stream.cuda_stream, None))
            out["b_adds_bytes_%d_pairs" % total] = f1 - free_bytes()
            del rec
        del S, hp, hi, hr, cnt
        torch.cuda.empty_cache()
    return out


def part_cfg2(n, repeats):
    qbuf, qoff, rbuf, roff = wl.make_cfg2(n)
    c = wl.CFG2
    L = c["len"]
    pad = np.zeros(16, dtype=np.uint8)
    d = [torch.from_numpy(x).to(dev) for x in (np.concatenate([qbuf, pad]), qoff, np.concatenate([rbuf, pad]), roff)]
    Q = pkg.SeqSet.wrap_device(d[0].data_ptr(), d[1].data_ptr(), n, len(qbuf), keep=d)
    R = pkg.SeqSet.wrap_device(d[2].data_ptr(), d[3].data_ptr(), n, len(rbuf), keep=d)
    pairs = np.zeros(n, dtype=pkg.PAIR_DTYPE)
    pairs["q"], pairs["r"], pairs["q_len"], pairs["r_len"] = np.arange(n), np.arange(n), -1, -1
    d_pairs = torch.from_numpy(pairs.view(np.uint8)).to(dev)
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, c["open"], c["ext"], 16, 0, m.inner)
    out_b = torch.zeros((n, 4), dtype=torch.int32, device=dev)

    def full():
        check(lib.pmx_align_pairs_device(C.byref(cfg), Q.inner, R.inner, n, d_pairs.data_ptr(), L, L, out_b.data_ptr(), None, stream.cuda_stream, None))
    full(); torch.cuda.synchronize(dev)
    min_score = int(torch.kthvalue(out_b[:, 0], n - n // 100).values.item())
    keep = torch.nonzero(out_b[:, 0] >= min_score).reshape(-1)
    passing = int(keep.numel())
    cap = passing + 1024
    hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
    hi = torch.zeros(cap, dtype=torch.int64, device=dev)
    hr = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def search():
        check(lib.pmx_search_pairs_device(C.byref(cfg), Q.inner, R.inner, pkg.PAIRS_LIST, 0, n, d_pairs.data_ptr(), L, L, min_score,
                                          hp.data_ptr(), hi.data_ptr(), hr.data_ptr(), None, cap, cnt.data_ptr(), stream.cuda_stream, None))
    search(); torch.cuda.synchronize(dev)
    equal = (cnt.cpu().tolist() == [passing, passing] and bool((hi[:passing] == keep).all().item()) and bool((hr[:passing] == out_b[keep]).all().item())
             and bool((hp[:passing * 32] == d_pairs.view(n, 32)[keep].reshape(-1)).all().item()))
    if not equal:
        raise SystemExit("set search and the filter of the full records differ")
    res = alternated({"a_search_pairs_device_list": search, "b_align_pairs_device": full}, repeats, event_ms)
    return {"pairs": n, "shape": "150 x 150 i.i.d. DNA (config 2 generator), SW, gaps 5/2, PMX_PAIRS_LIST", "min_score": min_score,
            "passing": passing, "hits_equal_filter_of_full_records": equal,
            "a_over_b": ratio(res, "a_search_pairs_device_list", "b_align_pairs_device"), "legs": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=4000)
    ap.add_argument("--families", type=int, default=40)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="memory,proteins,cfg2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = {"bench": "set_search", "device": torch.cuda.get_device_name(dev), "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    parts = a.parts.split(",")
    if "memory" in parts:                                           # first: the process has reserved no scratch yet
        line["memory"] = part_memory(a.nseq, a.families, a.members)
    if "proteins" in parts:
        line["proteins"] = part_proteins(a.nseq, a.repeats, a.families, a.members)
    if "cfg2" in parts:
        line["config2_shape"] = part_cfg2(a.n, a.repeats)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
