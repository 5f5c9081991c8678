#!/usr/bin/env python3
"""Profile database search (pmx_search_profile_device) on an MI355X at config 5's shape: one 1 kbp query against n references of
0.5-5 kbp (bench.py's per-GPU n by default), local, min_score 200, band 48, CIGAR text.  Device-resident references.

  a  pmx_search_profile_device: first pass, selection, gather, banded second pass with traceback over the hits
  b  pmx_align_profile_batch_device alone: the first pass
  c  pmx_align_batch_banded_cigar_device on the hits, gathered beforehand
  d  the host route a caller had before: first pass, D2H of all n records, numpy selection and re-pack, the host banded-CIGAR entry

One warm-up call per leg, then `--repeats` rounds that run every leg once each in turn.  a, b and c are timed with device events
(a's one host synchronisation sits between its events), d -- host work -- with the wall clock around a device synchronisation, and so
is a for that comparison.  The JSON line reports median / min / max per leg, a - b - c (selection + gather + the synchronisation) in
ms and as a share of b.  `--out FILE` writes it there as well."""
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


def summary(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
            "spread_pct": round(100.0 * (max(v) - min(v)) / float(np.median(v)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=wl.CFG5["n"] // 8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-score", type=int, default=200)
    ap.add_argument("--band", type=int, default=48)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, band, min_score = a.n, a.band, a.min_score
    q, rbuf, roff, planted = wl.make_cfg5(n)
    c = wl.CFG5
    d_rbuf, d_roff = torch.from_numpy(rbuf).to(dev), torch.from_numpy(roff).to(dev)
    max_rlen = int((roff[1:] - roff[:-1]).max())
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    prof = pkg.Profile.new(q, False, m)
    al = pkg.Aligner.new().local().profile(prof).matrix(m).gap_open(c["open"]).gap_extend(c["ext"]).build()
    cfg1 = pkg.pmx_config_t(pkg.MODE_SW, 0, c["open"], c["ext"], 0, pkg.WANT_SORTED, m.inner)
    cfg2 = pkg.pmx_config_t(pkg.MODE_SW, 0, c["open"], c["ext"], 0, pkg.WANT_CIGAR | pkg.WANT_SORTED, m.inner)
    cap = max(1, len(planted) * 2)
    text_cap = 4000 * cap
    first = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    hits = torch.zeros((cap, 10), dtype=torch.int32, device=dev)
    recs = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
    text = torch.zeros(text_cap + 1, dtype=torch.uint8, device=dev)
    toff = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)

    def leg_a():
        pkg.search_profile_device(cfg2, prof, n, d_rbuf.data_ptr(), d_roff.data_ptr(), max_rlen, min_score, 0, pkg.HITS_BY_INDEX, band,
                                  first.data_ptr(), hits.data_ptr(), recs.data_ptr(), None, cap, text.data_ptr(), text_cap,
                                  toff.data_ptr(), counts.data_ptr(), stream.cuda_stream)

    first_b = torch.zeros((n, 4), dtype=torch.int32, device=dev)

    def leg_b():
        pkg.align_profile_batch_device(cfg1, prof, n, d_rbuf.data_ptr(), d_roff.data_ptr(), max_rlen, first_b.data_ptr(), None,
                                       stream.cuda_stream)

    # the hits, gathered beforehand, for c
    leg_a()
    torch.cuda.synchronize(dev)
    kernel_a = lib.pmx_last_kernel().decode()
    h = int(counts[0].item())
    assert h <= cap and int(toff[h].item()) <= text_cap, (h, cap, int(toff[h].item()))
    hit_np = hits.cpu().numpy().view(pkg.HIT_DTYPE).reshape(-1)[:h]
    d_index = torch.from_numpy(np.ascontiguousarray(hit_np["index"])).to(dev)
    d_diag = torch.from_numpy(np.ascontiguousarray(hit_np["diag"])).to(dev)
    hbytes = int((roff[hit_np["index"] + 1] - roff[hit_np["index"]]).sum())
    g_rbuf = torch.zeros(hbytes + 16, dtype=torch.uint8, device=dev)
    g_roff = torch.zeros(h + 1, dtype=torch.int64, device=dev)
    pkg.gather_refs_device(d_rbuf.data_ptr(), d_roff.data_ptr(), n, d_index.data_ptr(), h, g_rbuf.data_ptr(), hbytes, g_roff.data_ptr(),
                           stream.cuda_stream)
    recs_c = torch.zeros((max(h, 1), 4), dtype=torch.int32, device=dev)
    text_c = torch.zeros(text_cap + 1, dtype=torch.uint8, device=dev)
    toff_c = torch.zeros(h + 1, dtype=torch.int64, device=dev)

    def leg_c():
        check(lib.pmx_align_batch_banded_cigar_device(C.byref(cfg2), prof.inner, h, None, None, g_rbuf.data_ptr(), g_roff.data_ptr(),
                                                      len(q), max_rlen, band, d_diag.data_ptr(), recs_c.data_ptr(), None,
                                                      text_c.data_ptr(), text_cap, toff_c.data_ptr(), stream.cuda_stream))

    route_d = {}

    def leg_d():
        leg_b()
        full = first_b.cpu().numpy().view(pkg.RECORD_DTYPE).reshape(-1)          # D2H of all n records
        index = np.nonzero(full["score"] >= min_score)[0]
        sub = [rbuf[roff[k]:roff[k + 1]].tobytes() for k in index]               # re-pack
        diag = (full["end_ref"][index] - full["end_query"][index]).astype(np.int32)
        route_d["out"] = al.align_batch_banded_cigar([], sub, band, diag)         # uploads the subset again

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
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    for fn in (leg_a, leg_b, leg_c, leg_d):
        fn()
    torch.cuda.synchronize(dev)
    ev = {"a": [], "b": [], "c": []}
    wall = {"a": [], "d": []}
    for _ in range(a.repeats):
        ev["a"].append(event_ms(leg_a)); ev["b"].append(event_ms(leg_b)); ev["c"].append(event_ms(leg_c))
        wall["a"].append(wall_ms(leg_a)); wall["d"].append(wall_ms(leg_d))
    # the three routes agree
    rec_a = recs.cpu().numpy().view(pkg.RECORD_DTYPE).reshape(-1)[:h]
    same_c = bool((recs_c[:h].cpu().numpy().view(pkg.RECORD_DTYPE).reshape(-1) == rec_a).all()) and \
        text_c[:int(toff_c[h].item())].cpu().numpy().tobytes() == text[:int(toff[h].item())].cpu().numpy().tobytes()
    same_d = bool((route_d["out"][0] == rec_a).all()) and "".join(route_d["out"][1]).encode() == text[:int(toff[h].item())].cpu().numpy().tobytes()
    over = [x - y - z for x, y, z in zip(ev["a"], ev["b"], ev["c"])]
    med = {k: float(np.median(v)) for k, v in ev.items()}
    line = {"bench": "search", "device": torch.cuda.get_device_name(dev), "n": n, "hits": h, "planted": int(len(planted)),
            "passing": int(counts[1].item()), "hit_reference_bytes": hbytes, "text_bytes": int(toff[h].item()),
            "min_score": min_score, "band": band, "repeats": a.repeats, "kernel": kernel_a,
            "events": {"a_search_device": summary(ev["a"]), "b_first_pass": summary(ev["b"]), "c_banded_cigar_on_hits": summary(ev["c"])},
            "a_minus_b_minus_c_ms": summary(over) if np.median(over) > 0 else {"median_ms": round(float(np.median(over)), 3),
                                                                              "min_ms": round(min(over), 3), "max_ms": round(max(over), 3)},
            "a_minus_b_minus_c_share_of_b_pct": round(100.0 * (med["a"] - med["b"] - med["c"]) / med["b"], 3),
            "wall": {"a_search_device": summary(wall["a"]), "d_host_route": summary(wall["d"])},
            "routes_agree": {"c": same_c, "d": same_d},
            "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
