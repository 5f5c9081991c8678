#!/usr/bin/env python3
"""Banded traceback (pmx_align_batch_banded_cigar_device) on an MI355X, device-resident inputs, device-event timing.

  1. config 4's generator: 1.25 M related 250 x 250 DNA pairs, semi-global (every end free), bands 15, 31 and 48 around the main
     diagonal, CIGAR text -- against the full-matrix device CIGAR entry (pmx_align_batch_cigar_device) on the same pairs;
  2. config 5's second pass with CIGAR text: one 1 kbp query (profile arm) against 1.25 M references of 0.5-5 kbp, local, band 48
     around the diagonal of a first full pass's end cell -- against the score-only banded pass (pmx_align_profile_batch_banded_device).

One warm-up call per leg, then `--repeats` rounds that run every leg of a part once each in turn (alternated), one event pair per
call; the JSON line reports median / min / max per leg.  `--out FILE` writes it there as well."""
import argparse
import ctypes as C
import json
import os
import sys

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


def alternated(legs, repeats):
    """legs: {name: fn}; one warm-up each, then `repeats` rounds over all legs in turn"""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(event_ms(fn))
    return {k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                "spread_pct": round(100.0 * (max(v) - min(v)) / float(np.median(v)), 2)} for k, v in times.items()}


def text_buffers(n, capacity):
    return torch.zeros(capacity + 1, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)


def part_cfg4(n, repeats, bands=(15, 31, 48)):
    qbuf, qoff, rbuf, roff = wl.make_cfg4(n)
    d = [torch.from_numpy(x).to(dev) for x in (qbuf, qoff, rbuf, roff)]
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    c = wl.CFG4
    out_full = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    cfg_full = pkg.pmx_config_t(pkg.MODE_SG, pkg.SG_ALL, c["open"], c["ext"], 16, 0, m.inner)
    cfg_band = pkg.pmx_config_t(pkg.MODE_SG, pkg.SG_ALL, c["open"], c["ext"], 32, pkg.WANT_CIGAR, m.inner)
    cap = 120 * n
    text_f, toff_f = text_buffers(n, cap)
    outs, texts = {}, {}

    def full():
        check(lib.pmx_align_batch_cigar_device(C.byref(cfg_full), n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                               250, 250, out_full.data_ptr(), text_f.data_ptr(), cap, toff_f.data_ptr(), stream.cuda_stream))
    legs = {"full_matrix_cigar": full}
    kernels = {}
    for band in bands:
        outs[band] = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        texts[band] = text_buffers(n, cap)

        def run(band=band):
            t, o = texts[band]
            check(lib.pmx_align_batch_banded_cigar_device(C.byref(cfg_band), None, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                          d[3].data_ptr(), 250, 250, band, None, outs[band].data_ptr(), None,
                                                          t.data_ptr(), cap, o.data_ptr(), stream.cuda_stream))
        legs["banded_cigar_band%d" % band] = run
    for k, fn in legs.items():
        fn(); torch.cuda.synchronize(dev)
        kernels[k] = lib.pmx_last_kernel().decode()
    res = alternated(legs, repeats)
    for k in legs:
        res[k]["kernel"] = kernels[k]
    res["full_matrix_cigar"]["text_bytes"] = int(toff_f[n].item())
    for band in bands:
        r = res["banded_cigar_band%d" % band]
        r["text_bytes"] = int(texts[band][1][n].item())
        r["share_with_the_full_score"] = round(float((outs[band][:, 0] == out_full[:, 0]).float().mean().item()), 4)
        r["band_cells_per_s_T"] = round(n * 250 * (2 * band + 1) / (r["median_ms"] * 1e-3) / 1e12, 3)
    assert int(toff_f[n].item()) <= cap and all(int(texts[b][1][n].item()) <= cap for b in texts)
    return {"pairs": n, "shape": "250 x 250 related DNA (config 4 generator), SG every end free, gaps 5/2", "legs": res}


def part_cfg5(n, repeats):
    q, rbuf, roff, planted = wl.make_cfg5(n)
    d = [torch.from_numpy(x).to(dev) for x in (rbuf, roff)]
    c = wl.CFG5
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    prof = pkg.Profile.new(q, False, m)
    max_rlen = int((roff[1:] - roff[:-1]).max())
    first = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    cfg1 = pkg.pmx_config_t(pkg.MODE_SW, 0, c["open"], c["ext"], 0, pkg.WANT_SORTED, m.inner)
    pkg.align_profile_batch_device(cfg1, prof, n, d[0].data_ptr(), d[1].data_ptr(), max_rlen, first.data_ptr(), None, stream.cuda_stream)
    torch.cuda.synchronize(dev)
    d_diag = (first[:, 2] - first[:, 1]).contiguous()
    band = 48
    cfg_s = pkg.pmx_config_t(pkg.MODE_SW, 0, c["open"], c["ext"], 0, 0, m.inner)
    cfg_c = pkg.pmx_config_t(pkg.MODE_SW, 0, c["open"], c["ext"], 0, pkg.WANT_CIGAR, m.inner)
    out_s = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    out_c = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    cap = 40 * n
    text, toff = text_buffers(n, cap)

    def score_only():
        check(lib.pmx_align_profile_batch_banded_device(C.byref(cfg_s), prof.inner, n, d[0].data_ptr(), d[1].data_ptr(), max_rlen, band,
                                                        d_diag.data_ptr(), out_s.data_ptr(), stream.cuda_stream))

    def with_cigar():
        check(lib.pmx_align_batch_banded_cigar_device(C.byref(cfg_c), prof.inner, n, None, None, d[0].data_ptr(), d[1].data_ptr(),
                                                      len(q), max_rlen, band, d_diag.data_ptr(), out_c.data_ptr(), None,
                                                      text.data_ptr(), cap, toff.data_ptr(), stream.cuda_stream))
    legs = {"banded_score_only": score_only, "banded_cigar": with_cigar}
    kernels = {}
    for k, fn in legs.items():
        fn(); torch.cuda.synchronize(dev)
        kernels[k] = lib.pmx_last_kernel().decode()
    res = alternated(legs, repeats)
    for k in legs:
        res[k]["kernel"] = kernels[k]
    res["banded_cigar"]["text_bytes"] = int(toff[n].item())
    assert int(toff[n].item()) <= cap
    res["banded_cigar"]["records_equal_score_only"] = bool((out_c == out_s).all().item())
    return {"pairs": n, "shape": "one 1 kbp query (profile arm) x 0.5-5 kbp references (config 5 generator), SW, gaps 5/2, band 48 "
                                 "around the first pass's end diagonal", "legs": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n4", type=int, default=1_250_000)
    ap.add_argument("--n5", type=int, default=1_250_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="4,5")
    ap.add_argument("--bands", default="15,31,48", help="part 4's bands")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = {"bench": "banded_cigar", "device": torch.cuda.get_device_name(dev),
            "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    if "4" in a.parts.split(","):
        line["cfg4_cigar"] = part_cfg4(a.n4, a.repeats, tuple(int(b) for b in a.bands.split(",")))
    if "5" in a.parts.split(","):
        line["cfg5_second_pass"] = part_cfg5(a.n5, a.repeats)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
