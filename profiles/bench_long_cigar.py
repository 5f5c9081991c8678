"""Long pairs with traceback: the tiled road (pmx_align_batch_cigar_long) against the byte-table roads, in one process.

(1) one pair, NW and SW, 5 / 20 / 50 kbp squared, text in host memory at the end: Aligner.use_trace().align() + get_cigar()
    (parasail_{nw,sw}_trace_striped_32 + parasail_result_get_cigar: a qlen x rlen byte table on the device, over PCIe and on the
    host) against the new host entry.  The two alternate and repeat, so the spread shows.
(2) 512 pairs of 5 kbp x 5 kbp: pmx_align_batch_cigar (12.8 GB of byte tables, if it can reserve them) against the new entry.
(3) 20 kbp x 20 kbp on the device, by events: the score-only pmx_align_batch_device against the new device entry under every offered
    tile_cols (what the traceback adds to the sweep), and under the default tile with the sweep's one-column form.  --profile runs only the new entry a few times, for
    rocprofv3 --kernel-trace --stats to split it into sweep-with-checkpoints and walk.
Prints one JSON document; --out writes it to a file too.

  python profiles/bench_long_cigar.py [--reps 5] [--sizes 5000,20000,50000] [--batch 512] [--out profiles/r08/bench_long_cigar.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="5000,20000,50000")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch                                            # (loaded before the library: torch's HIP runtime comes first)
    import __graft_entry__ as g
    from util import random_seqs, mutate
    pkg = g.load_pkg()
    dev = torch.device("cuda:0")
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    rng = np.random.default_rng(20)
    res = {"gaps": [5, 2], "matrix": "ACGT 2/-3", "reps": a.reps}

    def builder(mode):
        b = pkg.Aligner.new().matrix(pm).gap_open(5).gap_extend(2).solution_width(32)
        return b.global_() if mode == "nw" else b.local()

    def pair(L):
        q = random_seqs(rng, 1, L, L)[0]
        return q, mutate(rng, q, 0.08, 0.02)

    def device_inputs(qs, rs):
        qb, qo = pkg.pack(qs); rb, ro = pkg.pack(rs)
        return [torch.from_numpy(x).to(dev) for x in (qb, qo, rb, ro)], max(len(x) for x in qs), max(len(x) for x in rs)

    def events(fn):
        st = torch.cuda.current_stream()
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.steps):
                fn()
            e1.record(st)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / a.steps)
        return out

    def device_case(mode, L, tiles):
        q, r = pair(L)
        d, mq, mr = device_inputs([q], [r])
        out = torch.zeros((1, 4), dtype=torch.int32, device=dev); st = torch.zeros((1, 3), dtype=torch.int32, device=dev)
        text = torch.zeros(mq + mr + 64, dtype=torch.uint8, device=dev); toff = torch.zeros(2, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        m = pkg.MODE_NW if mode == "nw" else pkg.MODE_SW
        cfg0 = pkg.pmx_config_t(m, 0, 5, 2, 32, 0, pm.inner)
        cfg1 = pkg.pmx_config_t(m, 0, 5, 2, 32, pkg.WANT_CIGAR, pm.inner)
        row = {"ms": {}, "kernels": {}}
        if not a.profile:
            row["ms"]["score_only"] = events(lambda: pkg.align_batch_device(cfg0, 1, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), mq, mr, out.data_ptr(), None, stream))
            row["kernels"]["score_only"] = pkg.lib.pmx_last_kernel().decode()
        for tile in tiles:
            row["ms"]["tile_cols_%d" % tile] = events(lambda: pkg.align_batch_cigar_long_device(
                cfg1, 1, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), mq, mr, out.data_ptr(), st.data_ptr(),
                text.data_ptr(), mq + mr + 64, toff.data_ptr(), stream, tile, 0))
            row["kernels"]["tile_cols_%d" % tile] = pkg.lib.pmx_last_kernel().decode()
        if not a.profile:                                      # the sweep's one-column form under the default tile (a switch of the shared sweep)
            os.environ["PMX_LONG_ONE_COLUMN"] = "1"
            row["ms"]["tile_cols_128_one_column"] = events(lambda: pkg.align_batch_cigar_long_device(
                cfg1, 1, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), mq, mr, out.data_ptr(), st.data_ptr(),
                text.data_ptr(), mq + mr + 64, toff.data_ptr(), stream, 128, 0))
            row["kernels"]["tile_cols_128_one_column"] = pkg.lib.pmx_last_kernel().decode()
            del os.environ["PMX_LONG_ONE_COLUMN"]
        row["median_ms"] = {k: float(np.median(v)) for k, v in row["ms"].items()}
        return row

    if a.profile:
        res["profile_20kbp"] = {mode: device_case(mode, 20000, (128,)) for mode in ("nw", "sw")}
        print(json.dumps(res, indent=1))
        return

    # (1) one pair, text in host memory
    res["one_pair_host"] = {}
    for L in [int(x) for x in a.sizes.split(",")]:
        for mode in ("nw", "sw"):
            q, r = pair(L)
            tr = builder(mode).use_trace().build()
            al = builder(mode).build()
            ms = {"trace_table": [], "tiled": []}
            texts = {}
            for rep in range(a.reps + 1):                       # (the first repetition warms both roads up and is dropped)
                for label in (("trace_table", "tiled") if rep % 2 == 0 else ("tiled", "trace_table")):
                    t0 = time.perf_counter()
                    if label == "trace_table":
                        texts[label] = tr.align(q, r).get_cigar(q, r)
                    else:
                        texts[label] = al.align_batch_cigar_long([q], [r])[1][0]
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep:
                        ms[label].append(dt)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            res["one_pair_host"]["%s_%d" % (mode, L)] = {"ms": ms, "median_ms": med, "tiled_over_table": med["tiled"] / med["trace_table"],
                                                         "same_text": texts["trace_table"] == texts["tiled"],
                                                         "scratch_bytes_tiled": pkg.long_cigar_scratch_bytes(1, L, len(r)), "table_bytes": L * len(r)}

    # (2) a batch of 5 kbp pairs
    n = a.batch
    qs = random_seqs(rng, n, 5000, 5000)
    rs = [mutate(rng, q, 0.08, 0.02) for q in qs]
    al = builder("nw").build()
    ms = {"byte_tables": [], "tiled": []}
    got = {}
    for rep in range(a.reps + 1):
        for label in (("byte_tables", "tiled") if rep % 2 == 0 else ("tiled", "byte_tables")):
            if label == "byte_tables" and ms.get("byte_tables") is None:
                continue
            t0 = time.perf_counter()
            try:
                got[label] = al.align_batch_cigar(qs, rs)[1] if label == "byte_tables" else al.align_batch_cigar_long(qs, rs)[1]
            except pkg.BatchError as exc:
                ms["byte_tables"] = None
                res["batch_5kbp_byte_tables_error"] = str(exc)
                continue
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                ms[label].append(dt)
    res["batch_5kbp"] = {"pairs": n, "ms": ms, "median_ms": {k: float(np.median(v)) for k, v in ms.items() if v},
                         "same_text": got.get("byte_tables") == got.get("tiled") if "byte_tables" in got else None,
                         "scratch_bytes_tiled": pkg.long_cigar_scratch_bytes(n, 5000, max(len(x) for x in rs))}

    # (3) what the traceback adds to the sweep, on the device
    res["device_20kbp"] = {mode: device_case(mode, 20000, (64, 128, 256)) for mode in ("nw", "sw")}
    res["device_100kbp"] = {mode: device_case(mode, 100000, (128,)) for mode in ("nw",)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
