#!/usr/bin/env python3
"""Reference-side frameshift-aware set search (pmx_search_pairs_frameshift_ref_device, PMX_STRAND_BOTH) on an MI355X.

Workload (DESIGN 2.5j's): `--nq` proteins of 200 - 400 aa against `--nr` nucleotide references of 870 - 930 nt, PMX_PAIRS_RECT, SW,
BLOSUM62, gaps 11 / 1, frameshift 15, min_score 150.  Reference j carries, on a random strand and in a random frame, a 100-letter piece
of protein j % nq with 8 % substitutions, back-translated, between random flanks.  Two data sets from the same draw: `deleted` (one
nucleotide removed at mid-piece) and `intact`.

  (a) pmx_search_pairs_frameshift_ref_device, PMX_STRAND_BOTH: the three-frame DP with the codon stream on the columns (pmx_swfsc);
  (b) pmx_search_pairs_translated_ref_device, PMX_FRAMES_ALL: the same number of cells, the road without frameshifts (six plain frames);
  (c) pmx_search_pairs_frameshift_device with the sets exchanged: the same DP with the stream on the rows (pmx_swfs), the only
      frameshift road this data had before.

Device events around each leg, one warm-up each, then `--repeats` rounds that run the legs in turn; median / min / max, a / b and a / c.
The script exits with an error unless (a)'s hits equal (c)'s with query and reference exchanged, with equal scores and strands
(BLOSUM62 is symmetric, so the two recurrences are each other's transpose).  Device memory is read off hipMemGetInfo around each leg's
first call, (a) first.  `--long` adds one point no other road can run: 50 proteins against 200 windows of 20 000 nt, leg (a) alone.
`--legs a` runs one leg alone (for a kernel trace or a counter run).  `--out FILE` writes the JSON line there as well."""
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

pkg = g.load_pkg()
lib = pkg.lib
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)
WLO, WHI, PIECE = 870, 930, 100
MQ = 400
OPEN, EXT, FS = 11, 1, 15
AA = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE = pkg.genetic_code_table()


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
    for fn in legs.values():
        fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(event_ms(fn))
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "runs_ms": [round(x, 4) for x in v]} for k, v in times.items()}


def free_bytes():
    torch.cuda.synchronize(dev)
    return torch.cuda.mem_get_info(dev)[0]


def workload(nq, nr, rng, wlo=WLO, whi=WHI):
    """-> proteins, references with one nucleotide deleted at mid-piece, the same references intact"""
    back = {}
    for i, a in enumerate(CODE):
        back.setdefault(a, []).append(bytes(b"TCAG"[(i >> s) & 3] for s in (4, 2, 0)))
    comp = pkg.complement_table()
    prots = [AA[rng.integers(0, 20, size=int(l))].tobytes() for l in rng.integers(200, 401, size=nq)]
    deleted, intact = [], []
    for j in range(nr):
        src = prots[j % nq]
        at = int(rng.integers(0, len(src) - PIECE))
        piece = bytearray(src[at:at + PIECE])
        for x in np.nonzero(rng.random(PIECE) < 0.08)[0]:
            piece[x] = int(AA[rng.integers(0, 20)])
        f = int(rng.integers(0, 6))
        core = b"".join(back[a][int(rng.integers(0, len(back[a])))] for a in piece)           # 300 nt
        w = int(rng.integers(wlo, whi + 1))
        left = 3 * int(rng.integers(0, (w - len(core)) // 3)) + f % 3
        lf, rf = DNA[rng.integers(0, 4, size=left)].tobytes(), DNA[rng.integers(0, 4, size=w - left - len(core) + 1)].tobytes()
        for out, c, r in ((intact, core, rf[:-1]), (deleted, core[:150] + core[151:], rf)):       # (the same length either way)
            s = lf + c + r
            out.append(comp[np.frombuffer(s, dtype=np.uint8)[::-1]].tobytes() if f >= 3 else s)
    assert all(wlo <= len(s) <= whi for s in deleted + intact)
    return prots, deleted, intact


class Hits:
    def __init__(self, cap):
        self.cap = cap
        self.hi = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.hr = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.hb = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def take(self):
        passing, written = self.cnt.cpu().tolist()
        if passing > self.cap:
            raise SystemExit("hit buffer too small: %d hits" % passing)
        return self.hi[:written].cpu().numpy(), self.hr[:written].cpu().numpy(), self.hb[:written].cpu().numpy()


def run_set(name, prots, refs, cfg0, cfg16, min_score, repeats, which, first):
    nq, nr = len(prots), len(refs)
    n = nq * nr
    mr_stream = max(len(s) for s in refs) - 2
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    ha, hb, hc = (Hits(8 * nr + 1024) for _ in range(3))
    none = None

    def leg_a():
        check(lib.pmx_search_pairs_frameshift_ref_device(C.byref(cfg0), Q.inner, R.inner, pkg.PAIRS_RECT, 0, n, none, MQ, mr_stream, min_score, none,
                                                         ha.hi.data_ptr(), ha.hr.data_ptr(), none, ha.cap, ha.cnt.data_ptr(), stream.cuda_stream, none,
                                                         pkg.STRAND_BOTH, ha.hb.data_ptr(), FS, none))

    def leg_b():
        check(lib.pmx_search_pairs_translated_ref_device(C.byref(cfg16), Q.inner, R.inner, pkg.PAIRS_RECT, 0, n, none, MQ, (mr_stream + 2) // 3, min_score, none,
                                                         hb.hi.data_ptr(), hb.hr.data_ptr(), none, hb.cap, hb.cnt.data_ptr(), stream.cuda_stream, none,
                                                         pkg.FRAMES_ALL, none, hb.hb.data_ptr()))

    def leg_c():
        check(lib.pmx_search_pairs_frameshift_device(C.byref(cfg0), R.inner, Q.inner, pkg.PAIRS_RECT, 0, n, none, mr_stream, MQ, min_score, none,
                                                     hc.hi.data_ptr(), hc.hr.data_ptr(), none, hc.cap, hc.cnt.data_ptr(), stream.cuda_stream, none,
                                                     pkg.STRAND_BOTH, hc.hb.data_ptr(), FS, none))

    out = {"proteins": nq, "references": nr, "pairs": n, "cells_per_strand": int(sum(len(p) for p in prots)) * int(sum(len(s) - 2 for s in refs))}
    mem = {}
    kernels = {}
    legs = {}
    for key, fn, tag in (("a", leg_a, "a_frameshift_ref_both_strands"), ("b", leg_b, "b_translated_ref_all_frames"), ("c", leg_c, "c_frameshift_sets_exchanged")):
        if which and key not in which:
            continue
        f0 = free_bytes()
        fn()
        mem[tag + "_first_call_bytes"] = f0 - free_bytes()
        kernels[tag] = lib.pmx_last_kernel().decode()
        legs[tag] = fn
    if first:
        out["memory"] = dict(mem, note="hipMemGetInfo around each leg's first call in this process, in the order a, b, c: a leg's figure is what "
                                       "it adds to the scratch the thread already holds")
    out["kernels"] = kernels
    if "a_frameshift_ref_both_strands" in legs:
        ai, ar, ab = ha.take()
        out["a_hits"] = len(ai); out["a_median_score"] = float(np.median(ar[:, 0])) if len(ai) else None
        out["a_reverse_strand_hits"] = int(ab.sum())
    if "b_translated_ref_all_frames" in legs:
        bi, br, _ = hb.take()
        out["b_hits"] = len(bi); out["b_median_score"] = float(np.median(br[:, 0])) if len(bi) else None
    if "a_frameshift_ref_both_strands" in legs and "c_frameshift_sets_exchanged" in legs:
        ci, cr, cb = hc.take()
        a_set = sorted((int(p) // nr, int(p) % nr, int(r[0]), int(s)) for p, r, s in zip(ai, ar, ab))
        c_set = sorted((int(p) % nq, int(p) // nq, int(r[0]), int(s)) for p, r, s in zip(ci, cr, cb))
        if a_set != c_set:
            raise SystemExit("%s: the reference-side search and the query-side search over the exchanged sets differ: %d / %d hits" % (name, len(a_set), len(c_set)))
        out["a_hits_equal_c_hits_exchanged"] = True
    res = alternated(legs, repeats)
    out["legs"] = res
    a = res.get("a_frameshift_ref_both_strands")
    if a:
        out["a_gcups"] = round(2 * out["cells_per_strand"] / a["median_ms"] / 1e6, 1)
        for key, tag in (("a_over_b", "b_translated_ref_all_frames"), ("a_over_c", "c_frameshift_sets_exchanged")):
            if tag in res:
                out[key] = round(a["median_ms"] / res[tag]["median_ms"], 4)
                out[key + "_min_max"] = [round(a["min_ms"] / res[tag]["max_ms"], 4), round(a["max_ms"] / res[tag]["min_ms"], 4)]
    return out


def long_point(cfg0, min_score, repeats):
    rng = np.random.default_rng(20261020)
    prots, deleted, _ = workload(50, 200, rng, 20000, 20000)
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(deleted)
    n = 50 * 200
    h = Hits(8 * 200 + 1024)

    def leg():
        check(lib.pmx_search_pairs_frameshift_ref_device(C.byref(cfg0), Q.inner, R.inner, pkg.PAIRS_RECT, 0, n, None, MQ, 19998, min_score, None,
                                                         h.hi.data_ptr(), h.hr.data_ptr(), None, h.cap, h.cnt.data_ptr(), stream.cuda_stream, None,
                                                         pkg.STRAND_BOTH, h.hb.data_ptr(), FS, None))
    f0 = free_bytes()
    leg()
    grew = f0 - free_bytes()
    kernel = lib.pmx_last_kernel().decode()
    hi, hr, _ = h.take()
    res = alternated({"a_frameshift_ref_both_strands": leg}, repeats)
    cells = int(sum(len(p) for p in prots)) * 200 * 19998
    return {"proteins": 50, "references": 200, "window_nt": 20000, "pairs": n, "kernel": kernel, "hits": len(hi),
            "planted_pairs": 200, "planted_pairs_found": int(sum(1 for p in hi if (int(p) // 200) == (int(p) % 200) % 50)),
            "first_call_bytes": grew, "legs": res, "a_gcups": round(2 * cells / res["a_frameshift_ref_both_strands"]["median_ms"] / 1e6, 1),
            "note": "windows beyond PMX_FRAMESHIFT_MAX_WINDOW: the query-side entries refuse the exchanged sets, the translated entries cut the hits in two"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=500)
    ap.add_argument("--nr", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-score", type=int, default=150)
    ap.add_argument("--legs", default="", help="letters of the legs to run (default: all), e.g. a")
    ap.add_argument("--long", action="store_true", help="add the point of 50 proteins x 200 windows of 20 000 nt")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    prots, deleted, intact = workload(a.nq, a.nr, np.random.default_rng(20261019))
    warm = torch.zeros(16, device=dev); del warm
    m = pkg.Matrix.from_name("blosum62")
    cfg0 = pkg.pmx_config_t(pkg.MODE_SW, 0, OPEN, EXT, 0, 0, m.inner)
    cfg16 = pkg.pmx_config_t(pkg.MODE_SW, 0, OPEN, EXT, 16, 0, m.inner)
    line = {"bench": "frameshift_ref", "device": torch.cuda.get_device_name(dev),
            "shape": "proteins of 200 - 400 aa against references of 870 - 930 nt that carry on a random strand and frame a 100-letter piece (8 % "
                     "substitutions) of protein j % nq, PMX_PAIRS_RECT, SW, BLOSUM62, gaps 11/1, frameshift 15; (a), (c): width 0, (b): width 16",
            "min_score": a.min_score, "lane_rows": lib.pmx_swfsc_lane_rows(), "strip_rows": lib.pmx_swfsc_strip_rows(),
            "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    line["deleted_base"] = run_set("deleted", prots, deleted, cfg0, cfg16, a.min_score, a.repeats, a.legs, True)
    line["intact"] = run_set("intact", prots, intact, cfg0, cfg16, a.min_score, a.repeats, a.legs, False)
    if a.long:
        line["long_references"] = long_point(cfg0, a.min_score, max(3, a.repeats // 2))
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
