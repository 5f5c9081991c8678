#!/usr/bin/env python3
"""Reference-side frameshift traceback (pmx_align_pairs_frameshift_ref_cigar_device) on an MI355X: what the pass over a search's hits
costs beside the search, and what trace and walk cost per pair beside the score-only sweep.

Workload (profiles/bench_frameshift_ref.py's, the data set with the base deleted): `--nq` proteins of 200 - 400 aa against `--nr`
nucleotide references of 870 - 930 nt, SW, BLOSUM62, gaps 11 / 1, frameshift 15, min_score 150; reference j carries, on a random strand
and in a random frame, a 100-letter piece of protein j % nq with one nucleotide deleted at mid-piece, so the hits' texts contain '/'.

  (a) pmx_search_pairs_frameshift_ref_device over the rectangle, PMX_STRAND_BOTH, alone: the parent's figure;
  (b) the same search writing its hit descriptors too, the count read back, then pmx_align_pairs_frameshift_ref_cigar_device (text,
      begins, statistics) over the hit pairs and strand bytes as they lie on the device;
  (c) over the first `--listed` pairs of the rectangle as a listed batch, PMX_STRAND_BOTH: c1 pmx_align_pairs_frameshift_ref_device
      (scores), c2 pmx_align_pairs_frameshift_ref_cigar_device.  c2 / c1 is what trace and walk cost per pair; the trace is every cell
      of a slot's matrix, so the ratio depends on the bound on a part's trace (PMX_CIGAR_CHUNK_BYTES in the environment is recorded).

Device events around each leg, one warm-up each, then `--repeats` rounds that run the legs in turn; the JSON line reports median / min /
max, b - a, c2 / c1, and how many of the hits' texts hold a '/'.  The script exits with an error unless the records of (b) equal the
search's hit records and the records of c2 equal those of c1.  The one condition: b - a < a.  Device memory is read off hipMemGetInfo
around each leg's first call.  `--out FILE` writes the line there as well."""
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
import bench_frameshift_ref as br  # noqa: E402  (the workload, the timing loop and the hit buffers)

pkg, lib, dev, stream = br.pkg, br.lib, br.dev, br.stream
MQ, FS = br.MQ, br.FS


class Texts:
    """the outputs of the traceback entry for up to cap pairs"""

    def __init__(self, cap, text_bytes):
        self.rec = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.won = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.stats = torch.zeros((cap, 3), dtype=torch.int32, device=dev)
        self.beg = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
        self.text = torch.zeros(text_bytes, dtype=torch.uint8, device=dev)
        self.off = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self.capacity = text_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=500)
    ap.add_argument("--nr", type=int, default=2000)
    ap.add_argument("--listed", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-score", type=int, default=150)
    ap.add_argument("--legs", default="", help="letters of the legs to run (default: all), e.g. c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nq, nr, min_score = a.nq, a.nr, a.min_score
    n = nq * nr
    listed = min(a.listed, n)
    prots, deleted, _ = br.workload(nq, nr, np.random.default_rng(20261019))
    mr = max(len(s) for s in deleted) - 2
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, br.OPEN, br.EXT, 0, 0, m.inner)
    cfg_t = pkg.pmx_config_t(pkg.MODE_SW, 0, br.OPEN, br.EXT, 0, pkg.WANT_CIGAR | pkg.WANT_STATS, m.inner)
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(deleted)
    cap = 8 * nr + 1024
    ha, hb = br.Hits(cap), br.Hits(cap)
    hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
    th = Texts(cap, 64 * cap)
    found = {}

    def leg_a():
        br.check(lib.pmx_search_pairs_frameshift_ref_device(C.byref(cfg), Q.inner, R.inner, pkg.PAIRS_RECT, 0, n, None, MQ, mr, min_score, None,
                                                            ha.hi.data_ptr(), ha.hr.data_ptr(), None, ha.cap, ha.cnt.data_ptr(), stream.cuda_stream, None,
                                                            pkg.STRAND_BOTH, ha.hb.data_ptr(), FS, None))

    def leg_b():
        br.check(lib.pmx_search_pairs_frameshift_ref_device(C.byref(cfg), Q.inner, R.inner, pkg.PAIRS_RECT, 0, n, None, MQ, mr, min_score, hp.data_ptr(),
                                                            hb.hi.data_ptr(), hb.hr.data_ptr(), None, hb.cap, hb.cnt.data_ptr(), stream.cuda_stream, None,
                                                            pkg.STRAND_BOTH, hb.hb.data_ptr(), FS, None))
        passing, hits = (int(x) for x in hb.cnt.cpu())
        if passing > hb.cap:
            raise SystemExit("hit buffer too small: %d hits" % passing)
        found["hits"] = hits
        br.check(lib.pmx_align_pairs_frameshift_ref_cigar_device(C.byref(cfg_t), Q.inner, R.inner, hits, hp.data_ptr(), hb.hb.data_ptr(),
                                                                 pkg.STRAND_FORWARD, FS, None, MQ, mr, th.rec.data_ptr(), th.won.data_ptr(),
                                                                 th.stats.data_ptr(), th.beg.data_ptr(), th.text.data_ptr(), th.capacity,
                                                                 th.off.data_ptr(), stream.cuda_stream, None))
        found["kernel"] = lib.pmx_last_kernel().decode()

    # (c): the first `listed` pairs of the rectangle, listed
    d = np.zeros(listed, dtype=pkg.PAIR_DTYPE)
    d["q"] = np.arange(listed) // nr; d["r"] = np.arange(listed) % nr; d["q_len"] = -1; d["r_len"] = -1
    d_pairs = torch.from_numpy(d.view(np.uint8)).to(dev)
    c_rec = torch.zeros((listed, 4), dtype=torch.int32, device=dev); c_won = torch.zeros(listed, dtype=torch.uint8, device=dev)
    tc = Texts(listed, 64 * listed)

    def leg_c1():
        br.check(lib.pmx_align_pairs_frameshift_ref_device(C.byref(cfg), Q.inner, R.inner, listed, d_pairs.data_ptr(), None, pkg.STRAND_BOTH, FS, None,
                                                           MQ, mr, c_rec.data_ptr(), c_won.data_ptr(), stream.cuda_stream, None))

    def leg_c2():
        br.check(lib.pmx_align_pairs_frameshift_ref_cigar_device(C.byref(cfg_t), Q.inner, R.inner, listed, d_pairs.data_ptr(), None, pkg.STRAND_BOTH,
                                                                 FS, None, MQ, mr, tc.rec.data_ptr(), tc.won.data_ptr(), tc.stats.data_ptr(),
                                                                 tc.beg.data_ptr(), tc.text.data_ptr(), tc.capacity, tc.off.data_ptr(),
                                                                 stream.cuda_stream, None))

    legs, mem = {}, {}
    for key, tag, fn in (("a", "a_search", leg_a), ("b", "b_search_then_traceback_of_hits", leg_b), ("c", "c1_listed_scores", leg_c1),
                         ("c", "c2_listed_traceback", leg_c2)):
        if a.legs and key not in a.legs:
            continue
        f0 = br.free_bytes()
        fn()
        mem[tag + "_first_call_bytes"] = f0 - br.free_bytes()
        legs[tag] = fn
    res = br.alternated(legs, a.repeats)
    trace_slot = int(lib.pmx_swfsc_trace_bytes_per_slot(MQ, mr))
    line = {"bench": "frameshift_ref_cigar", "device": torch.cuda.get_device_name(dev), "proteins": nq, "references": nr, "pairs": n,
            "listed_pairs": listed,
            "shape": "proteins of 200 - 400 aa against references of 870 - 930 nt that carry on a random strand and frame a 100-letter piece (8 %% "
                     "substitutions, one nucleotide deleted at mid-piece) of protein j %% nq, SW, BLOSUM62, gaps 11/1, PMX_STRAND_BOTH, frameshift %d" % FS,
            "min_score": min_score, "frameshift": FS, "max_qlen": MQ, "max_rlen": mr, "trace_bytes_per_slot": trace_slot,
            "legs": res, "memory": dict(mem, note="hipMemGetInfo around each leg's first call in this process, in the order a, b, c1, c2: a leg's "
                                                  "figure is what it adds to the scratch the thread already holds"),
            "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    # what came out: the two searches agree, the pass returns the hits' records, the listed legs agree, the texts hold the deletion
    if "b_search_then_traceback_of_hits" in legs:
        hits = found["hits"]
        if not torch.equal(th.rec[:hits], hb.hr[:hits]) or not torch.equal(th.won[:hits], hb.hb[:hits]):
            raise SystemExit("the traceback's records differ from the search's hit records")
        if "a_search" in legs and (int(ha.cnt.cpu()[1]) != hits or not torch.equal(ha.hr[:hits], hb.hr[:hits])):
            raise SystemExit("the two searches differ")
        off = th.off[:hits + 1].cpu().numpy(); raw = th.text.cpu().numpy().tobytes()
        assert off[hits] <= th.capacity
        texts = [raw[off[k]:off[k + 1]].decode() for k in range(hits)]
        index = hb.hi[:hits].cpu().numpy()
        home = ((index % nr) % nq) == (index // nr)
        line.update({"hits": hits, "home_hits": int(home.sum()), "hit_texts_with_slash": sum("/" in t for t in texts),
                     "home_hit_texts_with_one_slash": sum(t.count("/") == 1 for t, h in zip(texts, home) if h),
                     "example_text": texts[0] if texts else None, "hit_text_bytes": int(off[hits]), "trace_kernel": found["kernel"]})
        if "a_search" in legs:
            ma, mb = res["a_search"]["median_ms"], res["b_search_then_traceback_of_hits"]["median_ms"]
            line["b_minus_a_ms"] = round(mb - ma, 4)
            line["pass_shorter_than_search"] = bool(mb - ma < ma)
    if "c2_listed_traceback" in legs:
        if not torch.equal(c_rec, tc.rec) or not torch.equal(c_won, tc.won):
            raise SystemExit("the listed traceback's records differ from the listed scores")
        assert int(tc.off[listed]) <= tc.capacity
        line["listed_text_bytes"] = int(tc.off[listed])
        line["c2_over_c1"] = round(res["c2_listed_traceback"]["median_ms"] / res["c1_listed_scores"]["median_ms"], 4)
        line["c2_over_c1_min_max"] = [round(res["c2_listed_traceback"]["min_ms"] / res["c1_listed_scores"]["max_ms"], 4),
                                      round(res["c2_listed_traceback"]["max_ms"] / res["c1_listed_scores"]["min_ms"], 4)]
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
