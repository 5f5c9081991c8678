#!/usr/bin/env python3
"""Frameshift traceback (pmx_align_pairs_frameshift_cigar_device) on an MI355X: what the pass over a search's hits costs beside the
search, and what trace and walk cost per pair beside the score-only sweep.

Workload (profiles/bench_frameshift.py's second table): `--nq` reads of 150 nt against `--nr` proteins of 200 - 400 aa, BLOSUM62, gaps
11 / 1, local, both strands, frameshift `--frameshift`, `--min-score`; read i codes for a 48-letter piece of protein i % nr and has
nucleotide 75 deleted (149 nt), so the hits' texts contain '/'.

  (a) pmx_search_pairs_frameshift_device over the rectangle, alone: the parent's figure;
  (b) the same search writing its hit descriptors too, the count read back, then pmx_align_pairs_frameshift_cigar_device (text, begins,
      statistics) over the hit pairs and strand bytes as they lie on the device;
  (c) over the first `--listed` pairs of the rectangle as a listed batch, PMX_STRAND_BOTH: c1 pmx_align_pairs_frameshift_device (scores),
      c2 pmx_align_pairs_frameshift_cigar_device.  c2 / c1 is what trace and walk cost per pair.

Device events around each leg, one warm-up each, then `--repeats` rounds that run the legs in turn; the JSON line reports median / min /
max, b - a, c2 / c1, and how many of the hits' texts hold a '/'.  The one condition: b - a < a (the hits are 0.2 % of the pairs; anything
else means the pass is not running over the hits only).  `--out FILE` writes the line there as well."""
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
W = bt.W - 1
MR = bt.MR


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
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--nr", type=int, default=500)
    ap.add_argument("--listed", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-score", type=int, default=120)
    ap.add_argument("--frameshift", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nq, nr, min_score, fsp = a.nq, a.nr, a.min_score, a.frameshift
    n = nq * nr
    listed = min(a.listed, n)
    reads, prots, frames = bt.workload(nq, nr, np.random.default_rng(20261019))
    cut = [s[:75] + s[76:] for s in reads]
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, bt.OPEN, bt.EXT, 0, 0, m.inner)
    cfg_t = pkg.pmx_config_t(pkg.MODE_SW, 0, bt.OPEN, bt.EXT, 0, pkg.WANT_CIGAR | pkg.WANT_STATS, m.inner)
    Q, R = pkg.SeqSet.new(cut), pkg.SeqSet.new(prots)
    cap = 8 * nq + 1024
    ha, hb = bt.Hits(cap), bt.Hits(cap)
    hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
    th = Texts(cap, 64 * cap)
    found = {}

    def leg_a():
        bt.check(lib.pmx_search_pairs_frameshift_device(C.byref(cfg), Q.inner, R.inner, pkg.PAIRS_RECT, 0, n, None, W - 2, MR, min_score, None,
                                                        ha.hi.data_ptr(), ha.hr.data_ptr(), None, ha.cap, ha.cnt.data_ptr(), stream.cuda_stream, None,
                                                        pkg.STRAND_BOTH, ha.hb.data_ptr(), fsp, None))

    def leg_b():
        bt.check(lib.pmx_search_pairs_frameshift_device(C.byref(cfg), Q.inner, R.inner, pkg.PAIRS_RECT, 0, n, None, W - 2, MR, min_score, hp.data_ptr(),
                                                        hb.hi.data_ptr(), hb.hr.data_ptr(), None, hb.cap, hb.cnt.data_ptr(), stream.cuda_stream, None,
                                                        pkg.STRAND_BOTH, hb.hb.data_ptr(), fsp, None))
        hits = int(hb.cnt.cpu()[1])
        found["hits"] = hits
        bt.check(lib.pmx_align_pairs_frameshift_cigar_device(C.byref(cfg_t), Q.inner, R.inner, hits, hp.data_ptr(), hb.hb.data_ptr(), pkg.STRAND_FORWARD,
                                                             fsp, None, W - 2, MR, th.rec.data_ptr(), th.won.data_ptr(), th.stats.data_ptr(),
                                                             th.beg.data_ptr(), th.text.data_ptr(), th.capacity, th.off.data_ptr(),
                                                             stream.cuda_stream, None))
        found["kernel"] = lib.pmx_last_kernel().decode()

    # (c): the first `listed` pairs of the rectangle, listed
    d = np.zeros(listed, dtype=pkg.PAIR_DTYPE)
    d["q"] = np.arange(listed) // nr; d["r"] = np.arange(listed) % nr; d["q_len"] = -1; d["r_len"] = -1
    d_pairs = torch.from_numpy(d.view(np.uint8)).to(dev)
    c_rec = torch.zeros((listed, 4), dtype=torch.int32, device=dev); c_won = torch.zeros(listed, dtype=torch.uint8, device=dev)
    tc = Texts(listed, 64 * listed)

    def leg_c1():
        bt.check(lib.pmx_align_pairs_frameshift_device(C.byref(cfg), Q.inner, R.inner, listed, d_pairs.data_ptr(), None, pkg.STRAND_BOTH, fsp, None,
                                                       W - 2, MR, c_rec.data_ptr(), c_won.data_ptr(), stream.cuda_stream, None))

    def leg_c2():
        bt.check(lib.pmx_align_pairs_frameshift_cigar_device(C.byref(cfg_t), Q.inner, R.inner, listed, d_pairs.data_ptr(), None, pkg.STRAND_BOTH,
                                                             fsp, None, W - 2, MR, tc.rec.data_ptr(), tc.won.data_ptr(), tc.stats.data_ptr(),
                                                             tc.beg.data_ptr(), tc.text.data_ptr(), tc.capacity, tc.off.data_ptr(),
                                                             stream.cuda_stream, None))

    legs = {"a_search": leg_a, "b_search_then_traceback_of_hits": leg_b, "c1_listed_scores": leg_c1, "c2_listed_traceback": leg_c2}
    res = bt.alternated(legs, a.repeats)
    # what came out: the two searches agree, the pass returns the hits' records, the listed legs agree, the texts hold the deletion
    hits = found["hits"]
    assert int(ha.cnt.cpu()[1]) == hits and torch.equal(ha.hr[:hits], hb.hr[:hits]) and torch.equal(th.rec[:hits], hb.hr[:hits])
    assert torch.equal(c_rec, tc.rec) and torch.equal(c_won, tc.won)
    off = th.off[:hits + 1].cpu().numpy(); raw = th.text.cpu().numpy().tobytes()
    assert off[hits] <= th.capacity and int(tc.off[listed]) <= tc.capacity
    texts = [raw[off[k]:off[k + 1]].decode() for k in range(hits)]
    index = hb.hi[:hits].cpu().numpy()
    home = (index % nr) == ((index // nr) % nr)
    line = {"bench": "frameshift_cigar", "device": torch.cuda.get_device_name(dev), "reads": nq, "proteins": nr, "pairs": n, "listed_pairs": listed,
            "shape": "149 nt reads (nucleotide 75 deleted) coding for 48-letter pieces (8 %% substitutions) of proteins of 200 - 400 aa, SW, BLOSUM62, "
                     "gaps 11/1, PMX_STRAND_BOTH, frameshift %d" % fsp,
            "min_score": min_score, "frameshift": fsp, "hits": hits, "home_hits": int(home.sum()),
            "hit_texts_with_slash": sum("/" in t for t in texts), "home_hit_texts_with_slash": sum("/" in t for t, h in zip(texts, home) if h),
            "example_text": texts[0] if texts else None, "hit_text_bytes": int(off[hits]), "listed_text_bytes": int(tc.off[listed]),
            "trace_kernel": found["kernel"], "legs": res,
            "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    ma, mb = res["a_search"]["median_ms"], res["b_search_then_traceback_of_hits"]["median_ms"]
    line["b_minus_a_ms"] = round(mb - ma, 4)
    line["pass_shorter_than_search"] = bool(mb - ma < ma)
    line["c2_over_c1"] = round(res["c2_listed_traceback"]["median_ms"] / res["c1_listed_scores"]["median_ms"], 4)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
