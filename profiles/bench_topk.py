#!/usr/bin/env python3
"""Per-query top-K set search (pmx_search_topk_device) on an MI355X.

Two shapes:
  proteins  many short rows: 4 000 synthetic proteins of 200-400 aa (bench_set_search.py's set and seed) against themselves, 16 M
            pairs, BLOSUM62, local, K = 10, skip_self, min_score = INT32_MIN;
  dna       few long rows: 8 DNA queries of 150 bp against 1 M references of 150 bp (config 2's generator), local, K = 100.
Legs, device-event timing, alternated in one process:
  (a) pmx_search_topk_device;
  (b) pmx_search_pairs_device over the same rectangle at the min_score 1 % of the pairs reach (the yardstick: an entry that existed
      before);
  (c) the full entry (rectangle descriptors + pmx_align_pairs_device, every record) followed by torch.topk per row: what a caller
      did before.
At benchmark size (a)'s outputs are compared with tests/topk_ref.py applied to the full entry's records; the script exits with an
error when they differ.  `memory` reads off hipMemGetInfo what (a) takes on the protein shape and what (c) adds on top, in a process
that has run nothing else.

One warm-up call per leg, then `--repeats` rounds that run the legs once each in turn; the JSON line reports median / min / max per
leg.  `--out FILE` writes it there as well (profiles/r11/bench_topk.json)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (torch's HIP runtime first)
import __graft_entry__ as g  # noqa: E402
import workloads as wl  # noqa: E402
import topk_ref  # noqa: E402
from bench_set_search import protein_set, alternated, event_ms, ratio, free_bytes, check  # noqa: E402

pkg = g.load_pkg()
lib = pkg.lib
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)
INT32_MIN = -(1 << 31)


class Rect:
    """the buffers and the three legs of one shape"""

    def __init__(self, cfg, Q, R, nq, nr, mq, mr, k, skip_self, with_c=True):
        self.cfg, self.Q, self.R, self.nq, self.nr, self.mq, self.mr, self.k, self.skip = cfg, Q, R, nq, nr, mq, mr, k, skip_self
        self.n = nq * nr
        cap = nq * min(k, nr)
        self.cap = cap
        self.hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        self.hi = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.hr = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        self.rp = torch.zeros(nq, dtype=torch.int64, device=dev)
        self.cnt = torch.zeros(3, dtype=torch.int64, device=dev)
        if with_c:
            self.descs = torch.zeros(self.n * 32, dtype=torch.uint8, device=dev)
            self.rec = torch.zeros((self.n, 4), dtype=torch.int32, device=dev)

    def topk(self):
        check(lib.pmx_search_topk_device(C.byref(self.cfg), self.Q.inner, self.R.inner, 0, self.nq, self.mq, self.mr, INT32_MIN, self.k,
                                         1 if self.skip else 0, self.hp.data_ptr(), self.hi.data_ptr(), self.hr.data_ptr(), None, self.cap,
                                         self.off.data_ptr(), self.rp.data_ptr(), self.cnt.data_ptr(), stream.cuda_stream, None))

    def full(self):
        check(lib.pmx_rect_pairs_enumerate_device(self.nq, self.nr, 0, self.n, self.descs.data_ptr(), stream.cuda_stream))
        check(lib.pmx_align_pairs_device(C.byref(self.cfg), self.Q.inner, self.R.inner, self.n, self.descs.data_ptr(), self.mq, self.mr,
                                         self.rec.data_ptr(), None, stream.cuda_stream, None))

    def full_then_torch(self):
        self.full()
        self.tk = torch.topk(self.rec[:, 0].view(self.nq, self.nr), min(self.k + (1 if self.skip else 0), self.nr), dim=1)

    def threshold_buffers(self):
        scores = self.rec[:, 0]
        self.min_score = int(torch.kthvalue(scores, self.n - self.n // 100).values.item())
        self.passing = int((scores >= self.min_score).sum().item())
        c = self.passing + 1024
        self.scap = c
        self.sp = torch.zeros(c * 32, dtype=torch.uint8, device=dev)
        self.si = torch.zeros(c, dtype=torch.int64, device=dev)
        self.sr = torch.zeros((c, 4), dtype=torch.int32, device=dev)
        self.scnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def search(self):
        check(lib.pmx_search_pairs_device(C.byref(self.cfg), self.Q.inner, self.R.inner, pkg.PAIRS_RECT, 0, self.n, None, self.mq, self.mr,
                                          self.min_score, self.sp.data_ptr(), self.si.data_ptr(), self.sr.data_ptr(), None, self.scap,
                                          self.scnt.data_ptr(), stream.cuda_stream, None))

    def verify(self):
        """(a) against tests/topk_ref.py on the full entry's records, at this size"""
        recs = self.rec.cpu().numpy()
        want = topk_ref.topk(recs, self.nr, 0, self.nq, self.k, INT32_MIN, self.skip)
        kept = want["counts"][0]
        ok = (self.cnt.cpu().tolist() == want["counts"] and self.off.cpu().numpy().tolist() == want["row_off"].tolist()
              and self.rp.cpu().numpy().tolist() == want["row_passing"].tolist()
              and self.hi.cpu().numpy()[:kept].tolist() == want["index"].tolist()
              and self.hr.cpu().numpy()[:kept].tobytes() == want["records"].tobytes()
              and self.hp.cpu().numpy()[:kept * 32].tobytes() == want["pairs"].tobytes())
        if not ok:
            raise SystemExit("pmx_search_topk_device and topk_ref over the full records differ (%d x %d, K = %d)" % (self.nq, self.nr, self.k))
        return kept

    def run(self, repeats):
        self.full(); torch.cuda.synchronize(dev)
        kernel = lib.pmx_last_kernel().decode()
        self.threshold_buffers()
        self.topk(); torch.cuda.synchronize(dev)
        kept = self.verify()
        res = alternated({"a_search_topk_device": self.topk, "b_search_pairs_device_rect": self.search, "c_full_entry_then_torch_topk": self.full_then_torch},
                         repeats, event_ms)
        return {"queries": self.nq, "references": self.nr, "pairs": self.n, "k": self.k, "skip_self": self.skip, "kernel": kernel, "kept": kept,
                "equal_topk_ref_over_full_records": True, "b_min_score": self.min_score, "b_passing": self.passing,
                "a_over_b": ratio(res, "a_search_topk_device", "b_search_pairs_device_rect"),
                "a_over_c": ratio(res, "a_search_topk_device", "c_full_entry_then_torch_topk"), "legs": res}


def protein_rect(nseq, with_c=True):
    seqs = protein_set(nseq, 40, 64)
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 11, 1, 16, 0, m.inner)
    S = pkg.SeqSet.new(seqs)
    mx = max(len(s) for s in seqs)
    r = Rect(cfg, S, S, nseq, nseq, mx, mx, 10, True, with_c)
    r.keep = (m, seqs)
    return r


def part_memory(nseq):
    warm = torch.zeros(16, device=dev); del warm
    free0 = free_bytes()
    r = protein_rect(nseq, with_c=False)
    r.topk()
    a_bytes = free0 - free_bytes()
    f1 = free_bytes()
    r.descs = torch.zeros(r.n * 32, dtype=torch.uint8, device=dev)
    r.rec = torch.zeros((r.n, 4), dtype=torch.int32, device=dev)
    r.full_then_torch()
    c_adds = f1 - free_bytes()
    out = {"a_bytes_%d_x_%d" % (nseq, nseq): a_bytes, "a_hit_buffer_bytes": r.cap * 56 + (2 * r.nq + 4) * 8, "c_adds_bytes": c_adds,
           "c_record_and_descriptor_bytes": r.n * 48}
    del r
    torch.cuda.empty_cache()
    return out


def part_dna(nq, nr, repeats):
    qbuf, qoff, rbuf, roff = wl.make_cfg2(nr)
    c = wl.CFG2
    L = c["len"]
    rs = [rbuf[roff[k]:roff[k + 1]].tobytes() for k in range(nr)]
    qs = [qbuf[qoff[k]:qoff[k + 1]].tobytes() for k in range(nq)]
    m = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, c["open"], c["ext"], 16, 0, m.inner)
    r = Rect(cfg, pkg.SeqSet.new(qs), pkg.SeqSet.new(rs), nq, nr, L, L, 100, False)
    r.keep = m
    return r.run(repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=4000)
    ap.add_argument("--nq", type=int, default=8)
    ap.add_argument("--nr", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="memory,proteins,dna")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = {"bench": "topk", "device": torch.cuda.get_device_name(dev), "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    parts = a.parts.split(",")
    if "memory" in parts:                                           # first: the process has reserved no scratch yet
        line["memory"] = part_memory(a.nseq)
    if "proteins" in parts:
        line["proteins"] = protein_rect(a.nseq).run(a.repeats)
        torch.cuda.empty_cache()
    if "dna" in parts:
        line["dna"] = part_dna(a.nq, a.nr, a.repeats)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
