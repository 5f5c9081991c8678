#!/usr/bin/env python3
"""Set search on both strands (pmx_search_pairs_stranded_device, PMX_STRAND_BOTH) on an MI355X.

  1. list: 1 M pairs of 150 x 150 DNA through PMX_PAIRS_LIST.  Read k is reference k with 5 % substitutions; every other read is stored
     reverse-complemented, so a forward search finds half of the true hits.  Device legs, device-event timing:
       (a) pmx_search_pairs_stranded_device, PMX_STRAND_BOTH: both strands aligned and folded inside the chunks, only the hits leave;
       (b) pmx_search_pairs_device, forward only, on the same pairs -- from this build and, with --parent-lib, from a second build of
           the library (the parent commit's) loaded beside it, alternated with the others in every round;
       (c) what a caller did before: pmx_align_pairs_ex_device over all pairs with strand 0 and with strand 1, a torch maximum over
           the two record arrays, then pmx_select_hits_device and a gather of the hits.
     The hits of (a) are compared with (c)'s; the device memory (a) takes and what (c) adds are read off hipMemGetInfo (this part
     runs first: the process has reserved no scratch yet).
  2. rect: 1 000 reads x 1 000 references of 150 bp, whole sequences, PMX_PAIRS_RECT; read i is a copy of reference i with 5 %
     substitutions, every other one stored reverse-complemented.  Legs (a) and (b).

One warm-up call per leg, then `--repeats` rounds that run the legs once each in turn; the JSON line reports median / min / max per
leg, a / (2 b) and the acceptance bound 2 b + 3 x the spread (max - min) of the parent's runs.  `--legs a` runs one leg alone (for a
kernel trace).  `--out FILE` writes the line there as well."""
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
L = 150
OPEN, EXT = 5, 2


def check(rc, which=lib):
    if rc:
        raise RuntimeError(which.pmx_last_error().decode())


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
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "runs_ms": [round(x, 4) for x in v]} for k, v in times.items()}


def free_bytes():
    torch.cuda.synchronize(dev)
    return torch.cuda.mem_get_info(dev)[0]


COMP = np.arange(256, dtype=np.uint8)
for a_, b_ in zip(b"ACGT", b"TGCA"):
    COMP[a_] = b_


def reads_of(refs2d, rng):
    """every row with 5 % substitutions; odd rows stored reverse-complemented"""
    reads = refs2d.copy()
    flip = rng.random(reads.shape) < 0.05
    reads[flip] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(flip.sum()))]
    reads[1::2] = COMP[reads[1::2, ::-1]]
    return reads


class Parent:
    """a second build of the library (the parent commit's), its own matrix and set handles; only entries the parent has"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.pmx_last_error.restype = C.c_char_p
        self.lib.parasail_matrix_create.restype = C.c_void_p
        self.lib.parasail_matrix_create.argtypes = [C.c_char_p, C.c_int, C.c_int]
        self.lib.pmx_seqset_wrap_device.restype = C.c_void_p
        self.lib.pmx_seqset_wrap_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        self.lib.pmx_search_pairs_device.restype = C.c_int
        self.lib.pmx_search_pairs_device.argtypes = lib.pmx_search_pairs_device.argtypes
        self.matrix = self.lib.parasail_matrix_create(b"ACGT", 2, -3)
        self.cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, OPEN, EXT, 16, 0, C.cast(self.matrix, C.POINTER(pkg.parasail_matrix_t)))

    def wrap(self, d_buf, d_off, count, nbytes):
        return self.lib.pmx_seqset_wrap_device(d_buf.data_ptr(), d_off.data_ptr(), count, nbytes)


class Case:
    """sets on the device (wrapped: the buffers are torch's), a configuration, hit buffers"""

    def __init__(self, qrows, rrows, parent):
        nq, nr = len(qrows), len(rrows)
        pad = np.zeros(16, dtype=np.uint8)
        self.keep = [torch.from_numpy(x).to(dev) for x in (np.concatenate([qrows.reshape(-1), pad]), np.arange(nq + 1, dtype=np.int64) * L,
                                                           np.concatenate([rrows.reshape(-1), pad]), np.arange(nr + 1, dtype=np.int64) * L)]
        self.Q = pkg.SeqSet.wrap_device(self.keep[0].data_ptr(), self.keep[1].data_ptr(), nq, nq * L, keep=self.keep)
        self.R = pkg.SeqSet.wrap_device(self.keep[2].data_ptr(), self.keep[3].data_ptr(), nr, nr * L, keep=self.keep)
        self.m = pkg.Matrix.create(b"ACGT", 2, -3)
        self.cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, OPEN, EXT, 16, 0, self.m.inner)
        self.parent = parent
        if parent:
            self.pQ, self.pR = parent.wrap(self.keep[0], self.keep[1], nq, nq * L), parent.wrap(self.keep[2], self.keep[3], nr, nr * L)

    def hit_buffers(self, cap):
        self.cap = cap
        self.hp = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        self.hi = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.hr = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.hb = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def search(self, shape, n, d_pairs, min_score, mode):
        check(lib.pmx_search_pairs_stranded_device(C.byref(self.cfg), self.Q.inner, self.R.inner, shape, 0, n, d_pairs, L, L, min_score,
                                                   self.hp.data_ptr(), self.hi.data_ptr(), self.hr.data_ptr(), None, self.cap, self.cnt.data_ptr(),
                                                   stream.cuda_stream, None, mode, self.hb.data_ptr()))

    def forward(self, shape, n, d_pairs, min_score, parent=False):
        if parent:
            p = self.parent
            check(p.lib.pmx_search_pairs_device(C.byref(p.cfg), self.pQ, self.pR, shape, 0, n, d_pairs, L, L, min_score, self.hp.data_ptr(),
                                                self.hi.data_ptr(), self.hr.data_ptr(), None, self.cap, self.cnt.data_ptr(), stream.cuda_stream, None), p.lib)
        else:
            check(lib.pmx_search_pairs_device(C.byref(self.cfg), self.Q.inner, self.R.inner, shape, 0, n, d_pairs, L, L, min_score, self.hp.data_ptr(),
                                              self.hi.data_ptr(), self.hr.data_ptr(), None, self.cap, self.cnt.data_ptr(), stream.cuda_stream, None))


def summary(res):
    out = {"legs": res}
    a, b = res.get("a_both_strands"), res.get("b_parent_forward") or res.get("b_forward")
    if a and b:
        spread = b["max_ms"] - b["min_ms"]
        out["b_is"] = "the parent's library" if "b_parent_forward" in res else "this build (no --parent-lib)"
        out["a_over_2b"] = round(a["median_ms"] / (2 * b["median_ms"]), 4)
        out["bound_ms_2b_plus_3_spreads"] = round(2 * b["median_ms"] + 3 * spread, 4)
        out["a_within_bound"] = a["median_ms"] <= 2 * b["median_ms"] + 3 * spread
        if "b_parent_forward" in res and "b_forward" in res:
            out["forward_this_build_minus_parent_ms"] = round(res["b_forward"]["median_ms"] - b["median_ms"], 4)
            out["forward_within_parent_spread"] = abs(res["b_forward"]["median_ms"] - b["median_ms"]) <= 3 * spread
    return out


def part_list(n, repeats, legs, parent):
    rng = np.random.default_rng(20261001)
    refs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, L))]
    reads = reads_of(refs, rng)
    warm = torch.zeros(16, device=dev); del warm
    free0 = free_bytes()
    c = Case(reads, refs, parent)
    pairs = np.zeros(n, dtype=pkg.PAIR_DTYPE)
    pairs["q"], pairs["r"], pairs["q_len"], pairs["r_len"] = np.arange(n), np.arange(n), -1, -1
    d_pairs = torch.from_numpy(pairs.view(np.uint8)).to(dev)
    min_score = 150                                                  # far above unrelated 150 x 150 DNA (about 30), below every planted pair
    c.hit_buffers(n + 1024)
    free_inputs = free_bytes()
    BOTH = pkg.STRAND_BOTH

    def leg_a():
        c.search(pkg.PAIRS_LIST, n, d_pairs.data_ptr(), min_score, BOTH)
    leg_a()
    a_bytes = free_inputs - free_bytes()                             # (a): the chunk scratch of the calling thread
    a_cnt = c.cnt.cpu().tolist()
    a_hits = (c.hi[:a_cnt[1]].clone(), c.hr[:a_cnt[1]].clone(), c.hb[:a_cnt[1]].clone())
    kernel = lib.pmx_last_kernel().decode()
    out = {"pairs": n, "shape": "150 x 150 DNA, reads = references with 5 % substitutions, every other read stored reverse-complemented, SW, "
                                "gaps 5/2, width 16, PMX_PAIRS_LIST", "kernel": kernel, "min_score": min_score, "hits_both": a_cnt[0],
           "hits_on_reverse_strand": int(a_hits[2].sum().item())}
    all_legs = {"a_both_strands": leg_a,
                "b_forward": lambda: c.forward(pkg.PAIRS_LIST, n, d_pairs.data_ptr(), min_score),
                "b_parent_forward": (lambda: c.forward(pkg.PAIRS_LIST, n, d_pairs.data_ptr(), min_score, True)) if parent else None}
    if legs and "c" not in legs:                                     # (a trace of single legs: no yardstick run beside them)
        out.update(summary(alternated({k: v for k, v in all_legs.items() if v and k[0] in legs}, repeats)))
        return out
    # (c): two full record arrays, strand arrays, the selection's index array
    free_c0 = free_bytes()
    rec0 = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    rec1 = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    s0 = torch.zeros(n, dtype=torch.uint8, device=dev)
    s1 = torch.ones(n, dtype=torch.uint8, device=dev)
    sel = torch.zeros(n + 1024, dtype=torch.int64, device=dev)
    ccnt = torch.zeros(2, dtype=torch.int64, device=dev)
    c_out = {}

    def leg_c():
        for s, rec in ((s0, rec0), (s1, rec1)):
            check(lib.pmx_align_pairs_ex_device(C.byref(c.cfg), c.Q.inner, c.R.inner, n, d_pairs.data_ptr(), s.data_ptr(), L, L, rec.data_ptr(), None,
                                                None, None, 0, None, stream.cuda_stream, None))
        won = rec1[:, 0] > rec0[:, 0]
        folded = torch.where(won[:, None], rec1, rec0)
        check(lib.pmx_select_hits_device(folded.data_ptr(), n, min_score, 0, pkg.HITS_BY_INDEX, sel.data_ptr(), n + 1024, ccnt.data_ptr(), stream.cuda_stream))
        c_out["folded"], c_out["won"] = folded, won
    leg_c()
    c_bytes = free_c0 - free_bytes()                                 # (torch's cache keeps the temporaries of the fold: they count)
    cc = ccnt.cpu().tolist()
    idx = sel[:cc[0]]
    equal = (a_cnt == [cc[0], cc[0]] and bool((a_hits[0] == idx).all().item()) and bool((a_hits[1] == c_out["folded"][idx]).all().item())
             and bool((a_hits[2] == c_out["won"][idx].to(torch.uint8)).all().item()))
    if not equal:
        raise SystemExit("the BOTH search and the fold of two _ex runs differ: counts %s / %s" % (a_cnt, cc))
    mem = {"inputs_and_hit_buffers_bytes": free0 - free_inputs, "a_scratch_bytes": a_bytes, "c_adds_bytes": c_bytes,
           "note": "a: chunk buffers for 2 slots per pair and slot records; c: two n x 16 record arrays, 2 n strand bytes, the fold's temporaries, "
                   "the selection's index array, on top of (a)'s chunk scratch, which _ex shares"}
    out["hits_equal_fold_of_two_ex_runs"], out["memory"] = equal, mem
    all_legs["c_two_ex_runs_max_select"] = leg_c
    res = alternated({k: v for k, v in all_legs.items() if v and (not legs or k[0] in legs)}, repeats)
    c.forward(pkg.PAIRS_LIST, n, d_pairs.data_ptr(), min_score)
    out["hits_forward_only"] = c.cnt.cpu().tolist()[0]
    out.update(summary(res))
    return out


def part_rect(nq, nr, repeats, legs, parent):
    rng = np.random.default_rng(20261002)
    refs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(nr, L))]
    reads = reads_of(refs[np.arange(nq) % nr], rng)
    c = Case(reads, refs, parent)
    n = nq * nr
    min_score = 150
    c.hit_buffers(4 * nq + 1024)
    all_legs = {"a_both_strands": lambda: c.search(pkg.PAIRS_RECT, n, None, min_score, pkg.STRAND_BOTH),
                "b_forward": lambda: c.forward(pkg.PAIRS_RECT, n, None, min_score),
                "b_parent_forward": (lambda: c.forward(pkg.PAIRS_RECT, n, None, min_score, True)) if parent else None}
    res = alternated({k: v for k, v in all_legs.items() if v and (not legs or k[0] in legs)}, repeats)
    hits = {}
    for name, mode in (("both", pkg.STRAND_BOTH), ("forward", pkg.STRAND_FORWARD), ("reverse", pkg.STRAND_REVERSE)):
        c.search(pkg.PAIRS_RECT, n, None, min_score, mode)
        hits[name] = c.cnt.cpu().tolist()[0]
    out = {"reads": nq, "references": nr, "pairs": n, "shape": "150 bp reads x 150 bp references, PMX_PAIRS_RECT, SW, gaps 5/2, width 16",
           "kernel": lib.pmx_last_kernel().decode(), "min_score": min_score, "hits": hits}
    out.update(summary(res))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--nr", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="list,rect")
    ap.add_argument("--legs", default="", help="letters of the legs to time (default: all), e.g. a")
    ap.add_argument("--parent-lib", default=None, help="a second build of libparasail_amd.so for leg (b)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = Parent(a.parent_lib) if a.parent_lib else None
    line = {"bench": "both_strands", "device": torch.cuda.get_device_name(dev), "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    parts = a.parts.split(",")
    if "list" in parts:                                             # first: its memory figures want a process that has reserved no scratch
        line["list"] = part_list(a.n, a.repeats, a.legs, parent)
    if "rect" in parts:
        line["rect"] = part_rect(a.nq, a.nr, a.repeats, a.legs, parent)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
