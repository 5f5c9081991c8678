#!/usr/bin/env python3
"""Reference-side translated set search (pmx_search_pairs_translated_ref_device, PMX_FRAMES_ALL) on an MI355X.

Workload: `--nq` proteins of 200 - 400 aa against `--nr` nucleotide references of about 900 nt (870 - 930), PMX_PAIRS_RECT, BLOSUM62,
gaps 11 / 1, local.  Reference j carries, in a random one of the six frames, a 100-letter piece of protein j % nq with 8 %
substitutions, back-translated, between random flanks.

  (a) pmx_search_pairs_translated_ref_device, PMX_FRAMES_ALL: six frames translated, aligned and folded inside the chunks, only the
      hits of the folded records leave;
  (b) the road a caller had before: the references translated on the host in each of the six frames, six protein sets uploaded
      beforehand (not timed), pmx_search_pairs_device over each -- six passes, summed.  With --parent-lib the passes run in a second
      build of the library (the parent commit's) loaded beside this one.

Device events around each leg, one warm-up each, then `--repeats` rounds that run the legs in turn; the JSON line reports median / min /
max and a / b.  Device memory of both roads is read off hipMemGetInfo: (a) first, in a process that has reserved no scratch yet; (b)
adds its six translated reference sets and six hit lists (its chunk scratch is shared with (a)'s, which is larger).  The hits of the two roads are
compared after a host-side fold of (b)'s (frame, pair) hits to pairs: the script exits with an error when they differ.
`--legs a` runs one leg alone (for a kernel trace).  `--out FILE` writes the line there as well."""
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
MQ, MR = 400, WHI // 3
OPEN, EXT = 11, 1
AA = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)
CODE = pkg.genetic_code_table()


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


def workload(nq, nr, rng):
    back = {}
    for i, a in enumerate(CODE):
        back.setdefault(a, []).append(bytes(b"TCAG"[(i >> s) & 3] for s in (4, 2, 0)))
    comp = pkg.complement_table()
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    prots = [AA[rng.integers(0, 20, size=int(l))].tobytes() for l in rng.integers(200, 401, size=nq)]
    refs, frames = [], []
    for j in range(nr):
        src = prots[j % nq]
        at = int(rng.integers(0, len(src) - PIECE))
        piece = bytearray(src[at:at + PIECE])
        for x in np.nonzero(rng.random(PIECE) < 0.08)[0]:
            piece[x] = int(AA[rng.integers(0, 20)])
        f = int(rng.integers(0, 6))
        core = b"".join(back[a][int(rng.integers(0, len(back[a])))] for a in piece)           # 300 nt
        w = int(rng.integers(WLO, WHI + 1))
        left = 3 * int(rng.integers(0, (w - len(core)) // 3)) + f % 3                          # the piece reads in frame f % 3 of the strand it lies on
        s = dna[rng.integers(0, 4, size=left)].tobytes() + core + dna[rng.integers(0, 4, size=w - left - len(core))].tobytes()
        refs.append(comp[np.frombuffer(s, dtype=np.uint8)[::-1]].tobytes() if f >= 3 else s)
        frames.append(f)
    assert all(WLO <= len(s) <= WHI for s in refs)
    return prots, refs, np.array(frames)


class Parent:
    """a second build of the library (the parent commit's), its own matrix and set handles; only entries the parent has"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.pmx_last_error.restype = C.c_char_p
        self.lib.parasail_matrix_lookup.restype = C.c_void_p
        self.lib.parasail_matrix_lookup.argtypes = [C.c_char_p]
        self.lib.pmx_seqset_create.restype = C.c_void_p
        self.lib.pmx_seqset_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        self.lib.pmx_search_pairs_device.restype = C.c_int
        self.lib.pmx_search_pairs_device.argtypes = lib.pmx_search_pairs_device.argtypes
        self.matrix = self.lib.parasail_matrix_lookup(b"blosum62")
        self.cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, OPEN, EXT, 16, 0, C.cast(self.matrix, C.POINTER(pkg.parasail_matrix_t)))

    def seqset(self, seqs):
        buf, off = pkg.pack(seqs)
        return self.lib.pmx_seqset_create(buf.ctypes.data, off.ctypes.data, len(seqs))


class Hits:
    def __init__(self, cap):
        self.cap = cap
        self.hi = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.hr = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.hb = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def take(self):
        written = int(self.cnt.cpu()[1])
        return self.hi[:written].cpu().numpy(), self.hr[:written].cpu().numpy(), self.hb[:written].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=500)
    ap.add_argument("--nr", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-score", type=int, default=150)
    ap.add_argument("--legs", default="", help="letters of the legs to time (default: all), e.g. a")
    ap.add_argument("--parent-lib", default=None, help="a second build of libparasail_amd.so for leg (b)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nq, nr, min_score = a.nq, a.nr, a.min_score
    n = nq * nr
    prots, refs, frames = workload(nq, nr, np.random.default_rng(20261019))
    warm = torch.zeros(16, device=dev); del warm
    free0 = free_bytes()
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, OPEN, EXT, 16, 0, m.inner)
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    ha = Hits(4 * nr + 1024)
    free_inputs = free_bytes()

    def leg_a():
        check(lib.pmx_search_pairs_translated_ref_device(C.byref(cfg), Q.inner, R.inner, pkg.PAIRS_RECT, 0, n, None, MQ, MR, min_score, None,
                                                         ha.hi.data_ptr(), ha.hr.data_ptr(), None, ha.cap, ha.cnt.data_ptr(), stream.cuda_stream, None,
                                                         pkg.FRAMES_ALL, None, ha.hb.data_ptr()))
    leg_a()
    a_bytes = free_inputs - free_bytes()
    a_cnt = ha.cnt.cpu().tolist()
    kernel = lib.pmx_last_kernel().decode()
    a_index, a_recs, a_frame = ha.take()
    line = {"bench": "translated_ref", "device": torch.cuda.get_device_name(dev), "proteins": nq, "references": nr, "pairs": n,
            "shape": "proteins of 200 - 400 aa against references of 870 - 930 nt that carry in a random frame a 100-letter piece (8 % substitutions) "
                     "of protein j % nq, PMX_PAIRS_RECT, SW, BLOSUM62, gaps 11/1, PMX_FRAMES_ALL", "kernel": kernel, "min_score": min_score, "hits": a_cnt[0],
            "hits_in_the_planted_frame": int((a_frame == frames[a_index % nr]).sum()) if a_cnt[0] <= ha.cap else None,
            "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}}
    legs = {"a_translated_all_frames": leg_a}
    if not a.legs or "b" in a.legs:
        parent = Parent(a.parent_lib) if a.parent_lib else None
        free_b0 = free_bytes()
        tsets = [[pkg.translate(s, f) for s in refs] for f in range(6)]                          # the six host-translated reference sets, uploaded beforehand
        if parent:
            pQ = parent.seqset(prots)
            Rf = [parent.seqset(t) for t in tsets]
        else:
            Rf = [pkg.SeqSet.new(t) for t in tsets]
        hb = [Hits(4 * nr + 1024) for _ in range(6)]

        def leg_b():
            for f in range(6):
                h = hb[f]
                if parent:
                    check(parent.lib.pmx_search_pairs_device(C.byref(parent.cfg), pQ, Rf[f], pkg.PAIRS_RECT, 0, n, None, MQ, MR, min_score, None,
                                                             h.hi.data_ptr(), h.hr.data_ptr(), None, h.cap, h.cnt.data_ptr(), stream.cuda_stream, None), parent.lib)
                else:
                    check(lib.pmx_search_pairs_device(C.byref(cfg), Q.inner, Rf[f].inner, pkg.PAIRS_RECT, 0, n, None, MQ, MR, min_score, None,
                                                      h.hi.data_ptr(), h.hr.data_ptr(), None, h.cap, h.cnt.data_ptr(), stream.cuda_stream, None))
        leg_b()
        b_bytes = free_b0 - free_bytes()
        # the host-side fold of the (frame, pair) hits: per pair the highest score, the lowest frame on a tie
        best = {}
        for f in range(6):
            index, recs, _ = hb[f].take()
            for k in range(len(index)):
                p = int(index[k])
                if p not in best or int(recs[k, 0]) > int(best[p][0][0]):
                    best[p] = (recs[k], f)
        order = sorted(best)
        same = (a_cnt[0] == len(order) and a_index.tolist() == order and all(a_recs[x].tolist() == best[p][0].tolist() for x, p in enumerate(order))
                and a_frame.tolist() == [best[p][1] for p in order])
        if not same:
            raise SystemExit("the reference-side translated search and the fold of six host-translated passes differ: %d / %d hits" % (a_cnt[0], len(order)))
        line["hits_equal_fold_of_six_passes"] = True
        line["hits_per_frame_pass_sum"] = int(sum(int(h.cnt.cpu()[0]) for h in hb))
        line["b_is"] = "the parent's library" if parent else "this build (no --parent-lib)"
        line["memory"] = {"inputs_and_hit_buffers_bytes": free0 - free_inputs, "a_scratch_bytes": a_bytes, "b_adds_bytes": b_bytes,
                          "note": "a: chunk buffers for 6 slots per pair and the slots' records; b: six translated reference sets and six hit lists, and " +
                                  ("the chunk scratch of the second library at one slot per pair (a library of its own shares no scratch with this one)" if parent
                                   else "nothing else: its one-slot chunk scratch fits inside a's, which this thread holds already")}
        legs["b_six_passes"] = leg_b
    res = alternated({k: v for k, v in legs.items() if not a.legs or k[0] in a.legs}, a.repeats)
    line["legs"] = res
    if "a_translated_all_frames" in res and "b_six_passes" in res:
        line["a_over_b"] = round(res["a_translated_all_frames"]["median_ms"] / res["b_six_passes"]["median_ms"], 4)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
