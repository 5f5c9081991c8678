#!/usr/bin/env python3
"""Windowed reference-side frameshift traceback (pmx_align_pairs_frameshift_ref_cigar_long_device) on an MI355X, against
the entry that traces the whole matrix (pmx_align_pairs_frameshift_ref_cigar_device), on shapes both run, and alone where that entry
refuses.  SW, BLOSUM62, gaps 11 / 1, frameshift 15, PMX_STRAND_BOTH, listed pairs (i, i), text, begins and statistics.

  contig   `--pairs` proteins of 400 aa, each planted whole -- 2 % substitutions, one nucleotide deleted at mid-gene -- on a random strand
           at a random place of a 20 kb reference: old entry and new entry;
  short    the hits' shape of profiles/bench_frameshift_ref_cigar.py, proteins of 200 - 400 aa against references of 870 - 930 nt that
           carry a 100-letter piece: old entry and new entry -- the shape on which the second sweep and the host round trip buy nothing;
  tiny     `--tiny-pairs` proteins of 30 aa planted whole in 120 nt references: old entry and new entry -- there is next to nothing to cut;
  long     `--long-pairs` proteins of 4 096 aa planted the same way (no substitutions) in 100 kb references: the new entry alone; the
           old entry's refusal text is recorded.

Device events around each leg, one warm-up each, then `--repeats` rounds that run a shape's legs in turn; median / min / max, the new
entry's parts per chunk and chunks, new / old.  The script exits with an error unless every output array of the new entry equals the
old entry's, byte for byte, on the shapes both run; how many texts hold exactly one '/' is reported.  The JSON line is printed and
written to `--out` (default: beside this script)."""
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
import bench_frameshift_ref as br  # noqa: E402  (the short workload and the timing loop)

pkg, lib, dev, stream = br.pkg, br.lib, br.dev, br.stream
OPEN, EXT, FS = br.OPEN, br.EXT, br.FS
NAMES = ("rec", "won", "stats", "beg", "off", "text")


class Out:
    def __init__(self, n, text_bytes):
        self.rec = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        self.won = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.stats = torch.zeros((n, 3), dtype=torch.int32, device=dev)
        self.beg = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        self.text = torch.zeros(text_bytes, dtype=torch.uint8, device=dev)
        self.off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self.capacity = text_bytes


def planted(rng, n, aa, nt, subs):
    """n proteins of `aa` letters and n references of `nt` nucleotides: reference i codes for protein i (a share `subs` of the letters
    replaced) with one nucleotide deleted at mid-gene, at a random place, every other one reverse-complemented"""
    back = {}
    for i, a in enumerate(br.CODE):
        back.setdefault(a, []).append(bytes(b"TCAG"[(i >> s) & 3] for s in (4, 2, 0)))
    comp = pkg.complement_table()
    prots, refs = [], []
    for i in range(n):
        p = br.AA[rng.integers(0, 20, size=aa)].tobytes()
        piece = bytearray(p)
        for x in np.nonzero(rng.random(aa) < subs)[0]:
            piece[x] = int(br.AA[rng.integers(0, 20)])
        core = b"".join(back[a][int(rng.integers(0, len(back[a])))] for a in piece)
        core = core[:len(core) // 2] + core[len(core) // 2 + 1:]
        left = int(rng.integers(0, nt - len(core)))
        s = br.DNA[rng.integers(0, 4, size=left)].tobytes() + core + br.DNA[rng.integers(0, 4, size=nt - left - len(core))].tobytes()
        prots.append(p)
        refs.append(comp[np.frombuffer(s, dtype=np.uint8)[::-1]].tobytes() if i % 2 else s)
    return prots, refs


def shape(name, prots, refs, pairs, cfg, repeats, both, what):
    n = len(pairs)
    mq, mr = max(len(p) for p in prots), max(len(r) for r in refs) - 2
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(refs)
    d_pairs = torch.from_numpy(pairs.view(np.uint8)).to(dev)
    new, old = Out(n, 256 * n), Out(n, 256 * n)
    info = {}

    def call(entry, o):
        return entry(C.byref(cfg), Q.inner, R.inner, n, d_pairs.data_ptr(), None, pkg.STRAND_BOTH, FS, None, mq, mr, o.rec.data_ptr(),
                     o.won.data_ptr(), o.stats.data_ptr(), o.beg.data_ptr(), o.text.data_ptr(), o.capacity, o.off.data_ptr(),
                     stream.cuda_stream, None)

    def leg_new():
        br.check(call(lib.pmx_align_pairs_frameshift_ref_cigar_long_device, new))
        info["parts"] = int(lib.pmx_frameshift_ref_cigar_long_parts())
        info["kernel"] = lib.pmx_last_kernel().decode()

    def leg_old():
        br.check(call(lib.pmx_align_pairs_frameshift_ref_cigar_device, old))

    legs = {"new_windowed": leg_new}
    if both:
        legs["old_whole_matrix"] = leg_old
    res = br.alternated(legs, repeats)
    four = 4 * int(lib.pmx_swfsc_trace_bytes_per_slot(mq, mr))
    line = {"what": what, "pairs": n, "max_qlen": mq, "max_rlen": mr, "four_slots_whole_matrix_bytes": four, "legs": res,
            "chunks": 1, "parts_per_chunk": info["parts"], "trace_kernel": info["kernel"]}
    off = new.off.cpu().numpy(); raw = new.text.cpu().numpy().tobytes()
    assert off[n] <= new.capacity
    texts = [raw[off[k]:off[k + 1]].decode() for k in range(n)]
    line["texts_with_one_slash"] = sum(t.count("/") == 1 for t in texts)
    line["example_text"] = texts[0]
    rec = new.rec.cpu().numpy()
    line["median_score"] = int(np.median(rec[:, 0]))
    if both:
        for nm in NAMES:
            if not torch.equal(getattr(new, nm), getattr(old, nm)):
                raise SystemExit("%s: the windowed entry's %s differs from the whole-matrix entry's" % (name, nm))
        line["new_over_old"] = round(res["new_windowed"]["median_ms"] / res["old_whole_matrix"]["median_ms"], 4)
        line["outputs_byte_identical"] = True
        bound = 256.0 * 1024 * 1024
        line["old_pairs_per_part"] = int(bound // (four // 4)) // 4 * 4 // 2
    else:
        rc = call(lib.pmx_align_pairs_frameshift_ref_cigar_device, old)
        line["old_entry"] = "refused: " + lib.pmx_last_error().decode() if rc else "ran"
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--short-pairs", type=int, default=2000)
    ap.add_argument("--long-pairs", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tiny-pairs", type=int, default=20000)
    ap.add_argument("--shapes", default="contig,short,tiny,long")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_frameshift_ref_cigar_long.json"))
    a = ap.parse_args()
    m = pkg.Matrix.from_name("blosum62")
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, OPEN, EXT, 0, pkg.WANT_CIGAR | pkg.WANT_STATS, m.inner)
    line = {"bench": "frameshift_ref_cigar_long", "device": torch.cuda.get_device_name(dev), "gaps": [OPEN, EXT], "frameshift": FS,
            "strand_mode": "both", "repeats": a.repeats, "env": {k: v for k, v in os.environ.items() if k.startswith("PMX_")}, "shapes": {}}

    def diagonal(n):
        d = np.zeros(n, dtype=pkg.PAIR_DTYPE)
        d["q"] = np.arange(n); d["r"] = np.arange(n); d["q_len"] = -1; d["r_len"] = -1
        return d

    if "contig" in a.shapes:
        prots, refs = planted(np.random.default_rng(20261020), a.pairs, 400, 20000, 0.02)
        line["shapes"]["contig"] = shape("contig", prots, refs, diagonal(a.pairs), cfg, a.repeats, True,
                                         "400 aa planted whole (2 % substitutions, one nucleotide deleted) in 20 kb references")
    if "short" in a.shapes:
        prots, deleted, _ = br.workload(500, a.short_pairs, np.random.default_rng(20261019))
        d = diagonal(a.short_pairs); d["q"] = np.arange(a.short_pairs) % 500
        line["shapes"]["short"] = shape("short", prots, deleted, d, cfg, a.repeats, True,
                                        "200 - 400 aa against 870 - 930 nt references that carry a 100-letter piece with one nucleotide deleted")
    if "tiny" in a.shapes:
        prots, refs = planted(np.random.default_rng(20261022), a.tiny_pairs, 30, 120, 0.0)
        line["shapes"]["tiny"] = shape("tiny", prots, refs, diagonal(a.tiny_pairs), cfg, a.repeats, True,
                                       "30 aa planted whole (one nucleotide deleted) in 120 nt references")
    if "long" in a.shapes:
        prots, refs = planted(np.random.default_rng(20261021), a.long_pairs, 4096, 100000, 0.0)
        line["shapes"]["long"] = shape("long", prots, refs, diagonal(a.long_pairs), cfg, max(1, a.repeats // 2), False,
                                       "4 096 aa planted whole (one nucleotide deleted) in 100 kb references")
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
