"""CPU tier: the stored-arithmetic model of the packed statistics kernel (tests/stats16p_model.c) against the oracle and at the
corners of the two host gates of pmx_launch_stats16p.

pmx_stats16p_kernel returns its six fields as final: no promotion pass stands behind it.  Its H / E / F live in 16-bit halves that
pmx_nwsgv_bias (the form WITHOUT a row offset, exported as pmx_window_nwsgv with rowx = 0) must keep inside [1024, 31743], its
statistics in 16-bit halves that `max_qlen + max_rlen + 2 <= 32767` must keep from wrapping or carrying into the other pair of the
lane slot.  The model replays one lane slot -- both halves, 32-bit adds, packed selects, captures, the clamped combine key -- and
counts what leaves its domain; here it must equal the oracle in all six fields and count nothing whenever the host admits the batch.

Which gate binds: pmx_nwsgv_bias refuses references above 30 000 letters and, with ext >= 1 (the kernel's own condition), every
reference above (31 743 - 2 048 - (max_qlen + 134) ext) / (2 ext) < 14 848 letters (the decline along the gaps and the column skew
each cost ext per column); the three shapes hold at most 640 rows.  So max_qlen + max_rlen + 2 stays below 15 500 wherever the proof
admits a batch: the PROOF binds in every case the search below visits (asserted there), the length gate never does, and no
statistics half comes near 32 767 (the largest one seen is printed)."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from util import AA, golden, random_seqs

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(16, 10), (32, 10), (64, 10)]


class Out(C.Structure):
    _fields_ = [(n, C.c_int * 2) for n in ("score", "end_query", "end_ref", "matches", "similar", "length")] + \
               [(n, C.c_int) for n in ("lo", "hi", "violations", "pad_violations", "pad_lo", "pad_hi", "dead_violations", "stat_hi", "stat_violations", "clamp_hits", "first_violation_kind")]

    def fields(self, h):
        return tuple(int(getattr(self, n)[h]) for n in ("score", "end_query", "end_ref", "matches", "similar", "length"))

    def counted(self):
        return (self.violations, self.pad_violations, self.stat_violations, self.clamp_hits)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stats16p_model") / "stats16p_model.so")
    subprocess.run(["gcc", "-O3", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "stats16p_model.c")], check=True)
    lib = C.CDLL(so)
    lib.stats16p_model.restype = C.c_int
    return lib


def _window(pkg, qlen, rlen, smin, smax, open_, ext, msize):
    """the bias pmx_launch_stats16p asks for: the proof without a row offset, shape rows left to its own estimate"""
    pkg.lib.pmx_window_nwsgv.restype = C.c_int
    return pkg.lib.pmx_window_nwsgv(int(qlen), int(rlen), int(msize), int(smin), int(smax), int(open_), int(ext), 0, 0)


def _admitted(pkg, qlen, rlen, smin, smax, open_, ext, msize):
    """both host gates of pmx_launch_stats16p; the bias, or 0"""
    if ext < 1 or qlen + rlen + 2 > 32767:
        return 0
    return _window(pkg, qlen, rlen, smin, smax, open_, ext, msize)


def _run(model, G, R, ml, pairs, max_rlen, mat, msize, open_, ext, sg, nb):
    """pairs: ((qA, rA), (qB, rB)) as mapped symbols (uint8 arrays)"""
    mat = np.ascontiguousarray(mat, dtype=np.int32)
    a = [np.ascontiguousarray(x, dtype=np.uint8) for p in pairs for x in p]
    out = Out()
    rc = model.stats16p_model(G, R, ml, a[0].ctypes.data_as(C.c_void_p), len(a[0]), a[1].ctypes.data_as(C.c_void_p), len(a[1]),
                              a[2].ctypes.data_as(C.c_void_p), len(a[2]), a[3].ctypes.data_as(C.c_void_p), len(a[3]), int(max_rlen),
                              mat.ctypes.data_as(C.c_void_p), msize, open_, ext, int(not (sg & 1)), int(not (sg & 4)), int(bool(sg & 2)), int(bool(sg & 8)),
                              nb, C.byref(out))
    assert rc == 0
    return out


def _run_all(model, jobs):
    """ctypes releases the interpreter lock for the model's run: a few threads work side by side.  Results in the jobs' order."""
    with ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as ex:
        return list(ex.map(lambda a: _run(model, *a), jobs))


def _oracle(orc, om, pairs, open_, ext, sg):
    """the six fields of the two pairs (bytes)"""
    qb, qo = orc.pack([p[0] for p in pairs]); rb, ro = orc.pack([p[1] for p in pairs])
    w = orc.align_stats_sample(orc.NW if sg == 0 else orc.SG, np.arange(len(pairs)), qb, qo, rb, ro, open_, ext, om, sg_flags=sg if sg else orc.SG_ALL, bits=32)
    return [tuple(int(x) for x in row[:6]) for row in w]


def _schemes(orc):
    """(oracle matrix, letters, size handed to the proof, alphabet, hot letter, cold letter)"""
    b62 = orc.Matrix.from_file(golden("blosum62.txt"))
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = {"b62": (b62, 24, AA, b"W", b"*")}
    for match, mis in ((2, -3), (1, -1), (5, -4), (3, -2), (9, -9), (1, -30)):
        out[(match, mis)] = (orc.Matrix.create("ACGT", match, mis), 5, dna, b"A", b"C")
    return out


def _mapped(om, seq):
    return om.mapper.astype(np.uint8)[np.frombuffer(seq, dtype=np.uint8)]


def test_model_matches_the_oracle_on_small_pairs(orc, pkg, model):
    """two different pairs in the two halves of a slot, the three shapes of the kernel and a small one, profile and matrix-lookup
    increments, all 16 free-end sets, gap models with open == ext: the six fields of both halves are the oracle's, nothing is counted"""
    rng = np.random.default_rng(7100)
    sch = _schemes(orc)
    n = 0
    seen_sg = set()
    for it in range(220):
        G, R = (SHAPES + [(4, 3)])[it % 4]
        key = ["b62", (2, -3), (1, -1), (5, -4), (9, -9)][int(rng.integers(0, 5))]
        om, msize, alphabet, _, _ = sch[key]
        smin, smax = int(om.scores[:msize, :msize].min()), int(om.scores[:msize, :msize].max())
        gaps = [g for g in ((11, 1), (10, 2), (11, 11), (4, 4), (5, 2), (1, 1), (3, 3), (20, 3), (9, 9)) if g[0] + smin >= 0]    # (a profile byte is score + open)
        open_, ext = gaps[int(rng.integers(0, len(gaps)))]
        sg = it % 16
        pairs = []
        below = {160: 0, 320: 160, 640: 320}.get(G * R, 0)             # (the launcher takes the smallest shape that holds the longest query)
        for h in range(2):
            qlen = int(rng.choice([1, 2, G * R, G * R - 1, int(rng.integers(1, G * R + 1))])) if h else int(rng.choice([below + 1, G * R, int(rng.integers(below + 1, G * R + 1))]))
            rlen = int(rng.choice([1, 2, 17, int(rng.integers(1, 260))]))
            q, r = random_seqs(rng, 1, qlen, qlen, alphabet)[0], random_seqs(rng, 1, rlen, rlen, alphabet)[0]
            if rng.random() < 0.5:
                r = (q * (rlen // qlen + 1))[:rlen]
            pairs.append((q, r))
        mq, mr = max(len(p[0]) for p in pairs), max(len(p[1]) for p in pairs)
        nb = _admitted(pkg, mq, mr, smin, smax, open_, ext, msize)
        assert nb, (key, open_, ext, mq, mr)
        want = _oracle(orc, om, pairs, open_, ext, sg)
        for ml in (0, 1):
            out = _run(model, G, R, ml, [(_mapped(om, q), _mapped(om, r)) for q, r in pairs], mr + int(rng.integers(0, 40)),
                       om.scores[:msize, :msize], msize, open_, ext, sg, nb)
            assert [out.fields(0), out.fields(1)] == want and out.counted() == (0, 0, 0, 0), \
                (G, R, ml, key, open_, ext, sg, pairs, [out.fields(0), out.fields(1)], want, out.counted(), out.lo, out.hi, out.pad_lo, out.pad_hi)
            n += 1
        seen_sg.add(sg)
    assert n >= 400 and len(seen_sg) == 16, (n, seen_sg)


# the scoring schemes of tests/test_window_models.py's window test, and BLOSUM62 under the production gap model
EDGE_SCHEMES = [((2, -3), 5, 2), ((1, -1), 1, 1), ((5, -4), 10, 1), ((3, -2), 4, 4), ((9, -9), 20, 3), ((1, -30), 60, 1), ((2, -3), 120, 5), ("b62", 11, 1)]


def test_nothing_leaves_its_domain_at_the_longest_reference_the_host_admits(orc, pkg, model):
    """Per scoring scheme and shape, the query filling the shape's last row (and, for BLOSUM62, one row past the shape before): the
    longest reference both gates admit and one short of it.  One half of the slot holds that reference, the other a reference of 37
    letters -- it runs thousands of pad columns past its end, its counters still incremented by the 32-bit adds -- in both
    orders.  Pairs that stretch the range: the hottest letter throughout, the query repeated, the query behind a long unrelated
    prefix, the coldest letter throughout, random.  No max3 operand leaves [1024, 31743] (not even in the pad columns), no
    statistics half passes 32 767 or carries, no last-column candidate falls below the combine key's clamp, and every fourth run
    equals the oracle in all six fields of both halves."""
    rng = np.random.default_rng(7200)
    sch = _schemes(orc)
    jobs, meta = [], []
    binds = {}
    for key, open_, ext in EDGE_SCHEMES:
        om, msize, alphabet, hot, cold = sch[key]
        smin, smax = int(om.scores[:msize, :msize].min()), int(om.scores[:msize, :msize].max())
        for G, R in SHAPES:
            for qlen in [G * R] + ([G * R // 2 + 1] if key == "b62" else []):
                assert _admitted(pkg, qlen, 1, smin, smax, open_, ext, msize), (key, open_, ext, qlen)
                lo, hi = 1, 32767
                while hi - lo > 0:                                   # the longest reference both gates admit
                    mid = (lo + hi + 1) // 2
                    lo, hi = (mid, hi) if _admitted(pkg, qlen, mid, smin, smax, open_, ext, msize) else (lo, mid - 1)
                longest = lo
                proof = not _window(pkg, qlen, longest + 1, smin, smax, open_, ext, msize)
                binds[(key, open_, ext, G, qlen)] = (longest, "proof" if proof else "length gate")
                for li, rlen in enumerate((longest, max(1, longest - 1))):
                    nb = _admitted(pkg, qlen, rlen, smin, smax, open_, ext, msize)
                    assert nb
                    q0 = random_seqs(rng, 1, qlen, qlen, alphabet)[0]
                    far = random_seqs(rng, 1, rlen, rlen, alphabet)[0]
                    fams = [(hot * qlen, hot * rlen), (q0, (q0 * (rlen // qlen + 1))[:rlen]), (q0, far[:rlen - qlen] + q0 if rlen > qlen else far),
                            (hot * qlen, cold * rlen), (q0, far)]
                    short = (random_seqs(rng, 1, max(1, qlen - 7), max(1, qlen - 7), alphabet)[0], random_seqs(rng, 1, 37, 37, alphabet)[0])
                    for fi, long_ in enumerate(fams if li == 0 else fams[:4:3] + fams[2:3]):
                        for sg in ((0, 15, 10, 5, 2, 8)[(fi + li) % 6], (0, 15, 10, 5, 2, 8)[(fi + li + 3) % 6]):
                            pairs = [long_, short] if (fi + sg) % 2 else [short, long_]
                            jobs.append((G, R, int(key == "b62" and fi % 2), [(_mapped(om, q), _mapped(om, r)) for q, r in pairs], rlen,
                                         om.scores[:msize, :msize], msize, open_, ext, sg, nb))
                            meta.append((key, pairs))
    for k, v in sorted(binds.items(), key=str):
        print("stats16p gates %s: longest reference admitted %d, bound by the %s" % (k, v[0], v[1]))
    assert {v[1] for v in binds.values()} == {"proof"}, binds           # (see the module's docstring: the length gate cannot bind)
    n = compared = tightest = stat_hi = 0
    for job, (key, pairs), out in zip(jobs, meta, _run_all(model, jobs)):
        G, R, open_, ext, sg = job[0], job[1], job[7], job[8], job[9]
        assert out.counted() == (0, 0, 0, 0), ("outside its domain", out.first_violation_kind, out.counted(), out.lo, out.hi, out.pad_lo, out.pad_hi, out.stat_hi,
                                               G, R, key, open_, ext, sg, [(len(q), len(r)) for q, r in pairs])
        tightest, stat_hi = max(tightest, out.hi), max(stat_hi, out.stat_hi)
        if n % 4 == 0:
            want = _oracle(orc, sch[key][0], pairs, open_, ext, sg)
            assert [out.fields(0), out.fields(1)] == want, (G, R, key, open_, ext, sg, [(len(q), len(r)) for q, r in pairs], [out.fields(0), out.fields(1)], want)
            compared += 1
        n += 1
    print("stats16p window edge: runs %d, compared with the oracle %d, tightest hi %d, largest statistics half %d" % (n, compared, tightest, stat_hi))
    assert n > 300 and compared > 75, (n, compared)
    assert tightest > 24000, tightest                                # the corners really are close to the top of the window
    assert 1000 < stat_hi < 32768, stat_hi                           # counts in the thousands, far from the int16 edge
