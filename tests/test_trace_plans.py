"""CPU tier: the traceback planners decide what they decided before they were given a plan struct to fill.

tests/golden/trace_plans.json was recorded from the planners as they stood with their `int *variant, int *Tmax, size_t *trace_bytes,
int *G_out, int *R_out` out-parameters (the variant numbers mapped to family, G and R by hand), over: NW / SG / SW; two DNA and two
protein scorings; the refusal corners (max + 2 open = 250 / 251, open < extend, max + open = 255 / 256, msize 8 / 9 where the
matrix-lookup sweeps take over); the query length at every shape's last row and one beyond, per-pair and shared (with and without a
PSSM); reference lengths 1, 1023, 1024, 30000, 30001 and, per context, every length at which the plan changes -- the 160 KiB LDS
test moving it to the next shape, the window proof refusing -- and that length plus one; n = 1, 63, 64, 4096; short_waves and
packed_ok both ways.  (Not the full cross product: a context refused at every reference length is one row, the corners take two
shape edges, n varies at the shapes' last rows.)  A context is the twelve inputs but max_rlen, then per reference length [max_rlen]
where the planner refuses, else [max_rlen, family, G, R, Tmax, trace_bytes].  The planners call no HIP function: the hook
pmx_trace_plan_probe runs them without a device."""
import ctypes as C
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trace_plans.json")
CONTEXT = ["mode", "msize", "score_min", "score_max", "pssm", "open", "ext", "n", "max_qlen", "q_shared", "short_waves", "packed_ok"]
PLANNED = ["max_rlen", "family", "G", "R", "Tmax", "trace_bytes"]


def test_plans_equal_the_recorded_ones(pkg):
    with open(GOLDEN) as f:
        table = json.load(f)
    assert table["context"] == CONTEXT and table["planned"] == PLANNED
    fam, G, R, T, tb = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
    seen, bad, rows = set(), [], 0
    for ctx in table["contexts"]:
        head, plans = ctx[:len(CONTEXT)], ctx[len(CONTEXT)]
        for want in plans:
            args = head[:9] + [want[0]] + head[9:]
            rc = pkg.lib.pmx_trace_plan_probe(*args, fam, G, R, T, tb)
            out = [fam.value, G.value, R.value, T.value, tb.value]
            assert rc == 0 or (rc == 1 and out == [0, 0, 0, 0, 0]), (args, rc, out)
            got = [want[0]] + (out if rc == 0 else [])
            seen.add(tuple(got[1:4]))
            rows += 1
            if got != want:
                bad.append((dict(zip(CONTEXT, head)), want, got))
    assert rows > 3000
    assert not bad, "%d of %d plans differ; the first: %r" % (len(bad), rows, bad[:3])
    # the table reaches every family and every shape a planner can hand out, and the refusal
    shapes = {0: [(32, 8), (64, 8), (64, 16)], 1: [(8, 16), (16, 16), (32, 16), (64, 16)], 2: [(16, 16), (32, 16), (64, 16)],
              3: [(8, 16), (16, 16), (32, 16), (64, 16)], 4: [(16, 16), (32, 16), (64, 16)],
              5: [(16, 10), (16, 16), (16, 19), (16, 20), (32, 10), (32, 16), (64, 16)]}
    assert seen == {()} | {(f, g, r) for f, gr in shapes.items() for g, r in gr}
