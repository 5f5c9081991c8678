"""CPU tier: the long-pair sweep is planned as it was before PmxLongPlan described it in one place.

tests/golden/long_plans.json was recorded from the commit before the plan struct, with a throw-away hook of the same signature as
pmx_long_plan_probe appended to that commit's pmx_api.hip: it ran that commit's own decision lines with the knobs as arguments instead
of reading the environment and hipMemGetInfo -- for road 0 the lines of long_batch (time model, switches, rows-per-lane fallback above
4 GiB per pair, refusal, pairs per chunk, then pmx_long_scratch_bytes for that chunk), for road 1 longcig_plan and long_cigar_device's
"two columns for a chunk of at most 16 pairs" with its switches -- and read the steps per boundary chunk off pmx_launch_long's macro
tower (`c16` / `c32`).  Inputs: NW / SG / SW (road 0; road 1 does not look at the mode); n 1, 2, 16, 17, 512; max_qlen at every band
edge of 128-, 256- and 1 024-row bands and beyond; max_rlen around the 64- and 128-column chunks and up to 2 M; the default ceiling,
a forced budget of 1e6 bytes and an unforced one of 4 096 bytes (a pair beyond it is refused on road 0); every switch alone and the
pairs of switches the GPU tests use; on road 1 tile_cols 0 / 64 / 128 / 256 x band_rows 0 / 128 / 256 / 1 024.  (Not the full cross
product: every max_qlen in most contexts, every max_rlen in three of them and two to four elsewhere; the contexts list what was
crossed.)  A context is the eleven inputs but the lengths, then per pair of lengths [max_qlen, max_rlen] where the planner refuses,
else those two and R, columns per step, steps per chunk, nbmax, bstride, pairs per chunk, the bytes in front of
the checkpoints (road 0: pmx_long_scratch_bytes of the chunk, what the launcher laid out and what the road reserves now; it used to
reserve 64 bytes per further pair more), checkpoint bytes, checkpoint slots.  The planner calls no HIP function: the hook runs
without a device."""
import ctypes as C
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_plans.json")
CONTEXT = ["road", "mode", "n", "budget", "budget_forced", "two_columns", "one_column", "rows_per_lane", "chunk_cols", "tile_cols", "band_rows"]
PLANNED = ["max_qlen", "max_rlen", "R", "columns", "steps", "nbmax", "bstride", "pairs", "sweep_bytes", "ck_bytes", "ckslots"]
CEILING = (4 << 30) + (64 << 20)
# rows of the checkpoint road at the default budget and without a switch, on which the public planner is asked too:
# (n, max_qlen, max_rlen, tile_cols, band_rows)
PUBLIC = [(1, 1, 1, 0, 0), (1, 20000, 5000, 0, 0), (2, 257, 128, 0, 0), (16, 1025, 2000000, 0, 0), (17, 513, 5000, 0, 0), (512, 300000, 128, 0, 0),
          (2, 129, 129, 64, 128), (512, 1025, 2000000, 64, 1024), (2, 300000, 2000000, 128, 0), (512, 1, 129, 128, 256), (2, 1025, 129, 256, 1024),
          (512, 300000, 2000000, 256, 128)]


def test_plans_equal_the_recorded_ones(pkg, monkeypatch):
    for name in ("PMX_LONG_CHUNK_BYTES", "PMX_LONG_TWO_COLUMNS", "PMX_LONG_ONE_COLUMN", "PMX_LONG_CHUNK_COLS", "PMX_LONG_ROWS_PER_LANE"):
        monkeypatch.delenv(name, raising=False)
    with open(GOLDEN) as f:
        table = json.load(f)
    assert table["context"] == CONTEXT and table["planned"] == PLANNED
    out = (C.c_longlong * 9)()
    seen, bad, rows, agreed = set(), [], 0, set()
    for ctx in table["contexts"]:
        head, plans = ctx[:len(CONTEXT)], ctx[len(CONTEXT)]
        for want in plans:
            rc = pkg.lib.pmx_long_plan_probe(head[0], head[1], head[2], want[0], want[1], float(head[3]), *head[4:], out)
            assert rc == 0 or (rc == 1 and list(out) == [0] * 9), (head, want, rc, list(out))
            got = want[:2] + (list(out) if rc == 0 else [])
            seen.add((got[2], got[3], got[4], head[0] == 1) if rc == 0 else ())
            rows += 1
            if got != want:
                bad.append((dict(zip(CONTEXT, head)), want, got))
            # the public planner of the checkpoint road reports the same chunk (default budget, no switch)
            key = (head[2], want[0], want[1], head[9], head[10])
            if head[0] == 1 and head[3:9] == [CEILING, 0, 0, 0, 0, 16] and key in PUBLIC:
                opts = pkg.pmx_long_cigar_opts_t(head[9], head[10])
                assert rc == 0 and pkg.lib.pmx_long_cigar_scratch_bytes(head[2], want[0], want[1], C.byref(opts)) == out[6] + out[7], (head, want)
                agreed.add(key)
    assert rows > 2000 and agreed == set(PUBLIC) and len(agreed) == 12
    assert not bad, "%d of %d plans differ; the first: %r" % (len(bad), rows, bad[:3])
    # the table reaches every launchable form, with and without checkpoints, and the refusal
    forms = [(2, 1, 16), (2, 1, 64), (4, 1, 16), (4, 1, 64), (16, 1, 64), (2, 2, 32), (2, 2, 64), (4, 2, 32), (4, 2, 64)]
    assert seen == {()} | {f + (ck,) for f in forms for ck in (False, True)}
