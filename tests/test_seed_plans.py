"""CPU tier: a seeding run is planned as it was before PmxSeedPlan described it in one place.

tests/golden/seed_plans.json was recorded from the commit before the plan struct, with a throw-away hook of the same signature as
pmx_seed_plan_probe appended to that commit's pmx_api.hip: it ran that commit's own lines with the match budget as an argument instead
of the thread's test setting -- seed_check's budget rule (the refusal), seed_mode_of for orients and first, the sizing lines of seed_run
(rows per slice, cap_m, positions, slots, key_bits, bytes per position slot) and the `slots` / `stride` lines of the three cluster
launchers (segments per row, position slots per segment and per row).  Inputs: all 18 modes -- DNA strand 0, 1, 2; letters -1, 0 .. 5,
6 .. 8, 9 .. 11; reference 0, 1 -- crossed with max_qlen 1, 2, 150, 151, 10 000, 2^20 and nq 1, 2, 1 000, 10^6 at the default knobs
(max_occ 64, slice_rows 0, the default budget, 1 000 reference sequences); then each knob alone against six of those rows -- max_occ 1
and 65 535, slice_rows 1 and 7, a budget of 4 096 bytes and of 2^34 -- the reference count 1, 2, 3, 2^29, 2^31 - 1 (the key_bits edges,
times six for a translated index) against two rows, and slice_rows x budget together.  A context is the six knobs, then per (nq,
max_qlen) those two alone where one row's worst case does not fit the budget, else those two and the eleven numbers of the probe.
`first` is -1 where the rows are read as they stand on a letters or translated index (the plan's rows_translated is false), as the
recorded commit had it.  The planner calls no HIP function: the hook runs without a device."""
import ctypes as C
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seed_plans.json")
CONTEXT = ["kind", "mode", "max_occ", "slice_rows", "budget", "ref_count"]
PLANNED = ["nq", "max_qlen", "orients", "first", "segs", "seg_slots", "row_slots", "pos_bytes", "slice_rows", "cap_m", "positions", "slots", "key_bits"]
MODES = [(0, 0), (0, 1), (0, 2)] + [(1, m) for m in range(-1, 12)] + [(2, 0), (2, 1)]


def test_plans_equal_the_recorded_ones(pkg):
    with open(GOLDEN) as f:
        table = json.load(f)
    assert table["context"] == CONTEXT and table["planned"] == PLANNED
    out = (C.c_longlong * 11)()
    seen, modes, bad, rows = set(), set(), [], 0
    for ctx in table["contexts"]:
        head, plans = ctx[:len(CONTEXT)], ctx[len(CONTEXT)]
        kind, mode, max_occ, slice_rows, budget, ref_count = head
        modes.add((kind, mode))
        for want in plans:
            rc = pkg.lib.pmx_seed_plan_probe(kind, mode, want[0], want[1], max_occ, slice_rows, budget, ref_count, out)
            assert rc == 0 or (rc == 1 and list(out) == [0] * 11), (head, want, rc, list(out))
            got = want[:2] + (list(out) if rc == 0 else [])
            # a geometry: the index kind, segments of one or three frames, rows as they stand or oriented, the reference mode
            seen.add((kind, got[5] // got[1], got[3] >= 0, mode if kind == 2 else 0) if rc == 0 else ())
            rows += 1
            if got != want:
                bad.append((dict(zip(CONTEXT, head)), want, got))
    assert rows > 1500 and modes == set(MODES)
    assert not bad, "%d of %d plans differ; the first: %r" % (len(bad), rows, bad[:3])
    # the table reaches the refusal and every geometry: DNA, letter frames (translated rows and protein rows), letter codons,
    # reference frames, reference codons
    assert seen == {(), (0, 1, True, 0), (1, 1, True, 0), (1, 1, False, 0), (1, 3, True, 0), (2, 1, False, 0), (2, 1, False, 1)}


def test_probe_refuses_what_no_entry_would_plan(pkg):
    out = (C.c_longlong * 11)()
    for args in ((3, 0, 1, 1, 64, 0, 0, 1), (-1, 0, 1, 1, 64, 0, 0, 1), (0, 0, 0, 1, 64, 0, 0, 1), (0, 0, 1, 0, 64, 0, 0, 1), (0, 0, 1, 1, 0, 0, 0, 1),
                 (0, 0, 1, 1, 64, -1, 0, 1)):
        assert pkg.lib.pmx_seed_plan_probe(*args, out) == -1
