"""Static size of everything the headline kernel, pmx_sw16_kernel<8,19,6>, runs OUTSIDE its sweep loop (no GPU needed): the
per-wave setup -- tables, dword staging of both sequences, selectors, strip initialisation -- and the epilogue.  Compiles
pmx_sw16.hip for gfx950 to assembly as tests/test_sw16_isa_budget.py does and counts v_* instructions only.

Before the per-wave setup was reworked this compiler gave 1479 VALU instructions outside the loop: a second copy of the step
(the peeled odd last step: 67 v_pk_maximum3_f16) behind 56 moves that re-seated the strips, bytewise staging and a per-row
selector build.  Now: one loop for both parities of the step count, 777 outside it (the query staging is unrolled: five
dwords per pair and lane, so the static count is above what a wave executes in its staging loops)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "parasail-rs_amd", "csrc", "pmx_sw16.hip")
KERNEL = "_Z15pmx_sw16_kernelILi8ELi19ELi6E"
OUTSIDE_VALU_MAX = 815        # 777 reached + 5 %; the bound asked for was <= 900, the parent had 1479
OUTSIDE_MAX3_MAX = 19         # fewer than 20: no copy of the step outside the loop (a step has 67)
MOV_RUN_MAX = 8               # between the loop and the epilogue: nothing re-seats the strips


def _hipcc():
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"), shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


@pytest.fixture(scope="module")
def kernel_blocks(tmp_path_factory):
    """[(label line, instructions)] of the kernel's basic blocks, and the indices of the sweep loop's blocks"""
    out = str(tmp_path_factory.mktemp("isa") / "pmx_sw16.s")
    subprocess.check_call([_hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                           SRC, "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read().split("\n")
    name = next(l.split(":")[0] for l in text if l.startswith(KERNEL) and l.split(":")[0].endswith("record"))
    start = next(i for i, l in enumerate(text) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
    blocks = [("entry", [])]
    cur = blocks[0]
    for l in text[start + 1:end]:
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
            cur = (l, []); blocks.append(cur); continue
        s = l.split(";")[0].strip()
        if s and not s.startswith("."):
            cur[1].append(s)
    loops = {}
    for idx, (label, _) in enumerate(blocks):
        m = re.search(r"Header=(BB\d+_\d+)", label) or re.search(r"^\.L(BB\d+_\d+):.*Loop Header", label)
        if m:
            loops.setdefault(m.group(1), []).append(idx)
    # the sweep: the loop with the most packed max3
    sweep = max(loops.values(), key=lambda bl: sum("v_pk_maximum3_f16" in i for b in bl for i in blocks[b][1]))
    assert sum("v_pk_maximum3_f16" in i for b in sweep for i in blocks[b][1]) >= 2 * (3 * 19 + 10)
    return blocks, set(sweep)


def test_sw16_headline_has_no_peeled_step(kernel_blocks):
    blocks, sweep = kernel_blocks
    outside = sum("v_pk_maximum3_f16" in i for idx, (_, insts) in enumerate(blocks) if idx not in sweep for i in insts)
    print("v_pk_maximum3_f16 outside the sweep loop:", outside)
    assert outside <= OUTSIDE_MAX3_MAX, outside


def test_sw16_headline_no_strip_moves_behind_the_loop(kernel_blocks):
    blocks, sweep = kernel_blocks
    longest = 0
    for idx, (_, insts) in enumerate(blocks):
        if idx <= max(sweep):
            continue                                  # (the strips' initialisation in front of the loop is a run of moves)
        run = 0
        for i in insts:
            run = run + 1 if i.startswith("v_mov_b32") else 0
            longest = max(longest, run)
    print("longest run of v_mov_b32 behind the sweep loop:", longest)
    assert longest <= MOV_RUN_MAX, longest


def test_sw16_headline_setup_valu_budget(kernel_blocks):
    blocks, sweep = kernel_blocks
    outside = sum(i.startswith("v_") for idx, (_, insts) in enumerate(blocks) if idx not in sweep for i in insts)
    print("VALU instructions outside the sweep loop:", outside)
    assert outside <= OUTSIDE_VALU_MAX, outside
