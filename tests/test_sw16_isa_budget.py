"""Static instruction budget of the headline kernel, pmx_sw16_kernel<8,19,6> (no GPU needed): compiles pmx_sw16.hip for
gfx950 to assembly and checks the sweep loop's VALU count per two steps (the strip-save and bound-exchange blocks
excluded), the register budget of 4 waves per SIMD, no scratch, and no static LDS (the perm-table variant reads its score
tables at LDS address 0)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "parasail-rs_amd", "csrc", "pmx_sw16.hip")
KERNEL = "_Z15pmx_sw16_kernelILi8ELi19ELi6E"
LOOP_VALU_MAX = 301          # per two steps; 315 before the perm-table addressing / one-compare improvement test


def _hipcc():
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"), shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "pmx_sw16.s")
    subprocess.check_call([_hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                           SRC, "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read().split("\n")
    name = next(l.split(":")[0] for l in text if l.startswith(KERNEL) and l.split(":")[0].endswith("record"))
    start = next(i for i, l in enumerate(text) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
    meta = "\n".join(l for l in text if name in l or "amdhsa_group_segment_fixed_size" in l)
    kd = next(i for i, l in enumerate(text) if l.strip().startswith(".amdhsa_kernel " + name))
    group = next(int(l.split()[-1]) for l in text[kd:] if "amdhsa_group_segment_fixed_size" in l)
    return name, text[start:end], meta, group


def _blocks(body):
    """(label line, instructions) per basic block"""
    blocks, cur = [], None
    for l in body:
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
            cur = (l, []); blocks.append(cur); continue
        s = l.split(";")[0].strip()
        if cur is not None and s and not s.startswith("."):
            cur[1].append(s)
    return blocks


def test_sw16_headline_loop_valu_budget(kernel_asm):
    _, body, _, _ = kernel_asm
    loops = {}
    for label, insts in _blocks(body):
        m = re.search(r"Header=(BB\d+_\d+)", label) or (re.search(r"^\.L(BB\d+_\d+):.*Loop Header", label))
        if m:
            loops.setdefault(m.group(1), []).append(insts)
    # the sweep: the loop with the most packed max3
    sweep = max(loops.values(), key=lambda bl: sum("v_pk_maximum3_f16" in i for b in bl for i in b))
    counted = 0
    for insts in sweep:
        valu = [i for i in insts if i.startswith("v_")]
        if sum(i.startswith("v_bfi_b32") for i in valu) >= 19:
            continue                                                    # strip save
        if any("row_ror" in i or i.startswith("ds_bpermute") for i in insts):
            continue                                                    # bound exchange
        counted += len(valu)
    assert sum("v_pk_maximum3_f16" in i for b in sweep for i in b) >= 2 * (3 * 19 + 10)
    assert counted <= LOOP_VALU_MAX, counted


def test_sw16_headline_register_budget(kernel_asm):
    name, _, meta, group = kernel_asm
    vgpr = int(re.search(re.escape(name) + r"\.num_vgpr, (\d+)", meta).group(1))
    scratch = int(re.search(re.escape(name) + r"\.private_seg_size, (\d+)", meta).group(1))
    assert vgpr <= 128, vgpr                  # 4 waves per SIMD
    assert scratch == 0
    assert group == 0                         # no static LDS: the dynamic LDS (and the PT score tables) start at 0
