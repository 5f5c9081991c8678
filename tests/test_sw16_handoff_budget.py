"""Static budget of the headline kernel pmx_sw16_kernel<8,19,6> with the fused lane hand-offs (no GPU needed): compiled as
test_sw16_isa_budget.py compiles it.  The sweep loop had 301 VALU instructions per two steps; handing F and H to the next lane
with one DPP VOP2 each saves two instructions per step, so the bound is 301 - 2 * 2 = 297.  The strip-save and bound-exchange
blocks are excluded the same way."""
import re
import subprocess

import pytest

import test_sw16_isa_budget as base

LOOP_VALU_MAX = 297


@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    """(kernel name, its instructions, its metadata lines, static LDS bytes), as test_sw16_isa_budget.py's fixture"""
    out = str(tmp_path_factory.mktemp("isa_handoff") / "pmx_sw16.s")
    subprocess.check_call([base._hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                           base.SRC, "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read().split("\n")
    name = next(l.split(":")[0] for l in text if l.startswith(base.KERNEL) and l.split(":")[0].endswith("record"))
    start = next(i for i, l in enumerate(text) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
    meta = "\n".join(l for l in text if name in l or "amdhsa_group_segment_fixed_size" in l)
    kd = next(i for i, l in enumerate(text) if l.strip().startswith(".amdhsa_kernel " + name))
    group = next(int(l.split()[-1]) for l in text[kd:] if "amdhsa_group_segment_fixed_size" in l)
    return name, text[start:end], meta, group


def _sweep(body):
    loops = {}
    for label, insts in base._blocks(body):
        m = re.search(r"Header=(BB\d+_\d+)", label) or (re.search(r"^\.L(BB\d+_\d+):.*Loop Header", label))
        if m:
            loops.setdefault(m.group(1), []).append(insts)
    return max(loops.values(), key=lambda bl: sum("v_pk_maximum3_f16" in i for b in bl for i in b))


def test_sw16_headline_loop_valu_with_fused_handoffs(kernel_asm):
    _, body, _, _ = kernel_asm
    sweep = _sweep(body)
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


def test_sw16_headline_handoffs_are_dpp_vop2(kernel_asm):
    """two hand-offs per step, each one DPP add / subtract with the group's shift; no plain DPP move of F or H is left"""
    _, body, _, _ = kernel_asm
    flat = [i for b in _sweep(body) for i in b]
    fused = [i for i in flat if re.match(r"v_(add|sub)_u32_dpp .*row_shr:2 row_mask:0xf bank_mask:0xf$", i)]
    assert len(fused) == 4, fused
    assert not [i for i in flat if i.startswith("v_mov_b32_dpp") and "row_shr" in i]
    # a DPP instruction reads no VGPR that one of the two instructions before it wrote: the wait states are in front of it
    for k, i in enumerate(flat):
        if "_dpp" in i and "row_shr" in i:
            assert flat[k - 1] == "s_nop 1", flat[k - 2:k + 1]


def test_sw16_headline_registers_scratch_lds(kernel_asm):
    name, _, meta, group = kernel_asm
    vgpr = int(re.search(re.escape(name) + r"\.num_vgpr, (\d+)", meta).group(1))
    scratch = int(re.search(re.escape(name) + r"\.private_seg_size, (\d+)", meta).group(1))
    assert vgpr <= 128, vgpr                  # 4 waves per SIMD
    assert scratch == 0
    assert group == 0                         # no static LDS
