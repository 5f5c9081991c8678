// pmx_pk16.h -- the packed-int16 and DPP lane primitives the fast kernels are built from.  gfx950 only.
//
// The exact window.  Packed kernels keep two int16 values per 32-bit register and take max3 / min3 of them with
// v_pk_maximum3_f16 / v_pk_minimum3_f16, which compare the halves as f16.  Bit patterns in [1024, 31743] are the
// positive normal f16 values, and for those the f16 order is the integer order of the patterns (sign 0, exponent above
// mantissa); 1 .. 1023 are denormals, 31744 = 0x7C00 is +inf and above it lie the NaNs.  So on values that are 0 or
// inside the window both instructions are an exact integer max3 / min3 (exhaustively checked on the chip:
// profiles/microbench/max3_f16_int.hip), and the clamped v_pk_sub_u16 keeps them there: a result that would fall below
// 0 stays 0, the "minus infinity" that loses every max3.  A pattern with the sign bit set (a pad score of -32768) is a
// negative f16 and loses every max3 as well.  Each kernel biases its values into the window, and the host proves before
// the launch that no live value can leave it (or flags the pairs whose best reaches PK16_RERUN_LIMIT for a 32-bit re-run).
#pragma once
#include <hip/hip_runtime.h>

constexpr int PK16_LO = 1024;              // lowest pattern of the exact window
constexpr int PK16_HI = 31743;             // highest pattern of the exact window (31744 = +inf)
constexpr int PK16_SW_BIAS = 2048;         // stored form of a true 0 in the local kernels (pmx_sw16*.hip)
constexpr int PK16_SW_BIAS2 = (PK16_SW_BIAS << 16) | PK16_SW_BIAS;
// a local kernel's best (stored form) at or above this may have left the window (maxs: the matrix's largest score): the
// pair is re-run in 32 bits
#define PK16_RERUN_LIMIT(maxs) (PK16_HI + 1 - ((maxs) > 0 ? (maxs) : 0))

typedef short v2s __attribute__((ext_vector_type(2)));
typedef unsigned short v2us __attribute__((ext_vector_type(2)));
typedef _Float16 v2h __attribute__((ext_vector_type(2)));

#define PK(x)  __builtin_bit_cast(v2s, (int)(x))
#define I32(x) __builtin_bit_cast(int, (x))

// ---- packed int16 arithmetic ----

// integer max3 on patterns in {0} U [PK16_LO, PK16_HI]: fmaximum(fmaximum(a, b), c) on v2f16 selects v_pk_maximum3_f16.
// A builtin rather than inline asm: the hazard recognizer pads every inline-asm result with an s_nop.
__device__ __forceinline__ v2s pk_max3(v2s a, v2s b, v2s c)
{
    const v2h r = __builtin_elementwise_maximum(__builtin_elementwise_maximum(__builtin_bit_cast(v2h, a), __builtin_bit_cast(v2h, b)),
                                                __builtin_bit_cast(v2h, c));
    return __builtin_bit_cast(v2s, r);
}
__device__ __forceinline__ int pk_max3(int a, int b, int c)
{
    const v2h r = __builtin_elementwise_maximum(__builtin_elementwise_maximum(__builtin_bit_cast(v2h, a), __builtin_bit_cast(v2h, b)),
                                                __builtin_bit_cast(v2h, c));
    return __builtin_bit_cast(int, r);
}
// the same instruction as inline asm, s_nop included (pmx_nwsg16_kernel, the first-generation nw / sg kernel)
__device__ __forceinline__ v2s pk_max3_asm(v2s a, v2s b, v2s c)
{
    int r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(I32(a)), "v"(I32(b)), "v"(I32(c)));
    return PK(r);
}

// v_pk_sub_u16 with clamp: saturates at 0
__device__ __forceinline__ v2s pk_subus(v2s a, v2s b)
{
    return __builtin_bit_cast(v2s, __builtin_elementwise_sub_sat(__builtin_bit_cast(v2us, a), __builtin_bit_cast(v2us, b)));
}
__device__ __forceinline__ int pk_subus(int a, int b)
{
    return __builtin_bit_cast(int, __builtin_elementwise_sub_sat(__builtin_bit_cast(v2us, a), __builtin_bit_cast(v2us, b)));
}

// per half: 0xFFFF where a < b, else 0 (values below 32768)
__device__ __forceinline__ int pk_lt(v2s a, v2s b) { const v2s sh = {15, 15}; return I32((a - b) >> sh); }
__device__ __forceinline__ int pk_lt(int a, int b) { return pk_lt(PK(a), PK(b)); }

// (m & a) | (~m & b) with the mask in a VGPR
__device__ __forceinline__ int bfi(int m, int a, int b)
{
    int r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}
// the same with a wave-uniform mask in an SGPR
__device__ __forceinline__ int bfi_sgpr(int m, int a, int b)
{
    int r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "s"(m), "v"(a), "v"(b));
    return r;
}

// ---- unpacked u16 lanes: full-rate VOP2 on the low 16 bits ----

__device__ __forceinline__ unsigned add_u16(unsigned a, unsigned b) { unsigned r; asm("v_add_u16_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ unsigned sub_u16(unsigned a, unsigned b) { unsigned r; asm("v_sub_u16_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ unsigned max_u16(unsigned a, unsigned b) { unsigned r; asm("v_max_u16_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// ---- DPP lane moves inside groups of G lanes (G = 16: DPP row, G = 32 / 64: whole wave) ----

// value of lane - 1 (row_shr:1 / wave_shr:1); a lane without a source (the first of its row or of the wave) gets `old`
// (operands in the order of __builtin_amdgcn_update_dpp).  Group boundaries inside a row or a wave are the caller's.
template <int G>
__device__ __forceinline__ int lane_prev(int old, int x)
{
    if (G <= 16) return __builtin_amdgcn_update_dpp(old, x, 0x111 /*row_shr:1*/, 0xF, 0xF, false);
    return __builtin_amdgcn_update_dpp(old, x, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
}
template <int G>
__device__ __forceinline__ int lane_prev(int x) { return lane_prev<G>(x, x); }

// value of lane - 1 inside a G-lane group; member g == 0 of the group gets `neutral`.
// IL (G == 8 only): two groups share a DPP row of 16 lanes, interleaved (lane = 2 g + (slot & 1) + 16 (slot >> 1)).
// row_shr:2 then moves every group up by one lane, and the row's first two lanes -- lane 0 of both groups --
// have no source and keep `neutral`: no select is needed.
template <int G, bool IL = false>
__device__ __forceinline__ int group_shift_up(int x, int neutral, int g)
{
    if (G == 1) return neutral;
    if (IL) return __builtin_amdgcn_update_dpp(neutral, x, 0x112 /*row_shr:2*/, 0xF, 0xF, false);
    const int r = lane_prev<G>(neutral, x);
    return (G == 16 || G == 64) ? r : (g == 0 ? neutral : r);
}

// The hand-off and the first thing done with it in one DPP VOP2, for the groups whose shift needs no select (interleaved 8,
// 16, 64): member g gets (x of member g - 1) + y resp. - y.  A lane without a source is not written and keeps `keep`, so the
// caller preloads what member 0 shall see.  Same control, row and bank masks as group_shift_up.  A DPP instruction must not
// read a VGPR that one of the two VALU instructions before it wrote; the compiler cannot see into the string, so the two
// wait states are part of it.  They are spent even where the scheduler happens to put independent instructions in front: the
// string cannot know its neighbours, so the wait is conservative by design (measured as a gain with it).
template <int G, bool IL>
constexpr bool group_shift_fusable = IL || G == 16 || G == 64;
#define PMX_DPP_VOP2(OP, CTRL) asm("s_nop 1\n\t" OP "_dpp %0, %1, %2 " CTRL " row_mask:0xf bank_mask:0xf" : "+v"(keep) : "v"(x), "v"(y))
template <int G, bool IL>
__device__ __forceinline__ int group_shift_up_add(int keep, int x, int y)
{
    static_assert(group_shift_fusable<G, IL>, "the other groups need a select behind the move");
    if constexpr (IL) PMX_DPP_VOP2("v_add_u32", "row_shr:2");
    else if constexpr (G == 16) PMX_DPP_VOP2("v_add_u32", "row_shr:1");
    else PMX_DPP_VOP2("v_add_u32", "wave_shr:1");
    return keep;
}
template <int G, bool IL>
__device__ __forceinline__ int group_shift_up_sub(int keep, int x, int y)
{
    static_assert(group_shift_fusable<G, IL>, "the other groups need a select behind the move");
    if constexpr (IL) PMX_DPP_VOP2("v_sub_u32", "row_shr:2");
    else if constexpr (G == 16) PMX_DPP_VOP2("v_sub_u32", "row_shr:1");
    else PMX_DPP_VOP2("v_sub_u32", "wave_shr:1");
    return keep;
}
#undef PMX_DPP_VOP2

// value of lane + 1 (row_shl:1 / wave_shl:1); a lane without a source keeps its own value
template <int G>
__device__ __forceinline__ int lane_next(int x)
{
    if (G <= 16) return __builtin_amdgcn_update_dpp(x, x, 0x101 /*row_shl:1*/, 0xF, 0xF, false);
    return __builtin_amdgcn_update_dpp(x, x, 0x130 /*wave_shl:1*/, 0xF, 0xF, false);
}
// value of lane + 1 over the wave; lane 63 gets 0 (bound_ctrl).  Without an `old` operand the result is not tied to
// the source's register: one v_mov_b32 less per move than lane_next<64>.
__device__ __forceinline__ int lane_next_untied(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x130 /*wave_shl:1*/, 0xF, 0xF, true); }

// x of another lane of the same DPP row, every lane having a source (row rotations, quad permutes, mirrors): no `old`
// operand, so the result is not tied to a register
template <int CTRL>
__device__ __forceinline__ int row_dpp(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true); }

// packed max3 over the G lanes of a group, result in every member (groups as in group_shift_up).  Inside a DPP row of
// 16 the rounds are DPP moves that keep every lane inside its group: row_ror for 16 adjacent lanes or for the
// interleaved 8-lane groups (a rotation by an even count keeps the parity), quad_perm / row_half_mirror for 2, 4 or 8
// adjacent lanes.  Groups wider than a row add one ds_bpermute round per doubling.
template <int G, bool IL = false>
__device__ __forceinline__ int group_max3(int v)
{
    if constexpr (IL || G >= 16) {
        if (!IL) { const int o = row_dpp<0x121 /*row_ror:1*/>(v); v = pk_max3(v, o, o); }
        { const int o = row_dpp<0x122 /*row_ror:2*/>(v); v = pk_max3(v, o, o); }
        { const int o = row_dpp<0x124 /*row_ror:4*/>(v); v = pk_max3(v, o, o); }
        { const int o = row_dpp<0x128 /*row_ror:8*/>(v); v = pk_max3(v, o, o); }
    } else {
        static_assert(G == 1 || G == 2 || G == 4 || G == 8, "adjacent groups inside a row");
        if (G >= 2) { const int o = row_dpp<0xB1 /*quad_perm:[1,0,3,2]*/>(v); v = pk_max3(v, o, o); }
        if (G >= 4) { const int o = row_dpp<0x4E /*quad_perm:[2,3,0,1]*/>(v); v = pk_max3(v, o, o); }
        if (G >= 8) { const int o = row_dpp<0x141 /*row_half_mirror*/>(v); v = pk_max3(v, o, o); }
    }
    if (G >= 32) { const int o = __builtin_amdgcn_ds_bpermute(((int)__lane_id() ^ 16) * 4, v); v = pk_max3(v, o, o); }
    if (G >= 64) { const int o = __builtin_amdgcn_ds_bpermute(((int)__lane_id() ^ 32) * 4, v); v = pk_max3(v, o, o); }
    return v;
}
