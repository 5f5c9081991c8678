// valu_mix.hip -- does the ORDER of a VOP2 / VOP3P mix change its issue rate?  Companion of valu_rate.hip, for the
// sw16 sweep loop (pmx_sw16.hip): per two rows that loop issues 7 v_pk_maximum3_f16, 2 v_perm_b32 (VOP3P / VOP3) and
// 4 v_sub_u32, 2 v_add_u32 (VOP2) -- 3 : 2.  Alone the VOP2 adds issue about 1.7 times as fast as the VOP3 forms.
// Build: hipcc -O3 --offload-arch=gfx950 -o valu_mix valu_mix.hip ; run on the GPU box.
// Prints wave64 VALU instructions per ns per SIMD at 2, 4 and 8 waves per SIMD, three repeats each.
//   a        independent instructions, the finest interleave of the multiset (V2 V3 V3 V2 V3 ...)
//   b<k>     the same multiset, VOP2 in runs of k between proportionally grouped VOP3
//   c        (a) with an s_nop 0 behind every v_pk_maximum3_f16
//   d        the kernel's row as one dependent chain (sub -> max3 -> nop -> sub -> max3 -> nop), 19 rows, alone
//   e        (d) with an independent max3 in each gap instead of the s_nop
//   f_alt    19 dependent perm / add pairs, alternating, in front of (d)
//   f_grp    19 perms, then their 19 adds, in front of (d)
// (a) to (c) are 285 instructions per trip (133 max3, 38 perm, 76 sub, 38 add); (d) is 76, (e) 114, (f) 114.
// (a) to (c) are one inline-asm statement per instruction; the compiler pads one s_nop 0 behind every eighth of them (33 per
// trip, the same in every case).  (d) to (f) are one asm string per trip and contain exactly what is written.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <utility>
#include <vector>

#define ITER 1024

enum { MAX3, PERM, SUB, ADD, NOP };
constexpr int N3 = 171, N2 = 114;

struct Seq { int n; unsigned char kind[512]; };
// VOP2 in runs of k, VOP3 behind each run until the 3 : 2 proportion is restored; nop: s_nop 0 behind every max3
constexpr Seq make_seq(int k, bool nop)
{
    Seq s{};
    int i2 = 0, i3 = 0;
    while (i2 < N2 || i3 < N3) {
        for (int j = 0; j < k && i2 < N2; ++j, ++i2) s.kind[s.n++] = (i2 % 3 == 2) ? ADD : SUB;
        while (i3 < N3 && (i3 * 2 < i2 * 3 || i2 == N2)) {
            const bool perm = i3 % 9 == 3 || i3 % 9 == 7;
            s.kind[s.n++] = perm ? PERM : MAX3;
            if (nop && !perm) s.kind[s.n++] = NOP;
            ++i3;
        }
    }
    return s;
}
constexpr Seq SEQ_A = make_seq(1, false), SEQ_B2 = make_seq(2, false), SEQ_B3 = make_seq(3, false), SEQ_B4 = make_seq(4, false),
              SEQ_B8 = make_seq(8, false), SEQ_B19 = make_seq(19, false), SEQ_C = make_seq(1, true);

template <int OP>
__device__ __forceinline__ void op(int &x, int b, int c)
{
    if constexpr (OP == MAX3) asm volatile("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c));
    if constexpr (OP == PERM) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c));
    if constexpr (OP == SUB) asm volatile("v_sub_u32 %0, %0, %1" : "+v"(x) : "v"(b), "v"(c));
    if constexpr (OP == ADD) asm volatile("v_add_u32 %0, %0, %1" : "+v"(x) : "v"(b), "v"(c));
    if constexpr (OP == NOP) asm volatile("s_nop 0");
}
// VALU instruction i of the trip works on accumulator i % 8: eight independent chains, as in valu_rate.hip
template <const Seq &S, size_t... I>
__device__ __forceinline__ void emit(int (&a)[8], int b, int c, std::index_sequence<I...>)
{
    (op<S.kind[I]>(a[I % 8], b, c), ...);
}

template <const Seq &S>
__global__ __launch_bounds__(64) void k_seq(int *out, int seed)
{
    int a[8];
    for (int i = 0; i < 8; ++i) a[i] = (seed + threadIdx.x) * (2 * i + 1);
    const int b = seed * 31 + 7, c = seed * 17 + 3;
    for (int i = 0; i < ITER; ++i) emit<S>(a, b, c, std::make_index_sequence<S.n>{});
    out[blockIdx.x * 64 + threadIdx.x] = a[0] ^ a[1] ^ a[2] ^ a[3] ^ a[4] ^ a[5] ^ a[6] ^ a[7];
}

#define R19(X) X X X X X X X X X X X X X X X X X X X
// %0 F (carried), %1 H, %2 Fe, %3 X, %4 / %5 constants (T, E, c, Zv of the kernel), %6 / %7 independent accumulators
#define ROW_D "v_sub_u32 %2, %0, %5\n v_pk_maximum3_f16 %1, %4, %5, %2\n s_nop 0\n v_sub_u32 %3, %1, %5\n v_pk_maximum3_f16 %0, %2, %3, %4\n s_nop 0\n"
#define ROW_E "v_sub_u32 %2, %0, %5\n v_pk_maximum3_f16 %1, %4, %5, %2\n v_pk_maximum3_f16 %6, %6, %4, %5\n" \
              "v_sub_u32 %3, %1, %5\n v_pk_maximum3_f16 %0, %2, %3, %4\n v_pk_maximum3_f16 %7, %7, %4, %5\n"
#define T19(X) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26)
#define F_PERM(i) "v_perm_b32 %" #i ", %4, %5, %" #i "\n"
#define F_ADD(i) "v_add_u32 %" #i ", %" #i ", %4\n"
#define F_PAIR(i) F_PERM(i) F_ADD(i)

template <int CASE /* 0 d, 1 e, 2 f_alt, 3 f_grp */>
__global__ __launch_bounds__(64) void k_chain(int *out, int seed)
{
    int f = seed + threadIdx.x, h = 0, fe = 0, x = 0, e0 = f * 3, e1 = f * 5;
    int b = seed * 31 + 7, c = seed * 17 + 3;
    int t[19];
    for (int i = 0; i < 19; ++i) t[i] = f * (2 * i + 7);
#define T_OPS "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]), "+v"(t[8]), "+v"(t[9]), \
              "+v"(t[10]), "+v"(t[11]), "+v"(t[12]), "+v"(t[13]), "+v"(t[14]), "+v"(t[15]), "+v"(t[16]), "+v"(t[17]), "+v"(t[18])
    for (int i = 0; i < ITER; ++i) {
        if constexpr (CASE == 0) asm volatile(R19(ROW_D) : "+v"(f), "+v"(h), "+v"(fe), "+v"(x) : "v"(b), "v"(c));
        if constexpr (CASE == 1) asm volatile(R19(ROW_E) : "+v"(f), "+v"(h), "+v"(fe), "+v"(x), "+v"(b), "+v"(c), "+v"(e0), "+v"(e1));
        if constexpr (CASE == 2) asm volatile(T19(F_PAIR) R19(ROW_D) : "+v"(f), "+v"(h), "+v"(fe), "+v"(x), "+v"(b), "+v"(c), "+v"(e0), "+v"(e1), T_OPS);
        if constexpr (CASE == 3) asm volatile(T19(F_PERM) T19(F_ADD) R19(ROW_D) : "+v"(f), "+v"(h), "+v"(fe), "+v"(x), "+v"(b), "+v"(c), "+v"(e0), "+v"(e1), T_OPS);
    }
    int r = f ^ h ^ fe ^ x ^ e0 ^ e1;
    for (int i = 0; i < 19; ++i) r ^= t[i];
    out[blockIdx.x * 64 + threadIdx.x] = r;
}

typedef void (*kfn)(int *, int);
struct Entry { const char *name; kfn f; int valu; };

int main()
{
    const Entry tests[] = {
        {"a   finest interleave", k_seq<SEQ_A>, N2 + N3}, {"b2  VOP2 runs of 2", k_seq<SEQ_B2>, N2 + N3}, {"b3  VOP2 runs of 3", k_seq<SEQ_B3>, N2 + N3},
        {"b4  VOP2 runs of 4", k_seq<SEQ_B4>, N2 + N3}, {"b8  VOP2 runs of 8", k_seq<SEQ_B8>, N2 + N3}, {"b19 VOP2 runs of 19", k_seq<SEQ_B19>, N2 + N3},
        {"c   (a) + s_nop behind max3", k_seq<SEQ_C>, N2 + N3}, {"d   row chain alone", k_chain<0>, 76}, {"e   row chain, max3 in gaps", k_chain<1>, 114},
        {"f   alternating T + chain", k_chain<2>, 114}, {"f   grouped T + chain", k_chain<3>, 114},
    };
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
    const int cus = prop.multiProcessorCount;
    printf("device %s, %d CUs, clock %d kHz\n", prop.name, cus, prop.clockRate);
    int *out;
    const int maxblocks = cus * 4 * 8;
    if (hipMalloc(&out, sizeof(int) * 64 * maxblocks) != hipSuccess) return 1;
    printf("%-30s %5s %26s %26s %26s   (wave64 VALU / ns / SIMD, three repeats)\n", "case", "VALU", "2 waves/SIMD", "4 waves/SIMD", "8 waves/SIMD");
    for (const Entry &t : tests) {
        printf("%-30s %5d", t.name, t.valu);
        for (int wps : {2, 4, 8}) {
            const int blocks = cus * 4 * wps;
            hipLaunchKernelGGL(t.f, dim3(blocks), dim3(64), 0, 0, out, 1);   // warm
            if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "\nkernel failed\n"); return 1; }
            printf("  ");
            for (int rep = 0; rep < 3; ++rep) {
                hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
                (void)hipEventRecord(e0);
                hipLaunchKernelGGL(t.f, dim3(blocks), dim3(64), 0, 0, out, 2 + rep);
                (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
                float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
                (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
                printf(" %7.4f", (double)ITER * t.valu * wps / (ms * 1e-3 * 1e9));
            }
        }
        printf("\n");
    }
    (void)hipFree(out);
    return 0;
}
