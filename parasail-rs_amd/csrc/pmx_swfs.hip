// pmx_swfs.hip -- frameshift-aware local alignment of a codon stream against a protein: the three-frame DP of DESIGN 2.5k
// (semantics: include/parasail_amd.h, "Frameshift-aware translated search").  gfx950 only.
//
// A slot is one codon stream T (N = W - 2 letters, letter i the translation of oriented nucleotides i .. i + 2, written by
// pmx_pairs_gather_codons_kernel) against one protein of m letters:
//
//   D(i,j) = max(0, H(i-3,j-1), H(i-2,j-1) - fs, H(i-4,j-1) - fs)        M = D + s(T[i], r[j])
//   E(i,j) = max(H(i,j-1) - open, E(i,j-1) - ext)                        F(i,j) = max(H(i-3,j) - open, F(i-3,j) - ext)
//   H(i,j) = max(0, M, E, F)
//
// Mapping (pmx_sw16m.hip's): a group of G lanes per slot, R consecutive rows per lane in registers, lane g on column t - g in step t,
// the transposed matrix in LDS, group_shift_up<G> for the lane hand-offs.  What differs is the reach of a cell: three rows up in its
// own column (H and F) and two to four rows up in the column before (H).  So a step hands SEVEN values to the lane below -- the last
// four H and the last three F of the column the lane above has just finished -- and every lane keeps the four H it was handed one
// step earlier: they are the column before, the diagonal's history.  R >= 4 keeps every such source inside one lane.
//
// Strips.  A window of more than G * R rows runs in strips of G * R rows, top to bottom.  The last lane of a strip stores its four
// H and three F per column (two int4) into the slot's boundary scratch, member 0 of the next strip loads them where the first strip
// takes the matrix's edge (H = 0, F = -inf).  Two boundary buffers alternate by strip parity, so a strip never reads the buffer it
// writes; a workgroup barrier with a fence separates the strips (one wave per workgroup).
//
// Arithmetic: 32-bit integers, one slot per lane group.  The largest score, 4 094 rows x 32 767, is below 2^28; penalties are clamped
// to 2^28 by the launcher (a penalty above every score acts as infinity: H >= 0, and a negative E, F or D term never wins), -inf is
// -2^29, so nothing can wrap and width 0 and width 32 are the same exact kernel.
// Plain C++, vector loads and stores only.
#include "pmx_common.h"
#include "pmx_pk16.h"
#include "pmx_fs.h"

#define PMX_SWFS_NEG (-(1 << 29))

// The trace form (TR; semantics: include/parasail_amd.h, "Frameshift traceback") stores one decision byte per cell
// beside the same sweep: bits 0 .. 2 say where H came from -- PMX_FSTR_START / _INFRAME / _SHORT / _LONG: from M, and which term D was;
// PMX_FSTR_F, PMX_FSTR_E; PMX_FSTR_ZERO -- bit 3 that E of the cell was opened, bit 4 that F was (pmx_common.h).  Layout, per slot of
// the launch: column-major, 12 bytes per lane and column -- the lane's R = 10 rows and two bytes of padding, three dword stores --
// so row i of column j is byte ((i / (G R) * max_rlen + j) * G + i % (G R) / R) * 12 + i % R of the slot's region.
template <int G, int R, bool TR>
__global__ __launch_bounds__(64)
void pmx_swfs_kernel(const uint8_t *__restrict__ qbuf, const int64_t *__restrict__ qoff,
                     const uint8_t *__restrict__ rbuf, const int64_t *__restrict__ roff,
                     long long n, int max_rows, int max_rlen,
                     const int16_t *__restrict__ gmat, const uint8_t *__restrict__ gmap, int msize,
                     int open, int ext, int fs,
                     int4 *bnd /* per slot of the launch: 2 buffers x max_rlen columns x 2 int4 */,
                     pmx_record_t *__restrict__ out,
                     uint32_t *__restrict__ trace /* TR: per slot of the launch, trace_stride dwords; else unused */, long long trace_stride)
{
    static_assert(!TR || R == 10, "the trace's 12 bytes per lane and column hold ten rows");
    static_assert(R >= 4, "the rows a cell reaches lie in its own lane or the lane above");
    static_assert(G == 16 || G == 64, "group_shift_up without a select");
    constexpr int NPW = 64 / G;                 // slots per wave = per workgroup
    constexpr int NEG = PMX_SWFS_NEG;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int16_t *matT = reinterpret_cast<int16_t *>(lds);              // matT[r * msize + q] = score(q, r)
    unsigned char *map = lds + (size_t)msize * msize * 2;

    const int lane = threadIdx.x;
    const int g = lane % G, slotw = lane / G;
    for (int i = lane; i < msize * msize; i += 64) matT[i] = gmat[(i % msize) * msize + i / msize];
    for (int i = lane; i < 256; i += 64) map[i] = gmap[i];
    __syncthreads();

    long long slot = (long long)blockIdx.x * NPW + slotw;
    const bool live = slot < n;
    if (!live) slot = n - 1;
    const long long qb = qoff[slot], rb = roff[slot];
    int N = (int)(qoff[slot + 1] - qb), m = (int)(roff[slot + 1] - rb);
    N = min(N, max_rows); m = min(m, max_rlen);                    // (resolve keeps both inside; scratch and loops rely on it)
    const uint8_t *qs = qbuf + qb, *ref = rbuf + rb;
    int4 *bslot = bnd ? bnd + ((size_t)blockIdx.x * NPW + slotw) * 4 * (size_t)max_rlen : nullptr;
    uint32_t *tslot = TR ? trace + ((size_t)blockIdx.x * NPW + slotw) * (size_t)trace_stride : nullptr;

    int wN = N, wm = m;                                            // the wave's longest window and reference: uniform trip counts
#pragma unroll
    for (int d = 32; d >= G; d >>= 1) { wN = max(wN, __shfl_xor(wN, d)); wm = max(wm, __shfl_xor(wm, d)); }
    const int nstrips = (wN + G * R - 1) / (G * R), T_ = wm + G - 1;

    int best = 0, bi = 0, bj = 0;                                   // a zero maximum ends at row 0, column 0
    for (int s = 0; s < nstrips; ++s) {
        const int row0 = s * G * R + g * R;
        int ql[R], vm[R];                                          // the rows' letters; -1 for a row of the stream, 0 for one beyond it
#pragma unroll
        for (int k = 0; k < R; ++k) { vm[k] = row0 + k < N ? -1 : 0; ql[k] = row0 + k < N ? (int)map[qs[row0 + k]] : 0; }
        int Hp[R], E[R], d4[4], oH[4], oF[3];
#pragma unroll
        for (int k = 0; k < R; ++k) { Hp[k] = 0; E[k] = NEG; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { d4[k] = 0; oH[k] = 0; }
#pragma unroll
        for (int k = 0; k < 3; ++k) oF[k] = NEG;
        const int4 *brd = s > 0 ? bslot + (size_t)((s - 1) & 1) * 2 * max_rlen : nullptr;
        int4 *bwr = s + 1 < nstrips ? bslot + (size_t)(s & 1) * 2 * max_rlen : nullptr;

        for (int t = 0; t < T_; ++t) {
            const int col = t - g;
            int uH[4], uF[3];                                      // the lane above: its last four H, last three F of column `col`
#pragma unroll
            for (int k = 0; k < 4; ++k) uH[k] = group_shift_up<G>(oH[k], 0, g);
#pragma unroll
            for (int k = 0; k < 3; ++k) uF[k] = group_shift_up<G>(oF[k], NEG, g);
            const bool valid = col >= 0 && col < m;
            if (valid) {
                if (g == 0 && brd) {                               // member 0 of a later strip: the strip above left the column here
                    const int4 a = brd[2 * col], b = brd[2 * col + 1];
                    uH[0] = a.x; uH[1] = a.y; uH[2] = a.z; uH[3] = a.w;
                    uF[0] = b.x; uF[1] = b.y; uF[2] = b.z;
                }
                const int16_t *mrow = matT + (int)map[ref[col]] * msize;
                int Hc[R], Fc[R];
                int cm = 0;                                        // the column's maximum over the rows of the stream (H >= 0)
                uint32_t tw[3] = {0u, 0u, 0u};                     // TR: the lane's ten decision bytes of this column
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    // column j - 1, rows i - 2, i - 3, i - 4: d4[0 .. 3] are rows -4 .. -1 of this lane, Hp[] rows 0 ..
                    const int hm2 = k >= 2 ? Hp[k - 2] : d4[k + 2];
                    const int hm3 = k >= 3 ? Hp[k - 3] : d4[k + 1];
                    const int hm4 = k >= 4 ? Hp[k - 4] : d4[k];
                    const int D = max(max(0, hm3), max(hm2, hm4) - fs);
                    const int M = D + (int)mrow[ql[k]];
                    const int e = max(Hp[k] - open, E[k] - ext);
                    // column j, row i - 3: uH[1 .. 3] / uF[0 .. 2] are rows -3 .. -1
                    const int h3 = k >= 3 ? Hc[k - 3] : uH[k + 1];
                    const int f3 = k >= 3 ? Fc[k - 3] : uF[k];
                    const int f = max(h3 - open, f3 - ext);
                    const int h = max(max(0, M), max(e, f));
                    if (TR) {                                      // the compares of the contract, on the values at hand
                        const uint32_t ds = D == 0 ? PMX_FSTR_START : hm3 == D ? PMX_FSTR_INFRAME : hm2 - fs == D ? PMX_FSTR_SHORT : PMX_FSTR_LONG;
                        uint32_t c = (M >= e && M >= f) ? ds : f >= e ? PMX_FSTR_F : PMX_FSTR_E;
                        c = h <= 0 ? PMX_FSTR_ZERO : c;
                        c |= (Hp[k] - open > E[k] - ext ? PMX_FSTR_EO : 0u) | (h3 - open > f3 - ext ? PMX_FSTR_FO : 0u);
                        tw[k / 4] |= c << (8 * (k % 4));
                    }
                    Hc[k] = h; Fc[k] = f; E[k] = e;
                    cm = max(cm, h & vm[k]);
                }
                if (TR) {
                    uint32_t *tc = tslot + (((size_t)s * max_rlen + col) * G + g) * 3;
                    tc[0] = tw[0]; tc[1] = tw[1]; tc[2] = tw[2];
                }
                // a new best is rare: one branch per column.  Columns ascend within a strip, so an equal score wins only from a
                // later strip at a smaller column; within the column the first row that holds the maximum.
                if (cm > best || (cm == best && col < bj)) {
                    best = cm; bj = col;
#pragma unroll
                    for (int k = R - 1; k >= 0; --k) if ((Hc[k] & vm[k]) == cm) bi = row0 + k;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) { d4[k] = uH[k]; oH[k] = Hc[R - 4 + k]; }
#pragma unroll
                for (int k = 0; k < 3; ++k) oF[k] = Fc[R - 3 + k];
#pragma unroll
                for (int k = 0; k < R; ++k) Hp[k] = Hc[k];
                if (g == G - 1 && bwr) {
                    bwr[2 * col] = make_int4(oH[0], oH[1], oH[2], oH[3]);
                    bwr[2 * col + 1] = make_int4(oF[0], oF[1], oF[2], 0);
                }
            }
        }
        if (s + 1 < nstrips) { __threadfence_block(); __syncthreads(); }
    }

    // the group's winner: highest score, then lowest column, then lowest row (the first maximum in column-major order)
#pragma unroll
    for (int d = G / 2; d >= 1; d >>= 1) {
        const int os = __shfl_xor(best, d), oj = __shfl_xor(bj, d), oi = __shfl_xor(bi, d);
        if (os > best || (os == best && (oj < bj || (oj == bj && oi < bi)))) { best = os; bj = oj; bi = oi; }
    }
    if (g == 0 && live) {
        pmx_record_t rec;
        rec.score = best; rec.end_query = bi + 2; rec.end_ref = bj; rec.flags = 0;
        out[slot] = rec;
    }
}

// The side's description (pmx_common.h): the launchers are pmx_fs.h's over the two forms of the kernel.
static long long swfs_bound_bytes_per_slot(int max_rlen) { return (long long)sizeof(int4) * 4 * (long long)max_rlen; }
static long long swfs_trace_bytes_per_slot(int max_rows, int max_rlen)
{
    const int strips = (max_rows + PMX_FSTR_STRIP_ROWS - 1) / PMX_FSTR_STRIP_ROWS;
    return (long long)strips * (long long)max_rlen * PMX_FSTR_COL_BYTES;
}
static_assert(PMX_FSTR_COL_BYTES == 16 * 12 && PMX_FSTR_LANE_ROWS == 10 && PMX_FSTR_STRIP_ROWS == 16 * 10, "the walk's addressing (pmx_walkfs.hip)");
const PmxFsSide &pmx_fs_query_side()
{
    static const PmxFsSide side = {
        false, 128, 16 * 10, 10, PMX_FRAMESHIFT_MAX_WINDOW - 2, swfs_bound_bytes_per_slot, swfs_trace_bytes_per_slot,
        pmx_fs_launch<int4, pmx_swfs_kernel<16, 10, false>, false, false>, pmx_fs_launch<int4, pmx_swfs_kernel<16, 10, true>, true, false>,
        {{"pmx_swfs_kernel<16,10>", "pmx_swfs_kernel<16,10>/strips"}, {"pmx_swfs_kernel<16,10,trace>", "pmx_swfs_kernel<16,10,trace>/strips"}}};
    return side;
}
