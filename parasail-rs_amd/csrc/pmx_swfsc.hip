// pmx_swfsc.hip -- frameshift-aware local alignment of a protein against a codon stream, "codons on columns": the three-frame DP of
// DESIGN 2.5m (semantics: include/parasail_amd.h, "Frameshift-aware translated search, reference side").  gfx950 only.
//
// A slot is one protein q of m letters (the rows) against one codon stream T of a nucleotide REFERENCE window (the columns: N = W - 2
// letters, letter j the translation of oriented nucleotides j .. j + 2, written by pmx_pairs_gather_codons_kernel<true>):
//
//   D(i,j) = max(0, H(i-1,j-3), H(i-1,j-2) - fs, H(i-1,j-4) - fs)        M = D + s(q[i], T[j])
//   E(i,j) = max(H(i,j-3) - open, E(i,j-3) - ext)                        F(i,j) = max(H(i-1,j) - open, F(i-1,j) - ext)
//   H(i,j) = max(0, M, E, F)
//
// It is pmx_swfs.hip's recurrence transposed, and the transposition moves the reach of a cell from the rows into the columns: one row
// up, and two to four columns back.  Mapping: a group of G lanes per slot, R consecutive rows per lane in registers, lane g on column
// t - g in step t, the transposed matrix in LDS (one stream letter selects the LDS row per step), group_shift_up<G> for the hand-off.
//   - A step hands TWO values to the lane below: H and F of the lane's last row in the column it has just finished (pmx_swfs: seven).
//   - The columns a cell reaches back to live in the lane: a ring of the last four columns' H (j - 1 .. j - 4) and a ring of E, R
//     values each.  Both rings are indexed by the step t & 3 -- every lane advances one column per step, so the step number and the
//     lane's column differ by a constant -- and the column loop is unrolled by four, which makes every ring index static: the rings
//     are registers and nothing is moved.  E of column j is read once, at column j + 3, and its slot is rewritten at column j + 4, so
//     three of the four E slots are live at a time.  A lane whose column is still negative does not write its rings: they keep the
//     matrix's edge (H = 0, E = -inf) for the columns that do not exist.
//   - The lane keeps the last four H it was handed in a ring of the same kind: the history of the row above its first row.
//
// Strips.  A query of more than G * R rows runs in strips of G * R rows, top to bottom.  The last lane of a strip stores (H, F) of its
// last row per column (one int2, 8 bytes) into the slot's boundary scratch, member 0 of the next strip loads the pair where the first
// strip takes the matrix's edge (H = 0, F = -inf) and keeps its own history of them.  Two boundary buffers alternate by strip parity,
// so a strip never reads the buffer it writes; a workgroup barrier with a fence separates the strips (one wave per workgroup).
// The stream has no cap: its length only sets the trip count and the boundary buffers' size.
//
// Arithmetic: 32-bit integers, one slot per lane group.  The largest score, 4 096 rows x 32 767, is below 2^28 however long the
// stream; penalties are clamped to 2^28 by the launcher (a penalty above every score acts as infinity: H >= 0, and a negative E, F or
// D term never wins), -inf is -2^29, so nothing can wrap and width 0 and width 32 are the same exact kernel.
// Plain C++, vector loads and stores only.
#include "pmx_common.h"
#include "pmx_pk16.h"
#include "pmx_fs.h"

#define PMX_SWFSC_NEG (-(1 << 29))

// The trace form (TR; semantics: include/parasail_amd.h, "Frameshift traceback, reference side") stores one decision byte
// per cell beside the same sweep, in PMX_FSTR_*'s encoding (pmx_common.h): bits 0 .. 2 where H came from -- START / INFRAME / SHORT /
// LONG: from M, and which term D was; F; E; ZERO -- bit 3 that E of the cell was opened, bit 4 that F was.  Layout, per slot of the
// launch: BY STEP, not by column.  In step t the group's lane g finishes its R = 10 rows of column t - g, so the 16 lanes' 12-byte
// pieces (ten decisions, two bytes of padding, three dword stores) of one step are 192 contiguous bytes: row i of column j is byte
// PMX_FSTRC_CELL(i, j, max_cols) = ((strip * (max_cols + G - 1) + j + lane) * G + lane) * 12 + i % R with strip = i / (G R) and
// lane = i % (G R) / R.  A step of a strip is j + lane <= max_cols - 1 + G - 1: inside the strip's max_cols + G - 1 steps.
template <int G, int R, bool TR>
__global__ __launch_bounds__(64)
void pmx_swfsc_kernel(const uint8_t *__restrict__ qbuf, const int64_t *__restrict__ qoff,
                      const uint8_t *__restrict__ rbuf, const int64_t *__restrict__ roff,
                      long long n, int max_qlen, int max_cols,
                      const int16_t *__restrict__ gmat, const uint8_t *__restrict__ gmap, int msize,
                      int open, int ext, int fs,
                      int2 *bnd /* per slot of the launch: 2 buffers x max_cols columns */,
                      pmx_record_t *__restrict__ out,
                      uint32_t *__restrict__ trace /* TR: per slot of the launch, trace_stride dwords; else unused */, long long trace_stride)
{
    static_assert(!TR || (R == PMX_FSTR_LANE_ROWS && G * R == PMX_FSTR_STRIP_ROWS), "the trace's 12 bytes per lane and step hold ten rows");
    static_assert(G == 16 || G == 64, "group_shift_up without a select");
    constexpr int NPW = 64 / G;                 // slots per wave = per workgroup
    constexpr int NEG = PMX_SWFSC_NEG;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int16_t *matT = reinterpret_cast<int16_t *>(lds);              // matT[t * msize + q] = score(q, t): the row of a stream letter
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
    int m = (int)(qoff[slot + 1] - qb), N = (int)(roff[slot + 1] - rb);
    m = min(m, max_qlen); N = min(N, max_cols);                    // (resolve keeps both inside; scratch and loops rely on it)
    const uint8_t *qs = qbuf + qb, *ts = rbuf + rb;
    int2 *bslot = bnd ? bnd + ((size_t)blockIdx.x * NPW + slotw) * 2 * (size_t)max_cols : nullptr;
    uint32_t *tslot = TR ? trace + ((size_t)blockIdx.x * NPW + slotw) * (size_t)trace_stride : nullptr;

    int wm = m, wN = N;                                            // the wave's longest query and stream: uniform trip counts
#pragma unroll
    for (int d = 32; d >= G; d >>= 1) { wm = max(wm, __shfl_xor(wm, d)); wN = max(wN, __shfl_xor(wN, d)); }
    const int nstrips = (wm + G * R - 1) / (G * R), T_ = wN + G - 1;

    int best = 0, bi = 0, bj = 0;                                   // a zero maximum ends at row 0, column 0
    for (int s = 0; s < nstrips; ++s) {
        const int row0 = s * G * R + g * R;
        int ql[R], vm[R];                                          // the rows' letters; -1 for a row of the query, 0 for one beyond it
#pragma unroll
        for (int k = 0; k < R; ++k) { vm[k] = row0 + k < m ? -1 : 0; ql[k] = row0 + k < m ? (int)map[qs[row0 + k]] : 0; }
        int Hh[4][R], Eh[4][R], top[4];                            // rings by t & 3: the lane's last four columns, the row above them
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            top[p] = 0;
#pragma unroll
            for (int k = 0; k < R; ++k) { Hh[p][k] = 0; Eh[p][k] = NEG; }
        }
        int oH = 0, oF = NEG;                                      // H and F of the lane's last row in the column it finished last
        const int2 *brd = s > 0 ? bslot + (size_t)((s - 1) & 1) * max_cols : nullptr;
        int2 *bwr = s + 1 < nstrips ? bslot + (size_t)(s & 1) * max_cols : nullptr;

        for (int t0 = 0; t0 < T_; t0 += 4) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {                          // t & 3 == p: slot p holds column j - 4 and receives column j,
                const int p3 = (p + 1) & 3, p2 = (p + 2) & 3;      // slots p3 and p2 hold columns j - 3 and j - 2
                const int col = t0 + p - g;
                int uH = group_shift_up<G>(oH, 0, g), uF = group_shift_up<G>(oF, NEG, g);   // the lane above, column `col`
                const bool valid = col >= 0 && col < N;            // (t >= T_ of the last round: col >= wN, no lane is valid)
                if (valid) {
                    if (g == 0 && brd) { const int2 a = brd[col]; uH = a.x; uF = a.y; }   // the strip above left the column here
                    const int16_t *mrow = matT + (int)map[ts[col]] * msize;
                    int a4 = top[p], a3 = top[p3], a2 = top[p2];   // row i - 1 in columns j - 4, j - 3, j - 2
                    int hu = uH, fu = uF;                          // row i - 1 in column j
                    top[p] = uH;
                    int cm = 0;                                    // the column's maximum over the rows of the query (H >= 0)
                    uint32_t tw[3] = {0u, 0u, 0u};                 // TR: the lane's ten decision bytes of this column
#pragma unroll
                    for (int k = 0; k < R; ++k) {
                        const int o4 = Hh[p][k], o3 = Hh[p3][k], o2 = Hh[p2][k];
                        const int D = max(max(0, a3), max(a2, a4) - fs);
                        const int M = D + (int)mrow[ql[k]];
                        const int e = max(o3 - open, Eh[p3][k] - ext);
                        const int f = max(hu - open, fu - ext);
                        const int h = max(max(0, M), max(e, f));
                        if (TR) {                                  // the compares of the contract, on the values at hand
                            const uint32_t ds = D == 0 ? PMX_FSTR_START : a3 == D ? PMX_FSTR_INFRAME : a2 - fs == D ? PMX_FSTR_SHORT : PMX_FSTR_LONG;
                            uint32_t c = (M >= e && M >= f) ? ds : f >= e ? PMX_FSTR_F : PMX_FSTR_E;
                            c = h <= 0 ? PMX_FSTR_ZERO : c;
                            c |= (o3 - open > Eh[p3][k] - ext ? PMX_FSTR_EO : 0u) | (hu - open > fu - ext ? PMX_FSTR_FO : 0u);
                            tw[k / 4] |= c << (8 * (k % 4));
                        }
                        Hh[p][k] = h; Eh[p][k] = e;
                        cm = max(cm, h & vm[k]);
                        a4 = o4; a3 = o3; a2 = o2; hu = h; fu = f;
                    }
                    if (TR) {                                      // step t0 + p = col + g of strip s: the group's 192 contiguous bytes
                        uint32_t *tc = tslot + (((size_t)s * (size_t)(max_cols + G - 1) + (size_t)(col + g)) * G + g) * 3;
                        tc[0] = tw[0]; tc[1] = tw[1]; tc[2] = tw[2];
                    }
                    // a new best is rare: one branch per column.  Columns ascend within a strip, so an equal score wins only from a
                    // later strip at a smaller column; within the column the first row that holds the maximum.
                    if (cm > best || (cm == best && col < bj)) {
                        best = cm; bj = col;
#pragma unroll
                        for (int k = R - 1; k >= 0; --k) if ((Hh[p][k] & vm[k]) == cm) bi = row0 + k;
                    }
                    oH = hu; oF = fu;
                    if (g == G - 1 && bwr) bwr[col] = make_int2(oH, oF);
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
        rec.score = best; rec.end_query = bi; rec.end_ref = bj + 2; rec.flags = 0;
        out[slot] = rec;
    }
}

#define PMX_SWFSC_G 16
#define PMX_SWFSC_R 10
extern "C" int pmx_swfsc_max_msize() { return 128; }
extern "C" int pmx_swfsc_lane_rows() { return PMX_SWFSC_R; }
extern "C" int pmx_swfsc_strip_rows() { return PMX_SWFSC_G * PMX_SWFSC_R; }
extern "C" long long pmx_swfsc_bound_bytes_per_slot(int max_rlen) { return (long long)sizeof(int2) * 2 * (long long)max_rlen; }
extern "C" long long pmx_swfsc_trace_bytes_per_slot(int max_qlen, int max_rlen)
{
    const int strips = (max_qlen + pmx_swfsc_strip_rows() - 1) / pmx_swfsc_strip_rows();
    return (long long)strips * ((long long)max_rlen + PMX_SWFSC_G - 1) * PMX_FSTR_COL_BYTES;
}

// The side's description (pmx_common.h): the exported hooks' values, and the launchers are pmx_fs.h's over the two forms of the kernel.
static_assert(PMX_FSTR_COL_BYTES == PMX_SWFSC_G * 12 && PMX_FSTR_LANE_ROWS == PMX_SWFSC_R && PMX_FSTR_STRIP_ROWS == PMX_SWFSC_G * PMX_SWFSC_R &&
              PMX_FSTRC_SKEW == PMX_SWFSC_G - 1, "the walk's addressing (PMX_FSTRC_CELL, pmx_walkfs.hip)");
const PmxFsSide &pmx_fs_ref_side()
{
    static const PmxFsSide side = {
        true, 128, PMX_SWFSC_G * PMX_SWFSC_R, PMX_SWFSC_R, PMX_FRAMESHIFT_REF_MAX_QUERY, pmx_swfsc_bound_bytes_per_slot, pmx_swfsc_trace_bytes_per_slot,
        pmx_fs_launch<int2, pmx_swfsc_kernel<PMX_SWFSC_G, PMX_SWFSC_R, false>, false, true>,
        pmx_fs_launch<int2, pmx_swfsc_kernel<PMX_SWFSC_G, PMX_SWFSC_R, true>, true, true>,
        {{"pmx_swfsc_kernel<16,10>", "pmx_swfsc_kernel<16,10>/strips"}, {"pmx_swfsc_kernel<16,10,trace>", "pmx_swfsc_kernel<16,10,trace>/strips"}}};
    return side;
}
