// pmx_ungap.hip -- the ungapped diagonal filter behind the seeding entries (semantics: include/parasail_amd.h): the best
// ungapped local score along the seeded diagonals of every candidate, and the selection behind it -- a score threshold and the best
// top_n candidates per query row, compacted in input order.
//
//   pmx_ungapped_kernel        the slots of one chunk (resolved and gathered by the pipeline of pmx_pairs.hip) -> one pmx_ungapped_t each
//   pmx_ungap_keys_kernel      a candidate's sort key (score descending, position ascending; a candidate that does not pass sorts last)
//                              and, without top_n, its keep flag
//   (rocPRIM                   one segmented radix sort over the row segments: rank = place in the sorted row)
//   pmx_ungap_rank_kernel      sorted place -> the keep flag at the candidate's input position
//   (rocPRIM                   one exclusive scan of the flags: the output positions, in input order)
//   pmx_ungap_compact_kernel   the kept candidates' columns to their positions below `capacity`
//   pmx_ungap_rowoff_kernel    the new row offsets and the two counts
//
// The hot kernel.  A candidate is L query letters against span = diag_max - diag_min + 1 diagonals of at most L cells each: tiny, and
// there are millions.  A group of PMX_UNGAP_LANES = 16 lanes takes one candidate (four per wave, the gather's own grouping) and divides
// itself by the span: g = 16, 8, 4, 2, 1 lanes per diagonal for spans of 1, 2, <= 4, <= 8, more, so that 16 / g diagonals are walked at
// once and a span of one -- the common case -- still keeps sixteen lanes busy.  The g lanes of a diagonal cut its cells into g
// contiguous pieces of whole PMX_UNGAP_STEP = 4-cell steps (one dword of each side per step, assembled from aligned dwords), and every
// lane folds its piece into the recurrence's monoid:
//     T total, P best prefix (>= 0), S floored suffix (h behind the piece's last cell), B best h, and the first positions of P and B.
//     A then C:  T = TA + TC,  P = max(PA, TA + PC),  S = max(SA + TC, SC),  B = max(BA, BC, SA + PC);  on ties the lower position.
// Integer arithmetic: the combine is exact however the pieces are cut.  One uniform butterfly of four steps over the group ends the
// candidate: a step below g combines neighbouring pieces in order, a step at or above g keeps the better diagonal (higher B, then the
// lower d).  With g = 1 a lane walks diagonals d, d + 16, ... in ascending order and keeps the first best.  Nothing is atomic and no
// lane waits for another group, so the output does not depend on the launch.
//
// The score table: matrix[mapper[x]][mapper[y]].  A table of at most 32 x 32 letters whose scores fit a byte is staged in LDS as bytes
// at a row stride of 32 beside the 256-byte mapper (1.25 KiB per block); any other square matrix is read from the device matrix's
// int16 table through the vector L1.  Plain C++, vector loads and stores only.
//
// The forms.  FORM says which cells a seed record's diagonals mean; the grouping, the pieces, the fold, the butterfly and
// both table forms are the same code in all of them.
//   PMX_UNGAP_PLAIN        both sides at stride 1, d = j - i, origin r_beg: the DNA, letters and query-frame lists.
//   PMX_UNGAP_CODONS       the query side is a codon stream (pmx_gather_pairs_codons_device) walked at stride 3: cell c is reference
//                          letter c against stream letter 3 c - d, d = D - 3 r_beg a NUCLEOTIDE diagonal.  Cells are counted in codons.
//   PMX_UNGAP_REF_CODONS   the reference side is the stream: cell c is query letter c against stream letter d + 3 c, d = D - lo, lo the
//                          oriented window's start in the whole sequence (strand 1: N - (r_beg + W), N from the set's offsets).
//   PMX_UNGAP_REF_FRAMES   stride 1 against a translated reference window (pmx_gather_pairs_translated_ref_device) whose origin is the
//                          letter lb of sequence frame g = seeds.reserved; a window that is not codon-aligned for g is a bad candidate.
// A strided step's four letters lie at byte distance 3, ten consecutive bytes: they come from the three aligned dwords that hold them
// (four when the first letter is a dword's last byte), never from byte loads, and never from outside the chunk buffer and its slack.
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include "pmx_common.h"
#include <rocprim/rocprim.hpp>

struct PmxUngapPiece { int T, P, S, B, pP, pB; };
#define PMX_UNGAP_NOPOS INT32_MAX           // the position of a P or B that is 0: no cell

static __device__ __forceinline__ void pmx_ungap_cell(PmxUngapPiece &m, int w, int i)
{
    m.T += w;
    if (m.T > m.P) { m.P = m.T; m.pP = i; }
    m.S = max(m.S + w, 0);
    if (m.S > m.B) { m.B = m.S; m.pB = i; }
}
// piece A followed by piece C
static __device__ __forceinline__ PmxUngapPiece pmx_ungap_combine(const PmxUngapPiece &a, const PmxUngapPiece &c)
{
    PmxUngapPiece r;
    r.T = a.T + c.T;
    const int x = a.T + c.P;
    r.P = max(a.P, x); r.pP = x > a.P ? c.pP : a.pP;
    r.S = max(a.S + c.T, c.S);
    const int cross = a.S + c.P;                // h from A's end, at its highest inside C: first reached at C's pP
    const int rb = max(cross, c.B);
    const int rp = cross > c.B ? c.pP : cross < c.B ? c.pB : min(c.pP, c.pB);
    r.B = max(a.B, rb); r.pB = rb > a.B ? rp : a.pB;
    return r;
}
// the four bytes at p from the aligned dwords that hold them; the chunk buffers are 256-byte aligned and end in 16 bytes of slack
static __device__ __forceinline__ uint32_t pmx_ungap_dword(const uint8_t *p)
{
    const uintptr_t sa = (uintptr_t)p & ~(uintptr_t)3;
    const unsigned sh = (unsigned)((uintptr_t)p & 3);
    const uint32_t lo = *reinterpret_cast<const uint32_t *>(sa);
    const uint32_t hi = sh ? *reinterpret_cast<const uint32_t *>(sa + 4) : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
}
// the four bytes at p, p + 3, p + 6 and p + 9, packed like a dword of a stride-1 side: ten bytes, at most p + 12 is touched (the slack)
static __device__ __forceinline__ uint32_t pmx_ungap_dword3(const uint8_t *p)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>((uintptr_t)p & ~(uintptr_t)3);
    const unsigned sh = (unsigned)((uintptr_t)p & 3);
    const uint32_t d0 = w[0], d1 = w[1], d2 = w[2], d3 = sh == 3 ? w[3] : 0u;
    const uint32_t a = __builtin_amdgcn_alignbyte(d1, d0, sh), b = __builtin_amdgcn_alignbyte(d2, d1, sh), c = __builtin_amdgcn_alignbyte(d3, d2, sh);
    return (a & 0xFFu) | ((a >> 24) << 8) | (b & 0x00FF0000u) | ((c << 16) & 0xFF000000u);          // bytes 0, 3, 6, 9
}
static __device__ __forceinline__ long long pmx_ungap_floor3(long long x) { return x >= 0 ? x / 3 : -((2 - x) / 3); }

// Slot k of the chunk: the oriented query window qbuf[qoff[k] .. qoff[k + 1]), the reference window rbuf[roff[k] .. roff[k + 1]), ok[k]
// from the resolve, the candidate's descriptor (for r_beg) and seed record (for the diagonals).  BYTES: the table staged in LDS as
// bytes (msize <= 32, every score in -128 .. 127); else scores[a * msize + b] from global memory.  FORM: see above; the two reference
// forms read the whole sequence's length from the set's offsets r_off, the translated side's W from tw[k] and the slot's byte from
// sflag[k] (the resolve's columns), the plain and the query-stream form read none of the three.
template <bool BYTES, int FORM>
__global__ __launch_bounds__(256)
void pmx_ungapped_kernel(long long n, const uint8_t *__restrict__ qbuf, const int64_t *__restrict__ qoff,
                         const uint8_t *__restrict__ rbuf, const int64_t *__restrict__ roff, const uint8_t *__restrict__ ok,
                         const pmx_pair_t *__restrict__ pairs, const pmx_seed_hit_t *__restrict__ seeds,
                         const int64_t *__restrict__ r_off, const int32_t *__restrict__ tw, const uint8_t *__restrict__ sflag,
                         const int16_t *__restrict__ scores, const uint8_t *__restrict__ mapper, int msize, pmx_ungapped_t *__restrict__ out)
{
    constexpr bool QS = FORM == PMX_UNGAP_CODONS, RS = FORM == PMX_UNGAP_REF_CODONS;       // the strided side: the query's, the reference's
    constexpr int SQ = QS ? 3 : 1, SR = RS ? 3 : 1;
    __shared__ uint8_t map[256];
    __shared__ int8_t tab[BYTES ? 32 * 32 : 4];
    map[threadIdx.x] = mapper[threadIdx.x];
    if (BYTES)
        for (int t = threadIdx.x; t < msize * msize; t += 256) tab[(t / msize) * 32 + t % msize] = (int8_t)scores[t];
    __syncthreads();
    const long long k = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int lane = threadIdx.x & (PMX_UNGAP_LANES - 1);
    const bool live = k < n;                    // (uniform per group; every lane reaches the shuffles)
    bool good = false;
    int L = 0, rlen = 0, r_beg = 0, dmin = 0;
    long long org = 0;                          // the seeds' diagonal of relative diagonal 0: r_beg, 3 r_beg, lo, lb
    long long dlo = 0, dhi = -1;                // the diagonals that can have cells, relative to the windows: SQ b - SR a over buffer letters a, b
    const uint8_t *q = qbuf, *r = rbuf;
    if (live) {
        const pmx_seed_hit_t s = seeds[k];
        dmin = s.diag_min;
        good = ok[k] != 0 && s.diag_min <= s.diag_max;
        if (good) {
            const pmx_pair_t pr = pairs[k];
            r_beg = pr.r_beg;
            if (FORM == PMX_UNGAP_PLAIN) org = r_beg;
            else if (QS) org = 3ll * r_beg;
            else {                              // ok[k]: pr.r is a sequence of the set
                const long long N = r_off[pr.r + 1] - r_off[pr.r], end = (long long)r_beg + tw[k];
                const unsigned f = sflag[k];
                if (RS) org = f ? N - end : r_beg;
                else {
                    const unsigned g = (unsigned)s.reserved, off = g % 3u;
                    const long long lead = f ? N - off - end : (long long)r_beg - off;      // the nucleotides of frame g in front of the window
                    good = (f == 0u || f == 3u) && g < 6u && g / 3u == f / 3u && lead % 3 == 0;
                    org = lead / 3;
                }
            }
        }
        if (good) {
            const long long q0 = qoff[k], r0 = roff[k];
            L = (int)(qoff[k + 1] - q0); rlen = (int)(roff[k + 1] - r0);
            q += q0; r += r0;
            dlo = max((long long)s.diag_min - org, -(long long)SR * (L - 1));
            dhi = min((long long)s.diag_max - org, (long long)SQ * (rlen - 1));
        }
    }
    const long long span = dhi - dlo + 1;       // <= SR L + SQ rlen
    int g = PMX_UNGAP_LANES;                    // lanes per diagonal
    while (g > 1 && PMX_UNGAP_LANES / g < span) g >>= 1;
    const int sub = lane & (g - 1), ndg = PMX_UNGAP_LANES / g;
    PmxUngapPiece best = {0, 0, 0, 0, PMX_UNGAP_NOPOS, PMX_UNGAP_NOPOS};
    int bd = INT32_MAX;                         // the diagonal of `best` (relative)
    for (long long dl = dlo + lane / g; dl <= dhi; dl += ndg) {
        const int d = (int)dl;
        // the diagonal's cells i0 .. i1 - 1, counted on the stride-1 side (a strided form: in codons; it may have none when the stream
        // is shorter than a codon's three frames): cell i is query letter i (QS: 3 i - d) against reference letter i + d (QS: i, RS: d + 3 i)
        int i0, i1;
        if (QS) { i0 = max(0, (int)pmx_ungap_floor3((long long)d + 2)); i1 = min(rlen, (int)pmx_ungap_floor3((long long)L - 1 + d) + 1); }
        else if (RS) { i0 = max(0, (int)pmx_ungap_floor3(2 - (long long)d)); i1 = min(L, (int)pmx_ungap_floor3((long long)rlen - 1 - d) + 1); }
        else { i0 = max(0, -d); i1 = min(L, rlen - d); }                            // cells >= 1 inside [dlo, dhi]
        const int cells = max(i1 - i0, 0);
        const int c = (cells + PMX_UNGAP_STEP * g - 1) / (PMX_UNGAP_STEP * g) * PMX_UNGAP_STEP;
        const int a = i0 + sub * c, b = min(i1, a + c);
        PmxUngapPiece m = {0, 0, 0, 0, PMX_UNGAP_NOPOS, PMX_UNGAP_NOPOS};
        const uint8_t *qp = q + (QS ? 3 * a - d : a), *rp = r + (QS ? a : RS ? d + 3 * a : a + d);
        for (int i = a; i < b; i += PMX_UNGAP_STEP, qp += SQ * PMX_UNGAP_STEP, rp += SR * PMX_UNGAP_STEP) {
            const uint32_t qd = QS ? pmx_ungap_dword3(qp) : pmx_ungap_dword(qp), rd = RS ? pmx_ungap_dword3(rp) : pmx_ungap_dword(rp);
#pragma unroll
            for (int t = 0; t < PMX_UNGAP_STEP; ++t) {
                if (i + t >= b) break;
                const int x = map[(qd >> (8 * t)) & 0xFF], y = map[(rd >> (8 * t)) & 0xFF];
                pmx_ungap_cell(m, BYTES ? (int)tab[x * 32 + y] : (int)scores[x * msize + y], i + t);
            }
        }
        if (g > 1 || m.B > best.B) { best = m; bd = d; }          // g > 1: the lane's only diagonal, its whole piece
    }
    // the group's butterfly: pieces of one diagonal in order below g, the better diagonal from g on
#pragma unroll
    for (int s = 1; s < PMX_UNGAP_LANES; s <<= 1) {
        PmxUngapPiece o;
        o.T = __shfl_xor(best.T, s, PMX_UNGAP_LANES); o.P = __shfl_xor(best.P, s, PMX_UNGAP_LANES); o.S = __shfl_xor(best.S, s, PMX_UNGAP_LANES);
        o.B = __shfl_xor(best.B, s, PMX_UNGAP_LANES); o.pP = __shfl_xor(best.pP, s, PMX_UNGAP_LANES); o.pB = __shfl_xor(best.pB, s, PMX_UNGAP_LANES);
        const int od = __shfl_xor(bd, s, PMX_UNGAP_LANES);
        if (s < g) best = (lane & s) ? pmx_ungap_combine(o, best) : pmx_ungap_combine(best, o);
        else if (o.B > best.B || (o.B == best.B && od < bd)) { best = o; bd = od; }
    }
    if (!live || lane) return;
    int4 w;
    if (!good) w = make_int4(-1, 0, -1, -1);
    else if (best.B <= 0) w = make_int4(0, dmin, -1, -1);
    else if (QS) w = make_int4(best.B, (int)(bd + org), 3 * best.pB - bd + 2, best.pB + r_beg);          // the codon's last nucleotide
    else if (RS) w = make_int4(best.B, (int)(bd + org), best.pB, (int)(org + bd + 3 * best.pB + 2));
    else w = make_int4(best.B, (int)(bd + org), best.pB, (int)(best.pB + bd + org));
    if (((uintptr_t)out & 15) == 0) *reinterpret_cast<int4 *>(out + k) = w;
    else { pmx_ungapped_t u; u.score = w.x; u.diag = w.y; u.end_query = w.z; u.end_ref = w.w; out[k] = u; }
}

int pmx_launch_ungapped(long long n, const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff, const uint8_t *ok,
                        const pmx_pair_t *pairs, const pmx_seed_hit_t *seeds, int form, const int64_t *r_off, const int32_t *tw, const uint8_t *sflag,
                        const PmxDevMatrix &m, pmx_ungapped_t *out, hipStream_t st)
{
    if (m.pssm || m.msize > 255) return 1;
    if (form < PMX_UNGAP_PLAIN || form > PMX_UNGAP_REF_FRAMES) return 1;
    if (form >= PMX_UNGAP_REF_CODONS && (!r_off || !tw || !sflag)) return 1;
    if (n <= 0) return 0;
    const bool bytes = m.msize <= 32 && m.min >= -128 && m.max <= 127;
    using Kernel = decltype(&pmx_ungapped_kernel<false, PMX_UNGAP_PLAIN>);
    static const Kernel kernels[8] = {pmx_ungapped_kernel<false, PMX_UNGAP_PLAIN>, pmx_ungapped_kernel<true, PMX_UNGAP_PLAIN>,
                                 pmx_ungapped_kernel<false, PMX_UNGAP_CODONS>, pmx_ungapped_kernel<true, PMX_UNGAP_CODONS>,
                                 pmx_ungapped_kernel<false, PMX_UNGAP_REF_CODONS>, pmx_ungapped_kernel<true, PMX_UNGAP_REF_CODONS>,
                                 pmx_ungapped_kernel<false, PMX_UNGAP_REF_FRAMES>, pmx_ungapped_kernel<true, PMX_UNGAP_REF_FRAMES>};
    const Kernel kernel = kernels[2 * form + (bytes ? 1 : 0)];
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n * PMX_UNGAP_LANES + 255) / 256)), dim3(256), 0, st, n, qbuf, qoff, rbuf, roff, ok, pairs, seeds,
                       r_off, tw, sflag, m.scores, m.mapper, m.msize, out);
    return pmx_launched();
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------------
// An offset of the caller's row_off, held inside [0, n]: the selection reads device data the entry cannot check, and stays in bounds
// whatever it holds.
static __device__ __host__ __forceinline__ long long pmx_ungap_clamp(int64_t v, long long n) { return v < 0 ? 0 : v > n ? n : (long long)v; }
// segment t of the sort: row t, as [begin, end) with end never below begin (one type for both ends: `end` says which)
struct PmxUngapSeg {
    const int64_t *row_off; long long n; bool end;
    __device__ __host__ unsigned operator()(unsigned t) const
    {
        const long long a = pmx_ungap_clamp(row_off[t], n);
        if (!end) return (unsigned)a;
        const long long z = pmx_ungap_clamp(row_off[t + 1], n);
        return (unsigned)(z > a ? z : a);
    }
};

// key[x] = (2^31 - 1 - score) << 32 | x for a candidate that passes, 0xFFFFFFFF << 32 | x for one that does not: ascending keys are
// score descending, then position ascending, with the rest behind.  sort false (no top_n): flag[x] = passes, and no key.
__global__ __launch_bounds__(256)
void pmx_ungap_keys_kernel(const pmx_ungapped_t *__restrict__ ung, long long n, int min_score, bool sort, uint64_t *__restrict__ keys,
                           uint32_t *__restrict__ flag)
{
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const int sc = ung[x].score;
    const bool pass = sc >= min_score;          // (min_score >= 0: a bad candidate's -1 never passes)
    if (sort) keys[x] = ((uint64_t)(pass ? (uint32_t)(INT32_MAX - sc) : 0xFFFFFFFFu) << 32) | (uint64_t)(uint32_t)x;
    else flag[x] = pass ? 1u : 0u;
}

// Sorted place y lies in the row whose segment holds it: flag[x] = 1 for the candidate x found there when it passes and y is among the
// row's first top_n places.  flag is zeroed before.
__global__ __launch_bounds__(256)
void pmx_ungap_rank_kernel(const uint64_t *__restrict__ sorted, long long n, const int64_t *__restrict__ row_off, long long nq, int top_n,
                           uint32_t *__restrict__ flag)
{
    const long long y = (long long)blockIdx.x * 256 + threadIdx.x;
    if (y >= n) return;
    long long a = 0, z = nq;                    // the last t with row_off[t] <= y (rows that are empty share a start)
    while (a < z) { const long long mid = (a + z + 1) >> 1; if (pmx_ungap_clamp(row_off[mid], n) <= y) a = mid; else z = mid - 1; }
    const long long beg = pmx_ungap_clamp(row_off[a], n);
    if (a >= nq || y < beg) return;             // (behind the last row or in front of the first: a list that is not the rows')
    const uint64_t key = sorted[y];
    const long long x = (long long)(uint32_t)key;
    if ((uint32_t)(key >> 32) != 0xFFFFFFFFu && y - beg < top_n && x < n) flag[x] = 1u;
}

// pos[x + 1] - pos[x] = 1 for a kept candidate: its columns to position pos[x] where that lies below `capacity`.
__global__ __launch_bounds__(256)
void pmx_ungap_compact_kernel(const uint32_t *__restrict__ pos, long long n, long long capacity, const pmx_pair_t *__restrict__ pairs,
                              const uint8_t *__restrict__ byte, const pmx_seed_hit_t *__restrict__ seeds, const pmx_ungapped_t *__restrict__ ung,
                              pmx_pair_t *__restrict__ out_pairs, uint8_t *__restrict__ out_byte, pmx_seed_hit_t *__restrict__ out_seeds,
                              pmx_ungapped_t *__restrict__ out_ung, int64_t *__restrict__ out_source)
{
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= n || pos[x + 1] == pos[x]) return;
    const long long at = pos[x];
    if (at >= capacity) return;
    if (out_pairs) out_pairs[at] = pairs[x];
    if (out_byte) out_byte[at] = byte ? byte[x] : 0;
    if (out_seeds) out_seeds[at] = seeds[x];
    if (out_ung) out_ung[at] = ung[x];
    if (out_source) out_source[at] = x;
}

// out_row_off[t] = the kept candidates in front of row t, t = 0 .. nq (uncapped); counts = [kept, written]
__global__ __launch_bounds__(256)
void pmx_ungap_rowoff_kernel(const uint32_t *__restrict__ pos, long long n, const int64_t *__restrict__ row_off, long long nq, long long capacity,
                             int64_t *__restrict__ out_row_off, int64_t *__restrict__ counts)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t > nq) return;
    out_row_off[t] = (int64_t)pos[pmx_ungap_clamp(row_off[t], n)];
    if (t == 0) { const int64_t kept = (int64_t)pos[n]; counts[0] = kept; counts[1] = kept < capacity ? kept : capacity; }
}

// rocPRIM scratch of the selection: the segmented sort of n keys in nq segments and the scan of n + 1 flags, used one after the other
size_t pmx_ungap_select_temp_bytes(long long n, long long nq)
{
    size_t a = 0, b = 0;
    auto beg = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0u), PmxUngapSeg{nullptr, 0, false});
    auto end = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0u), PmxUngapSeg{nullptr, 0, true});
    (void)rocprim::segmented_radix_sort_keys(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr, (unsigned)n, (unsigned)nq, beg, end, 0, 64, nullptr);
    (void)rocprim::exclusive_scan(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)(n + 1), rocprim::plus<uint32_t>(), nullptr);
    return std::max(a, b) + 256;
}

// The n >= 1 scored candidates of nq >= 1 rows -> the kept ones' columns (each optional), row offsets and counts.  keys_a / keys_b: n keys
// each (unused without top_n); flag: n + 1 entries; min_score >= 0.
int pmx_launch_ungap_select(const pmx_ungapped_t *ung, long long n, const int64_t *row_off, long long nq, int min_score, int top_n,
                            const pmx_pair_t *pairs, const uint8_t *byte, const pmx_seed_hit_t *seeds,
                            uint64_t *keys_a, uint64_t *keys_b, uint32_t *flag, void *temp, size_t temp_bytes,
                            pmx_pair_t *out_pairs, uint8_t *out_byte, pmx_seed_hit_t *out_seeds, pmx_ungapped_t *out_ung, int64_t *out_source,
                            long long capacity, int64_t *out_row_off, int64_t *counts, hipStream_t st)
{
    int rc = 0;
    const unsigned nb = (unsigned)((n + 255) / 256);
    const bool sort = top_n > 0;
    if (hipMemsetAsync(flag, 0, sizeof(uint32_t) * (size_t)(n + 1), st) != hipSuccess) return -1;
    hipLaunchKernelGGL(pmx_ungap_keys_kernel, dim3(nb), dim3(256), 0, st, ung, n, min_score, sort, keys_a, flag);
    if ((rc = pmx_launched())) return rc;
    if (sort) {
        auto beg = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0u), PmxUngapSeg{row_off, n, false});
        auto end = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0u), PmxUngapSeg{row_off, n, true});
        size_t tb = temp_bytes;
        const hipError_t e = rocprim::segmented_radix_sort_keys(temp, tb, (const uint64_t *)keys_a, keys_b, (unsigned)n, (unsigned)nq, beg, end, 0, 64, st);
        if (e != hipSuccess) return -(int)e;
        hipLaunchKernelGGL(pmx_ungap_rank_kernel, dim3(nb), dim3(256), 0, st, (const uint64_t *)keys_b, n, row_off, nq, top_n, flag);
        if ((rc = pmx_launched())) return rc;
    }
    size_t tb = temp_bytes;
    const hipError_t e = rocprim::exclusive_scan(temp, tb, flag, flag, 0u, (size_t)(n + 1), rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return -(int)e;
    if (capacity > 0) {
        hipLaunchKernelGGL(pmx_ungap_compact_kernel, dim3(nb), dim3(256), 0, st, (const uint32_t *)flag, n, capacity, pairs, byte, seeds, ung,
                           out_pairs, out_byte, out_seeds, out_ung, out_source);
        if ((rc = pmx_launched())) return rc;
    }
    hipLaunchKernelGGL(pmx_ungap_rowoff_kernel, dim3((unsigned)((nq + 1 + 255) / 256)), dim3(256), 0, st, (const uint32_t *)flag, n, row_off, nq, capacity,
                       out_row_off, counts);
    return pmx_launched();
}
