// pmx_select.hip -- hit selection over the records of a database search, and the gather of the selected references.  gfx950 only.
//
// Selection (pmx_select_hits_device, the search entries): P = { k : score_k >= min_score }; with max_hits > 0 and |P| > max_hits the
// max_hits members of P that come first under (score descending, index ascending).  Everything is decided on the device, nothing
// depends on the order in which workgroups finish:
//   pmx_select_hist_kernel / pmx_select_pick_kernel   radix select of the K-th score T over the biased scores (score ^ 0x80000000),
//                                                     digits of 11, 11 and 10 bits from the top: an LDS histogram per block, one
//                                                     global integer atomic per non-empty bin; a one-block kernel picks the digit that
//                                                     holds rank K and narrows the prefix.  The first histogram also counts |P|; when
//                                                     nothing has to be cut the later passes return at once.
//   pmx_select_count_kernel / pmx_select_scan_kernel  per block of 2048 records the number above T and the number equal to T, and
//                                                     their exclusive scan over the blocks.
//   pmx_select_scatter_kernel                         record k goes to position (above T before k) + min(equal to T before k, E), E =
//                                                     K - (number above T): ascending index, the first E members of the tie run.
//   by score: a stable descending rocPRIM radix sort of the selected (score, index) pairs, then pmx_select_take_kernel.
// Gather: pmx_select_hitlen_kernel (diagonal and length of every hit), an exclusive scan of the lengths (pmx_launch_text_offsets),
// pmx_gather_refs_kernel (one wave per hit, destination dwords aligned, each assembled from two source dwords with a byte funnel
// shift; never a byte outside [rbuf, rbuf + roff[n]) is read).
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include "pmx_common.h"
#include <rocprim/rocprim.hpp>

#define SEL_TILE 2048            // records per block of the count / scatter kernels (256 threads x 8)
#define SEL_BINS 2048

struct PmxSelState {
    unsigned long long krem;     // rank still to find inside the current prefix
    unsigned long long n_pass;   // |P|
    unsigned long long gt;       // members of P above T
    unsigned long long eq_take;  // E: members of the tie run at T that are kept
    unsigned long long h;        // number selected
    uint32_t prefix, mask, cut, Tu;
};

static __device__ __forceinline__ uint32_t sel_key(const pmx_record_t *recs, long long k) { return (uint32_t)recs[k].score ^ 0x80000000u; }

__global__ __launch_bounds__(256)
void pmx_select_hist_kernel(const pmx_record_t *__restrict__ recs, long long n, uint32_t min_u, const PmxSelState *__restrict__ state,
                            unsigned long long *__restrict__ hist, int shift, int bits, int first)
{
    __shared__ unsigned s_hist[SEL_BINS];
    uint32_t prefix = 0, mask = 0;
    if (!first) {
        if (!state->cut) return;
        prefix = state->prefix; mask = state->mask;
    }
    for (int x = threadIdx.x; x < SEL_BINS; x += 256) s_hist[x] = 0;
    __syncthreads();
    const uint32_t dmask = (1u << bits) - 1u;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long long)gridDim.x * 256) {
        const uint32_t u = sel_key(recs, k);
        if (u >= min_u && (u & mask) == prefix) atomicAdd(&s_hist[(u >> shift) & dmask], 1u);
    }
    __syncthreads();
    for (int x = threadIdx.x; x < SEL_BINS; x += 256)
        if (s_hist[x]) atomicAdd(&hist[x], (unsigned long long)s_hist[x]);
}

// One block.  Reads the histogram of the pass, narrows the prefix by the digit that holds rank krem, and clears the histogram.
__global__ __launch_bounds__(256)
void pmx_select_pick_kernel(PmxSelState *__restrict__ state, unsigned long long *__restrict__ hist, int shift, int bits, int first,
                            long long max_hits)
{
    __shared__ unsigned long long s_hist[SEL_BINS];
    const int nb = 1 << bits;
    for (int x = threadIdx.x; x < SEL_BINS; x += 256) { s_hist[x] = hist[x]; hist[x] = 0; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    PmxSelState s = *state;
    if (first) {
        unsigned long long tot = 0;
        for (int d = 0; d < nb; ++d) tot += s_hist[d];
        s.n_pass = tot; s.gt = 0; s.eq_take = 0; s.prefix = 0; s.mask = 0; s.Tu = 0;
        s.cut = max_hits > 0 && tot > (unsigned long long)max_hits;
        s.krem = (unsigned long long)max_hits;
        s.h = s.cut ? (unsigned long long)max_hits : tot;
    }
    if (s.cut) {
        unsigned long long acc = 0; int d = nb - 1;
        for (; d > 0; --d) {
            if (acc + s_hist[d] >= s.krem) break;
            acc += s_hist[d];
        }
        s.gt += acc; s.krem -= acc;
        s.prefix |= (uint32_t)d << shift; s.mask |= ((1u << bits) - 1u) << shift;
        if (shift == 0) { s.Tu = s.prefix; s.eq_take = s.krem; }
    }
    *state = s;
}

// above: the record is selected whatever the ties do; equal: it belongs to the tie run at T
static __device__ __forceinline__ void sel_classify(uint32_t u, uint32_t min_u, uint32_t cut, uint32_t Tu, bool live, bool *above, bool *equal)
{
    *above = live && (cut ? u > Tu : u >= min_u);
    *equal = live && cut && u == Tu;
}

__global__ __launch_bounds__(256)
void pmx_select_count_kernel(const pmx_record_t *__restrict__ recs, long long n, uint32_t min_u, const PmxSelState *__restrict__ state,
                             unsigned long long *__restrict__ blk_gt, unsigned long long *__restrict__ blk_eq)
{
    __shared__ unsigned s_gt[4], s_eq[4];
    const uint32_t cut = state->cut, Tu = state->Tu;
    const long long base = (long long)blockIdx.x * SEL_TILE;
    unsigned g = 0, e = 0;
    for (int it = 0; it < SEL_TILE / 256; ++it) {
        const long long k = base + it * 256 + threadIdx.x;
        const bool live = k < n;
        bool a, q;
        sel_classify(live ? sel_key(recs, k) : 0u, min_u, cut, Tu, live, &a, &q);
        g += (unsigned)__popcll(__ballot(a)); e += (unsigned)__popcll(__ballot(q));
    }
    if ((threadIdx.x & 63) == 0) { s_gt[threadIdx.x >> 6] = g; s_eq[threadIdx.x >> 6] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_gt[blockIdx.x] = (unsigned long long)s_gt[0] + s_gt[1] + s_gt[2] + s_gt[3];
        blk_eq[blockIdx.x] = (unsigned long long)s_eq[0] + s_eq[1] + s_eq[2] + s_eq[3];
    }
}

// One block: exclusive scan of both block-count arrays in place, and the two public counts.
__global__ __launch_bounds__(256)
void pmx_select_scan_kernel(unsigned long long *__restrict__ blk_gt, unsigned long long *__restrict__ blk_eq, long long nb,
                            const PmxSelState *__restrict__ state, int64_t *__restrict__ counts)
{
    __shared__ unsigned long long s_g[256], s_e[256];
    const long long per = (nb + 255) / 256, a = per * threadIdx.x, b = a + per < nb ? a + per : nb;
    unsigned long long g = 0, e = 0;
    for (long long x = a; x < b; ++x) { g += blk_gt[x]; e += blk_eq[x]; }
    s_g[threadIdx.x] = g; s_e[threadIdx.x] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long rg = 0, re = 0;
        for (int t = 0; t < 256; ++t) {
            const unsigned long long tg = s_g[t], te = s_e[t];
            s_g[t] = rg; s_e[t] = re; rg += tg; re += te;
        }
        if (counts) { counts[0] = (int64_t)state->h; counts[1] = (int64_t)state->n_pass; }
    }
    __syncthreads();
    g = s_g[threadIdx.x]; e = s_e[threadIdx.x];
    for (long long x = a; x < b; ++x) {
        const unsigned long long tg = blk_gt[x], te = blk_eq[x];
        blk_gt[x] = g; blk_eq[x] = e; g += tg; e += te;
    }
}

__global__ __launch_bounds__(256)
void pmx_select_scatter_kernel(const pmx_record_t *__restrict__ recs, long long n, uint32_t min_u, const PmxSelState *__restrict__ state,
                               const unsigned long long *__restrict__ blk_gt, const unsigned long long *__restrict__ blk_eq,
                               int64_t *__restrict__ out_idx, uint32_t *__restrict__ out_key, long long limit)
{
    __shared__ unsigned s_gt[4], s_eq[4];
    const uint32_t cut = state->cut, Tu = state->Tu;
    const unsigned long long E = state->eq_take;
    const long long base = (long long)blockIdx.x * SEL_TILE;
    unsigned long long g0 = blk_gt[blockIdx.x], e0 = blk_eq[blockIdx.x];        // above / equal before this step's first record
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int it = 0; it < SEL_TILE / 256; ++it) {
        const long long k = base + it * 256 + threadIdx.x;
        const bool live = k < n;
        const uint32_t u = live ? sel_key(recs, k) : 0u;
        bool a, q;
        sel_classify(u, min_u, cut, Tu, live, &a, &q);
        const unsigned long long ba = __ballot(a), bq = __ballot(q);
        if (lane == 0) { s_gt[w] = (unsigned)__popcll(ba); s_eq[w] = (unsigned)__popcll(bq); }
        __syncthreads();
        unsigned long long g = g0, e = e0;
        for (int x = 0; x < w; ++x) { g += s_gt[x]; e += s_eq[x]; }
        g += (unsigned)__popcll(ba & below); e += (unsigned)__popcll(bq & below);
        if (a || (q && e < E)) {
            const unsigned long long pos = g + (e < E ? e : E);
            if (pos < (unsigned long long)limit) { out_idx[pos] = k; if (out_key) out_key[pos] = u; }
        }
        g0 += s_gt[0] + s_gt[1] + s_gt[2] + s_gt[3]; e0 += s_eq[0] + s_eq[1] + s_eq[2] + s_eq[3];
        __syncthreads();
    }
}

__global__ void pmx_select_take_kernel(const int64_t *__restrict__ sorted, const PmxSelState *__restrict__ state,
                                       int64_t *__restrict__ hit_index, long long capacity)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long h = state->h;
    if (p < capacity && (unsigned long long)p < h) hit_index[p] = sorted[p];
}

// scratch layout: [state 256][hist SEL_BINS][blk_gt nb][blk_eq nb] and, by score, [keys_in m][keys_out m][vals_in m][vals_out m][temp]
// with m = the most that can be selected
static long long sel_blocks(long long n) { return (n + SEL_TILE - 1) / SEL_TILE; }
static long long sel_most(long long n, long long max_hits) { return max_hits > 0 && max_hits < n ? max_hits : n; }
static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t sel_sort_temp(long long m)
{
    size_t temp = 0;
    (void)rocprim::radix_sort_pairs_desc(nullptr, temp, (uint32_t *)nullptr, (uint32_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr,
                                         (size_t)m, 0, 32, nullptr);
    return temp;
}
size_t pmx_select_scratch_bytes(long long n, long long max_hits, int order)
{
    if (n <= 0) return 256;
    const long long nb = sel_blocks(n), m = sel_most(n, max_hits);
    size_t b = 256 + al256(SEL_BINS * 8) + 2 * al256((size_t)nb * 8);
    if (order == PMX_HITS_BY_SCORE) b += 2 * al256((size_t)m * 4) + 2 * al256((size_t)m * 8) + al256(sel_sort_temp(m)) + 256;
    return b;
}

int pmx_launch_select(const pmx_record_t *recs, long long n, int min_score, long long max_hits, int order,
                      int64_t *hit_index, long long capacity, int64_t *counts, void *scratch, hipStream_t st)
{
#define SEL_OK(expr) do { const hipError_t e__ = (expr); if (e__ != hipSuccess) return -(int)e__; } while (0)
    if (n <= 0) { if (counts) SEL_OK(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st)); return 0; }
    unsigned char *p = (unsigned char *)scratch;
    PmxSelState *state = (PmxSelState *)p; p += 256;
    unsigned long long *hist = (unsigned long long *)p; p += al256(SEL_BINS * 8);
    const long long nb = sel_blocks(n), m = sel_most(n, max_hits);
    unsigned long long *blk_gt = (unsigned long long *)p; p += al256((size_t)nb * 8);
    unsigned long long *blk_eq = (unsigned long long *)p; p += al256((size_t)nb * 8);
    const uint32_t min_u = (uint32_t)min_score ^ 0x80000000u;
    SEL_OK(hipMemsetAsync(scratch, 0, 256 + al256(SEL_BINS * 8), st));
    const unsigned hgrid = (unsigned)std::min<long long>((n + 255) / 256, 1024);
    static const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
    for (int ps = 0; ps < 3; ++ps) {
        if (ps && max_hits <= 0) break;                       // (no limit: nothing to cut)
        hipLaunchKernelGGL(pmx_select_hist_kernel, dim3(hgrid), dim3(256), 0, st, recs, n, min_u, state, hist, shifts[ps], widths[ps], ps == 0);
        hipLaunchKernelGGL(pmx_select_pick_kernel, dim3(1), dim3(256), 0, st, state, hist, shifts[ps], widths[ps], ps == 0, max_hits);
    }
    hipLaunchKernelGGL(pmx_select_count_kernel, dim3((unsigned)nb), dim3(256), 0, st, recs, n, min_u, state, blk_gt, blk_eq);
    hipLaunchKernelGGL(pmx_select_scan_kernel, dim3(1), dim3(256), 0, st, blk_gt, blk_eq, nb, state, counts);
    if (order != PMX_HITS_BY_SCORE) {
        hipLaunchKernelGGL(pmx_select_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, st, recs, n, min_u, state, blk_gt, blk_eq,
                           hit_index, (uint32_t *)nullptr, capacity);
        SEL_OK(hipGetLastError());
        return 0;
    }
    uint32_t *keys_in = (uint32_t *)p; p += al256((size_t)m * 4);
    uint32_t *keys_out = (uint32_t *)p; p += al256((size_t)m * 4);
    int64_t *vals_in = (int64_t *)p; p += al256((size_t)m * 8);
    int64_t *vals_out = (int64_t *)p; p += al256((size_t)m * 8);
    size_t temp_bytes = sel_sort_temp(m);
    // slots beyond the number selected keep key 0, the lowest: the stable descending sort leaves them behind every hit
    SEL_OK(hipMemsetAsync(keys_in, 0, (size_t)m * 4, st));
    SEL_OK(hipMemsetAsync(vals_in, 0, (size_t)m * 8, st));
    hipLaunchKernelGGL(pmx_select_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, st, recs, n, min_u, state, blk_gt, blk_eq,
                       vals_in, keys_in, m);
    SEL_OK(hipGetLastError());
    SEL_OK(rocprim::radix_sort_pairs_desc((void *)p, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)m, 0, 32, st));
    const long long take = std::min<long long>(m, capacity);
    if (take > 0)
        hipLaunchKernelGGL(pmx_select_take_kernel, dim3((unsigned)((take + 255) / 256)), dim3(256), 0, st, vals_out, state, hit_index, capacity);
    SEL_OK(hipGetLastError());
    return 0;
}

// ---- the hits of a search: diagonal and reference length per hit, the hit records, the begins ------------------------------------
// positions [0, cap) of a list the selection filled up to min(counts[0], cap): lengths beyond it are 0, so the scan of all cap + 1
// entries ends in the number of reference bytes the hits hold (counts == NULL: all cap are there; recs / diag == NULL: lengths only)
__global__ void pmx_select_hitlen_kernel(const int64_t *__restrict__ idx, const int64_t *__restrict__ counts, long long cap,
                                         const pmx_record_t *__restrict__ recs, const int64_t *__restrict__ roff,
                                         int32_t *__restrict__ diag, int32_t *__restrict__ hlen)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= cap + 2) return;
    int32_t d = 0, l = 0;
    if (p < cap && (!counts || p < counts[0])) {
        const long long k = idx[p];
        if (recs) { const pmx_record_t r = recs[k]; d = r.end_ref - r.end_query; }
        l = (int32_t)(roff[k + 1] - roff[k]);
    }
    if (diag && p < cap) diag[p] = d;
    hlen[p] = l;
}

__global__ void pmx_select_hits_kernel(const int64_t *__restrict__ idx, const pmx_record_t *__restrict__ recs,
                                       const int32_t *__restrict__ diag, long long h, pmx_hit_t *__restrict__ hits)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= h) return;
    pmx_hit_t t;
    t.index = idx[p]; t.first = recs[t.index]; t.diag = diag[p]; t.beg_query = -1; t.beg_ref = -1; t.reserved = 0;
    hits[p] = t;
}

__global__ void pmx_select_begins_kernel(const int32_t *__restrict__ beg, long long h, pmx_hit_t *__restrict__ hits)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= h) return;
    hits[p].beg_query = beg[2 * p]; hits[p].beg_ref = beg[2 * p + 1];
}

int pmx_launch_hit_lengths(const int64_t *idx, const int64_t *counts, long long cap, const pmx_record_t *recs, const int64_t *roff,
                           int32_t *diag, int32_t *hlen, hipStream_t st)
{
    hipLaunchKernelGGL(pmx_select_hitlen_kernel, dim3((unsigned)((cap + 2 + 255) / 256)), dim3(256), 0, st, idx, counts, cap, recs, roff, diag, hlen);
    return pmx_launched();
}
int pmx_launch_hit_records(const int64_t *idx, const pmx_record_t *recs, const int32_t *diag, long long h, pmx_hit_t *hits, hipStream_t st)
{
    if (h <= 0) return 0;
    hipLaunchKernelGGL(pmx_select_hits_kernel, dim3((unsigned)((h + 255) / 256)), dim3(256), 0, st, idx, recs, diag, h, hits);
    return pmx_launched();
}
int pmx_launch_hit_begins(const int32_t *beg, long long h, pmx_hit_t *hits, hipStream_t st)
{
    if (h <= 0) return 0;
    hipLaunchKernelGGL(pmx_select_begins_kernel, dim3((unsigned)((h + 255) / 256)), dim3(256), 0, st, beg, h, hits);
    return pmx_launched();
}

// ---- gather: reference idx[p] -> out[ooff[p] .. ooff[p + 1]) ------------------------------------------------------------------------
// One wave per hit.  Up to three head bytes bring the destination to a dword boundary; each destination dword is then assembled from
// the two aligned source dwords that hold its four bytes (one when the source is aligned too); the tail goes byte by byte.  A dword
// whose aligned source dwords would reach outside [rbuf, rbuf + roff[n]) -- the first or last few bytes of the caller's buffer, which
// has no promised slack -- is assembled from its own four bytes instead.  A hit whose end would cross out_cap is not written.
__global__ __launch_bounds__(256)
void pmx_gather_refs_kernel(const uint8_t *__restrict__ rbuf, const int64_t *__restrict__ roff, long long n,
                            const int64_t *__restrict__ idx, long long h, uint8_t *__restrict__ out, const int64_t *__restrict__ ooff,
                            long long out_cap)
{
    const long long p = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (p >= h) return;
    const long long k = idx[p];
    const long long len = roff[k + 1] - roff[k], o = ooff[p];
    if (o + len > out_cap) return;
    const uint8_t *src = rbuf + roff[k];
    uint8_t *dst = out + o;
    const uintptr_t lo_bound = (uintptr_t)rbuf, hi_bound = (uintptr_t)(rbuf + roff[n]);
    long long head = (4 - (long long)((uintptr_t)dst & 3)) & 3;
    if (head > len) head = len;
    if (lane < head) dst[lane] = src[lane];
    const long long nd = (len - head) >> 2;
    const uint8_t *s0 = src + head;
    uint32_t *d0 = reinterpret_cast<uint32_t *>(dst + head);
    for (long long x = lane; x < nd; x += 64) {
        const uint8_t *s = s0 + 4 * x;
        const uintptr_t sa = (uintptr_t)s & ~(uintptr_t)3;
        const unsigned sh = (unsigned)((uintptr_t)s & 3);
        uint32_t v;
        if (sa >= lo_bound && sa + (sh ? 8 : 4) <= hi_bound) {
            const uint32_t lo = *reinterpret_cast<const uint32_t *>(sa);
            const uint32_t hi = sh ? *reinterpret_cast<const uint32_t *>(sa + 4) : 0u;
            v = __builtin_amdgcn_alignbyte(hi, lo, sh);
        } else
            v = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
        d0[x] = v;
    }
    const long long done = head + 4 * nd;
    if (lane < len - done) dst[done + lane] = src[done + lane];
}

int pmx_launch_gather_refs(const uint8_t *rbuf, const int64_t *roff, long long n, const int64_t *idx, long long h,
                           uint8_t *out, const int64_t *ooff, long long out_cap, hipStream_t st)
{
    if (h <= 0) return 0;
    hipLaunchKernelGGL(pmx_gather_refs_kernel, dim3((unsigned)((h + 3) / 4)), dim3(256), 0, st, rbuf, roff, n, idx, h, out, ooff, out_cap);
    return pmx_launched();
}
