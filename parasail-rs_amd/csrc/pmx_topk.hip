// pmx_topk.hip -- per-query top-K of a rectangular set search: the best K references of every query row, kept across the chunks of
// the run.  gfx950 only.  Semantics: include/parasail_amd.h (pmx_search_topk[_device]); DESIGN 2.5g.
//
// The order.  key(score, j) = (score ^ 0x80000000) << 32 | (0x7FFFFFFF - j) is unique within a row and never 0 (j <= 2^31 - 2), and
// descending key order is exactly (score descending, j ascending).  "The K best of a row" is therefore the set of its K largest keys:
// no tie rule is left to implement, and a set does not depend on the order in which candidates were looked at.  0 marks an empty slot.
//
// The collector (topk_push / topk_settle).  A workgroup keeps 2 KP (key, source) slots in LDS, KP = the power of two at or above
// max(K, 256).  Candidates arrive 256 at a time; those above the current bound are appended behind a ballot / popcount scan.  When
// the next 256 might not fit, a bitonic network sorts the 2 KP slots in descending order, everything behind the K-th is dropped and
// the K-th key becomes the bound.  Whatever the arrival order, the slots end as the K largest keys seen, sorted.
//
// Per chunk (a contiguous range of p = i |R| + j, so per row a contiguous range of j: a segment):
//   pmx_topk_tile_kernel   one workgroup per tile of at most TOPK_TILE records of one segment (tiles never cross a row): the candidates
//                          -- score >= min_score, not the self pair, key above the K-th key of the row's list when that list is full
//                          -- reduced to the tile's at most K best keys, and the tile's number of passing records.
//   pmx_topk_row_kernel    one workgroup per row of the chunk: the row's list and the survivors of its tiles (a thread per tile, best
//                          first, until the tile's next key no longer beats the bound) through the collector,
//                          then records and statistics gathered by source (list slot or chunk record) into registers, a barrier,
//                          and the list written back in order.  |P_i| grows by the tiles' passing counts.
// After the last chunk:
//   (pmx_launch_text_offsets: the rows' numbers held -> d_row_off)
//   pmx_topk_emit_kernel   one wave per row: the list to its CSR position below `capacity`, descriptor and p generated from the key.
//   pmx_topk_counts_kernel one workgroup: kept, written, passing.
// No kernel has an atomic; every output position is arithmetic on the scan and the sorted order.
#include "pmx_common.h"

#define TOPK_TILE 2048
#define TOPK_LIST 1024u                 // sources below it are list slots, the others TOPK_LIST + the record's position in the chunk

static __device__ __forceinline__ uint64_t topk_key(int32_t score, uint32_t j)
{
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint64_t)(0x7FFFFFFFu - j);
}

// Descending bitonic sort of n2 (a power of two >= 512) slots by 256 threads.  Starts and ends behind a barrier.
static __device__ void topk_sort(uint64_t *key, uint32_t *src, unsigned n2)
{
    __syncthreads();
    for (unsigned k = 2; k <= n2; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned t = threadIdx.x; t < n2 / 2; t += 256) {
                const unsigned a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const uint64_t ka = key[a], kb = key[b];
                const bool desc = (a & k) == 0;
                if (desc ? ka < kb : ka > kb) {
                    key[a] = kb; key[b] = ka;
                    const uint32_t sa = src[a]; src[a] = src[b]; src[b] = sa;
                }
            }
            __syncthreads();
        }
}

struct TopkBuf { uint64_t *key; uint32_t *src; unsigned *wave; unsigned n2, ks, count; uint64_t floor, bound; bool dirty /* appended since the last sort */, changed /* appended at all */; };

// Sort, keep the ks best, raise the bound.  Uniform across the workgroup.
static __device__ void topk_settle(TopkBuf &b)
{
    topk_sort(b.key, b.src, b.n2);
    for (unsigned x = b.ks + threadIdx.x; x < b.n2; x += 256) b.key[x] = 0;
    __syncthreads();
    if (b.count > b.ks) b.count = b.ks;
    b.bound = b.count == b.ks ? b.key[b.ks - 1] : b.floor;
    b.dirty = false;
}

// Every thread of the workgroup calls it with one candidate (k == 0: none).  Uniform control flow.
static __device__ void topk_push(TopkBuf &b, uint64_t k, uint32_t s)
{
    if (b.count + 256 > b.n2) topk_settle(b);
    const bool take = k > b.bound;
    if (!__syncthreads_or(take)) return;
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(take);
    if (lane == 0) b.wave[w] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned pos = b.count, total = 0;
    for (unsigned x = 0; x < 4; ++x) { const unsigned c = b.wave[x]; if (x < w) pos += c; total += c; }
    pos += (unsigned)__popcll(m & (lane ? (~0ull >> (64 - lane)) : 0ull));
    if (take) { b.key[pos] = k; b.src[pos] = s; }                 // pos < count + 256 <= n2
    b.count += total; b.dirty = true; b.changed = true;
}

static __device__ void topk_buf_init(TopkBuf &b, uint64_t *mem, unsigned kp, unsigned ks)
{
    b.n2 = 2 * kp; b.ks = ks; b.count = 0; b.floor = 0; b.bound = 0; b.dirty = false; b.changed = false;
    b.key = mem; b.src = (uint32_t *)(mem + b.n2); b.wave = b.src + b.n2;
    for (unsigned x = threadIdx.x; x < b.n2; x += 256) b.key[x] = 0;
    __syncthreads();
}
static size_t topk_lds_bytes(unsigned kp) { return (size_t)2 * kp * 12 + 16; }

// The geometry of row `rc` of a chunk that holds pairs [p0, p0 + cn) of the rectangle: absolute row, and its segment [j0, j1).
struct TopkSeg { unsigned long long ai; unsigned j0, j1; long long base; /* chunk position of (ai, 0), may be negative */ };
static __device__ __forceinline__ TopkSeg topk_segment(unsigned long long p0, unsigned long long cn, unsigned long long nr, unsigned long long rc)
{
    TopkSeg s;
    s.ai = p0 / nr + rc;
    const unsigned long long r0 = s.ai * nr, lo = p0 > r0 ? p0 : r0, hi = p0 + cn < r0 + nr ? p0 + cn : r0 + nr;
    s.j0 = (unsigned)(lo - r0); s.j1 = (unsigned)(hi - r0);
    s.base = (long long)r0 - (long long)p0;
    return s;
}

// Grid: rows of the chunk x tps (tiles a segment can touch).  Slot blockIdx.x of t_keys (tstride keys each) / t_cnt / t_pass.
__global__ __launch_bounds__(256)
void pmx_topk_tile_kernel(const pmx_record_t *__restrict__ rec, unsigned long long p0, unsigned long long cn, unsigned long long nr,
                          long long q_first, unsigned ks, unsigned kp, int32_t min_score, int skip_self, unsigned tps, unsigned tstride,
                          const uint64_t *__restrict__ st_keys, const int32_t *__restrict__ st_held,
                          uint64_t *__restrict__ t_keys, int32_t *__restrict__ t_cnt, int32_t *__restrict__ t_pass)
{
    extern __shared__ uint64_t s_mem[];
    __shared__ unsigned s_pass[4];
    const unsigned long long rc = blockIdx.x / tps;
    const TopkSeg g = topk_segment(p0, cn, nr, rc);
    const unsigned long long t = g.j0 / TOPK_TILE + blockIdx.x % tps;
    const unsigned long long ta = t * TOPK_TILE, tb = ta + TOPK_TILE;
    const unsigned a = ta > g.j0 ? (unsigned)ta : g.j0, e = tb < g.j1 ? (unsigned)tb : g.j1;
    if (ta >= g.j1 || a >= e) return;                                  // (a slot the row kernel never reads)
    const long long li = (long long)g.ai - q_first;
    TopkBuf b;
    topk_buf_init(b, s_mem, kp, ks);
    if ((unsigned)st_held[li] == ks) b.floor = b.bound = st_keys[(size_t)li * ks + ks - 1];
    unsigned pass = 0;
    for (unsigned x = a; x < e; x += 256) {                            // uniform trip count
        const unsigned j = x + threadIdx.x;
        uint64_t k = 0;
        if (j < e) {
            const int32_t sc = rec[g.base + (long long)j].score;
            if (sc >= min_score && !(skip_self && (unsigned long long)j == g.ai)) { ++pass; k = topk_key(sc, j); }
        }
        topk_push(b, k, j);
    }
    if (b.dirty) topk_settle(b); else __syncthreads();
    for (unsigned x = threadIdx.x; x < b.count; x += 256) t_keys[(size_t)blockIdx.x * tstride + x] = b.key[x];
    for (int o = 32; o > 0; o >>= 1) pass += __shfl_down(pass, o);
    if ((threadIdx.x & 63) == 0) s_pass[threadIdx.x >> 6] = pass;
    __syncthreads();
    if (threadIdx.x == 0) { t_cnt[blockIdx.x] = (int32_t)b.count; t_pass[blockIdx.x] = (int32_t)(s_pass[0] + s_pass[1] + s_pass[2] + s_pass[3]); }
}

// Grid: the rows of the chunk.
__global__ __launch_bounds__(256)
void pmx_topk_row_kernel(const pmx_record_t *__restrict__ rec, const pmx_stats_t *__restrict__ stats,
                         unsigned long long p0, unsigned long long cn, unsigned long long nr, long long q_first,
                         unsigned ks, unsigned kp, unsigned tps, unsigned tstride,
                         const uint64_t *__restrict__ t_keys, const int32_t *__restrict__ t_cnt, const int32_t *__restrict__ t_pass,
                         uint64_t *st_keys, pmx_record_t *st_recs, pmx_stats_t *st_stats, int32_t *st_held, int64_t *st_passing)
{
    extern __shared__ uint64_t s_mem[];
    __shared__ unsigned long long s_pass[4];
    const TopkSeg g = topk_segment(p0, cn, nr, blockIdx.x);
    const long long li = (long long)g.ai - q_first;
    const unsigned nt = (g.j1 - 1) / TOPK_TILE - g.j0 / TOPK_TILE + 1;       // tiles of the segment (j1 > j0: the row is in the chunk)
    const size_t slot0 = (size_t)blockIdx.x * tps;
    const size_t l0 = (size_t)li * ks;
    // |P_i|
    unsigned long long pass = 0;
    for (unsigned x = threadIdx.x; x < nt; x += 256) pass += (unsigned long long)t_pass[slot0 + x];
    for (int o = 32; o > 0; o >>= 1) pass += __shfl_down(pass, o);
    if ((threadIdx.x & 63) == 0) s_pass[threadIdx.x >> 6] = pass;
    // the list, then the tiles' survivors
    TopkBuf b;
    topk_buf_init(b, s_mem, kp, ks);                                         // (its barrier publishes s_pass)
    if (threadIdx.x == 0) st_passing[li] += (int64_t)(s_pass[0] + s_pass[1] + s_pass[2] + s_pass[3]);
    const unsigned held = (unsigned)st_held[li];
    for (unsigned x = threadIdx.x; x < held; x += 256) { b.key[x] = st_keys[l0 + x]; b.src[x] = x; }
    __syncthreads();
    b.count = held;
    if (held == ks) b.floor = b.bound = b.key[ks - 1];
    // a thread per tile, 256 tiles at a time; a tile's survivors are sorted, so a thread is done at its first key at or below the bound
    for (unsigned x0 = 0; x0 < nt; x0 += 256) {
        const unsigned x = x0 + threadIdx.x;
        unsigned c = x < nt ? (unsigned)t_cnt[slot0 + x] : 0u;
        const uint64_t *tk = t_keys + (slot0 + (x < nt ? x : 0u)) * tstride;
        for (unsigned y = 0; __syncthreads_or(y < c); ++y) {
            uint64_t k = 0; uint32_t s = 0;
            if (y < c) {
                k = tk[y];
                if (k > b.bound) s = TOPK_LIST + (uint32_t)(g.base + (long long)(0x7FFFFFFFu - (uint32_t)k));      // j from the key -> the record's place in the chunk
                else { k = 0; c = 0; }
            }
            topk_push(b, k, s);
        }
    }
    if (!b.changed) return;                                                  // nothing entered: the list stands
    if (b.dirty) topk_settle(b);
    // gather by source into registers, then write the list back: a slot is read by one thread and written by another
    uint4 r[4]; int32_t q[4][3]; uint64_t kk[4];                           // (records are 16 bytes on 16-byte boundaries, statistics 3 ints)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned x = threadIdx.x + 256u * u;
        r[u] = make_uint4(0, 0, 0, 0); q[u][0] = q[u][1] = q[u][2] = 0; kk[u] = 0;
        if (x < b.count) {
            const uint32_t s = b.src[x];
            const bool listed = s < TOPK_LIST;
            const size_t at = listed ? l0 + s : (size_t)(s - TOPK_LIST);
            kk[u] = b.key[x];
            r[u] = *reinterpret_cast<const uint4 *>(listed ? st_recs + at : rec + at);
            if (st_stats) {
                const int32_t *ps = reinterpret_cast<const int32_t *>(listed ? st_stats + at : stats + at);
                q[u][0] = ps[0]; q[u][1] = ps[1]; q[u][2] = ps[2];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned x = threadIdx.x + 256u * u;
        if (x < b.count) {
            st_keys[l0 + x] = kk[u];
            *reinterpret_cast<uint4 *>(st_recs + l0 + x) = r[u];
            if (st_stats) { int32_t *ps = reinterpret_cast<int32_t *>(st_stats + l0 + x); ps[0] = q[u][0]; ps[1] = q[u][1]; ps[2] = q[u][2]; }
        }
    }
    if (threadIdx.x == 0) st_held[li] = (int32_t)b.count;
}

// One wave per row.  Stores to the caller's hit arrays only at positions below `capacity`.  The stranded search: the lists' records carry
// their strand as PMX_FLAG_STRAND1 (`marked`), taken out here; hit_strand (optional) receives it as a byte.  marked == 2 (the
// translated search): they carry their frame in PMX_FLAG_FRAME_MASK instead, and the byte is the frame.
__global__ __launch_bounds__(256)
void pmx_topk_emit_kernel(long long nq, long long q_first, unsigned long long nr, unsigned ks,
                          const uint64_t *__restrict__ st_keys, const pmx_record_t *__restrict__ st_recs, const pmx_stats_t *__restrict__ st_stats,
                          const int32_t *__restrict__ st_held, const int64_t *__restrict__ st_passing, const int64_t *__restrict__ row_off,
                          long long capacity, pmx_pair_t *__restrict__ hit_pairs, int64_t *__restrict__ hit_index,
                          pmx_record_t *__restrict__ hit_recs, pmx_stats_t *__restrict__ hit_stats, int64_t *__restrict__ row_passing,
                          uint8_t *__restrict__ hit_strand, int marked)
{
    const long long li = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const unsigned lane = threadIdx.x & 63;
    if (li >= nq) return;
    if (row_passing && lane == 0) row_passing[li] = st_passing[li];
    const long long off = row_off[li];
    const unsigned h = (unsigned)st_held[li];
    const size_t l0 = (size_t)li * ks;
    const long long ai = q_first + li;
    for (unsigned x = lane; x < h; x += 64) {
        const long long pos = off + x;
        if (pos >= capacity) return;                                   // (positions ascend with x)
        const long long j = (long long)(0x7FFFFFFFu - (uint32_t)st_keys[l0 + x]);
        if (hit_pairs) { pmx_pair_t d; d.q = ai; d.r = j; d.q_beg = 0; d.q_len = -1; d.r_beg = 0; d.r_len = -1; hit_pairs[pos] = d; }
        if (hit_index) hit_index[pos] = (int64_t)((unsigned long long)ai * nr + (unsigned long long)j);
        pmx_record_t r = st_recs[l0 + x];
        if (marked == 2) {                                             // (the translated search: the byte is the frame)
            if (hit_strand) hit_strand[pos] = (uint8_t)((r.flags & PMX_FLAG_FRAME_MASK) >> PMX_FLAG_FRAME_SHIFT);
            r.flags &= ~PMX_FLAG_FRAME_MASK;
        } else {
            if (hit_strand) hit_strand[pos] = (uint8_t)((r.flags & PMX_FLAG_STRAND1) != 0);
            if (marked) r.flags &= ~PMX_FLAG_STRAND1;
        }
        hit_recs[pos] = r;
        if (hit_stats) hit_stats[pos] = st_stats[l0 + x];
    }
}

__global__ __launch_bounds__(256)
void pmx_topk_counts_kernel(long long nq, const int64_t *__restrict__ st_passing, const int64_t *__restrict__ row_off, long long capacity,
                            int64_t *__restrict__ counts)
{
    __shared__ long long s_sum[4];
    long long sum = 0;
    for (long long x = threadIdx.x; x < nq; x += 256) sum += st_passing[x];
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long kept = row_off[nq];
        counts[0] = kept; counts[1] = kept < capacity ? kept : capacity; counts[2] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static unsigned topk_kp(unsigned ks) { unsigned kp = 256; while (kp < ks) kp <<= 1; return kp; }

void pmx_topk_geometry(long long chunk, long long nr, int ks, long long *rows, long long *tps, long long *tstride)
{
    const long long tpr = (nr + TOPK_TILE - 1) / TOPK_TILE, per_chunk = chunk / TOPK_TILE + 2;
    *rows = chunk / nr + 2;
    *tps = tpr < per_chunk ? tpr : per_chunk;
    *tstride = ks < TOPK_TILE ? ks : TOPK_TILE;
}

int pmx_launch_topk_merge(const pmx_record_t *rec, const pmx_stats_t *stats, long long p0, long long cn, long long nr, long long q_first,
                          int ks, int32_t min_score, int skip_self, long long tps, long long tstride,
                          uint64_t *t_keys, int32_t *t_cnt, int32_t *t_pass,
                          uint64_t *st_keys, pmx_record_t *st_recs, pmx_stats_t *st_stats, int32_t *st_held, int64_t *st_passing, hipStream_t st)
{
    if (cn <= 0) return 0;
    const long long rows = (p0 + cn - 1) / nr - p0 / nr + 1;
    if (rows * tps > 0x7FFFFFFFLL) return -(int)hipErrorInvalidValue;
    const unsigned kp = topk_kp((unsigned)ks);
    const size_t lds = topk_lds_bytes(kp);
    hipLaunchKernelGGL(pmx_topk_tile_kernel, dim3((unsigned)(rows * tps)), dim3(256), lds, st, rec, (unsigned long long)p0, (unsigned long long)cn,
                       (unsigned long long)nr, q_first, (unsigned)ks, kp, min_score, skip_self, (unsigned)tps, (unsigned)tstride,
                       st_keys, st_held, t_keys, t_cnt, t_pass);
    hipLaunchKernelGGL(pmx_topk_row_kernel, dim3((unsigned)rows), dim3(256), lds, st, rec, stats, (unsigned long long)p0, (unsigned long long)cn,
                       (unsigned long long)nr, q_first, (unsigned)ks, kp, (unsigned)tps, (unsigned)tstride, t_keys, t_cnt, t_pass,
                       st_keys, st_recs, st_stats, st_held, st_passing);
    return pmx_launched();
}

int pmx_launch_topk_emit(long long nq, long long q_first, long long nr, int ks, const uint64_t *st_keys, const pmx_record_t *st_recs,
                         const pmx_stats_t *st_stats, const int32_t *st_held, const int64_t *st_passing, const int64_t *row_off, long long capacity,
                         pmx_pair_t *hit_pairs, int64_t *hit_index, pmx_record_t *hit_recs, pmx_stats_t *hit_stats, int64_t *row_passing,
                         int64_t *counts, hipStream_t st, uint8_t *hit_strand, int marked)
{
    if (nq <= 0) return 0;
    hipLaunchKernelGGL(pmx_topk_emit_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, nq, q_first, (unsigned long long)nr, (unsigned)ks,
                       st_keys, st_recs, st_stats, st_held, st_passing, row_off, capacity, hit_pairs, hit_index, hit_recs, hit_stats, row_passing, hit_strand, marked);
    hipLaunchKernelGGL(pmx_topk_counts_kernel, dim3(1), dim3(256), 0, st, nq, st_passing, row_off, capacity, counts);
    return pmx_launched();
}
