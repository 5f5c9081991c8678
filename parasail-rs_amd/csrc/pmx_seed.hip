// pmx_seed.hip -- k-mer seeding (semantics: include/parasail_amd.h): the k-mer index of a DNA set and the candidate
// windows of queries against it -- exact k-mer matches, clustered by diagonal, as descriptors for pmx_align_pairs_ex_device.
//
// Index.  Every byte position of the reference buffer gets one entry: the 2k-bit key of the k-mer that starts there, or the key
// 1 << 2k where no k-mer starts (a sequence end inside, an invalid letter, no sequence).  rocPRIM's stable radix sort on bits
// [0, 2k + 1) leaves the k-mers in (kmer, seq, pos) order in front and the empty positions behind them, so nothing is compacted.  A
// bucket table on the top min(2k, 22) bits (16 MiB at most: it stays in the Infinity Cache) turns a lookup into one table read and a
// binary search inside one bucket.
//
// Seeding, per slice of rows.  A position slot is (row, strand, i): count looks the slot's k-mer up (first entry, occurrences; 0 above
// max_occ), a scan gives every slot its place in the match buffer, emit writes a match as the key (r << 32) | biased diagonal, a
// segmented radix sort orders each (row, strand) segment by (r, d).  Clusters are then runs of the sorted keys: a head flag per match, a
// max-scan that carries each head's index to its run, a candidate flag at each run's last match, a scan of those flags for the output
// positions.  Every position comes from a scan over sorted data; the only atomic in this file counts the index's entries.
//
// The letters and translated indexes run the same pipeline: a run is described once by PmxSeedPlan (pmx_common.h),
// the two launchers at the end of this file read it, and emit and hits are one template each over the plan's geometry.
//
// Chaining is the DNA road with another middle: the matches sorted by (r, j) with i beside them, one wave per segment
// that scores collinear chains with gap costs, a walk from every chain's tail -- and the same count pass, cut, flag scan and row offsets.
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include "pmx_common.h"
#include <rocprim/rocprim.hpp>

// letter -> 2-bit code, A/a 0, C/c 1, G/g 2, T/t/U/u 3; -1: not a nucleotide
__device__ __forceinline__ int pmx_seed_code(uint32_t b)
{
    const uint32_t u = b & 0xDFu;
    const bool ok = u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'U';
    const int c = (int)((u >> 1) & 3u);
    return ok ? (c ^ (c >> 1)) : -1;
}

// ---- index build ---------------------------------------------------------------------------------------------------------------------
#define PMX_SEED_TILE 16        // positions per thread of the extraction: one rolling key over 16 + k - 1 bytes

// What the three extract kernels share.  The sequence a walk is in: region r of byte p0 -- -1 before the first sequence, count behind
// the last one, else sequence r = [b, e) = [off[r], off[r + 1]).  Offsets are read at indices 0 .. count only and a byte only below
// `bytes`, whatever a wrapped set's offsets hold.
struct PmxSeedRegion { long long r, b, e; };
__device__ __forceinline__ PmxSeedRegion pmx_seed_region(const int64_t *__restrict__ off, long long count, long long p0)
{
    long long lo = 0, hi = count + 1;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (off[mid] <= p0) lo = mid + 1; else hi = mid; }
    PmxSeedRegion g;
    g.r = lo - 1;
    g.e = g.r < count ? off[g.r + 1] : INT64_MAX;
    g.b = g.r >= 0 ? off[g.r] : 0;
    return g;
}
// on to the region of byte x; true: a boundary was crossed (the caller's runs start over)
__device__ __forceinline__ bool pmx_seed_region_advance(PmxSeedRegion &g, const int64_t *__restrict__ off, long long count, long long x)
{
    bool crossed = false;
    while (x >= g.e && g.r < count) { ++g.r; g.b = g.e; g.e = g.r < count ? off[g.r + 1] : INT64_MAX; crossed = true; }
    return crossed;
}
// byte x lies in a sequence of the set
__device__ __forceinline__ bool pmx_seed_region_inside(const PmxSeedRegion &g, long long count, long long bytes, long long x)
{
    return g.r >= 0 && g.r < count && g.b >= 0 && g.b <= x && x < g.e && g.e <= bytes;
}
// entry slots [s0, s1) at which no k-mer starts; base: the slot number of keys[0]
__device__ __forceinline__ void pmx_seed_no_kmers(uint64_t *__restrict__ keys, uint64_t *__restrict__ vals, long long base, long long s0, long long s1,
                                                  uint64_t invalid)
{
    for (long long s = s0; s < s1; ++s) { keys[s] = invalid; vals[s] = (uint64_t)(base + s); }
}
// *n_valid += the block's k-mers, `total` zeroed and a barrier passed before: one add per block, the sum does not depend on the order of arrival
__device__ __forceinline__ void pmx_seed_block_sum(unsigned &total, unsigned found, unsigned long long *n_valid)
{
    if (found) atomicAdd(&total, found);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(n_valid, (unsigned long long)total);
}

// keys[p] / vals[p] for every p < bytes; *n_valid += the k-mers found.  The key rolls in 2-bit arithmetic: no table.
__global__ void __launch_bounds__(256) pmx_seed_extract_kernel(const uint8_t *__restrict__ buf, const int64_t *__restrict__ off, long long count,
                                                               long long bytes, int k, uint64_t *__restrict__ keys, uint64_t *__restrict__ vals,
                                                               unsigned long long *n_valid)
{
    const long long p0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * PMX_SEED_TILE;
    unsigned found = 0;
    if (p0 < bytes) {
        const uint64_t invalid = (uint64_t)1 << (2 * k), mask = invalid - 1;
        PmxSeedRegion g = pmx_seed_region(off, count, p0);
        const long long pend = min(p0 + PMX_SEED_TILE, bytes), xend = min(pend + k - 1, bytes);
        uint64_t key = 0; int run = 0;
        for (long long x = p0; x < xend; ++x) {
            if (pmx_seed_region_advance(g, off, count, x)) run = 0;
            const int c = pmx_seed_region_inside(g, count, bytes, x) ? pmx_seed_code(buf[x]) : -1;
            if (c < 0) { run = 0; key = 0; } else { key = (key << 2) | (uint64_t)c; ++run; }
            const long long s = x - k + 1;
            if (s >= p0) {
                const bool have = run >= k && s >= g.b;
                keys[s] = have ? (key & mask) : invalid;
                vals[s] = have ? ((uint64_t)g.r << 32) | (uint64_t)(uint32_t)(s - g.b) : (uint64_t)s;
                found += have ? 1u : 0u;
            }
        }
        pmx_seed_no_kmers(keys, vals, 0, max(p0, xend - k + 1), pend, invalid);
    }
    __shared__ unsigned total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    pmx_seed_block_sum(total, found, n_valid);
}

// bucket[b] = the first entry whose key's top bits are >= b, for b in 0 .. nb (bucket[nb] = n); n > 0
__global__ void __launch_bounds__(256) pmx_seed_buckets_kernel(const uint64_t *__restrict__ keys, long long n, int shift, long long nb,
                                                               uint32_t *__restrict__ bucket)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long b = (long long)(keys[i] >> shift), prev = i ? (long long)(keys[i - 1] >> shift) : -1;
    for (long long x = prev + 1; x <= b; ++x) bucket[x] = (uint32_t)i;
    if (i == n - 1) for (long long x = b + 1; x <= nb; ++x) bucket[x] = (uint32_t)n;
}

__global__ void __launch_bounds__(256) pmx_seed_entries_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ vals,
                                                               long long first, long long count, uint64_t *kmer, int64_t *seq, int32_t *pos)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t v = vals[first + i];
    if (kmer) kmer[i] = keys[first + i];
    if (seq) seq[i] = (int64_t)(v >> 32);
    if (pos) pos[i] = (int32_t)(uint32_t)v;
}

size_t pmx_seed_index_sort_bytes(long long bytes, int k)
{
    size_t temp = 0;
    uint64_t *nul = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, temp, nul, nul, nul, nul, (size_t)bytes, 0, 2 * k + 1, nullptr);
    return temp + 256;
}

// keys_out / vals_out: the sorted index; keys_in / vals_in: `bytes` entries of scratch; n_valid: one zeroed counter on the device
int pmx_launch_seed_index(const uint8_t *buf, const int64_t *off, long long count, long long bytes, int k,
                          uint64_t *keys_in, uint64_t *vals_in, uint64_t *keys_out, uint64_t *vals_out, void *temp, size_t temp_bytes,
                          unsigned long long *n_valid, hipStream_t stream)
{
    if (bytes <= 0) return 0;
    const long long threads = (bytes + PMX_SEED_TILE - 1) / PMX_SEED_TILE;
    hipLaunchKernelGGL(pmx_seed_extract_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, buf, off, count, bytes, k,
                       keys_in, vals_in, n_valid);
    int rc = pmx_launched();
    if (rc) return rc;
    const hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)bytes, 0, 2 * k + 1, stream);
    return e == hipSuccess ? 0 : -(int)e;
}

int pmx_launch_seed_buckets(const uint64_t *keys, long long n, int shift, long long nb, uint32_t *bucket, hipStream_t stream)
{
    if (n <= 0) return hipMemsetAsync(bucket, 0, sizeof(uint32_t) * (size_t)(nb + 1), stream) == hipSuccess ? 0 : -1;
    hipLaunchKernelGGL(pmx_seed_buckets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, keys, n, shift, nb, bucket);
    return pmx_launched();
}

int pmx_launch_seed_entries(const uint64_t *keys, const uint64_t *vals, long long first, long long count, uint64_t *kmer, int64_t *seq,
                            int32_t *pos, hipStream_t stream)
{
    if (count <= 0) return 0;
    hipLaunchKernelGGL(pmx_seed_entries_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, keys, vals, first, count, kmer, seq, pos);
    return pmx_launched();
}

// ---- minimizers: the (w, k) sketch of a set's buffer or of oriented rows -----------------------------------------------
// Definitions: include/parasail_amd.h.  A position loses to p iff it has no k-mer or its (hash, position) is larger; a window of w
// consecutive k-mer positions of one sequence selects the position every other one loses to; a minimizer is a position some window
// selects.  The kernel decides each position on its own by the equivalent rule: with l the consecutive left neighbours that lose to p
// (at most w - 1, none before the sequence's first position) and r the same to the right (none behind its last k-mer position nk - 1),
// p is a minimizer iff it has a k-mer and l + r + 1 >= min(w, nk).  A thread writes only its own positions' bytes: no marking across
// threads, no atomics, the same bytes every run.
//
// One body, two forms.  A workgroup owns a tile of T = 256 C positions of a position space -- the set's buffer (C = 4: byte p of the
// buffer is position p, whatever sequence it lies in) or one (row, orientation) segment of max_qlen slots (C = 1: reads are short) --
// and stages the 2-bit codes of the tile, a halo of w - 1 positions on both sides and the k - 1 letters behind it in LDS, each byte read
// from memory once.  Every thread then rolls the keys of a contiguous piece of tile + halo out of LDS and leaves their hashes there.
// Traps:
//   * "no k-mer" is PMX_SKETCH_NONE = 2^64 - 1, which no hash takes: mix is a bijection on 2 k <= 62 bits, so a hash is below 2^62.
//   * the halo never lets a window cross a sequence end: the staged codes know nothing of sequences (a key rolled across an end is a
//     valid-looking hash), so the scan of p is clamped to the k-mer positions [b, e - k] of p's OWN sequence [b, e), which the thread
//     finds itself (pmx_seed_region); a row's segment is one sequence, [0, nk).
//   * strand 1 is read backwards through the complement into the staged codes, so positions, windows and the leftmost-wins rule are all
//     in oriented coordinates: the scans below never see the stored order.
#define PMX_SKETCH_NONE (~(uint64_t)0)
#define PMX_SKETCH_WMAX 64
#define PMX_SKETCH_KMAX 31
#define PMX_SKETCH_SET_C 4      // positions per thread, set form: T = 1024
#define PMX_SKETCH_ROW_C 1      // row form: T = 256

// the staged letters of the set form: position x is byte x of the buffer
struct PmxSketchSetCodes {
    const uint8_t *__restrict__ buf; long long bytes;
    __device__ __forceinline__ uint32_t operator()(long long x) const
    {
        if (x < 0 || x >= bytes) return 4u;
        const int c = pmx_seed_code(buf[x]);
        return c < 0 ? 4u : (uint32_t)c;
    }
};
// ... and of the row form: position x of the oriented row w of L letters (strand 1: comp[w[L - 1 - x]], never materialised)
struct PmxSketchRowCodes {
    const uint8_t *__restrict__ w; long long L; int strand;
    __device__ __forceinline__ uint32_t operator()(long long x) const
    {
        if (x < 0 || x >= L) return 4u;
        const int c = pmx_seed_code(strand ? w[L - 1 - x] : w[x]);
        return c < 0 ? 4u : (uint32_t)(strand ? 3 - c : c);
    }
};

// H[a] = the hash of position t0 - (w - 1) + a for a in [0, T + 2 (w - 1)), PMX_SKETCH_NONE where k valid letters do not start there.
// cod: T + 2 (w - 1) + k - 1 bytes of LDS.  Every thread of the workgroup calls it (two barriers).
template <int C, typename Codes>
__device__ __forceinline__ void pmx_sketch_hashes(const Codes &codes, long long t0, int k, int w, uint64_t *H, uint8_t *cod)
{
    const int S = 256 * C + 2 * (w - 1), nbytes = S + k - 1;
    const long long x0 = t0 - (w - 1);
    for (int a = threadIdx.x; a < nbytes; a += 256) cod[a] = (uint8_t)codes(x0 + a);
    __syncthreads();
    const int per = (S + 255) / 256, a0 = (int)threadIdx.x * per, a1 = min(a0 + per, S);
    const uint64_t mask = ((uint64_t)1 << (2 * k)) - 1;
    uint64_t key = 0; int run = 0;
    for (int a = a0; a0 < a1 && a < a1 + k - 1; ++a) {
        const uint32_t c = cod[a];
        run = c > 3u ? 0 : run + 1;
        key = (key << 2) | (uint64_t)(c & 3u);
        if (a - (k - 1) >= a0) H[a - (k - 1)] = run >= k ? pmx_seed_mix_bits(key & mask, k) : PMX_SKETCH_NONE;
    }
    __syncthreads();
}

// The per-position rule on the hashes in LDS: a = p's index in H, [lo, hi] = the indices of the positions of p's sequence that a window
// with p may hold (lo >= a - (w - 1), hi <= a + (w - 1)), need = min(w, nk).  Left neighbours lose on a larger hash (an equal one is
// left of p and wins), right ones on a larger or equal one; the scan stops at the first that does not lose or once `need` are together.
__device__ __forceinline__ bool pmx_sketch_selected(const uint64_t *H, int a, int lo, int hi, int need)
{
    const uint64_t hp = H[a];
    if (hp == PMX_SKETCH_NONE) return false;
    int got = 1;
    for (int q = a - 1; q >= lo && got < need && H[q] > hp; --q) ++got;
    for (int q = a + 1; q <= hi && got < need && H[q] >= hp; ++q) ++got;
    return got >= need;
}

struct PmxSketchArgs {
    const uint8_t *buf; const int64_t *off; long long count, bytes;       // set form: the set; row form: Q's buffer, offsets, -, bytes
    long long row0; int strands, strand0, max_qlen, tiles;                 // row form: the slice's first row, orientations, tiles per segment
    int k, w;
    uint8_t *flags;                                                        // one byte per position (set form) / per position slot (row form)
};

// flags[p] = 1 where position p is a minimizer, 0 elsewhere, for every position of the space.
// ROWS false: the set's buffer, walked as pmx_seed_extract_kernel walks it (offsets read at 0 .. count only, bytes below `bytes` only);
//   a thread owns C = 4 consecutive bytes and packs their flags into one store.
// ROWS true: block = (segment, tile); segment t = (row_local * strands + s), slot (t * max_qlen + i).  A row longer than max_qlen or
//   with bad offsets has no minimizer.
template <bool ROWS>
__global__ void __launch_bounds__(256) pmx_seed_sketch_kernel(PmxSketchArgs g)
{
    constexpr int C = ROWS ? PMX_SKETCH_ROW_C : PMX_SKETCH_SET_C, T = 256 * C;
    __shared__ uint64_t H[T + 2 * (PMX_SKETCH_WMAX - 1)];
    __shared__ uint8_t cod[T + 2 * (PMX_SKETCH_WMAX - 1) + PMX_SKETCH_KMAX - 1 + 2];
    const int k = g.k, w = g.w, halo = w - 1;
    if (ROWS) {
        const long long t = (long long)blockIdx.x / g.tiles, t0 = ((long long)blockIdx.x - t * g.tiles) * T;
        const long long row = g.row0 + t / g.strands;
        const int strand = g.strands == 2 ? (int)(t & 1) : g.strand0;
        const long long b = g.off[row], e = g.off[row + 1];
        const bool good = b >= 0 && e >= b && e <= g.bytes && e - b <= g.max_qlen;
        const long long L = good ? e - b : 0, nk = L - k + 1;
        const long long i = t0 + threadIdx.x;
        uint8_t *out = g.flags + t * g.max_qlen;
        if (t0 >= nk) { if (i < g.max_qlen) out[i] = 0; return; }          // (the whole workgroup: nothing of the tile has a k-mer)
        pmx_sketch_hashes<C>(PmxSketchRowCodes{g.buf + b, L, strand}, t0, k, w, H, cod);
        if (i >= g.max_qlen) return;
        bool sel = false;
        if (i < nk) {
            const int a = (int)threadIdx.x + halo;
            sel = pmx_sketch_selected(H, a, a - (int)min((long long)halo, i), a + (int)min((long long)halo, nk - 1 - i), (int)min((long long)w, nk));
        }
        out[i] = sel ? 1 : 0;
    } else {
        const long long t0 = (long long)blockIdx.x * T;
        pmx_sketch_hashes<C>(PmxSketchSetCodes{g.buf, g.bytes}, t0, k, w, H, cod);
        const long long p0 = t0 + (long long)threadIdx.x * C;
        if (p0 >= g.bytes) return;
        PmxSeedRegion r = pmx_seed_region(g.off, g.count, p0);
        uint32_t packed = 0;
        const int n = (int)min((long long)C, g.bytes - p0);
        for (int j = 0; j < n; ++j) {
            const long long p = p0 + j;
            (void)pmx_seed_region_advance(r, g.off, g.count, p);
            bool sel = false;
            if (pmx_seed_region_inside(r, g.count, g.bytes, p) && p + k <= r.e) {
                const long long nk = r.e - r.b - k + 1;
                const int a = (int)(p - t0) + halo;
                sel = pmx_sketch_selected(H, a, a - (int)min((long long)halo, p - r.b), a + (int)min((long long)halo, r.e - k - p), (int)min((long long)w, nk));
            }
            packed |= (sel ? 1u : 0u) << (8 * j);
        }
        if (n == C) *(uint32_t *)(g.flags + p0) = packed;                   // p0 is a multiple of 4 and so is the buffer's address
        else for (int j = 0; j < n; ++j) g.flags[p0 + j] = (uint8_t)(packed >> (8 * j));
    }
}

// The compact entries of a minimizer index: pmx_seed_extract_kernel's walk, writing only the flagged positions, each at its scanned
// place at[p] -- input order is buffer order, so the stable sort leaves (kmer, seq, pos) order.
__global__ void __launch_bounds__(256) pmx_seed_scatter_kernel(const uint8_t *__restrict__ buf, const int64_t *__restrict__ off, long long count,
                                                               long long bytes, int k, const uint8_t *__restrict__ flags, const uint32_t *__restrict__ at,
                                                               uint64_t *__restrict__ keys, uint64_t *__restrict__ vals)
{
    const long long p0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * PMX_SEED_TILE;
    if (p0 >= bytes) return;
    const uint64_t mask = ((uint64_t)1 << (2 * k)) - 1;
    PmxSeedRegion g = pmx_seed_region(off, count, p0);
    const long long pend = min(p0 + PMX_SEED_TILE, bytes), xend = min(pend + k - 1, bytes);
    uint64_t key = 0; int run = 0;
    for (long long x = p0; x < xend; ++x) {
        if (pmx_seed_region_advance(g, off, count, x)) run = 0;
        const int c = pmx_seed_region_inside(g, count, bytes, x) ? pmx_seed_code(buf[x]) : -1;
        if (c < 0) { run = 0; key = 0; } else { key = (key << 2) | (uint64_t)c; ++run; }
        const long long s = x - k + 1;
        if (s >= p0 && flags[s] && run >= k && s >= g.b) {
            const uint32_t o = at[s];
            keys[o] = key & mask;
            vals[o] = ((uint64_t)g.r << 32) | (uint64_t)(uint32_t)(s - g.b);
        }
    }
}

struct PmxWidenU8 { __device__ __host__ uint32_t operator()(uint8_t v) const { return (uint32_t)v; } };

void pmx_seed_sketch_tiles(int *row_tile, int *set_tile)
{
    if (row_tile) *row_tile = 256 * PMX_SKETCH_ROW_C;
    if (set_tile) *set_tile = 256 * PMX_SKETCH_SET_C;
}

size_t pmx_seed_sketch_scan_bytes(long long bytes)
{
    size_t temp = 0;
    auto in = rocprim::make_transform_iterator((const uint8_t *)nullptr, PmxWidenU8());
    (void)rocprim::exclusive_scan(nullptr, temp, in, (uint32_t *)nullptr, 0u, (size_t)(bytes + 1), rocprim::plus<uint32_t>(), nullptr);
    return temp + 256;
}

// flags: bytes + 1 bytes (the last one zeroed here: the scan's total), 4-byte aligned; at: bytes + 1 places, at[bytes] = the entries
int pmx_launch_seed_sketch_set(const uint8_t *buf, const int64_t *off, long long count, long long bytes, int k, int w, uint8_t *flags, uint32_t *at,
                               void *temp, size_t temp_bytes, hipStream_t stream)
{
    if (bytes <= 0) return 0;
    if (hipMemsetAsync(flags + bytes, 0, 1, stream) != hipSuccess) return -1;
    PmxSketchArgs g = {};
    g.buf = buf; g.off = off; g.count = count; g.bytes = bytes; g.k = k; g.w = w; g.flags = flags;
    const long long T = 256 * PMX_SKETCH_SET_C;
    hipLaunchKernelGGL(pmx_seed_sketch_kernel<false>, dim3((unsigned)((bytes + T - 1) / T)), dim3(256), 0, stream, g);
    int rc = pmx_launched();
    if (rc) return rc;
    auto in = rocprim::make_transform_iterator((const uint8_t *)flags, PmxWidenU8());
    const hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, in, at, 0u, (size_t)(bytes + 1), rocprim::plus<uint32_t>(), stream);
    return e == hipSuccess ? 0 : -(int)e;
}

// the n > 0 flagged positions as compact entries into keys_in / vals_in, sorted into keys_out / vals_out (n entries each; temp:
// pmx_seed_index_sort_bytes(n, k))
int pmx_launch_seed_index_selected(const uint8_t *buf, const int64_t *off, long long count, long long bytes, int k, const uint8_t *flags,
                                   const uint32_t *at, long long n, uint64_t *keys_in, uint64_t *vals_in, uint64_t *keys_out, uint64_t *vals_out,
                                   void *temp, size_t temp_bytes, hipStream_t stream)
{
    if (bytes <= 0 || n <= 0) return 0;
    const long long threads = (bytes + PMX_SEED_TILE - 1) / PMX_SEED_TILE;
    hipLaunchKernelGGL(pmx_seed_scatter_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, buf, off, count, bytes, k, flags, at,
                       keys_in, vals_in);
    int rc = pmx_launched();
    if (rc) return rc;
    const hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, 2 * k + 1, stream);
    return e == hipSuccess ? 0 : -(int)e;
}

// flags: segs * max_qlen bytes, every one written; segs = rows x strands of the slice (segs x tiles per segment < 2^31)
int pmx_launch_seed_sketch_rows(const uint8_t *qbuf, const int64_t *qoff, long long q_bytes, long long row0, long long segs, int strands, int strand0,
                                int max_qlen, int k, int w, uint8_t *flags, hipStream_t stream)
{
    if (segs <= 0) return 0;
    const int T = 256 * PMX_SKETCH_ROW_C;
    PmxSketchArgs g = {};
    g.buf = qbuf; g.off = qoff; g.bytes = q_bytes; g.row0 = row0; g.strands = strands; g.strand0 = strand0; g.max_qlen = max_qlen;
    g.tiles = (int)(((long long)max_qlen + T - 1) / T); g.k = k; g.w = w; g.flags = flags;
    hipLaunchKernelGGL(pmx_seed_sketch_kernel<true>, dim3((unsigned)(segs * g.tiles)), dim3(256), 0, stream, g);
    return pmx_launched();
}

// ---- seeding -------------------------------------------------------------------------------------------------------------------------
// The index's entries of `key`: lo = the first one, cnt = how many; 0 / 0 where the k-mer is absent or occurs more than max_occ times.
// One read of the bucket table, a lower bound inside the bucket, the probe at lo + max_occ, an upper bound below it.
__device__ __forceinline__ void pmx_seed_lookup(uint64_t key, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ bucket, int shift,
                                                int max_occ, uint32_t &lo, uint32_t &cnt)
{
    const uint32_t s = bucket[key >> shift], t1 = bucket[(key >> shift) + 1];
    uint32_t a = s, z = t1;
    while (a < z) { const uint32_t mid = a + ((z - a) >> 1); if (keys[mid] < key) a = mid + 1; else z = mid; }
    if (a < t1 && keys[a] == key) {
        lo = a;
        const uint32_t lim = (uint32_t)min((unsigned long long)t1, (unsigned long long)a + (unsigned long long)max_occ);
        if (!(lim < t1 && keys[lim] == key)) {                 // (else: more than max_occ occurrences, ignored entirely)
            uint32_t u = a + 1; z = lim;
            while (u < z) { const uint32_t mid = u + ((z - u) >> 1); if (keys[mid] == key) u = mid + 1; else z = mid; }
            cnt = u - a;
        }
    }
}

// Position slot p = (row_local * strands + s) * max_qlen + i.  lo[p]: the first index entry of the slot's k-mer, cnt[p]: its
// occurrences, 0 where the oriented query has no k-mer at i, the k-mer is absent or it occurs more than max_occ times.  cnt has one
// entry more than there are slots (0: the scan's total).  The key comes straight from the row's bytes: no code stage on this road.
__device__ __forceinline__ void pmx_seed_count_slot(const uint8_t *__restrict__ qbuf, const int64_t *__restrict__ qoff, long long q_bytes,
                                                    long long row0, long long slots, int strands, int strand0, int max_qlen, int k,
                                                    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ bucket, int shift,
                                                    int max_occ, const uint8_t *__restrict__ mflag, uint32_t *__restrict__ lo_out,
                                                    uint32_t *__restrict__ cnt_out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = slots * max_qlen;
    if (p > total) return;
    if (p == total) { cnt_out[p] = 0; return; }
    uint32_t lo = 0, cnt = 0;
    if (mflag && !mflag[p]) { lo_out[p] = lo; cnt_out[p] = cnt; return; }      // not a minimizer of the oriented row: no look-up
    const long long t = p / max_qlen;
    const int i = (int)(p - t * max_qlen);
    const long long row = row0 + t / strands;
    const int strand = strands == 2 ? (int)(t & 1) : strand0;
    const long long b = qoff[row], e = qoff[row + 1];
    if (b >= 0 && e >= b && e <= q_bytes && e - b <= max_qlen && i + k <= e - b) {
        const uint8_t *w = qbuf + b;
        const int L = (int)(e - b);
        uint64_t key = 0; bool ok = true;
        for (int x = 0; x < k; ++x) {
            const int c = strand ? pmx_seed_code(w[L - 1 - (i + x)]) : pmx_seed_code(w[i + x]);
            ok = ok && c >= 0;
            key = (key << 2) | (uint64_t)((strand ? 3 - c : c) & 3);
        }
        if (ok) pmx_seed_lookup(key, keys, bucket, shift, max_occ, lo, cnt);
    }
    lo_out[p] = lo; cnt_out[p] = cnt;
}
__global__ void __launch_bounds__(256) pmx_seed_count_kernel(const uint8_t *__restrict__ qbuf, const int64_t *__restrict__ qoff, long long q_bytes,
                                                             long long row0, long long slots, int strands, int strand0, int max_qlen, int k,
                                                             const uint64_t *__restrict__ keys, const uint32_t *__restrict__ bucket, int shift,
                                                             int max_occ, uint32_t *__restrict__ lo_out, uint32_t *__restrict__ cnt_out)
{
    pmx_seed_count_slot(qbuf, qoff, q_bytes, row0, slots, strands, strand0, max_qlen, k, keys, bucket, shift, max_occ, nullptr, lo_out, cnt_out);
}
// The flagged form (a minimizer index, w > 1): mflag[p] is the row form's byte of the slot (pmx_seed_sketch_kernel); a slot whose flag is
// 0 writes lo = cnt = 0 without a look-up.
__global__ void __launch_bounds__(256) pmx_seed_count_flagged_kernel(const uint8_t *__restrict__ qbuf, const int64_t *__restrict__ qoff, long long q_bytes,
                                                                     long long row0, long long slots, int strands, int strand0, int max_qlen, int k,
                                                                     const uint64_t *__restrict__ keys, const uint32_t *__restrict__ bucket, int shift,
                                                                     int max_occ, const uint8_t *__restrict__ mflag, uint32_t *__restrict__ lo_out,
                                                                     uint32_t *__restrict__ cnt_out)
{
    pmx_seed_count_slot(qbuf, qoff, q_bytes, row0, slots, strands, strand0, max_qlen, k, keys, bucket, shift, max_occ, mflag, lo_out, cnt_out);
}

// out[0] = the largest m <= rows whose matches moff[m * stride] fit `cap`; out[1] = that number of matches
__global__ void pmx_seed_cut_kernel(const int64_t *__restrict__ moff, long long rows, long long stride, long long cap, int64_t *out)
{
    long long a = 0, z = rows;                  // moff[a * stride] <= cap holds for a == 0
    while (a < z) { const long long mid = (a + z + 1) >> 1; if (moff[mid * stride] <= cap) a = mid; else z = mid - 1; }
    out[0] = a; out[1] = moff[a * stride];
}

// A match key: (id << 32) | the diagonal, biased so that the keys sort by (id, diagonal).
__device__ __forceinline__ uint64_t pmx_seed_key(uint64_t id, long long d) { return (id << 32) | (uint64_t)((uint32_t)(int32_t)d ^ 0x80000000u); }

// The match key of index value v met at position i of orientation slot t = p / max_qlen (G: PmxSeedGeom; count: the set's sequences).
// DNA, FRAMES: v = r << 32 | j, the key's id is r and its diagonal d = j - i, in letters of the index.
// CODONS: the nucleotide diagonal D = 3 j - (off + 3 i), off = the slot's frame % 3 = its orientation slot % 3 (orients is 3 or 6 and
//   `first` 0 or 3 there).  |D| < 2^31 by the slot's i < 2^31 / 3 and the index's j < 2^29.
// A translated index: v = (s * count + r) << 32 | x.  REF_FRAMES: id = g * count + r with the sequence frame g = 3 s + x % 3, and the
//   diagonal d = x / 3 - i in letters.  REF_CODONS: id = s * count + r and the nucleotide diagonal D = x - 3 i.  |d| < 2^31 by
//   x < 2^30 and 3 i < 2^31 (a row's worst case fits the match buffer).
template <int G>
__device__ __forceinline__ uint64_t pmx_seed_match_key(uint64_t v, long long t, long long i, long long count)
{
    const long long j = (long long)(uint32_t)v, id0 = (long long)(v >> 32);
    if (G == PMX_SEED_GEOM_CODONS) return pmx_seed_key((uint64_t)id0, 3 * j - ((long long)(t % 3) + 3 * i));
    if (G == PMX_SEED_GEOM_REF_CODONS) return pmx_seed_key((uint64_t)id0, j - 3 * i);
    if (G == PMX_SEED_GEOM_REF_FRAMES) {
        const long long s = id0 >= count ? 1 : 0;
        return pmx_seed_key((uint64_t)((3 * s + j % 3) * count + (id0 - s * count)), j / 3 - i);
    }
    return pmx_seed_key((uint64_t)id0, j - i);
}

// the matches of position slot p, behind moff[p].  CHAIN (a DNA index): the key is the index value itself, r << 32 | j, and the match's
// i goes beside it into mvals -- anchors sort by (r, j), not by diagonal.
template <int G, bool CHAIN = false>
__global__ void __launch_bounds__(256) pmx_seed_emit_kernel(long long total, int max_qlen, long long count, const uint32_t *__restrict__ lo,
                                                            const uint32_t *__restrict__ cnt, const int64_t *__restrict__ moff,
                                                            const uint64_t *__restrict__ vals, uint64_t *__restrict__ mkeys,
                                                            uint32_t *__restrict__ mvals)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const uint32_t n = cnt[p];
    if (!n) return;
    const long long t = p / max_qlen;
    const long long i = p - t * max_qlen;
    const uint32_t first = lo[p];
    const int64_t at = moff[p];
    uint64_t *out = mkeys + at;
    if (CHAIN) for (uint32_t x = 0; x < n; ++x) { out[x] = vals[first + x]; mvals[at + x] = (uint32_t)i; }
    else for (uint32_t x = 0; x < n; ++x) out[x] = pmx_seed_match_key<G>(vals[first + x], t, i, count);
}

// segment t of the sort: the matches of (row, strand) slot t
struct PmxSeedSegOff {
    const int64_t *moff; long long stride;
    __device__ __host__ unsigned operator()(unsigned t) const { return (unsigned)moff[(long long)t * stride]; }
};

__device__ __forceinline__ int32_t pmx_seed_diag(uint64_t key) { return (int32_t)((uint32_t)key ^ 0x80000000u); }

// flag[x] = 1 where a (row, strand) segment starts (flag zeroed before)
__global__ void __launch_bounds__(256) pmx_seed_segstart_kernel(const int64_t *__restrict__ moff, long long slots, long long stride, uint32_t *flag)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= slots) return;
    const int64_t a = moff[t * stride], z = moff[(t + 1) * stride];
    if (z > a) flag[a] = 1;
}

// head[x] = x where match x opens a cluster (a new segment, another reference, a diagonal more than `band` past the previous one), else 0
__global__ void __launch_bounds__(256) pmx_seed_heads_kernel(const uint64_t *__restrict__ mkeys, long long m, int band, const uint32_t *__restrict__ segstart,
                                                             uint32_t *__restrict__ head)
{
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= m) return;
    bool h = x == 0 || segstart[x] != 0;
    if (!h) {
        const uint64_t a = mkeys[x - 1], b = mkeys[x];
        h = (a >> 32) != (b >> 32) || (long long)pmx_seed_diag(b) - (long long)pmx_seed_diag(a) > band;
    }
    head[x] = h ? (uint32_t)x : 0u;
}

// head: after the max-scan, the index of the head of x's cluster.  flag[x] = 1 where x closes a cluster of at least min_seeds matches.
__global__ void __launch_bounds__(256) pmx_seed_flags_kernel(const uint32_t *__restrict__ head, long long m, int min_seeds, uint32_t *__restrict__ flag)
{
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= m) return;
    const bool tail = x == m - 1 || head[x + 1] == (uint32_t)(x + 1);
    flag[x] = tail && x - (long long)head[x] + 1 >= min_seeds ? 1u : 0u;
}

// floor(a / 3) for either sign
__device__ __forceinline__ long long pmx_seed_floor3(long long a) { return a >= 0 ? a / 3 : -((2 - a) / 3); }

// What the hits kernel hands a geometry besides the cluster: the rows' layout of the plan and the two sets' offsets.
struct PmxSeedWindowArgs {
    long long row0; int segs, first; bool rows_translated; long long count; int pad;
    const int64_t *__restrict__ qoff, *__restrict__ roff;
};
struct PmxSeedWindow { long long row, r, beg, end; int byte, reserved; };

// The candidate of a closed cluster: segment a of the slice, id of its match keys, diagonals dmin .. dmax (G: PmxSeedGeom).
// DNA, FRAMES: a segment is (row, orientation); byte = the strand / the frame (0 where the rows are letters); the window from the
//   letter diagonals and the oriented row's letters L: its bytes, or the translation's length (W - frame % 3) / 3.
// CODONS: a segment is (row, strand), three frames wide; byte = the strand (`first` is the first FRAME, 0 or 3); the window from the
//   nucleotide diagonals and W, in letters of the reference.
// A translated index, a segment is a row of m letters, N = len(r).  REF_FRAMES: id = g * count + r; the letter window [lb, le) =
//   [max(0, d_min - pad), min((N - g % 3) / 3, d_max + m + pad)) of frame g as stored nucleotides, codon-aligned: [g % 3 + 3 lb,
//   g % 3 + 3 le) on strand 0, [N - g % 3 - 3 le, N - g % 3 - 3 lb) on strand 1, so the frame byte relative to the window is 0 or 3;
//   reserved = g.  REF_CODONS: id = s * count + r; the oriented window [max(0, D_min - pad), min(N, D_max + 3 m + pad)), stored
//   [lo, hi) or [N - hi, N - lo); byte = s.
template <int G>
__device__ __forceinline__ PmxSeedWindow pmx_seed_window(const PmxSeedWindowArgs &g, long long a, long long id, long long dmin, long long dmax)
{
    PmxSeedWindow w; w.reserved = 0;
    if (G == PMX_SEED_GEOM_REF_FRAMES || G == PMX_SEED_GEOM_REF_CODONS) {
        w.row = g.row0 + a;
        const long long o = id / g.count;       // the sequence frame g (REF_FRAMES), the strand (REF_CODONS)
        w.r = id - o * g.count;
        const long long len = g.qoff[w.row + 1] - g.qoff[w.row], N = g.roff[w.r + 1] - g.roff[w.r];
        if (G == PMX_SEED_GEOM_REF_CODONS) {
            const long long wlo = max(0ll, dmin - g.pad), whi = min(N, dmax + 3 * len + g.pad);
            w.beg = o ? N - whi : wlo; w.end = o ? N - wlo : whi;
            w.byte = (int)o;
        } else {
            const long long ph = o % 3, lb = max(0ll, dmin - g.pad), le = min((N - ph) / 3, dmax + len + g.pad);
            w.beg = o >= 3 ? N - ph - 3 * le : ph + 3 * lb; w.end = o >= 3 ? N - ph - 3 * lb : ph + 3 * le;
            w.byte = o >= 3 ? 3 : 0; w.reserved = (int)o;
        }
        return w;
    }
    w.row = g.row0 + a / g.segs; w.r = id;
    w.byte = (G == PMX_SEED_GEOM_CODONS ? g.first / 3 : g.first) + (int)(a % g.segs);
    const long long W = g.qoff[w.row + 1] - g.qoff[w.row], rlen = g.roff[w.r + 1] - g.roff[w.r];
    if (G == PMX_SEED_GEOM_CODONS) {
        w.beg = max(0ll, pmx_seed_floor3(dmin) - g.pad);
        w.end = min(rlen, pmx_seed_floor3(dmax + W - 1) + 1 + g.pad);
    } else {
        const long long L = g.rows_translated ? (W - w.byte % 3) / 3 : W;
        w.beg = max(0ll, dmin - g.pad);
        w.end = min(rlen, dmax + L + g.pad);
    }
    return w;
}

// candidate tails -> outputs at base + pos[x], below `capacity`; base = counts[0], the candidates of the slices before.  The
// segments: `slots` of them, `stride` position slots each.
template <int G>
__global__ void __launch_bounds__(256) pmx_seed_hits_kernel(const uint64_t *__restrict__ mkeys, const uint32_t *__restrict__ head, const uint32_t *__restrict__ pos,
                                                            long long m, const int64_t *__restrict__ moff, long long slots, long long stride,
                                                            PmxSeedWindowArgs g, const int64_t *__restrict__ counts, long long capacity,
                                                            pmx_pair_t *__restrict__ hit_pairs, uint8_t *__restrict__ hit_byte, pmx_seed_hit_t *__restrict__ hit_seeds)
{
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= m || pos[x + 1] == pos[x]) return;
    const long long at = counts[0] + (long long)pos[x];
    if (at >= capacity) return;
    long long a = 0, z = slots - 1;             // the segment of x: the last t with moff[t * stride] <= x (empty segments share a start)
    while (a < z) { const long long mid = (a + z + 1) >> 1; if (moff[mid * stride] <= x) a = mid; else z = mid - 1; }
    const uint32_t h = head[x];
    const uint64_t kh = mkeys[h], kt = mkeys[x];
    const long long dmin = pmx_seed_diag(kh), dmax = pmx_seed_diag(kt);
    const PmxSeedWindow w = pmx_seed_window<G>(g, a, (long long)(kt >> 32), dmin, dmax);
    pmx_pair_t pr; pr.q = w.row; pr.r = w.r; pr.q_beg = 0; pr.q_len = -1; pr.r_beg = (int32_t)w.beg; pr.r_len = (int32_t)(w.end - w.beg);
    hit_pairs[at] = pr;
    hit_byte[at] = (uint8_t)w.byte;
    if (hit_seeds) { pmx_seed_hit_t s; s.n_seeds = (int32_t)(x - h + 1); s.diag_min = (int32_t)dmin; s.diag_max = (int32_t)dmax; s.reserved = w.reserved; hit_seeds[at] = s; }
}

// row_off[x + 1] = base + the candidates of the slice's rows 0 .. x (pos == NULL: the slice has no match)
__global__ void __launch_bounds__(256) pmx_seed_rowoff_kernel(const uint32_t *__restrict__ pos, const int64_t *__restrict__ moff, long long rows, long long stride,
                                                              const int64_t *__restrict__ counts, int64_t *__restrict__ row_off)
{
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= rows) return;
    row_off[x + 1] = counts[0] + (pos ? (int64_t)pos[moff[(x + 1) * stride]] : 0);
}

// behind the slice: counts[0] += its candidates, counts[1] = what is written so far
__global__ void pmx_seed_advance_kernel(const uint32_t *pos, long long m, long long capacity, int64_t *counts)
{
    const int64_t total = counts[0] + (pos ? (int64_t)pos[m] : 0);
    counts[0] = total; counts[1] = total < capacity ? total : capacity;
}

struct PmxMaxU32 { __device__ __host__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct PmxWidenU32 { __device__ __host__ int64_t operator()(uint32_t v) const { return (int64_t)v; } };

// rocPRIM scratch of one slice: the scan over `positions` + 1 slot counts, the sort of `matches` keys in `slots` segments, the two scans
// over the matches -- used one after the other, so the largest counts
size_t pmx_seed_temp_bytes(long long positions, long long matches, long long slots, bool chain)
{
    size_t a = 0, b = 0, c = 0, d = 0;
    auto in = rocprim::make_transform_iterator((const uint32_t *)nullptr, PmxWidenU32());
    (void)rocprim::exclusive_scan(nullptr, a, in, (int64_t *)nullptr, (int64_t)0, (size_t)(positions + 1), rocprim::plus<int64_t>(), nullptr);
    auto seg = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0u), PmxSeedSegOff{nullptr, 1});
    (void)rocprim::segmented_radix_sort_keys(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (unsigned)matches, (unsigned)slots, seg, seg, 0, 64,
                                             nullptr);
    if (chain) {                                // a chaining run sorts (key, i) pairs in place of keys
        size_t bp = 0;
        (void)rocprim::segmented_radix_sort_pairs(nullptr, bp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                  (unsigned)matches, (unsigned)slots, seg, seg, 0, 64, nullptr);
        b = std::max(b, bp);
    }
    (void)rocprim::inclusive_scan(nullptr, c, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)matches, PmxMaxU32(), nullptr);
    (void)rocprim::exclusive_scan(nullptr, d, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)(matches + 1), rocprim::plus<uint32_t>(), nullptr);
    return std::max(std::max(a, b), std::max(c, d)) + 256;
}

// ---- letters: a protein index over a reduced alphabet, proteins or translated reads as queries --------------------------
// The index is the DNA one with a run-time number of bits per letter and the letter's group read from a 256-byte table staged in LDS.
// Seeding adds one stage in front of the count pass: a code byte per position slot -- the group of the letter there, 255 where there
// is none -- so that a codon is read and translated once per frame and the count pass forms its keys from k code bytes.  A position
// slot is p = ((row_local * orients) + o) * max_qlen + i; orientation o of a row is frame `first` + o (rows that are letters: the row
// itself).  The codon modes' (row, strand, frame, i) is the same number with orients = 3 strands: only the segments of the sort differ,
// three frames wide there, and with them the geometry (pmx_seed_match_key, pmx_seed_window).

// keys[p] / vals[p] for every p < bytes, as pmx_seed_extract_kernel: `bits` bits per letter, table[b] = the group of byte b or 255
__global__ void __launch_bounds__(256) pmx_seedl_extract_kernel(const uint8_t *__restrict__ buf, const int64_t *__restrict__ off, long long count,
                                                                long long bytes, int k, int bits, const uint8_t *__restrict__ table,
                                                                uint64_t *__restrict__ keys, uint64_t *__restrict__ vals, unsigned long long *n_valid)
{
    __shared__ uint8_t grp[256];
    __shared__ unsigned total;
    grp[threadIdx.x] = table[threadIdx.x];
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const long long p0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * PMX_SEED_TILE;
    unsigned found = 0;
    if (p0 < bytes) {
        const uint64_t invalid = (uint64_t)1 << (k * bits), mask = invalid - 1;
        PmxSeedRegion g = pmx_seed_region(off, count, p0);
        const long long pend = min(p0 + PMX_SEED_TILE, bytes), xend = min(pend + k - 1, bytes);
        uint64_t key = 0; int run = 0;
        for (long long x = p0; x < xend; ++x) {
            if (pmx_seed_region_advance(g, off, count, x)) run = 0;
            const uint32_t c = pmx_seed_region_inside(g, count, bytes, x) ? (uint32_t)grp[buf[x]] : 255u;
            if (c == 255u) { run = 0; key = 0; } else { key = (key << bits) | (uint64_t)c; ++run; }
            const long long s = x - k + 1;
            if (s >= p0) {
                const bool have = run >= k && s >= g.b;
                keys[s] = have ? (key & mask) : invalid;
                vals[s] = have ? ((uint64_t)g.r << 32) | (uint64_t)(uint32_t)(s - g.b) : (uint64_t)s;
                found += have ? 1u : 0u;
            }
        }
        pmx_seed_no_kmers(keys, vals, 0, max(p0, xend - k + 1), pend, invalid);
    }
    pmx_seed_block_sum(total, found, n_valid);
}

size_t pmx_seed_index_sort_bytes_letters(long long bytes, int k, int bits)
{
    size_t temp = 0;
    uint64_t *nul = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, temp, nul, nul, nul, nul, (size_t)bytes, 0, k * bits + 1, nullptr);
    return temp + 256;
}

int pmx_launch_seed_index_letters(const uint8_t *buf, const int64_t *off, long long count, long long bytes, int k, int bits, const uint8_t *table,
                                  uint64_t *keys_in, uint64_t *vals_in, uint64_t *keys_out, uint64_t *vals_out, void *temp, size_t temp_bytes,
                                  unsigned long long *n_valid, hipStream_t stream)
{
    if (bytes <= 0) return 0;
    const long long threads = (bytes + PMX_SEED_TILE - 1) / PMX_SEED_TILE;
    hipLaunchKernelGGL(pmx_seedl_extract_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, buf, off, count, bytes, k, bits, table,
                       keys_in, vals_in, n_valid);
    int rc = pmx_launched();
    if (rc) return rc;
    const hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)bytes, 0, k * bits + 1, stream);
    return e == hipSuccess ? 0 : -(int)e;
}

// base -> its class in the genetic code's order T/U 0, C 1, A 2, G 3 (either case); 4: not a nucleotide
__device__ __forceinline__ uint32_t pmx_seedl_base(uint32_t b)
{
    const uint32_t u = b & 0xDFu;
    return u == 'T' || u == 'U' ? 0u : u == 'C' ? 1u : u == 'A' ? 2u : u == 'G' ? 3u : 4u;
}

// codes[p] for every position slot of the slice.  Rows that are letters (translated false): the slot's letter is the row's byte i.
// Else the slot's frame is f = first + o, off = f % 3, and its letter is the codon at bytes off + 3 i .. of the row as stored (f < 3) or
// of its reverse complement (f >= 3): the three bytes at W - 1 - (off + 3 i) downwards, complemented by the index ^ 42 -- nothing is
// materialised.  A codon with a byte that is no nucleotide is X.  The letter goes through the index's table.  255: no letter there
// (behind the translation's end, a bad row, a row whose W / 3 (rows that are letters: W) exceeds max_qlen) or a letter outside the alphabet.
__global__ void __launch_bounds__(256) pmx_seedl_codes_kernel(const uint8_t *__restrict__ qbuf, const int64_t *__restrict__ qoff, long long q_bytes,
                                                              long long row0, long long total, int orients, int first, bool translated, int max_qlen,
                                                              const uint8_t *__restrict__ table, PmxCodeTable code, uint8_t *__restrict__ codes)
{
    __shared__ uint8_t grp[256];
    __shared__ uint8_t cod[64];
    grp[threadIdx.x] = table[threadIdx.x];
    if (threadIdx.x < 64) cod[threadIdx.x] = code.v[threadIdx.x];
    __syncthreads();
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const long long t = p / max_qlen;
    const long long i = p - t * max_qlen;
    const long long row = row0 + t / orients;
    const long long b = qoff[row], e = qoff[row + 1];
    uint32_t c = 255u;
    if (b >= 0 && e >= b && e <= q_bytes) {
        const long long W = e - b;
        const uint8_t *w = qbuf + b;
        if (!translated) {
            if (W <= max_qlen && i < W) c = grp[w[i]];
        } else {
            const int f = first + (int)(t % orients), off = f % 3;
            const long long x = off + 3 * i;
            if (W / 3 <= max_qlen && x + 3 <= W) {
                uint32_t b0, b1, b2, flip;
                if (f < 3) { b0 = w[x]; b1 = w[x + 1]; b2 = w[x + 2]; flip = 0u; }
                else { b0 = w[W - 1 - x]; b1 = w[W - 2 - x]; b2 = w[W - 3 - x]; flip = 42u; }
                const uint32_t idx = (pmx_seedl_base(b0) << 4) | (pmx_seedl_base(b1) << 2) | pmx_seedl_base(b2);
                const bool ok = (pmx_seedl_base(b0) | pmx_seedl_base(b1) | pmx_seedl_base(b2)) < 4u;
                c = grp[ok ? (uint32_t)cod[(idx & 63u) ^ flip] : (uint32_t)'X'];
            }
        }
    }
    codes[p] = (uint8_t)c;
}

// pmx_seed_count_kernel with the key formed from the slot's k code bytes (they end at the slot's orientation: i + k <= max_qlen)
__global__ void __launch_bounds__(256) pmx_seedl_count_kernel(const uint8_t *__restrict__ codes, long long total, int max_qlen, int k, int bits,
                                                              const uint64_t *__restrict__ keys, const uint32_t *__restrict__ bucket, int shift,
                                                              int max_occ, uint32_t *__restrict__ lo_out, uint32_t *__restrict__ cnt_out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > total) return;
    if (p == total) { cnt_out[p] = 0; return; }
    const int i = (int)(p % max_qlen);
    uint32_t lo = 0, cnt = 0;
    if (i + k <= max_qlen && codes[p] != 255) {
        uint64_t key = 0; bool ok = true;
        for (int x = 0; x < k; ++x) {
            const uint32_t c = codes[p + x];
            ok = ok && c != 255u;
            key = (key << bits) | (uint64_t)(c & 31u);
        }
        if (ok) pmx_seed_lookup(key, keys, bucket, shift, max_occ, lo, cnt);
    }
    lo_out[p] = lo; cnt_out[p] = cnt;
}

// ---- translated references: a six-frame index of a nucleotide set, proteins as queries ---------------------------------
// An oriented position x of sequence r on strand s (0: as stored, 1: reverse-complemented, read from the end downwards through the
// complement, nothing materialised) starts the codon of oriented bytes x .. x + 2; the k-mer at x is the k codons' letters at x, x + 3,
// ..., so the index holds the k-mers of all three frames of a strand and x % 3 is the frame's offset.  Entry slot of (s, r, x):
// s_local * bytes + off[r] + x -- the stable sort then leaves (kmer, s, r, x) order with nothing compacted.  Seeding runs the letters
// road's code stage and count pass on the protein rows; the REF geometries carry the mode's id, diagonal and window.
#define PMX_SEEDT_TILE 48       // slots per thread: a multiple of 3, so a slot's phase is its place in the step unrolled by three

// keys[sl * bytes + p] / vals[..] for every p < bytes of the nstr strands held (strand of sl: strand0 + sl); *n_valid += the k-mers.
// A thread owns one strand and PMX_SEEDT_TILE slots, reads 3 k - 1 bytes past them and rolls one key per phase: each byte enters a
// rolling 6-bit codon index once, the codon's letter goes through the genetic code and the table (both in LDS), and the key of that
// phase takes it.  Strand 1 rolls the stored bytes' classes and complements the index by ^ 42, as pmx_seedl_codes_kernel.  'X' (a
// byte that is no nucleotide), '*' and the table's 255 break a k-mer; so does a sequence end.  Offsets are read at 0 .. count only and
// a byte only below `bytes`.
__global__ void __launch_bounds__(256) pmx_seedt_extract_kernel(const uint8_t *__restrict__ buf, const int64_t *__restrict__ off, long long count,
                                                                long long bytes, int k, int bits, const uint8_t *__restrict__ table, PmxCodeTable code,
                                                                int nstr, int strand0, long long tiles, uint64_t *__restrict__ keys,
                                                                uint64_t *__restrict__ vals, unsigned long long *n_valid)
{
    __shared__ uint8_t grp[256];
    __shared__ uint8_t cod[64];
    __shared__ unsigned total;
    grp[threadIdx.x] = table[threadIdx.x];
    if (threadIdx.x < 64) cod[threadIdx.x] = code.v[threadIdx.x];
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long sl = t / tiles, p0 = (t - sl * tiles) * PMX_SEEDT_TILE;
    unsigned found = 0;
    if (sl < nstr && p0 < bytes) {
        const int strand = strand0 + (int)sl;
        const uint32_t flip = strand ? 42u : 0u;
        const uint64_t invalid = (uint64_t)1 << (k * bits), mask = invalid - 1, id0 = (uint64_t)strand * (uint64_t)count;
        const long long span = 3ll * k - 1, base = sl * bytes;
        PmxSeedRegion g = pmx_seed_region(off, count, p0);
        const long long pend = min(p0 + PMX_SEEDT_TILE, bytes), xend = min(pend + span, bytes);
        uint64_t key0 = 0, key1 = 0, key2 = 0;
        int run0 = 0, run1 = 0, run2 = 0, nrun = 0;
        uint32_t c6 = 0;
        long long x = p0;
        // one slot of the walk: the byte at x closes the codon that starts at x - 2, whose letter the phase's key takes.  An invalid
        // letter is not cleared out of the key (pmx_seedl_extract_kernel zeroes it): its bits go in as g & 31 and RUN = 0, and a slot is
        // valid again only after k further letters of the phase, which shift them above `mask`.  No `s >= b` test either: every run is
        // reset at a sequence end, so RUN >= k means k codons of this phase inside the sequence, the first of them at s
#define PMX_SEEDT_STEP(KEY, RUN)                                                                                                        \
        if (x < xend) {                                                                                                                 \
            if (pmx_seed_region_advance(g, off, count, x)) { nrun = 0; run0 = run1 = run2 = 0; }                                        \
            const bool inside = pmx_seed_region_inside(g, count, bytes, x);                                                             \
            const uint32_t cls = inside ? pmx_seedl_base(buf[strand ? g.b + g.e - 1 - x : x]) : 4u;                                     \
            nrun = cls > 3u ? 0 : nrun + 1;                                                                                             \
            c6 = ((c6 << 2) | (cls & 3u)) & 63u;                                                                                        \
            const uint32_t letter = cod[c6 ^ flip];                                                                                     \
            const uint32_t grpl = nrun >= 3 && letter != (uint32_t)'X' && letter != (uint32_t)'*' ? (uint32_t)grp[letter] : 255u;       \
            KEY = (KEY << bits) | (uint64_t)(grpl & 31u);                                                                               \
            RUN = grpl == 255u ? 0 : RUN + 1;                                                                                           \
            const long long s = x - span;                                                                                               \
            if (s >= p0) {                                                                                                              \
                const bool have = RUN >= k;                                                                                             \
                keys[base + s] = have ? (KEY & mask) : invalid;                                                                         \
                vals[base + s] = have ? ((id0 + (uint64_t)g.r) << 32) | (uint64_t)(uint32_t)(s - g.b) : (uint64_t)(base + s);           \
                found += have ? 1u : 0u;                                                                                                \
            }                                                                                                                           \
            ++x;                                                                                                                        \
        }
        while (x < xend) { PMX_SEEDT_STEP(key0, run0) PMX_SEEDT_STEP(key1, run1) PMX_SEEDT_STEP(key2, run2) }
#undef PMX_SEEDT_STEP
        pmx_seed_no_kmers(keys + base, vals + base, base, max(p0, xend - span), pend, invalid);
    }
    pmx_seed_block_sum(total, found, n_valid);
}

// keys_in / vals_in / keys_out / vals_out: nstr * bytes entry slots each
int pmx_launch_seed_index_translated(const uint8_t *buf, const int64_t *off, long long count, long long bytes, int k, int bits, const uint8_t *table,
                                     const PmxCodeTable &code, int nstr, int strand0, uint64_t *keys_in, uint64_t *vals_in, uint64_t *keys_out,
                                     uint64_t *vals_out, void *temp, size_t temp_bytes, unsigned long long *n_valid, hipStream_t stream)
{
    if (bytes <= 0) return 0;
    const long long tiles = (bytes + PMX_SEEDT_TILE - 1) / PMX_SEEDT_TILE, threads = tiles * nstr;
    hipLaunchKernelGGL(pmx_seedt_extract_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, buf, off, count, bytes, k, bits, table,
                       code, nstr, strand0, tiles, keys_in, vals_in, n_valid);
    int rc = pmx_launched();
    if (rc) return rc;
    const hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)(bytes * nstr), 0, k * bits + 1, stream);
    return e == hipSuccess ? 0 : -(int)e;
}

// ---- a slice of a seeding run, by its plan (pmx_common.h: PmxSeedPlan) ---------------------------------------------------------------
// The slice's count pass, scan and cut: rows row0 .. row0 + rows of Q; s.cut (device, 2 entries) receives how many of them fit p.cap_m
// matches and their matches.  A DNA index forms its keys from the rows' bytes; the others from the code stage's bytes.
int pmx_launch_seed_count(const PmxSeedPlan &p, const PmxSeedSlice &s, const PmxSeedSource &src, long long row0, long long rows, hipStream_t stream)
{
    const long long total = rows * p.row_slots;
    const dim3 cb((unsigned)((total + 1 + 255) / 256));
    int rc = 0;
    if (p.kind == PMX_SEED_KIND_DNA && p.w > 1) {           // a minimizer index: the rows' own minimizers first, then only their look-ups
        if ((rc = pmx_launch_seed_sketch_rows(src.qbuf, src.qoff, src.q_bytes, row0, rows * p.orients, p.orients, p.first, p.max_qlen, p.k, p.w, s.mflag, stream)))
            return rc;
        hipLaunchKernelGGL(pmx_seed_count_flagged_kernel, cb, dim3(256), 0, stream, src.qbuf, src.qoff, src.q_bytes, row0, rows * p.orients, p.orients, p.first,
                           p.max_qlen, p.k, src.keys, src.bucket, src.shift, p.max_occ, (const uint8_t *)s.mflag, s.lo, s.cnt);
    } else if (p.kind == PMX_SEED_KIND_DNA)
        hipLaunchKernelGGL(pmx_seed_count_kernel, cb, dim3(256), 0, stream, src.qbuf, src.qoff, src.q_bytes, row0, rows * p.orients, p.orients, p.first,
                           p.max_qlen, p.k, src.keys, src.bucket, src.shift, p.max_occ, s.lo, s.cnt);
    else {
        hipLaunchKernelGGL(pmx_seedl_codes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src.qbuf, src.qoff, src.q_bytes, row0, total,
                           p.orients, p.first, p.rows_translated, p.max_qlen, src.table, p.code, s.codes);
        if ((rc = pmx_launched())) return rc;
        hipLaunchKernelGGL(pmx_seedl_count_kernel, cb, dim3(256), 0, stream, (const uint8_t *)s.codes, total, p.max_qlen, p.k, p.bits, src.keys, src.bucket,
                           src.shift, p.max_occ, s.lo, s.cnt);
    }
    if ((rc = pmx_launched())) return rc;
    auto in = rocprim::make_transform_iterator((const uint32_t *)s.cnt, PmxWidenU32());
    size_t tb = s.temp_bytes;
    const hipError_t e = rocprim::exclusive_scan(s.temp, tb, in, s.moff, (int64_t)0, (size_t)(total + 1), rocprim::plus<int64_t>(), stream);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(pmx_seed_cut_kernel, dim3(1), dim3(1), 0, stream, (const int64_t *)s.moff, rows, p.row_slots, p.cap_m, s.cut);
    return pmx_launched();
}

// Between emit and hits, whatever the geometry: the m matches of s.keys_a sorted per segment (`segs` segments of p.seg_slots position
// slots each) into s.keys_b, head[x] = the head of x's cluster, flag[x + 1] - flag[x] = 1 where x closes a candidate (flag: m + 1 entries).
static int pmx_seed_sort_clusters(const PmxSeedPlan &p, const PmxSeedSlice &s, long long m, long long segs, hipStream_t stream)
{
    int rc = 0;
    const unsigned mb = (unsigned)((m + 255) / 256);
    auto seg = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0u), PmxSeedSegOff{s.moff, p.seg_slots});
    size_t tb = s.temp_bytes;
    hipError_t e = rocprim::segmented_radix_sort_keys(s.temp, tb, (const uint64_t *)s.keys_a, s.keys_b, (unsigned)m, (unsigned)segs, seg, seg + 1, 0, p.key_bits,
                                                      stream);
    if (e != hipSuccess) return -(int)e;
    if (hipMemsetAsync(s.flag, 0, sizeof(uint32_t) * (size_t)(m + 1), stream) != hipSuccess) return -1;
    hipLaunchKernelGGL(pmx_seed_segstart_kernel, dim3((unsigned)((segs + 255) / 256)), dim3(256), 0, stream, (const int64_t *)s.moff, segs, p.seg_slots, s.flag);
    if ((rc = pmx_launched())) return rc;
    hipLaunchKernelGGL(pmx_seed_heads_kernel, dim3(mb), dim3(256), 0, stream, (const uint64_t *)s.keys_b, m, p.band, (const uint32_t *)s.flag, s.head);
    if ((rc = pmx_launched())) return rc;
    tb = s.temp_bytes;
    e = rocprim::inclusive_scan(s.temp, tb, s.head, s.head, (size_t)m, PmxMaxU32(), stream);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(pmx_seed_flags_kernel, dim3(mb), dim3(256), 0, stream, (const uint32_t *)s.head, m, p.min_seeds, s.flag);
    if ((rc = pmx_launched())) return rc;
    tb = s.temp_bytes;
    e = rocprim::exclusive_scan(s.temp, tb, s.flag, s.flag, 0u, (size_t)(m + 1), rocprim::plus<uint32_t>(), stream);
    return e == hipSuccess ? 0 : -(int)e;
}

// ---- chaining: collinear chains with gap costs in place of diagonal clusters (definitions: include/parasail_amd.h) --------
// The anchors of a (row, strand) segment are its matches sorted by (r, j, i): the key r << 32 | j, the value i.  pmx_seed_chain_kernel
// walks a segment in that order with one wave and leaves f, pred and child per anchor; a thread per anchor then walks back from every
// tail over the kept links (chains are disjoint: m steps in all) and flags the candidates; the scan of the flags, the row offsets and
// the running counts are the cluster road's.  pred and child are anchor numbers of the slice (int32, -1: none; m < 2^31).

// the largest of v over the wave, in every lane: four DPP rotations leave each row of 16 its maximum, four v_readlane the rows'
__device__ __forceinline__ int pmx_seed_wave_max(int v)
{
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x121 /*row_ror:1*/, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x122 /*row_ror:2*/, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x124 /*row_ror:4*/, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x128 /*row_ror:8*/, 0xF, 0xF, true));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// One wave (a workgroup of 64) per segment t = [moff[t * stride], moff[(t + 1) * stride]).  For anchor a the lanes evaluate the
// predecessors a - 1 - lane, in rounds of 64 up to `lookback` and never before the first anchor of a's reference (a change of r empties
// the window).  (j, i, f, child) of the last `ring` >= lookback anchors live in LDS, ring a power of two, anchor b in slot b & (ring - 1):
// slot a & (ring - 1) is read (as a - ring, when lookback == ring) before lane 0 overwrites it with a.
//   * nearest predecessor among equal values: inside a round the lowest lane is the nearest (the first set bit of the ballot), and a
//     later round -- farther anchors -- replaces the best only by a strictly larger value; the same strict > against k takes no link
//     at a value of k.
//   * child: the ring's child of b is the anchor with the largest f among those that chose b so far; anchors arrive in ascending
//     order and replace it only by a strictly larger f, so the smallest wins among equals.  A child is nearer than a than its parent
//     is, so its f is still in the ring.  The child of an anchor goes to memory when the anchor leaves the ring, or at the segment's end.
//   * arithmetic: f <= k x (anchors of a chain) <= 31 x max_qlen < 2^31 (i rises strictly along a chain; max_qlen <= 2^26), cost < 2^28,
//     and dj - di is formed only where both are in 1 .. max_gap <= 2^20: nothing leaves int32.
// The ring is written by lane 0 and read by all lanes of the same wave; the workgroup is that one wave, so the barrier behind the
// write is a wait for the wave's own LDS traffic and orders the two.  The next 64 anchors are loaded, coalesced, while 64 are walked.
__global__ void __launch_bounds__(PMX_SEED_CHAIN_LANES) pmx_seed_chain_kernel(const uint64_t *__restrict__ mkeys, const uint32_t *__restrict__ mvals,
                                                                              const int64_t *__restrict__ moff, long long stride, int k, int band, int max_gap,
                                                                              int lookback, int gap_scale, int ring, int32_t *__restrict__ f_out,
                                                                              int32_t *__restrict__ pred_out, int32_t *__restrict__ child_out)
{
    extern __shared__ int32_t pmx_chain_lds[];
    const long long t = blockIdx.x;
    const int64_t beg = moff[t * stride];
    const int n = (int)(moff[(t + 1) * stride] - beg);
    if (n <= 0) return;
    int32_t *rj = pmx_chain_lds, *ri = rj + ring, *rf = ri + ring, *rc = rf + ring;
    const int lane = (int)threadIdx.x, mask = ring - 1;
    mkeys += beg; mvals += beg; f_out += beg; pred_out += beg; child_out += beg;
    uint64_t nk = lane < n ? mkeys[lane] : 0;
    uint32_t ni = lane < n ? mvals[lane] : 0;
    uint32_t cur_r = 0; int wbeg = 0;                    // the reference of the window and its first anchor
    for (int base = 0; base < n; base += PMX_SEED_CHAIN_LANES) {
        const int rlo = (int)(uint32_t)nk, rhi = (int)(uint32_t)(nk >> 32), ci = (int)ni;
        if (base + PMX_SEED_CHAIN_LANES + lane < n) { nk = mkeys[base + PMX_SEED_CHAIN_LANES + lane]; ni = mvals[base + PMX_SEED_CHAIN_LANES + lane]; }
        const int cnt = min(PMX_SEED_CHAIN_LANES, n - base);
        int myf = 0, mypred = -1;                        // lane x: those of anchor base + x
        for (int x = 0; x < cnt; ++x) {
            const int a = base + x;
            const int ja = __builtin_amdgcn_readlane(rlo, x), ia = __builtin_amdgcn_readlane(ci, x);
            const uint32_t ra = (uint32_t)__builtin_amdgcn_readlane(rhi, x);
            if (a == 0 || ra != cur_r) { cur_r = ra; wbeg = a; }
            const int reach = min(lookback, a - wbeg);
            int best = k, bestb = -1;
            for (int off = 0; off < reach; off += PMX_SEED_CHAIN_LANES) {
                int v = INT32_MIN;
                if (off + lane < reach) {
                    const int s = (a - 1 - off - lane) & mask;
                    const int dj = ja - rj[s], di = ia - ri[s];
                    const bool near = dj >= 1 && di >= 1 && dj <= max_gap && di <= max_gap;
                    const int g = near ? abs(dj - di) : 0;
                    if (near && g <= band) v = rf[s] + min(min(di, dj), k) - pmx_seed_chain_cost(g, gap_scale);
                }
                const int vm = pmx_seed_wave_max(v);
                if (vm > best) { best = vm; bestb = a - 1 - off - (__ffsll((unsigned long long)__ballot(v == vm)) - 1); }
            }
            if (lane == 0) {
                if (bestb >= 0) {
                    const int c = rc[bestb & mask];
                    if (c < 0 || best > rf[c & mask]) rc[bestb & mask] = a;
                }
                const int sa = a & mask;
                if (a >= ring) { const int c = rc[sa]; child_out[a - ring] = c < 0 ? -1 : (int32_t)(beg + c); }
                rj[sa] = ja; ri[sa] = ia; rf[sa] = best; rc[sa] = -1;
            }
            if (lane == x) { myf = best; mypred = bestb < 0 ? -1 : (int32_t)(beg + bestb); }
            __syncthreads();
        }
        if (lane < cnt) { f_out[base + lane] = myf; pred_out[base + lane] = mypred; }
    }
    for (int e = max(0, n - ring) + lane; e < n; e += PMX_SEED_CHAIN_LANES) { const int c = rc[e & mask]; child_out[e] = c < 0 ? -1 : (int32_t)(beg + c); }
}

// The chain that ends in tail x, walked back over the kept links (a -> pred(a) is kept iff child(pred(a)) == a).
struct PmxSeedChainWalk { int32_t n, score, head, dmin, dmax; };
__device__ __forceinline__ PmxSeedChainWalk pmx_seed_chain_walk(const uint64_t *__restrict__ mkeys, const uint32_t *__restrict__ mvals, const int32_t *__restrict__ f,
                                                                const int32_t *__restrict__ pred, const int32_t *__restrict__ child, int32_t x)
{
    PmxSeedChainWalk w;
    w.n = 1; w.score = f[x];
    w.dmin = w.dmax = (int32_t)(uint32_t)mkeys[x] - (int32_t)mvals[x];
    for (;;) {
        const int32_t b = pred[x];
        if (b < 0) break;
        if (child[b] != x) { w.score -= f[b]; break; }
        x = b; ++w.n;
        const int32_t d = (int32_t)(uint32_t)mkeys[x] - (int32_t)mvals[x];
        w.dmin = min(w.dmin, d); w.dmax = max(w.dmax, d);
    }
    w.head = x;
    return w;
}

// flag[x] = 1 where anchor x is the tail of a candidate (flag: m + 1 entries, the last one 0: the scan's total)
__global__ void __launch_bounds__(256) pmx_seed_chain_tails_kernel(const uint64_t *__restrict__ mkeys, const uint32_t *__restrict__ mvals, const int32_t *__restrict__ f,
                                                                   const int32_t *__restrict__ pred, const int32_t *__restrict__ child, long long m,
                                                                   int min_score, int min_seeds, uint32_t *__restrict__ flag)
{
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x > m) return;
    if (x == m || child[x] >= 0) { flag[x] = 0; return; }
    const PmxSeedChainWalk w = pmx_seed_chain_walk(mkeys, mvals, f, pred, child, (int32_t)x);
    flag[x] = w.score >= min_score && w.n >= min_seeds ? 1u : 0u;
}

// the chain form of pmx_seed_hits_kernel: candidate tails -> outputs at counts[0] + pos[x], below `capacity`; the tail's walk again
__global__ void __launch_bounds__(256) pmx_seed_chain_hits_kernel(const uint64_t *__restrict__ mkeys, const uint32_t *__restrict__ mvals, const int32_t *__restrict__ f,
                                                                  const int32_t *__restrict__ pred, const int32_t *__restrict__ child,
                                                                  const uint32_t *__restrict__ pos, long long m, const int64_t *__restrict__ moff, long long slots,
                                                                  long long stride, int k, PmxSeedWindowArgs g, const int64_t *__restrict__ counts, long long capacity,
                                                                  pmx_pair_t *__restrict__ hit_pairs, uint8_t *__restrict__ hit_byte, pmx_seed_hit_t *__restrict__ hit_seeds,
                                                                  pmx_seed_chain_t *__restrict__ hit_chains)
{
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= m || pos[x + 1] == pos[x]) return;
    const long long at = counts[0] + (long long)pos[x];
    if (at >= capacity) return;
    long long a = 0, z = slots - 1;             // the segment of x, as pmx_seed_hits_kernel finds it
    while (a < z) { const long long mid = (a + z + 1) >> 1; if (moff[mid * stride] <= x) a = mid; else z = mid - 1; }
    const PmxSeedChainWalk c = pmx_seed_chain_walk(mkeys, mvals, f, pred, child, (int32_t)x);
    const uint64_t kt = mkeys[x];
    const PmxSeedWindow w = pmx_seed_window<PMX_SEED_GEOM_DNA>(g, a, (long long)(kt >> 32), c.dmin, c.dmax);
    pmx_pair_t pr; pr.q = w.row; pr.r = w.r; pr.q_beg = 0; pr.q_len = -1; pr.r_beg = (int32_t)w.beg; pr.r_len = (int32_t)(w.end - w.beg);
    hit_pairs[at] = pr;
    hit_byte[at] = (uint8_t)w.byte;
    if (hit_seeds) { pmx_seed_hit_t s; s.n_seeds = c.n; s.diag_min = c.dmin; s.diag_max = c.dmax; s.reserved = 0; hit_seeds[at] = s; }
    if (hit_chains) {
        pmx_seed_chain_t o;
        o.score = c.score; o.n_anchors = c.n; o.q_beg = (int32_t)mvals[c.head]; o.q_end = (int32_t)mvals[x] + k;
        o.r_beg = (int32_t)(uint32_t)mkeys[c.head]; o.r_end = (int32_t)(uint32_t)kt + k; o.diag_min = c.dmin; o.diag_max = c.dmax;
        hit_chains[at] = o;
    }
}

void pmx_seed_chain_shape(int32_t *lanes, int32_t *ring)
{
    if (lanes) *lanes = PMX_SEED_CHAIN_LANES;
    if (ring) *ring = PMX_SEED_CHAIN_RING;
}

// A chaining slice between the cut and the row offsets: the m > 0 matches emitted as (r << 32 | j, i), sorted per segment, chained,
// flagged, scanned and written.  The sort is stable and a segment's matches are emitted in ascending i (position slots ascend with i
// inside an orientation, and a slot's entries are distinct (r, j)), so the sorted order is (r, j, i) whatever the sort does inside.
static int pmx_seed_chain_slice(const PmxSeedPlan &p, const PmxSeedSlice &s, const PmxSeedOut &out, const PmxSeedSource &src, long long row0, long long m,
                                long long segs, long long total, hipStream_t stream)
{
    int rc = 0;
    const unsigned mb = (unsigned)((m + 1 + 255) / 256);
    hipLaunchKernelGGL((pmx_seed_emit_kernel<PMX_SEED_GEOM_DNA, true>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, p.max_qlen, p.ref_count,
                       (const uint32_t *)s.lo, (const uint32_t *)s.cnt, (const int64_t *)s.moff, src.vals, s.keys_a, s.vals_a);
    if ((rc = pmx_launched())) return rc;
    auto seg = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0u), PmxSeedSegOff{s.moff, p.seg_slots});
    size_t tb = s.temp_bytes;
    hipError_t e = rocprim::segmented_radix_sort_pairs(s.temp, tb, (const uint64_t *)s.keys_a, s.keys_b, (const uint32_t *)s.vals_a, s.vals_b, (unsigned)m,
                                                       (unsigned)segs, seg, seg + 1, 0, p.key_bits, stream);
    if (e != hipSuccess) return -(int)e;
    int ring = PMX_SEED_CHAIN_LANES;
    while (ring < p.lookback) ring *= 2;                 // lookback <= PMX_SEED_CHAIN_RING
    hipLaunchKernelGGL(pmx_seed_chain_kernel, dim3((unsigned)segs), dim3(PMX_SEED_CHAIN_LANES), (size_t)ring * 4 * sizeof(int32_t), stream,
                       (const uint64_t *)s.keys_b, (const uint32_t *)s.vals_b, (const int64_t *)s.moff, p.seg_slots, p.k, p.band, p.max_gap, p.lookback,
                       p.gap_scale, ring, s.f, s.pred, s.child);
    if ((rc = pmx_launched())) return rc;
    hipLaunchKernelGGL(pmx_seed_chain_tails_kernel, dim3(mb), dim3(256), 0, stream, (const uint64_t *)s.keys_b, (const uint32_t *)s.vals_b, (const int32_t *)s.f,
                       (const int32_t *)s.pred, (const int32_t *)s.child, m, p.min_score, p.min_seeds, s.flag);
    if ((rc = pmx_launched())) return rc;
    tb = s.temp_bytes;
    e = rocprim::exclusive_scan(s.temp, tb, s.flag, s.flag, 0u, (size_t)(m + 1), rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return -(int)e;
    if (out.capacity > 0) {
        const PmxSeedWindowArgs g = {row0, p.segs, p.first, p.rows_translated, p.ref_count, p.pad, src.qoff, src.roff};
        hipLaunchKernelGGL(pmx_seed_chain_hits_kernel, dim3(mb), dim3(256), 0, stream, (const uint64_t *)s.keys_b, (const uint32_t *)s.vals_b, (const int32_t *)s.f,
                           (const int32_t *)s.pred, (const int32_t *)s.child, (const uint32_t *)s.flag, m, (const int64_t *)s.moff, segs, p.seg_slots, p.k, g,
                           (const int64_t *)out.counts, out.capacity, out.pairs, out.byte, out.seeds, out.chains);
        if ((rc = pmx_launched())) return rc;
    }
    return 0;
}

// The slice's `rows` rows (what the cut kept) with their m matches: emit, sort, clusters, outputs behind counts[0], then the slice's
// row offsets and the running counts.  The geometry chooses the instantiation here and nowhere else; DNA is FRAMES with rows as they
// stand, bit for bit.
int pmx_launch_seed_cluster(const PmxSeedPlan &p, const PmxSeedSlice &s, const PmxSeedOut &out, const PmxSeedSource &src, long long row0,
                            long long rows, long long m, hipStream_t stream)
{
    const long long segs = rows * p.segs, total = rows * p.row_slots;
    int rc = 0;
    if (m > 0 && p.chain) {
        if ((rc = pmx_seed_chain_slice(p, s, out, src, row0, m, segs, total, stream))) return rc;
    } else if (m > 0) {
        decltype(&pmx_seed_emit_kernel<PMX_SEED_GEOM_FRAMES>) emit = nullptr;
        decltype(&pmx_seed_hits_kernel<PMX_SEED_GEOM_FRAMES>) hits = nullptr;
        switch (p.geom) {
        case PMX_SEED_GEOM_DNA:
        case PMX_SEED_GEOM_FRAMES:     emit = pmx_seed_emit_kernel<PMX_SEED_GEOM_FRAMES>;     hits = pmx_seed_hits_kernel<PMX_SEED_GEOM_FRAMES>; break;
        case PMX_SEED_GEOM_CODONS:     emit = pmx_seed_emit_kernel<PMX_SEED_GEOM_CODONS>;     hits = pmx_seed_hits_kernel<PMX_SEED_GEOM_CODONS>; break;
        case PMX_SEED_GEOM_REF_FRAMES: emit = pmx_seed_emit_kernel<PMX_SEED_GEOM_REF_FRAMES>; hits = pmx_seed_hits_kernel<PMX_SEED_GEOM_REF_FRAMES>; break;
        case PMX_SEED_GEOM_REF_CODONS: emit = pmx_seed_emit_kernel<PMX_SEED_GEOM_REF_CODONS>; hits = pmx_seed_hits_kernel<PMX_SEED_GEOM_REF_CODONS>; break;
        default: return -1;
        }
        hipLaunchKernelGGL(emit, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, p.max_qlen, p.ref_count, (const uint32_t *)s.lo,
                           (const uint32_t *)s.cnt, (const int64_t *)s.moff, src.vals, s.keys_a, (uint32_t *)nullptr);
        if ((rc = pmx_launched())) return rc;
        if ((rc = pmx_seed_sort_clusters(p, s, m, segs, stream))) return rc;
        if (out.capacity > 0) {
            const PmxSeedWindowArgs g = {row0, p.segs, p.first, p.rows_translated, p.ref_count, p.pad, src.qoff, src.roff};
            hipLaunchKernelGGL(hits, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, (const uint64_t *)s.keys_b, (const uint32_t *)s.head,
                               (const uint32_t *)s.flag, m, (const int64_t *)s.moff, segs, p.seg_slots, g, (const int64_t *)out.counts, out.capacity,
                               out.pairs, out.byte, out.seeds);
            if ((rc = pmx_launched())) return rc;
        }
    }
    const uint32_t *pos = m > 0 ? s.flag : nullptr;
    hipLaunchKernelGGL(pmx_seed_rowoff_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, pos, (const int64_t *)s.moff, rows, p.row_slots,
                       (const int64_t *)out.counts, out.row_off);
    if ((rc = pmx_launched())) return rc;
    hipLaunchKernelGGL(pmx_seed_advance_kernel, dim3(1), dim3(1), 0, stream, pos, m, out.capacity, out.counts);
    return pmx_launched();
}

