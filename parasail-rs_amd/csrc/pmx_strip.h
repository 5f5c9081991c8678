// pmx_strip.h -- what the strip-systolic kernels share around the recurrence: the per-pair table in LDS, the staging of
// matrix, mapper and reference symbols, the reduction over a slot's lanes, the rule for where a global / semi-global
// alignment ends, and the launchers' boundary flags.  DESIGN.md 2.1a states the three conventions; everything here runs
// before the first step or after the last.  gfx950 only.
#pragma once
#include "pmx_common.h"

// ---- pair table: five long long per pair of the block (q offset, qlen, r offset, rlen, pair index or -1) ----
// pmx_nwsg16q_kernel / pmx_sw16q_kernel (one shared query: three entries) and pmx_trace16_kernel (four ints relative to the
// block's first pair, dword-aligned) keep their own smaller tables: this layout would cost them LDS.
#define PMX_PAIRTAB_BYTES 40
struct PmxPairTab {
    long long *t;
    // slot idx of the block that starts at position pair0; positions at or beyond n repeat pair n - 1 with index -1
    __device__ __forceinline__ void fill(int idx, long long pair0, long long n, const unsigned *__restrict__ perm,
                                         const int64_t *__restrict__ qoff, const int64_t *__restrict__ roff, int q_shared) const
    {
        long long pos = pair0 + idx; if (pos >= n) pos = n - 1;
        const long long pi = perm ? (long long)perm[pos] : pos;
        const long long qb = q_shared ? 0 : qoff[pi], rb = roff[pi];
        t[5 * idx + 0] = qb;
        t[5 * idx + 1] = q_shared ? q_shared : (qoff[pi + 1] - qb);
        t[5 * idx + 2] = rb;
        t[5 * idx + 3] = roff[pi + 1] - rb;
        t[5 * idx + 4] = (pair0 + idx < n) ? pi : -1;
    }
    __device__ __forceinline__ long long qbeg(int p) const { return t[5 * p + 0]; }
    __device__ __forceinline__ int qlen(int p) const { return (int)t[5 * p + 1]; }
    __device__ __forceinline__ long long rbeg(int p) const { return t[5 * p + 2]; }
    __device__ __forceinline__ int rlen(int p) const { return (int)t[5 * p + 3]; }
    __device__ __forceinline__ long long index(int p) const { return t[5 * p + 4]; }
    __device__ __forceinline__ long long *behind(int np) const { return t + 5 * np; }      // what the kernel keeps after np pairs
};

// ---- matrix and mapper into LDS; the 8-byte-aligned address behind the mapper ----
__device__ __forceinline__ void pmx_stage_matrix(int16_t *mat, unsigned char *map, const int16_t *__restrict__ gmat,
                                                 const uint8_t *__restrict__ gmap, int cells, int tid, int NT)
{
    for (int i = tid; i < cells; i += NT) mat[i] = gmat[i];
    for (int i = tid; i < 256; i += NT) map[i] = gmap[i];
}
__device__ __forceinline__ unsigned char *pmx_after_matrix(unsigned char *map, int cells)
{
    return map + 256 + ((8 - ((cells * 2) & 7)) & 7);
}

// ---- one pair's reference symbols: G - 1 virtual columns in front, the pad symbol `msize` behind, RP bytes in all ----
// U loads per thread are in flight before the first is mapped.
template <int G, int U>
__device__ __forceinline__ void pmx_stage_ref_symbols(unsigned char *rsym, int RP, const uint8_t *__restrict__ ref, int rl,
                                                      const unsigned char *map, int msize, int tid, int NT)
{
    for (int j0 = 0; j0 < RP; j0 += NT * U) {
        unsigned char raw[U]; bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * NT + tid, jj = j - (G - 1);
            ok[u] = j < RP && jj >= 0 && jj < rl;
            raw[u] = ok[u] ? ref[jj] : (unsigned char)0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * NT + tid;
            if (j < RP) rsym[j] = ok[u] ? map[raw[u]] : (unsigned char)msize;
        }
    }
}

// half h (0 low, 1 high) of a packed pair of unsigned 16-bit values
__device__ __forceinline__ int pmx_half(int x, int h) { return (int)(h ? ((unsigned)x >> 16) : (x & 0xFFFF)); }

// ---- reduction over the G lanes of a slot (STRIDE 2: the interleaved 8-lane groups of pmx_pk16.h) ----
// A last-column candidate is the key (value << 16) | (0xFFFF - row): the maximum is the highest value at the lowest row.
__device__ __forceinline__ unsigned pmx_slot_key(unsigned value, unsigned row) { return (value << 16) | (0xFFFFu - row); }
__device__ __forceinline__ int pmx_key_value(unsigned key) { return (int)(key >> 16); }
__device__ __forceinline__ int pmx_key_row(unsigned key) { return (int)(0xFFFFu - (key & 0xFFFFu)); }
template <int G, int STRIDE = 1, class K>
__device__ __forceinline__ K pmx_slot_best_key(K key)
{
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) {
        const K o = __shfl_xor(key, off * STRIDE, 64);
        key = o > key ? o : key;
    }
    return key;
}
template <int G>
__device__ __forceinline__ unsigned long long pmx_slot_mask(int lane)      // the lanes of this lane's slot, as a ballot mask
{
    return (G == 64) ? ~0ULL : (((1ULL << G) - 1ULL) << ((lane / G) * G));
}

// ---- where a global / semi-global alignment ends (the oracle's rule) ----
// 0: the corner cell, 1: the best of the last row, 2: the best of the last column.  brow / bcol are true (un-biased) scores,
// or biased alike.
__host__ __device__ __forceinline__ int pmx_sg_choice(int s1_end, int s2_end, int brow, int bcol)
{
    if (!s1_end && !s2_end) return 0;
    return (s1_end && (!s2_end || bcol > brow)) ? 2 : 1;        // the last row wins ties against the last column
}
struct PmxEnd { int score, end_query, end_ref; };
__host__ __device__ __forceinline__ PmxEnd pmx_sg_end(int s1_end, int s2_end, int ql, int rl, int corner,
                                                      int brow, int browj, int bcol, int bcoli)
{
    const int c = pmx_sg_choice(s1_end, s2_end, brow, bcol);
    PmxEnd e;
    e.score = c == 0 ? corner : c == 1 ? brow : bcol;
    e.end_query = c == 2 ? bcoli : ql - 1;
    e.end_ref = c == 1 ? browj : rl - 1;
    return e;
}

// ---- boundary flags of (mode, sg_flags): nw penalises both boundaries, sg a boundary unless its begin is free, sw none;
// a free end exists only in sg ----
struct PmxEnds { int col_pen /* H(i, -1) penalised */, row_pen /* H(-1, j) penalised */, s1_end /* query end free */, s2_end /* reference end free */; };
__host__ __device__ static inline PmxEnds pmx_ends(int mode, int sg_flags)
{
    const bool nw = mode == PMX_MODE_NW, sg = mode == PMX_MODE_SG;
    PmxEnds e;
    e.col_pen = nw || (sg && !(sg_flags & PMX_SG_QB));
    e.row_pen = nw || (sg && !(sg_flags & PMX_SG_DB));
    e.s1_end = sg && (sg_flags & PMX_SG_QE);
    e.s2_end = sg && (sg_flags & PMX_SG_DE);
    return e;
}

// bytes of a staged reference row: the virtual columns in front, the pad and the two-step read-ahead behind
static inline int pmx_strip_ref_cols(int max_rlen, int G) { return ((max_rlen + 2 * (G - 1) + 4 + 7) / 4) * 4; }
// The width the trace planners put into their launchers' LDS sums: pmx_strip_ref_cols() plus a margin of 3 to 6 bytes, so a plan at
// the 160 KiB edge moves to the next shape a few reference bytes before its launcher would have to refuse.
static inline int pmx_strip_ref_cols_plan(int max_rlen, int G) { return max_rlen + 2 * G + 12; }
