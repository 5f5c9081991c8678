// pmx_trace16.hip -- fast kernel for global / semi-global alignment WITH traceback, for the batch
// CIGAR entry (BASELINE config 4: `sg_trace_striped_16` + CIGAR, /root/reference/src/alignment/mod.rs:
// 390-419 for the single-pair counterpart).  gfx950 only.
//
// Mapping: the strip-systolic layout of pmx_nwsg16.hip (G lanes per pair, R query rows per lane in
// VGPRs, one reference column per step, DPP skew, LDS query profile, virtual rows / columns that
// reproduce the boundary conditions), but ONE pair per slot and unpacked 16-bit lanes:
//
//   * All DP arithmetic is full-rate 32-bit-encoded VOP2 on the low 16 bits of a VGPR
//     (v_add_u16 / v_sub_u16 / v_max_u16, values biased by 32768): 8 instructions per cell.
//   * The four traceback decisions of a cell are four v_cmp_lt_u16 (VOPC -> VCC), each followed by
//     v_addc_co_u32 plane, plane, plane, vcc  -- "shift the lane's trace word left and insert the
//     bit" in one VOP2.  After R = 8 rows the word holds eight 4-bit cells:
//        bit3 ND  : H came from E or F            (T < H)
//        bit2 NDL : not from F                    (F < H)      [ND && !NDL -> DEL, ND && NDL -> INS]
//        bit1 EO  : E of the NEXT column opened   (E - ext < H - open)
//        bit0 FO  : F of the NEXT row opened      (F - ext < H - open)
//     Ties resolve exactly as in the oracle: diag, then F, then E; "open" only when strictly greater.
//   * One coalesced dword store per lane and step: 4 bits per cell in HBM instead of the reference
//     layout's byte per cell (which only the single-pair API still materialises).
//   * pmx_walk16_kernel (one lane per pair) walks the nibbles from the captured end position and
//     emits run-length BAM ops.
#include "pmx_common.h"
#include "pmx_switches.h"
#include "pmx_pk16.h"
#include "pmx_strip.h"
#include <cstdlib>

#define TB 32768                 // bias of the u16 lanes
#define TNEG (-16384)            // finite "-inf": loses against every value of the exact window
#define OP_I 1u
#define OP_D 2u
#define OP_EQ 7u
#define OP_X 8u
#define OP_FOR_INS_STATE PMX_BAM_OP_FOR_INS_STATE    // include/pmx_conventions.h
#define OP_FOR_DEL_STATE PMX_BAM_OP_FOR_DEL_STATE    // include/pmx_conventions.h

// plane = plane * 2 + (a < b)   (unsigned 16-bit compare)
__device__ __forceinline__ void push_lt(unsigned &plane, unsigned a, unsigned b)
{
    asm("v_cmp_lt_u16_e32 vcc, %1, %2\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(plane) : "v"(a), "v"(b) : "vcc");
}

template <int G, int R, bool SW>
__global__ __launch_bounds__(64)
void pmx_trace16_kernel(const uint8_t *__restrict__ qbuf, const int64_t *__restrict__ qoff,
                        const uint8_t *__restrict__ rbuf, const int64_t *__restrict__ roff,
                        long long n, const int16_t *__restrict__ gmat, const uint8_t *__restrict__ gmap,
                        int msize, int open, int ext, int RP, int Tmax,
                        int col_pen, int row_pen, int s1_end, int s2_end,
                        pmx_record_t *__restrict__ out, uint32_t *__restrict__ tbuf)
{
    static_assert(R == 8 || R == 16, "one trace dword per 8 rows");
    constexpr int QP = G * R;
    constexpr int NP = 64 / G;             // pairs per wave
    constexpr int TW = R / 8;              // trace dwords per lane and step
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int lane = threadIdx.x;
    const int g = lane % G;
    const int slot = lane / G;
    const int MS1 = msize + 1;
    const int PROF_STRIDE = MS1 * QP * 2;

    int16_t *prof = reinterpret_cast<int16_t *>(lds);
    unsigned char *rsym = lds + NP * PROF_STRIDE;
    int16_t *mat = reinterpret_cast<int16_t *>(rsym + NP * RP);
    unsigned char *map = reinterpret_cast<unsigned char *>(mat + msize * msize);
    // per pair four ints relative to the block's first pair, dword-aligned: 16 bytes, not the 40 of PmxPairTab
    int *ptab = reinterpret_cast<int *>(map + 256 + ((4 - ((msize * msize * 2) & 3)) & 3));

    const long long pair0 = (long long)blockIdx.x * NP;
    pmx_stage_matrix(mat, map, gmat, gmap, msize * msize, lane, 64);
    if (lane < NP) {
        long long pi = pair0 + lane; if (pi >= n) pi = n - 1;
        const long long qb = qoff[pi], rb = roff[pi];
        ptab[4 * lane + 0] = (int)(qb - qoff[pair0]);
        ptab[4 * lane + 1] = (int)(qoff[pi + 1] - qb);
        ptab[4 * lane + 2] = (int)(rb - roff[pair0]);
        ptab[4 * lane + 3] = (int)(roff[pi + 1] - rb);
    }
    __syncthreads();
    const uint8_t *qbase = qbuf + qoff[pair0];
    const uint8_t *rbase = rbuf + roff[pair0];

    int max_rlen = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) max_rlen = max(max_rlen, ptab[4 * p + 3]);

    for (int p = 0; p < NP; ++p)
        pmx_stage_ref_symbols<G, 4>(rsym + p * RP, RP, rbase + ptab[4 * p + 2], ptab[4 * p + 3], map, msize, lane, 64);
    // extended profile: P virtual rows on top, then the qlen real rows
    const int vrow_score = row_pen ? TNEG : 0, vcol_score = col_pen ? TNEG : 0;
    for (int p = 0; p < NP; ++p) {
        const int P = QP - ptab[4 * p + 1];
        const uint8_t *qp = qbase + ptab[4 * p + 0];
        int16_t *pp = prof + p * (PROF_STRIDE / 2);
        for (int er0 = 0; er0 < QP; er0 += 64 * 4) {
            int qs[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int er = er0 + u * 64 + lane;
                qs[u] = (er < QP && er >= P) ? (int)qp[er - P] : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int er = er0 + u * 64 + lane;
                if (er < QP) {
                    const int q0 = qs[u] < 0 ? -1 : map[qs[u]];
                    for (int sym = 0; sym < msize; ++sym)
                        pp[sym * QP + er] = (int16_t)((q0 < 0) ? vrow_score : mat[q0 * msize + sym]);
                    pp[msize * QP + er] = (int16_t)((q0 < 0) ? 0 : vcol_score);
                }
            }
        }
    }
    __syncthreads();

    // ---- per-lane state --------------------------------------------------------------------
    const unsigned short *profL = reinterpret_cast<const unsigned short *>(lds + slot * PROF_STRIDE) + g * R;
    const unsigned char *rs = rsym + slot * RP + (G - 1) - g;
    const int ql = ptab[4 * slot + 1], rl = ptab[4 * slot + 3];
    const int P = QP - ql;
    const unsigned vOpen = (unsigned)open, vExt = (unsigned)ext;

    auto left_h = [&](int er) -> unsigned {
        const int i = er - P;
        return (unsigned)(TB + ((i >= 0 && col_pen) ? -(open + i * ext) : 0));
    };
    unsigned HA[R], HB[R], E[R];
#pragma unroll
    for (int k = 0; k < R; ++k) { HA[k] = left_h(g * R + k); HB[k] = HA[k]; E[k] = HA[k] - vOpen; }
    unsigned Hout = HA[R - 1];
    unsigned Fout;
    {
        const int i = (g + 1) * R - P;
        Fout = (unsigned)(TB + ((i >= 0 && col_pen) ? -(open + i * ext) : -open));
    }
    unsigned diag0 = (g == 0) ? (unsigned)TB : left_h(g * R - 1);

    int res = TB, bestrow = 0, bestrowj = 0, bestcol = 0, bestcoli = 0;
    // local alignment: running best of this lane, the column where it was first exceeded, the strip at that column
    unsigned swbest = (unsigned)TB, swcol = 0u, swsave[R];
#pragma unroll
    for (int k = 0; k < R; ++k) swsave[k] = (unsigned)TB;
    uint32_t *tw = tbuf + ((size_t)blockIdx.x * Tmax) * (64 * TW) + lane * TW;

    auto load_scores = [&](int sym, unsigned (&w)[R]) {
        const unsigned short *sp = profL + sym * QP;
#pragma unroll
        for (int k = 0; k < R; ++k) w[k] = sp[k];
    };
    auto step = [&](const unsigned (&Hold)[R], unsigned (&Hnew)[R], const unsigned (&w)[R], int t) {
        const unsigned Hin = group_shift_up<G>(Hout, TB, g);
        unsigned F = group_shift_up<G>(Fout, TB + TNEG, g);
        unsigned plane[TW];
#pragma unroll
        for (int x = 0; x < TW; ++x) plane[x] = 0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const unsigned d = (k == 0) ? diag0 : Hold[k - 1];
            const unsigned Tt = add_u16(d, w[k]);
            unsigned H = max_u16(max_u16(Tt, E[k]), F);
            if (SW) H = max_u16(H, (unsigned)TB);      // local: floor at zero (the walk stops where the score is used up)
            push_lt(plane[k / 8], Tt, H);          // ND
            push_lt(plane[k / 8], F, H);           // NDL
            const unsigned Ho = sub_u16(H, vOpen);
            const unsigned Ee = sub_u16(E[k], vExt), Fe = sub_u16(F, vExt);
            push_lt(plane[k / 8], Ee, Ho);         // EO (next column)
            push_lt(plane[k / 8], Fe, Ho);         // FO (next row)
            E[k] = max_u16(Ee, Ho);
            F = max_u16(Fe, Ho);
            Hnew[k] = H;
        }
        diag0 = Hin;
        Hout = Hnew[R - 1];
        Fout = F;
#pragma unroll
        for (int x = 0; x < TW; ++x) tw[(size_t)t * (64 * TW) + x] = plane[x];

        // ---- captures ----
        const int jcol = t - g;
        if (SW) {
            unsigned cm = Hnew[0] & 0xFFFFu;
#pragma unroll
            for (int k = 1; k < R; ++k) cm = max_u16(cm, Hnew[k]) & 0xFFFFu;
            const bool imp = cm > swbest;          // strictly greater: the first column reaching a value keeps it
            swbest = imp ? cm : swbest;
            swcol = imp ? (unsigned)jcol : swcol;
#pragma unroll
            for (int k = 0; k < R; ++k) swsave[k] = imp ? Hnew[k] : swsave[k];
            return;
        }
        const int hl = (int)(Hout & 0xFFFF);
        if (jcol == rl - 1) res = hl;
        if (s2_end && jcol >= 0 && jcol < rl && hl > bestrow) { bestrow = hl; bestrowj = jcol; }
        if (s1_end && jcol == rl - 1) {
            int cm = 0, cr = 0;
#pragma unroll
            for (int k = R - 1; k >= 0; --k) {
                const int er = g * R + k;
                const int v = (er >= P) ? (int)(Hnew[k] & 0xFFFF) : 0;
                if (v >= cm) { cm = v; cr = er; }          // descending k with >= : smallest row among equals
            }
            if (cm > bestcol) { bestcol = cm; bestcoli = cr; }
        }
    };

    const int T = (max_rlen + G - 1 + 1) & ~1;
    unsigned w0[R], w1[R];
    load_scores(rs[0], w0);
    int ns = rs[1];
    for (int t = 0; t < T; t += 2) {
        load_scores(ns, w1);
        ns = rs[t + 2];
        __builtin_amdgcn_sched_barrier(0);
        step(HA, HB, w0, t);
        __builtin_amdgcn_sched_barrier(0);
        load_scores(ns, w0);
        ns = rs[t + 3];
        __builtin_amdgcn_sched_barrier(0);
        step(HB, HA, w1, t + 1);
        __builtin_amdgcn_sched_barrier(0);
    }

    if (SW) {
        int krow = 0;
#pragma unroll
        for (int k = R - 1; k >= 0; --k) if ((swsave[k] & 0xFFFFu) == swbest) krow = k;
        const unsigned long long key = pmx_slot_best_key<G>(((unsigned long long)swbest << 32) | ((unsigned long long)(0xFFFFu - (swcol & 0xFFFFu)) << 16) |
                                                             (unsigned long long)(0xFFFFu - (unsigned)(g * R + krow)));
        if (g == 0) {
            const long long pi = pair0 + slot;
            if (pi < n) {
                pmx_record_t rec; rec.flags = 0;
                rec.score = (int)(key >> 32) - TB;
                rec.end_ref = 0xFFFF - (int)((key >> 16) & 0xFFFF);
                rec.end_query = 0xFFFF - (int)(key & 0xFFFF) - P;
                if (rec.score == 0) { rec.end_query = 0; rec.end_ref = 0; }      // all-zero table: (0, 0) like the oracle
                out[pi] = rec;
            }
        }
        return;
    }
    // ---- combine: the end rule of DESIGN.md 2.1a ------------------------------------------------
    const unsigned key = pmx_slot_best_key<G>(pmx_slot_key((unsigned)bestcol, (unsigned)bestcoli));
    const int lastlane = slot * G + G - 1;
    const int resL = __shfl(res, lastlane, 64), browL = __shfl(bestrow, lastlane, 64), browjL = __shfl(bestrowj, lastlane, 64);
    if (g == 0) {
        const long long pi = pair0 + slot;
        if (pi < n) {
            const PmxEnd e = pmx_sg_end(s1_end, s2_end, ql, rl, resL - TB, browL - TB, browjL, pmx_key_value(key) - TB, pmx_key_row(key) - P);
            pmx_record_t rec; rec.score = e.score; rec.end_query = e.end_query; rec.end_ref = e.end_ref; rec.flags = 0;
            out[pi] = rec;
        }
    }
}

// ---- walk over the 4-bit trace ---------------------------------------------------------------
// (the first-generation layout only: the packed sweeps' records are walked by pmx_walkp.hip)
template <int G, int R>
__global__ void pmx_walk16_kernel(const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                                  long long n, const uint8_t *mapper, const int16_t *scores, int msize, int open, int ext,
                                  int mode, int Tmax, int stage /* LDS bytes reserved for each of the block's queries / references, 0 = none */,
                                  pmx_stats_t *stats_out /* != nullptr: count matches / similar / length along the path instead of emitting ops */,
                                  int row_pen, int col_pen /* stats: the begin gaps along the reference / query are part of the alignment */,
                                  const uint32_t *tbuf, const pmx_record_t *recs,
                                  uint32_t *ops, const int64_t *ops_off /* nullptr: slot of pair k starts at qoff[k] + roff[k] + k - ops_base */,
                                  long long ops_base, int32_t *nops, int32_t *beg, int32_t *textlen /* optional: bytes of the CIGAR text */)
{
    extern __shared__ unsigned char w_lds[];
    constexpr int QP = G * R, NP = 64 / G, TW = R / 8;
    // mapper and matrix in LDS: the walk is a chain of dependent loads, keep all but the trace fetch short
    __shared__ unsigned char s_map[256];
    __shared__ int16_t s_scores[PMX_MAX_FAST_MSIZE * PMX_MAX_FAST_MSIZE];
    for (int x = threadIdx.x; x < 256; x += blockDim.x) s_map[x] = mapper[x];
    for (int x = threadIdx.x; x < msize * msize; x += blockDim.x) s_scores[x] = scores[x];
    // The block's sequences are contiguous in the packed buffers: stage them in LDS with coalesced loads, so
    // that the only scattered global access left per step is the trace nibble.
    const long long p0 = (long long)blockIdx.x * blockDim.x;
    const long long p1 = p0 + blockDim.x < n ? p0 + blockDim.x : n;
    const long long qlo = qoff[p0], rlo = roff[p0];
    if (stage) {
        const int qn = (int)(qoff[p1] - qlo), rn = (int)(roff[p1] - rlo);
        for (int x = threadIdx.x; x < qn; x += blockDim.x) w_lds[x] = qbuf[qlo + x];
        for (int x = threadIdx.x; x < rn; x += blockDim.x) w_lds[stage + x] = rbuf[rlo + x];
    }
    __syncthreads();
    const long long pair = p0 + threadIdx.x;
    if (pair >= n) return;
    const long long qb = qoff[pair], rb = roff[pair];
    const int ql = (int)(qoff[pair + 1] - qb), rl = (int)(roff[pair + 1] - rb);
    const uint8_t *q = qbuf + qb, *r = rbuf + rb;
    const unsigned char *sq = w_lds + (qb - qlo), *sr = w_lds + stage + (rb - rlo);
    const long long block = pair / NP; const int slot = (int)(pair % NP);
    // R / 8 words per lane and step, step-major
    const uint32_t *tb = tbuf + (size_t)block * Tmax * (64 * TW);
    const int P = QP - ql;
    auto ldw = [&](int i, int j) -> uint32_t {         // the trace word holding cell (i, j); 0 outside i >= -1, j >= 0
        if (i < -1 || j < 0) return 0u;
        const int er = i + P;
        if (er < 0) return 0u;
        const int g = er / R, k = er % R;
        return tb[(size_t)(j + g) * (64 * TW) + (slot * G + g) * TW + (k / 8)];
    };
    auto nibof = [&](uint32_t w, int i) -> unsigned { return (w >> (28 - 4 * (((i + P) % R) % 8))) & 0xFu; };
    auto nib = [&](int i, int j) -> unsigned { return nibof(ldw(i, j), i); };
    const bool st = stats_out != nullptr;
    uint32_t *o = st ? nullptr : ops + (ops_off ? ops_off[pair] : qb + rb + pair - ops_base);
    const pmx_record_t rec = recs[pair];
    int i = rec.end_query, j = rec.end_ref, cnt = 0;
    uint32_t cur_op = 0, cur_len = 0;
    int tlen = 0;                    // text bytes: digits of every run length + one letter
    auto digits = [](uint32_t v) -> int { return v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : 10; };
    int nM = 0, nS = 0, nL = 0;      // statistics of the path = the coupled stats tables of the reference (same decisions, same ties)
    auto emit = [&](uint32_t op) {
        if (st) { ++nL; return; }
        if (op == cur_op) ++cur_len;
        else { if (cur_len) { o[cnt++] = (cur_len << 4) | cur_op; tlen += digits(cur_len) + 1; } cur_op = op; cur_len = 1; }
    };
    if (mode == PMX_MODE_SG && !st) {
        if (i + 1 == ql) { for (int k = rl - 1; k > j; --k) emit(OP_FOR_INS_STATE); }
        else if (j + 1 == rl) { for (int k = ql - 1; k > i; --k) emit(OP_FOR_DEL_STATE); }
    }
    int where = 0;   // 0 DIAG, 1 INS, 2 DEL
    const bool sw = mode == PMX_MODE_SW;
    int rem = rec.score;       // local alignment: value of the current H / E / F cell; the path starts where it is used up
    while (i >= 0 || j >= 0) {
        if (i < 0) { if (sw || (st && !row_pen)) break; emit(OP_FOR_INS_STATE); --j; continue; }
        if (j < 0) { if (sw || (st && !col_pen)) break; emit(OP_FOR_DEL_STATE); --i; continue; }
        if (where == 0) {
            if (sw && rem <= 0) break;                       // ZERO cell
            const unsigned t = nib(i, j);
            if (!(t & 8u)) {
                const int a = s_map[stage ? sq[i] : q[i]], b = s_map[stage ? sr[j] : r[j]];
                emit(a == b ? OP_EQ : OP_X);
                if (st) { nM += a == b; nS += s_scores[a * msize + b] > 0; }
                if (sw) rem -= s_scores[a * msize + b];
                --i; --j;
            }
            else if (!(t & 4u)) where = 2;
            else where = 1;
        } else if (where == 1) {
            emit(OP_FOR_INS_STATE);
            if (j > 0 && (nib(i, j - 1) & 2u)) { where = 0; rem += open; } else rem += ext;
            --j;
        } else {
            emit(OP_FOR_DEL_STATE);
            if (nib(i - 1, j) & 1u) { where = 0; rem += open; } else rem += ext;
            --i;
        }
    }
    if (st) { pmx_stats_t r3; r3.matches = nM; r3.similar = nS; r3.length = nL; stats_out[pair] = r3; return; }
    if (cur_len) { o[cnt++] = (cur_len << 4) | cur_op; tlen += digits(cur_len) + 1; }
    if (textlen) textlen[pair] = tlen;
    for (int k = 0; k < cnt / 2; ++k) { const uint32_t tmp = o[k]; o[k] = o[cnt - 1 - k]; o[cnt - 1 - k] = tmp; }
    nops[pair] = cnt;
    beg[2 * pair] = i + 1; beg[2 * pair + 1] = j + 1;
}

// ------------------------------------------------------------------------ host side ----
// LDS bytes per side for staging a 64-pair block's queries / references in the walk (0: too long, read them from HBM)
static int walk_stage_bytes(const PmxBatch &b)
{
    const long long m = 64LL * (b.max_qlen > b.max_rlen ? b.max_qlen : b.max_rlen);
    return (m <= 60 * 1024) ? (int)((m + 15) / 16 * 16) : 0;
}

// The first-generation shapes in try order: f(G, R) as integral constants until one returns true.
template <typename F> static bool for_each_gen1_shape(F &&f)
{
    using std::integral_constant;
    return f(integral_constant<int, 32>{}, integral_constant<int, 8>{}) || f(integral_constant<int, 64>{}, integral_constant<int, 8>{}) || f(integral_constant<int, 64>{}, integral_constant<int, 16>{});
}

template <int G, int R, bool SW>
static int launch_trace(const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext,
                        pmx_record_t *d_out, uint32_t *tbuf, int Tmax,
                        uint32_t *ops, const int64_t *ops_off, int32_t *nops, int32_t *beg, pmx_stats_t *stats_out, hipStream_t stream)
{
    constexpr int QP = G * R, NP = 64 / G;
    const int RP = pmx_strip_ref_cols(b.max_rlen, G);
    const size_t lds = (size_t)NP * (m.msize + 1) * QP * 2 + (size_t)NP * RP +
                       (size_t)m.msize * m.msize * 2 + 256 + 4 + (size_t)NP * 16;
    if (lds > 160 * 1024) return 1;
    { const int rc = pmx_ensure_lds_attr(reinterpret_cast<const void *>(&pmx_trace16_kernel<G, R, SW>)); if (rc) return rc; }
    const PmxEnds ends = pmx_ends(mode, sg_flags);
    const long long blocks = (b.n + NP - 1) / NP;
    hipLaunchKernelGGL((pmx_trace16_kernel<G, R, SW>), dim3((unsigned)blocks), dim3(64), lds, stream,
                       b.qbuf, b.qoff, b.rbuf, b.roff, (long long)b.n, m.scores, m.mapper,
                       m.msize, open, ext, RP, Tmax, ends.col_pen, ends.row_pen, ends.s1_end, ends.s2_end, d_out, tbuf);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return -(int)e;
    const int stage = walk_stage_bytes(b);
    { const int rc = pmx_ensure_lds_attr(reinterpret_cast<const void *>(&pmx_walk16_kernel<G, R>), 128 * 1024); if (rc) return rc; }
    hipLaunchKernelGGL((pmx_walk16_kernel<G, R>), dim3((unsigned)((b.n + 63) / 64)), dim3(64), 2 * (size_t)stage, stream,
                       b.qbuf, b.qoff, b.rbuf, b.roff, (long long)b.n, m.mapper, m.scores, m.msize, open, ext, mode, Tmax, stage, stats_out, ends.row_pen, ends.col_pen,
                       (const uint32_t *)tbuf, (const pmx_record_t *)d_out, ops, ops_off, 0LL, nops, beg, (int32_t *)nullptr);
    return pmx_launched();
}

// Picks the sweep; p->trace_bytes tells the caller how much trace scratch to provide.  Returns 1 when the batch is not eligible.
int pmx_trace16_plan(const PmxBatch &b, const PmxDevMatrix &m, int mode, int open, int ext, PmxTracePlan *p, bool packed_ok)
{
    if (m.pssm) return 1;                                   // (symbol profiles only: a PSSM takes the general kernel)
    if (pmx_env("PMX_NO_FAST_TRACE")) return 1;
    if (mode != PMX_MODE_NW && mode != PMX_MODE_SG && mode != PMX_MODE_SW) return 1;
    if (m.msize > PMX_MAX_FAST_MSIZE - 1) return 1;
    if (open < ext || open < 0 || ext < 0 || open > 4096) return 1;
    if (b.max_rlen > 30000 || b.q_shared) return 1;
    // packed traceback of the second-generation nw/sg kernel, of the local kernel
    if (packed_ok && !pmx_env("PMX_TRACE16_GEN1") && pmx_nwsgv_trace_plan(b, m, mode, open, ext, p) == 0) return 0;
    if (packed_ok && mode == PMX_MODE_SW && pmx_sw16_trace_plan(b, m, open, ext, p) == 0) return 0;
    const long long lo = mode == PMX_MODE_SW ? -(2LL * open + 2LL * ext + (m.min < 0 ? -m.min : 0))
                                             : -(3LL * open + (long long)(b.max_qlen + b.max_rlen + 2) * ext + (m.min < 0 ? -m.min : 0));
    const long long hi = (long long)(b.max_qlen < b.max_rlen ? b.max_qlen : b.max_rlen) * (m.max > 0 ? m.max : 0) + (m.max > 0 ? m.max : 0);
    if (lo < -15000 || hi > 15000) return 1;
    int G = 0, R = 0;
    for_each_gen1_shape([&](auto g, auto r) { if (b.max_qlen > g * r - 1) return false; G = g; R = r; return true; });
    if (!G) return 1;
    p->family = PMX_TRACE_GEN1; p->G = G; p->R = R; p->pairs_per_wg = 64 / G;
    p->Tmax = (b.max_rlen + G - 1 + 1) & ~1;
    p->trace_bytes = (size_t)((b.n + p->pairs_per_wg - 1) / p->pairs_per_wg) * (size_t)p->Tmax * 64 * (R / 8) * sizeof(uint32_t);
    p->top_aligned = false; p->fills_blockflag = false; p->walk = PMX_TRACE_WALK16;
    return 0;
}

extern "C" int pmx_trace_plan_probe(int mode, int msize, int score_min, int score_max, int pssm, int open, int ext, long long n,
                                    int max_qlen, int max_rlen, int q_shared, int short_waves, int packed_ok,
                                    int *family, int *G, int *R, int *Tmax, long long *trace_bytes)
{
    PmxBatch b = {}; PmxDevMatrix m = {}; PmxTracePlan p = {};
    b.n = n; b.max_qlen = max_qlen; b.max_rlen = max_rlen; b.q_shared = q_shared;
    m.msize = msize; m.min = score_min; m.max = score_max; m.pssm = pssm; m.rows = pssm ? (q_shared ? q_shared : max_qlen) : msize;
    const int rc = q_shared ? pmx_nwsgq_trace_plan(b, m, mode, open, ext, &p, short_waves) : pmx_trace16_plan(b, m, mode, open, ext, &p, packed_ok != 0);
    if (rc) p = PmxTracePlan();
    *family = (int)p.family; *G = p.G; *R = p.R; *Tmax = p.Tmax; *trace_bytes = (long long)p.trace_bytes;
    return rc;
}

int pmx_launch_trace16(const PmxTracePlan &p, const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext,
                       pmx_record_t *d_out, uint32_t *tbuf, uint32_t *ops, const int64_t *ops_off, int32_t *nops, int32_t *beg, hipStream_t stream,
                       const char **sweep_name, pmx_stats_t *stats_out, const PmxWalkSplit *split)
{
    if (m.pssm) return 1;                                   // (symbol profiles only: a PSSM takes the general kernel)
    const bool sw = mode == PMX_MODE_SW;
    const PmxEnds ends = pmx_ends(mode, sg_flags);
    if (p.walk == PMX_TRACE_WALKP) {
        int rc = p.top_aligned ? pmx_launch_sw16_trace(p, b, m, open, ext, d_out, tbuf, stream, sweep_name)
                               : pmx_launch_nwsgv_trace(p, b, m, mode, sg_flags, open, ext, d_out, tbuf, stream, sweep_name);
        if (rc) return rc;
        hipStream_t wstream = stream;
        if (split && split->walk_stream != stream) {      // the walk runs beside the next chunk's sweep
            hipError_t e1 = hipEventRecord(split->sweep_done, stream);
            if (e1 == hipSuccess) e1 = hipStreamWaitEvent(split->walk_stream, split->sweep_done, 0);
            if (e1 != hipSuccess) return -(int)e1;
            wstream = split->walk_stream;
        }
        const long long ops_base = split ? split->ops_base : 0;
        int32_t *textlen = split ? split->textlen : nullptr;
        rc = pmx_launch_walkp(p.G, p.R, b, m, mode, open, ext, p.Tmax, p.top_aligned, stats_out, ends.row_pen, ends.col_pen,
                              (const uint32_t *)tbuf, (const pmx_record_t *)d_out, ops, ops_off, ops_base, nops, beg, textlen, wstream,
                              p.fills_blockflag ? b.blockflag : nullptr);
        if (rc) return rc;
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && split && split->walk_done) e = hipEventRecord(split->walk_done, wstream);
        return e == hipSuccess ? 0 : -(int)e;
    }
    if (split) return 1;                 // the split form is only built for the packed (second-generation) sweeps
    int rc = 1;
    for_each_gen1_shape([&](auto g, auto r) {
        if (g != p.G || r != p.R) return false;
        rc = sw ? launch_trace<g, r, true>(b, m, mode, sg_flags, open, ext, d_out, tbuf, p.Tmax, ops, ops_off, nops, beg, stats_out, stream)
                : launch_trace<g, r, false>(b, m, mode, sg_flags, open, ext, d_out, tbuf, p.Tmax, ops, ops_off, nops, beg, stats_out, stream);
        return true;
    });
    if (rc == 0) *sweep_name = "pmx_trace16_kernel";
    return rc;
}
