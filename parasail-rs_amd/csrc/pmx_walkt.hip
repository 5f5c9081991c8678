// pmx_walkt.hip -- traceback of long pairs in linear memory: re-derive, tile by tile and from the end cell backwards, only the tiles
// the optimal path enters.  gfx950 only.  Specification: tests/tilewalk_model.c (checked against the oracle on the CPU tier).
//
// The checkpoint form of the long-pair sweep (pmx_long32_kernel<.., CK = true>, pmx_long.hip) leaves, per pair,
//   * row granules: band b < NB - 1, column j -> (H, F) leaving the band's last row il = (b + 1) * BR - 1 (what band b + 1 consumed):
//         H = H(il, j) - open + SKEW (il + j + 1) ext,   F = F(il + 1, j) + SKEW (il + 1 + j) ext     (local: max(F, 0))
//   * column checkpoints: band b, slot s, row x of the band -> (H, E) of column jc = (s + 1) * C - 1:
//         H = H(x, jc) - open + SKEW (x + jc + 1) ext,   E = E(x, jc) + SKEW (x + jc) ext
//     at ck[((pair * nbmax + b) * ckslots + s) * BR + (x - b * BR)], 8 bytes each (consecutive rows = consecutive granules),
// SKEW = 1 for global / semi-global (the sweep's column-and-row offset), 0 for local.  Tile (b, c) -- rows of band b, columns
// [c * C, (c + 1) * C) -- follows from the granules of band b - 1 and slot c - 1 alone (or the matrix's first row / column).
//
// One wave per pair.  For the tile that holds the walk's cell (ie, je) the wave recomputes rows b * BR .. ie, columns c * C .. je in
// sub-blocks of 64 rows: lane g owns one row and works on column t - g at step t (the sweep's systolic order; H and F cross to lane
// g + 1 by DPP wave_shr:1, lane 0 reads the row above from the LDS, the last lane leaves its row there for the next sub-block).
// Each cell's four decisions ND NDL EO FO (the oracle's strict comparisons) go into the LDS, eight cells a dword, rows
// padded by one dword (lanes write different rows at the same column: the pad spreads them over the banks).  Lane 0 then walks the
// oracle's state machine over the tile -- symbols and scores from the LDS too -- until it leaves through the top row or the left
// column, CARRYING ITS STATE: DIAG, INS, DEL, or a resolve state (a gap op has been emitted and the cell it came from must still say,
// by its EO / FO, whether the gap opened there; that cell may be in the next tile).  Ops, op count, text length and statistics by the
// rules of pmx_walkb.hip / pmx_walkp.hip.  The kernel reads finished launches only; a launch whose sweep gave up (abort word) gets
// empty outputs, and the host turns that into an error.
#include "pmx_common.h"
#include "pmx_pk16.h"
#include "pmx_strip.h"

#define OP_EQ 7u
#define OP_X 8u
#define OP_FOR_INS_STATE PMX_BAM_OP_FOR_INS_STATE    // include/pmx_conventions.h
#define OP_FOR_DEL_STATE PMX_BAM_OP_FOR_DEL_STATE    // include/pmx_conventions.h
#define T_NEG (-(1 << 30))

struct PmxWalktArgs {
    const uint8_t *qbuf; const int64_t *qoff; const uint8_t *rbuf; const int64_t *roff; long long n;
    const uint8_t *mapper; const int16_t *scores; int msize; int open, ext, mode, row_pen, col_pen;
    const pmx_record_t *recs;
    const unsigned long long *bound; long long bstride; int nbmax;
    const int2 *ck; long long ckslots; int ckshift; int BR;
    const int *abort_word;
    const int64_t *slot_qoff; long long ops_base; uint32_t *ops; int32_t *nops, *textlen; pmx_stats_t *stats;
};

enum { W_DIAG = 0, W_INS = 1, W_DEL = 2, W_INSR = 3, W_DELR = 4 };

template <bool SW>
__global__ __launch_bounds__(64)
void pmx_walkt_kernel(PmxWalktArgs a)
{
    constexpr int SKEW = SW ? 0 : 1;
    const int lane = threadIdx.x;
    const long long pair = blockIdx.x;
    const int msize = a.msize, open = a.open, ext = a.ext, BR = a.BR, C = 1 << a.ckshift, RS = C / 8 + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    uint32_t *bits = reinterpret_cast<uint32_t *>(lds);                 // [BR][RS]
    int *tH = reinterpret_cast<int *>(bits + (size_t)BR * RS);          // [2][C + 1]: H(row above the sub-block, j0 - 1 ..)
    int *tF = tH + 2 * (C + 1);                                         // [2][C + 1]: F entering the sub-block's first row
    int16_t *s_scores = reinterpret_cast<int16_t *>(tF + 2 * (C + 1));  // [msize * msize]
    unsigned char *s_map = reinterpret_cast<unsigned char *>(s_scores + msize * msize);
    unsigned char *qsym = s_map + 256, *rsym = qsym + BR;               // mapped symbols of the tile's rows / columns
    for (int x = lane; x < 256; x += 64) s_map[x] = a.mapper[x];
    for (int x = lane; x < msize * msize; x += 64) s_scores[x] = a.scores[x];
    __syncthreads();

    const long long qb = a.qoff[pair], rb = a.roff[pair];
    const int ql = (int)(a.qoff[pair + 1] - qb), rl = (int)(a.roff[pair + 1] - rb);
    const uint8_t *q = a.qbuf + qb, *r = a.rbuf + rb;
    const pmx_record_t rec = a.recs[pair];
    const bool dead = *a.abort_word != 0 || (rec.flags & PMX_FLAG_RERUN);
    auto left = [&](int i) -> int { return i < 0 ? 0 : (a.col_pen ? -(open + i * ext) : 0); };      // H(i, -1); H(-1, -1) = 0
    auto top = [&](int j) -> int { return j < 0 ? 0 : (a.row_pen ? -(open + j * ext) : 0); };       // H(-1, j)

    // ---- lane 0: the walk's state and outputs ----
    uint32_t *o_end = a.ops ? a.ops + (a.slot_qoff[pair + 1] + a.roff[pair + 1] + pair + 1 - a.ops_base) : nullptr;
    int cnt = 0, tlen = 0, nM = 0, nS = 0, nL = 0;
    uint32_t cur_op = 0, cur_len = 0;
    auto digits = [](uint32_t v) -> int { int d = 1; while (v >= 10) { v /= 10; ++d; } return d; };
    auto flush = [&]() { if (cur_len) { ++cnt; o_end[-cnt] = (cur_len << 4) | cur_op; tlen += digits(cur_len) + 1; } };
    auto add_run = [&](uint32_t op, int len) {
        if (len <= 0 || !o_end) return;
        if (op == cur_op) cur_len += (uint32_t)len;
        else { flush(); cur_op = op; cur_len = (uint32_t)len; }
    };
    int i = rec.end_query, j = rec.end_ref, where = W_DIAG, rem = rec.score;
    int done = dead ? 1 : 0;
    if (!done && lane == 0 && a.mode == PMX_MODE_SG) {     // the unaligned tail beyond (end_query, end_ref): end gaps (not in the statistics)
        if (i + 1 == ql) add_run(OP_FOR_INS_STATE, rl - 1 - j);
        else if (j + 1 == rl) add_run(OP_FOR_DEL_STATE, ql - 1 - i);
    }

    while (!done) {                                        // (i, j, where, done are wave-uniform here)
        if (i < 0 || j < 0) {                              // one sequence is used up: the rest of the other is one gap run
            if (!SW && lane == 0) {
                if (i < 0 && j >= 0) { add_run(OP_FOR_INS_STATE, j + 1); if (a.row_pen) nL += j + 1; }
                else if (j < 0 && i >= 0) { add_run(OP_FOR_DEL_STATE, i + 1); if (a.col_pen) nL += i + 1; }
            }
            break;
        }
        // ---- re-derive tile (b, c) up to the entry cell (ie, je) ----
        const int b = i / BR, c = j >> a.ckshift, i0 = b * BR, j0 = c * C, ie = i, je = j;
        const int nrows = ie - i0 + 1, ncols = je - j0 + 1;
        const unsigned long long *bin = b ? a.bound + ((size_t)pair * a.nbmax + b - 1) * a.bstride : nullptr;
        const int2 *ckin = c ? a.ck + (((size_t)pair * a.nbmax + b) * (size_t)a.ckslots + (c - 1)) * BR : nullptr;
        __syncthreads();                                   // (the previous tile's walk is over: its LDS may be overwritten)
        for (int x = lane; x <= ncols; x += 64) {          // x = y - j0 + 1: H(i0 - 1, y) and F(i0, y), y = j0 - 1 .. je
            const int y = j0 - 1 + x;
            int h, f;
            if (!bin) { h = top(y); f = h - open; }
            else if (y < 0) { h = left(i0 - 1); f = T_NEG; }
            else {
                const unsigned long long g = bin[y];
                h = (int)(unsigned)(g & 0xFFFFFFFFu) - SKEW * (i0 + y) * ext + open;
                f = (int)(unsigned)(g >> 32) - SKEW * (i0 + y) * ext;
            }
            tH[x] = h; tF[x] = f;
        }
        for (int x = lane; x < nrows; x += 64) qsym[x] = s_map[q[i0 + x]];
        for (int x = lane; x < ncols; x += 64) rsym[x] = s_map[r[j0 + x]];
        __syncthreads();
        int cur = 0;
        for (int sb = 0; sb * 64 < nrows; ++sb, cur ^= 1) {
            const int xl = sb * 64 + lane, x = i0 + xl;   // this lane's row
            const bool row_on = xl < nrows;
            const int *cH = tH + cur * (C + 1), *cF = tF + cur * (C + 1);
            int *nH = tH + (cur ^ 1) * (C + 1), *nF = tF + (cur ^ 1) * (C + 1);
            int hl = 0, E = T_NEG;
            if (row_on) {
                if (!ckin) hl = left(x);
                else { const int2 p = ckin[xl]; hl = p.x - SKEW * (x + j0) * ext + open; E = p.y - SKEW * (x + j0 - 1) * ext; }
            }
            int diag = lane_prev<64>(cH[0], hl);           // H(x - 1, j0 - 1): the lane above, or the row above the sub-block
            if (lane == 63 && row_on) nH[0] = hl;
            const int qoffs = row_on ? (int)qsym[xl] * msize : 0;
            uint32_t acc = 0;
            int Hout = 0, Fout = 0;
            const int rows_here = nrows - sb * 64 < 64 ? nrows - sb * 64 : 64;
            const int steps = ncols + rows_here - 1;
            for (int t = 0; t < steps; ++t) {
                const int t0 = t < ncols ? t : ncols - 1;
                const int up = lane_prev<64>(cH[t0 + 1], Hout), F = lane_prev<64>(cF[t0 + 1], Fout);
                const int col = t - lane;
                if (row_on && col >= 0 && col < ncols) {
                    E = max(E - ext, hl - open);
                    const int d = diag + (int)s_scores[qoffs + rsym[col]];
                    int H = max(max(d, E), F);
                    uint32_t nb = (!(d >= E && d >= F) ? 8u : 0u) | (E > F ? 4u : 0u);
                    if (SW) H = max(H, 0);
                    const int Ho = H - open;
                    nb |= (Ho > E - ext ? 2u : 0u) | (Ho > F - ext ? 1u : 0u);
                    acc |= nb << (4 * (col & 7));
                    if ((col & 7) == 7 || col == ncols - 1) { bits[(size_t)xl * RS + (col >> 3)] = acc; acc = 0; }
                    diag = up; hl = H; Hout = H; Fout = max(F - ext, Ho);
                    if (lane == 63) { nH[col + 1] = H; nF[col + 1] = Fout; }
                }
            }
            __syncthreads();
        }
        // ---- walk the tile (lane 0) ----
        if (lane == 0) {
            while (i >= i0 && j >= j0) {
                const int t = (int)((bits[(size_t)(i - i0) * RS + ((j - j0) >> 3)] >> (4 * ((j - j0) & 7))) & 15u);
                if (where == W_DIAG) {
                    if (SW && rem <= 0) { done = 1; break; }                 // ZERO cell
                    if (t & 8) { where = (t & 4) ? W_INS : W_DEL; continue; }
                    const int sa = qsym[i - i0], sb2 = rsym[j - j0];
                    const int sc = s_scores[sa * msize + sb2];
                    nM += sa == sb2; nS += sc > 0; nL += 1;
                    add_run(sa == sb2 ? OP_EQ : OP_X, 1);
                    if (SW) rem -= sc;
                    --i; --j;
                } else if (where == W_INS) { add_run(OP_FOR_INS_STATE, 1); nL += 1; --j; where = W_INSR; }
                else if (where == W_DEL) { add_run(OP_FOR_DEL_STATE, 1); nL += 1; --i; where = W_DELR; }
                else if (where == W_INSR) { if (t & 2) { where = W_DIAG; rem += open; } else { where = W_INS; rem += ext; } }
                else { if (t & 1) { where = W_DIAG; rem += open; } else { where = W_DEL; rem += ext; } }
            }
            if (SW && where == W_DIAG && rem <= 0) done = 1;
        }
        i = __builtin_amdgcn_readfirstlane(i); j = __builtin_amdgcn_readfirstlane(j);
        where = __builtin_amdgcn_readfirstlane(where); done = __builtin_amdgcn_readfirstlane(done);
    }
    if (lane == 0) {
        if (a.stats) { pmx_stats_t s3; s3.matches = nM; s3.similar = nS; s3.length = nL; a.stats[pair] = s3; }
        if (o_end) { flush(); a.nops[pair] = cnt; a.textlen[pair] = tlen; }
    }
}

size_t pmx_walkt_lds_bytes(int msize, int BR, int tile_cols)
{
    return (size_t)BR * (tile_cols / 8 + 1) * 4 + (size_t)4 * (tile_cols + 1) * 4 + (size_t)msize * msize * 2 + 256 + BR + tile_cols + 16;
}

// 0 launched, 1 not eligible (LDS), <0 HIP error.  The scratch is the one pmx_launch_long filled for the same batch by the same plan.
int pmx_launch_walkt(const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext, const PmxLongPlan &p,
                     const void *scratch, const pmx_record_t *recs,
                     const int64_t *slot_qoff, long long ops_base, uint32_t *ops, int32_t *nops, int32_t *textlen,
                     pmx_stats_t *stats_out, hipStream_t stream)
{
    if (m.pssm || b.q_shared || b.n <= 0 || b.n > p.pairs || !p.ck || m.msize != p.msize || b.max_qlen > p.max_qlen || b.max_rlen > p.max_rlen) return 1;
    PmxWalktArgs a;
    a.qbuf = b.qbuf; a.qoff = b.qoff; a.rbuf = b.rbuf; a.roff = b.roff; a.n = b.n;
    a.mapper = m.mapper; a.scores = m.scores; a.msize = m.msize; a.open = open; a.ext = ext; a.mode = mode;
    const PmxEnds ends = pmx_ends(mode, sg_flags);
    a.col_pen = ends.col_pen; a.row_pen = ends.row_pen;
    a.recs = recs;
    const unsigned char *base = reinterpret_cast<const unsigned char *>(scratch);
    a.abort_word = reinterpret_cast<const int *>(base + p.off_abort);
    a.bound = reinterpret_cast<const unsigned long long *>(base + p.off_bound);
    a.bstride = p.bstride; a.nbmax = p.nbmax;
    a.ck = reinterpret_cast<const int2 *>(base + p.off_ck); a.ckslots = p.ckslots; a.ckshift = p.ckshift;
    a.BR = 64 * p.R;
    a.slot_qoff = slot_qoff; a.ops_base = ops_base; a.ops = ops; a.nops = nops; a.textlen = textlen; a.stats = stats_out;
    const size_t lds = pmx_walkt_lds_bytes(m.msize, a.BR, p.tile_cols);
    if (lds > 160 * 1024) return 1;
    if (mode == PMX_MODE_SW) {
        const int rc = pmx_ensure_lds_attr(reinterpret_cast<const void *>(&pmx_walkt_kernel<true>)); if (rc) return rc;
        hipLaunchKernelGGL((pmx_walkt_kernel<true>), dim3((unsigned)b.n), dim3(64), lds, stream, a);
    } else {
        const int rc = pmx_ensure_lds_attr(reinterpret_cast<const void *>(&pmx_walkt_kernel<false>)); if (rc) return rc;
        hipLaunchKernelGGL((pmx_walkt_kernel<false>), dim3((unsigned)b.n), dim3(64), lds, stream, a);
    }
    return pmx_launched();
}
