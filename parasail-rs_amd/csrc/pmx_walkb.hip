// pmx_walkb.hip -- on-device traceback walk over the anti-diagonal trace records of the banded kernels' trace form
// (pmx_banded_staged_kernel / pmx_banded_kernel with a PmxBandTrace argument).  gfx950 only.
//
// Same state machine, tie priorities and outputs as pmx_walkp.hip (and oracle/pmx_oracle.c:orc_walk): from the record's end cell
// back to the beginning, run-length ops (BAM codes) written from the end of the pair's slot backwards, with their count and the
// text length -- or, in the statistics form, matches / similar / length along the path.  Local alignment stops where the path's
// score is used up (the value of the current H / E / F cell is tracked, as in pmx_walkp); global and semi-global alignment emit the
// boundary gaps once a sequence is exhausted, and semi-global the unaligned tail beyond the end cell.
//
// One lane per pair.  Cell (i, j) of the band (u = (j - i) - diag + band) is nibble u & 1 of byte (i - A + u / 2) * LP + u / 2 of
// the pair's region, A = (s0 + band - diag) / 2 (layout: pmx_common.h).  A path along a diagonal reads one lane's column of the
// region, LP bytes apart: eight or more consecutive cells share a cache line.  The walk reads only cells of the band inside the
// matrix; a step that would leave them ends the walk.
#include "pmx_common.h"
#include "pmx_strip.h"

#define OP_EQ 7u
#define OP_X 8u
#define OP_FOR_INS_STATE PMX_BAM_OP_FOR_INS_STATE    // include/pmx_conventions.h
#define OP_FOR_DEL_STATE PMX_BAM_OP_FOR_DEL_STATE    // include/pmx_conventions.h
#define B_NEG (INT32_MIN / 2)

// BG: also the cell where the walk stops -- the path's first cell (beg_query, beg_ref of oracle/pmx_oracle.c:orc_walk; 0 / 0 once a global
// or semi-global path has used up a sequence; -1 / -1 without a path) -- two ints per pair.  Without BG `beg` is not looked at.
template <bool ST, bool SW, bool BG>
__global__ __launch_bounds__(256)
void pmx_walkb_kernel(const uint8_t *__restrict__ qbuf, const int64_t *__restrict__ qoff, int q_shared,
                      const uint8_t *__restrict__ rbuf, const int64_t *__restrict__ roff, long long n,
                      const uint8_t *__restrict__ mapper, const int16_t *__restrict__ scores, int msize, int open, int ext,
                      int mode, int row_pen, int col_pen, int band, const int32_t *__restrict__ diag,
                      const pmx_record_t *__restrict__ recs, PmxBandTrace tr, int LP,
                      const int64_t *__restrict__ slot_qoff, long long ops_base, uint32_t *__restrict__ ops,
                      int32_t *__restrict__ nops, int32_t *__restrict__ textlen, pmx_stats_t *__restrict__ stats_out,
                      int32_t *__restrict__ beg)
{
    __shared__ unsigned char s_map[256];
    __shared__ int16_t s_scores[PMX_MAX_FAST_MSIZE * PMX_MAX_FAST_MSIZE];
    for (int x = threadIdx.x; x < 256; x += blockDim.x) s_map[x] = mapper[x];
    for (int x = threadIdx.x; x < msize * msize; x += blockDim.x) s_scores[x] = scores[x];
    __syncthreads();

    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const long long qb = q_shared ? 0 : qoff[k], rb = roff[k];
    const int ql = q_shared ? q_shared : (int)(qoff[k + 1] - qb), rl = (int)(roff[k + 1] - rb);
    const uint8_t *q = qbuf + qb, *r = rbuf + rb;
    const int d0 = diag ? diag[k] : 0;
    const pmx_record_t rec = recs[k];
    const PmxBandSteps bs = pmx_band_steps(ql, rl, band, d0);
    const int A = (bs.s0 + band - d0) >> 1;
    const uint8_t *tb = tr.buf + k * tr.stride;
    // the nibble ND NDL EO FO of cell (i, j); -1 outside the band or the matrix
    auto nib = [&](int i, int j) -> int {
        const int u = j - i - d0 + band;
        if (u < 0 || u > 2 * band || i < 0 || i >= ql || j < 0 || j >= rl) return -1;
        const int x = u >> 1, m = i - A + x;
        if (m < 0 || (long long)m * LP >= tr.stride) return -1;
        const unsigned b = tb[(size_t)m * LP + x];
        return (int)((u & 1) ? b >> 4 : b & 15u);
    };

    uint32_t *o_end = ST ? nullptr : ops + (slot_qoff[k + 1] + roff[k + 1] + k + 1 - ops_base);
    int cnt = 0, tlen = 0, nM = 0, nS = 0, nL = 0;
    uint32_t cur_op = 0, cur_len = 0;
    int bi = -1, bj = -1;
    auto digits = [](uint32_t v) -> int { int d = 1; while (v >= 10) { v /= 10; ++d; } return d; };
    auto flush = [&]() { if (cur_len) { ++cnt; o_end[-cnt] = (cur_len << 4) | cur_op; tlen += digits(cur_len) + 1; } };
    auto add_run = [&](uint32_t op, int len) {
        if (len <= 0) return;
        if (ST) { nL += len; return; }
        if (op == cur_op) cur_len += (uint32_t)len;
        else { flush(); cur_op = op; cur_len = (uint32_t)len; }
    };

    if (rec.score != B_NEG) {                            // (a band that misses the end cell: no path)
        int i = rec.end_query, j = rec.end_ref;
        if (mode == PMX_MODE_SG && !ST) {                // the unaligned tail beyond (end_query, end_ref): end gaps
            if (i + 1 == ql) add_run(OP_FOR_INS_STATE, rl - 1 - j);
            else if (j + 1 == rl) add_run(OP_FOR_DEL_STATE, ql - 1 - i);
        }
        int where = 0;                                   // 0 DIAG, 1 INS (E), 2 DEL (F)
        int rem = rec.score;                             // local alignment: value of the current H / E / F cell
        for (;;) {
            if (i < 0 || j < 0) {                        // one sequence is used up: the rest of the other is one gap run
                if (!SW) {
                    if (i < 0 && j >= 0 && !(ST && !row_pen)) add_run(OP_FOR_INS_STATE, j + 1);
                    else if (j < 0 && i >= 0 && !(ST && !col_pen)) add_run(OP_FOR_DEL_STATE, i + 1);
                }
                break;
            }
            if (where == 0) {
                if (SW && rem <= 0) break;               // ZERO cell
                const int t = nib(i, j);
                if (t < 0) break;
                if (t & 8) { where = (t & 4) ? 1 : 2; continue; }
                const int a = s_map[q[i]], b = s_map[r[j]];
                const int sc = s_scores[a * msize + b];
                if (ST) { nM += a == b; nS += sc > 0; nL += 1; }
                else add_run(a == b ? OP_EQ : OP_X, 1);
                if (SW) rem -= sc;
                --i; --j;
            } else if (where == 1) {                     // E(i, j) opened iff EO of (i, j - 1)
                add_run(OP_FOR_INS_STATE, 1);
                const int t = j > 0 ? nib(i, j - 1) : 0;
                if (t < 0) break;
                if (t & 2) { where = 0; rem += open; } else rem += ext;
                --j;
            } else {                                     // F(i, j) opened iff FO of (i - 1, j)
                add_run(OP_FOR_DEL_STATE, 1);
                const int t = i > 0 ? nib(i - 1, j) : 0;
                if (t < 0) break;
                if (t & 1) { where = 0; rem += open; } else rem += ext;
                --i;
            }
        }
        if (BG) {
            if (!SW && (i < 0 || j < 0)) i = j = -1;      // (the boundary gap run went to the matrix's corner)
            bi = i + 1; bj = j + 1;
        }
    }
    if (BG) { beg[2 * k] = bi; beg[2 * k + 1] = bj; }
    if (ST) { pmx_stats_t s3; s3.matches = nM; s3.similar = nS; s3.length = nL; stats_out[k] = s3; return; }
    flush();
    nops[k] = cnt;
    textlen[k] = tlen;
}

int pmx_launch_walkb(int mode, int sg_flags, int open, int ext, const PmxDevMatrix &m, long long n,
                     const uint8_t *qbuf, const int64_t *qoff, int q_shared, const uint8_t *rbuf, const int64_t *roff,
                     int band, const int32_t *diag, const pmx_record_t *recs, const PmxBandTrace &tr,
                     const int64_t *slot_qoff, long long ops_base, uint32_t *ops, int32_t *nops, int32_t *textlen,
                     pmx_stats_t *stats_out, hipStream_t stream, int32_t *beg)
{
    if (m.pssm) return 1;                                   // (symbol profiles only: a PSSM takes the general kernel)
    if (n <= 0) return 0;
    const PmxEnds ends = pmx_ends(mode, sg_flags);
    const int LP = pmx_bandtr_geometry_of(1, 1, band).LP;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#define WB2(STV, SWV, BGV) hipLaunchKernelGGL((pmx_walkb_kernel<STV, SWV, BGV>), grid, block, 0, stream, qbuf, qoff, q_shared, rbuf, roff, n, \
        m.mapper, m.scores, m.msize, open, ext, mode, ends.row_pen, ends.col_pen, band, diag, recs, tr, LP, slot_qoff, ops_base, ops, nops, textlen, stats_out, beg)
#define WB(STV, SWV) do { if (beg) WB2(STV, SWV, true); else WB2(STV, SWV, false); } while (0)
    const bool sw = mode == PMX_MODE_SW;
    if (stats_out) { if (sw) WB(true, true); else WB(true, false); }
    else { if (sw) WB(false, true); else WB(false, false); }
#undef WB
#undef WB2
    return pmx_launched();
}

__global__ void pmx_shared_offsets_kernel(int64_t *off, long long n, int qlen)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= n) off[k] = k * qlen;
}
int pmx_launch_shared_offsets(int64_t *off, long long n, int qlen, hipStream_t stream)
{
    hipLaunchKernelGGL(pmx_shared_offsets_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, off, n, qlen);
    return pmx_launched();
}
