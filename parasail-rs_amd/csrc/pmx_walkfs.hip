// pmx_walkfs.hip -- on-device traceback walk over the decision bytes of the frameshift sweep's trace form
// (pmx_swfs_kernel<16,10,true>, pmx_swfs.hip; semantics: include/parasail_amd.h, "Frameshift traceback").  gfx950 only.
//
// The state machine of pmx_walkb.hip with the wider recurrence's six move kinds: from the record's end cell (end_query - 2, end_ref) in
// state H back to the START cell.  State H: a cell whose H came from M emits a match column ('=' where the two letters map to one matrix
// index, else 'X') and goes on by what D was -- START ends the path, IN-FRAME to (i - 3, j - 1), SHORT emits '/' and goes to
// (i - 2, j - 1), LONG emits '\' and goes to (i - 4, j - 1); a cell whose H came from F or E changes the state.  State F: one codon
// against a gap, to (i - 3, j), back to H where F was opened.  State E: one reference letter against a gap, to (i, j - 1), back to H
// where E was opened.  Run-length ops are written from the end of the pair's op slots backwards, as the other walks do.
//
// One lane per logical pair: the hits are few and a path is at most N / 3 + m dependent reads of one byte.  A pair's trace is the one of
// the slot that won the strand fold.  The walk reads only cells inside the slot's N x m matrix and stores at most as many ops as the
// pair's op slots hold; a step that would leave either ends the walk (the sweep's decisions never ask for one).
//
// REF (semantics: "Frameshift traceback, reference side"): the trace of pmx_swfsc_kernel<16,10,true>, the recurrence
// transposed.  The state machine is the same; the side changes four things -- the step vectors (a match column goes one row up and two
// to four columns back, F goes one row up, E three columns back), the start cell (end_query, end_ref - 2), the cell's address (stored by
// step: PMX_FSTRC_CELL) and which buffer holds the protein (the query's; the stream is the reference's).
// Plain C++, vector loads and stores only.
#include "pmx_common.h"

#define OP_EQ 7u
#define OP_X 8u
#define OP_FS_SHORT PMX_OP_FRAMESHIFT_SHORT           // '/': one nucleotide missing from the read
#define OP_FS_LONG PMX_OP_FRAMESHIFT_LONG             // the backslash: one nucleotide too many
#define OP_FOR_INS_STATE PMX_BAM_OP_FOR_INS_STATE    // E: a reference letter (REF: a whole reference codon) against a gap (include/pmx_conventions.h)
#define OP_FOR_DEL_STATE PMX_BAM_OP_FOR_DEL_STATE    // F: a codon (REF: a query letter) against a gap

template <bool REF>
__global__ __launch_bounds__(256)
void pmx_walkfs_kernel(const uint8_t *__restrict__ qbuf, const int64_t *__restrict__ qoff,
                       const uint8_t *__restrict__ rbuf, const int64_t *__restrict__ roff, long long n, int per,
                       const uint8_t *__restrict__ win, const uint8_t *__restrict__ mapper, const int16_t *__restrict__ scores, int msize,
                       int max_rlen, const pmx_record_t *__restrict__ recs, const uint8_t *__restrict__ trace, long long trace_stride,
                       uint32_t *__restrict__ ops, int32_t *__restrict__ nops, int32_t *__restrict__ textlen,
                       int64_t *__restrict__ pair_qoff, int64_t *__restrict__ pair_roff,
                       int32_t *__restrict__ beg, pmx_stats_t *__restrict__ stats_out)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const long long s0 = (long long)per * k, s1 = s0 + per;
    // the pair's op slots: the qlen + rlen + 1 entries of each of its slots, counted from the launch's first slot
    const long long q0 = qoff[0], r0 = roff[0];
    const long long o_beg = (qoff[s0] - q0) + (roff[s0] - r0) + s0, o_fin = (qoff[s1] - q0) + (roff[s1] - r0) + s1;
    if (k == 0) { pair_qoff[0] = 0; pair_roff[0] = 0; }
    pair_qoff[k + 1] = (qoff[s1] - q0) + (long long)(per - 1) * (k + 1);      // the render finds pair_qoff + pair_roff + k + 1 = o_fin
    pair_roff[k + 1] = roff[s1] - r0;
    uint32_t *o_end = ops + o_fin;
    const int cap = (int)(o_fin - o_beg);

    const pmx_record_t rec = recs[k];
    const long long slot = s0 + (win ? (long long)(win[k] & 1) : 0);
    const long long qb = qoff[slot], rb = roff[slot];
    const int N = (int)(qoff[slot + 1] - qb), m = min((int)(roff[slot + 1] - rb), max_rlen);
    const uint8_t *q = qbuf + qb, *r = rbuf + rb;
    const uint8_t *tb = trace + (size_t)slot * (size_t)trace_stride;
    // the decision byte of cell (i, j) (layout: pmx_common.h)
    auto cell = [&](int i, int j) -> unsigned {
        if (REF) return tb[PMX_FSTRC_CELL(i, j, max_rlen)];
        const int strip = i / PMX_FSTR_STRIP_ROWS, in = i - strip * PMX_FSTR_STRIP_ROWS, lane = in / PMX_FSTR_LANE_ROWS;
        return tb[((size_t)strip * max_rlen + j) * PMX_FSTR_COL_BYTES + lane * 12 + (in - lane * PMX_FSTR_LANE_ROWS)];
    };

    int cnt = 0, tlen = 0, nM = 0, nS = 0, nL = 0;
    uint32_t cur_op = 0, cur_len = 0;
    auto digits = [](uint32_t v) -> int { int d = 1; while (v >= 10) { v /= 10; ++d; } return d; };
    auto flush = [&]() { if (cur_len && cnt < cap) { ++cnt; o_end[-cnt] = (cur_len << 4) | cur_op; tlen += digits(cur_len) + 1; } };
    auto add = [&](uint32_t op) {
        if (op == cur_op) ++cur_len;
        else { flush(); cur_op = op; cur_len = 1; }
    };

    int bi = -1, bj = -1;
    if (!(rec.flags & PMX_FLAG_BAD_PAIR)) {
        int i = REF ? rec.end_query : rec.end_query - 2, j = REF ? rec.end_ref - 2 : rec.end_ref;
        bi = rec.end_query + 1; bj = rec.end_ref + 1;      // an empty path, as the local walks report it
        int where = 0;                                   // 0 H, 1 E, 2 F
        bool open_path = rec.score > 0;
        while (open_path && i >= 0 && j >= 0 && i < N && j < m) {
            const unsigned t = cell(i, j), src = t & 7u;
            if (where == 0) {
                if (src == PMX_FSTR_ZERO) break;
                if (src == PMX_FSTR_F) { where = 2; continue; }
                if (src == PMX_FSTR_E) { where = 1; continue; }
                const int a = mapper[q[i]], b = mapper[r[j]];
                add(a == b ? OP_EQ : OP_X);
                nM += a == b; nS += scores[a * msize + b] > 0; nL += 1;
                bi = i; bj = j;
                if (src == PMX_FSTR_START) open_path = false;
                else if (src == PMX_FSTR_INFRAME) (REF ? j : i) -= 3;
                else if (src == PMX_FSTR_SHORT) { add(OP_FS_SHORT); (REF ? j : i) -= 2; }
                else { add(OP_FS_LONG); (REF ? j : i) -= 4; }
                --(REF ? i : j);
            } else if (where == 1) {
                add(OP_FOR_INS_STATE); nL += 1;
                if (t & PMX_FSTR_EO) where = 0;
                j -= REF ? 3 : 1;
            } else {
                add(OP_FOR_DEL_STATE); nL += 1;
                if (t & PMX_FSTR_FO) where = 0;
                i -= REF ? 1 : 3;
            }
        }
    }
    flush();
    nops[k] = cnt;
    textlen[k] = tlen;
    if (beg) { beg[2 * k] = bi; beg[2 * k + 1] = bj; }
    if (stats_out) { pmx_stats_t s3; s3.matches = nM; s3.similar = nS; s3.length = nL; stats_out[k] = s3; }
}

int pmx_launch_walkfs(const PmxDevMatrix &m, long long n, int per, const uint8_t *win,
                      const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff, int max_rlen,
                      const pmx_record_t *recs, const uint8_t *trace, long long trace_bytes_per_slot,
                      uint32_t *ops, int32_t *nops, int32_t *textlen, int64_t *pair_qoff, int64_t *pair_roff,
                      int32_t *beg, pmx_stats_t *stats_out, hipStream_t stream, bool ref)
{
    if (m.pssm || (per != 1 && per != 2)) return 1;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(ref ? pmx_walkfs_kernel<true> : pmx_walkfs_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       qbuf, qoff, rbuf, roff, n, per, win,
                       m.mapper, m.scores, m.msize, max_rlen, recs, trace, trace_bytes_per_slot, ops, nops, textlen, pair_qoff, pair_roff,
                       beg, stats_out);
    return pmx_launched();
}
