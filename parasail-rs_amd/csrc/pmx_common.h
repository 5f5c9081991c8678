// pmx_common.h -- internal declarations shared by the HIP kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/parasail_amd.h"
#include "../../include/pmx_conventions.h"

#define PMX_MAX_FAST_MSIZE 32      // fast kernels stage the matrix in LDS as int16[msize*msize]

// Raise the dynamic-LDS limit of a kernel once per (kernel, device); thread-safe.
int pmx_ensure_lds_attr(const void *kernel, int bytes = 160 * 1024);

// What a launcher returns behind its launch: 0, or the launch's HIP error negated.
static inline int pmx_launched() { const hipError_t e = hipGetLastError(); return e == hipSuccess ? 0 : -(int)e; }

// Device-side view of a substitution matrix (built once per parasail_matrix_t, cached).
struct PmxDevMatrix {
    const int16_t *scores;   // [rows*msize]: scores[qsym*msize + rsym], or for a PSSM scores[i*msize + rsym] (query row i)  (device)
    const uint8_t *mapper;   // [256] byte -> symbol index                  (device)
    int msize;
    int min, max;
    int pssm;                // 1: a PSSM of `rows` query positions; only the kernels that declare a PSSM form take one
    int rows;                // rows of `scores`: msize, or the PSSM's length
};

// Batch of pairs, device-resident, packed layout of include/parasail_amd.h.
struct PmxBatch {
    const uint8_t *qbuf; const int64_t *qoff;
    const uint8_t *rbuf; const int64_t *roff;
    int64_t n;
    int max_qlen, max_rlen;
    int q_shared;            // > 0: one shared query of that many bytes at qbuf (profile arm), qoff unused
    const unsigned *perm;    // optional processing order (pmx_sort.hip): position -> pair index
    unsigned *retry_list;    // optional scratch, n entries + one int: lets the sw16 launcher use kernels that hand
    int *retry_count;        //   some pairs back for a second launch (decided on the device, no host sync)
    int q_has_wildcard;      // shared query only: it holds a letter beyond the first four of the alphabet
    int sat_above;           // sw16 only, 0 = off: scores above this set PMX_FLAG_SATURATED (width 8: 127; local H >= 0, so the
                             //   maximum H is the score and the oracle's saturation rule needs nothing else)
    int track8;              // nwsg16v only: width 8 -- track the range of H and flag pairs that leave [-128, 127]
    int *blockflag;          // nwsg16v only, optional scratch of (n + 15) / 2 ints: lets the launcher run the perm-table form first, which
                             //   marks the blocks (of 2 * 64 / G pairs) it leaves to the LDS-profile form; the walk reads the flags too
};
#define PMX_FLAG_RETRY16 4   // internal record flag: redo with the LDS-profile variant of the fast kernel
#define PMX_FLAG_STRAND1 0x40000000   // internal record flag, chunk scratch of the stranded searches only: the record is the reverse strand's
// internal record flags, chunk scratch of the translated searches only: three bits that hold the frame of the record
#define PMX_FLAG_FRAME_SHIFT 27
#define PMX_FLAG_FRAME_MASK 0x38000000

// Fast path: local alignment, score + end positions, packed int16 lanes.
// Returns 0 if launched, 1 if the shape is not supported by any instantiation (caller falls
// through to the general kernel), <0 on a HIP error.
int pmx_launch_sw16(const PmxBatch &b, const PmxDevMatrix &m, int open, int ext,
                    pmx_record_t *d_out, hipStream_t stream, const char **kernel_name);

// A planned traceback sweep: what its launcher, the walk behind it and the caller's chunking need to know.  The planners fill it
// (0 planned, 1 not eligible: *p untouched) and call no HIP function; the launch entries take it back (0 launched, 1 not eligible,
// <0 HIP error) and name the sweep that really ran through *kernel_name.  GEN1: pmx_trace16_kernel, one pair per lane group, R / 8
// trace words per lane and step; the others, packed: two pairs per group, (R + 3) / 4 * 4 bytes per lane and step (SW16: VAR 7).
enum PmxTraceFamily { PMX_TRACE_GEN1, PMX_TRACE_NWSG16V, PMX_TRACE_NWSG16M, PMX_TRACE_SW16, PMX_TRACE_SW16M, PMX_TRACE_NWSG16Q };
enum PmxTraceWalk { PMX_TRACE_WALK16, PMX_TRACE_WALKP };     // pmx_walk16_kernel (pmx_trace16.hip) / pmx_walkp_kernel (pmx_walkp.hip)
struct PmxTracePlan {
    PmxTraceFamily family;
    int G, R;                // lanes per pair (group), query rows per lane
    int pairs_per_wg;
    int Tmax;                // steps of a lane's trace stream (the packed sweeps: a multiple of 16, the walk reads windows of 16 records)
    size_t trace_bytes;      // trace scratch for the planned b.n pairs
    bool top_aligned;        // the query's rows start at the first lane's first row (local sweeps); else they end at the last lane's last
    bool fills_blockflag;    // the launcher fills PmxBatch::blockflag (0 = a block with top-aligned rows) and the walk reads it
    PmxTraceWalk walk;
};
// The plan of a packed sweep of shape <G, R> with `waves` waves per workgroup over n pairs whose longest reference takes `steps` steps.
static inline PmxTracePlan pmx_packed_trace_plan(PmxTraceFamily family, int G, int R, int waves, int steps, long long n)
{
    PmxTracePlan p;
    p.family = family; p.G = G; p.R = R; p.pairs_per_wg = 2 * (64 / G) * waves;
    p.Tmax = (steps + 15) & ~15;
    p.trace_bytes = (size_t)((n + p.pairs_per_wg - 1) / p.pairs_per_wg) * (size_t)waves * (size_t)p.Tmax * 64 * (size_t)((R + 3) / 4 * 4);
    p.top_aligned = family == PMX_TRACE_SW16 || family == PMX_TRACE_SW16M; p.fills_blockflag = family == PMX_TRACE_NWSG16V; p.walk = PMX_TRACE_WALKP;
    return p;
}

// The lane groups G0, 2 G0, .. 64 of the per-pair packed trace shapes <G, 16>, smallest first: f(G) with G an integral constant until
// one returns true.  Planner and launcher of a family walk the same list.
template <int G0, typename F> static inline bool pmx_for_each_trace_group(F &&f)
{
    if constexpr (G0 <= 64) return f(std::integral_constant<int, G0>{}) || pmx_for_each_trace_group<2 * G0>(f);
    else return false;
}

// Traceback variant of the local kernel (pmx_sw16.hip, VAR 7; large alphabets: pmx_sw16m.hip): same trace layout, rows top-aligned.
int pmx_sw16_trace_plan(const PmxBatch &b, const PmxDevMatrix &m, int open, int ext, PmxTracePlan *p);
int pmx_launch_sw16_trace(const PmxTracePlan &p, const PmxBatch &b, const PmxDevMatrix &m, int open, int ext,
                          pmx_record_t *d_out, uint32_t *tbuf, hipStream_t stream, const char **kernel_name);

// Bias of the second-generation nw/sg arithmetic (0: its exact window does not hold for this batch).
int pmx_nwsgv_bias(const PmxBatch &b, const PmxDevMatrix &m, int open, int ext, int rowx = 0, int shape_rows = 0 /* > 0: the rows of the shape that will run */);
// Packed statistics kernel (pmx_stats16p.hip): 0 launched, 1 not eligible, <0 HIP error.
int pmx_launch_stats16p(const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext,
                        pmx_record_t *d_out, pmx_stats_t *d_stats, hipStream_t stream, const char **kernel_name);

// Traceback variant of the second-generation nw/sg kernel (pmx_nwsg16.hip); the walk lives in pmx_trace16.hip.
// (*kernel_name: kernel + "/packed trace" + the decision form, "/bfi" or "/shift", + "/permtable ..." where that form ran first)
int pmx_nwsgv_trace_plan(const PmxBatch &b, const PmxDevMatrix &m, int mode, int open, int ext, PmxTracePlan *p);
int pmx_launch_nwsgv_trace(const PmxTracePlan &p, const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext,
                           pmx_record_t *d_out, uint32_t *tbuf, hipStream_t stream, const char **kernel_name);

// Traceback with a shared query (pmx_nwsg16q_kernel<..., TR>): statistics of the profile arm are counted along the path.
long long pmx_nwsgq_trace_round_pairs(const PmxTracePlan &p, const PmxDevMatrix &m, int mode, int sg_flags);
int pmx_nwsgq_trace_plan(const PmxBatch &b, const PmxDevMatrix &m, int mode, int open, int ext, PmxTracePlan *p, int short_waves = 0);
int pmx_launch_nwsgq_trace(const PmxTracePlan &p, const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext,
                           pmx_record_t *d_out, uint32_t *tbuf, hipStream_t stream, const char **kernel_name);

// Shared-query variant of the local kernel (pmx_sw16q.hip); called by pmx_launch_sw16 once the skewed byte-profile
// variant's conditions hold.  0 launched, 1 not eligible, <0 HIP error.
int pmx_launch_sw16q(const PmxBatch &b, const PmxDevMatrix &m, int open, int ext,
                     pmx_record_t *d_out, hipStream_t stream, const char **kernel_name);

// Matrix-lookup variant of the local kernel for per-pair queries over large alphabets (pmx_sw16m.hip); same contract.
int pmx_launch_sw16m(const PmxBatch &b, const PmxDevMatrix &m, int open, int ext,
                     pmx_record_t *d_out, hipStream_t stream, const char **kernel_name);

int pmx_launch_sw16m_trace(const PmxTracePlan &p, const PmxBatch &b, const PmxDevMatrix &m, int open, int ext,
                           pmx_record_t *d_out, uint32_t *tbuf, hipStream_t stream);

// 2-bit packed input -> ASCII letters (pmx_sort.hip)
int pmx_launch_unpack2(const uint8_t *in, uint8_t *out, long long lo, long long hi, uint32_t letters, hipStream_t stream);

// Length-sorted processing order for ragged batches (pmx_sort.hip).
size_t pmx_sort_scratch_bytes(long long n);
int pmx_build_length_perm(const int64_t *d_roff, long long n, void *scratch, const unsigned **perm_out, hipStream_t stream);
// Processing order for banded batches: by the number of anti-diagonal steps of each pair's band (same scratch size).
int pmx_build_band_perm(const int64_t *d_qoff, int q_shared, const int64_t *d_roff, const int32_t *d_diag, int band, long long n,
                        void *scratch, const unsigned **perm_out, hipStream_t stream, bool by_entry_row = false);

// Fast path: global / semi-global, score + end positions, biased packed lanes (pmx_nwsg16.hip).
int pmx_launch_nwsg16(const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext,
                      pmx_record_t *d_out, hipStream_t stream, const char **kernel_name);

// Fast path with statistics (pmx_stats16.hip): matches / similar / length travel with H, E, F.
int pmx_launch_stats16(const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext,
                       pmx_record_t *d_out, pmx_stats_t *d_stats, hipStream_t stream, const char **kernel_name);

// Fast path with traceback (pmx_trace16.hip): 4-bit trace in HBM + on-device walk -> run-length ops.
int pmx_trace16_plan(const PmxBatch &b, const PmxDevMatrix &m, int mode, int open, int ext, PmxTracePlan *p, bool packed_ok = true /* false: first generation only */);
// Walk over the packed records (pmx_walkp.hip).  ops: run-length BAM ops written from the END of the pair's slot backwards
// (slot = ops_off[k] .. + qlen + rlen + 1, or implicit: qoff[k] + roff[k] + k - ops_base): the forward list is the last nops[k] entries.
int pmx_launch_walkp(int G, int R, const PmxBatch &b, const PmxDevMatrix &m, int mode, int open, int ext, int Tmax, int top_aligned,
                     pmx_stats_t *stats_out, int row_pen, int col_pen, const uint32_t *tbuf, const pmx_record_t *recs,
                     uint32_t *ops, const int64_t *ops_off, long long ops_base, int32_t *nops, int32_t *beg, int32_t *textlen,
                     hipStream_t stream, const int *blockflag = nullptr /* per sweep block: 0 = top-aligned rows (perm-table sweep) */);
// Optional second stream for the walk (device CIGAR entry: the walk of chunk c runs beside the sweep of chunk c+1).
struct PmxWalkSplit {
    hipStream_t walk_stream;   // == the sweep's stream: no split
    hipEvent_t sweep_done;     // recorded on the sweep stream after the sweep, awaited by the walk stream
    hipEvent_t walk_done;      // recorded after the walk (may be null)
    long long ops_base;        // ops_off == nullptr: slot of pair k starts at qoff[k] + roff[k] + k - ops_base
    int32_t *textlen;          // optional, per pair: bytes of its CIGAR text
};
// The planned sweep and its walk; *sweep_name: the sweep as its launcher named it.
int pmx_launch_trace16(const PmxTracePlan &p, const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext,
                       pmx_record_t *d_out, uint32_t *tbuf, uint32_t *ops, const int64_t *ops_off, int32_t *nops, int32_t *beg, hipStream_t stream,
                       const char **sweep_name, pmx_stats_t *stats_out = nullptr /* count the path's statistics instead of emitting ops */,
                       const PmxWalkSplit *split = nullptr);

// ---- general kernel (all modes, stats, tables, rows/cols, trace, band) -------------------
struct PmxGeneralArgs {
    // inputs
    const uint8_t *qbuf; const int64_t *qoff;     // qoff == nullptr: one shared query of shared_qlen bytes at qbuf
    const uint8_t *rbuf; const int64_t *roff;
    long long n;
    int max_rlen;             // longest reference in the launch (sizes the LDS symbol buffer)
    const int64_t *index;     // optional: block b works on pair index[b] (promotion re-runs); n = number of blocks
    int shared_qlen;
    const int16_t *scores; const uint8_t *mapper; int msize;
    int mat_rows;             // rows of `scores`: msize for a square matrix, query length for a PSSM
    int pssm;                 // 1: row of `scores` is the query position, not the query symbol
    int mode, sg_flags, open, ext;
    int band;                 // < 0: no band; else cells with |(j - i) - diag[pair]| > band are excluded (nw_banded: diag == nullptr)
    const int32_t *diag;      // optional per-pair band centre (indexed like roff)
    int bits;                 // 0/32/64: no range check; 8 or 16: report saturation of that range
    // per-pair scratch: boundary row between 64-row bands, 8 ints per reference column
    int32_t *bound; long long bound_stride;       // ints per pair
    // optional per-block scratch (max_rlen + 8 bytes each) for references that do not fit the LDS; see pmx_general_lds_fits()
    uint8_t *rs_scratch; long long rs_stride;
    // outputs (device); any may be null
    pmx_record_t *rec; pmx_stats_t *stats;
    // table-like outputs: cell offset of pair k is tab_off[k] (nullptr -> pair 0 at 0, n must be 1)
    const int64_t *tab_off;
    int32_t *score_table, *matches_table, *similar_table, *length_table;
    int8_t *trace_table;
    int trace_lds;            // set by the launcher: stage one band of trace bytes in LDS, flush coalesced
    int max_qlen;             // longest query of the launch (0: unknown); lets the launcher share one long pair among several waves
    int mw_sched_off;         // set by the launcher (multi-wave form): LDS offset of the band schedule
    // row/col outputs: row offset = roff[k], col offset = qoff[k] (or 0 for n == 1)
    int32_t *score_row, *matches_row, *similar_row, *length_row;
    int32_t *score_col, *matches_col, *similar_col, *length_col;
};
int pmx_launch_general(const PmxGeneralArgs &a, bool want_stats, hipStream_t stream);
// true if the general kernel can keep a reference of max_rlen symbols (and the matrix) in the LDS; otherwise rs_scratch is needed
static inline bool pmx_general_lds_fits(int mat_rows, int msize, int max_rlen)
{
    return ((((size_t)mat_rows * msize * 2 + 15) & ~(size_t)15) + (((size_t)max_rlen + 8 + 15) & ~(size_t)15)) <= 160 * 1024;
}

// Banded fast kernel (pmx_banded.hip): lanes over the band's diagonals, one query row per step, only the band's cells are
// computed.  0 launched, 1 not eligible (the general kernel masks instead), <0 HIP error.
int pmx_launch_banded(int mode, int sg_flags, int open, int ext, const PmxDevMatrix &m, long long n,
                      const uint8_t *qbuf, const int64_t *qoff, int q_shared, const uint8_t *rbuf, const int64_t *roff,
                      int max_qlen, int max_rlen, int band, const int32_t *diag, pmx_record_t *out, hipStream_t stream, const char **kernel_name = nullptr,
                      void *sort_scratch = nullptr /* pmx_sort_scratch_bytes(n) bytes: lets the packed forms pair up bands of equal length */,
                      unsigned *retry_list = nullptr, int *retry_count = nullptr /* [count][n entries] twice (retry_count first): lets the band-strip kernel hand pairs back */);
// Trace form of the 32-bit banded kernels (pmx_banded.hip) and its walk (pmx_walkb.hip).  Layout: a pair's steps s = i + j are
// counted from the even origin s0 (s0 + band - d0 even, s0 = s_first or s_first - 1); on step s lane x of the pair's lane group holds
// band diagonal u = 2x + ((s - s0) & 1), and step pair m = (s - s0) / 2 of lane x is the byte buf[pair * stride + m * LP + x]: the
// nibble ND NDL EO FO (as in pmx_walkp.hip) of the even step low, of the odd step high.  Every cell of step pair m lies in row
// m + (s0 + band - d0) / 2 - x.
struct PmxBandTrace { uint8_t *buf; long long stride; };
// Step range of one pair's band: the band's cells inside the matrix lie on steps s_first .. s_last (s_last = -1: none); rows = the
// pair's step pairs from s0.
struct PmxBandSteps { int s_first, s_last, s0, rows; };
__host__ __device__ inline PmxBandSteps pmx_band_steps(int ql, int rl, int band, int d0)
{
    PmxBandSteps r;
    const int dlo = d0 - band, dhi = d0 + band;
    r.s_first = dlo > 0 ? dlo : dhi < 0 ? -dhi : 0;
    int i1 = ql - 1, j1 = rl - 1;
    if (j1 - i1 > dhi) j1 = i1 + dhi; else if (j1 - i1 < dlo) i1 = j1 - dlo;
    r.s_last = (i1 >= 0 && j1 >= 0 && !(dlo > rl - 1 || dhi < -(ql - 1))) ? i1 + j1 : -1;
    r.s0 = r.s_first - ((r.s_first + band - d0) & 1);
    r.rows = r.s_last >= r.s0 ? ((r.s_last - r.s0) >> 1) + 1 : 0;
    return r;
}
// The one bound of a launch (exported as the test hook pmx_bandtr_geometry): LP lanes per pair, at most `rows` step pairs per pair
// of up to max_qlen x max_rlen (any centre), stride = rows * LP bytes per pair region.  Scratch sizing and walk addressing use it.
struct PmxBandTrGeometry { int LP, rows; long long stride; };
PmxBandTrGeometry pmx_bandtr_geometry_of(int max_qlen, int max_rlen, int band);
// The traced sweep: staged form where both sequences fit the LDS, else the checked form.  0 launched, <0 HIP error.
int pmx_launch_banded_trace(int mode, int sg_flags, int open, int ext, const PmxDevMatrix &m, long long n,
                            const uint8_t *qbuf, const int64_t *qoff, int q_shared, const uint8_t *rbuf, const int64_t *roff,
                            int max_qlen, int max_rlen, int band, const int32_t *diag, pmx_record_t *out, const PmxBandTrace &tr,
                            hipStream_t stream, const char **kernel_name);
// Walk over the traced band (pmx_walkb.hip): ops (pmx_walkp's slot format; slot of pair k ends at slot_qoff[k + 1] + roff[k + 1] + k + 1
// - ops_base) with nops / textlen, or the path's statistics (stats_out != nullptr).  0 launched, <0 HIP error.
int pmx_launch_walkb(int mode, int sg_flags, int open, int ext, const PmxDevMatrix &m, long long n,
                     const uint8_t *qbuf, const int64_t *qoff, int q_shared, const uint8_t *rbuf, const int64_t *roff,
                     int band, const int32_t *diag, const pmx_record_t *recs, const PmxBandTrace &tr,
                     const int64_t *slot_qoff, long long ops_base, uint32_t *ops, int32_t *nops, int32_t *textlen,
                     pmx_stats_t *stats_out, hipStream_t stream, int32_t *beg = nullptr /* two ints per pair: the path's first cell */);
// off[k] = k * qlen, k = 0 .. n: the query offsets a shared query stands for (slot placement of the profile arm).
int pmx_launch_shared_offsets(int64_t *off, long long n, int qlen, hipStream_t stream);
// Band-strip kernel (pmx_bstrip.hip): band coordinates, packed int16, alphabets of <= 4 letters (+ wildcard).  Same contract.
int pmx_launch_bstrip(int mode, int sg_flags, int open, int ext, const PmxDevMatrix &m, long long n,
                      const uint8_t *qbuf, const int64_t *qoff, int q_shared, const uint8_t *rbuf, const int64_t *roff,
                      int max_qlen, int max_rlen, int band, const int32_t *diag, pmx_record_t *out, hipStream_t stream,
                      const char **kernel_name, void *sort_scratch, unsigned *retry_list, int *retry_count);

// Score tables / last rows and columns, row by row at HBM write speed (pmx_table.hip).  0 launched, 1 not eligible, <0 HIP error.
int pmx_launch_table(int mode, int sg_flags, int open, int ext, const PmxDevMatrix &m, long long n,
                     const uint8_t *qbuf, const int64_t *qoff, int q_shared, const uint8_t *rbuf, const int64_t *roff,
                     int max_qlen, int max_rlen, const int64_t *tab_off, int32_t *table, int32_t *row_out, int32_t *col_out,
                     pmx_record_t *out, hipStream_t stream, int8_t *trace = nullptr);

// On-device traceback walk: trace tables -> run-length ops (BAM-encoded uint32 per run).
// ops_off[k] = first slot of pair k in `ops` (capacity qlen+rlen each), nops[k] = runs written.
struct PmxWalkArgs {
    const uint8_t *qbuf; const int64_t *qoff; const uint8_t *rbuf; const int64_t *roff;
    long long n; int shared_qlen;
    const uint8_t *mapper; int mode;
    const int8_t *trace_table; const int64_t *tab_off;
    const pmx_record_t *rec;
    uint32_t *ops; const int64_t *ops_off; int32_t *nops; int32_t *beg; /* 2 per pair */
};
int pmx_launch_walk(const PmxWalkArgs &a, hipStream_t stream);
int pmx_launch_cigar_textlen(const uint32_t *ops, const int64_t *ops_off, const int32_t *nops, int32_t *textlen, long long n, hipStream_t stream);
int pmx_launch_cigar_render(const uint32_t *ops, const int64_t *ops_off, const int32_t *nops,
                            const int64_t *text_off, char *text, long long n, hipStream_t stream);
// Device CIGAR entry: exclusive scan of the per-pair text lengths (n + 1 entries in, the last one ignored) into int64
// offsets (n + 1 entries out, the last one = total bytes), and the render with implicit op slots and a capacity limit.
size_t pmx_text_scan_scratch_bytes(long long n);
int pmx_launch_text_offsets(const int32_t *textlen, long long n, int64_t *text_off, void *scratch, size_t scratch_bytes, hipStream_t stream);
int pmx_launch_cigar_render_slots(const uint32_t *ops, const int64_t *qoff, const int64_t *roff, long long ops_base, const int32_t *nops,
                                  const int64_t *text_off, char *text, long long capacity, long long n, hipStream_t stream);

// Hit selection and reference gather of the profile search (pmx_select.hip; semantics: include/parasail_amd.h).  `scratch` holds
// pmx_select_scratch_bytes() bytes.  All asynchronous on `stream`; 0 launched, <0 HIP error.
size_t pmx_select_scratch_bytes(long long n, long long max_hits, int order);
int pmx_launch_select(const pmx_record_t *recs, long long n, int min_score, long long max_hits, int order,
                      int64_t *hit_index, long long capacity, int64_t *counts, void *scratch, hipStream_t stream);
// diag[p] = end_ref - end_query and hlen[p] = reference length of hit idx[p], p < min(counts[0], cap); 0 up to hlen[cap + 1]
int pmx_launch_hit_lengths(const int64_t *idx, const int64_t *counts, long long cap, const pmx_record_t *recs, const int64_t *roff,
                           int32_t *diag, int32_t *hlen, hipStream_t stream);
int pmx_launch_hit_records(const int64_t *idx, const pmx_record_t *recs, const int32_t *diag, long long h, pmx_hit_t *hits, hipStream_t stream);
int pmx_launch_hit_begins(const int32_t *beg, long long h, pmx_hit_t *hits, hipStream_t stream);
int pmx_launch_gather_refs(const uint8_t *rbuf, const int64_t *roff, long long n, const int64_t *idx, long long h,
                           uint8_t *out, const int64_t *ooff, long long out_cap, hipStream_t stream);

// Sequence-set batches (pmx_pairs.hip; semantics: include/parasail_amd.h).  All asynchronous on `stream`; 0 launched, <0 HIP error.
// resolve: n descriptors -> per * n alignment slots (per 1 or 2), slot per * k + i on the strand s0 + i, s0 = strand ? strand[k] : first
// (strand: n bytes or NULL).  qlen / rlen hold per * n + 2 entries (the scan's input), qsrc / rsrc / ok / sflag per * n; sflag = the
// slot's strand, NULL where none is kept (the plain entries: strand NULL, first 0, per 1).  A bad descriptor and a strand s0 + per > 2
// make every slot of the pair 1 x 1 with ok = 0.  The _ex entries: a strand byte per pair, per 1.  The strand chosen by the entry
// (DESIGN 2.5h): per 1 all reverse (first 1); per 2 slot 2 k forward, 2 k + 1 reverse (first 0).
int pmx_launch_pairs_resolve(const pmx_pair_t *pairs, const uint8_t *strand, int first, int per, long long n,
                             const int64_t *q_off, long long q_count, long long q_bytes,
                             const int64_t *r_off, long long r_count, long long r_bytes, int32_t max_qlen, int32_t max_rlen,
                             int32_t *qlen, int32_t *rlen, int64_t *qsrc, int64_t *rsrc, uint8_t *ok, uint8_t *sflag, hipStream_t stream);
int pmx_launch_pairs_gather(long long n, const uint8_t *q_buf, long long q_bytes, const uint8_t *r_buf, long long r_bytes,
                            const int32_t *qlen, const int32_t *rlen, const int64_t *qsrc, const int64_t *rsrc, const uint8_t *ok,
                            const int64_t *qoff, const int64_t *roff, uint8_t *qout, uint8_t *rout, hipStream_t stream);
int pmx_launch_pairs_fixup(const uint8_t *ok, long long n, pmx_record_t *rec, pmx_stats_t *stats /* may be NULL */, hipStream_t stream);
// The gather that can reverse-complement the query side (sflag); a window whose end would cross q_cap / r_cap is not written.
int pmx_launch_pairs_gather_stranded(long long n, const uint8_t *q_buf, long long q_bytes, const uint8_t *r_buf, long long r_bytes,
                                     const int32_t *qlen, const int32_t *rlen, const int64_t *qsrc, const int64_t *rsrc, const uint8_t *ok,
                                     const uint8_t *sflag, const int64_t *qoff, const int64_t *roff,
                                     uint8_t *qout, long long q_cap, uint8_t *rout, long long r_cap, hipStream_t stream);
// Bad pairs of a chunk on the device CIGAR road, between the walk and the text scan: record, no ops, no text, begins -1 / -1 (beg may be NULL).
int pmx_launch_pairs_fixup_cigar(const uint8_t *ok, long long n, pmx_record_t *rec, int32_t *nops, int32_t *textlen, int32_t *beg, hipStream_t stream);
// A chunk's text offsets behind the running total: text_off[j] = text_off[0] + local[j], j = 1 .. n (text_off[0] is the total so far).
int pmx_launch_text_rebase(const int64_t *local, long long n, int64_t *text_off, hipStream_t stream);
void pmx_complement_table_host(uint8_t table[256]);
int pmx_launch_all_pairs_enumerate(long long nseq, long long first, long long count, pmx_pair_t *pairs, hipStream_t stream);
// Set search.  rect: pair first + t of Q x nr, row-major.  append_hits: the chunk's hits idx[0 .. chunk_counts[0]) (chunk-local,
// ascending; n = the chunk's pairs) go behind the counts[0] hits before them, below `capacity`: descriptor (hit_pairs, optional), index0 +
// position (hit_index, optional), record, statistics (optional); then counts[0] += chunk_counts[0], counts[1] = min(counts[0], capacity),
// in that order on `stream`.  first_bad[0] = min(first_bad[0], index0 + k) over the bad pairs of a chunk.
int pmx_launch_rect_pairs_enumerate(long long nr, long long first, long long count, pmx_pair_t *pairs, hipStream_t stream);
int pmx_launch_pairs_append_hits(const int64_t *idx, const int64_t *chunk_counts, long long n, long long capacity, long long index0,
                                 const pmx_pair_t *pairs, const pmx_record_t *rec, const pmx_stats_t *stats,
                                 pmx_pair_t *hit_pairs, int64_t *hit_index, pmx_record_t *hit_recs, pmx_stats_t *hit_stats, int64_t *counts, hipStream_t stream,
                                 uint8_t *hit_strand = nullptr /* optional: the strand byte of every hit written */,
                                 int marked = 0 /* 1: the records carry PMX_FLAG_STRAND1, 2: their frame in PMX_FLAG_FRAME_MASK; to be taken out */);
// fold: per * n slot records (statistics optional) -> n records, statistics, the winners' sflag bytes -- a strand or a frame -- (optional)
// and validity bytes (optional): of the slots with ok != 0 the highest score, the lowest slot on a tie; a pair without one gets its
// bad-pair record here.  mark 1: PMX_FLAG_STRAND1 is set in the records of winners with a byte other than 0; mark 2: the byte rides
// in PMX_FLAG_FRAME_MASK (the `marked` of pmx_launch_pairs_append_hits).
int pmx_launch_pairs_fold(const pmx_record_t *slot_rec, const pmx_stats_t *slot_stats, const uint8_t *ok, const uint8_t *sflag,
                          long long n, int per, int mark, pmx_record_t *rec, pmx_stats_t *stats, uint8_t *byte, uint8_t *okf, hipStream_t stream);
int pmx_launch_pairs_first_bad(const uint8_t *ok, long long n, long long index0, int64_t *first_bad, hipStream_t stream);
// A translated side (the query; 2.5j, ref = true: the reference).  resolve_frames: n descriptors -> per * n slots, slot
// per * k + i the frame (frame ? frame[k] : first + i); the translated side's length = the translated length L, tw = its nucleotide
// window's length W, its source = the window's first byte, sflag = the frame byte, ok = the slot is a candidate (a frame that does not
// exist, and every slot of a bad pair, is a 1 x 1 placeholder with ok = 0); arrays sized per * n (+ 2 for the lengths).
// gather_translated: the stranded gather with codon -> letter on the translated side.  The slots' records fold with pmx_launch_pairs_fold.
struct PmxCodeTable { uint8_t v[64]; };
void pmx_genetic_code_host(uint8_t table[64]);
int pmx_launch_pairs_resolve_frames(const pmx_pair_t *pairs, const uint8_t *frame, int first, int per, long long n,
                                    const int64_t *q_off, long long q_count, long long q_bytes,
                                    const int64_t *r_off, long long r_count, long long r_bytes, int32_t max_qlen, int32_t max_rlen,
                                    int32_t *qlen, int32_t *rlen, int32_t *tw, int64_t *qsrc, int64_t *rsrc, uint8_t *ok, uint8_t *sflag, hipStream_t stream,
                                    bool ref = false);
int pmx_launch_pairs_gather_translated(long long n, const uint8_t *q_buf, long long q_bytes, const uint8_t *r_buf, long long r_bytes,
                                       const int32_t *qlen, const int32_t *rlen, const int32_t *tw, const int64_t *qsrc, const int64_t *rsrc,
                                       const uint8_t *ok, const uint8_t *sflag, const int64_t *qoff, const int64_t *roff,
                                       uint8_t *qout, long long q_cap, uint8_t *rout, long long r_cap, const PmxCodeTable &code, hipStream_t stream,
                                       bool ref = false);
// Codon streams (the _frameshift entries).  resolve_codons: n descriptors -> per * n slots, one per strand (strand ? strand[k]
// : per == 2 ? forward, reverse : first); the query's length = the stream's N = W - 2, tw = W, sflag = the strand; W < 3, a strand byte
// above 1 and N > max_qlen make every slot a 1 x 1 placeholder with ok = 0.  gather_codons: letter p of a query slot = the codon at
// oriented bytes p .. p + 2.  The slots' records fold with pmx_launch_pairs_fold.  ref (the _frameshift_ref
// entries): the sides exchanged -- the reference's window becomes the stream, N <= max_rlen, and the query is copied.
int pmx_launch_pairs_resolve_codons(const pmx_pair_t *pairs, const uint8_t *strand, int first, int per, long long n,
                                    const int64_t *q_off, long long q_count, long long q_bytes,
                                    const int64_t *r_off, long long r_count, long long r_bytes, int32_t max_qlen, int32_t max_rlen,
                                    int32_t *qlen, int32_t *rlen, int32_t *tw, int64_t *qsrc, int64_t *rsrc, uint8_t *ok, uint8_t *sflag, hipStream_t stream,
                                    bool ref = false);
int pmx_launch_pairs_gather_codons(long long n, const uint8_t *q_buf, long long q_bytes, const uint8_t *r_buf, long long r_bytes,
                                   const int32_t *qlen, const int32_t *rlen, const int32_t *tw, const int64_t *qsrc, const int64_t *rsrc,
                                   const uint8_t *ok, const uint8_t *sflag, const int64_t *qoff, const int64_t *roff,
                                   uint8_t *qout, long long q_cap, uint8_t *rout, long long r_cap, const PmxCodeTable &code, hipStream_t stream,
                                   bool ref = false);
// The three-frame local DP over codon streams, one description per side.  Query side (pmx_swfs.hip): the stream on the rows,
// n slots of up to b.max_qlen stream rows x b.max_rlen protein columns.  Reference side (pmx_swfsc.hip): the same DP with the
// stream on the columns, b.max_qlen protein rows x b.max_rlen stream columns.  32-bit scores.  Both launchers are pmx_fs.h's.
struct PmxFsSide {
    bool ref;                // the reference's side: the walk's `ref`, pmx_launch_pairs_resolve_codons' and _gather_codons'
    int max_msize;           // the kernel keeps the matrix in LDS
    int strip_rows;          // b.max_qlen above this: the sweep runs in strips and needs boundary scratch
    int lane_rows;           // rows per lane; strip_rows / lane_rows lanes per slot
    int max_rows;            // the cap on b.max_qlen: PMX_FRAMESHIFT_MAX_WINDOW - 2 stream letters, PMX_FRAMESHIFT_REF_MAX_QUERY protein letters
    // boundary scratch of one slot of a launch whose b.max_qlen exceeds strip_rows: two buffers of max_rlen columns
    long long (*bound_bytes_per_slot)(int max_rlen);
    // the trace form's scratch of one slot: the query side's sweep stores by column, the reference side's by step (below)
    long long (*trace_bytes_per_slot)(int max_qlen, int max_rlen);
    // launch: the score form, trace NULL; bnd holds bnd_slots slots and the launch runs in parts of as many.  launch_trace: one launch
    // over b.n slots; trace (and bnd, when strips are needed) hold the bytes of b.n slots rounded up to a multiple of four, bnd_slots is
    // not read.  0 launched, 1 not eligible, <0 HIP error.
    int (*launch)(const PmxBatch &b, const PmxDevMatrix &m, int open, int ext, int fs, void *bnd, long long bnd_slots, void *trace,
                  pmx_record_t *d_out, hipStream_t stream, const char **kernel_name);
    decltype(launch) launch_trace;
    const char *names[2][2]; // pmx_last_kernel(): [trace form][several strips]
};
const PmxFsSide &pmx_fs_query_side();     // pmx_swfs.hip
const PmxFsSide &pmx_fs_ref_side();       // pmx_swfsc.hip
static inline const PmxFsSide &pmx_fs_side(bool ref) { return ref ? pmx_fs_ref_side() : pmx_fs_query_side(); }
// The trace form of the sweep and its walk (semantics: include/parasail_amd.h, "Frameshift traceback").  A cell's decision
// byte: bits 0 .. 2 where H came from (START .. LONG: from M, and which term D was), bit 3 E was opened, bit 4 F was opened.  The byte of
// row i, column j of a slot: ((i / STRIP_ROWS * max_rlen + j) * COL_BYTES) + i % STRIP_ROWS / LANE_ROWS * 12 + i % LANE_ROWS.
enum { PMX_FSTR_START = 0, PMX_FSTR_INFRAME = 1, PMX_FSTR_SHORT = 2, PMX_FSTR_LONG = 3, PMX_FSTR_F = 4, PMX_FSTR_E = 5, PMX_FSTR_ZERO = 6,
       PMX_FSTR_EO = 8, PMX_FSTR_FO = 16,
       PMX_FSTR_LANE_ROWS = 10, PMX_FSTR_STRIP_ROWS = 160, PMX_FSTR_COL_BYTES = 192 };
// The reference side's trace (pmx_swfsc.hip; semantics: "Frameshift traceback, reference side"): the same decision bytes,
// STORED BY STEP.  Lane g of a slot's group finishes its ten rows of column t - g in step t, so a strip of a slot has
// max_cols + PMX_FSTRC_SKEW steps of COL_BYTES bytes, and the byte of row i (a protein letter), column j (a stream letter) is
// PMX_FSTRC_CELL(i, j, max_cols): ((strip * (max_cols + 15) + j + lane) * 16 + lane) * 12 + i % 10, strip = i / 160, lane = i % 160 / 10.
enum { PMX_FSTRC_SKEW = PMX_FSTR_COL_BYTES / 12 - 1 };
#define PMX_FSTRC_CELL(i, j, max_cols)                                                                                                      \
    ((((size_t)((i) / PMX_FSTR_STRIP_ROWS) * (size_t)((max_cols) + PMX_FSTRC_SKEW) + (size_t)((j) + (i) % PMX_FSTR_STRIP_ROWS / PMX_FSTR_LANE_ROWS)) \
          * (PMX_FSTR_COL_BYTES / 12) + (size_t)((i) % PMX_FSTR_STRIP_ROWS / PMX_FSTR_LANE_ROWS)) * 12 + (size_t)((i) % PMX_FSTR_LANE_ROWS))
// The walk over that trace (pmx_walkfs.hip), one lane per logical pair k of n: its record recs[k] (a bad pair's is flagged), its slot
// per * k + (win ? win[k] : 0) of the sweep's launch; qoff / roff are the launch's, per * n + 1 entries.  ops: run-length ops
// (len << 4 | op; '/' = 9, '\\' = 10) from the end of the PAIR's op slots backwards -- a pair owns the qlen + rlen + 1 entries of each of
// its slots -- with nops and textlen; pair_qoff / pair_roff [n + 1]: the offsets with which pmx_launch_cigar_render_slots (ops_base 0)
// finds the pairs' op slots; beg (2 n) and stats_out are optional.  ref: the trace is the reference side's (PmxFsSide::launch_trace of pmx_swfsc.hip), rows the query protein.
int pmx_launch_walkfs(const PmxDevMatrix &m, long long n, int per, const uint8_t *win,
                      const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff, int max_rlen,
                      const pmx_record_t *recs, const uint8_t *trace, long long trace_bytes_per_slot,
                      uint32_t *ops, int32_t *nops, int32_t *textlen, int64_t *pair_qoff, int64_t *pair_roff,
                      int32_t *beg, pmx_stats_t *stats_out, hipStream_t stream, bool ref = false);
// The windowed form of that traceback (pmx_pairs.hip; the bound: pmx_fswin.h).  window: n folded records of the score
// pass with their strand bytes and descriptors -> npairs, the descriptors of the sub-windows the records' paths lie in (a bad record: a
// descriptor that is bad whatever the maxima), ashift, the oriented column each narrowed window starts at, and nlen (2 n), the narrowed
// query letters and stream letters (0 / 0 for a bad record).  rebase: ashift onto end_ref of rec and onto beg[2 k + 1] (beg may be
// NULL), and violations[0] += the records that then differ from `first`.  0 launched, 1 not eligible, <0 HIP error.
extern "C" long long pmx_swfsc_window_cols(long long rowmax_prefix, long long score, long long rows, long long open, long long extend, long long fs);
int pmx_launch_fsref_window(const pmx_pair_t *pairs, const pmx_record_t *rec, const uint8_t *strand, long long n, const uint8_t *q_buf,
                            const int64_t *q_off, long long q_count, long long q_bytes, const int64_t *r_off, long long r_count, long long r_bytes,
                            const PmxDevMatrix &m, int open, int ext, int fs, pmx_pair_t *npairs, int32_t *ashift, int32_t *nlen, hipStream_t stream);
int pmx_launch_fsref_rebase(const pmx_record_t *first, const int32_t *ashift, long long n, pmx_record_t *rec, int32_t *beg, unsigned *violations,
                            hipStream_t stream);
// Per-query top-K (pmx_topk.hip; semantics: include/parasail_amd.h).  ks = min(k, |R|).  The running state of local row
// li: st_keys / st_recs / st_stats[li * ks ..) hold st_held[li] entries in (score descending, j ascending) order, st_passing[li] = |P_i|
// so far; the caller zeroes st_held (nq + 1 entries, the scan's input) and st_passing before the first chunk.  geometry: what the tile
// buffers of a run with chunks of `chunk` pairs hold -- rows * tps slots of tstride keys (t_keys), one count and one passing count per
// slot.  merge: a chunk's records [p0, p0 + cn) of the rectangle (p0 absolute) into the lists of its rows; chunks in ascending p0 on
// one stream.  emit: the lists to row_off[li] + x below `capacity` (row_off: the exclusive scan of st_held), row_passing (optional)
// and counts[3] = kept, written, passing.
void pmx_topk_geometry(long long chunk, long long nr, int ks, long long *rows, long long *tps, long long *tstride);
int pmx_launch_topk_merge(const pmx_record_t *rec, const pmx_stats_t *stats /* may be NULL */, long long p0, long long cn, long long nr, long long q_first,
                          int ks, int32_t min_score, int skip_self, long long tps, long long tstride,
                          uint64_t *t_keys, int32_t *t_cnt, int32_t *t_pass,
                          uint64_t *st_keys, pmx_record_t *st_recs, pmx_stats_t *st_stats, int32_t *st_held, int64_t *st_passing, hipStream_t stream);
int pmx_launch_topk_emit(long long nq, long long q_first, long long nr, int ks, const uint64_t *st_keys, const pmx_record_t *st_recs,
                         const pmx_stats_t *st_stats, const int32_t *st_held, const int64_t *st_passing, const int64_t *row_off, long long capacity,
                         pmx_pair_t *hit_pairs, int64_t *hit_index, pmx_record_t *hit_recs, pmx_stats_t *hit_stats, int64_t *row_passing,
                         int64_t *counts, hipStream_t stream, uint8_t *hit_strand = nullptr, int marked = 0 /* as in append_hits */);
// K-mer seeding (pmx_seed.hip; semantics: include/parasail_amd.h, DESIGN 2.5p .. 2.5r).  index: one entry per byte of the set's buffer
// into keys_in / vals_in, sorted into keys_out / vals_out (the k-mers in front, *n_valid of them; val = seq << 32 | pos); buckets: the
// table of nb + 1 first-entry numbers on the keys' top bits (key >> shift).
#define PMX_SEED_MATCH_BYTES 24        // per match: two sort buffers of 8-byte keys, the head index, the candidate flag / position
#define PMX_SEED_MATCH_BYTES_CHAIN 40  // ... of a chaining run: two sort buffers of 8-byte keys and of 4-byte values (i), f, pred, child, the flag / position
#define PMX_SEED_CHAIN_LANES 64        // the chain kernel: one wave per (row, strand) segment, a lane per predecessor of a round
#define PMX_SEED_CHAIN_RING 1024       // ... and the most anchors its LDS ring holds (the largest lookback)
#define PMX_SEED_POS_BYTES   16        // per position slot: first entry, occurrences, match offset
#define PMX_SEED_POS_BYTES_LETTERS (PMX_SEED_POS_BYTES + 1)        // ... and the code byte of a letters or translated index
#define PMX_SEED_POS_BYTES_MINIMIZERS (PMX_SEED_POS_BYTES + 1)     // ... or the flag byte of a minimizer index (w > 1)
size_t pmx_seed_index_sort_bytes(long long bytes, int k);
int pmx_launch_seed_index(const uint8_t *buf, const int64_t *off, long long count, long long bytes, int k,
                          uint64_t *keys_in, uint64_t *vals_in, uint64_t *keys_out, uint64_t *vals_out, void *temp, size_t temp_bytes,
                          unsigned long long *n_valid, hipStream_t stream);
int pmx_launch_seed_buckets(const uint64_t *keys, long long n, int shift, long long nb, uint32_t *bucket, hipStream_t stream);
int pmx_launch_seed_entries(const uint64_t *keys, const uint64_t *vals, long long first, long long count, uint64_t *kmer, int64_t *seq,
                            int32_t *pos, hipStream_t stream);
// A letters index: `bits` bits per letter, table: 256 group bytes on the device.
size_t pmx_seed_index_sort_bytes_letters(long long bytes, int k, int bits);
int pmx_launch_seed_index_letters(const uint8_t *buf, const int64_t *off, long long count, long long bytes, int k, int bits, const uint8_t *table,
                                  uint64_t *keys_in, uint64_t *vals_in, uint64_t *keys_out, uint64_t *vals_out, void *temp, size_t temp_bytes,
                                  unsigned long long *n_valid, hipStream_t stream);
// A translated index: the six-frame k-mers of a nucleotide set, nstr strands from strand0, nstr * bytes entry slots
// (val = (strand * count + seq) << 32 | oriented position).
int pmx_launch_seed_index_translated(const uint8_t *buf, const int64_t *off, long long count, long long bytes, int k, int bits, const uint8_t *table,
                                     const PmxCodeTable &code, int nstr, int strand0, uint64_t *keys_in, uint64_t *vals_in, uint64_t *keys_out,
                                     uint64_t *vals_out, void *temp, size_t temp_bytes, unsigned long long *n_valid, hipStream_t stream);
// Minimizers (definitions: include/parasail_amd.h).  mix: the order of the k-mers, a bijection on the 2 k bits of a key --
// every step (xor with a constant, multiplication by an odd number modulo 2^2k, xor with the own upper half) is one.
__host__ __device__ __forceinline__ uint64_t pmx_seed_mix_bits(uint64_t key, int k)
{
    const uint64_t m = ((uint64_t)1 << (2 * k)) - 1;
    uint64_t h = (key ^ PMX_SEED_MIX_XOR) & m;
    h = (h * PMX_SEED_MIX_MUL1) & m; h ^= h >> k;
    h = (h * PMX_SEED_MIX_MUL2) & m; h ^= h >> k;
    return h;
}
// The sketch kernel's two forms (pmx_seed_sketch_kernel).  set: flags[p] for every byte p of the set's buffer and their exclusive scan
// at[0 .. bytes] (at[bytes] = the minimizers; flags: bytes + 1 bytes, 4-byte aligned; temp: pmx_seed_sketch_scan_bytes(bytes)).
// selected: the flagged positions as compact (key, val) pairs, sorted (n > 0 of them; temp: pmx_seed_index_sort_bytes(n, k)).  rows:
// one byte per position slot (seg * max_qlen + i) of `segs` (row, orientation) segments from row0.  tiles: positions per workgroup.
void pmx_seed_sketch_tiles(int *row_tile, int *set_tile);
size_t pmx_seed_sketch_scan_bytes(long long bytes);
int pmx_launch_seed_sketch_set(const uint8_t *buf, const int64_t *off, long long count, long long bytes, int k, int w, uint8_t *flags, uint32_t *at,
                               void *temp, size_t temp_bytes, hipStream_t stream);
int pmx_launch_seed_index_selected(const uint8_t *buf, const int64_t *off, long long count, long long bytes, int k, const uint8_t *flags,
                                   const uint32_t *at, long long n, uint64_t *keys_in, uint64_t *vals_in, uint64_t *keys_out, uint64_t *vals_out,
                                   void *temp, size_t temp_bytes, hipStream_t stream);
int pmx_launch_seed_sketch_rows(const uint8_t *qbuf, const int64_t *qoff, long long q_bytes, long long row0, long long segs, int strands, int strand0,
                                int max_qlen, int k, int w, uint8_t *flags, hipStream_t stream);
// A seeding run, described once (filled by seed_plan of pmx_api.hip, host arithmetic only; pinned by tests/test_seed_plans.py).
// A row has `orients` orientations of max_qlen position slots each: the strands of a DNA query, the frames of a translated one, the row
// itself.  The sort's segments -- what one candidate's matches share -- are `segs` per row of seg_slots position slots each, and the
// geometry says how a match's id and diagonal and a cluster's window and byte are formed:
//   DNA          segment (row, strand);         id = r;                d = j - i;          byte = strand
//   FRAMES       segment (row, frame or row);   id = r;                d = j - i letters;  byte = frame (0: rows that are letters)
//   CODONS       segment (row, strand), its three frames; id = r;      D = 3 j - (f % 3 + 3 i) nucleotides; byte = strand
//   REF_FRAMES   segment row;  id = g * count + r, g = 3 s + x % 3;    d = x / 3 - i letters; byte 0 / 3, reserved = g
//   REF_CODONS   segment row;  id = s * count + r;                     D = x - 3 i nucleotides; byte = s
enum PmxSeedKind { PMX_SEED_KIND_DNA = 0, PMX_SEED_KIND_LETTERS = 1, PMX_SEED_KIND_TRANSLATED = 2 };
enum PmxSeedGeom { PMX_SEED_GEOM_DNA = 0, PMX_SEED_GEOM_FRAMES = 1, PMX_SEED_GEOM_CODONS = 2, PMX_SEED_GEOM_REF_FRAMES = 3, PMX_SEED_GEOM_REF_CODONS = 4 };
struct PmxSeedPlan {
    int kind, geom;                        // PmxSeedKind of the index, PmxSeedGeom of the run
    bool rows_translated;                  // the rows are nucleotides read as codons (orientation o: frame first + o), else as they stand
    int orients, first;                    // orientations per row; the first one's strand (DNA) or frame (translated rows), else 0
    int segs; long long seg_slots;         // segments per row, position slots per segment
    long long row_slots; int pos_bytes;    // position slots per row (orients * max_qlen); scratch bytes per position slot
    int max_qlen, k, bits, key_bits;       // bits per letter of the index; the sorted bits of a match key (the diagonal and the id)
    long long ref_count;                   // the sequences of the indexed set
    int band, min_seeds, pad, max_occ;
    int w;                                 // the window of a DNA index: 1 every k-mer, > 1 minimizers (one flag byte more per position slot)
    bool chain;                            // candidates are collinear chains (pmx_seed_chains; a DNA index), else diagonal clusters
    int max_gap, lookback, gap_scale, min_score;        // read where chain: pmx_seed_chain_opts_t's
    int match_bytes;                       // scratch bytes per match: PMX_SEED_MATCH_BYTES, PMX_SEED_MATCH_BYTES_CHAIN where chain
    PmxCodeTable code;                     // read where rows_translated
    long long slice_rows, cap_m, positions, slots;      // a slice: its rows at most, matches at most, position slots, rows x orients
};
// ... the index and the rows it reads (device) ...
struct PmxSeedSource {
    const uint64_t *keys, *vals; const uint32_t *bucket; int shift; const uint8_t *table;     // table: NULL of a DNA index
    const int64_t *roff;                                                                      // offsets of the indexed set
    const uint8_t *qbuf; const int64_t *qoff; long long q_bytes;
};
// ... a slice's scratch (lo, moff: positions, cnt: positions + 1; keys_a / keys_b / head: cap_m, flag: cap_m + 1; cut: 2; codes:
// positions, NULL with a DNA index; mflag: positions, the rows' minimizer flags, NULL unless the plan's w > 1; temp:
// pmx_seed_temp_bytes(positions, cap_m, slots, chain)).  A chaining run has no head; it has vals_a / vals_b (the matches' i beside
// the two key buffers), f, pred and child, cap_m entries each ...
struct PmxSeedSlice {
    uint32_t *lo, *cnt; int64_t *moff; uint64_t *keys_a, *keys_b; uint32_t *head, *flag; int64_t *cut; uint8_t *codes; void *temp; size_t temp_bytes;
    uint8_t *mflag;
    uint32_t *vals_a, *vals_b; int32_t *f, *pred, *child;
};
// ... and where the candidates go: `capacity` entries each (seeds optional; chains optional, a chaining run's), row offsets, counts[0 .. 1].
struct PmxSeedOut { pmx_pair_t *pairs; uint8_t *byte; pmx_seed_hit_t *seeds; long long capacity; int64_t *row_off, *counts; pmx_seed_chain_t *chains; };
size_t pmx_seed_temp_bytes(long long positions, long long matches, long long slots, bool chain = false);
// count: the lookups of rows row0 .. row0 + rows of Q (with a letters or translated index behind the code stage), the scan of their
// matches into moff and cut[0 .. 1] = the rows that fit cap_m / their matches.  cluster: those rows' m matches emitted, sorted per
// segment and turned into candidates behind counts[0], row offsets (out.row_off points at the entry of the slice's first row) and counts.
int pmx_launch_seed_count(const PmxSeedPlan &p, const PmxSeedSlice &s, const PmxSeedSource &src, long long row0, long long rows, hipStream_t stream);
int pmx_launch_seed_cluster(const PmxSeedPlan &p, const PmxSeedSlice &s, const PmxSeedOut &out, const PmxSeedSource &src, long long row0,
                            long long rows, long long m, hipStream_t stream);
// The gap cost of a chain link (include/parasail_amd.h): integers only; g <= 2^20 and scale <= 65 535 keep it below 2^28.
__host__ __device__ __forceinline__ int32_t pmx_seed_chain_cost(int32_t g, int32_t scale)
{
    if (g < 1) return 0;
    return (int32_t)(((int64_t)g * scale) >> 8) + ((32 - __builtin_clz((unsigned)g)) >> 1);
}
// The ungapped diagonal filter (pmx_ungap.hip; semantics: include/parasail_amd.h).  The hot kernel's shape: a group of
// PMX_UNGAP_LANES lanes per candidate, pieces of whole PMX_UNGAP_STEP-cell steps per lane.
#define PMX_UNGAP_LANES 16
#define PMX_UNGAP_STEP 4
// The n slots of a chunk (packed windows, offsets and validity bytes of the set batches' pipeline; the chunk's descriptors and seed
// records) -> n records.  0 launched, 1 not eligible (a PSSM), <0 HIP error.
// form: which cells the seed records' diagonals mean -- PLAIN both sides at stride 1 from r_beg; CODONS the query side a
// codon stream, nucleotide diagonals; REF_CODONS the reference side a codon stream; REF_FRAMES a translated reference window whose
// origin is a letter of sequence frame seeds.reserved.  The two REF forms read r_off (the reference set's offsets) and the resolve's
// tw and sflag columns; the others take NULL.
#define PMX_UNGAP_PLAIN 0
#define PMX_UNGAP_CODONS 1
#define PMX_UNGAP_REF_CODONS 2
#define PMX_UNGAP_REF_FRAMES 3
int pmx_launch_ungapped(long long n, const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff, const uint8_t *ok,
                        const pmx_pair_t *pairs, const pmx_seed_hit_t *seeds, int form, const int64_t *r_off, const int32_t *tw, const uint8_t *sflag,
                        const PmxDevMatrix &m, pmx_ungapped_t *out, hipStream_t st);
// The selection over the scored list: keys_a / keys_b n keys each (NULL without top_n), flag n + 1 entries, temp of
// pmx_ungap_select_temp_bytes(n, nq) bytes; every output column optional.
size_t pmx_ungap_select_temp_bytes(long long n, long long nq);
int pmx_launch_ungap_select(const pmx_ungapped_t *ung, long long n, const int64_t *row_off, long long nq, int min_score, int top_n,
                            const pmx_pair_t *pairs, const uint8_t *byte, const pmx_seed_hit_t *seeds,
                            uint64_t *keys_a, uint64_t *keys_b, uint32_t *flag, void *temp, size_t temp_bytes,
                            pmx_pair_t *out_pairs, uint8_t *out_byte, pmx_seed_hit_t *out_seeds, pmx_ungapped_t *out_ung, int64_t *out_source,
                            long long capacity, int64_t *out_row_off, int64_t *counts, hipStream_t st);
// out[0] / out[1] (zeroed by the caller): the longest good query / reference window; pairs == NULL: the n sequences of the first set
int pmx_launch_pairs_maxlen(const pmx_pair_t *pairs, long long n, const int64_t *q_off, long long q_count, long long q_bytes,
                            const int64_t *r_off, long long r_count, long long r_bytes, int32_t *out, hipStream_t stream);
// p -> (i, j) of the strict upper triangle of nseq x nseq (2 <= nseq <= 2^31 - 1, p in range): the arithmetic the kernel runs
void pmx_all_pairs_index_host(unsigned long long nseq, unsigned long long p, unsigned long long *i, unsigned long long *j);

// One long pair (or a few) across the chip: bands of the query on different CUs, pipelined through HBM granules (pmx_long.hip).
// What a road asks of the sweep (long_batch, long_cigar_device: which form runs without a switch is the road's own decision) ...
struct PmxLongWant {
    long long n; int max_qlen, max_rlen, msize;
    int R;                   // rows per lane: 2, 4 or 16 (bands of 128, 256 or 1 024 query rows)
    int cols;                // columns per step: 1 or 2 (R = 16 has the one-column form only and gets it)
    int cols_few;            // 0, or the columns per step when the chunk turns out to be of at most 16 pairs (the chunk does not depend on them)
    int chunk_cols;          // PMX_LONG_CHUNK_COLS, 16 or 64: boundary columns a band takes over at a time; the two-column form counts steps of two
                             //   columns and has no chunk below 32 of them, so 16 means 32 steps (64 columns) there and 64 means 64 steps (128 columns)
    int tile_cols;           // 0: scores only; 64, 128, 256: the checkpoint form -- the (H, E) of every tile_cols-th column stay for pmx_walkt.hip
    size_t budget;           // bytes of scratch one chunk of pairs may take (one pair always gets what it needs ...
    bool refuse_above_budget;     // ... unless this is set: then a pair beyond the budget is refused)
    bool r16_above_4g;       // a pair whose scratch passes 4 GiB takes R = 16 instead (fewer bands: fewer row granules)
    bool clamp_blocks;       // a chunk of more than 2^31 - 1 (pair, band) workgroups: shorten it (else: refused)
};
// ... and the sweep the planner makes of it: what pmx_launch_long, pmx_launch_walkt and the roads' chunk loops need to know.  A chunk's
// scratch is [abort word, 64 bytes][boundary granules][candidates, 8 ints per (pair, band)][checkpoints, from the next 256-byte boundary];
// pmx_long_plan is the one place that lays it out.  The first 64 bytes are the call's abort word: the caller zeroes them before the first
// launch and reads them after the last (non-zero: a band's bounded wait ran out -- every record of the call is marked PMX_FLAG_RERUN and
// has to be redone elsewhere).
struct PmxLongPlan {
    int R, cols, steps;      // rows per lane, columns per step, steps per boundary chunk (16 / 64 one-column, 32 / 64 two-column)
    bool ck; int tile_cols, ckshift; long long ckslots;     // checkpoint form: tile_cols = 1 << ckshift, slots per (pair, band)
    int nbmax; long long bstride;                            // bands of the longest query; granules per (pair, band) boundary
    long long pairs;         // per chunk: a launch takes at most that many
    int msize, max_qlen, max_rlen;                           // what it was planned for: a launch may not exceed it
    size_t off_abort, abort_bytes, off_bound, off_cand, off_ck, total;    // bytes within a chunk's scratch (off_ck = total without checkpoints)
    size_t ck_bytes;         // total - off_ck
    size_t lds;              // dynamic LDS of the sweep
    const char *name;        // the instance and its road as pmx_last_kernel() shows them (static storage)
};
// 0 planned, 1 refused (no such form, or it cannot be launched: alphabet, LDS, budget); calls no HIP function.
int pmx_long_plan(const PmxLongWant &w, PmxLongPlan *p);
// 0 launched, 1 not eligible, <0 HIP error.  b.n <= p.pairs pairs into `scratch` (p.total bytes).
int pmx_launch_long(const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext, const PmxLongPlan &p,
                    void *scratch, pmx_record_t *d_out, int sat_above, int force_sat, int spin_limit, hipStream_t stream);
// Tiled traceback over what the checkpoint sweep left (pmx_walkt.hip): one wave per pair re-derives the tiles the path enters.  Run-length
// ops / nops / textlen as pmx_launch_walkb (ops == NULL: none) and / or the path's statistics (stats_out != NULL), in one pass.
// 0 launched, 1 not eligible (the tile's decision bits do not fit the LDS), <0 HIP error.  `scratch`: what pmx_launch_long filled by `p`.
size_t pmx_walkt_lds_bytes(int msize, int BR, int tile_cols);
int pmx_launch_walkt(const PmxBatch &b, const PmxDevMatrix &m, int mode, int sg_flags, int open, int ext, const PmxLongPlan &p,
                     const void *scratch, const pmx_record_t *recs,
                     const int64_t *slot_qoff, long long ops_base, uint32_t *ops, int32_t *nops, int32_t *textlen,
                     pmx_stats_t *stats_out, hipStream_t stream);

// Run-time CIGAR letter convention (switch PMX_CIGAR_SWAP_ID, read per call): 1 = exchange I and D in everything handed out.
int pmx_cigar_swapped();

// Collect the indices of records whose flags intersect `mask`: list[0..*count) (device), any order.
int pmx_launch_collect_saturated(const pmx_record_t *rec, long long n, int64_t *list, int *count, int mask, hipStream_t stream);
