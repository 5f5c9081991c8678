// pmx_pairs.hip -- sequence-set batches: pair descriptors (index + window into device-resident sequence sets) -> the packed chunk
// buffers every alignment kernel reads (semantics: include/parasail_amd.h; pipeline: pmx_api.hip).
//
//   pmx_pairs_resolve_kernel        descriptor -> `per` alignment slots (1 or 2, one per strand): two lengths, two source byte offsets, a
//                                   validity byte, a strand byte (a bad pair: 1 x 1 placeholders)
//   (pmx_launch_text_offsets        the chunk's packed qoff / roff from the lengths: pmx_sort.hip)
//   pmx_pairs_gather_kernel         the windows into the chunk's packed buffers, a 16-lane group per sequence
//   pmx_pairs_fixup_kernel          the records (and statistics) of bad pairs, after the chunk's alignment
//   pmx_all_pairs_enumerate_kernel  p -> (i, j) of the strict upper triangle, whole-sequence descriptors
//   pmx_pairs_maxlen_kernel         the longest resolved window per side (host entries over wrapped sets)
// for set search (pmx_search_pairs[_device]):
//   pmx_rect_pairs_enumerate_kernel p -> (p / |R|, p % |R|) of Q x R, whole-sequence descriptors
//   pmx_pairs_append_hits_kernel    a chunk's hits (positions from pmx_launch_select) behind the running total: descriptor, absolute
//                                   index, record, statistics
//   pmx_pairs_advance_hits_kernel   one thread, behind the append: the running total and the two public counts
//   pmx_pairs_first_bad_kernel      the lowest absolute index of a bad pair (host entry over wrapped sets)
// and, for the entries with strands and CIGAR output (pmx_align_pairs_ex[_device], pmx_gather_pairs_device):
//   pmx_pairs_gather_stranded_kernel    the gather that can reverse-complement a query window
//   pmx_pairs_fixup_cigar_kernel        bad pairs on the CIGAR road: record, empty text, begins
//   pmx_text_rebase_kernel              a chunk's text offsets behind the running total of the chunks before it
// and, for every entry whose pairs are more than one slot or whose slot is chosen by the entry (both strands; a translated
// side, 2.5i / 2.5j; codon streams, 2.5k / 2.5m):
//   pmx_pairs_fold_kernel               the slots' records (and statistics) -> one record, statistics and strand or frame per logical pair
// and, for a translated side (the _translated entries: the query; the _translated_ref entries: the reference):
//   pmx_pairs_resolve_frames_kernel     one descriptor -> `per` slots (1, 3 or 6), one per frame: translated length, nucleotide window
//   pmx_pairs_gather_translated_kernel  the gather that turns codons of that side's window into amino acids, on either strand
// and, for codon streams (the _frameshift entries: the query's; the _frameshift_ref entries: the reference's):
//   pmx_pairs_resolve_codons_kernel     one descriptor -> `per` slots (1 or 2), one per strand: the stream's length, nucleotide window
//   pmx_pairs_gather_codons_kernel      the gather that writes the stride-1 codon stream of that side's window, on either strand
// and, for the windowed reference-side frameshift traceback (the _frameshift_ref_cigar_long entries):
//   pmx_fsref_window_kernel             a folded record and its strand -> the descriptor of the sub-window its path lies in, the shift
//   pmx_fsref_rebase_kernel             the trace pass's end_ref and beg_ref back into the pair's window; the proof's check
// The resolve kernels share pmx_resolve_pair / pmx_slot_store, the gather kernels pmx_gather_group / pmx_gather_copy.
//
// All of them are bandwidth kernels in plain C++: vector loads and stores only.
#include "pmx_common.h"
#include "pmx_fswin.h"

// One side of a descriptor against its set.  0 = bad; otherwise the window's length, *src = its first byte in the set's buffer.
// A set wrapped around caller buffers has unchecked offsets: a window is good only when it lies inside [0, bytes).
static __device__ __forceinline__ int32_t pmx_resolve_side(const int64_t *__restrict__ off, long long count, long long bytes,
                                                           long long idx, int32_t beg, int32_t len, int32_t max_len, long long *src)
{
    if (idx < 0 || idx >= count || beg < 0 || len < -1) return 0;
    const long long o0 = off[idx], o1 = off[idx + 1];
    if (o0 < 0 || o1 < o0 || o1 > bytes) return 0;
    const long long slen = o1 - o0;
    const long long l = len < 0 ? slen - (long long)beg : (long long)len;
    if (l < 1 || (long long)beg + l > slen || l > (long long)max_len) return 0;
    *src = o0 + beg;
    return (int32_t)l;
}

// What the three resolve kernels share.  Both sides of descriptor p against their sets and maxima: true when both windows are good.
static __device__ __forceinline__ bool pmx_resolve_pair(const pmx_pair_t &p, const int64_t *__restrict__ q_off, long long q_count, long long q_bytes,
                                                        const int64_t *__restrict__ r_off, long long r_count, long long r_bytes,
                                                        int32_t max_qlen, int32_t max_rlen, int32_t *ql, int32_t *rl, long long *qs, long long *rs)
{
    *ql = pmx_resolve_side(q_off, q_count, q_bytes, p.q, p.q_beg, p.q_len, max_qlen, qs);
    *rl = pmx_resolve_side(r_off, r_count, r_bytes, p.r, p.r_beg, p.r_len, max_rlen, rs);
    return *ql > 0 && *rl > 0;
}
// The columns of a chunk's alignment slots, and the two threads behind the last pair: the scans read per * n + 1 lengths.
struct PmxSlotCols { int32_t *qlen, *rlen; int64_t *qsrc, *rsrc; uint8_t *ok, *sflag; };
static __device__ __forceinline__ void pmx_slot_tail(const PmxSlotCols &c, long long n, int per, long long k)
{
    const long long t = (long long)per * n + (k - n);
    c.qlen[t] = 0; c.rlen[t] = 0;
}
// Slot t: the two windows and the slot's flag byte, or (have false) the 1 x 1 placeholder with ok = 0.  sflag may be NULL (no flags kept).
static __device__ __forceinline__ void pmx_slot_store(const PmxSlotCols &c, long long t, bool have, int32_t ql, int32_t rl, long long qs, long long rs,
                                                      uint8_t flag)
{
    c.qlen[t] = have ? ql : 1; c.rlen[t] = have ? rl : 1; c.qsrc[t] = have ? qs : 0; c.rsrc[t] = have ? rs : 0;
    c.ok[t] = have ? 1 : 0;
    if (c.sflag) c.sflag[t] = flag;
}

// Logical pair k becomes `per` alignment slots per * k + i with the strand s0 + i in sflag, s0 = strand ? strand[k] : first -- the same
// lengths and sources in every slot, so the gather and every alignment kernel see an ordinary batch of per * n pairs.  The plain
// entries: no strand, first 0, per 1, sflag NULL.  A strand byte per pair (the _ex entries): per 1.  The strand chosen by the entry
// (DESIGN 2.5h): PMX_STRAND_REVERSE first 1, per 1; PMX_STRAND_BOTH first 0, per 2 -- slot 2 k the pair as stored, slot 2 k + 1 the pair
// with its query window reverse-complemented.  A bad descriptor and s0 + per > 2 -- a strand byte above 1 -- make every slot of the
// pair a 1 x 1 placeholder with ok = 0 and sflag = 0.
__global__ __launch_bounds__(256)
void pmx_pairs_resolve_kernel(const pmx_pair_t *__restrict__ pairs, const uint8_t *__restrict__ strand, int first, int per, long long n,
                              const int64_t *__restrict__ q_off, long long q_count, long long q_bytes,
                              const int64_t *__restrict__ r_off, long long r_count, long long r_bytes,
                              int32_t max_qlen, int32_t max_rlen,
                              int32_t *__restrict__ qlen, int32_t *__restrict__ rlen,
                              int64_t *__restrict__ qsrc, int64_t *__restrict__ rsrc, uint8_t *__restrict__ ok, uint8_t *__restrict__ sflag)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    const PmxSlotCols c = {qlen, rlen, qsrc, rsrc, ok, sflag};
    if (k >= n + 2) return;
    if (k >= n) { pmx_slot_tail(c, n, per, k); return; }
    const unsigned s0 = strand ? strand[k] : (unsigned)first;
    long long qs = 0, rs = 0; int32_t ql = 0, rl = 0;
    const bool good = pmx_resolve_pair(pairs[k], q_off, q_count, q_bytes, r_off, r_count, r_bytes, max_qlen, max_rlen, &ql, &rl, &qs, &rs) &&
                      s0 + (unsigned)per <= 2u;
    for (int i = 0; i < per; ++i)
        pmx_slot_store(c, (long long)per * k + i, good, ql, rl, qs, rs, good ? (uint8_t)(s0 + (unsigned)i) : 0);
}

// The four bytes at s (anywhere inside a window of the set [lo_bound, hi_bound)): from the one or two aligned dwords that hold them, or
// byte by byte where those would reach outside the set -- the first or last few bytes of a set, which has no promised slack.
static __device__ __forceinline__ uint32_t pmx_window_dword(const uint8_t *s, uintptr_t lo_bound, uintptr_t hi_bound)
{
    const uintptr_t sa = (uintptr_t)s & ~(uintptr_t)3;
    const unsigned sh = (unsigned)((uintptr_t)s & 3);
    if (sa >= lo_bound && sa + (sh ? 8 : 4) <= hi_bound) {
        const uint32_t lo = *reinterpret_cast<const uint32_t *>(sa);
        const uint32_t hi = sh ? *reinterpret_cast<const uint32_t *>(sa + 4) : 0u;
        return __builtin_amdgcn_alignbyte(hi, lo, sh);
    }
    return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
}

// What the four gather kernels share.  Group g = 2 * slot + side writes one window: four windows per wave, both sides of a slot in
// neighbouring groups.  Up to three head bytes bring the destination to a dword boundary, `nd` aligned destination dwords follow, the
// tail goes byte by byte.  pmx_gather_group finds the calling thread's group and returns false where it has nothing more to do: behind
// the last group, a window whose end would cross its side's capacity (not written), and a bad slot (its one byte is written here).
// Without a capacity (INT64_MAX: the chunk pipeline) destinations lie inside the chunk buffer by construction: every length is at
// most the maximum the buffer was sized by.
struct PmxGatherGroup {
    long long k; bool side; int lane;                           // the slot, its side (true: the reference) and the thread's lane of 16
    uint8_t *dst; const uint8_t *src;                           // the packed window; the window's first byte in the set
    uintptr_t lo_bound, hi_bound;                               // the set's buffer
    long long len, head, nd, done;                              // destination bytes; head bytes, dwords, bytes before the tail
    uint32_t *d0;                                               // destination dword 0
};
static __device__ __forceinline__ bool pmx_gather_group(long long n, const uint8_t *__restrict__ q_buf, long long q_bytes,
                                                        const uint8_t *__restrict__ r_buf, long long r_bytes,
                                                        const int32_t *__restrict__ qlen, const int32_t *__restrict__ rlen,
                                                        const int64_t *__restrict__ qsrc, const int64_t *__restrict__ rsrc, const uint8_t *__restrict__ ok,
                                                        const int64_t *__restrict__ qoff, const int64_t *__restrict__ roff,
                                                        uint8_t *__restrict__ qout, long long q_cap, uint8_t *__restrict__ rout, long long r_cap,
                                                        PmxGatherGroup *out)
{
    PmxGatherGroup g;
    const long long group = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
    g.lane = threadIdx.x & 15;
    if (group >= 2 * n) return false;
    g.k = group >> 1;
    g.side = (group & 1) != 0;
    if ((g.side ? roff[g.k + 1] : qoff[g.k + 1]) > (g.side ? r_cap : q_cap)) return false;     // (never with INT64_MAX: the load goes too)
    g.dst = g.side ? rout + roff[g.k] : qout + qoff[g.k];
    if (!ok[g.k]) { if (g.lane == 0) g.dst[0] = 0; return false; }
    const uint8_t *buf = g.side ? r_buf : q_buf;
    g.len = g.side ? rlen[g.k] : qlen[g.k];
    g.src = buf + (g.side ? rsrc[g.k] : qsrc[g.k]);
    g.lo_bound = (uintptr_t)buf; g.hi_bound = (uintptr_t)(buf + (g.side ? r_bytes : q_bytes));
    g.head = (4 - (long long)((uintptr_t)g.dst & 3)) & 3;
    if (g.head > g.len) g.head = g.len;
    g.nd = (g.len - g.head) >> 2; g.done = g.head + 4 * g.nd;
    g.d0 = reinterpret_cast<uint32_t *>(g.dst + g.head);
    *out = g;
    return true;
}
// The window as it is stored: each destination dword from the aligned source dwords that hold its four bytes.
static __device__ __forceinline__ void pmx_gather_copy(const PmxGatherGroup &g)
{
    if (g.lane < g.head) g.dst[g.lane] = g.src[g.lane];
    const uint8_t *s0 = g.src + g.head;
    for (long long x = g.lane; x < g.nd; x += 16)
        g.d0[x] = pmx_window_dword(s0 + 4 * x, g.lo_bound, g.hi_bound);
    if (g.lane < g.len - g.done) g.dst[g.done + g.lane] = g.src[g.done + g.lane];
}

// The gather every untranslated forward batch runs: both windows copied, no table in LDS, no capacities, no flags.
__global__ __launch_bounds__(256)
void pmx_pairs_gather_kernel(long long n, const uint8_t *__restrict__ q_buf, long long q_bytes, const uint8_t *__restrict__ r_buf, long long r_bytes,
                             const int32_t *__restrict__ qlen, const int32_t *__restrict__ rlen,
                             const int64_t *__restrict__ qsrc, const int64_t *__restrict__ rsrc, const uint8_t *__restrict__ ok,
                             const int64_t *__restrict__ qoff, const int64_t *__restrict__ roff,
                             uint8_t *__restrict__ qout, uint8_t *__restrict__ rout)
{
    PmxGatherGroup g;
    if (!pmx_gather_group(n, q_buf, q_bytes, r_buf, r_bytes, qlen, rlen, qsrc, rsrc, ok, qoff, roff, qout, INT64_MAX, rout, INT64_MAX, &g)) return;
    pmx_gather_copy(g);
}

// ---- strands (the _ex entries) --------------------------------------------------------------------------------------------------
// The complement of include/parasail_amd.h: IUPAC letters in both cases, every other byte itself.
struct PmxCompTable { uint8_t v[256]; };
static constexpr PmxCompTable pmx_make_comp_table()
{
    PmxCompTable t{};
    for (int i = 0; i < 256; ++i) t.v[i] = (uint8_t)i;
    const char from[] = "ACGTUMRWSYKVHDBN", to[] = "TGCAAKYWSRMBDHVN";
    for (int k = 0; k < 16; ++k) {
        t.v[(unsigned char)from[k]] = (uint8_t)to[k];
        t.v[(unsigned char)from[k] + 32] = (uint8_t)(to[k] + 32);
    }
    return t;
}
static constexpr PmxCompTable pmx_comp_host = pmx_make_comp_table();
__device__ const PmxCompTable pmx_comp_dev = pmx_make_comp_table();

// The gather of pmx_pairs_gather_kernel for both strands: the same group per window, the reference and a strand-0 query copied as
// there.  A strand-1 query window is read backwards: destination byte x is comp[src[len - 1 - x]], so the destination dword at bytes
// p .. p + 3 holds source bytes len - 4 - p .. len - 1 - p in reversed order -- assembled like a forward dword from the aligned source
// dwords around them, reversed by one v_perm, complemented by four byte reads of the table staged in LDS.  The strand is uniform per
// group (not per wave: a wave holds four windows), so the branch sits outside the dword loop.
__global__ __launch_bounds__(256)
void pmx_pairs_gather_stranded_kernel(long long n, const uint8_t *__restrict__ q_buf, long long q_bytes, const uint8_t *__restrict__ r_buf, long long r_bytes,
                                      const int32_t *__restrict__ qlen, const int32_t *__restrict__ rlen,
                                      const int64_t *__restrict__ qsrc, const int64_t *__restrict__ rsrc, const uint8_t *__restrict__ ok,
                                      const uint8_t *__restrict__ sflag, const int64_t *__restrict__ qoff, const int64_t *__restrict__ roff,
                                      uint8_t *__restrict__ qout, long long q_cap, uint8_t *__restrict__ rout, long long r_cap)
{
    __shared__ uint8_t comp[256];
    comp[threadIdx.x] = pmx_comp_dev.v[threadIdx.x];
    __syncthreads();
    PmxGatherGroup g;
    if (!pmx_gather_group(n, q_buf, q_bytes, r_buf, r_bytes, qlen, rlen, qsrc, rsrc, ok, qoff, roff, qout, q_cap, rout, r_cap, &g)) return;
    if (g.side || !sflag[g.k]) { pmx_gather_copy(g); return; }
    const int lane = g.lane;
    const uint8_t *last = g.src + g.len - 1;                    // destination byte x <- comp[last[-x]]
    if (lane < g.head) g.dst[lane] = comp[last[-lane]];
    const uint8_t *s0 = last - g.head - 3;                      // the lowest source byte of destination dword 0
    for (long long x = lane; x < g.nd; x += 16) {
        const uint32_t v = __builtin_amdgcn_perm(0u, pmx_window_dword(s0 - 4 * x, g.lo_bound, g.hi_bound), 0x00010203u);      // bytes 3 2 1 0
        g.d0[x] = (uint32_t)comp[v & 0xFF] | ((uint32_t)comp[(v >> 8) & 0xFF] << 8) | ((uint32_t)comp[(v >> 16) & 0xFF] << 16) |
                  ((uint32_t)comp[v >> 24] << 24);
    }
    if (lane < g.len - g.done) g.dst[g.done + lane] = comp[last[-(g.done + lane)]];
}

// ---- the fold (every entry whose pairs are several slots, or whose one slot the entry chose) ---------------------------------------
// The slots of logical pair k back to one record: among the slots with ok != 0 the highest score, the lowest slot -- the forward
// strand, the lowest frame -- on a tie (only the score is compared).  The record is the winner's sixteen bytes, the statistics are the
// winner's, the byte (a strand or a frame) is the winner's sflag.  No candidate (a bad descriptor, or no frame exists): {0, -1, -1,
// PMX_FLAG_BAD_PAIR}, zero statistics, byte 0 -- no fix-up pass follows.  mark: the byte also rides in the record -- 1 as
// PMX_FLAG_STRAND1, 2 in PMX_FLAG_FRAME_MASK, what pmx_pairs_append_hits_kernel reads as `marked` -- for records that stay in chunk
// scratch on their way through selection or the top-K lists; the kernels that write a caller's hit arrays strip it.  okf (optional):
// the logical pair's validity byte.  The strand and codon resolves give every slot of a pair the same ok, so for them "the slots
// with ok != 0" is all or none, and this is the fold that looked at the first slot's ok alone.  One thread per logical pair; slot
// records are read as 16-byte vectors (scratch is 16-byte aligned), records are stored that way where the destination is aligned.
__global__ __launch_bounds__(256)
void pmx_pairs_fold_kernel(const pmx_record_t *__restrict__ slot_rec, const pmx_stats_t *__restrict__ slot_stats,
                           const uint8_t *__restrict__ ok, const uint8_t *__restrict__ sflag, long long n, int per, int mark,
                           pmx_record_t *__restrict__ rec, pmx_stats_t *__restrict__ stats, uint8_t *__restrict__ byte,
                           uint8_t *__restrict__ okf)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const long long s = (long long)per * k;
    uint4 w = make_uint4(0u, 0xFFFFFFFFu, 0xFFFFFFFFu, (uint32_t)PMX_FLAG_BAD_PAIR);
    pmx_stats_t ws; ws.matches = 0; ws.similar = 0; ws.length = 0;
    const uint4 *sr = reinterpret_cast<const uint4 *>(slot_rec + s);
    long long from = -1;
    for (int i = 0; i < per; ++i) {
        if (!ok[s + i]) continue;
        const uint4 b = sr[i];
        if (from < 0 || (int32_t)b.x > (int32_t)w.x) { w = b; from = s + i; }
    }
    unsigned fb = 0;
    if (from >= 0) {
        fb = sflag[from];
        if (stats) ws = slot_stats[from];
    }
    if (mark == 1 && fb) w.w |= (uint32_t)PMX_FLAG_STRAND1;
    if (mark == 2) w.w |= fb << PMX_FLAG_FRAME_SHIFT;
    if (((uintptr_t)rec & 15) == 0)
        *reinterpret_cast<uint4 *>(rec + k) = w;
    else {
        pmx_record_t r; r.score = (int32_t)w.x; r.end_query = (int32_t)w.y; r.end_ref = (int32_t)w.z; r.flags = (int32_t)w.w;
        rec[k] = r;
    }
    if (stats) stats[k] = ws;
    if (byte) byte[k] = (uint8_t)fb;
    if (okf) okf[k] = from >= 0 ? 1 : 0;
}

// ---- translated queries (pmx_align_pairs_translated[_device], the _translated searches, pmx_gather_pairs_translated_device) --
// The standard genetic code in NCBI order and the base classes its index is made of: T / U = 0, C = 1, A = 2, G = 3 in both cases,
// every other byte 64 -- one such base lifts the index 16 b0 + 4 b1 + b2 to 64 or above, which is how a codon becomes 'X'.  The
// complement of a base is its class ^ 2 and leaves every other byte what it was, so a reverse frame is the forward look-up with the
// three bases read downwards and the index ^ 42.
static const char pmx_code_std[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
struct PmxBaseTable { uint8_t v[256]; };
static constexpr PmxBaseTable pmx_make_base_table()
{
    PmxBaseTable t{};
    for (int i = 0; i < 256; ++i) t.v[i] = 64;
    const char from[] = "TCAGU"; const uint8_t to[] = {0, 1, 2, 3, 0};
    for (int k = 0; k < 5; ++k) { t.v[(unsigned char)from[k]] = to[k]; t.v[(unsigned char)from[k] + 32] = to[k]; }
    return t;
}
__device__ const PmxBaseTable pmx_base_dev = pmx_make_base_table();

// The resolve step for a translated side (REF false: the query, true: the reference): logical pair k becomes `per` alignment slots,
// slot per * k + i in frame f = (frame ? frame[k] : first + i).  The translated side resolves to its nucleotide window (W bytes, any
// length), the other side against its maximum; slot i then holds L = (W - off) / 3 letters on the translated side, off = f % 3.  A
// frame with L = 0 does not exist: a 1 x 1 placeholder with ok = 0, which the fold passes over.  A bad descriptor, a frame byte above
// 5 and a frame of the call whose L exceeds the translated side's maximum make every slot of the pair such a placeholder.  tw: the
// translated side's W per slot.  The scans read per * n + 1 lengths.
template <bool REF>
__global__ __launch_bounds__(256)
void pmx_pairs_resolve_frames_kernel(const pmx_pair_t *__restrict__ pairs, const uint8_t *__restrict__ frame, int first, int per, long long n,
                                     const int64_t *__restrict__ q_off, long long q_count, long long q_bytes,
                                     const int64_t *__restrict__ r_off, long long r_count, long long r_bytes,
                                     int32_t max_qlen, int32_t max_rlen,
                                     int32_t *__restrict__ qlen, int32_t *__restrict__ rlen, int32_t *__restrict__ tw,
                                     int64_t *__restrict__ qsrc, int64_t *__restrict__ rsrc, uint8_t *__restrict__ ok, uint8_t *__restrict__ sflag)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    const PmxSlotCols c = {qlen, rlen, qsrc, rsrc, ok, sflag};
    if (k >= n + 2) return;
    if (k >= n) { pmx_slot_tail(c, n, per, k); return; }
    const unsigned f0 = frame ? frame[k] : (unsigned)first;
    long long qs = 0, rs = 0; int32_t ql = 0, rl = 0;
    bool good = pmx_resolve_pair(pairs[k], q_off, q_count, q_bytes, r_off, r_count, r_bytes, REF ? max_qlen : INT32_MAX, REF ? INT32_MAX : max_rlen,
                                 &ql, &rl, &qs, &rs) && f0 + (unsigned)per <= 6u;
    const int32_t W = REF ? rl : ql, max_l = REF ? max_rlen : max_qlen;
    for (int i = 0; i < per; ++i) {                                // (the shortest offset of the call's frames has the longest L)
        const int off = (int)((f0 + (unsigned)i) % 3u);
        if (W > off && (W - off) / 3 > max_l) good = false;
    }
    const long long s = (long long)per * k;
    for (int i = 0; i < per; ++i) {
        const unsigned f = f0 + (unsigned)i;
        const int off = (int)(f % 3u);
        const int32_t L = good && W > off ? (W - off) / 3 : 0;
        pmx_slot_store(c, s + i, L > 0, REF ? ql : L, REF ? L : rl, qs, rs, good ? (uint8_t)f : 0);
        tw[s + i] = L > 0 ? W : 0;
    }
}

// One amino acid: the three bases' classes to the index of the code, `flip` 0 for a forward frame and 42 for a reverse one.
static __device__ __forceinline__ uint32_t pmx_codon(const uint8_t *cls, const uint8_t *cod, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t flip)
{
    const uint32_t i = ((uint32_t)cls[b0] << 4) | ((uint32_t)cls[b1] << 2) | (uint32_t)cls[b2];
    return i < 64u ? (uint32_t)cod[i ^ flip] : (uint32_t)'X';
}

// The gather of pmx_pairs_gather_stranded_kernel with one side translated (REF false: the query, true: the reference): the same
// 16-lane group per window, the same forward walk over the destination in aligned dwords, the other side copied as there.  A
// destination dword of the translated side holds four letters, twelve source bytes: three calls of pmx_window_dword (the same
// in-bounds test, the same byte-by-byte fallback at a set's first and last bytes).  Forward frame `off`: letter p is the codon at
// window bytes off + 3 p ..; reverse frame: the codon at bytes W - 1 - off - 3 p downwards, complemented -- the reversal is the order
// the twelve bytes are taken in, the complement the index ^ 42.  Classes (256 bytes) and code (64 bytes, a kernel argument: a caller
// may bring its own) are staged in LDS.  The frame is uniform per group, so the branch sits outside the dword loop.  A window whose
// end would cross its capacity is not written.  tw: the translated side's W per slot.
template <bool REF>
__global__ __launch_bounds__(256)
void pmx_pairs_gather_translated_kernel(long long n, const uint8_t *__restrict__ q_buf, long long q_bytes, const uint8_t *__restrict__ r_buf, long long r_bytes,
                                        const int32_t *__restrict__ qlen, const int32_t *__restrict__ rlen, const int32_t *__restrict__ tw,
                                        const int64_t *__restrict__ qsrc, const int64_t *__restrict__ rsrc, const uint8_t *__restrict__ ok,
                                        const uint8_t *__restrict__ sflag, const int64_t *__restrict__ qoff, const int64_t *__restrict__ roff,
                                        uint8_t *__restrict__ qout, long long q_cap, uint8_t *__restrict__ rout, long long r_cap, PmxCodeTable code)
{
    __shared__ uint8_t cls[256];
    __shared__ uint8_t cod[64];
    cls[threadIdx.x] = pmx_base_dev.v[threadIdx.x];
    if (threadIdx.x < 64) cod[threadIdx.x] = code.v[threadIdx.x];
    __syncthreads();
    PmxGatherGroup g;
    if (!pmx_gather_group(n, q_buf, q_bytes, r_buf, r_bytes, qlen, rlen, qsrc, rsrc, ok, qoff, roff, qout, q_cap, rout, r_cap, &g)) return;
    if (g.side != REF) { pmx_gather_copy(g); return; }
    const int lane = g.lane;
    const long long k = g.k, len = g.len, head = g.head, nd = g.nd, done = g.done;      // len: letters on the translated side
    uint8_t *dst = g.dst; const uint8_t *src = g.src; uint32_t *d0 = g.d0;
    const uintptr_t lo_bound = g.lo_bound, hi_bound = g.hi_bound;
    const unsigned f = sflag[k];
    if (f >= 3) {
        const uint8_t *top = src + tw[k] - 1 - (f - 3);         // letter p: top[-3 p], top[-3 p - 1], top[-3 p - 2], complemented
        if (lane < head) dst[lane] = (uint8_t)pmx_codon(cls, cod, top[-3 * lane], top[-3 * lane - 1], top[-3 * lane - 2], 42u);
        const uint8_t *s0 = top - 3 * head - 11;                // the lowest source byte of destination dword 0
        for (long long x = lane; x < nd; x += 16) {
            const uint8_t *s = s0 - 12 * x;
            const uint32_t a = pmx_window_dword(s, lo_bound, hi_bound), b = pmx_window_dword(s + 4, lo_bound, hi_bound),
                           c = pmx_window_dword(s + 8, lo_bound, hi_bound);
            d0[x] = pmx_codon(cls, cod, c >> 24, (c >> 16) & 0xFF, (c >> 8) & 0xFF, 42u) |
                    (pmx_codon(cls, cod, c & 0xFF, b >> 24, (b >> 16) & 0xFF, 42u) << 8) |
                    (pmx_codon(cls, cod, (b >> 8) & 0xFF, b & 0xFF, a >> 24, 42u) << 16) |
                    (pmx_codon(cls, cod, (a >> 16) & 0xFF, (a >> 8) & 0xFF, a & 0xFF, 42u) << 24);
        }
        if (lane < len - done) {
            const uint8_t *t = top - 3 * (done + lane);
            dst[done + lane] = (uint8_t)pmx_codon(cls, cod, t[0], t[-1], t[-2], 42u);
        }
        return;
    }
    const uint8_t *base = src + f;                              // letter p: base[3 p], base[3 p + 1], base[3 p + 2]
    if (lane < head) dst[lane] = (uint8_t)pmx_codon(cls, cod, base[3 * lane], base[3 * lane + 1], base[3 * lane + 2], 0u);
    const uint8_t *s0 = base + 3 * head;
    for (long long x = lane; x < nd; x += 16) {
        const uint8_t *s = s0 + 12 * x;
        const uint32_t a = pmx_window_dword(s, lo_bound, hi_bound), b = pmx_window_dword(s + 4, lo_bound, hi_bound),
                       c = pmx_window_dword(s + 8, lo_bound, hi_bound);
        d0[x] = pmx_codon(cls, cod, a & 0xFF, (a >> 8) & 0xFF, (a >> 16) & 0xFF, 0u) |
                (pmx_codon(cls, cod, a >> 24, b & 0xFF, (b >> 8) & 0xFF, 0u) << 8) |
                (pmx_codon(cls, cod, (b >> 16) & 0xFF, b >> 24, c & 0xFF, 0u) << 16) |
                (pmx_codon(cls, cod, (c >> 8) & 0xFF, (c >> 16) & 0xFF, c >> 24, 0u) << 24);
    }
    if (lane < len - done) {
        const uint8_t *t = base + 3 * (done + lane);
        dst[done + lane] = (uint8_t)pmx_codon(cls, cod, t[0], t[1], t[2], 0u);
    }
}

// ---- codon streams (the _frameshift entries, pmx_gather_pairs_codons_device; REF: the _frameshift_ref entries, 2.5m) ----
// The resolve step of the frameshift-aware entries: logical pair k becomes `per` alignment slots, one per strand -- strand ?
// strand[k] (per 1) : per == 2 ? forward then reverse : `first` (0 or 1).  REF false: the query resolves to its nucleotide window (W
// bytes, any length), the reference against its maximum; a slot holds the codon stream's N = W - 2 letters.  W < 3 has no stream: 1 x 1
// placeholders with ok = 0, as a bad descriptor, a strand byte above 1 and N > max_qlen give.  REF true: the sides exchanged -- the
// reference resolves to its nucleotide window with no bound but N <= max_rlen, the query against max_qlen.  tw: W per slot, sflag: the
// strand.
template <bool REF>
__global__ __launch_bounds__(256)
void pmx_pairs_resolve_codons_kernel(const pmx_pair_t *__restrict__ pairs, const uint8_t *__restrict__ strand, int first, int per, long long n,
                                     const int64_t *__restrict__ q_off, long long q_count, long long q_bytes,
                                     const int64_t *__restrict__ r_off, long long r_count, long long r_bytes,
                                     int32_t max_qlen, int32_t max_rlen,
                                     int32_t *__restrict__ qlen, int32_t *__restrict__ rlen, int32_t *__restrict__ tw,
                                     int64_t *__restrict__ qsrc, int64_t *__restrict__ rsrc, uint8_t *__restrict__ ok, uint8_t *__restrict__ sflag)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    const PmxSlotCols c = {qlen, rlen, qsrc, rsrc, ok, sflag};
    if (k >= n + 2) return;
    if (k >= n) { pmx_slot_tail(c, n, per, k); return; }
    const unsigned s0 = strand ? strand[k] : (unsigned)first;
    long long qs = 0, rs = 0; int32_t ql = 0, rl = 0;
    bool good = pmx_resolve_pair(pairs[k], q_off, q_count, q_bytes, r_off, r_count, r_bytes, REF ? max_qlen : INT32_MAX, REF ? INT32_MAX : max_rlen,
                                 &ql, &rl, &qs, &rs) && s0 + (unsigned)per <= 2u;
    const int32_t W = REF ? rl : ql;
    good = good && W >= 3 && W - 2 <= (REF ? max_rlen : max_qlen);
    const long long s = (long long)per * k;
    for (int i = 0; i < per; ++i) {
        pmx_slot_store(c, s + i, good, REF ? ql : W - 2, REF ? W - 2 : rl, qs, rs, good ? (uint8_t)(s0 + (unsigned)i) : 0);
        tw[s + i] = good ? W : 0;
    }
}

// The stride-1 form of pmx_pairs_gather_translated_kernel<false>: destination letter p of a query slot is the codon at oriented bytes
// p, p + 1, p + 2 of the window, so the N = W - 2 letters hold all three forward frames of the strand interleaved.  A destination
// dword is four letters from six source bytes: one pmx_window_dword (its four bytes lie inside the window) and two byte reads -- the
// last letter's third base is the window's last byte, and no byte outside a set's buffer is read.  Strand 1 walks the window
// downwards with the index ^ 42, as the reverse frames there.  The reference side is copied.  REF true: the sides exchanged -- the
// reference slot receives its window's stream, the query is copied.
template <bool REF>
__global__ __launch_bounds__(256)
void pmx_pairs_gather_codons_kernel(long long n, const uint8_t *__restrict__ q_buf, long long q_bytes, const uint8_t *__restrict__ r_buf, long long r_bytes,
                                    const int32_t *__restrict__ qlen, const int32_t *__restrict__ rlen, const int32_t *__restrict__ tw,
                                    const int64_t *__restrict__ qsrc, const int64_t *__restrict__ rsrc, const uint8_t *__restrict__ ok,
                                    const uint8_t *__restrict__ sflag, const int64_t *__restrict__ qoff, const int64_t *__restrict__ roff,
                                    uint8_t *__restrict__ qout, long long q_cap, uint8_t *__restrict__ rout, long long r_cap, PmxCodeTable code)
{
    __shared__ uint8_t cls[256];
    __shared__ uint8_t cod[64];
    cls[threadIdx.x] = pmx_base_dev.v[threadIdx.x];
    if (threadIdx.x < 64) cod[threadIdx.x] = code.v[threadIdx.x];
    __syncthreads();
    PmxGatherGroup g;
    if (!pmx_gather_group(n, q_buf, q_bytes, r_buf, r_bytes, qlen, rlen, qsrc, rsrc, ok, qoff, roff, qout, q_cap, rout, r_cap, &g)) return;
    if (g.side != REF) { pmx_gather_copy(g); return; }
    const int lane = g.lane;
    const long long k = g.k, len = g.len, head = g.head, nd = g.nd, done = g.done;      // len: letters of the stream
    uint8_t *dst = g.dst; const uint8_t *src = g.src; uint32_t *d0 = g.d0;
    const uintptr_t lo_bound = g.lo_bound, hi_bound = g.hi_bound;
    if (sflag[k]) {
        const uint8_t *top = src + tw[k] - 1;                   // letter p: top[-p], top[-p - 1], top[-p - 2], complemented
        if (lane < head) dst[lane] = (uint8_t)pmx_codon(cls, cod, top[-lane], top[-lane - 1], top[-lane - 2], 42u);
        for (long long x = lane; x < nd; x += 16) {
            const uint8_t *t = top - (head + 4 * x);            // the first base of the dword's first letter; its letters reach t[-5]
            const uint32_t a = pmx_window_dword(t - 3, lo_bound, hi_bound);     // t[-3] .. t[0]
            const uint32_t b0 = a >> 24, b1 = (a >> 16) & 0xFF, b2 = (a >> 8) & 0xFF, b3 = a & 0xFF, b4 = t[-4], b5 = t[-5];
            d0[x] = pmx_codon(cls, cod, b0, b1, b2, 42u) | (pmx_codon(cls, cod, b1, b2, b3, 42u) << 8) |
                    (pmx_codon(cls, cod, b2, b3, b4, 42u) << 16) | (pmx_codon(cls, cod, b3, b4, b5, 42u) << 24);
        }
        if (lane < len - done) {
            const uint8_t *t = top - (done + lane);
            dst[done + lane] = (uint8_t)pmx_codon(cls, cod, t[0], t[-1], t[-2], 42u);
        }
        return;
    }
    if (lane < head) dst[lane] = (uint8_t)pmx_codon(cls, cod, src[lane], src[lane + 1], src[lane + 2], 0u);
    for (long long x = lane; x < nd; x += 16) {
        const uint8_t *t = src + head + 4 * x;                  // the dword's letters read t[0] .. t[5]
        const uint32_t a = pmx_window_dword(t, lo_bound, hi_bound);
        const uint32_t b0 = a & 0xFF, b1 = (a >> 8) & 0xFF, b2 = (a >> 16) & 0xFF, b3 = a >> 24, b4 = t[4], b5 = t[5];
        d0[x] = pmx_codon(cls, cod, b0, b1, b2, 0u) | (pmx_codon(cls, cod, b1, b2, b3, 0u) << 8) |
                (pmx_codon(cls, cod, b2, b3, b4, 0u) << 16) | (pmx_codon(cls, cod, b3, b4, b5, 0u) << 24);
    }
    if (lane < len - done) {
        const uint8_t *t = src + done + lane;
        dst[done + lane] = (uint8_t)pmx_codon(cls, cod, t[0], t[1], t[2], 0u);
    }
}

// ---- the windowed reference-side frameshift traceback (the _frameshift_ref_cigar_long entries) -------------------------
// Between the score pass and the trace pass: pair k's folded record (score S, end cell (eq, er) in the oriented reference window) and
// strand byte become the descriptor of the only sub-window a path of that record can lie in -- query rows [0, eq], oriented nucleotides
// [a, er + 1) with a = max(0, er + 1 - W), W = pmx_fswin_cols (pmx_fswin.h) -- in stored coordinates: oriented [a, b) of a strand-1
// window is stored [r_beg + rl - b, r_beg + rl - a), rl the resolved length (r_len -1 is resolved here).  A 16-lane group per pair:
// the lanes sum max(0, max_b s(q_i, b)) over the query letters 0 .. eq, lane-strided, from a table of the matrix's row maxima staged
// in LDS, and a shuffle reduction over the group leaves P in lane 0.  A zero-score record (eq 0, er 2) gets the 1 x 3 window the
// formula gives, which scores zero again.  A bad record, or one whose end cell lies outside its resolved windows, gets a descriptor
// that is bad whatever the maxima (q = -1), shift 0 and lengths 0.  A narrowed r_beg that would not fit 32 bits leaves the pair's
// descriptor as it is (shift 0): the whole window is a sound window.  nlen[2 k], nlen[2 k + 1]: the narrowed query letters and the
// narrowed stream's letters, what the host cuts the parts of the trace pass by.
__global__ __launch_bounds__(256)
void pmx_fsref_window_kernel(const pmx_pair_t *__restrict__ pairs, const pmx_record_t *__restrict__ rec, const uint8_t *__restrict__ strand,
                             long long n, const uint8_t *__restrict__ q_buf,
                             const int64_t *__restrict__ q_off, long long q_count, long long q_bytes,
                             const int64_t *__restrict__ r_off, long long r_count, long long r_bytes,
                             const int16_t *__restrict__ scores, const uint8_t *__restrict__ mapper, int msize, int open, int ext, int fs,
                             pmx_pair_t *__restrict__ npairs, int32_t *__restrict__ ashift, int32_t *__restrict__ nlen)
{
    __shared__ int rowmax[256];                                   // max(0, the row's largest score); 0 for an index the matrix does not have
    __shared__ uint8_t map[256];
    {
        const int t = threadIdx.x;
        int v = 0;
        if (t < msize) for (int b = 0; b < msize; ++b) v = max(v, (int)scores[t * msize + b]);
        rowmax[t] = v; map[t] = mapper[t];
    }
    __syncthreads();
    const long long k = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int lane = threadIdx.x & 15;
    const bool live = k < n;                                      // (uniform per group; every lane reaches the shuffles)
    pmx_pair_t p = {}; pmx_record_t r = {};
    long long qs = 0, rs = 0; int32_t ql = 0, rl = 0;
    bool good = false;
    if (live) {
        p = pairs[k]; r = rec[k];
        good = !(r.flags & PMX_FLAG_BAD_PAIR) &&
               pmx_resolve_pair(p, q_off, q_count, q_bytes, r_off, r_count, r_bytes, INT32_MAX, INT32_MAX, &ql, &rl, &qs, &rs) &&
               r.end_query >= 0 && r.end_query < ql && r.end_ref >= 2 && r.end_ref < rl;
    }
    int P = 0;                                                    // (at most 4 096 rows x 32 767)
    if (good) for (int i = lane; i <= r.end_query; i += 16) P += rowmax[map[q_buf[qs + i]]];
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) P += __shfl_xor(P, d, 16);
    if (!live || lane) return;
    pmx_pair_t o = p; int32_t a = 0, nq = 0, nr = 0;
    if (!good) o.q = -1;
    else {
        const long long W = pmx_fswin_cols(P, r.score, (long long)r.end_query + 1, open, ext, fs);
        const long long b = (long long)r.end_ref + 1, lo = W >= b ? 0 : b - W;
        const long long beg = (long long)p.r_beg + (strand[k] ? (long long)rl - b : lo);
        if (beg <= (long long)INT32_MAX) {
            a = (int32_t)lo;
            o.q_len = r.end_query + 1; o.r_beg = (int32_t)beg; o.r_len = (int32_t)(b - lo);
            nq = o.q_len; nr = o.r_len - 2;
        } else { nq = ql; nr = rl - 2; }
    }
    npairs[k] = o; ashift[k] = a; nlen[2 * k] = nq; nlen[2 * k + 1] = nr;
}

// Behind the trace pass over the narrowed descriptors: end_ref and beg_ref back into the pair's own oriented window (+ a), and the proof
// of DESIGN 2.5o held against the score pass -- the rebased record equals the first pass's record field by field, or the pair is
// counted in violations[0].  A bad pair and a zero-score record have a = 0.
__global__ __launch_bounds__(256)
void pmx_fsref_rebase_kernel(const pmx_record_t *__restrict__ first, const int32_t *__restrict__ ashift, long long n,
                             pmx_record_t *__restrict__ rec, int32_t *__restrict__ beg, unsigned *__restrict__ violations)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    pmx_record_t r = rec[k];
    const pmx_record_t f = first[k];
    const int32_t a = ashift[k];
    if (a) { r.end_ref += a; rec[k] = r; if (beg) beg[2 * k + 1] += a; }
    if (r.score != f.score || r.end_query != f.end_query || r.end_ref != f.end_ref || r.flags != f.flags) atomicAdd(violations, 1u);
}

// Bad pairs on the device CIGAR road, between the walk and the text scan: the record, no ops, no text, begins -1 / -1.
__global__ __launch_bounds__(256)
void pmx_pairs_fixup_cigar_kernel(const uint8_t *__restrict__ ok, long long n, pmx_record_t *__restrict__ rec,
                                  int32_t *__restrict__ nops, int32_t *__restrict__ textlen, int32_t *__restrict__ beg)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n || ok[k]) return;
    pmx_record_t r; r.score = 0; r.end_query = -1; r.end_ref = -1; r.flags = PMX_FLAG_BAD_PAIR;
    rec[k] = r; nops[k] = 0; textlen[k] = 0;
    if (beg) { beg[2 * k] = -1; beg[2 * k + 1] = -1; }
}

// A later chunk's text offsets: its own scan (from 0) behind the running total the previous chunk left in text_off[0].
__global__ __launch_bounds__(256)
void pmx_text_rebase_kernel(const int64_t *__restrict__ local, long long n, int64_t *text_off)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x + 1;
    if (j > n) return;
    text_off[j] = text_off[0] + local[j];
}

__global__ __launch_bounds__(256)
void pmx_pairs_fixup_kernel(const uint8_t *__restrict__ ok, long long n, pmx_record_t *__restrict__ rec, pmx_stats_t *__restrict__ stats)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n || ok[k]) return;
    pmx_record_t r; r.score = 0; r.end_query = -1; r.end_ref = -1; r.flags = PMX_FLAG_BAD_PAIR;
    rec[k] = r;
    if (stats) { pmx_stats_t s; s.matches = 0; s.similar = 0; s.length = 0; stats[k] = s; }
}

// Row i of the strict upper triangle of N x N starts at pair s(i) = i (2 N - i - 1) / 2; i is the largest row with s(i) <= p.  The root
// of (2 N - 1)^2 - 8 p in floating point gives i to within a step or two; the loops settle it in unsigned 64-bit arithmetic, exactly.
// (2 N - 1)^2 < 2^64 and i (2 N - i - 1) < 2^63 for N <= 2^31 - 1.
static __host__ __device__ inline unsigned long long pmx_row_start(unsigned long long N, unsigned long long i) { return i * (2 * N - i - 1) / 2; }
static __host__ __device__ inline void pmx_pair_of(unsigned long long N, unsigned long long p, unsigned long long *pi, unsigned long long *pj)
{
    const unsigned long long b = 2 * N - 1, d = b * b - 8 * p;
    const double root = sqrt((double)d);
    double est = ((double)b - root) * 0.5;
    unsigned long long i = est <= 0.0 ? 0 : (unsigned long long)est;
    if (i > N - 2) i = N - 2;
    while (i > 0 && pmx_row_start(N, i) > p) --i;
    while (i < N - 2 && pmx_row_start(N, i + 1) <= p) ++i;
    *pi = i; *pj = i + 1 + (p - pmx_row_start(N, i));
}

__global__ __launch_bounds__(256)
void pmx_all_pairs_enumerate_kernel(long long nseq, long long first, long long count, pmx_pair_t *__restrict__ pairs)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    unsigned long long i, j;
    pmx_pair_of((unsigned long long)nseq, (unsigned long long)(first + t), &i, &j);
    pmx_pair_t d; d.q = (int64_t)i; d.r = (int64_t)j; d.q_beg = 0; d.q_len = -1; d.r_beg = 0; d.r_len = -1;
    pairs[t] = d;
}

// Row-major Q x R: pair p is (p / nr, p % nr), the descriptor form of the kernel above.  p < nq * nr <= INT64_MAX, in unsigned 64-bit.
__global__ __launch_bounds__(256)
void pmx_rect_pairs_enumerate_kernel(unsigned long long nr, long long first, long long count, pmx_pair_t *__restrict__ pairs)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const unsigned long long p = (unsigned long long)(first + t), i = p / nr;
    pmx_pair_t d; d.q = (int64_t)i; d.r = (int64_t)(p - i * nr); d.q_beg = 0; d.q_len = -1; d.r_beg = 0; d.r_len = -1;
    pairs[t] = d;
}

// ---- set search: a chunk's hits behind the hits of the chunks before it ----------------------------------------------------------
// idx[0 .. chunk_counts[0]) are the chunk-local positions of the chunk's hits in ascending order (pmx_launch_select, by index, no
// limit); counts[0] is the number of hits of the earlier chunks.  Hit x of the chunk goes to position counts[0] + x when that lies
// below `capacity`: where a hit lands depends on the selection's scan and the total alone, never on which block runs first.  counts is
// only read here; pmx_pairs_advance_hits_kernel moves it, behind this kernel on the same stream.  A descriptor is 32 bytes: two
// 16-byte accesses where both sides are 16-byte aligned (they are for hipMalloc'ed arrays), four 8-byte ones otherwise.
// The stranded searches: `marked` says the chunk's records carry their strand as PMX_FLAG_STRAND1, which is taken out of the record on
// its way to the caller; hit_strand (optional) receives it as a byte.  A launch without either copies the record as it is.
// marked == 2 (the translated searches): the records carry their frame in PMX_FLAG_FRAME_MASK instead, and the byte is the frame.
__global__ __launch_bounds__(256)
void pmx_pairs_append_hits_kernel(const int64_t *__restrict__ idx, const int64_t *__restrict__ chunk_counts, const int64_t *__restrict__ counts,
                                  long long capacity, long long index0, const pmx_pair_t *__restrict__ pairs,
                                  const pmx_record_t *__restrict__ rec, const pmx_stats_t *__restrict__ stats,
                                  pmx_pair_t *__restrict__ hit_pairs, int64_t *__restrict__ hit_index,
                                  pmx_record_t *__restrict__ hit_recs, pmx_stats_t *__restrict__ hit_stats,
                                  uint8_t *__restrict__ hit_strand, int marked)
{
    const long long h = chunk_counts[0], base = counts[0];
    const bool wide = (((uintptr_t)pairs | (uintptr_t)hit_pairs) & 15) == 0;
    for (long long x = (long long)blockIdx.x * 256 + threadIdx.x; x < h; x += (long long)gridDim.x * 256) {
        const long long pos = base + x;
        if (pos >= capacity) return;                              // (positions ascend with x)
        const long long k = idx[x];
        if (hit_pairs) {
            if (wide) {
                const uint4 *s = reinterpret_cast<const uint4 *>(pairs + k);
                uint4 *d = reinterpret_cast<uint4 *>(hit_pairs + pos);
                const uint4 a = s[0], b = s[1];
                d[0] = a; d[1] = b;
            } else
                hit_pairs[pos] = pairs[k];
        }
        if (hit_index) hit_index[pos] = index0 + k;
        pmx_record_t r = rec[k];
        if (marked == 2) {                                        // (the translated searches: the byte is the frame)
            if (hit_strand) hit_strand[pos] = (uint8_t)((r.flags & PMX_FLAG_FRAME_MASK) >> PMX_FLAG_FRAME_SHIFT);
            r.flags &= ~PMX_FLAG_FRAME_MASK;
        } else {
            if (hit_strand) hit_strand[pos] = (uint8_t)((r.flags & PMX_FLAG_STRAND1) != 0);
            if (marked) r.flags &= ~PMX_FLAG_STRAND1;
        }
        hit_recs[pos] = r;
        if (hit_stats) hit_stats[pos] = stats[k];
    }
}

__global__ void pmx_pairs_advance_hits_kernel(const int64_t *__restrict__ chunk_counts, long long capacity, int64_t *__restrict__ counts)
{
    const long long total = counts[0] + chunk_counts[0];
    counts[0] = total; counts[1] = total < capacity ? total : capacity;
}

// first_bad[0] (the caller sets it to INT64_MAX) = the lowest index0 + k with ok[k] == 0.  One atomic per wave that holds a bad pair.
__global__ __launch_bounds__(256)
void pmx_pairs_first_bad_kernel(const uint8_t *__restrict__ ok, long long n, long long index0, unsigned long long *__restrict__ first_bad)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long bad = __ballot(k < n && !ok[k]);
    if (bad && (threadIdx.x & 63) == 0) atomicMin(first_bad, (unsigned long long)(index0 + k + __ffsll((long long)bad) - 1));
}

// out[0] / out[1] = the longest good query / reference window (0: none), the caller zeroes them.  pairs == nullptr: the n whole
// sequences of the query-side set.  One atomic per wave and side.
__global__ __launch_bounds__(256)
void pmx_pairs_maxlen_kernel(const pmx_pair_t *__restrict__ pairs, long long n,
                             const int64_t *__restrict__ q_off, long long q_count, long long q_bytes,
                             const int64_t *__restrict__ r_off, long long r_count, long long r_bytes, int32_t *__restrict__ out)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    int32_t ql = 0, rl = 0;
    if (k < n) {
        long long s = 0;
        if (pairs) {
            const pmx_pair_t p = pairs[k];
            ql = pmx_resolve_side(q_off, q_count, q_bytes, p.q, p.q_beg, p.q_len, INT32_MAX, &s);
            rl = pmx_resolve_side(r_off, r_count, r_bytes, p.r, p.r_beg, p.r_len, INT32_MAX, &s);
        } else
            ql = rl = pmx_resolve_side(q_off, q_count, q_bytes, k, 0, -1, INT32_MAX, &s);
    }
    for (int d = 32; d >= 1; d >>= 1) { ql = max(ql, __shfl_xor(ql, d)); rl = max(rl, __shfl_xor(rl, d)); }
    if ((threadIdx.x & 63) == 0) { if (ql > 0) atomicMax(&out[0], ql); if (rl > 0) atomicMax(&out[1], rl); }
}

int pmx_launch_pairs_resolve(const pmx_pair_t *pairs, const uint8_t *strand, int first, int per, long long n,
                             const int64_t *q_off, long long q_count, long long q_bytes,
                             const int64_t *r_off, long long r_count, long long r_bytes, int32_t max_qlen, int32_t max_rlen,
                             int32_t *qlen, int32_t *rlen, int64_t *qsrc, int64_t *rsrc, uint8_t *ok, uint8_t *sflag, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_pairs_resolve_kernel, dim3((unsigned)((n + 2 + 255) / 256)), dim3(256), 0, st, pairs, strand, first, per, n,
                       q_off, q_count, q_bytes, r_off, r_count, r_bytes, max_qlen, max_rlen, qlen, rlen, qsrc, rsrc, ok, sflag);
    return pmx_launched();
}
int pmx_launch_pairs_gather(long long n, const uint8_t *q_buf, long long q_bytes, const uint8_t *r_buf, long long r_bytes,
                            const int32_t *qlen, const int32_t *rlen, const int64_t *qsrc, const int64_t *rsrc, const uint8_t *ok,
                            const int64_t *qoff, const int64_t *roff, uint8_t *qout, uint8_t *rout, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_pairs_gather_kernel, dim3((unsigned)((2 * n + 15) / 16)), dim3(256), 0, st, n, q_buf, q_bytes, r_buf, r_bytes,
                       qlen, rlen, qsrc, rsrc, ok, qoff, roff, qout, rout);
    return pmx_launched();
}
int pmx_launch_pairs_fixup(const uint8_t *ok, long long n, pmx_record_t *rec, pmx_stats_t *stats, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_pairs_fixup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ok, n, rec, stats);
    return pmx_launched();
}
int pmx_launch_pairs_gather_stranded(long long n, const uint8_t *q_buf, long long q_bytes, const uint8_t *r_buf, long long r_bytes,
                                     const int32_t *qlen, const int32_t *rlen, const int64_t *qsrc, const int64_t *rsrc, const uint8_t *ok,
                                     const uint8_t *sflag, const int64_t *qoff, const int64_t *roff,
                                     uint8_t *qout, long long q_cap, uint8_t *rout, long long r_cap, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_pairs_gather_stranded_kernel, dim3((unsigned)((2 * n + 15) / 16)), dim3(256), 0, st, n, q_buf, q_bytes, r_buf, r_bytes,
                       qlen, rlen, qsrc, rsrc, ok, sflag, qoff, roff, qout, q_cap, rout, r_cap);
    return pmx_launched();
}
int pmx_launch_pairs_fold(const pmx_record_t *slot_rec, const pmx_stats_t *slot_stats, const uint8_t *ok, const uint8_t *sflag,
                          long long n, int per, int mark, pmx_record_t *rec, pmx_stats_t *stats, uint8_t *byte, uint8_t *okf, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_pairs_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slot_rec, slot_stats, ok, sflag,
                       n, per, mark, rec, stats, byte, okf);
    return pmx_launched();
}
void pmx_genetic_code_host(uint8_t table[64]) { for (int i = 0; i < 64; ++i) table[i] = (uint8_t)pmx_code_std[i]; }
// (the translated side is a template argument of these four kernels: the launcher picks the instance)
int pmx_launch_pairs_resolve_frames(const pmx_pair_t *pairs, const uint8_t *frame, int first, int per, long long n,
                                    const int64_t *q_off, long long q_count, long long q_bytes,
                                    const int64_t *r_off, long long r_count, long long r_bytes, int32_t max_qlen, int32_t max_rlen,
                                    int32_t *qlen, int32_t *rlen, int32_t *tw, int64_t *qsrc, int64_t *rsrc, uint8_t *ok, uint8_t *sflag, hipStream_t st,
                                    bool ref)
{
    if (n <= 0) return 0;
    const auto kernel = ref ? pmx_pairs_resolve_frames_kernel<true> : pmx_pairs_resolve_frames_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 2 + 255) / 256)), dim3(256), 0, st, pairs, frame, first, per, n,
                       q_off, q_count, q_bytes, r_off, r_count, r_bytes, max_qlen, max_rlen, qlen, rlen, tw, qsrc, rsrc, ok, sflag);
    return pmx_launched();
}
int pmx_launch_pairs_gather_translated(long long n, const uint8_t *q_buf, long long q_bytes, const uint8_t *r_buf, long long r_bytes,
                                       const int32_t *qlen, const int32_t *rlen, const int32_t *tw, const int64_t *qsrc, const int64_t *rsrc,
                                       const uint8_t *ok, const uint8_t *sflag, const int64_t *qoff, const int64_t *roff,
                                       uint8_t *qout, long long q_cap, uint8_t *rout, long long r_cap, const PmxCodeTable &code, hipStream_t st,
                                       bool ref)
{
    if (n <= 0) return 0;
    const auto kernel = ref ? pmx_pairs_gather_translated_kernel<true> : pmx_pairs_gather_translated_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((2 * n + 15) / 16)), dim3(256), 0, st, n, q_buf, q_bytes, r_buf, r_bytes,
                       qlen, rlen, tw, qsrc, rsrc, ok, sflag, qoff, roff, qout, q_cap, rout, r_cap, code);
    return pmx_launched();
}
int pmx_launch_pairs_resolve_codons(const pmx_pair_t *pairs, const uint8_t *strand, int first, int per, long long n,
                                    const int64_t *q_off, long long q_count, long long q_bytes,
                                    const int64_t *r_off, long long r_count, long long r_bytes, int32_t max_qlen, int32_t max_rlen,
                                    int32_t *qlen, int32_t *rlen, int32_t *tw, int64_t *qsrc, int64_t *rsrc, uint8_t *ok, uint8_t *sflag, hipStream_t st,
                                    bool ref)
{
    if (n <= 0) return 0;
    const auto kernel = ref ? pmx_pairs_resolve_codons_kernel<true> : pmx_pairs_resolve_codons_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 2 + 255) / 256)), dim3(256), 0, st, pairs, strand, first, per, n,
                       q_off, q_count, q_bytes, r_off, r_count, r_bytes, max_qlen, max_rlen, qlen, rlen, tw, qsrc, rsrc, ok, sflag);
    return pmx_launched();
}
int pmx_launch_pairs_gather_codons(long long n, const uint8_t *q_buf, long long q_bytes, const uint8_t *r_buf, long long r_bytes,
                                   const int32_t *qlen, const int32_t *rlen, const int32_t *tw, const int64_t *qsrc, const int64_t *rsrc,
                                   const uint8_t *ok, const uint8_t *sflag, const int64_t *qoff, const int64_t *roff,
                                   uint8_t *qout, long long q_cap, uint8_t *rout, long long r_cap, const PmxCodeTable &code, hipStream_t st,
                                   bool ref)
{
    if (n <= 0) return 0;
    const auto kernel = ref ? pmx_pairs_gather_codons_kernel<true> : pmx_pairs_gather_codons_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((2 * n + 15) / 16)), dim3(256), 0, st, n, q_buf, q_bytes, r_buf, r_bytes,
                       qlen, rlen, tw, qsrc, rsrc, ok, sflag, qoff, roff, qout, q_cap, rout, r_cap, code);
    return pmx_launched();
}
extern "C" long long pmx_swfsc_window_cols(long long rowmax_prefix, long long score, long long rows, long long open, long long extend, long long fs)
{
    return pmx_fswin_cols(rowmax_prefix, score, rows, open, extend, fs);
}
int pmx_launch_fsref_window(const pmx_pair_t *pairs, const pmx_record_t *rec, const uint8_t *strand, long long n, const uint8_t *q_buf,
                            const int64_t *q_off, long long q_count, long long q_bytes, const int64_t *r_off, long long r_count, long long r_bytes,
                            const PmxDevMatrix &m, int open, int ext, int fs, pmx_pair_t *npairs, int32_t *ashift, int32_t *nlen, hipStream_t st)
{
    if (m.pssm || m.msize > 256) return 1;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_fsref_window_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, pairs, rec, strand, n, q_buf,
                       q_off, q_count, q_bytes, r_off, r_count, r_bytes, m.scores, m.mapper, m.msize, open, ext, fs, npairs, ashift, nlen);
    return pmx_launched();
}
int pmx_launch_fsref_rebase(const pmx_record_t *first, const int32_t *ashift, long long n, pmx_record_t *rec, int32_t *beg, unsigned *violations,
                            hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_fsref_rebase_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, first, ashift, n, rec, beg, violations);
    return pmx_launched();
}
int pmx_launch_pairs_fixup_cigar(const uint8_t *ok, long long n, pmx_record_t *rec, int32_t *nops, int32_t *textlen, int32_t *beg, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_pairs_fixup_cigar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ok, n, rec, nops, textlen, beg);
    return pmx_launched();
}
int pmx_launch_text_rebase(const int64_t *local, long long n, int64_t *text_off, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_text_rebase_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, local, n, text_off);
    return pmx_launched();
}
void pmx_complement_table_host(uint8_t table[256])
{
    for (int i = 0; i < 256; ++i) table[i] = pmx_comp_host.v[i];
}
int pmx_launch_all_pairs_enumerate(long long nseq, long long first, long long count, pmx_pair_t *pairs, hipStream_t st)
{
    if (count <= 0) return 0;
    hipLaunchKernelGGL(pmx_all_pairs_enumerate_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, nseq, first, count, pairs);
    return pmx_launched();
}
int pmx_launch_rect_pairs_enumerate(long long nr, long long first, long long count, pmx_pair_t *pairs, hipStream_t st)
{
    if (count <= 0) return 0;
    hipLaunchKernelGGL(pmx_rect_pairs_enumerate_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (unsigned long long)nr, first, count, pairs);
    return pmx_launched();
}
int pmx_launch_pairs_append_hits(const int64_t *idx, const int64_t *chunk_counts, long long n, long long capacity, long long index0,
                                 const pmx_pair_t *pairs, const pmx_record_t *rec, const pmx_stats_t *stats,
                                 pmx_pair_t *hit_pairs, int64_t *hit_index, pmx_record_t *hit_recs, pmx_stats_t *hit_stats, int64_t *counts, hipStream_t st,
                                 uint8_t *hit_strand, int marked)
{
    if (n <= 0) return 0;
    if (capacity > 0) {                                            // (the hit count is on the device: a grid for the chunk, capped; the loop strides)
        const long long blocks = (n + 255) / 256;
        hipLaunchKernelGGL(pmx_pairs_append_hits_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, idx, chunk_counts,
                           (const int64_t *)counts, capacity, index0, pairs, rec, stats, hit_pairs, hit_index, hit_recs, hit_stats, hit_strand, marked);
    }
    hipLaunchKernelGGL(pmx_pairs_advance_hits_kernel, dim3(1), dim3(1), 0, st, chunk_counts, capacity, counts);
    return pmx_launched();
}
int pmx_launch_pairs_first_bad(const uint8_t *ok, long long n, long long index0, int64_t *first_bad, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_pairs_first_bad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ok, n, index0, (unsigned long long *)first_bad);
    return pmx_launched();
}
int pmx_launch_pairs_maxlen(const pmx_pair_t *pairs, long long n, const int64_t *q_off, long long q_count, long long q_bytes,
                            const int64_t *r_off, long long r_count, long long r_bytes, int32_t *out, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pmx_pairs_maxlen_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pairs, n, q_off, q_count, q_bytes,
                       r_off, r_count, r_bytes, out);
    return pmx_launched();
}
void pmx_all_pairs_index_host(unsigned long long nseq, unsigned long long p, unsigned long long *i, unsigned long long *j)
{
    pmx_pair_of(nseq, p, i, j);
}
