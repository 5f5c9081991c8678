// pmx_fs.h -- the one launcher of the two frameshift sweeps (pmx_swfs.hip: the codon stream on the rows; pmx_swfsc.hip: on the columns).
// Host code only: the kernels' text stays in their files, byte for byte ("One launcher").  Each file instantiates the
// launcher twice -- the score form and the trace form of its kernel -- and fills its PmxFsSide (pmx_common.h) with them.
#pragma once
#include "pmx_common.h"

// What the two kernels share: everything but the element type of the boundary scratch (int4: seven values per column; int2: two).
template <typename Bnd>
using PmxFsKernel = void (*)(const uint8_t *, const int64_t *, const uint8_t *, const int64_t *, long long, int, int, const int16_t *, const uint8_t *, int,
                             int, int, int, Bnd *, pmx_record_t *, uint32_t *, long long);

// LDS of a launch: the transposed matrix as int16 and the byte map.
static inline size_t pmx_fs_lds_bytes(int msize) { return (size_t)msize * msize * 2 + 256; }

// n slots of up to b.max_qlen rows x b.max_rlen columns through kernel K of the side pmx_fs_side(REF), whose launch / launch_trace the
// instantiation is.  0 launched, 1 not eligible, <0 HIP error.
//   score form (trace == NULL, K without TR): bnd is boundary scratch for `bnd_slots` slots, needed when b.max_qlen exceeds one strip;
//     the launch then runs in parts of bnd_slots slots, one behind the other on `stream`.
//   trace form (TRACED, K with TR): the same sweep and records, and every cell's decision byte into `trace`, which
//     holds side.trace_bytes_per_slot bytes for each of the launch's slots ROUNDED UP TO WHOLE WORKGROUPS of four (the idle slots of the
//     last workgroup repeat slot n - 1 into their own regions); bnd: boundary scratch for as many slots when b.max_qlen exceeds one
//     strip.  One launch: the caller cuts a chunk into parts that fit its scratch.
template <typename Bnd, PmxFsKernel<Bnd> K, bool TRACED, bool REF>
static int pmx_fs_launch(const PmxBatch &b, const PmxDevMatrix &m, int open, int ext, int fs, void *bnd, long long bnd_slots, void *trace,
                         pmx_record_t *d_out, hipStream_t stream, const char **kernel_name)
{
    const PmxFsSide &side = pmx_fs_side(REF);
    const int NPW = 64 / (side.strip_rows / side.lane_rows);      // slots per wave = per workgroup
    if (m.pssm || m.msize > side.max_msize || b.q_shared || (TRACED && !trace)) return 1;
    if (b.n <= 0) return 0;
    const int cap = 1 << 28;
    open = open < cap ? open : cap; ext = ext < cap ? ext : cap; fs = fs < cap ? fs : cap;
    const bool strips = b.max_qlen > side.strip_rows;
    if (strips && (!bnd || (!TRACED && bnd_slots < NPW))) return 1;
    const long long part = strips && !TRACED ? bnd_slots / NPW * NPW : b.n;
    const long long trace_stride = TRACED ? side.trace_bytes_per_slot(b.max_qlen, b.max_rlen) / 4 : 0LL;
    for (long long p0 = 0; p0 < b.n; p0 += part) {
        const long long pn = b.n - p0 < part ? b.n - p0 : part;
        hipLaunchKernelGGL(K, dim3((unsigned)((pn + NPW - 1) / NPW)), dim3(64), pmx_fs_lds_bytes(m.msize), stream,
                           b.qbuf, b.qoff + p0, b.rbuf, b.roff + p0, pn, b.max_qlen, b.max_rlen, m.scores, m.mapper, m.msize,
                           open, ext, fs, strips ? (Bnd *)bnd : nullptr, d_out + p0, (uint32_t *)trace, trace_stride);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return -(int)e;
    }
    if (kernel_name) *kernel_name = side.names[TRACED][strips];
    return 0;
}
