// pmx_fswin.h -- the window bound of the windowed reference-side frameshift traceback: how many nucleotides of the
// oriented reference window, counted back from a record's end_ref, a local path of that record's score can span.  One function, shared
// by pmx_fsref_window_kernel (pmx_pairs.hip) and the test hook pmx_swfsc_window_cols.
//
// A path of pmx_swfsc's recurrence with score S that ends in row eq has mc <= rows = eq + 1 match columns on distinct rows, cg codon-gap
// columns and ns frameshift operators of the long kind (a short one only shortens the path), ns <= mc - 1: an operator leads into a
// match column other than the first.  Its match columns score at most P = sum over rows 0 .. eq of max(0, max_b s(q_i, b)); a run of k
// codon gaps costs open + (k - 1) extend >= k gmin with gmin = min(open, extend), query gaps cost too and span nothing, an operator
// costs fs.  So cg gmin + ns fs <= P - S = slack, and the span 3 (mc + cg) + ns - #short is at most
//     W = 3 rows + 3 floor(slack / gmin) + min(rows - 1, floor(slack / fs))                    (fs = 0: the last term is rows - 1).
// gmin = 0 bounds nothing: PMX_FSWIN_ALL, the whole window.  Penalties are read as the kernel reads them, capped at 2^28.
#pragma once
#include <stdint.h>

#define PMX_FSWIN_ALL INT64_MAX

static __host__ __device__ inline long long pmx_fswin_cols(long long rowmax_prefix, long long score, long long rows,
                                                           long long open, long long ext, long long fs)
{
    const long long cap = 1LL << 28;
    open = open < cap ? open : cap; ext = ext < cap ? ext : cap; fs = fs < cap ? fs : cap;
    const long long gmin = open < ext ? open : ext, slack = rowmax_prefix - score;
    if (gmin <= 0 || fs < 0 || rows < 1 || slack < 0 || slack > (1LL << 40) || rows > (1LL << 40)) return PMX_FSWIN_ALL;
    const long long shifts = fs > 0 && slack / fs < rows - 1 ? slack / fs : rows - 1;
    return 3 * rows + 3 * (slack / gmin) + shifts;
}
