/* swfsc_trace_model.c -- CPU model of the reference-side frameshift traceback (test infrastructure only), written from the contract in
 * include/parasail_amd.h ("Frameshift traceback, reference side"): the three-frame recurrence with the protein on the rows and the
 * reference's codon stream on the columns over whole matrices, the decisions of every cell, the walk with its six move kinds, begins
 * and statistics, and the strand fold.  It restates the recurrence of swfsc_model.c on purpose: the tests hold the two against each
 * other.  Nothing here follows a kernel's layout. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG_INF (-(1LL << 60))
/* run-length ops are (count << 4) | code; codes: BAM's "MIDNSHP=X", then '/' = 9 and '\' = 10 */
enum { OP_QUERY_GAP = 1 /* 'I' by default: the F state */, OP_CODON_GAP = 2 /* 'D' by default: the E state */, OP_EQ = 7, OP_X = 8,
       OP_SHORT = 9, OP_LONG = 10 };
enum { SRC_M = 0, SRC_F = 1, SRC_E = 2, SRC_ZERO = 3 };
enum { D_START = 0, D_INFRAME = 1, D_SHORT = 2, D_LONG = 3 };

static int base_class(uint8_t b)
{
    switch (b) {
    case 'T': case 't': case 'U': case 'u': return 0;
    case 'C': case 'c': return 1;
    case 'A': case 'a': return 2;
    case 'G': case 'g': return 3;
    }
    return -1;
}

static uint8_t complement(uint8_t b)
{
    switch (b) {
    case 'A': return 'T'; case 'a': return 't';
    case 'C': return 'G'; case 'c': return 'g';
    case 'G': return 'C'; case 'g': return 'c';
    case 'T': case 'U': return 'A'; case 't': case 'u': return 'a';
    }
    return b;
}

static void codon_stream(const uint8_t *window, int W, int strand, const uint8_t *code, uint8_t *out)
{
    uint8_t *o = (uint8_t *)malloc((size_t)W);
    for (int i = 0; i < W; ++i) o[i] = strand ? complement(window[W - 1 - i]) : window[i];
    for (int i = 0; i + 2 < W; ++i) {
        const int a = base_class(o[i]), b = base_class(o[i + 1]), c = base_class(o[i + 2]);
        out[i] = (a < 0 || b < 0 || c < 0) ? (uint8_t)'X' : code[16 * a + 4 * b + c];
    }
    free(o);
}

/* q: the protein, m rows; T: the codon stream, N columns.  ops: room for m + N entries, filled from the front in path order; returns
 * their count.  beg[2] = (query letter, reference nucleotide), stats[3] = matches, similar, length. */
int swfsc_trace_align(const uint8_t *q, int m, const uint8_t *T, int N, const int32_t *scores, const int32_t *mapper, int msize,
                      int open, int ext, long long fs, int32_t *rec, uint32_t *ops, int32_t *beg, int32_t *stats)
{
    const size_t cells = (size_t)m * N;
    long long *H = (long long *)malloc(sizeof(long long) * cells), *E = (long long *)malloc(sizeof(long long) * cells),
              *F = (long long *)malloc(sizeof(long long) * cells);
    uint8_t *hsrc = (uint8_t *)malloc(cells), *dsrc = (uint8_t *)malloc(cells), *eo = (uint8_t *)malloc(cells), *fo = (uint8_t *)malloc(cells);
#define AT(X, i, j, none) (((i) < 0 || (j) < 0) ? (none) : X[(size_t)(i) * N + (j)])
    long long best = 0; int bi = 0, bj = 0;
    for (int j = 0; j < N; ++j)                             /* column-major: the first maximum is the smallest end_ref, then end_query */
        for (int i = 0; i < m; ++i) {
            const size_t c = (size_t)i * N + j;
            const long long h3 = AT(H, i - 1, j - 3, 0), h2 = AT(H, i - 1, j - 2, 0) - fs, h4 = AT(H, i - 1, j - 4, 0) - fs;
            long long D = 0;
            if (h3 > D) D = h3;
            if (h2 > D) D = h2;
            if (h4 > D) D = h4;
            dsrc[c] = D == 0 ? D_START : h3 == D ? D_INFRAME : h2 == D ? D_SHORT : D_LONG;
            const long long M = D + scores[mapper[q[i]] * msize + mapper[T[j]]];          /* s(query letter, stream letter) */
            const long long eopen = AT(H, i, j - 3, 0) - open, eext = AT(E, i, j - 3, NEG_INF) - ext;
            const long long fopen = AT(H, i - 1, j, 0) - open, fext = AT(F, i - 1, j, NEG_INF) - ext;
            eo[c] = eopen > eext; fo[c] = fopen > fext;
            const long long e = eo[c] ? eopen : eext, f = fo[c] ? fopen : fext;
            long long h; int src;
            if (M >= e && M >= f) { h = M; src = SRC_M; }
            else if (f >= e) { h = f; src = SRC_F; }
            else { h = e; src = SRC_E; }
            if (h <= 0) { h = 0; src = SRC_ZERO; }
            hsrc[c] = (uint8_t)src;
            H[c] = h; E[c] = e; F[c] = f;
            if (h > best) { best = h; bi = i; bj = j; }
        }
#undef AT
    rec[0] = (int32_t)best; rec[1] = bi; rec[2] = bj + 2; rec[3] = 0;
    free(H); free(E); free(F);

    /* the walk, from the end cell backwards; `back` collects single ops in reverse path order */
    uint8_t *back = (uint8_t *)malloc((size_t)2 * (N + m) + 8);
    int nb = 0, i = bi, j = bj, state = SRC_M, nM = 0, nS = 0, nL = 0;
    int begi = bi + 1, begj = bj + 3;                       /* an empty path: (end_query + 1, end_ref + 1) */
    if (best > 0)
        for (;;) {
            const size_t c = (size_t)i * N + j;
            if (state == SRC_M) {
                if (hsrc[c] == SRC_F) { state = SRC_F; continue; }
                if (hsrc[c] == SRC_E) { state = SRC_E; continue; }
                if (hsrc[c] == SRC_ZERO) abort();           /* no path passes through a ZERO cell */
                const int a = mapper[q[i]], b = mapper[T[j]];
                back[nb++] = a == b ? OP_EQ : OP_X;
                nM += a == b; nS += scores[a * msize + b] > 0; nL += 1;
                if (dsrc[c] == D_START) { begi = i; begj = j; break; }
                if (dsrc[c] == D_INFRAME) { j -= 3; }
                else if (dsrc[c] == D_SHORT) { back[nb++] = OP_SHORT; j -= 2; }
                else { back[nb++] = OP_LONG; j -= 4; }
                i -= 1;
            } else if (state == SRC_F) {                    /* one query letter against a gap */
                back[nb++] = OP_QUERY_GAP; nL += 1;
                if (fo[c]) state = SRC_M;
                i -= 1;
            } else {                                        /* one whole reference codon against a gap */
                back[nb++] = OP_CODON_GAP; nL += 1;
                if (eo[c]) state = SRC_M;
                j -= 3;
            }
            if (i < 0 || j < 0) abort();
        }
    int nops = 0;
    for (int k = nb - 1; k >= 0; --k) {
        if (nops && (ops[nops - 1] & 15u) == back[k]) ops[nops - 1] += 16u;
        else ops[nops++] = 16u | back[k];
    }
    beg[0] = begi; beg[1] = begj;
    stats[0] = nM; stats[1] = nS; stats[2] = nL;
    free(back); free(hsrc); free(dsrc); free(eo); free(fo);
    return nops;
}

/* One pair on the reference strands of `mode` (0 forward, 1 reverse, 2 both: the reverse strand's result where its score is higher, a
 * tie goes to forward).  W < 3: the bad record {0, -1, -1, 8}, strand 0, no ops, begins -1 / -1, zero statistics.  ops: room for m + W. */
int swfsc_trace_pair(const uint8_t *q, int m, const uint8_t *window, int W, int mode, const uint8_t *code,
                     const int32_t *scores, const int32_t *mapper, int msize, int open, int ext, long long fs,
                     int32_t *rec, uint8_t *strand, uint32_t *ops, int32_t *beg, int32_t *stats)
{
    if (W < 3 || m < 1) {
        rec[0] = 0; rec[1] = -1; rec[2] = -1; rec[3] = 8; *strand = 0; beg[0] = beg[1] = -1; stats[0] = stats[1] = stats[2] = 0;
        return 0;
    }
    uint8_t *T = (uint8_t *)malloc((size_t)W);
    const int first = mode == 1 ? 1 : 0;
    codon_stream(window, W, first, code, T);
    int nops = swfsc_trace_align(q, m, T, W - 2, scores, mapper, msize, open, ext, fs, rec, ops, beg, stats);
    *strand = (uint8_t)first;
    if (mode == 2) {
        int32_t r1[4], b1[2], s1[3];
        uint32_t *o1 = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(W + m));
        codon_stream(window, W, 1, code, T);
        const int n1 = swfsc_trace_align(q, m, T, W - 2, scores, mapper, msize, open, ext, fs, r1, o1, b1, s1);
        if (r1[0] > rec[0]) {
            memcpy(rec, r1, sizeof r1); memcpy(beg, b1, sizeof b1); memcpy(stats, s1, sizeof s1);
            memcpy(ops, o1, sizeof(uint32_t) * (size_t)n1); nops = n1; *strand = 1;
        }
        free(o1);
    }
    free(T);
    return nops;
}
