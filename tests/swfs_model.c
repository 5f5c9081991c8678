/* swfs_model.c -- CPU model of the frameshift-aware translated alignment (test infrastructure only), written from the contract in
 * include/parasail_amd.h ("Frameshift-aware translated search"): the codon stream of a window on either strand, the three-frame
 * recurrence over whole matrices, the record with its tie rule, and the strand fold.  Nothing here follows the kernel's layout. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG_INF (-(1LL << 60))

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

/* the complement of a base; every byte that is no base stays no base under the IUPAC complement, so it is left as it is */
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

/* out: W - 2 letters (nothing for W < 3).  Returns N. */
int swfs_codon_stream(const uint8_t *window, int W, int strand, const uint8_t *code /* 64 letters */, uint8_t *out)
{
    if (W < 3) return 0;
    uint8_t *o = (uint8_t *)malloc((size_t)W);
    for (int i = 0; i < W; ++i) o[i] = strand ? complement(window[W - 1 - i]) : window[i];
    for (int i = 0; i + 2 < W; ++i) {
        const int a = base_class(o[i]), b = base_class(o[i + 1]), c = base_class(o[i + 2]);
        out[i] = (a < 0 || b < 0 || c < 0) ? (uint8_t)'X' : code[16 * a + 4 * b + c];
    }
    free(o);
    return W - 2;
}

/* T: N letters, r: m letters; scores[q * msize + r], mapper[256].  rec: score, end_query (= i + 2, nucleotides), end_ref, flags.
 * no_shift: the two frameshift terms are left out of D. */
void swfs_model_align(const uint8_t *T, int N, const uint8_t *r, int m, const int32_t *scores, const int32_t *mapper, int msize,
                      int open, int ext, long long fs, int no_shift, int32_t *rec)
{
    long long *H = (long long *)malloc(sizeof(long long) * (size_t)N * m), *E = (long long *)malloc(sizeof(long long) * (size_t)N * m),
              *F = (long long *)malloc(sizeof(long long) * (size_t)N * m);
#define AT(M, i, j, none) (((i) < 0 || (j) < 0) ? (none) : M[(size_t)(i) * m + (j)])
    long long best = 0; int bi = 0, bj = 0;
    for (int j = 0; j < m; ++j)                         /* column-major: the first maximum in this order is the record's cell */
        for (int i = 0; i < N; ++i) {
            long long D = 0, v;
            if ((v = AT(H, i - 3, j - 1, 0)) > D) D = v;
            if (!no_shift) {
                if ((v = AT(H, i - 2, j - 1, 0) - fs) > D) D = v;
                if ((v = AT(H, i - 4, j - 1, 0) - fs) > D) D = v;
            }
            const long long M = D + scores[mapper[T[i]] * msize + mapper[r[j]]];
            long long e = AT(H, i, j - 1, 0) - open, f = AT(H, i - 3, j, 0) - open;
            if ((v = AT(E, i, j - 1, NEG_INF) - ext) > e) e = v;
            if ((v = AT(F, i - 3, j, NEG_INF) - ext) > f) f = v;
            long long h = 0;
            if (M > h) h = M;
            if (e > h) h = e;
            if (f > h) h = f;
            H[(size_t)i * m + j] = h; E[(size_t)i * m + j] = e; F[(size_t)i * m + j] = f;
            if (h > best) { best = h; bi = i; bj = j; }
        }
#undef AT
    rec[0] = (int32_t)best; rec[1] = bi + 2; rec[2] = bj; rec[3] = 0;
    free(H); free(E); free(F);
}

/* One pair on the strands of `mode` (0 forward, 1 reverse, 2 both: the reverse strand's record where its score is higher, a tie
 * goes to forward).  W < 3: the bad record {0, -1, -1, 8}, strand 0. */
void swfs_model_pair(const uint8_t *window, int W, const uint8_t *r, int m, int mode, const uint8_t *code,
                     const int32_t *scores, const int32_t *mapper, int msize, int open, int ext, long long fs,
                     int32_t *rec, uint8_t *strand)
{
    if (W < 3 || m < 1) { rec[0] = 0; rec[1] = -1; rec[2] = -1; rec[3] = 8; *strand = 0; return; }
    uint8_t *T = (uint8_t *)malloc((size_t)W);
    int32_t r1[4];
    const int first = mode == 1 ? 1 : 0;
    swfs_codon_stream(window, W, first, code, T);
    swfs_model_align(T, W - 2, r, m, scores, mapper, msize, open, ext, fs, 0, rec);
    *strand = (uint8_t)first;
    if (mode == 2) {
        swfs_codon_stream(window, W, 1, code, T);
        swfs_model_align(T, W - 2, r, m, scores, mapper, msize, open, ext, fs, 0, r1);
        if (r1[0] > rec[0]) { memcpy(rec, r1, sizeof r1); *strand = 1; }
    }
    free(T);
}
