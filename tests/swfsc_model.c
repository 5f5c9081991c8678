/* swfsc_model.c -- CPU model of the reference-side frameshift-aware alignment (test infrastructure only), written from the contract
 * in include/parasail_amd.h ("Frameshift-aware translated search, reference side"): the codon stream of a reference window on either
 * strand, the recurrence over whole matrices with the protein on the rows and the stream on the columns, the record with its tie
 * rule, the strand fold and the bad-pair rule.  Nothing here follows the kernel's layout. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MINUS_INF (-(1LL << 60))

/* 0 .. 3 in the order of the genetic code's index (T C A G, U as T, either case); -1: no base */
static int code_digit(uint8_t b)
{
    static const char order[] = "TCAG";
    if (b >= 'a' && b <= 'z') b = (uint8_t)(b - 'a' + 'A');
    if (b == 'U') b = 'T';
    for (int d = 0; d < 4; ++d) if (b == (uint8_t)order[d]) return d;
    return -1;
}

/* the oriented window: as stored, or from the window's end downwards with every base complemented (case kept, U -> A; any other
 * byte stays what it is and is no base either way) */
static void orient(const uint8_t *window, int W, int strand, uint8_t *o)
{
    for (int x = 0; x < W; ++x) {
        if (!strand) { o[x] = window[x]; continue; }
        const uint8_t b = window[W - 1 - x];
        const int lower = b >= 'a' && b <= 'z';
        const uint8_t up = lower ? (uint8_t)(b - 'a' + 'A') : b;
        uint8_t c = up;
        if (up == 'A') c = 'T'; else if (up == 'T' || up == 'U') c = 'A'; else if (up == 'C') c = 'G'; else if (up == 'G') c = 'C';
        o[x] = lower && c != up ? (uint8_t)(c - 'A' + 'a') : (c != up ? c : b);
    }
}

/* T[j] = the translation of oriented bytes j, j + 1, j + 2.  out: W - 2 letters; returns N (0 for W < 3). */
int swfsc_stream(const uint8_t *window, int W, int strand, const uint8_t *code /* 64 letters */, uint8_t *out)
{
    if (W < 3) return 0;
    uint8_t *o = (uint8_t *)malloc((size_t)W);
    orient(window, W, strand, o);
    for (int j = 0; j + 2 < W; ++j) {
        const int a = code_digit(o[j]), b = code_digit(o[j + 1]), c = code_digit(o[j + 2]);
        out[j] = (a < 0 || b < 0 || c < 0) ? (uint8_t)'X' : code[16 * a + 4 * b + c];
    }
    free(o);
    return W - 2;
}

/* q: m letters (rows), T: N letters (columns); scores[query letter * msize + reference letter], mapper[256].
 * rec: score, end_query (= i, letters), end_ref (= j + 2, nucleotides), flags.  no_shift: D has no frameshift terms. */
void swfsc_align(const uint8_t *q, int m, const uint8_t *T, int N, const int32_t *scores, const int32_t *mapper, int msize,
                 long long open, long long ext, long long fs, int no_shift, int32_t *rec)
{
    const size_t cells = (size_t)m * (size_t)N;
    long long *H = (long long *)malloc(sizeof(long long) * cells), *E = (long long *)malloc(sizeof(long long) * cells),
              *F = (long long *)malloc(sizeof(long long) * cells);
#define CELL(A, i, j, none) (((i) < 0 || (j) < 0) ? (none) : A[(size_t)(j) * m + (i)])
    long long top = 0; int ti = 0, tj = 0;
    for (int j = 0; j < N; ++j)                          /* columns first, rows within: the order of the tie rule */
        for (int i = 0; i < m; ++i) {
            long long d = 0, v;
            v = CELL(H, i - 1, j - 3, 0); if (v > d) d = v;
            if (!no_shift) {
                v = CELL(H, i - 1, j - 2, 0) - fs; if (v > d) d = v;
                v = CELL(H, i - 1, j - 4, 0) - fs; if (v > d) d = v;
            }
            const long long mm = d + scores[(size_t)mapper[q[i]] * msize + mapper[T[j]]];
            long long e = CELL(H, i, j - 3, 0) - open; v = CELL(E, i, j - 3, MINUS_INF) - ext; if (v > e) e = v;
            long long f = CELL(H, i - 1, j, 0) - open; v = CELL(F, i - 1, j, MINUS_INF) - ext; if (v > f) f = v;
            long long h = 0;
            if (mm > h) h = mm;
            if (e > h) h = e;
            if (f > h) h = f;
            H[(size_t)j * m + i] = h; E[(size_t)j * m + i] = e; F[(size_t)j * m + i] = f;
            if (h > top) { top = h; ti = i; tj = j; }
        }
#undef CELL
    rec[0] = (int32_t)top; rec[1] = ti; rec[2] = tj + 2; rec[3] = 0;
    free(H); free(E); free(F);
}

/* One pair on the reference's strands of `mode` (0 forward, 1 reverse, 2 both: the reverse strand's record only where its score is
 * higher).  W < 3 (or no query): the bad record {0, -1, -1, 8}, strand 0. */
void swfsc_pair(const uint8_t *q, int m, const uint8_t *window, int W, int mode, const uint8_t *code,
                const int32_t *scores, const int32_t *mapper, int msize, long long open, long long ext, long long fs, int no_shift,
                int32_t *rec, uint8_t *strand)
{
    if (W < 3 || m < 1) { rec[0] = 0; rec[1] = -1; rec[2] = -1; rec[3] = 8; *strand = 0; return; }
    uint8_t *T = (uint8_t *)malloc((size_t)W);
    const int first = mode == 1 ? 1 : 0;
    swfsc_stream(window, W, first, code, T);
    swfsc_align(q, m, T, W - 2, scores, mapper, msize, open, ext, fs, no_shift, rec);
    *strand = (uint8_t)first;
    if (mode == 2) {
        int32_t other[4];
        swfsc_stream(window, W, 1, code, T);
        swfsc_align(q, m, T, W - 2, scores, mapper, msize, open, ext, fs, no_shift, other);
        if (other[0] > rec[0]) { memcpy(rec, other, sizeof other); *strand = 1; }
    }
    free(T);
}
