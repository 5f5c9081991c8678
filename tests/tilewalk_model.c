/* CPU model of the tiled (checkpoint-and-recompute) traceback of long pairs: pmx_long32_kernel<.., CK> + pmx_walkt_kernel.
 *
 * It restates exactly what the kernels keep and how the walk uses it, with the tile sizes as parameters:
 *
 *   stored by the sweep (value form of the sweep: SKEW = 1 for global / semi-global, 0 for local)
 *     row granule   (band b, column j), b < NB - 1, il = (b + 1) * BR - 1 the band's last row:
 *         H = H(il, j) - open + SKEW * (il + j + 1) * ext
 *         F = F(il + 1, j)    + SKEW * (il + 1 + j) * ext          (local: max(F, 0) -- the sweep folds the zero floor into F)
 *     column checkpoint (row i, slot s), column jc = (s + 1) * C - 1 < rlen:
 *         H = H(i, jc) - open + SKEW * (i + jc + 1) * ext
 *         E = E(i, jc)        + SKEW * (i + jc) * ext
 *   with E(i, j) = max(E(i, j - 1) - ext, H(i, j - 1) - open) and F(i, j) = max(F(i - 1, j) - ext, H(i - 1, j) - open).
 *
 *   re-derived by the walk, for tile (b, c) and entry cell (ie, je) inside it: rows b * BR .. ie, columns c * C .. je, from the
 *   granules of band b - 1 (or the first-row boundary), the checkpoint slot c - 1 (or the first-column boundary); per cell the
 *   four decisions  ND  = !(diag >= E && diag >= F)      NDL = E > F  (with ND: 1 = E, 0 = F)
 *                   EO  = H - open > E - ext             FO  = H - open > F - ext
 *   -- the oracle's strict comparisons (oracle/pmx_oracle.c), EO / FO kept at the cell the gap would open FROM.
 *
 *   carried over a tile border: the cell (i, j) and one of five states -- DIAG, INS (emit an insertion at this cell), DEL, and the
 *   two "resolve" states INSR / DELR: a gap op has been emitted and the cell it came from has to say (EO / FO) whether the gap opened
 *   there.  That cell may lie in the tile to the left / above, which is why the question travels with the state.
 *
 * Returns the number of ops (forward order, letters = X I D by include/pmx_conventions.h), or < 0.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../include/pmx_conventions.h"

#define TW_NEG (-(1 << 30))
enum { TW_NW = 0, TW_SG = 1, TW_SW = 2 };                 /* include/parasail_amd.h: PMX_MODE_* */
enum { SG_QB = 1, SG_QE = 2, SG_DB = 4, SG_DE = 8 };      /* PMX_SG_* */
enum { W_DIAG = 0, W_INS = 1, W_DEL = 2, W_INSR = 3, W_DELR = 4 };

static int imax(int a, int b) { return a > b ? a : b; }

int tilewalk_model(int mode, int sg_flags, const uint8_t *q, int ql, const uint8_t *r, int rl, int open, int ext,
                   const int32_t *matrix, int msize, const int32_t *mapper, int BR, int C,
                   int score, int end_query, int end_ref,
                   char *ops_out /* >= ql + rl + 1 */, int *beg /* 2 */, int *stats /* matches, similar, length */, long *cells /* re-derived */)
{
    const int SW = mode == TW_SW, SKEW = !SW;
    const int pen_col = mode == TW_NW || (mode == TW_SG && !(sg_flags & SG_QB));
    const int pen_row = mode == TW_NW || (mode == TW_SG && !(sg_flags & SG_DB));
    const int NB = (ql + BR - 1) / BR, NS = rl / C + 1;
#define LEFT(i) ((i) < 0 ? 0 : (pen_col ? -(open + (i) * ext) : 0))
#define TOP(j) ((j) < 0 ? 0 : (pen_row ? -(open + (j) * ext) : 0))
    int *gH = malloc(sizeof(int) * (size_t)NB * rl), *gF = malloc(sizeof(int) * (size_t)NB * rl);
    int *cH = malloc(sizeof(int) * (size_t)ql * NS), *cE = malloc(sizeof(int) * (size_t)ql * NS);
    int *Hp = malloc(sizeof(int) * (rl + 1)), *Fp = malloc(sizeof(int) * (rl + 1));
    unsigned char *nib = malloc((size_t)BR * C);
    int *tH = malloc(sizeof(int) * (C + 1)), *tF = malloc(sizeof(int) * (C + 1));
    char *rev = malloc((size_t)ql + rl + 2);
    int i, j, n = 0;
    *cells = 0;

    /* ---- the sweep, as far as it stores ---- */
    for (j = 0; j < rl; ++j) { Hp[j + 1] = TOP(j); Fp[j + 1] = TW_NEG; }
    Hp[0] = 0;
    for (i = 0; i < ql; ++i) {
        int diag = Hp[0], hl = LEFT(i), E = TW_NEG;
        Hp[0] = hl;
        for (j = 0; j < rl; ++j) {
            const int up = Hp[j + 1];
            const int F = imax(Fp[j + 1] - ext, up - open);
            int H;
            E = imax(E - ext, hl - open);
            H = imax(imax(diag + matrix[msize * mapper[q[i]] + mapper[r[j]]], E), F);
            if (SW && H < 0) H = 0;
            diag = up; Hp[j + 1] = H; Fp[j + 1] = F; hl = H;
            if ((j + 1) % C == 0) { cH[(size_t)i * NS + (j + 1) / C - 1] = H - open + SKEW * (i + j + 1) * ext; cE[(size_t)i * NS + (j + 1) / C - 1] = E + SKEW * (i + j) * ext; }
            if ((i + 1) % BR == 0 && i + 1 < ql) {
                const int Fn = imax(F - ext, H - open);
                gH[(size_t)(i / BR) * rl + j] = H - open + SKEW * (i + j + 1) * ext;
                gF[(size_t)(i / BR) * rl + j] = (SW ? imax(Fn, 0) : Fn) + SKEW * (i + 1 + j) * ext;
            }
        }
    }

    /* ---- the walk ---- */
    {
        int where = W_DIAG, rem = score, done = 0, nM = 0, nS = 0, nL = 0, k;
        i = end_query; j = end_ref;
        if (mode == TW_SG) {
            if (i + 1 == ql) for (k = rl - 1; k > j; --k) rev[n++] = PMX_CIGAR_LETTER_FOR_INS_STATE;
            else if (j + 1 == rl) for (k = ql - 1; k > i; --k) rev[n++] = PMX_CIGAR_LETTER_FOR_DEL_STATE;
        }
        while (!done) {
            if (i < 0 || j < 0) {
                if (!SW) {
                    if (i < 0 && j >= 0) { for (k = 0; k <= j; ++k) rev[n++] = PMX_CIGAR_LETTER_FOR_INS_STATE; if (pen_row) nL += j + 1; j = -1; }
                    else if (j < 0 && i >= 0) { for (k = 0; k <= i; ++k) rev[n++] = PMX_CIGAR_LETTER_FOR_DEL_STATE; if (pen_col) nL += i + 1; i = -1; }
                }
                break;
            }
            if (SW && where == W_DIAG && rem <= 0) break;
            {   /* re-derive tile (b, c) up to the entry cell */
                const int b = i / BR, c = j / C, i0 = b * BR, j0 = c * C, ie = i, je = j;
                int x, y;
                for (y = j0 - 1; y <= je; ++y) {          /* tH[y - j0 + 1] = H(i0 - 1, y), tF[..] = F(i0, y) */
                    if (i0 == 0) { tH[y - j0 + 1] = TOP(y); tF[y - j0 + 1] = TOP(y) - open; }
                    else if (y < 0) { tH[0] = LEFT(i0 - 1); tF[0] = TW_NEG; }
                    else {
                        tH[y - j0 + 1] = gH[(size_t)(b - 1) * rl + y] - SKEW * (i0 - 1 + y + 1) * ext + open;
                        tF[y - j0 + 1] = gF[(size_t)(b - 1) * rl + y] - SKEW * (i0 + y) * ext;
                    }
                }
                for (x = i0; x <= ie; ++x) {
                    int hl, E, diag = tH[0];
                    if (j0 == 0) { hl = LEFT(x); E = TW_NEG; }
                    else { hl = cH[(size_t)x * NS + c - 1] - SKEW * (x + j0) * ext + open; E = cE[(size_t)x * NS + c - 1] - SKEW * (x + j0 - 1) * ext; }
                    tH[0] = hl;
                    for (y = j0; y <= je; ++y) {
                        const int up = tH[y - j0 + 1], F = tF[y - j0 + 1];
                        int H, d, t = 0;
                        E = imax(E - ext, hl - open);
                        d = diag + matrix[msize * mapper[q[x]] + mapper[r[y]]];
                        H = imax(imax(d, E), F);
                        if (!(d >= E && d >= F)) t |= 8;
                        if (E > F) t |= 4;
                        if (SW && H < 0) H = 0;
                        if (H - open > E - ext) t |= 2;
                        if (H - open > F - ext) t |= 1;
                        nib[(size_t)(x - i0) * C + (y - j0)] = (unsigned char)t;
                        diag = up; tH[y - j0 + 1] = H; tF[y - j0 + 1] = imax(F - ext, H - open); hl = H;
                        ++*cells;
                    }
                }
                while (i >= i0 && j >= j0) {
                    const int t = nib[(size_t)(i - i0) * C + (j - j0)];
                    if (where == W_DIAG) {
                        if (SW && rem <= 0) { done = 1; break; }
                        if (t & 8) { where = (t & 4) ? W_INS : W_DEL; continue; }
                        {
                            const int a = mapper[q[i]], bb = mapper[r[j]], sc = matrix[msize * a + bb];
                            rev[n++] = a == bb ? '=' : 'X';
                            nM += a == bb; nS += sc > 0; nL += 1;
                            rem -= sc; --i; --j;
                        }
                    } else if (where == W_INS) { rev[n++] = PMX_CIGAR_LETTER_FOR_INS_STATE; nL += 1; --j; where = W_INSR; }
                    else if (where == W_DEL) { rev[n++] = PMX_CIGAR_LETTER_FOR_DEL_STATE; nL += 1; --i; where = W_DELR; }
                    else if (where == W_INSR) { if (t & 2) { where = W_DIAG; rem += open; } else { where = W_INS; rem += ext; } }
                    else { if (t & 1) { where = W_DIAG; rem += open; } else { where = W_DEL; rem += ext; } }
                }
            }
        }
        beg[0] = i + 1; beg[1] = j + 1;
        stats[0] = nM; stats[1] = nS; stats[2] = nL;
    }
    for (i = 0; i < n; ++i) ops_out[i] = rev[n - 1 - i];
    ops_out[n] = 0;
    free(gH); free(gF); free(cH); free(cE); free(Hp); free(Fp); free(nib); free(tH); free(tF); free(rev);
    return n;
}
