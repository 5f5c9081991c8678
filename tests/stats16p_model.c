/* stats16p_model.c -- CPU model of the STORED arithmetic of the packed statistics kernel (test infrastructure only).
 *
 * parasail-rs_amd/csrc/pmx_stats16p.hip carries two pairs per lane slot in the 16-bit halves of 32-bit registers: H / E / F as
 * value + nb + (column + G) ext, which must stay inside [1024, 31743] (the range on which v_pk_maximum3_f16 orders bit patterns
 * like integers), and the three statistics (matches, similar, length) as plain counters that are incremented with 32-bit adds of
 * 0x00010001 -- a half that passes 65535 carries into its neighbour, one that passes 32767 has left what the host's gate
 * (max_qlen + max_rlen + 2 <= 32767) promises.  No promotion pass exists behind the kernel: the host (pmx_nwsgv_bias in its form
 * without a row offset, and that gate) must PROVE both from lengths and scoring alone.  This file replays one lane slot -- G lanes,
 * R rows per lane, both halves -- lane for lane and step for step the way pmx_stats16p_kernel does: the query top-aligned, the G - 1
 * virtual columns in front of the reference (a penalised one scores -open and still counts a length), the closed-form row above
 * lane 0, every select as a v_bfi_b32 on a packed sign mask, every add and subtract on the whole 32-bit word, the captures and the
 * combine with its clamped key.  It counts
 *   * every operand of a max3 outside [1024, 31743]: at cells that can reach a captured cell (row < qlen, column < rlen, the virtual
 *     columns included) in `violations`; at the other cells of a row that one of the two queries reaches (the rows below the shorter
 *     query, the pad columns behind a reference) in `pad_violations` -- nothing reads them, but a carry or borrow of theirs would land
 *     in the other half; in the rows below BOTH queries in `dead_violations`: the shape's rows beyond the batch's longest query, which
 *     the proof does not cover (it knows max_qlen, not G * R), which no row above ever reads, and whose carries land in dead cells;
 *   * every statistics half above 32767 at a cell that can reach a captured cell, and every counter add whose low half carries into
 *     the high half (or whose high half carries out) while one of the two halves can: `stat_violations`.
 * tests/test_stats_window_model.py drives it: the six fields of both halves must equal the oracle's, and nothing may be counted
 * whenever the host admits the batch.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int score[2], end_query[2], end_ref[2], matches[2], similar[2], length[2];
    int lo, hi;                 /* extreme max3 operands at cells that can reach a captured cell */
    int violations;             /* such operands outside [1024, 31743], profile bytes outside [0, 255] */
    int pad_violations;         /* max3 operands outside the window at cells that cannot reach a captured cell */
    int pad_lo, pad_hi;         /* extreme max3 operands at those cells */
    int dead_violations;        /* max3 operands outside the window in rows below both queries (harmless: see above) */
    int stat_hi;                /* the largest statistics half at a cell that can reach a captured cell */
    int stat_violations;        /* halves above 32767 there, and carries or borrows between the halves (counters and values) */
    int clamp_hits;             /* halves whose best last-column candidate lies below the combine key's clamp (-16000) */
    int first_violation_kind;   /* 1 max3 operand, 2 profile byte, 3 statistics half, 4 carry or borrow between the halves */
} stats16p_model_out;

#define WLO 1024
#define WHI 31743

typedef struct { int H, i, jL, MS; } cand_t;

typedef struct {
    stats16p_model_out *o;
    int live[2];                /* the cell in hand can reach a captured cell, per half */
    int dead;                   /* the cell in hand lies below both queries */
} ctx_t;

static uint32_t pack2(int a, int b) { return ((uint32_t)a & 0xFFFFu) | ((uint32_t)b << 16); }
static int half_of(uint32_t v, int h) { return h ? (int)(v >> 16) : (int)(v & 0xFFFFu); }
static int join(int lo, int hi) { return (int)((uint32_t)lo | ((uint32_t)hi << 16)); }
static uint32_t bfi(uint32_t m, uint32_t a, uint32_t b) { return (m & a) | (~m & b); }

/* v_pk_sub_i16, v_pk_ashrrev_i16 by 15: 0xFFFF where a < b (differences below 32768), per half */
static uint32_t pk_lt(uint32_t a, uint32_t b)
{
    const uint32_t lo = (((a & 0xFFFFu) - (b & 0xFFFFu)) & 0x8000u) ? 0xFFFFu : 0u;
    const uint32_t hi = ((((a >> 16) - (b >> 16)) & 0x8000u) ? 0xFFFFu : 0u) << 16;
    return lo | hi;
}

static void flag(ctx_t *c, int kind, int pad)
{
    if (pad) { if (c->dead) c->o->dead_violations++; else c->o->pad_violations++; return; }
    if (!c->o->violations && !c->o->stat_violations) c->o->first_violation_kind = kind;
    if (kind <= 2) c->o->violations++; else c->o->stat_violations++;
}

/* v_pk_maximum3_f16: the integer max3 of the halves while every operand is inside the window */
static uint32_t max3(ctx_t *c, uint32_t a, uint32_t b, uint32_t d)
{
    uint32_t r = 0;
    for (int h = 0; h < 2; ++h) {
        const int v[3] = {half_of(a, h), half_of(b, h), half_of(d, h)};
        int m = -(1 << 30);
        for (int x = 0; x < 3; ++x) {
            if (c->live[h]) { if (v[x] < c->o->lo) c->o->lo = v[x]; if (v[x] > c->o->hi) c->o->hi = v[x]; }
            else if (!c->dead) { if (v[x] < c->o->pad_lo) c->o->pad_lo = v[x]; if (v[x] > c->o->pad_hi) c->o->pad_hi = v[x]; }
            if (v[x] < WLO || v[x] > WHI) flag(c, 1, !c->live[h]);
            const int s = (int)(int16_t)v[x];                      /* (outside the window: ordered as int16, and counted) */
            if (s > m) m = s;
        }
        r |= ((uint32_t)m & 0xFFFFu) << (16 * h);
    }
    return r;
}

/* a 32-bit add of two packed counters: the carry out of either half is counted where it can do harm */
static uint32_t addc(ctx_t *c, uint32_t a, uint32_t b)
{
    if ((a & 0xFFFFu) + (b & 0xFFFFu) > 0xFFFFu && (c->live[0] || c->live[1])) flag(c, 4, 0);
    if ((uint64_t)a + b > 0xFFFFFFFFull && c->live[1]) flag(c, 4, 0);
    return a + b;
}

/* the 32-bit add / subtract of packed values: a carry or borrow out of the low half lands in the other pair's value */
static uint32_t vadd(ctx_t *c, uint32_t a, uint32_t b)
{
    if ((a & 0xFFFFu) + (b & 0xFFFFu) > 0xFFFFu && (c->live[0] || c->live[1])) flag(c, 4, 0);
    return a + b;
}
static uint32_t vsub(ctx_t *c, uint32_t a, uint32_t b)
{
    if ((a & 0xFFFFu) < (b & 0xFFFFu) && (c->live[0] || c->live[1])) flag(c, 4, 0);
    return a - b;
}

/* a statistics word that was just written at the cell in hand */
static void stat(ctx_t *c, uint32_t v)
{
    for (int h = 0; h < 2; ++h) {
        if (!c->live[h]) continue;
        const int x = half_of(v, h);
        if (x > c->o->stat_hi) c->o->stat_hi = x;
        if (x > 32767) flag(c, 3, 0);
    }
}

/* q*, r*: mapped symbols (0 .. msize-1) of the pair in the low (A) and in the high (B) half.  ml: the matrix-lookup form (the match
 * increment is a packed comparison of letter codes, the similar increment the sign of open - score byte).  max_rlen: the longest
 * reference of the wave (>= rlA, rlB): the sweep runs (max_rlen + G) & ~1 steps.  Returns 0, or -1 on bad arguments. */
int stats16p_model(int G, int R, int ml,
                   const unsigned char *qA, int qlA, const unsigned char *rA, int rlA,
                   const unsigned char *qB, int qlB, const unsigned char *rB, int rlB, int max_rlen,
                   const int *mat, int msize, int open, int ext, int col_pen, int row_pen, int s1_end, int s2_end, int nb,
                   stats16p_model_out *out)
{
    const int QP = G * R;
    if (G < 1 || R < 1 || qlA < 1 || qlA > QP || qlB < 1 || qlB > QP || rlA < 1 || rlB < 1 || rlA > max_rlen || rlB > max_rlen) return -1;
    memset(out, 0, sizeof *out);
    out->lo = out->pad_lo = 1 << 30; out->hi = out->pad_hi = -(1 << 30);
    ctx_t cx = {out, {0, 0}, 0}, *c = &cx;
    const unsigned char *qq[2] = {qA, qB}, *rr[2] = {rA, rB};
    const int ql[2] = {qlA, qlB}, rl[2] = {rlA, rlB};
    const int vcol_b = col_pen ? 0 : open;

    /* score bytes [h][sym][row], sym == msize: the pad symbol */
    unsigned char *sc[2];
    for (int h = 0; h < 2; ++h) {
        sc[h] = (unsigned char *)malloc((size_t)(msize + 1) * QP);
        for (int sym = 0; sym <= msize; ++sym)
            for (int i = 0; i < QP; ++i) {
                const int v = i < ql[h] ? (sym < msize ? mat[qq[h][i] * msize + sym] + open : vcol_b) : open;
                if (v < 0 || v > 255) { c->live[0] = c->live[1] = 1; flag(c, 2, 0); }
                sc[h][(size_t)sym * QP + i] = (unsigned char)v;
            }
    }

    const uint32_t one2 = 0x00010001u;
    const uint32_t vExt = pack2(ext, ext), vC = pack2(open - ext, open - ext), vOpenP = pack2(open, open);
    uint32_t *X = malloc(sizeof(uint32_t) * QP), *E = malloc(sizeof(uint32_t) * QP);
    uint32_t *hM = malloc(sizeof(uint32_t) * QP), *hS = malloc(sizeof(uint32_t) * QP), *hL = malloc(sizeof(uint32_t) * QP);
    uint32_t *eM = malloc(sizeof(uint32_t) * QP), *eS = malloc(sizeof(uint32_t) * QP), *eL = malloc(sizeof(uint32_t) * QP);
    /* per lane: what it hands down (out), what it was handed (in), its diagonal */
    uint32_t *lane = malloc(sizeof(uint32_t) * G * 20);
    uint32_t *Hout = lane, *HMout = lane + G, *HSout = lane + 2 * G, *HLout = lane + 3 * G;
    uint32_t *Fout = lane + 4 * G, *FMout = lane + 5 * G, *FSout = lane + 6 * G, *FLout = lane + 7 * G;
    uint32_t *diag0 = lane + 8 * G, *dM0 = lane + 9 * G, *dS0 = lane + 10 * G, *dL0 = lane + 11 * G;
    uint32_t *Hin = lane + 12 * G, *HMin = lane + 13 * G, *HSin = lane + 14 * G, *HLin = lane + 15 * G;
    uint32_t *Fin = lane + 16 * G, *FMin = lane + 17 * G, *FSin = lane + 18 * G, *FLin = lane + 19 * G;
    cand_t *corner = malloc(sizeof(cand_t) * 2 * G), *brow = malloc(sizeof(cand_t) * 2 * G), *bcol = malloc(sizeof(cand_t) * 2 * G);
    uint32_t *T = malloc(sizeof(uint32_t) * R * 4), *TM = T + R, *TS = T + 2 * R, *TL = T + 3 * R;

    for (int g = 0; g < G; ++g) {
        const int base = nb + (G - g) * ext - open;
        for (int k = 0; k < R; ++k) {
            const int i = g * R + k;
            const int ht = col_pen ? -(open + i * ext) : 0, lt = col_pen ? i + 1 : 0;
            X[i] = pack2(base + ht, base + ht); E[i] = X[i];
            hM[i] = hS[i] = 0; hL[i] = pack2(lt, lt);
            eM[i] = eS[i] = 0; eL[i] = pack2(lt + 1, lt + 1);
        }
        Hout[g] = X[g * R + R - 1]; HMout[g] = HSout[g] = 0; HLout[g] = hL[g * R + R - 1];
        {
            const int i = (g + 1) * R;
            const int ft = col_pen ? -(open + i * ext) : -open;
            Fout[g] = pack2(base + open + ft, base + open + ft);
            FMout[g] = FSout[g] = 0;
            FLout[g] = col_pen ? pack2(i + 1, i + 1) : one2;
        }
        dM0[g] = dS0[g] = 0;
        if (g == 0) { diag0[g] = pack2(base, base); dL0[g] = 0; }
        else {
            const int i = g * R - 1;
            const int ht = col_pen ? -(open + i * ext) : 0;
            diag0[g] = pack2(base + ht, base + ht); dL0[g] = col_pen ? pack2(i + 1, i + 1) : 0;
        }
        for (int h = 0; h < 2; ++h) {
            cand_t z = {-(1 << 30), 0, 0, 0};
            corner[2 * g + h] = brow[2 * g + h] = bcol[2 * g + h] = z;
        }
    }
    uint32_t topX = row_pen ? pack2(nb + (G + 1) * ext - 2 * open, nb + (G + 1) * ext - 2 * open)
                            : pack2(nb + (G + 1) * ext - open, nb + (G + 1) * ext - open);
    const uint32_t topStep = row_pen ? 0 : vExt;
    uint32_t topL = row_pen ? one2 : 0;
    const uint32_t topLStep = row_pen ? one2 : 0;
    const int gL[2] = {(qlA - 1) / R, (qlB - 1) / R}, kL[2] = {(qlA - 1) % R, (qlB - 1) % R};

    const int T_ = (max_rlen + G - 1 + 1) & ~1;
    for (int t = 0; t < T_; ++t) {
        /* the hand-offs of the step: every lane reads what the lane above left after the step before */
        for (int g = 0; g < G; ++g) {
            if (g == 0) {
                c->live[0] = t < rlA; c->live[1] = t < rlB; c->dead = 0;
                Hin[g] = topX; HMin[g] = 0; HSin[g] = 0; HLin[g] = topL;
                Fin[g] = topX; FMin[g] = 0; FSin[g] = 0; FLin[g] = addc(c, topL, one2);
            } else {
                Hin[g] = Hout[g - 1]; HMin[g] = HMout[g - 1]; HSin[g] = HSout[g - 1]; HLin[g] = HLout[g - 1];
                Fin[g] = Fout[g - 1]; FMin[g] = FMout[g - 1]; FSin[g] = FSout[g - 1]; FLin[g] = FLout[g - 1];
            }
        }
        for (int g = 0; g < G; ++g) {
            const int jcol = t - g;
            const uint32_t linc = jcol < 0 ? (col_pen ? one2 : 0) : ((jcol < rlA ? 1u : 0u) | (jcol < rlB ? 0x10000u : 0u));
            int sym[2];
            for (int h = 0; h < 2; ++h) sym[h] = (jcol >= 0 && jcol < rl[h]) ? rr[h][jcol] : msize;
            uint32_t F = Fin[g], fM = FMin[g], fS = FSin[g], fL = FLin[g];
            for (int k = 0; k < R; ++k) {
                const int i = g * R + k;
                c->live[0] = i < qlA && jcol < rlA; c->live[1] = i < qlB && jcol < rlB; c->dead = i >= qlA && i >= qlB;
                const uint32_t s = (uint32_t)sc[0][(size_t)sym[0] * QP + i] | ((uint32_t)sc[1][(size_t)sym[1] * QP + i] << 16);
                uint32_t im = 0, is = 0;
                if (ml) {
                    const int qc[2] = {i < qlA ? qA[i] : msize, i < qlB ? qB[i] : msize};
                    for (int h = 0; h < 2; ++h) {
                        is |= ((((uint32_t)half_of(vOpenP, h) - (uint32_t)half_of(s, h)) & 0xFFFFu) >> 15) << (16 * h);
                        im |= (((((uint32_t)qc[h] ^ (uint32_t)sym[h]) - 1u) & 0xFFFFu) >> 15) << (16 * h);
                    }
                } else {
                    for (int h = 0; h < 2; ++h) {
                        const int real = i < ql[h] && sym[h] < msize;
                        im |= (uint32_t)(real && qq[h][i] == sym[h]) << (16 * h);
                        is |= (uint32_t)(real && mat[qq[h][i] * msize + sym[h]] > 0) << (16 * h);
                    }
                }
                T[k] = vadd(c, k == 0 ? diag0[g] : X[i - 1], s);
                TM[k] = addc(c, k == 0 ? dM0[g] : hM[i - 1], im);
                TS[k] = addc(c, k == 0 ? dS0[g] : hS[i - 1], is);
                TL[k] = addc(c, k == 0 ? dL0[g] : hL[i - 1], linc);
            }
            /* (the kernel computes every T of the step before the first H: X[i - 1] above is the column before's) */
            for (int k = 0; k < R; ++k) {
                const int i = g * R + k;
                c->live[0] = i < qlA && jcol < rlA; c->live[1] = i < qlB && jcol < rlB; c->dead = i >= qlA && i >= qlB;
                const uint32_t Fe = vsub(c, F, vExt);
                const uint32_t H = max3(c, T[k], E[i], Fe);
                const uint32_t Xn = vsub(c, H, vC);
                const uint32_t mNDL = pk_lt(Fe, H);
                const uint32_t xM = bfi(mNDL, eM[i], fM), xS = bfi(mNDL, eS[i], fS), xL = bfi(mNDL, eL[i], fL);
                const uint32_t mND = pk_lt(T[k], H);
                const uint32_t nM = bfi(mND, xM, TM[k]), nS = bfi(mND, xS, TS[k]), nL = bfi(mND, xL, TL[k]);
                const uint32_t mEO = pk_lt(E[i], Xn);
                eM[i] = bfi(mEO, nM, eM[i]); eS[i] = bfi(mEO, nS, eS[i]); eL[i] = addc(c, bfi(mEO, nL, eL[i]), one2);
                const uint32_t mFO = pk_lt(Fe, Xn);
                fM = bfi(mFO, nM, fM); fS = bfi(mFO, nS, fS); fL = addc(c, bfi(mFO, nL, fL), one2);
                E[i] = max3(c, E[i], Xn, Xn);
                F = max3(c, Fe, Xn, Xn);
                T[k] = Xn;                                         /* (X[i] is still the diagonal of row i + 1: written below) */
                hM[i] = nM; hS[i] = nS; hL[i] = nL;
                stat(c, nM); stat(c, nS); stat(c, nL); stat(c, eL[i]); stat(c, fL);
            }
            for (int k = 0; k < R; ++k) X[g * R + k] = T[k];
            diag0[g] = Hin[g]; dM0[g] = HMin[g]; dS0[g] = HSin[g]; dL0[g] = HLin[g];
            Hout[g] = X[g * R + R - 1]; HMout[g] = hM[g * R + R - 1]; HSout[g] = hS[g * R + R - 1]; HLout[g] = hL[g * R + R - 1];
            Fout[g] = F; FMout[g] = fM; FSout[g] = fS; FLout[g] = fL;

            /* captures */
            const int unsk = nb + (jcol + G) * ext - open + ext;
            for (int h = 0; h < 2; ++h) {
                if (!(jcol >= 0 && jcol < rl[h])) continue;
                if (g == gL[h] && (s2_end || jcol == rl[h] - 1)) {
                    const int i = g * R + kL[h];
                    cand_t cd = {half_of(X[i], h) - unsk, ql[h] - 1, join(jcol, half_of(hL[i], h)), join(half_of(hM[i], h), half_of(hS[i], h))};
                    if (jcol == rl[h] - 1) corner[2 * g + h] = cd;
                    if (s2_end && cd.H > brow[2 * g + h].H) brow[2 * g + h] = cd;
                }
                if (s1_end && jcol == rl[h] - 1) {
                    for (int k = 0; k < R; ++k) {
                        const int i = g * R + k, hv = half_of(X[i], h) - unsk;
                        if (i < ql[h] && hv > bcol[2 * g + h].H) {
                            cand_t cd = {hv, i, join(jcol, half_of(hL[i], h)), join(half_of(hM[i], h), half_of(hS[i], h))};
                            bcol[2 * g + h] = cd;
                        }
                    }
                }
            }
        }
        topX += topStep;
        c->live[0] = t + 1 < rlA; c->live[1] = t + 1 < rlB; c->dead = 0;
        topL = addc(c, topL, topLStep);
    }

    /* combine per half: last-column candidates over the slot (value descending, row ascending), then the oracle's rule */
    for (int h = 0; h < 2; ++h) {
        uint32_t best = 0;
        int top = -(1 << 30);
        for (int g = 0; g < G; ++g) {
            const cand_t *b = &bcol[2 * g + h];
            const uint32_t key = ((uint32_t)(b->H < -16000 ? 0 : b->H + 16384) << 16) | (0xFFFFu - (uint32_t)b->i);
            if (key > best) best = key;
            if (b->H > top) top = b->H;
        }
        if (s1_end && top < -16000) out->clamp_hits++;
        int wl = 0, found = 0;
        for (int g = 0; g < G && !found; ++g) {
            const cand_t *b = &bcol[2 * g + h];
            const uint32_t key = ((uint32_t)(b->H < -16000 ? 0 : b->H + 16384) << 16) | (0xFFFFu - (uint32_t)b->i);
            if (key == best && b->H > -(1 << 29)) { wl = g; found = 1; }
        }
        const cand_t bc = bcol[2 * wl + h], co = corner[2 * gL[h] + h], br = brow[2 * gL[h] + h];
        cand_t res;
        if (!s1_end && !s2_end) res = co;
        else {
            const cand_t z = {-(1 << 30), 0, 0, 0};
            res = z;
            if (s2_end) res = br;
            if (s1_end && bc.H > res.H) res = bc;
        }
        out->score[h] = res.H; out->end_query[h] = res.i; out->end_ref[h] = res.jL & 0xFFFF;
        out->matches[h] = res.MS & 0xFFFF; out->similar[h] = (int)((uint32_t)res.MS >> 16); out->length[h] = (int)((uint32_t)res.jL >> 16);
    }
    free(sc[0]); free(sc[1]); free(X); free(E); free(hM); free(hS); free(hL); free(eM); free(eS); free(eL);
    free(lane); free(corner); free(brow); free(bcol); free(T);
    return 0;
}
