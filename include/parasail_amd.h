/*
 * parasail_amd.h -- C ABI of libparasail_amd.so, the MI355X (gfx950) engine behind the
 * parasail-rs `Aligner::align()` hot path.
 *
 * Two groups of entry points:
 *
 *  (1) The `parasail_*` symbols that parasail-rs binds through libparasail-sys
 *      (reference file:line given per declaration).  Same names, same argument order and
 *      meaning, same ownership and error convention (NULL = failure; alignment functions
 *      never return NULL), so the Rust L2 layer links against this library unchanged
 *      (INTEGRATION.md).  Every alignment call runs its DP fill on the GPU; there is no
 *      CPU fallback -- if no HIP device is usable the call aborts with a message on stderr.
 *
 *  (2) Additive `pmx_*` batch entry points (no reference counterpart: the reference is
 *      one pair per call, src/aligner/mod.rs:397).  They take many pairs in packed
 *      buffers and are what BASELINE.json's throughput configs are measured on.
 *
 * Plain C types only; no torch / HIP types in any signature (streams are passed as void*).
 */
#ifndef PARASAIL_AMD_H
#define PARASAIL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ types ---- */

/* Layout read directly by Rust: .type_ (src/matrix/mod.rs:193), .size (:228,:257),
 * .length (:256), .matrix (:258).  [EXTERNAL] field order follows upstream parasail.h. */
typedef struct parasail_matrix {
    const char *name;
    const int *matrix;      /* length x size, row-major */
    const int *mapper;      /* 256 entries: byte -> column index */
    int size;               /* alphabet size incl. the wildcard column */
    int max;
    int min;
    int *user_matrix;       /* non-NULL for matrices owned by the caller (set_value allowed) */
    int type;               /* 0 = square, 1 = PSSM */
    int length;             /* rows: == size for square, query length for PSSM */
    const char *alphabet;
    const char *query;      /* PSSM only */
} parasail_matrix_t;

#define PARASAIL_MATRIX_TYPE_SQUARE 0
#define PARASAIL_MATRIX_TYPE_PSSM   1

/* Opaque to Rust (only passed back): src/alignment/mod.rs:55-60, src/profile/mod.rs:281-285 */
typedef struct parasail_result parasail_result_t;
typedef struct parasail_profile parasail_profile_t;
typedef parasail_profile_t parasail_profile;   /* bindgen alias used at src/profile/mod.rs:115 */
typedef parasail_matrix_t parasail_matrix;

/* src/alignment/mod.rs:368-374 reads .query/.comp/.ref_; each is a malloc'd C string that
 * Rust adopts with CString::from_raw. */
typedef struct parasail_traceback {
    char *query;
    char *comp;
    char *ref;
} parasail_traceback_t;

typedef struct parasail_cigar {
    uint32_t *seq;          /* BAM encoding: len << 4 | op, op index into "MIDNSHP=X" */
    int len;
    int beg_query;
    int beg_ref;
} parasail_cigar_t;

/* src/alignment/mod.rs:513-543 */
typedef struct parasail_result_ssw {
    uint16_t score1;
    int32_t ref_begin1;
    int32_t ref_end1;
    int32_t read_begin1;
    int32_t read_end1;
    uint32_t *cigar;
    int32_t cigarLen;
} parasail_result_ssw_t;

/* trace-table flag values: src/alignment/table.rs:127-142 */
#define PARASAIL_ZERO_MASK 120
#define PARASAIL_E_MASK    103
#define PARASAIL_F_MASK     31
#define PARASAIL_ZERO   0
#define PARASAIL_INS    1
#define PARASAIL_DEL    2
#define PARASAIL_DIAG   4
#define PARASAIL_DIAG_E 8
#define PARASAIL_INS_E  16
#define PARASAIL_DIAG_F 32
#define PARASAIL_DEL_F  64

typedef parasail_result_t *parasail_function_t(const char *s1, const int s1Len,
                                               const char *s2, const int s2Len,
                                               const int open, const int gap,
                                               const parasail_matrix_t *matrix);
typedef parasail_result_t *parasail_pfunction_t(const parasail_profile_t *profile,
                                                const char *s2, const int s2Len,
                                                const int open, const int gap);
typedef parasail_profile_t *parasail_pcreator_t(const char *s1, const int s1Len,
                                                const parasail_matrix_t *matrix);

/* --------------------------------------------------------------- dispatch ---- */
/* src/aligner/mod.rs:345 / :349 -- name grammar src/aligner/mod.rs:319-329:
 *   {nw|sg[_q{b,e,x}][_d{b,e,x}]|sw}[_trace][_stats][_table|_rowcol]_{striped|scan|diag}[_profile]_{sat|8|16|32|64}
 * A name with or without the leading "parasail_" is accepted.  Unknown name -> NULL. */
parasail_function_t  *parasail_lookup_function(const char *funcname);
parasail_pfunction_t *parasail_lookup_pfunction(const char *funcname);

/* src/aligner/mod.rs:470-481 */
parasail_result_t *parasail_nw_banded(const char *s1, const int s1Len, const char *s2, const int s2Len,
                                      const int open, const int gap, const int k,
                                      const parasail_matrix_t *matrix);
/* src/aligner/mod.rs:500-510, src/profile/mod.rs:345 */
parasail_result_ssw_t *parasail_ssw(const char *s1, const int s1Len, const char *s2, const int s2Len,
                                    const int open, const int gap, const parasail_matrix_t *matrix);
parasail_profile_t *parasail_ssw_init(const char *s1, const int s1Len,
                                      const parasail_matrix_t *matrix, const int8_t score_size);
void parasail_result_ssw_free(parasail_result_ssw_t *result);

/* ------------------------------------------------------------------ result --- */
/* src/alignment/mod.rs:64-98 */
int parasail_result_get_score(const parasail_result_t *result);
int parasail_result_get_end_query(const parasail_result_t *result);
int parasail_result_get_end_ref(const parasail_result_t *result);
int parasail_result_get_matches(const parasail_result_t *result);
int parasail_result_get_similar(const parasail_result_t *result);
int parasail_result_get_length(const parasail_result_t *result);
/* src/alignment/mod.rs:123-192: [query_len][ref_len] int32 row-major, valid until result_free */
int *parasail_result_get_score_table(const parasail_result_t *result);
int *parasail_result_get_matches_table(const parasail_result_t *result);
int *parasail_result_get_similar_table(const parasail_result_t *result);
int *parasail_result_get_length_table(const parasail_result_t *result);
/* src/alignment/mod.rs:195-288: rows have ref_len entries, cols have query_len entries */
int *parasail_result_get_score_row(const parasail_result_t *result);
int *parasail_result_get_matches_row(const parasail_result_t *result);
int *parasail_result_get_similar_row(const parasail_result_t *result);
int *parasail_result_get_length_row(const parasail_result_t *result);
int *parasail_result_get_score_col(const parasail_result_t *result);
int *parasail_result_get_matches_col(const parasail_result_t *result);
int *parasail_result_get_similar_col(const parasail_result_t *result);
int *parasail_result_get_length_col(const parasail_result_t *result);
/* src/alignment/mod.rs:291-307: [query_len][ref_len] one byte per cell */
int *parasail_result_get_trace_table(const parasail_result_t *result);
/* src/alignment/mod.rs:356-366, :400-410, :324-339 */
parasail_traceback_t *parasail_result_get_traceback(parasail_result_t *result,
        const char *seqA, int lena, const char *seqB, int lenb,
        const parasail_matrix_t *matrix, char match, char pos, char neg);
void parasail_traceback_free(parasail_traceback_t *traceback);
void parasail_traceback_generic(const char *seqA, int lena, const char *seqB, int lenb,
        const char *nameA, const char *nameB, const parasail_matrix_t *matrix,
        parasail_result_t *result, char match, char pos, char neg,
        int width, int name_width, int use_stats);
parasail_cigar_t *parasail_result_get_cigar(parasail_result_t *result,
        const char *seqA, int lena, const char *seqB, int lenb, const parasail_matrix_t *matrix);
char *parasail_cigar_decode(parasail_cigar_t *cigar);      /* malloc'd, caller frees */
void parasail_cigar_free(parasail_cigar_t *cigar);
/* src/alignment/mod.rs:422-494 */
int parasail_result_is_nw(const parasail_result_t *result);
int parasail_result_is_sg(const parasail_result_t *result);
int parasail_result_is_sw(const parasail_result_t *result);
int parasail_result_is_saturated(const parasail_result_t *result);
int parasail_result_is_banded(const parasail_result_t *result);
int parasail_result_is_scan(const parasail_result_t *result);
int parasail_result_is_striped(const parasail_result_t *result);
int parasail_result_is_diag(const parasail_result_t *result);
int parasail_result_is_blocked(const parasail_result_t *result);
int parasail_result_is_stats(const parasail_result_t *result);
int parasail_result_is_stats_table(const parasail_result_t *result);
int parasail_result_is_table(const parasail_result_t *result);
int parasail_result_is_rowcol(const parasail_result_t *result);
int parasail_result_is_stats_rowcol(const parasail_result_t *result);
int parasail_result_is_trace(const parasail_result_t *result);
/* src/alignment/mod.rs:498-504 */
void parasail_result_free(parasail_result_t *result);

/* ------------------------------------------------------------------ matrix --- */
/* src/matrix/mod.rs:40, :62, :140, :158, :188-197, :238, :281, :304 */
parasail_matrix_t *parasail_matrix_create(const char *alphabet, const int match, const int mismatch);
const parasail_matrix_t *parasail_matrix_lookup(const char *matrixname);
parasail_matrix_t *parasail_matrix_from_file(const char *filename);
parasail_matrix_t *parasail_matrix_pssm_create(const char *alphabet, const int *values, const int length);
parasail_matrix_t *parasail_matrix_convert_square_to_pssm(const parasail_matrix_t *matrix,
                                                          const char *s1, int s1Len);
parasail_matrix_t *parasail_matrix_copy(const parasail_matrix_t *matrix);
void parasail_matrix_set_value(parasail_matrix_t *matrix, int row, int col, int value);
void parasail_matrix_free(parasail_matrix_t *matrix);

/* ----------------------------------------------------------------- profile --- */
/* src/profile/mod.rs:113-277 picks one of these by (stats, ISA, width); on the GPU the ISA
 * slot is meaningless, so all ISA-suffixed names are aliases of the generic ones. */
#define PMX_DECLARE_PROFILE_CREATORS(ISA) \
    parasail_profile_t *parasail_profile_create##ISA##_sat(const char *, const int, const parasail_matrix_t *); \
    parasail_profile_t *parasail_profile_create##ISA##_8(const char *, const int, const parasail_matrix_t *);   \
    parasail_profile_t *parasail_profile_create##ISA##_16(const char *, const int, const parasail_matrix_t *);  \
    parasail_profile_t *parasail_profile_create##ISA##_32(const char *, const int, const parasail_matrix_t *);  \
    parasail_profile_t *parasail_profile_create##ISA##_64(const char *, const int, const parasail_matrix_t *);  \
    parasail_profile_t *parasail_profile_create_stats##ISA##_sat(const char *, const int, const parasail_matrix_t *); \
    parasail_profile_t *parasail_profile_create_stats##ISA##_8(const char *, const int, const parasail_matrix_t *);   \
    parasail_profile_t *parasail_profile_create_stats##ISA##_16(const char *, const int, const parasail_matrix_t *);  \
    parasail_profile_t *parasail_profile_create_stats##ISA##_32(const char *, const int, const parasail_matrix_t *);  \
    parasail_profile_t *parasail_profile_create_stats##ISA##_64(const char *, const int, const parasail_matrix_t *);
PMX_DECLARE_PROFILE_CREATORS()
PMX_DECLARE_PROFILE_CREATORS(_sse_128)
PMX_DECLARE_PROFILE_CREATORS(_avx_256)
PMX_DECLARE_PROFILE_CREATORS(_neon_128)
PMX_DECLARE_PROFILE_CREATORS(_altivec_128)
/* src/profile/mod.rs:384-390 */
void parasail_profile_free(parasail_profile_t *profile);

/* ------------------------------------------------- additive batch interface --- */

#define PMX_MODE_NW 0
#define PMX_MODE_SG 1
#define PMX_MODE_SW 2
/* semi-global free ends: q = query (s1), d = reference (s2) */
#define PMX_SG_QB 1
#define PMX_SG_QE 2
#define PMX_SG_DB 4
#define PMX_SG_DE 8
#define PMX_SG_ALL 15

#define PMX_WANT_STATS 1     /* matches / similar / length per pair */
#define PMX_WANT_CIGAR 2     /* on-device traceback, CIGAR text per pair */
#define PMX_WANT_SORTED 4    /* lengths are ragged: let the engine process pairs in length order (records stay in
                                input order).  The host-buffer entries set it themselves when it pays. */

#define PMX_FLAG_SATURATED 1 /* result record flag: the requested width overflowed */
#define PMX_FLAG_RERUN 2     /* internal: a fast kernel left its exact range; never visible to callers */

typedef struct pmx_config {
    int mode;                /* PMX_MODE_* */
    int sg_flags;            /* PMX_SG_* (ignored unless mode == SG) */
    int open;                /* positive; a gap of length k costs open + (k-1)*extend */
    int extend;
    int width;               /* 0 = sat (promote on overflow), 8, 16, 32, 64 */
    int want;                /* PMX_WANT_* */
    const parasail_matrix_t *matrix;
} pmx_config_t;

/* One record per pair, 16 bytes. */
typedef struct pmx_record {
    int32_t score;
    int32_t end_query;       /* 0-based inclusive */
    int32_t end_ref;
    int32_t flags;           /* PMX_FLAG_* */
} pmx_record_t;

typedef struct pmx_stats {
    int32_t matches, similar, length;
} pmx_stats_t;

/* Sequences are packed back to back: pair k's query is qbuf[qoff[k] .. qoff[k+1]).
 * Returns 0 on success, <0 on error (pmx_last_error() describes it).
 *
 * PSSM matrices (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) are taken by pmx_align_batch / _2bit / _device,
 * pmx_align_profile_batch / _device, pmx_align_batch_cigar and the _multi entries, in every mode (nw, sg with any free ends, sw)
 * and width, with or without PMX_WANT_STATS.  Every query (or the profile's query) must have the PSSM's length; cell (i, j) scores
 * pssm[i][mapper[r[j]]], `matches` counts mapper[q[i]] == mapper[r[j]] along the path and `similar` counts pssm[i][.] > 0: each record,
 * its statistics and its CIGAR equal those of the one-pair call with the same PSSM.  Refused with -1 and a pmx_last_error() text
 * before any GPU work: a query length different from the PSSM's (device entries: max_qlen; the caller keeps every query at that
 * length), and a PSSM whose length x size int16 rows do not fit 160 KB.  Banded and table batches do not take a PSSM. */

/* Host buffers in, host records out (H2D + kernels + D2H inside). */
int pmx_align_batch(const pmx_config_t *cfg, int64_t n,
                    const uint8_t *qbuf, const int64_t *qoff,
                    const uint8_t *rbuf, const int64_t *roff,
                    pmx_record_t *out, pmx_stats_t *stats_out /* NULL unless WANT_STATS */);   /* PSSM: every query has its length */

/* The same with 2-bit packed sequences (additive input form for 4-letter alphabets): base b of a buffer sits in byte b / 4 at
 * bits 2 (b % 4) and holds the index of its letter in the matrix alphabet (0..3); the offsets count BASES.  A quarter of the
 * bytes cross PCIe; a small kernel spells the letters out on the device before the usual path runs. */
int pmx_align_batch_2bit(const pmx_config_t *cfg, int64_t n,
                         const uint8_t *q2, const int64_t *qoff,
                         const uint8_t *r2, const int64_t *roff,
                         pmx_record_t *out, pmx_stats_t *stats_out);

/* Device-resident buffers (all pointers are device pointers on the current device),
 * asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream).
 * Internal scratch (length-sort permutation, retry list of the perm-table kernel) belongs to the calling
 * host thread and is reused by its next call: a thread may queue calls back to back on ONE stream; to run
 * on several streams at once, call from several threads.  Internal record flag values (PMX_FLAG_RERUN, 4)
 * never survive to the caller. */
int pmx_align_batch_device(const pmx_config_t *cfg, int64_t n,
                           const uint8_t *d_qbuf, const int64_t *d_qoff,
                           const uint8_t *d_rbuf, const int64_t *d_roff,
                           int32_t max_qlen, int32_t max_rlen,
                           pmx_record_t *d_out, pmx_stats_t *d_stats_out, void *stream);   /* PSSM: max_qlen == its length, and every query */

/* One reused query profile against many references (profile arm, src/aligner/mod.rs:431-450).  A PSSM: the profile's query
 * length must equal the PSSM's length (the database search of one position-specific profile). */
int pmx_align_profile_batch(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                            const uint8_t *rbuf, const int64_t *roff,
                            pmx_record_t *out, pmx_stats_t *stats_out);

/* The same with device-resident references (device pointers, asynchronous on `stream`); the same PSSM rule. */
int pmx_align_profile_batch_device(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                   const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_rlen,
                                   pmx_record_t *d_out, pmx_stats_t *d_stats_out, void *stream);

/* Banded batches (extension).  The reference has one banded entry -- Aligner::banded_nw -> parasail_nw_banded above: global, main
 * diagonal.  The batch form takes any mode and an optional per-pair band centre: cell (i, j) of pair k belongs to the band iff
 * |(j - i) - diag[k]| <= band (diag == NULL: 0 for every pair); cells outside it cannot be entered or left.  Only the band's
 * cells are computed (band <= 63; wider bands run the general kernel with a mask).  BASELINE config 5's "banded SW" is
 * mode = PMX_MODE_SW with diag[k] = end_ref - end_query of a first full pass, or a seed's diagonal.  Score and end positions
 * only; 32-bit lanes (cfg->width is ignored).  profile != NULL: the profile arm (qbuf / qoff are ignored). */
int pmx_align_batch_banded(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                           const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                           int32_t band, const int32_t *diag, pmx_record_t *out);
int pmx_align_batch_banded_device(const pmx_config_t *cfg, int64_t n,
                                  const uint8_t *d_qbuf, const int64_t *d_qoff,
                                  const uint8_t *d_rbuf, const int64_t *d_roff,
                                  int32_t max_qlen, int32_t max_rlen, int32_t band, const int32_t *d_diag,
                                  pmx_record_t *d_out, void *stream);
int pmx_align_profile_batch_banded_device(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                          const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_rlen,
                                          int32_t band, const int32_t *d_diag, pmx_record_t *d_out, void *stream);
/* Banded batches with traceback (extension).  Same band rule as pmx_align_batch_banded: cell (i, j) of pair k belongs to the band
 * iff |(j - i) - diag[k]| <= band.  cfg->want must contain PMX_WANT_CIGAR and/or PMX_WANT_STATS; PMX_WANT_SORTED is allowed.
 * Records are the 32-bit banded records (cfg->width is ignored), identical to pmx_align_batch_banded's.  A pair whose band misses
 * its end cell has score INT32_MIN / 2, an empty CIGAR and zero statistics.  profile != NULL: the profile arm (qbuf / qoff and
 * max_qlen are ignored).  The CIGAR text follows pmx_align_batch_cigar (a block freed with pmx_free, cigar_off n + 1 entries); the
 * device entry follows pmx_align_batch_cigar_device (n + 1 offsets; a pair whose text would cross cigar_capacity is not written;
 * offsets start at 0).  NW, SG with any free ends, SW; square matrices of size <= 32 (31 letters + the wildcard: "ACGTA", nuc44 and
 * BLOSUM62 included); any open / extend; bands 0 .. 63; any lengths.  Refused
 * with -1 and a pmx_last_error() text before any GPU work: bands above 63, larger alphabets, PSSM matrices, a want without
 * PMX_WANT_CIGAR and PMX_WANT_STATS. */
int pmx_align_batch_banded_cigar(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                 const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                                 int32_t band, const int32_t *diag,
                                 pmx_record_t *out, pmx_stats_t *stats_out /* NULL unless WANT_STATS */,
                                 char **cigar_buf, int64_t *cigar_off /* NULL unless WANT_CIGAR */);
int pmx_align_batch_banded_cigar_device(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                        const uint8_t *d_qbuf, const int64_t *d_qoff, const uint8_t *d_rbuf, const int64_t *d_roff,
                                        int32_t max_qlen, int32_t max_rlen, int32_t band, const int32_t *d_diag,
                                        pmx_record_t *d_out, pmx_stats_t *d_stats_out,
                                        char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off, void *stream);

/* Profile database search (extension): one reused profile against n references, the references that score at least min_score --
 * at most the best max_hits of them -- and, for each of those hits, a banded second pass with traceback around the first pass's
 * diagonal.  Selection, compaction of the selected references and the second pass all run on the device; the references are
 * uploaded once.
 *
 * Selection (pmx_select_hits_device, and the search entries through it).  The passing set is P = { k : score_k >= min_score }: only
 * the score of a record is looked at.  With max_hits > 0 and |P| > max_hits the max_hits members of P that come first under (score
 * descending, index ascending) are kept, the members inside the tie run at the last kept score included; max_hits == 0: no limit.
 * PMX_HITS_BY_INDEX lists the selected in ascending index, PMX_HITS_BY_SCORE in (score descending, index ascending).  At most
 * `capacity` indices are written, the first ones in that order; d_counts[0] is the full number selected and d_counts[1] is |P|.  The
 * result is bit-identical from run to run.  Asynchronous on `stream`, no host synchronisation; scratch belongs to the calling thread
 * like that of the other device entries (by score: 24 bytes per selectable hit for the sort). */
#define PMX_HITS_BY_INDEX 0
#define PMX_HITS_BY_SCORE 1
int pmx_select_hits_device(const pmx_record_t *d_rec, int64_t n, int32_t min_score, int64_t max_hits /* 0 = no limit */, int order,
                           int64_t *d_hit_index, int64_t capacity, int64_t *d_counts /* [0] selected, [1] passing the threshold */,
                           void *stream);
/* References d_index[0 .. h) of a packed device buffer, back to back in d_out: d_out_off receives h + 1 offsets starting at 0, a
 * reference whose end would cross out_capacity is not written (the cigar_capacity rule).  No byte outside
 * [d_rbuf, d_rbuf + d_roff[n]) is read.  Asynchronous on `stream`. */
int pmx_gather_refs_device(const uint8_t *d_rbuf, const int64_t *d_roff, int64_t n, const int64_t *d_index, int64_t h,
                           uint8_t *d_out, int64_t out_capacity, int64_t *d_out_off, void *stream);

/* band < 0: no second pass -- hits with their first-pass records only, begins -1, any matrix the first pass takes (a PSSM too).
 * band 0 .. 63: the second pass of pmx_align_batch_banded_cigar in its profile arm over the hits, diag = end_ref - end_query of the
 * first pass; its limits hold (square matrices of size <= 32, no PSSM) and cfg->want must contain PMX_WANT_CIGAR and / or
 * PMX_WANT_STATS.  The first pass is the score-only batch pmx_align_profile_batch_device runs for cfg (PMX_WANT_SORTED is passed on to
 * both passes, the other want bits to the second). */
typedef struct pmx_search_opts { int32_t min_score; int64_t max_hits; int32_t order; int32_t band; } pmx_search_opts_t;
/* beg_query / beg_ref: the first cell of the second pass's path (what the one-pair parasail_cigar_t reports; 0 / 0 for global and
 * semi-global paths), -1 without a second pass or where the band misses the end cell. */
typedef struct pmx_hit { int64_t index; pmx_record_t first; int32_t diag, beg_query, beg_ref, reserved; } pmx_hit_t;
/* One block, released with pmx_search_result_free: hits, recs (second-pass records; NULL with band < 0), stats (NULL unless
 * PMX_WANT_STATS and band >= 0), cigar text (NULL unless PMX_WANT_CIGAR and band >= 0) and cigar_off (n_hits + 1 entries, always
 * there; all 0 without text) point into it.  n_passing = |P|. */
typedef struct pmx_search_result {
    int64_t n_hits, n_passing;
    pmx_hit_t *hits;
    pmx_record_t *recs;
    pmx_stats_t *stats;
    char *cigar;
    int64_t *cigar_off;
} pmx_search_result_t;
/* Host references in, one callee-allocated result out (*result is NULL on failure).  Zero hits is success with empty outputs and
 * cigar_off[0] == 0.  Refused with -1 and a pmx_last_error() text before any GPU work: a NULL profile or opts, an order other than
 * PMX_HITS_BY_*, a negative max_hits, a band above 63, a PSSM or a matrix beyond size 32 with band >= 0, a want without
 * PMX_WANT_CIGAR and PMX_WANT_STATS with band >= 0. */
int pmx_search_profile(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                       const uint8_t *rbuf, const int64_t *roff, const pmx_search_opts_t *opts, pmx_search_result_t **result);
void pmx_search_result_free(pmx_search_result_t *result);
/* Device references in, device outputs into caller buffers: d_first (n first-pass records; NULL: internal scratch), d_hits / d_recs /
 * d_stats (`capacity` entries each; d_recs and d_stats as cfg->want and band ask), d_cigar_text / d_cigar_off (capacity + 1 offsets)
 * following pmx_align_batch_banded_cigar_device: offsets of the hits written start at 0 and a hit whose text would cross
 * cigar_capacity is not written.  min(d_counts[0], capacity) hits are written, the first ones in output order; entries beyond them
 * are untouched.  A negative capacity is refused like the cases above.  The call synchronises `stream` ONCE, between the passes, to
 * read the hit count; everything else is asynchronous on `stream`. */
int pmx_search_profile_device(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                              const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_rlen, const pmx_search_opts_t *opts,
                              pmx_record_t *d_first, pmx_hit_t *d_hits, pmx_record_t *d_recs, pmx_stats_t *d_stats, int64_t capacity,
                              char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off, int64_t *d_counts, void *stream);

/* Sequence-set batches (extension): sequence sets that live on the device, batches whose pairs are index + window descriptors into
 * those sets, and an all-vs-all entry that enumerates its pairs on the device.  A read aligned against several windows of a resident
 * reference, or a set compared with itself, moves 32 bytes per pair over the link instead of both sequences once per pair.
 *
 * Sets.  pmx_seqset_create uploads a packed buffer (sequence k is buf[off[k] .. off[k + 1]), off non-decreasing from off[0] >= 0)
 * and keeps a host copy of the offsets (8 bytes per sequence) for validation.  pmx_seqset_wrap_device copies nothing: d_buf (`bytes`
 * bytes) and d_off (count + 1 entries) are the caller's device buffers and must outlive the set.  A set belongs to the device current
 * at its creation.  NULL on failure (pmx_last_error() tells why).
 *
 * Results.  Record k is the record pmx_align_batch_device gives for the pair (query window, reference window) of descriptor k: the
 * same score, the same end positions RELATIVE TO THE WINDOWS, the same flags, and the same statistics with PMX_WANT_STATS.  Every
 * mode, width and matrix pmx_align_batch_device takes is taken, a PSSM under its rule (every query window has the PSSM's length;
 * device entries: max_qlen == that length).  PMX_WANT_SORTED is passed on; PMX_WANT_CIGAR is refused.  Q and R may be the same set.
 * Records are in pair order whatever the chunking: inside, the batch is cut into chunks of opts->chunk_pairs pairs (0 / NULL: a
 * default derived from the maxima) whose windows a gather kernel packs into chunk buffers beside the previous chunk's alignment.
 * chunk_pairs never changes a result.
 *
 * Bad descriptors: an index outside its set, beg < 0, a len below -1, a window reaching past the sequence's end, a resolved length
 * of 0, a resolved length above max_qlen / max_rlen (device entries).  The device entries give a bad pair the record
 * {0, -1, -1, PMX_FLAG_BAD_PAIR} and zero statistics; every other pair is unaffected and no byte outside a set's buffer is read (a
 * wrapped set's offsets are checked against `bytes` too).  The host entries refuse the call with -1 and a pmx_last_error() text that
 * names the first bad pair: before any GPU work when both sets carry host offsets, otherwise after the device pass has flagged it
 * (`out` is then unspecified).
 *
 * Refused with -1 and a pmx_last_error() text before any GPU work: NULL sets or pairs; negative n, first or count; first + count
 * beyond pmx_all_pairs_count(); a set of more than 2^31 - 1 sequences in the all-pairs entries; chunk_pairs < 0; max_qlen / max_rlen /
 * max_len < 1; a set of another device than the current one; what pmx_align_batch_device refuses.  n == 0 / count == 0 succeeds and
 * touches nothing.
 *
 * The device entries are asynchronous on `stream` (all pointers but the sets, cfg and opts are device pointers): a call whose scratch is
 * already large enough returns without a host synchronisation; the first call of a thread, and one that needs more scratch than any
 * before it, allocate, which synchronises.  Scratch belongs to the calling thread like that of the other device entries: two sets of
 * chunk buffers of at most 256 MiB each (one chunk of one pair when a single pair needs more) and 41 bytes per pair of a chunk.
 * pmx_last_kernel() names the alignment kernel the last chunk ran. */
typedef struct pmx_seqset pmx_seqset_t;
pmx_seqset_t *pmx_seqset_create(const uint8_t *buf, const int64_t *off, int64_t count);
pmx_seqset_t *pmx_seqset_wrap_device(const uint8_t *d_buf, const int64_t *d_off, int64_t count, int64_t bytes);
void    pmx_seqset_free(pmx_seqset_t *set);
int64_t pmx_seqset_count(const pmx_seqset_t *set);          /* -1 for NULL */

typedef struct pmx_pair {            /* 32 bytes */
    int64_t q, r;                    /* sequence index in the query set / the reference set */
    int32_t q_beg, q_len;            /* window inside that sequence; len -1 = from beg to its end */
    int32_t r_beg, r_len;
} pmx_pair_t;
typedef struct pmx_pairs_opts { int64_t chunk_pairs; } pmx_pairs_opts_t;   /* 0 / NULL = default */

#define PMX_FLAG_BAD_PAIR 8  /* result record flag of the set-batch device entries: the descriptor was bad, nothing was aligned */

int pmx_align_pairs(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                    int64_t n, const pmx_pair_t *pairs,
                    pmx_record_t *out, pmx_stats_t *stats_out /* NULL unless WANT_STATS */, const pmx_pairs_opts_t *opts);
int pmx_align_pairs_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                           int64_t n, const pmx_pair_t *d_pairs, int32_t max_qlen, int32_t max_rlen,
                           pmx_record_t *d_out, pmx_stats_t *d_stats_out, void *stream,
                           const pmx_pairs_opts_t *opts);

/* All-vs-all: pairs [first, first + count) of the strict upper triangle of S x S in row-major order,
 * p = i (2 N - i - 1) / 2 + (j - i - 1) with i < j; query = sequence i, reference = sequence j, whole sequences.  The descriptors are
 * generated on the device chunk by chunk: nothing but the records crosses the link.  pmx_all_pairs_count: N (N - 1) / 2, or -1 for
 * N < 0 or N > 2^31 - 1.  pmx_all_pairs_index: the exact (i, j) of pair p on the host; -1 for p outside [0, count). */
int64_t pmx_all_pairs_count(int64_t nseq);
int pmx_all_pairs_index(int64_t nseq, int64_t p, int64_t *i, int64_t *j);
int pmx_align_all_pairs(const pmx_config_t *cfg, const pmx_seqset_t *S, int64_t first, int64_t count,
                        pmx_record_t *out, pmx_stats_t *stats_out, const pmx_pairs_opts_t *opts);
int pmx_align_all_pairs_device(const pmx_config_t *cfg, const pmx_seqset_t *S, int64_t first, int64_t count,
                               int32_t max_len, pmx_record_t *d_out, pmx_stats_t *d_stats_out, void *stream,
                               const pmx_pairs_opts_t *opts);
/* Test hook: the descriptors the all-pairs entries generate, `count` of them into d_pairs; asynchronous on `stream`. */
int pmx_all_pairs_enumerate_device(int64_t nseq, int64_t first, int64_t count, pmx_pair_t *d_pairs, void *stream);

/* Strands and CIGAR output for set batches: the extension stage of a read mapper (a read against candidate windows of a resident
 * reference, half of them on the reverse strand, alignments and not only scores).
 *
 * Strand: one byte per pair (NULL: all 0).  0 = the query window as stored; 1 = the query window reverse-complemented: window bytes
 * w[0 .. L) become w'[x] = comp[w[L - 1 - x]].  The reference window is never reversed.  comp is one fixed table of 256 bytes
 * (pmx_complement_table): "ACGTUMRWSYKVHDBN" -> "TGCAAKYWSRMBDHVN", the lower-case letters the same way to lower case, every other
 * byte to itself.  It is applied to the raw bytes before the matrix mapper, whatever the matrix (a caller aligning proteins passes no
 * strands).  ALL POSITIONS OF A STRAND-1 PAIR -- end_query and beg_query alike -- ARE RELATIVE TO THE REVERSE-COMPLEMENTED WINDOW:
 * position p of it is stored byte q_beg + L - 1 - p of the sequence.  A strand byte other than 0 or 1 is a bad descriptor: the device
 * entry writes PMX_FLAG_BAD_PAIR, the host entry refuses and names the first such pair.
 *
 * Without PMX_WANT_CIGAR the _ex entries are pmx_align_pairs[_device] with the strand applied (record k and its statistics are what
 * pmx_align_batch_device gives for the two resolved windows; with no strands the results are byte-identical to
 * pmx_align_pairs_device); beg / d_beg and the text buffers must then be NULL.
 *
 * With PMX_WANT_CIGAR records, text and offsets are byte-identical to what pmx_align_batch_cigar_device writes for the same windows
 * packed back to back: d_cigar_off holds n + 1 offsets from 0, d_cigar_off[n] is the number of bytes the batch needs, a pair whose
 * text would cross cigar_capacity is not written.  d_beg (optional, 2 n) receives the walk's begin cell as pmx_hit_t documents it: the
 * path's first cell, 0 / 0 for global and semi-global paths.  A bad pair gets {0, -1, -1, PMX_FLAG_BAD_PAIR}, an empty text
 * (off[k + 1] == off[k]) and begins -1 / -1; every other pair is unaffected.  chunk_pairs never changes a byte of any output: every
 * chunk's text starts at the running total, which stays on the device.  The window is that of pmx_align_batch_cigar_device -- no
 * width 8, no PSSM, open >= extend, score + open within a byte, queries up to 1023 symbols; outside it both entries refuse with -1
 * before any alignment runs (the check reads the maxima only) and point to pmx_align_batch_cigar.  PMX_WANT_CIGAR together with
 * PMX_WANT_STATS is refused.  All-vs-all with CIGARs: pmx_all_pairs_enumerate_device, then the _ex entry.
 *
 * The host entry validates like pmx_align_pairs (strand bytes included; before any GPU work when both sets carry host offsets),
 * uploads 32 + 1 bytes per pair and, for CIGAR, sizes the device text at half a byte per symbol + 16 per pair and runs once more at
 * the exact size when the text did not fit.  *cigar_buf is a block released with pmx_free (NULL on failure), cigar_off has n + 1
 * entries.  The device entry is asynchronous on `stream` under the rule of the other set entries (with strand bytes the chunk scratch
 * is one byte per pair larger; the CIGAR road adds the scratch of pmx_align_batch_cigar_device for one chunk).  pmx_last_kernel() is
 * what the last chunk's road left. */
void pmx_complement_table(uint8_t table[256]);
int pmx_align_pairs_ex_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                              int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand /* n bytes; NULL: all forward */,
                              int32_t max_qlen, int32_t max_rlen,
                              pmx_record_t *d_out, pmx_stats_t *d_stats_out,
                              int32_t *d_beg /* 2 n: beg_query, beg_ref; optional, PMX_WANT_CIGAR only */,
                              char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off /* n + 1; PMX_WANT_CIGAR only */,
                              void *stream, const pmx_pairs_opts_t *opts);
int pmx_align_pairs_ex(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                       int64_t n, const pmx_pair_t *pairs, const uint8_t *strand,
                       pmx_record_t *out, pmx_stats_t *stats_out, int32_t *beg,
                       char **cigar_buf, int64_t *cigar_off, const pmx_pairs_opts_t *opts);
/* Building block and test hook: the resolved windows themselves (strand applied), packed back to back into d_qout / d_rout.  d_qoff /
 * d_roff receive n + 1 offsets from 0; a window whose end would cross its capacity is not written (the pmx_gather_refs_device rule);
 * a bad pair's placeholder is one zero byte on either side and d_ok[k] = 0 (d_ok: n validity bytes, optional).  No byte outside a
 * set's buffer is read.  Asynchronous on `stream`. */
int pmx_gather_pairs_device(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                            const uint8_t *d_strand, int32_t max_qlen, int32_t max_rlen,
                            uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                            uint8_t *d_ok /* n validity bytes, optional */, void *stream);

/* Set search (extension): the thresholded, compacted form of the set batches.  The pairs of an enumeration -- a window of the strict
 * upper triangle of Q x Q, a window of the rectangle Q x R, or a descriptor list -- are aligned chunk by chunk by the kernels of the set
 * batches, and only the pairs with score >= min_score leave their chunk, as one compact hit list in enumeration order.  Device memory is
 * bounded by the chunk scratch and the hit buffers, not by the number of pairs: an all-vs-all of 100 000 sequences (5 10^9 pairs, 80 GB
 * of records) runs in the memory of one chunk plus its hits.
 *
 * The hit set.  Let record k be what pmx_align_pairs_device / pmx_align_all_pairs_device write for pair k of the enumeration (RECT: for
 * the descriptor pmx_rect_pairs_enumerate_device generates).  The hits are { k : record_k.score >= min_score } in ascending k: only the
 * score is looked at, as in pmx_select_hits_device, so a bad descriptor's record {0, -1, -1, PMX_FLAG_BAD_PAIR} is a hit when
 * min_score <= 0 and keeps its flag (the host entry refuses bad pairs, as pmx_align_pairs does).
 *
 * The outputs of hit x, a structure of arrays: d_hit_pairs[x] the pair's descriptor -- for the enumerated shapes exactly what the
 * enumerator generated, for PMX_PAIRS_LIST the caller's descriptor with its windows; d_hit_index[x] its absolute number p in the
 * enumeration (first + k; LIST: k); d_hit_recs[x] the record, byte for byte; d_hit_stats[x] its statistics.  d_hit_pairs is a valid
 * d_pairs argument: the CIGAR pass over the hits is pmx_align_pairs_ex_device(..., n = d_counts[1], d_hit_pairs, ...) with nothing in
 * between, which is why PMX_WANT_CIGAR is refused here.  min(passing, capacity) hits are written, the first ones in enumeration order;
 * entries beyond them are untouched; d_counts[0] is the full number passing and d_counts[1] the number written; capacity == 0 counts
 * only.  d_hit_pairs and d_hit_index are optional (NULL: not written).
 *
 * Determinism.  The output is bit-identical from run to run, and chunk_pairs / slice_pairs never change a byte of any output: a
 * chunk's hit positions come from the selection's scan (ascending index), its hits go behind the running total, which lives on the
 * device (in d_counts) and advances in chunk order on the caller's stream.  No position depends on which workgroup finishes first.
 *
 * Every mode, width and matrix of pmx_align_pairs_device is accepted, a PSSM under its rule; PMX_WANT_SORTED is passed on.  Refused with
 * -1 and a pmx_last_error() text before any GPU work: everything pmx_align_pairs_device / pmx_align_all_pairs_device refuse; an unknown
 * shape; TRIANGLE with an R that is neither NULL nor Q; RECT or LIST without R; LIST with first != 0 or NULL pairs; another shape with
 * non-NULL pairs; first + n beyond the shape's count; a rectangle whose count overflows; a negative capacity, max_hits or slice_pairs;
 * NULL d_hit_recs with capacity > 0; NULL d_counts; PMX_WANT_STATS without d_hit_stats, or d_hit_stats without PMX_WANT_STATS;
 * PMX_WANT_CIGAR.  n == 0 succeeds and writes zero counts (d_counts may then be NULL).
 *
 * The device entry is asynchronous on `stream` under the rule of the other set entries: no host synchronisation once the calling
 * thread's scratch is large enough -- the chunk buffers of pmx_align_pairs_device and, per pair of a chunk, 16 bytes of record, 12 of
 * statistics (PMX_WANT_STATS), 8 of hit position and the selection's block counts: about 45 bytes.
 *
 * The host entry works in slices of opts->slice_pairs pairs (0: 2^24): device hit buffers are sized to the slice (to max_hits when that
 * is smaller), so they cannot overflow; one stream synchronisation per slice reads the slice's count, then its hits are copied behind
 * those of the slices before.  Those buffers are thread scratch of 56 bytes per pair of a slice (68 with PMX_WANT_STATS): 0.94 GB
 * (1.14 GB) at the default slice once n reaches 2^24, however few pairs pass -- a smaller slice_pairs, or max_hits, bounds them.  It validates as pmx_align_pairs / pmx_align_all_pairs do and names the first bad pair (RECT: "pair k
 * (i, j): side: cause", the all-pairs rule): before any GPU work when both sets carry host offsets, otherwise at the end of the slice
 * whose device pass met it.  max_hits > 0 stops storing after that many hits, in enumeration order, and goes on counting n_passing;
 * max_hits == 0: no limit.  LIST descriptors are uploaded slice by slice, 32 bytes per pair; the enumerated shapes upload nothing.
 * *result is one callee-allocated block (NULL on failure) released with pmx_pair_hits_free: pairs, index and recs hold n_hits entries,
 * stats too with PMX_WANT_STATS (else NULL).  Zero hits is success with empty arrays. */
#define PMX_PAIRS_LIST     0   /* the n descriptors of pairs / d_pairs (first must be 0) */
#define PMX_PAIRS_TRIANGLE 1   /* pairs [first, first + n) of the strict upper triangle of Q (R NULL or == Q): pmx_all_pairs_index numbering */
#define PMX_PAIRS_RECT     2   /* pairs [first, first + n) of Q x R, row-major: p = i * |R| + j, query = Q[i], reference = R[j], whole
                                  sequences; Q == R allowed (i == j included) */
int64_t pmx_rect_pairs_count(int64_t nq, int64_t nr);          /* nq * nr, -1 if negative or beyond INT64_MAX */
/* Test hook, like pmx_all_pairs_enumerate_device: the descriptors PMX_PAIRS_RECT generates. */
int pmx_rect_pairs_enumerate_device(int64_t nq, int64_t nr, int64_t first, int64_t count, pmx_pair_t *d_pairs, void *stream);
int pmx_search_pairs_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                            int64_t first, int64_t n, const pmx_pair_t *d_pairs /* LIST only, else NULL */,
                            int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                            pmx_pair_t *d_hit_pairs /* optional */, int64_t *d_hit_index /* optional */,
                            pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats /* iff PMX_WANT_STATS */, int64_t capacity,
                            int64_t *d_counts /* [0] passing, [1] written = min(passing, capacity) */,
                            void *stream, const pmx_pairs_opts_t *opts);
typedef struct pmx_pair_search_opts { int32_t min_score, shape; int64_t max_hits, chunk_pairs, slice_pairs; } pmx_pair_search_opts_t;   /* 32 bytes */
typedef struct pmx_pair_hits { int64_t n_hits, n_passing; pmx_pair_t *pairs; int64_t *index; pmx_record_t *recs; pmx_stats_t *stats; } pmx_pair_hits_t;
int  pmx_search_pairs(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                      const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, pmx_pair_hits_t **result);
void pmx_pair_hits_free(pmx_pair_hits_t *hits);

/* Per-query top-K set search (extension): for every query row of the rectangle Q x R the best k references, selected on the device
 * while the rows' pairs go through the chunk pipeline of the set batches.  Set search above keeps what passes ONE score for the whole
 * enumeration; many queries against a database want the best k of EACH query, which no single threshold gives.  Device memory is
 * bounded by the chunk scratch, k entries per row and the hits, not by the number of pairs.
 *
 * Inputs.  The query rows [q_first, q_first + nq) of Q against all of R (R == Q allowed; R == NULL means Q), whole sequences; min_score
 * (INT32_MIN: pure top-K); k, 1 .. PMX_TOPK_MAX; skip_self (R must be Q: the pair (i, i) is never a candidate); chunk_pairs as in the
 * other set entries.  |R| <= 2^31 - 1.
 *
 * Candidates and the cut.  Let rec(i, j) be the record pmx_align_pairs_device writes for the descriptor
 * pmx_rect_pairs_enumerate_device generates for pair p = i |R| + j.  P_i = { j : rec(i, j).score >= min_score } (without j == i under
 * skip_self): only the score is looked at, as in pmx_select_hits_device, so a bad descriptor's record {0, -1, -1, PMX_FLAG_BAD_PAIR} is
 * a candidate when min_score <= 0 and keeps its flag.  Row i keeps the first min(k, |P_i|) members of P_i under (score descending, j
 * ascending): the cut falls inside the tie run at the k-th score by ascending j, the rule of pmx_select_hits_device applied per row.
 *
 * Outputs of the device entry, CSR: d_row_off receives nq + 1 offsets starting at 0 and is always written in full; row i's hits lie at
 * [off[i - q_first], off[i - q_first + 1]) in (score descending, j ascending) order.  Per hit, a structure of arrays like set
 * search's: d_hit_pairs (optional) the descriptor {i, j, 0, -1, 0, -1}, a valid d_pairs argument for pmx_align_pairs_ex_device;
 * d_hit_index (optional) p, absolute; d_hit_recs the record, byte for byte; d_hit_stats the statistics, iff PMX_WANT_STATS.
 * d_row_passing (optional): nq values of |P_i|.  d_counts[0] = hits kept in total (= off[nq]), d_counts[1] = hits written
 * (min(kept, capacity)), d_counts[2] = the sum of |P_i|.  Only hit positions below `capacity` are written, entries behind them are
 * untouched; capacity == 0 counts only.
 *
 * Determinism.  The output is bit-identical from run to run and chunk_pairs / slice_rows never change a byte: (score, j) orders a row
 * totally, the kept set is the k first under that order whatever the order of arrival, and every output position comes from the sorted
 * lists and a scan of their lengths.  The selection kernels contain no atomic.
 *
 * Refused with -1 and a pmx_last_error() text before any GPU work: everything pmx_search_pairs_device refuses for PMX_PAIRS_RECT
 * (PMX_WANT_CIGAR with the same text: the hit pairs go to pmx_align_pairs_ex[_device]); k outside 1 .. PMX_TOPK_MAX (larger k:
 * pmx_search_pairs over the rows, then pmx_select_hits_device per row); a negative q_first or nq, rows beyond |Q|; |R| above
 * 2^31 - 1; skip_self with R != Q; a negative capacity; NULL d_hit_recs with capacity > 0; NULL d_row_off or d_counts with nq > 0;
 * PMX_WANT_STATS without d_hit_stats, or d_hit_stats without PMX_WANT_STATS.  nq == 0 succeeds and writes zero counts (and
 * d_row_off[0] = 0) where those pointers are given.
 *
 * The device entry is asynchronous on `stream` under the rule of the other set entries.  Scratch of the calling thread: the chunk
 * buffers of pmx_align_pairs_device; per pair of a chunk 16 bytes of record, 12 of statistics (PMX_WANT_STATS) and at most 8 of tile
 * survivors; per row min(k, |R|) x (8 + 16 (+ 12)) bytes of running state.
 *
 * The host entry validates as pmx_search_pairs does for a rectangle and names the first bad pair "pair x (i, j): side: cause" (x counts
 * from the first pair of row q_first): before any GPU work when both sets carry host offsets, otherwise at the end of the slice whose
 * device pass met it.  It works in slices of opts->slice_rows rows (0: as many as keep a slice's running state within 256 MiB, the
 * bound of the chunk buffers), one stream synchronisation per slice.  *result is one callee-allocated block (NULL on failure) released
 * with pmx_topk_hits_free: row_off holds n_rows + 1 entries, row_passing n_rows, pairs / index / recs n_hits, stats too with
 * PMX_WANT_STATS (else NULL); n_passing is the sum of row_passing. */
#define PMX_TOPK_MAX 1024
int pmx_search_topk_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                           int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                           pmx_pair_t *d_hit_pairs /* optional */, int64_t *d_hit_index /* optional */,
                           pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats /* iff PMX_WANT_STATS */, int64_t capacity,
                           int64_t *d_row_off /* nq + 1 */, int64_t *d_row_passing /* nq, optional */,
                           int64_t *d_counts /* [0] kept, [1] written, [2] passing */, void *stream, const pmx_pairs_opts_t *opts);
typedef struct pmx_topk_opts { int32_t min_score, k, skip_self; int64_t chunk_pairs, slice_rows; } pmx_topk_opts_t;   /* 32 bytes */
typedef struct pmx_topk_hits { int64_t n_rows, n_hits, n_passing; int64_t *row_off, *row_passing; pmx_pair_t *pairs; int64_t *index; pmx_record_t *recs; pmx_stats_t *stats; } pmx_topk_hits_t;
int  pmx_search_topk(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                     const pmx_topk_opts_t *opts, pmx_topk_hits_t **result);
void pmx_topk_hits_free(pmx_topk_hits_t *hits);
/* Test hook of the top-K kernels (parasail-rs_amd/csrc/pmx_topk.hip; reference: tests/topk_ref.py): the selection of
 * pmx_search_topk[_stranded]_device on records the caller supplies instead of alignments, so that scores over all of int32, rows of
 * hundreds of tiles and any flag bits reach the tile, row and emit kernels.  d_rec[li * nr + j] (and d_stats, optional) is the record of
 * pair (q_first + li, j).  The nq * nr records are walked in consecutive chunks of chunk_pairs (0: PMX_TOPK_RECORDS_CHUNK; at most 2^26,
 * the entries' bound), each chunk goes through the entries' merge with the entries' geometry, and the run ends in their offsets scan,
 * emit and counts: the outputs are those documented for pmx_search_topk_device.  skip_self leaves out j == q_first + li.  marked != 0 is
 * the stranded entries' emit: flag bit 0x40000000, their internal mark of a reverse-strand record, is cleared in the emitted records and
 * every other bit is kept; d_hit_strand (optional, one byte per written hit) receives that bit whatever `marked`.  Refused with -1 and a pmx_last_error() text before any GPU work: a negative q_first, nq or nr;
 * nr above 2^31 - 1; (q_first + nq) * nr beyond 2^63 - 1; k outside 1 .. PMX_TOPK_MAX; NULL d_rec, d_row_off or d_counts; a negative
 * capacity or chunk_pairs; NULL d_hit_recs with capacity > 0; d_hit_stats without d_stats.  Asynchronous on `stream`; scratch of the
 * calling thread, the one of pmx_search_topk_device without the chunk buffers. */
#define PMX_TOPK_RECORDS_CHUNK ((int64_t)1 << 22)
int pmx_topk_records_device(const pmx_record_t *d_rec, const pmx_stats_t *d_stats /* optional */,
                            int64_t q_first, int64_t nq, int64_t nr,
                            int32_t min_score, int32_t k, int32_t skip_self, int64_t chunk_pairs /* 0: PMX_TOPK_RECORDS_CHUNK */,
                            int32_t marked, uint8_t *d_hit_strand /* optional */,
                            pmx_pair_t *d_hit_pairs /* optional */, int64_t *d_hit_index /* optional */, pmx_record_t *d_hit_recs,
                            pmx_stats_t *d_hit_stats /* optional, needs d_stats */, int64_t capacity, int64_t *d_row_off /* nq + 1 */,
                            int64_t *d_row_passing /* nq, optional */, int64_t *d_counts, void *stream);

/* Both strands (extension): the set entries for DNA whose orientation is unknown.  Every pair is aligned on the forward and on the
 * reverse strand inside its chunk and the two records become one BEFORE selection, so hits, counts, top-K cuts and device memory
 * are per pair, not per (pair, strand).
 *
 * Semantics, through pmx_align_pairs_ex_device.  Let rec0(k) / stats0(k) be what it writes for descriptor k with strand byte 0 and
 * rec1(k) / stats1(k) with strand byte 1 (for the enumerated shapes descriptor k is the one the enumerator generates).  The folded
 * record of PMX_STRAND_BOTH is the winner's record BYTE FOR BYTE, flags included, its statistics are the winner's and its strand byte
 * says which one won.  Only the score is compared (the rule of pmx_select_hits_device).  All positions of a strand-1 winner are relative
 * to the reverse-complemented window, exactly as the _ex entries document; pmx_complement_table is applied to the raw bytes whatever
 * the matrix.  A bad descriptor is bad on both strands: {0, -1, -1, PMX_FLAG_BAD_PAIR}, zero statistics, strand byte 0 (in every mode).
 * Selection (min_score, max_hits, capacity) and the top-K order work on the FOLDED records; the top-K order stays (score descending,
 * reference index ascending), the strand is not part of the key: a pair is one candidate and a reference appears at most once in a
 * row.  Outputs are bit-identical from run to run; chunk_pairs, slice_pairs and slice_rows count LOGICAL pairs or rows and never
 * change a byte.
 *
 * Refused with -1 and a pmx_last_error() text before any GPU work: a strand mode outside 0 .. 2; a mode other than PMX_STRAND_FORWARD
 * with a PSSM matrix (a reversed query has no PSSM); everything the corresponding entry without strands refuses, with the same texts.
 * n == 0 / nq == 0 behave as there.
 *
 * Scratch.  PMX_STRAND_BOTH keeps two alignment slots per logical pair -- slot 2 k is pair k as stored, slot 2 k + 1 pair k with its
 * query window reverse-complemented -- in the chunk buffers of pmx_align_pairs_device, so the default chunk, derived from the 256 MiB
 * bound, is half as many logical pairs; beside them per pair of a chunk 2 x 16 bytes of slot records, 2 x 12 of slot statistics
 * (PMX_WANT_STATS), one validity byte and 2 strand bytes.  PMX_STRAND_REVERSE has one slot per pair.  PMX_STRAND_FORWARD launches
 * exactly what the entries without strands launch.  pmx_last_kernel() names what the last chunk's alignment ran. */
#define PMX_STRAND_FORWARD 0   /* rec0, strand byte 0 */
#define PMX_STRAND_REVERSE 1   /* rec1, strand byte 1 */
#define PMX_STRAND_BOTH    2   /* rec1 if rec1.score > rec0.score, else rec0: the higher score, a tie goes to the forward strand */
/* Listed pairs, always PMX_STRAND_BOTH: the arguments of pmx_align_pairs[_device] and strand_out / d_strand_out, n bytes, required.
 * PMX_WANT_CIGAR is refused: the CIGAR pass is pmx_align_pairs_ex[_device] with the returned strand bytes.  The device entry gives bad
 * pairs their record and strand 0; the host entry refuses them as pmx_align_pairs does. */
int pmx_align_pairs_both_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                int64_t n, const pmx_pair_t *d_pairs, int32_t max_qlen, int32_t max_rlen,
                                pmx_record_t *d_out, pmx_stats_t *d_stats_out, uint8_t *d_strand_out /* n bytes */, void *stream,
                                const pmx_pairs_opts_t *opts);
int pmx_align_pairs_both(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                         int64_t n, const pmx_pair_t *pairs,
                         pmx_record_t *out, pmx_stats_t *stats_out /* NULL unless WANT_STATS */, uint8_t *strand_out /* n bytes */,
                         const pmx_pairs_opts_t *opts);
/* Set search with a strand mode: the argument list of pmx_search_pairs_device, then strand_mode and d_hit_strand (optional: one byte
 * per written hit, parallel to d_hit_recs).  With PMX_STRAND_FORWARD every output is byte-identical to pmx_search_pairs_device's and
 * the strand bytes are 0; with PMX_STRAND_REVERSE it is byte-identical to pmx_search_pairs_device over a query set whose sequences
 * were reverse-complemented (whole-sequence shapes), strand bytes 1.  The CIGAR pass over the hits needs nothing new:
 * pmx_align_pairs_ex_device(..., n = d_counts[1], d_hit_pairs, d_hit_strand, ...).  The host result is a pmx_strand_hits_t: the fields
 * of pmx_pair_hits_t followed by the strand bytes (n_hits of them), one block released with pmx_strand_hits_free. */
int pmx_search_pairs_stranded_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                     int64_t first, int64_t n, const pmx_pair_t *d_pairs /* LIST only, else NULL */,
                                     int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                     pmx_pair_t *d_hit_pairs /* optional */, int64_t *d_hit_index /* optional */,
                                     pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats /* iff PMX_WANT_STATS */, int64_t capacity,
                                     int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts,
                                     int strand_mode, uint8_t *d_hit_strand /* optional */);
typedef struct pmx_strand_hits { int64_t n_hits, n_passing; pmx_pair_t *pairs; int64_t *index; pmx_record_t *recs; pmx_stats_t *stats; uint8_t *strand; } pmx_strand_hits_t;
int  pmx_search_pairs_stranded(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                               const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int strand_mode, pmx_strand_hits_t **result);
void pmx_strand_hits_free(pmx_strand_hits_t *hits);
/* Per-query top-K with a strand mode: the argument list of pmx_search_topk_device, then strand_mode and d_hit_strand (optional, one
 * byte per written hit).  skip_self is unchanged: (i, i) is never a candidate, on either strand.  PMX_STRAND_FORWARD is byte-identical
 * to pmx_search_topk_device.  The hit pairs and strand bytes feed pmx_align_pairs_ex_device as above.  The host result is a
 * pmx_topk_strand_hits_t: the fields of pmx_topk_hits_t followed by the strand bytes, released with pmx_topk_strand_hits_free. */
int pmx_search_topk_stranded_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                    int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                    pmx_pair_t *d_hit_pairs /* optional */, int64_t *d_hit_index /* optional */,
                                    pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats /* iff PMX_WANT_STATS */, int64_t capacity,
                                    int64_t *d_row_off /* nq + 1 */, int64_t *d_row_passing /* nq, optional */,
                                    int64_t *d_counts /* [0] kept, [1] written, [2] passing */, void *stream, const pmx_pairs_opts_t *opts,
                                    int strand_mode, uint8_t *d_hit_strand /* optional */);
typedef struct pmx_topk_strand_hits { int64_t n_rows, n_hits, n_passing; int64_t *row_off, *row_passing; pmx_pair_t *pairs; int64_t *index; pmx_record_t *recs; pmx_stats_t *stats; uint8_t *strand; } pmx_topk_strand_hits_t;
int  pmx_search_topk_stranded(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                              const pmx_topk_opts_t *opts, int strand_mode, pmx_topk_strand_hits_t **result);
void pmx_topk_strand_hits_free(pmx_topk_strand_hits_t *hits);

/* Translated set search (extension): nucleotide queries against a protein set, the query window translated in up to six frames
 * inside its chunk and the frames' records folded to one BEFORE selection, so hits, counts, top-K cuts and device memory are per
 * pair, not per (pair, frame).  Nothing below the gather changes: the alignment kernels see protein against protein.
 *
 * Genetic code.  pmx_genetic_code_table exports the standard code (NCBI table 1) in NCBI order: index = 16 b0 + 4 b1 + b2 with
 * T = 0, C = 1, A = 2, G = 3, "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG".  A base is one of "ACGTU" or
 * "acgtu", U reads as T; a codon holding any other byte translates to 'X', a stop to '*'; output letters are upper case.  `code`
 * (every translated entry; a host pointer, read during the call) carries a caller's own 64 letters in the same order, written as
 * they are; NULL: the standard code.  One genetic code per call.
 *
 * Frames.  One byte f.  f = 0, 1, 2: the query window as stored, read from offset off = f.  f = 3, 4, 5: the query window
 * reverse-complemented exactly as the _ex entries define it (pmx_complement_table, then reversed), read from offset off = f - 3.
 * Any other byte is a bad descriptor.  With W the window's length in nucleotides the translated query has L = (W - off) / 3 letters
 * (integer division; 0 for W < off); letter p is the codon at positions off + 3 p .. off + 3 p + 2 of that (possibly
 * reverse-complemented) window.  A frame with L = 0 does not exist for the pair.  The reference window is never translated.
 * ALL POSITIONS OF A RECORD (end_query, begins of a CIGAR pass) ARE IN LETTERS OF THE TRANSLATED QUERY.  Back to stored bytes:
 * letter p of a forward frame is sequence bytes q_beg + off + 3 p .. q_beg + off + 3 p + 2; letter p of a reverse frame is sequence
 * bytes q_beg + W - 1 - (off + 3 p) downwards (three bytes, complemented).  max_qlen of the device entries bounds L -- what the
 * alignment kernels see -- so the nucleotide window may be up to 3 max_qlen + 2 bytes; a frame of the call's mode whose L exceeds
 * max_qlen makes the pair bad.
 *
 * Frame modes.  0 .. 5: that one frame for every pair, one alignment slot.  PMX_FRAMES_FORWARD / _REVERSE / _ALL: the best of
 * frames 0 1 2 / 3 4 5 / all six, 3 / 3 / 6 slots per pair.  Fold rule: among the frames that exist for the pair the highest score
 * wins, only the score is compared, a tie goes to the lowest frame number.  The folded record is the winner's record BYTE FOR BYTE,
 * flags included, the statistics are the winner's, one frame byte says which frame won.  A pair with no existing frame, or a bad
 * descriptor, gets {0, -1, -1, PMX_FLAG_BAD_PAIR}, zero statistics and frame 0.  Selection (min_score, max_hits, capacity) and the
 * top-K order (score descending, reference index ascending) work on folded records; the frame is not part of the key, so a
 * reference appears at most once in a row and row_passing counts pairs.  chunk_pairs, slice_pairs and slice_rows count logical
 * pairs or rows and never change a byte; outputs are bit-identical from run to run.
 *
 * The defining equivalence.  In a single-frame mode every output of a translated entry is byte-identical to the corresponding
 * untranslated entry (pmx_align_pairs_device, pmx_search_pairs_device, pmx_search_topk_device) over a query set whose sequences
 * were translated on the host in that frame (whole-sequence descriptors; a window: against the translated window).  In a
 * multi-frame mode every output equals the fold rule applied to the single-frame results.
 *
 * Refused with -1 and a pmx_last_error() text before any GPU work: a frame mode outside the defined values; a PSSM matrix;
 * PMX_WANT_CIGAR (the CIGAR route: pmx_gather_pairs_translated_device over the pairs and their frame bytes, then
 * pmx_align_batch_cigar_device over the packed buffers); everything the corresponding untranslated entry refuses, with the same
 * texts.  n == 0 behaves as it does there.  The host entries name the first pair that is bad or has no frame.
 *
 * Scratch.  The chunk buffers hold `slots` windows per pair (1, 3 or 6; the default chunk holds that many fewer pairs), and per
 * pair of a chunk 46 bytes per slot, 16 (+ 12 with statistics) per slot for the slots' records in the search entries, and one
 * validity byte.  pmx_last_kernel() names what the last chunk's alignment ran. */
#define PMX_FRAMES_FORWARD 6   /* the best of frames 0, 1, 2 */
#define PMX_FRAMES_REVERSE 7   /* the best of frames 3, 4, 5 */
#define PMX_FRAMES_ALL     8   /* the best of all six */
void pmx_genetic_code_table(uint8_t table[64]);
/* Building block, test hook and the CIGAR route: pmx_gather_pairs_device with the query windows translated.  d_frame: one frame
 * byte per pair (NULL: all frame 0).  d_qout receives the translated query windows, d_rout the reference windows, packed back to
 * back; d_qoff / d_roff receive n + 1 offsets from 0; a window whose end would cross its capacity is not written; a pair that is
 * bad or whose frame does not exist has a one-zero-byte placeholder on either side and d_ok[k] = 0.  No byte outside a set's buffer
 * is read.  Asynchronous on `stream`. */
int pmx_gather_pairs_translated_device(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                                       const uint8_t *d_frame, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                       uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                                       uint8_t *d_ok /* n validity bytes, optional */, void *stream);
/* Listed pairs.  d_frame / frame: a frame byte per pair (then frame_mode must be 0), or NULL and a frame mode for all pairs.
 * d_frame_out / frame_out (n bytes; required in a multi-frame mode, else optional): the frame of every record. */
int pmx_align_pairs_translated_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                      int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_frame, int frame_mode, const uint8_t *code,
                                      int32_t max_qlen, int32_t max_rlen,
                                      pmx_record_t *d_out, pmx_stats_t *d_stats_out, uint8_t *d_frame_out, void *stream,
                                      const pmx_pairs_opts_t *opts);
int pmx_align_pairs_translated(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                               int64_t n, const pmx_pair_t *pairs, const uint8_t *frame, int frame_mode, const uint8_t *code,
                               pmx_record_t *out, pmx_stats_t *stats_out /* NULL unless WANT_STATS */, uint8_t *frame_out,
                               const pmx_pairs_opts_t *opts);
/* Set search and per-query top-K: the argument lists of the stranded entries with frame_mode, code and d_hit_frame (optional, one
 * byte per written hit) in place of the strand arguments.  The hit descriptors stay valid d_pairs: with the frame bytes they feed
 * pmx_gather_pairs_translated_device.  The host results are laid out like pmx_strand_hits_t / pmx_topk_strand_hits_t with `frame`
 * bytes, one block each, released with their own free functions. */
int pmx_search_pairs_translated_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                       int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                                       int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                       pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                       int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts,
                                       int frame_mode, const uint8_t *code, uint8_t *d_hit_frame /* optional */);
typedef struct pmx_frame_hits { int64_t n_hits, n_passing; pmx_pair_t *pairs; int64_t *index; pmx_record_t *recs; pmx_stats_t *stats; uint8_t *frame; } pmx_frame_hits_t;
int  pmx_search_pairs_translated(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                                 const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int frame_mode, const uint8_t *code,
                                 pmx_frame_hits_t **result);
void pmx_frame_hits_free(pmx_frame_hits_t *hits);
int pmx_search_topk_translated_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                      int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                      pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                      int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                                      void *stream, const pmx_pairs_opts_t *opts,
                                      int frame_mode, const uint8_t *code, uint8_t *d_hit_frame /* optional */);
typedef struct pmx_topk_frame_hits { int64_t n_rows, n_hits, n_passing; int64_t *row_off, *row_passing; pmx_pair_t *pairs; int64_t *index; pmx_record_t *recs; pmx_stats_t *stats; uint8_t *frame; } pmx_topk_frame_hits_t;
int  pmx_search_topk_translated(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                const pmx_topk_opts_t *opts, int frame_mode, const uint8_t *code, pmx_topk_frame_hits_t **result);
void pmx_topk_frame_hits_free(pmx_topk_frame_hits_t *hits);

/* Frameshift-aware translated search (extension): nucleotide queries against a protein set, aligned by a three-frame local DP so
 * that one alignment may change its reading frame.  The translated entries above align every frame on its own: one inserted or
 * deleted nucleotide cuts an alignment in two and the fold keeps the better half.  Here a path may step over two or four nucleotides
 * instead of three, at the price of a penalty `frameshift`.  The pipeline around the kernel is the one of the stranded entries.
 *
 * Q holds nucleotides and R holds proteins.  The genetic code, the base classes and the `code` argument are those of the translated
 * entries above.
 *
 * The codon stream.  A query window of W nucleotides is read as stored (strand 0) or reverse-complemented exactly as the _ex entries
 * define it (strand 1: pmx_complement_table, then reversed): the oriented window.  Its codon stream T has N = W - 2 letters; T[i] is
 * the translation of oriented bytes i, i + 1, i + 2.  Rows i = f, f + 3, f + 6, .. of T are exactly frame f (strand 0) or frame 3 + f
 * (strand 1) of the translated entries.  A window with W < 3 has no stream: the pair is treated as a pair without an existing frame
 * is there -- the bad record {0, -1, -1, PMX_FLAG_BAD_PAIR}, strand 0.
 *
 * The recurrence.  Local alignment only.  Rows i = 0 .. N - 1 of T, columns j = 0 .. m - 1 of reference r, s the matrix score, open
 * and extend the call's gap penalties (a gap of length g costs open + (g - 1) extend), fs = frameshift >= 0:
 *     D(i,j) = max(0, H(i-3,j-1), H(i-2,j-1) - fs, H(i-4,j-1) - fs)
 *     M(i,j) = D(i,j) + s(T[i], r[j])
 *     E(i,j) = max(H(i,j-1) - open, E(i,j-1) - extend)          a reference letter against a gap
 *     F(i,j) = max(H(i-3,j) - open, F(i-3,j) - extend)          a whole codon against a gap
 *     H(i,j) = max(0, M, E, F)
 * A term with a negative index does not exist: for H it counts as 0, for E and F as minus infinity.  The i - 2 predecessor is a path
 * that found one nucleotide missing from the read, the i - 4 predecessor one nucleotide too many; gaps keep their frame.  With the
 * two frameshift terms taken out, the score is the best plain local score over T[0::3], T[1::3] and T[2::3]: the
 * PMX_FRAMES_FORWARD (strand 1: PMX_FRAMES_REVERSE) fold of the translated entries, which a large `frameshift` therefore returns.
 *
 * The record.  score = the maximum H; end_ref = its j; end_query = its i + 2, THE LAST NUCLEOTIDE OF THE LAST CODON, 0-BASED
 * INCLUSIVE, IN THE ORIENTED WINDOW -- IN NUCLEOTIDES, UNLIKE THE TRANSLATED ENTRIES, WHOSE POSITIONS ARE LETTERS.  Back to stored
 * bytes: oriented byte x of a strand-0 window is sequence byte q_beg + x, of a strand-1 window sequence byte q_beg + W - 1 - x
 * (complemented).  Ties: the first maximum in column-major order, that is the smallest end_ref, then the smallest end_query; a zero
 * maximum therefore ends at end_query 2, end_ref 0.  flags = 0.
 *
 * Strand modes.  PMX_STRAND_FORWARD, PMX_STRAND_REVERSE and PMX_STRAND_BOTH mean what they mean for the stranded entries: one or two
 * alignment slots per pair, the better strand kept BEFORE the threshold and the top-K cut (only the score is compared, a tie goes to
 * the forward strand), the strand byte beside each record or hit.  The listed-pairs entry also takes one strand byte per pair
 * (d_strand / strand; the strand mode must then be PMX_STRAND_FORWARD; a byte above 1 makes the pair bad).  chunk_pairs, slice_pairs
 * and slice_rows count logical pairs or rows and never change a byte; outputs are bit-identical from run to run.
 *
 * Limits.  cfg->mode PMX_MODE_SW; cfg->width 0 or 32, both exact: the kernel computes in 32 bits, and open, extend and frameshift
 * above 2^28 are read as 2^28, which is above every score a window can reach, so nothing wraps.  Windows of up to
 * PMX_FRAMESHIFT_MAX_WINDOW nucleotides.  max_qlen of the device entries bounds N = W - 2, the rows the kernel sees; a window whose N
 * exceeds max_qlen makes the pair bad.  The host entries size max_qlen from the longest window.
 *
 * Refused with -1 and a pmx_last_error() text before any GPU work: any other mode or width; PMX_WANT_STATS and PMX_WANT_CIGAR (these
 * entries have no traceback with frameshift operators: the _frameshift_cigar entries below are the pass that has); a PSSM matrix; a matrix of more than 128 symbols; frameshift < 0; a strand mode outside
 * 0 .. 2; strand bytes per pair together with a strand mode other than PMX_STRAND_FORWARD; max_qlen above
 * PMX_FRAMESHIFT_MAX_WINDOW - 2 (host entries: a window above PMX_FRAMESHIFT_MAX_WINDOW); everything the corresponding stranded or
 * untranslated entry refuses, with the same texts.  n == 0 / nq == 0 behave as there.  The host entries name the first pair that is
 * bad or has no stream.
 *
 * Scratch.  The chunk buffers of the stranded entries with N + m bytes per slot, 16 bytes of slot record per slot and, for windows of
 * more than 162 nucleotides, 64 bytes per reference column and slot for the strips' boundary columns, at most 256 MiB of them (the
 * kernel then runs over a chunk's slots in parts).  pmx_last_kernel() names the instantiation of the last chunk's alignment. */
#define PMX_FRAMESHIFT_MAX_WINDOW 4096
int32_t pmx_frameshift_max_window(void);            /* PMX_FRAMESHIFT_MAX_WINDOW of the library loaded */
/* Building block and test hook: pmx_gather_pairs_translated_device in its stride-1 form, with d_strand (one strand byte per pair;
 * NULL: all forward) in place of d_frame.  d_qout receives the codon streams (W - 2 letters each), d_rout the reference windows;
 * max_qlen bounds W - 2.  A pair that is bad or has W < 3 has a one-zero-byte placeholder on either side and d_ok[k] = 0.  No byte
 * outside a set's buffer is read.  Asynchronous on `stream`. */
int pmx_gather_pairs_codons_device(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                                   const uint8_t *d_strand, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                   uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                                   uint8_t *d_ok /* n validity bytes, optional */, void *stream);
/* Listed pairs.  d_strand / strand: a strand byte per pair (then strand_mode must be PMX_STRAND_FORWARD), or NULL and a strand mode
 * for all pairs.  d_strand_out / strand_out (n bytes; required with PMX_STRAND_BOTH, else optional): the strand of every record.
 * The device entry gives bad pairs their record and strand 0; the host entry refuses them, naming the first. */
int pmx_align_pairs_frameshift_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                      int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                      int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                      pmx_record_t *d_out, uint8_t *d_strand_out, void *stream, const pmx_pairs_opts_t *opts);
int pmx_align_pairs_frameshift(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                               int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                               int32_t frameshift, const uint8_t *code,
                               pmx_record_t *out, uint8_t *strand_out, const pmx_pairs_opts_t *opts);
/* Set search and per-query top-K: the argument lists of the stranded entries, then frameshift and code.  d_hit_stats must be NULL.
 * The hit descriptors stay valid d_pairs: with the strand bytes they feed pmx_align_pairs_frameshift_device and
 * pmx_gather_pairs_codons_device.  The host results are pmx_strand_hits_t / pmx_topk_strand_hits_t, released with their free
 * functions. */
int pmx_search_pairs_frameshift_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                       int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                                       int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                       pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                       int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts,
                                       int strand_mode, uint8_t *d_hit_strand /* optional */, int32_t frameshift, const uint8_t *code);
int pmx_search_pairs_frameshift(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                                const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int strand_mode,
                                int32_t frameshift, const uint8_t *code, pmx_strand_hits_t **result);
int pmx_search_topk_frameshift_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                      int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                      pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                      int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                                      void *stream, const pmx_pairs_opts_t *opts,
                                      int strand_mode, uint8_t *d_hit_strand /* optional */, int32_t frameshift, const uint8_t *code);
int pmx_search_topk_frameshift(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                               const pmx_topk_opts_t *opts, int strand_mode, int32_t frameshift, const uint8_t *code,
                               pmx_topk_strand_hits_t **result);

/* Frameshift traceback (extension): the alignment behind a frameshift record -- CIGAR text with frameshift operators, the begin of the
 * path, and statistics -- as a second pass over listed pairs, typically the hit pairs and strand bytes a frameshift search returned
 * (the hit list is the interface, as for every other search here).  The recurrence, the codon stream, the record, the strand rules
 * and the limits are those of the section above; records and strand bytes are byte-identical to pmx_align_pairs_frameshift[_device].
 * New is the path.  It is deterministic and follows the precedence of the project's other tracebacks, carried over to the wider
 * recurrence.
 *
 * Decisions at cell (i, j).
 *   H source.  If M >= E and M >= F the source is M; otherwise if F >= E it is F; otherwise it is E.  If the resulting H <= 0 the cell
 *     is ZERO: H = 0 and no path passes through it.
 *   D source (where the H source is M).  With h3 = H(i-3,j-1), h2 = H(i-2,j-1) - fs, h4 = H(i-4,j-1) - fs, D = max(0, h3, h2, h4):
 *     START if D == 0 (zero wins every tie: a path never begins with a frameshift that buys nothing); otherwise IN-FRAME if h3 == D;
 *     otherwise SHORT (2 rows) if h2 == D; otherwise LONG (4 rows).  Terms with a negative index are 0 for H, as in the recurrence.
 *   E opened iff H(i,j-1) - open > E(i,j-1) - extend, strictly; otherwise it is extended.
 *   F opened iff H(i-3,j) - open > F(i-3,j) - extend, strictly.
 *
 * The walk starts at cell (end_query - 2, end_ref) in state H.
 *   State H, M source: emit a match column -- '=' if the two letters map to the same matrix index, otherwise 'X' -- then: START: the
 *     path begins at this cell, stop; IN-FRAME: go to (i-3, j-1); SHORT: emit '/' and go to (i-2, j-1); LONG: emit '\' and go to
 *     (i-4, j-1).
 *   State H, F source / E source: switch to state F / E at the same cell.
 *   State F at (i, j): emit one codon-against-gap op and go to (i-3, j); the state becomes H if F(i, j) was opened, else stays F.
 *   State E at (i, j): emit one reference-letter-against-gap op and go to (i, j-1); the state becomes H if E(i, j) was opened.
 *
 * The text is in path order from begin to end, run-length encoded as <count><op> like every CIGAR here.  '=' and 'X' stand for one
 * codon against one reference letter.  The codon-gap op is the letter of the F / DEL state and the reference-gap op the letter of the
 * E / INS state: 'I' and 'D' by default, following PMX_CIGAR_SWAP_ID (pmx_conventions.h).  '/' means one nucleotide is missing from
 * the read -- the next codon overlaps the previous one by one base; '\' means one nucleotide too many.  A frameshift op sits directly
 * in front of the match column it leads into; two of them are never adjacent, so their count is always 1.
 * UNITS: '=', 'X' AND THE CODON-GAP OP CONSUME THREE QUERY NUCLEOTIDES; '/' TAKES ONE BACK; '\' ADDS ONE.  '=', 'X' AND THE
 * REFERENCE-GAP OP CONSUME ONE REFERENCE LETTER.
 *
 * Begins.  beg[2k] = beg_query is the first nucleotide of the first codon -- row i of the START cell -- in the oriented window,
 * beg[2k+1] = beg_ref its column.  A zero-score record has an empty text and begins (end_query + 1, end_ref + 1) = (3, 1), what the
 * other local walks report for an empty path.  A bad pair has the bad record, strand 0, an empty text, begins -1 / -1 and zero
 * statistics; its neighbours are unaffected.
 *
 * Statistics (pmx_stats_t).  matches = the number of '=' columns; similar = the number of match columns with a positive matrix score;
 * length = match columns + gap columns, a codon gap counting 1.  Frameshift ops are not columns.
 *
 * What follows, for every non-empty text:
 *   - its first and its last op are match columns;
 *   - end_query - beg_query + 1 == 3 (match columns + codon gaps) - #'/' + #'\';
 *   - end_ref - beg_ref + 1 == match columns + reference gaps;
 *   - re-scoring the text from (beg_query, beg_ref) -- matrix scores, open / extend per gap run of one kind, fs per frameshift op --
 *     gives exactly the record's score and end cell;
 *   - it has at most N + m ops.
 *
 * cfg->want must hold PMX_WANT_CIGAR, optionally with PMX_WANT_STATS (here the two may be combined: one walk produces both); the
 * statistics buffer is present iff PMX_WANT_STATS is set.  Everything else is refused as pmx_align_pairs_frameshift[_device] refuses
 * it, with the same texts, before any GPU work.  Strand modes and strand bytes are those of the score entry; with PMX_STRAND_BOTH both
 * strands are swept and the walk runs over the winner's trace.  d_beg (2 n) is optional.  The text buffer follows
 * pmx_align_pairs_ex_device: offsets start at 0, d_cigar_off[n] is the number of bytes needed, a pair whose text would cross
 * cigar_capacity is not written, chunk_pairs never changes a byte; the host entry sizes the buffer, runs once more at the exact size
 * if the text did not fit, and *cigar_buf is released with pmx_free.
 *
 * Scratch.  Beside the score entry's: 192 bytes of trace per reference column and strip of 160 rows for each slot, bounded at 256 MiB
 * per chunk (the value switch PMX_CIGAR_CHUNK_BYTES sets another bound): a chunk whose slots need more runs in parts, sweep then walk,
 * and no byte of any output depends on the parts.  A call in which four slots -- one workgroup -- exceed the bound is refused before
 * any GPU work.  pmx_last_kernel() names the trace instantiation of the last part, with "/strips" for windows beyond 162 nucleotides. */
int pmx_align_pairs_frameshift_cigar_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                            int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                            int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                            pmx_record_t *d_out, uint8_t *d_strand_out, pmx_stats_t *d_stats /* iff PMX_WANT_STATS */,
                                            int32_t *d_beg /* 2 n, optional */,
                                            char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off /* n + 1 */,
                                            void *stream, const pmx_pairs_opts_t *opts);
int pmx_align_pairs_frameshift_cigar(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                     int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                                     int32_t frameshift, const uint8_t *code,
                                     pmx_record_t *out, uint8_t *strand_out, pmx_stats_t *stats_out /* iff PMX_WANT_STATS */,
                                     int32_t *beg /* 2 n, optional */, char **cigar_buf, int64_t *cigar_off /* n + 1 */,
                                     const pmx_pairs_opts_t *opts);

/* Reference-side translation (extension): protein queries against a set of nucleotide sequences -- genes, transcripts, contigs --,
 * the tblastn pairing.  The text above holds with the sides exchanged; what follows states it in full.
 *
 * Q holds proteins and R holds nucleotides.  The genetic code, the `code` argument, the base classes ("ACGTUacgtu"; any other byte in
 * a codon gives 'X'; stops give '*'), the tables and the frame modes (0 .. 5, PMX_FRAMES_FORWARD / _REVERSE / _ALL) are the ones
 * above.  Frame f = 0, 1, 2 reads the REFERENCE window as stored, from offset off = f; f = 3, 4, 5 reads the reference window
 * reverse-complemented as pmx_complement_table defines it (complemented, then reversed), from offset off = f - 3.  A window of W
 * nucleotides has L = (W - off) / 3 letters (integer division; 0 for W < off); a frame with L = 0 does not exist for the pair.
 * max_rlen bounds L -- what the alignment kernels see -- so the nucleotide window may be up to 3 max_rlen + 2 bytes; a frame of the
 * call's mode with L > max_rlen makes the pair bad.  The query window is bounded by max_qlen as in the untranslated entries and is
 * never translated: no entry takes two frame arguments.
 * ALL POSITIONS OF A RECORD (end_ref, begins of a CIGAR pass) ARE IN LETTERS OF THE TRANSLATED REFERENCE.  Back to stored bytes:
 * letter p of a forward frame is sequence bytes r_beg + off + 3 p .. r_beg + off + 3 p + 2; letter p of a reverse frame is sequence
 * bytes r_beg + W - 1 - (off + 3 p) downwards (three bytes, complemented).
 *
 * The fold rule is the one above: among the frames that exist the highest score wins, only the score is compared, a tie goes to the
 * lowest frame; record and statistics are the winner's, byte for byte; no frame, or a bad descriptor: {0, -1, -1,
 * PMX_FLAG_BAD_PAIR}, zero statistics, frame 0.  Selection, the counts and the top-K order (score descending, reference index
 * ascending) work on folded records, so a reference appears at most once in a row.  The frame byte of a record or hit names the
 * REFERENCE's frame.
 *
 * The defining equivalence.  In a single-frame mode every output is byte-identical to the corresponding untranslated entry
 * (pmx_align_pairs_device, pmx_search_pairs_device, pmx_search_topk_device) over a reference set whose sequences -- for a windowed
 * descriptor: whose window -- were translated on the host in that frame.  In a multi-frame mode every output equals the fold rule
 * applied to the single-frame results.
 *
 * Refused with -1 and a pmx_last_error() text before any GPU work: a frame mode outside 0 .. 8; a frame byte per pair together with
 * a frame mode other than 0; a PSSM matrix (it would belong to the protein query, but the batch PSSM forms are not wired through
 * these entries); PMX_WANT_CIGAR (the CIGAR route: hit pairs + frame bytes -> pmx_gather_pairs_translated_ref_device ->
 * pmx_align_batch_cigar_device); a multi-frame mode without a frame output (the device search entries: with capacity > 0);
 * everything the corresponding untranslated entry refuses, with the same texts.  The host entries size max_rlen from the longest
 * nucleotide reference window and name the first pair that is bad or has no frame.
 *
 * The argument lists are those of the _translated entries; d_frame / frame_mode / d_frame_out / d_hit_frame speak of the reference's
 * frame; the result blocks pmx_frame_hits_t and pmx_topk_frame_hits_t and their free functions are reused.
 * pmx_gather_pairs_translated_ref_device: d_qout receives the query windows as they are, d_rout the translated reference windows. */
int pmx_gather_pairs_translated_ref_device(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                                           const uint8_t *d_frame, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                           uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                                           uint8_t *d_ok /* n validity bytes, optional */, void *stream);
int pmx_align_pairs_translated_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                          int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_frame, int frame_mode, const uint8_t *code,
                                          int32_t max_qlen, int32_t max_rlen,
                                          pmx_record_t *d_out, pmx_stats_t *d_stats_out, uint8_t *d_frame_out, void *stream,
                                          const pmx_pairs_opts_t *opts);
int pmx_align_pairs_translated_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                   int64_t n, const pmx_pair_t *pairs, const uint8_t *frame, int frame_mode, const uint8_t *code,
                                   pmx_record_t *out, pmx_stats_t *stats_out /* NULL unless WANT_STATS */, uint8_t *frame_out,
                                   const pmx_pairs_opts_t *opts);
int pmx_search_pairs_translated_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                           int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                                           int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                           pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                           int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts,
                                           int frame_mode, const uint8_t *code, uint8_t *d_hit_frame);
int pmx_search_pairs_translated_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                                    const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int frame_mode, const uint8_t *code,
                                    pmx_frame_hits_t **result);
int pmx_search_topk_translated_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                          int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                          pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                          int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                                          void *stream, const pmx_pairs_opts_t *opts,
                                          int frame_mode, const uint8_t *code, uint8_t *d_hit_frame);
int pmx_search_topk_translated_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                   const pmx_topk_opts_t *opts, int frame_mode, const uint8_t *code, pmx_topk_frame_hits_t **result);

/* Frameshift-aware translated search, reference side (extension): protein queries against a set of nucleotide sequences -- genes,
 * transcripts, contigs -- aligned by the three-frame local DP, so that one alignment may change its reading frame: tblastn with
 * frameshifts.  The reference-side translated entries above align every frame on its own, and one inserted or deleted base in a
 * contig cuts a hit in two.  Exchanging the sets and calling the query-side frameshift entries transposes the records, turns the
 * per-query top-K into "best proteins per contig" and bounds the nucleotide side by PMX_FRAMESHIFT_MAX_WINDOW.  Here the nucleotide
 * reference is streamed one letter per step AT ANY LENGTH and the protein sits on the rows.
 *
 * Q holds proteins and R holds nucleotides.  The genetic code, the base classes and the `code` argument are those of the translated
 * entries.
 *
 * The codon stream.  A REFERENCE window of W nucleotides is read as stored (strand 0) or reverse-complemented (strand 1) exactly as
 * frames 3 .. 5 of the reference-side translated entries read it (pmx_complement_table, from the window's end downwards): the
 * oriented window.  Its codon stream T has N = W - 2 letters; T[j] is the translation of oriented bytes j, j + 1, j + 2.  Columns
 * j = f, f + 3, f + 6, .. of T are exactly frame f (strand 0) or frame 3 + f (strand 1) of the reference-side translated entries.  A
 * window with W < 3 has no stream: the pair gets the bad record {0, -1, -1, PMX_FLAG_BAD_PAIR} and strand 0.
 *
 * The recurrence.  Local alignment only.  Rows i = 0 .. m - 1 of the query protein q, columns j = 0 .. N - 1 of T, s the matrix
 * score INDEXED (QUERY LETTER, REFERENCE LETTER), open and extend the call's gap penalties, fs = frameshift >= 0:
 *     D(i,j) = max(0, H(i-1,j-3), H(i-1,j-2) - fs, H(i-1,j-4) - fs)
 *     M(i,j) = D(i,j) + s(q[i], T[j])
 *     E(i,j) = max(H(i,j-3) - open, E(i,j-3) - extend)          a whole reference codon against a gap
 *     F(i,j) = max(H(i-1,j) - open, F(i-1,j) - extend)          a query letter against a gap
 *     H(i,j) = max(0, M, E, F)
 * A term with a negative index does not exist: for H it counts as 0, for E and F as minus infinity.  The j - 2 predecessor is a path
 * that found one nucleotide missing from the reference, the j - 4 predecessor one nucleotide too many; gaps keep their frame.
 * Two identities follow.  (1) The recurrence is the transpose of the query-side one: the score equals the query-side score of the
 * same stream with the roles exchanged and the matrix transposed; only the end cell may differ, by the tie rule.  (2) With the two
 * frameshift terms taken out, the score is the best plain local score over T[0::3], T[1::3] and T[2::3]: the PMX_FRAMES_FORWARD
 * (strand 1: PMX_FRAMES_REVERSE) fold of the reference-side translated entries, which a large `frameshift` therefore returns.
 *
 * The record.  score = the maximum H; end_query = its i, in letters; end_ref = its j + 2, THE LAST NUCLEOTIDE OF THE LAST CODON,
 * 0-BASED INCLUSIVE, IN THE ORIENTED REFERENCE WINDOW -- IN NUCLEOTIDES.  Back to stored bytes: oriented byte x of a strand-0 window
 * is sequence byte r_beg + x, of a strand-1 window sequence byte r_beg + W - 1 - x (complemented).  Ties: the first maximum in
 * column-major order, that is the smallest end_ref, then the smallest end_query; a zero maximum therefore ends at end_query 0,
 * end_ref 2.  flags = 0.
 *
 * Strand modes.  PMX_STRAND_FORWARD, PMX_STRAND_REVERSE and PMX_STRAND_BOTH behave as for the stranded and the query-side frameshift
 * entries, but THE STRAND IS THE REFERENCE'S: one or two alignment slots per pair, the better strand kept BEFORE the threshold and
 * the top-K cut (only the score is compared, a tie goes to the forward strand), the strand byte beside each record or hit.  The
 * listed-pairs entry also takes one strand byte per pair (the strand mode must then be PMX_STRAND_FORWARD; a byte above 1 makes the
 * pair bad).  chunk_pairs, slice_pairs and slice_rows never change a byte; outputs are bit-identical from run to run.
 *
 * Limits.  cfg->mode PMX_MODE_SW; cfg->width 0 or 32, both exact: the kernel computes in 32 bits, and open, extend and frameshift
 * above 2^28 are read as 2^28.  Query windows of up to PMX_FRAMESHIFT_REF_MAX_QUERY letters: 4 096 x 32 767 < 2^28, so nothing wraps
 * however long the reference is.  REFERENCE WINDOWS HAVE NO CAP OF THEIR OWN: max_rlen of the device entries bounds N = W - 2, the
 * columns the kernel sees, and a window whose N exceeds it makes the pair bad; max_qlen bounds the query window as in the untranslated
 * entries.  The host entries size both from the longest windows.
 *
 * Refused with -1 and a pmx_last_error() text before any GPU work: any other mode or width; PMX_WANT_STATS and PMX_WANT_CIGAR (these
 * entries have no traceback; the hit list is the interface for the pass that has: the _frameshift_ref_cigar entries below); a PSSM matrix; a matrix of more than 128
 * symbols; frameshift < 0; a strand mode outside 0 .. 2; strand bytes per pair together with a strand mode other than
 * PMX_STRAND_FORWARD; max_qlen above PMX_FRAMESHIFT_REF_MAX_QUERY; a device search with PMX_STRAND_BOTH, capacity > 0 and no strand
 * output; everything the corresponding stranded or untranslated entry refuses, with the same texts.  n == 0 / nq == 0 behave as
 * there.  The device entries give bad pairs their record and strand 0; the host entries name the first pair that is bad or has no
 * stream.
 *
 * Scratch.  The chunk buffers of the stranded entries with m + N bytes per slot (two slots per pair in PMX_STRAND_BOTH), 16 bytes of
 * slot record per slot and, for queries of more than pmx_swfsc_strip_rows() letters, 16 bytes per reference column and slot for the
 * strips' boundary rows, at most 256 MiB of them (the kernel then runs over a chunk's slots in parts).  pmx_last_kernel() names the
 * instantiation of the last chunk's alignment, with "/strips" for queries beyond one strip.
 *
 * The argument lists are those of the query-side frameshift entries; d_strand / strand_mode / d_strand_out / d_hit_strand speak of
 * the reference's strand; the result blocks pmx_strand_hits_t and pmx_topk_strand_hits_t and their free functions are reused.  Hit
 * descriptors plus strand bytes are valid input to the listed entry and to the gather hook.
 * pmx_gather_pairs_codons_ref_device: pmx_gather_pairs_codons_device with the sides exchanged -- d_qout receives the query windows as
 * they are, d_rout the reference windows' codon streams (W - 2 letters each), d_strand applies to R, max_rlen bounds W - 2. */
#define PMX_FRAMESHIFT_REF_MAX_QUERY 4096
int32_t pmx_frameshift_ref_max_query(void);         /* PMX_FRAMESHIFT_REF_MAX_QUERY of the library loaded */
int pmx_gather_pairs_codons_ref_device(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                                       const uint8_t *d_strand, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                       uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                                       uint8_t *d_ok /* n validity bytes, optional */, void *stream);
int pmx_align_pairs_frameshift_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                          int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                          int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                          pmx_record_t *d_out, uint8_t *d_strand_out, void *stream, const pmx_pairs_opts_t *opts);
int pmx_align_pairs_frameshift_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                   int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                                   int32_t frameshift, const uint8_t *code,
                                   pmx_record_t *out, uint8_t *strand_out, const pmx_pairs_opts_t *opts);
int pmx_search_pairs_frameshift_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                           int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                                           int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                           pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                           int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts,
                                           int strand_mode, uint8_t *d_hit_strand, int32_t frameshift, const uint8_t *code);
int pmx_search_pairs_frameshift_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                                    const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int strand_mode,
                                    int32_t frameshift, const uint8_t *code, pmx_strand_hits_t **result);
int pmx_search_topk_frameshift_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                          int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                          pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                          int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                                          void *stream, const pmx_pairs_opts_t *opts,
                                          int strand_mode, uint8_t *d_hit_strand, int32_t frameshift, const uint8_t *code);
int pmx_search_topk_frameshift_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                   const pmx_topk_opts_t *opts, int strand_mode, int32_t frameshift, const uint8_t *code,
                                   pmx_topk_strand_hits_t **result);
/* Test hooks of the kernel (parasail-rs_amd/csrc/pmx_swfsc.hip; model: tests/swfsc_model.c): the rows of one strip and of one lane,
 * the boundary scratch of one slot for streams of up to max_rlen letters, the largest matrix. */
int pmx_swfsc_strip_rows(void);
int pmx_swfsc_lane_rows(void);
long long pmx_swfsc_bound_bytes_per_slot(int max_rlen);
int pmx_swfsc_max_msize(void);

/* Frameshift traceback, reference side (extension): the alignment behind a reference-side frameshift record -- CIGAR text with
 * frameshift operators, the begin of the path, and statistics -- as a second pass over listed pairs, typically the hit pairs and strand
 * bytes a pmx_search_*_frameshift_ref search returned (the hit list is the interface).  It tells WHERE in a contig the frameshift is.
 * The recurrence, the codon stream, the record, the strand rules and the limits are those of "Frameshift-aware translated search,
 * reference side" above: rows i are the query protein's letters, columns j the letters of the oriented reference window's codon stream
 * T, s is indexed (query letter, stream letter); records and strand bytes are byte-identical to
 * pmx_align_pairs_frameshift_ref[_device].  New is the path.  It is deterministic and keeps the precedence of the query-side
 * "Frameshift traceback" section, state by state.
 *
 * Decisions at cell (i, j).
 *   H source.  If M >= E and M >= F the source is M; otherwise if F >= E it is F; otherwise it is E.  If the resulting H <= 0 the cell
 *     is ZERO: H = 0 and no path passes through it.
 *   D source (where the H source is M).  With h3 = H(i-1,j-3), h2 = H(i-1,j-2) - fs, h4 = H(i-1,j-4) - fs, D = max(0, h3, h2, h4):
 *     START if D == 0 (zero wins every tie); otherwise IN-FRAME if h3 == D; otherwise SHORT (2 columns) if h2 == D; otherwise LONG
 *     (4 columns).  Terms with a negative index are 0 for H, as in the recurrence.
 *   E opened iff H(i,j-3) - open > E(i,j-3) - extend, strictly; otherwise it is extended.
 *   F opened iff H(i-1,j) - open > F(i-1,j) - extend, strictly.
 *
 * The walk starts at cell (end_query, end_ref - 2) in state H.
 *   State H, M source: emit a match column -- '=' if the two letters map to the same matrix index, otherwise 'X' -- then: START: the
 *     path begins at this cell, stop; IN-FRAME: go to (i-1, j-3); SHORT: emit '/' and go to (i-1, j-2); LONG: emit '\' and go to
 *     (i-1, j-4).
 *   State H, F source / E source: switch to state F / E at the same cell.
 *   State F at (i, j): one query letter against a gap -- emit the query-gap op and go to (i-1, j); the state becomes H if F(i, j) was
 *     opened, else stays F.
 *   State E at (i, j): one whole reference codon against a gap -- emit the codon-gap op and go to (i, j-3); the state becomes H if
 *     E(i, j) was opened.
 *
 * The text is in path order from begin to end, run-length encoded as <count><op>.  '=' and 'X' stand for one query letter against one
 * reference codon.  The query-gap op is the letter of the F / DEL state and the codon-gap op the letter of the E / INS state: 'I' and
 * 'D' by default, following PMX_CIGAR_SWAP_ID (pmx_conventions.h) -- so 'I' is, as everywhere here, query material the reference lacks
 * and 'D' reference material the query lacks.  '/' means one nucleotide is missing from the reference -- the next codon overlaps the
 * previous one by one base; '\' means one nucleotide too many.  A frameshift op sits directly in front of the match column it leads
 * into; two of them are never adjacent, so their count is always 1.
 * UNITS: '=', 'X' AND THE CODON-GAP OP CONSUME THREE REFERENCE NUCLEOTIDES; '/' TAKES ONE BACK; '\' ADDS ONE.  '=', 'X' AND THE
 * QUERY-GAP OP CONSUME ONE QUERY LETTER.
 *
 * Begins.  beg[2k] = beg_query is the row of the START cell, in letters; beg[2k+1] = beg_ref its column: the first nucleotide of the
 * first codon in the oriented reference window.  A zero-score record has an empty text and begins (end_query + 1, end_ref + 1) =
 * (1, 3).  A bad pair has the bad record, strand 0, an empty text, begins -1 / -1 and zero statistics; its neighbours are unaffected.
 *
 * Statistics (pmx_stats_t).  matches = the number of '=' columns; similar = the number of match columns with a positive matrix score;
 * length = match columns + gap columns, a codon gap counting 1.  Frameshift ops are not columns.
 *
 * What follows, for every non-empty text:
 *   - its first and its last op are match columns;
 *   - end_query - beg_query + 1 == match columns + query gaps;
 *   - end_ref - beg_ref + 1 == 3 (match columns + codon gaps) - #'/' + #'\';
 *   - re-scoring the text from (beg_query, beg_ref) -- matrix scores, open / extend per gap run of one kind, fs per frameshift op --
 *     gives exactly the record's score and end cell;
 *   - it has at most m + N ops.
 *
 * cfg->want must hold PMX_WANT_CIGAR, optionally with PMX_WANT_STATS; the statistics buffer is present iff PMX_WANT_STATS is set.
 * Refused with -1 and the existing pmx_last_error() texts before any GPU work: everything pmx_align_pairs_frameshift_ref[_device]
 * refuses (max_qlen above PMX_FRAMESHIFT_REF_MAX_QUERY among it), everything the query-side traceback entries refuse about their
 * outputs, and a call in which four slots -- one workgroup -- exceed the bound on a chunk's trace.  The score and search entries of
 * this side keep refusing PMX_WANT_CIGAR.  Strand arguments speak of the REFERENCE's strand; with PMX_STRAND_BOTH both strands are
 * swept and the walk runs over the winner's trace.  d_beg (2 n) is optional.  The text buffer follows
 * pmx_align_pairs_frameshift_cigar[_device]: offsets start at 0, d_cigar_off[n] is the number of bytes needed, a pair whose text would
 * cross cigar_capacity is not written, chunk_pairs never changes a byte; the host entry sizes the text at 32 bytes per pair, runs once
 * more at the exact size if that was too little, and *cigar_buf is released with pmx_free.
 *
 * Scratch.  Beside the score entry's: 192 bytes of trace per step and strip of 160 query letters for each slot, a strip having
 * max_rlen + 15 steps -- pmx_swfsc_trace_bytes_per_slot(max_qlen, max_rlen), EVERY CELL OF THE m x N MATRIX, so the bound is what
 * limits a long reference -- bounded at 256 MiB per chunk (the value switch PMX_CIGAR_CHUNK_BYTES sets another bound): a chunk whose
 * slots need more runs in parts, sweep then walk, and no byte of any output depends on the parts.  pmx_last_kernel() names the trace
 * instantiation of the last part, "pmx_swfsc_kernel<16,10,trace>", with "/strips" for queries beyond one strip. */
int pmx_align_pairs_frameshift_ref_cigar_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                                int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                                pmx_record_t *d_out, uint8_t *d_strand_out, pmx_stats_t *d_stats /* iff PMX_WANT_STATS */,
                                                int32_t *d_beg /* 2 n, optional */,
                                                char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off /* n + 1 */,
                                                void *stream, const pmx_pairs_opts_t *opts);
int pmx_align_pairs_frameshift_ref_cigar(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                         int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                                         int32_t frameshift, const uint8_t *code,
                                         pmx_record_t *out, uint8_t *strand_out, pmx_stats_t *stats_out /* iff PMX_WANT_STATS */,
                                         int32_t *beg /* 2 n, optional */, char **cigar_buf, int64_t *cigar_off /* n + 1 */,
                                         const pmx_pairs_opts_t *opts);
/* Test hook: the trace scratch of one slot of the reference-side trace sweep for queries of up to max_qlen letters and streams of up
 * to max_rlen letters. */
long long pmx_swfsc_trace_bytes_per_slot(int max_qlen, int max_rlen);

/* Windowed frameshift traceback, reference side (extension): pmx_align_pairs_frameshift_ref_cigar[_device] for LONG REFERENCES --
 * contigs, chromosomes' worth of window -- whose m x N matrix of decision bytes does not fit the bound on a chunk's trace.  The
 * arguments are exactly those of pmx_align_pairs_frameshift_ref_cigar[_device], and EVERY OUTPUT -- records, strand bytes, statistics,
 * begins, text and offsets -- IS BYTE-IDENTICAL to what that entry writes for the same arguments, wherever that entry runs.
 *
 * How.  A local path behind a record (score S, end cell (end_query, end_ref)) has paid for every codon gap and every frameshift
 * operator out of S, so it spans few columns.  With rows = end_query + 1, P = the sum over query letters 0 .. end_query of
 * max(0, the largest score of the letter's matrix row), slack = P - S and gmin = min(open, extend), a path of score S that ends at the
 * end cell spans at most
 *     W = 3 rows + 3 floor(slack / gmin) + min(rows - 1, floor(slack / frameshift))         (frameshift 0: the last term is rows - 1)
 * nucleotides (gmin = 0 bounds nothing: the whole window).  The entry runs the score road of pmx_align_pairs_frameshift_ref_device over
 * the full windows, cuts every pair down to query letters [0, end_query] and oriented nucleotides [max(0, end_ref + 1 - W), end_ref]
 * on the device, runs the trace sweep and the walk of the _ref_cigar entries over those windows on the winner's strand, and moves
 * end_ref and beg_ref back into the pair's own oriented window.  Every decision on the walked path, and the end cell under the tie
 * rule, are those of the full matrix (DESIGN 2.5o has the proof); the entry holds the second pass's record against the first pass's,
 * and a difference ends the call with -1 and "window proof violated" -- a bug to report, not an input condition.
 *
 * Refusals.  Everything pmx_align_pairs_frameshift_ref_cigar[_device] refuses, with the same texts, EXCEPT the bound on four slots of
 * the un-narrowed shape: 4 096 letters x 100 kb is taken.  Behind the score pass of a chunk, a pair whose own narrowed window exceeds
 * the bound with four slots is refused with that bound's text, naming the narrowed figures.
 *
 * Scratch and parts.  The trace pass runs a chunk in parts of consecutive pairs, cut on the host so that a part's slots times
 * pmx_swfsc_trace_bytes_per_slot(the part's longest narrowed query, the part's longest narrowed stream) stay under the bound (256 MiB,
 * or the value switch PMX_CIGAR_CHUNK_BYTES): a weak hit with a wide window shrinks its own part only.  Beside the score entry's
 * scratch, 61 bytes per pair of a chunk.  chunk_pairs, the bound and the parts never change an output byte.
 * THE DEVICE ENTRY SYNCHRONISES THE CALLER'S STREAM ONCE PER CHUNK (the narrowed lengths come to the host, which cuts the parts) AND
 * ONCE BEHIND THE LAST CHUNK (the proof's check): when it returns 0 all outputs are written.  pmx_last_kernel() names the trace
 * instantiation of the last part, as the _ref_cigar entries do.
 * pmx_frameshift_ref_cigar_long_parts(): the number of parts the calling thread's last call of either entry ran, over all chunks (the
 * host entry: of its last pass). */
int pmx_align_pairs_frameshift_ref_cigar_long_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                     int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                                     int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                                     pmx_record_t *d_out, uint8_t *d_strand_out, pmx_stats_t *d_stats /* iff PMX_WANT_STATS */,
                                                     int32_t *d_beg /* 2 n, optional */,
                                                     char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off /* n + 1 */,
                                                     void *stream, const pmx_pairs_opts_t *opts);
int pmx_align_pairs_frameshift_ref_cigar_long(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                              int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                                              int32_t frameshift, const uint8_t *code,
                                              pmx_record_t *out, uint8_t *strand_out, pmx_stats_t *stats_out /* iff PMX_WANT_STATS */,
                                              int32_t *beg /* 2 n, optional */, char **cigar_buf, int64_t *cigar_off /* n + 1 */,
                                              const pmx_pairs_opts_t *opts);
int64_t pmx_frameshift_ref_cigar_long_parts(void);
/* Test hook: W of the bound above (parasail-rs_amd/csrc/pmx_fswin.h, the function the kernel runs) for P = rowmax_prefix, S = score and
 * rows = end_query + 1; 2^63 - 1 where nothing is bounded (min(open, extend) = 0). */
long long pmx_swfsc_window_cols(long long rowmax_prefix, long long score, long long rows, long long open, long long extend, long long fs);

/* K-mer seeding (extension): the stage in front of the _ex entries -- which windows of a resident reference a read is worth aligning
 * against.  An index of the k-mers of a DNA set, and an entry that turns the exact k-mer matches of queries into diagonal clusters and
 * the clusters into window descriptors and strand bytes, on the device (kernels: parasail-rs_amd/csrc/pmx_seed.hip).
 *
 * Letters: A/a = 0, C/c = 1, G/g = 2, T/t/U/u = 3, every other byte is invalid (pmx_complement_table maps valid letters to valid ones
 * and invalid bytes to invalid ones).  Sequence r has a k-mer at position j iff j + k <= len(r) and its k letters are valid; its key
 * holds 2 bits per letter, the first letter most significant.  k is 8 .. 31.
 *
 * The index is every k-mer of R at stride 1 as (kmer, seq, pos), ascending in that lexicographic order: 16 bytes per entry on the
 * device, a bucket table of at most 16 MiB, and while it is built twice that again.  pmx_seed_index_build synchronises (it allocates
 * and reads the number of entries back); `stream` is where its kernels run.  R must outlive the index, which belongs to R's device.
 * Refused (NULL, pmx_last_error()): a NULL set, k outside 8 .. 31, a set of another device than the current one, a set of more than
 * 2^31 - 1 bytes or sequences.  Wrapped sets are read under the rule of the set batches: no byte outside `bytes`, whatever the offsets.
 *
 * Seeding.  The oriented query of (q, strand) is Q[q] as stored (strand 0) or w'[x] = comp[w[L - 1 - x]] (strand 1, the _ex entries'
 * rule); all positions are relative to it.  opts->strand is a PMX_STRAND_* mode; PMX_STRAND_BOTH seeds both strands and lists them
 * separately (a candidate is a locus on a strand, nothing is folded).  A match of (q, s, r) is a pair (i, j): the oriented query has a
 * k-mer at i, R[r] has the same k-mer at j, and that k-mer has at most max_occ entries in the whole index (one with more is ignored
 * entirely; 1 .. 65535).  Its diagonal is d = j - i.  The matches of (q, s, r) ordered by d fall into clusters, maximal runs whose
 * consecutive diagonals differ by at most `band` (0 .. 2^20); matches of different r never share one.  A cluster of at least min_seeds
 * matches is a candidate:
 *   d_hit_pairs   {q, r, 0, -1, r_beg, r_len}: r_beg = max(0, diag_min - pad), r_end = min(len(r), diag_max + qlen + pad)
 *   d_hit_strand  the strand byte
 *   d_hit_seeds   {n_seeds, diag_min, diag_max, 0}, diagonals relative to the whole reference (optional)
 * d_hit_pairs / d_hit_strand are valid d_pairs / d_strand arguments of pmx_align_pairs_ex_device with nothing in between, and
 * diag - r_beg is the banded entries' diag for the gathered window.  Row q's candidates are ascending in (strand, r, diag_min).
 * d_row_off receives nq + 1 offsets from 0 and is always written in full, uncapped; only positions below `capacity` are written, entries
 * behind them are untouched; capacity == 0 counts only.  d_counts[0] = candidates, d_counts[1] = written.  A query longer than max_qlen
 * has no candidates.
 *
 * Determinism.  The output is bit-identical from run to run and slice_rows never changes a byte: matches are sorted per (row, strand)
 * by (r, d), clusters are runs of that order, and every output position is a scan over it plus the running total, which lives on the
 * device (d_counts[0]) and advances in row order on the caller's stream.
 *
 * Slices.  The number of matches is known only on the device, so the entry works in slices of rows: a count pass (one index lookup
 * per query position), a scan, and a cut -- the longest prefix of the slice whose matches fit the match buffer -- that THE ENTRY READS
 * BACK: pmx_seed_pairs_device synchronises `stream` once per slice and is not asynchronous.  opts->slice_rows bounds a slice
 * (0: as many rows as 256 MiB of position scratch hold, 16 bytes per (row, strand, position)).  Thread scratch: that, and the match
 * buffer of 256 MiB at 24 bytes per match.  Refused before any GPU work when one row's worst case, max_qlen x strands x max_occ x 24
 * bytes, does not fit the match buffer.
 *
 * Refused with -1 and a pmx_last_error() text before any GPU work: a NULL set, index or opts; NULL d_row_off or d_counts with nq > 0; a
 * set or index of another device than the current one; a negative q_first, nq, capacity, max_hits or slice_rows; rows beyond |Q|;
 * max_qlen < 1; an unknown strand mode; min_seeds < 1; band or pad negative or above 2^20; max_occ outside 1 .. 65535; non-zero
 * reserved; NULL d_hit_pairs or d_hit_strand with capacity > 0; the per-row budget above.  nq == 0 succeeds and writes zero counts and
 * d_row_off[0] = 0 where those pointers are given.
 *
 * The host entry runs the device entry on a stream of its own with room for two candidates per row (max_hits when that is less)
 * and, where more have to be stored, once more with buffers of the exact size.  It
 * returns one callee-allocated block released with pmx_seed_hits_free: row_off holds n_rows + 1 uncapped offsets, pairs / strand / seeds
 * n_hits entries, n_passing is the number of candidates.  max_hits > 0 stops storing after that many candidates, in row order, and
 * goes on counting (n_hits = min(n_passing, max_hits)); 0: no limit.  max_qlen is the longest query of the rows. */
typedef struct pmx_seed_index pmx_seed_index_t;
pmx_seed_index_t *pmx_seed_index_build(const pmx_seqset_t *R, int32_t k, void *stream);
void    pmx_seed_index_free(pmx_seed_index_t *index);
int64_t pmx_seed_index_count(const pmx_seed_index_t *index);          /* entries; -1 for NULL */
/* Test hook: entries [first, first + count) in index order (each output optional); asynchronous on `stream`. */
int pmx_seed_index_entries_device(const pmx_seed_index_t *index, int64_t first, int64_t count,
                                  uint64_t *d_kmer, int64_t *d_seq, int32_t *d_pos, void *stream);
typedef struct pmx_seed_hit { int32_t n_seeds, diag_min, diag_max, reserved; } pmx_seed_hit_t;   /* 16 bytes */
typedef struct pmx_seed_opts { int32_t strand, min_seeds, band, pad, max_occ, reserved; int64_t max_hits, slice_rows; } pmx_seed_opts_t;   /* 40 bytes */
int pmx_seed_pairs_device(const pmx_seqset_t *Q, const pmx_seed_index_t *index, int64_t q_first, int64_t nq, int32_t max_qlen,
                          const pmx_seed_opts_t *opts,
                          pmx_pair_t *d_hit_pairs, uint8_t *d_hit_strand, pmx_seed_hit_t *d_hit_seeds /* optional */, int64_t capacity,
                          int64_t *d_row_off /* nq + 1 */, int64_t *d_counts /* [0] candidates, [1] written */, void *stream);
typedef struct pmx_seed_hits { int64_t n_rows, n_hits, n_passing; int64_t *row_off; pmx_pair_t *pairs; uint8_t *strand; pmx_seed_hit_t *seeds; } pmx_seed_hits_t;
int  pmx_seed_pairs(const pmx_seqset_t *Q, const pmx_seed_index_t *index, int64_t q_first, int64_t nq,
                    const pmx_seed_opts_t *opts, pmx_seed_hits_t **result);
void pmx_seed_hits_free(pmx_seed_hits_t *hits);
/* Test hook: the calling thread's match buffer in bytes for the calls that follow (0: the default of 256 MiB); returns the bound it
 * replaces.  A small bound makes the cut of a slice fall after a few rows. */
int64_t pmx_seed_match_budget(int64_t bytes);

/* Minimizer seeding (extension): a (w, k) sketch in place of every k-mer at stride 1, on both sides of a DNA index -- the index and the
 * number of look-ups shrink by about (w + 1) / 2 (kernel: pmx_seed_sketch_kernel of parasail-rs_amd/csrc/pmx_seed.hip).
 * Letters, validity and keys are those above.  DNA indexes only: the letters and translated builds take no w.
 *
 * Definitions.  A sequence of n bytes has nk = n - k + 1 k-mer positions (none if nk <= 0).  Position p HAS A K-MER iff its k letters
 * are valid; its key is K(p).
 *   Order.     h(p) = mix(K(p)), with mix on B = 2 k bits, M = 2^B - 1, all arithmetic in 64 bits:
 *                h = (K ^ PMX_SEED_MIX_XOR) & M;  h = (h * PMX_SEED_MIX_MUL1) & M;  h ^= h >> k;  h = (h * PMX_SEED_MIX_MUL2) & M;  h ^= h >> k
 *              Every step is a bijection on B bits (an xor with a constant, a multiplication by an odd number modulo 2^B, an xor with
 *              the own upper half), so equal hashes mean equal k-mers, and a hash is below 2^62: "no k-mer" is never a hash value.
 *              pmx_seed_mix(key, k) returns it (0 for k outside 8 .. 31).  Position q LOSES TO p iff q has no k-mer or
 *              (h(q), q) > (h(p), p): the smaller hash wins and among equal k-mers the leftmost.
 *   Windows.   If nk >= w the windows are [s, s + w) for s = 0 .. nk - w; if 0 < nk < w there is the single window [0, nk).  A window
 *              never crosses a sequence end.  A window selects the position in it that every other position of it loses to; a window
 *              without a k-mer selects nothing.
 *   Minimizers of a sequence: the positions selected by at least one window.  Equivalently, with l the number of consecutive left
 *              neighbours that lose to p (capped at w - 1, stopping at position 0) and r the same to the right (stopping at nk - 1):
 *              p is a minimizer iff p has a k-mer and l + r + 1 >= min(w, nk).
 *   Strand 1.  The minimizers of the ORIENTED read (the reverse complement, w'[x] = comp[w[L - 1 - x]]), positions and the leftmost
 *              rule in oriented coordinates.
 *   w = 1 is every k-mer: the index of pmx_seed_index_build and its hits.
 *   Guarantee. If an oriented query and a reference sequence share a stretch of L >= w + k - 1 valid, equal letters and both have at
 *              least w k-mer positions, they share a minimizer at corresponding positions inside the stretch: the stretch holds a whole
 *              window of each, both windows hold the same k-mers in the same order, so both select the same offset.
 *
 * pmx_seed_index_build_minimizers: the index holds an entry (K, seq, pos) for the minimizer positions of R's sequences only, in the
 * order and layout of pmx_seed_index_build: 16 bytes per ENTRY plus the bucket table resident, and while it is built 5 bytes per byte
 * of the set (flags and their scan) plus twice the entries and rocPRIM's scratch.  It synchronises, as pmx_seed_index_build does.
 * pmx_seed_index_count, _entries_device, _bits and _free serve it; max_occ counts entries of THIS index.  pmx_seed_index_window: w; 1 of
 * every other build.  pmx_seed_index_bytes: the device bytes an index of any kind owns.  Refused (NULL, pmx_last_error()) before any
 * GPU work: a NULL set, k outside 8 .. 31, w outside 1 .. 64, a set of more than 2^31 - 1 bytes or sequences, a set of another device.
 * An empty set builds with no device work.
 *
 * Seeding.  pmx_seed_pairs[_device] take a minimizer index as it is and read w from it: a match is an (i, j) where i is a minimizer of
 * the oriented query, j an entry, the keys are equal and the key has at most max_occ entries.  Everything else -- diagonals, clusters,
 * min_seeds, band, pad, windows, order, capacity, slices, determinism, the refusals and the row budget rule -- is what is documented
 * above (a position slot takes 17 bytes of scratch in place of 16).
 *
 * pmx_seed_sketch[_device]: the minimizers of rows q_first .. q_first + nq of Q alone.  flags receives one byte per position slot
 * (row_local * strands + s) * max_qlen + i, strands = 2 with PMX_STRAND_BOTH (s = the strand) and 1 otherwise: 1 where oriented
 * position i is a minimizer, 0 elsewhere -- every slot is written.  A row longer than max_qlen has no minimizer.  The device entry is
 * ASYNCHRONOUS on `stream`; the host entry takes a host array.  Refused with -1 and a pmx_last_error() text before any GPU work: a NULL
 * set; k outside 8 .. 31; w outside 1 .. 64; a negative q_first or nq; rows beyond |Q|; a bad strand mode; max_qlen < 1; more than
 * 2^31 - 1 position slots; NULL flags with nq > 0; a set of another device.  nq == 0 succeeds and writes nothing. */
#define PMX_SEED_MIX_XOR  0x9E3779B97F4A7C15ull
#define PMX_SEED_MIX_MUL1 0xBF58476D1CE4E5B9ull
#define PMX_SEED_MIX_MUL2 0x94D049BB133111EBull
uint64_t pmx_seed_mix(uint64_t key, int32_t k);
pmx_seed_index_t *pmx_seed_index_build_minimizers(const pmx_seqset_t *R, int32_t k, int32_t w, void *stream);
int32_t pmx_seed_index_window(const pmx_seed_index_t *index);         /* w; 1 for every other build; -1 for NULL */
int64_t pmx_seed_index_bytes(const pmx_seed_index_t *index);          /* device bytes the index owns; -1 for NULL */
int pmx_seed_sketch_device(const pmx_seqset_t *Q, int64_t q_first, int64_t nq, int32_t max_qlen, int32_t k, int32_t w, int strand_mode,
                           uint8_t *d_flags /* nq x strands x max_qlen */, void *stream);
int pmx_seed_sketch(const pmx_seqset_t *Q, int64_t q_first, int64_t nq, int32_t max_qlen, int32_t k, int32_t w, int strand_mode,
                    uint8_t *flags /* host, nq x strands x max_qlen */, void *stream);
/* The longest of rows q_first .. q_first + nq of Q, a max_qlen for the entries above (0 for nq == 0; -1: a NULL set, rows beyond |Q|). */
int64_t pmx_seed_rows_max_len(const pmx_seqset_t *Q, int64_t q_first, int64_t nq);
/* Test hook: the positions a workgroup of the sketch kernel owns, in its row form and its set form. */
void pmx_seed_sketch_shape(int32_t *row_tile, int32_t *set_tile);

/* Seed chaining (extension): collinear chains with gap costs in place of diagonal clusters, for a DNA index -- stride 1 or minimizers,
 * any w (kernel: pmx_seed_chain_kernel of parasail-rs_amd/csrc/pmx_seed.hip).  A cluster knows a match's diagonal only;
 * a chain also knows where along the read it lies, so a long indel does not split a locus and two distant matches on one diagonal
 * do not merge.  Opt-in and additive: pmx_seed_pairs[_device] and every other entry do what they did.
 *
 * Definitions.  Letters, k-mers, the oriented query, max_occ, the matches (i, j) of (q, s, r) and minimizer sampling are
 * pmx_seed_pairs' definitions above, unchanged.
 *   Anchor order.  The matches of (q, s, r) are ordered ascending by (j, i).  a and b are positions in that order, which has no ties:
 *              an (i, j) occurs once.
 *   Link.      b < a may precede a iff, with dj = j_a - j_b and di = i_a - i_b, all of these hold:
 *                dj >= 1 and di >= 1;   dj <= max_gap and di <= max_gap;   g = |dj - di| <= band;   a - b <= lookback.
 *              Anchors of different r, strand or row never link.
 *   Cost.      Integers only: cost(0) = 0; for g >= 1: cost(g) = ((int64)g * gap_scale >> 8) + ((32 - clz(g)) >> 1).
 *              With gap_scale = 38 this is about minimap2's 0.01 k g + 0.5 log2 g at k = 15.
 *   Score.     f(a) = max(k, max_b f(b) + min(di, dj, k) - cost(g)) over the admissible b.  pred(a) is the b that attains the
 *              maximum, taken only when the value is strictly above k; among equal values the nearest b (the largest) wins;
 *              pred(a) = -1 otherwise.
 *   Chains.    child(b) is, among the a with pred(a) = b, the one with the largest f(a); among equal values the smallest a wins.
 *              The link a -> pred(a) is kept iff child(pred(a)) = a.  Chains are the maximal paths of kept links, so they are disjoint
 *              and every anchor is in exactly one.  The head h of a chain has no kept link to a predecessor, the tail t has no child.
 *              A chain's score is f(t) - f(pred(h)), or f(t) when pred(h) = -1.
 *   Candidate. A chain is a candidate iff score >= min_score and n_anchors >= min_seeds.  d_hit_pairs, d_hit_strand and
 *              d_hit_seeds = {n_anchors, diag_min, diag_max, 0} follow the cluster road's rule exactly, over the chain's own anchors
 *              (d = j - i): r_beg = max(0, diag_min - pad), r_end = min(len(r), diag_max + qlen + pad).  A chained list therefore goes
 *              unchanged into pmx_align_pairs_ex[_device], pmx_seed_ungapped and pmx_seed_filter[_device] with PMX_SEED_BYTE_STRAND.
 *              In addition an optional 32-byte record is written per candidate: pmx_seed_chain_t {score, n_anchors, q_beg = i_h,
 *              q_end = i_t + k, r_beg = j_h, r_end = j_t + k, diag_min, diag_max}, coordinates of the oriented query and of the whole
 *              reference.  Row q's candidates are ascending in (strand, r, the tail's (j, i)).
 *   Determinism.  The output is bit-identical from run to run, under any slice_rows and any match budget.  No output position and no
 *              tie is decided by an atomic: the sort is stable over matches emitted in ascending i, one wave walks a segment in anchor
 *              order, and every output position is a scan.
 *   Arithmetic.  f fits int32: i rises strictly along a chain, so a chain has at most max_qlen anchors of gain <= k <= 31 each, and
 *              max_qlen <= 2^26 is required; cost < 2^28 (g <= 2^20, gap_scale < 2^16), so no intermediate leaves int32 either.
 *
 * pmx_seed_opts_t: strand, min_seeds, pad, max_occ, max_hits and slice_rows mean what they mean to pmx_seed_pairs; band (0 .. 2^20) is
 * the link's bound on |dj - di|.  Capacity, d_row_off, d_counts, the one stream synchronisation per slice, nq == 0, the host entry's
 * two-pass sizing and max_hits are pmx_seed_pairs[_device]'s, by the same code.  A match takes 40 bytes of scratch in place of 24.
 *
 * Refused with -1 and a pmx_last_error() text before any GPU work: everything pmx_seed_pairs_device refuses, with its texts; NULL
 * copts; max_gap outside 1 .. 2^20; lookback outside 1 .. 1024; gap_scale outside 0 .. 65 535; min_score < 0; non-zero reserved; a
 * letters or translated index (chaining takes a DNA index); max_qlen above 2^26; the per-row budget max_qlen x strands x max_occ x 40
 * bytes.
 *
 * pmx_seed_chains returns one callee-allocated block released with pmx_seed_chained_free: hits as pmx_seed_pairs fills it, chains with
 * hits.n_hits records.  pmx_seed_chain_shape (test hook): the lanes that evaluate predecessors at once and the anchors the kernel's
 * ring holds at most. */
typedef struct pmx_seed_chain_opts { int32_t max_gap, lookback, gap_scale, min_score, reserved[4]; } pmx_seed_chain_opts_t;   /* 32 bytes */
typedef struct pmx_seed_chain { int32_t score, n_anchors, q_beg, q_end, r_beg, r_end, diag_min, diag_max; } pmx_seed_chain_t;  /* 32 bytes */
int pmx_seed_chains_device(const pmx_seqset_t *Q, const pmx_seed_index_t *index, int64_t q_first, int64_t nq, int32_t max_qlen,
                           const pmx_seed_opts_t *opts, const pmx_seed_chain_opts_t *copts,
                           pmx_pair_t *d_hit_pairs, uint8_t *d_hit_strand, pmx_seed_hit_t *d_hit_seeds /* optional */,
                           pmx_seed_chain_t *d_hit_chains /* optional */, int64_t capacity,
                           int64_t *d_row_off /* nq + 1 */, int64_t *d_counts /* [0] candidates, [1] written */, void *stream);
typedef struct pmx_seed_chained { pmx_seed_hits_t hits; pmx_seed_chain_t *chains; } pmx_seed_chained_t;
int  pmx_seed_chains(const pmx_seqset_t *Q, const pmx_seed_index_t *index, int64_t q_first, int64_t nq,
                     const pmx_seed_opts_t *opts, const pmx_seed_chain_opts_t *copts, pmx_seed_chained_t **result);
void pmx_seed_chained_free(pmx_seed_chained_t *chained);
void pmx_seed_chain_shape(int32_t *lanes, int32_t *ring);

/* Protein seeding (extension): the same stage in front of the translated entries -- a k-mer index of a PROTEIN set over a reduced
 * alphabet, and a seeding entry whose queries are proteins or nucleotide reads translated on the device in up to six frames.  Its
 * candidate lists go unchanged into pmx_align_pairs_translated[_device] (a frame byte per pair) and pmx_align_pairs_frameshift[_device]
 * (a strand byte per pair) (kernels: parasail-rs_amd/csrc/pmx_seed.hip).  pmx_seed_pairs[_device] refuses a letters index
 * and names this entry; this entry refuses a DNA index and names pmx_seed_pairs.
 *
 * Alphabet.  `table` maps a byte to its group 0 .. G - 1 or to 255 (invalid); G = the largest group + 1 must be 2 .. 32 and a letter
 * takes bits = ceil(log2 G) bits.  pmx_seed_alphabet fills one of the built-in tables (-1: a NULL table, an unknown `which`):
 * AA20, the twenty amino acids ACDEFGHIKLMNPQRSTVWY, one group each in that order (5 bits), and AA11, the groups KREDQN | C | G | H |
 * ILV | M | F | Y | W | P | STA in that order (4 bits); either case; '*', 'X', 'B', 'Z' and every other byte are invalid in both.
 *
 * Index.  Sequence r has a k-mer at j iff j + k <= len(r) and all k letters are valid.  Its key holds `bits` bits per letter, the first
 * letter most significant; an empty position's key is 1 << (k * bits).  Order (kmer, seq, pos) ascending, entry layout, the bucket
 * table (on the top min(k * bits, 22) bits), pmx_seed_index_count, _entries_device and _free: as for a DNA index.  The index owns a
 * device copy of the table.  pmx_seed_index_bits: the bits per letter, 2 for a DNA index.  Refused before any GPU work (NULL,
 * pmx_last_error()): a NULL set or table; a table with a group above 31 or with fewer than 2 groups (no valid byte, one group);
 * k < 2 or k * bits > 62; a set of more than 2^29 - 1 bytes (the nucleotide diagonals below multiply a reference position by 3) or
 * 2^31 - 1 sequences: index in parts; a set of another device than the current one.
 *
 * Queries.  query_mode says what Q holds and which orientations of a row are seeded:
 *   PMX_SEED_QUERY_LETTERS     Q is in the index's alphabet: one orientation, the row itself, L = W letters; byte 0
 *   0 .. 5, PMX_FRAMES_*       Q holds nucleotides; an orientation is a FRAME f, candidates per frame; byte = f
 *   PMX_SEED_CODONS_*          Q holds nucleotides; an orientation is a STRAND s over its three frames 3 s .. 3 s + 2; byte = s
 * Translation is the translated entries' rule: frame f reads the row as stored (f < 3) or reverse-complemented through
 * pmx_complement_table (f >= 3) from offset off = f % 3, L_f = (W - off) / 3 letters (none when W < off + 3); `code` (64 letters, NCBI
 * order) replaces pmx_genetic_code_table, NULL: the standard code; a codon with a byte outside A C G T U (either case) is 'X'.  The
 * translated letter then goes through the index's table, so 'X' and '*' break a k-mer under the built-in alphabets.
 *
 * Frame modes and letters mode.  Position p is a letter of the orientation's translation.  A match is (p, j): the translation has a
 * k-mer at p, R[r] has a k-mer with the same key at j, and that k-mer has at most max_occ entries in the whole index.  Its diagonal is
 * d = j - p, in letters.  Clusters, min_seeds, band and pad are the DNA entry's.  The candidate is {q, r, 0, -1, r_beg, r_len} with
 * r_beg = max(0, d_min - pad), r_end = min(len(r), d_max + L + pad); d_hit_seeds is {n_seeds, d_min, d_max, 0}.  d_hit_pairs /
 * d_hit_byte are valid d_pairs / d_frame of pmx_align_pairs_translated_device (frame_mode 0) and, in letters mode, d_pairs of
 * pmx_align_pairs_device, with nothing in between.
 *
 * Codon modes.  The matches of frames 3 s, 3 s + 1 and 3 s + 2 are taken TOGETHER, each on its nucleotide diagonal
 * D = 3 j - (off + 3 p), so D mod 3 tells the frame.  The matches of (q, s, r) ordered by D fall into maximal runs whose consecutive D
 * differ by at most `band`, in nucleotides here; a run of at least min_seeds matches is a candidate with
 * r_beg = max(0, floor(D_min / 3) - pad), r_end = min(len(r), floor((D_max + W - 1) / 3) + 1 + pad), floor towards minus infinity,
 * pad in reference letters; d_hit_seeds is {n_seeds, D_min, D_max, 0}.  A read with one base inserted or deleted therefore yields ONE
 * candidate whose seeds come from two frames, where the frame modes yield two.  d_hit_pairs / d_hit_byte are valid d_pairs / d_strand
 * of pmx_align_pairs_frameshift_device.
 *
 * max_qlen bounds the letters of the longest translation, W / 3 (letters mode: W); a row above it has no candidates; the host entry
 * sizes it from the rows.  Position slots are (row, orientation, p), in the codon modes (row, strand, frame, p): max_qlen x 1, 3 or 6
 * per row (one frame or the row itself; three frames; six), 17 bytes each.  Row q's candidates ascend in (byte, r, diag_min).
 *
 * pmx_seed_opts_t and pmx_seed_hits_t are reused: opts->strand must be 0, and the result's `strand` array holds the byte.  capacity,
 * d_row_off, d_counts, max_hits, slices and the cut read back once per slice, pmx_seed_match_budget, determinism and nq == 0 are what
 * pmx_seed_pairs[_device] documents.  Refused with -1 before any GPU work: everything pmx_seed_pairs_device refuses, with its texts
 * (the strand mode apart); opts->strand != 0; a query_mode outside the values below; a DNA index; one row's worst case,
 * max_qlen x orientations x max_occ x 24 bytes, above the match buffer. */
#define PMX_SEED_ALPHABET_AA20 0   /* ACDEFGHIKLMNPQRSTVWY, one group each, either case: 5 bits */
#define PMX_SEED_ALPHABET_AA11 1   /* KREDQN | C | G | H | ILV | M | F | Y | W | P | STA, either case: 4 bits */
int  pmx_seed_alphabet(int which, uint8_t table[256]);          /* group 0 .. G-1 per byte, 255 = invalid */
pmx_seed_index_t *pmx_seed_index_build_letters(const pmx_seqset_t *R, int32_t k, const uint8_t table[256], void *stream);
int32_t pmx_seed_index_bits(const pmx_seed_index_t *index);     /* bits per letter; 2 for a DNA index; -1 for NULL */
#define PMX_SEED_QUERY_LETTERS  (-1)  /* Q is in the index's alphabet; one orientation, byte 0 */
/* 0 .. 5, PMX_FRAMES_FORWARD / _REVERSE / _ALL: Q holds nucleotides; candidates per FRAME, byte = frame */
#define PMX_SEED_CODONS_FORWARD  9    /* Q holds nucleotides; candidates per STRAND over its three frames, byte = strand 0 */
#define PMX_SEED_CODONS_REVERSE 10    /* ... byte = strand 1 */
#define PMX_SEED_CODONS_BOTH    11    /* both strands, listed separately */
int pmx_seed_pairs_letters_device(const pmx_seqset_t *Q, const pmx_seed_index_t *index, int64_t q_first, int64_t nq, int32_t max_qlen,
                                  const pmx_seed_opts_t *opts, int query_mode, const uint8_t *code /* 64 letters or NULL */,
                                  pmx_pair_t *d_hit_pairs, uint8_t *d_hit_byte, pmx_seed_hit_t *d_hit_seeds, int64_t capacity,
                                  int64_t *d_row_off, int64_t *d_counts, void *stream);
int pmx_seed_pairs_letters(const pmx_seqset_t *Q, const pmx_seed_index_t *index, int64_t q_first, int64_t nq,
                           const pmx_seed_opts_t *opts, int query_mode, const uint8_t *code, pmx_seed_hits_t **result);

/* Seeding translated references (extension): the tblastn pairing -- a six-frame k-mer index of a NUCLEOTIDE set over a reduced
 * alphabet, seeded by protein queries.  Its candidate lists go unchanged into pmx_align_pairs_translated_ref[_device] (a frame byte per
 * pair) and pmx_align_pairs_frameshift_ref[_device] and its traceback entries (a strand byte per pair) (kernels:
 * parasail-rs_amd/csrc/pmx_seed.hip).  Each index kind refuses the other kinds' seeding entries and names its own.
 *
 * The set and the strands.  R holds nucleotides.  `table` is the 256-byte table of pmx_seed_index_build_letters (same bits, same
 * built-ins), `code` 64 letters in NCBI order or NULL for pmx_genetic_code_table.  strand_mode (PMX_STRAND_FORWARD, _REVERSE, _BOTH) is
 * fixed when the index is built: seeding uses exactly the strands the index holds, there is no per-call filter, and max_occ counts a
 * k-mer's entries over the index as built.
 *
 * Oriented coordinates.  A sequence r of N nucleotides is read as stored (strand s = 0) or reverse-complemented (s = 1): exactly the
 * reading of frames 3 .. 5 of the reference-side translated entries, through pmx_complement_table from the end downwards; nothing is
 * materialised.  Oriented position x = 0 .. N - 3 starts the codon of oriented bytes x, x + 1, x + 2; its letter is the translation by
 * the translated entries' rule (a byte outside A C G T U, either case, gives 'X') put through the table.  'X', '*' and every letter
 * the table maps to 255 are invalid.  The k-mer at x is the k letters at x, x + 3, ..., x + 3 (k - 1): it needs x + 3 k <= N and k
 * valid letters, so it never crosses a sequence end.  Keys: `bits` per letter, first letter most significant; an empty position has
 * the key 1 << (k * bits); the bucket table is on the top min(k * bits, 22) bits.
 *
 * Index.  One entry per (s, r, x) with a k-mer, sorted by (kmer, s, r, x); value (s * count + r) << 32 | x, count = the sequences of
 * R; pmx_seed_index_entries_device reports d_seq = s * count + r and d_pos = x.  The index therefore holds the k-mers of all three
 * frames of each held strand: x % 3 is the frame's offset and g = 3 s + x % 3 the SEQUENCE FRAME.  Refused before any GPU work
 * (NULL, pmx_last_error()): what pmx_seed_index_build_letters refuses about set, table and k (k >= 2, k * bits <= 62), with its texts;
 * a strand mode outside 0 .. 2; more than 2^30 - 1 bytes (two entry slots per byte with both strands; entry numbers and bucket
 * contents are 32-bit) or more than 2^29 sequences (6 * count fits the upper half of a match key): index in parts.  Resident: 16 bytes
 * per entry slot -- one slot per byte and held strand, 32 bytes per nucleotide with both -- plus the bucket table (16 MiB at most);
 * while it is built twice that plus rocPRIM's scratch.  pmx_seed_index_strands: the strand mode; -2 for a DNA or letters index.
 *
 * Seeding.  Q holds proteins in the index's alphabet: one orientation, the row itself, m letters (max_qlen bounds m).  A match is
 * (p, s, r, x): the row has a k-mer at p, the index an entry (s, r, x) with the same key, and that key has at most max_occ entries.
 *
 * PMX_SEED_REF_FRAMES: candidates per sequence frame.  The matches of (q, g, r) lie on the letter diagonal d = (x - x % 3) / 3 - p;
 * runs, band, min_seeds and pad are pmx_seed_pairs', in letters.  With L_g = (N - g % 3) / 3 the letter window of frame g is
 * [lb, le) = [max(0, d_min - pad), min(L_g, d_max + m + pad)), and the descriptor's reference window is that range in STORED
 * nucleotides, codon-aligned, off = g % 3: [off + 3 lb, off + 3 le) on strand 0, [N - off - 3 le, N - off - 3 lb) on strand 1.  The
 * byte is the frame RELATIVE TO THE WINDOW, by the alignment always 0 (strand 0) or 3 (strand 1): d_hit_pairs / d_hit_byte are valid
 * d_pairs / d_frame of pmx_align_pairs_translated_ref_device.  d_hit_seeds is {n_seeds, d_min, d_max, g}: `reserved` carries the
 * sequence frame, which tells where in the contig the frame lies.  Row q's candidates ascend in (g, r, d_min).  These candidates --
 * entries, row offsets, order, n_seeds, d_min, d_max -- equal those of pmx_seed_pairs_letters (PMX_SEED_QUERY_LETTERS) over a letters
 * index of the protein set R6 whose sequence g * count + r is the translation of R[r] in frame g (held strands only; same table, k,
 * options), with r' -> (g, r) and the letter window mapped as above.
 *
 * PMX_SEED_REF_CODONS: candidates per strand over its three frames.  The matches of (q, s, r) lie on the NUCLEOTIDE diagonal
 * D = x - 3 p; band and pad are in nucleotides.  The oriented window is [lo, hi) = [max(0, D_min - pad), min(N, D_max + 3 m + pad)),
 * stored [lo, hi) on strand 0 and [N - hi, N - lo) on strand 1; the byte is the strand: d_hit_pairs / d_hit_byte are valid d_pairs /
 * d_strand of pmx_align_pairs_frameshift_ref_device and of the frameshift_ref traceback entries.  d_hit_seeds is {n_seeds, D_min,
 * D_max, 0}.  One base inserted or deleted in the contig moves a hit by one nucleotide diagonal, so it stays ONE candidate carrying
 * the seeds of both frames where the frame mode gives two shorter ones.  Row q's candidates ascend in (s, r, D_min).
 *
 * pmx_seed_opts_t and pmx_seed_hits_t are reused: opts->strand must be 0, the result's `strand` array holds the byte.  Position slots
 * are (row, p), max_qlen per row, 17 bytes each.  capacity, d_row_off, d_counts, max_hits and the uncapped offsets, slices, the cut
 * and one stream synchronisation per slice, pmx_seed_match_budget, nq == 0 and determinism are what pmx_seed_pairs[_device] documents,
 * by the same code.  Refused with -1 before any GPU work: everything pmx_seed_pairs_letters refuses about the shared arguments, with
 * its texts; opts->strand != 0; a ref_mode outside 0 .. 1; a DNA or letters index; one row's worst case, max_qlen x max_occ x 24
 * bytes, above the match buffer. */
pmx_seed_index_t *pmx_seed_index_build_translated(const pmx_seqset_t *R, int32_t k, const uint8_t table[256],
                                                  const uint8_t *code /* 64 letters or NULL */, int strand_mode, void *stream);
int32_t pmx_seed_index_strands(const pmx_seed_index_t *index);  /* the PMX_STRAND_* mode of a translated index; -2: a DNA or letters index; -1 for NULL */
#define PMX_SEED_REF_FRAMES 0   /* candidates per sequence frame, letter diagonals; byte = frame relative to the window (0 or 3) */
#define PMX_SEED_REF_CODONS 1   /* candidates per strand over its three frames, nucleotide diagonals; byte = strand */
int pmx_seed_pairs_translated_ref_device(const pmx_seqset_t *Q, const pmx_seed_index_t *index, int64_t q_first, int64_t nq, int32_t max_qlen,
                                         const pmx_seed_opts_t *opts, int ref_mode,
                                         pmx_pair_t *d_hit_pairs, uint8_t *d_hit_byte, pmx_seed_hit_t *d_hit_seeds, int64_t capacity,
                                         int64_t *d_row_off, int64_t *d_counts, void *stream);
int pmx_seed_pairs_translated_ref(const pmx_seqset_t *Q, const pmx_seed_index_t *index, int64_t q_first, int64_t nq,
                                  const pmx_seed_opts_t *opts, int ref_mode, pmx_seed_hits_t **result);

/* Ungapped diagonal filter (extension): the stage between a seeding entry and a gapped extension -- the best ungapped local score along
 * the seeded diagonals of every candidate, a score threshold and the best top_n candidates per query row, all on the device (DESIGN
 * 2.5s; kernels: parasail-rs_amd/csrc/pmx_ungap.hip).  A filtered list is again a candidate list: it goes unchanged wherever the
 * unfiltered one goes.
 *
 * A candidate is what the seeding entries write: a descriptor {q, r, q_beg, q_len, r_beg, r_len}, one byte and a seed record {n_seeds,
 * diag_min, diag_max, reserved}.  byte_kind says what the byte is:
 *   PMX_SEED_BYTE_STRAND   a strand, the _ex entries' rule (d_byte NULL: all forward).  The lists of pmx_seed_pairs[_device], and of
 *                          pmx_seed_pairs_letters[_device] with PMX_SEED_QUERY_LETTERS, whose byte is 0.  `code` is not read.
 *   PMX_SEED_BYTE_FRAME    a frame 0 .. 5 of the query (d_byte NULL: all frame 0), translated with `code` (64 letters or NULL, the
 *                          standard code).  The lists of pmx_seed_pairs_letters[_device] in a frame mode.  max_qlen bounds the letters
 *                          of a translation, as in pmx_gather_pairs_translated_device.
 * Let x[0 .. L) be the oriented query window, exactly what pmx_gather_pairs_device (STRAND) or pmx_gather_pairs_translated_device
 * (FRAME) writes for the pair, and y the reference window [r_beg, r_beg + r_len) as gathered.  Diagonals are in the seeds' coordinates:
 * d = j - i, j a position in the WHOLE reference sequence, i a position in x.  Cell (i, j) exists iff 0 <= i < L and r_beg <= j <
 * r_beg + r_len, and scores w = matrix[mapper[x[i]]][mapper[y[j - r_beg]]], the alignment kernels' rule for the same cfg->matrix (of
 * cfg only the matrix is read besides the usual checks).  For each d in [diag_min, diag_max], along the diagonal's existing cells in
 * ascending i: h(d, i) = max(0, h(d, i - 1) + w), h = 0 in front of the first cell.  The ungapped score is U = max h over all those
 * cells, exact in int32.  The record:
 *   U > 0           {U, d, i, i + d}: among the cells with h = U the lowest d, then the lowest i (end_ref is relative to the whole reference)
 *   no positive h   {0, diag_min, -1, -1} (also when no cell exists)
 *   bad candidate   {-1, 0, -1, -1}: a bad descriptor under the gather's own validity rule (with PMX_SEED_BYTE_FRAME also a frame that
 *                   holds no codon), a byte outside its kind's range, or diag_min > diag_max
 *
 * pmx_seed_ungapped[_device]: the records of n listed candidates and nothing else.  The device entry is ASYNCHRONOUS on `stream` (n is
 * known on the host); a call that needs more thread scratch than any before it allocates, which synchronises.  opts: chunk_pairs as
 * in the set batches; it never changes a byte.
 *
 * pmx_seed_filter[_device]: the selection over a CSR list -- d_row_off holds nq + 1 offsets and the caller passes the COMPLETE list, n =
 * row_off[nq].  A candidate passes iff score >= max(min_score, 0) (a bad candidate never does).  With top_n > 0 only the top_n best
 * passing candidates of a row are kept: by score descending, then position in the row ascending.  Kept candidates leave in their input
 * order, so the output is again ascending in (byte, r, diag_min) per row and a valid input of every entry that takes the unfiltered
 * list.  Per kept candidate: descriptor, byte, seed record, ungapped record and `source`, its index in the input list (each output
 * optional).  d_out_row_off receives nq + 1 offsets, uncapped and always written in full; `capacity` and d_counts = [kept, written]
 * follow pmx_seed_pairs_device: only positions below capacity are written, entries behind them are untouched, capacity == 0 counts
 * only.  No atomic decides an output position: ranks come from one segmented sort of (score descending, position) keys per row,
 * positions from one scan of the keep flags in input order, so the output is bit-identical from run to run and under any chunk_pairs.
 * The device entry is asynchronous on `stream` like the one above.  Offsets that are not those of the list (not ascending, outside
 * 0 .. n) give an unspecified selection but no access outside the arrays.
 *
 * Thread scratch on the device: the chunk buffers of the _ex entries (two sets of at most 256 MiB of packed windows and 34 bytes per
 * slot), and for the filter 16 bytes per candidate of records, 16 of sort keys with top_n > 0, 4 of flags and rocPRIM's temporary
 * storage.
 *
 * Refused with -1 and a pmx_last_error() text before any GPU work: a NULL set, configuration, matrix, d_pairs, d_seeds or record
 * output with n > 0; negative n, nq, capacity or chunk_pairs; max_qlen or max_rlen below 1; a PSSM; an unknown byte_kind; max |w| x
 * max_qlen >= 2^31; sets of another device than the current one; for the filter also NULL opts, top_n < 0, min_score < 0, non-zero
 * reserved fields, NULL d_row_off, d_out_row_off or d_counts, and n above 2^31 - 1.  n == 0 succeeds: zero counts and nq + 1 zero offsets.
 *
 * Not for these four entries, and they cannot tell: the lists of the codon modes (PMX_SEED_CODONS_*) and of a translated index
 * (pmx_seed_pairs_translated_ref).  Their diagonals are in nucleotides over three frames or belong to frames of the reference; passing
 * them here scores other cells than the seeds'.  They go to pmx_seed_ungapped_translated[_device] and
 * pmx_seed_filter_translated[_device] below, which take a list_kind in place of the byte_kind.
 *
 * The host entries run the device entries on a stream of their own over uploaded arrays.  pmx_seed_filter takes a pmx_seed_hits_t and
 * returns one callee-allocated block released with pmx_seed_filtered_free: hits is a pmx_seed_hits_t of the kept candidates (n_passing
 * = n_hits = kept), ungapped and source hold n_hits entries.  It refuses a list that max_hits cut (n_hits < n_passing): the selection
 * needs every row in full. */
#define PMX_SEED_BYTE_STRAND 0
#define PMX_SEED_BYTE_FRAME  1
typedef struct pmx_ungapped { int32_t score, diag, end_query, end_ref; } pmx_ungapped_t;   /* 16 bytes */
typedef struct pmx_seed_filter_opts { int32_t min_score, top_n, reserved[2]; } pmx_seed_filter_opts_t;   /* 16 bytes; top_n 0: no limit */
int pmx_seed_ungapped_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                             const pmx_pair_t *d_pairs, const uint8_t *d_byte /* or NULL */, int byte_kind, const uint8_t *code,
                             const pmx_seed_hit_t *d_seeds, int32_t max_qlen, int32_t max_rlen,
                             pmx_ungapped_t *d_out /* n */, void *stream, const pmx_pairs_opts_t *opts);
int pmx_seed_ungapped(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                      const pmx_pair_t *pairs, const uint8_t *byte /* or NULL */, int byte_kind, const uint8_t *code,
                      const pmx_seed_hit_t *seeds, pmx_ungapped_t *out /* n */, const pmx_pairs_opts_t *opts);
int pmx_seed_filter_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                           const pmx_pair_t *d_pairs, const uint8_t *d_byte /* or NULL */, int byte_kind, const uint8_t *code,
                           const pmx_seed_hit_t *d_seeds, int32_t max_qlen, int32_t max_rlen,
                           int64_t nq, const int64_t *d_row_off /* nq + 1 */, const pmx_seed_filter_opts_t *fopts,
                           pmx_pair_t *d_out_pairs, uint8_t *d_out_byte, pmx_seed_hit_t *d_out_seeds, pmx_ungapped_t *d_out_ungapped,
                           int64_t *d_out_source, int64_t capacity, int64_t *d_out_row_off /* nq + 1 */,
                           int64_t *d_counts /* [0] kept, [1] written */, void *stream, const pmx_pairs_opts_t *opts);
typedef struct pmx_seed_filtered { pmx_seed_hits_t hits; pmx_ungapped_t *ungapped; int64_t *source; } pmx_seed_filtered_t;
int  pmx_seed_filter(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, const pmx_seed_hits_t *hits,
                     int byte_kind, const uint8_t *code, const pmx_seed_filter_opts_t *fopts, const pmx_pairs_opts_t *opts,
                     pmx_seed_filtered_t **result);
void pmx_seed_filtered_free(pmx_seed_filtered_t *result);
/* Test hook: the hot kernel's lanes per candidate and cells per lane step. */
void pmx_seed_ungapped_shape(int32_t *lanes, int32_t *step);

/* Ungapped diagonal filter for the codon and translated-index lists (extension): the same stage for the three seeding roads whose
 * diagonals are not letter diagonals of one query frame (the same kernel in three more forms).  Everything the block
 * above defines stays as it is: pmx_ungapped_t, the recurrence h = max(0, h + w) along a diagonal's existing cells and U = max h, exact
 * in int32; the three record forms {U, diag, end_query, end_ref}, {0, diag_min, -1, -1} when no cell is positive (also when no cell
 * exists) and {-1, 0, -1, -1} for a bad candidate; the tie rule (the lowest diagonal, then the earliest cell); the selection
 * (threshold max(min_score, 0), top_n by score descending then position ascending, kept candidates in input order with `source`,
 * `capacity`, d_counts = [kept, written], uncapped row offsets always written); w = matrix[mapper[query letter]][mapper[reference
 * letter]].  list_kind says which cells a seed record's diagonals [diag_min, diag_max] mean; `code` (64 letters in NCBI order, NULL: the
 * standard code) is read by all three kinds.
 *
 *   PMX_SEED_LIST_CODONS       The lists of pmx_seed_pairs_letters[_device] in a codon mode; the byte is a strand of the query (d_byte
 *                              NULL: all forward).  Q holds nucleotides, R proteins.  T is the codon stream of the oriented query window,
 *                              W - 2 letters, exactly what pmx_gather_pairs_codons_device writes; y is the reference window [r_beg,
 *                              r_beg + r_len).  Cell (n, j) exists iff 0 <= n < W - 2, r_beg <= j < r_beg + r_len and n = 3 j - D for a D
 *                              in [diag_min, diag_max] -- the seeds' rule D = 3 j - (off + 3 p) -- and scores T[n] against y[j - r_beg].
 *                              The cells of one D are walked in ascending j.  Record {U, D, n + 2, j}: end_query is the last nucleotide
 *                              of the last codon in the oriented window, the frameshift record's convention.
 *   PMX_SEED_LIST_REF_FRAMES   The lists of pmx_seed_pairs_translated_ref[_device] with PMX_SEED_REF_FRAMES; the byte is the frame relative
 *                              to the window (0 or 3; d_byte NULL: all 0) and seeds.reserved the sequence frame g.  x is the query window,
 *                              y the translated reference window, exactly what pmx_gather_pairs_translated_ref_device writes.  Letter t
 *                              of y is letter lb + t of frame g's translation of the WHOLE sequence of N nucleotides, off = g % 3:
 *                              lb = (r_beg - off) / 3 on strand 0, lb = (N - off - (r_beg + r_len)) / 3 on strand 1 (r_len as resolved).
 *                              Diagonals are the seeds': d = j - i, j a letter of that whole-frame translation; cell (i, j) exists iff
 *                              0 <= i < L and lb <= j < lb + len(y).  Record {U, d, i, i + d}.  Bad candidate, besides the gather's own
 *                              rule: a byte other than 0 or 3; g outside 0 .. 5 or g / 3 != byte / 3; a window that is not codon-aligned
 *                              for frame g (one of the two divisions above leaves a remainder); diag_min > diag_max.
 *   PMX_SEED_LIST_REF_CODONS   The lists of pmx_seed_pairs_translated_ref[_device] with PMX_SEED_REF_CODONS; the byte is a strand of the
 *                              reference.  x is the query window of m letters; T is the codon stream of the oriented reference window
 *                              [lo, hi), hi - lo - 2 letters, as pmx_gather_pairs_codons_ref_device writes it; lo = r_beg on strand 0,
 *                              lo = N - (r_beg + r_len) on strand 1.  Cell (p, x) exists iff 0 <= p < m, lo <= x <= hi - 3 and x = D + 3 p
 *                              for a D in [diag_min, diag_max]; x is an oriented position in the WHOLE sequence, the seeds' coordinate,
 *                              and the cell scores x[p] against T[x - lo].  The cells of one D are walked in ascending p.  Record
 *                              {U, D, p, x + 2}: end_ref is the last nucleotide of the last codon, in oriented whole-sequence coordinates.
 * In the codon kinds a bad candidate is what the gather makes one (a bad descriptor, a byte above 1, a window of fewer than three
 * nucleotides) or diag_min > diag_max.
 *
 * max_qlen and max_rlen bound what the corresponding gather entry bounds: letters; on a codon side the stream's W - 2; on the translated
 * side of PMX_SEED_LIST_REF_FRAMES the letters of the window's translation.  An ungapped score is a sum over at most the cells of the
 * longest diagonal -- one per codon of a stream, and never more than the other side's letters --, and max |w| times that count has to
 * fit int32.
 *
 * The entries take the arguments of their untranslated counterparts with list_kind in place of byte_kind, use the same thread scratch,
 * and behave like them: both device entries are ASYNCHRONOUS on the caller's stream, pmx_seed_filter_translated returns a
 * pmx_seed_filtered_t released with pmx_seed_filtered_free, n == 0 succeeds, the selection is the same code.  Refused with -1 and a
 * pmx_last_error() text before any GPU work: everything the entries above refuse, with their texts; an unknown list_kind (the text names
 * the three constants); max |w| x the longest diagonal's cells >= 2^31.  pmx_last_kernel() reports the form that ran.
 *
 * Out of scope: x-drop, begin positions, narrowing the window of a kept candidate, PSSM, both sides translated. */
#define PMX_SEED_LIST_CODONS     1
#define PMX_SEED_LIST_REF_FRAMES 2
#define PMX_SEED_LIST_REF_CODONS 3
int pmx_seed_ungapped_translated_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                                        const pmx_pair_t *d_pairs, const uint8_t *d_byte /* or NULL */, int list_kind, const uint8_t *code,
                                        const pmx_seed_hit_t *d_seeds, int32_t max_qlen, int32_t max_rlen,
                                        pmx_ungapped_t *d_out /* n */, void *stream, const pmx_pairs_opts_t *opts);
int pmx_seed_ungapped_translated(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                                 const pmx_pair_t *pairs, const uint8_t *byte /* or NULL */, int list_kind, const uint8_t *code,
                                 const pmx_seed_hit_t *seeds, pmx_ungapped_t *out /* n */, const pmx_pairs_opts_t *opts);
int pmx_seed_filter_translated_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                                      const pmx_pair_t *d_pairs, const uint8_t *d_byte /* or NULL */, int list_kind, const uint8_t *code,
                                      const pmx_seed_hit_t *d_seeds, int32_t max_qlen, int32_t max_rlen,
                                      int64_t nq, const int64_t *d_row_off /* nq + 1 */, const pmx_seed_filter_opts_t *fopts,
                                      pmx_pair_t *d_out_pairs, uint8_t *d_out_byte, pmx_seed_hit_t *d_out_seeds, pmx_ungapped_t *d_out_ungapped,
                                      int64_t *d_out_source, int64_t capacity, int64_t *d_out_row_off /* nq + 1 */,
                                      int64_t *d_counts /* [0] kept, [1] written */, void *stream, const pmx_pairs_opts_t *opts);
int pmx_seed_filter_translated(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, const pmx_seed_hits_t *hits,
                               int list_kind, const uint8_t *code, const pmx_seed_filter_opts_t *fopts, const pmx_pairs_opts_t *opts,
                               pmx_seed_filtered_t **result);

/* Long pairs with traceback in linear memory (extension).  pmx_align_batch_cigar and the one-pair *_trace_* functions keep one byte
 * per DP cell outside the packed kernels' window (20 kbp x 20 kbp: 400 MB, 100 kbp x 100 kbp: 10 GB on the device and the host).
 * This entry keeps tile boundaries only: the long-pair sweep (the bands of a pair spread across the chip) stores the row it hands from
 * band to band and the (H, E) of every tile_cols-th column, and a walk re-derives, from the end cell backwards, just the tiles the
 * optimal path enters.  No buffer on the device or the host is proportional to qlen x rlen; pmx_long_cigar_scratch_bytes() tells the
 * checkpoint scratch of one chunk of pairs for given maxima (no GPU needed; -1 with a pmx_last_error() text for options not offered).
 * Beside it the call keeps, for the whole batch, 4 bytes per op slot (qlen + rlen + 1 slots per pair; the device entry, which sees
 * only the maxima, n x (max_qlen + max_rlen + 1)), 8 bytes per pair and the text.
 * cfg->want must contain PMX_WANT_CIGAR and/or PMX_WANT_STATS; PMX_WANT_SORTED is allowed.  NW, SG with any free ends, SW; square
 * matrices of up to 64 letters; any open >= 0, extend >= 0 the long-pair kernel takes; any lengths >= 1 (pairs shorter than a band or a
 * tile are correct, not fast).  Records are the 32-bit records of pmx_align_batch for the same pair (cfg->width is ignored); CIGAR text,
 * letters (PMX_CIGAR_SWAP_ID) and statistics are those of pmx_align_batch_cigar / the statistics kernels.  The text follows
 * pmx_align_batch_cigar (a block freed with pmx_free, cigar_off n + 1 entries); the device entry follows
 * pmx_align_batch_cigar_device (n + 1 offsets starting at 0; a pair whose text would cross cigar_capacity is not written; asynchronous
 * on `stream`: a call whose scratch is already large enough returns without a host synchronisation; the first call of a thread, and
 * one that needs more scratch than any before it, allocate, which synchronises).  opts == NULL or a zero field: the default.  tile_cols: 64, 128 or 256; band_rows: 128, 256 or
 * 1024.  The choice never changes a result.
 * The bands of a pair wait for one another with a bounded wait (pmx_align_batch on long pairs does the same); should a wait run out,
 * the host entry returns -3 with a pmx_last_error() text and no alignment; the device entry leaves every record of that chunk of
 * pairs and of the later ones with PMX_FLAG_RERUN, an empty text and zero statistics (earlier chunks are complete): a record with
 * PMX_FLAG_RERUN means the call has to be redone.  Refused with -1 and a pmx_last_error() text before any GPU work: PSSM matrices,
 * a want without PMX_WANT_CIGAR and PMX_WANT_STATS, options not offered, bad offsets. */
typedef struct pmx_long_cigar_opts { int tile_cols; int band_rows; } pmx_long_cigar_opts_t;   /* 0 = default */
int pmx_align_batch_cigar_long(const pmx_config_t *cfg, int64_t n,
                               const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                               pmx_record_t *out, pmx_stats_t *stats_out /* NULL unless WANT_STATS */,
                               char **cigar_buf, int64_t *cigar_off /* NULL unless WANT_CIGAR */,
                               const pmx_long_cigar_opts_t *opts);
int pmx_align_batch_cigar_long_device(const pmx_config_t *cfg, int64_t n,
                                      const uint8_t *d_qbuf, const int64_t *d_qoff, const uint8_t *d_rbuf, const int64_t *d_roff,
                                      int32_t max_qlen, int32_t max_rlen, pmx_record_t *d_out, pmx_stats_t *d_stats_out,
                                      char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off, void *stream,
                                      const pmx_long_cigar_opts_t *opts);
long long pmx_long_cigar_scratch_bytes(int64_t n, int32_t max_qlen, int32_t max_rlen, const pmx_long_cigar_opts_t *opts);

/* CIGAR text for a batch (semi-global / global / local with traceback done on the device).
 * cigar_off has n+1 entries; *cigar_buf is malloc'd by the callee and freed with pmx_free.  A PSSM: every query has its length. */
int pmx_align_batch_cigar(const pmx_config_t *cfg, int64_t n,
                          const uint8_t *qbuf, const int64_t *qoff,
                          const uint8_t *rbuf, const int64_t *roff,
                          pmx_record_t *out, char **cigar_buf, int64_t *cigar_off);
void pmx_free(void *p);

/* The same with device-resident pairs (all pointers are device pointers on the current device, the offset arrays
 * start at 0), asynchronous on `stream`.  d_cigar_off receives n+1 offsets into d_cigar_text (the last one is the
 * number of text bytes the batch needs); a pair whose text would cross cigar_capacity is not written, so a caller
 * that sees d_cigar_off[n] > cigar_capacity calls again with a larger buffer.  Inside, the traceback sweep and the
 * walk of consecutive chunks overlap on two streams.  Returns <0 when the configuration has no packed-traceback
 * kernel (width 8, PSSM, open < extend, score + open beyond a byte, queries beyond 1023 symbols); the host entry
 * above handles those. */
int pmx_align_batch_cigar_device(const pmx_config_t *cfg, int64_t n,
                                 const uint8_t *d_qbuf, const int64_t *d_qoff,
                                 const uint8_t *d_rbuf, const int64_t *d_roff,
                                 int32_t max_qlen, int32_t max_rlen,
                                 pmx_record_t *d_out, char *d_cigar_text, int64_t cigar_capacity,
                                 int64_t *d_cigar_off, void *stream);

/* Score tables for a batch (extension: the reference returns one table per call, src/alignment/mod.rs:123-192).  All pointers are
 * device pointers, asynchronous on `stream`.  d_tab_off[k] (n + 1 entries) = cells before pair k's [qlen][rlen] int32 row-major
 * table in d_score_table; d_score_row (last rows) is packed like the references, d_score_col (last columns) like the queries;
 * any of the three outputs, and d_out, may be NULL.  4 bytes per cell: this is the one output of the path that is bound by HBM
 * write bandwidth. */
int pmx_align_batch_table_device(const pmx_config_t *cfg, int64_t n,
                                 const uint8_t *d_qbuf, const int64_t *d_qoff,
                                 const uint8_t *d_rbuf, const int64_t *d_roff,
                                 int32_t max_qlen, int32_t max_rlen,
                                 const int64_t *d_tab_off, int32_t *d_score_table,
                                 int32_t *d_score_row, int32_t *d_score_col,
                                 pmx_record_t *d_out, void *stream);

/* Multi-GPU (one process driving several GPUs of a node).  Pairs are independent, so the batch is cut into ndev contiguous
 * blocks with about equal numbers of cells (sum of qlen * rlen; pmx_shard_bounds_by_cells is the planner), block g runs on
 * devices[g] from its own persistent host thread, and every block's records land in `out` at its pairs' positions: input order,
 * no collective.  A device may be listed more than once.  (One process per GPU instead: shard with the same planner and gather
 * the 16-byte records, e.g. RCCL over xGMI -- see INTEGRATION.md.) */
int pmx_align_batch_multi(const pmx_config_t *cfg, int64_t n,
                          const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                          const int *devices, int ndev, pmx_record_t *out, pmx_stats_t *stats_out);
int pmx_align_profile_batch_multi(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                  const uint8_t *rbuf, const int64_t *roff,
                                  const int *devices, int ndev, pmx_record_t *out, pmx_stats_t *stats_out);
/* (a PSSM: the rules of pmx_align_batch / pmx_align_profile_batch) */
/* bounds[0..parts]: block g = pairs [bounds[g], bounds[g+1]).  qoff == NULL: one shared query.  Pure host arithmetic. */
int pmx_shard_bounds_by_cells(int64_t n, const int64_t *qoff, const int64_t *roff, int parts, int64_t *bounds);

/* Optional: page-lock caller-owned host buffers once, so the host-buffer entries above move them at full PCIe rate. */
int pmx_host_register(void *p, size_t bytes);
int pmx_host_unregister(void *p);

/* Runtime. */
int pmx_device_count(void);
int pmx_set_device(int device);            /* per calling thread, like hipSetDevice */
const char *pmx_last_error(void);
const char *pmx_version(void);
/* Name of the kernel family the dispatcher would use for a config and size (diagnostics). */
const char *pmx_kernel_for(const pmx_config_t *cfg, int32_t max_qlen, int32_t max_rlen);
/* Name (with template shape and arithmetic variant) of the kernel the calling thread's last batch call launched. */
const char *pmx_last_kernel(void);
/* Every environment switch the library reads, one "NAME\tkind\twhat\n" line each (parasail-rs_amd/csrc/pmx_switches.h). */
const char *pmx_switches(void);
/* Deferred results (environment switch PMX_DEFER_ALIGN=1): the one-pair alignment functions (score and statistics names) queue the
 * pair and return a PENDING parasail_result_t; the first accessor (parasail_result_get_score, ...) of any pending result of that
 * thread -- or a queue of 262 144 pairs, or a call with another configuration -- runs the queue as ONE batch launch.  The mode / width
 * predicates answer at once; freeing a pending result withdraws it.  pmx_flush_deferred() runs the calling thread's queue now. */
void pmx_flush_deferred(void);
/* The 66 matrix names the reference documents (src/matrix/mod.rs:46-50), one per line, into buf (NUL-terminated, truncated to cap);
 * returns the bytes needed.  parasail_matrix_lookup() embeds blosum62 / nuc44 and resolves the others from files (pmx_last_error()
 * tells a documented name whose file is missing from an unknown name, and why a file was refused). */
int pmx_documented_matrix_names(char *buf, int cap);
/* Test hooks of the band-strip kernel (parasail-rs_amd/csrc/pmx_bstrip.hip; model: tests/bstrip_model.py): the host's window
 * predicate -- 1 and the bias / low constants of the stored form when the int16 window holds a launch of that shape, else 0 -- and
 * the lane shape (lanes per pair, offsets per lane) chosen for a band. */
int pmx_bstrip_window(int mode, int max_qlen, int max_rlen, int open, int extend, int score_min, int score_max, int capacity, int rows,
                      int double_skew, int *bias, int *low);
int pmx_bstrip_shape(int band, int *lanes_per_pair, int *offsets_per_lane);
/* Launch geometry of the band-strip kernel for a batch with queries <= max_qlen and references <= max_rlen (band, lane shape, one
 * shared query or not): the most row steps a pair runs, the bytes per lane group of the query and selector streams, the dynamic
 * LDS.  1, or 0 on an argument out of range. */
int pmx_bstrip_geometry(int max_qlen, int max_rlen, int band, int lanes_per_pair, int offsets_per_lane, int q_shared,
                        int *rows, int *query_stream, int *selector_stream, long long *lds);
/* Test hook of the banded traceback (parasail-rs_amd/csrc/pmx_banded.hip): the one bound of its trace scratch for a batch with
 * queries <= max_qlen and references <= max_rlen (one shared query or not) -- lanes per pair, step pairs per pair, bytes per pair
 * region (rows * lanes).  1, or 0 on an argument out of range. */
int pmx_bandtr_geometry(int max_qlen, int max_rlen, int band, int q_shared, int *lanes_per_pair, int *rows, long long *stride);
/* Test hook of the packed global / semi-global kernels (pmx_nwsg16.hip; model: tests/nwsgv_model.c): the host's range proof --
 * the bias nb of the stored form when the int16 window holds every pair of up to max_qlen x max_rlen under this scoring in a shape of
 * shape_rows rows (0: the dispatcher's estimate before a shape is picked), else 0.  rowx: the row-offset form (every width but 8). */
int pmx_window_nwsgv(int max_qlen, int max_rlen, int msize, int score_min, int score_max, int open, int extend, int rowx, int shape_rows);
/* Test hook of the traceback planners (host arithmetic only, no device needed; expected values: tests/golden/trace_plans.json): the
 * sweep planned for n pairs of up to max_qlen x max_rlen under this scoring -- the per-pair plan (packed_ok 0: first-generation sweeps
 * only), or with q_shared > 0 the shared-query plan (short_waves 1: without the shapes of 19 and 20 rows per lane).  Returns 0 with the
 * family (0 trace16, 1 nwsg16v, 2 nwsg16m, 3 sw16, 4 sw16m, 5 nwsg16q), lanes per pair G, rows per lane R, steps Tmax and the trace
 * scratch in bytes; or 1, not eligible, with all five 0. */
int pmx_trace_plan_probe(int mode, int msize, int score_min, int score_max, int pssm, int open, int extend, long long n,
                         int max_qlen, int max_rlen, int q_shared, int short_waves, int packed_ok,
                         int *family, int *G, int *R, int *Tmax, long long *trace_bytes);
/* Test hook of the long-pair sweep's planning (host arithmetic only, no device needed; expected values: tests/golden/long_plans.json):
 * the sweep planned for n pairs of up to max_qlen x max_rlen on road 0 (pmx_align_batch's score road: mode feeds its time model) or
 * road 1 (pmx_align_batch_cigar_long: tile_cols / band_rows as in pmx_long_cigar_opts_t), with what the PMX_LONG_* switches and the
 * device would say as arguments: the scratch budget of one chunk in bytes and whether it was forced, two_columns / one_column (0 / 1),
 * rows_per_lane (0 = not set) and chunk_cols (16 or 64).  Returns 0 with out[0 .. 8] = rows per lane, columns per step, steps per
 * boundary chunk, bands of the longest query, granules per (pair, band) boundary, pairs per chunk, bytes of a chunk's scratch in front
 * of the checkpoints, bytes of the checkpoints, checkpoint slots per (pair, band); or 1, refused, with all nine 0. */
int pmx_long_plan_probe(int road, int mode, long long n, int max_qlen, int max_rlen, double budget, int budget_forced,
                        int two_columns, int one_column, int rows_per_lane, int chunk_cols, int tile_cols, int band_rows, long long *out);
/* Test hook of the seeding entries' planning (host arithmetic only, no device needed; expected values: tests/golden/seed_plans.json):
 * the run planned for nq rows of up to max_qlen letters by the entries of an index of `kind` (0 pmx_seed_pairs, 1 pmx_seed_pairs_letters,
 * 2 pmx_seed_pairs_translated_ref) under `mode` (opts->strand, query_mode, ref_mode) with opts->max_occ and opts->slice_rows, against a
 * set of ref_count sequences, with what pmx_seed_match_budget would say as an argument (budget in bytes, 0: the default).  Returns 0 with
 * out[0 .. 10] = orientations per row, the first one's strand or frame (-1 where a letters or translated index reads the rows as they
 * stand), segments per row, position slots per segment, position slots per row, scratch bytes per position slot, rows per slice, the
 * match buffer's entries, position slots per slice, rows x orientations per slice, sorted bits of a match key; 1 with all eleven 0
 * where one row's worst case does not fit the budget; -1 on an argument no entry would plan. */
int pmx_seed_plan_probe(int kind, int mode, long long nq, int max_qlen, int max_occ, long long slice_rows, long long budget,
                        long long ref_count, long long *out);
/* ... and with the window of the index as an argument: w = 1 is pmx_seed_plan_probe, number for number; w in 2 .. 64 (kind 0 only) is the
 * plan of a minimizer index, whose position slots take one scratch byte more.  -1 also for w outside 1 .. 64 or w > 1 with kind != 0. */
int pmx_seed_plan_probe_w(int kind, int mode, long long nq, int max_qlen, int max_occ, long long slice_rows, long long budget,
                          long long ref_count, int w, long long *out);

#ifdef __cplusplus
}
#endif
#endif /* PARASAIL_AMD_H */
