//! Additive batch entry points of `libparasail_amd.so` for parasail-rs' `Aligner`.
//!
//! NOT COMPILED in the image this repository is built in (no rustc / cargo there): written against parasail-rs as found under
//! `/root/reference` (`src/aligner/mod.rs`, `src/alignment/mod.rs`, `src/matrix/mod.rs`, `src/profile/mod.rs`) and against the
//! C declarations in `include/parasail_amd.h`, which are exercised through the ctypes and C++ mirrors of this same interface.
//!
//! `Aligner::align()` keeps the reference's one-pair semantics (`src/aligner/mod.rs:397-452`); the functions here hand MANY
//! independent pairs to the GPU in one call, which is where the throughput is (one pair cannot fill 256 compute units).
//!
//! Fields to add to `struct Aligner` (`src/aligner/mod.rs:372-382`), filled in `AlignerBuilder::build()` (`:339-369`) from what
//! the builder already knows:
//!
//! ```ignore
//! // batch: 0 nw, 1 sg, 2 sw                    <- self.mode  ("nw" | "sg" | "sw", :59-61)
//! pub(crate) mode_id: i32,
//! // batch: 1 query begin | 2 query end | 4 ref begin | 8 ref end are free  <- allow_query_gaps / allow_ref_gaps (:270-299);
//! //        plain "sg" = 15
//! pub(crate) sg_flags: i32,
//! // batch: 0 = sat, 8, 16, 32, 64               <- self.solution_width (:125-137)
//! pub(crate) width: i32,
//! // batch: use_stats / use_trace                <- self.use_stats, self.use_trace (:210-267)
//! pub(crate) want_stats: bool,
//! pub(crate) want_trace: bool,
//! ```
use crate::{Aligner, Error, Result};
use libparasail_sys::{parasail_matrix_t, parasail_profile_t};
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

/// `pmx_config_t` (include/parasail_amd.h)
#[repr(C)]
pub struct PmxConfig {
    pub mode: c_int,     // 0 nw, 1 sg, 2 sw
    pub sg_flags: c_int, // 1 qb | 2 qe | 4 db | 8 de
    pub open: c_int,
    pub extend: c_int,
    pub width: c_int, // 0 sat, 8, 16, 32, 64
    pub want: c_int,  // 1 stats | 2 cigar | 4 ragged lengths: process in length-sorted order
    pub matrix: *const parasail_matrix_t,
}

/// `pmx_record_t`: what `Alignment::{get_score,get_end_query,get_end_ref}` return (`src/alignment/mod.rs:64-76`), plus
/// `flags` (bit 0: saturated in the requested width -- `Alignment::is_saturated`, `:436-440`).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct PmxRecord {
    pub score: i32,
    pub end_query: i32,
    pub end_ref: i32,
    pub flags: i32,
}

/// `pmx_stats_t`: `Alignment::{get_matches,get_similar,get_length}` (`src/alignment/mod.rs:79-98`).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct PmxStats {
    pub matches: i32,
    pub similar: i32,
    pub length: i32,
}

/// `pmx_long_cigar_opts_t`: tile width and band height of the tiled long-pair traceback (0 = default; never change a result).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct PmxLongCigarOpts {
    pub tile_cols: c_int,
    pub band_rows: c_int,
}

/// `pmx_search_opts_t`: threshold, limit (0 = none), order and band of a profile search (`band < 0`: no second pass).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct PmxSearchOpts {
    pub min_score: i32,
    pub max_hits: i64,
    pub order: i32,
    pub band: i32,
}

/// `pmx_hit_t`: one hit of a profile search -- index of the reference, its first-pass record, the diagonal the second pass was
/// centred on and the first cell of the second pass's path (-1 without one).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct PmxHit {
    pub index: i64,
    pub first: PmxRecord,
    pub diag: i32,
    pub beg_query: i32,
    pub beg_ref: i32,
    pub reserved: i32,
}

/// `pmx_search_result_t`: one callee-allocated block, released with `pmx_search_result_free`.
#[repr(C)]
pub struct PmxSearchResult {
    pub n_hits: i64,
    pub n_passing: i64,
    pub hits: *mut PmxHit,
    pub recs: *mut PmxRecord,
    pub stats: *mut PmxStats,
    pub cigar: *mut c_char,
    pub cigar_off: *mut i64,
}

pub const PMX_HITS_BY_INDEX: i32 = 0;
pub const PMX_HITS_BY_SCORE: i32 = 1;
pub const PMX_WANT_STATS: c_int = 1;
pub const PMX_WANT_CIGAR: c_int = 2;
pub const PMX_WANT_SORTED: c_int = 4;

/// One pair of a sequence-set batch (`pmx_pair_t`, 32 bytes): sequence indices and windows; a length of -1 runs to the sequence's end.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct PmxPair {
    pub q: i64,
    pub r: i64,
    pub q_beg: i32,
    pub q_len: i32,
    pub r_beg: i32,
    pub r_len: i32,
}

impl PmxPair {
    /// Whole sequences `q` and `r`.
    pub fn whole(q: i64, r: i64) -> PmxPair {
        PmxPair { q, r, q_beg: 0, q_len: -1, r_beg: 0, r_len: -1 }
    }
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct PmxPairsOpts {
    pub chunk_pairs: i64, // 0 = default; never changes a result
}

/// Record flag of the set-batch device entries: the descriptor was bad, nothing was aligned.
pub const PMX_FLAG_BAD_PAIR: i32 = 8;

/// Shapes of a set search: a descriptor list, a window of the strict upper triangle of Q, a window of the row-major rectangle Q x R.
pub const PMX_PAIRS_LIST: c_int = 0;
pub const PMX_PAIRS_TRIANGLE: c_int = 1;
pub const PMX_PAIRS_RECT: c_int = 2;

/// `pmx_pair_search_opts_t` (32 bytes).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct PmxPairSearchOpts {
    pub min_score: i32,
    pub shape: i32,
    pub max_hits: i64,    // 0 = no limit
    pub chunk_pairs: i64, // 0 = default; never changes a result
    pub slice_pairs: i64, // 0 = 2^24; never changes a result
}

/// `pmx_pair_hits_t`: one callee-allocated block, released with `pmx_pair_hits_free`.
#[repr(C)]
pub struct PmxPairHits {
    pub n_hits: i64,
    pub n_passing: i64,
    pub pairs: *mut PmxPair,
    pub index: *mut i64,
    pub recs: *mut PmxRecord,
    pub stats: *mut PmxStats,
}

/// `pmx_topk_opts_t` (32 bytes).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct PmxTopkOpts {
    pub min_score: i32,   // i32::MIN = pure top-K
    pub k: i32,           // 1 ..= PMX_TOPK_MAX
    pub skip_self: i32,   // R must be Q: the pair (i, i) is never a candidate
    pub chunk_pairs: i64, // 0 = default; never changes a result
    pub slice_rows: i64,  // 0 = default; never changes a result
}

pub const PMX_TOPK_MAX: i32 = 1024;

/// `pmx_topk_hits_t`: one callee-allocated block, released with `pmx_topk_hits_free`.
#[repr(C)]
pub struct PmxTopkHits {
    pub n_rows: i64,
    pub n_hits: i64,
    pub n_passing: i64,
    pub row_off: *mut i64,
    pub row_passing: *mut i64,
    pub pairs: *mut PmxPair,
    pub index: *mut i64,
    pub recs: *mut PmxRecord,
    pub stats: *mut PmxStats,
}

/// Opaque `pmx_seqset_t`.
#[repr(C)]
pub struct PmxSeqSet {
    _private: [u8; 0],
}

#[link(name = "parasail_amd")]
extern "C" {
    fn pmx_seqset_create(buf: *const u8, off: *const i64, count: i64) -> *mut PmxSeqSet;
    fn pmx_seqset_wrap_device(d_buf: *const u8, d_off: *const i64, count: i64, bytes: i64) -> *mut PmxSeqSet;
    fn pmx_seqset_free(set: *mut PmxSeqSet);
    fn pmx_seqset_count(set: *const PmxSeqSet) -> i64;
    fn pmx_align_pairs(
        cfg: *const PmxConfig, q: *const PmxSeqSet, r: *const PmxSeqSet, n: i64, pairs: *const PmxPair,
        out: *mut PmxRecord, stats_out: *mut PmxStats, opts: *const PmxPairsOpts,
    ) -> c_int;
    pub fn pmx_align_pairs_device(
        cfg: *const PmxConfig, q: *const PmxSeqSet, r: *const PmxSeqSet, n: i64, d_pairs: *const PmxPair,
        max_qlen: i32, max_rlen: i32, d_out: *mut PmxRecord, d_stats_out: *mut PmxStats, stream: *mut c_void,
        opts: *const PmxPairsOpts,
    ) -> c_int;
    /// The 256-byte complement a strand-1 query window is mapped through.
    pub fn pmx_complement_table(table: *mut u8);
    /// Set batches with one strand byte per pair (NULL: all forward) and, with PMX_WANT_CIGAR, CIGAR text (a block released with
    /// pmx_free, `cigar_off` n + 1 entries) and the begins of the paths (2 n, optional).
    pub fn pmx_align_pairs_ex(
        cfg: *const PmxConfig, q: *const PmxSeqSet, r: *const PmxSeqSet, n: i64, pairs: *const PmxPair, strand: *const u8,
        out: *mut PmxRecord, stats_out: *mut PmxStats, beg: *mut i32, cigar_buf: *mut *mut c_char, cigar_off: *mut i64,
        opts: *const PmxPairsOpts,
    ) -> c_int;
    pub fn pmx_align_pairs_ex_device(
        cfg: *const PmxConfig, q: *const PmxSeqSet, r: *const PmxSeqSet, n: i64, d_pairs: *const PmxPair, d_strand: *const u8,
        max_qlen: i32, max_rlen: i32, d_out: *mut PmxRecord, d_stats_out: *mut PmxStats, d_beg: *mut i32,
        d_cigar_text: *mut c_char, cigar_capacity: i64, d_cigar_off: *mut i64, stream: *mut c_void, opts: *const PmxPairsOpts,
    ) -> c_int;
    pub fn pmx_gather_pairs_device(
        q: *const PmxSeqSet, r: *const PmxSeqSet, n: i64, d_pairs: *const PmxPair, d_strand: *const u8, max_qlen: i32, max_rlen: i32,
        d_qout: *mut u8, q_capacity: i64, d_qoff: *mut i64, d_rout: *mut u8, r_capacity: i64, d_roff: *mut i64, d_ok: *mut u8,
        stream: *mut c_void,
    ) -> c_int;
    fn pmx_all_pairs_count(nseq: i64) -> i64;
    fn pmx_all_pairs_index(nseq: i64, p: i64, i: *mut i64, j: *mut i64) -> c_int;
    fn pmx_align_all_pairs(
        cfg: *const PmxConfig, s: *const PmxSeqSet, first: i64, count: i64,
        out: *mut PmxRecord, stats_out: *mut PmxStats, opts: *const PmxPairsOpts,
    ) -> c_int;
    pub fn pmx_align_all_pairs_device(
        cfg: *const PmxConfig, s: *const PmxSeqSet, first: i64, count: i64, max_len: i32,
        d_out: *mut PmxRecord, d_stats_out: *mut PmxStats, stream: *mut c_void, opts: *const PmxPairsOpts,
    ) -> c_int;
    pub fn pmx_all_pairs_enumerate_device(nseq: i64, first: i64, count: i64, d_pairs: *mut PmxPair, stream: *mut c_void) -> c_int;
    fn pmx_rect_pairs_count(nq: i64, nr: i64) -> i64;
    pub fn pmx_rect_pairs_enumerate_device(nq: i64, nr: i64, first: i64, count: i64, d_pairs: *mut PmxPair, stream: *mut c_void) -> c_int;
    /// Set search into caller buffers on the device: `d_counts[0]` pairs pass, `d_counts[1] = min(passing, capacity)` are written.
    pub fn pmx_search_pairs_device(
        cfg: *const PmxConfig, q: *const PmxSeqSet, r: *const PmxSeqSet, shape: c_int, first: i64, n: i64, d_pairs: *const PmxPair,
        max_qlen: i32, max_rlen: i32, min_score: i32, d_hit_pairs: *mut PmxPair, d_hit_index: *mut i64, d_hit_recs: *mut PmxRecord,
        d_hit_stats: *mut PmxStats, capacity: i64, d_counts: *mut i64, stream: *mut c_void, opts: *const PmxPairsOpts,
    ) -> c_int;
    fn pmx_search_pairs(
        cfg: *const PmxConfig, q: *const PmxSeqSet, r: *const PmxSeqSet, first: i64, n: i64, pairs: *const PmxPair,
        opts: *const PmxPairSearchOpts, result: *mut *mut PmxPairHits,
    ) -> c_int;
    fn pmx_pair_hits_free(hits: *mut PmxPairHits);
    /// Per-query top-K into caller buffers on the device, CSR: `d_row_off` gets `nq + 1` offsets, `d_counts` kept / written / passing.
    pub fn pmx_search_topk_device(
        cfg: *const PmxConfig, q: *const PmxSeqSet, r: *const PmxSeqSet, q_first: i64, nq: i64, max_qlen: i32, max_rlen: i32,
        min_score: i32, k: i32, skip_self: i32, d_hit_pairs: *mut PmxPair, d_hit_index: *mut i64, d_hit_recs: *mut PmxRecord,
        d_hit_stats: *mut PmxStats, capacity: i64, d_row_off: *mut i64, d_row_passing: *mut i64, d_counts: *mut i64,
        stream: *mut c_void, opts: *const PmxPairsOpts,
    ) -> c_int;
    fn pmx_search_topk(
        cfg: *const PmxConfig, q: *const PmxSeqSet, r: *const PmxSeqSet, q_first: i64, nq: i64, opts: *const PmxTopkOpts,
        result: *mut *mut PmxTopkHits,
    ) -> c_int;
    fn pmx_topk_hits_free(hits: *mut PmxTopkHits);
    fn pmx_align_batch(
        cfg: *const PmxConfig, n: i64,
        qbuf: *const u8, qoff: *const i64, rbuf: *const u8, roff: *const i64,
        out: *mut PmxRecord, stats_out: *mut PmxStats,
    ) -> c_int;
    fn pmx_align_profile_batch(
        cfg: *const PmxConfig, profile: *const parasail_profile_t, n: i64,
        rbuf: *const u8, roff: *const i64,
        out: *mut PmxRecord, stats_out: *mut PmxStats,
    ) -> c_int;
    fn pmx_align_batch_cigar(
        cfg: *const PmxConfig, n: i64,
        qbuf: *const u8, qoff: *const i64, rbuf: *const u8, roff: *const i64,
        out: *mut PmxRecord, cigar_buf: *mut *mut c_char, cigar_off: *mut i64,
    ) -> c_int;
    fn pmx_align_batch_banded(
        cfg: *const PmxConfig, profile: *const parasail_profile_t, n: i64,
        qbuf: *const u8, qoff: *const i64, rbuf: *const u8, roff: *const i64,
        band: i32, diag: *const i32, out: *mut PmxRecord,
    ) -> c_int;
    fn pmx_align_batch_banded_cigar(
        cfg: *const PmxConfig, profile: *const parasail_profile_t, n: i64,
        qbuf: *const u8, qoff: *const i64, rbuf: *const u8, roff: *const i64,
        band: i32, diag: *const i32, out: *mut PmxRecord, stats_out: *mut PmxStats,
        cigar_buf: *mut *mut c_char, cigar_off: *mut i64,
    ) -> c_int;
    pub fn pmx_align_batch_banded_cigar_device(
        cfg: *const PmxConfig, profile: *const parasail_profile_t, n: i64,
        d_qbuf: *const u8, d_qoff: *const i64, d_rbuf: *const u8, d_roff: *const i64,
        max_qlen: i32, max_rlen: i32, band: i32, d_diag: *const i32,
        d_out: *mut PmxRecord, d_stats_out: *mut PmxStats,
        d_cigar_text: *mut c_char, cigar_capacity: i64, d_cigar_off: *mut i64, stream: *mut c_void,
    ) -> c_int;
    fn pmx_align_batch_cigar_long(
        cfg: *const PmxConfig, n: i64,
        qbuf: *const u8, qoff: *const i64, rbuf: *const u8, roff: *const i64,
        out: *mut PmxRecord, stats_out: *mut PmxStats,
        cigar_buf: *mut *mut c_char, cigar_off: *mut i64, opts: *const PmxLongCigarOpts,
    ) -> c_int;
    pub fn pmx_align_batch_cigar_long_device(
        cfg: *const PmxConfig, n: i64,
        d_qbuf: *const u8, d_qoff: *const i64, d_rbuf: *const u8, d_roff: *const i64,
        max_qlen: i32, max_rlen: i32, d_out: *mut PmxRecord, d_stats_out: *mut PmxStats,
        d_cigar_text: *mut c_char, cigar_capacity: i64, d_cigar_off: *mut i64, stream: *mut c_void,
        opts: *const PmxLongCigarOpts,
    ) -> c_int;
    pub fn pmx_long_cigar_scratch_bytes(n: i64, max_qlen: i32, max_rlen: i32, opts: *const PmxLongCigarOpts) -> i64;
    fn pmx_align_batch_multi(
        cfg: *const PmxConfig, n: i64,
        qbuf: *const u8, qoff: *const i64, rbuf: *const u8, roff: *const i64,
        devices: *const c_int, ndev: c_int, out: *mut PmxRecord, stats_out: *mut PmxStats,
    ) -> c_int;
    fn pmx_align_profile_batch_multi(
        cfg: *const PmxConfig, profile: *const parasail_profile_t, n: i64,
        rbuf: *const u8, roff: *const i64,
        devices: *const c_int, ndev: c_int, out: *mut PmxRecord, stats_out: *mut PmxStats,
    ) -> c_int;
    fn pmx_align_batch_2bit(
        cfg: *const PmxConfig, n: i64,
        q2: *const u8, qoff: *const i64, r2: *const u8, roff: *const i64,
        out: *mut PmxRecord, stats_out: *mut PmxStats,
    ) -> c_int;
    // device-pointer entries (asynchronous on a hipStream_t): for callers that already hold their sequences in HBM
    pub fn pmx_align_batch_device(
        cfg: *const PmxConfig, n: i64,
        d_qbuf: *const u8, d_qoff: *const i64, d_rbuf: *const u8, d_roff: *const i64,
        max_qlen: i32, max_rlen: i32,
        d_out: *mut PmxRecord, d_stats: *mut PmxStats, stream: *mut c_void,
    ) -> c_int;
    pub fn pmx_align_profile_batch_device(
        cfg: *const PmxConfig, profile: *const parasail_profile_t, n: i64,
        d_rbuf: *const u8, d_roff: *const i64, max_rlen: i32,
        d_out: *mut PmxRecord, d_stats: *mut PmxStats, stream: *mut c_void,
    ) -> c_int;
    pub fn pmx_align_batch_cigar_device(
        cfg: *const PmxConfig, n: i64,
        d_qbuf: *const u8, d_qoff: *const i64, d_rbuf: *const u8, d_roff: *const i64,
        max_qlen: i32, max_rlen: i32, d_out: *mut PmxRecord,
        d_cigar_text: *mut c_char, cigar_capacity: i64, d_cigar_off: *mut i64, stream: *mut c_void,
    ) -> c_int;
    pub fn pmx_align_batch_table_device(
        cfg: *const PmxConfig, n: i64,
        d_qbuf: *const u8, d_qoff: *const i64, d_rbuf: *const u8, d_roff: *const i64,
        max_qlen: i32, max_rlen: i32, d_tab_off: *const i64, d_score_table: *mut i32,
        d_score_row: *mut i32, d_score_col: *mut i32, d_out: *mut PmxRecord, stream: *mut c_void,
    ) -> c_int;
    fn pmx_search_profile(
        cfg: *const PmxConfig, profile: *const parasail_profile_t, n: i64,
        rbuf: *const u8, roff: *const i64, opts: *const PmxSearchOpts, result: *mut *mut PmxSearchResult,
    ) -> c_int;
    fn pmx_search_result_free(result: *mut PmxSearchResult);
    pub fn pmx_search_profile_device(
        cfg: *const PmxConfig, profile: *const parasail_profile_t, n: i64,
        d_rbuf: *const u8, d_roff: *const i64, max_rlen: i32, opts: *const PmxSearchOpts,
        d_first: *mut PmxRecord, d_hits: *mut PmxHit, d_recs: *mut PmxRecord, d_stats: *mut PmxStats, capacity: i64,
        d_cigar_text: *mut c_char, cigar_capacity: i64, d_cigar_off: *mut i64, d_counts: *mut i64, stream: *mut c_void,
    ) -> c_int;
    pub fn pmx_select_hits_device(
        d_rec: *const PmxRecord, n: i64, min_score: i32, max_hits: i64, order: c_int,
        d_hit_index: *mut i64, capacity: i64, d_counts: *mut i64, stream: *mut c_void,
    ) -> c_int;
    pub fn pmx_gather_refs_device(
        d_rbuf: *const u8, d_roff: *const i64, n: i64, d_index: *const i64, h: i64,
        d_out: *mut u8, out_capacity: i64, d_out_off: *mut i64, stream: *mut c_void,
    ) -> c_int;
    pub fn pmx_shard_bounds_by_cells(n: i64, qoff: *const i64, roff: *const i64, parts: c_int, bounds: *mut i64) -> c_int;
    pub fn pmx_host_register(p: *mut c_void, bytes: usize) -> c_int;
    pub fn pmx_host_unregister(p: *mut c_void) -> c_int;
    fn pmx_free(p: *mut c_void);
    fn pmx_last_error() -> *const c_char;
    pub fn pmx_last_kernel() -> *const c_char;
    pub fn pmx_switches() -> *const c_char;
}

/// Sequences packed back to back with `n + 1` byte offsets: the layout of every `pmx_*` batch entry.
pub struct Packed {
    pub buf: Vec<u8>,
    pub off: Vec<i64>,
}

impl Packed {
    pub fn from_slices(seqs: &[&[u8]]) -> Packed {
        let mut off = Vec::with_capacity(seqs.len() + 1);
        let mut buf = Vec::with_capacity(seqs.iter().map(|s| s.len()).sum());
        off.push(0i64);
        for s in seqs {
            buf.extend_from_slice(s);
            off.push(buf.len() as i64);
        }
        Packed { buf, off }
    }
    pub fn len(&self) -> usize {
        self.off.len() - 1
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
}

/// Records, optional statistics.
pub struct BatchResult {
    pub records: Vec<PmxRecord>,
    pub stats: Option<Vec<PmxStats>>,
}

/// CIGAR text of a batch: one callee-allocated block, released with `pmx_free` on drop
/// (the per-pair `CigarString` of `src/alignment/mod.rs:32-44` owns its block the same way).
pub struct BatchCigars {
    text: *mut c_char,
    off: Vec<i64>,
}

impl BatchCigars {
    pub fn len(&self) -> usize {
        self.off.len() - 1
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    /// CIGAR text of pair `k` (e.g. `"93=1X20=2D134="`), the format `Alignment::get_cigar` returns (`src/alignment/mod.rs:390-419`).
    pub fn get(&self, k: usize) -> &str {
        let (a, e) = (self.off[k] as usize, self.off[k + 1] as usize);
        // digits and the letters = X I D only
        unsafe { std::str::from_utf8_unchecked(std::slice::from_raw_parts(self.text.add(a) as *const u8, e - a)) }
    }
}

impl Drop for BatchCigars {
    fn drop(&mut self) {
        if !self.text.is_null() {
            unsafe { pmx_free(self.text as *mut c_void) }
        }
    }
}

unsafe impl Send for BatchCigars {}

/// Hits of a profile search: the callee's block, released with `pmx_search_result_free` on drop.
pub struct SearchHits {
    inner: *mut PmxSearchResult,
}

impl SearchHits {
    fn r(&self) -> &PmxSearchResult {
        unsafe { &*self.inner }
    }
    pub fn len(&self) -> usize {
        self.r().n_hits as usize
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    /// References that reached `min_score`, before `max_hits` cut them.
    pub fn passing(&self) -> i64 {
        self.r().n_passing
    }
    pub fn hits(&self) -> &[PmxHit] {
        unsafe { std::slice::from_raw_parts(self.r().hits, self.len()) }
    }
    /// Records of the banded second pass (`None` with `band < 0`).
    pub fn records(&self) -> Option<&[PmxRecord]> {
        let p = self.r().recs;
        if p.is_null() { None } else { Some(unsafe { std::slice::from_raw_parts(p, self.len()) }) }
    }
    pub fn stats(&self) -> Option<&[PmxStats]> {
        let p = self.r().stats;
        if p.is_null() { None } else { Some(unsafe { std::slice::from_raw_parts(p, self.len()) }) }
    }
    /// CIGAR text of hit `k` (`""` without a second pass).
    pub fn cigar(&self, k: usize) -> &str {
        let r = self.r();
        if r.cigar.is_null() {
            return "";
        }
        let off = unsafe { std::slice::from_raw_parts(r.cigar_off, self.len() + 1) };
        let (a, e) = (off[k] as usize, off[k + 1] as usize);
        unsafe { std::str::from_utf8_unchecked(std::slice::from_raw_parts(r.cigar.add(a) as *const u8, e - a)) }
    }
}

impl Drop for SearchHits {
    fn drop(&mut self) {
        if !self.inner.is_null() {
            unsafe { pmx_search_result_free(self.inner) }
        }
    }
}

unsafe impl Send for SearchHits {}

/// Hits of a set search: the callee's block, released with `pmx_pair_hits_free` on drop.  Hit `x` is the x-th pair of the
/// enumeration that reached `min_score`.
pub struct PairHits {
    inner: *mut PmxPairHits,
}

impl PairHits {
    fn r(&self) -> &PmxPairHits {
        unsafe { &*self.inner }
    }
    pub fn len(&self) -> usize {
        self.r().n_hits as usize
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    /// Pairs that reached `min_score`, before `max_hits` cut them.
    pub fn passing(&self) -> i64 {
        self.r().n_passing
    }
    /// The hits' descriptors: a valid pair list for `Aligner::align_pairs`.
    pub fn pairs(&self) -> &[PmxPair] {
        if self.is_empty() { &[] } else { unsafe { std::slice::from_raw_parts(self.r().pairs, self.len()) } }
    }
    /// The hits' numbers in the enumeration.
    pub fn index(&self) -> &[i64] {
        if self.is_empty() { &[] } else { unsafe { std::slice::from_raw_parts(self.r().index, self.len()) } }
    }
    pub fn records(&self) -> &[PmxRecord] {
        if self.is_empty() { &[] } else { unsafe { std::slice::from_raw_parts(self.r().recs, self.len()) } }
    }
    pub fn stats(&self) -> Option<&[PmxStats]> {
        let p = self.r().stats;
        if p.is_null() { None } else { Some(unsafe { std::slice::from_raw_parts(p, self.len()) }) }
    }
}

impl Drop for PairHits {
    fn drop(&mut self) {
        if !self.inner.is_null() {
            unsafe { pmx_pair_hits_free(self.inner) }
        }
    }
}

unsafe impl Send for PairHits {}

/// Hits of a per-query top-K search, CSR by query row: the callee's block, released with `pmx_topk_hits_free` on drop.  Row `i`'s hits
/// are `row_off()[i] .. row_off()[i + 1]`, in (score descending, reference index ascending) order.
pub struct TopKHits {
    inner: *mut PmxTopkHits,
}

impl TopKHits {
    fn r(&self) -> &PmxTopkHits {
        unsafe { &*self.inner }
    }
    pub fn len(&self) -> usize {
        self.r().n_hits as usize
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    pub fn rows(&self) -> usize {
        self.r().n_rows as usize
    }
    /// References at or above `min_score`, summed over the rows, kept or not.
    pub fn passing(&self) -> i64 {
        self.r().n_passing
    }
    pub fn row_off(&self) -> &[i64] {
        unsafe { std::slice::from_raw_parts(self.r().row_off, self.rows() + 1) }
    }
    pub fn row_passing(&self) -> &[i64] {
        if self.rows() == 0 { &[] } else { unsafe { std::slice::from_raw_parts(self.r().row_passing, self.rows()) } }
    }
    /// The hits of local row `i` as a range into `pairs()` / `index()` / `records()` / `stats()`.
    pub fn row(&self, i: usize) -> std::ops::Range<usize> {
        let off = self.row_off();
        off[i] as usize..off[i + 1] as usize
    }
    /// The hits' descriptors: a valid pair list for `Aligner::align_pairs`.
    pub fn pairs(&self) -> &[PmxPair] {
        if self.is_empty() { &[] } else { unsafe { std::slice::from_raw_parts(self.r().pairs, self.len()) } }
    }
    /// `p = i * |R| + j` of every hit.
    pub fn index(&self) -> &[i64] {
        if self.is_empty() { &[] } else { unsafe { std::slice::from_raw_parts(self.r().index, self.len()) } }
    }
    pub fn records(&self) -> &[PmxRecord] {
        if self.is_empty() { &[] } else { unsafe { std::slice::from_raw_parts(self.r().recs, self.len()) } }
    }
    pub fn stats(&self) -> Option<&[PmxStats]> {
        let p = self.r().stats;
        if p.is_null() { None } else { Some(unsafe { std::slice::from_raw_parts(p, self.len()) }) }
    }
}

impl Drop for TopKHits {
    fn drop(&mut self) {
        if !self.inner.is_null() {
            unsafe { pmx_topk_hits_free(self.inner) }
        }
    }
}

unsafe impl Send for TopKHits {}

/// What a set search enumerates.
pub enum PairShape<'a> {
    /// These descriptors of `q x r`.
    List(&'a [PmxPair]),
    /// Pairs `[first, first + count)` of the strict upper triangle of `q` (`all_pairs_index`); `count` `None`: to the last pair.
    Triangle { first: i64, count: Option<i64> },
    /// Pairs `[first, first + count)` of `q x r`, row-major: pair `p` is `(p / r.len(), p % r.len())`.
    Rect { first: i64, count: Option<i64> },
}

/// Pairs of the rectangle `nq x nr`.
pub fn rect_pairs_count(nq: i64, nr: i64) -> Result<i64> {
    let v = unsafe { pmx_rect_pairs_count(nq, nr) };
    if v < 0 {
        return Err(last_error());
    }
    Ok(v)
}

fn last_error() -> Error {
    Error::Batch(unsafe { CStr::from_ptr(pmx_last_error()) }.to_string_lossy().into_owned())
}

/// A set of sequences resident on the device current at its creation (`pmx_seqset_t`), released on drop.
pub struct SeqSet {
    inner: *mut PmxSeqSet,
}

impl SeqSet {
    /// Uploads the packed sequences once.
    pub fn new(seqs: &Packed) -> Result<SeqSet> {
        let inner = unsafe { pmx_seqset_create(seqs.buf.as_ptr(), seqs.off.as_ptr(), seqs.len() as i64) };
        if inner.is_null() {
            return Err(last_error());
        }
        Ok(SeqSet { inner })
    }
    /// No copy: the caller's device buffers (`d_off`: `count + 1` entries).
    ///
    /// # Safety
    /// Both buffers are device memory of the current device and outlive the set.
    pub unsafe fn wrap_device(d_buf: *const u8, d_off: *const i64, count: i64, bytes: i64) -> Result<SeqSet> {
        let inner = pmx_seqset_wrap_device(d_buf, d_off, count, bytes);
        if inner.is_null() {
            return Err(last_error());
        }
        Ok(SeqSet { inner })
    }
    pub fn len(&self) -> usize {
        unsafe { pmx_seqset_count(self.inner) as usize }
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    /// For the `_device` entries.
    pub fn as_ptr(&self) -> *const PmxSeqSet {
        self.inner
    }
}

impl Drop for SeqSet {
    fn drop(&mut self) {
        unsafe { pmx_seqset_free(self.inner) }
    }
}

unsafe impl Send for SeqSet {}

/// Pairs of the strict upper triangle of `nseq x nseq`.
pub fn all_pairs_count(nseq: i64) -> Result<i64> {
    let v = unsafe { pmx_all_pairs_count(nseq) };
    if v < 0 {
        return Err(last_error());
    }
    Ok(v)
}

/// `(i, j)`, `i < j`, of pair `p` in the row-major order of `Aligner::align_all_pairs`.
pub fn all_pairs_index(nseq: i64, p: i64) -> Result<(i64, i64)> {
    let (mut i, mut j) = (0i64, 0i64);
    if unsafe { pmx_all_pairs_index(nseq, p, &mut i, &mut j) } != 0 {
        return Err(last_error());
    }
    Ok((i, j))
}

impl Aligner {
    fn pmx_config(&self, want: c_int) -> PmxConfig {
        PmxConfig {
            mode: self.mode_id,
            sg_flags: self.sg_flags,
            open: self.gap_open,
            extend: self.gap_extend,
            width: self.width,
            want,
            matrix: **self.matrix,
        }
    }

    /// Align many independent pairs in one call.  With a profile (`AlignerBuilder::profile`) pass `None` for the queries, as
    /// `align()` does (`src/aligner/mod.rs:394-396`): every reference is aligned against the profile's query.  A PSSM matrix
    /// (`Matrix::create_pssm` / `from_file` / `to_pssm`) is taken when the profile's query, or every query, has the PSSM's length;
    /// each record and its statistics equal `align()`'s with the same PSSM.
    pub fn align_batch(&self, queries: Option<&Packed>, references: &Packed) -> Result<BatchResult> {
        let n = references.len();
        let mut records = vec![PmxRecord::default(); n];
        let with_profile = !self.profile.is_null();
        let want_stats = if with_profile { self.profile.use_stats } else { self.want_stats };
        let mut stats = if want_stats { Some(vec![PmxStats::default(); n]) } else { None };
        let stats_ptr = stats.as_mut().map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let cfg = self.pmx_config(if want_stats { PMX_WANT_STATS } else { 0 });
        let rc = if with_profile {
            unsafe {
                pmx_align_profile_batch(&cfg, **self.profile, n as i64, references.buf.as_ptr(), references.off.as_ptr(),
                                        records.as_mut_ptr(), stats_ptr)
            }
        } else {
            let q = queries.expect("Query sequences are required for alignment without a profile.");
            assert_eq!(q.len(), n, "one query per reference");
            unsafe {
                pmx_align_batch(&cfg, n as i64, q.buf.as_ptr(), q.off.as_ptr(), references.buf.as_ptr(), references.off.as_ptr(),
                                records.as_mut_ptr(), stats_ptr)
            }
        };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(BatchResult { records, stats })
    }

    /// Score, end positions and CIGAR text per pair (an aligner built with `use_trace()`).  A PSSM: every query has its length.
    pub fn align_batch_cigar(&self, queries: &Packed, references: &Packed) -> Result<(Vec<PmxRecord>, BatchCigars)> {
        let n = references.len();
        assert_eq!(queries.len(), n, "one query per reference");
        let mut records = vec![PmxRecord::default(); n];
        let mut off = vec![0i64; n + 1];
        let mut text: *mut c_char = std::ptr::null_mut();
        let cfg = self.pmx_config(PMX_WANT_CIGAR);
        let rc = unsafe {
            pmx_align_batch_cigar(&cfg, n as i64, queries.buf.as_ptr(), queries.off.as_ptr(),
                                  references.buf.as_ptr(), references.off.as_ptr(),
                                  records.as_mut_ptr(), &mut text, off.as_mut_ptr())
        };
        if rc != 0 {
            return Err(last_error());
        }
        Ok((records, BatchCigars { text, off }))
    }

    /// Profile database search (extension, `pmx_search_profile`; an aligner built with `.profile()`): the references that score at
    /// least `opts.min_score` -- the best `opts.max_hits` of them, 0 = all -- each with its first-pass record and, with
    /// `opts.band >= 0`, the record, begin, CIGAR and (`want_stats`) statistics of a banded second pass around the first pass's
    /// diagonal.  Selection, compaction of the selected references and the second pass run on the device.
    pub fn search_profile(&self, references: &Packed, opts: PmxSearchOpts, want_stats: bool) -> Result<SearchHits> {
        if self.profile.is_null() {
            return Err(Error::Batch("aligner has no profile".to_string()));
        }
        let want = if opts.band >= 0 { PMX_WANT_CIGAR | if want_stats { PMX_WANT_STATS } else { 0 } } else { 0 };
        let cfg = self.pmx_config(want);
        let mut inner: *mut PmxSearchResult = std::ptr::null_mut();
        let rc = unsafe {
            pmx_search_profile(&cfg, **self.profile, references.len() as i64, references.buf.as_ptr(), references.off.as_ptr(),
                               &opts, &mut inner)
        };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(SearchHits { inner })
    }

    /// Banded batch: the extension of `banded_nw` (`src/aligner/mod.rs:454-489`) to many pairs, any mode, and an optional
    /// per-pair band centre (cells with `|(j - i) - diag[k]| > bandwidth` are excluded).
    pub fn banded_batch(&self, queries: Option<&Packed>, references: &Packed, diag: Option<&[i32]>) -> Result<Vec<PmxRecord>> {
        let band = self.bandwidth.ok_or(Error::NoBandwidth)?;
        let n = references.len();
        let mut records = vec![PmxRecord::default(); n];
        let cfg = self.pmx_config(0);
        let (qb, qo) = queries.map_or((std::ptr::null(), std::ptr::null()), |q| (q.buf.as_ptr(), q.off.as_ptr()));
        let prof = if self.profile.is_null() { std::ptr::null() } else { **self.profile as *const parasail_profile_t };
        let rc = unsafe {
            pmx_align_batch_banded(&cfg, prof, n as i64, qb, qo, references.buf.as_ptr(), references.off.as_ptr(),
                                   band, diag.map_or(std::ptr::null(), |d| d.as_ptr()), records.as_mut_ptr())
        };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(records)
    }

    /// Long pairs with traceback in linear memory (extension, `pmx_align_batch_cigar_long`): records, CIGAR text and, with
    /// `want_stats`, matches / similar / length along each path.  No buffer is proportional to `qlen x rlen`.
    pub fn cigar_long_batch(&self, queries: &Packed, references: &Packed, want_stats: bool, opts: Option<PmxLongCigarOpts>)
                            -> Result<(Vec<PmxRecord>, BatchCigars, Option<Vec<PmxStats>>)> {
        let n = references.len();
        let mut records = vec![PmxRecord::default(); n];
        let mut stats = if want_stats { Some(vec![PmxStats::default(); n]) } else { None };
        let stats_ptr = stats.as_mut().map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let mut off = vec![0i64; n + 1];
        let mut text: *mut c_char = std::ptr::null_mut();
        let cfg = self.pmx_config(PMX_WANT_CIGAR | if want_stats { PMX_WANT_STATS } else { 0 });
        let opts = opts.unwrap_or_default();
        let rc = unsafe {
            pmx_align_batch_cigar_long(&cfg, n as i64, queries.buf.as_ptr(), queries.off.as_ptr(),
                                       references.buf.as_ptr(), references.off.as_ptr(),
                                       records.as_mut_ptr(), stats_ptr, &mut text, off.as_mut_ptr(), &opts)
        };
        if rc != 0 {
            return Err(last_error());
        }
        Ok((records, BatchCigars { text, off }, stats))
    }

    /// Banded batch with traceback (extension): the records of `banded_batch`, the CIGAR text of each pair's path inside the band
    /// (empty where the band misses the end cell) and, with `want_stats`, matches / similar / length along that path.
    pub fn banded_cigar_batch(&self, queries: Option<&Packed>, references: &Packed, diag: Option<&[i32]>, want_stats: bool)
                              -> Result<(Vec<PmxRecord>, BatchCigars, Option<Vec<PmxStats>>)> {
        let band = self.bandwidth.ok_or(Error::NoBandwidth)?;
        let n = references.len();
        let mut records = vec![PmxRecord::default(); n];
        let mut stats = if want_stats { Some(vec![PmxStats::default(); n]) } else { None };
        let stats_ptr = stats.as_mut().map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let mut off = vec![0i64; n + 1];
        let mut text: *mut c_char = std::ptr::null_mut();
        let cfg = self.pmx_config(PMX_WANT_CIGAR | if want_stats { PMX_WANT_STATS } else { 0 });
        let (qb, qo) = queries.map_or((std::ptr::null(), std::ptr::null()), |q| (q.buf.as_ptr(), q.off.as_ptr()));
        let prof = if self.profile.is_null() { std::ptr::null() } else { **self.profile as *const parasail_profile_t };
        let rc = unsafe {
            pmx_align_batch_banded_cigar(&cfg, prof, n as i64, qb, qo, references.buf.as_ptr(), references.off.as_ptr(),
                                         band, diag.map_or(std::ptr::null(), |d| d.as_ptr()), records.as_mut_ptr(), stats_ptr,
                                         &mut text, off.as_mut_ptr())
        };
        if rc != 0 {
            return Err(last_error());
        }
        Ok((records, BatchCigars { text, off }, stats))
    }

    /// One process driving several GPUs of the node: contiguous blocks of about equal cell counts, one per listed device;
    /// records come back in input order.  A PSSM: the length rule of `align_batch`.
    pub fn align_batch_multi(&self, queries: Option<&Packed>, references: &Packed, devices: &[i32]) -> Result<BatchResult> {
        let n = references.len();
        let mut records = vec![PmxRecord::default(); n];
        let with_profile = !self.profile.is_null();
        let want_stats = if with_profile { self.profile.use_stats } else { self.want_stats };
        let mut stats = if want_stats { Some(vec![PmxStats::default(); n]) } else { None };
        let stats_ptr = stats.as_mut().map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let cfg = self.pmx_config(if want_stats { PMX_WANT_STATS } else { 0 });
        let rc = if with_profile {
            unsafe {
                pmx_align_profile_batch_multi(&cfg, **self.profile, n as i64, references.buf.as_ptr(), references.off.as_ptr(),
                                              devices.as_ptr(), devices.len() as c_int, records.as_mut_ptr(), stats_ptr)
            }
        } else {
            let q = queries.expect("Query sequences are required for alignment without a profile.");
            unsafe {
                pmx_align_batch_multi(&cfg, n as i64, q.buf.as_ptr(), q.off.as_ptr(), references.buf.as_ptr(), references.off.as_ptr(),
                                      devices.as_ptr(), devices.len() as c_int, records.as_mut_ptr(), stats_ptr)
            }
        };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(BatchResult { records, stats })
    }

    /// Pairs by index and window into device-resident sets (`q` may be `r`): record k belongs to the pair (query window, reference
    /// window) k, end positions relative to the windows.  A bad descriptor is an error that names the first.
    pub fn align_pairs(&self, q: &SeqSet, r: &SeqSet, pairs: &[PmxPair], chunk_pairs: i64) -> Result<BatchResult> {
        assert!(self.profile.is_null(), "align_pairs takes no profile");
        let n = pairs.len();
        let mut records = vec![PmxRecord::default(); n];
        let mut stats = if self.want_stats { Some(vec![PmxStats::default(); n]) } else { None };
        let stats_ptr = stats.as_mut().map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let cfg = self.pmx_config(if self.want_stats { PMX_WANT_STATS } else { 0 });
        let opts = PmxPairsOpts { chunk_pairs };
        let rc = unsafe { pmx_align_pairs(&cfg, q.inner, r.inner, n as i64, pairs.as_ptr(), records.as_mut_ptr(), stats_ptr, &opts) };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(BatchResult { records, stats })
    }

    /// Pairs `[first, first + count)` of the strict upper triangle of `s x s` (row-major, `all_pairs_index`), whole sequences,
    /// enumerated on the device.  `count` `None`: to the last pair.
    pub fn align_all_pairs(&self, s: &SeqSet, first: i64, count: Option<i64>, chunk_pairs: i64) -> Result<BatchResult> {
        assert!(self.profile.is_null(), "align_all_pairs takes no profile");
        let count = match count {
            Some(c) => c,
            None => all_pairs_count(s.len() as i64)? - first,
        };
        let n = count.max(0) as usize;
        let mut records = vec![PmxRecord::default(); n];
        let mut stats = if self.want_stats { Some(vec![PmxStats::default(); n]) } else { None };
        let stats_ptr = stats.as_mut().map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let cfg = self.pmx_config(if self.want_stats { PMX_WANT_STATS } else { 0 });
        let opts = PmxPairsOpts { chunk_pairs };
        let rc = unsafe { pmx_align_all_pairs(&cfg, s.inner, first, count, records.as_mut_ptr(), stats_ptr, &opts) };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(BatchResult { records, stats })
    }

    /// Set search: the pairs of the enumeration that score at least `min_score`, in enumeration order, with their descriptors,
    /// numbers, records and (stats aligner) statistics.  Only the hits leave the device.  `r` `None`: `q` (lists, rectangles) --
    /// a triangle takes one set.  `max_hits > 0` keeps the first `max_hits` hits and goes on counting `passing()`.
    pub fn search_pairs(&self, q: &SeqSet, r: Option<&SeqSet>, shape: PairShape, min_score: i32, max_hits: i64, chunk_pairs: i64,
                        slice_pairs: i64) -> Result<PairHits> {
        assert!(self.profile.is_null(), "search_pairs takes no profile");
        let rset = r.unwrap_or(q);
        let (code, first, count, list, rptr) = match shape {
            PairShape::List(p) => (PMX_PAIRS_LIST, 0, p.len() as i64, if p.is_empty() { std::ptr::null() } else { p.as_ptr() }, rset.inner as *const PmxSeqSet),
            PairShape::Triangle { first, count } => {
                let c = match count { Some(c) => c, None => all_pairs_count(q.len() as i64)? - first };
                (PMX_PAIRS_TRIANGLE, first, c, std::ptr::null(), std::ptr::null())
            }
            PairShape::Rect { first, count } => {
                let c = match count { Some(c) => c, None => rect_pairs_count(q.len() as i64, rset.len() as i64)? - first };
                (PMX_PAIRS_RECT, first, c, std::ptr::null(), rset.inner as *const PmxSeqSet)
            }
        };
        let cfg = self.pmx_config(if self.want_stats { PMX_WANT_STATS } else { 0 });
        let opts = PmxPairSearchOpts { min_score, shape: code, max_hits, chunk_pairs, slice_pairs };
        let mut inner: *mut PmxPairHits = std::ptr::null_mut();
        let rc = unsafe { pmx_search_pairs(&cfg, q.inner, rptr, first, count, list, &opts, &mut inner) };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(PairHits { inner })
    }

    /// Per-query top-K: for every query row `first_row .. first_row + rows` of `q` (`rows` `None`: to the last) the best `k`
    /// references of `r` (`None`: `q`) with score at least `min_score` (`i32::MIN`: pure top-K), in (score descending, reference
    /// index ascending) order.  `skip_self` (`r` is `q`) leaves the pair (i, i) out.  Only the hits leave the device.
    pub fn search_topk(&self, q: &SeqSet, r: Option<&SeqSet>, k: i32, min_score: i32, skip_self: bool, first_row: i64, rows: Option<i64>,
                       chunk_pairs: i64, slice_rows: i64) -> Result<TopKHits> {
        assert!(self.profile.is_null(), "search_topk takes no profile");
        let nq = rows.unwrap_or(q.len() as i64 - first_row);
        let rptr = r.map_or(std::ptr::null(), |s| s.inner as *const PmxSeqSet);
        let cfg = self.pmx_config(if self.want_stats { PMX_WANT_STATS } else { 0 });
        let opts = PmxTopkOpts { min_score, k, skip_self: skip_self as i32, chunk_pairs, slice_rows };
        let mut inner: *mut PmxTopkHits = std::ptr::null_mut();
        let rc = unsafe { pmx_search_topk(&cfg, q.inner, rptr, first_row, nq, &opts, &mut inner) };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(TopKHits { inner })
    }

    /// 2-bit packed DNA (base b in byte b / 4 at bits 2 * (b % 4); code c = letter c of the matrix alphabet; offsets count
    /// bases): a quarter of the bytes cross PCIe.
    pub fn align_batch_2bit(&self, q2: &[u8], qoff: &[i64], r2: &[u8], roff: &[i64]) -> Result<Vec<PmxRecord>> {
        let n = roff.len() - 1;
        assert_eq!(qoff.len(), roff.len());
        let mut records = vec![PmxRecord::default(); n];
        let cfg = self.pmx_config(0);
        let rc = unsafe {
            pmx_align_batch_2bit(&cfg, n as i64, q2.as_ptr(), qoff.as_ptr(), r2.as_ptr(), roff.as_ptr(),
                                 records.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            return Err(last_error());
        }
        Ok(records)
    }
}

#[cfg(test)]
mod tests {
    //! The reference's KAT style (`tests/test_parasail.rs:65-122`), on batches.
    use super::*;
    use crate::Matrix;

    #[test]
    fn batch_of_identical_pairs() -> crate::Result<()> {
        let q: Vec<&[u8]> = vec![b"ACGT"; 1000];
        let (qs, rs) = (Packed::from_slices(&q), Packed::from_slices(&q));
        let aligner = Aligner::new().local().build();
        let out = aligner.align_batch(Some(&qs), &rs)?;
        assert!(out.records.iter().all(|r| (r.score, r.end_query, r.end_ref) == (4, 3, 3)));
        Ok(())
    }

    #[test]
    fn batch_cigar() -> crate::Result<()> {
        let matrix = Matrix::create(b"ACGT", 2, -3)?;
        let q: Vec<&[u8]> = vec![b"ACGTACGTAC"; 64];
        let r: Vec<&[u8]> = vec![b"ACGTACGTAC"; 64];
        let aligner = Aligner::new().global().matrix(matrix).gap_open(5).gap_extend(2).use_trace().build();
        let (rec, cig) = aligner.align_batch_cigar(&Packed::from_slices(&q), &Packed::from_slices(&r))?;
        assert_eq!(rec[0].score, 20);
        assert_eq!(cig.get(0), "10=");
        Ok(())
    }
}
