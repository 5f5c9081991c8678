"""parasail_rs_amd -- host-side mirror of the parasail-rs interface over libparasail_amd.so.

Rust is not available in the build image, so the reference's L2/L3 layer
(`Aligner` / `AlignerBuilder` / `Matrix` / `Profile` / `Alignment`,
/root/reference/src/{aligner,matrix,profile,alignment}/mod.rs) is mirrored here
with the same names, argument meaning, defaults, quirks and error behaviour, on
top of the C ABI in include/parasail_amd.h (ctypes; nothing here computes).
`global()` is spelled `global_()` because `global` is a Python keyword; Rust
panics become `PanicError`; `Err(...)` values become the exception classes below.

The DP always runs in the HIP kernels.  There is no CPU fallback: if the shared
library is missing, importing this package raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libparasail_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "parasail_amd.h")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libparasail_amd.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C parasail-rs_amd`. There is no CPU fallback." % LIB_PATH)
lib = C.CDLL(LIB_PATH)


# ------------------------------------------------------------------ C types ----
class parasail_matrix_t(C.Structure):
    _fields_ = [("name", C.c_char_p), ("matrix", C.POINTER(C.c_int)), ("mapper", C.POINTER(C.c_int)),
                ("size", C.c_int), ("max", C.c_int), ("min", C.c_int),
                ("user_matrix", C.POINTER(C.c_int)), ("type_", C.c_int), ("length", C.c_int),
                ("alphabet", C.c_char_p), ("query", C.c_char_p)]


class parasail_traceback_t(C.Structure):
    _fields_ = [("query", C.c_void_p), ("comp", C.c_void_p), ("ref_", C.c_void_p)]


class parasail_cigar_t(C.Structure):
    _fields_ = [("seq", C.POINTER(C.c_uint32)), ("len", C.c_int), ("beg_query", C.c_int), ("beg_ref", C.c_int)]


class parasail_result_ssw_t(C.Structure):
    _fields_ = [("score1", C.c_uint16), ("ref_begin1", C.c_int32), ("ref_end1", C.c_int32),
                ("read_begin1", C.c_int32), ("read_end1", C.c_int32),
                ("cigar", C.POINTER(C.c_uint32)), ("cigarLen", C.c_int32)]


class pmx_config_t(C.Structure):
    _fields_ = [("mode", C.c_int), ("sg_flags", C.c_int), ("open", C.c_int), ("extend", C.c_int),
                ("width", C.c_int), ("want", C.c_int), ("matrix", C.POINTER(parasail_matrix_t))]


class pmx_long_cigar_opts_t(C.Structure):
    _fields_ = [("tile_cols", C.c_int), ("band_rows", C.c_int)]


class pmx_record_t(C.Structure):
    _fields_ = [("score", C.c_int32), ("end_query", C.c_int32), ("end_ref", C.c_int32), ("flags", C.c_int32)]


class pmx_search_opts_t(C.Structure):
    _fields_ = [("min_score", C.c_int32), ("max_hits", C.c_int64), ("order", C.c_int32), ("band", C.c_int32)]


class pmx_hit_t(C.Structure):
    _fields_ = [("index", C.c_int64), ("first", pmx_record_t), ("diag", C.c_int32), ("beg_query", C.c_int32),
                ("beg_ref", C.c_int32), ("reserved", C.c_int32)]


class pmx_search_result_t(C.Structure):
    _fields_ = [("n_hits", C.c_int64), ("n_passing", C.c_int64), ("hits", C.c_void_p), ("recs", C.c_void_p),
                ("stats", C.c_void_p), ("cigar", C.c_void_p), ("cigar_off", C.c_void_p)]


class pmx_pair_t(C.Structure):
    _fields_ = [("q", C.c_int64), ("r", C.c_int64), ("q_beg", C.c_int32), ("q_len", C.c_int32),
                ("r_beg", C.c_int32), ("r_len", C.c_int32)]


class pmx_pairs_opts_t(C.Structure):
    _fields_ = [("chunk_pairs", C.c_int64)]


class pmx_pair_search_opts_t(C.Structure):
    _fields_ = [("min_score", C.c_int32), ("shape", C.c_int32), ("max_hits", C.c_int64), ("chunk_pairs", C.c_int64),
                ("slice_pairs", C.c_int64)]


class pmx_pair_hits_t(C.Structure):
    _fields_ = [("n_hits", C.c_int64), ("n_passing", C.c_int64), ("pairs", C.c_void_p), ("index", C.c_void_p),
                ("recs", C.c_void_p), ("stats", C.c_void_p)]


class pmx_topk_opts_t(C.Structure):
    _fields_ = [("min_score", C.c_int32), ("k", C.c_int32), ("skip_self", C.c_int32), ("chunk_pairs", C.c_int64),
                ("slice_rows", C.c_int64)]


class pmx_topk_hits_t(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("n_hits", C.c_int64), ("n_passing", C.c_int64), ("row_off", C.c_void_p),
                ("row_passing", C.c_void_p), ("pairs", C.c_void_p), ("index", C.c_void_p), ("recs", C.c_void_p),
                ("stats", C.c_void_p)]


class pmx_strand_hits_t(C.Structure):
    _fields_ = pmx_pair_hits_t._fields_ + [("strand", C.c_void_p)]


class pmx_topk_strand_hits_t(C.Structure):
    _fields_ = pmx_topk_hits_t._fields_ + [("strand", C.c_void_p)]


class pmx_frame_hits_t(C.Structure):
    _fields_ = pmx_pair_hits_t._fields_ + [("frame", C.c_void_p)]


class pmx_topk_frame_hits_t(C.Structure):
    _fields_ = pmx_topk_hits_t._fields_ + [("frame", C.c_void_p)]


class pmx_seed_hit_t(C.Structure):
    _fields_ = [("n_seeds", C.c_int32), ("diag_min", C.c_int32), ("diag_max", C.c_int32), ("reserved", C.c_int32)]


class pmx_seed_opts_t(C.Structure):
    _fields_ = [("strand", C.c_int32), ("min_seeds", C.c_int32), ("band", C.c_int32), ("pad", C.c_int32), ("max_occ", C.c_int32),
                ("reserved", C.c_int32), ("max_hits", C.c_int64), ("slice_rows", C.c_int64)]


class pmx_seed_hits_t(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("n_hits", C.c_int64), ("n_passing", C.c_int64), ("row_off", C.c_void_p),
                ("pairs", C.c_void_p), ("strand", C.c_void_p), ("seeds", C.c_void_p)]


class pmx_ungapped_t(C.Structure):
    _fields_ = [("score", C.c_int32), ("diag", C.c_int32), ("end_query", C.c_int32), ("end_ref", C.c_int32)]


class pmx_seed_filter_opts_t(C.Structure):
    _fields_ = [("min_score", C.c_int32), ("top_n", C.c_int32), ("reserved", C.c_int32 * 2)]


class pmx_seed_filtered_t(C.Structure):
    _fields_ = [("hits", pmx_seed_hits_t), ("ungapped", C.c_void_p), ("source", C.c_void_p)]


class pmx_seed_chain_opts_t(C.Structure):
    _fields_ = [("max_gap", C.c_int32), ("lookback", C.c_int32), ("gap_scale", C.c_int32), ("min_score", C.c_int32), ("reserved", C.c_int32 * 4)]


class pmx_seed_chain_t(C.Structure):
    _fields_ = [("score", C.c_int32), ("n_anchors", C.c_int32), ("q_beg", C.c_int32), ("q_end", C.c_int32), ("r_beg", C.c_int32),
                ("r_end", C.c_int32), ("diag_min", C.c_int32), ("diag_max", C.c_int32)]


class pmx_seed_chained_t(C.Structure):
    _fields_ = [("hits", pmx_seed_hits_t), ("chains", C.c_void_p)]


SEED_HIT_DTYPE = np.dtype([("n_seeds", "<i4"), ("diag_min", "<i4"), ("diag_max", "<i4"), ("reserved", "<i4")])
SEED_CHAIN_DTYPE = np.dtype([("score", "<i4"), ("n_anchors", "<i4"), ("q_beg", "<i4"), ("q_end", "<i4"), ("r_beg", "<i4"), ("r_end", "<i4"),
                             ("diag_min", "<i4"), ("diag_max", "<i4")])
UNGAPPED_DTYPE = np.dtype([("score", "<i4"), ("diag", "<i4"), ("end_query", "<i4"), ("end_ref", "<i4")])
SEED_BYTE_STRAND, SEED_BYTE_FRAME = 0, 1
SEED_LIST_CODONS, SEED_LIST_REF_FRAMES, SEED_LIST_REF_CODONS = 1, 2, 3
TOPK_MAX = 1024
INT32_MIN = -(1 << 31)
RECORD_DTYPE = np.dtype([("score", "<i4"), ("end_query", "<i4"), ("end_ref", "<i4"), ("flags", "<i4")])
STATS_DTYPE = np.dtype([("matches", "<i4"), ("similar", "<i4"), ("length", "<i4")])
HIT_DTYPE = np.dtype([("index", "<i8"), ("first", RECORD_DTYPE), ("diag", "<i4"), ("beg_query", "<i4"), ("beg_ref", "<i4"),
                      ("reserved", "<i4")])
HITS_BY_INDEX, HITS_BY_SCORE = 0, 1
PAIR_DTYPE = np.dtype([("q", "<i8"), ("r", "<i8"), ("q_beg", "<i4"), ("q_len", "<i4"), ("r_beg", "<i4"), ("r_len", "<i4")])
PAIRS_LIST, PAIRS_TRIANGLE, PAIRS_RECT = 0, 1, 2
STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = 0, 1, 2
FRAMES_FORWARD, FRAMES_REVERSE, FRAMES_ALL = 6, 7, 8          # frame modes beside the single frames 0 .. 5

MODE_NW, MODE_SG, MODE_SW = 0, 1, 2
SG_QB, SG_QE, SG_DB, SG_DE, SG_ALL = 1, 2, 4, 8, 15
WANT_STATS, WANT_CIGAR, WANT_SORTED = 1, 2, 4
FLAG_SATURATED = 1
FLAG_BAD_PAIR = 8

_MP = C.POINTER(parasail_matrix_t)
_FN = C.CFUNCTYPE(C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, _MP)
_PFN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int)


def _sig(name, res, *args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


_sig("parasail_lookup_function", C.c_void_p, C.c_char_p)
_sig("parasail_lookup_pfunction", C.c_void_p, C.c_char_p)
_sig("parasail_nw_banded", C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, _MP)
_sig("parasail_ssw", C.POINTER(parasail_result_ssw_t), C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, _MP)
_sig("parasail_ssw_init", C.c_void_p, C.c_char_p, C.c_int, _MP, C.c_int8)
_sig("parasail_result_ssw_free", None, C.POINTER(parasail_result_ssw_t))
for _n in ("score", "end_query", "end_ref", "matches", "similar", "length"):
    _sig("parasail_result_get_" + _n, C.c_int, C.c_void_p)
for _k in ("score", "matches", "similar", "length"):
    for _w in ("table", "row", "col"):
        _sig("parasail_result_get_%s_%s" % (_k, _w), C.POINTER(C.c_int), C.c_void_p)
_sig("parasail_result_get_trace_table", C.POINTER(C.c_int), C.c_void_p)
for _n in ("nw", "sg", "sw", "saturated", "banded", "scan", "striped", "diag", "blocked", "stats",
           "stats_table", "table", "rowcol", "stats_rowcol", "trace"):
    _sig("parasail_result_is_" + _n, C.c_int, C.c_void_p)
_sig("parasail_result_free", None, C.c_void_p)
_sig("parasail_result_get_traceback", C.POINTER(parasail_traceback_t), C.c_void_p, C.c_char_p, C.c_int,
     C.c_char_p, C.c_int, _MP, C.c_char, C.c_char, C.c_char)
_sig("parasail_traceback_free", None, C.POINTER(parasail_traceback_t))
_sig("parasail_traceback_generic", None, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, _MP,
     C.c_void_p, C.c_char, C.c_char, C.c_char, C.c_int, C.c_int, C.c_int)
_sig("parasail_result_get_cigar", C.POINTER(parasail_cigar_t), C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int, _MP)
_sig("parasail_cigar_decode", C.c_void_p, C.POINTER(parasail_cigar_t))
_sig("parasail_cigar_free", None, C.POINTER(parasail_cigar_t))
_sig("parasail_matrix_create", _MP, C.c_char_p, C.c_int, C.c_int)
_sig("parasail_matrix_lookup", _MP, C.c_char_p)
_sig("parasail_matrix_from_file", _MP, C.c_char_p)
_sig("parasail_matrix_pssm_create", _MP, C.c_char_p, C.POINTER(C.c_int), C.c_int)
_sig("parasail_matrix_convert_square_to_pssm", _MP, _MP, C.c_char_p, C.c_int)
_sig("parasail_matrix_copy", _MP, _MP)
_sig("parasail_matrix_set_value", None, _MP, C.c_int, C.c_int, C.c_int)
_sig("parasail_matrix_free", None, _MP)
_sig("parasail_profile_free", None, C.c_void_p)
_sig("pmx_free", None, C.c_void_p)
_sig("pmx_last_error", C.c_char_p)
_sig("pmx_version", C.c_char_p)
_sig("pmx_device_count", C.c_int)
_sig("pmx_set_device", C.c_int, C.c_int)
_sig("pmx_kernel_for", C.c_char_p, C.POINTER(pmx_config_t), C.c_int32, C.c_int32)
_sig("pmx_last_kernel", C.c_char_p)
_sig("pmx_switches", C.c_char_p)
_sig("pmx_align_batch", C.c_int, C.POINTER(pmx_config_t), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_align_batch_device", C.c_int, C.POINTER(pmx_config_t), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_align_profile_batch", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p)
_sig("pmx_align_profile_batch_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_align_batch_cigar", C.c_int, C.POINTER(pmx_config_t), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p)
_sig("pmx_align_batch_cigar_device", C.c_int, C.POINTER(pmx_config_t), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)
_sig("pmx_align_batch_banded", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)
_sig("pmx_align_batch_banded_device", C.c_int, C.POINTER(pmx_config_t), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_align_profile_batch_banded_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_align_batch_banded_cigar", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p)
_sig("pmx_align_batch_banded_cigar_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_void_p)
_sig("pmx_align_batch_cigar_long", C.c_int, C.POINTER(pmx_config_t), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(pmx_long_cigar_opts_t))
_sig("pmx_align_batch_cigar_long_device", C.c_int, C.POINTER(pmx_config_t), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_long_cigar_opts_t))
_sig("pmx_long_cigar_scratch_bytes", C.c_longlong, C.c_int64, C.c_int32, C.c_int32, C.POINTER(pmx_long_cigar_opts_t))
_sig("pmx_align_batch_multi", C.c_int, C.POINTER(pmx_config_t), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
_sig("pmx_align_profile_batch_multi", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
_sig("pmx_shard_bounds_by_cells", C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
_sig("pmx_align_batch_table_device", C.c_int, C.POINTER(pmx_config_t), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_host_register", C.c_int, C.c_void_p, C.c_size_t)
_sig("pmx_host_unregister", C.c_int, C.c_void_p)
_sig("pmx_align_batch_2bit", C.c_int, C.POINTER(pmx_config_t), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_select_hits_device", C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
     C.c_void_p)
_sig("pmx_gather_refs_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
     C.c_void_p)
_sig("pmx_search_profile", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_search_opts_t), C.POINTER(C.POINTER(pmx_search_result_t)))
_sig("pmx_search_result_free", None, C.POINTER(pmx_search_result_t))
_sig("pmx_search_profile_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
     C.POINTER(pmx_search_opts_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
     C.c_void_p, C.c_void_p)
_sig("pmx_seqset_create", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)
_sig("pmx_seqset_wrap_device", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)
_sig("pmx_seqset_free", None, C.c_void_p)
_sig("pmx_seqset_count", C.c_int64, C.c_void_p)
_sig("pmx_align_pairs", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_complement_table", None, C.c_void_p)
_sig("pmx_align_pairs_ex", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_ex_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_gather_pairs_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_all_pairs_count", C.c_int64, C.c_int64)
_sig("pmx_all_pairs_index", C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64))
_sig("pmx_align_all_pairs", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_all_pairs_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
     C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_all_pairs_enumerate_device", C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p)
_sig("pmx_rect_pairs_count", C.c_int64, C.c_int64, C.c_int64)
_sig("pmx_rect_pairs_enumerate_device", C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p)
_sig("pmx_search_pairs_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_pairs_opts_t))
_sig("pmx_search_pairs", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
     C.POINTER(pmx_pair_search_opts_t), C.POINTER(C.POINTER(pmx_pair_hits_t)))
_sig("pmx_pair_hits_free", None, C.POINTER(pmx_pair_hits_t))
_sig("pmx_search_topk_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_search_topk", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
     C.POINTER(pmx_topk_opts_t), C.POINTER(C.POINTER(pmx_topk_hits_t)))
_sig("pmx_topk_hits_free", None, C.POINTER(pmx_topk_hits_t))
_sig("pmx_seed_index_build", C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)
_sig("pmx_seed_index_free", None, C.c_void_p)
_sig("pmx_seed_index_count", C.c_int64, C.c_void_p)
_sig("pmx_seed_index_entries_device", C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_seed_pairs_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(pmx_seed_opts_t),
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_seed_pairs", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(pmx_seed_opts_t),
     C.POINTER(C.POINTER(pmx_seed_hits_t)))
_sig("pmx_seed_hits_free", None, C.POINTER(pmx_seed_hits_t))
_sig("pmx_seed_match_budget", C.c_int64, C.c_int64)
_sig("pmx_seed_chains_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(pmx_seed_opts_t),
     C.POINTER(pmx_seed_chain_opts_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_seed_chains", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(pmx_seed_opts_t), C.POINTER(pmx_seed_chain_opts_t),
     C.POINTER(C.POINTER(pmx_seed_chained_t)))
_sig("pmx_seed_chained_free", None, C.POINTER(pmx_seed_chained_t))
_sig("pmx_seed_chain_shape", None, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
_sig("pmx_seed_mix", C.c_uint64, C.c_uint64, C.c_int32)
_sig("pmx_seed_index_build_minimizers", C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p)
_sig("pmx_seed_index_window", C.c_int32, C.c_void_p)
_sig("pmx_seed_index_bytes", C.c_int64, C.c_void_p)
_sig("pmx_seed_sketch_device", C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p)
_sig("pmx_seed_sketch", C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p)
_sig("pmx_seed_rows_max_len", C.c_int64, C.c_void_p, C.c_int64, C.c_int64)
_sig("pmx_seed_sketch_shape", None, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
_sig("pmx_seed_alphabet", C.c_int, C.c_int, C.c_void_p)
_sig("pmx_seed_index_build_letters", C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)
_sig("pmx_seed_index_bits", C.c_int32, C.c_void_p)
_sig("pmx_seed_pairs_letters_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(pmx_seed_opts_t), C.c_int,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_seed_pairs_letters", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(pmx_seed_opts_t), C.c_int, C.c_void_p,
     C.POINTER(C.POINTER(pmx_seed_hits_t)))
_sig("pmx_seed_index_build_translated", C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
_sig("pmx_seed_index_strands", C.c_int32, C.c_void_p)
_sig("pmx_seed_pairs_translated_ref_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(pmx_seed_opts_t), C.c_int,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_seed_pairs_translated_ref", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(pmx_seed_opts_t), C.c_int,
     C.POINTER(C.POINTER(pmx_seed_hits_t)))
_sig("pmx_seed_ungapped_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
     C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_seed_ungapped", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
     C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_seed_filter_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
     C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(pmx_seed_filter_opts_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_seed_filter", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.POINTER(pmx_seed_hits_t), C.c_int, C.c_void_p,
     C.POINTER(pmx_seed_filter_opts_t), C.POINTER(pmx_pairs_opts_t), C.POINTER(C.POINTER(pmx_seed_filtered_t)))
_sig("pmx_seed_ungapped_translated_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
     C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_seed_ungapped_translated", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
     C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_seed_filter_translated_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
     C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(pmx_seed_filter_opts_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_seed_filter_translated", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.POINTER(pmx_seed_hits_t), C.c_int, C.c_void_p,
     C.POINTER(pmx_seed_filter_opts_t), C.POINTER(pmx_pairs_opts_t), C.POINTER(C.POINTER(pmx_seed_filtered_t)))
_sig("pmx_seed_filtered_free", None, C.POINTER(pmx_seed_filtered_t))
_sig("pmx_seed_ungapped_shape", None, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
_sig("pmx_topk_records_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_align_pairs_both", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_both_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_search_pairs_stranded_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_pairs_opts_t), C.c_int, C.c_void_p)
_sig("pmx_search_pairs_stranded", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
     C.POINTER(pmx_pair_search_opts_t), C.c_int, C.POINTER(C.POINTER(pmx_strand_hits_t)))
_sig("pmx_strand_hits_free", None, C.POINTER(pmx_strand_hits_t))
_sig("pmx_search_topk_stranded_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.POINTER(pmx_pairs_opts_t), C.c_int, C.c_void_p)
_sig("pmx_search_topk_stranded", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
     C.POINTER(pmx_topk_opts_t), C.c_int, C.POINTER(C.POINTER(pmx_topk_strand_hits_t)))
_sig("pmx_topk_strand_hits_free", None, C.POINTER(pmx_topk_strand_hits_t))
_sig("pmx_genetic_code_table", None, C.c_void_p)
_sig("pmx_gather_pairs_translated_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_align_pairs_translated_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_translated", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_search_pairs_translated_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_pairs_opts_t), C.c_int, C.c_void_p, C.c_void_p)
_sig("pmx_search_pairs_translated", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
     C.POINTER(pmx_pair_search_opts_t), C.c_int, C.c_void_p, C.POINTER(C.POINTER(pmx_frame_hits_t)))
_sig("pmx_frame_hits_free", None, C.POINTER(pmx_frame_hits_t))
_sig("pmx_search_topk_translated_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.POINTER(pmx_pairs_opts_t), C.c_int, C.c_void_p, C.c_void_p)
_sig("pmx_search_topk_translated", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
     C.POINTER(pmx_topk_opts_t), C.c_int, C.c_void_p, C.POINTER(C.POINTER(pmx_topk_frame_hits_t)))
_sig("pmx_topk_frame_hits_free", None, C.POINTER(pmx_topk_frame_hits_t))
_sig("pmx_gather_pairs_translated_ref_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_align_pairs_translated_ref_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_translated_ref", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_search_pairs_translated_ref_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_pairs_opts_t), C.c_int, C.c_void_p, C.c_void_p)
_sig("pmx_search_pairs_translated_ref", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
     C.POINTER(pmx_pair_search_opts_t), C.c_int, C.c_void_p, C.POINTER(C.POINTER(pmx_frame_hits_t)))
_sig("pmx_search_topk_translated_ref_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.POINTER(pmx_pairs_opts_t), C.c_int, C.c_void_p, C.c_void_p)
_sig("pmx_search_topk_translated_ref", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
     C.POINTER(pmx_topk_opts_t), C.c_int, C.c_void_p, C.POINTER(C.POINTER(pmx_topk_frame_hits_t)))
_sig("pmx_frameshift_max_window", C.c_int32)
_sig("pmx_gather_pairs_codons_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_align_pairs_frameshift_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_frameshift", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_frameshift_cigar_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_frameshift_cigar", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_search_pairs_frameshift_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_pairs_opts_t), C.c_int, C.c_void_p, C.c_int32, C.c_void_p)
_sig("pmx_search_pairs_frameshift", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
     C.POINTER(pmx_pair_search_opts_t), C.c_int, C.c_int32, C.c_void_p, C.POINTER(C.POINTER(pmx_strand_hits_t)))
_sig("pmx_search_topk_frameshift_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.POINTER(pmx_pairs_opts_t), C.c_int, C.c_void_p, C.c_int32, C.c_void_p)
_sig("pmx_search_topk_frameshift", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
     C.POINTER(pmx_topk_opts_t), C.c_int, C.c_int32, C.c_void_p, C.POINTER(C.POINTER(pmx_topk_strand_hits_t)))
_sig("pmx_frameshift_ref_max_query", C.c_int32)
_sig("pmx_swfsc_strip_rows", C.c_int)
_sig("pmx_swfsc_lane_rows", C.c_int)
_sig("pmx_swfsc_bound_bytes_per_slot", C.c_longlong, C.c_int)
_sig("pmx_swfsc_max_msize", C.c_int)
_sig("pmx_gather_pairs_codons_ref_device", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("pmx_align_pairs_frameshift_ref_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_frameshift_ref", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_search_pairs_frameshift_ref_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_pairs_opts_t), C.c_int, C.c_void_p, C.c_int32, C.c_void_p)
_sig("pmx_search_pairs_frameshift_ref", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
     C.POINTER(pmx_pair_search_opts_t), C.c_int, C.c_int32, C.c_void_p, C.POINTER(C.POINTER(pmx_strand_hits_t)))
_sig("pmx_search_topk_frameshift_ref_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.POINTER(pmx_pairs_opts_t), C.c_int, C.c_void_p, C.c_int32, C.c_void_p)
_sig("pmx_search_topk_frameshift_ref", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
     C.POINTER(pmx_topk_opts_t), C.c_int, C.c_int32, C.c_void_p, C.POINTER(C.POINTER(pmx_topk_strand_hits_t)))
_sig("pmx_swfsc_trace_bytes_per_slot", C.c_longlong, C.c_int, C.c_int)
_sig("pmx_align_pairs_frameshift_ref_cigar_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_frameshift_ref_cigar", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_frameshift_ref_cigar_long_device", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
     C.c_int, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
     C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_align_pairs_frameshift_ref_cigar_long", C.c_int, C.POINTER(pmx_config_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pmx_pairs_opts_t))
_sig("pmx_frameshift_ref_cigar_long_parts", C.c_int64)
_sig("pmx_swfsc_window_cols", C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong)
_sig("pmx_trace_plan_probe", C.c_int, *([C.c_int] * 7 + [C.c_longlong] + [C.c_int] * 5 + [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_longlong)]))
_sig("pmx_long_plan_probe", C.c_int, *([C.c_int] * 2 + [C.c_longlong] + [C.c_int] * 2 + [C.c_double] + [C.c_int] * 7 + [C.POINTER(C.c_longlong)]))
_sig("pmx_seed_plan_probe", C.c_int, *([C.c_int] * 2 + [C.c_longlong] + [C.c_int] * 2 + [C.c_longlong] * 3 + [C.POINTER(C.c_longlong)]))
_sig("pmx_seed_plan_probe_w", C.c_int, *([C.c_int] * 2 + [C.c_longlong] + [C.c_int] * 2 + [C.c_longlong] * 3 + [C.c_int, C.POINTER(C.c_longlong)]))
_libc_free = C.CDLL(None).free
_libc_free.argtypes = [C.c_void_p]


# ------------------------------------------------------------------ errors ----
class Error(Exception):
    """src/error.rs:8-17"""


class PanicError(RuntimeError):
    """A Rust `panic!` / `assert!` in the reference."""


class InteriorNulByte(Error): pass          # src/aligner/error.rs:7
class NoBandwidth(Error): pass              # src/aligner/error.rs:8
class NoStats(Error): pass                  # src/alignment/error.rs:6-10
class NoTable(Error): pass
class NoStatsTable(Error): pass
class NoRowCol(Error): pass
class NoTrace(Error): pass
class FailedLookup(Error): pass             # src/matrix/mod.rs:65-67
class NullMatrix(Error): pass
class NotSquare(Error): pass
class NotBuiltIn(Error): pass
class InvalidIndex(Error): pass
class FileNotFound(Error): pass
class NullProfile(Error): pass              # src/profile/mod.rs:101-103
class QueryIsEmpty(Error): pass             # src/profile/mod.rs:299-301
class BatchError(Error): pass               # additive batch API


def _cstring(b):
    b = bytes(b)
    if b"\0" in b:
        raise InteriorNulByte("nul byte found in provided data")     # CString::new, src/aligner/mod.rs:399,:409
    return b


# ------------------------------------------------------------------ Matrix ----
class Matrix:
    """src/matrix/mod.rs:25-312"""

    def __init__(self, inner, builtin):
        self.inner = inner
        self.builtin = builtin

    @classmethod
    def create(cls, alphabet, match_score, mismatch_score):
        if not (match_score >= 0 and mismatch_score <= 0):
            raise PanicError("Match score should be a positive integer and mismatch score should be a negative integer.")
        if len(alphabet) == 0:
            raise PanicError("Alphabet should not be empty.")
        return cls(lib.parasail_matrix_create(_cstring(alphabet), match_score, mismatch_score), False)

    @classmethod
    def from_name(cls, matrix_name):
        """`Matrix::from(name)`, src/matrix/mod.rs:57-73"""
        if not matrix_name:
            raise PanicError("Matrix name should not be empty.")
        m = lib.parasail_matrix_lookup(_cstring(matrix_name.encode()))
        if not m:
            raise FailedLookup(matrix_name)
        return cls(m, True)

    @classmethod
    def from_file(cls, file):
        if not os.path.exists(file):
            raise FileNotFound(file)
        m = lib.parasail_matrix_from_file(_cstring(file.encode()))
        if not m:
            raise NullMatrix()
        return cls(m, False)

    @classmethod
    def create_pssm(cls, alphabet, values, rows):
        vals = (C.c_int * max(len(values), rows * len(alphabet)))(*values)
        m = lib.parasail_matrix_pssm_create(_cstring(alphabet.encode() if isinstance(alphabet, str) else alphabet),
                                            vals, rows)
        if not m:
            raise NullMatrix()
        return cls(m, False)

    def to_pssm(self, pssm_query):
        if len(pssm_query) == 0:
            raise PanicError("PSSM query sequence should not be empty.")
        if self.inner.contents.type_ != 0:
            raise NotSquare()
        m = lib.parasail_matrix_convert_square_to_pssm(self.inner, _cstring(pssm_query), len(pssm_query))
        if not m:
            raise NullMatrix()
        return Matrix(m, False)

    def set_value(self, row, col, value):
        if self.builtin:
            raise NotBuiltIn()
        size = self.inner.contents.size - 2
        if size < 0:
            raise NullMatrix()
        if row < 0 or row > size or col < 0 or col > size:
            raise InvalidIndex(row, col)
        lib.parasail_matrix_set_value(self.inner, row, col, value)

    @classmethod
    def default(cls):
        return cls.create(b"ACGTA", 1, -1)           # src/matrix/mod.rs:246-250

    def clone(self):
        return Matrix(lib.parasail_matrix_copy(self.inner), False)

    @property
    def size(self):
        return self.inner.contents.size

    @property
    def length(self):
        return self.inner.contents.length

    def to_numpy(self):
        c = self.inner.contents
        return np.ctypeslib.as_array(c.matrix, shape=(c.length, c.size)).copy()

    def mapper(self):
        return np.ctypeslib.as_array(self.inner.contents.mapper, shape=(256,)).copy()

    def __str__(self):                               # src/matrix/mod.rs:253-268
        return "".join(" ".join(str(v) for v in row) + " \n" for row in self.to_numpy())

    def __del__(self):
        try:
            if not self.builtin and self.inner:
                lib.parasail_matrix_free(self.inner)
        except Exception:
            pass


# ------------------------------------------------------------------ Profile ---
class SolutionWidth:
    Sat, Bit8, Bit16, Bit32, Bit64 = "sat", "8", "16", "32", "64"      # src/prelude.rs:9-15


class InstructionSet:
    Best, SSE2, SSE41, AVX2, AltiVec, Neon = "", "_sse_128", "_sse_128", "_avx_256", "_altivec_128", "_neon_128"


class Profile:
    """src/profile/mod.rs:281-395"""

    def __init__(self, inner, use_stats, query_len, matrix=None):
        self.inner = inner
        self.use_stats = use_stats
        self.query_len = query_len
        self._matrix = matrix          # keep the matrix alive (the C profile borrows it)

    @classmethod
    def new(cls, query_bytes, with_stats, matrix):
        if len(query_bytes) == 0:
            raise QueryIsEmpty()
        q = _cstring(query_bytes)
        name = "parasail_profile_create_stats_sat" if with_stats else "parasail_profile_create_sat"
        return cls._create(name, q, with_stats, matrix)

    @classmethod
    def _create(cls, name, q, with_stats, matrix):
        f = getattr(lib, name)
        f.restype = C.c_void_p
        f.argtypes = [C.c_char_p, C.c_int, _MP]
        p = f(q, len(q), matrix.inner)
        if not p:
            raise NullProfile()
        return cls(p, bool(with_stats), len(q), matrix)

    @classmethod
    def builder(cls, query, matrix):
        return ProfileBuilder(query, matrix)

    @classmethod
    def new_ssw(cls, query_bytes, matrix, score_size):
        if len(query_bytes) == 0:
            raise PanicError("Query sequence has length 0.")
        q = _cstring(query_bytes)
        p = lib.parasail_ssw_init(q, len(q), matrix.inner, score_size)
        if not p:
            raise NullProfile()
        return cls(p, True, len(q), matrix)

    @classmethod
    def default(cls):
        return cls(None, False, 0)                   # null profile = "no profile", src/profile/mod.rs:365-373

    def is_null(self):
        return not self.inner

    def __del__(self):
        try:
            if self.inner:
                lib.parasail_profile_free(self.inner)
        except Exception:
            pass


class ProfileBuilder:
    """src/profile/mod.rs:42-278"""

    def __init__(self, query, matrix):
        self.query, self.matrix = query, matrix
        self._stats, self._width, self._isa = False, SolutionWidth.Sat, InstructionSet.Best

    def use_stats(self):
        self._stats = True
        return self

    def solution_width(self, w):
        self._width = w
        return self

    def instruction_set(self, isa):
        self._isa = isa
        return self

    def build(self):
        name = "parasail_profile_create%s%s_%s" % ("_stats" if self._stats else "", self._isa, self._width)
        return Profile._create(name, _cstring(self.query), self._stats, self.matrix)


# ------------------------------------------------------------------ tables ----
class TraceFlags:
    """src/alignment/table.rs:127-142"""
    ZERO_MASK, E_MASK, F_MASK = 120, 103, 31
    ZERO, INS, DEL, DIAG, DIAG_E, INS_E, DIAG_F, DEL_F = 0, 1, 2, 4, 8, 16, 32, 64


class Table:
    """src/alignment/table.rs:33-108 (row-major [query_len][ref_len] int32 view)"""

    def __init__(self, data, rows, cols, owner):
        self.inner, self._rows, self._cols, self._owner = data, rows, cols, owner

    def get(self, row, col):
        if row < self._rows and col < self._cols:
            return int(self.inner[row * self._cols + col])
        return None

    def rows(self):
        return self._rows

    def cols(self):
        return self._cols

    def as_slice(self):
        return self.inner

    def last(self):
        return int(self.inner[len(self.inner) - 1])


class TracebackTable(Table):
    """src/alignment/table.rs:197-300 (1 byte per cell)"""

    def get(self, row, col):
        v = self.get_detailed(row, col)
        return None if v is None else v & (TraceFlags.DIAG | TraceFlags.INS | TraceFlags.DEL)

    def get_detailed(self, row, col):
        if row < self._rows and col < self._cols:
            return int(self.inner[row * self._cols + col]) & 127
        return None


class Traceback:
    def __init__(self, query, comparison, reference):
        self.query, self.comparison, self.reference = query, comparison, reference


# ------------------------------------------------------------------ Alignment --
class Alignment:
    """src/alignment/mod.rs:54-504"""

    def __init__(self, inner, matrix, query_len, ref_len):
        self.inner, self.matrix, self.query_len, self.ref_len = inner, matrix, query_len, ref_len

    def get_score(self): return lib.parasail_result_get_score(self.inner)
    def get_end_query(self): return lib.parasail_result_get_end_query(self.inner)
    def get_end_ref(self): return lib.parasail_result_get_end_ref(self.inner)

    def get_matches(self):
        if self.is_stats():
            return lib.parasail_result_get_matches(self.inner)
        raise NoStats("get_matches()")

    def get_similar(self):                       # no is_stats guard in the reference (:87-89)
        return lib.parasail_result_get_similar(self.inner)

    def get_length(self):
        if self.is_stats():
            return lib.parasail_result_get_length(self.inner)
        raise NoStats("get_length()")

    def _table(self, kind):
        p = getattr(lib, "parasail_result_get_%s_table" % kind)(self.inner)
        n = self.query_len * self.ref_len
        return Table(np.ctypeslib.as_array(p, shape=(n,)), self.query_len, self.ref_len, self)

    def get_score_table(self):
        if self.is_table() or self.is_stats_table():
            return self._table("score")
        raise NoTable("get_score_table()")

    def get_matches_table(self):
        if self.is_stats_table():
            return self._table("matches")
        raise NoStatsTable("get_matches_table()")

    def get_similar_table(self):
        if self.is_stats_table():
            return self._table("similar")
        raise NoStatsTable("get_similar_table()")

    def get_length_table(self):
        if self.is_stats_table():
            return self._table("length")
        raise NoStatsTable("get_length_table()")

    def _rowcol(self, kind, which, fname):
        plain_ok = kind == "score" and self.is_rowcol()
        if not (plain_ok or self.is_stats_rowcol()):
            raise NoRowCol(fname)
        p = getattr(lib, "parasail_result_get_%s_%s" % (kind, which))(self.inner)
        n = self.ref_len if which == "row" else self.query_len
        return np.ctypeslib.as_array(p, shape=(n,))

    def get_score_row(self): return self._rowcol("score", "row", "get_score_row()")
    def get_matches_row(self): return self._rowcol("matches", "row", "get_matches_row()")
    def get_similar_row(self): return self._rowcol("similar", "row", "get_similar_row()")
    def get_length_row(self): return self._rowcol("length", "row", "get_length_row()")
    def get_score_col(self): return self._rowcol("score", "col", "get_score_col()")
    def get_matches_col(self): return self._rowcol("matches", "col", "get_matches_col()")
    def get_similar_col(self): return self._rowcol("similar", "col", "get_similar_col()")
    def get_length_col(self): return self._rowcol("length", "col", "get_length_col()")

    def get_trace_table(self):
        if not self.is_trace():
            raise NoTrace("get_trace_table()")
        p = C.cast(lib.parasail_result_get_trace_table(self.inner), C.POINTER(C.c_int8))
        n = self.query_len * self.ref_len
        return TracebackTable(np.ctypeslib.as_array(p, shape=(n,)), self.query_len, self.ref_len, self)

    def print_traceback(self, query, reference):
        if self.is_trace():
            lib.parasail_traceback_generic(_cstring(query), len(query), _cstring(reference), len(reference),
                                           b"Query:", b"Target:", self.matrix.inner, self.inner,
                                           b"|", b" ", b" ", 80, 7, 1)
        else:
            print("Alignment string is not available without traceback enabled. "
                  "Consider using the `use_trace` method on AlignerBuilder.")

    def get_traceback_strings(self, query, reference):
        if not self.is_trace():
            raise NoTrace("get_traceback_strings()")
        tb = lib.parasail_result_get_traceback(self.inner, _cstring(query), len(query), _cstring(reference),
                                               len(reference), self.matrix.inner, b"|", b" ", b" ")
        if not tb:
            raise NoTrace("get_traceback_strings()")
        out = Traceback(*(C.string_at(getattr(tb.contents, f)).decode() for f in ("query", "comp", "ref_")))
        lib.parasail_traceback_free(tb)
        return out

    def get_cigar(self, query, reference):
        if not self.is_trace():
            raise NoTrace("get_cigar()")
        c = lib.parasail_result_get_cigar(self.inner, _cstring(query), len(query), _cstring(reference),
                                          len(reference), self.matrix.inner)
        if not c:
            raise NoTrace("get_cigar()")
        s = lib.parasail_cigar_decode(c)
        text = C.string_at(s).decode()
        _libc_free(s)                 # plain malloc block (Rust adopts it with CString::from_raw, :410)
        lib.parasail_cigar_free(c)
        return text

    def get_cigar_begin(self, query, reference):
        """(beg_query, beg_ref) of the walked alignment -- fields of parasail_cigar_t."""
        c = lib.parasail_result_get_cigar(self.inner, _cstring(query), len(query), _cstring(reference),
                                          len(reference), self.matrix.inner)
        out = (c.contents.beg_query, c.contents.beg_ref)
        lib.parasail_cigar_free(c)
        return out

    def is_global(self): return lib.parasail_result_is_nw(self.inner) != 0
    def is_semi_global(self): return lib.parasail_result_is_sg(self.inner) != 0
    def is_local(self): return lib.parasail_result_is_sw(self.inner) != 0
    def is_saturated(self): return lib.parasail_result_is_saturated(self.inner) != 0
    def is_banded(self): return lib.parasail_result_is_banded(self.inner) != 0
    def is_scan(self): return lib.parasail_result_is_scan(self.inner) != 0
    def is_striped(self): return lib.parasail_result_is_striped(self.inner) != 0
    def is_diag(self): return lib.parasail_result_is_diag(self.inner) != 0
    def is_blocked(self): return lib.parasail_result_is_blocked(self.inner) != 0
    def is_stats(self): return lib.parasail_result_is_stats(self.inner) != 0
    def is_stats_table(self): return lib.parasail_result_is_stats_table(self.inner) != 0
    def is_table(self): return lib.parasail_result_is_table(self.inner) != 0
    def is_rowcol(self): return lib.parasail_result_is_rowcol(self.inner) != 0
    def is_stats_rowcol(self): return lib.parasail_result_is_stats_rowcol(self.inner) != 0
    def is_trace(self): return lib.parasail_result_is_trace(self.inner) != 0

    def __del__(self):
        try:
            lib.parasail_result_free(self.inner)
        except Exception:
            pass


class SSWResult:
    """src/alignment/mod.rs:506-551"""

    def __init__(self, inner):
        self.inner = inner

    def score(self): return self.inner.contents.score1
    def ref_start(self): return self.inner.contents.ref_begin1
    def ref_end(self): return self.inner.contents.ref_end1
    def query_start(self): return self.inner.contents.read_begin1
    def query_end(self): return self.inner.contents.read_end1
    def cigar(self): return self.inner.contents.cigar
    def cigar_len(self): return self.inner.contents.cigarLen

    def __del__(self):
        try:
            lib.parasail_result_ssw_free(self.inner)
        except Exception:
            pass


# ------------------------------------------------------------------ Aligner ---
class AlignerBuilder:
    """src/aligner/mod.rs:67-370"""

    def __init__(self):
        self._mode = "nw"
        self._solution_width = "sat"
        self._matrix = Matrix.default()
        self._gap_open = 0                       # defaults are 0/0 (:92-93) although the docs say 5 and 2
        self._gap_extend = 0
        self._profile = Profile.default()
        self._allow_query_gaps = []
        self._allow_ref_gaps = []
        self._vec_strategy = "_striped"
        self._use_stats = ""
        self._use_table = ""
        self._use_trace = ""
        self._bandwidth = None

    def global_(self): self._mode = "nw"; return self
    def semi_global(self): self._mode = "sg"; return self
    def local(self): self._mode = "sw"; return self
    def solution_width(self, w): self._solution_width = str(int(w)); return self
    def matrix(self, m): self._matrix = m; return self
    def gap_open(self, v): self._gap_open = v; return self
    def gap_extend(self, v): self._gap_extend = v; return self
    def profile(self, p): self._profile = p; return self
    def allow_query_gaps(self, g): self._allow_query_gaps = list(g); return self
    def allow_ref_gaps(self, g): self._allow_ref_gaps = list(g); return self
    def striped(self): self._vec_strategy = "_striped"; return self
    def scan(self): self._vec_strategy = "_scan"; return self
    def diag(self): self._vec_strategy = "_diag"; return self

    def use_stats(self):                         # :213-223
        self._use_stats = "_stats"
        self._use_trace = ""
        return self

    def use_table(self):                         # :228-237
        self._use_table = "_table"
        self._use_trace = ""
        return self

    def use_last_rowcol(self):                   # :243-246 (does not clear trace)
        self._use_table = "_rowcol"
        return self

    def use_trace(self):                         # :251-267
        self._use_trace = "_trace"
        self._use_table = ""
        self._use_stats = ""
        return self

    def bandwidth(self, k): self._bandwidth = k; return self

    @staticmethod
    def _allowed_gaps(prefix, gaps):             # :270-286
        if gaps:
            if "prefix" in gaps and "suffix" in gaps:
                return "_%sx" % prefix
            if "prefix" in gaps:
                return "_%sb" % prefix
            if "suffix" in gaps:
                return "_%se" % prefix
        return ""

    def get_parasail_fn_name(self):              # :289-331
        sg = ""
        if self._mode == "sg":
            sg = self._allowed_gaps("q", self._allow_query_gaps) + self._allowed_gaps("d", self._allow_ref_gaps)
            if sg == "_qx_dx":
                sg = ""
        if self._profile.is_null():
            profile, stats = "", self._use_stats
        else:
            if self._vec_strategy not in ("_striped", "_scan"):
                raise PanicError("Vectorization strategy must be striped or scan for alignment with a profile.")
            profile = "_profile"
            stats = "_stats" if self._profile.use_stats else ""
        return "%s%s%s%s%s%s%s_%s" % (self._mode, sg, self._use_trace, stats, self._use_table,
                                      self._vec_strategy, profile, self._solution_width)

    def build(self):                             # :339-369
        name = self.get_parasail_fn_name()
        if self._profile.is_null():
            f = lib.parasail_lookup_function(name.encode())
            fn = _FN(f) if f else None
        else:
            f = lib.parasail_lookup_pfunction(name.encode())
            fn = _PFN(f) if f else None
        if fn is None:
            raise PanicError("Parasail function: %s, not found." % name)
        return Aligner(fn, name, self._matrix, self._gap_open, self._gap_extend, self._profile,
                       self._vec_strategy, self._bandwidth)


class Aligner:
    """src/aligner/mod.rs:372-535"""

    def __init__(self, fn, fn_name, matrix, gap_open, gap_extend, profile, vec_strategy, bandwidth):
        self._fn, self.fn_name = fn, fn_name
        self.matrix, self.gap_open, self.gap_extend = matrix, gap_open, gap_extend
        self._profile, self.vec_strategy, self._bandwidth = profile, vec_strategy, bandwidth
        # batch entries of a semi-global aligner only: a set of SG_* flags that replaces the one the function name spells
        # (a name cannot say "no free end": without a specifier it means all four)
        self.sg_flags = None

    @staticmethod
    def new():
        return AlignerBuilder()

    def clone(self):
        al = Aligner(self._fn, self.fn_name, self.matrix, self.gap_open, self.gap_extend, self._profile,
                     self.vec_strategy, self._bandwidth)
        al.sg_flags = self.sg_flags
        return al

    def align(self, query, reference):           # :397-452
        ref_len = len(reference)
        reference = _cstring(reference)
        if self._profile.is_null():
            if query is None:
                raise PanicError("Query sequence is required for alignment without a profile.")
            query_len = len(query)
            q = _cstring(query)
            res = self._fn(q, query_len, reference, ref_len, self.gap_open, self.gap_extend, self.matrix.inner)
            return Alignment(res, self.matrix, query_len, ref_len)
        res = self._fn(self._profile.inner, reference, ref_len, self.gap_open, self.gap_extend)
        return Alignment(res, self.matrix, self._profile.query_len, ref_len)

    def banded_nw(self, query, reference):       # :457-489
        ref_len, query_len = len(reference), len(query)
        reference, q = _cstring(reference), _cstring(query)
        if self._bandwidth is None:
            raise NoBandwidth()
        res = lib.parasail_nw_banded(q, query_len, reference, ref_len, self.gap_open, self.gap_extend,
                                     self._bandwidth, self.matrix.inner)
        return Alignment(res, self.matrix, query_len, ref_len)

    def ssw(self, query, reference):             # :492-529
        ref_len = len(reference)
        reference = _cstring(reference)
        if query is None:
            raise PanicError("Query sequence is required for SSW alignment for now.")
        q = _cstring(query)
        return SSWResult(lib.parasail_ssw(q, len(q), reference, ref_len, self.gap_open, self.gap_extend,
                                          self.matrix.inner))

    # ---- additive batch interface (no reference counterpart) -----------------------------
    def _config(self, want=0):
        name = self.fn_name
        mode = {"nw": MODE_NW, "sg": MODE_SG, "sw": MODE_SW}[name[:2]]
        flags = 0
        if mode == MODE_SG:
            head = name.split("_striped")[0].split("_scan")[0].split("_diag")[0]
            q = [t for t in ("_qb", "_qe", "_qx") if t in head]
            d = [t for t in ("_db", "_de", "_dx") if t in head]
            if not q and not d:
                flags = SG_ALL
            else:
                for t in q + d:
                    flags |= {"_qb": SG_QB, "_qe": SG_QE, "_qx": SG_QB | SG_QE,
                              "_db": SG_DB, "_de": SG_DE, "_dx": SG_DB | SG_DE}[t]
            if self.sg_flags is not None:
                flags = int(self.sg_flags) & SG_ALL
        width = name.rsplit("_", 1)[1]
        if "_stats" in name:
            want |= WANT_STATS
        cfg = pmx_config_t(mode, flags, self.gap_open, self.gap_extend, 0 if width == "sat" else int(width),
                           want, self.matrix.inner)
        return cfg

    def align_batch(self, queries, references):
        """Many independent pairs in one call.  Returns a structured array with fields
        score, end_query, end_ref, flags (and, for a stats aligner, a second array with
        matches, similar, length).  A PSSM matrix is taken when every query (or the profile's
        query) has the PSSM's length; each record equals align()'s with the same PSSM."""
        qbuf, qoff = pack(queries)
        rbuf, roff = pack(references)
        return self.align_batch_packed(qbuf, qoff, rbuf, roff)

    def align_batch_packed(self, qbuf, qoff, rbuf, roff, out=None):
        """`out`: a RECORD_DTYPE array of n records to fill (a caller that aligns batch after batch reuses one, already paged in)."""
        n = len(roff) - 1
        cfg = self._config()
        out = _record_buffer(out, n)
        stats = np.zeros(n, dtype=STATS_DTYPE) if cfg.want & WANT_STATS else None
        if self._profile.is_null():
            if len(qoff) - 1 != n:
                raise BatchError("queries and references differ in count")
            rc = lib.pmx_align_batch(C.byref(cfg), n, qbuf.ctypes.data, qoff.ctypes.data, rbuf.ctypes.data,
                                     roff.ctypes.data, out.ctypes.data, stats.ctypes.data if stats is not None else None)
        else:
            rc = lib.pmx_align_profile_batch(C.byref(cfg), self._profile.inner, n, rbuf.ctypes.data,
                                             roff.ctypes.data, out.ctypes.data,
                                             stats.ctypes.data if stats is not None else None)
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        return (out, stats) if stats is not None else out

    def align_pairs(self, Q, R, pairs, chunk_pairs=0, strand=None, cigar=False, frame=None, code=None, ref_frame=None, frameshift=None,
                    ref_frameshift=None, ref_strand=None):
        """Pairs by index and window into device-resident sequence sets (SeqSet; Q may be R).  `pairs`: a PAIR_DTYPE array, or
        an iterable of (q, r) / (q, r, q_beg, q_len, r_beg, r_len) tuples (len -1: to the sequence's end).  Record k is the record
        of the pair (query window, reference window) k, end positions relative to the windows.  A bad descriptor raises BatchError
        naming the first.  `strand`: one byte per pair, 1 = the query window reverse-complemented (complement_table(); every
        position of such a pair is relative to the reverse-complemented window).  cigar=True returns (records, CIGAR strings,
        int32 [n, 2] begins of the paths) instead.  strand="both": every pair on both strands, the better one kept (a tie: the
        forward strand) -- (records, strand) or (records, stats, strand), strand a uint8 array saying which one won; with
        cigar=True the CIGARs of the winners, (records, cigars, begins, strand).  `frame` (not together with strand): Q holds
        nucleotides, R proteins, and the query windows are translated (translate() restates the rule) -- a frame 0 .. 5, "forward" /
        "reverse" / "all" (FRAMES_*: the best of those frames, a tie to the lowest) or one frame byte per pair; positions are in
        letters of the translated query; returns (records, frames) or (records, stats, frames).  code: 64 letters that replace
        genetic_code_table().  `ref_frame` (not together with frame or strand): the opposite pairing -- Q holds proteins, R
        nucleotides, the REFERENCE windows are translated; the same values and results, positions in letters of the translated
        reference, the frames are the reference's.  `frameshift` (a penalty >= 0; not together with frame or ref_frame): Q holds
        nucleotides, R proteins, and every pair is aligned by the three-frame local DP that may change its reading frame
        (codon_stream() restates the query side) -- strand None or 0: as stored, 1: reverse-complemented, "both", or one byte per
        pair; end_query is in NUCLEOTIDES of the oriented window; returns (records, strand).  `ref_frameshift` (a penalty >= 0; not
        together with frame, ref_frame, frameshift, strand or cigar): the opposite pairing -- Q holds proteins, R nucleotides of any
        length, and the three-frame DP runs over the REFERENCE window's codon stream; ref_strand None or 0: the reference as stored,
        1: reverse-complemented, "both", or one byte per pair; end_ref is in NUCLEOTIDES of the oriented reference window, end_query
        in letters; returns (records, strand), the strand being the reference's."""
        if not self._profile.is_null():
            raise BatchError("align_pairs takes no profile")
        pairs = as_pairs(pairs)
        n = len(pairs)
        cfg = self._config()
        out = np.zeros(n, dtype=RECORD_DTYPE)
        stats = np.zeros(n, dtype=STATS_DTYPE) if cfg.want & WANT_STATS else None
        opts = pmx_pairs_opts_t(int(chunk_pairs))
        ref_side = _ref_frameshift_side(ref_frameshift, ref_strand, frame, ref_frame, frameshift, strand is not None, cigar)
        if frameshift is not None or ref_side:
            if ref_side:
                frameshift, strand = ref_frameshift, ref_strand
            else:
                _frameshift_side(frame, ref_frame)
            if cigar:
                cfg.want |= WANT_CIGAR                   # (refused by the entry)
            per_pair = None
            if strand is None or isinstance(strand, str) or np.ndim(strand) == 0:
                mode = _strand_mode(0 if strand is None else strand)
            else:
                mode, per_pair = STRAND_FORWARD, np.ascontiguousarray(strand, dtype=np.uint8)
                if len(per_pair) != n:
                    raise BatchError("strand and pairs differ in count")
            code = _code_arg(code)
            won = np.zeros(n, dtype=np.uint8)
            entry = lib.pmx_align_pairs_frameshift_ref if ref_side else lib.pmx_align_pairs_frameshift
            rc = entry(C.byref(cfg), Q._handle(), R._handle(), n, pairs.ctypes.data,
                       per_pair.ctypes.data if per_pair is not None else None, mode, int(frameshift),
                       code.ctypes.data if code is not None else None, out.ctypes.data, won.ctypes.data, C.byref(opts))
            if rc:
                raise BatchError(lib.pmx_last_error().decode())
            return out, won
        entry, frame = _frame_side(frame, ref_frame, strand is not None, lib.pmx_align_pairs_translated, lib.pmx_align_pairs_translated_ref)
        if frame is not None:
            if cigar:
                cfg.want |= WANT_CIGAR                   # (refused by the entry, which names the route)
            mode, per_pair = _frame_mode(frame, n)
            code = _code_arg(code)
            won = np.zeros(n, dtype=np.uint8)
            rc = entry(C.byref(cfg), Q._handle(), R._handle(), n, pairs.ctypes.data,
                       per_pair.ctypes.data if per_pair is not None else None, mode,
                       code.ctypes.data if code is not None else None, out.ctypes.data,
                       stats.ctypes.data if stats is not None else None, won.ctypes.data, C.byref(opts))
            if rc:
                raise BatchError(lib.pmx_last_error().decode())
            return (out, stats, won) if stats is not None else (out, won)
        if isinstance(strand, str):
            if strand != "both":
                raise BatchError("strand is a byte per pair or \"both\"")
            won = np.zeros(n, dtype=np.uint8)
            if cigar:                                   # the fold needs scores only; the CIGAR pass runs the winners' strands
                cfg.want &= ~WANT_STATS
                stats = None
            rc = lib.pmx_align_pairs_both(C.byref(cfg), Q._handle(), R._handle(), n, pairs.ctypes.data, out.ctypes.data,
                                          stats.ctypes.data if stats is not None else None, won.ctypes.data, C.byref(opts))
            if rc:
                raise BatchError(lib.pmx_last_error().decode())
            if cigar:
                return self.align_pairs(Q, R, pairs, chunk_pairs=chunk_pairs, strand=won, cigar=True) + (won,)
            return (out, stats, won) if stats is not None else (out, won)
        if strand is None and not cigar:
            rc = lib.pmx_align_pairs(C.byref(cfg), Q._handle(), R._handle(), n, pairs.ctypes.data, out.ctypes.data,
                                     stats.ctypes.data if stats is not None else None, C.byref(opts))
            if rc:
                raise BatchError(lib.pmx_last_error().decode())
            return (out, stats) if stats is not None else out
        if strand is not None:
            strand = np.ascontiguousarray(strand, dtype=np.uint8)
            if len(strand) != n:
                raise BatchError("strand and pairs differ in count")
        sp = strand.ctypes.data if strand is not None else None
        if not cigar:
            rc = lib.pmx_align_pairs_ex(C.byref(cfg), Q._handle(), R._handle(), n, pairs.ctypes.data, sp, out.ctypes.data,
                                        stats.ctypes.data if stats is not None else None, None, None, None, C.byref(opts))
            if rc:
                raise BatchError(lib.pmx_last_error().decode())
            return (out, stats) if stats is not None else out
        cfg.want |= WANT_CIGAR
        beg = np.zeros((n, 2), dtype=np.int32)
        coff = np.zeros(n + 1, dtype=np.int64)
        cbuf = C.c_void_p()
        rc = lib.pmx_align_pairs_ex(C.byref(cfg), Q._handle(), R._handle(), n, pairs.ctypes.data, sp, out.ctypes.data, None,
                                    beg.ctypes.data, C.byref(cbuf), coff.ctypes.data, C.byref(opts))
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        return out, _take_cigars(cbuf, coff), beg

    def align_pairs_frameshift_cigar(self, Q, R, pairs, frameshift, strand=0, code=None, stats=False, chunk_pairs=0):
        """The alignments behind align_pairs(..., frameshift=): the same records and strand bytes, and for every pair the CIGAR text
        of its path -- '=' / 'X' one codon against one reference letter, 'I' a codon against a gap, 'D' a reference letter against
        a gap, '/' one nucleotide missing from the read, '\\' one too many (include/parasail_amd.h, "Frameshift traceback") -- and
        the path's begin, int32 [n, 2]: the first nucleotide of the first codon in the oriented window, and its reference column.
        `strand` is 0, 1, "both" or one byte per pair, as align_pairs(frameshift=) takes it: PairHits.pairs and PairHits.strand of
        search_pairs(frameshift=) or search_topk(frameshift=) are accepted as they are.  Returns (records, cigars, begins, strand)
        or, with stats=True, (records, cigars, begins, strand, stats): matches, similar and length along the path."""
        return self._frameshift_cigar(lib.pmx_align_pairs_frameshift_cigar, "align_pairs_frameshift_cigar", Q, R, pairs, frameshift, strand,
                                      code, stats, chunk_pairs)

    def align_pairs_frameshift_ref_cigar(self, Q, R, pairs, ref_frameshift, ref_strand=0, code=None, stats=False, chunk_pairs=0):
        """The alignments behind align_pairs(..., ref_frameshift=): the same records and strand bytes, and for every pair the CIGAR
        text of its path -- '=' / 'X' one query letter against one reference codon, 'I' a query letter against a gap, 'D' a whole
        reference codon against a gap, '/' one nucleotide missing from the REFERENCE, '\\' one too many (include/parasail_amd.h,
        "Frameshift traceback, reference side") -- and the path's begin, int32 [n, 2]: the query letter, and the first nucleotide of
        the first codon in the oriented reference window.  `ref_strand` is 0, 1, "both" or one byte per pair, as
        align_pairs(ref_frameshift=) takes it: PairHits.pairs and PairHits.strand of search_pairs(ref_frameshift=) or
        search_topk(ref_frameshift=) are accepted as they are.  Returns (records, cigars, begins, strand) or, with stats=True,
        (records, cigars, begins, strand, stats): matches, similar and length along the path."""
        return self._frameshift_cigar(lib.pmx_align_pairs_frameshift_ref_cigar, "align_pairs_frameshift_ref_cigar", Q, R, pairs, ref_frameshift,
                                      ref_strand, code, stats, chunk_pairs)

    def align_pairs_frameshift_ref_cigar_long(self, Q, R, pairs, ref_frameshift, ref_strand=0, code=None, stats=False, chunk_pairs=0):
        """align_pairs_frameshift_ref_cigar for long references: the same arguments and, byte for byte, the same results, but the
        traceback runs only over the window of each reference that a path of the record's score can span (include/parasail_amd.h,
        "Windowed frameshift traceback, reference side"), so a protein against a 100 kb contig is taken where
        align_pairs_frameshift_ref_cigar refuses the trace of the whole matrix."""
        return self._frameshift_cigar(lib.pmx_align_pairs_frameshift_ref_cigar_long, "align_pairs_frameshift_ref_cigar_long", Q, R, pairs,
                                      ref_frameshift, ref_strand, code, stats, chunk_pairs)

    def _frameshift_cigar(self, entry, name, Q, R, pairs, frameshift, strand, code, stats, chunk_pairs):
        """The host traceback entry of either side (`entry`) over listed pairs."""
        if not self._profile.is_null():
            raise BatchError(name + " takes no profile")
        pairs = as_pairs(pairs)
        n = len(pairs)
        cfg = self._config()
        cfg.want = (cfg.want & ~WANT_STATS) | WANT_CIGAR | (WANT_STATS if stats else 0)
        per_pair = None
        if strand is None or isinstance(strand, str) or np.ndim(strand) == 0:
            mode = _strand_mode(0 if strand is None else strand)
        else:
            mode, per_pair = STRAND_FORWARD, np.ascontiguousarray(strand, dtype=np.uint8)
            if len(per_pair) != n:
                raise BatchError("strand and pairs differ in count")
        code = _code_arg(code)
        out = np.zeros(n, dtype=RECORD_DTYPE)
        won = np.zeros(n, dtype=np.uint8)
        st = np.zeros(n, dtype=STATS_DTYPE) if stats else None
        beg = np.zeros((n, 2), dtype=np.int32)
        coff = np.zeros(n + 1, dtype=np.int64)
        cbuf = C.c_void_p()
        opts = pmx_pairs_opts_t(int(chunk_pairs))
        rc = entry(C.byref(cfg), Q._handle(), R._handle(), n, pairs.ctypes.data,
                   per_pair.ctypes.data if per_pair is not None else None, mode, int(frameshift),
                   code.ctypes.data if code is not None else None, out.ctypes.data, won.ctypes.data,
                   st.ctypes.data if st is not None else None, beg.ctypes.data, C.byref(cbuf),
                   coff.ctypes.data, C.byref(opts))
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        res = (out, _take_cigars(cbuf, coff), beg, won)
        return res + (st,) if stats else res

    def align_all_pairs(self, S, first=0, count=None, chunk_pairs=0):
        """Pairs [first, first + count) of the strict upper triangle of S x S (row-major; all_pairs_index gives (i, j) of a
        pair), whole sequences, enumerated on the device.  count None: to the last pair."""
        if not self._profile.is_null():
            raise BatchError("align_all_pairs takes no profile")
        if count is None:
            count = all_pairs_count(len(S)) - int(first)
        cfg = self._config()
        out = np.zeros(max(int(count), 0), dtype=RECORD_DTYPE)
        stats = np.zeros(len(out), dtype=STATS_DTYPE) if cfg.want & WANT_STATS else None
        opts = pmx_pairs_opts_t(int(chunk_pairs))
        rc = lib.pmx_align_all_pairs(C.byref(cfg), S._handle(), int(first), int(count), out.ctypes.data,
                                     stats.ctypes.data if stats is not None else None, C.byref(opts))
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        return (out, stats) if stats is not None else out

    def search_pairs(self, Q, R=None, min_score=0, pairs=None, first=0, count=None, stats=False, max_hits=0, chunk_pairs=0,
                     slice_pairs=0, strand=0, frame=None, code=None, ref_frame=None, frameshift=None, ref_frameshift=None, ref_strand=None):
        """Set search: the pairs of an enumeration that score at least min_score, as a PairHits in enumeration order.  `pairs`
        given: those descriptors of Q x R (as align_pairs takes them; R None: Q); else R None: pairs [first, first + count) of the
        strict upper triangle of Q (the numbering of align_all_pairs); else the same window of the rectangle Q x R, row-major
        (pair p = (p // len(R), p % len(R)); R may be Q, the diagonal included).  count None: to the last pair.  stats=True adds the
        hits' statistics.  max_hits > 0 keeps the first max_hits hits and goes on counting n_passing.  Only the hits leave the
        device; chunk_pairs and slice_pairs never change the result.  strand: 0 the queries as stored, 1 reverse-complemented,
        "both" (or STRAND_BOTH) the better strand of every pair, chosen before the threshold; PairHits.strand tells which.
        frame (not together with strand): nucleotide queries against proteins, translated in frame 0 .. 5 or the best of "forward" /
        "reverse" / "all" frames, chosen before the threshold; PairHits.frame tells which (code: as in align_pairs).  ref_frame (not
        together with frame or strand): protein queries against nucleotide references, the references translated the same way;
        PairHits.frame is then the reference's frame.  frameshift (a penalty >= 0; with strand, not together with frame or
        ref_frame): nucleotide queries against proteins by the three-frame DP of align_pairs(frameshift=); PairHits.strand tells the
        strand, end_query is in nucleotides; align_pairs_frameshift_cigar(Q, R, hits.pairs, frameshift, strand=hits.strand) gives the
        hits' alignments.  ref_frameshift (a penalty >= 0; with ref_strand -- 0, 1 or "both" --, not together with frame, ref_frame,
        frameshift or strand): protein queries against nucleotide references of any length by the three-frame DP of
        align_pairs(ref_frameshift=); PairHits.strand tells the REFERENCE's strand, end_ref is in nucleotides."""
        if not self._profile.is_null():
            raise BatchError("search_pairs takes no profile")
        cfg = self._config()
        if stats:
            cfg.want |= WANT_STATS
        if pairs is not None:
            shape, R = PAIRS_LIST, (Q if R is None else R)
            pairs = as_pairs(pairs)
            first, count = 0, len(pairs)
        elif R is None:
            shape = PAIRS_TRIANGLE
            if count is None:
                count = all_pairs_count(len(Q)) - int(first)
        else:
            shape = PAIRS_RECT
            if count is None:
                count = rect_pairs_count(len(Q), len(R)) - int(first)
        opts = pmx_pair_search_opts_t(int(min_score), shape, int(max_hits), int(chunk_pairs), int(slice_pairs))
        args = (C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(first), int(count),
                pairs.ctypes.data if pairs is not None and len(pairs) else None, C.byref(opts))
        mode = _strand_mode(strand)
        if _ref_frameshift_side(ref_frameshift, ref_strand, frame, ref_frame, frameshift, mode != STRAND_FORWARD, False):
            code = _code_arg(code)
            return _hits_call(lib.pmx_search_pairs_frameshift_ref, args + (_strand_mode(0 if ref_strand is None else ref_strand), int(ref_frameshift),
                                                                           code.ctypes.data if code is not None else None),
                              pmx_strand_hits_t, PairHits, lib.pmx_strand_hits_free)
        if frameshift is not None:
            _frameshift_side(frame, ref_frame)
            code = _code_arg(code)
            return _hits_call(lib.pmx_search_pairs_frameshift, args + (mode, int(frameshift), code.ctypes.data if code is not None else None),
                              pmx_strand_hits_t, PairHits, lib.pmx_strand_hits_free)
        entry, frame = _frame_side(frame, ref_frame, mode != STRAND_FORWARD, lib.pmx_search_pairs_translated, lib.pmx_search_pairs_translated_ref)
        if frame is not None:
            code = _code_arg(code)
            return _hits_call(entry, args + (_frame_mode(frame)[0], code.ctypes.data if code is not None else None),
                              pmx_frame_hits_t, PairHits, lib.pmx_frame_hits_free)
        if mode != STRAND_FORWARD:
            return _hits_call(lib.pmx_search_pairs_stranded, args + (mode,), pmx_strand_hits_t, PairHits, lib.pmx_strand_hits_free)
        return _hits_call(lib.pmx_search_pairs, args, pmx_pair_hits_t, PairHits, lib.pmx_pair_hits_free)

    def search_topk(self, Q, R=None, k=10, min_score=INT32_MIN, skip_self=False, first_row=0, rows=None, stats=False, chunk_pairs=0,
                    slice_rows=0, strand=0, frame=None, code=None, ref_frame=None, frameshift=None, ref_frameshift=None, ref_strand=None):
        """Per-query top-K: for each query row [first_row, first_row + rows) of Q the best k references of R (None: Q) with score
        >= min_score, in (score descending, reference index ascending) order, as a TopKHits.  rows None: to the last row.
        skip_self (R is Q) leaves the pair (i, i) out.  stats=True adds the hits' statistics.  Only the hits leave the device;
        chunk_pairs and slice_rows never change the result.  strand as in search_pairs: with "both" a reference is one
        candidate with its better strand, and TopKHits.strand tells which.  frame as in search_pairs: a reference is one candidate
        with its best frame, and TopKHits.frame tells which.  ref_frame as in search_pairs: the references are the translated side.
        frameshift as in search_pairs: a reference is one candidate with its better strand under the three-frame DP, and
        align_pairs_frameshift_cigar takes TopKHits.pairs and TopKHits.strand as they are.  ref_frameshift with ref_strand as in
        search_pairs: a nucleotide reference is one candidate with its better strand, the best loci per protein."""
        if not self._profile.is_null():
            raise BatchError("search_topk takes no profile")
        cfg = self._config()
        if stats:
            cfg.want |= WANT_STATS
        if rows is None:
            rows = len(Q) - int(first_row)
        opts = pmx_topk_opts_t(int(min_score), int(k), 1 if skip_self else 0, int(chunk_pairs), int(slice_rows))
        args = (C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(first_row), int(rows), C.byref(opts))
        mode = _strand_mode(strand)
        if _ref_frameshift_side(ref_frameshift, ref_strand, frame, ref_frame, frameshift, mode != STRAND_FORWARD, False):
            code = _code_arg(code)
            return _hits_call(lib.pmx_search_topk_frameshift_ref, args + (_strand_mode(0 if ref_strand is None else ref_strand), int(ref_frameshift),
                                                                          code.ctypes.data if code is not None else None),
                              pmx_topk_strand_hits_t, TopKHits, lib.pmx_topk_strand_hits_free)
        if frameshift is not None:
            _frameshift_side(frame, ref_frame)
            code = _code_arg(code)
            return _hits_call(lib.pmx_search_topk_frameshift, args + (mode, int(frameshift), code.ctypes.data if code is not None else None),
                              pmx_topk_strand_hits_t, TopKHits, lib.pmx_topk_strand_hits_free)
        entry, frame = _frame_side(frame, ref_frame, mode != STRAND_FORWARD, lib.pmx_search_topk_translated, lib.pmx_search_topk_translated_ref)
        if frame is not None:
            code = _code_arg(code)
            return _hits_call(entry, args + (_frame_mode(frame)[0], code.ctypes.data if code is not None else None),
                              pmx_topk_frame_hits_t, TopKHits, lib.pmx_topk_frame_hits_free)
        if mode != STRAND_FORWARD:
            return _hits_call(lib.pmx_search_topk_stranded, args + (mode,), pmx_topk_strand_hits_t, TopKHits, lib.pmx_topk_strand_hits_free)
        return _hits_call(lib.pmx_search_topk, args, pmx_topk_hits_t, TopKHits, lib.pmx_topk_hits_free)

    def align_batch_2bit(self, q2, qoff, r2, roff, out=None):
        """2-bit packed input (see pack_2bit): offsets count bases.  `out` as in align_batch_packed."""
        n = len(roff) - 1
        cfg = self._config()
        out = _record_buffer(out, n)
        stats = np.zeros(n, dtype=STATS_DTYPE) if cfg.want & WANT_STATS else None
        rc = lib.pmx_align_batch_2bit(C.byref(cfg), n, q2.ctypes.data, qoff.ctypes.data, r2.ctypes.data, roff.ctypes.data,
                                      out.ctypes.data, stats.ctypes.data if stats is not None else None)
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        return (out, stats) if stats is not None else out

    def align_batch_multi(self, qbuf, qoff, rbuf, roff, devices):
        """One batch across several GPUs of the node (cell-balanced contiguous blocks, records in input order)."""
        n = len(roff) - 1
        cfg = self._config()
        out = np.zeros(n, dtype=RECORD_DTYPE)
        stats = np.zeros(n, dtype=STATS_DTYPE) if cfg.want & WANT_STATS else None
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        if self._profile.is_null():
            rc = lib.pmx_align_batch_multi(C.byref(cfg), n, qbuf.ctypes.data, qoff.ctypes.data, rbuf.ctypes.data, roff.ctypes.data,
                                           dev.ctypes.data, len(dev), out.ctypes.data, stats.ctypes.data if stats is not None else None)
        else:
            rc = lib.pmx_align_profile_batch_multi(C.byref(cfg), self._profile.inner, n, rbuf.ctypes.data, roff.ctypes.data,
                                                   dev.ctypes.data, len(dev), out.ctypes.data,
                                                   stats.ctypes.data if stats is not None else None)
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        return (out, stats) if stats is not None else out

    def align_batch_banded(self, queries, references, band, diag=None):
        """Banded batch (extension): cells with |(j - i) - diag[k]| > band are excluded; score and end positions."""
        rbuf, roff = pack(references)
        n = len(roff) - 1
        cfg = self._config()
        cfg.want = 0
        out = np.zeros(n, dtype=RECORD_DTYPE)
        d = None if diag is None else np.ascontiguousarray(diag, dtype=np.int32)
        if self._profile.is_null():
            qbuf, qoff = pack(queries)
            rc = lib.pmx_align_batch_banded(C.byref(cfg), None, n, qbuf.ctypes.data, qoff.ctypes.data, rbuf.ctypes.data,
                                            roff.ctypes.data, int(band), d.ctypes.data if d is not None else None, out.ctypes.data)
        else:
            rc = lib.pmx_align_batch_banded(C.byref(cfg), self._profile.inner, n, None, None, rbuf.ctypes.data,
                                            roff.ctypes.data, int(band), d.ctypes.data if d is not None else None, out.ctypes.data)
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        return out

    def align_batch_banded_cigar(self, queries, references, band, diag=None, stats=False):
        """Banded batch with traceback (extension): the records of align_batch_banded, the CIGAR string of each pair's path inside
        the band ("" where the band misses the end cell) and, with stats=True, matches / similar / length along it.
        Returns (records, cigars) or (records, cigars, stats)."""
        rbuf, roff = pack(references)
        n = len(roff) - 1
        cfg = self._config()
        cfg.want = WANT_CIGAR | (WANT_STATS if stats else 0)
        out = np.zeros(n, dtype=RECORD_DTYPE)
        st = np.zeros(n, dtype=STATS_DTYPE) if stats else None
        coff = np.zeros(n + 1, dtype=np.int64)
        d = None if diag is None else np.ascontiguousarray(diag, dtype=np.int32)
        if self._profile.is_null():
            qbuf, qoff = pack(queries)
            if len(qoff) - 1 != n:
                raise BatchError("queries and references differ in count")
            prof, qp, qop = None, qbuf.ctypes.data, qoff.ctypes.data
        else:
            prof, qp, qop = self._profile.inner, None, None
        cbuf = C.c_void_p()
        rc = lib.pmx_align_batch_banded_cigar(C.byref(cfg), prof, n, qp, qop, rbuf.ctypes.data, roff.ctypes.data, int(band),
                                              d.ctypes.data if d is not None else None, out.ctypes.data,
                                              st.ctypes.data if st is not None else None, C.byref(cbuf), coff.ctypes.data)
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        cigars = _take_cigars(cbuf, coff)
        return (out, cigars, st) if stats else (out, cigars)

    def search_profile(self, references, min_score, max_hits=0, order=HITS_BY_INDEX, band=48, stats=False):
        """Profile database search (extension; the aligner needs a profile): the references that score at least min_score -- at most
        the best max_hits of them, 0 = no limit -- in ascending index or by (score descending, index ascending), each with its
        first-pass record and, with band >= 0, a banded second pass around the first pass's diagonal: record, begin of the path,
        CIGAR and (stats=True) matches / similar / length.  band < 0: no second pass (begins -1, no CIGAR).  Selection, the
        compaction of the selected references and the second pass run on the device.  Returns a SearchHits."""
        rbuf, roff = pack(references)
        return self.search_profile_packed(rbuf, roff, min_score, max_hits, order, band, stats)

    def search_profile_packed(self, rbuf, roff, min_score, max_hits=0, order=HITS_BY_INDEX, band=48, stats=False):
        if self._profile.is_null():
            raise NullProfile()
        n = len(roff) - 1
        cfg = self._config()
        cfg.want = (WANT_CIGAR | (WANT_STATS if stats else 0)) if band >= 0 else 0
        opts = pmx_search_opts_t(int(min_score), int(max_hits), int(order), int(band))
        res = C.POINTER(pmx_search_result_t)()
        rc = lib.pmx_search_profile(C.byref(cfg), self._profile.inner, n, rbuf.ctypes.data, roff.ctypes.data, C.byref(opts),
                                    C.byref(res))
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        try:
            return SearchHits(res.contents)
        finally:
            lib.pmx_search_result_free(res)

    def align_batch_cigar_long(self, queries, references, stats=False, cigar=True, tile_cols=0, band_rows=0):
        """Long pairs with traceback in linear memory (extension): the records of align_batch, each pair's CIGAR string and, with
        stats=True, matches / similar / length along the path.  tile_cols / band_rows: 0 = default (never change a result).
        Returns (records, cigars), (records, cigars, stats) or, with cigar=False, (records, stats)."""
        qbuf, qoff = pack(queries)
        rbuf, roff = pack(references)
        n = len(roff) - 1
        if len(qoff) - 1 != n:
            raise BatchError("queries and references differ in count")
        cfg = self._config()
        cfg.want = (WANT_CIGAR if cigar else 0) | (WANT_STATS if stats else 0)
        out = np.zeros(n, dtype=RECORD_DTYPE)
        st = np.zeros(n, dtype=STATS_DTYPE) if stats else None
        coff = np.zeros(n + 1, dtype=np.int64)
        opts = pmx_long_cigar_opts_t(int(tile_cols), int(band_rows))
        cbuf = C.c_void_p()
        rc = lib.pmx_align_batch_cigar_long(C.byref(cfg), n, qbuf.ctypes.data, qoff.ctypes.data, rbuf.ctypes.data, roff.ctypes.data,
                                            out.ctypes.data, st.ctypes.data if st is not None else None,
                                            C.byref(cbuf) if cigar else None, coff.ctypes.data if cigar else None, C.byref(opts))
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        if not cigar:
            return out, st
        cigars = _take_cigars(cbuf, coff)
        return (out, cigars, st) if stats else (out, cigars)

    def align_batch_cigar(self, queries, references):
        qbuf, qoff = pack(queries)
        rbuf, roff = pack(references)
        out, text, coff = self.align_batch_cigar_packed(qbuf, qoff, rbuf, roff)
        raw = text.tobytes()
        return out, [raw[coff[k]:coff[k + 1]].decode() for k in range(len(roff) - 1)]

    def align_batch_cigar_packed(self, qbuf, qoff, rbuf, roff, out=None, coff=None):
        """Packed in, packed out: (records, CIGAR text as one uint8 array, int64 offsets[n+1]).  `out` / `coff`: arrays to fill
        (a caller that aligns batch after batch reuses them; the text block is recycled by the library once its array is gone)."""
        n = len(roff) - 1
        cfg = self._config()
        cfg.want &= ~WANT_STATS
        out = _record_buffer(out, n)
        if coff is None:
            coff = np.zeros(n + 1, dtype=np.int64)
        elif coff.dtype != np.int64 or coff.shape != (n + 1,) or not coff.flags.c_contiguous:
            raise BatchError("coff must be a contiguous int64 array of %d offsets" % (n + 1))
        cbuf = C.c_void_p()
        rc = lib.pmx_align_batch_cigar(C.byref(cfg), n, qbuf.ctypes.data, qoff.ctypes.data, rbuf.ctypes.data,
                                       roff.ctypes.data, out.ctypes.data, C.byref(cbuf), coff.ctypes.data)
        if rc:
            raise BatchError(lib.pmx_last_error().decode())
        # a view of the callee's malloc block (no copy); released with pmx_free when the array goes away
        nbytes = int(coff[n])
        # The owner hangs on the ctypes array, the ULTIMATE base of every numpy view (numpy collapses the base chain of
        # derived arrays down to it: np.asarray(text), text.view(np.ndarray) and slices all keep the block alive).
        raw = (C.c_ubyte * max(nbytes, 1)).from_address(cbuf.value)
        raw._pmx_owner = _OwnedBuffer(cbuf)
        text = np.frombuffer(raw, dtype=np.uint8, count=nbytes)
        return out, text, coff


class SearchHits:
    """Result of Aligner.search_profile: n_hits, n_passing, hits (HIT_DTYPE: index, first, diag, beg_query, beg_ref), recs
    (RECORD_DTYPE of the second pass, None without one), stats (STATS_DTYPE or None), cigar_off (int64 [n_hits + 1]), cigar_text
    (uint8) and cigars (list of str; empty strings without a second pass).  Shortcuts: index, score, end_query, end_ref (of the
    second pass when there is one, else of the first), beg_query, beg_ref."""

    def __init__(self, r):
        h = int(r.n_hits)
        self.n_hits, self.n_passing = h, int(r.n_passing)

        def take(ptr, dtype, count):
            if not ptr or not count:
                return np.zeros(count, dtype=dtype)
            return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).copy()
        self.hits = take(r.hits, HIT_DTYPE, h)
        self.recs = take(r.recs, RECORD_DTYPE, h) if r.recs else None
        self.stats = take(r.stats, STATS_DTYPE, h) if r.stats else None
        self.cigar_off = take(r.cigar_off, np.int64, h + 1)
        self.cigar_text = take(r.cigar, np.uint8, int(self.cigar_off[h])) if r.cigar else np.zeros(0, dtype=np.uint8)
        raw = self.cigar_text.tobytes()
        self.cigars = [raw[self.cigar_off[k]:self.cigar_off[k + 1]].decode() for k in range(h)]
        best = self.recs if self.recs is not None else self.hits["first"]
        self.index = self.hits["index"]
        self.score, self.end_query, self.end_ref = best["score"], best["end_query"], best["end_ref"]
        self.beg_query, self.beg_ref = self.hits["beg_query"], self.hits["beg_ref"]

    def __len__(self):
        return self.n_hits


def _strand_mode(strand):
    """0 / 1 / 2 or "forward" / "reverse" / "both" -> STRAND_*."""
    names = {"forward": STRAND_FORWARD, "reverse": STRAND_REVERSE, "both": STRAND_BOTH}
    if isinstance(strand, str):
        if strand not in names:
            raise BatchError("strand is 0, 1 or \"both\"")
        return names[strand]
    return int(strand)


def _frame_side(frame, ref_frame, stranded, query_entry, ref_entry):
    """frame= / ref_frame= of align_pairs, search_pairs and search_topk -> (the entry that translates that side, the frame argument);
    (None, None) without either."""
    if ref_frame is not None and frame is not None:
        raise BatchError("frame and ref_frame exclude each other: no entry translates both sides")
    if ref_frame is not None and stranded:
        raise BatchError("ref_frame and strand exclude each other: a strand is the query's, and the query is protein")
    if frame is not None and stranded:
        raise BatchError("frame and strand exclude each other: a reverse frame is the reverse strand translated")
    if ref_frame is not None:
        return ref_entry, ref_frame
    return (query_entry, frame) if frame is not None else (None, None)


def _frameshift_side(frame, ref_frame):
    """frameshift= of align_pairs, search_pairs and search_topk excludes the two frame arguments."""
    if frame is not None or ref_frame is not None:
        raise BatchError("frameshift excludes frame and ref_frame: the three-frame alignment reads every frame of a strand at once")


def _ref_frameshift_side(ref_frameshift, ref_strand, frame, ref_frame, frameshift, stranded, cigar):
    """ref_frameshift= / ref_strand= of align_pairs, search_pairs and search_topk: True when the reference-side three-frame
    alignment is asked for, after what it excludes."""
    if ref_frameshift is None:
        if ref_strand is not None:
            raise BatchError("ref_strand belongs to ref_frameshift: the reference has a strand only where it is the nucleotide side")
        return False
    if frame is not None or ref_frame is not None:
        raise BatchError("ref_frameshift excludes frame and ref_frame: the three-frame alignment reads every frame of a strand at once")
    if frameshift is not None:
        raise BatchError("ref_frameshift and frameshift exclude each other: no entry translates both sides")
    if stranded:
        raise BatchError("ref_frameshift and strand exclude each other: a strand is the query's, and the query is protein; ref_strand is the reference's")
    if cigar:
        raise BatchError("ref_frameshift excludes cigar: the reference side has no traceback with frameshift operators yet")
    return True


def _frame_mode(frame, n=None):
    """A frame argument -> (frame mode, frame bytes per pair or None): 0 .. 5, FRAMES_* or "forward" / "reverse" / "all"; with n
    (align_pairs) also one frame byte per pair."""
    names = {"forward": FRAMES_FORWARD, "reverse": FRAMES_REVERSE, "all": FRAMES_ALL}
    if isinstance(frame, str):
        if frame not in names:
            raise BatchError("frame is 0 .. 5, \"forward\", \"reverse\" or \"all\"")
        return names[frame], None
    if np.ndim(frame) == 0:
        return int(frame), None
    if n is None:
        raise BatchError("a frame byte per pair is for align_pairs: a search takes one frame mode")
    per_pair = np.ascontiguousarray(frame, dtype=np.uint8)
    if len(per_pair) != n:
        raise BatchError("frame and pairs differ in count")
    return 0, per_pair


def _code_arg(code):
    """A caller's genetic code (64 letters in NCBI order) as a uint8 array, or None for the standard one."""
    if code is None:
        return None
    code = np.frombuffer(code.encode() if isinstance(code, str) else bytes(code), dtype=np.uint8).copy()
    if len(code) != 64:
        raise BatchError("a genetic code has 64 letters, not %d" % len(code))
    return code


def genetic_code_table():
    """The standard genetic code (NCBI table 1) in NCBI order: 64 bytes, index 16 b0 + 4 b1 + b2 with T = 0, C = 1, A = 2, G = 3."""
    tab = np.zeros(64, dtype=np.uint8)
    lib.pmx_genetic_code_table(tab.ctypes.data)
    return tab.tobytes()


def translate(seq, frame, code=None):
    """The translation of a nucleotide window as the _translated entries define it, on the host: frame 0 .. 2 reads `seq` from offset
    frame, frame 3 .. 5 its reverse complement (complement_table(), then reversed) from offset frame - 3; (len - offset) // 3 letters;
    a codon with a byte outside ACGTUacgtu is X.  b"" when the frame does not exist."""
    frame = int(frame)
    if not 0 <= frame <= 5:
        raise BatchError("frame %d is outside 0 .. 5" % frame)
    code = genetic_code_table() if code is None else _code_arg(code).tobytes()
    s = np.frombuffer(bytes(seq), dtype=np.uint8)
    if frame >= 3:
        s = complement_table()[s[::-1]]
    off = frame % 3
    cls = {ord(c): v for c, v in zip("TCAGUtcagu", (0, 1, 2, 3, 0) * 2)}
    out = bytearray()
    for p in range(max(len(s) - off, 0) // 3):
        b = [cls.get(int(x), 64) for x in s[off + 3 * p: off + 3 * p + 3]]
        out.append(code[16 * b[0] + 4 * b[1] + b[2]] if max(b) < 64 else ord("X"))
    return bytes(out)


def codon_stream(seq, strand=0, code=None):
    """The codon stream of a nucleotide window as the _frameshift entries define it, on the host: `seq` as stored (strand 0) or its
    reverse complement (strand 1: complement_table(), then reversed); letter i is the translation of oriented bytes i, i + 1, i + 2,
    len - 2 letters, so codon_stream(seq, s)[f::3] == translate(seq, 3 * s + f).  b"" for fewer than three bytes."""
    strand = int(strand)
    if strand not in (0, 1):
        raise BatchError("strand %d is neither 0 nor 1" % strand)
    code = genetic_code_table() if code is None else _code_arg(code).tobytes()
    s = np.frombuffer(bytes(seq), dtype=np.uint8)
    if strand:
        s = complement_table()[s[::-1]]
    cls = np.full(256, 64, dtype=np.int64)
    for c, v in zip(b"TCAGUtcagu", (0, 1, 2, 3, 0) * 2):
        cls[c] = v
    if len(s) < 3:
        return b""
    b = cls[s]
    idx = 16 * b[:-2] + 4 * b[1:-1] + b[2:]
    lut = np.frombuffer(bytes(code), dtype=np.uint8)
    return np.where(idx < 64, lut[np.minimum(idx, 63)], ord("X")).astype(np.uint8).tobytes()


def frameshift_ref_max_query():
    """The longest query window, in letters, the _frameshift_ref entries take (PMX_FRAMESHIFT_REF_MAX_QUERY of the library)."""
    return int(lib.pmx_frameshift_ref_max_query())


def frameshift_max_window():
    """The longest query window, in nucleotides, the _frameshift entries take (PMX_FRAMESHIFT_MAX_WINDOW of the library)."""
    return int(lib.pmx_frameshift_max_window())


def _hits_call(entry, args, block_t, wrap, free):
    """entry(*args, &block) of the host search entries: BatchError on failure, else wrap(block) with the block released."""
    res = C.POINTER(block_t)()
    if entry(*args, C.byref(res)):
        raise BatchError(lib.pmx_last_error().decode())
    try:
        return wrap(res.contents)
    finally:
        free(res)


class PairHits:
    """Result of Aligner.search_pairs: n_hits, n_passing (all pairs at or above min_score, stored or not) and, per hit in
    enumeration order, pairs (PAIR_DTYPE: the descriptor, fit for align_pairs), index (int64: the pair's number in the
    enumeration), records (RECORD_DTYPE), stats (STATS_DTYPE, or None when not asked for), strand (uint8: the strand of the
    record, all 0 for a forward search) and frame (uint8: the frame of the record of a translated search, else all 0)."""

    def __init__(self, r):
        h = int(r.n_hits)
        self.n_hits, self.n_passing = h, int(r.n_passing)

        def take(ptr, dtype):
            if not ptr or not h:
                return np.zeros(h, dtype=dtype)
            return np.frombuffer(C.string_at(ptr, h * np.dtype(dtype).itemsize), dtype=dtype).copy()
        self.pairs = take(r.pairs, PAIR_DTYPE)
        self.index = take(r.index, np.int64)
        self.records = take(r.recs, RECORD_DTYPE)
        self.stats = take(r.stats, STATS_DTYPE) if r.stats else None
        self.strand = take(getattr(r, "strand", None), np.uint8)
        self.frame = take(getattr(r, "frame", None), np.uint8)

    def __len__(self):
        return self.n_hits


class TopKHits:
    """Result of Aligner.search_topk, CSR by query row: row_off (int64, n_rows + 1), row_passing (int64: the references at or above
    min_score per row, kept or not), n_passing (their sum) and, per hit, pairs (PAIR_DTYPE: the descriptor, fit for align_pairs),
    index (int64: p = i * len(R) + j), records (RECORD_DTYPE) and stats (STATS_DTYPE, or None when not asked for).  A row's hits
    are in (score descending, reference index ascending) order; row(i) slices them out.  strand (uint8 per hit): the strand of the
    record, all 0 for a forward search; frame (uint8 per hit): the frame of the record of a translated search, else all 0."""

    def __init__(self, r):
        h, n = int(r.n_hits), int(r.n_rows)
        self.n_rows, self.n_hits, self.n_passing = n, h, int(r.n_passing)

        def take(ptr, count, dtype):
            if not ptr or not count:
                return np.zeros(count, dtype=dtype)
            return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).copy()
        self.row_off = take(r.row_off, n + 1, np.int64)
        self.row_passing = take(r.row_passing, n, np.int64)
        self.pairs = take(r.pairs, h, PAIR_DTYPE)
        self.index = take(r.index, h, np.int64)
        self.records = take(r.recs, h, RECORD_DTYPE)
        self.stats = take(r.stats, h, STATS_DTYPE) if r.stats else None
        self.strand = take(getattr(r, "strand", None), h, np.uint8)
        self.frame = take(getattr(r, "frame", None), h, np.uint8)

    def __len__(self):
        return self.n_hits

    def row(self, i):
        """(pairs, index, records, stats) of local row i (0 = first_row)."""
        a, b = int(self.row_off[i]), int(self.row_off[i + 1])
        return self.pairs[a:b], self.index[a:b], self.records[a:b], (self.stats[a:b] if self.stats is not None else None)


def _take_cigars(cbuf, coff):
    """The per-pair CIGAR strings out of a callee-allocated text block (offsets coff[n + 1]); the block is released."""
    n = len(coff) - 1
    try:
        raw = C.string_at(cbuf.value, int(coff[n])) if cbuf.value and coff[n] else b""
    finally:
        if cbuf.value:
            lib.pmx_free(cbuf)
    return [raw[coff[k]:coff[k + 1]].decode() for k in range(n)]


class _OwnedBuffer:
    """Keeps a callee-allocated block alive for numpy views of it; pmx_free on collection."""

    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            if self.ptr:
                lib.pmx_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def pack(seqs):
    """list of bytes -> (uint8 buffer, int64 offsets[n+1]) in the layout of include/parasail_amd.h."""
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    buf = np.frombuffer(b"".join(bytes(s) for s in seqs), dtype=np.uint8).copy()
    if len(buf) == 0:
        buf = np.zeros(1, dtype=np.uint8)
    return buf, off


class SeqSet:
    """A set of sequences resident on the device current at its creation (pmx_seqset_t).  Released by close() or on deletion."""

    def __init__(self, inner, keep=None):
        self.inner = inner
        self._keep = keep                     # wrapped sets: whatever owns the device buffers

    @classmethod
    def new(cls, seqs):
        buf, off = pack(seqs)
        return cls.packed(buf, off)

    @classmethod
    def packed(cls, buf, off):
        """Sequence k is buf[off[k]:off[k + 1]] (uint8 buffer, int64 offsets): uploaded once."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        if len(off) < 1:
            raise BatchError("offsets need count + 1 entries")
        inner = lib.pmx_seqset_create(buf.ctypes.data, off.ctypes.data, len(off) - 1)
        if not inner:
            raise BatchError(lib.pmx_last_error().decode())
        return cls(inner)

    @classmethod
    def wrap_device(cls, d_buf, d_off, count, nbytes, keep=None):
        """No copy: raw device addresses of the caller's buffer (`nbytes` bytes) and offsets (count + 1 int64), which must
        outlive the set; `keep` is held for that purpose (e.g. the torch tensors)."""
        inner = lib.pmx_seqset_wrap_device(d_buf, d_off, int(count), int(nbytes))
        if not inner:
            raise BatchError(lib.pmx_last_error().decode())
        return cls(inner, keep)

    def _handle(self):
        if not self.inner:
            raise BatchError("the sequence set is closed")
        return self.inner

    def __len__(self):
        return int(lib.pmx_seqset_count(self._handle()))

    def close(self):
        if self.inner:
            lib.pmx_seqset_free(self.inner)
            self.inner = None
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SEED_ALPHABET_AA20, SEED_ALPHABET_AA11 = 0, 1
SEED_QUERY_LETTERS, SEED_CODONS_FORWARD, SEED_CODONS_REVERSE, SEED_CODONS_BOTH = -1, 9, 10, 11
SEED_REF_FRAMES, SEED_REF_CODONS = 0, 1


def seed_alphabet(which):
    """A built-in reduced alphabet as the 256-byte table a letters index takes (uint8 [256]: group per byte, 255 = invalid):
    "aa20" / SEED_ALPHABET_AA20, the twenty amino acids, or "aa11" / SEED_ALPHABET_AA11, eleven groups of them."""
    if isinstance(which, str):
        names = {"aa20": SEED_ALPHABET_AA20, "aa11": SEED_ALPHABET_AA11}
        if which not in names:
            raise BatchError("alphabet is \"aa20\", \"aa11\" or a table of 256 bytes")
        which = names[which]
    tab = np.zeros(256, dtype=np.uint8)
    if lib.pmx_seed_alphabet(int(which), tab.ctypes.data):
        raise BatchError(lib.pmx_last_error().decode())
    return tab


class SeedIndex:
    """The k-mer index of a set (pmx_seed_index_t): every k-mer of R as (kmer, seq, pos), sorted, on R's device -- of a DNA set, or
    with `alphabet` of a protein set over a reduced alphabet (a letters index; .letters, .bits per letter), or with `alphabet` and
    `translated` of a nucleotide set read in the three frames of the strands named (a translated index; .translated, .strands: the
    strand mode it holds, else None).  A DNA index built with w > 1 holds the (w, k) minimizers of R only (.w: the window, 1 of every
    other index); seed_pairs reads w from the index.  .nbytes: the device bytes the index owns.  R is held: it outlives the index.
    len(): the entries.  Released by close() or on deletion."""

    def __init__(self, inner, R, k, letters=False, strands=None):
        self.inner, self.R, self.k, self.letters = inner, R, int(k), bool(letters)
        self.translated, self.strands = strands is not None, strands

    @classmethod
    def build(cls, R, k, alphabet=None, stream=0, translated=None, code=None, w=1):
        """alphabet: None (a DNA index), "aa20", "aa11" or 256 bytes that map a byte to its group 0 .. 31 or to 255.  An integer in
        its place is the stream of a DNA index, build(R, k, stream), as before there were alphabets.  translated: "forward",
        "reverse" or "both" -- R holds nucleotides and the index their six-frame (or three-frame) k-mers over `alphabet`, for
        seed_pairs(ref_frames=); code: 64 letters that replace the standard genetic code of a translated index.  w: 1 .. 64, the
        window of a DNA index -- with w > 1 the index holds minimizers only; the letters and translated builds take no w."""
        if isinstance(alphabet, (int, np.integer)) and not isinstance(alphabet, bool):
            alphabet, stream = None, int(alphabet)
        if int(w) != 1 and alphabet is not None:
            raise BatchError("w= is for a DNA index: a letters or translated index (alphabet=) holds every k-mer")
        if translated is not None and alphabet is None:
            raise BatchError("translated= needs alphabet=: a translated index holds letters of a reduced alphabet")
        if code is not None and translated is None:
            raise BatchError("code= is for a translated index (translated=)")
        if alphabet is None and int(w) != 1:
            inner = lib.pmx_seed_index_build_minimizers(R._handle(), int(k), int(w), stream)
        elif alphabet is None:
            inner = lib.pmx_seed_index_build(R._handle(), int(k), stream)
        else:
            if isinstance(alphabet, str):
                table = seed_alphabet(alphabet)
            else:
                table = np.ascontiguousarray(np.frombuffer(alphabet, dtype=np.uint8) if isinstance(alphabet, (bytes, bytearray)) else alphabet,
                                             dtype=np.uint8)
                if table.shape != (256,):
                    raise BatchError("alphabet is \"aa20\", \"aa11\" or a table of 256 bytes")
            if translated is not None:
                if translated not in ("forward", "reverse", "both"):
                    raise BatchError("translated is \"forward\", \"reverse\" or \"both\"")
                code = _code_arg(code)
                inner = lib.pmx_seed_index_build_translated(R._handle(), int(k), table.ctypes.data, code.ctypes.data if code is not None else None,
                                                            _strand_mode(translated), stream)
            else:
                inner = lib.pmx_seed_index_build_letters(R._handle(), int(k), table.ctypes.data, stream)
        if not inner:
            raise BatchError(lib.pmx_last_error().decode())
        return cls(inner, R, k, alphabet is not None and translated is None, translated)

    @property
    def bits(self):
        return int(lib.pmx_seed_index_bits(self._handle()))

    @property
    def w(self):
        return int(lib.pmx_seed_index_window(self._handle()))

    @property
    def nbytes(self):
        return int(lib.pmx_seed_index_bytes(self._handle()))

    def _handle(self):
        if not self.inner:
            raise BatchError("the seed index is closed")
        return self.inner

    def __len__(self):
        return int(lib.pmx_seed_index_count(self._handle()))

    def close(self):
        if self.inner:
            lib.pmx_seed_index_free(self.inner)
            self.inner = None
            self.R = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SeedHits:
    """Result of seed_pairs, CSR by query row: row_off (int64, n_rows + 1, never capped by max_hits), n_passing (the candidates)
    and, per stored candidate, pairs (PAIR_DTYPE: query, reference and reference window, fit for Aligner.align_pairs), strand
    (uint8) and seeds (SEED_HIT_DTYPE: matches and the diagonals' range).  A row's candidates are in (strand, reference,
    diag_min) order; row(i) slices out those that were stored.  Of a letters index (seed_pairs(frames=)) the byte per candidate
    is a frame in the frame modes -- .frame holds it, else .frame is None -- and a strand in the codon modes -- .strand holds it;
    .strand is zeros in the letters and frame modes.  Of a translated index (seed_pairs(ref_frames=)) .frame holds the byte with
    "frames" (0 or 3, relative to the window; seeds["reserved"] is the sequence frame) and .strand holds it with "codons".
    kind says which list this is: "strand" (a DNA index), "letters", "frame" or "codons" (a letters index), "ref_frames" or
    "ref_codons" (a translated index); seed_filter and seed_filter_translated read it.  A list that either returns has .ungapped (UNGAPPED_DTYPE) and
    .source (int64: the candidate's index in the list that was filtered) as well; the list of seed_chains has .chains
    (SEED_CHAIN_DTYPE, one record per stored candidate)."""

    def __init__(self, r, byte_is_frame=False, kind=None):
        self.kind = kind
        h, n = int(r.n_hits), int(r.n_rows)
        self.n_rows, self.n_hits, self.n_passing = n, h, int(r.n_passing)

        def take(ptr, count, dtype):
            if not ptr or not count:
                return np.zeros(count, dtype=dtype)
            return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).copy()
        self.row_off = take(r.row_off, n + 1, np.int64)
        self.pairs = take(r.pairs, h, PAIR_DTYPE)
        self.strand = take(r.strand, h, np.uint8)
        self.seeds = take(r.seeds, h, SEED_HIT_DTYPE)
        self.frame = None
        if byte_is_frame:
            self.frame, self.strand = self.strand, np.zeros(h, dtype=np.uint8)

    def __len__(self):
        return self.n_hits

    def row(self, i):
        """(pairs, strand, seeds) of local row i (0 = first_row)."""
        a, b = min(int(self.row_off[i]), self.n_hits), min(int(self.row_off[i + 1]), self.n_hits)
        return self.pairs[a:b], self.strand[a:b], self.seeds[a:b]


def _seed_opts(strand, min_seeds, band, pad, max_occ, max_hits=0, slice_rows=0):
    return pmx_seed_opts_t(_strand_mode(strand), int(min_seeds), int(band), int(pad), int(max_occ), 0, int(max_hits), int(slice_rows))


def _seed_ref_mode(index, ref_frames, frames, strand, code):
    """ref_frames= of seed_pairs -> the ref_mode of a translated index (None: another index, which does not take it)."""
    if not getattr(index, "translated", False):
        if ref_frames is not None:
            raise BatchError("ref_frames= is for a translated index (SeedIndex.build(alphabet=, translated=))")
        return None
    if strand is not None or frames is not None:
        raise BatchError("a translated index holds the strands it was built with and takes ref_frames= (\"frames\" or \"codons\"), "
                         "not strand= or frames=")
    if code is not None:
        raise BatchError("code= belongs to the build of a translated index; its queries are proteins")
    names = {"frames": SEED_REF_FRAMES, "codons": SEED_REF_CODONS}
    if ref_frames not in names:
        raise BatchError("a translated index needs ref_frames=: \"frames\" or \"codons\"")
    return names[ref_frames]


def _seed_query_mode(index, frames, strand):
    """frames= of seed_pairs -> the query mode of a letters index (None: a DNA index, which takes strand= instead)."""
    if not index.letters:
        if frames is not None:
            raise BatchError("frames= is for a letters index (SeedIndex.build(alphabet=)); a DNA index takes strand=")
        return None
    if frames is None:
        raise BatchError("a letters index needs frames=: \"letters\", a frame 0 .. 5, \"forward\", \"reverse\", \"all\", \"codons\", "
                         "\"codons-reverse\" or \"codons-both\"")
    if strand is not None:
        raise BatchError("strand= is for a DNA index; frames= chooses the orientations of a letters index")
    names = {"letters": SEED_QUERY_LETTERS, "forward": FRAMES_FORWARD, "reverse": FRAMES_REVERSE, "all": FRAMES_ALL,
             "codons": SEED_CODONS_FORWARD, "codons-reverse": SEED_CODONS_REVERSE, "codons-both": SEED_CODONS_BOTH}
    if isinstance(frames, str):
        if frames not in names:
            raise BatchError("frames is \"letters\", 0 .. 5, \"forward\", \"reverse\", \"all\", \"codons\", \"codons-reverse\" or \"codons-both\"")
        return names[frames]
    if isinstance(frames, (bool, np.bool_)) or not 0 <= int(frames) <= 5:
        raise BatchError("frames is \"letters\", 0 .. 5, \"forward\", \"reverse\", \"all\", \"codons\", \"codons-reverse\" or \"codons-both\"")
    return int(frames)


def _seed_entry(index, strand, frames, code, ref_frames, min_seeds, band, pad, max_occ, max_hits, slice_rows):
    """What seed_pairs and seed_pairs_device call for this index and these arguments: (the host entry, the device entry, opts, the
    entry's own arguments behind opts, byte_is_frame, what those arguments point into)."""
    ref_mode = _seed_ref_mode(index, ref_frames, frames, strand, code)
    if ref_mode is not None:
        opts = _seed_opts(0, min_seeds, band, pad, max_occ, max_hits, slice_rows)
        return lib.pmx_seed_pairs_translated_ref, lib.pmx_seed_pairs_translated_ref_device, opts, (ref_mode,), ref_mode == SEED_REF_FRAMES, None
    mode = _seed_query_mode(index, frames, strand)
    opts = _seed_opts(0 if mode is not None else "both" if strand is None else strand, min_seeds, band, pad, max_occ, max_hits, slice_rows)
    if mode is None:
        if code is not None:
            raise BatchError("code= is for a letters index")
        return lib.pmx_seed_pairs, lib.pmx_seed_pairs_device, opts, (), False, None
    code = _code_arg(code)
    extra = (mode, code.ctypes.data if code is not None else None)
    return lib.pmx_seed_pairs_letters, lib.pmx_seed_pairs_letters_device, opts, extra, 0 <= mode <= FRAMES_ALL, code


def _seed_kind(index, frames, ref_frames):
    """The SeedHits.kind of a seed_pairs call whose arguments _seed_entry has accepted."""
    if getattr(index, "translated", False):
        return "ref_frames" if ref_frames == "frames" else "ref_codons"
    if not index.letters:
        return "strand"
    if isinstance(frames, str) and frames.startswith("codons"):
        return "codons"
    return "letters" if isinstance(frames, str) and frames == "letters" else "frame"


def seed_pairs(Q, index, strand=None, min_seeds=2, band=8, pad=16, max_occ=64, first_row=0, rows=None, max_hits=0, slice_rows=0,
               frames=None, code=None, ref_frames=None):
    """Candidate windows of the queries Q[first_row : first_row + rows] in the indexed reference: exact k-mer matches, clustered
    by diagonal (consecutive diagonals at most `band` apart), clusters of at least min_seeds matches widened by `pad`.
    hits.pairs and hits.strand go unchanged into Aligner.align_pairs(Q, R, pairs, strand=, cigar=True)  (strand: "both" unless given).
    With a letters index `frames` says what Q holds: "letters" (proteins in the index's alphabet), a frame 0 .. 5, "forward", "reverse"
    or "all" (nucleotides, candidates per frame: align_pairs(Q, R, hits.pairs, frame=hits.frame)), "codons", "codons-reverse" or
    "codons-both" (nucleotides, candidates per strand over its three frames, diagonals and band in nucleotides:
    align_pairs(Q, R, hits.pairs, frameshift=fs, strand=hits.strand)); code: 64 letters that replace the standard genetic code.
    With a translated index Q holds proteins and `ref_frames` chooses the candidates: "frames" (per sequence frame, letter diagonals:
    align_pairs(Q, R, hits.pairs, ref_frame=hits.frame)) or "codons" (per strand over its three frames, diagonals, band and pad in
    nucleotides: align_pairs(Q, R, hits.pairs, ref_frameshift=fs, ref_strand=hits.strand) and the frameshift_ref_cigar entries)."""
    if rows is None:
        rows = max(0, len(Q) - int(first_row))
    host, _, opts, extra, byte_is_frame, _keep = _seed_entry(index, strand, frames, code, ref_frames, min_seeds, band, pad, max_occ, max_hits, slice_rows)
    res = C.POINTER(pmx_seed_hits_t)()
    if host(Q._handle(), index._handle(), int(first_row), int(rows), C.byref(opts), *extra, C.byref(res)):
        raise BatchError(lib.pmx_last_error().decode())
    try:
        return SeedHits(res.contents, byte_is_frame=byte_is_frame, kind=_seed_kind(index, frames, ref_frames))
    finally:
        lib.pmx_seed_hits_free(res)


def seed_pairs_device(Q, index, q_first, nq, max_qlen, d_hit_pairs, d_hit_strand, d_hit_seeds, capacity, d_row_off, d_counts,
                      strand=None, min_seeds=2, band=8, pad=16, max_occ=64, slice_rows=0, stream=0, frames=None, code=None, ref_frames=None):
    """Device-pointer entry of seed_pairs: the candidates go to d_hit_pairs / d_hit_strand / d_hit_seeds (optional), `capacity`
    entries each, d_row_off gets nq + 1 offsets and d_counts [candidates, written].  Synchronises `stream` once per slice.  With a
    letters index (frames=) d_hit_strand receives the frame or strand byte and max_qlen bounds the letters of a translation; with a
    translated index (ref_frames=) it receives the window's frame byte or the strand and max_qlen bounds the letters of a protein."""
    _, device, opts, extra, _, _keep = _seed_entry(index, strand, frames, code, ref_frames, min_seeds, band, pad, max_occ, 0, slice_rows)
    if device(Q._handle(), index._handle(), int(q_first), int(nq), int(max_qlen), C.byref(opts), *extra, d_hit_pairs, d_hit_strand, d_hit_seeds,
              int(capacity), d_row_off, d_counts, stream):
        raise BatchError(lib.pmx_last_error().decode())


def _seed_chain_opts(max_gap, lookback, gap_scale, min_score):
    return pmx_seed_chain_opts_t(int(max_gap), int(lookback), int(gap_scale), int(min_score), (C.c_int32 * 4)(0, 0, 0, 0))


def seed_chains(Q, index, strand=None, min_seeds=2, min_score=0, band=500, max_gap=5000, lookback=64, gap_scale=38, pad=16, max_occ=64,
                first_row=0, rows=None, max_hits=0, slice_rows=0):
    """Candidate windows of the queries Q[first_row : first_row + rows] by collinear chaining (include/parasail_amd.h, "Seed chaining"):
    the matches of a (row, strand, reference) in (j, i) order, linked where both steps are 1 .. max_gap, their difference is at most
    `band` and the predecessor is among the `lookback` anchors before; a link costs (g * gap_scale >> 8) + (bit length of g >> 1) for a
    diagonal change g.  A chain of at least min_seeds anchors and a score of at least min_score is a candidate.  Takes a DNA index
    (stride 1 or minimizers).  Returns a SeedHits of kind "strand" -- seed_filter and Aligner.align_pairs(Q, R, hits.pairs,
    strand=hits.strand) take it as it is -- with .chains (SEED_CHAIN_DTYPE) added: score, n_anchors and the chain's extent on the
    oriented query [q_beg, q_end) and the reference [r_beg, r_end).  strand: "both" unless given."""
    if rows is None:
        rows = max(0, len(Q) - int(first_row))
    opts = _seed_opts("both" if strand is None else strand, min_seeds, band, pad, max_occ, max_hits, slice_rows)
    copts = _seed_chain_opts(max_gap, lookback, gap_scale, min_score)
    res = C.POINTER(pmx_seed_chained_t)()
    if lib.pmx_seed_chains(Q._handle(), index._handle(), int(first_row), int(rows), C.byref(opts), C.byref(copts), C.byref(res)):
        raise BatchError(lib.pmx_last_error().decode())
    try:
        hits = SeedHits(res.contents.hits, kind="strand")
        ptr, n = res.contents.chains, hits.n_hits
        hits.chains = (np.frombuffer(C.string_at(ptr, n * SEED_CHAIN_DTYPE.itemsize), dtype=SEED_CHAIN_DTYPE).copy() if ptr and n
                       else np.zeros(n, dtype=SEED_CHAIN_DTYPE))
        return hits
    finally:
        lib.pmx_seed_chained_free(res)


def seed_chains_device(Q, index, q_first, nq, max_qlen, d_hit_pairs, d_hit_strand, d_hit_seeds, d_hit_chains, capacity, d_row_off, d_counts,
                       strand=None, min_seeds=2, min_score=0, band=500, max_gap=5000, lookback=64, gap_scale=38, pad=16, max_occ=64,
                       slice_rows=0, stream=0):
    """Device-pointer entry of seed_chains, as seed_pairs_device: the candidates go to d_hit_pairs / d_hit_strand / d_hit_seeds
    (optional) / d_hit_chains (optional), `capacity` entries each, d_row_off gets nq + 1 offsets and d_counts [candidates, written].
    Synchronises `stream` once per slice."""
    opts = _seed_opts("both" if strand is None else strand, min_seeds, band, pad, max_occ, 0, slice_rows)
    copts = _seed_chain_opts(max_gap, lookback, gap_scale, min_score)
    if lib.pmx_seed_chains_device(Q._handle(), index._handle(), int(q_first), int(nq), int(max_qlen), C.byref(opts), C.byref(copts), d_hit_pairs,
                                  d_hit_strand, d_hit_seeds, d_hit_chains, int(capacity), d_row_off, d_counts, stream):
        raise BatchError(lib.pmx_last_error().decode())


def seed_chain_shape():
    """(lanes that evaluate predecessors at once, the most anchors the ring holds = the largest lookback) of the chain kernel (test hook)."""
    a, b = C.c_int32(), C.c_int32()
    lib.pmx_seed_chain_shape(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def ungapped_shape():
    """(lanes per candidate, cells per lane step) of the ungapped filter's kernel (test hook)."""
    g, st = C.c_int32(), C.c_int32()
    lib.pmx_seed_ungapped_shape(C.byref(g), C.byref(st))
    return int(g.value), int(st.value)


def _ungapped_config(matrix):
    """The configuration the ungapped entries read: the matrix, nothing else."""
    if not isinstance(matrix, Matrix):
        raise BatchError("matrix: a Matrix")
    return pmx_config_t(MODE_SW, 0, 0, 0, 0, 0, matrix.inner)


def _ungapped_kind(kind):
    if kind not in ("strand", "frame"):
        raise BatchError("kind is \"strand\" or \"frame\"")
    return SEED_BYTE_FRAME if kind == "frame" else SEED_BYTE_STRAND


def _ungapped_list_kind(kind):
    names = {"codons": SEED_LIST_CODONS, "ref_frames": SEED_LIST_REF_FRAMES, "ref_codons": SEED_LIST_REF_CODONS}
    if kind not in names:
        raise BatchError("kind is \"codons\", \"ref_frames\" or \"ref_codons\"")
    return names[kind]


def seed_ungapped(Q, R, pairs, byte, seeds, matrix, kind="strand", code=None, chunk_pairs=0):
    """The ungapped score of listed candidates (UNGAPPED_DTYPE: score, diag, end_query, end_ref): the best run of matches and
    mismatches under `matrix` along the diagonals seeds["diag_min"] .. seeds["diag_max"] of each pair's windows.  byte: a strand
    per candidate (kind "strand"; None: all forward) or a frame 0 .. 5 of the query (kind "frame", with code).  A candidate
    without a positive cell gets (0, diag_min, -1, -1), a bad one (-1, 0, -1, -1)."""
    return _seed_ungapped(lib.pmx_seed_ungapped, _ungapped_kind(kind), Q, R, pairs, byte, seeds, matrix, code, chunk_pairs)


def seed_ungapped_translated(Q, R, pairs, byte, seeds, matrix, kind, code=None, chunk_pairs=0):
    """seed_ungapped for the lists whose diagonals are not letter diagonals of one query frame.  kind "codons": Q nucleotides, R
    proteins, byte a strand of the query, nucleotide diagonals D = 3 j - n over the query's codon stream, record (U, D, last
    nucleotide of the codon in the oriented window, j).  kind "ref_frames": Q proteins, R nucleotides, byte the window's frame (0
    or 3), seeds["reserved"] the sequence frame, letter diagonals of that frame's whole translation.  kind "ref_codons": byte a
    strand of the reference, nucleotide diagonals D = x - 3 p in oriented whole-sequence coordinates, record (U, D, p, x + 2).
    code: 64 letters that replace the standard genetic code."""
    return _seed_ungapped(lib.pmx_seed_ungapped_translated, _ungapped_list_kind(kind), Q, R, pairs, byte, seeds, matrix, code, chunk_pairs)


def _seed_ungapped(entry, bk, Q, R, pairs, byte, seeds, matrix, code, chunk_pairs):
    cfg = _ungapped_config(matrix)
    pairs = as_pairs(pairs)
    n = len(pairs)
    seeds = np.ascontiguousarray(seeds, dtype=SEED_HIT_DTYPE)
    if len(seeds) != n:
        raise BatchError("seeds and pairs differ in count")
    if byte is not None:
        byte = np.ascontiguousarray(byte, dtype=np.uint8)
        if len(byte) != n:
            raise BatchError("byte and pairs differ in count")
    code = _code_arg(code)
    out = np.zeros(n, dtype=UNGAPPED_DTYPE)
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    if entry(C.byref(cfg), Q._handle(), R._handle(), n, pairs.ctypes.data, byte.ctypes.data if byte is not None else None, bk,
             code.ctypes.data if code is not None else None, seeds.ctypes.data, out.ctypes.data, C.byref(opts)):
        raise BatchError(lib.pmx_last_error().decode())
    return out


def seed_ungapped_device(Q, R, n, d_pairs, d_byte, d_seeds, max_qlen, max_rlen, matrix, d_out, kind="strand", code=None, stream=0, chunk_pairs=0):
    """Device-pointer entry of seed_ungapped: n records into d_out; asynchronous on `stream`."""
    _seed_ungapped_device(lib.pmx_seed_ungapped_device, _ungapped_kind(kind), Q, R, n, d_pairs, d_byte, d_seeds, max_qlen, max_rlen, matrix, d_out,
                          code, stream, chunk_pairs)


def seed_ungapped_translated_device(Q, R, n, d_pairs, d_byte, d_seeds, max_qlen, max_rlen, matrix, d_out, kind, code=None, stream=0, chunk_pairs=0):
    """Device-pointer entry of seed_ungapped_translated: n records into d_out; asynchronous on `stream`.  max_qlen / max_rlen bound
    what the kind's gather bounds: on a codon side the stream's W - 2 letters."""
    _seed_ungapped_device(lib.pmx_seed_ungapped_translated_device, _ungapped_list_kind(kind), Q, R, n, d_pairs, d_byte, d_seeds, max_qlen, max_rlen,
                          matrix, d_out, code, stream, chunk_pairs)


def _seed_ungapped_device(entry, bk, Q, R, n, d_pairs, d_byte, d_seeds, max_qlen, max_rlen, matrix, d_out, code, stream, chunk_pairs):
    cfg = _ungapped_config(matrix)
    code = _code_arg(code)
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    if entry(C.byref(cfg), Q._handle(), R._handle(), int(n), d_pairs, d_byte, bk, code.ctypes.data if code is not None else None, d_seeds,
             int(max_qlen), int(max_rlen), d_out, stream, C.byref(opts)):
        raise BatchError(lib.pmx_last_error().decode())


_SEED_FILTER_KINDS = {"strand": "strand", "letters": "strand", "frame": "frame"}


def seed_filter(Q, R, hits, matrix, min_score=0, top_n=0, code=None, chunk_pairs=0):
    """The candidates of a seed_pairs result that are worth a gapped extension: every candidate gets its ungapped score
    (seed_ungapped), one below max(min_score, 0) is dropped, and with top_n > 0 only the top_n best of a query row stay (score
    descending, then position).  Returns a SeedHits of the kept candidates in their input order -- pairs / strand / frame go into
    Aligner.align_pairs as those of `hits` would -- with .ungapped and .source added.  hits.kind chooses the byte's meaning; the
    lists of the codon modes and of a translated index ("codons", "ref_frames", "ref_codons") are refused: they go to
    seed_filter_translated."""
    kind = hits.kind if getattr(hits, "kind", None) is not None else ("frame" if hits.frame is not None else "strand")
    if kind not in _SEED_FILTER_KINDS:
        raise BatchError("seed_filter does not take a list of kind \"%s\": its diagonals are not letter diagonals of one query frame "
                         "(supported: \"strand\", \"letters\", \"frame\")" % kind)
    byte_kind = _SEED_FILTER_KINDS[kind]
    return _seed_filter(lib.pmx_seed_filter, _ungapped_kind(byte_kind), byte_kind == "frame", kind, Q, R, hits, matrix, min_score, top_n, code,
                        chunk_pairs)


def seed_filter_translated(Q, R, hits, matrix, min_score=0, top_n=0, code=None, chunk_pairs=0):
    """seed_filter for the lists it refuses: hits.kind "codons" (seed_pairs(frames="codons..."): Q nucleotides, R proteins),
    "ref_frames" and "ref_codons" (a translated index: Q proteins, R nucleotides); the cells a candidate's diagonals mean are those
    of seed_ungapped_translated.  The result keeps kind, .strand / .frame and .seeds (with "reserved") and adds .ungapped and
    .source; it goes where the unfiltered list goes: align_pairs(..., frameshift=, strand=hits.strand), align_pairs(...,
    ref_frame=hits.frame), align_pairs(..., ref_frameshift=, ref_strand=hits.strand) and the frameshift_ref_cigar entries.  code: the
    genetic code the list was seeded with (None: the standard code)."""
    kind = getattr(hits, "kind", None)
    if kind in _SEED_FILTER_KINDS or kind is None:
        raise BatchError("seed_filter_translated takes the lists of kind \"codons\", \"ref_frames\" and \"ref_codons\"; a list of kind "
                         "\"%s\" goes to seed_filter" % ("strand / letters / frame" if kind is None else kind))
    return _seed_filter(lib.pmx_seed_filter_translated, _ungapped_list_kind(kind), kind == "ref_frames", kind, Q, R, hits, matrix, min_score,
                        top_n, code, chunk_pairs)


def _seed_filter(entry, kind_value, byte_is_frame, kind, Q, R, hits, matrix, min_score, top_n, code, chunk_pairs):
    cfg = _ungapped_config(matrix)
    byte = np.ascontiguousarray(hits.frame if byte_is_frame else hits.strand, dtype=np.uint8)
    pairs = np.ascontiguousarray(hits.pairs, dtype=PAIR_DTYPE)
    seeds = np.ascontiguousarray(hits.seeds, dtype=SEED_HIT_DTYPE)
    row_off = np.ascontiguousarray(hits.row_off, dtype=np.int64)
    n = len(pairs)
    if len(byte) != n or len(seeds) != n or len(row_off) != hits.n_rows + 1:
        raise BatchError("the arrays of hits differ in length")
    h = pmx_seed_hits_t(int(hits.n_rows), n, int(hits.n_passing), row_off.ctypes.data, pairs.ctypes.data if n else None,
                        byte.ctypes.data if n else None, seeds.ctypes.data if n else None)
    code = _code_arg(code)
    fopts = pmx_seed_filter_opts_t(int(min_score), int(top_n))
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    res = C.POINTER(pmx_seed_filtered_t)()
    if entry(C.byref(cfg), Q._handle(), R._handle(), C.byref(h), kind_value, code.ctypes.data if code is not None else None, C.byref(fopts),
             C.byref(opts), C.byref(res)):
        raise BatchError(lib.pmx_last_error().decode())
    try:
        r = res.contents
        out = SeedHits(r.hits, byte_is_frame=byte_is_frame, kind=kind)
        k = out.n_hits
        out.ungapped = (np.frombuffer(C.string_at(r.ungapped, k * UNGAPPED_DTYPE.itemsize), dtype=UNGAPPED_DTYPE).copy() if k
                        else np.zeros(0, dtype=UNGAPPED_DTYPE))
        out.source = np.frombuffer(C.string_at(r.source, k * 8), dtype=np.int64).copy() if k else np.zeros(0, dtype=np.int64)
        return out
    finally:
        lib.pmx_seed_filtered_free(res)


def seed_filter_device(Q, R, n, d_pairs, d_byte, d_seeds, max_qlen, max_rlen, matrix, nq, d_row_off, d_out_pairs, d_out_byte, d_out_seeds,
                       d_out_ungapped, d_out_source, capacity, d_out_row_off, d_counts, kind="strand", code=None, min_score=0, top_n=0,
                       stream=0, chunk_pairs=0):
    """Device-pointer entry of seed_filter over the complete list of nq rows (n = row_off[nq]): the kept candidates' columns (each
    optional, `capacity` entries), d_out_row_off gets nq + 1 offsets and d_counts [kept, written].  Asynchronous on `stream`."""
    _seed_filter_device(lib.pmx_seed_filter_device, _ungapped_kind(kind), Q, R, n, d_pairs, d_byte, d_seeds, max_qlen, max_rlen, matrix, nq, d_row_off,
                        d_out_pairs, d_out_byte, d_out_seeds, d_out_ungapped, d_out_source, capacity, d_out_row_off, d_counts, code, min_score, top_n,
                        stream, chunk_pairs)


def seed_filter_translated_device(Q, R, n, d_pairs, d_byte, d_seeds, max_qlen, max_rlen, matrix, nq, d_row_off, d_out_pairs, d_out_byte,
                                  d_out_seeds, d_out_ungapped, d_out_source, capacity, d_out_row_off, d_counts, kind, code=None, min_score=0,
                                  top_n=0, stream=0, chunk_pairs=0):
    """Device-pointer entry of seed_filter_translated (kind "codons", "ref_frames" or "ref_codons"), with seed_filter_device's
    arguments and outputs.  Asynchronous on `stream`."""
    _seed_filter_device(lib.pmx_seed_filter_translated_device, _ungapped_list_kind(kind), Q, R, n, d_pairs, d_byte, d_seeds, max_qlen, max_rlen,
                        matrix, nq, d_row_off, d_out_pairs, d_out_byte, d_out_seeds, d_out_ungapped, d_out_source, capacity, d_out_row_off, d_counts,
                        code, min_score, top_n, stream, chunk_pairs)


def _seed_filter_device(entry, kind_value, Q, R, n, d_pairs, d_byte, d_seeds, max_qlen, max_rlen, matrix, nq, d_row_off, d_out_pairs, d_out_byte,
                        d_out_seeds, d_out_ungapped, d_out_source, capacity, d_out_row_off, d_counts, code, min_score, top_n, stream, chunk_pairs):
    cfg = _ungapped_config(matrix)
    code = _code_arg(code)
    fopts = pmx_seed_filter_opts_t(int(min_score), int(top_n))
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    if entry(C.byref(cfg), Q._handle(), R._handle(), int(n), d_pairs, d_byte, kind_value, code.ctypes.data if code is not None else None, d_seeds,
             int(max_qlen), int(max_rlen), int(nq), d_row_off, C.byref(fopts), d_out_pairs, d_out_byte, d_out_seeds, d_out_ungapped, d_out_source,
             int(capacity), d_out_row_off, d_counts, stream, C.byref(opts)):
        raise BatchError(lib.pmx_last_error().decode())


def seed_mix(key, k):
    """The order of the minimizers: mix of include/parasail_amd.h on the 2 k bits of a k-mer's key."""
    return int(lib.pmx_seed_mix(int(key), int(k)))


def seed_sketch_shape():
    """(row_tile, set_tile): the positions one workgroup of the sketch kernel owns in its row form and in its set form."""
    r, s = C.c_int32(0), C.c_int32(0)
    lib.pmx_seed_sketch_shape(C.byref(r), C.byref(s))
    return int(r.value), int(s.value)


def seed_minimizers(Q, k, w, strand="both", first_row=0, rows=None, max_qlen=None, stream=0):
    """The (w, k) minimizers of the rows of Q (pmx_seed_sketch): a uint8 array of shape (rows, orientations, max_qlen), 1 where the
    oriented position is a minimizer; orientations = 2 with strand "both" (index 1: the reverse complement, positions in oriented
    coordinates).  max_qlen: None -- the longest of the rows; a row longer than max_qlen has no minimizer."""
    rows = len(Q) - int(first_row) if rows is None else int(rows)
    mode = _strand_mode(strand)
    if max_qlen is None:
        max_qlen = int(lib.pmx_seed_rows_max_len(Q._handle(), int(first_row), rows))
        if max_qlen < 0:
            raise BatchError(lib.pmx_last_error().decode())
        max_qlen = max(1, max_qlen)
    orients = 2 if mode == STRAND_BOTH else 1
    out = np.zeros((max(rows, 0), orients, max(int(max_qlen), 0)), dtype=np.uint8)
    if lib.pmx_seed_sketch(Q._handle(), int(first_row), rows, int(max_qlen), int(k), int(w), mode, out.ctypes.data if out.size else None, stream):
        raise BatchError(lib.pmx_last_error().decode())
    return out


def seed_minimizers_device(Q, q_first, nq, max_qlen, k, w, d_flags, strand="both", stream=0):
    """Device-pointer entry of seed_minimizers: one byte per position slot (row_local * orientations + s) * max_qlen + i into d_flags;
    asynchronous on `stream`."""
    if lib.pmx_seed_sketch_device(Q._handle(), int(q_first), int(nq), int(max_qlen), int(k), int(w), _strand_mode(strand), d_flags, stream):
        raise BatchError(lib.pmx_last_error().decode())


def seed_index_entries_device(index, first, count, d_kmer, d_seq, d_pos, stream=0):
    """Entries [first, first + count) of the index in its order: key (uint64), sequence (int64), position (int32) (test hook)."""
    if lib.pmx_seed_index_entries_device(index._handle(), int(first), int(count), d_kmer, d_seq, d_pos, stream):
        raise BatchError(lib.pmx_last_error().decode())


def as_pairs(pairs):
    """PAIR_DTYPE array from an array of that dtype or from (q, r) / (q, r, q_beg, q_len, r_beg, r_len) tuples."""
    if isinstance(pairs, np.ndarray) and pairs.dtype == PAIR_DTYPE:
        return np.ascontiguousarray(pairs)
    rows = list(pairs)
    a = np.zeros(len(rows), dtype=PAIR_DTYPE)
    a["q_len"] = -1
    a["r_len"] = -1
    for k, t in enumerate(rows):
        if len(t) == 2:
            a[k]["q"], a[k]["r"] = t
        else:
            a[k] = tuple(t)
    return a


def all_pairs_count(nseq):
    """Pairs of the strict upper triangle of nseq x nseq."""
    v = lib.pmx_all_pairs_count(int(nseq))
    if v < 0:
        raise BatchError(lib.pmx_last_error().decode())
    return int(v)


def all_pairs_index(nseq, p):
    """(i, j), i < j, of pair p in the row-major order of the all-pairs entries."""
    i, j = C.c_int64(), C.c_int64()
    if lib.pmx_all_pairs_index(int(nseq), int(p), C.byref(i), C.byref(j)):
        raise BatchError(lib.pmx_last_error().decode())
    return int(i.value), int(j.value)


def align_pairs_device(cfg, Q, R, n, d_pairs, max_qlen, max_rlen, d_out, d_stats=None, stream=0, chunk_pairs=0):
    """Device-pointer entry of the set batches: n PAIR_DTYPE descriptors in, n records (and statistics) out, all in device memory.
    A bad descriptor gets the record (0, -1, -1, FLAG_BAD_PAIR)."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    rc = lib.pmx_align_pairs_device(C.byref(cfg), Q._handle(), R._handle(), n, d_pairs, max_qlen, max_rlen, d_out, d_stats, stream,
                                    C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def complement_table():
    """The 256-byte complement a strand-1 query window is mapped through (uint8 [256])."""
    tab = np.zeros(256, dtype=np.uint8)
    lib.pmx_complement_table(tab.ctypes.data)
    return tab


def align_pairs_ex_device(cfg, Q, R, n, d_pairs, d_strand, max_qlen, max_rlen, d_out, d_stats=None, d_beg=None, d_text=None, capacity=0,
                          d_text_off=None, stream=0, chunk_pairs=0):
    """Device-pointer entry of the set batches with strands (d_strand: n bytes or None) and, with WANT_CIGAR in cfg.want, CIGAR text
    (d_text / capacity / d_text_off as align_batch_cigar_device) and begins (d_beg: 2 n int32, optional)."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    rc = lib.pmx_align_pairs_ex_device(C.byref(cfg), Q._handle(), R._handle(), n, d_pairs, d_strand, max_qlen, max_rlen, d_out, d_stats,
                                       d_beg, d_text, capacity, d_text_off, stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def gather_pairs_device(Q, R, n, d_pairs, d_strand, max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff,
                        d_ok=None, stream=0):
    """The resolved windows of n descriptors (strand applied), packed back to back in device memory; d_qoff / d_roff get n + 1 offsets."""
    rc = lib.pmx_gather_pairs_device(Q._handle(), R._handle(), n, d_pairs, d_strand, max_qlen, max_rlen, d_qout, q_capacity, d_qoff,
                                     d_rout, r_capacity, d_roff, d_ok, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_all_pairs_device(cfg, S, first, count, max_len, d_out, d_stats=None, stream=0, chunk_pairs=0):
    """Device-pointer all-vs-all entry: pairs [first, first + count) of the upper triangle of S x S."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    rc = lib.pmx_align_all_pairs_device(C.byref(cfg), S._handle(), first, count, max_len, d_out, d_stats, stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def all_pairs_enumerate_device(nseq, first, count, d_pairs, stream=0):
    """The descriptors the all-pairs entries generate, into `count` PAIR_DTYPE slots of device memory (test hook)."""
    if lib.pmx_all_pairs_enumerate_device(int(nseq), int(first), int(count), d_pairs, stream):
        raise BatchError(lib.pmx_last_error().decode())


def rect_pairs_count(nq, nr):
    """Pairs of the rectangle nq x nr."""
    v = lib.pmx_rect_pairs_count(int(nq), int(nr))
    if v < 0:
        raise BatchError(lib.pmx_last_error().decode())
    return int(v)


def rect_pairs_enumerate_device(nq, nr, first, count, d_pairs, stream=0):
    """The descriptors a rectangular set search generates, into `count` PAIR_DTYPE slots of device memory (test hook)."""
    if lib.pmx_rect_pairs_enumerate_device(int(nq), int(nr), int(first), int(count), d_pairs, stream):
        raise BatchError(lib.pmx_last_error().decode())


def search_pairs_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs,
                        d_hit_stats, capacity, d_counts, stream=0, chunk_pairs=0):
    """Device-pointer entry of the set search: the pairs of the enumeration (shape PAIRS_LIST / PAIRS_TRIANGLE / PAIRS_RECT) with
    score >= min_score, compacted in enumeration order into d_hit_pairs / d_hit_index (optional), d_hit_recs and d_hit_stats
    (`capacity` entries each); d_counts gets [passing, written]."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    rc = lib.pmx_search_pairs_device(C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(shape), int(first), int(n),
                                     d_pairs, max_qlen, max_rlen, int(min_score), d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                                     int(capacity), d_counts, stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def search_topk_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs,
                       d_hit_stats, capacity, d_row_off, d_row_passing, d_counts, stream=0, chunk_pairs=0):
    """Device-pointer entry of the per-query top-K: rows [q_first, q_first + nq) of Q against R (None: Q); per row the best k
    references with score >= min_score, CSR: d_row_off gets nq + 1 offsets, the hits go to d_hit_pairs / d_hit_index (optional),
    d_hit_recs and d_hit_stats (`capacity` entries each), d_row_passing (optional) the rows' passing counts and d_counts
    [kept, written, passing]."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    rc = lib.pmx_search_topk_device(C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(q_first), int(nq),
                                    max_qlen, max_rlen, int(min_score), int(k), 1 if skip_self else 0, d_hit_pairs, d_hit_index,
                                    d_hit_recs, d_hit_stats, int(capacity), d_row_off, d_row_passing, d_counts, stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def topk_records_device(d_rec, d_stats, q_first, nq, nr, min_score, k, skip_self, chunk_pairs, marked, d_hit_strand, d_hit_pairs, d_hit_index,
                        d_hit_recs, d_hit_stats, capacity, d_row_off, d_row_passing, d_counts, stream=0):
    """The selection of search_topk_device on the caller's nq * nr records (d_rec[li * nr + j]: pair (q_first + li, j)) instead of
    alignments, through the same kernels (test hook).  marked: flag bit 0x40000000 is taken out of the emitted records."""
    rc = lib.pmx_topk_records_device(d_rec, d_stats, int(q_first), int(nq), int(nr), int(min_score), int(k), 1 if skip_self else 0,
                                     int(chunk_pairs), 1 if marked else 0, d_hit_strand, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                                     int(capacity), d_row_off, d_row_passing, d_counts, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_pairs_both_device(cfg, Q, R, n, d_pairs, max_qlen, max_rlen, d_out, d_stats, d_strand_out, stream=0, chunk_pairs=0):
    """align_pairs_device on both strands: record k (and its statistics) is the better strand's, byte for byte, a tie going to the
    forward strand; d_strand_out (n bytes) says which one won."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    rc = lib.pmx_align_pairs_both_device(C.byref(cfg), Q._handle(), R._handle(), n, d_pairs, max_qlen, max_rlen, d_out, d_stats,
                                         d_strand_out, stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def search_pairs_stranded_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs,
                                 d_hit_stats, capacity, d_counts, strand_mode, d_hit_strand=None, stream=0, chunk_pairs=0):
    """search_pairs_device with a strand mode (STRAND_*): the threshold looks at the folded records; d_hit_strand (optional, one byte
    per hit) receives the hits' strands.  d_hit_pairs and d_hit_strand feed align_pairs_ex_device unchanged."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    rc = lib.pmx_search_pairs_stranded_device(C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(shape), int(first),
                                              int(n), d_pairs, max_qlen, max_rlen, int(min_score), d_hit_pairs, d_hit_index, d_hit_recs,
                                              d_hit_stats, int(capacity), d_counts, stream, C.byref(opts), int(strand_mode), d_hit_strand)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def search_topk_stranded_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs,
                                d_hit_stats, capacity, d_row_off, d_row_passing, d_counts, strand_mode, d_hit_strand=None, stream=0,
                                chunk_pairs=0):
    """search_topk_device with a strand mode (STRAND_*): a reference is one candidate with its folded record; d_hit_strand
    (optional, one byte per hit) receives the hits' strands."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    rc = lib.pmx_search_topk_stranded_device(C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(q_first), int(nq),
                                             max_qlen, max_rlen, int(min_score), int(k), 1 if skip_self else 0, d_hit_pairs, d_hit_index,
                                             d_hit_recs, d_hit_stats, int(capacity), d_row_off, d_row_passing, d_counts, stream,
                                             C.byref(opts), int(strand_mode), d_hit_strand)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def gather_pairs_translated_device(Q, R, n, d_pairs, d_frame, max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff,
                                   d_ok=None, stream=0, code=None):
    """gather_pairs_device with the query windows translated (d_frame: a frame byte per pair or None for frame 0; max_qlen bounds the
    translated length): the building block of a CIGAR pass over translated hits."""
    code = _code_arg(code)
    rc = lib.pmx_gather_pairs_translated_device(Q._handle(), R._handle(), n, d_pairs, d_frame, code.ctypes.data if code is not None else None,
                                                max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff, d_ok, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_pairs_translated_device(cfg, Q, R, n, d_pairs, d_frame, frame_mode, max_qlen, max_rlen, d_out, d_stats=None, d_frame_out=None,
                                  stream=0, chunk_pairs=0, code=None):
    """align_pairs_device with translated queries: d_frame (a frame byte per pair, frame_mode 0) or None and a frame mode (0 .. 5,
    FRAMES_*); record k is the best frame's, byte for byte, d_frame_out (n bytes) says which."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_align_pairs_translated_device(C.byref(cfg), Q._handle(), R._handle(), n, d_pairs, d_frame, int(frame_mode),
                                               code.ctypes.data if code is not None else None, max_qlen, max_rlen, d_out, d_stats, d_frame_out,
                                               stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def search_pairs_translated_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs,
                                   d_hit_stats, capacity, d_counts, frame_mode, d_hit_frame=None, stream=0, chunk_pairs=0, code=None):
    """search_pairs_device with translated queries and a frame mode: the threshold looks at the folded records; d_hit_frame (optional,
    one byte per hit) receives the hits' frames.  d_hit_pairs and d_hit_frame feed gather_pairs_translated_device unchanged."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_search_pairs_translated_device(C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(shape), int(first),
                                                int(n), d_pairs, max_qlen, max_rlen, int(min_score), d_hit_pairs, d_hit_index, d_hit_recs,
                                                d_hit_stats, int(capacity), d_counts, stream, C.byref(opts), int(frame_mode),
                                                code.ctypes.data if code is not None else None, d_hit_frame)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def search_topk_translated_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs,
                                  d_hit_stats, capacity, d_row_off, d_row_passing, d_counts, frame_mode, d_hit_frame=None, stream=0,
                                  chunk_pairs=0, code=None):
    """search_topk_device with translated queries and a frame mode: a reference is one candidate with its folded record; d_hit_frame
    (optional, one byte per hit) receives the hits' frames."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_search_topk_translated_device(C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(q_first), int(nq),
                                               max_qlen, max_rlen, int(min_score), int(k), 1 if skip_self else 0, d_hit_pairs, d_hit_index,
                                               d_hit_recs, d_hit_stats, int(capacity), d_row_off, d_row_passing, d_counts, stream,
                                               C.byref(opts), int(frame_mode), code.ctypes.data if code is not None else None, d_hit_frame)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def gather_pairs_codons_device(Q, R, n, d_pairs, d_strand, max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff,
                               d_ok=None, stream=0, code=None):
    """gather_pairs_translated_device in its stride-1 form: the query windows become codon streams (codon_stream(); d_strand: a strand
    byte per pair or None for forward; max_qlen bounds the stream's length, the window's minus 2)."""
    code = _code_arg(code)
    rc = lib.pmx_gather_pairs_codons_device(Q._handle(), R._handle(), n, d_pairs, d_strand, code.ctypes.data if code is not None else None,
                                            max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff, d_ok, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_pairs_frameshift_device(cfg, Q, R, n, d_pairs, d_strand, strand_mode, frameshift, max_qlen, max_rlen, d_out, d_strand_out=None,
                                  stream=0, chunk_pairs=0, code=None):
    """align_pairs_device by the three-frame local DP: d_strand (a strand byte per pair, strand_mode STRAND_FORWARD) or None and a
    strand mode; record k is the better strand's, d_strand_out (n bytes) says which.  max_qlen bounds the codon stream, W - 2."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_align_pairs_frameshift_device(C.byref(cfg), Q._handle(), R._handle(), n, d_pairs, d_strand, int(strand_mode), int(frameshift),
                                               code.ctypes.data if code is not None else None, max_qlen, max_rlen, d_out, d_strand_out,
                                               stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def gather_pairs_codons_ref_device(Q, R, n, d_pairs, d_strand, max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff,
                                   d_ok=None, stream=0, code=None):
    """gather_pairs_codons_device with the sides exchanged: the REFERENCE windows become codon streams (d_strand: the reference's
    strand byte per pair or None for forward; max_rlen bounds the stream's length, the window's minus 2), the queries are copied."""
    code = _code_arg(code)
    rc = lib.pmx_gather_pairs_codons_ref_device(Q._handle(), R._handle(), n, d_pairs, d_strand, code.ctypes.data if code is not None else None,
                                                max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff, d_ok, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_pairs_frameshift_ref_device(cfg, Q, R, n, d_pairs, d_strand, strand_mode, frameshift, max_qlen, max_rlen, d_out, d_strand_out=None,
                                      stream=0, chunk_pairs=0, code=None):
    """align_pairs_frameshift_device with the sides exchanged: protein queries of up to max_qlen letters against the codon streams of
    nucleotide reference windows; the strands are the reference's, max_rlen bounds the stream, W - 2, and has no cap."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_align_pairs_frameshift_ref_device(C.byref(cfg), Q._handle(), R._handle(), n, d_pairs, d_strand, int(strand_mode), int(frameshift),
                                                   code.ctypes.data if code is not None else None, max_qlen, max_rlen, d_out, d_strand_out,
                                                   stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_pairs_frameshift_cigar_device(cfg, Q, R, n, d_pairs, d_strand, strand_mode, frameshift, max_qlen, max_rlen, d_out, d_strand_out,
                                        d_stats, d_beg, d_cigar_text, cigar_capacity, d_cigar_off, stream=0, chunk_pairs=0, code=None):
    """align_pairs_frameshift_device with the traceback behind it (cfg.want: WANT_CIGAR, with WANT_STATS iff d_stats): the same records
    and strand bytes, the CIGAR text with the frameshift ops '/' and '\\' at d_cigar_off[k] of d_cigar_text (align_pairs_ex_device's
    buffer rules), begins in d_beg (2 n int32, optional), the paths' statistics in d_stats."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_align_pairs_frameshift_cigar_device(C.byref(cfg), Q._handle(), R._handle(), n, d_pairs, d_strand, int(strand_mode),
                                                     int(frameshift), code.ctypes.data if code is not None else None, max_qlen, max_rlen,
                                                     d_out, d_strand_out, d_stats, d_beg, d_cigar_text, int(cigar_capacity), d_cigar_off,
                                                     stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_pairs_frameshift_ref_cigar_device(cfg, Q, R, n, d_pairs, d_strand, strand_mode, frameshift, max_qlen, max_rlen, d_out, d_strand_out,
                                            d_stats, d_beg, d_cigar_text, cigar_capacity, d_cigar_off, stream=0, chunk_pairs=0, code=None):
    """align_pairs_frameshift_ref_device with the traceback behind it (cfg.want: WANT_CIGAR, with WANT_STATS iff d_stats): the same
    records and strand bytes -- the REFERENCE's strand --, the CIGAR text at d_cigar_off[k] of d_cigar_text, begins in d_beg (2 n int32,
    optional: query letter, reference nucleotide), the paths' statistics in d_stats.  max_rlen bounds W - 2, the stream's letters."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_align_pairs_frameshift_ref_cigar_device(C.byref(cfg), Q._handle(), R._handle(), n, d_pairs, d_strand, int(strand_mode),
                                                         int(frameshift), code.ctypes.data if code is not None else None, max_qlen, max_rlen,
                                                         d_out, d_strand_out, d_stats, d_beg, d_cigar_text, int(cigar_capacity), d_cigar_off,
                                                         stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_pairs_frameshift_ref_cigar_long_device(cfg, Q, R, n, d_pairs, d_strand, strand_mode, frameshift, max_qlen, max_rlen, d_out, d_strand_out,
                                                 d_stats, d_beg, d_cigar_text, cigar_capacity, d_cigar_off, stream=0, chunk_pairs=0, code=None):
    """align_pairs_frameshift_ref_cigar_device for long references: the same arguments and byte-identical outputs, the traceback over
    each record's window only.  Synchronises `stream` once per chunk and once at the end."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_align_pairs_frameshift_ref_cigar_long_device(C.byref(cfg), Q._handle(), R._handle(), n, d_pairs, d_strand, int(strand_mode),
                                                              int(frameshift), code.ctypes.data if code is not None else None, max_qlen,
                                                              max_rlen, d_out, d_strand_out, d_stats, d_beg, d_cigar_text,
                                                              int(cigar_capacity), d_cigar_off, stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def search_pairs_frameshift_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs,
                                   capacity, d_counts, strand_mode, frameshift, d_hit_strand=None, stream=0, chunk_pairs=0, code=None):
    """search_pairs_stranded_device by the three-frame local DP (no statistics): the threshold looks at the folded records;
    d_hit_strand (optional, one byte per hit) receives the hits' strands."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_search_pairs_frameshift_device(C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(shape), int(first),
                                                int(n), d_pairs, max_qlen, max_rlen, int(min_score), d_hit_pairs, d_hit_index, d_hit_recs,
                                                None, int(capacity), d_counts, stream, C.byref(opts), int(strand_mode), d_hit_strand,
                                                int(frameshift), code.ctypes.data if code is not None else None)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def search_topk_frameshift_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs,
                                  capacity, d_row_off, d_row_passing, d_counts, strand_mode, frameshift, d_hit_strand=None, stream=0,
                                  chunk_pairs=0, code=None):
    """search_topk_stranded_device by the three-frame local DP (no statistics): a reference is one candidate with its folded record;
    d_hit_strand (optional, one byte per hit) receives the hits' strands."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_search_topk_frameshift_device(C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(q_first), int(nq),
                                               max_qlen, max_rlen, int(min_score), int(k), 1 if skip_self else 0, d_hit_pairs, d_hit_index,
                                               d_hit_recs, None, int(capacity), d_row_off, d_row_passing, d_counts, stream,
                                               C.byref(opts), int(strand_mode), d_hit_strand, int(frameshift),
                                               code.ctypes.data if code is not None else None)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def gather_pairs_translated_ref_device(Q, R, n, d_pairs, d_frame, max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff,
                                   d_ok=None, stream=0, code=None):
    """gather_pairs_device with the reference windows translated (d_frame: a frame byte per pair or None for frame 0; max_rlen bounds
    the translated length): the building block of a CIGAR pass over the hits of a reference-side translated search."""
    code = _code_arg(code)
    rc = lib.pmx_gather_pairs_translated_ref_device(Q._handle(), R._handle(), n, d_pairs, d_frame, code.ctypes.data if code is not None else None,
                                                max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff, d_ok, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_pairs_translated_ref_device(cfg, Q, R, n, d_pairs, d_frame, frame_mode, max_qlen, max_rlen, d_out, d_stats=None, d_frame_out=None,
                                  stream=0, chunk_pairs=0, code=None):
    """align_pairs_device with translated references (Q proteins, R nucleotides): d_frame (a frame byte per pair, frame_mode 0) or None and a frame mode (0 .. 5,
    FRAMES_*); record k is the best frame's, byte for byte, d_frame_out (n bytes) says which."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_align_pairs_translated_ref_device(C.byref(cfg), Q._handle(), R._handle(), n, d_pairs, d_frame, int(frame_mode),
                                               code.ctypes.data if code is not None else None, max_qlen, max_rlen, d_out, d_stats, d_frame_out,
                                               stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def search_pairs_translated_ref_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs,
                                   d_hit_stats, capacity, d_counts, frame_mode, d_hit_frame=None, stream=0, chunk_pairs=0, code=None):
    """search_pairs_device with translated references and a frame mode: the threshold looks at the folded records; d_hit_frame (one
    byte per hit; required in a multi-frame mode with capacity > 0) receives the hits' frames.  d_hit_pairs and d_hit_frame feed
    gather_pairs_translated_ref_device unchanged."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_search_pairs_translated_ref_device(C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(shape), int(first),
                                                int(n), d_pairs, max_qlen, max_rlen, int(min_score), d_hit_pairs, d_hit_index, d_hit_recs,
                                                d_hit_stats, int(capacity), d_counts, stream, C.byref(opts), int(frame_mode),
                                                code.ctypes.data if code is not None else None, d_hit_frame)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def search_topk_translated_ref_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs,
                                  d_hit_stats, capacity, d_row_off, d_row_passing, d_counts, frame_mode, d_hit_frame=None, stream=0,
                                  chunk_pairs=0, code=None):
    """search_topk_device with translated references and a frame mode: a reference is one candidate with its folded record;
    d_hit_frame (one byte per hit; required in a multi-frame mode with capacity > 0) receives the hits' frames."""
    opts = pmx_pairs_opts_t(int(chunk_pairs))
    code = _code_arg(code)
    rc = lib.pmx_search_topk_translated_ref_device(C.byref(cfg), Q._handle(), R._handle() if R is not None else None, int(q_first), int(nq),
                                               max_qlen, max_rlen, int(min_score), int(k), 1 if skip_self else 0, d_hit_pairs, d_hit_index,
                                               d_hit_recs, d_hit_stats, int(capacity), d_row_off, d_row_passing, d_counts, stream,
                                               C.byref(opts), int(frame_mode), code.ctypes.data if code is not None else None, d_hit_frame)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_batch_device(cfg, n, d_qbuf, d_qoff, d_rbuf, d_roff, max_qlen, max_rlen, d_out, d_stats=None, stream=0):
    """Device-pointer entry (ints are raw device addresses, `stream` a hipStream_t value)."""
    rc = lib.pmx_align_batch_device(C.byref(cfg), n, d_qbuf, d_qoff, d_rbuf, d_roff, max_qlen, max_rlen,
                                    d_out, d_stats, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_batch_cigar_device(cfg, n, d_qbuf, d_qoff, d_rbuf, d_roff, max_qlen, max_rlen, d_out, d_text, capacity, d_text_off, stream=0):
    """Device-pointer CIGAR entry: records + CIGAR text + n+1 text offsets, all in device memory."""
    rc = lib.pmx_align_batch_cigar_device(C.byref(cfg), n, d_qbuf, d_qoff, d_rbuf, d_roff, max_qlen, max_rlen,
                                          d_out, d_text, capacity, d_text_off, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def align_batch_cigar_long_device(cfg, n, d_qbuf, d_qoff, d_rbuf, d_roff, max_qlen, max_rlen, d_out, d_stats, d_text, capacity, d_text_off,
                                  stream=0, tile_cols=0, band_rows=0):
    """Device-pointer entry of the tiled long-pair traceback: records, statistics, CIGAR text + n+1 text offsets in device memory."""
    opts = pmx_long_cigar_opts_t(int(tile_cols), int(band_rows))
    rc = lib.pmx_align_batch_cigar_long_device(C.byref(cfg), n, d_qbuf, d_qoff, d_rbuf, d_roff, max_qlen, max_rlen,
                                               d_out, d_stats, d_text, capacity, d_text_off, stream, C.byref(opts))
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def long_cigar_scratch_bytes(n, max_qlen, max_rlen, tile_cols=0, band_rows=0):
    """Device scratch of one chunk of the tiled long-pair traceback (a planner: no GPU needed)."""
    opts = pmx_long_cigar_opts_t(int(tile_cols), int(band_rows))
    v = lib.pmx_long_cigar_scratch_bytes(n, max_qlen, max_rlen, C.byref(opts))
    if v < 0:
        raise BatchError(lib.pmx_last_error().decode())
    return int(v)


def align_profile_batch_device(cfg, profile, n, d_rbuf, d_roff, max_rlen, d_out, d_stats=None, stream=0):
    """One reused query profile against device-resident references."""
    rc = lib.pmx_align_profile_batch_device(C.byref(cfg), profile.inner, n, d_rbuf, d_roff, max_rlen, d_out, d_stats, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def select_hits_device(d_rec, n, min_score, max_hits, order, d_hit_index, capacity, d_counts, stream=0):
    """Device-pointer hit selection over n 16-byte records: indices of the records with score >= min_score (the best max_hits of
    them, 0 = all) into d_hit_index (at most `capacity`), the numbers selected and passing into d_counts[0:2] (int64)."""
    rc = lib.pmx_select_hits_device(d_rec, n, int(min_score), int(max_hits), int(order), d_hit_index, capacity, d_counts, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def gather_refs_device(d_rbuf, d_roff, n, d_index, h, d_out, out_capacity, d_out_off, stream=0):
    """References d_index[0:h] of a packed device buffer back to back into d_out, their h + 1 offsets into d_out_off."""
    rc = lib.pmx_gather_refs_device(d_rbuf, d_roff, n, d_index, h, d_out, out_capacity, d_out_off, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def search_profile_device(cfg, profile, n, d_rbuf, d_roff, max_rlen, min_score, max_hits, order, band, d_first, d_hits, d_recs,
                          d_stats, capacity, d_text, cigar_capacity, d_text_off, d_counts, stream=0):
    """Device-pointer profile search: hits (HIT_DTYPE), second-pass records / statistics / CIGAR text + offsets for at most
    `capacity` hits into caller buffers, counts into d_counts[0:2].  Synchronises `stream` once, between the passes."""
    opts = pmx_search_opts_t(int(min_score), int(max_hits), int(order), int(band))
    rc = lib.pmx_search_profile_device(C.byref(cfg), profile.inner if profile is not None else None, n, d_rbuf, d_roff, max_rlen,
                                       C.byref(opts), d_first, d_hits, d_recs, d_stats, capacity, d_text, cigar_capacity, d_text_off,
                                       d_counts, stream)
    if rc:
        raise BatchError(lib.pmx_last_error().decode())


def pack_2bit(buf, alphabet=b"ACGT"):
    """ASCII letters -> 2 bits per base (base b in byte b / 4 at bits 2 (b % 4)), the input form of pmx_align_batch_2bit."""
    lut = np.zeros(256, dtype=np.uint8)
    for i, ch in enumerate(alphabet[:4]):
        lut[ch] = i; lut[ord(chr(ch).lower())] = i
    codes = lut[buf]
    pad = (-len(codes)) % 4
    if pad:
        codes = np.concatenate([codes, np.zeros(pad, dtype=np.uint8)])
    c = codes.reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8)


def _record_buffer(out, n):
    if out is None:
        return np.zeros(n, dtype=RECORD_DTYPE)
    if out.dtype != RECORD_DTYPE or out.shape != (n,) or not out.flags.c_contiguous:
        raise BatchError("out must be a contiguous RECORD_DTYPE array of %d records" % n)
    return out


def switches():
    """[(name, kind, what)] for every environment switch the library reads (csrc/pmx_switches.h)."""
    return [tuple(line.split("\t")) for line in lib.pmx_switches().decode().splitlines()]


def host_register(*arrays):
    """Page-lock numpy arrays handed to the host-buffer batch entries (full PCIe rate); undo with host_unregister."""
    for a in arrays:
        if lib.pmx_host_register(a.ctypes.data, a.nbytes):
            raise BatchError(lib.pmx_last_error().decode())


def host_unregister(*arrays):
    for a in arrays:
        lib.pmx_host_unregister(a.ctypes.data)


def shard_bounds_by_cells(qoff, roff, parts):
    """The C planner behind pmx_align_batch_multi (qoff None: one shared query)."""
    roff = np.ascontiguousarray(roff, dtype=np.int64)
    n = len(roff) - 1
    b = np.zeros(parts + 1, dtype=np.int64)
    q = None if qoff is None else np.ascontiguousarray(qoff, dtype=np.int64)
    if lib.pmx_shard_bounds_by_cells(n, q.ctypes.data if q is not None else None, roff.ctypes.data, parts, b.ctypes.data):
        raise BatchError("planner failed")
    return [int(x) for x in b]


def version():
    return lib.pmx_version().decode()
