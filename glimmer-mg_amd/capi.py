"""ctypes prototypes for include/gmg.h and include/gmg_icm.h.  Loading fails loudly when the
library is missing: there is no Python or CPU fallback."""
import ctypes as C
import os

from .build import LIB

_lib = None

vp = C.c_void_p
u64 = C.c_uint64
i32 = C.c_int


class Segment(C.Structure):
    _fields_ = [("read", C.c_uint32), ("lo", C.c_uint32), ("len", C.c_uint32), ("orient", C.c_uint32)]


class GeneRegion(C.Structure):
    _fields_ = [("read", C.c_uint32), ("first", C.c_int32), ("len", C.c_int32), ("strand", C.c_int32)]


class Coord(C.Structure):
    _fields_ = [("read", C.c_uint32), ("dir", C.c_int32), ("start", C.c_int64), ("end", C.c_int64)]


class TextParams(C.Structure):
    _fields_ = [("fwd", C.c_uint8 * 256), ("rev", C.c_uint8 * 256), ("width", C.c_uint32), ("reserved", C.c_uint32)]


class RunsTextParams(C.Structure):
    _fields_ = [("up", C.c_uint8 * 256), ("down", C.c_uint8 * 256), ("sub_up", C.c_uint8 * 256), ("sub_down", C.c_uint8 * 256),
                ("literal", C.c_uint8 * 4), ("pad", C.c_uint8), ("unknown", C.c_uint8), ("reserved", C.c_uint8 * 2), ("aa", C.c_char * 64),
                ("width", C.c_uint32), ("mode", C.c_uint32)]


class SpliceRun(C.Structure):
    _fields_ = [("read", C.c_uint32), ("first", C.c_uint32), ("len", C.c_uint32), ("kind", C.c_uint32)]


class EditGene(C.Structure):
    _fields_ = [("read", C.c_uint32), ("frame", C.c_int32), ("col2", C.c_int64), ("col3", C.c_int64), ("n_ins", C.c_uint32),
                ("n_del", C.c_uint32), ("n_sub", C.c_uint32), ("reserved", C.c_uint32)]


class EditString(C.Structure):
    _fields_ = [("gene", C.c_uint64), ("start", C.c_int64), ("end", C.c_int64), ("strand", C.c_int32), ("pad_front", C.c_uint32),
                ("pad_behind", C.c_uint32), ("reserved", C.c_uint32)]


class FeatureGene(C.Structure):
    _fields_ = [("read", C.c_uint32), ("strand", C.c_int32), ("start", C.c_int32), ("end", C.c_int32), ("start_codon", C.c_int32)]


class FeaturesParams(C.Structure):
    _fields_ = [("min_length", C.c_int32), ("max_overlap", C.c_int32), ("drop_tga", C.c_int32), ("reserved", C.c_int32)]


class FeaturesTable(C.Structure):
    _fields_ = [("n_lengths", C.c_uint64), ("lengths", C.POINTER(C.c_int64)), ("starts", C.c_int64 * 3), ("orient", C.c_double * 4),
                ("orient_raw", C.c_double * 4), ("n_dist", C.c_uint64 * 3), ("dist", C.POINTER(C.c_double) * 3)]


class AuditParams(C.Structure):
    _fields_ = [("n_start_codons", C.c_int32), ("n_stop_codons", C.c_int32), ("start_codon", (C.c_char * 4) * 8),
                ("stop_codon", (C.c_char * 4) * 8), ("flags", C.c_int32), ("reserved", C.c_int32)]


class MgGroup(C.Structure):
    _fields_ = [("gene", C.c_void_p), ("read_begin", C.c_uint64), ("read_end", C.c_uint64)]


class OrfParams(C.Structure):
    _fields_ = [("min_gene_len", C.c_int32), ("allow_truncated", C.c_int32), ("use_first_start", C.c_int32),
                ("ignore_score_len", C.c_int32), ("start_threshold", C.c_double), ("n_start_codons", C.c_int32),
                ("start_codon", (C.c_char * 4) * 8)]


class MgParams(C.Structure):
    _fields_ = [("min_gene_len", C.c_int32), ("allow_truncated", C.c_int32), ("ignore_score_len", C.c_int32),
                ("n_start_codons", C.c_int32), ("n_stop_codons", C.c_int32), ("flags", C.c_int32),
                ("start_threshold", C.c_double), ("start_codon", (C.c_char * 4) * 8),
                ("stop_codon", (C.c_char * 4) * 8),
                # the error branch (GMG_MG_ALLOW_INDELS / GMG_MG_ALLOW_SUBS)
                ("min_indel_orf_len", C.c_int32), ("indel_quality_threshold", C.c_int32), ("indel_max", C.c_int32),
                ("circular", C.c_int32), ("indel_suffix_score_threshold", C.c_double), ("quality", C.c_void_p),
                # classification mode: per-read null model / Ignore_Score_Len
                ("nulls", C.c_void_p), ("read_null", C.c_void_p), ("read_ignore_score_len", C.c_void_p),
                # gmg_find_orfs only: ignore regions (glimmer3 -i)
                ("n_ignore_regions", C.c_int32), ("reserved2", C.c_int32), ("ignore_lo", C.c_void_p), ("ignore_hi", C.c_void_p)]


TOPHITS_MAX_FIELD = 19                      # GMG_TOPHITS_MAX_FIELD (include/gmg.h)

PROTOTYPES = {
    # include/gmg.h
    "gmg_init": (i32, [i32]),
    "gmg_device_count": (i32, []),
    "gmg_last_error": (C.c_char_p, []),
    "gmg_version": (C.c_char_p, []),
    "gmg_synchronize": (i32, [vp]),
    "gmg_shard_plan": (i32, [vp, u64, i32, vp]),
    "gmg_fasta_shard_ranges": (i32, [C.c_char_p, u64, i32, vp]),
    "gmg_gc_fraction": (C.c_double, [vp, vp, i32, i32]),
    "gmg_set_option": (i32, [C.c_char_p, C.c_longlong]),
    "gmg_get_option": (i32, [C.c_char_p, C.POINTER(C.c_longlong)]),
    "gmg_base_code": (i32, [i32]),
    "gmg_pack_bases": (i32, [C.c_char_p, u64, u64, vp]),
    "gmg_packed_words": (u64, [u64]),
    "gmg_model_upload": (i32, [vp, vp, i32, i32, i32, i32, C.POINTER(vp)]),
    "gmg_model_free": (i32, [vp]),
    "gmg_model_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "gmg_icm_bytes_info": (i32, [vp, u64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(u64)]),
    "gmg_model_set_load": (i32, [vp, vp, i32, C.POINTER(vp), vp]),
    "gmg_model_set_finish": (i32, [vp, C.POINTER(i32)]),
    "gmg_model_set_model": (vp, [vp, i32]),
    "gmg_model_set_free": (i32, [vp]),
    "gmg_model_blob": (i32, [vp, vp, C.POINTER(C.c_size_t)]),
    "gmg_model_value_stats": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "gmg_reads_upload": (i32, [vp, vp, u64, C.POINTER(vp)]),
    "gmg_reads_wrap_device": (i32, [vp, vp, u64, u64, C.POINTER(vp)]),
    "gmg_reads_free": (i32, [vp]),
    "gmg_reads_info": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
    "gmg_reads_download": (i32, [vp, vp, vp]),
    "gmg_reads_select": (i32, [vp, vp, u64, C.POINTER(vp)]),
    "gmg_reads_extract": (i32, [vp, vp, u64, i32, vp, vp, u64, C.POINTER(vp)]),
    "gmg_fasta_ambiguous": (i32, [C.c_char_p, u64, vp, vp, u64, C.POINTER(u64)]),
    "gmg_extract_plan": (i32, [vp, u64, vp, u64, i32, C.c_int64, vp, vp, C.POINTER(u64)]),
    "gmg_letters_upload": (i32, [vp, vp, u64, C.POINTER(vp)]),
    "gmg_letters_free": (i32, [vp]),
    "gmg_letters_kernel_ms": (i32, [vp, C.POINTER(C.c_float)]),
    "gmg_text_params_reference": (i32, [vp, C.c_uint32]),
    "gmg_regions_text": (i32, [vp, vp, u64, vp, vp, vp, vp, C.POINTER(C.c_size_t), vp]),
    "gmg_regions_text_device": (i32, [vp, vp, u64, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t), vp]),
    "gmg_runs_text_params_script": (i32, [vp, i32, i32]),
    "gmg_runs_text": (i32, [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_size_t), vp]),
    "gmg_runs_text_device": (i32, [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t), vp]),
    "gmg_reads_splice": (i32, [vp, vp, u64, vp, u64, i32, C.POINTER(vp)]),
    "gmg_edits_plan": (i32, [vp, u64, vp, u64, vp, vp, C.c_char_p, u64, vp, u64, C.POINTER(u64), vp, vp]),
    "gmg_single_create": (i32, [C.POINTER(vp)]),
    "gmg_single_stage": (i32, [vp, C.c_char_p, u64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "gmg_single_fetch": (i32, [vp, vp, C.c_size_t]),
    "gmg_single_free": (i32, [vp]),
    "gmg_single_window": (i32, [vp, vp, vp, i32, i32, vp, vp]),
    "gmg_segments_upload": (i32, [vp, vp, u64, vp, C.POINTER(u64), C.POINTER(vp)]),
    "gmg_segments_free": (i32, [vp]),
    "gmg_frame_score6": (i32, [vp, vp, vp, vp, vp]),
    "gmg_frame_score6_strided": (i32, [vp, vp, vp, vp, u64, vp]),
    "gmg_null_set_upload": (i32, [vp, i32, C.POINTER(vp)]),
    "gmg_null_set_from_tables": (i32, [vp, vp, i32, C.POINTER(vp)]),
    "gmg_null_set_build": (i32, [vp, i32, vp, i32, C.POINTER(vp)]),
    "gmg_null_set_free": (i32, [vp]),
    "gmg_frame_score6_nulls": (i32, [vp, vp, vp, vp, vp, u64, vp]),
    "gmg_segment_frame_score": (i32, [vp, vp, vp, i32, vp, vp]),
    "gmg_segment_cumscore": (i32, [vp, vp, vp, i32, vp, vp]),
    "gmg_score_string": (i32, [vp, vp, vp, i32, vp, vp]),
    "gmg_segment_partial_prob": (i32, [vp, vp, vp, i32, vp, vp]),
    "gmg_all_frame_score": (i32, [vp, vp, vp, vp, vp, vp, vp]),
    "gmg_window_distrib": (i32, [vp, vp, vp, u64, vp, vp, vp]),
    "gmg_mg_score_reads": (i32, [vp, vp, vp, vp, vp, C.POINTER(vp), vp]),
    "gmg_mg_score_groups": (i32, [vp, i32, vp, vp, vp, C.POINTER(vp), vp]),
    "gmg_find_orfs": (i32, [vp, vp, C.POINTER(vp), vp]),
    "gmg_mg_result_info": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
    "gmg_mg_result_fetch": (i32, [vp, vp, vp, vp]),
    "gmg_mg_result_fetch_errors": (i32, [vp, vp]),
    "gmg_mg_result_free": (i32, [vp]),
    "gmg_trim_cache": (i32, []),
    "gmg_debug_owned_blocks": (i32, [C.POINTER(u64)]),
    "gmg_score_reads_strings": (i32, [vp, i32, vp, vp, vp]),
    "gmg_host_register": (i32, [vp, C.c_size_t]),
    "gmg_host_unregister": (i32, [vp]),
    "gmg_fasta_ingest": (i32, [C.c_char_p, u64, C.POINTER(vp), C.POINTER(vp)]),
    "gmg_fasta_ingest_on": (i32, [C.c_char_p, u64, C.POINTER(vp), C.POINTER(vp), vp]),
    "gmg_fasta_split": (i32, [C.c_char_p, u64, u64, vp, i32]),
    "gmg_mg_result_fetch_on": (i32, [vp, vp, vp, vp, vp]),
    "gmg_stream_create": (i32, [C.POINTER(vp)]),
    "gmg_stream_destroy": (i32, [vp]),
    "gmg_fasta_info": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
    "gmg_fasta_headers": (i32, [vp, vp, vp]),
    "gmg_fasta_free": (i32, [vp]),
    "gmg_orfs_upload": (i32, [vp, vp, u64, C.POINTER(u64), C.POINTER(vp)]),
    "gmg_orf_batch_free": (i32, [vp]),
    "gmg_score_orfs": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "gmg_score_orfs_begin": (i32, [vp, vp, vp, vp, vp, C.POINTER(u64), vp]),
    "gmg_score_orfs_fetch": (i32, [vp, vp, vp, vp]),
    "gmg_classes_load": (i32, [C.c_char_p, u64, C.c_char_p, C.POINTER(vp)]),
    "gmg_classes_free": (i32, [vp]),
    "gmg_classes_info": (i32, [vp, C.POINTER(u64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64)]),
    "gmg_classes_icm_file": (C.c_char_p, [vp, C.c_uint32]),
    "gmg_classes_plan": (i32, [vp, vp, vp, u64, vp, vp, vp, vp, C.POINTER(u64)]),
    "gmg_stop_codons_by_code": (i32, [i32, vp, C.POINTER(i32)]),
    "gmg_ignore_score_len": (i32, [C.c_double, vp, i32, C.POINTER(C.c_int32)]),
    "gmg_xlate_table": (i32, [i32, vp]),
    "gmg_entropy_regions": (i32, [vp, vp, u64, vp, vp, vp, vp, vp, vp]),
    "gmg_entropy_orfs": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "gmg_entropy_from_counts": (i32, [vp, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gmg_entropy_default_profiles": (i32, [vp, vp]),
    "gmg_genes_audit": (i32, [vp, vp, u64, vp, vp, u64, C.POINTER(vp), vp]),
    "gmg_audit_info": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
    "gmg_audit_fetch": (i32, [vp, vp, vp, vp]),
    "gmg_audit_free": (i32, [vp]),
    "gmg_window_counts": (i32, [vp, C.c_int64, C.c_int64, vp, u64, C.POINTER(vp), vp]),
    "gmg_windows_info": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
    "gmg_windows_fetch": (i32, [vp, vp, vp]),
    "gmg_windows_device": (i32, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "gmg_windows_free": (i32, [vp]),
    "gmg_regions_uncovered": (i32, [vp, vp, u64, C.c_int64, C.POINTER(vp), vp]),
    "gmg_gaps_info": (i32, [vp, C.POINTER(u64)]),
    "gmg_gaps_fetch": (i32, [vp, vp, vp]),
    "gmg_gaps_free": (i32, [vp]),
    "gmg_uncovered_plan": (i32, [vp, u64, vp, u64, i32, vp, C.POINTER(u64)]),
    "gmg_trainer_create": (i32, [vp, i32, i32, i32, C.POINTER(vp)]),
    "gmg_trainer_level_counts": (i32, [vp, i32, vp, vp]),
    "gmg_trainer_free": (i32, [vp]),
    "gmg_fixed_model_upload": (i32, [i32, vp, vp, vp, vp, vp, C.POINTER(vp)]),
    "gmg_fixed_model_free": (i32, [vp]),
    "gmg_fixed_model_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(u64)]),
    "gmg_fixed_score": (i32, [vp, vp, vp, i32, i32, vp, vp]),
    "gmg_tophits_create": (i32, [vp, i32, C.POINTER(vp)]),
    "gmg_tophits_free": (i32, [vp]),
    "gmg_tophits_update_sums": (i32, [vp, vp, i32, i32, vp, i32, vp]),
    "gmg_tophits_scores": (i32, [vp, vp, i32, i32, vp, i32, vp, C.POINTER(vp)]),
    "gmg_tophits_fetch": (i32, [vp, vp, vp]),
    "gmg_tophits_format_rows": (i32, [vp, vp, i32, i32, vp, C.POINTER(C.c_size_t), vp]),
    "gmg_features_count": (i32, [vp, vp, u64, vp, u64, vp, C.POINTER(vp), vp]),
    "gmg_features_fetch": (i32, [vp, i32, vp]),
    "gmg_features_info": (i32, [vp, C.POINTER(u64), C.POINTER(u64), vp]),
    "gmg_features_free": (i32, [vp]),
    "gmg_fasta_not_upper_acgt": (i32, [C.c_char_p, u64, vp, u64, C.POINTER(u64)]),
    "gmg_features_format": (i32, [vp, C.c_char_p, i32, i32, vp, C.POINTER(C.c_size_t)]),
    "gmg_device_malloc": (i32, [C.POINTER(vp), C.c_size_t]),
    "gmg_device_free": (i32, [vp]),
    "gmg_memcpy_h2d": (i32, [vp, vp, C.c_size_t, vp]),
    "gmg_memcpy_d2h": (i32, [vp, vp, C.c_size_t, vp]),
    # include/gmg_icm.h
    "gmg_icm_new": (i32, [i32, i32, i32, C.POINTER(vp)]),
    "gmg_icm_train": (i32, [C.POINTER(C.c_char_p), i32, i32, i32, i32, C.POINTER(vp)]),
    "gmg_icm_train_reads": (i32, [vp, i32, i32, i32, C.POINTER(vp)]),
    "gmg_icm_open": (i32, [C.c_char_p, C.POINTER(vp)]),
    "gmg_icm_build_indep": (i32, [vp, C.c_double, C.POINTER(C.c_char_p), i32]),
    "gmg_icm_write": (i32, [vp, C.c_char_p]),
    "gmg_icm_free": (i32, [vp]),
    "gmg_icm_params": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "gmg_icm_tables": (i32, [vp, vp, vp]),
    "gmg_icm_device_model": (i32, [vp, C.POINTER(vp)]),
    "gmg_fixed_icm_read": (i32, [C.c_char_p, C.POINTER(vp)]),
    "gmg_fixed_icm_train": (i32, [C.POINTER(C.c_char_p), i32, i32, i32, vp, C.POINTER(vp)]),
    "gmg_fixed_icm_write": (i32, [vp, C.c_char_p, i32]),
    "gmg_fixed_icm_params": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), vp]),
    "gmg_fixed_icm_score": (i32, [vp, C.POINTER(C.c_char_p), i32, i32, i32, vp]),
    "gmg_fixed_icm_device_model": (i32, [vp, C.POINTER(vp)]),
    "gmg_fixed_icm_free": (i32, [vp]),
}

# debug exports: not declared in include/*.h
DEBUG_PROTOTYPES = {
    "gmg_debug_cache_stats": (i32, [vp]),   # out[4]: busy blocks, busy bytes, idle blocks, idle bytes of the device block cache
    "gmg_debug_stall": (i32, [vp, C.c_uint32]),   # (stream, microseconds <= 250 000): one wave that holds the stream back (tests/test_gpu_streams.py)
    "gmg_debug_thread_streams": (i32, [C.POINTER(u64)]),   # live streams + events the library made for host threads (tests/test_gpu_threads.py)
    "gmg_debug_icm_score_string": (i32, [vp, C.c_char_p, i32, i32, C.POINTER(C.c_double)]),   # (gmg_icm, string, len, frame, out): ICM_t::Score_String on the calling thread's staging
}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise RuntimeError("%s is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                               "there is no fallback path" % LIB)
        # GMG_LIB_PATH: a variant build of the same sources (kernel experiments, tools/build_variants.sh); never a fallback
        _lib = C.CDLL(os.environ.get("GMG_LIB_PATH") or LIB)
        for name, (res, args) in list(PROTOTYPES.items()) + list(DEBUG_PROTOTYPES.items()):
            fn = getattr(_lib, name)      # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
    return _lib
