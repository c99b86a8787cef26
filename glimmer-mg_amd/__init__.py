"""glimmer-mg_amd -- MI355X (gfx950) native IMM scorer for Glimmer-MG.

The product is the C-ABI shared library `lib/libgmg.so` (include/gmg.h, include/gmg_icm.h):
hand-written HIP kernels + the host-side C++ ICM_t.  This Python package is only a ctypes
binding over that ABI for tests and bench.py; it contains no scoring code and no fallback.
"""
from . import build as build            # noqa: F401
from . import capi as capi              # noqa: F401
from . import synth as synth            # noqa: F401
from . import shard as shard            # noqa: F401
from .api import (ModelSet, icm_bytes_info, model_info, model_blob, model_value_stats, Icm, FixedIcm, FixedModel, fixed_score, Reads, NullSet, Segments, Trainer, init, frame_score6, segment_frame_score, segment_cumscore,  # noqa: F401
                  score_string, segment_partial_prob, all_frame_score, window_distrib, score_orfs, find_orfs, mg_score_reads, score_reads_strings, TopHits, GmgError,
                  FORWARD, REVERSED, COMPLEMENTED, REVCOMP, read_fasta, set_option, get_option, option,
                  OrfResult, xlate_table, entropy_default_profiles, entropy_from_counts, entropy_regions, entropy_orfs,
                  fasta_ambiguous, extract_plan, edits_plan, RUN_UP, RUN_DOWN, RUN_SUB_UP, RUN_SUB_DOWN, RUN_LITERAL, RUN_LITERAL_AS_IS, icm_train_reads, EXTRACT_REVERSED, COORD_USE_DIR, COORD_NOWRAP, COORD_SKIP_START, COORD_SKIP_STOP, COORD_MULTI,
                  fasta_not_upper_acgt, FeatureTable, features_format, features_count, FEATURES_BLOCK, FEATURES_LENGTHS, FEATURES_STARTS, FEATURES_ORIENTS,
                  FEATURES_DIST, AUDIT_NEXT_STOP, GENE_AUDIT_DTYPE, audit_params, genes_audit,
                  window_counts, regions_uncovered, uncovered_plan, Letters, text_params, memcpy_d2h,
                  runs_text_params, RUNS_TEXT_DNA, RUNS_TEXT_PROTEIN)
