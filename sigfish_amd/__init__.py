"""sigfish_amd -- MI355X-native subsequence-DTW signal-to-reference alignment stage.

The product is the C-ABI shared library (include/sigfish_amd.h, built from sigfish_amd/csrc/ into
sigfish_amd/lib/libsigfish_amd.so).  This package is only a thin ctypes binding used by bench.py and the tests;
it never falls back to a CPU implementation: importing works without a GPU, creating an Aligner does not.
"""
from .api import (END, DTW, EVENT_DTYPE, INV, REF, RNA, RESULT_DTYPE, SESSION_NO_START, SESSION_RESWEEP, SESSION_SPREAD, Aligner, Blow5File, RefModel, SfaError, build_id,
                  detect_events, detect_query_start, paf_row, r2qevent_map, read_fasta, read_kmer_model, sam_row, sam_row_from_map, select_query, session_bytes, version, znormalise, Session,
                  EventStream, session_raw_bytes, SESSION_RAW_INFO_DTYPE, RAW_CALIBRATED, RAW_FULL, RAW_ENDED, RAW_POISONED, RAW_RECALIBRATED, RECAL_AT_END,
                  recal_window, recal_double, auto_start_target, session_auto_bytes, SESSION_AUTO_DTYPE, AUTO_PENDING, AUTO_RESOLVED, AUTO_NO_TARGET,
                  AUTO_NO_EVENT, AUTO_BEYOND_MAX, AUTO_AT_FINAL, session_keep_bytes, session_coverage_bytes, session_group_coverage_bytes, GROUP_COVER_DTYPE, map_offsets, BLOW5_INFLATE, BLOW5_FIELDS, BLOW5_STREAM, PRESS_NONE, PRESS_ZLIB, PRESS_ZSTD, zstd_decompress,
                  TARGET_DTYPE, CLASS_DTYPE, ENRICH, DEPLETE, target_decide, read_targets,
                  REACH_TARGET_DTYPE, REACH_NONE, REACH_BELOW_TRACK, REACH_LEAD_MAX, read_reach_targets, session_reach_bytes,
                  REACH_GROUP_TARGET_DTYPE, read_reach_target_groups, session_group_reach_bytes,
                  GROUP_TARGET_DTYPE, GROUP_BEST_DTYPE, GROUP_HEAD_DTYPE, GROUP_MAX, group_decide, read_target_groups,
                  OPEN_CLASS_DTYPE, open_words, QuotaBook,
                  read_truth, truth_class, truth_edge, truth_group, truth_verdict, truth_group_verdict)
from .realtime import replay, format_line, format_sam_line

__all__ = ["Aligner", "Session", "session_bytes", "session_raw_bytes", "EventStream", "RefModel", "SfaError", "RESULT_DTYPE", "RNA", "DTW", "INV", "REF", "END", "paf_row", "replay", "format_line", "format_sam_line", "session_keep_bytes", "session_coverage_bytes", "session_group_coverage_bytes", "GROUP_COVER_DTYPE",
           "read_fasta", "version", "znormalise",
           "GROUP_TARGET_DTYPE", "GROUP_BEST_DTYPE", "GROUP_HEAD_DTYPE", "GROUP_MAX", "group_decide", "read_target_groups",
           "OPEN_CLASS_DTYPE", "open_words", "QuotaBook",
           "REACH_TARGET_DTYPE", "REACH_NONE", "REACH_BELOW_TRACK", "REACH_LEAD_MAX", "read_reach_targets", "session_reach_bytes",
           "REACH_GROUP_TARGET_DTYPE", "read_reach_target_groups", "session_group_reach_bytes",
           "read_truth", "truth_class", "truth_edge", "truth_group", "truth_verdict", "truth_group_verdict"]
