"""ctypes loader for sigfish_amd/lib/libsigfish_amd.so (the C-ABI in include/sigfish_amd.h)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SFA_LIB") or os.path.join(HERE, "lib", "libsigfish_amd.so")  # SFA_LIB: A/B builds

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)


class SfaRef(C.Structure):
    _fields_ = [("num_ref", C.c_int32), ("ref_lengths", i32p), ("ref_st_offset", i32p),
                ("forward", C.POINTER(f32p)), ("reverse", C.POINTER(f32p))]


class SfaResult(C.Structure):
    _fields_ = [("rid", C.c_int32), ("pos_st", C.c_int32), ("pos_end", C.c_int32), ("score", C.c_float),
                ("score2", C.c_float), ("strand", C.c_int8), ("mapq", C.c_uint8), ("valid", C.c_uint8),
                ("pad", C.c_uint8)]


class SfaProfile(C.Structure):
    _fields_ = [("fill_ms", C.c_double), ("trace_ms", C.c_double), ("finalize_ms", C.c_double),
                ("total_ms", C.c_double), ("cells", C.c_int64), ("fill_launches", C.c_int64),
                ("ckpt_interval", C.c_int64), ("ckpt_bytes", C.c_int64), ("n_tasks", C.c_int64),
                ("n_chunks", C.c_int64), ("n_segments", C.c_int64), ("segment_reruns", C.c_int64),
                ("events_ms", C.c_double), ("normalise_ms", C.c_double), ("non_finite_reads", C.c_int64), ("decode_ms", C.c_double), ("blow5_fallbacks", C.c_int64), ("lds_ckpt", C.c_int64), ("trace_margin", C.c_int64), ("fused_trace", C.c_int64), ("lck_fallbacks", C.c_int64), ("lck_from_scratch", C.c_int64),
                ("class_ms", C.c_double)]


class SfaPlanInfo(C.Structure):
    _fields_ = [("n_quads", C.c_int32), ("n_chunks", C.c_int32), ("n_classes", C.c_int32),
                ("max_rows_per_lane", C.c_int32), ("ckpt_interval", C.c_int32), ("trace_margin", C.c_int32),
                ("ckpt_bytes", C.c_int64), ("n_tasks", C.c_int64), ("max_lanes_per_read", C.c_int32),
                ("lane_widening", C.c_int32)]


class SfaQueryInfo(C.Structure):
    _fields_ = [("n_events", C.c_int64), ("qstart", C.c_int64), ("qend", C.c_int64), ("start_raw_idx", C.c_uint64),
                ("end_raw_idx", C.c_uint64), ("status", C.c_int32), ("pad", C.c_int32)]


class SfaReadHead(C.Structure):
    _fields_ = [("read_id", C.c_char * 128), ("id_len", C.c_int32), ("pad", C.c_int32), ("n_samples", C.c_int64),
                ("digitisation", C.c_double), ("offset", C.c_double), ("range", C.c_double), ("record_bytes", C.c_int64)]


class SfaEvent(C.Structure):
    _fields_ = [("start", C.c_uint64), ("length", C.c_float), ("mean", C.c_float), ("stdv", C.c_float)]


class SfaSessionRawInfo(C.Structure):
    _fields_ = [("n_samples", C.c_int64), ("n_events", C.c_int64), ("q_events", C.c_int64), ("norm_mean", C.c_float),
                ("norm_sd", C.c_float), ("status", C.c_int32), ("norm_window", C.c_int32)]


class SfaTarget(C.Structure):
    _fields_ = [("contig", C.c_int32), ("begin", C.c_int32), ("end", C.c_int32)]


class SfaReachTarget(C.Structure):
    _fields_ = [("contig", C.c_int32), ("begin", C.c_int32), ("end", C.c_int32), ("lead", C.c_int32), ("strand", C.c_int8), ("pad", C.c_int8 * 3)]


class SfaReachGroupTarget(C.Structure):
    _fields_ = [("contig", C.c_int32), ("begin", C.c_int32), ("end", C.c_int32), ("lead", C.c_int32), ("group", C.c_int32), ("strand", C.c_int8),
                ("pad", C.c_int8 * 3)]


class SfaClass(C.Structure):
    _fields_ = [("on_score", C.c_float), ("off_score", C.c_float), ("on_rid", C.c_int32), ("on_pos_end", C.c_int32), ("off_rid", C.c_int32),
                ("off_pos_end", C.c_int32), ("on_strand", C.c_int8), ("off_strand", C.c_int8), ("pad", C.c_int8 * 2), ("n_events", C.c_int32),
                ("valid", C.c_int32)]


class SfaGroupTarget(C.Structure):
    _fields_ = [("contig", C.c_int32), ("begin", C.c_int32), ("end", C.c_int32), ("group", C.c_int32)]


class SfaGroupBest(C.Structure):
    _fields_ = [("score", C.c_float), ("rid", C.c_int32), ("pos_end", C.c_int32), ("strand", C.c_int8), ("pad", C.c_int8 * 3)]


class SfaGroupHead(C.Structure):
    _fields_ = [("best", C.c_int32), ("second", C.c_int32), ("best_score", C.c_float), ("second_score", C.c_float), ("n_events", C.c_int32),
                ("valid", C.c_int32)]


class SfaGroupCover(C.Structure):
    _fields_ = [("columns", C.c_int64), ("capped", C.c_int64), ("depth_sum", C.c_uint64), ("depth_min", C.c_uint32), ("depth_max", C.c_uint32)]


class SfaSessionAuto(C.Structure):
    _fields_ = [("target", C.c_int64), ("frozen_at", C.c_int64), ("skip", C.c_int32), ("status", C.c_int32)]


# every symbol include/sigfish_amd.h declares (checked by tests/test_capi_host.py::test_library_exports_every_declared_symbol)
SYMBOLS = ["sfa_init", "sfa_init_devices", "sfa_n_devices", "sfa_align_batch", "sfa_submit_batch", "sfa_wait_batch", "sfa_align_batch_device", "sfa_align_events", "sfa_align_raw", "sfa_align_raw_ex", "sfa_align_blow5", "sfa_zstd_device", "sfa_inflate_zlib_device", "sfa_decode_blow5_device", "sfa_detect_events_device", "sfa_pinned_alloc", "sfa_pinned_free", "sfa_sync",
           "sfa_get_profile", "sfa_stream", "sfa_set_option", "sfa_plan_batch", "sfa_destroy", "sfa_last_error", "sfa_version", "sfa_build_id", "sfa_gen_ref_record",
           "sfa_znormalise", "sfa_paf_row", "sfa_sam_row", "sfa_paf_row_ex", "sfa_sam_row_ex", "sfa_secondary_rows", "sfa_event_maps", "sfa_sam_row_from_map", "sfa_r2qevent_map", "sfa_detect_events", "sfa_select_query", "sfa_detect_query_start", "sfa_set_pore", "sfa_read_kmer_model",
           "sfa_blow5_open", "sfa_blow5_attr", "sfa_blow5_next", "sfa_blow5_close", "sfa_blow5_select_shard", "sfa_blow5_select_records", "sfa_inflate_zlib", "sfa_inflate_zlib_pair", "sfa_zstd_decompress", "sfa_device_memory",
           "sfa_session_create", "sfa_session_extend", "sfa_session_reset", "sfa_session_lengths", "sfa_session_destroy", "sfa_session_bytes",
           "sfa_event_stream_create", "sfa_event_stream_push", "sfa_event_stream_finish", "sfa_event_stream_destroy",
           "sfa_session_raw_config", "sfa_session_extend_raw", "sfa_session_events", "sfa_session_raw_bytes", "sfa_session_query_span", "sfa_session_row",
           "sfa_session_raw_recalibrate", "sfa_session_candidates_config", "sfa_session_candidates",
           "sfa_session_raw_auto_start", "sfa_session_auto_start", "sfa_session_auto_bytes", "sfa_auto_start_target", "sfa_session_auto_ms",
           "sfa_session_event_maps", "sfa_session_keep_events", "sfa_session_keep_bytes",
           "sfa_session_targets", "sfa_session_target_columns", "sfa_session_classes", "sfa_target_decide",
           "sfa_session_target_groups", "sfa_session_group_count", "sfa_session_group_bests", "sfa_group_decide",
           "sfa_session_open_classes",
           "sfa_session_coverage_config", "sfa_session_coverage_add", "sfa_session_coverage_depth", "sfa_session_coverage_bytes",
           "sfa_session_group_coverage_config", "sfa_session_group_coverage", "sfa_session_group_coverage_bytes",
           "sfa_session_targets_reach", "sfa_session_reach_tables", "sfa_session_reach_bytes",
           "sfa_session_target_groups_reach", "sfa_session_group_reach_tables", "sfa_session_group_reach_bytes",
           "sfa_truth_class", "sfa_truth_edge", "sfa_truth_group", "sfa_truth_verdict", "sfa_truth_group_verdict"]

_lib = None


def load():
    """Load the native library; fails loudly when it has not been built (no fallback of any kind)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C sigfish_amd/csrc` "
                          "(or `python -c 'import __graft_entry__ as g; g.build()'`)")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.sfa_init.argtypes = [C.POINTER(vp), C.POINTER(SfaRef), C.c_uint32, C.c_int]
    L.sfa_init_devices.argtypes = [C.POINTER(vp), C.POINTER(SfaRef), C.c_uint32, C.POINTER(C.c_int), C.c_int]
    L.sfa_n_devices.argtypes = [vp]
    L.sfa_align_batch.argtypes = [vp, f32p, i64p, C.c_int32, vp]
    L.sfa_submit_batch.argtypes = [vp, f32p, i64p, C.c_int32]
    L.sfa_wait_batch.argtypes = [vp, vp, C.c_int32]
    L.sfa_align_batch_device.argtypes = [vp, vp, i64p, C.c_int32, vp, C.c_int]
    L.sfa_align_events.argtypes = [vp, C.POINTER(C.POINTER(SfaEvent)), i64p, i64p, i64p, C.c_int32, vp]
    L.sfa_align_raw.argtypes = [vp, C.POINTER(C.c_int16), i64p, C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_int32, vp, vp]
    L.sfa_align_raw_ex.argtypes = [vp, C.POINTER(C.c_int16), i64p, C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
    L.sfa_align_blow5.argtypes = [vp, vp, i64p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
    L.sfa_inflate_zlib_device.argtypes = [vp, vp, i64p, C.c_int32, vp, i64p, i32p]
    L.sfa_zstd_device.argtypes = [vp, vp, i64p, C.c_int32, vp, i64p, i32p]
    L.sfa_decode_blow5_device.argtypes = [vp, vp, i64p, C.c_int32, C.c_int32, C.c_int32, i32p, vp, i64p, C.POINTER(C.c_int16), C.c_int64]
    L.sfa_detect_events_device.argtypes = [vp, C.POINTER(C.c_int16), i64p, C.POINTER(C.c_double), C.c_int32, vp, i32p, i32p, f32p, f32p]
    L.sfa_pinned_alloc.argtypes = [C.c_size_t]
    L.sfa_pinned_alloc.restype = vp
    L.sfa_pinned_free.argtypes = [vp]
    L.sfa_pinned_free.restype = None
    L.sfa_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.sfa_plan_batch.argtypes = [i64p, C.c_int32, i32p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, i32p, C.POINTER(SfaPlanInfo)]
    L.sfa_sync.argtypes = [vp]
    L.sfa_get_profile.argtypes = [vp, C.POINTER(SfaProfile)]
    L.sfa_stream.argtypes = [vp]
    L.sfa_stream.restype = vp
    L.sfa_destroy.argtypes = [vp]
    L.sfa_destroy.restype = None
    L.sfa_last_error.restype = C.c_char_p
    L.sfa_version.restype = C.c_char_p
    L.sfa_build_id.restype = C.c_char_p
    L.sfa_gen_ref_record.argtypes = [C.c_char_p, C.c_int32, f32p, C.c_uint32, C.c_uint32, C.c_int32, f32p, f32p,
                                     i32p]
    L.sfa_gen_ref_record.restype = C.c_int32
    L.sfa_znormalise.argtypes = [f32p, C.c_uint64]
    L.sfa_znormalise.restype = None
    L.sfa_paf_row.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(SfaResult), C.c_char_p, C.c_char_p, C.c_uint64,
                              C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
    i16p = C.POINTER(C.c_int16)
    L.sfa_sam_row.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(SfaResult), C.c_char_p, C.c_char_p, C.POINTER(SfaEvent),
                              C.c_int64, C.c_int64, f32p, C.c_int32, C.c_int32, C.c_uint32]
    L.sfa_paf_row_ex.argtypes = L.sfa_paf_row.argtypes + [C.c_char]
    L.sfa_sam_row_ex.argtypes = L.sfa_sam_row.argtypes + [C.c_int]
    L.sfa_secondary_rows.argtypes = [vp, vp, C.c_int32]
    L.sfa_event_maps.argtypes = [vp, vp, i32p, C.c_int32, i64p, i32p, i32p]
    L.sfa_sam_row_from_map.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(SfaResult), C.c_char_p, C.c_char_p, C.POINTER(SfaEvent),
                                       C.c_int64, C.c_int64, i32p, C.c_int32, C.c_uint32, C.c_int]
    L.sfa_r2qevent_map.argtypes = [C.POINTER(SfaResult), C.POINTER(SfaEvent), C.c_int64, C.c_int64, f32p, C.c_int32, C.c_int32,
                                   C.c_uint32, i32p, C.c_int32]
    L.sfa_r2qevent_map.restype = C.c_int32
    L.sfa_detect_events.argtypes = [i16p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(SfaEvent),
                                    C.c_int64]
    L.sfa_detect_events.restype = C.c_int64
    L.sfa_select_query.argtypes = [C.POINTER(SfaEvent), C.c_int64, i16p, C.c_int64, C.c_double, C.c_double, C.c_double,
                                   C.c_int32, C.c_int32, C.c_uint32, C.c_int, i64p, i64p]
    L.sfa_detect_query_start.argtypes = [i16p, C.c_int64, C.c_double, C.c_double, C.c_double, C.POINTER(SfaEvent), C.c_int64,
                                         C.c_int]
    L.sfa_detect_query_start.restype = C.c_int64
    L.sfa_set_pore.argtypes = [vp, C.c_int]
    L.sfa_read_kmer_model.argtypes = [C.c_char_p, f32p, C.POINTER(C.c_uint32)]
    L.sfa_blow5_open.argtypes = [C.c_char_p]
    L.sfa_blow5_open.restype = vp
    L.sfa_blow5_attr.argtypes = [vp, C.c_char_p]
    L.sfa_blow5_attr.restype = C.c_char_p
    L.sfa_blow5_next.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(i16p), i64p]
    L.sfa_blow5_close.argtypes = [vp]
    L.sfa_blow5_close.restype = None
    L.sfa_blow5_select_shard.argtypes = [vp, C.c_int32, C.c_int32]
    L.sfa_blow5_select_records.argtypes = [vp, C.c_int64, C.c_int64]
    L.sfa_inflate_zlib.argtypes = [C.c_char_p, C.c_size_t, vp, C.c_size_t]
    L.sfa_inflate_zlib_pair.restype = C.c_int
    L.sfa_inflate_zlib_pair.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, i64p]
    L.sfa_inflate_zlib.restype = C.c_int64
    L.sfa_zstd_decompress.argtypes = [C.c_char_p, C.c_size_t, vp, C.c_size_t]
    L.sfa_zstd_decompress.restype = C.c_int64
    L.sfa_device_memory.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sfa_session_create.argtypes = [vp, C.c_int32, C.c_uint32, C.POINTER(vp)]
    L.sfa_session_extend.argtypes = [vp, i32p, f32p, i64p, C.c_int32, vp]
    L.sfa_session_reset.argtypes = [vp, i32p, C.c_int32]
    L.sfa_session_lengths.argtypes = [vp, i32p, C.c_int32, i64p]
    L.sfa_session_destroy.argtypes = [vp]
    L.sfa_session_destroy.restype = None
    L.sfa_session_row.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, f32p, i32p]
    L.sfa_session_row.restype = C.c_int64
    L.sfa_session_candidates_config.argtypes = [vp, C.c_int32]
    L.sfa_session_candidates.argtypes = [vp, i32p, C.c_int32, vp]
    L.sfa_session_bytes.argtypes = [C.c_int64, C.c_int32, C.c_uint32]
    L.sfa_session_bytes.restype = C.c_int64
    L.sfa_event_stream_create.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int]
    L.sfa_event_stream_create.restype = vp
    L.sfa_event_stream_push.argtypes = [vp, i16p, C.c_int64, C.POINTER(SfaEvent), C.c_int64]
    L.sfa_event_stream_push.restype = C.c_int64
    L.sfa_event_stream_finish.argtypes = [vp, C.POINTER(SfaEvent), C.c_int64]
    L.sfa_event_stream_finish.restype = C.c_int64
    L.sfa_event_stream_destroy.argtypes = [vp]
    L.sfa_event_stream_destroy.restype = None
    L.sfa_session_raw_config.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.sfa_session_raw_recalibrate.argtypes = [vp, i32p, C.c_int32, C.c_uint32]
    L.sfa_session_extend_raw.argtypes = [vp, i32p, i16p, i64p, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_int32, vp, vp]
    L.sfa_session_events.argtypes = [vp, C.c_int32, C.c_int64, C.POINTER(SfaEvent), C.c_int64]
    L.sfa_session_events.restype = C.c_int64
    L.sfa_session_raw_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.sfa_session_raw_bytes.restype = C.c_int64
    L.sfa_session_query_span.argtypes = [vp, i32p, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sfa_session_raw_auto_start.argtypes = [vp, C.c_int32, C.c_int32, C.c_uint32]
    L.sfa_session_auto_start.argtypes = [vp, i32p, C.c_int32, vp]
    L.sfa_session_auto_bytes.argtypes = [C.c_int32, C.c_int32]
    L.sfa_session_auto_bytes.restype = C.c_int64
    L.sfa_auto_start_target.argtypes = [i16p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int]
    L.sfa_auto_start_target.restype = C.c_int64
    L.sfa_session_auto_ms.argtypes = [vp]
    L.sfa_session_auto_ms.restype = C.c_double
    L.sfa_session_event_maps.argtypes = [vp, vp, i32p, C.c_int32, i64p, i32p, i32p]
    L.sfa_session_keep_events.argtypes = [vp, C.c_int32]
    L.sfa_session_keep_bytes.argtypes = [C.c_int32, C.c_int32]
    L.sfa_session_keep_bytes.restype = C.c_int64
    L.sfa_session_targets.argtypes = [vp, C.POINTER(SfaTarget), C.c_int32]
    L.sfa_session_target_columns.argtypes = [vp]
    L.sfa_session_target_columns.restype = C.c_int64
    L.sfa_session_classes.argtypes = [vp, i32p, C.c_int32, vp]
    L.sfa_target_decide.argtypes = [C.POINTER(SfaClass), C.c_int32, C.c_int32, C.c_float]
    L.sfa_session_target_groups.argtypes = [vp, C.POINTER(SfaGroupTarget), C.c_int32, C.c_int32]
    L.sfa_session_group_count.argtypes = [vp]
    L.sfa_session_group_count.restype = C.c_int32
    L.sfa_session_group_bests.argtypes = [vp, i32p, C.c_int32, vp, vp]
    L.sfa_group_decide.argtypes = [C.POINTER(SfaGroupHead), C.c_int32, C.c_float]
    L.sfa_session_open_classes.argtypes = [vp, i32p, C.c_int32, C.POINTER(C.c_uint32), C.c_int32, vp]
    L.sfa_session_coverage_config.argtypes = [vp, C.c_int32]
    L.sfa_session_coverage_add.argtypes = [vp, C.POINTER(SfaTarget), C.c_int32, i64p]
    L.sfa_session_coverage_depth.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint32), C.c_int32]
    L.sfa_session_coverage_bytes.argtypes = [C.POINTER(SfaRef), C.c_int]
    L.sfa_session_coverage_bytes.restype = C.c_size_t
    L.sfa_session_group_coverage_config.argtypes = [vp, C.c_int32]
    L.sfa_session_group_coverage.argtypes = [vp, C.POINTER(SfaGroupCover), C.c_int32]
    L.sfa_session_group_coverage_bytes.argtypes = [C.POINTER(SfaRef), C.c_int, C.c_int32]
    L.sfa_session_group_coverage_bytes.restype = C.c_size_t
    L.sfa_session_targets_reach.argtypes = [vp, C.POINTER(SfaReachTarget), C.c_int32]
    L.sfa_session_reach_tables.argtypes = [vp, C.POINTER(C.c_uint32), C.c_size_t, i32p, C.c_int64]
    L.sfa_session_reach_bytes.argtypes = [C.POINTER(SfaRef), C.c_int]
    L.sfa_session_reach_bytes.restype = C.c_size_t
    L.sfa_session_target_groups_reach.argtypes = [vp, C.POINTER(SfaReachGroupTarget), C.c_int32, C.c_int32]
    L.sfa_session_group_reach_tables.argtypes = [vp, C.POINTER(C.c_uint16), i32p, C.c_int64]
    L.sfa_session_group_reach_bytes.argtypes = [C.POINTER(SfaRef), C.c_int]
    L.sfa_session_group_reach_bytes.restype = C.c_size_t
    L.sfa_truth_class.argtypes = L.sfa_truth_edge.argtypes = [C.POINTER(SfaTarget), C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.sfa_truth_group.argtypes = [C.POINTER(SfaGroupTarget), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.sfa_truth_group.restype = C.c_int32
    L.sfa_truth_verdict.argtypes = [C.c_int, C.c_int]
    L.sfa_truth_group_verdict.argtypes = [C.c_int32, C.c_int32]
    _lib = L
    return L
