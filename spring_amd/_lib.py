"""ctypes binding of lib/libspring_reorder_hip.so (C ABI: include/spring_reorder.h)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPRING_AMD_LIB") or os.path.join(HERE, "lib", "libspring_reorder_hip.so")  # env: A/B runs

EXPORTS = [
    "spring_reorder_default_opts", "spring_reorder_last_error", "spring_reorder_trim_pool", "spring_reorder_run", "spring_reorder_create",
    "spring_reorder_destroy", "spring_reorder_load_dna", "spring_reorder_load_dna_device",
    "spring_reorder_build_dict", "spring_reorder_run_chains", "spring_reorder_auto_chains", "spring_reorder_finalize",
    "spring_reorder_mg_begin", "spring_reorder_mg_search", "spring_reorder_mg_slice", "spring_reorder_mg_slices",
    "spring_reorder_mg_apply",
    "spring_reorder_mg_end", "spring_reorder_mg_exchange_virtual", "spring_reorder_debug_check_seed_state",
    "spring_mg_rccl_unique_id", "spring_mg_comm_create_rccl", "spring_mg_comm_create_host", "spring_mg_comm_destroy",
    "spring_reorder_mg_run",
    "spring_reorder_get_stats", "spring_reorder_download", "spring_reorder_tid_split", "spring_reorder_emit_dna",
    "spring_reorder_dict_lookup", "spring_reorder_presence_table", "spring_reorder_download_reads", "spring_synth_dna_bytes",
    "spring_reorder_load_fastq", "spring_reorder_fastq_N",
    "spring_order_invert_se", "spring_order_invert_pe", "spring_order_correct", "spring_order_pe_encode",
    "spring_fastq_reorder",
    "spring_synth_dna_host", "spring_synth_genome_host", "spring_synth_dna_device", "spring_reorder_load_synth", "spring_reorder_download_dna",
    "spring_encoder_create", "spring_encoder_destroy", "spring_encoder_set_split_tables", "spring_encoder_encode_reorder", "spring_encoder_download",
    "spring_encoder_download_seq_packed", "spring_encoder_get_info", "spring_reorder_encode_run", "spring_encoder_encode_host", "spring_encoder_run",
]

# include/spring_streams.h: a list of its own (EXPORTS mirrors spring_reorder.h + spring_encoder.h exactly)
STREAMS_EXPORTS = [
    "spring_streams_create", "spring_streams_destroy", "spring_streams_from_encoder", "spring_streams_from_host",
    "spring_streams_download", "spring_streams_get_info", "spring_streams_run",
]
STREAMS_NUM = 9  # SPRING_STREAMS_NUM

# include/spring_decode.h: a list of its own as well
DECODE_EXPORTS = [
    "spring_decode_create", "spring_decode_destroy", "spring_decode_seq_from_encoder", "spring_decode_seq_from_host",
    "spring_decode_seq_from_files", "spring_decode_from_streams", "spring_decode_from_host", "spring_decode_from_files",
    "spring_decode_download", "spring_decode_get_info",
]

# include/spring_qualid.h: a list of its own as well
QUALID_EXPORTS = [
    "spring_qualid_create", "spring_qualid_destroy", "spring_qualid_order_from_host", "spring_qualid_order_from_encoder",
    "spring_qualid_from_fastq", "spring_qualid_from_lines", "spring_qualid_download", "spring_qualid_get_info",
    "spring_quality_table", "spring_id_pattern",
]

# include/spring_fastq_out.h: a list of its own as well
FASTQ_OUT_EXPORTS = [
    "spring_fastq_out_create", "spring_fastq_out_destroy", "spring_fastq_out_assemble", "spring_fastq_out_download",
    "spring_fastq_out_write", "spring_fastq_out_get_info",
]

# include/spring_gzip.h: a list of its own as well
GZIP_EXPORTS = [
    "spring_gzip_create", "spring_gzip_destroy", "spring_gzip_set_chunk_bytes", "spring_gzip_set_token_bytes",
    "spring_gzip_from_fastq_out", "spring_gzip_from_host", "spring_gzip_download", "spring_gzip_write",
    "spring_gzip_get_info",
]

# include/spring_bwt.h: a list of its own as well
BWT_EXPORTS = [
    "spring_bwt_create", "spring_bwt_destroy", "spring_bwt_set_block_bytes", "spring_bwt_set_workspace_bytes",
    "spring_bwt_workspace_need", "spring_bwt_from_host", "spring_bwt_from_streams", "spring_bwt_download",
    "spring_bwt_segments", "spring_bwt_get_info", "spring_bwt_encode_inplace", "spring_bwt_set_run_keys",
    "spring_bwt_from_qualid", "spring_bwt_round_entries",
]
BWT_MAX_INDEXES = 256  # SPRING_BWT_MAX_INDEXES
BWT_SRC_QUALITY, BWT_SRC_ID = -2, -3  # SPRING_BWT_SRC_QUALITY, SPRING_BWT_SRC_ID

# include/spring_unbwt.h: a list of its own as well
UNBWT_EXPORTS = [
    "spring_unbwt_create", "spring_unbwt_destroy", "spring_unbwt_set_workspace_bytes", "spring_unbwt_workspace_need",
    "spring_unbwt_set_head_spacing", "spring_unbwt_from_host", "spring_unbwt_from_bwt", "spring_unbwt_download",
    "spring_unbwt_get_info", "spring_unbwt_decode_inplace", "spring_unbwt_from_unqlfc",
]
UNBWT_PASSES = 6  # SPRING_UNBWT_PASSES

# include/spring_idcodec.h: a list of its own as well
IDCODEC_EXPORTS = [
    "spring_idcodec_create", "spring_idcodec_destroy", "spring_idcodec_set_workspace_bytes",
    "spring_idcodec_workspace_need", "spring_idcodec_from_qualid", "spring_idcodec_from_host", "spring_idcodec_download",
    "spring_idcodec_symbols", "spring_idcodec_get_info",
]
# include/spring_qlfc.h: a list of its own as well
QLFC_EXPORTS = [
    "spring_qlfc_create", "spring_qlfc_destroy", "spring_qlfc_set_state_tables", "spring_qlfc_set_workspace_bytes",
    "spring_qlfc_workspace_need", "spring_qlfc_from_host", "spring_qlfc_from_bwt", "spring_qlfc_download",
    "spring_qlfc_get_info", "spring_qlfc_compress",
]
QLFC_RANK_TABLE, QLFC_RUN_TABLE = 32768, 8192  # SPRING_QLFC_RANK_TABLE, SPRING_QLFC_RUN_TABLE
QLFC_PASSES = 6                                # SPRING_QLFC_PASSES
QLFC_NOT_COMPRESSIBLE = -16                    # SPRING_QLFC_NOT_COMPRESSIBLE
QLFC_EVENT_BYTES = 160                         # SPRING_QLFC_EVENT_BYTES

# include/spring_unqlfc.h: a list of its own as well
UNQLFC_EXPORTS = [
    "spring_unqlfc_create", "spring_unqlfc_destroy", "spring_unqlfc_set_state_tables", "spring_unqlfc_set_workspace_bytes",
    "spring_unqlfc_workspace_need", "spring_unqlfc_from_host", "spring_unqlfc_from_qlfc", "spring_unqlfc_download",
    "spring_unqlfc_get_info", "spring_unqlfc_decompress",
]
UNQLFC_PASSES = 3                              # SPRING_UNQLFC_PASSES
UNQLFC_MODEL_BYTES = 1619200                   # SPRING_UNQLFC_MODEL_BYTES

# include/spring_bsc.h: a list of its own as well
BSC_EXPORTS = [
    "spring_bsc_create", "spring_bsc_destroy", "spring_bsc_from_streams", "spring_bsc_from_qualid", "spring_bsc_from_host",
    "spring_bsc_download", "spring_bsc_files", "spring_bsc_get_info", "spring_bsc_adler32", "spring_bsc_compress",
]
BSC_HEADER_BYTES = 28                          # SPRING_BSC_HEADER_BYTES
BSC_PASSES = 3                                 # SPRING_BSC_PASSES
BSC_BLOCKS, BSC_FILE, BSC_STR_ARRAY = 0, 1, 2  # framing: SPRING_BSC_BLOCKS, _FILE, _STR_ARRAY
BSC_CODED, BSC_STORED_SMALL, BSC_STORED_CODER, BSC_STORED_NO_GAIN = 0, 1, 2, 3   # block_kind


class Opts(C.Structure):
    _fields_ = [("device", C.c_int32), ("num_chains", C.c_uint32), ("num_thr", C.c_int32),
                ("collect_stats", C.c_int32), ("time_search", C.c_int32), ("force_literal_update", C.c_int32),
                ("rounds_per_sync", C.c_int32), ("long_budget", C.c_int32),
                ("first_shifts", C.c_int32), ("seed_wide", C.c_int32), ("tab_scale", C.c_int32),
                ("search_wpb", C.c_int32), ("dbg_search_lds", C.c_int32), ("dbg_apply_lds", C.c_int32),
                ("fused", C.c_int32), ("deep_bins", C.c_int32),
                ("num_devices", C.c_int32), ("devices", C.c_int32 * 8), ("mg_host_transport", C.c_int32),
                ("table_mode", C.c_int32), ("plan0", C.c_int32 * 6), ("plan1", C.c_int32 * 6), ("long_min", C.c_int32),
                ("long_blocks", C.c_int32), ("debug", C.c_int32), ("long_split", C.c_int32), ("entry_flags", C.c_int32),
                ("out_writers", C.c_int32), ("alternatives", C.c_int32), ("phases", C.c_int32), ("known_absent", C.c_int32),
                ("sort_prefix_bits", C.c_int32), ("dict_build_mode", C.c_int32), ("strand_filter", C.c_int32)]


class Info(C.Structure):
    """What the library reports about a finished call; asdict() gives array fields as lists."""

    def asdict(self):
        d = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            d[k] = list(v) if hasattr(v, "__len__") else v
        return d


class FastqInfo(C.Structure):
    _fields_ = [("num_reads", C.c_uint32 * 2), ("num_reads_clean", C.c_uint32 * 2), ("num_reads_N", C.c_uint32 * 2),
                ("max_readlen", C.c_uint32), ("pad", C.c_uint32), ("ms_device", C.c_double)]


class EncoderInfo(Info):
    _fields_ = ([(k, C.c_uint64) for k in ("n_aligned", "n_total", "seq_len", "noise_bytes", "n_noisepos",
                                           "unaligned_bytes", "len_unaligned", "num_contigs")]
                + [(k, C.c_uint32) for k in ("matched_s", "matched_N", "align_passes", "max_bin")]
                + [("ms_device", C.c_double), ("ms_phase", C.c_double * 8)])


class StreamsInfo(Info):
    _fields_ = ([("num_units", C.c_uint64), ("num_blocks", C.c_uint64), ("bytes", C.c_uint64 * STREAMS_NUM),
                 ("flag_count", C.c_uint64 * 5), ("pos_escapes", C.c_uint64), ("n_aligned", C.c_uint64),
                 ("ms_device", C.c_double), ("ms_file", C.c_double)])


class QualIdInfo(Info):
    _fields_ = [("num_units", C.c_uint64), ("num_blocks", C.c_uint64), ("bytes", C.c_uint64 * 2),
                ("bytes_changed", C.c_uint64), ("max_len", C.c_uint32 * 2), ("ms_device", C.c_double)]


class FastqOutParams(C.Structure):
    _fields_ = ([(k, C.c_uint32) for k in ("first_block", "num_blocks", "num_reads", "num_reads_per_block")]
                + [(k, C.c_int32) for k in ("paired_end", "mate", "preserve_quality", "id_mode", "paired_id_code", "pad")]
                + [("range_start", C.c_uint64), ("range_end", C.c_uint64)])


class FastqOutSources(C.Structure):
    _fields_ = [("decode", C.c_void_p), ("bases", C.c_void_p), ("read_off", C.c_void_p),
                ("quality_ctx", C.c_void_p), ("quality", C.c_void_p), ("quality_bytes", C.c_uint64),
                ("quality_block_off", C.c_void_p),
                ("id_ctx", C.c_void_p), ("ids", C.c_void_p), ("id_bytes", C.c_uint64), ("id_block_off", C.c_void_p)]


class FastqOutInfo(Info):
    _fields_ = [("num_units", C.c_uint64), ("first_slot", C.c_uint64), ("bytes", C.c_uint64),
                ("ms_device", C.c_double), ("ms_file", C.c_double)]


class GzipInfo(Info):
    _fields_ = ([(k, C.c_uint64) for k in ("num_members", "bytes_in", "bytes_out", "chunk_bytes", "num_chunks",
                                           "chunks_stored")]
                + [("ms_device", C.c_double), ("ms_file", C.c_double), ("ms_pass", C.c_double * 6),
                   ("num_batches", C.c_uint64)])


class BwtInfo(Info):
    _fields_ = ([(k, C.c_uint64) for k in ("num_segments", "bytes", "max_segment", "sub_batches", "rounds",
                                           "rounds_total", "workspace_bytes")]
                + [("ms_device", C.c_double), ("ms_pass", C.c_double * 5), ("run_positions", C.c_uint64)])


class UnbwtInfo(Info):
    _fields_ = ([(k, C.c_uint64) for k in ("num_segments", "bytes", "max_segment", "sub_batches", "heads", "head_spacing",
                                           "max_walk", "rank_rounds", "workspace_bytes")]
                + [("ms_device", C.c_double), ("ms_pass", C.c_double * UNBWT_PASSES)])


class IdCodecInfo(Info):
    _fields_ = ([(k, C.c_uint64) for k in ("num_lines", "num_blocks", "num_symbols", "bytes", "max_tokens", "sub_batches")]
                + [("ms_tokens", C.c_double), ("ms_coder", C.c_double)])


class DecodeInfo(Info):
    _fields_ = ([(k, C.c_uint64) for k in ("seq_len", "first_block", "num_blocks", "num_units")]
                + [("bases", C.c_uint64 * 2)]
                + [(k, C.c_uint64) for k in ("n_aligned", "n_unaligned", "pos_escapes")]
                + [("ms_device", C.c_double), ("ms_file", C.c_double)])


class Stats(Info):
    _fields_ = ([(k, C.c_uint64) for k in ("n_reads", "n_matched", "n_single", "unmatched", "probes", "keyok",
                                          "cands", "hits", "iterations", "rounds", "lost")]
                + [("numkeys", C.c_uint64 * 2), ("dict_numreads", C.c_uint64 * 2)]
                + [(k, C.c_double) for k in ("ms_unpack", "ms_dict", "ms_chains", "ms_finalize", "ms_total",
                                             "ms_search_kernel")]
                + [("search_launches", C.c_uint64), ("device_bytes", C.c_uint64),
                   ("ms_exchange", C.c_double), ("ms_resolve_mark", C.c_double), ("chains", C.c_uint64),
                   ("deep_pool", C.c_uint64), ("long_searches", C.c_uint64),
                   ("table_minz", C.c_uint64), ("table_marked_lines", C.c_uint64), ("long_splits", C.c_uint64), ("alternatives", C.c_uint64), ("phases", C.c_uint64),
                   ("ms_search_busy", C.c_double),
                   ("sort_prefix_bits", C.c_uint64), ("sort_repaired_runs", C.c_uint64), ("sort_full_sorts", C.c_uint64),
                   ("sort_long_runs", C.c_uint64), ("sort_list_overflows", C.c_uint64), ("dict_build_path", C.c_uint64),
                   ("strand_filter", C.c_uint64), ("strand_filter_dropped", C.c_uint64),
                   ("strand_filter_build", C.c_uint64)])


# every export returns int (0 or a negative error code) except these
NOT_INT = {"spring_reorder_last_error": C.c_char_p, "spring_synth_dna_bytes": C.c_size_t,
           "spring_reorder_default_opts": None, "spring_reorder_trim_pool": None, "spring_mg_comm_destroy": None}
NOT_INT.update({p + "_destroy": None for p in ("spring_reorder", "spring_encoder", "spring_streams", "spring_decode",
                                               "spring_qualid", "spring_fastq_out", "spring_gzip", "spring_bwt",
                                               "spring_unbwt", "spring_idcodec", "spring_qlfc", "spring_bsc",
                                               "spring_unqlfc")})
NOT_INT.update({p + "_workspace_need": C.c_uint64 for p in ("spring_bwt", "spring_unbwt", "spring_idcodec", "spring_qlfc",
                                                             "spring_unqlfc")})

# spring_mg_allgather_fn (include/spring_reorder.h): host_buf, slice_off, slice_bytes, total_bytes, user -> 0 on success
MG_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p)

_lib = None


def lib():
    """Loads the HIP library; fails loudly if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "spring_amd: %s is missing. Build it with `python -m spring_amd.build` "
            "(or __graft_entry__.build()); there is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u8p = C.c_void_p, C.c_void_p
    L.spring_reorder_default_opts.argtypes = [C.POINTER(Opts)]
    L.spring_reorder_run.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32,
                                     C.POINTER(Opts)]
    L.spring_reorder_create.argtypes = [C.POINTER(vp), C.POINTER(Opts)]
    L.spring_reorder_destroy.argtypes = [vp]
    L.spring_reorder_load_dna.argtypes = [vp, u8p, C.c_size_t, C.c_uint32, C.c_uint32]
    L.spring_reorder_load_dna_device.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int32]
    L.spring_reorder_build_dict.argtypes = [vp]
    L.spring_reorder_run_chains.argtypes = [vp]
    L.spring_reorder_auto_chains.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    L.spring_reorder_finalize.argtypes = [vp]
    L.spring_reorder_mg_begin.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.spring_reorder_mg_search.argtypes = [vp]
    L.spring_reorder_mg_slice.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.spring_reorder_mg_slices.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_uint32)]
    L.spring_reorder_debug_check_seed_state.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64)]
    L.spring_reorder_mg_apply.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint32)]
    L.spring_reorder_mg_end.argtypes = [vp]
    L.spring_reorder_mg_exchange_virtual.argtypes = [C.POINTER(vp), C.c_uint32]
    L.spring_mg_rccl_unique_id.argtypes = [vp]
    L.spring_mg_comm_create_rccl.argtypes = [C.POINTER(vp), C.c_int32, vp, C.c_uint32, C.c_uint32]
    L.spring_mg_comm_create_host.argtypes = [C.POINTER(vp), MG_ALLGATHER_FN, vp, C.c_uint32, C.c_uint32]
    L.spring_mg_comm_destroy.argtypes = [vp]
    L.spring_reorder_mg_run.argtypes = [vp, vp, C.c_uint32]
    L.spring_reorder_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.spring_reorder_download.argtypes = [vp] + [vp] * 8
    L.spring_reorder_tid_split.argtypes = [vp, vp, vp]
    L.spring_reorder_emit_dna.argtypes = [vp, C.c_int32, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.spring_reorder_dict_lookup.argtypes = [vp, C.c_int32, vp, C.c_uint32, vp, vp, C.c_size_t]
    L.spring_reorder_presence_table.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int32)]
    L.spring_reorder_download_reads.argtypes = [vp, vp, vp]
    L.spring_reorder_load_fastq.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(FastqInfo)]
    L.spring_reorder_fastq_N.argtypes = [vp, C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.POINTER(C.c_uint32)]
    L.spring_order_invert_se.argtypes = [vp, C.c_uint32, vp, C.POINTER(C.c_double)]
    L.spring_order_invert_pe.argtypes = [vp, C.c_uint32, vp, C.POINTER(C.c_double)]
    L.spring_fastq_reorder.argtypes = [u8p, C.c_size_t, vp, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_size_t),
                                       C.POINTER(C.c_double)]
    L.spring_order_pe_encode.argtypes = [vp, C.c_uint32, vp, C.POINTER(C.c_double)]
    L.spring_order_correct.argtypes = [vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    L.spring_synth_dna_bytes.argtypes = [C.c_uint32, C.c_uint32]
    L.spring_synth_dna_host.argtypes = [u8p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]
    L.spring_synth_genome_host.argtypes = [u8p, C.c_uint64, C.c_uint64, C.c_uint32]
    L.spring_synth_dna_device.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]
    L.spring_reorder_load_synth.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]
    L.spring_reorder_download_dna.argtypes = [vp, u8p, C.c_size_t]
    L.spring_encoder_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_encoder_destroy.argtypes = [vp]
    L.spring_encoder_encode_reorder.argtypes = [vp, vp, u8p, C.c_uint64, vp, C.c_uint32, C.POINTER(EncoderInfo)]
    L.spring_encoder_download.argtypes = [vp] + [vp] * 9
    L.spring_encoder_download_seq_packed.argtypes = [vp, vp, vp]
    L.spring_encoder_encode_host.argtypes = [vp, C.c_uint32, C.c_int32, vp, u8p, C.c_uint64, vp, vp, vp, vp, vp, u8p,
                                             C.c_uint64, vp, C.c_uint32, u8p, C.c_uint64, vp, C.c_uint32,
                                             C.POINTER(EncoderInfo)]
    L.spring_encoder_run.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32,
                                     C.POINTER(EncoderInfo)]
    L.spring_encoder_get_info.argtypes = [vp, C.POINTER(EncoderInfo)]
    L.spring_reorder_encode_run.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.POINTER(Opts), C.POINTER(EncoderInfo)]
    L.spring_streams_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_streams_destroy.argtypes = [vp]
    L.spring_streams_from_encoder.argtypes = [vp, vp, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32,
                                              C.POINTER(StreamsInfo)]
    L.spring_streams_from_host.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp,
                                           C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(StreamsInfo)]
    L.spring_streams_download.argtypes = [vp, C.c_int32, vp, vp]
    L.spring_streams_get_info.argtypes = [vp, C.POINTER(StreamsInfo)]
    L.spring_streams_run.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32,
                                     C.POINTER(StreamsInfo)]
    L.spring_decode_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_decode_destroy.argtypes = [vp]
    L.spring_decode_seq_from_encoder.argtypes = [vp, vp]
    L.spring_decode_seq_from_host.argtypes = [vp, C.c_int32, vp, vp, vp]
    L.spring_decode_seq_from_files.argtypes = [vp, C.c_char_p, C.c_int32]
    L.spring_decode_from_streams.argtypes = [vp, vp, C.POINTER(DecodeInfo)]
    L.spring_decode_from_host.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                          C.c_uint32, C.POINTER(DecodeInfo)]
    L.spring_decode_from_files.argtypes = [vp, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                           C.c_uint32, C.POINTER(DecodeInfo)]
    L.spring_decode_download.argtypes = [vp, C.c_int32, vp, vp]
    L.spring_decode_get_info.argtypes = [vp, C.POINTER(DecodeInfo)]
    L.spring_qualid_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_qualid_destroy.argtypes = [vp]
    L.spring_qualid_order_from_host.argtypes = [vp, vp, C.c_uint32, C.c_int32]
    L.spring_qualid_order_from_encoder.argtypes = [vp, vp, C.c_uint32, C.c_int32]
    L.spring_qualid_from_fastq.argtypes = [vp, u8p, C.c_size_t, C.c_int32, u8p, C.c_uint32, C.POINTER(QualIdInfo)]
    L.spring_qualid_from_lines.argtypes = [vp, C.c_int32, u8p, C.c_size_t, u8p, C.c_uint32, C.POINTER(QualIdInfo)]
    L.spring_qualid_download.argtypes = [vp, C.c_int32, u8p, vp, vp]
    L.spring_qualid_get_info.argtypes = [vp, C.POINTER(QualIdInfo)]
    L.spring_quality_table.argtypes = [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, u8p]
    L.spring_id_pattern.argtypes = [u8p, C.c_size_t, u8p, C.c_size_t, C.c_int32, C.POINTER(C.c_uint8),
                                    C.POINTER(C.c_double)]
    L.spring_fastq_out_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_fastq_out_destroy.argtypes = [vp]
    L.spring_fastq_out_assemble.argtypes = [vp, C.POINTER(FastqOutParams), C.POINTER(FastqOutSources),
                                            C.POINTER(FastqOutInfo)]
    L.spring_fastq_out_download.argtypes = [vp, u8p, vp]
    L.spring_fastq_out_write.argtypes = [vp, C.c_char_p, C.c_int32, C.POINTER(FastqOutInfo)]
    L.spring_fastq_out_get_info.argtypes = [vp, C.POINTER(FastqOutInfo)]
    L.spring_gzip_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_gzip_destroy.argtypes = [vp]
    L.spring_gzip_set_chunk_bytes.argtypes = [vp, C.c_uint32]
    L.spring_gzip_set_token_bytes.argtypes = [vp, C.c_uint64]
    L.spring_gzip_from_fastq_out.argtypes = [vp, vp, C.c_uint64, C.c_int32, C.POINTER(GzipInfo)]
    L.spring_gzip_from_host.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint64, C.c_int32, C.POINTER(GzipInfo)]
    L.spring_gzip_download.argtypes = [vp, u8p, vp]
    L.spring_gzip_write.argtypes = [vp, C.c_char_p, C.c_int32, C.POINTER(GzipInfo)]
    L.spring_gzip_get_info.argtypes = [vp, C.POINTER(GzipInfo)]
    L.spring_bwt_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_bwt_destroy.argtypes = [vp]
    L.spring_bwt_set_block_bytes.argtypes = [vp, C.c_uint64]
    L.spring_bwt_set_workspace_bytes.argtypes = [vp, C.c_uint64]
    L.spring_bwt_workspace_need.argtypes = [C.c_uint64, C.c_uint64]
    L.spring_bwt_from_host.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint64, C.POINTER(BwtInfo)]
    L.spring_bwt_from_streams.argtypes = [vp, vp, C.c_uint32, C.POINTER(BwtInfo)]
    L.spring_bwt_download.argtypes = [vp, u8p, vp, vp, vp, vp]
    L.spring_bwt_segments.argtypes = [vp, vp, vp, vp]
    L.spring_bwt_get_info.argtypes = [vp, C.POINTER(BwtInfo)]
    L.spring_bwt_encode_inplace.argtypes = [vp, u8p, C.c_int32, vp, vp]
    L.spring_bwt_set_run_keys.argtypes = [vp, C.c_int32, C.c_uint32]
    L.spring_bwt_round_entries.argtypes = [vp, vp, C.c_uint64]
    L.spring_bwt_from_qualid.argtypes = [vp, vp, C.c_int32, C.c_uint64, C.POINTER(BwtInfo)]
    L.spring_unbwt_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_unbwt_destroy.argtypes = [vp]
    L.spring_unbwt_set_workspace_bytes.argtypes = [vp, C.c_uint64]
    L.spring_unbwt_workspace_need.argtypes = [C.c_uint64, C.c_uint64]
    L.spring_unbwt_set_head_spacing.argtypes = [vp, C.c_uint32]
    L.spring_unbwt_from_host.argtypes = [vp, u8p, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(UnbwtInfo)]
    L.spring_unbwt_from_bwt.argtypes = [vp, vp, C.POINTER(UnbwtInfo)]
    L.spring_unbwt_download.argtypes = [vp, u8p, vp]
    L.spring_unbwt_get_info.argtypes = [vp, C.POINTER(UnbwtInfo)]
    L.spring_unbwt_decode_inplace.argtypes = [vp, u8p, C.c_int32, C.c_int32, C.c_uint8, vp]
    L.spring_unbwt_from_unqlfc.argtypes = [vp, vp, vp, C.POINTER(UnbwtInfo)]
    L.spring_idcodec_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_idcodec_destroy.argtypes = [vp]
    L.spring_idcodec_set_workspace_bytes.argtypes = [vp, C.c_uint64]
    L.spring_idcodec_workspace_need.argtypes = [C.c_uint64, C.c_uint64]
    L.spring_idcodec_from_qualid.argtypes = [vp, vp, C.POINTER(IdCodecInfo)]
    L.spring_idcodec_from_host.argtypes = [vp, u8p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(IdCodecInfo)]
    L.spring_idcodec_download.argtypes = [vp, u8p, vp]
    L.spring_idcodec_symbols.argtypes = [vp, vp, vp]
    L.spring_idcodec_get_info.argtypes = [vp, C.POINTER(IdCodecInfo)]
    L.spring_qlfc_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_qlfc_destroy.argtypes = [vp]
    L.spring_qlfc_set_state_tables.argtypes = [vp, u8p, u8p]
    L.spring_qlfc_set_workspace_bytes.argtypes = [vp, C.c_uint64]
    L.spring_qlfc_workspace_need.argtypes = [C.c_uint64, C.c_uint64]
    L.spring_qlfc_from_host.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint64, vp]   # the last: spring_amd.qlfc.QlfcInfo *
    L.spring_qlfc_from_bwt.argtypes = [vp, vp, vp]
    L.spring_qlfc_download.argtypes = [vp, u8p, vp, vp]
    L.spring_qlfc_get_info.argtypes = [vp, vp]
    L.spring_qlfc_compress.argtypes = [vp, u8p, u8p, C.c_int32]
    L.spring_unqlfc_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_unqlfc_destroy.argtypes = [vp]
    L.spring_unqlfc_set_state_tables.argtypes = [vp, u8p, u8p]
    L.spring_unqlfc_set_workspace_bytes.argtypes = [vp, C.c_uint64]
    L.spring_unqlfc_workspace_need.argtypes = [C.c_uint64, C.c_uint64]
    L.spring_unqlfc_from_host.argtypes = [vp, u8p, C.c_uint64, vp, vp, C.c_uint64, vp]   # the last: spring_amd.unqlfc.UnqlfcInfo *
    L.spring_unqlfc_from_qlfc.argtypes = [vp, vp, vp]
    L.spring_unqlfc_download.argtypes = [vp, u8p, vp]
    L.spring_unqlfc_get_info.argtypes = [vp, vp]
    L.spring_unqlfc_decompress.argtypes = [vp, u8p, C.c_int32, u8p, C.c_int32]
    L.spring_bsc_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.spring_bsc_destroy.argtypes = [vp]
    L.spring_bsc_from_streams.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]   # the last: spring_amd.bsc.BscInfo *
    L.spring_bsc_from_qualid.argtypes = [vp, vp, vp, vp, C.c_int32, C.c_uint64, vp]
    L.spring_bsc_from_host.argtypes = [vp, vp, vp, u8p, C.c_uint64, vp, C.c_uint64, C.c_int32, vp, C.c_uint64, vp]
    L.spring_bsc_download.argtypes = [vp, u8p, vp, vp, vp]
    L.spring_bsc_files.argtypes = [vp, vp, vp, vp]
    L.spring_bsc_get_info.argtypes = [vp, vp]
    L.spring_bsc_adler32.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint64, vp]
    L.spring_bsc_compress.argtypes = [vp, vp, vp, u8p, u8p, C.c_int32]
    for name in (EXPORTS + STREAMS_EXPORTS + DECODE_EXPORTS + QUALID_EXPORTS + FASTQ_OUT_EXPORTS + GZIP_EXPORTS
                 + BWT_EXPORTS + UNBWT_EXPORTS + IDCODEC_EXPORTS + QLFC_EXPORTS + UNQLFC_EXPORTS + BSC_EXPORTS):
        getattr(L, name).restype = NOT_INT.get(name, C.c_int)
    _lib = L
    return L
