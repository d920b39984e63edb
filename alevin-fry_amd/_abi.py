"""ctypes view of include/afquant.h (struct layouts and prototypes).

Kept separate from the loader so the CPU oracle binding (oracle/oracle.py, test
infrastructure) can share the struct definitions without loading the HIP library.
"""
import ctypes as C

AFQ_ABI_VERSION = 3

AFQ_OK = 0
AFQ_ERR_INVALID_ARG = -1
AFQ_ERR_BAD_INPUT = -2
AFQ_ERR_UNSUPPORTED = -3
AFQ_ERR_HIP = -4
AFQ_ERR_NO_DEVICE = -5
AFQ_ERR_STATE = -6
AFQ_ERR_OOM = -7

# ResolutionStrategy spellings of the CLI (src/quant.rs:98-111 of the reference)
RESOLUTIONS = {
    "trivial": 0,
    "cr-like": 1,
    "cr-like-em": 2,
    "parsimony-em": 3,
    "parsimony": 4,
    "parsimony-gene-em": 5,
    "parsimony-gene": 6,
}

CELL_TINY_PATH = 0x1
CELL_ALT_RES = 0x2
CELL_EMPTY = 0x4


class AfqConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("resolution", C.c_uint32),
        ("sa_model", C.c_uint32),
        ("usa_mode", C.c_uint32),
        ("num_genes", C.c_uint32),
        ("num_rows", C.c_uint32),
        ("small_thresh", C.c_uint32),
        ("large_graph_thresh", C.c_uint32),
        ("pug_exact_umi", C.c_uint32),
        ("em_init_uniform", C.c_uint32),
        ("bc_bytes", C.c_uint32),
        ("umi_bytes", C.c_uint32),
        ("profile", C.c_uint32),
        ("umi_len", C.c_uint32),
        ("dump_eq", C.c_uint32),
        ("bc_split", C.c_uint32),
        ("num_bootstraps", C.c_uint32),
        ("summary_stat", C.c_uint32),
        ("boot_seed", C.c_uint64),
    ]


class AfqResult(C.Structure):
    _fields_ = [
        ("n_cells", C.c_uint64),
        ("first_cell_index", C.c_uint64),
        ("nnz", C.c_uint64),
        ("cell_ptr", C.POINTER(C.c_uint64)),
        ("gene", C.POINTER(C.c_uint32)),
        ("val", C.POINTER(C.c_float)),
        ("bc", C.POINTER(C.c_uint64)),
        ("nrec", C.POINTER(C.c_uint32)),
        ("flags", C.POINTER(C.c_uint8)),
        ("opaque", C.c_void_p),
    ]


class AfqEqclasses(C.Structure):
    _fields_ = [
        ("n_cells", C.c_uint64),
        ("n_classes", C.c_uint64),
        ("n_words", C.c_uint64),
        ("cell_ptr", C.POINTER(C.c_uint64)),
        ("label_ptr", C.POINTER(C.c_uint64)),
        ("labels", C.POINTER(C.c_uint32)),
        ("count", C.POINTER(C.c_uint32)),
    ]


class AfqBootstraps(C.Structure):
    _fields_ = [
        ("n_cells", C.c_uint64),
        ("mean_ptr", C.POINTER(C.c_uint64)), ("mean_col", C.POINTER(C.c_uint32)), ("mean_val", C.POINTER(C.c_float)),
        ("var_ptr", C.POINTER(C.c_uint64)), ("var_col", C.POINTER(C.c_uint32)), ("var_val", C.POINTER(C.c_float)),
    ]


class AfqKernelTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", C.c_double), ("launches", C.c_uint32), ("pad", C.c_uint32)]


class AfqBatchStats(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64),
        ("n_ref_words", C.c_uint64),
        ("n_keys", C.c_uint64),
        ("n_buckets", C.c_uint64),
        ("n_overflow_buckets", C.c_uint64),
        ("input_bytes", C.c_uint64),
        ("n_fallback_cells", C.c_uint64),
    ]


# every symbol include/afquant.h declares (tests check the .so exports them all)
EXPORTS = [
    "afq_create",
    "afq_destroy",
    "afq_submit",
    "afq_submit_device",
    "afq_submit_reader",
    "afq_set_aln_extra_bytes",
    "afq_collect",
    "afq_result_release",
    "afq_result_eqclasses",
    "afq_result_bootstraps",
    "afq_infer",
    "afq_atac_dedup",
    "afq_atac_dedup_rad",
    "afq_atac_sort_rad",
    "afq_atac_sort_limits",
    "afq_atac_sort_leaf_limits",
    "afq_atac_sort_table_slot",
    "afq_gpl_hist_rad",
    "afq_gpl_correct",
    "afq_gpl_limits",
    "afq_gpl_table_slot",
    "afq_atac_gpl_hist_rad",
    "afq_atac_gpl_limits",
    "afq_gpl_multi_hist_rad",
    "afq_gpl_multi_limits",
    "afq_collate_rad",
    "afq_collate_limits",
    "afq_collate_multi_rad",
    "afq_collate_multi_limits",
    "afq_atac_collate_rad",
    "afq_atac_collate_limits",
    "afq_convert_bam_rad",
    "afq_convert_limits",
    "afq_snappy_frame_encode",
    "afq_snappy_limits",
    "afq_snappy_frame_decode_device",
    "afq_snappy_decode_limits",
    "afq_collated_chunk_table",
    "afq_bgzf_inflate_device",
    "afq_inflate_limits",
    "afq_set_collate_compress",
    "afq_device_warmup", "afq_device_pci_bus_id", "afq_label_rehash_count", "afq_pool_regrow_count", "afq_em_resize_count", "afq_mono_cell_count", "afq_resolve_divert_count",
    "afq_em_instance_counts",
    "afq_range_pipeline_counts",
    "afq_free",
    "afq_get_kernel_times",
    "afq_get_batch_stats",
    "afq_last_error",
    "afq_abi_version",
]


class AfqAtacStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_multimapped", C.c_uint64), ("n_not_mapped_pair", C.c_uint64), ("n_distinct", C.c_uint64),
                ("n_deduplicated", C.c_uint64), ("n_long_fragments", C.c_uint64), ("n_fallback_cells", C.c_uint64)]


class AfqAtacSortStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_unmapped", C.c_uint64), ("n_multimapped", C.c_uint64), ("n_uncorrected", C.c_uint64),
                ("n_kept", C.c_uint64), ("n_distinct", C.c_uint64), ("n_long_fragments", C.c_uint64), ("n_repartitioned_bins", C.c_uint64)]


class AfqGplHistStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_compatible", C.c_uint64), ("max_ambig", C.c_uint64), ("n_long_records", C.c_uint64)]


class AfqGplMultiHistStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_compatible", C.c_uint64), ("n_routed", C.c_uint64), ("n_unrouted", C.c_uint64),
                ("n_long_records", C.c_uint64)]


class AfqGplCorrectionStats(C.Structure):
    _fields_ = [("exact_distinct", C.c_uint64), ("exact_reads", C.c_uint64), ("corrected_distinct", C.c_uint64), ("corrected_reads", C.c_uint64),
                ("ambiguous_distinct", C.c_uint64), ("ambiguous_reads", C.c_uint64), ("not_found_distinct", C.c_uint64), ("not_found_reads", C.c_uint64)]


class AfqAtacGplHistStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_unmapped", C.c_uint64), ("n_multimapped", C.c_uint64), ("n_binned", C.c_uint64),
                ("max_ambig", C.c_uint64), ("max_bin", C.c_uint64)]


class AfqAtacGplOpts(C.Structure):
    """afq_atac_gpl_opts of include/afquant_host.h (afq_atac_generate_permit_list)."""
    _fields_ = [("input_dir", C.c_char_p), ("output_dir", C.c_char_p), ("list_file", C.c_char_p), ("min_reads", C.c_uint64), ("rc", C.c_uint32),
                ("num_threads", C.c_uint32), ("frequency", C.c_uint32), ("neighborhood", C.c_uint32), ("conf_num", C.c_uint64), ("conf_den", C.c_uint64),
                ("device", C.c_uint32), ("fill_bytes", C.c_uint64), ("cmdline", C.c_char_p), ("stats_out", C.POINTER(AfqAtacGplHistStats))]


class AfqGplMultiOpts(C.Structure):
    """afq_gpl_multi_opts of include/afquant_host.h (afq_generate_permit_list_multi)."""
    _fields_ = [("input_dir", C.c_char_p), ("output_dir", C.c_char_p), ("expected_ori", C.c_uint32), ("method", C.c_uint32), ("method_count", C.c_uint64),
                ("list_file", C.c_char_p), ("min_reads", C.c_uint64), ("frequency", C.c_uint32), ("neighborhood", C.c_int32), ("conf_num", C.c_uint64),
                ("conf_den", C.c_uint64), ("num_threads", C.c_uint32), ("device", C.c_uint32), ("cmdline", C.c_char_p), ("fill_bytes", C.c_uint64),
                ("sample_bc_list", C.c_char_p), ("sample_correction", C.c_uint32), ("sample_neighborhood", C.c_uint32), ("sample_conf_num", C.c_uint64),
                ("sample_conf_den", C.c_uint64), ("sample_bc_ori", C.c_uint32), ("stats_out", C.POINTER(AfqGplMultiHistStats))]


class AfqCollateStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_compatible", C.c_uint64), ("n_uncorrected", C.c_uint64), ("n_kept", C.c_uint64),
                ("n_alignments_in", C.c_uint64), ("n_alignments_kept", C.c_uint64), ("n_long_records", C.c_uint64), ("out_bytes", C.c_uint64)]


class AfqCollateMultiStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_compatible", C.c_uint64), ("n_unrouted", C.c_uint64), ("n_uncorrected", C.c_uint64), ("n_kept", C.c_uint64),
                ("n_alignments_in", C.c_uint64), ("n_alignments_kept", C.c_uint64), ("n_long_records", C.c_uint64), ("out_bytes", C.c_uint64)]


class AfqCollateMultiOpts(C.Structure):
    """afq_collate_multi_opts of include/afquant_host.h (afq_collate_multi)."""
    _fields_ = [("input_dir", C.c_char_p), ("rad_dir", C.c_char_p), ("num_threads", C.c_uint32), ("compress", C.c_uint32), ("max_records", C.c_uint32),
                ("device", C.c_uint32), ("cmdline", C.c_char_p), ("stats_out", C.POINTER(AfqCollateMultiStats))]


class AfqCollateOpts(C.Structure):
    """afq_collate_opts of include/afquant_host.h (afq_collate, afq_collate_sz)."""
    _fields_ = AfqCollateMultiOpts._fields_[:-1] + [("stats_out", C.POINTER(AfqCollateStats))]


class AfqAtacCollateStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_unmapped", C.c_uint64), ("n_multimapped", C.c_uint64), ("n_uncorrected", C.c_uint64),
                ("n_kept", C.c_uint64), ("n_cells_out", C.c_uint64), ("n_cells_empty", C.c_uint64), ("out_bytes", C.c_uint64)]


class AfqAtacCollateOpts(C.Structure):
    """afq_atac_collate_opts of include/afquant_host.h (afq_atac_collate, afq_atac_collate_sz)."""
    _fields_ = AfqCollateMultiOpts._fields_[:-1] + [("stats_out", C.POINTER(AfqAtacCollateStats))]


class AfqConvertStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_dropped_by_flag", C.c_uint64), ("n_runs", C.c_uint64), ("n_runs_dropped_n", C.c_uint64),
                ("n_runs_written", C.c_uint64), ("n_alignments_in", C.c_uint64), ("n_alignments_written", C.c_uint64), ("n_long_runs", C.c_uint64),
                ("n_chunks", C.c_uint64), ("out_bytes", C.c_uint64)]


class AfqSnappyStats(C.Structure):
    _fields_ = [("n_in", C.c_uint64), ("n_out", C.c_uint64), ("n_blocks", C.c_uint64), ("n_blocks_stored", C.c_uint64),
                ("n_literal_bytes", C.c_uint64), ("n_copies", C.c_uint64)]


class AfqInflateStats(C.Structure):
    _fields_ = [("n_in", C.c_uint64), ("n_out", C.c_uint64), ("n_blocks", C.c_uint64), ("n_blocks_empty", C.c_uint64), ("n_stored", C.c_uint64),
                ("n_fixed", C.c_uint64), ("n_dynamic", C.c_uint64), ("n_literals", C.c_uint64), ("n_copies", C.c_uint64)]


AFQ_CONVERT_INFLATE_ON_DEVICE = 1


class AfqConvertOpts(C.Structure):
    """afq_convert_opts of include/afquant_host.h (afq_convert)."""
    _fields_ = [("bam", C.c_char_p), ("rad_out", C.c_char_p), ("num_threads", C.c_uint32), ("filter_best", C.c_uint32), ("device", C.c_uint32),
                ("stats_out", C.POINTER(AfqConvertStats))]


# afq_gpl_hist_rad's expected_ori, afq_gpl_correct's neighborhood / resolution / decisions
GPL_ORI = {"both": 0, "either": 0, "fw": 1, "rc": 2}
GPL_NEIGHBORHOODS = {"hamming-1": 0, "substitution-or-shift-1": 1, "edit-1": 1}
GPL_RESOLUTIONS = {"unique": 0, "frequency": 1}
GPL_METHODS = {"knee": 0, "expect": 1, "force": 2, "valid_bc": 3, "unfiltered": 4}                 # AFQ_GPL_*
GPL_SAMPLE_CORRECTIONS = {"exact": 0, "unique": 1, "frequency": 2, "1-edit": 3}                     # AFQ_GPL_SAMPLE_*
GPL_SAMPLE_ORI = {"forward": 0, "reverse": 1}
GPL_EXACT, GPL_CORRECTED, GPL_AMBIGUOUS, GPL_NOT_FOUND = 0, 1, 2, 3
GPL_NO_TARGET = 0xFFFFFFFF
