"""ctypes binding of libbramble_amd.so (C ABI: include/bramble_amd.h).

The projection path is HIP only: if the shared library is missing, or no HIP
device is usable, every call raises -- there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbramble_amd.so")
_P = C.POINTER

K_SEGMENT, K_COUNT, K_EMIT, K_PAIR_COUNT, K_PAIR_EMIT, K_GATHER, K_SCAN, K_EMIT_AUX, K_KSW, K_BAM, K_PARSE, K_CODEC, K_EMIT_SIMPLE, K_PRIMARY, K_CIGAR_POOL, K_COUNT_WALK, K_EXPAND, K_GROUP_IDS, K_P1, K_P1_WALK, K_EMIT_WL, K_NAME_SEED, K_PAIR_MASK, K_PAIR_BIG, K_GROUP_DESC, K_EXPAND_ROWS, K_EMIT_ROWS_SIMPLE, K_EMIT_ROWS, K_BIG_EMIT, K_SAM_FORMAT, K_NUM = range(31)
KERNEL_NAMES = ["k_segment", "k_project<G,false,false,1>", "k_emit_dense<false,2>", "k_pair<false>", "k_pair<true>",
                "k_rows", "k_scan_*", "k_project<64,true>", "k_ksw", "k_bam_scan+k_bam_size+k_bam_encode",
                "k_rec_fields+k_group_off+k_rec_copy+k_mates+k_seq_*", "k_deflate_*+k_bgzf_compact",
                "k_emit_dense<false,1>", "k_primary", "(unused)", "k_project<G,false,false,2>", "k_expand", "k_group_ids",
                "(unused)", "(unused)", "(unused)", "k_name_seed", "k_pair_mask", "k_big<0>+k_pair_big", "k_group_desc",
                "k_expand_rows", "k_emit_rows<1>", "k_emit_rows<2>", "k_big<1>", "k_samfmt_*"]


class BrambleError(RuntimeError):
    pass


class BrExon(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32)]


class BrTranscript(C.Structure):
    _fields_ = [("id", C.c_char_p), ("seqname", C.c_char_p), ("strand", C.c_char),
                ("exons", _P(BrExon)), ("n_exons", C.c_uint32)]


class BrFastaSeq(C.Structure):
    _fields_ = [("name", C.c_char_p), ("seq", C.c_char_p), ("len", C.c_uint64)]


class BrConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("lr", "lr_hq", "strict", "use_fasta", "fr", "rf", "has_max_clip", "has_max_junc_ins",
                 "has_max_junc_gap", "has_sim_thr", "has_max_error_exon")] + \
               [(n, C.c_uint32) for n in ("max_clip", "max_junc_ins", "max_junc_gap", "max_error_exon")] + \
               [("sim_thr", C.c_float), ("junc_miss_discount", C.c_double)]


class BrThresholds(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("max_clip", "max_junc_ins", "max_junc_gap", "max_error_exon")] + \
               [("ignore_small_exons", C.c_int32), ("filter_by_similarity", C.c_int32),
                ("similarity_threshold", C.c_float)]


class BrBatch(C.Structure):
    _fields_ = [("n_aln", C.c_int64), ("ref_id", C.c_void_p), ("ref_start", C.c_void_p), ("flags", C.c_void_p),
                ("xs", C.c_void_p), ("ts", C.c_void_p), ("cigar_off", C.c_void_p), ("cigar", C.c_void_p),
                ("mate_ref_id", C.c_void_p), ("mate_start", C.c_void_p), ("name_off", C.c_void_p),
                ("names", C.c_void_p), ("seq_off", C.c_void_p), ("seqs", C.c_void_p), ("l_qseq", C.c_void_p)]


_ROW_FIELDS = [("input_index", np.int32), ("transcript_id", np.uint32), ("pos", np.uint32), ("strand", np.int8),
               ("cigar_off", np.uint64), ("cigar", np.uint32), ("similarity_score", np.float64),
               ("clip_score", np.int32), ("junc_hits", np.int32), ("aligned_len", np.int32),
               ("nh", np.uint32), ("hi", np.uint32), ("mapq", np.uint32)]
_ROW_TAIL = [("is_paired", np.uint8), ("same_transcript_as_mate", np.uint8), ("is_first", np.uint8),
             ("mate_transcript_id", np.int32), ("mate_pos", np.int32), ("insert_size", np.int32),
             ("group", np.uint32)]
_COUNTERS = [("total_complete", C.c_uint64), ("total_unique", C.c_uint64), ("dropped_reads", C.c_uint64),
             ("total_processed", C.c_uint64)]


class BrRows(C.Structure):
    _fields_ = [("n_rows", C.c_int64)] + [(n, C.c_void_p) for n, _ in _ROW_FIELDS] + \
               [("is_primary", C.c_void_p)] + [(n, C.c_void_p) for n, _ in _ROW_TAIL] + _COUNTERS


class BrDeviceBatch(C.Structure):
    _fields_ = [("n_aln", C.c_int64), ("n_groups", C.c_int64), ("ref_id", C.c_void_p), ("ref_start", C.c_void_p),
                ("flags", C.c_void_p), ("xs", C.c_void_p), ("ts", C.c_void_p), ("cigar_off", C.c_void_p),
                ("cigar", C.c_void_p), ("mate_idx", C.c_void_p), ("group_off", C.c_void_p), ("l_qseq", C.c_void_p),
                ("seq_off", C.c_void_p), ("seqs", C.c_void_p), ("n_cigar_words", C.c_int64),
                ("max_n_cigar", C.c_int32), ("seq_src", C.c_void_p), ("max_soft_clip", C.c_int32),
                ("name_off", C.c_void_p), ("names", C.c_void_p)]


class BrDeviceRows(C.Structure):
    """Packed rows (ABI version 2): a = {tid, pos, meta, nh}, cigar = inline ops or pool offset, x = {input, junc_hits,
    aligned_len, hi}."""
    _fields_ = [("n_rows", C.c_int64), ("n_matches", C.c_int64), ("n_pool_words", C.c_int64),
                ("a", C.c_void_p), ("cigar", C.c_void_p), ("x", C.c_void_p), ("similarity_score", C.c_void_p),
                ("clip_score", C.c_void_p), ("pool", C.c_void_p), ("row_off", C.c_void_p)] + _COUNTERS


class BrDeviceWideRows(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("n_cigar_words", C.c_int64)] + \
               [(n, C.c_void_p) for n, _ in _ROW_FIELDS] + [(n, C.c_void_p) for n, _ in _ROW_TAIL] + \
               [("is_primary", C.c_void_p)]


class BrAlignment(C.Structure):  # br_alignment = GenomicAlignment (bramble-rs/src/api.rs:73-126)
    _fields_ = [("query_name", C.c_char_p), ("ref_id", C.c_int32), ("ref_start", C.c_int64),
                ("is_reverse", C.c_uint8), ("is_paired", C.c_uint8), ("is_first_in_pair", C.c_uint8),
                ("mate_is_unmapped", C.c_uint8), ("xs_strand", C.c_char), ("ts_strand", C.c_char),
                ("hit_index", C.c_int32), ("mate_ref_id", C.c_int32), ("mate_ref_start", C.c_int64),
                ("cigar", C.c_void_p), ("n_cigar", C.c_uint32), ("sequence", C.c_char_p), ("sequence_len", C.c_uint32),
                ("read_len", C.c_uint32)]


class BrProjected(C.Structure):  # br_projected = ProjectedAlignment (api.rs:135-176) + mapq + rewritten CIGAR
    _fields_ = [("transcript_id", C.c_uint32), ("transcript_start", C.c_uint32), ("transcript_end", C.c_uint32),
                ("aligned_len", C.c_uint32), ("query_aligned_len", C.c_uint32), ("is_reverse", C.c_uint8),
                ("transcript_strand", C.c_char), ("similarity_score", C.c_double), ("nh", C.c_uint32), ("hi", C.c_uint32), ("is_primary", C.c_uint8),
                ("same_transcript_as_mate", C.c_uint8), ("is_paired_out", C.c_uint8), ("insert_size", C.c_int32),
                ("input_index", C.c_uint64), ("mapq", C.c_uint32), ("cigar", _P(C.c_uint32)), ("n_cigar", C.c_uint32)]


class BrHostRows(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("n_aln", C.c_int64), ("n_groups", C.c_int64), ("n_pool_words", C.c_int64),
                ("a", C.c_void_p), ("cigar", C.c_void_p), ("pool", C.c_void_p), ("row_off", C.c_void_p),
                ("mate_idx", C.c_void_p), ("x", C.c_void_p), ("similarity_score", C.c_void_p),
                ("clip_score", C.c_void_p)] + _COUNTERS


ROW_MINUS, ROW_PAIRED, ROW_SAME_TX, ROW_FIRST, ROW_PRIMARY = 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28


class BrDeviceRecords(C.Structure):
    _fields_ = [("blob", C.c_void_p), ("rec_off", C.c_void_p), ("n_aln", C.c_int64), ("rec_len", C.c_void_p)]


class BrBamBundle(C.Structure):
    _fields_ = [("blob", C.c_void_p), ("n_bytes", C.c_uint64), ("rec_off", C.c_void_p), ("rec_len", C.c_void_p),
                ("n_records", C.c_int64), ("ref_map", C.c_void_p), ("n_ref_map", C.c_int32), ("bgzf_on_device", C.c_int32)]


OUT_SAM_TEXT = 2   # br_bam_bundle.bgzf_on_device / br_project_bam_resident: SAM lines instead of records or BGZF blocks
OUT_RESIDENT = 3    # BR_OUT_RESIDENT: the projected records stay in HBM (br_ctx_last_device_bam)

BGZF_BLOCK = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("clen", "<u4"), ("ulen", "<u4"), ("crc", "<u4"), ("pad", "<u4")])


def bgzf_scan(data, cap=None):
    """br_bgzf_scan over a numpy uint8 array of BGZF bytes: (block table, bytes consumed, inflated bytes)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cap = int(cap) if cap is not None else data.size // 28 + 1
    blocks = np.zeros(cap, dtype=BGZF_BLOCK)
    n, consumed, total = C.c_int64(), C.c_uint64(), C.c_uint64()
    L = lib()
    L.br_bgzf_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_void_p, _P(C.c_int64), _P(C.c_uint64), _P(C.c_uint64)]
    check(L.br_bgzf_scan(data.ctypes.data, data.size, cap, blocks.ctypes.data, C.byref(n), C.byref(consumed), C.byref(total)), "br_bgzf_scan")
    return blocks[:n.value], int(consumed.value), int(total.value)


class BrHostBam(C.Structure):
    _fields_ = [("data", C.c_void_p), ("n_bytes", C.c_uint64), ("n_rows", C.c_int64)] + _COUNTERS


class BrDeviceBam(C.Structure):
    _fields_ = [("data", C.c_void_p), ("n_bytes", C.c_uint64), ("row_off", C.c_void_p), ("n_rows", C.c_int64)]


KT_NONE = 0xffffffff   # Context.direct_tidwords: base of an alignment without a tid word (kernels.h)
# the pairing flags per alignment that Context.direct_diag returns (kernels.h)
PF_PAIRED, PF_SAME, PF_MATE, PF_BIG = 1, 2, 4, 8

# every symbol include/bramble_amd.h declares
EXPORTS = ["br_index_build", "br_index_build_flat", "br_index_free", "br_index_num_transcripts", "br_index_transcript_name",
           "br_index_transcript_len", "br_index_num_refs", "br_index_num_intervals", "br_index_device_bytes", "br_config_short_read",
           "br_config_long_read", "br_config_resolve", "br_batch_prepare", "br_batch_seq_source", "br_ctx_new", "br_ctx_free",
           "br_project_batch", "br_project_batch_device", "br_device_rows_expand", "br_batch_stage", "br_project_staged", "br_host_rows_wait", "br_project_batch_packed",
           "br_pin_host", "br_unpin_host", "br_project_group", "br_project_groups", "br_bam_encode_device", "br_project_bam_device", "br_project_bam_bundle", "br_bam_bundle_stage", "br_project_bam_staged", "br_bam_split", "br_annotation_load", "br_annotation_load_mt", "br_annotation_free",
           "br_annotation_num_transcripts", "br_annotation_transcripts", "br_annotation_num_refs", "br_annotation_refnames", "br_annotation_gene_ids", "br_cli_main", "br_cli_exit_at_end", "br_device_warmup", "br_project_bam_staged_nowait", "br_host_bam_wait", "br_bgzf_scan", "br_bgzf_inflate_device", "br_bam_split_device", "br_bam_reader_new", "br_bam_reader_next", "br_bam_reader_set_piece_blocks", "br_bam_reader_release", "br_bam_reader_free", "br_bam_piece_upload", "br_bam_piece_process", "br_bam_reader_seconds", "br_bam_reader_upload_seconds", "br_project_bam_resident", "br_bgzf_write_file", "br_bgzf_read_file",
           "br_ctx_set_sam_refs", "br_sam_format_device",
           "br_sam_header_scan", "br_sam_reader_new", "br_sam_reader_next", "br_sam_reader_upload", "br_sam_reader_next_staged", "br_sam_reader_release", "br_sam_reader_free", "br_sam_reader_error", "br_sam_reader_stats",
           "br_collator_new", "br_collator_add", "br_collator_finish", "br_collator_next", "br_collator_order", "br_collator_set_param",
           "br_collator_stats", "br_collator_free",
           "br_sorter_new", "br_sorter_set_param", "br_sorter_add", "br_sorter_finish", "br_sorter_next", "br_sorter_order", "br_sorter_stats",
           "br_sorter_index", "br_sorter_free", "br_ctx_last_device_bam", "br_device_bam_download",
           "br_ctx_unprojected_stats", "br_ctx_unprojected_next", "br_ctx_unprojected_reset",
           "br_quant_new", "br_quant_set_param", "br_quant_set_tolerance", "br_quant_set_vb_prior", "br_quant_digamma", "br_quant_add", "br_quant_add_rows", "br_quant_add_last", "br_quant_finish",
           "br_quant_classes", "br_quant_em", "br_quant_result", "br_quant_fld", "br_quant_eff_lengths", "br_quant_stats", "br_quant_free",
           "br_quant_bootstrap", "br_quant_boot_counts", "br_quant_boot_theta", "br_quant_boot_summary", "br_quant_boot_stats",
           "br_quant_genes", "br_quant_gene_classes", "br_quant_gene_result", "br_quant_gene_boot", "br_quant_gene_boot_summary", "br_quant_gene_stats",
           "br_quant_name_classes", "br_quant_posteriors",
           "br_coverage_new", "br_coverage_set_param", "br_coverage_add_rows", "br_coverage_add_last", "br_coverage_finish", "br_coverage_runs",
           "br_coverage_depth", "br_coverage_summary", "br_coverage_stats", "br_coverage_free",
           "br_coverage_add_names", "br_coverage_finish_em", "br_coverage_runs64", "br_coverage_depth64", "br_coverage_summary64",
           "br_coverage_bigwig", "br_coverage_bigwig_read", "br_coverage_bigwig_stats", "br_zlib_sections_device",
           "br_assign_new", "br_assign_set_param", "br_assign_add", "br_assign_add_last", "br_assign_finish", "br_assign_values", "br_assign_next",
           "br_assign_stats", "br_assign_free",
           "br_dedup_new", "br_dedup_set_param", "br_dedup_add", "br_dedup_add_last", "br_dedup_finish", "br_dedup_umis", "br_dedup_result",
           "br_dedup_hist", "br_dedup_flags", "br_dedup_next", "br_dedup_stats", "br_dedup_free", "br_quant_drop_names",
           "br_cells_new", "br_cells_set_param", "br_cells_set_tolerance", "br_cells_add", "br_cells_add_last", "br_cells_barcodes", "br_cells_finish",
           "br_cells_cell_barcodes", "br_cells_name_cells", "br_cells_matrix", "br_cells_cell_stats", "br_cells_stats", "br_cells_free",
           "br_whitelist_new", "br_whitelist_barcodes", "br_whitelist_match", "br_whitelist_stats", "br_whitelist_free", "br_cells_set_whitelist",
           "br_dedup_set_whitelist", "br_cells_name_status", "br_cells_whitelist_stats", "br_dedup_whitelist_stats",
           "br_cellcall_new", "br_cellcall_set_param", "br_cellcall_set_real", "br_cellcall_run", "br_cellcall_calls", "br_cellcall_ambient",
           "br_cellcall_logtable", "br_cellcall_candidates", "br_cellcall_wanted", "br_cellcall_sims", "br_cellcall_stats", "br_cellcall_sgt",
           "br_cellcall_free", "br_cells_call", "br_cells_matrix_called",
           "br_free_buffer", "br_bgzf_codec", "br_bgzf_deflate_device", "br_ctx_set_profiling",
           "br_ctx_set_param", "br_ctx_kernel_ms", "br_ctx_kernel_ms_sum", "br_ctx_collect_counters", "br_ctx_last_counters", "br_ctx_direct_diag", "br_ctx_direct_tidwords", "br_ctx_rescue_stats", "br_ctx_ksw_diag", "br_device_rows_detail", "br_ctx_ksw_pairs", "br_primary_pick", "br_row_mapq", "br_version", "br_strerror"]

_LIB = None


def bam_split(data, cap=None):
    """Host walk of the block_size chain: numpy uint8 alignment section -> (rec_off uint64[n], rec_len uint32[n],
    n_unmapped, consumed bytes); unmapped records are skipped."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cap = int(cap if cap is not None else max(data.size // 36 + 1, 1))
    off = np.zeros(cap, dtype=np.uint64)
    ln = np.zeros(cap, dtype=np.uint32)
    n, un, used = C.c_int64(), C.c_int64(), C.c_uint64()
    check(lib().br_bam_split(data.ctypes.data, data.size, cap, off.ctypes.data, ln.ctypes.data, C.byref(n), C.byref(un),
                             C.byref(used)), "br_bam_split")
    return off[:n.value].copy(), ln[:n.value].copy(), un.value, used.value


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise BrambleError("libbramble_amd.so is not built (run __graft_entry__.build() or "
                               "`make -C bramble_amd/csrc`); there is no CPU fallback for the projection path")
        # One HIP runtime per process: torch bundles its own libamdhip64 (same SONAME as
        # /opt/rocm's).  Importing torch first makes libbramble_amd.so bind to that copy,
        # so torch tensors' device pointers and streams are valid for our launches; two
        # runtimes side by side leave the second one without a usable device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.br_index_build.argtypes = [_P(BrTranscript), C.c_size_t, _P(C.c_char_p), C.c_size_t, _P(BrFastaSeq),
                                     C.c_size_t, C.c_int, _P(C.c_void_p)]
        L.br_index_build_flat.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, _P(BrFastaSeq), C.c_int, _P(C.c_void_p)]
        L.br_index_free.argtypes = [C.c_void_p]
        L.br_index_num_transcripts.restype = C.c_size_t
        L.br_index_num_transcripts.argtypes = [C.c_void_p]
        L.br_index_transcript_name.restype = C.c_char_p
        L.br_index_transcript_name.argtypes = [C.c_void_p, C.c_uint32]
        L.br_index_transcript_len.restype = C.c_int64
        L.br_index_transcript_len.argtypes = [C.c_void_p, C.c_uint32]
        L.br_index_num_intervals.restype = C.c_size_t
        L.br_index_num_intervals.argtypes = [C.c_void_p]
        L.br_index_device_bytes.restype = C.c_size_t
        L.br_index_device_bytes.argtypes = [C.c_void_p]
        L.br_config_short_read.argtypes = [_P(BrConfig)]
        L.br_config_long_read.argtypes = [_P(BrConfig)]
        L.br_config_resolve.argtypes = [_P(BrConfig), _P(BrThresholds)]
        L.br_batch_prepare.argtypes = [_P(BrBatch), C.c_void_p, C.c_void_p, _P(C.c_int64)]
        L.br_batch_seq_source.argtypes = [_P(BrBatch), C.c_void_p, C.c_int64, C.c_void_p]
        L.br_ctx_new.argtypes = [C.c_void_p, _P(C.c_void_p)]
        L.br_ctx_free.argtypes = [C.c_void_p]
        L.br_project_batch.argtypes = [C.c_void_p, _P(BrConfig), _P(BrBatch), _P(BrRows)]
        L.br_project_batch_device.argtypes = [C.c_void_p, _P(BrConfig), _P(BrDeviceBatch), C.c_void_p,
                                              _P(BrDeviceRows)]
        L.br_project_group.argtypes = [C.c_void_p, _P(BrConfig), _P(BrAlignment), C.c_size_t, _P(_P(BrProjected)),
                                       _P(C.c_size_t)]
        L.br_project_groups.argtypes = L.br_project_group.argtypes
        L.br_batch_stage.argtypes = [C.c_void_p, _P(BrBatch), C.c_int]
        L.br_project_staged.argtypes = [C.c_void_p, _P(BrConfig), C.c_int, _P(BrHostRows)]
        L.br_host_rows_wait.argtypes = [C.c_void_p, C.c_int]
        L.br_project_batch_packed.argtypes = [C.c_void_p, _P(BrConfig), _P(BrBatch), _P(BrHostRows)]
        L.br_pin_host.argtypes = [C.c_void_p, C.c_size_t]
        L.br_unpin_host.argtypes = [C.c_void_p]
        L.br_row_mapq.restype = C.c_uint32
        L.br_row_mapq.argtypes = [C.c_uint32, C.c_int]
        L.br_device_rows_expand.argtypes = [C.c_void_p, C.c_void_p, _P(BrDeviceWideRows)]
        L.br_bam_encode_device.argtypes = [C.c_void_p, _P(BrConfig), _P(BrDeviceRecords), C.c_void_p, _P(BrDeviceBam)]
        L.br_project_bam_device.argtypes = [C.c_void_p, _P(BrConfig), _P(BrDeviceRecords), C.c_void_p, C.c_int32, C.c_void_p,
                                            _P(BrDeviceRows), _P(BrDeviceBam)]
        L.br_project_bam_bundle.argtypes = [C.c_void_p, _P(BrConfig), _P(BrBamBundle), _P(BrHostBam)]
        L.br_bam_split.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, _P(C.c_int64), _P(C.c_int64),
                                   _P(C.c_uint64)]
        L.br_index_num_refs.restype = C.c_size_t
        L.br_index_num_refs.argtypes = [C.c_void_p]
        L.br_bgzf_deflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, _P(C.c_void_p), _P(C.c_uint64)]
        L.br_ctx_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.br_ctx_set_param.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.br_ctx_kernel_ms.argtypes = [C.c_void_p, C.c_int, _P(C.c_double), _P(C.c_int32)]
        L.br_ctx_collect_counters.argtypes = [C.c_void_p, _P(BrDeviceBatch), C.c_void_p]
        L.br_ctx_last_counters.argtypes = [C.c_void_p, C.c_void_p]
        L.br_ctx_direct_diag.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.br_ctx_direct_tidwords.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.br_ctx_rescue_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.br_ctx_ksw_diag.argtypes = [C.c_void_p, C.c_void_p]
        L.br_device_rows_detail.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.br_ctx_ksw_pairs.argtypes = [C.c_void_p, C.c_int64, _P(C.c_char_p), _P(C.c_char_p), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.br_primary_pick.restype = C.c_uint32
        L.br_primary_pick.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32]
        L.br_version.restype = C.c_char_p
        L.br_strerror.restype = C.c_char_p
        L.br_strerror.argtypes = [C.c_int]
        _LIB = L
    return _LIB


def load_annotation(path, threads=None):
    """The guide loader (br_annotation_load / br_annotation_load_mt with `threads`) on a GTF / GFF3 file, plain or gzip -> dict of
    refnames (order of first appearance), transcripts ({id, seqname, strand, exons (1-based half-open)}, in the loader's order)
    and gene_ids (the gene of every transcript, in that order)."""
    L = lib()
    L.br_annotation_load.argtypes = [C.c_char_p, _P(C.c_void_p)]
    L.br_annotation_load_mt.argtypes = [C.c_char_p, C.c_int, _P(C.c_void_p)]
    L.br_annotation_free.argtypes = [C.c_void_p]
    for name, res in (("num_transcripts", C.c_size_t), ("num_refs", C.c_size_t), ("transcripts", _P(BrTranscript)),
                      ("refnames", _P(C.c_char_p)), ("gene_ids", _P(C.c_char_p))):
        f = getattr(L, "br_annotation_" + name)
        f.restype, f.argtypes = res, [C.c_void_p]
    h = C.c_void_p()
    if threads is None:
        check(L.br_annotation_load(os.fsencode(path), C.byref(h)), "br_annotation_load")
    else:
        check(L.br_annotation_load_mt(os.fsencode(path), int(threads), C.byref(h)), "br_annotation_load_mt")
    try:
        n, t, g, rn = L.br_annotation_num_transcripts(h), L.br_annotation_transcripts(h), L.br_annotation_gene_ids(h), L.br_annotation_refnames(h)
        txs = [{"id": t[i].id.decode(), "seqname": t[i].seqname.decode(), "strand": t[i].strand.decode(),
                "exons": [[t[i].exons[k].start, t[i].exons[k].end] for k in range(t[i].n_exons)]} for i in range(n)]
        return {"refnames": [rn[i].decode() for i in range(L.br_annotation_num_refs(h))], "transcripts": txs,
                "gene_ids": [g[i].decode() for i in range(n)]}
    finally:
        L.br_annotation_free(h)


def check(rc, what):
    if rc != 0:
        raise BrambleError("%s failed: %s (%d)" % (what, lib().br_strerror(rc).decode(), rc))


def make_config(**kw):
    """lr, lr_hq, strict, use_fasta, fr, rf + optional max_clip, max_junc_ins, max_junc_gap,
    max_error_exon, sim_thr overrides (bramble CLI flags, src/bramble.cpp:457-485)."""
    c = BrConfig()
    lib().br_config_short_read(C.byref(c))
    for k, v in kw.items():
        if k in ("max_clip", "max_junc_ins", "max_junc_gap", "max_error_exon", "sim_thr"):
            setattr(c, "has_" + k, 1)
        setattr(c, k, v)
    return c


def resolve_config(cfg):
    t = BrThresholds()
    check(lib().br_config_resolve(C.byref(cfg), C.byref(t)), "br_config_resolve")
    return {"max_clip": t.max_clip, "max_junc_ins": t.max_junc_ins, "max_junc_gap": t.max_junc_gap,
            "max_error_exon": t.max_error_exon, "ignore_small_exons": bool(t.ignore_small_exons),
            "filter_by_similarity": bool(t.filter_by_similarity),
            "similarity_threshold": float(t.similarity_threshold)}


class Index:
    """g2tTree replacement: flattened exon tables, uploaded to `device` (-1: host only)."""

    def __init__(self, annotation, device=0):
        L = lib()
        txs = annotation["transcripts"]
        refnames = [r.encode() for r in annotation["refnames"]]
        arr = (BrTranscript * max(len(txs), 1))()
        keep = []
        for i, t in enumerate(txs):
            ex = (BrExon * max(len(t["exons"]), 1))()
            for k, (s, e) in enumerate(t["exons"]):
                ex[k].start, ex[k].end = int(s), int(e)
            keep.append(ex)
            arr[i].id = t["id"].encode()
            arr[i].seqname = (t["seqname"] if "seqname" in t else annotation["refnames"][t["ref_id"]]).encode()
            arr[i].strand = t["strand"].encode()
            arr[i].exons = ex
            arr[i].n_exons = len(t["exons"])
        rn = (C.c_char_p * max(len(refnames), 1))(*refnames)
        fa, nfa = None, 0
        seqs = annotation.get("ref_seqs")
        if seqs:
            items = sorted(seqs.items())
            fa = (BrFastaSeq * len(items))()
            for i, (rid, s) in enumerate(items):
                sb = s.encode() if isinstance(s, str) else bytes(s)
                keep.append(sb)
                fa[i].name = annotation["refnames"][rid].encode()
                fa[i].seq = sb
                fa[i].len = len(sb)
            nfa = len(items)
        h = C.c_void_p()
        check(L.br_index_build(arr, len(txs), rn, len(refnames), fa, nfa, device, C.byref(h)), "br_index_build")
        self.h = h
        self.device = device

    @classmethod
    def from_flat(cls, flat, device=0):
        """flat: dict with n_refs, tx_ref int32[], tx_strand int8[], tx_exon_off uint64[], ex_start/ex_end
        uint32[] (half-open) and optional ref_seqs (list of bytes or None per reference)."""
        self = cls.__new__(cls)
        ref = np.ascontiguousarray(flat["tx_ref"], dtype=np.int32)
        strand = np.ascontiguousarray(flat["tx_strand"], dtype=np.int8)
        off = np.ascontiguousarray(flat["tx_exon_off"], dtype=np.uint64)
        es = np.ascontiguousarray(flat["ex_start"], dtype=np.uint32)
        ee = np.ascontiguousarray(flat["ex_end"], dtype=np.uint32)
        fa = None
        keep = []
        if flat.get("ref_seqs") is not None:
            fa = (BrFastaSeq * flat["n_refs"])()
            for r, sq in enumerate(flat["ref_seqs"]):
                if sq is None:
                    continue
                sb = sq if isinstance(sq, (bytes, bytearray)) else bytes(sq)
                keep.append(sb)
                fa[r].name = b"ref%d" % r
                fa[r].seq = sb
                fa[r].len = len(sb)
        h = C.c_void_p()
        check(lib().br_index_build_flat(len(ref), ref.ctypes.data, strand.ctypes.data, off.ctypes.data,
                                        es.ctypes.data, ee.ctypes.data, None, int(flat["n_refs"]), fa, device,
                                        C.byref(h)), "br_index_build_flat")
        self.h = h
        self.device = device
        return self

    def num_transcripts(self):
        return lib().br_index_num_transcripts(self.h)

    def transcript_name(self, tid):
        s = lib().br_index_transcript_name(self.h, tid)
        return s.decode() if s is not None else None

    def transcript_len(self, tid):
        v = lib().br_index_transcript_len(self.h, tid)
        return None if v < 0 else int(v)

    def num_intervals(self):
        return lib().br_index_num_intervals(self.h)

    def device_bytes(self):
        return lib().br_index_device_bytes(self.h)

    def close(self):
        if self.h:
            lib().br_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _batch_struct(batch, keep):
    b = BrBatch()
    b.n_aln = int(batch["n_aln"])

    def put(name, dtype):
        a = np.ascontiguousarray(batch[name], dtype=dtype)
        keep.append(a)
        setattr(b, name, a.ctypes.data)

    for name, dt in (("ref_id", np.int32), ("ref_start", np.int32), ("flags", np.uint16), ("xs", np.int8),
                     ("ts", np.int8), ("cigar_off", np.uint64), ("cigar", np.uint32), ("mate_ref_id", np.int32),
                     ("mate_start", np.int32), ("name_off", np.uint64), ("names", np.uint8), ("l_qseq", np.int32)):
        put(name, dt)
    if batch.get("seq_off") is not None:
        put("seq_off", np.uint64)
        put("seqs", np.uint8)
    return b


def prepare_batch(batch):
    """Host-side input contract (br_batch_prepare): returns (mate_idx int32[n], group_off uint32[g+1])."""
    keep = []
    b = _batch_struct(batch, keep)
    n = int(batch["n_aln"])
    mate = np.full(max(n, 1), -1, dtype=np.int32)
    goff = np.zeros(n + 1, dtype=np.uint32)
    ng = C.c_int64()
    check(lib().br_batch_prepare(C.byref(b), mate.ctypes.data, goff.ctypes.data, C.byref(ng)), "br_batch_prepare")
    return mate[:n], goff[:ng.value + 1].copy()


def _view(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n).copy()


def host_rows_to_numpy(r):
    """BrHostRows -> dict of numpy copies: a uint32 [n, 4] = {tid, pos, meta, nh}, cigar uint64 [n], pool uint32,
    row_off uint64 [n_aln + 1], mate_idx int32 [n_aln], optional x / similarity_score / clip_score."""
    n, na = int(r.n_rows), int(r.n_aln)
    out = {"n_rows": n, "n_aln": na, "n_groups": int(r.n_groups),
           "a": _view(r.a, 4 * n, np.uint32).reshape(n, 4), "cigar": _view(r.cigar, n, np.uint64),
           "pool": _view(r.pool, int(r.n_pool_words), np.uint32), "row_off": _view(r.row_off, na + 1, np.uint64),
           "mate_idx": _view(r.mate_idx, na, np.int32)}
    if r.x:
        out["x"] = _view(r.x, 4 * n, np.uint32).reshape(n, 4)
    if r.similarity_score:
        out["similarity_score"] = _view(r.similarity_score, n, np.float64)
        out["clip_score"] = _view(r.clip_score, n, np.int32)
    for name, _ in _COUNTERS:
        out[name] = int(getattr(r, name))
    return out


def unpack_host_rows(p, l_qseq, long_reads=False):
    """Packed host rows (host_rows_to_numpy, with the x array) -> the wide dict project_batch returns (minus `group`),
    derived on the host exactly as include/bramble_amd.h documents: HI / MAPQ / mate fields / insert size."""
    n = p["n_rows"]
    a, x = p["a"], p["x"]
    meta = a[:, 2]
    ncig = (meta & 0xffffff).astype(np.int64)
    w = {"n_rows": n, "transcript_id": a[:, 0].copy(), "pos": a[:, 1].copy(), "nh": a[:, 3].copy(),
         "strand": np.where(meta & ROW_MINUS, ord("-"), ord("+")).astype(np.int8),
         "is_paired": ((meta & ROW_PAIRED) != 0).astype(np.uint8),
         "same_transcript_as_mate": ((meta & ROW_SAME_TX) != 0).astype(np.uint8),
         "is_first": ((meta & ROW_FIRST) != 0).astype(np.uint8), "is_primary": ((meta & ROW_PRIMARY) != 0).astype(np.uint8),
         "input_index": x[:, 0].astype(np.int32), "junc_hits": x[:, 1].astype(np.int32),
         "aligned_len": x[:, 2].astype(np.int32), "hi": x[:, 3].copy()}
    nh = w["nh"]
    if long_reads:
        w["mapq"] = np.where(nh > 1, 0, 3).astype(np.uint32)
    else:
        w["mapq"] = np.select([nh == 1, nh == 2, (nh == 3) | (nh == 4)], [255, 3, 1], 0).astype(np.uint32)
    coff = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(ncig, out=coff[1:])
    cig = np.zeros(int(coff[-1]), dtype=np.uint32)
    c = p["cigar"]
    one = np.nonzero(ncig >= 1)[0]
    inl = ncig <= 2
    i1 = np.nonzero(inl & (ncig >= 1))[0]
    cig[coff[i1].astype(np.int64)] = (c[i1] & np.uint64(0xffffffff)).astype(np.uint32)
    i2 = np.nonzero(ncig == 2)[0]
    cig[coff[i2].astype(np.int64) + 1] = (c[i2] >> np.uint64(32)).astype(np.uint32)
    for r in np.nonzero(~inl)[0]:
        o = int(c[r])
        cig[int(coff[r]):int(coff[r + 1])] = p["pool"][o:o + int(ncig[r])]
    del one
    w["cigar_off"], w["cigar"] = coff, cig
    paired = w["is_paired"].astype(bool)
    first = w["is_first"].astype(bool)
    idx = np.arange(n)
    nb = np.where(first, idx + 1, idx - 1)
    nb = np.where(paired, nb, idx)
    mate_pos = np.where(paired, a[nb, 1].astype(np.int64), -1)
    same = w["same_transcript_as_mate"].astype(bool)
    mate_tid = np.where(paired, np.where(same, a[:, 0].astype(np.int64), a[nb, 0].astype(np.int64)), -1)
    lq = np.asarray(l_qseq, dtype=np.int64)[w["input_index"]] if n else np.zeros(0, np.int64)
    my = a[:, 1].astype(np.int64)
    isz = np.where(my <= mate_pos, (mate_pos + lq) - my, -((my + lq) - mate_pos))
    w["mate_transcript_id"] = mate_tid.astype(np.int32)
    w["mate_pos"] = mate_pos.astype(np.int32)
    w["insert_size"] = np.where(paired & same, isz, 0).astype(np.int32)
    w["similarity_score"] = p.get("similarity_score", np.zeros(n))
    w["clip_score"] = p.get("clip_score", np.zeros(n, np.int32))
    for k in ("total_complete", "total_unique", "dropped_reads", "total_processed"):
        w[k] = p[k]
    return w


class Context:
    """ProjectionContext: device scratch + stream-ordered pipeline for one index."""

    def __init__(self, index):
        h = C.c_void_p()
        check(lib().br_ctx_new(index.h, C.byref(h)), "br_ctx_new")
        self.h = h
        self.index = index

    def set_param(self, key, value):
        check(lib().br_ctx_set_param(self.h, key.encode(), int(value)), "br_ctx_set_param")

    def set_profiling(self, enabled):
        check(lib().br_ctx_set_profiling(self.h, 1 if enabled else 0), "br_ctx_set_profiling")

    def kernel_ms(self):
        out = {}
        for k in range(K_NUM):
            ms, ln = C.c_double(), C.c_int32()
            check(lib().br_ctx_kernel_ms(self.h, k, C.byref(ms), C.byref(ln)), "br_ctx_kernel_ms")
            out[KERNEL_NAMES[k]] = (ms.value, ln.value)
        return out

    def kernel_ms_sum(self):
        """{kernel name: (ms, launches)} summed over the calls since set_profiling(True)."""
        out = {}
        L = lib()
        L.br_ctx_kernel_ms_sum.argtypes = [C.c_void_p, C.c_int, _P(C.c_double), _P(C.c_int64)]
        for k in range(K_NUM):
            ms, ln = C.c_double(), C.c_int64()
            check(L.br_ctx_kernel_ms_sum(self.h, k, C.byref(ms), C.byref(ln)), "br_ctx_kernel_ms_sum")
            out[KERNEL_NAMES[k]] = (ms.value, ln.value)
        return out

    def project_batch(self, cfg, batch):
        """Host batch in, rows (dict of numpy arrays) out: convert_reads minus BAM writing."""
        keep = []
        b = _batch_struct(batch, keep)
        r = BrRows()
        check(lib().br_project_batch(self.h, C.byref(cfg), C.byref(b), C.byref(r)), "br_project_batch")
        n = r.n_rows
        rows = {"n_rows": n}
        for name, dt in _ROW_FIELDS + [("is_primary", np.uint8)] + _ROW_TAIL:
            if name == "cigar_off":
                rows[name] = _view(r.cigar_off, n + 1, dt)
            elif name == "cigar":
                continue
            else:
                rows[name] = _view(getattr(r, name), n, dt)
        rows["cigar"] = _view(r.cigar, int(rows["cigar_off"][-1]) if n else 0, np.uint32)
        for name, _ in _COUNTERS:
            rows[name] = int(getattr(r, name))
        return rows

    @staticmethod
    def _device_batch_struct(dev_batch):
        db = BrDeviceBatch()
        db.n_aln = dev_batch["n_aln"]
        db.n_groups = dev_batch["n_groups"]
        for name in ("ref_id", "ref_start", "flags", "xs", "ts", "cigar_off", "cigar", "mate_idx", "group_off",
                     "l_qseq"):
            setattr(db, name, dev_batch[name].data_ptr())
        db.n_cigar_words = dev_batch["n_cigar_words"]
        db.max_n_cigar = dev_batch["max_n_cigar"]
        if dev_batch.get("seqs") is not None:
            db.seq_off = dev_batch["seq_off"].data_ptr()
            db.seqs = dev_batch["seqs"].data_ptr()
            db.seq_src = dev_batch["seq_src"].data_ptr()
            db.max_soft_clip = dev_batch["max_soft_clip"]
        if dev_batch.get("names") is not None:
            db.name_off = dev_batch["name_off"].data_ptr()
            db.names = dev_batch["names"].data_ptr()
        return db

    def collect_counters(self, dev_batch, stream=0):
        """Exact algorithmic-bytes counters of the batch projected last."""
        db = self._device_batch_struct(dev_batch)
        check(lib().br_ctx_collect_counters(self.h, C.byref(db), C.c_void_p(stream)), "br_ctx_collect_counters")
        out = (C.c_uint64 * 8)()
        check(lib().br_ctx_last_counters(self.h, out), "br_ctx_last_counters")
        keys = ("B_in", "B_idx", "B_out", "n_cigar", "read_exons", "overlap_hits", "matches", "out_cigar_words")
        return dict(zip(keys, [int(v) for v in out]))

    def direct_diag(self, n_aln=None):
        """What the last call (a direct-rows call) left on the device: {"n_big": big_list length, "side_attempts",
        "side_used": arena entries the last attempt asked for, "side_cap": its capacity, "pm_n": windows sent to
        k_pair_mask_wide, "light": work-list entries of the light two-exon class, "pm_list": PAIR alignments k_pair_mask resolved by
        tid lists, not by 64-bit tid masks (counted with "pair_bitmask" 1)}, plus "pflags" (uint8 [n_aln]: PF_PAIRED 1 | PF_SAME 2 | PF_MATE 4 | PF_BIG 8) when n_aln is given."""
        out = (C.c_uint64 * 8)()
        pf = np.zeros(n_aln, dtype=np.uint8) if n_aln is not None else None
        check(lib().br_ctx_direct_diag(self.h, out, pf.ctypes.data if pf is not None and n_aln else None), "br_ctx_direct_diag")
        d = dict(zip(("n_big", "side_attempts", "side_used", "side_cap", "pm_n", "light", "pm_list"), [int(v) for v in out[:7]]))
        if pf is not None:
            d["pflags"] = pf
        return d

    def direct_tidwords(self, n_aln):
        """The tid words the last call's (a direct-rows call's) pairing left, one per alignment: (common uint64 [n_aln], base
        uint32 [n_aln]).  base[a] != KT_NONE: bit b of common[a] = transcript base[a] + b is kept, and the emit kernels ranked the
        alignment's records by counting bits; KT_NONE: no word, ranked by the loop (always, after a call with "emit_rank_tids" 0).
        Diagnostic only; the words of alignments that keep nothing mean nothing."""
        common, base = np.zeros(n_aln, dtype=np.uint64), np.zeros(n_aln, dtype=np.uint32)
        check(lib().br_ctx_direct_tidwords(self.h, common.ctypes.data if n_aln else None, base.ctypes.data if n_aln else None), "br_ctx_direct_tidwords")
        return common, base

    def project_bam_device(self, cfg, blob, rec_off, rec_len, ref_map, stream=0):
        """Raw mapped BAM records resident in HBM -> (BrDeviceRows, BrDeviceBam): reader side, projection and
        record re-encoding, all on the device.  blob uint8 / rec_off int64 [n] / rec_len int32 [n] are torch CUDA
        tensors; ref_map is a host int32 array (input refID -> annotation reference index)."""
        recs = BrDeviceRecords()
        recs.blob = blob.data_ptr()
        recs.rec_off = rec_off.data_ptr()
        recs.n_aln = rec_len.numel()
        recs.rec_len = rec_len.data_ptr()
        rm = np.ascontiguousarray(ref_map, dtype=np.int32)
        rows, out = BrDeviceRows(), BrDeviceBam()
        check(lib().br_project_bam_device(self.h, C.byref(cfg), C.byref(recs), rm.ctypes.data, len(rm), C.c_void_p(stream),
                                          C.byref(rows), C.byref(out)), "br_project_bam_device")
        return rows, out

    def bgzf_deflate_device(self, src, stream=0):
        """src: torch CUDA uint8 tensor -> torch CUDA uint8 tensor view of the concatenated BGZF blocks (valid until the
        next call on this context)."""
        import torch
        from .device import _DevArray
        out, n = C.c_void_p(), C.c_uint64()
        check(lib().br_bgzf_deflate_device(self.h, C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(stream), C.byref(out),
                                           C.byref(n)), "br_bgzf_deflate_device")
        if n.value == 0:
            return torch.zeros(0, dtype=torch.uint8, device=src.device)
        return torch.as_tensor(_DevArray(out.value, n.value, "|u1"), device=src.device)

    def bgzf_inflate_device(self, src, blocks, stream=0):
        """src: torch CUDA uint8 tensor holding BGZF bytes, blocks: the table bgzf_scan made of the same bytes -> torch CUDA
        uint8 tensor view of the inflated stream (valid until the next call on this context)."""
        import torch
        from .device import _DevArray
        out, n = C.c_void_p(), C.c_uint64()
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK)
        L = lib()
        L.br_bgzf_inflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64, C.c_void_p, _P(C.c_void_p), _P(C.c_uint64)]
        check(L.br_bgzf_inflate_device(self.h, C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(blocks.ctypes.data), len(blocks),
                                       C.c_void_p(stream), C.byref(out), C.byref(n)), "br_bgzf_inflate_device")
        if n.value == 0:
            return torch.zeros(0, dtype=torch.uint8, device=src.device)
        return torch.as_tensor(_DevArray(out.value, n.value, "|u1"), device=src.device)

    def set_sam_refs(self, names):
        """The reference names SAM text prints as RNAME / RNEXT, in refID order (br_ctx_set_sam_refs)."""
        arr = (C.c_char_p * max(len(names), 1))(*[n.encode() if isinstance(n, str) else bytes(n) for n in names])
        L = lib()
        L.br_ctx_set_sam_refs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        check(L.br_ctx_set_sam_refs(self.h, arr, len(names)), "br_ctx_set_sam_refs")

    def sam_format_device(self, data, row_off=None, stream=0):
        """br_sam_format_device: a record stream in HBM ([block_size][record]...) -> torch CUDA uint8 view of its SAM lines (valid
        until the next call on this context).  data: a BrDeviceBam (as project_bam_device returns it), or a torch CUDA uint8
        tensor with row_off, a torch CUDA int64 tensor of each record's offset."""
        import torch
        from .device import _DevArray
        if isinstance(data, BrDeviceBam):
            db, dev = data, torch.device("cuda", torch.cuda.current_device())
        else:
            db, dev = BrDeviceBam(), data.device
            db.data, db.n_bytes = data.data_ptr() if data.numel() else None, data.numel()
            db.row_off, db.n_rows = row_off.data_ptr() if row_off.numel() else None, row_off.numel()
        out, n = C.c_void_p(), C.c_uint64()
        L = lib()
        L.br_sam_format_device.argtypes = [C.c_void_p, _P(BrDeviceBam), C.c_void_p, _P(C.c_void_p), _P(C.c_uint64)]
        check(L.br_sam_format_device(self.h, C.byref(db), C.c_void_p(stream), C.byref(out), C.byref(n)), "br_sam_format_device")
        if n.value == 0:
            return torch.zeros(0, dtype=torch.uint8, device=dev)
        return torch.as_tensor(_DevArray(out.value, n.value, "|u1"), device=dev)

    def project_bam_resident(self, cfg, recs, ref_map, sam_text=False):
        """br_project_bam_resident over a BrDeviceRecords that is in HBM already (a reader's or a Collator's bundle):
        (stream uint8[], counters dict) as project_bam_bundle; with sam_text the stream is the records' SAM lines."""
        rm = np.ascontiguousarray(ref_map, dtype=np.int32)
        out = BrHostBam()
        L = lib()
        L.br_project_bam_resident.argtypes = [C.c_void_p, _P(BrConfig), _P(BrDeviceRecords), C.c_void_p, C.c_int32, C.c_int, C.c_int,
                                              _P(BrHostBam)]
        check(L.br_project_bam_resident(self.h, C.byref(cfg), C.byref(recs), rm.ctypes.data, len(rm), OUT_SAM_TEXT if sam_text else 0, 0,
                                        C.byref(out)),
              "br_project_bam_resident")
        n = int(out.n_bytes)
        data = np.ctypeslib.as_array(C.cast(out.data, _P(C.c_uint8)), shape=(n,)).copy() if n else np.zeros(0, np.uint8)
        return data, {"n_rows": int(out.n_rows), "total_complete": int(out.total_complete),
                      "total_unique": int(out.total_unique), "dropped_reads": int(out.dropped_reads),
                      "total_processed": int(out.total_processed)}

    def project_bam_resident_kept(self, cfg, recs, ref_map):
        """br_project_bam_resident with BR_OUT_RESIDENT: the projected records stay in HBM -> (BrDeviceBam valid until the context's
        next call, counters dict).  A Sorter takes the BrDeviceBam (add_device)."""
        rm = np.ascontiguousarray(ref_map, dtype=np.int32)
        out, db = BrHostBam(), BrDeviceBam()
        L = lib()
        L.br_project_bam_resident.argtypes = [C.c_void_p, _P(BrConfig), _P(BrDeviceRecords), C.c_void_p, C.c_int32, C.c_int, C.c_int,
                                              _P(BrHostBam)]
        L.br_ctx_last_device_bam.argtypes = [C.c_void_p, _P(BrDeviceBam)]
        check(L.br_project_bam_resident(self.h, C.byref(cfg), C.byref(recs), rm.ctypes.data, len(rm), OUT_RESIDENT, 0, C.byref(out)),
              "br_project_bam_resident")
        check(L.br_ctx_last_device_bam(self.h, C.byref(db)), "br_ctx_last_device_bam")
        return db, {"n_rows": int(out.n_rows), "total_complete": int(out.total_complete), "total_unique": int(out.total_unique),
                    "dropped_reads": int(out.dropped_reads), "total_processed": int(out.total_processed)}

    def device_bam_download(self, piece, out_mode=0):
        """br_device_bam_download: a record stream in HBM (a Sorter piece) -> numpy uint8 of its bytes (out_mode 0), its BGZF
        blocks (1) or its SAM lines (OUT_SAM_TEXT)."""
        out = BrHostBam()
        L = lib()
        L.br_device_bam_download.argtypes = [C.c_void_p, _P(BrDeviceBam), C.c_int, C.c_int, _P(BrHostBam)]
        check(L.br_device_bam_download(self.h, C.byref(piece), int(out_mode), 0, C.byref(out)), "br_device_bam_download")
        n = int(out.n_bytes)
        return np.ctypeslib.as_array(C.cast(out.data, _P(C.c_uint8)), shape=(n,)).copy() if n else np.zeros(0, np.uint8)

    UNPROJECTED_STATS = ("records", "unprojected", "bytes", "names", "names_none", "names_partial", "held_bytes", "peak_bytes")

    def unprojected_stats(self):
        """br_ctx_unprojected_stats as a dict (UNPROJECTED_STATS): sums over the bundle calls since the last reset, made with
        set_param("keep_unprojected", 1 | 2)."""
        out = (C.c_uint64 * 8)()
        L = lib()
        L.br_ctx_unprojected_stats.argtypes = [C.c_void_p, C.c_void_p]
        check(L.br_ctx_unprojected_stats(self.h, out), "br_ctx_unprojected_stats")
        return dict(zip(self.UNPROJECTED_STATS, [int(v) for v in out]))

    def unprojected_records(self, max_bytes):
        """br_ctx_unprojected_next as it is: the next piece as a BrDeviceBam in HBM (n_rows = 0 at the end; valid until the next
        call on the context)."""
        piece = BrDeviceBam()
        L = lib()
        L.br_ctx_unprojected_next.argtypes = [C.c_void_p, C.c_uint64, _P(BrDeviceBam)]
        check(L.br_ctx_unprojected_next(self.h, int(max_bytes), C.byref(piece)), "br_ctx_unprojected_next")
        return piece

    def unprojected_next(self, max_bytes):
        """The next unprojected records in input order, up to max_bytes and at least one, as numpy copies: (uint8 stream of
        [block_size][record]..., uint64 row_off [n_rows + 1] into it); both empty when that was all."""
        import torch
        from .device import _DevArray
        p = self.unprojected_records(max_bytes)
        n = int(p.n_rows)
        if n == 0:
            return np.zeros(0, np.uint8), np.zeros(0, np.uint64)
        dev = "cuda:%d" % self.index.device
        off = torch.as_tensor(_DevArray(p.row_off, n + 1, "<u8"), device=dev).cpu().numpy().astype(np.uint64)
        data = torch.as_tensor(_DevArray(p.data, int(p.n_bytes), "|u1"), device=dev).cpu().numpy().copy()
        return data, off

    def unprojected_reset(self):
        L = lib()
        L.br_ctx_unprojected_reset.argtypes = [C.c_void_p]
        check(L.br_ctx_unprojected_reset(self.h), "br_ctx_unprojected_reset")

    def project_bam_bundle(self, cfg, blob, rec_off, rec_len, ref_map, bgzf_on_device=False, sam_text=False):
        """Host form: numpy blob / rec_off (uint64) / rec_len (uint32) in, (stream uint8[], counters dict) out; with sam_text the
        stream is the projected records' SAM lines (set_sam_refs names their references)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        rec_len = np.ascontiguousarray(rec_len, dtype=np.uint32)
        rm = np.ascontiguousarray(ref_map, dtype=np.int32)
        bb = BrBamBundle(blob.ctypes.data, blob.size, rec_off.ctypes.data, rec_len.ctypes.data, len(rec_len),
                         rm.ctypes.data, len(rm), OUT_SAM_TEXT if sam_text else 1 if bgzf_on_device else 0)
        out = BrHostBam()
        check(lib().br_project_bam_bundle(self.h, C.byref(cfg), C.byref(bb), C.byref(out)), "br_project_bam_bundle")
        n = int(out.n_bytes)
        data = np.ctypeslib.as_array(C.cast(out.data, _P(C.c_uint8)), shape=(n,)).copy() if n else np.zeros(0, np.uint8)
        return data, {"n_rows": int(out.n_rows), "total_complete": int(out.total_complete),
                      "total_unique": int(out.total_unique), "dropped_reads": int(out.dropped_reads),
                      "total_processed": int(out.total_processed)}

    def bam_encode_device(self, cfg, blob, rec_off, stream=0):
        """Re-encode every row of the last project_batch_device call as BAM records.
        blob / rec_off: torch CUDA tensors (uint8 record bytes, int64 offsets n_aln+1)."""
        recs = BrDeviceRecords()
        recs.blob = blob.data_ptr()
        recs.rec_off = rec_off.data_ptr()
        recs.n_aln = rec_off.numel() - 1
        recs.rec_len = None
        out = BrDeviceBam()
        check(lib().br_bam_encode_device(self.h, C.byref(cfg), C.byref(recs), C.c_void_p(stream), C.byref(out)),
              "br_bam_encode_device")
        return out

    def ksw_pairs(self, pairs, cap=None, sides=None, segments=False):
        """Diagnostic: k_ksw alone on [(target, query)] -> (ok int32[n], max int32[n], [cigar uint32[] per pair]).
        sides: per pair 0 (left-side problem: both strings already reversed by the caller) or 1 (right; the default).
        segments: also (refc int32[n], [clip-segment override ops uint32[] per pair]) at the end of the tuple."""
        n = len(pairs)
        cap = int(cap or max([len(t) + len(q) + 4 for t, q in pairs] + [8]))
        ts = (C.c_char_p * max(n, 1))(*[t.encode() for t, _ in pairs])
        qs = (C.c_char_p * max(n, 1))(*[q.encode() for _, q in pairs])
        ok = np.zeros(max(n, 1), np.int32)
        mx = np.zeros(max(n, 1), np.int32)
        nc = np.zeros(max(n, 1), np.uint32)
        cig = np.zeros(max(n, 1) * cap, np.uint32)
        sd = None if sides is None else np.ascontiguousarray(np.asarray(sides, dtype=np.uint8))
        assert sd is None or sd.shape == (n,)
        refc = np.zeros(max(n, 1), np.int32) if segments else None
        ns = np.zeros(max(n, 1), np.uint32) if segments else None
        seg = np.zeros(max(n, 1) * cap, np.uint32) if segments else None
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data   # noqa: E731
        check(lib().br_ctx_ksw_pairs(self.h, n, ts, qs, ok.ctypes.data, mx.ctypes.data, nc.ctypes.data, cig.ctypes.data, cap,
                                     ptr(sd), ptr(refc), ptr(ns), ptr(seg)), "br_ctx_ksw_pairs")
        out = (ok[:n], mx[:n], [cig[p * cap:p * cap + int(nc[p])].copy() for p in range(n)])
        if segments:
            assert int(ns[:n].max(initial=0)) <= cap
            out += (refc[:n], [seg[p * cap:p * cap + int(ns[p])].copy() for p in range(n)])
        return out

    def rescue_stats(self):
        out = (C.c_uint64 * 4)()
        check(lib().br_ctx_rescue_stats(self.h, out), "br_ctx_rescue_stats")
        return dict(zip(("problems", "dp_cells", "rescued", "seq_bytes"), [int(v) for v in out]))

    def rows_detail(self, stream=0):
        """Device pointer of the br_row_x array of the last call's rows (derived on first request)."""
        x = C.c_void_p()
        check(lib().br_device_rows_detail(self.h, C.c_void_p(stream), C.byref(x)), "br_device_rows_detail")
        return x.value

    def ksw_diag(self):
        out = (C.c_uint64 * 16)()
        check(lib().br_ctx_ksw_diag(self.h, out), "br_ctx_ksw_diag")
        v = [int(x) for x in out]
        return {"pieces": v[0], "per_shape": v[1:5], "leftover_before": v[5], "tape_bytes": v[6], "leftover_after": v[7],
                "rows_per_shape": v[8:12]}

    def project_batch_packed(self, cfg, batch):
        """Host batch in, packed host rows (dict of numpy arrays copied out of the context's pinned buffers) out."""
        keep = []
        b = _batch_struct(batch, keep)
        r = BrHostRows()
        check(lib().br_project_batch_packed(self.h, C.byref(cfg), C.byref(b), C.byref(r)), "br_project_batch_packed")
        return host_rows_to_numpy(r)

    def project_groups(self, cfg, alns):
        """br_project_groups: any number of name-collated groups in one call (same dicts as project_group)."""
        return self.project_group(cfg, alns, _many=True)

    def project_group(self, cfg, alns, _many=False):
        """project_group_with (bramble-rs/src/api.rs:285-290): alns = list of dicts with the GenomicAlignment fields
        (query_name, ref_id, ref_start, cigar [uint32 BAM-packed] and optional is_reverse, is_paired, is_first_in_pair,
        mate_is_unmapped, xs_strand, ts_strand, hit_index, mate_ref_id, mate_ref_start, sequence, read_len) -> list of
        dicts with the br_projected fields.  Raises BrambleError(BR_ERR_INVALID_ARG) when the query names differ."""
        n = len(alns)
        arr = (BrAlignment * max(n, 1))()
        keep = []
        for i, a in enumerate(alns):
            cg = np.ascontiguousarray(a["cigar"], dtype=np.uint32)
            keep.append(cg)
            x = arr[i]
            x.query_name = a["query_name"].encode()
            x.ref_id = int(a["ref_id"])
            x.ref_start = int(a["ref_start"])
            x.is_reverse = int(bool(a.get("is_reverse")))
            x.is_paired = int(bool(a.get("is_paired")))
            x.is_first_in_pair = int(bool(a.get("is_first_in_pair")))
            x.mate_is_unmapped = int(bool(a.get("mate_is_unmapped")))
            x.xs_strand = (a.get("xs_strand") or "\0").encode()
            x.ts_strand = (a.get("ts_strand") or "\0").encode()
            x.hit_index = int(a.get("hit_index", 0))
            x.mate_ref_id = int(a.get("mate_ref_id", -1))
            x.mate_ref_start = int(a.get("mate_ref_start", 0))
            x.cigar = cg.ctypes.data if len(cg) else None
            x.n_cigar = len(cg)
            sq = a.get("sequence")
            if sq:
                sb = sq.encode() if isinstance(sq, str) else bytes(sq)
                keep.append(sb)
                x.sequence = sb
                x.sequence_len = len(sb)
            x.read_len = int(a.get("read_len", 0))
        out, n_out = _P(BrProjected)(), C.c_size_t()
        fn = lib().br_project_groups if _many else lib().br_project_group
        check(fn(self.h, C.byref(cfg), arr, n, C.byref(out), C.byref(n_out)), "br_project_groups" if _many else "br_project_group")
        res = []
        for k in range(n_out.value):
            p = out[k]
            d = {f: getattr(p, f) for f, _ in BrProjected._fields_ if f != "cigar"}
            d["transcript_strand"] = p.transcript_strand.decode()
            d["cigar"] = np.array([p.cigar[j] for j in range(p.n_cigar)], dtype=np.uint32)
            res.append(d)
        return res

    def expand_rows(self, stream=0):
        """Wide (one array per field) view of the last projection call's rows: BrDeviceWideRows."""
        out = BrDeviceWideRows()
        check(lib().br_device_rows_expand(self.h, C.c_void_p(stream), C.byref(out)), "br_device_rows_expand")
        return out

    def project_batch_device(self, cfg, dev_batch, stream=0):
        """dev_batch: dict of torch CUDA tensors (see bramble_amd.device.upload_batch).  Returns the
        BrDeviceRows struct (packed rows; device pointers owned by the context)."""
        db = self._device_batch_struct(dev_batch)
        out = BrDeviceRows()
        check(lib().br_project_batch_device(self.h, C.byref(cfg), C.byref(db), C.c_void_p(stream), C.byref(out)),
              "br_project_batch_device")
        return out

    def close(self):
        if self.h:
            lib().br_ctx_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sam_header_scan(data):
    """br_sam_header_scan: bytes of the leading '@' lines of `data` (bytes)."""
    hb = C.c_uint64()
    L = lib()
    L.br_sam_header_scan.argtypes = [C.c_char_p, C.c_uint64, _P(C.c_uint64)]
    check(L.br_sam_header_scan(data, len(data), C.byref(hb)), "br_sam_header_scan")
    return int(hb.value)


class SamError(BrambleError):
    """A malformed SAM line: .line is its 1-based number from the reader's start, .reason what is wrong with it."""

    def __init__(self, line, reason):
        super().__init__("SAM line %d: %s" % (line, reason))
        self.line, self.reason = line, reason


class SamReader:
    """br_sam_reader on `device`: SAM record text in, the bundles' mapped BAM records out as host bytes (for tests and tools;
    the command line hands the device-resident bundles to the projection instead)."""

    def __init__(self, header_text, device=0):
        L = lib()
        L.br_sam_reader_new.argtypes = [C.c_int, C.c_char_p, C.c_uint64, _P(C.c_void_p)]
        L.br_sam_reader_next.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, _P(C.c_uint64), _P(BrDeviceRecords),
                                         _P(C.c_int64), _P(C.c_int64), _P(C.c_int64)]
        L.br_sam_reader_release.argtypes = [C.c_void_p, C.c_int64]
        L.br_sam_reader_free.argtypes = [C.c_void_p]
        L.br_sam_reader_error.argtypes = [C.c_void_p]
        L.br_sam_reader_error.restype = C.c_char_p
        L.br_sam_reader_stats.argtypes = [C.c_void_p, _P(C.c_double), _P(C.c_double), _P(C.c_int64), _P(C.c_uint64), _P(C.c_int64)]
        self.h = None
        self.device = device
        h = C.c_void_p()
        header_text = header_text.encode() if isinstance(header_text, str) else bytes(header_text)
        check(L.br_sam_reader_new(device, header_text, len(header_text), C.byref(h)), "br_sam_reader_new")
        self.h = h

    def next(self, text, last, fetch=True):
        """-> dict(stream = uint8 [block_size][record]... of the mapped records (fetch=False: not downloaded), n, n_unmapped,
        consumed)."""
        L = lib()
        recs, rid, un, bad, used = BrDeviceRecords(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_uint64()
        rc = L.br_sam_reader_next(self.h, bytes(text), len(text), 1 if last else 0, C.byref(used), C.byref(recs), C.byref(rid),
                                  C.byref(un), C.byref(bad))
        if rc == -1 and bad.value > 0:
            raise SamError(int(bad.value), L.br_sam_reader_error(self.h).decode())
        check(rc, "br_sam_reader_next")
        n = int(recs.n_aln)
        stream = np.zeros(0, dtype=np.uint8)
        try:
            if n and fetch:
                import torch
                from .device import _DevArray
                dev = "cuda:%d" % self.device
                off = torch.as_tensor(_DevArray(recs.rec_off, n, "<u8"), device=dev).cpu().numpy().astype(np.uint64)
                ln = torch.as_tensor(_DevArray(recs.rec_len, n, "<i4"), device=dev).cpu().numpy().view(np.uint32).astype(np.uint64)
                lo, hi = int(off[0]) - 4, int(off[-1] + ln[-1])
                blob = torch.as_tensor(_DevArray(recs.blob + lo, hi - lo, "|u1"), device=dev).cpu().numpy()
                parts = [blob[int(o) - 4 - lo:int(o + l) - lo] for o, l in zip(off, ln)]
                stream = np.concatenate(parts).astype(np.uint8)
        finally:
            if rid.value >= 0:
                check(L.br_sam_reader_release(self.h, rid.value), "br_sam_reader_release")
        return {"stream": stream, "n": n, "n_unmapped": int(un.value), "consumed": int(used.value)}

    def stats(self):
        up, parse, ch, nb, nl = C.c_double(), C.c_double(), C.c_int64(), C.c_uint64(), C.c_int64()
        check(lib().br_sam_reader_stats(self.h, C.byref(up), C.byref(parse), C.byref(ch), C.byref(nb), C.byref(nl)),
              "br_sam_reader_stats")
        return {"upload_s": up.value, "parse_s": parse.value, "chunks": int(ch.value), "bytes": int(nb.value), "lines": int(nl.value)}

    def close(self):
        if self.h:
            lib().br_sam_reader_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Accumulator:
    """What the wrappers of the run accumulators (br_collator, br_sorter, br_quant, br_coverage, br_assign) share: the handle, made by
    br_<NAME>_new and freed by br_<NAME>_free, and the calls of br_<NAME>_<what> on it.  A subclass gives NAME and ARGTYPES
    (<what> -> the argument types)."""
    NAME, ARGTYPES, h = None, {}, None

    def _open(self, device, *args):
        L = lib()
        for what, types in self.ARGTYPES.items():
            getattr(L, "br_%s_%s" % (self.NAME, what)).argtypes = types
        self.device = device
        h = C.c_void_p()
        check(getattr(L, "br_%s_new" % self.NAME)(device, *args, C.byref(h)), "br_%s_new" % self.NAME)
        self.h = h

    def _raw(self, what, *args):
        """br_<NAME>_<what> on the handle as it is: the return code (0, or a BR_ERR_* value)."""
        return getattr(lib(), "br_%s_%s" % (self.NAME, what))(self.h, *args)

    def _call(self, what, *args):
        check(self._raw(what, *args), "br_%s_%s" % (self.NAME, what))

    def set_param(self, name, value):
        self._call("set_param", name.encode(), int(value))

    def close(self):
        if self.h:
            self._raw("free")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Collator(_Accumulator):
    """br_collator on `device`: mapped records in any order in, bundles of whole read-name groups out (groups in the order of
    their first record, records in input order inside a group)."""

    NAME = "collator"
    ARGTYPES = {"new": [C.c_int, _P(C.c_void_p)], "add": [C.c_void_p, _P(BrDeviceRecords), C.c_int, C.c_void_p],
                "finish": [C.c_void_p, _P(C.c_int64), _P(C.c_int64)], "next": [C.c_void_p, C.c_int64, _P(BrDeviceRecords)],
                "order": [C.c_void_p, C.c_void_p], "set_param": [C.c_void_p, C.c_char_p, C.c_int64],
                "stats": [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_double), _P(C.c_double)], "free": [C.c_void_p]}

    def __init__(self, device=0):
        self.n = 0
        self._open(device)

    def add_records(self, recs, on_device, stream=None):
        """br_collator_add as it is: the return code (0, or a BR_ERR_* value)."""
        return self._raw("add", C.byref(recs), 1 if on_device else 0, C.c_void_p(stream or 0))

    def add_host(self, stream_np):
        """An uncompressed BAM alignment section in host memory ([block_size][record]..., unmapped records skipped)."""
        data = np.ascontiguousarray(stream_np, dtype=np.uint8)
        off, ln, _, used = bam_split(data)
        assert used == data.size
        recs = BrDeviceRecords(data.ctypes.data if data.size else None, off.ctypes.data if off.size else None, len(off),
                               ln.ctypes.data if ln.size else None)
        check(self.add_records(recs, False), "br_collator_add")

    def add_device(self, blob, rec_off, rec_len):
        """torch CUDA tensors: blob uint8 (each record's block_size in the 4 bytes in front of rec_off[i]), rec_off int64 [n],
        rec_len int32 [n]."""
        import torch
        recs = BrDeviceRecords(blob.data_ptr(), rec_off.data_ptr(), rec_len.numel(), rec_len.data_ptr())
        check(self.add_records(recs, True, torch.cuda.current_stream(blob.device).cuda_stream), "br_collator_add")

    def finish(self):
        n, g = C.c_int64(), C.c_int64()
        self._call("finish", C.byref(n), C.byref(g))
        self.n = int(n.value)
        return self.n, int(g.value)

    def order(self):
        out = np.zeros(max(self.n, 1), dtype=np.int64)
        self._call("order", out.ctypes.data)
        return out[:self.n]

    def next_records(self, max_records):
        """The next bundle as a BrDeviceRecords in HBM (n_aln = 0 at the end)."""
        recs = BrDeviceRecords()
        self._call("next", int(max_records), C.byref(recs))
        return recs

    def stats(self):
        a, p, ad, fi = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double()
        self._call("stats", C.byref(a), C.byref(p), C.byref(ad), C.byref(fi))
        return {"arena_bytes": int(a.value), "peak_bytes": int(p.value), "add_s": ad.value, "finish_s": fi.value}

    def bundles(self, max_records):
        """Yields each bundle's records as a numpy copy: uint8 [block_size][record]... in output order."""
        import torch
        from .device import _DevArray
        dev = "cuda:%d" % self.device
        arena = None
        while True:
            recs = self.next_records(max_records)
            n = int(recs.n_aln)
            if n == 0:
                return
            if arena is None:
                arena = torch.as_tensor(_DevArray(recs.blob, self.stats()["arena_bytes"], "|u1"), device=dev).cpu().numpy()
            off = torch.as_tensor(_DevArray(recs.rec_off, n, "<u8"), device=dev).cpu().numpy().astype(np.int64)
            ln = torch.as_tensor(_DevArray(recs.rec_len, n, "<i4"), device=dev).cpu().numpy().view(np.uint32).astype(np.int64)
            yield np.concatenate([arena[o - 4:o + l] for o, l in zip(off, ln)]).astype(np.uint8)


class BrBgzfSpan(C.Structure):
    _fields_ = [("coffset", C.c_uint64), ("uoffset", C.c_uint64)]


class Sorter(_Accumulator):
    """br_sorter on `device`: projected records ([block_size][record] rows) in, the same records in coordinate order out (key
    (u32)refID << 32 | (u32)(pos + 1) << 1 | reverse strand, ties in the order they were added), and the BAI index of that
    order."""

    NAME = "sorter"
    ARGTYPES = {"new": [C.c_int, _P(C.c_void_p)], "set_param": [C.c_void_p, C.c_char_p, C.c_int64],
                "add": [C.c_void_p, _P(BrDeviceBam), C.c_int, C.c_void_p], "finish": [C.c_void_p, _P(C.c_int64)],
                "next": [C.c_void_p, C.c_uint64, _P(BrDeviceBam)], "order": [C.c_void_p, C.c_void_p],
                "stats": [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_double), _P(C.c_double), _P(C.c_double)],
                "index": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_uint64, _P(C.c_void_p), _P(C.c_uint64)], "free": [C.c_void_p]}

    def __init__(self, device=0):
        lib().br_free_buffer.argtypes = [C.c_void_p]
        self.n = 0
        self._open(device)

    def add_records(self, recs, on_device, stream=None):
        """br_sorter_add as it is: the return code (0, or a BR_ERR_* value)."""
        return self._raw("add", C.byref(recs), 1 if on_device else 0, C.c_void_p(stream or 0))

    @staticmethod
    def row_offsets(stream_np):
        """offsets (uint64, n + 1) of the rows of an uncompressed record stream in host memory"""
        data = np.ascontiguousarray(stream_np, dtype=np.uint8)
        off, p = [0], 0
        while p < data.size:
            p += 4 + int(data[p:p + 4].view("<u4")[0])
            off.append(p)
        assert p == data.size
        return np.asarray(off, dtype=np.uint64)

    def add_host(self, stream_np):
        """An uncompressed record stream in host memory ([block_size][record]..., every record is taken)."""
        data = np.ascontiguousarray(stream_np, dtype=np.uint8)
        off = self.row_offsets(data)
        recs = BrDeviceBam(data.ctypes.data if data.size else None, data.size, off.ctypes.data, len(off) - 1)
        check(self.add_records(recs, False), "br_sorter_add")

    def add_device(self, data, row_off):
        """add_device(data, row_off): torch CUDA tensors, data uint8 ([block_size][record] rows, contiguous) and row_off int64
        [n + 1].  add_device(bam, None): a BrDeviceBam that describes rows in HBM (what project_bam_device or
        project_bam_resident_kept return, or a slice of it); it is read after the null stream's work."""
        import torch
        if isinstance(data, BrDeviceBam):
            check(self.add_records(data, True, None), "br_sorter_add")
            return
        recs = BrDeviceBam(data.data_ptr(), data.numel(), row_off.data_ptr(), row_off.numel() - 1)
        check(self.add_records(recs, True, torch.cuda.current_stream(data.device).cuda_stream), "br_sorter_add")

    def finish(self):
        n = C.c_int64()
        self._call("finish", C.byref(n))
        self.n = int(n.value)
        return self.n

    def order(self):
        out = np.zeros(max(self.n, 1), dtype=np.int64)
        self._call("order", out.ctypes.data)
        return out[:self.n]

    def next_records(self, max_bytes):
        """The next piece as a BrDeviceBam in HBM (n_rows = 0 at the end; valid until the second next call)."""
        piece = BrDeviceBam()
        self._call("next", int(max_bytes), C.byref(piece))
        return piece

    def pieces(self, max_bytes):
        """Yields each piece as numpy copies: (uint8 records, int64 row_off [n_rows + 1])."""
        import torch
        from .device import _DevArray
        dev = "cuda:%d" % self.device
        while True:
            p = self.next_records(max_bytes)
            n = int(p.n_rows)
            if n == 0:
                return
            data = torch.as_tensor(_DevArray(p.data, int(p.n_bytes), "|u1"), device=dev).cpu().numpy().copy()
            off = torch.as_tensor(_DevArray(p.row_off, n + 1, "<u8"), device=dev).cpu().numpy().astype(np.int64)
            yield data, off

    def index(self, n_ref, blocks, eof_coffset):
        """br_sorter_index: blocks = [(coffset, uoffset)] of the BGZF blocks that hold the sorted stream -> the BAI file's bytes."""
        arr = (BrBgzfSpan * max(len(blocks), 1))()
        for k, (co, uo) in enumerate(blocks):
            arr[k].coffset, arr[k].uoffset = int(co), int(uo)
        out, n = C.c_void_p(), C.c_uint64()
        self._call("index", int(n_ref), C.cast(arr, C.c_void_p), len(blocks), int(eof_coffset), C.byref(out), C.byref(n))
        try:
            return C.string_at(out.value, n.value)
        finally:
            lib().br_free_buffer(out)

    def stats(self):
        a, p, ad, fi, nx = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double(), C.c_double()
        self._call("stats", C.byref(a), C.byref(p), C.byref(ad), C.byref(fi), C.byref(nx))
        return {"arena_bytes": int(a.value), "peak_bytes": int(p.value), "add_s": ad.value, "finish_s": fi.value, "next_s": nx.value}


class Quant(_Accumulator):
    """br_quant on `device`: read names (the rows of projected batches) in, equivalence classes and the EM's per-transcript
    abundances out.  lengths: one per transcript (None: no length normalisation)."""

    NAME = "quant"
    ARGTYPES = {"new": [C.c_int, C.c_int64, C.c_void_p, _P(C.c_void_p)], "set_param": [C.c_void_p, C.c_char_p, C.c_int64],
                "set_tolerance": [C.c_void_p, C.c_double], "set_vb_prior": [C.c_void_p, C.c_double],
                "add": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p],
                "add_rows": [C.c_void_p, _P(BrDeviceRows), C.c_void_p, C.c_int64, C.c_int, C.c_void_p], "add_last": [C.c_void_p, C.c_void_p],
                "fld": [C.c_void_p, C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)], "eff_lengths": [C.c_void_p, C.c_void_p],
                "finish": [C.c_void_p, _P(C.c_int64), _P(C.c_int64)], "classes": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                "em": [C.c_void_p, _P(C.c_int32), _P(C.c_double)], "result": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                "stats": [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_double), _P(C.c_double), _P(C.c_double), _P(C.c_uint64),
                          _P(C.c_int64), _P(C.c_int64)], "free": [C.c_void_p],
                "bootstrap": [C.c_void_p, C.c_void_p], "boot_counts": [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p],
                "boot_theta": [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p], "boot_summary": [C.c_void_p, C.c_void_p, C.c_void_p],
                "boot_stats": [C.c_void_p, _P(C.c_double), _P(C.c_double), _P(C.c_int64)],
                "genes": [C.c_void_p, C.c_void_p, C.c_int64, _P(C.c_int64)],
                "gene_classes": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                "gene_result": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                "gene_boot": [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p], "gene_boot_summary": [C.c_void_p, C.c_void_p, C.c_void_p],
                "gene_stats": [C.c_void_p, _P(C.c_double), _P(C.c_int64), _P(C.c_uint64)],
                "name_classes": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p], "posteriors": [C.c_void_p, C.c_void_p],
                "drop_names": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, _P(C.c_int64)]}

    def __init__(self, n_transcripts, lengths=None, device=0, vb=None, vb_prior=None, vb_per_nucleotide=None):
        self.n_transcripts = int(n_transcripts)
        self.n_names = self.n_classes = 0
        self.n_genes = self.n_gene_classes = 0
        self.eff_len = False
        self.fld_max = 1000
        self.bootstraps = 0
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int64)
        assert lens is None or lens.size == self.n_transcripts
        self._open(device, self.n_transcripts, lens.ctypes.data if lens is not None else None)
        if lens is None:
            self.set_param("length_norm", 0)
        for name, value in (("vb", vb), ("vb_prior", vb_prior), ("vb_per_nucleotide", vb_per_nucleotide)):
            if value is not None:
                self.set_param(name, value)

    def set_param(self, name, value):
        """"vb", "vb_per_nucleotide" (0 / 1: the variational Bayes EM and its prior per nucleotide), "vb_prior" (a float), "hash_bits", "length_norm", "max_iters", "eff_len", "fld_max", "keep_names", "bootstraps", "boot_seed" (the bits of an int64: a seed
        of 2^63 or more is taken modulo 2^64), "boot_chunk" (integers) or "tolerance" (a float)."""
        if name == "tolerance":
            self._call("set_tolerance", float(value))
        elif name == "vb_prior":
            self._call("set_vb_prior", float(value))
        else:
            if name == "boot_seed":
                value = C.c_int64(int(value) & 0xffffffffffffffff).value
            super().set_param(name, value)
            if name == "fld_max":
                self.fld_max = int(value)
            if name == "bootstraps":
                self.bootstraps = int(value)
            if name == "eff_len":
                self.eff_len = bool(value)

    def add_raw(self, a, row_off, group_off, n_groups, on_device, stream=None):
        """br_quant_add as it is: the return code (0, or a BR_ERR_* value)."""
        return self._raw("add", C.c_void_p(a), C.c_void_p(row_off), C.c_void_p(group_off), int(n_groups), 1 if on_device else 0,
                         C.c_void_p(stream or 0))

    def add_host(self, rows_a, row_off, group_off):
        """rows_a: uint32 [n_rows, 4] (br_row_a: transcript_id, pos, meta, nh), row_off uint64 [n_aln + 1], group_off uint32
        [n_groups + 1], in host memory."""
        a = np.ascontiguousarray(rows_a, dtype=np.uint32).reshape(-1, 4)
        ro = np.ascontiguousarray(row_off, dtype=np.uint64)
        go = np.ascontiguousarray(group_off, dtype=np.uint32)
        check(self.add_raw(a.ctypes.data if a.size else None, ro.ctypes.data, go.ctypes.data, len(go) - 1, False), "br_quant_add")

    def add_device(self, rows_a, row_off, group_off, g0=0, g1=None):
        """The same tables as torch CUDA tensors (rows_a int32 / uint8 storage of br_row_a, row_off int64, group_off int32); the
        read names [g0, g1) of them are added."""
        import torch
        g1 = group_off.numel() - 1 if g1 is None else g1
        check(self.add_raw(rows_a.data_ptr(), row_off.data_ptr(), group_off.data_ptr() + 4 * g0, g1 - g0, True,
                           torch.cuda.current_stream(row_off.device).cuda_stream), "br_quant_add")

    def add_rows_raw(self, a, cigar, pool, row_off, n_rows, n_pool_words, group_off, n_groups, on_device, stream=None):
        """br_quant_add_rows as it is (the tables as addresses): the return code (0, or a BR_ERR_* value)."""
        rows = BrDeviceRows()
        rows.n_rows, rows.n_pool_words = int(n_rows), int(n_pool_words)
        rows.a, rows.cigar, rows.pool, rows.row_off = a, cigar, pool, row_off
        return self._raw("add_rows", C.byref(rows), C.c_void_p(group_off), int(n_groups), 1 if on_device else 0, C.c_void_p(stream or 0))

    def add_rows_host(self, rows_a, cigar, pool, row_off, group_off):
        """add_host with the whole row table: cigar uint64 [n_rows] (the ops themselves up to two, else an offset into pool),
        pool uint32, in host memory."""
        a = np.ascontiguousarray(rows_a, dtype=np.uint32).reshape(-1, 4)
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        pl = np.ascontiguousarray(pool, dtype=np.uint32)
        ro = np.ascontiguousarray(row_off, dtype=np.uint64)
        go = np.ascontiguousarray(group_off, dtype=np.uint32)
        assert len(cg) == len(a)
        check(self.add_rows_raw(a.ctypes.data if a.size else None, cg.ctypes.data, pl.ctypes.data if pl.size else None, ro.ctypes.data,
                                len(a), len(pl), go.ctypes.data, len(go) - 1, False), "br_quant_add_rows")

    def add_rows_device(self, rows_a, cigar, pool, row_off, group_off, g0=0, g1=None):
        """The same tables as torch CUDA tensors (cigar int64, pool int32); the read names [g0, g1) of them are added."""
        import torch
        g1 = group_off.numel() - 1 if g1 is None else g1
        check(self.add_rows_raw(rows_a.data_ptr(), cigar.data_ptr(), pool.data_ptr() if pool.numel() else None, row_off.data_ptr(),
                                cigar.numel(), pool.numel(), group_off.data_ptr() + 4 * g0, g1 - g0, True,
                                torch.cuda.current_stream(row_off.device).cuda_stream), "br_quant_add_rows")

    def add_last(self, ctx):
        """The read names of the last projection call on `ctx` (a Context), from where that call left them in HBM."""
        self._call("add_last", ctx.h)

    def drop_names(self, flags):
        """Before finish: the names with a non-zero flag count as names without rows.  flags: a finished Dedup (its duplicates, from
        where they lie in HBM), a torch CUDA uint8 tensor or a host array, one byte per name added -> the names dropped."""
        k = C.c_int64()
        if isinstance(flags, Dedup):
            ptr, n = flags.flags()
            self._call("drop_names", C.c_void_p(ptr), n, 1, C.byref(k))
        elif hasattr(flags, "data_ptr"):
            self._call("drop_names", C.c_void_p(flags.data_ptr() if flags.numel() else None), flags.numel(), 1, C.byref(k))
        else:
            f = np.ascontiguousarray(flags, dtype=np.uint8)
            self._call("drop_names", C.c_void_p(f.ctypes.data if f.size else None), f.size, 0, C.byref(k))
        return int(k.value)

    def finish(self):
        n, c = C.c_int64(), C.c_int64()
        self._call("finish", C.byref(n), C.byref(c))
        self.n_names, self.n_classes = int(n.value), int(c.value)
        return self.n_names, self.n_classes

    def classes(self):
        """-> (label_off uint64 [C + 1], labels uint32, counts uint64 [C], first_name uint64 [C])"""
        nc = self.n_classes
        off = np.zeros(nc + 1, dtype=np.uint64)
        cnt, first = np.zeros(max(nc, 1), dtype=np.uint64), np.zeros(max(nc, 1), dtype=np.uint64)
        self._call("classes", off.ctypes.data, None, None, None)
        labels = np.zeros(max(int(off[-1]), 1), dtype=np.uint32)
        self._call("classes", None, labels.ctypes.data, cnt.ctypes.data, first.ctypes.data)
        return off, labels[:int(off[-1])], cnt[:nc], first[:nc]

    def em(self):
        """-> (iterations, the last relative change looked at)"""
        n, r = C.c_int32(), C.c_double()
        self._call("em", C.byref(n), C.byref(r))
        return int(n.value), float(r.value)

    def result(self, em=True):
        """-> dict of theta, tpm (float64; with em) and unique, ambig (uint64), one entry per transcript"""
        nt = max(self.n_transcripts, 1)
        out = {"unique": np.zeros(nt, dtype=np.uint64), "ambig": np.zeros(nt, dtype=np.uint64)}
        if em:
            out["theta"], out["tpm"] = np.zeros(nt, dtype=np.float64), np.zeros(nt, dtype=np.float64)
        self._call("result", out["theta"].ctypes.data if em else None, out["tpm"].ctypes.data if em else None, out["unique"].ctypes.data,
                   out["ambig"].ctypes.data)
        return {k: v[:self.n_transcripts] for k, v in out.items()}

    def bootstrap(self):
        """The "bootstraps" replicates: resampled counts and an EM each -> the iterations every replicate ran (int32 [B])"""
        it = np.zeros(max(self.bootstraps, 1), dtype=np.int32)
        self._call("bootstrap", it.ctypes.data)
        return it[:self.bootstraps]

    def boot_counts(self, first=0, count=None):
        """-> uint32 [count, C]: the resampled class counts of replicates first .. first + count - 1, generated again"""
        count = self.bootstraps - first if count is None else count
        out = np.zeros(max(count * self.n_classes, 1), dtype=np.uint32)
        self._call("boot_counts", first, count, out.ctypes.data)
        return out[:count * self.n_classes].reshape(count, self.n_classes)

    def boot_theta(self, first=0, count=None):
        """-> float64 [count, T]: theta of replicates first .. first + count - 1 (after bootstrap)"""
        count = self.bootstraps - first if count is None else count
        out = np.zeros(max(count * self.n_transcripts, 1), dtype=np.float64)
        self._call("boot_theta", first, count, out.ctypes.data)
        return out[:count * self.n_transcripts].reshape(count, self.n_transcripts)

    def boot_summary(self):
        """-> (mean, var) per transcript over the replicates (var over B - 1; 0 for B = 1)"""
        mean, var = np.zeros(max(self.n_transcripts, 1), dtype=np.float64), np.zeros(max(self.n_transcripts, 1), dtype=np.float64)
        self._call("boot_summary", mean.ctypes.data, var.ctypes.data)
        return mean[:self.n_transcripts], var[:self.n_transcripts]

    def boot_stats(self):
        s, e, n = C.c_double(), C.c_double(), C.c_int64()
        self._call("boot_stats", C.byref(s), C.byref(e), C.byref(n))
        return {"sample_s": s.value, "em_s": e.value, "iterations_total": int(n.value)}

    def genes_raw(self, tx_gene, n_genes):
        """br_quant_genes as it is (tx_gene: an address or None): the return code (0, or a BR_ERR_* value)."""
        return self._raw("genes", C.c_void_p(tx_gene), int(n_genes), None)

    def genes(self, tx_gene, n_genes):
        """The gene tables from tx_gene (one gene number below n_genes per transcript), after finish -> the number of gene classes"""
        m = np.ascontiguousarray(tx_gene, dtype=np.uint32)
        assert m.size == self.n_transcripts
        n = C.c_int64()
        self._call("genes", m.ctypes.data if m.size else None, int(n_genes), C.byref(n))
        self.n_genes, self.n_gene_classes = int(n_genes), int(n.value)
        return self.n_gene_classes

    def gene_classes(self):
        """-> (label_off uint64 [C + 1], labels uint32, counts uint64 [C], first_name uint64 [C]) of the gene classes"""
        nc = self.n_gene_classes
        off = np.zeros(nc + 1, dtype=np.uint64)
        cnt, first = np.zeros(max(nc, 1), dtype=np.uint64), np.zeros(max(nc, 1), dtype=np.uint64)
        self._call("gene_classes", off.ctypes.data, None, None, None)
        labels = np.zeros(max(int(off[-1]), 1), dtype=np.uint32)
        self._call("gene_classes", None, labels.ctypes.data, cnt.ctypes.data, first.ctypes.data)
        return off, labels[:int(off[-1])], cnt[:nc], first[:nc]

    def gene_result(self, em=True):
        """-> dict of num_reads, tpm, length (float64; with em; eff_length as well with "eff_len" on) and unique, ambig (uint64),
        n_transcripts (uint32), one entry per gene"""
        ng = max(self.n_genes, 1)
        out = {"unique": np.zeros(ng, dtype=np.uint64), "ambig": np.zeros(ng, dtype=np.uint64), "n_transcripts": np.zeros(ng, dtype=np.uint32)}
        fl = (["num_reads", "tpm", "length"] + (["eff_length"] if self.eff_len else [])) if em else []
        for k in fl:
            out[k] = np.zeros(ng, dtype=np.float64)
        ptr = [out[k].ctypes.data if k in out else None for k in ("num_reads", "tpm", "length", "eff_length", "unique", "ambig", "n_transcripts")]
        self._call("gene_result", *ptr)
        return {k: v[:self.n_genes] for k, v in out.items()}

    def gene_boot(self, first=0, count=None):
        """-> float64 [count, G]: the genes' num_reads of replicates first .. first + count - 1 (after genes and bootstrap)"""
        count = self.bootstraps - first if count is None else count
        out = np.zeros(max(count * self.n_genes, 1), dtype=np.float64)
        self._call("gene_boot", first, count, out.ctypes.data)
        return out[:count * self.n_genes].reshape(count, self.n_genes)

    def gene_boot_summary(self):
        """-> (mean, var) per gene over the replicates (var over B - 1; 0 for B = 1)"""
        mean, var = np.zeros(max(self.n_genes, 1), dtype=np.float64), np.zeros(max(self.n_genes, 1), dtype=np.float64)
        self._call("gene_boot_summary", mean.ctypes.data, var.ctypes.data)
        return mean[:self.n_genes], var[:self.n_genes]

    def gene_stats(self):
        s, n, co = C.c_double(), C.c_int64(), C.c_uint64()
        self._call("gene_stats", C.byref(s), C.byref(n), C.byref(co))
        return {"seconds": s.value, "n_gene_labels": int(n.value), "collisions": int(co.value)}

    def name_classes(self, first=0, n=None):
        """-> uint32 [n]: the class of add-order names first .. first + n - 1, 0xffffffff for a name without rows ("keep_names" = 1,
        after finish)"""
        n = self.n_names - first if n is None else n
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._call("name_classes", int(first), int(n), out.ctypes.data)
        return out[:n]

    def posteriors(self, fetch=True):
        """-> float64 [n_labels]: the posterior of every label entry, parallel to classes()[1] (after em); fetch = False only makes
        the table on the device"""
        if not fetch:
            self._call("posteriors", None)
            return None
        out = np.zeros(max(self.stats()["n_labels"], 1), dtype=np.float64)
        self._call("posteriors", out.ctypes.data)
        return out[:self.stats()["n_labels"]]

    def fld(self):
        """-> dict of hist (uint64 [fld_max + 1]: observed fragment lengths of the read names of one label) and n_obs,
        n_no_fragment, n_out_of_range, of the adds so far"""
        hist = np.zeros(self.fld_max + 1, dtype=np.uint64)
        n, u, r = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._call("fld", hist.ctypes.data, C.byref(n), C.byref(u), C.byref(r))
        return {"hist": hist, "n_obs": int(n.value), "n_no_fragment": int(u.value), "n_out_of_range": int(r.value)}

    def eff_lengths(self):
        """-> float64 per transcript: the effective lengths ("eff_len" = 1, after finish)"""
        eff = np.zeros(max(self.n_transcripts, 1), dtype=np.float64)
        self._call("eff_lengths", eff.ctypes.data)
        return eff[:self.n_transcripts]

    def stats(self):
        h, p, co = C.c_uint64(), C.c_uint64(), C.c_uint64()
        ad, fi, em = C.c_double(), C.c_double(), C.c_double()
        un, nl = C.c_int64(), C.c_int64()
        self._call("stats", C.byref(h), C.byref(p), C.byref(ad), C.byref(fi), C.byref(em), C.byref(co), C.byref(un), C.byref(nl))
        return {"held_bytes": int(h.value), "peak_bytes": int(p.value), "add_s": ad.value, "finish_s": fi.value, "em_s": em.value,
                "collisions": int(co.value), "n_unassigned": int(un.value), "n_labels": int(nl.value)}


def quant_digamma(a, device=0):
    """br_quant_digamma: the device's psi (br_quant's `psi`) over a float64 array -> an array of its shape"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.zeros(max(a.size, 1), dtype=np.float64)
    L = lib()
    L.br_quant_digamma.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    check(L.br_quant_digamma(int(device), a.ctypes.data if a.size else None, a.size, out.ctypes.data), "br_quant_digamma")
    return out[:a.size].reshape(a.shape)


class BrBigwigOpts(C.Structure):  # br_bigwig_opts: a field that is 0 takes its default
    _fields_ = [("items_per_slot", C.c_uint32), ("block_size", C.c_uint32), ("zoom_levels", C.c_int32), ("first_reduction", C.c_uint32),
                ("compress", C.c_int32)]


def zlib_sections(device, payloads, mode=0):
    """br_zlib_sections_device: every payload (bytes, at most 131072 each) as a zlib stream of its own, made on `device` -> list of
    bytes.  mode 0: one fixed-Huffman block, or stored where that is not smaller than the payload; 1: stored."""
    payloads = [bytes(p) for p in payloads]
    src = np.frombuffer(b"".join(payloads), dtype=np.uint8)
    off = np.zeros(len(payloads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in payloads], dtype=np.uint64)
    out_off = np.zeros(len(payloads) + 1, dtype=np.uint64)
    out = C.c_void_p()
    L = lib()
    L.br_zlib_sections_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, _P(C.c_void_p), C.c_void_p]
    L.br_free_buffer.argtypes = [C.c_void_p]
    check(L.br_zlib_sections_device(int(device), src.ctypes.data if src.size else None, off.ctypes.data, len(payloads), int(mode), C.byref(out),
                                    out_off.ctypes.data), "br_zlib_sections_device")
    try:
        blob = C.string_at(out.value, int(out_off[-1]))
    finally:
        L.br_free_buffer(out)
    return [blob[int(a):int(b)] for a, b in zip(out_off, out_off[1:])]


class Coverage(_Accumulator):
    """br_coverage on `device`: the rows of projected batches in, the depth of coverage along every transcript out (runs of equal
    depth, per-transcript summary, the depth itself).  lengths: one per transcript.  set_param: "primary_only" 0 / 1 and "weight"
    0 / 1 / 2 (unit, 1 / NH, the EM's posteriors: WEIGHTS), before the first add.  In a weighted mode a depth is a uint64 in units
    of 2^-32 and runs64 / depth64 / summary64 are the getters; weight em takes add_names_* (or add_last) and finish_em(quant)."""

    WEIGHTS = {"unit": 0, "nh": 1, "em": 2}

    RUN_PAGE = 1 << 20

    NAME = "coverage"
    ARGTYPES = {"new": [C.c_int, C.c_int64, C.c_void_p, _P(C.c_void_p)], "set_param": [C.c_void_p, C.c_char_p, C.c_int64],
                "add_rows": [C.c_void_p, _P(BrDeviceRows), C.c_int64, C.c_int64, C.c_int, C.c_void_p], "add_last": [C.c_void_p, C.c_void_p],
                "finish": [C.c_void_p, _P(C.c_int64)], "runs": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                "depth": [C.c_void_p, C.c_int64, C.c_void_p], "summary": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                "stats": [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_double),
                          _P(C.c_double)], "free": [C.c_void_p],
                "add_names": [C.c_void_p, _P(BrDeviceRows), C.c_void_p, C.c_int64, C.c_int, C.c_void_p],
                "finish_em": [C.c_void_p, C.c_void_p, _P(C.c_int64)],
                "runs64": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                "depth64": [C.c_void_p, C.c_int64, C.c_void_p], "summary64": [C.c_void_p] * 7,
                "bigwig": [C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_uint64)], "bigwig_read": [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p],
                "bigwig_stats": [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_int32), C.c_void_p, _P(C.c_uint64), _P(C.c_uint64),
                                 _P(C.c_uint64), _P(C.c_double)]}
    BIGWIG_PAGE = 64 << 20

    def __init__(self, lengths, device=0):
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int64)
        self.n_transcripts = int(self.lengths.size)
        self.n_runs = 0
        self._open(device, self.n_transcripts, self.lengths.ctypes.data if self.n_transcripts else None)

    def add_rows_raw(self, a, cigar, pool, n_rows, n_pool_words, r0, r1, on_device, stream=None):
        """br_coverage_add_rows as it is (the tables as addresses): the return code (0, or a BR_ERR_* value)."""
        rows = BrDeviceRows()
        rows.n_rows, rows.n_pool_words = int(n_rows), int(n_pool_words)
        rows.a, rows.cigar, rows.pool = a, cigar, pool
        return self._raw("add_rows", C.byref(rows), int(r0), int(r1), 1 if on_device else 0, C.c_void_p(stream or 0))

    def add_rows_host(self, rows_a, cigar, pool, r0=0, r1=None):
        """rows_a: uint32 [n_rows, 4] (br_row_a: transcript_id, pos, meta, nh), cigar uint64 [n_rows] (the ops themselves up to two,
        else an offset into pool), pool uint32, in host memory; the rows [r0, r1) of them are added."""
        a = np.ascontiguousarray(rows_a, dtype=np.uint32).reshape(-1, 4)
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        pl = np.ascontiguousarray(pool, dtype=np.uint32)
        assert len(cg) == len(a)
        r1 = len(a) if r1 is None else r1
        check(self.add_rows_raw(a.ctypes.data if a.size else None, cg.ctypes.data if cg.size else None, pl.ctypes.data if pl.size else None,
                                len(a), len(pl), r0, r1, False), "br_coverage_add_rows")

    def add_rows_device(self, rows_a, cigar, pool, r0=0, r1=None):
        """The same tables as torch CUDA tensors (rows_a int32 / uint8 storage of br_row_a, cigar int64, pool int32)."""
        import torch
        r1 = cigar.numel() if r1 is None else r1
        check(self.add_rows_raw(rows_a.data_ptr() if cigar.numel() else None, cigar.data_ptr() if cigar.numel() else None,
                                pool.data_ptr() if pool.numel() else None, cigar.numel(), pool.numel(), r0, r1, True,
                                torch.cuda.current_stream(cigar.device).cuda_stream), "br_coverage_add_rows")

    def add_last(self, ctx):
        """All rows of the last projection call on `ctx` (a Context), from where that call left them in HBM."""
        self._call("add_last", ctx.h)

    def add_names_raw(self, a, cigar, pool, row_off, n_rows, n_pool_words, group_off, n_groups, on_device, stream=None):
        """br_coverage_add_names as it is (the tables as addresses): the return code (0, or a BR_ERR_* value)."""
        rows = BrDeviceRows()
        rows.n_rows, rows.n_pool_words = int(n_rows), int(n_pool_words)
        rows.a, rows.cigar, rows.pool, rows.row_off = a, cigar, pool, row_off
        return self._raw("add_names", C.byref(rows), C.c_void_p(group_off), int(n_groups), 1 if on_device else 0, C.c_void_p(stream or 0))

    def add_names_host(self, rows_a, cigar, pool, row_off, group_off):
        """The rows of the read names group_off[0 .. n] (the tables of Quant.add_rows_host, in host memory)."""
        a = np.ascontiguousarray(rows_a, dtype=np.uint32).reshape(-1, 4)
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        pl = np.ascontiguousarray(pool, dtype=np.uint32)
        ro = np.ascontiguousarray(row_off, dtype=np.uint64)
        go = np.ascontiguousarray(group_off, dtype=np.uint32)
        assert len(cg) == len(a)
        check(self.add_names_raw(a.ctypes.data if a.size else None, cg.ctypes.data if cg.size else None, pl.ctypes.data if pl.size else None,
                                 ro.ctypes.data, len(a), len(pl), go.ctypes.data, len(go) - 1, False), "br_coverage_add_names")

    def add_names_device(self, rows_a, cigar, pool, row_off, group_off, g0=0, g1=None):
        """The same tables as torch CUDA tensors; the read names [g0, g1) of them are added."""
        import torch
        g1 = group_off.numel() - 1 if g1 is None else g1
        check(self.add_names_raw(rows_a.data_ptr() if cigar.numel() else None, cigar.data_ptr() if cigar.numel() else None,
                                 pool.data_ptr() if pool.numel() else None, row_off.data_ptr(), cigar.numel(), pool.numel(),
                                 group_off.data_ptr() + 4 * g0, g1 - g0, True, torch.cuda.current_stream(row_off.device).cuda_stream),
              "br_coverage_add_names")

    def finish(self):
        n = C.c_int64()
        self._call("finish", C.byref(n))
        self.n_runs = int(n.value)
        return self.n_runs

    def finish_em(self, quant):
        """weight em: finish with the posteriors of `quant` (a Quant with "keep_names", after em, fed the same names)."""
        n = C.c_int64()
        self._call("finish_em", quant.h, C.byref(n))
        self.n_runs = int(n.value)
        return self.n_runs

    def runs64(self, page=None):
        """weighted modes -> (tid, start, end: uint32 [n_runs]; depth: uint64 [n_runs], in units of 2^-32)"""
        page = int(page or self.RUN_PAGE)
        out = [np.zeros(max(self.n_runs, 1), dtype=np.uint32) for _ in range(3)] + [np.zeros(max(self.n_runs, 1), dtype=np.uint64)]
        for first in range(0, self.n_runs, page):
            n = min(page, self.n_runs - first)
            self._call("runs64", first, n, *[o[first:].ctypes.data for o in out])
        return tuple(o[:self.n_runs] for o in out)

    def depth64(self, tid):
        """weighted modes -> uint64 [max(L[tid], 0)]"""
        d = np.zeros(max(int(self.lengths[tid]), 1), dtype=np.uint64)
        self._call("depth64", int(tid), d.ctypes.data)
        return d[:max(int(self.lengths[tid]), 0)]

    def summary64(self):
        """weighted modes -> dict of records, weight_sum, aligned_hi, aligned_lo, covered_bases, max_depth (uint64 per transcript)"""
        nt = max(self.n_transcripts, 1)
        keys = ("records", "weight_sum", "aligned_hi", "aligned_lo", "covered_bases", "max_depth")
        out = {k: np.zeros(nt, dtype=np.uint64) for k in keys}
        self._call("summary64", *[out[k].ctypes.data for k in keys])
        return {k: v[:self.n_transcripts] for k, v in out.items()}

    def runs(self, page=None):
        """-> (tid, start, end, depth), uint32 [n_runs] each, ordered by (tid, start); fetched in pages of `page` runs"""
        page = int(page or self.RUN_PAGE)
        out = [np.zeros(max(self.n_runs, 1), dtype=np.uint32) for _ in range(4)]
        for first in range(0, self.n_runs, page):
            n = min(page, self.n_runs - first)
            self._call("runs", first, n, *[o[first:].ctypes.data for o in out])
        return tuple(o[:self.n_runs] for o in out)

    def depth(self, tid):
        """-> uint32 [max(L[tid], 0)]"""
        d = np.zeros(max(int(self.lengths[tid]), 1), dtype=np.uint32)
        self._call("depth", int(tid), d.ctypes.data)
        return d[:max(int(self.lengths[tid]), 0)]

    def summary(self):
        """-> dict of records, aligned_bases, covered_bases (uint64) and max_depth (uint32), one entry per transcript"""
        nt = max(self.n_transcripts, 1)
        out = {"records": np.zeros(nt, dtype=np.uint64), "aligned_bases": np.zeros(nt, dtype=np.uint64),
               "covered_bases": np.zeros(nt, dtype=np.uint64), "max_depth": np.zeros(nt, dtype=np.uint32)}
        self._call("summary", out["records"].ctypes.data, out["aligned_bases"].ctypes.data, out["covered_bases"].ctypes.data,
                   out["max_depth"].ctypes.data)
        return {k: v[:self.n_transcripts] for k, v in out.items()}

    def bigwig_raw(self, names, **opts):
        """br_coverage_bigwig as it is: (the return code, the size of the image).  names: one per transcript, str, bytes or None."""
        arr = (C.c_char_p * max(len(names), 1))(*[n.encode() if isinstance(n, str) else n for n in names])
        o = BrBigwigOpts(**{k: int(v) for k, v in opts.items()})
        n = C.c_uint64()
        return self._raw("bigwig", arr if len(names) else None, C.byref(o) if opts else None, C.byref(n)), int(n.value)

    def bigwig(self, names, page=None, **opts):
        """After finish: the coverage as a bigWig file image, built on the device and read home in pages -> bytes.  opts: the fields of
        br_bigwig_opts (items_per_slot, block_size, zoom_levels, first_reduction, compress)."""
        rc, n = self.bigwig_raw(names, **opts)
        check(rc, "br_coverage_bigwig")
        page = int(page or self.BIGWIG_PAGE)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        for first in range(0, n, page):
            self._call("bigwig_read", first, min(page, n - first), out[first:].ctypes.data)
        return out[:n].tobytes()

    def bigwig_stats(self):
        """of the last bigwig(): chromosomes, sections, zoom_levels, zoom_records (per level), raw_bytes and data_bytes (sections and zoom
        blocks before and after compression), n_bytes (the file), seconds"""
        nc, ns, rb, db, nb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        z, sec = C.c_int32(), C.c_double()
        zr = np.zeros(10, dtype=np.uint64)
        self._call("bigwig_stats", C.byref(nc), C.byref(ns), C.byref(z), zr.ctypes.data, C.byref(rb), C.byref(db), C.byref(nb), C.byref(sec))
        return {"chromosomes": int(nc.value), "sections": int(ns.value), "zoom_levels": int(z.value),
                "zoom_records": [int(v) for v in zr[:z.value]], "raw_bytes": int(rb.value), "data_bytes": int(db.value),
                "n_bytes": int(nb.value), "seconds": sec.value}

    def stats(self):
        rc, rs, cb, h, p = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        ad, fi = C.c_double(), C.c_double()
        self._call("stats", C.byref(rc), C.byref(rs), C.byref(cb), C.byref(h), C.byref(p), C.byref(ad), C.byref(fi))
        return {"rows_counted": int(rc.value), "rows_skipped": int(rs.value), "clipped_bases": int(cb.value), "held_bytes": int(h.value),
                "peak_bytes": int(p.value), "add_s": ad.value, "finish_s": fi.value}


class Assign(_Accumulator):
    """br_assign on `device`: the rows of projected batches by read name, and (or not: on every add or on none) the records they
    were encoded to, in; after finish(quant) the posterior weight w of every record's placement (values), and the records again
    with ZW:f appended -- all of them ("mode" 0, tag) or one drawn placement per read name ("mode" 1, sample: MODES).  set_param:
    "mode", "seed", "long_reads", "max_bytes", before the first add."""

    MODES = {"tag": 0, "sample": 1}
    BAD = ("names", "classes", "transcripts", "posteriors")

    NAME = "assign"
    ARGTYPES = {"new": [C.c_int, _P(C.c_void_p)], "set_param": [C.c_void_p, C.c_char_p, C.c_int64],
                "add": [C.c_void_p, C.c_void_p, _P(BrDeviceRows), C.c_void_p, C.c_int64, C.c_int, C.c_void_p],
                "add_last": [C.c_void_p, C.c_void_p], "finish": [C.c_void_p, C.c_void_p, _P(C.c_int64), _P(C.c_int64)],
                "values": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
                "next": [C.c_void_p, C.c_uint64, _P(BrDeviceBam)],
                "stats": [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_double), _P(C.c_double), _P(C.c_double), C.c_void_p],
                "free": [C.c_void_p]}

    def __init__(self, device=0, **params):
        self.n = self.n_out = self.n_named = 0
        self._open(device)
        for k, v in params.items():
            self.set_param(k, v)

    def add_raw(self, recs, a, row_off, n_rows, group_off, n_groups, on_device, stream=None):
        """br_assign_add as it is (recs: a BrDeviceBam or None; the tables as addresses): the return code (0, or a BR_ERR_* value)."""
        rows = BrDeviceRows()
        rows.n_rows, rows.a, rows.row_off = int(n_rows), a, row_off
        rc = self._raw("add", C.cast(C.byref(recs), C.c_void_p) if recs is not None else None, C.byref(rows), C.c_void_p(group_off), int(n_groups),
                       1 if on_device else 0, C.c_void_p(stream or 0))
        return rc

    def add_host(self, rows_a, row_off, group_off, stream_np=None, rec_off=None):
        """The rows of the read names group_off[0 .. n] (rows_a uint32 [n_rows, 4], row_off uint64 per alignment, in host memory);
        stream_np: the rows' records as an uncompressed record stream in host memory (row i = record i), or None."""
        a = np.ascontiguousarray(rows_a, dtype=np.uint32).reshape(-1, 4)
        ro = np.ascontiguousarray(row_off, dtype=np.uint64)
        go = np.ascontiguousarray(group_off, dtype=np.uint32)
        recs = None
        if stream_np is not None:
            data = np.ascontiguousarray(stream_np, dtype=np.uint8)
            off = Sorter.row_offsets(data) if rec_off is None else np.ascontiguousarray(rec_off, dtype=np.uint64)
            recs = BrDeviceBam(data.ctypes.data if data.size else None, data.size, off.ctypes.data, len(off) - 1)
        check(self.add_raw(recs, a.ctypes.data if a.size else None, ro.ctypes.data, len(a), go.ctypes.data, len(go) - 1, False), "br_assign_add")

    def add_device(self, rows_a, row_off, group_off, n_rows, recs=None, g0=0, g1=None):
        """The same tables as torch CUDA tensors; the read names [g0, g1) of them are added.  recs: a BrDeviceBam of the rows'
        records in HBM (what project_bam_resident_kept returns), or None."""
        import torch
        g1 = group_off.numel() - 1 if g1 is None else g1
        check(self.add_raw(recs, rows_a.data_ptr() if n_rows else None, row_off.data_ptr(), n_rows, group_off.data_ptr() + 4 * g0, g1 - g0, True,
                           torch.cuda.current_stream(row_off.device).cuda_stream), "br_assign_add")

    def add_last(self, ctx):
        """The rows, names and records of the last projection call on `ctx` (a Context), from where that call left them in HBM."""
        self._call("add_last", ctx.h)

    def finish(self, quant):
        """With the posteriors of `quant` (a Quant with "keep_names", after em, fed the same names) -> (records that will be
        written, names with records)."""
        n, m = C.c_int64(), C.c_int64()
        self._call("finish", quant.h, C.byref(n), C.byref(m))
        self.n_out, self.n_named = int(n.value), int(m.value)
        return self.n_out, self.n_named

    def values(self, first, n):
        """-> w (float64), zw (float32), kept (uint8) of the add-order records [first, first + n)"""
        k = max(int(n), 1)
        w, zw, kept = np.zeros(k, np.float64), np.zeros(k, np.float32), np.zeros(k, np.uint8)
        self._call("values", int(first), int(n), w.ctypes.data, zw.ctypes.data, kept.ctypes.data)
        return w[:n], zw[:n], kept[:n]

    def next_records(self, max_bytes):
        """The next piece as a BrDeviceBam in HBM (n_rows = 0 at the end; valid until the second next call)."""
        piece = BrDeviceBam()
        self._call("next", int(max_bytes), C.byref(piece))
        return piece

    pieces = Sorter.pieces

    def stats(self):
        h, p, ad, fi, nx = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double(), C.c_double()
        bad = np.zeros(4, np.uint64)
        self._call("stats", C.byref(h), C.byref(p), C.byref(ad), C.byref(fi), C.byref(nx), bad.ctypes.data)
        out = {"held_bytes": int(h.value), "peak_bytes": int(p.value), "add_s": ad.value, "finish_s": fi.value, "next_s": nx.value}
        out.update({"bad_" + k: int(v) for k, v in zip(self.BAD, bad)})
        return out


class Dedup(_Accumulator):
    """br_dedup on `device`: the rows of projected batches by read name and the records they were encoded to, in; after finish() per
    read name whether it is a PCR copy (result: rep, group_first, dup), the molecules' size histogram (hist) and, with
    "keep_records", the records again without the duplicates' ("mark" 0) or with 0x400 set on them ("mark" 1).  set_param: "method"
    (METHODS), "umi_source" (SOURCES), "umi_sep", "umi_tag", "keep_records", "mark", "max_bytes", "hist_max" before the first add,
    "hash_bits" before finish.  "cell_source" (CELL_SOURCES) and "cell_tag" before the first add: position groups per cell."""

    METHODS = {"unique": 0, "directional": 1}
    SOURCES = {"name": 0, "tag": 1}
    CELL_SOURCES = {"none": 0, "name": 1, "tag": 2}
    STATS = ("names", "names_with_rows", "no_umi", "umi_too_long", "bad_aux", "groups", "nodes", "edges", "sweeps", "max_group_nodes",
             "collisions", "held_bytes", "peak_bytes", "add_us", "finish_us", "records_out")

    NAME = "dedup"
    ARGTYPES = {"new": [C.c_int, _P(C.c_void_p)], "set_param": [C.c_void_p, C.c_char_p, C.c_int64],
                "add": [C.c_void_p, C.c_void_p, _P(BrDeviceRows), C.c_void_p, C.c_int64, C.c_int, C.c_void_p],
                "add_last": [C.c_void_p, C.c_void_p], "finish": [C.c_void_p, _P(C.c_int64), _P(C.c_int64), _P(C.c_int64)],
                "umis": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p],
                "result": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p], "hist": [C.c_void_p, C.c_void_p],
                "flags": [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)], "next": [C.c_void_p, C.c_uint64, _P(BrDeviceBam)],
                "stats": [C.c_void_p, C.c_void_p], "free": [C.c_void_p],
                "set_whitelist": [C.c_void_p, C.c_void_p, C.c_int], "whitelist_stats": [C.c_void_p, C.c_void_p]}

    def __init__(self, device=0, **params):
        self.n_names = self.n_molecules = self.n_duplicates = 0
        self.hist_max = 1000
        self._open(device)
        for k, v in params.items():
            self.set_param(k, v)

    def set_param(self, name, value):
        if name in ("umi_tag", "cell_tag") and not isinstance(value, int):
            b = value.encode() if isinstance(value, str) else bytes(value)
            value = b[0] | b[1] << 8
        if name == "umi_sep" and not isinstance(value, int):
            value = (value.encode() if isinstance(value, str) else bytes(value))[0]
        super().set_param(name, value)
        if name == "hist_max":
            self.hist_max = int(value)

    def add_raw(self, recs, a, cigar, pool, row_off, n_rows, n_pool_words, group_off, n_groups, on_device, stream=None):
        """br_dedup_add as it is (recs: a BrDeviceBam or None; the tables as addresses): the return code (0, or a BR_ERR_* value)."""
        rows = BrDeviceRows()
        rows.n_rows, rows.n_pool_words = int(n_rows), int(n_pool_words)
        rows.a, rows.cigar, rows.pool, rows.row_off = a, cigar, pool, row_off
        return self._raw("add", C.cast(C.byref(recs), C.c_void_p) if recs is not None else None, C.byref(rows), C.c_void_p(group_off), int(n_groups),
                         1 if on_device else 0, C.c_void_p(stream or 0))

    def add_host(self, rows_a, cigar, pool, row_off, group_off, stream_np, rec_off=None):
        """The rows of the read names group_off[0 .. n] (rows_a uint32 [n_rows, 4], cigar uint64 [n_rows], pool uint32, row_off uint64
        per alignment) and their records as an uncompressed record stream (row i = record i), all in host memory."""
        a = np.ascontiguousarray(rows_a, dtype=np.uint32).reshape(-1, 4)
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        pl = np.ascontiguousarray(pool, dtype=np.uint32)
        ro = np.ascontiguousarray(row_off, dtype=np.uint64)
        go = np.ascontiguousarray(group_off, dtype=np.uint32)
        data = np.ascontiguousarray(stream_np, dtype=np.uint8)
        off = Sorter.row_offsets(data) if rec_off is None else np.ascontiguousarray(rec_off, dtype=np.uint64)
        recs = BrDeviceBam(data.ctypes.data if data.size else None, data.size, off.ctypes.data, len(off) - 1)
        check(self.add_raw(recs, a.ctypes.data if a.size else None, cg.ctypes.data if cg.size else None, pl.ctypes.data if pl.size else None,
                           ro.ctypes.data, len(a), len(pl), go.ctypes.data, len(go) - 1, False), "br_dedup_add")

    def add_device(self, rows_a, cigar, pool, row_off, group_off, recs, g0=0, g1=None):
        """The same tables as torch CUDA tensors; the read names [g0, g1) of them are added.  recs: a BrDeviceBam of the rows' records
        in HBM."""
        import torch
        g1 = group_off.numel() - 1 if g1 is None else g1
        n_rows = cigar.numel()
        check(self.add_raw(recs, rows_a.data_ptr() if n_rows else None, cigar.data_ptr() if n_rows else None, pool.data_ptr() if pool.numel() else None,
                           row_off.data_ptr(), n_rows, pool.numel(), group_off.data_ptr() + 4 * g0, g1 - g0, True,
                           torch.cuda.current_stream(row_off.device).cuda_stream), "br_dedup_add")

    def add_last(self, ctx):
        """The rows, names and records of the last projection call on `ctx` (a Context), from where that call left them in HBM."""
        self._call("add_last", ctx.h)

    def set_whitelist(self, whitelist, correct="1mm"):
        """Before finish, with "cell_source": the cell barcodes are resolved against `whitelist` (a Whitelist on this device, kept
        alive here) under `correct` (Whitelist.CORRECT) before the per-cell groups are made."""
        self._call("set_whitelist", whitelist.h if whitelist is not None else None, Whitelist.correct_value(correct))
        self._whitelist = whitelist

    def whitelist_stats(self):
        out = np.zeros(8, np.uint64)
        self._call("whitelist_stats", out.ctypes.data)
        return {k: int(v) for k, v in zip(Whitelist.RESOLVE_STATS, out)}

    def finish(self):
        """-> (names added, molecules, duplicates)"""
        n, m, d = C.c_int64(), C.c_int64(), C.c_int64()
        self._call("finish", C.byref(n), C.byref(m), C.byref(d))
        self.n_names, self.n_molecules, self.n_duplicates = int(n.value), int(m.value), int(d.value)
        return self.n_names, self.n_molecules, self.n_duplicates

    def umis(self, first, n):
        """-> (umi uint8 [n, 32] zero padded, len uint8 [n]) of the add-order names [first, first + n)"""
        k = max(int(n), 1)
        umi, ln = np.zeros((k, 32), np.uint8), np.zeros(k, np.uint8)
        self._call("umis", int(first), int(n), umi.ctypes.data, ln.ctypes.data)
        return umi[:n], ln[:n]

    def result(self, first=0, n=None):
        """-> rep (uint32), group_first (uint32), dup (uint8) of the add-order names [first, first + n)"""
        n = self.n_names - first if n is None else n
        k = max(int(n), 1)
        rep, gf, dup = np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(k, np.uint8)
        self._call("result", int(first), int(n), rep.ctypes.data, gf.ctypes.data, dup.ctypes.data)
        return rep[:n], gf[:n], dup[:n]

    def hist(self):
        h = np.zeros(self.hist_max + 1, np.uint64)
        self._call("hist", h.ctypes.data)
        return h

    def flags(self):
        """-> (the address of dup in HBM, the names)"""
        p, n = C.c_void_p(), C.c_int64()
        self._call("flags", C.byref(p), C.byref(n))
        return p.value, int(n.value)

    def next_records(self, max_bytes):
        """The next piece as a BrDeviceBam in HBM (n_rows = 0 at the end; valid until the second next call)."""
        piece = BrDeviceBam()
        self._call("next", int(max_bytes), C.byref(piece))
        return piece

    pieces = Sorter.pieces

    def stats(self):
        out = np.zeros(16, np.uint64)
        self._call("stats", out.ctypes.data)
        return {k: int(v) for k, v in zip(self.STATS, out)}


class Whitelist(_Accumulator):
    """br_whitelist on `device`: the allowed cell barcodes (a list of bytes / str, 1..32 bytes each), sorted, made distinct and
    hashed into a table in HBM.  Read-only once made: Cells.set_whitelist and Dedup.set_whitelist share one.  match() resolves
    barcodes given directly, one name each."""

    CORRECT = {"exact": 0, "1mm": 1, "1mm-multi": 2}
    STATUS = ("none", "exact", "corrected", "no_match", "ambiguous")
    STATS = ("given", "distinct", "slots", "longest_chain", "build_us", "hash_bits", "held_bytes", "peak_bytes")
    RESOLVE_STATS = ("no_barcode", "exact", "corrected", "no_match", "ambiguous", "distinct_observed", "resolve_us", "correct")
    NONE = 0xffffffff

    NAME = "whitelist"
    ARGTYPES = {"new": [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, _P(C.c_void_p)],
                "barcodes": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p],
                "match": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p],
                "stats": [C.c_void_p, C.c_void_p], "free": [C.c_void_p]}

    @classmethod
    def correct_value(cls, correct):
        return cls.CORRECT[correct] if isinstance(correct, str) else int(correct)

    @staticmethod
    def pack(barcodes):
        """a list of bytes / str / None (no barcode) -> (uint8 [n, 32] zero padded, uint8 [n]); a length above 255 is stored as 255"""
        n = len(barcodes)
        cb, ln = np.zeros((max(n, 1), 32), np.uint8), np.zeros(max(n, 1), np.uint8)
        for i, b in enumerate(barcodes):
            b = b"" if b is None else b.encode() if isinstance(b, str) else bytes(b)
            ln[i] = min(len(b), 255)
            k = min(len(b), 32)
            cb[i, :k] = np.frombuffer(b[:k], np.uint8)
        return cb, ln

    @classmethod
    def new_raw(cls, device, cb, ln, n, hash_bits=64):
        """br_whitelist_new as it is -> (the return code, the handle's value or None)"""
        L = lib()
        L.br_whitelist_new.argtypes = cls.ARGTYPES["new"]
        L.br_whitelist_free.argtypes = cls.ARGTYPES["free"]
        h = C.c_void_p()
        rc = L.br_whitelist_new(int(device), cb.ctypes.data, ln.ctypes.data, int(n), int(hash_bits), C.byref(h))
        if rc == 0:
            L.br_whitelist_free(h)
        return rc, h.value

    def __init__(self, barcodes, device=0, hash_bits=64):
        """barcodes: a list of bytes / str, or what pack() returns: (uint8 [n, 32] zero padded, uint8 [n])"""
        packed = isinstance(barcodes, tuple) and len(barcodes) == 2 and isinstance(barcodes[0], np.ndarray)
        cb, ln = barcodes if packed else self.pack(barcodes)
        cb, ln = np.ascontiguousarray(cb, dtype=np.uint8), np.ascontiguousarray(ln, dtype=np.uint8)
        self._open(device, cb.ctypes.data, ln.ctypes.data, len(ln) if packed else len(barcodes), int(hash_bits))
        self.n = self.stats()["distinct"]

    def barcodes(self, first=0, n=None):
        """-> the distinct entries [first, first + n) as a list of bytes, in entry order"""
        n = self.n - first if n is None else n
        k = max(int(n), 1)
        cb, ln = np.zeros((k, 32), np.uint8), np.zeros(k, np.uint8)
        self._call("barcodes", int(first), int(n), cb.ctypes.data, ln.ctypes.data)
        return [bytes(cb[i, :ln[i]]) for i in range(int(n))]

    def match_raw(self, cb, ln, n, correct):
        """br_whitelist_match as it is -> (the return code, entry uint32 [n], status uint8 [n])"""
        entry, status = np.zeros(max(int(n), 1), np.uint32), np.zeros(max(int(n), 1), np.uint8)
        rc = self._raw("match", cb.ctypes.data, ln.ctypes.data, int(n), int(correct), entry.ctypes.data, status.ctypes.data)
        return rc, entry[:n], status[:n]

    def match(self, barcodes, correct="1mm"):
        """barcodes: one per name (bytes / str, None or empty: no barcode) -> (entry uint32, NONE for none; status uint8)"""
        cb, ln = self.pack(barcodes)
        rc, entry, status = self.match_raw(cb, ln, len(barcodes), self.correct_value(correct))
        check(rc, "br_whitelist_match")
        return entry, status

    def stats(self):
        out = np.zeros(8, np.uint64)
        self._call("stats", out.ctypes.data)
        return {k: int(v) for k, v in zip(self.STATS, out)}


class Cells(_Accumulator):
    """br_cells on `device`: the names of projected batches and the records they were encoded to, in; after finish(quant, tx_feature,
    n_features) the cell x feature matrix of the quantifier's classes (matrix: CSR by cell), the cells' barcodes and numbers.
    set_param before the first add: "barcode_source" (SOURCES), "barcode_sep", "barcode_tag", "mode" (MODES), "max_iters", "hash_bits",
    "lds_bytes"; `tolerance` likewise."""

    SOURCES = {"name": 0, "tag": 1}
    MODES = {"unique": 0, "uniform": 1, "em": 2}
    STATS = ("names", "counted", "no_barcode", "barcode_too_long", "bad_aux", "cells", "entries", "pairs", "slots", "matrix_entries",
             "wave_cells", "block_cells", "hbm_cells", "add_us", "finish_us", "values_us")

    NAME = "cells"
    ARGTYPES = {"new": [C.c_int, _P(C.c_void_p)], "set_param": [C.c_void_p, C.c_char_p, C.c_int64], "set_tolerance": [C.c_void_p, C.c_double],
                "add": [C.c_void_p, C.c_void_p, _P(BrDeviceRows), C.c_void_p, C.c_int64, C.c_int, C.c_void_p],
                "add_last": [C.c_void_p, C.c_void_p], "barcodes": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p],
                "finish": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, _P(C.c_int64), _P(C.c_int64)],
                "cell_barcodes": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p],
                "name_cells": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p],
                "matrix": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
                "cell_stats": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                "stats": [C.c_void_p, C.c_void_p], "free": [C.c_void_p],
                "set_whitelist": [C.c_void_p, C.c_void_p, C.c_int], "name_status": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p],
                "whitelist_stats": [C.c_void_p, C.c_void_p], "call": [C.c_void_p, C.c_void_p, C.c_int64],
                "matrix_called": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]}

    def __init__(self, device=0, tolerance=None, **params):
        self.n_cells = self.n_entries = 0
        self._open(device)
        for k, v in params.items():
            self.set_param(k, v)
        if tolerance is not None:
            self.set_tolerance(tolerance)

    def set_param(self, name, value):
        if name == "barcode_tag" and not isinstance(value, int):
            b = value.encode() if isinstance(value, str) else bytes(value)
            value = b[0] | b[1] << 8
        if name == "barcode_sep" and not isinstance(value, int):
            value = (value.encode() if isinstance(value, str) else bytes(value))[0]
        super().set_param(name, value)

    def set_tolerance(self, tolerance):
        self._call("set_tolerance", float(tolerance))

    def set_whitelist(self, whitelist, correct="1mm"):
        """Before finish: the barcodes are resolved against `whitelist` (a Whitelist on this device, kept alive here) under
        `correct` (Whitelist.CORRECT) before the cells are made."""
        self._call("set_whitelist", whitelist.h if whitelist is not None else None, Whitelist.correct_value(correct))
        self._whitelist = whitelist

    def name_status(self, first, n):
        """After a finish with a whitelist -> uint8 per add-order name (Whitelist.STATUS)"""
        out = np.zeros(max(int(n), 1), np.uint8)
        self._call("name_status", int(first), int(n), out.ctypes.data)
        return out[:n]

    def whitelist_stats(self):
        out = np.zeros(8, np.uint64)
        self._call("whitelist_stats", out.ctypes.data)
        return {k: int(v) for k, v in zip(Whitelist.RESOLVE_STATS, out)}

    def add_raw(self, recs, row_off, n_rows, group_off, n_groups, on_device, stream=None):
        """br_cells_add as it is (recs: a BrDeviceBam or None; the tables as addresses): the return code (0, or a BR_ERR_* value)."""
        rows = BrDeviceRows()
        rows.n_rows, rows.n_pool_words = int(n_rows), 0
        rows.a, rows.cigar, rows.pool, rows.row_off = None, None, None, row_off
        return self._raw("add", C.cast(C.byref(recs), C.c_void_p) if recs is not None else None, C.byref(rows), C.c_void_p(group_off), int(n_groups),
                         1 if on_device else 0, C.c_void_p(stream or 0))

    def add_host(self, row_off, group_off, stream_np, rec_off=None):
        """The read names group_off[0 .. n] (row_off uint64 per alignment) and their rows' records as an uncompressed record stream
        (row i = record i), all in host memory."""
        ro = np.ascontiguousarray(row_off, dtype=np.uint64)
        go = np.ascontiguousarray(group_off, dtype=np.uint32)
        data = np.ascontiguousarray(stream_np, dtype=np.uint8)
        off = Sorter.row_offsets(data) if rec_off is None else np.ascontiguousarray(rec_off, dtype=np.uint64)
        recs = BrDeviceBam(data.ctypes.data if data.size else None, data.size, off.ctypes.data, len(off) - 1)
        check(self.add_raw(recs, ro.ctypes.data, len(off) - 1, go.ctypes.data, len(go) - 1, False), "br_cells_add")

    def add_device(self, row_off, group_off, recs, g0=0, g1=None):
        """The same tables as torch CUDA tensors; the read names [g0, g1) of them are added.  recs: a BrDeviceBam of the rows' records
        in HBM."""
        import torch
        g1 = group_off.numel() - 1 if g1 is None else g1
        check(self.add_raw(recs, row_off.data_ptr(), recs.n_rows, group_off.data_ptr() + 4 * g0, g1 - g0, True,
                           torch.cuda.current_stream(row_off.device).cuda_stream), "br_cells_add")

    def add_last(self, ctx):
        """The names and records of the last projection call on `ctx` (a Context), from where that call left them in HBM."""
        self._call("add_last", ctx.h)

    @staticmethod
    def _barcode_list(cb, ln):
        return [bytes(cb[i, :ln[i]]) if ln[i] else None for i in range(len(ln))]

    def barcodes(self, first, n):
        """-> (barcode uint8 [n, 32] zero padded, len uint8 [n]) of the add-order names [first, first + n)"""
        k = max(int(n), 1)
        cb, ln = np.zeros((k, 32), np.uint8), np.zeros(k, np.uint8)
        self._call("barcodes", int(first), int(n), cb.ctypes.data, ln.ctypes.data)
        return cb[:n], ln[:n]

    def finish_raw(self, quant, tx_feature, n_features):
        """br_cells_finish as it is -> the return code"""
        tf = np.ascontiguousarray(tx_feature, dtype=np.uint32)
        n, z = C.c_int64(), C.c_int64()
        rc = self._raw("finish", quant.h if quant is not None else None, tf.ctypes.data if tf.size else None, int(n_features), C.byref(n), C.byref(z))
        if rc == 0:
            self.n_cells, self.n_entries = int(n.value), int(z.value)
        return rc

    def finish(self, quant, tx_feature, n_features):
        """quant: a Quant after finish() with "keep_names"; tx_feature: uint32 per transcript -> (cells, matrix entries)"""
        check(self.finish_raw(quant, tx_feature, n_features), "br_cells_finish")
        return self.n_cells, self.n_entries

    def cell_barcodes(self, first=0, n=None):
        """-> the cells' barcodes as a list of bytes"""
        n = self.n_cells - first if n is None else n
        k = max(int(n), 1)
        cb, ln = np.zeros((k, 32), np.uint8), np.zeros(k, np.uint8)
        self._call("cell_barcodes", int(first), int(n), cb.ctypes.data, ln.ctypes.data)
        return self._barcode_list(cb[:n], ln[:n])

    def name_cells(self, first, n):
        """-> uint32 per add-order name: its cell, 0xffffffff for a name in none"""
        out = np.zeros(max(int(n), 1), np.uint32)
        self._call("name_cells", int(first), int(n), out.ctypes.data)
        return out[:n]

    def matrix(self, first=0, n=None):
        """-> (cell_off uint64 [n + 1], feature uint32, value float64): CSR by cell, features ascending"""
        n = self.n_cells - first if n is None else n
        off = np.zeros(int(n) + 1, np.uint64)
        self._call("matrix", int(first), int(n), off.ctypes.data, None, None)
        z = int(off[-1])
        feat, val = np.zeros(max(z, 1), np.uint32), np.zeros(max(z, 1), np.float64)
        self._call("matrix", int(first), int(n), off.ctypes.data, feat.ctypes.data, val.ctypes.data)
        return off, feat[:z], val[:z]

    def call(self, cellcall, n_features):
        """After finish(), with "call_counts": runs `cellcall` (a CellCall with its parameters set) on the cells' unique counts"""
        self._call("call", cellcall.h, int(n_features))
        cellcall.n_cells, cellcall.n_features = self.n_cells, int(n_features)
        st = cellcall.stats()
        self.n_called = st["called_simple"] + st["called_emptydrops"]
        return cellcall

    def matrix_called(self, first=0, n=None):
        """After call() -> (cells uint32 [n], cell_off uint64 [n + 1], feature uint32, value float64): the called cells' rows"""
        n = self.n_called - first if n is None else n
        cells, off = np.zeros(max(int(n), 1), np.uint32), np.zeros(int(n) + 1, np.uint64)
        self._call("matrix_called", int(first), int(n), cells.ctypes.data, off.ctypes.data, None, None)
        z = int(off[-1])
        feat, val = np.zeros(max(z, 1), np.uint32), np.zeros(max(z, 1), np.float64)
        self._call("matrix_called", int(first), int(n), None, off.ctypes.data, feat.ctypes.data, val.ctypes.data)
        return cells[:n], off, feat[:z], val[:z]

    def cell_stats(self, first=0, n=None):
        """-> dict of per-cell arrays: names, unique, multi (uint64), features, iterations (uint32)"""
        n = self.n_cells - first if n is None else n
        k = max(int(n), 1)
        names, uniq, multi = np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros(k, np.uint64)
        feat, iters = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        self._call("cell_stats", int(first), int(n), names.ctypes.data, uniq.ctypes.data, multi.ctypes.data, feat.ctypes.data, iters.ctypes.data)
        return {"names": names[:n], "unique": uniq[:n], "multi": multi[:n], "features": feat[:n], "iterations": iters[:n]}

    def stats(self):
        out = np.zeros(16, np.uint64)
        self._call("stats", out.ctypes.data)
        return {k: int(v) for k, v in zip(self.STATS, out)}


class CellCall(_Accumulator):
    """br_cellcall on `device`: which barcodes of a cell x feature count matrix (CSR by cell) are cells.  Parameters (PARAMS integers,
    REALS reals; "method" also by name) before run(); after it calls(), ambient(), logtable(), candidates(), wanted(), sims() and
    stats()."""

    METHODS = {"topcells": 0, "cr2.2": 1, "emptydrops": 2}
    PARAMS = ("method", "expected", "ind_min", "ind_max", "umi_min", "cand_max", "sims", "seed", "sim_bytes", "keep_sims")
    REALS = ("percentile", "ratio", "umi_frac", "fdr")
    FALLBACK = ("none", "empty_window", "zero_ambient", "no_candidates")
    STATS = ("cells", "called_simple", "called_emptydrops", "threshold", "n_simple", "window", "ambient_counts", "active_features", "p_route",
             "slope_bits", "lo", "candidates", "n_max", "wanted_totals", "sim_chunks", "fallback", "rank_us", "ambient_us", "simulate_us",
             "pvalue_us", "method", "sims", "held_bytes", "peak_bytes", "entries", "features")

    NAME = "cellcall"
    ARGTYPES = {"new": [C.c_int, _P(C.c_void_p)], "set_param": [C.c_void_p, C.c_char_p, C.c_int64], "set_real": [C.c_void_p, C.c_char_p, C.c_double],
                "run": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
                "calls": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
                "ambient": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                "logtable": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p],
                "candidates": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                "wanted": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p],
                "sims": [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p],
                "stats": [C.c_void_p, C.c_void_p], "free": [C.c_void_p]}

    def __init__(self, device=0, **params):
        self.n_cells = self.n_features = 0
        self._open(device)
        for k, v in params.items():
            self.set_param(k, v)

    def set_param(self, name, value):
        if name in self.REALS:
            self._call("set_real", name.encode(), float(value))
        else:
            super().set_param(name, self.METHODS[value] if name == "method" and isinstance(value, str) else value)

    @staticmethod
    def sgt(amb, active):
        """br_cellcall_sgt (host only) -> (p float64, info: route, slope, active features, distinct counts)"""
        L = lib()
        L.br_cellcall_sgt.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        amb, active = np.ascontiguousarray(amb, dtype=np.uint64), np.ascontiguousarray(active, dtype=np.uint8)
        p, info = np.zeros(max(len(amb), 1), np.float64), np.zeros(4, np.uint64)
        check(L.br_cellcall_sgt(amb.ctypes.data, active.ctypes.data, len(amb), p.ctypes.data, info.ctypes.data), "br_cellcall_sgt")
        return p[:len(amb)], {"route": int(info[0]), "slope": float(info[1:2].view(np.float64)[0]), "active": int(info[2]), "distinct": int(info[3])}

    def run_raw(self, n_cells, n_features, cell_off, feature, count, on_device=False, stream=None):
        """br_cellcall_run as it is (the tables as addresses) -> the return code"""
        rc = self._raw("run", int(n_cells), int(n_features), C.c_void_p(cell_off), C.c_void_p(feature), C.c_void_p(count), 1 if on_device else 0,
                       C.c_void_p(stream or 0))
        if rc == 0:
            self.n_cells, self.n_features = int(n_cells), int(n_features)
        return rc

    def run(self, cell_off, feature, count, n_features):
        """The matrix as host arrays (cell_off uint64 [K + 1], feature uint32, count uint32)"""
        off = np.ascontiguousarray(cell_off, dtype=np.uint64)
        feat, cnt = np.ascontiguousarray(feature, dtype=np.uint32), np.ascontiguousarray(count, dtype=np.uint32)
        check(self.run_raw(len(off) - 1, n_features, off.ctypes.data, feat.ctypes.data if feat.size else None, cnt.ctypes.data if cnt.size else None),
              "br_cellcall_run")
        return self

    def run_device(self, cell_off, feature, count, n_features):
        """The same tables as torch CUDA tensors (uint64 offsets as int64, uint32 as int32)"""
        import torch
        check(self.run_raw(cell_off.numel() - 1, n_features, cell_off.data_ptr(), feature.data_ptr(), count.data_ptr(), True,
                           torch.cuda.current_stream(cell_off.device).cuda_stream), "br_cellcall_run")
        return self

    def calls(self, first=0, n=None):
        """-> (status uint8, rank uint32, total uint64) per cell"""
        n = self.n_cells - first if n is None else n
        k = max(int(n), 1)
        status, rank, total = np.zeros(k, np.uint8), np.zeros(k, np.uint32), np.zeros(k, np.uint64)
        self._call("calls", int(first), int(n), status.ctypes.data, rank.ctypes.data, total.ctypes.data)
        return status[:n], rank[:n], total[:n]

    def ambient(self, first=0, n=None, counts_only=False):
        """-> dict of per-feature arrays: amb (uint64), p, lp (float64), T (uint64)"""
        n = self.n_features - first if n is None else n
        k = max(int(n), 1)
        amb, p, lp, T = np.zeros(k, np.uint64), np.zeros(k, np.float64), np.zeros(k, np.float64), np.zeros(k, np.uint64)
        if counts_only:
            self._call("ambient", int(first), int(n), amb.ctypes.data, None, None, None)
            return {"amb": amb[:n]}
        self._call("ambient", int(first), int(n), amb.ctypes.data, p.ctypes.data, lp.ctypes.data, T.ctypes.data)
        return {"amb": amb[:n], "p": p[:n], "lp": lp[:n], "T": T[:n]}

    def logtable(self):
        """-> ln, float64 [n_max + 2] (empty without candidates)"""
        st = self.stats()
        n = st["n_max"] + 2 if st["candidates"] else 0
        out = np.zeros(max(n, 1), np.float64)
        self._call("logtable", 0, n, out.ctypes.data)
        return out[:n]

    def candidates(self):
        """-> dict of per-candidate arrays in rank order: cell, O, lower, pval, padj"""
        n = self.stats()["candidates"]
        k = max(n, 1)
        cell, O, lower = np.zeros(k, np.uint32), np.zeros(k, np.float64), np.zeros(k, np.uint32)
        pval, padj = np.zeros(k, np.float64), np.zeros(k, np.float64)
        self._call("candidates", 0, n, cell.ctypes.data, O.ctypes.data, lower.ctypes.data, pval.ctypes.data, padj.ctypes.data)
        return {"cell": cell[:n], "O": O[:n], "lower": lower[:n], "pval": pval[:n], "padj": padj[:n]}

    def wanted(self):
        """-> the wanted totals, ascending (uint64)"""
        n = self.stats()["wanted_totals"]
        out = np.zeros(max(n, 1), np.uint64)
        self._call("wanted", 0, n, out.ctypes.data)
        return out[:n]

    def sims(self, s_first=0, n_s=None, w_first=0, n_w=None):
        """With "keep_sims" -> L float64 [n_w, n_s]: row w the wanted total w_first + w, column s the simulation s_first + s"""
        st = self.stats()
        n_s = st["sims"] - s_first if n_s is None else n_s
        n_w = st["wanted_totals"] - w_first if n_w is None else n_w
        out = np.zeros((max(int(n_w), 1), max(int(n_s), 1)), np.float64)
        self._call("sims", int(s_first), int(n_s), int(w_first), int(n_w), out.ctypes.data)
        return out[:n_w, :n_s]

    def stats(self):
        out = np.zeros(32, np.uint64)
        self._call("stats", out.ctypes.data)
        d = {k: int(v) for k, v in zip(self.STATS, out)}
        d["slope"] = float(out[9:10].view(np.float64)[0])
        return d
