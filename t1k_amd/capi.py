"""ctypes binding of include/t1k_gpu.h (libt1k_gpu.so, built in-tree by __graft_entry__.build()).

There is deliberately no fallback: if the HIP library is missing, or no GPU is visible when a context is created,
an exception is raised.  Nothing here touches oracle/.
"""
import ctypes as C
import gzip
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    return os.environ.get("T1K_GPU_LIB") or os.path.join(_HERE, "lib", "libt1k_gpu.so")


class T1kError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [("kmer_length", C.c_int32), ("radius", C.c_int32), ("hit_len_required", C.c_int32),
                ("ref_seq_similarity", C.c_double), ("relax_intron_align", C.c_int32), ("max_assign_cnt", C.c_int32),
                ("max_read_len", C.c_int32), ("workgroups", C.c_int32), ("group_cap", C.c_int64),
                ("cand_cap", C.c_int64), ("ovl_cap", C.c_int64), ("row_cap", C.c_int64), ("n_base_code", C.c_int32), ("store_chunk_mb", C.c_int32)]


class JobParams(C.Structure):
    _fields_ = [("dev", Params), ("filter_frac", C.c_double), ("filter_cov", C.c_double),
                ("cross_gene_rate", C.c_double), ("squarem_min_alpha", C.c_double), ("allele_digit_units", C.c_int32),
                ("allele_delimiter", C.c_char), ("threads", C.c_int32), ("device", C.c_int32),
                ("output_read_assignment", C.c_int32), ("batch_fragments", C.c_int32), ("bootstrap_seed", C.c_uint64),
                ("bootstrap", C.c_int32), ("alternatives", C.c_int32), ("diplotypes", C.c_int32), ("diplo_candidates", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("read_ends", "lookups", "postings", "hits", "groups", "candidates", "extended",
                                          "near_best", "dp_calls", "rows", "batches")] + \
               [(n, C.c_double) for n in ("ms_seed", "ms_chain", "ms_extend", "ms_select", "ms_fullalign", "ms_pair", "ms_em", "ms_total")] + \
               [(n, C.c_uint64) for n in ("read_ends_total", "pair_overlaps", "dp_cells")] + \
               [(n, C.c_double) for n in ("ms_load", "ms_device", "ms_coalesce", "ms_write")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class UmiStats(C.Structure):  # t1k_umi_stats
    _fields_ = [(n, C.c_uint64) for n in ("distinct", "keys", "corrected", "split", "no_umi")] + [("kernel_ms", C.c_double)]


OVERLAP_DTYPE = np.dtype([("seq_idx", "<i4"), ("read_start", "<i4"), ("read_end", "<i4"), ("seq_start", "<i4"),
                          ("seq_end", "<i4"), ("strand", "<i4"), ("match_cnt", "<i4"), ("left_clip", "<i4"),
                          ("right_clip", "<i4"), ("relaxed_match_cnt", "<i4"), ("similarity", "<f8")])
ROW_DTYPE = np.dtype([("allele_idx", "<i4"), ("start", "<i4"), ("end", "<i4"), ("weight", "<f4"), ("qual", "<f4"),
                      ("adjust_weight", "<f4")])
GROUP_DTYPE = np.dtype([("allele", "<i4"), ("start", "<i4"), ("end", "<i4"), ("weight", "<f4"), ("adjust_weight", "<f4")])  # t1k_group_entry
assert OVERLAP_DTYPE.itemsize == 48 and ROW_DTYPE.itemsize == 24 and GROUP_DTYPE.itemsize == 20
# t1k_frag_assignment / t1k_variant (novel-variant calling of the analyzer stage, host code)
FRAG_ASG_DTYPE = np.dtype([("allele_idx", "<i4"), ("has_mate_pair", "<i4"), ("o1_from_r2", "<i4"), ("_pad", "<i4"), ("o1", OVERLAP_DTYPE), ("o2", OVERLAP_DTYPE),
                           ("ops1", "<u8"), ("ops2", "<u8"), ("n_ops1", "<u4"), ("n_ops2", "<u4")])
VARIANT_DTYPE = np.dtype([("allele_idx", "<i4"), ("ref_pos", "<i4"), ("exon_pos", "<i4"), ("ref", "S1"), ("var", "S1"), ("_pad", "S2"), ("qual", "<i4"), ("group", "<i4"),
                          ("output_group", "<i4"), ("_pad2", "<i4"), ("var_support", "<f8"), ("all_support", "<f8"), ("var_uniq_support", "<f8")])
assert FRAG_ASG_DTYPE.itemsize == 136 and VARIANT_DTYPE.itemsize == 56

# t1k_pileup_aln (per-base pileup) and the names of the 14 counter planes of its table
PILEUP_ALN_DTYPE = np.dtype([("allele", "<u4"), ("seq_start", "<u4"), ("read_at", "<u8"), ("ops_at", "<u8"), ("n_ops", "<u4"), ("w_all", "<u4"), ("w_uniq", "<u4"),
                             ("reserved", "<u4")])
PHASE_NO_MATE = 0xFFFFFFFF
PHASE_STATES = ("A", "C", "G", "T", "N", "-")
PILEUP_COUNTERS = ("A", "C", "G", "T", "N", "del", "ins", "A_uniq", "C_uniq", "G_uniq", "T_uniq", "N_uniq", "del_uniq", "ins_uniq")
assert PILEUP_ALN_DTYPE.itemsize == 40
# t1k_support_rec / t1k_support_book (support at sites), the states of its lines, and where its second key family begins
SUPPORT_REC_DTYPE = np.dtype([("read_len", "<u4"), ("clip_front", "<u4"), ("strand", "<u4")])
SUPPORT_BOOK_DTYPE = np.dtype([("flags", "<u4"), ("t_start", "<u4"), ("t_end", "<u4")])
SUPPORT_STATES = ("A", "C", "G", "T", "N", "-", "+")
SUPPORT_FAMILY_B = 1 << 57
assert SUPPORT_REC_DTYPE.itemsize == 12 and SUPPORT_BOOK_DTYPE.itemsize == 12
# t1k_route_totals / t1k_route_rec / T1K_ROUTE_* (route report)
ROUTE_TOTALS = ("ranges", "ranges_nw5", "ranges_nw10", "ranges_xlong", "groups", "fast", "slow", "jobs", "retry", "finish", "general", "wave", "genjobs", "big",
                "eq", "band", "wide", "extjobs", "extretry")
ROUTE_REC_DTYPE = np.dtype([("read_end", "<u4"), ("allele", "<u4"), ("n", "<u4"), ("strand", "u1"), ("near_done", "u1"), ("simple", "u1"), ("route", "u1"),
                            ("nw", "u1"), ("xlong", "u1"), ("reserved", "u1", (2,))])
ROUTE_NAMES = ("general_lane", "wave_small", "wave_large", "big_by_size", "big_by_scratch")
assert ROUTE_REC_DTYPE.itemsize == 20
# t1k_seed_used / T1K_SEED_MASK_WORDS (seed report)
SEED_USED_DTYPE = np.dtype([("read_off", "<u4"), ("list_len", "<u4"), ("strand", "u1"), ("reserved", "u1", (3,))])
SEED_MASK_WORDS = 10
assert SEED_USED_DTYPE.itemsize == 12
# t1k_ref_view_*: the arrays of the reference index in the order of the T1K_REF_* enum, with the dtype of one element
POSTING_DTYPE = np.dtype([("allele", "<u4"), ("offset", "<u4")])
REF_ARRAYS = (("bases", "<u8"), ("nmask", "<u8"), ("exon", "<u8"), ("posted", "<u8"), ("basesT", "<u8"), ("blockT", "<u4"), ("alleleOff", "<u8"), ("alleleLen", "<u4"),
              ("alleleHasN", "u1"), ("sepStart", "<u4"), ("sepPos", "<i4"), ("kStart", "<u4"), ("kHas", "<u4"), ("kMulti", "<u4"), ("kHasPre", "<u4"), ("kDirIdx", "<u4"),
              ("kDir", "<u4"), ("kDirMask", "<u8"), ("kPost", POSTING_DTYPE), ("kPostAllele", "<u4"))


class RefGeometry(C.Structure):  # t1k_ref_geometry
    _fields_ = [("n_alleles", C.c_uint32), ("k", C.c_uint32), ("total_bases", C.c_uint64), ("n_words", C.c_uint64), ("n_postings", C.c_uint64),
                ("bases_t_len", C.c_uint64), ("n_sep", C.c_uint64), ("dir_rows", C.c_uint32), ("dir_stride", C.c_uint32), ("dir_mask_words", C.c_uint32),
                ("has_bases_t", C.c_uint32), ("len", C.c_uint64 * len(REF_ARRAYS)), ("elem_bytes", C.c_uint32 * len(REF_ARRAYS))]


CIGAR_FILL = 0xAB  # what Context.cigar_batch fills its output arrays with before the call
ALT_FILL = 0xCD    # what Context.alt_batch fills its tables with before the call
ALT_EMPTY = 0xFFFFFFFF  # slotOf of an allele that is not called
DIPLO_FILL = 0xD1  # what Context.diplo_batch fills its matrix with before the call

ALLREDUCE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_void_p)

_lib = None


def lib():
    """Load libt1k_gpu.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise T1kError("%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` first" % p)
    L = C.CDLL(p)
    vp, u64p, u32p, u8p, i32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    L.t1k_params_default.argtypes = [C.POINTER(Params)]
    L.t1k_ctx_create.argtypes = [C.c_int, C.POINTER(Params), C.POINTER(vp)]
    L.t1k_ctx_destroy.argtypes = [vp]
    L.t1k_last_error.argtypes = [vp]
    L.t1k_last_error.restype = C.c_char_p
    L.t1k_device_count.restype = C.c_int
    L.t1k_ref_upload.argtypes = [vp, C.c_char_p, vp, vp, C.c_uint32]
    L.t1k_reads_upload.argtypes = [vp, C.c_char_p, vp, vp, C.c_uint32]
    L.t1k_assign_batch.argtypes = [vp]
    L.t1k_assign_range.argtypes = [vp, C.c_uint64, C.c_uint32]
    L.t1k_overlaps_download.argtypes = [vp, vp, vp, C.c_uint64, u64p]
    L.t1k_pair_batch.argtypes = [vp, vp, vp, vp, C.c_uint32]
    L.t1k_rows_download.argtypes = [vp, vp, vp, vp, C.c_uint64, u64p]
    L.t1k_coverage_get.argtypes = [vp, vp, C.c_uint64]
    L.t1k_coverage_reset.argtypes = [vp]
    L.t1k_missing_coverage.argtypes = [vp, vp]
    L.t1k_coverage_absorb.argtypes = [vp, vp]
    L.t1k_align_batch.argtypes = [vp, C.c_char_p, vp, vp, C.c_char_p, vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
    L.t1k_align_count_batch.argtypes = [vp, C.c_char_p, vp, C.c_char_p, vp, vp, C.c_uint32, vp]
    L.t1k_gap_count_batch.argtypes = [vp, C.c_char_p, vp, vp, C.c_char_p, vp, vp, C.c_uint32, vp]
    L.t1k_em_setup.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, ALLREDUCE_FN, vp]
    L.t1k_em_update.argtypes = [vp, vp, vp, vp, vp]
    L.t1k_em_shard.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.t1k_em_limits.argtypes = [vp]
    L.t1k_em_limits.restype = None
    L.t1k_em_set_count.argtypes = [vp, vp]
    L.t1k_boot_begin.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_int]
    L.t1k_boot_stride.argtypes = [C.c_uint32]
    L.t1k_boot_stride.restype = C.c_uint32
    L.t1k_boot_nonempty.argtypes = [vp, vp]
    L.t1k_boot_counts.argtypes = [vp, vp, vp]
    L.t1k_boot_update.argtypes = [vp, vp, vp, vp, vp, vp]
    L.t1k_boot_end.argtypes = [vp]
    L.t1k_boot_end.restype = None
    L.t1k_boot_limits.argtypes = [vp]
    L.t1k_boot_limits.restype = None
    L.t1k_boot_times.argtypes = [vp, vp]
    L.t1k_boot_times.restype = None
    L.t1k_job_bootstrap_text.argtypes = [vp, C.c_char_p, C.c_uint64, u64p]
    L.t1k_job_bootstrap_matrix.argtypes = [vp, vp, vp, vp, u32p, u32p]
    L.t1k_job_em_alleles.argtypes = [vp, vp, vp, vp, vp, u32p]
    L.t1k_job_series_names.argtypes = [vp, C.c_char_p, C.c_uint64, u64p]
    L.t1k_barcode_em.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, C.c_double, C.c_double, C.c_int32, vp, vp, C.POINTER(C.c_double)]
    L.t1k_umi_collapse.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_int32, vp, C.POINTER(C.c_uint32), vp, vp, vp, vp, vp, vp,
                                   C.POINTER(UmiStats)]
    L.t1k_pileup_begin.argtypes = [vp, C.c_uint32, vp]
    L.t1k_pileup_add.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_double)]
    L.t1k_pileup_get.argtypes = [vp, vp]
    L.t1k_pileup_end.argtypes = [vp]
    L.t1k_sitepile_begin.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64]
    L.t1k_sitepile_add.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_double)]
    L.t1k_sitepile_get.argtypes = [vp, vp, vp, C.c_uint64, u64p]
    L.t1k_sitepile_stats.argtypes = [vp, u64p, u64p, C.POINTER(C.c_double)]
    L.t1k_sitepile_end.argtypes = [vp]
    L.t1k_support_begin.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp, vp]
    L.t1k_support_add.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_double)]
    L.t1k_support_get.argtypes = [vp, vp, vp, C.c_uint64, u64p]
    L.t1k_support_stats.argtypes = [vp, u64p, u64p, C.POINTER(C.c_double)]
    L.t1k_support_end.argtypes = [vp]
    L.t1k_indel_begin.argtypes = [vp, C.c_uint32, vp, vp]
    L.t1k_indel_add.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_double)]
    L.t1k_indel_get.argtypes = [vp, vp, vp, C.c_uint64, u64p]
    L.t1k_indel_stats.argtypes = [vp, u64p, u64p, u64p, u64p, u64p, u64p, C.POINTER(C.c_double)]
    L.t1k_indel_end.argtypes = [vp]
    L.t1k_phase_begin.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp, vp]
    L.t1k_phase_add.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_double)]
    L.t1k_phase_get.argtypes = [vp, vp, vp, C.c_uint64, u64p]
    L.t1k_phase_stats.argtypes = [vp, u64p, u64p, u64p, u64p, u64p, C.POINTER(C.c_double)]
    L.t1k_phase_end.argtypes = [vp]
    L.t1k_cigar_batch.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, C.POINTER(C.c_double)]
    L.t1k_alt_batch.argtypes = [vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.POINTER(C.c_double)]
    L.t1k_ctx_mem_report.argtypes = [vp, C.c_char_p, C.c_int]
    L.t1k_ctx_mem_report.restype = C.c_uint64
    L.t1k_alt_pieces.argtypes = [C.c_uint64, vp]
    L.t1k_alt_pieces.restype = C.c_uint64
    L.t1k_job_alternatives_text.argtypes = [vp, C.c_char_p, C.c_uint64, u64p]
    L.t1k_diplo_batch.argtypes = [vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp, C.POINTER(C.c_double)]
    L.t1k_diplo_pieces.argtypes = [C.c_uint64, vp]
    L.t1k_diplo_pieces.restype = C.c_uint64
    L.t1k_job_diplotypes_text.argtypes = [vp, C.c_char_p, C.c_uint64, u64p]
    L.t1k_job_allele_table.argtypes = [vp, vp, vp, u32p]
    L.t1k_extract_batch.argtypes = [vp, C.c_uint32, vp, vp]
    L.t1k_extractor_main.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.t1k_stats_get.argtypes = [vp, C.POINTER(Stats)]
    L.t1k_route_report_enable.argtypes = [vp, C.c_int]
    L.t1k_route_report_get.argtypes = [vp, vp, vp, C.c_uint64, u64p]
    L.t1k_seed_report_enable.argtypes = [vp, C.c_int]
    L.t1k_seed_report_get.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, u64p]
    L.t1k_ref_view_geometry.argtypes = [vp, vp]
    L.t1k_ref_view_copy.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.t1k_genotyper_main.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.t1k_job_params_default.argtypes = [C.POINTER(JobParams)]
    L.t1k_job_create.argtypes = [C.POINTER(JobParams), C.c_char_p, C.POINTER(vp)]
    L.t1k_job_destroy.argtypes = [vp]
    L.t1k_job_last_error.argtypes = [vp]
    L.t1k_job_last_error.restype = C.c_char_p
    L.t1k_job_load_reads.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p]
    L.t1k_job_set_reads.argtypes = [vp, C.c_char_p, vp, C.c_char_p, vp, C.c_uint32]
    L.t1k_job_run.argtypes = [vp]
    L.t1k_job_write_outputs.argtypes = [vp, C.c_char_p]
    L.t1k_pool_release.restype = C.c_uint64
    L.t1k_pool_release.argtypes = []
    L.t1k_job_load_reads_multi.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p]
    L.t1k_reads_open.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.c_int, C.POINTER(vp)]
    L.t1k_reads_open_stream.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.c_int, C.POINTER(vp)]
    L.t1k_reads_last_error.argtypes = [vp]
    L.t1k_reads_last_error.restype = C.c_char_p
    L.t1k_reads_fragments.argtypes = [vp, u64p]
    L.t1k_reads_close.argtypes = [vp]
    L.t1k_reads_close.restype = None
    L.t1k_job_attach_reads.argtypes = [vp, vp]
    L.t1k_job_genotype_text.argtypes = [vp, C.c_char_p, C.c_uint64, u64p]
    L.t1k_job_counts.argtypes = [vp, u64p, u64p, u64p, u64p, i32p]
    L.t1k_job_stats.argtypes = [vp, C.POINTER(Stats)]
    L.t1k_job_ctx.argtypes = [vp]
    L.t1k_job_ctx.restype = vp
    L.t1k_job_run_local.argtypes = [vp]
    L.t1k_job_finish.argtypes = [vp]
    L.t1k_job_groups_serialize.argtypes = [vp, vp, C.c_uint64, u64p]
    L.t1k_reads_dedupe.argtypes = [vp, vp, u32p]
    L.t1k_job_groups_merge.argtypes = [vp, vp, vp, C.c_uint32]
    L.t1k_job_coalesce_rows.argtypes = [vp, vp, vp, vp, C.c_uint32]
    L.t1k_variants_call.argtypes = [vp, vp, C.c_int32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]
    L.t1k_fragment_details.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.c_int, vp, C.c_uint32, vp]
    L.t1k_variants_count.argtypes = [vp]
    L.t1k_variants_count.restype = C.c_uint32
    L.t1k_variants_get.argtypes = [vp, vp]
    L.t1k_variants_vcf.argtypes = [vp, vp, C.c_uint64, u64p]
    L.t1k_variants_adjust.argtypes = [vp, vp, C.c_uint32, vp, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, vp]
    L.t1k_variants_destroy.argtypes = [vp]
    L.t1k_job_set_shard.argtypes = [vp, C.c_int, C.c_int, vp]
    L.t1k_job_share_reads.argtypes = [vp, vp]
    L.t1k_job_ctx.restype = vp
    L.t1k_job_ctx.argtypes = [vp]
    L.t1k_comm_unique_id.argtypes = [vp]
    L.t1k_comm_init.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.POINTER(vp)]
    L.t1k_comm_bind.argtypes = [vp, vp]
    L.t1k_comm_destroy.argtypes = [vp]
    L.t1k_comm_last_error.restype = C.c_char_p
    L.t1k_comm_last_error.argtypes = [vp]
    L.t1k_comm_is_rccl.argtypes = [vp]
    L.t1k_comm_group_create.restype = vp
    L.t1k_comm_group_create.argtypes = [C.c_int]
    L.t1k_comm_group_destroy.argtypes = [vp]
    L.t1k_coverage_device.argtypes = [vp, C.POINTER(vp), u64p]
    L.t1k_device_memory.argtypes = [C.c_int, u64p, u64p]
    L.t1k_ctx_set_coverage_mode.argtypes = [vp, C.c_int]
    L.t1k_readset_detach.argtypes = [vp, C.POINTER(vp)]
    L.t1k_readset_take_store.argtypes = [vp, vp, C.c_int]
    L.t1k_readset_bytes.argtypes = [vp]
    L.t1k_readset_bytes.restype = C.c_uint64
    L.t1k_readset_size.argtypes = [vp]
    L.t1k_readset_size.restype = C.c_uint32
    L.t1k_readset_destroy.argtypes = [vp]
    L.t1k_coverage_selected.argtypes = [vp, vp, vp, u64p]
    L.t1k_overlaps_upload.argtypes = [vp, vp, vp]
    L.t1k_pair_limits.argtypes = [vp]
    L.t1k_pair_limits.restype = None
    L.t1k_pair_direct_cap.argtypes = []
    L.t1k_pair_direct_cap.restype = C.c_uint32
    L.t1k_rowset_create.argtypes = [vp, C.c_uint64, vp, C.POINTER(vp)]
    L.t1k_rowset_destroy.argtypes = [vp]
    L.t1k_rowset_destroy.restype = None
    L.t1k_rowset_set_raw.argtypes = [vp, C.c_int]
    L.t1k_rowset_last_error.argtypes = [vp]
    L.t1k_rowset_last_error.restype = C.c_char_p
    L.t1k_pair_into.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64]
    L.t1k_rowset_rows_download.argtypes = [vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, u64p]
    L.t1k_rowset_assigned_range.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    L.t1k_rowset_coalesce.argtypes = [vp, u64p, u64p, u64p]
    L.t1k_rowset_groups_download.argtypes = [vp, vp, vp, vp]
    L.t1k_rowset_device_bytes.argtypes = [vp, u64p, u64p]
    L.t1k_coalesce_limits.argtypes = [vp]
    L.t1k_coalesce_limits.restype = None
    L.t1k_rowset_exchange.argtypes = [vp, vp, C.c_uint64]
    L.t1k_rowset_groups_gather.argtypes = [vp, vp, u64p, u64p, u64p]
    L.t1k_rowset_groups_download_all.argtypes = [vp, vp, vp, vp]
    L.t1k_comm_abort.argtypes = [vp]
    L.t1k_ref_share.argtypes = [vp, vp]
    L.t1k_reads_share.argtypes = [vp, vp]
    L.t1k_xwin_create.argtypes = [vp, C.c_uint64, C.c_uint32, C.POINTER(vp)]
    L.t1k_xwin_destroy.argtypes = [vp]
    L.t1k_xwin_destroy.restype = None
    L.t1k_xwin_last_error.argtypes = [vp]
    L.t1k_xwin_last_error.restype = C.c_char_p
    L.t1k_xwin_link.argtypes = [vp, vp, C.c_uint32, u32p]
    L.t1k_xwin_resolve.argtypes = [vp, vp, C.c_uint32]
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _u8(text):
    """bytes, a bytearray or an array as a uint8 array"""
    return np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, np.uint8)


def _pieces(cuts, n):
    """the (lo, hi) pieces of 0 .. n split at the indices `cuts`"""
    edges = [0] + [int(c) for c in cuts] + [int(n)]
    return zip(edges[:-1], edges[1:])


def _concat(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    blob = "".join(seqs).encode("ascii")
    return blob, offs


class Context:
    """One GPU context (t1k_ctx)."""

    def __init__(self, device=0, **kw):
        L = lib()
        p = Params()
        L.t1k_params_default(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        self.params = p
        h = C.c_void_p()
        rc = L.t1k_ctx_create(device, C.byref(p), C.byref(h))
        if rc != 0:
            raise T1kError("t1k_ctx_create failed (%d): no usable GPU / bad parameters" % rc)
        self.h = h
        self.n_read_ends = 0
        self.allele_len = None

    def _check(self, rc, what):
        if rc != 0:
            raise T1kError("%s failed (%d): %s" % (what, rc, lib().t1k_last_error(self.h).decode()))

    def close(self):
        if self.h:
            lib().t1k_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ref_upload(self, seqs, exon_masks=None):
        blob, offs = _concat(seqs)
        ex = None
        if exon_masks is not None:
            ex = np.concatenate([np.asarray(m, dtype=np.uint8) for m in exon_masks]) if len(seqs) else np.zeros(0, np.uint8)
        self.allele_len = np.array([len(s) for s in seqs], dtype=np.int64)
        self._check(lib().t1k_ref_upload(self.h, blob, _ptr(offs), _ptr(ex), len(seqs)), "t1k_ref_upload")

    def ref_share(self, src):
        """this context reads the reference another context of the same GPU uploaded (t1k_ref_share); src must outlive it"""
        self.allele_len = src.allele_len
        self._check(lib().t1k_ref_share(self.h, src.h), "t1k_ref_share")

    def reads_share(self, src):
        """this context reads the read set (and the list table) another context of the same GPU uploaded (t1k_reads_share); src must outlive it"""
        self.n_read_ends = src.n_read_ends
        self._check(lib().t1k_reads_share(self.h, src.h), "t1k_reads_share")

    def reads_upload(self, seqs, weights=None):
        blob, offs = _concat(seqs)
        w = None if weights is None else np.asarray(weights, dtype=np.uint32)
        self.n_read_ends = len(seqs)
        self._check(lib().t1k_reads_upload(self.h, blob, _ptr(offs), _ptr(w), len(seqs)), "t1k_reads_upload")

    def reads_dedupe(self):
        """identical read-ends collapse (t1k_reads_dedupe): the context's read set becomes the distinct sequences; returns distinct_of[n_uploaded]"""
        out = np.zeros(self.n_read_ends, dtype=np.uint32)
        nd = C.c_uint32()
        self._check(lib().t1k_reads_dedupe(self.h, _ptr(out), C.byref(nd)), "t1k_reads_dedupe")
        self.n_uploaded, self.n_read_ends = self.n_read_ends, nd.value
        return out

    def assign(self):
        self._check(lib().t1k_assign_batch(self.h), "t1k_assign_batch")

    def extract(self, ends_per_fragment=1):
        """IsGoodCandidate of every fragment of the uploaded batch (t1k_extract_batch): (good[nFragments] uint8, stats dict)."""
        good = np.zeros(self.n_read_ends // ends_per_fragment, dtype=np.uint8)
        st = np.zeros(8, dtype=np.uint64)
        self._check(lib().t1k_extract_batch(self.h, ends_per_fragment, _ptr(good), _ptr(st)), "t1k_extract_batch")
        return good, dict(zip(("read_ends", "lookups", "postings", "read_ends_with_hits", "read_ends_chained", "screen_ns", "main_ns", "big_shape"), (int(x) for x in st)))

    def overlaps(self):
        n = self.n_read_ends
        counts = np.zeros(n, dtype=np.uint32)
        tot = C.c_uint64()
        self._check(lib().t1k_overlaps_download(self.h, _ptr(counts), None, 0, C.byref(tot)), "t1k_overlaps_download")
        out = np.zeros(tot.value, dtype=OVERLAP_DTYPE)
        self._check(lib().t1k_overlaps_download(self.h, _ptr(counts), _ptr(out), tot.value, C.byref(tot)), "t1k_overlaps_download")
        return counts, out

    def overlaps_upload(self, counts, ovl):
        """test-only (t1k_overlaps_upload): overlap lists made by the host become the lists of the uploaded read set"""
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        o = np.ascontiguousarray(ovl, dtype=OVERLAP_DTYPE)
        assert len(c) == self.n_read_ends and int(c.sum()) == len(o)
        self._check(lib().t1k_overlaps_upload(self.h, _ptr(c), _ptr(o)), "t1k_overlaps_upload")

    def pair(self, end1, end2, has_n):
        e1 = np.asarray(end1, dtype=np.uint32)
        e2 = None if end2 is None else np.asarray(end2, dtype=np.uint32)
        hn = np.asarray(has_n, dtype=np.uint8)
        self.n_fragments = len(e1)
        self._check(lib().t1k_pair_batch(self.h, _ptr(e1), _ptr(e2), _ptr(hn), len(e1)), "t1k_pair_batch")

    def rows(self):
        n = self.n_fragments
        counts = np.zeros(n, dtype=np.uint32)
        assigned = np.zeros(n, dtype=np.uint8)
        tot = C.c_uint64()
        self._check(lib().t1k_rows_download(self.h, _ptr(counts), _ptr(assigned), None, 0, C.byref(tot)), "t1k_rows_download")
        out = np.zeros(tot.value, dtype=ROW_DTYPE)
        self._check(lib().t1k_rows_download(self.h, _ptr(counts), _ptr(assigned), _ptr(out), tot.value, C.byref(tot)), "t1k_rows_download")
        return counts, assigned, out

    def coverage(self):
        tot = int(self.allele_len.sum())
        out = np.zeros(tot, dtype=np.int32)
        self._check(lib().t1k_coverage_get(self.h, _ptr(out), tot), "t1k_coverage_get")
        return out

    def set_coverage_mode(self, deferred):
        """deferred: t1k_assign_range adds no per-base coverage (t1k_coverage_selected adds it later for the alleles that need it)"""
        self._check(lib().t1k_ctx_set_coverage_mode(self.h, 1 if deferred else 0), "t1k_ctx_set_coverage_mode")

    def detach_readset(self, slot=0):
        """the context's read set and the final overlap lists it holds change owner (t1k_readset_detach + t1k_readset_take_store)"""
        h = C.c_void_p()
        self._check(lib().t1k_readset_detach(self.h, C.byref(h)), "t1k_readset_detach")
        rs = Readset(h)
        self._check(lib().t1k_readset_take_store(rs.h, self.h, slot), "t1k_readset_take_store")
        return rs

    def coverage_selected(self, readset, selected):
        """adds the coverage of the read set's near-best overlaps on the alleles with selected[a] != 0; returns the records aligned"""
        sel = np.ascontiguousarray(selected, dtype=np.uint8)
        n = C.c_uint64()
        self._check(lib().t1k_coverage_selected(self.h, readset.h, _ptr(sel), C.byref(n)), "t1k_coverage_selected")
        return n.value

    def coverage_reset(self):
        self._check(lib().t1k_coverage_reset(self.h), "t1k_coverage_reset")

    def missing_coverage(self):
        """per allele: exon positions with coverage below max(1, 1 % of the allele's median exon coverage)"""
        out = np.zeros(len(self.allele_len), dtype=np.int32)
        self._check(lib().t1k_missing_coverage(self.h, _ptr(out)), "t1k_missing_coverage")
        return out

    def stats(self):
        s = Stats()
        lib().t1k_stats_get(self.h, C.byref(s))
        return s.as_dict()

    def route_report_enable(self, on=True):
        """starts (and clears) or stops the route report (t1k_route_report_enable)"""
        self._check(lib().t1k_route_report_enable(self.h, 1 if on else 0), "t1k_route_report_enable")

    def route_report(self):
        """(totals dict, records as ROUTE_REC_DTYPE) of the ranges finished since route_report_enable(); ROUTE_NAMES[rec["route"]] names the kernel"""
        n = C.c_uint64()
        self._check(lib().t1k_route_report_get(self.h, None, None, 0, C.byref(n)), "t1k_route_report_get")
        tot = np.zeros(len(ROUTE_TOTALS), np.uint64)
        recs = np.zeros(n.value, ROUTE_REC_DTYPE)
        self._check(lib().t1k_route_report_get(self.h, _ptr(tot), _ptr(recs), n.value, C.byref(n)), "t1k_route_report_get")
        return dict(zip(ROUTE_TOTALS, (int(x) for x in tot))), recs

    def assign_range(self, first, count):
        """t1k_assign_range: the read-ends [first, first + count) of the uploaded set as one range"""
        self._check(lib().t1k_assign_range(self.h, first, count), "t1k_assign_range")

    def seed_report_enable(self, on=True):
        """starts (and clears) or stops the seed report (t1k_seed_report_enable)"""
        self._check(lib().t1k_seed_report_enable(self.h, 1 if on else 0), "t1k_seed_report_enable")

    def seed_report(self):
        """the used k-mers of the read-ends of the ranges finished since seed_report_enable(): (seen[n] uint8, counts[n, 2], masks[n, 2,
        SEED_MASK_WORDS], used_ptr[n + 1], used as SEED_USED_DTYPE); read-end i's entries are used[used_ptr[i]:used_ptr[i + 1]], the
        read-end as given first"""
        n = self.n_read_ends
        tot = C.c_uint64()
        self._check(lib().t1k_seed_report_get(self.h, None, None, None, None, 0, C.byref(tot)), "t1k_seed_report_get")
        seen = np.zeros(n, np.uint8)
        counts = np.zeros((n, 2), np.uint32)
        masks = np.zeros((n, 2, SEED_MASK_WORDS), np.uint32)
        used = np.zeros(tot.value, SEED_USED_DTYPE)
        self._check(lib().t1k_seed_report_get(self.h, _ptr(seen), _ptr(counts), _ptr(masks), _ptr(used), tot.value, C.byref(tot)), "t1k_seed_report_get")
        ptr = np.zeros(n + 1, np.int64)
        np.cumsum(counts.sum(axis=1, dtype=np.int64), out=ptr[1:])
        assert int(ptr[-1]) == len(used)
        return seen, counts, masks, ptr, used

    def ref_geometry(self):
        """the sizes of the reference index (t1k_ref_view_geometry) as a dict; "len" maps every name of REF_ARRAYS to its element count"""
        g = RefGeometry()
        self._check(lib().t1k_ref_view_geometry(self.h, C.byref(g)), "t1k_ref_view_geometry")
        out = {f: int(getattr(g, f)) for f, _ in RefGeometry._fields_[:11]}
        out["len"] = {name: int(g.len[i]) for i, (name, _) in enumerate(REF_ARRAYS)}
        assert all(g.elem_bytes[i] == np.dtype(t).itemsize for i, (_, t) in enumerate(REF_ARRAYS))
        return out

    def ref_array(self, name, first=0, count=None):
        """elements [first, first + count) of one array of the reference index (t1k_ref_view_copy); count None: up to the array's end"""
        i = [n for n, _ in REF_ARRAYS].index(name)
        if count is None:
            count = self.ref_geometry()["len"][name] - first
        out = np.zeros(max(count, 0), REF_ARRAYS[i][1])
        self._check(lib().t1k_ref_view_copy(self.h, i, first, count, _ptr(out)), "t1k_ref_view_copy")
        return out

    def align_batch(self, texts, pats, want_ops=True):
        n = len(texts)
        tb, toff = _concat(texts)
        pb, poff = _concat(pats)
        tlen = np.array([len(t) for t in texts], dtype=np.uint32)
        plen = np.array([len(p) for p in pats], dtype=np.uint32)
        toff32, poff32 = toff[:-1].astype(np.uint32), poff[:-1].astype(np.uint32)
        score = np.zeros(n, np.int32); nm = np.zeros(n, np.int32); nx = np.zeros(n, np.int32); ni = np.zeros(n, np.int32)
        ops_off = np.zeros(n, np.uint32)
        if n:
            ops_off[1:] = np.cumsum((tlen + plen + 2)[:-1], dtype=np.uint64).astype(np.uint32)
        ops = np.zeros(int((tlen + plen + 2).sum()) + 8, np.int8)
        nops = np.zeros(n, np.uint32)
        self._check(lib().t1k_align_batch(self.h, tb, _ptr(toff32), _ptr(tlen), pb, _ptr(poff32), _ptr(plen), n, _ptr(score), _ptr(nm),
                                          _ptr(nx), _ptr(ni), _ptr(ops) if want_ops else None, _ptr(ops_off), _ptr(nops)), "t1k_align_batch")
        op_list = [ops[ops_off[i]:ops_off[i] + nops[i]].copy() for i in range(n)] if want_ops else None
        return score, nm, nx, ni, op_list

    def align_count_batch(self, texts, pats):
        """production match-count routine (exact fast path + banded forward sweep), equal-length jobs"""
        n = len(texts)
        tb, toff = _concat(texts)
        pb, poff = _concat(pats)
        ln = np.array([len(t) for t in texts], dtype=np.uint32)
        out = np.zeros(n, np.int32)
        self._check(lib().t1k_align_count_batch(self.h, tb, _ptr(toff[:-1].astype(np.uint32)), pb, _ptr(poff[:-1].astype(np.uint32)), _ptr(ln), n,
                                                _ptr(out)), "t1k_align_count_batch")
        return out

    def gap_count_batch(self, texts, pats, lead=""):
        """the routine of the dense DP phase (gapAlign: no fast path), one lane per job, |len(text) - len(pat)| <= 4.  The texts lie back to back in one
        packed stream behind `lead` (which shifts them against the stream's word boundaries), the patterns back to back in another; a stream of
        texts without N is read without its N mask, as a reference without N is"""
        n = len(texts)
        tb, toff = _concat([lead] + list(texts))
        pb, poff = _concat(pats)
        tlen = np.array([len(t) for t in texts], dtype=np.uint32)
        plen = np.array([len(p) for p in pats], dtype=np.uint32)
        out = np.zeros(n, np.int32)
        self._check(lib().t1k_gap_count_batch(self.h, tb, _ptr(toff[1:-1].astype(np.uint32)), _ptr(tlen), pb, _ptr(poff[:-1].astype(np.uint32)), _ptr(plen), n,
                                              _ptr(out)), "t1k_gap_count_batch")
        return out

    def em_setup(self, row_ptr, ec_idx, count, ec_len, allreduce=None, raw=False):
        """raw=True returns the status code instead of raising (argument-error tests)"""
        self._em_keep = (np.ascontiguousarray(row_ptr, np.uint64), np.ascontiguousarray(ec_idx, np.uint32), np.ascontiguousarray(count, np.float64),
                         np.ascontiguousarray(ec_len, np.int32))
        rp, ei, ct, el = self._em_keep
        assert len(rp) == len(ct) + 1 and int(rp[-1]) == len(ei)
        self._em_cb = ALLREDUCE_FN(allreduce) if allreduce else C.cast(None, ALLREDUCE_FN)
        self._em_nec = len(el)
        rc = lib().t1k_em_setup(self.h, _ptr(rp), _ptr(ei), _ptr(ct), _ptr(el), len(ct), len(el), self._em_cb, None)
        if raw:
            return rc
        self._check(rc, "t1k_em_setup")

    def em_shard(self, row_begin, row_end, comm=None, raw=False):
        """this rank's t1k_em_update sums the read groups [row_begin, row_end) only (t1k_em_shard; collective when comm has several ranks:
        the ranks' ranges partition the read groups in rank order).  raw=True returns the status code instead of raising"""
        rc = lib().t1k_em_shard(self.h, row_begin, row_end, comm.h if comm is not None else None)
        if raw:
            return rc
        self._check(rc, "t1k_em_shard")

    def last_error(self):
        return lib().t1k_last_error(self.h).decode()

    def em_update(self, x0):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        x1 = np.zeros(self._em_nec, np.float64)
        n = np.zeros(self._em_nec, np.float64)
        diff = C.c_double()
        self._check(lib().t1k_em_update(self.h, _ptr(x0), _ptr(x1), _ptr(n), C.byref(diff)), "t1k_em_update")
        return x1, n, diff.value

    def em_set_count(self, count):
        """replaces the counts of the structure em_setup left (t1k_em_set_count)"""
        ct = np.ascontiguousarray(count, np.float64)
        assert len(ct) == len(self._em_keep[2])
        self._check(lib().t1k_em_set_count(self.h, _ptr(ct)), "t1k_em_set_count")

    # bootstrap of the EM over the structure em_setup left (t1k_boot_*).  The library's arrays are replicate-minor with stride
    # boot_stride(B); the binding hands out and takes replicate-major ones, [replicate][...], of the B + 1 real replicates.
    def boot_begin(self, n_replicates, seed=1, identity=False, raw=False):
        rc = lib().t1k_boot_begin(self.h, n_replicates, seed, 1 if identity else 0)
        if raw:
            return rc
        self._check(rc, "t1k_boot_begin")
        self._boot_reps, self._boot_stride = n_replicates + 1, boot_stride(n_replicates)

    def boot_nonempty(self):
        """[B + 1] bool: the replicate has a count that is not 0"""
        out = np.zeros(self._boot_stride, np.uint8)
        self._check(lib().t1k_boot_nonempty(self.h, _ptr(out)), "t1k_boot_nonempty")
        assert not out[self._boot_reps:].any()
        return out[:self._boot_reps].astype(bool)

    def boot_counts(self):
        """(k uint32 [B + 1][G], c' float64 [B + 1][G]); the padding replicates must be empty"""
        G = len(self._em_keep[2])
        k, c = np.zeros((G, self._boot_stride), np.uint32), np.zeros((G, self._boot_stride), np.float64)
        self._check(lib().t1k_boot_counts(self.h, _ptr(k), _ptr(c)), "t1k_boot_counts")
        assert not k[:, self._boot_reps:].any() and not c[:, self._boot_reps:].any()
        return np.ascontiguousarray(k[:, :self._boot_reps].T), np.ascontiguousarray(c[:, :self._boot_reps].T)

    def boot_update(self, active, x0, fill=None):
        """one update of the replicates with active[r]: x0 [B + 1][E] -> (x1 [B + 1][E], n [B + 1][E], diff [B + 1]).  The output arrays
        are filled with `fill` (default 0.0) before the call: what an inactive replicate's outputs must still hold after it"""
        R, S, E = self._boot_reps, self._boot_stride, self._em_nec
        act = np.zeros(S, np.uint8)
        act[:R] = np.asarray(active, bool)
        xin = np.zeros((E, S), np.float64)
        xin[:, :R] = np.asarray(x0, np.float64).T
        f = 0.0 if fill is None else fill
        x1, n, diff = np.full((E, S), f, np.float64), np.full((E, S), f, np.float64), np.full(S, f, np.float64)
        self._check(lib().t1k_boot_update(self.h, _ptr(act), _ptr(xin), _ptr(x1), _ptr(n), _ptr(diff)), "t1k_boot_update")
        for a in (x1[:, R:], n[:, R:], diff[R:]):
            assert (a == f).all() or (np.isnan(f) and np.isnan(a).all())
        return np.ascontiguousarray(x1[:, :R].T), np.ascontiguousarray(n[:, :R].T), diff[:R].copy()

    def boot_times(self):
        out = np.zeros(3, np.float64)
        lib().t1k_boot_times(self.h, _ptr(out))
        return dict(rows_ms=out[0], cols_ms=out[1], updates=int(out[2]))

    def boot_end(self):
        lib().t1k_boot_end(self.h)

    def barcode_em(self, bc_allele_ptr, bc_allele, bc_group_ptr, group_count, group_entry_ptr, entry_local, rho, n_alleles, alpha=0.0, tol=1e-7,
                   max_iter=1000, raw=False):
        """per-barcode allele EM (t1k_barcode_em): returns (n laid out as bc_allele, updates per barcode, kernel ms); raw=True returns the
        status code instead of raising (argument-error tests)"""
        ap = np.ascontiguousarray(bc_allele_ptr, np.uint64)
        al = np.ascontiguousarray(bc_allele, np.uint32)
        gp = np.ascontiguousarray(bc_group_ptr, np.uint64)
        gc = np.ascontiguousarray(group_count, np.float64)
        ep = np.ascontiguousarray(group_entry_ptr, np.uint64)
        el = np.ascontiguousarray(entry_local, np.uint32)
        rh = None if rho is None else np.ascontiguousarray(rho, np.float64)
        nb = max(len(ap) - 1, 0)
        n = np.zeros(len(al), np.float64)
        iters = np.zeros(nb, np.int32)
        ms = C.c_double()
        rc = lib().t1k_barcode_em(self.h, nb, _ptr(ap), _ptr(al), _ptr(gp), _ptr(gc), _ptr(ep), _ptr(el), _ptr(rh), n_alleles, alpha, tol, max_iter,
                                  _ptr(n), _ptr(iters), C.byref(ms))
        if raw:
            return rc
        self._check(rc, "t1k_barcode_em")
        return n, iters, ms.value

    def umi_collapse(self, frag_row, frag_umi, list_ptr, list_allele, n_rows, allele_gene, n_genes, mismatch=1, raw=False):
        """UMI collapse of per-barcode allele lists (t1k_umi_collapse).  frag_umi: code in bits 0-31, length in bits 32-36, all ones for
        none; list_ptr may be a slice of a larger table's offsets (list_allele whole).  Returns a dict with the molecule table
        canonicalised -- molecules sorted by (row, smallest fragment index), frag_mol renumbered to match: frag_mol, mol_row, mol_frags,
        mol_list_ptr, mol_list, frac and uniq [n_rows, n_alleles], stats.  raw=True returns the status code instead of raising."""
        fr = np.ascontiguousarray(frag_row, np.uint32)
        fu = np.ascontiguousarray(frag_umi, np.uint64)
        lp = np.ascontiguousarray(list_ptr, np.uint64)
        la = np.ascontiguousarray(list_allele, np.uint32)
        ag = np.ascontiguousarray(allele_gene, np.uint32)
        nf, na = len(fr), len(ag)
        if len(fu) != nf or len(lp) != nf + 1:
            raise ValueError("umi_collapse: frag_row, frag_umi and list_ptr do not describe the same fragments")
        # output room by the upper bounds: molecules <= fragments, their list entries <= the fragments' (an offset array that lies is the
        # library's to reject: the room only has to be there when the offsets are sound)
        ne = int(lp[-1]) - int(lp[0]) if nf and int(lp[-1]) >= int(lp[0]) else 0
        ne = min(ne, len(la))
        frag_mol = np.zeros(nf, np.uint32)
        mol_row = np.zeros(nf, np.uint32)
        mol_frags = np.zeros(nf, np.uint32)
        mol_ptr = np.zeros(nf + 1, np.uint64)
        mol_list = np.zeros(max(ne, 1), np.uint32)
        frac = np.zeros((int(n_rows), na), np.float64)
        uniq = np.zeros((int(n_rows), na), np.int32)
        n_mol = C.c_uint32()
        st = UmiStats()
        rc = lib().t1k_umi_collapse(self.h, nf, _ptr(fr), _ptr(fu), _ptr(lp), _ptr(la), int(n_rows), _ptr(ag), na, int(n_genes), int(mismatch), _ptr(frag_mol), C.byref(n_mol),
                                    _ptr(mol_row), _ptr(mol_frags), _ptr(mol_ptr), _ptr(mol_list), _ptr(frac), _ptr(uniq), C.byref(st))
        if raw:
            return rc
        self._check(rc, "t1k_umi_collapse")
        m = n_mol.value
        mol_row, mol_frags, mol_ptr = mol_row[:m], mol_frags[:m], mol_ptr[:m + 1].astype(np.int64)
        first = np.full(m, nf, np.int64)
        np.minimum.at(first, frag_mol, np.arange(nf))
        order = np.lexsort((first, mol_row))
        rank = np.empty(m, np.uint32)
        rank[order] = np.arange(m, dtype=np.uint32)
        lens = np.diff(mol_ptr)[order]
        new_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        take = np.repeat(mol_ptr[:-1][order] - new_ptr[:-1].astype(np.int64), lens) + np.arange(int(lens.sum()))
        return dict(frag_mol=rank[frag_mol], mol_row=mol_row[order], mol_frags=mol_frags[order], mol_list_ptr=new_ptr, mol_list=mol_list[take] if m else mol_list[:0],
                    frac=frac, uniq=uniq,
                    stats=dict(distinct=int(st.distinct), keys=int(st.keys), corrected=int(st.corrected), split=int(st.split), no_umi=int(st.no_umi), kernel_ms=float(st.kernel_ms)))

    # per-base pileup (t1k_pileup_begin / _add / _get / _end); raw=True returns the status code instead of raising
    def pileup_begin(self, allele_off, raw=False):
        off = np.ascontiguousarray(allele_off, np.uint64)
        rc = lib().t1k_pileup_begin(self.h, max(len(off) - 1, 0), _ptr(off))
        if rc == 0:
            self._pileup_total = int(off[-1])
        if raw:
            return rc
        self._check(rc, "t1k_pileup_begin")

    def pileup_add(self, aln, text, ops, raw=False):
        """aln: PILEUP_ALN_DTYPE records; text: bytes (or uint8 array) of strand-corrected read bases; ops: int8 edit columns.  Returns the
        kernels' device time in ms"""
        a = np.ascontiguousarray(aln, PILEUP_ALN_DTYPE)
        t, o = _u8(text), np.ascontiguousarray(ops, np.int8)
        ms = C.c_double()
        rc = lib().t1k_pileup_add(self.h, _ptr(a), len(a), _ptr(t), len(t), _ptr(o), len(o), C.byref(ms))
        if raw:
            return rc
        self._check(rc, "t1k_pileup_add")
        return ms.value

    def pileup_get(self):
        """the table as int32 [14, positions]: row c = counter PILEUP_COUNTERS[c], column alleleOff[a] + p"""
        counts = np.zeros((14, getattr(self, "_pileup_total", 0)), np.int32)
        self._check(lib().t1k_pileup_get(self.h, _ptr(counts)), "t1k_pileup_get")
        return counts

    def pileup_end(self, raw=False):
        rc = lib().t1k_pileup_end(self.h)
        if raw:
            return rc
        self._check(rc, "t1k_pileup_end")

    def pileup(self, allele_off, aln, text, ops, cuts=()):
        """begin, add (the records split at the indices `cuts` into several calls), get, end: the table and the kernels' ms"""
        a = np.ascontiguousarray(aln, PILEUP_ALN_DTYPE)
        self.pileup_begin(allele_off)
        try:
            ms = sum(self.pileup_add(a[lo:hi], text, ops) for lo, hi in _pieces(cuts, len(a)))
            return self.pileup_get(), ms
        finally:
            self.pileup_end()

    # runner-up evidence per called allele (t1k_alt_batch)
    def alt_batch(self, group_ptr, entry_allele, q, allele_gene, n_genes, slot_of, raw=False):
        """the read groups as a CSR (uint64 group_ptr [G + 1], uint32 entry_allele), uint64 q [G], uint32 allele_gene / slot_of [A] (ALT_EMPTY:
        not called) -> (tables uint64 [4, A]: total, both0, both1, neither; the kernels' device time in ms).  raw=True: (status code, tables, ms)
        without raising; the tables are filled with ALT_FILL bytes before the call."""
        gp = np.ascontiguousarray(group_ptr, np.uint64)
        ent = np.ascontiguousarray(entry_allele, np.uint32)
        qq = np.ascontiguousarray(q, np.uint64)
        ag = np.ascontiguousarray(allele_gene, np.uint32)
        so = np.ascontiguousarray(slot_of, np.uint32)
        assert len(ag) == len(so) and len(gp) == len(qq) + 1
        tables = np.empty((4, len(ag)), np.uint64)
        tables.view(np.uint8)[:] = ALT_FILL
        ms = C.c_double()
        rc = lib().t1k_alt_batch(self.h, len(qq), _ptr(gp), _ptr(ent), _ptr(qq), len(ag), _ptr(ag), n_genes, _ptr(so), _ptr(tables), C.byref(ms))
        if raw:
            return rc, tables, ms.value
        self._check(rc, "t1k_alt_batch")
        return tables, ms.value

    # co-occurrence of the allele-pair candidates of every gene (t1k_diplo_batch)
    def diplo_batch(self, group_ptr, entry_cand, q, cand_ptr, raw=False):
        """the read groups as a CSR over candidate ids (uint64 group_ptr [G + 1], uint32 entry_cand), uint64 q [G], uint32 cand_ptr [genes + 1]
        -> (matrix uint64 [sum of n_x^2]: per gene its n_x * n_x block, cell (i, j) at i * n_x + j, i <= j; the kernels' device time in ms).
        raw=True: (status code, matrix, ms) without raising; the matrix is filled with DIPLO_FILL bytes before the call.  (More than 2^29
        cells are refused by the call before it writes: the array then holds 1024 cells only.)"""
        gp = np.ascontiguousarray(group_ptr, np.uint64)
        ent = np.ascontiguousarray(entry_cand, np.uint32)
        qq = np.ascontiguousarray(q, np.uint64)
        cp = np.ascontiguousarray(cand_ptr, np.uint32)
        assert len(gp) == len(qq) + 1 and len(cp) >= 1
        cells = sum((int(cp[x + 1]) - int(cp[x])) ** 2 for x in range(len(cp) - 1))
        matrix = np.empty(cells if cells <= 1 << 29 else 1024, np.uint64)
        matrix.view(np.uint8)[:] = DIPLO_FILL
        ms = C.c_double()
        rc = lib().t1k_diplo_batch(self.h, len(qq), _ptr(gp), _ptr(ent), _ptr(qq), len(cp) - 1, _ptr(cp), _ptr(matrix), C.byref(ms))
        if raw:
            return rc, matrix, ms.value
        self._check(rc, "t1k_diplo_batch")
        return matrix, ms.value

    # CIGAR / MD / NM of alignments (t1k_cigar_batch)
    def cigar_batch(self, aln, ops, allele_off, allele_text, clip=None, cigar_cap=None, md_cap=None, raw=False):
        """aln: PILEUP_ALN_DTYPE records (read_at and the weights are ignored); ops: int8 edit columns; allele_text: the alleles' bases back
        to back (bytes or uint8 array); clip: uint32 [n, 2] front / back soft clips or None.  The arenas hold cigar_cap / md_cap bytes
        (default: the header's bounds, 2 * n_ops + 22 and 3 * n_ops + 11 per record).  -> dict(cigar_ptr, cigar, md_ptr, md, nm, ref_span,
        ms): uint64 [n + 1] offsets into the uint8 arenas, uint32 [n] counts, the kernels' device time.  raw=True: (status code, the same
        dict) without raising; every output array is filled with CIGAR_FILL bytes before the call."""
        a = np.ascontiguousarray(aln, PILEUP_ALN_DTYPE)
        n = len(a)
        o = np.ascontiguousarray(ops, np.int8)
        off = np.ascontiguousarray(allele_off, np.uint64)
        t = _u8(allele_text)
        c = None if clip is None else np.ascontiguousarray(clip, np.uint32).reshape(-1)
        assert c is None or len(c) == 2 * n
        n_ops = a["n_ops"].astype(np.int64)
        cigar_cap = int((2 * n_ops + 22).sum()) if cigar_cap is None else int(cigar_cap)
        md_cap = int((3 * n_ops + 11).sum()) if md_cap is None else int(md_cap)
        out = dict(cigar_ptr=np.empty(n + 1, np.uint64), cigar=np.empty(cigar_cap, np.uint8), md_ptr=np.empty(n + 1, np.uint64), md=np.empty(md_cap, np.uint8),
                   nm=np.empty(n, np.uint32), ref_span=np.empty(n, np.uint32))
        for v in out.values():
            v.view(np.uint8)[:] = CIGAR_FILL
        ms = C.c_double()
        rc = lib().t1k_cigar_batch(self.h, _ptr(a), n, None if c is None else _ptr(c), _ptr(o), len(o), max(len(off) - 1, 0), _ptr(off), _ptr(t),
                                   _ptr(out["cigar_ptr"]), _ptr(out["cigar"]), cigar_cap, _ptr(out["md_ptr"]), _ptr(out["md"]), md_cap, _ptr(out["nm"]), _ptr(out["ref_span"]),
                                   C.byref(ms))
        out["ms"] = ms.value
        if raw:
            return rc, out
        self._check(rc, "t1k_cigar_batch")
        out["cigar"] = out["cigar"][:int(out["cigar_ptr"][n])]
        out["md"] = out["md"][:int(out["md_ptr"][n])]
        return out

    # ---- the four sparse-table stages (sitepile, support, indel, phase): what their methods below share ----
    def _done(self, rc, what, raw, value=None):
        """the tail of a call: the status code as it is (raw), or checked, and then `value`"""
        if raw:
            return rc
        self._check(rc, what)
        return value

    def _stage_begin(self, stage, allele_off, site_allele, site_pos, *more, raw=False):
        off = np.ascontiguousarray(allele_off, np.uint64)
        sa, sp = np.ascontiguousarray(site_allele, np.uint32), np.ascontiguousarray(site_pos, np.uint32)
        assert len(sa) == len(sp)
        what = "t1k_%s_begin" % stage
        return self._done(getattr(lib(), what)(self.h, max(len(off) - 1, 0), _ptr(off), len(sa), _ptr(sa), _ptr(sp), *more), what, raw)

    def _stage_add(self, stage, a, mid, text, ops, raw):
        """mid: the stage's own arguments between (aln, n) and (text, textBytes, ops, opsBytes, kernelMs).  The kernels' device time in ms"""
        t, o = _u8(text), np.ascontiguousarray(ops, np.int8)
        ms = C.c_double()
        what = "t1k_%s_add" % stage
        rc = getattr(lib(), what)(self.h, _ptr(a), len(a), *mid, _ptr(t), len(t), _ptr(o), len(o), C.byref(ms))
        return self._done(rc, what, raw, ms.value)

    def _stage_get(self, stage, raw):
        """the size query, then the runs: (keys uint64, counts int32)"""
        get = getattr(lib(), "t1k_%s_get" % stage)
        n = C.c_uint64()
        rc = get(self.h, None, None, 0, C.byref(n))
        keys, counts = np.zeros(n.value, np.uint64), np.zeros(n.value, np.int32)
        if rc == 0 and n.value:
            rc = get(self.h, _ptr(keys), _ptr(counts), n.value, C.byref(n))
        return self._done(rc, "t1k_%s_get" % stage, raw, (keys, counts))

    def _stage_stats(self, stage, n_counts, raw=False):
        """the n_counts uint64 of t1k_<stage>_stats and its fold ms"""
        v = [C.c_uint64() for _ in range(n_counts)]
        ms = C.c_double()
        rc = getattr(lib(), "t1k_%s_stats" % stage)(self.h, *[C.byref(x) for x in v], C.byref(ms))
        return self._done(rc, "t1k_%s_stats" % stage, raw, tuple(x.value for x in v) + (ms.value,))

    def _stage_end(self, stage, raw):
        return self._done(getattr(lib(), "t1k_%s_end" % stage)(self.h), "t1k_%s_end" % stage, raw)

    def _stage_run(self, stage, n, add, stats, cuts):
        """behind the stage's _begin: add(lo, hi) for each piece of 0 .. n split at `cuts`, get, stats(), end: (keys, counts, summed ms, what
        stats() gives)"""
        try:
            ms = sum(add(lo, hi) for lo, hi in _pieces(cuts, n))
            keys, counts = self._stage_get(stage, False)
            return keys, counts, ms, stats()
        finally:
            self._stage_end(stage, False)

    # per-barcode pileup at sites (t1k_sitepile_begin / _add / _get / _end); raw=True returns the status code instead of raising
    def sitepile_begin(self, allele_off, site_allele, site_pos, n_barcodes, raw=False):
        return self._stage_begin("sitepile", allele_off, site_allele, site_pos, int(n_barcodes), raw=raw)

    def sitepile_add(self, aln, book_ptr, book, text, ops, raw=False):
        """aln: PILEUP_ALN_DTYPE records; record i books once per entry of book[book_ptr[i]:book_ptr[i + 1]] (barcode << 1 | uniq); text / ops
        as for pileup_add.  Returns the kernels' device time in ms"""
        a = np.ascontiguousarray(aln, PILEUP_ALN_DTYPE)
        bp, bk = np.ascontiguousarray(book_ptr, np.uint64), np.ascontiguousarray(book, np.uint32)
        assert len(bp) == len(a) + 1
        return self._stage_add("sitepile", a, (_ptr(bp), _ptr(bk)), text, ops, raw)

    def sitepile_get(self, raw=False):
        """the table's runs, ascending: (keys uint64, counts int32); key = ((barcode * nSites + site) * 7 + plane) * 2 + (1 - uniq)"""
        return self._stage_get("sitepile", raw)

    def sitepile_stats(self):
        """(keys emitted, folds, device ms of the folds) of the open table"""
        return self._stage_stats("sitepile", 2)

    def sitepile_end(self, raw=False):
        return self._stage_end("sitepile", raw)

    def sitepile(self, allele_off, site_allele, site_pos, n_barcodes, aln, book_ptr, book, text, ops, cuts=()):
        """begin, add (the records split at the indices `cuts` into several calls), get, end: (keys, counts, kernels' ms, folds)"""
        a = np.ascontiguousarray(aln, PILEUP_ALN_DTYPE)
        bp = np.ascontiguousarray(book_ptr, np.uint64)
        self.sitepile_begin(allele_off, site_allele, site_pos, n_barcodes)
        return self._stage_run("sitepile", len(a),
                               lambda lo, hi: self.sitepile_add(a[lo:hi], bp[lo:hi + 1], book, text, ops), lambda: self.sitepile_stats()[1], cuts)

    # strand / mate / end-distance / template support at sites (t1k_support_begin / _add / _get / _stats / _end); raw=True returns the status
    # code instead of raising
    def support_begin(self, allele_off, site_allele, site_pos, raw=False):
        return self._stage_begin("support", allele_off, site_allele, site_pos, raw=raw)

    def support_add(self, aln, rec, book_ptr, book, text, ops, raw=False):
        """aln: PILEUP_ALN_DTYPE records; rec: one SUPPORT_REC_DTYPE per record (its read-end's length, the bases in front of the window, the
        strand); record i books once per entry of book[book_ptr[i]:book_ptr[i + 1]] (SUPPORT_BOOK_DTYPE: flags = uniq | mate << 1 |
        orient << 2, the template's extent); text / ops as for pileup_add.  Returns the kernels' device time in ms"""
        a = np.ascontiguousarray(aln, PILEUP_ALN_DTYPE)
        rc_ = np.ascontiguousarray(rec, SUPPORT_REC_DTYPE)
        bp, bk = np.ascontiguousarray(book_ptr, np.uint64), np.ascontiguousarray(book, SUPPORT_BOOK_DTYPE)
        assert len(bp) == len(a) + 1 and len(rc_) == len(a)
        return self._stage_add("support", a, (_ptr(rc_), _ptr(bp), _ptr(bk)), text, ops, raw)

    def support_get(self, raw=False):
        """the table's runs, ascending: (keys uint64, counts int32).  Below SUPPORT_FAMILY_B: key = ((((site * 7 + state) * 2 + strand) * 2 + mate)
        * 512 + d) * 2 + (1 - uniq); from there on: SUPPORT_FAMILY_B | ((site * 7 + state) * 2 + orient) << 24 | dStart << 12 | dEnd, one run per
        distinct template"""
        return self._stage_get("support", raw)

    def support_stats(self):
        """(keys emitted, folds, device ms of the folds) of the open table"""
        return self._stage_stats("support", 2)

    def support_end(self, raw=False):
        return self._stage_end("support", raw)

    def support(self, allele_off, site_allele, site_pos, aln, rec, book_ptr, book, text, ops, cuts=()):
        """begin, add (the records split at the indices `cuts` into several calls), get, end: (keys, counts, kernels' ms, folds)"""
        a = np.ascontiguousarray(aln, PILEUP_ALN_DTYPE)
        rc_ = np.ascontiguousarray(rec, SUPPORT_REC_DTYPE)
        bp = np.ascontiguousarray(book_ptr, np.uint64)
        self.support_begin(allele_off, site_allele, site_pos)
        return self._stage_run("support", len(a),
                               lambda lo, hi: self.support_add(a[lo:hi], rc_[lo:hi], bp[lo:hi + 1], book, text, ops), lambda: self.support_stats()[1], cuts)

    # novel indel evidence, left-aligned (t1k_indel_begin / _add / _get / _stats / _end); raw=True returns the status code instead of raising
    def indel_begin(self, allele_off, allele_text, raw=False):
        """allele_text: the alleles' bases back to back (bytes or uint8, A C G T N), allele a at allele_text[allele_off[a]:allele_off[a + 1]]"""
        off = np.ascontiguousarray(allele_off, np.uint64)
        t = _u8(allele_text)
        assert len(off) == 0 or len(t) == int(off[-1])
        return self._done(lib().t1k_indel_begin(self.h, max(len(off) - 1, 0), _ptr(off), _ptr(t)), "t1k_indel_begin", raw)

    def indel_add(self, aln, strand, book_ptr, book_uniq, text, ops, raw=False):
        """aln: PILEUP_ALN_DTYPE records; strand: one uint8 per record (0 forward, 1 reverse); record i books once per entry of
        book_uniq[book_ptr[i]:book_ptr[i + 1]] (uint8: 1 when the booking's fragment has a single assignment); text / ops as for pileup_add.
        Returns the kernels' device time in ms"""
        a = np.ascontiguousarray(aln, PILEUP_ALN_DTYPE)
        s = np.ascontiguousarray(strand, np.uint8)
        bp, bk = np.ascontiguousarray(book_ptr, np.uint64), np.ascontiguousarray(book_uniq, np.uint8)
        assert len(bp) == len(a) + 1 and len(s) == len(a)
        return self._stage_add("indel", a, (_ptr(s), _ptr(bp), _ptr(bk)), text, ops, raw)

    def indel_get(self, raw=False):
        """the table's runs, ascending: (keys uint64, counts int32); key = ((((g << 2 | type) << 27 | payload) << 1 | strand) << 1) | (1 - uniq)
        with g = allele_off[allele] + the normalised position, type 0 DEL (payload = length), 1 short INS (payload = 1 << 2 L | bases),
        2 long INS (payload = length)"""
        return self._stage_get("indel", raw)

    def indel_stats(self):
        """(events, shifted, edge del columns x bookings, edge ins columns x bookings, keys emitted, folds, device ms of the folds) of the open table"""
        return self._stage_stats("indel", 6)

    def indel_end(self, raw=False):
        return self._stage_end("indel", raw)

    def indel(self, allele_off, allele_text, aln, strand, book_ptr, book_uniq, text, ops, cuts=()):
        """begin, add (the records split at the indices `cuts` into several calls), get, stats, end: (keys, counts, kernels' ms, stats)"""
        a = np.ascontiguousarray(aln, PILEUP_ALN_DTYPE)
        s = np.ascontiguousarray(strand, np.uint8)
        bp = np.ascontiguousarray(book_ptr, np.uint64)
        self.indel_begin(allele_off, allele_text)
        return self._stage_run("indel", len(a),
                               lambda lo, hi: self.indel_add(a[lo:hi], s[lo:hi], bp[lo:hi + 1], book_uniq, text, ops), self.indel_stats, cuts)

    # read-backed phasing of site pairs (t1k_phase_begin / _add / _get / _stats / _end); raw=True returns the status code instead of raising
    def phase_begin(self, allele_off, site_allele, site_pos, raw=False):
        return self._stage_begin("phase", allele_off, site_allele, site_pos, raw=raw)

    def phase_add(self, aln, book_rec, book_uniq, text, ops, raw=False):
        """aln: PILEUP_ALN_DTYPE records; booking b is the fragment-assignment of records book_rec[b] = (rec1, rec2 or PHASE_NO_MATE), both
        indices into aln, with book_uniq[b] set when its fragment has one assignment; text / ops as for pileup_add.  Returns the kernels'
        device time in ms"""
        a = np.ascontiguousarray(aln, PILEUP_ALN_DTYPE)
        br, bu = np.ascontiguousarray(book_rec, np.uint32).reshape(-1, 2), np.ascontiguousarray(book_uniq, np.uint8)
        assert len(br) == len(bu)
        return self._stage_add("phase", a, (len(bu), _ptr(br), _ptr(bu)), text, ops, raw)

    def phase_get(self, raw=False):
        """the table's runs, ascending: (keys uint64, counts int32); key = (((s * nSites + t) * 36 + x * 6 + y) << 1) | (1 - uniq)"""
        return self._stage_get("phase", raw)

    def phase_stats(self, raw=False):
        """{observations, bookings (with two observed sites or more), keys, discordant, folds, fold_ms} of the open table"""
        v = self._stage_stats("phase", 5, raw)
        return v if raw else dict(zip(("observations", "bookings", "keys", "discordant", "folds", "fold_ms"), v))

    def phase_end(self, raw=False):
        return self._stage_end("phase", raw)

    def phase(self, allele_off, site_allele, site_pos, aln, book_rec, book_uniq, text, ops, cuts=()):
        """begin, add, get, end: (keys, counts, kernels' ms, stats).  cuts: booking indices at which the bookings are split into several
        calls; every call gets all the records"""
        br, bu = np.ascontiguousarray(book_rec, np.uint32).reshape(-1, 2), np.ascontiguousarray(book_uniq, np.uint8)
        self.phase_begin(allele_off, site_allele, site_pos)
        return self._stage_run("phase", len(bu),
                               lambda lo, hi: self.phase_add(aln, br[lo:hi], bu[lo:hi], text, ops), self.phase_stats, cuts)

    def mem_bytes(self):
        """bytes of device memory the context holds right now (t1k_ctx_mem_report, nothing printed)"""
        return int(lib().t1k_ctx_mem_report(self.h, None, 0))


def alt_pieces(group_ptr):
    """pieces a t1k_alt_batch call with this group_ptr uploads its entries in (env T1K_ALT_PIECE as the call itself reads it)"""
    gp = np.ascontiguousarray(group_ptr, np.uint64)
    return int(lib().t1k_alt_pieces(max(len(gp) - 1, 0), _ptr(gp)))


def diplo_pieces(group_ptr):
    """pieces a t1k_diplo_batch call with this group_ptr uploads its entries in (env T1K_DIPLO_PIECE as the call itself reads it)"""
    gp = np.ascontiguousarray(group_ptr, np.uint64)
    return int(lib().t1k_diplo_pieces(max(len(gp) - 1, 0), _ptr(gp)))


def pair_limits():
    """(LDS join capacity, first launch's fragment capacity, rank-sort tile, records per streamed round) of the pairing kernel as built"""
    out = np.zeros(4, dtype=np.uint32)
    lib().t1k_pair_limits(_ptr(out))
    return tuple(int(x) for x in out)


def pair_direct_cap():
    """allele numbers a fragment's lists may span to take the pairing kernel's LDS table indexed by allele offset"""
    return int(lib().t1k_pair_direct_cap())


class Rowset:
    """All fragment rows of a job on one GPU (t1k_rowset): filled by pair_into, read back row by row or coalesced into read groups."""

    def __init__(self, ctx, n_fragments, whitelist=None, raw=False):
        wl = None if whitelist is None else np.ascontiguousarray(whitelist, dtype=np.uint8)
        h = C.c_void_p()
        ctx._check(lib().t1k_rowset_create(ctx.h, n_fragments, _ptr(wl), C.byref(h)), "t1k_rowset_create")
        self.h, self.ctx, self.n_fragments = h, ctx, n_fragments
        self._counts = self._all = None   # (groups, entries) of the last coalesce() / groups_gather()
        if raw:
            self._check(lib().t1k_rowset_set_raw(self.h, 1), "t1k_rowset_set_raw")

    def _check(self, rc, what):
        if rc != 0:
            raise T1kError("%s failed (%d): %s" % (what, rc, lib().t1k_rowset_last_error(self.h).decode()))

    def close(self):
        if self.h:
            lib().t1k_rowset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def pair_into(self, ctx, end1, end2, has_n, frag_base=0):
        e1 = np.asarray(end1, dtype=np.uint32)
        e2 = None if end2 is None else np.asarray(end2, dtype=np.uint32)
        hn = np.asarray(has_n, dtype=np.uint8)
        ctx._check(lib().t1k_pair_into(ctx.h, self.h, _ptr(e1), _ptr(e2), _ptr(hn), len(e1), frag_base), "t1k_pair_into")

    def rows(self, first=0, count=None):
        """(row counts, rows in the reference's row order) of fragments [first, first + count)"""
        count = self.n_fragments - first if count is None else count
        counts = np.zeros(count, dtype=np.uint32)
        tot = C.c_uint64()
        self._check(lib().t1k_rowset_rows_download(self.h, first, count, _ptr(counts), None, 0, C.byref(tot)), "t1k_rowset_rows_download")
        out = np.zeros(tot.value, dtype=ROW_DTYPE)
        self._check(lib().t1k_rowset_rows_download(self.h, first, count, _ptr(counts), _ptr(out), tot.value, C.byref(tot)), "t1k_rowset_rows_download")
        return counts, out

    def assigned(self, first=0, count=None):
        count = self.n_fragments - first if count is None else count
        out = np.zeros(count, dtype=np.uint8)
        self._check(lib().t1k_rowset_assigned_range(self.h, first, count, _ptr(out)), "t1k_rowset_assigned_range")
        return out

    def coalesce(self):
        """(read groups, their entries, fragments with the fragmentAssigned flag)"""
        g, e, a = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(lib().t1k_rowset_coalesce(self.h, C.byref(g), C.byref(e), C.byref(a)), "t1k_rowset_coalesce")
        self._counts = (g.value, e.value)
        return g.value, e.value, a.value

    def groups(self):
        """the read-group table of the last coalesce() (t1k_rowset_groups_download): (group_ptr uint64 [G + 1], entries as GROUP_DTYPE,
        first_fragment uint32 [G])"""
        if self._counts is None:
            raise T1kError("Rowset.groups: coalesce() has not been called")
        g, e = self._counts
        ptr, ent, first = np.zeros(g + 1, dtype=np.uint64), np.zeros(e, dtype=GROUP_DTYPE), np.zeros(g, dtype=np.uint32)
        self._check(lib().t1k_rowset_groups_download(self.h, _ptr(ptr), _ptr(ent), _ptr(first)), "t1k_rowset_groups_download")
        return ptr, ent, first

    def device_bytes(self):
        """(device bytes of the per-fragment arrays and the row chunks, row entries the calls have taken from the chunks so far)"""
        b, n = C.c_uint64(), C.c_uint64()
        self._check(lib().t1k_rowset_device_bytes(self.h, C.byref(b), C.byref(n)), "t1k_rowset_device_bytes")
        return b.value, n.value

    # ---- multi-GPU (collective calls: every rank's thread or process makes them in the same order) ----
    def exchange(self, comm, frag_base):
        """every fragment row goes to the rank that owns its pattern (t1k_rowset_exchange); frag_base = global index of this rank's first fragment"""
        self._check(lib().t1k_rowset_exchange(self.h, comm.h, frag_base), "t1k_rowset_exchange")

    def groups_gather(self, comm):
        """after coalesce() on every rank: all ranks' tables on every rank (t1k_rowset_groups_gather): (groups, entries, fragments with a row)"""
        g, e, a = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(lib().t1k_rowset_groups_gather(self.h, comm.h, C.byref(g), C.byref(e), C.byref(a)), "t1k_rowset_groups_gather")
        self._all = (g.value, e.value)
        return g.value, e.value, a.value

    def groups_all(self):
        """the gathered tables, concatenated in rank order (t1k_rowset_groups_download_all): (sizes uint32 [G], entries as GROUP_DTYPE,
        first_fragment uint32 [G] -- global fragment indices)"""
        if self._all is None:
            raise T1kError("Rowset.groups_all: groups_gather() has not been called")
        g, e = self._all
        sizes, ent, first = np.zeros(g, dtype=np.uint32), np.zeros(e, dtype=GROUP_DTYPE), np.zeros(g, dtype=np.uint32)
        self._check(lib().t1k_rowset_groups_download_all(self.h, _ptr(sizes), _ptr(ent), _ptr(first)), "t1k_rowset_groups_download_all")
        return sizes, ent, first


def boot_limits():
    """(entries requested ahead of the additions, the n_g from which the lanes share a replicate's draws, replicates per block) of t1k_boot_* as built"""
    out = np.zeros(3, np.uint32)
    lib().t1k_boot_limits(_ptr(out))
    return int(out[0]), int(out[1]), int(out[2])


def boot_stride(n_replicates):
    """the stride of the library's replicate-minor arrays: B + 1 replicates padded to whole blocks"""
    return int(lib().t1k_boot_stride(n_replicates))


def em_limits():
    """(entries per ordered piece, entries per step of the class pass) of t1k_em_update's sums as built"""
    out = np.zeros(2, dtype=np.uint32)
    lib().t1k_em_limits(_ptr(out))
    return tuple(int(x) for x in out)


def coalesce_limits():
    """(rows per batch, run length from which a group is folded by the four-wavefront kernel in this process, slots per tile) of the read-group fold"""
    out = np.zeros(3, dtype=np.uint32)
    lib().t1k_coalesce_limits(_ptr(out))
    return tuple(int(x) for x in out)


class Readset:
    """A finished read set kept resident (t1k_readset): distinct read-ends + their final overlap lists."""

    def __init__(self, h):
        self.h = h

    def bytes(self):
        return int(lib().t1k_readset_bytes(self.h))

    def size(self):
        return int(lib().t1k_readset_size(self.h))

    def close(self):
        if self.h:
            lib().t1k_readset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Xwin:
    """The table of read-ends across the windows of a job (t1k_xwin; test use: a job makes its own).  A window is a context whose read set
    t1k_reads_dedupe has collapsed; the contexts, or the read sets detached from them, must outlive the table's use."""

    def __init__(self, owner, max_read_ends, max_windows):
        h = C.c_void_p()
        owner._check(lib().t1k_xwin_create(owner.h, max_read_ends, max_windows, C.byref(h)), "t1k_xwin_create")
        self.h = h

    def _check(self, rc, what):
        if rc != 0:
            raise T1kError("%s failed (%d): %s" % (what, rc, self.last_error()))

    def last_error(self):
        return lib().t1k_xwin_last_error(self.h).decode()

    def close(self):
        if self.h:
            lib().t1k_xwin_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def link(self, reader, window, raw=False):
        """the distinct read-ends of `reader` (window `window`) whose sequence an earlier window holds are marked, the others become known to
        later windows (t1k_xwin_link): how many were marked.  raw=True: (status code, that count) without raising"""
        n = C.c_uint32()
        rc = lib().t1k_xwin_link(self.h, reader.h, window, C.byref(n))
        if raw:
            return rc, n.value
        self._check(rc, "t1k_xwin_link")
        return n.value

    def resolve(self, ctx, window, raw=False):
        """the marked read-ends of window `window` take the list-table entries of the windows that assigned their sequences (t1k_xwin_resolve);
        raw=True returns the status code instead of raising"""
        rc = lib().t1k_xwin_resolve(self.h, ctx.h, window)
        if raw:
            return rc
        self._check(rc, "t1k_xwin_resolve")


class Reads:
    """The read files of a job, mapped and indexed on their own (t1k_reads_open): needs no GPU and no job, so a second thread can open
    them while Job(...) parses the reference and brings the contexts up (ctypes releases the GIL for both calls); Job.attach_reads
    takes the input over.  f1 / f2 / barcode as in Job.load_reads."""

    def __init__(self, f1, f2=None, barcode=None, threads=0, stream=False):
        """stream=True: t1k_reads_open_stream -- ordinary .gz files are handed to Job.run while they are still being inflated"""
        l1 = [f1] if isinstance(f1, str) else list(f1)
        l2 = [] if not f2 else ([f2] if isinstance(f2, str) else list(f2))
        a1 = (C.c_char_p * len(l1))(*[x.encode() for x in l1])
        a2 = (C.c_char_p * len(l2))(*[x.encode() for x in l2]) if l2 else None
        h = C.c_void_p()
        opener = lib().t1k_reads_open_stream if stream else lib().t1k_reads_open
        rc = opener(a1, len(l1), a2, len(l2), barcode.encode() if barcode else None, threads, C.byref(h))
        if rc != 0:
            msg = lib().t1k_reads_last_error(h).decode() if h else "bad arguments"
            if h:
                lib().t1k_reads_close(h)
            raise T1kError("t1k_reads_open failed (%d): %s" % (rc, msg))
        self.h = h

    def fragments(self):
        n = C.c_uint64()
        if lib().t1k_reads_fragments(self.h, C.byref(n)) != 0:
            raise T1kError("t1k_reads_fragments failed")
        return n.value

    def close(self):
        if self.h:
            lib().t1k_reads_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Job:
    """Whole-stage job (t1k_job): host C++ around the device stages; same behaviour as the `genotyper` executable."""

    def __init__(self, ref_fasta, **kw):
        L = lib()
        p = JobParams()
        L.t1k_job_params_default(C.byref(p))
        for k, v in kw.items():
            if hasattr(p.dev, k):
                setattr(p.dev, k, v)
            elif k == "allele_delimiter":
                p.allele_delimiter = v.encode() if isinstance(v, str) else v
            else:
                setattr(p, k, v)
        self.params = p
        h = C.c_void_p()
        rc = L.t1k_job_create(C.byref(p), ref_fasta.encode(), C.byref(h))
        if rc != 0:
            msg = L.t1k_job_last_error(h).decode() if h else "no GPU / cannot read reference"
            raise T1kError("t1k_job_create failed (%d): %s" % (rc, msg))
        self.h = h

    def _check(self, rc, what):
        if rc != 0:
            raise T1kError("%s failed (%d): %s" % (what, rc, lib().t1k_job_last_error(self.h).decode()))

    def close(self):
        if self.h:
            lib().t1k_job_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_reads(self, f1, f2=None, barcode=None):
        """f1 / f2: a path, or a list of paths read back to back (every -1 / -2 of the executable).  On a rank of a sharded job
        (set_shard came first) the call is collective and indexes this rank's fragments only."""
        l1 = [f1] if isinstance(f1, str) else list(f1)
        l2 = [] if not f2 else ([f2] if isinstance(f2, str) else list(f2))
        a1 = (C.c_char_p * len(l1))(*[x.encode() for x in l1])
        a2 = (C.c_char_p * len(l2))(*[x.encode() for x in l2]) if l2 else None
        self._check(lib().t1k_job_load_reads_multi(self.h, a1, len(l1), a2, len(l2), barcode.encode() if barcode else None), "t1k_job_load_reads")

    def attach_reads(self, reads):
        """take over a Reads object (consumed, also on failure): the same state load_reads leaves"""
        h, reads.h = reads.h, None
        self._check(lib().t1k_job_attach_reads(self.h, h), "t1k_job_attach_reads")

    def set_reads(self, seqs1, seqs2=None):
        b1, o1 = _concat(seqs1)
        b2, o2 = _concat(seqs2) if seqs2 is not None else (None, None)
        self._check(lib().t1k_job_set_reads(self.h, b1, _ptr(o1), b2, _ptr(o2), len(seqs1)), "t1k_job_set_reads")

    def run(self):
        self._check(lib().t1k_job_run(self.h), "t1k_job_run")

    def set_output_prefix(self, prefix):
        lib().t1k_job_set_output_prefix.argtypes = [C.c_void_p, C.c_char_p]
        self._check(lib().t1k_job_set_output_prefix(self.h, prefix.encode()), "t1k_job_set_output_prefix")

    def write_outputs(self, prefix):
        self._check(lib().t1k_job_write_outputs(self.h, prefix.encode()), "t1k_job_write_outputs")

    def genotype_text(self):
        need = C.c_uint64()
        lib().t1k_job_genotype_text(self.h, None, 0, C.byref(need))
        buf = C.create_string_buffer(need.value + 1)
        self._check(lib().t1k_job_genotype_text(self.h, buf, need.value + 1, C.byref(need)), "t1k_job_genotype_text")
        return buf.value.decode()

    def alternatives_text(self):
        """the text of <prefix>_alternatives.tsv (a job created with alternatives=N, after run())"""
        need = C.c_uint64()
        self._check(lib().t1k_job_alternatives_text(self.h, None, 0, C.byref(need)), "t1k_job_alternatives_text")
        buf = C.create_string_buffer(need.value + 1)
        self._check(lib().t1k_job_alternatives_text(self.h, buf, need.value + 1, C.byref(need)), "t1k_job_alternatives_text")
        return buf.value.decode()

    def diplotypes_text(self):
        """the text of <prefix>_diplotypes.tsv (a job created with diplotypes=N, after run())"""
        need = C.c_uint64()
        self._check(lib().t1k_job_diplotypes_text(self.h, None, 0, C.byref(need)), "t1k_job_diplotypes_text")
        buf = C.create_string_buffer(need.value + 1)
        self._check(lib().t1k_job_diplotypes_text(self.h, buf, need.value + 1, C.byref(need)), "t1k_job_diplotypes_text")
        return buf.value.decode()

    def bootstrap_text(self):
        """the text of <prefix>_bootstrap.tsv (a job created with bootstrap=B, after run())"""
        need = C.c_uint64()
        self._check(lib().t1k_job_bootstrap_text(self.h, None, 0, C.byref(need)), "t1k_job_bootstrap_text")
        buf = C.create_string_buffer(need.value + 1)
        self._check(lib().t1k_job_bootstrap_text(self.h, buf, need.value + 1, C.byref(need)), "t1k_job_bootstrap_text")
        return buf.value.decode()

    def bootstrap_matrix(self):
        """(abundance float64 [B + 1][A], rounds int32 [B + 1], valid bool [B + 1]) of the replicates 0 .. B (0: the data)"""
        b, a = C.c_uint32(), C.c_uint32()
        self._check(lib().t1k_job_bootstrap_matrix(self.h, None, None, None, C.byref(b), C.byref(a)), "t1k_job_bootstrap_matrix")
        ab, rounds, valid = np.zeros((b.value + 1, a.value), np.float64), np.zeros(b.value + 1, np.int32), np.zeros(b.value + 1, np.uint8)
        self._check(lib().t1k_job_bootstrap_matrix(self.h, _ptr(ab), _ptr(rounds), _ptr(valid), C.byref(b), C.byref(a)), "t1k_job_bootstrap_matrix")
        return ab, rounds, valid.astype(bool)

    def em_alleles(self):
        """(ec, weight, eff_len, series: int32 [A] each) of the job's alleles: what its EM ran on besides the read groups (t1k_job_em_alleles)"""
        n = C.c_uint32()
        self._check(lib().t1k_job_em_alleles(self.h, None, None, None, None, C.byref(n)), "t1k_job_em_alleles")
        out = [np.zeros(n.value, np.int32) for _ in range(4)]
        self._check(lib().t1k_job_em_alleles(self.h, *[_ptr(a) for a in out], C.byref(n)), "t1k_job_em_alleles")
        return tuple(out)

    def series_names(self):
        need = C.c_uint64()
        self._check(lib().t1k_job_series_names(self.h, None, 0, C.byref(need)), "t1k_job_series_names")
        buf = C.create_string_buffer(need.value + 1)
        self._check(lib().t1k_job_series_names(self.h, buf, need.value + 1, C.byref(need)), "t1k_job_series_names")
        return buf.value.decode().splitlines()

    def allele_table(self):
        """(gene int32 [A], abundance float64 [A]) of the job's alleles, in the order of its reference"""
        n = C.c_uint32()
        self._check(lib().t1k_job_allele_table(self.h, None, None, C.byref(n)), "t1k_job_allele_table")
        gene, ab = np.zeros(n.value, np.int32), np.zeros(n.value, np.float64)
        self._check(lib().t1k_job_allele_table(self.h, _ptr(gene), _ptr(ab), C.byref(n)), "t1k_job_allele_table")
        return gene, ab

    def counts(self):
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        e = C.c_int32()
        self._check(lib().t1k_job_counts(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)), "t1k_job_counts")
        return dict(fragments=a.value, assigned_fragments=b.value, groups=c.value, ecs=d.value, em_iterations=e.value)

    def stats(self):
        s = Stats()
        lib().t1k_job_stats(self.h, C.byref(s))
        return s.as_dict()

    # ---- multi-GPU building blocks (include/t1k_gpu.h, "multi-GPU jobs") ----
    def set_shard(self, rank, n_ranks, comm):
        """this job is rank `rank` of `n_ranks`: it owns the fragments [F*rank/n, F*(rank+1)/n) of the loaded input"""
        self._comm = comm
        self._check(lib().t1k_job_set_shard(self.h, rank, n_ranks, comm.h if comm is not None else None), "t1k_job_set_shard")

    def share_reads(self, other):
        self._check(lib().t1k_job_share_reads(self.h, other.h), "t1k_job_share_reads")

    def ctx(self):
        return lib().t1k_job_ctx(self.h)

    def run_local(self):
        self._check(lib().t1k_job_run_local(self.h), "t1k_job_run_local")

    def finish(self):
        self._check(lib().t1k_job_finish(self.h), "t1k_job_finish")

    def groups_serialize(self):
        need = C.c_uint64()
        self._check(lib().t1k_job_groups_serialize(self.h, None, 0, C.byref(need)), "t1k_job_groups_serialize")
        buf = np.zeros(need.value, dtype=np.uint8)
        self._check(lib().t1k_job_groups_serialize(self.h, _ptr(buf), need.value, C.byref(need)), "t1k_job_groups_serialize")
        return buf

    def groups_merge(self, bufs):
        """the group tables of all pattern owners (byte strings of groups_serialize) become this job's table, ordered by first fragment"""
        bufs = [np.ascontiguousarray(b, dtype=np.uint8) for b in bufs]
        ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
        lens = np.array([b.size for b in bufs], dtype=np.uint64)
        self._check(lib().t1k_job_groups_merge(self.h, ptrs, _ptr(lens), len(bufs)), "t1k_job_groups_merge")

    def coalesce_rows(self, rows, row_counts, fragments=None):
        rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
        rc = np.ascontiguousarray(row_counts, dtype=np.uint32)
        fr = None if fragments is None else np.ascontiguousarray(fragments, dtype=np.uint32)
        self._check(lib().t1k_job_coalesce_rows(self.h, _ptr(rows), _ptr(rc), _ptr(fr), len(rc)), "t1k_job_coalesce_rows")

    def call_variants(self, abundance, var_max_group, asg_ptr, asg, ops, reads1, reads2=None):
        """VariantCaller::ComputeVariant on this job's alleles (t1k_variants_call; host code, a device=-1 job will do): asg[asg_ptr[f] :
        asg_ptr[f + 1]] = fragment f's assignment list (FRAG_ASG_DTYPE), ops = the edit strings its ops1 / ops2 offsets point into"""
        ab = np.ascontiguousarray(abundance, dtype=np.float64)
        ap = np.ascontiguousarray(asg_ptr, dtype=np.uint64)
        asg = np.ascontiguousarray(asg, dtype=FRAG_ASG_DTYPE)
        ops = np.ascontiguousarray(ops, dtype=np.int8)
        n = len(ap) - 1

        def side(reads):
            b = [r.encode() if isinstance(r, str) else r for r in reads]
            return b, (C.c_char_p * n)(*b), np.array([len(x) for x in b], dtype=np.uint32)
        b1, p1, l1 = side(reads1)
        b2, p2, l2 = side(reads2) if reads2 is not None else (None, None, None)
        h = C.c_void_p()
        self._check(lib().t1k_variants_call(self.h, _ptr(ab), var_max_group, n, _ptr(ap), _ptr(asg), _ptr(ops), p1, _ptr(l1), p2, _ptr(l2), C.byref(h)), "t1k_variants_call")
        return Variants(h, self)

    def coverage_device(self):
        """(device pointer, element count) of the int32 coverage difference array"""
        p, n = C.c_void_p(), C.c_uint64()
        ctx = lib().t1k_job_ctx(self.h)
        if lib().t1k_coverage_device(ctx, C.byref(p), C.byref(n)) != 0:
            raise T1kError("t1k_coverage_device failed")
        return p.value, n.value


def fragment_details(l1, l2, alleles, paired=True):
    """t1k_fragment_details: the overlaps behind a fragment's kept assignments (OVERLAP_DTYPE lists of its read-ends -> FRAG_ASG_DTYPE)"""
    l1 = np.ascontiguousarray(l1, dtype=OVERLAP_DTYPE)
    l2 = np.ascontiguousarray(l2 if l2 is not None else [], dtype=OVERLAP_DTYPE)
    al = np.ascontiguousarray(alleles, dtype=np.int32)
    out = np.zeros(len(al), dtype=FRAG_ASG_DTYPE)
    rc = lib().t1k_fragment_details(_ptr(l1), len(l1), _ptr(l2), len(l2), 1 if paired else 0, _ptr(al), len(al), _ptr(out))
    if rc != 0:
        raise T1kError("t1k_fragment_details failed (%d): an allele of the row has no candidate in the lists" % rc)
    return out


class Variants:
    """called variants of an analyzer run (t1k_variants): VariantCaller's finalVariants and what reads them"""

    def __init__(self, h, job):
        self.h, self.job = h, job  # (the job must outlive the result)

    def close(self):
        if self.h:
            lib().t1k_variants_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def records(self):
        out = np.zeros(lib().t1k_variants_count(self.h), dtype=VARIANT_DTYPE)
        if len(out) and lib().t1k_variants_get(self.h, _ptr(out)) != 0:
            raise T1kError("t1k_variants_get failed")
        return out

    def vcf(self):
        """the text of <prefix>_allele.vcf"""
        need = C.c_uint64()
        if lib().t1k_variants_vcf(self.h, None, 0, C.byref(need)) != 0:
            raise T1kError("t1k_variants_vcf failed")
        buf = C.create_string_buffer(need.value + 1)
        if lib().t1k_variants_vcf(self.h, buf, need.value + 1, C.byref(need)) != 0:
            raise T1kError("t1k_variants_vcf failed")
        return buf.value.decode()

    def adjust(self, asg, ops, read1, read2=None):
        """VariantCaller::AdjustFragmentAssignment for one fragment: a 0/1 flag per assignment"""
        asg = np.ascontiguousarray(asg, dtype=FRAG_ASG_DTYPE)
        ops = np.ascontiguousarray(ops, dtype=np.int8)
        keep = np.zeros(len(asg), dtype=np.uint8)
        b1 = read1.encode() if isinstance(read1, str) else read1
        b2 = None if read2 is None else (read2.encode() if isinstance(read2, str) else read2)
        if lib().t1k_variants_adjust(self.h, _ptr(asg), len(asg), _ptr(ops), b1, len(b1), b2, len(b2) if b2 else 0, _ptr(keep)) != 0:
            raise T1kError("t1k_variants_adjust failed")
        return keep


class CommGroup:
    """meeting point of the rank threads of one process (t1k_comm_group)"""

    def __init__(self, n_ranks):
        self.h = lib().t1k_comm_group_create(n_ranks)

    def close(self):
        if self.h:
            lib().t1k_comm_group_destroy(self.h)
            self.h = None


def pool_release():
    """give the process-wide device memory pool back to the driver; returns the bytes released"""
    return int(lib().t1k_pool_release())


def comm_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 calls this and hands them to the other ranks)"""
    buf = np.zeros(128, dtype=np.uint8)
    if lib().t1k_comm_unique_id(_ptr(buf)) != 0:
        raise T1kError("t1k_comm_unique_id failed: RCCL not available")
    return buf


class Comm:
    """One rank's communicator (t1k_comm): RCCL over xGMI between processes / GPUs, in-process transport between threads that share a GPU."""

    def __init__(self, owner, n_ranks, rank, unique_id=None, group=None, transport=-1):
        """owner: a Job or a Context on this rank's device (the communicator uses its stream until bind() moves it)"""
        h = C.c_void_p()
        uid = None if unique_id is None else np.ascontiguousarray(unique_id, dtype=np.uint8)
        ctx = owner.ctx() if hasattr(owner, "ctx") else owner.h
        rc = lib().t1k_comm_init(ctx, n_ranks, rank, _ptr(uid), group.h if group is not None else None, transport, C.byref(h))
        self.h = h
        if rc != 0:
            msg = lib().t1k_comm_last_error(h).decode() if h else ""
            if h:
                lib().t1k_comm_abort(h)   # the ranks that wait for this one at the group's meeting point are released
            raise T1kError("t1k_comm_init failed (%d): %s" % (rc, msg))

    def bind(self, owner):
        """owner: a Job or a Context, as in __init__"""
        ctx = owner.ctx() if hasattr(owner, "ctx") else owner.h
        if lib().t1k_comm_bind(self.h, ctx) != 0:
            raise T1kError("t1k_comm_bind failed")

    def is_rccl(self):
        return bool(lib().t1k_comm_is_rccl(self.h))

    def abort(self):
        """a rank that cannot go on releases the ranks waiting for it (t1k_comm_abort): their collectives fail instead of waiting"""
        if self.h:
            lib().t1k_comm_abort(self.h)

    def close(self):
        if self.h:
            lib().t1k_comm_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------------------------------------------------------------
# small host-side helpers for tests / bench (format conventions of the reference's ReadFiles.hpp / SeqSet::InputRefSeq)
# ---------------------------------------------------------------------------------------------------------------------
def _open(path):
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path, "rt")


def read_fastx(path):
    """-> list of (id, comment, seq).  id loses a trailing /1 or /2 (ReadFiles.hpp:185-189)."""
    out = []
    with _open(path) as f:
        lines = [l.rstrip("\r\n") for l in f]
    i = 0
    while i < len(lines):
        l = lines[i]
        if not l or l[0] not in ">@":
            i += 1
            continue
        fq = l[0] == "@"
        head = l[1:].split(None, 1)
        rid = head[0] if head else ""
        comment = head[1] if len(head) > 1 else ""
        if len(rid) >= 2 and rid[-2] == "/" and rid[-1] in "12":
            rid = rid[:-2]
        i += 1
        seq = []
        while i < len(lines) and not (lines[i][:1] in (">", "@", "+") and lines[i][:1] != ""):
            seq.append(lines[i])
            i += 1
        seq = "".join(seq)
        if fq and i < len(lines) and lines[i][:1] == "+":
            i += 1
            q = 0
            while i < len(lines) and q < len(seq):
                q += len(lines[i])
                i += 1
        out.append((rid, comment, seq))
    return out


def load_reference_fasta(path):
    """Reference loading as Genotyper::InitRefSet does it (Genotyper.hpp:707-730): identical sequences collapse onto the
    first name; exon mask from the header comment (SeqSet.hpp:933-976).  -> names, seqs, exon masks (uint8 arrays), weights"""
    names, seqs, masks, weights, seen = [], [], [], [], {}
    for rid, comment, seq in read_fastx(path):
        if seq in seen:
            weights[seen[seq]] += 1
            continue
        seen[seq] = len(seqs)
        L = len(seq)
        exons = []
        if comment:
            nums, n = [], 0
            for ch in comment:
                if ch.isdigit():
                    n = n * 10 + int(ch)
                else:
                    nums.append(n)
                    n = 0
            if n:
                nums.append(n)
            if nums:
                for i in range(1, len(nums), 2):
                    exons.append((nums[i], nums[i + 1] if i + 1 < len(nums) else 0))
            else:
                exons.append((0, L - 1))
        else:
            exons.append((0, L - 1))
        m = np.zeros(L, dtype=np.uint8)
        for a, b in exons:
            m[max(a, 0):min(b, L - 1) + 1] = 1
        names.append(rid); seqs.append(seq); masks.append(m); weights.append(1)
    return names, seqs, masks, weights
