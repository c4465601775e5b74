"""ctypes binding of libbiogpu.so (include/biogpu.h).  No CPU fallback: if the library or a
gfx950 device is missing, everything that needs the GPU raises."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libbiogpu.so")
CSRC = os.path.join(_HERE, "csrc")

BG_OK = 0
ERRORS = {-1: "INVALID_ARG", -2: "NO_DEVICE", -3: "HIP", -4: "OOM", -5: "SENTINEL",
          -6: "POSITIVE_PENALTY", -7: "OUT_OF_ALPHABET", -8: "TOO_LARGE", -9: "OPS_CAP",
          -10: "TRACEBACK", -11: "UNSUPPORTED", -12: "IO"}
MIN_SCORE = -858993459
# BG_STRAND_* (which strands bg_seed_extend_strands_batch[_dev] maps) and BG_HIT_* (the strand of a read's winner)
STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = 1, 2, 3
HIT_FORWARD, HIT_REVERSE, HIT_NONE = 0, 1, 255
# BG_FILL_* (include/biogpu.h): fill kernel families, as Context.last_fill_kernels() reports them
FILL = {"K1_WIDE": 0x1, "K1_NARROW": 0x2, "K1_LF": 0x4, "K1P": 0x8, "K1P_LF": 0x10, "K3": 0x20, "K3V2_WIDE": 0x40,
        "K3V2_NARROW": 0x80, "K3I": 0x100, "K3P": 0x200}


class BiogpuError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        msg = lib().bg_strerror(status).decode()
        last = lib().bg_last_error().decode()
        super().__init__(f"{where}: {ERRORS.get(status, status)}: {msg}" + (f" [{last}]" if last else ""))


class SentinelError(BiogpuError, ValueError):
    """suffix_array.rs:431-437 assert"""


class PenaltyError(BiogpuError, AssertionError):
    """pairwise/mod.rs:265-266,554-571 asserts"""


class AlphabetError(BiogpuError, IndexError):
    """fmindex.rs:229 / bwt.rs:158 index out of bounds"""


_EXC = {-5: SentinelError, -6: PenaltyError, -7: AlphabetError}


def check(status, where=""):
    if status != BG_OK:
        raise _EXC.get(status, BiogpuError)(status, where)


class ScoringC(C.Structure):
    _fields_ = [("gap_open", C.c_int32), ("gap_extend", C.c_int32),
                ("xclip_prefix", C.c_int32), ("xclip_suffix", C.c_int32),
                ("yclip_prefix", C.c_int32), ("yclip_suffix", C.c_int32),
                ("match_score", C.c_int32), ("mismatch_score", C.c_int32),
                ("match_scores_some", C.c_int32),
                ("matrix", C.POINTER(C.c_int32))]


class TimingC(C.Structure):
    _fields_ = [("fill_ms", C.c_float), ("traceback_ms", C.c_float), ("fm_ms", C.c_float),
                ("fill_launches", C.c_uint32), ("traceback_launches", C.c_uint32),
                ("fm_launches", C.c_uint32)]


# bg_alignment_t
ALN_DTYPE = np.dtype([("score", "<i4"), ("xstart", "<u4"), ("xend", "<u4"), ("ystart", "<u4"),
                      ("yend", "<u4"), ("xlen", "<u4"), ("ylen", "<u4"), ("n_ops", "<u4"),
                      ("ops_off", "<u8"), ("clip_len", "<u4", (4,)), ("n_clips", "u1"),
                      ("mode", "u1"), ("status", "i1"), ("_pad", "u1"), ("_tail", "<u4")])
assert ALN_DTYPE.itemsize == 64, ALN_DTYPE.itemsize
# bg_seed_hit_t
SEED_HIT_DTYPE = np.dtype([("aln", ALN_DTYPE), ("window_start", "<u8"), ("ref_start", "<u8"), ("ref_end", "<u8"),
                           ("n_candidates", "<u4"), ("n_seed_hits", "<u4")])
assert SEED_HIT_DTYPE.itemsize == 96, SEED_HIT_DTYPE.itemsize


class SeedParamsC(C.Structure):
    _fields_ = [("seed_len", C.c_uint32), ("stride", C.c_uint32), ("max_occ", C.c_uint32), ("pad", C.c_uint32)]


# bg_smem_seed_params_t (bg_seed_extend_smem_batch[_dev])
class SMEM_SEED_PARAMS(C.Structure):
    _fields_ = [("min_seed_len", C.c_uint32), ("max_smems", C.c_uint32), ("max_occ", C.c_uint32), ("pad", C.c_uint32)]


assert C.sizeof(SMEM_SEED_PARAMS) == 16, C.sizeof(SMEM_SEED_PARAMS)


# bg_tiered_seed_params_t (bg_seed_extend_tiered_batch[_dev]) and BG_TIER_* (tier[r] of a read)
class TIERED_SEED_PARAMS(C.Structure):
    _fields_ = [("window", SeedParamsC), ("smem", SMEM_SEED_PARAMS), ("reseed_below", C.c_int32)]


assert C.sizeof(TIERED_SEED_PARAMS) == 36, C.sizeof(TIERED_SEED_PARAMS)
TIER_NONE, TIER_FIRST, TIER_SECOND = 0, 1, 2


# bg_pair_params_t (bg_seed_extend_pairs_batch[_dev])
class PAIR_PARAMS(C.Structure):
    _fields_ = [("min_span", C.c_uint32), ("max_span", C.c_uint32), ("pen_unpaired", C.c_int32)]


assert C.sizeof(PAIR_PARAMS) == 12, C.sizeof(PAIR_PARAMS)
# bg_pair_hit_t
PAIR_HIT_DTYPE = np.dtype([("span", "<u8"), ("n_proper", "<u4"), ("proper", "u1"), ("reserved", "u1", (3,))])
assert PAIR_HIT_DTYPE.itemsize == 16, PAIR_HIT_DTYPE.itemsize


# bg_rescue_params_t (bg_seed_extend_pairs_rescue_batch[_dev])
class RESCUE_PARAMS(C.Structure):
    _fields_ = [("max_anchors", C.c_uint32), ("min_score", C.c_int32)]


assert C.sizeof(RESCUE_PARAMS) == 8, C.sizeof(RESCUE_PARAMS)
RESCUE_MAX_ANCHORS = 4


# bg_multi_params_t (bg_seed_extend_multi_batch[_dev])
SEED_MAX_HITS = 8


class MULTI_PARAMS(C.Structure):
    _fields_ = [("max_hits", C.c_uint32), ("min_score", C.c_int32), ("mapq_cap", C.c_uint32)]


assert C.sizeof(MULTI_PARAMS) == 12, C.sizeof(MULTI_PARAMS)
# bg_multi_hit_t
MULTI_HIT_DTYPE = np.dtype([("sub_score", "<i4"), ("n_loci", "<u4"), ("n_reported", "u1"), ("mapq", "u1"), ("reserved", "u1", (6,))])
assert MULTI_HIT_DTYPE.itemsize == 16, MULTI_HIT_DTYPE.itemsize


# bg_pairq_params_t (bg_seed_extend_pairs_mapq_batch[_dev])
class PAIRQ_PARAMS(C.Structure):
    _fields_ = [("min_score", C.c_int32), ("mapq_cap", C.c_uint32)]


assert C.sizeof(PAIRQ_PARAMS) == 8, C.sizeof(PAIRQ_PARAMS)


# bg_fastq_record_t
FQREC_DTYPE = np.dtype([("id_off", "<u8"), ("desc_off", "<u8"), ("seq_off", "<u8"), ("qual_off", "<u8"),
                        ("id_len", "<u4"), ("desc_len", "<u4"), ("seq_len", "<u4"), ("qual_len", "<u4"),
                        ("has_desc", "<i4"), ("check", "<i4")])
assert FQREC_DTYPE.itemsize == 56, FQREC_DTYPE.itemsize

# bg_fasta_record_t, BG_FASTA_TILE (the bytes of the text one block of the FASTA kernels works on) and BG_FASTA_REF_*
FAREC_DTYPE = np.dtype([("id_off", "<u8"), ("desc_off", "<u8"), ("seq_off", "<u8"), ("seq_len", "<u8"),
                        ("id_len", "<u4"), ("desc_len", "<u4"), ("has_desc", "<i4"), ("check", "<i4")])
assert FAREC_DTYPE.itemsize == 48, FAREC_DTYPE.itemsize
FASTA_TILE = 8192
FASTA_REF_FMD, FASTA_REF_UPPER = 1, 2

# bg_sam_contig_t, BG_SAM_* and bg_sam_params_t (bg_sam_header, bg_sam_emit_batch[_dev])
SAM_CONTIG_DTYPE = np.dtype([("start", "<u8"), ("len", "<u8"), ("name_off", "<u8"), ("name_len", "<u4"), ("reserved", "<u4")])
assert SAM_CONTIG_DTYPE.itemsize == 32, SAM_CONTIG_DTYPE.itemsize
SAM_PAIRED, SAM_SECONDARY, SAM_TAG_NM, SAM_TAG_MD = 1, 2, 4, 8


class SAM_PARAMS(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("max_hits", C.c_uint32)]


assert C.sizeof(SAM_PARAMS) == 8, C.sizeof(SAM_PARAMS)

# bg_markdup_params_t and BG_SAM_SO_* (bg_sam_markdup[_dev], bg_sam_header_so)
MARKDUP_PARAMS_DTYPE = np.dtype([("flags", "<u4"), ("max_hits", "<u4"), ("phred_offset", "<u4"), ("min_qual", "<u4")])
assert MARKDUP_PARAMS_DTYPE.itemsize == 16, MARKDUP_PARAMS_DTYPE.itemsize
SAM_SO_UNSORTED, SAM_SO_COORDINATE = 0, 1
BGZF_EOF = 1  # BG_BGZF_EOF
BAM_READS_ORIGINAL = 1  # BG_BAM_READS_ORIGINAL


# bg_bam_reads_t (bg_bam_reads[_dev])
class BAM_READS(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("require", C.c_uint16), ("exclude", C.c_uint16)]


assert C.sizeof(BAM_READS) == 8, C.sizeof(BAM_READS)

# bg_bam_region_t, bg_bam_pileup_t, BG_PILEUP_* and BG_PILEUP_TILE of csrc/bam_pileup_rule.h (bg_bam_pileup[_dev])
BAM_REGION_DTYPE = np.dtype([("ref", "<i4"), ("beg", "<i4"), ("end", "<i4")])
assert BAM_REGION_DTYPE.itemsize == 12, BAM_REGION_DTYPE.itemsize
BAM_PILEUP_DTYPE = np.dtype([("flags", "<u4"), ("require", "<u2"), ("exclude", "<u2"), ("min_mapq", "u1"), ("min_baseq", "u1"), ("reserved", "<u2")])
assert BAM_PILEUP_DTYPE.itemsize == 12, BAM_PILEUP_DTYPE.itemsize
PILEUP_STRANDS = 1
PILEUP_A, PILEUP_C, PILEUP_G, PILEUP_T, PILEUP_OTHER, PILEUP_DEL, PILEUP_SKIP, PILEUP_INS, PILEUP_COLS = range(9)
PILEUP_TILE = 512
# bg_bam_sites_t, bg_bam_site_t, bg_bam_region_summary_t and BG_SITE_* (bg_bam_sites[_dev])
BAM_SITES_DTYPE = np.dtype([("flags", "<u4"), ("require", "<u2"), ("exclude", "<u2"), ("min_mapq", "u1"), ("min_baseq", "u1"), ("reserved", "<u2"),
                            ("min_depth", "<u4"), ("min_alt", "<u4"), ("min_alt_permille", "<u4"), ("min_alt_strand", "<u4"), ("cover", "<u4", (4,))])
assert BAM_SITES_DTYPE.itemsize == 44, BAM_SITES_DTYPE.itemsize
BAM_SITE_DTYPE = np.dtype([("ref", "<i4"), ("pos", "<i4"), ("region", "<u4"), ("kind", "u1"), ("ref_base", "u1"), ("alt", "u1"), ("reserved", "u1"),
                           ("depth", "<u4"), ("ref_count", "<u4"), ("alt_fwd", "<u4"), ("alt_rev", "<u4")])
assert BAM_SITE_DTYPE.itemsize == 32, BAM_SITE_DTYPE.itemsize
BAM_REGION_SUMMARY_DTYPE = np.dtype([("sum_depth", "<u8"), ("match", "<u8"), ("mismatch", "<u8"), ("covered", "<u4", (4,)), ("max_depth", "<u4"),
                                     ("n_ref_other", "<u4")])
assert BAM_REGION_SUMMARY_DTYPE.itemsize == 48, BAM_REGION_SUMMARY_DTYPE.itemsize
SITE_SNV, SITE_DEL, SITE_INS = range(3)
# bg_bam_indels_t and bg_bam_indel_t (bg_bam_indels[_dev])
BAM_INDELS_DTYPE = np.dtype([("flags", "<u4"), ("require", "<u2"), ("exclude", "<u2"), ("min_mapq", "u1"), ("min_baseq", "u1"), ("reserved", "<u2"),
                             ("min_depth", "<u4"), ("min_alt", "<u4"), ("min_alt_permille", "<u4"), ("min_alt_strand", "<u4")])
assert BAM_INDELS_DTYPE.itemsize == 28, BAM_INDELS_DTYPE.itemsize
BAM_INDEL_DTYPE = np.dtype([("ref", "<i4"), ("pos", "<i4"), ("region", "<u4"), ("kind", "u1"), ("reserved", "u1", (3,)), ("len", "<u4"), ("depth", "<u4"),
                            ("alt_fwd", "<u4"), ("alt_rev", "<u4"), ("seq_off", "<u8")])
assert BAM_INDEL_DTYPE.itemsize == 40, BAM_INDEL_DTYPE.itemsize
# bg_bam_indels_left_t (bg_bam_indels_left[_dev]): bg_bam_indels_t, then max_shift
BAM_INDELS_LEFT_DTYPE = np.dtype(BAM_INDELS_DTYPE.descr + [("max_shift", "<u4")])
assert BAM_INDELS_LEFT_DTYPE.itemsize == 32, BAM_INDELS_LEFT_DTYPE.itemsize
# bg_vcf_params_t (bg_vcf_emit[_dev])
VCF_PARAMS_DTYPE = np.dtype([("flags", "<u4"), ("reserved", "<u4")])
assert VCF_PARAMS_DTYPE.itemsize == 8, VCF_PARAMS_DTYPE.itemsize

# bg_myers_pattern_t, BG_MYERS_* and BG_TRIM_* (bg_myers_*_batch[_dev], bg_fastq_trim[_dev])
MYERS_PATTERN_DTYPE = np.dtype([("peq", "<u8", (256,)), ("m", "<u4"), ("_reserved", "<u4")])
assert MYERS_PATTERN_DTYPE.itemsize == 2056, MYERS_PATTERN_DTYPE.itemsize
MYERS_ENDS_ONLY, MYERS_MAX_PATTERNS, MYERS_MAX_HITS = 1, 1024, 64
MYERS_LONG_MAX_M = 1024
TRIM_3P, TRIM_5P = 0, 1
# bg_fastq_filter_t and BG_FQF_* (bg_fastq_filter[_dev])
FQ_FILTER_DTYPE = np.dtype([("flags", "<u4"), ("min_len", "<u4"), ("max_len", "<u4"), ("max_n", "<u4")])
assert FQ_FILTER_DTYPE.itemsize == 16, FQ_FILTER_DTYPE.itemsize
FQF_PAIRED, FQF_PAIR_BOTH, FQF_DISCARD_UNTRIMMED, FQF_DISCARD_TRIMMED, FQF_CHECK_OK = 1, 2, 4, 8, 16
# bg_demux_params_t and BG_DMX_* (bg_fastq_demux_assign[_dev], bg_fastq_demux_split[_dev])
DEMUX_PARAMS_DTYPE = np.dtype([("flags", "<u4"), ("n_bins", "<u4"), ("min_margin", "<u4"), ("max_offset", "<u4")])
assert DEMUX_PARAMS_DTYPE.itemsize == 16, DEMUX_PARAMS_DTYPE.itemsize
DMX_ANCHOR_5P, DMX_ANCHOR_3P, DMX_PAIRED, DMX_MATE1, DMX_MATE2 = 1, 2, 4, 8, 16
DMX_IGNORE, DMX_MAX_BINS = 0xFFFFFFFF, 1024
# bg_qual_cut_t, bg_qual_select_t, bg_qual_stats_t, BG_QCUT_*, BG_QSEL_* and BG_QC_MAX_CYCLES (bg_fastq_qual_cut[_dev],
# bg_fastq_qual_select[_dev], bg_fastq_qc_tables[_dev])
QUAL_CUT_DTYPE = np.dtype([("phred_offset", "<u4"), ("method_5p", "<u4"), ("method_3p", "<u4"), ("cutoff_5p", "<u4"), ("cutoff_3p", "<u4"),
                           ("window", "<u4")])
assert QUAL_CUT_DTYPE.itemsize == 24, QUAL_CUT_DTYPE.itemsize
QUAL_SELECT_DTYPE = np.dtype([("flags", "<u4"), ("phred_offset", "<u4"), ("min_mean_q", "<u4"), ("low_q", "<u4"), ("max_low_pct", "<u4"),
                              ("_reserved", "<u4"), ("max_weight", "<u8")])
assert QUAL_SELECT_DTYPE.itemsize == 32, QUAL_SELECT_DTYPE.itemsize
QUAL_STATS_DTYPE = np.dtype([("sum_q", "<u8"), ("weight_sum", "<u8"), ("len", "<u4"), ("n_low", "<u4"), ("min_q", "<u4"), ("_reserved", "<u4")])
assert QUAL_STATS_DTYPE.itemsize == 32, QUAL_STATS_DTYPE.itemsize
QCUT_NONE, QCUT_RUNSUM, QCUT_WINDOW = 0, 1, 2
QSEL_PAIRED, QSEL_PAIR_BOTH = 1, 2
QC_MAX_CYCLES = 1024

SYMBOLS = ["bg_device_count", "bg_init", "bg_free", "bg_strerror", "bg_last_error",
           "bg_set_option", "bg_suffix_array", "bg_bwt", "bg_less", "bg_fm_build", "bg_fm_free",
           "bg_fm_device_bytes", "bg_fm_set_option", "bg_fm_backward_search_batch", "bg_fm_backward_search_batch_dev",
           "bg_fm_set_suffix_array", "bg_fm_set_sampled_suffix_array", "bg_sa_get_batch", "bg_sa_get_batch_dev",
           "bg_interval_occ_batch", "bg_interval_occ_batch_dev", "bg_fmd_smems_batch", "bg_fmd_smems_batch_dev", "bg_fmd_interval_batch",
           "bg_align_batch", "bg_align_batch_dev", "bg_align_banded_batch", "bg_align_banded_batch_dev", "bg_band_create_batch",
           "bg_align_banded_bands_batch", "bg_band_from_matches_batch", "bg_sparse_find_kmer_matches", "bg_sparse_sdpkpp",
           "bg_sparse_lcskpp", "bg_sparse_sdpkpp_union_lcskpp_path", "bg_sparse_expand_kmer_matches", "bg_fastq_parse",
           "bg_fastq_parse_dev", "bg_cigar_batch", "bg_cigar_batch_dev", "bg_get_timing", "bg_enable_timing", "bg_band_redo_pairs", "bg_last_fill_kernels", "bg_last_fill_framed", "bg_last_fill_max3", "bg_pack2_host",
           "bg_pretty_batch", "bg_suffix_array_dev", "bg_bwt_dev", "bg_sa_sample_dev", "bg_suffix_array_dev64", "bg_bwt_dev64", "bg_sa_sample_dev64", "bg_fm_build_dev", "bg_fm_set_text", "bg_fm_set_text_dev", "bg_seed_extend_batch", "bg_seed_extend_batch_dev",
           "bg_seed_extend_strands_batch", "bg_seed_extend_strands_batch_dev", "bg_revcomp_batch_dev",
           "bg_seed_extend_smem_batch", "bg_seed_extend_smem_batch_dev",
           "bg_seed_extend_tiered_batch", "bg_seed_extend_tiered_batch_dev",
           "bg_seed_extend_pairs_batch", "bg_seed_extend_pairs_batch_dev",
           "bg_seed_extend_pairs_rescue_batch", "bg_seed_extend_pairs_rescue_batch_dev",
           "bg_seed_extend_multi_batch", "bg_seed_extend_multi_batch_dev",
           "bg_seed_extend_pairs_mapq_batch", "bg_seed_extend_pairs_mapq_batch_dev",
           "bg_seed_extend_pairs_rescue_mapq_batch", "bg_seed_extend_pairs_rescue_mapq_batch_dev",
           "bg_sam_header", "bg_sam_emit_batch", "bg_sam_emit_batch_dev",
           "bg_sam_markdup", "bg_sam_markdup_dev", "bg_sam_emit_dup_batch", "bg_sam_emit_dup_batch_dev", "bg_sam_sort_keys",
           "bg_sam_sort_keys_dev", "bg_sam_sort", "bg_sam_sort_dev", "bg_sam_header_so",
           "bg_bam_header", "bg_bam_emit_batch", "bg_bam_emit_batch_dev", "bg_bgzf_frame", "bg_bgzf_frame_dev",
           "bg_bgzf_deflate", "bg_bgzf_deflate_dev", "bg_bam_index", "bg_bam_index_dev",
           "bg_bgzf_blocks", "bg_bgzf_blocks_dev", "bg_bgzf_inflate", "bg_bgzf_inflate_dev",
           "bg_bam_header_parse", "bg_bam_records", "bg_bam_records_dev", "bg_bam_reads", "bg_bam_reads_dev",
           "bg_bam_sort_keys", "bg_bam_sort_keys_dev", "bg_bam_index_blocks", "bg_bam_index_blocks_dev",
           "bg_bam_pileup", "bg_bam_pileup_dev", "bg_bam_sites", "bg_bam_sites_dev", "bg_bam_indels", "bg_bam_indels_dev", "bg_bam_indels_left", "bg_bam_indels_left_dev",
           "bg_vcf_header", "bg_vcf_emit", "bg_vcf_emit_dev",
           "bg_fasta_parse", "bg_fasta_parse_dev", "bg_fasta_reference", "bg_fasta_reference_dev",
           "bg_pack2_dev", "bg_unpack2_dev", "bg_fm_pattern_codes", "bg_fm_backward_search_packed_dev",
           "bg_fm_backward_search_count_lines_dev", "bg_align_batch_packed_dev", "bg_fm_step2_bytes",
           "bg_shard_range", "bg_shard_balanced", "bg_comm_unique_id", "bg_comm_init", "bg_comm_init_host",
           "bg_gather_records", "bg_gather_records_cap", "bg_gather_records_host", "bg_comm_free", "bg_fm_save", "bg_fm_load",
           "bg_fm_len", "bg_fm_less", "bg_fm_bwt", "bg_fm_bwt_dev", "bg_comm_world",
           "bg_fmd_smems_batch64", "bg_fmd_smems_batch64_dev", "bg_fmd_interval_batch64",
           "bg_myers_best_batch", "bg_myers_best_batch_dev", "bg_myers_find_all_batch", "bg_myers_find_all_batch_dev",
           "bg_myers_long_best_batch", "bg_myers_long_best_batch_dev", "bg_myers_long_find_all_batch", "bg_myers_long_find_all_batch_dev",
           "bg_fastq_trim", "bg_fastq_trim_dev", "bg_fastq_filter", "bg_fastq_filter_dev", "bg_fastq_emit", "bg_fastq_emit_dev",
           "bg_fastq_demux_assign", "bg_fastq_demux_assign_dev", "bg_fastq_demux_split", "bg_fastq_demux_split_dev",
           "bg_qc_tables_words", "bg_fastq_qual_cut", "bg_fastq_qual_cut_dev", "bg_fastq_qual_select", "bg_fastq_qual_select_dev",
           "bg_fastq_qc_tables", "bg_fastq_qc_tables_dev"]


def build(force=False):
    """Compile every HIP source for gfx950 into rust-bio_amd/libbiogpu.so (hipcc
    cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean", "-s"])
    subprocess.check_call(["make", "-C", CSRC, "-j8", "-s"])
    return SO_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; "
                               "g.build()'` (the engine has no CPU fallback)")
        L = C.CDLL(SO_PATH)
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.bg_strerror.restype = C.c_char_p
        L.bg_strerror.argtypes = [i32]
        L.bg_last_error.restype = C.c_char_p
        L.bg_device_count.restype = i32
        L.bg_init.argtypes = [i32, C.POINTER(vp)]
        L.bg_free.argtypes = [vp]
        L.bg_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
        L.bg_suffix_array.argtypes = [vp, u64, vp]
        L.bg_bwt.argtypes = [vp, vp, u64, vp]
        L.bg_less.argtypes = [vp, u64, vp, u32, vp, C.POINTER(u32)]
        L.bg_fm_build.argtypes = [vp, vp, u64, vp, u32, u32, vp, u32, C.POINTER(vp)]
        L.bg_fm_free.argtypes = [vp]
        L.bg_fm_save.argtypes = [vp, C.c_char_p]
        L.bg_fm_load.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
        L.bg_fm_len.argtypes = [vp, C.POINTER(u64)]
        L.bg_fm_less.argtypes = [vp, vp, C.POINTER(u32)]
        L.bg_fm_bwt.argtypes = [vp, vp]
        L.bg_fm_bwt_dev.argtypes = [vp, vp, vp]
        L.bg_fm_build_dev.argtypes = [vp, vp, u64, u32, vp, u32, vp, C.POINTER(vp), vp]
        L.bg_fm_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
        L.bg_fm_device_bytes.restype = u64
        L.bg_fm_device_bytes.argtypes = [vp]
        L.bg_fm_step2_bytes.restype = u64
        L.bg_fm_step2_bytes.argtypes = [vp]
        L.bg_shard_range.argtypes = [u64, i32, i32, C.POINTER(u64), C.POINTER(u64)]
        L.bg_shard_balanced.argtypes = [vp, u64, i32, vp]
        L.bg_comm_unique_id.argtypes = [vp]
        L.bg_comm_init.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
        L.bg_comm_init_host.argtypes = [vp, i32, i32, C.c_char_p, C.POINTER(vp)]
        L.bg_gather_records.argtypes = [vp, vp, u64, u32, vp, vp, vp]
        L.bg_gather_records_cap.argtypes = [vp, vp, u64, u32, vp, u64, vp, vp]
        L.bg_gather_records_host.argtypes = [vp, vp, u64, u32, vp, u64, vp]
        L.bg_comm_free.argtypes = [vp]
        L.bg_comm_world.argtypes = [vp, vp]
        L.bg_fm_backward_search_batch.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
        L.bg_fm_backward_search_batch_dev.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
        L.bg_fmd_interval_batch.argtypes = [vp, u64, vp, vp, vp, vp]
        L.bg_fmd_smems_batch.argtypes = [vp, i32, u64, vp, vp, vp, u32, u32, vp, vp]
        L.bg_fmd_smems_batch_dev.argtypes = [vp, i32, u64, vp, vp, vp, u32, u32, u32, vp, vp, vp]
        L.bg_fmd_interval_batch64.argtypes = [vp, u64, vp, vp, vp, vp]
        L.bg_fmd_smems_batch64.argtypes = [vp, i32, u64, vp, vp, vp, u32, u32, vp, vp]
        L.bg_fmd_smems_batch64_dev.argtypes = [vp, i32, u64, vp, vp, vp, u32, u32, u32, vp, vp, vp]
        L.bg_fm_set_suffix_array.argtypes = [vp, vp, u64]
        L.bg_fm_set_sampled_suffix_array.argtypes = [vp, vp, u64, u32, C.c_uint8, vp, vp, u64]
        L.bg_sa_get_batch.argtypes = [vp, u64, vp, vp]
        L.bg_fastq_parse.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(i32), C.POINTER(u64)]
        L.bg_fastq_parse_dev.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(i32), C.POINTER(u64), vp]
        L.bg_fasta_parse.argtypes = [vp, vp, u64, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(i32), C.POINTER(u64)]
        L.bg_fasta_parse_dev.argtypes = [vp, vp, u64, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(i32), C.POINTER(u64), vp]
        L.bg_fasta_reference.argtypes = [vp, u64, vp, vp, vp, u32, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.bg_fasta_reference_dev.argtypes = [vp, u64, vp, vp, vp, u32, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_cigar_batch.argtypes = [vp, u64, vp, vp, u64, i32, vp, u64, vp]
        L.bg_cigar_batch_dev.argtypes = [vp, u64, vp, vp, i32, vp, u64, vp, vp]
        L.bg_sa_get_batch_dev.argtypes = [vp, u64, vp, vp, vp]
        L.bg_interval_occ_batch.argtypes = [vp, u64, vp, vp, vp, vp, u64]
        L.bg_interval_occ_batch_dev.argtypes = [vp, u64, vp, vp, u64, vp, vp]
        L.bg_align_batch.argtypes = [vp, C.POINTER(ScoringC), i32, u64, vp, vp, vp, vp, vp, vp,
                                     u64, C.POINTER(u64)]
        L.bg_align_batch_dev.argtypes = [vp, C.POINTER(ScoringC), i32, u64, vp, vp, vp, vp, u32,
                                         u32, vp, vp, u64, vp]
        L.bg_align_banded_batch.argtypes = [vp, C.POINTER(ScoringC), i32, u32, u32, u64, vp, vp,
                                            vp, vp, vp, vp, u64, C.POINTER(u64), vp]
        L.bg_align_banded_batch_dev.argtypes = [vp, C.POINTER(ScoringC), i32, u32, u32, u64, vp, vp, vp, vp, vp, vp, u64, vp, vp]
        L.bg_band_create_batch.argtypes = [C.POINTER(ScoringC), i32, u32, u32, u64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.bg_align_banded_bands_batch.argtypes = [vp, C.POINTER(ScoringC), i32, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                  u64, C.POINTER(u64), vp]
        L.bg_band_from_matches_batch.argtypes = [C.POINTER(ScoringC), i32, u32, u32, u64, vp, vp, vp, vp, vp, vp, vp, vp,
                                                 vp, vp]
        for name, args in [("bg_sparse_find_kmer_matches", [vp, u64, vp, u64, u32, vp, u64]),
                           ("bg_sparse_sdpkpp", [vp, u64, u32, u32, C.c_int32, C.c_int32, vp, u64]),
                           ("bg_sparse_lcskpp", [vp, u64, u32, vp, u64, C.POINTER(u32)]),
                           ("bg_sparse_sdpkpp_union_lcskpp_path", [vp, u64, u32, u32, C.c_int32, C.c_int32, vp, u64]),
                           ("bg_sparse_expand_kmer_matches", [vp, u64, vp, u64, u32, vp, u64, u32, vp, u64])]:
            getattr(L, name).restype = u64
            getattr(L, name).argtypes = args
        L.bg_pretty_batch.argtypes = [vp, u64, vp, vp, u64, vp, vp, vp, vp, u32, vp, u64, vp]
        L.bg_suffix_array_dev.argtypes = [vp, vp, u64, vp, vp]
        L.bg_bwt_dev.argtypes = [vp, vp, vp, u64, vp, vp]
        L.bg_sa_sample_dev.argtypes = [vp, vp, vp, u64, u32, C.c_uint8, vp, vp, vp, u64, C.POINTER(u64), vp]
        L.bg_suffix_array_dev64.argtypes = [vp, vp, u64, vp, vp]
        L.bg_bwt_dev64.argtypes = [vp, vp, vp, u64, vp, vp]
        L.bg_sa_sample_dev64.argtypes = [vp, vp, vp, u64, u32, C.c_uint8, vp, vp, vp, u64, C.POINTER(u64), vp]
        L.bg_fm_set_text.argtypes = [vp, vp, u64]
        L.bg_fm_set_text_dev.argtypes = [vp, vp, u64]
        L.bg_seed_extend_batch.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), u64, vp, vp, vp, vp, u64, C.POINTER(u64)]
        L.bg_seed_extend_batch_dev.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), u64, vp, vp, u32, vp, vp, u64, vp, vp]
        L.bg_seed_extend_strands_batch.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), u32, u64, vp, vp, vp, vp, vp, u64,
                                                   C.POINTER(u64)]
        L.bg_seed_extend_strands_batch_dev.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), u32, u64, vp, vp, u32, vp, vp,
                                                       vp, u64, vp, vp]
        L.bg_seed_extend_smem_batch.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SMEM_SEED_PARAMS), u32, u64, vp, vp, vp, vp, vp, u64,
                                                C.POINTER(u64)]
        L.bg_seed_extend_smem_batch_dev.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SMEM_SEED_PARAMS), u32, u64, vp, vp, u32, vp, vp,
                                                    vp, u64, vp, vp]
        L.bg_seed_extend_tiered_batch.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(TIERED_SEED_PARAMS), u32, u64, vp, vp, vp, vp, vp, vp,
                                                  u64, C.POINTER(u64)]
        L.bg_seed_extend_tiered_batch_dev.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(TIERED_SEED_PARAMS), u32, u64, vp, vp, u32, vp,
                                                      vp, vp, vp, u64, vp, vp]
        L.bg_seed_extend_pairs_batch.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), C.POINTER(PAIR_PARAMS), u64, vp, vp, vp,
                                                 vp, vp, vp, u64, C.POINTER(u64)]
        L.bg_seed_extend_pairs_batch_dev.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), C.POINTER(PAIR_PARAMS), u64, vp, vp,
                                                     u32, vp, vp, vp, vp, u64, vp, vp]
        L.bg_seed_extend_pairs_rescue_batch.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), C.POINTER(PAIR_PARAMS),
                                                        C.POINTER(RESCUE_PARAMS), u64, vp, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64)]
        L.bg_seed_extend_pairs_rescue_batch_dev.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), C.POINTER(PAIR_PARAMS),
                                                            C.POINTER(RESCUE_PARAMS), u64, vp, vp, u32, vp, vp, vp, vp, vp, u64, vp, vp]
        L.bg_seed_extend_multi_batch.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), C.POINTER(MULTI_PARAMS), u32, u64, vp, vp,
                                                 vp, vp, vp, vp, u64, C.POINTER(u64)]
        L.bg_seed_extend_multi_batch_dev.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), C.POINTER(MULTI_PARAMS), u32, u64, vp,
                                                     vp, u32, vp, vp, vp, vp, u64, vp, vp]
        L.bg_seed_extend_pairs_mapq_batch.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), C.POINTER(PAIR_PARAMS),
                                                      C.POINTER(PAIRQ_PARAMS), u64, vp, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64)]
        L.bg_seed_extend_pairs_mapq_batch_dev.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), C.POINTER(PAIR_PARAMS),
                                                          C.POINTER(PAIRQ_PARAMS), u64, vp, vp, u32, vp, vp, vp, vp, vp, u64, vp, vp]
        L.bg_seed_extend_pairs_rescue_mapq_batch.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), C.POINTER(PAIR_PARAMS),
                                                             C.POINTER(RESCUE_PARAMS), C.POINTER(PAIRQ_PARAMS), u64, vp, vp, vp, vp, vp,
                                                             vp, vp, vp, u64, C.POINTER(u64)]
        L.bg_seed_extend_pairs_rescue_mapq_batch_dev.argtypes = [vp, C.POINTER(ScoringC), C.POINTER(SeedParamsC), C.POINTER(PAIR_PARAMS),
                                                                 C.POINTER(RESCUE_PARAMS), C.POINTER(PAIRQ_PARAMS), u64, vp, vp, u32, vp,
                                                                 vp, vp, vp, vp, vp, u64, vp, vp]
        L.bg_revcomp_batch_dev.argtypes = [vp, u64, vp, vp, vp, vp]
        L.bg_sam_header.argtypes = [vp, u64, vp, vp, u64, C.POINTER(u64)]
        L.bg_sam_emit_batch_dev.argtypes = [vp, C.POINTER(SAM_PARAMS), u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, vp,
                                            C.POINTER(u64), vp]
        L.bg_sam_emit_batch.argtypes = [vp, C.POINTER(SAM_PARAMS), u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, vp,
                                        C.POINTER(u64)]
        L.bg_sam_markdup_dev.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp]
        L.bg_sam_markdup.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp]
        L.bg_sam_emit_dup_batch_dev.argtypes = [vp, C.POINTER(SAM_PARAMS), u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64,
                                                vp, C.POINTER(u64), vp]
        L.bg_sam_emit_dup_batch.argtypes = [vp, C.POINTER(SAM_PARAMS), u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, vp,
                                            C.POINTER(u64)]
        L.bg_sam_sort_keys_dev.argtypes = [vp, C.POINTER(SAM_PARAMS), u64, vp, u64, vp, vp, vp, vp]
        L.bg_sam_sort_keys.argtypes = [vp, C.POINTER(SAM_PARAMS), u64, vp, u64, vp, vp, vp]
        L.bg_sam_sort_dev.argtypes = [vp, u64, vp, vp, vp, u64, vp, u64, vp, vp, vp]
        L.bg_sam_sort.argtypes = [vp, u64, vp, vp, vp, u64, vp, u64, vp, vp]
        L.bg_sam_header_so.argtypes = [vp, u64, vp, i32, vp, u64, C.POINTER(u64)]
        L.bg_bam_header.argtypes = [vp, u64, vp, i32, vp, u64, C.POINTER(u64)]
        L.bg_bam_emit_batch_dev.argtypes = L.bg_sam_emit_dup_batch_dev.argtypes
        L.bg_bam_emit_batch.argtypes = L.bg_sam_emit_dup_batch.argtypes
        L.bg_bgzf_frame_dev.argtypes = [vp, vp, u64, u32, vp, u64, C.POINTER(u64), vp]
        L.bg_bgzf_frame.argtypes = [vp, vp, u64, u32, vp, u64, C.POINTER(u64)]
        L.bg_bgzf_deflate_dev.argtypes = [vp, vp, u64, u32, vp, u64, vp, C.POINTER(u64), vp]
        L.bg_bgzf_deflate.argtypes = [vp, vp, u64, u32, vp, u64, vp, C.POINTER(u64)]
        L.bg_bgzf_blocks_dev.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_bgzf_blocks.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.bg_bgzf_inflate_dev.argtypes = [vp, vp, u64, u64, vp, vp, vp, u64, vp, C.POINTER(u64), vp]
        L.bg_bgzf_inflate.argtypes = [vp, vp, u64, u64, vp, vp, vp, u64, vp, C.POINTER(u64)]
        L.bg_bam_index_dev.argtypes = [vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_bam_index.argtypes = [vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
        L.bg_bam_header_parse.argtypes = [vp, u64, vp, u64, vp, u64] + [C.POINTER(u64)] * 6
        L.bg_bam_records_dev.argtypes = [vp, vp, u64, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_bam_records.argtypes = [vp, vp, u64, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.bg_bam_reads_dev.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, u64, vp, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_bam_reads.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, u64, vp, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.bg_bam_sort_keys_dev.argtypes = [vp, u64, vp, vp, vp, u64, vp, C.POINTER(u64), vp]
        L.bg_bam_sort_keys.argtypes = [vp, u64, vp, vp, vp, u64, vp, C.POINTER(u64)]
        L.bg_bam_index_blocks_dev.argtypes = [vp, u64, vp, vp, vp, u64, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_bam_index_blocks.argtypes = [vp, u64, vp, vp, vp, u64, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
        L.bg_bam_pileup_dev.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_bam_pileup.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64)]
        L.bg_bam_sites_dev.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_bam_sites.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(u64)]
        L.bg_bam_indels_dev.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_bam_indels.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.bg_bam_indels_left_dev.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_bam_indels_left.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.bg_vcf_header.argtypes = [vp, u64, vp, vp, u64, C.POINTER(u64)]
        L.bg_vcf_emit_dev.argtypes = [vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]
        L.bg_vcf_emit.argtypes = [vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.bg_pack2_dev.argtypes = [vp, vp, u64, vp, vp, vp, vp]
        L.bg_unpack2_dev.argtypes = [vp, vp, u64, vp, vp, vp]
        L.bg_fm_pattern_codes.argtypes = [vp, vp]
        L.bg_fm_backward_search_packed_dev.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
        L.bg_fm_backward_search_count_lines_dev.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
        L.bg_align_batch_packed_dev.argtypes = [vp, C.POINTER(ScoringC), i32, u64, vp, vp, vp, vp, vp, u32, u32, vp, vp, u64, vp]
        L.bg_get_timing.argtypes = [vp, C.POINTER(TimingC)]
        L.bg_enable_timing.argtypes = [vp, i32]
        L.bg_band_redo_pairs.argtypes = [vp, C.POINTER(u64)]
        L.bg_last_fill_kernels.argtypes = [vp, C.POINTER(u32)]
        L.bg_last_fill_framed.argtypes = [vp, C.POINTER(i32)]
        L.bg_last_fill_max3.argtypes = [vp, C.POINTER(i32)]
        L.bg_pack2_host.argtypes = [vp, u64, vp, vp]
        L.bg_myers_best_batch.argtypes = [vp, vp, u32, u32, u64, vp, vp, vp, vp, u64]
        L.bg_myers_best_batch_dev.argtypes = [vp, vp, u32, u32, u64, vp, vp, vp, vp, u64, vp]
        L.bg_myers_find_all_batch.argtypes = [vp, vp, u32, u32, u32, u32, u64, vp, vp, vp, vp]
        L.bg_myers_find_all_batch_dev.argtypes = [vp, vp, u32, u32, u32, u32, u64, vp, vp, vp, vp, vp]
        L.bg_myers_long_best_batch.argtypes = [vp, vp, vp, vp, u32, u32, u64, vp, vp, vp, vp, u64]
        L.bg_myers_long_best_batch_dev.argtypes = [vp, vp, vp, vp, u32, u32, u64, vp, vp, vp, vp, u64, vp]
        L.bg_myers_long_find_all_batch.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, u64, vp, vp, vp, vp]
        L.bg_myers_long_find_all_batch_dev.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, u64, vp, vp, vp, vp, vp]
        L.bg_fastq_trim.argtypes = [vp, u64, i32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.bg_fastq_trim_dev.argtypes = [vp, u64, i32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.bg_fastq_filter.argtypes = [vp, u64, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.bg_fastq_filter_dev.argtypes = [vp, u64, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.bg_fastq_emit.argtypes = [vp, u64, u64, u64, vp, vp, vp, vp, vp, u64, vp, C.POINTER(u64)]
        L.bg_fastq_emit_dev.argtypes = [vp, u64, u64, u64, vp, vp, vp, vp, vp, u64, vp, C.POINTER(u64), vp]
        L.bg_fastq_demux_assign.argtypes = [vp, u64, vp, vp, u32, vp, vp, vp, vp]
        L.bg_fastq_demux_assign_dev.argtypes = [vp, u64, vp, vp, u32, vp, vp, vp, vp, vp]
        L.bg_fastq_demux_split.argtypes = [vp, u64, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.bg_fastq_demux_split_dev.argtypes = [vp, u64, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.bg_qc_tables_words.restype = u64
        L.bg_qc_tables_words.argtypes = [u32]
        L.bg_fastq_qual_cut.argtypes = [vp, u64, vp, vp, vp, vp, vp]
        L.bg_fastq_qual_cut_dev.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
        L.bg_fastq_qual_select.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
        L.bg_fastq_qual_select_dev.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.bg_fastq_qc_tables.argtypes = [vp, u64, u64, u64, u32, u32, vp, vp, vp, vp, vp]
        L.bg_fastq_qc_tables_dev.argtypes = [vp, u64, u64, u64, u32, u32, vp, vp, vp, vp, vp, vp]
        for s in SYMBOLS:
            if getattr(L, s).restype is C.c_int or s.startswith("bg_") and getattr(L, s).restype is None:
                pass
        _lib = L
    return _lib


class Context:
    """bg_ctx: one per device, not thread-safe (like `&mut Aligner`)."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        check(lib().bg_init(device, C.byref(self.h)), "bg_init")
        self.device = device

    def set_option(self, key, value):
        check(lib().bg_set_option(self.h, key.encode(), int(value)), "bg_set_option")

    def enable_timing(self, on=True):
        check(lib().bg_enable_timing(self.h, 1 if on else 0))

    def timing(self):
        t = TimingC()
        check(lib().bg_get_timing(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in TimingC._fields_}

    def band_redo_pairs(self):
        """pairs of the last banded call that the packed fill flagged and the int32 kernels recomputed"""
        v = C.c_uint64(0)
        check(lib().bg_band_redo_pairs(self.h, C.byref(v)))
        return int(v.value)

    def last_fill_kernels(self):
        """BG_FILL_* bits (FILL) of the fill kernel families the last align call on this ctx launched"""
        v = C.c_uint32(0)
        check(lib().bg_last_fill_kernels(self.h, C.byref(v)))
        return int(v.value)

    def last_fill_framed(self):
        """True when the last align call ran K1p's LF flavour with its keys in the offset frame (FILL["K1P_LF"] either way)"""
        v = C.c_int(0)
        check(lib().bg_last_fill_framed(self.h, C.byref(v)))
        return bool(v.value)

    def last_fill_max3(self):
        """True when that framed cell took its best key with v_pk_maximum3_f16 (every key below 0x7c00; option no_pk16_max3)"""
        v = C.c_int(0)
        check(lib().bg_last_fill_max3(self.h, C.byref(v)))
        return bool(v.value)

    def close(self):
        if self.h:
            lib().bg_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=None):
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if lib().bg_device_count() > 1 else 0
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def as_u8(b):
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8)


# The five FASTQ columns (recs, seq, seq_off, qual, qual_off) of myers.trim, fastq.filter_arrays and fastq.demux_split_arrays
# and of their *_dev twins.  `rec_slots`: the records the output record column is allocated for; the callers differ in it
# (n, or max(1, n) where the call refuses a null record column).
def fq_columns(recs, seq, seq_off, qual, qual_off):
    """the five host columns, contiguous and of the dtypes the C ABI reads"""
    return (np.ascontiguousarray(recs, dtype=FQREC_DTYPE), as_u8(seq), np.ascontiguousarray(seq_off, dtype=np.uint64), as_u8(qual),
            np.ascontiguousarray(qual_off, dtype=np.uint64))


def fq_host_outputs(n, rec_slots, seq, qual):
    """host output columns for n records of at most the bytes of `seq` and `qual`"""
    return (np.zeros(rec_slots, dtype=FQREC_DTYPE), np.zeros(max(1, len(seq)), dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64),
            np.zeros(max(1, len(qual)), dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64))


def fq_dev_outputs(n, rec_slots, d_seq, d_qual):
    """device output columns (torch) for n records of at most the bytes of d_seq and d_qual, on their device"""
    import torch
    dev = d_seq.device
    return (torch.empty(rec_slots * 56, dtype=torch.uint8, device=dev), torch.empty(max(1, int(d_seq.numel())), dtype=torch.uint8, device=dev),
            torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(max(1, int(d_qual.numel())), dtype=torch.uint8, device=dev),
            torch.empty(n + 1, dtype=torch.int64, device=dev))


def concat(seqs):
    """list of bytes -> (uint8 buffer, uint64 offsets[n+1])"""
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(bytes(s) for s in seqs), dtype=np.uint8)
    return buf, off
