"""Python host mirror of the C ABI (include/strling_amd.h) via ctypes.

This is plumbing for tests, bench.py and scripting: every compute call goes through
libstrling_amd.so into the HIP kernels.  There is no CPU fallback -- if the library is missing or
no HIP device is present the calls raise.
"""
import ctypes as C
import os
import numpy as np

from . import build as _build
from .records import RecordBatch, GenomeStr

_LIB = None


class StrlingError(RuntimeError):
    pass


class Opts(C.Structure):
    _fields_ = [("median_fragment_length", C.c_int32), ("proportion_repeat", C.c_double), ("min_mapq", C.c_uint8)]


class CGenomeStr(C.Structure):
    _fields_ = [("n_tid", C.c_int32), ("has_chrom", C.c_void_p), ("iv_off", C.c_void_p), ("iv_start", C.c_void_p),
                ("iv_stop", C.c_void_p)]


class CRecords(C.Structure):
    _fields_ = [("n", C.c_int64), ("tid", C.c_void_p), ("pos", C.c_void_p), ("mtid", C.c_void_p), ("mpos", C.c_void_p),
                ("flag", C.c_void_p), ("mapq", C.c_void_p), ("cigar_off", C.c_void_p), ("cigar", C.c_void_p),
                ("seq_off", C.c_void_p), ("l_seq", C.c_void_p), ("seq4", C.c_void_p), ("qname_off", C.c_void_p),
                ("qnames", C.c_void_p)]


class CReadSoa(C.Structure):
    _fields_ = [("n", C.c_uint64), ("tid", C.c_void_p), ("pos", C.c_void_p), ("end", C.c_void_p), ("seq_off", C.c_void_p),
                ("l_seq", C.c_void_p), ("clip_l", C.c_void_p), ("clip_r", C.c_void_p), ("mapq", C.c_void_p),
                ("cig", C.c_void_p), ("seq4", C.c_void_p), ("seq4_bytes", C.c_uint64), ("max_l_seq", C.c_uint32),
                ("mem", C.c_int32), ("meta", C.c_void_p)]


class CPairSoa(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("qhash", C.c_void_p)]


PAIR_REC_DTYPE = np.dtype([("tid", "<i4"), ("pos", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("end", "<i4"), ("flag", "<u2"), ("l_seq", "<u2"),
                           ("clip_l", "<u2"), ("clip_r", "<u2"), ("mapq", "u1"), ("cig", "u1"), ("pad", "<u2")])
assert PAIR_REC_DTYPE.itemsize == 32


class FrontChunk(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_primary", C.c_uint64), ("last_placed", C.c_int64), ("tail_primary", C.c_uint64),
                ("max_l_seq", C.c_uint32), ("scan_slow_segments", C.c_uint32)]


class BamindexInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_no_coor", C.c_uint64), ("n_runs", C.c_uint64), ("n_chunks", C.c_uint64)]


class BamsortInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_no_ref", C.c_uint64), ("stream_bytes", C.c_uint64), ("already_sorted", C.c_uint32), ("n_slabs", C.c_uint32),
                ("arena_bytes", C.c_uint64), ("sort_ms", C.c_double), ("layout_ms", C.c_double), ("gather_ms", C.c_double)]


class MarkdupInfo(C.Structure):
    """strl_markdup_info: the counts of `sort --markdup` and the HIP-event time of the device step's parts"""
    _fields_ = [("n_pairs", C.c_uint64), ("n_dup_pairs", C.c_uint64), ("n_fragments", C.c_uint64), ("n_dup_fragments", C.c_uint64), ("n_ineligible", C.c_uint64),
                ("record_ms", C.c_double), ("join_ms", C.c_double), ("pairs_ms", C.c_double), ("fragments_ms", C.c_double), ("flag_ms", C.c_double)]


class FastqOpts(C.Structure):
    """strl_fastq_opts: -F, -N, -v, interleaved (-o) or split (-1 -2), and whether the singles' stream is laid out (-s)"""
    _fields_ = [("filter", C.c_uint32), ("suffix", C.c_uint32), ("default_qual", C.c_uint32), ("interleaved", C.c_uint32), ("singles", C.c_uint32)]


class FastqInfo(C.Structure):
    """strl_fastq_info: the six counts of `strling fastq`, the three streams' lengths and the HIP-event time of the device step's parts"""
    _fields_ = [("n_kept", C.c_uint64), ("n_filtered", C.c_uint64), ("n_empty", C.c_uint64), ("n_pairs", C.c_uint64), ("n_singles", C.c_uint64), ("n_singles_unwritten", C.c_uint64),
                ("stream_bytes", C.c_uint64 * 3), ("text_bytes", C.c_uint64), ("record_ms", C.c_double), ("join_ms", C.c_double), ("layout_ms", C.c_double), ("text_ms", C.c_double)]


class ViewOpts(C.Structure):
    """strl_view_opts: -f, -F, -G, -q and a region (tid = -2: none)"""
    _fields_ = [("require", C.c_uint32), ("exclude", C.c_uint32), ("exclude_all", C.c_uint32), ("min_mapq", C.c_uint32), ("tid", C.c_int32), ("beg", C.c_int32), ("end", C.c_int32)]


class ViewInfo(C.Structure):
    """strl_view_info: the counts of `strling view`, the chunks and the HIP-event time of the two kernels"""
    _fields_ = [("records", C.c_uint64), ("written", C.c_uint64), ("dropped", C.c_uint64), ("text_bytes", C.c_uint64), ("chunks", C.c_uint64), ("host_chunks", C.c_uint64),
                ("size_ms", C.c_double), ("text_ms", C.c_double)]


def _view_opts(require=0, exclude=0, exclude_all=0, min_mapq=0, tid=-2, beg=0, end=0):
    return ViewOpts(int(require), int(exclude), int(exclude_all), int(min_mapq), int(tid), int(beg), int(end))


def _view_info(info):
    return {k: getattr(info, k) for k, _ in ViewInfo._fields_}


def _fastq_opts(filter=0x900, suffix=False, default_qual=1, interleaved=True, singles=False):
    return FastqOpts(int(filter), int(bool(suffix)), int(default_qual), int(bool(interleaved)), int(bool(singles)))


def _fastq_info(info):
    d = {k: getattr(info, k) for k, _ in FastqInfo._fields_ if k != "stream_bytes"}
    d["stream_bytes"] = [int(x) for x in info.stream_bytes]
    return d


class BamsortSamFigures(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("text_bytes", C.c_uint64), ("host_finished", C.c_uint64), ("chunks", C.c_uint64),
                ("copy_ms", C.c_double), ("scan_ms", C.c_double), ("size_ms", C.c_double), ("encode_ms", C.c_double)]


class SweepInfo(C.Structure):
    _fields_ = [("n_answered", C.c_uint64), ("n_seam", C.c_uint64), ("n_passed_on", C.c_uint64), ("n_chunks", C.c_uint64), ("n_records", C.c_uint64),
                ("sweep_ms", C.c_double), ("evidence_ms", C.c_double)]


def _front_chunk(c):
    return {k: int(getattr(c, k)) for k, _ in FrontChunk._fields_}


class ScoreStats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_skipped", C.c_uint64), ("n_scored", C.c_uint64), ("n_soft_items", C.c_uint64),
                ("ms_classify", C.c_float), ("ms_score", C.c_float), ("ms_soft", C.c_float), ("n_stage_b_whole", C.c_uint32),
                ("n_stage_b_soft", C.c_uint32)]


class ClusterStats(C.Structure):
    _fields_ = [("n_treads", C.c_uint64), ("n_groups", C.c_uint64), ("n_clusters", C.c_uint64), ("n_bounds", C.c_uint64),
                ("n_tie_fixups", C.c_uint64), ("ms_sort", C.c_float), ("ms_sweep", C.c_float), ("ms_bounds", C.c_float)]


class AssignInfo(C.Structure):
    _fields_ = [("n_loci", C.c_uint64), ("n_groups", C.c_uint64), ("n_assigned", C.c_uint64), ("n_lost", C.c_uint64), ("seconds", C.c_double)]


class BinInfo(C.Structure):
    _fields_ = [("proportion_repeat", C.c_float), ("min_mapq", C.c_uint8), ("frag", C.c_uint32 * 4096),
                ("header_len", C.c_int32), ("n_reads", C.c_int32), ("qnames_bytes", C.c_uint64)]


SOFT_DTYPE = np.dtype([("read_side", "<u4"), ("res_first", "<u4"), ("res_after", "<u4"), ("seg_len", "<u4")])
TREAD_DTYPE = np.dtype([("tid", "<i4"), ("position", "<u4"), ("repeat", "S6"), ("flag", "<u2"), ("split", "u1"),
                        ("mapping_quality", "u1"), ("repeat_count", "u1"), ("align_length", "u1"), ("qname_id", "<i8")],
                       align=True)
REGION_REQ_DTYPE = np.dtype([("first_block", "<u4"), ("n_blocks", "<u4"), ("in_block", "<u4"), ("tid", "<i4"), ("beg", "<i4"), ("end", "<i4")])
# `strling pull` (strl_pull_row / strl_pull_tile / strl_pull_req of include/strling_amd.h)
PULL_ROW_DTYPE = np.dtype([("off", "<u8"), ("tid", "<i4"), ("pos", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("size", "<u4"), ("hash", "<u4"), ("flag", "<u2"),
                           ("l_name", "u1"), ("found", "u1"), ("count", "<u4")])
PULL_TILE_DTYPE = np.dtype([("tid", "<i4"), ("beg", "<i4"), ("end", "<i4"), ("own_beg", "<i4"), ("own_end", "<i4")])
PULL_REQ_DTYPE = np.dtype([("hash", "<u4"), ("beg", "<i4"), ("end", "<i4"), ("name_off", "<u4"), ("flag", "<u2"), ("name_len", "u1"), ("pad", "u1")])
BOUNDS_DTYPE = np.dtype([("tid", "<i4"), ("left", "<u4"), ("left_most", "<u4"), ("right", "<u4"), ("right_most", "<u4"),
                         ("center_mass", "<u4"), ("n_left", "<u2"), ("n_right", "<u2"), ("n_total", "<u2"),
                         ("repeat", "S7")], align=True)
UNPLACED_DTYPE = np.dtype([("repeat", "S7"), ("count", "<i8")], align=True)
assert TREAD_DTYPE.itemsize == 32 and BOUNDS_DTYPE.itemsize == 40 and UNPLACED_DTYPE.itemsize == 16

SUPPORT_DTYPE = np.dtype([("type", "u1"), ("repeat_count", "u1"), ("cigar_ins", "u1"), ("cigar_del", "u1"), ("fragment_length", "<u4"),
                          ("fragment_percentile", "<f8"), ("rec", "<i8")], align=True)
CALL_DTYPE = np.dtype([("tid", "<i4"), ("start", "<u4"), ("stop", "<u4"), ("repeat", "S7"), ("allele1", "<f8"), ("allele2", "<f8"),
                       ("overlapping_reads", "<u4"), ("anchored_reads", "<u4"), ("spanning_reads", "<u4"), ("spanning_pairs", "<u4"),
                       ("left_clips", "<u4"), ("right_clips", "<u4"), ("sum_str_counts", "<u4"), ("expected_spanning_fragments", "<f4"),
                       ("spanning_fragments_oe_percentile", "<f4"), ("unplaced_reads", "<i4"), ("depth", "<f8"), ("is_large", "<i4")],
                      align=True)
assert SUPPORT_DTYPE.itemsize == 24 and CALL_DTYPE.itemsize == 96, (SUPPORT_DTYPE.itemsize, CALL_DTYPE.itemsize)
SUPPORT_TYPES = ["SpanningFragment", "SpanningRead", "OverlappingRead"]


SPAN_SUMMARY_DTYPE = np.dtype([("median_depth", "<i4"), ("expected_spanners", "<f4"), ("n_support", "<u8")], align=True)
assert SPAN_SUMMARY_DTYPE.itemsize == 16


class SpanSummary(C.Structure):
    _fields_ = [("median_depth", C.c_int32), ("expected_spanners", C.c_float), ("n_support", C.c_uint64)]


class CallOpts(C.Structure):
    _fields_ = [("median_fragment_length", C.c_int32), ("min_support", C.c_int32), ("min_clip", C.c_uint16), ("min_clip_total", C.c_uint16)]


LOCUS_DTYPE = np.dtype([("b", BOUNDS_DTYPE), ("name", "S128")], align=True)
assert LOCUS_DTYPE.itemsize == 168, LOCUS_DTYPE.itemsize
SOFT_TAKEN = 255
MEM_HOST, MEM_DEVICE = 0, 1
MODE_MERGE, MODE_CALL = 0, 1

# every symbol include/strling_amd.h declares
EXPORTS = ["strl_dev_alloc", "strl_dev_free", "strl_copy", "strl_outliers_row_medians", "strl_outliers_huber", "strl_outliers_scores",
           "strl_outliers_order", "strl_version", "strl_last_error", "strl_device_count", "strl_ctx_create", "strl_ctx_destroy", "strl_ctx_stream",
           "strl_ctx_sync", "strl_ctx_set_opts", "strl_ctx_set_genome", "strl_soa_from_records", "strl_score_reads", "strl_index_chrom", "strl_index_regions",
           "strl_ctx_enable_timing", "strl_ctx_kernel_times", "strl_ctx_kernel_times_detail", "strl_pair_reads", "strl_pairer_create", "strl_pairer_destroy", "strl_pairer_add",
           "strl_pairer_result", "strl_qname_hash", "strl_extract", "strl_cluster", "strl_cluster_replay", "strl_frag_median",
           "strl_bin_write", "strl_bin_read", "strl_bounds_row", "strl_cluster_members", "strl_spanners", "strl_genotype",
           "strl_calls_finish", "strl_unplaced_order", "strl_call_row", "strl_canonical_repeat", "strl_assign_reads_loci", "strl_assign_reads_loci_device", "strl_assign_info_last", "strl_group_order",
           "strl_extract_device", "strl_treads_fetch", "strl_ctx_pair_times", "strl_sort_pairs", "strl_cluster_resident", "strl_ctx_cluster_times", "strl_pair_rows", "strl_extract_begin", "strl_extract_add", "strl_extract_finish", "strl_pair_rule", "strl_bounds_bare", "strl_ctx_treads_device", "strl_cluster_gathered", "strl_inflate_blocks", "strl_ctx_inflate_ms", "strl_regions_fetch", "strl_evidence_records", "strl_regions_evidence", "strl_front_begin", "strl_front_push", "strl_front_push_after", "strl_front_reserve", "strl_front_stage", "strl_front_enqueue_after", "strl_front_collect", "strl_ctxs_extract_gather", "strl_front_finish", "strl_front_fragwords", "strl_front_fragwords_async", "strl_event_wait", "strl_front_records", "strl_front_tids", "strl_front_qnames", "strl_front_treads_named", "strl_pinned_alloc", "strl_pinned_free", "strl_comm_unique_id", "strl_ctx_comm_init", "strl_ctxs_comm_init", "strl_ctx_comm_info", "strl_cluster_exchange", "strl_ctxs_cluster_exchange", "strl_exchange_treads", "strl_ctx_set_treads", "strl_cluster_collect", "strl_ctx_tail_stream", "strl_ctx_mem_info", "strl_bin_peek", "strl_front_trim_next", "strl_front_tail_bytes", "strl_ctx_blocking_waits", "strl_score_read_host", "strl_front_end",
           "strl_bamindex_begin", "strl_bamindex_reserve", "strl_bamindex_push", "strl_bamindex_finish", "strl_bamindex_fetch", "strl_bamindex_end",
           "strl_front_index_begin", "strl_front_index_blocks", "strl_front_index_finish", "strl_bamindex_begin_csi", "strl_front_index_begin_csi",
           "strl_sweep_begin", "strl_sweep_reserve", "strl_sweep_push", "strl_sweep_finish", "strl_sweep_end",
           "strl_pull_select", "strl_pull_mates", "strl_pull_select_host", "strl_pull_counts_host", "strl_pull_mates_host", "strl_pull_order",
           "strl_bgzf_deflate", "strl_bgzf_deflate_bound", "strl_bgzf_deflate_host", "strl_ctx_deflate_ms", "strl_bgzf_deflate_mode", "strl_bgzf_deflate_host_mode",
           "strl_bamsort_deflate_mode",
           "strl_bamsort_begin", "strl_bamsort_reserve", "strl_bamsort_push", "strl_bamsort_finish", "strl_bamsort_fetch", "strl_bamsort_fetch_bgzf", "strl_bamsort_order",
           "strl_bamsort_info_now", "strl_bamsort_end", "strl_bamsort_key", "strl_bamsort_key_bits", "strl_bamsort_header",
           "strl_bamsort_index", "strl_bamsort_index_fetch", "strl_bamsort_voff", "strl_bamsort_members",
           "strl_bamsort_begin_windowed", "strl_bamsort_window_limit", "strl_bamsort_window_begin", "strl_bamsort_window_push", "strl_bamsort_window_end",
           "strl_bamsort_window_plan",
           "strl_bamsort_sam_begin", "strl_bamsort_sam_reserve", "strl_bamsort_push_sam", "strl_bamsort_sam_info", "strl_sam_encode", "strl_sam_header",
           "strl_bamsort_markdup_mode", "strl_bamsort_markdup", "strl_markdup_host",
           "strl_bamsort_fastq_mode", "strl_bamsort_fastq", "strl_bamsort_fastq_fetch", "strl_bamsort_fastq_info_now", "strl_fastq_host",
           "strl_view_begin", "strl_view_reserve", "strl_view_push", "strl_view_finish", "strl_view_end", "strl_view_records", "strl_view_host", "strl_view_records_at", "strl_view_count_only"]


def lib_path():
    return _build.LIB


def load(build_if_missing=True):
    """dlopen the in-tree library (building it with hipcc when missing). Raises when impossible."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.environ.get("STRL_LIB", _build.LIB)   # STRL_LIB: A/B a differently built copy of the same library
    if not os.path.exists(path):
        if not build_if_missing:
            raise StrlingError(f"{path} is missing: build it with `python -m strling_amd.build` (no CPU fallback)")
        _build.build()
    L = C.CDLL(path)
    L.strl_last_error.restype = C.c_char_p
    L.strl_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.strl_ctx_destroy.argtypes = [C.c_void_p]
    L.strl_ctx_stream.argtypes = [C.c_void_p]
    L.strl_ctx_stream.restype = C.c_void_p
    L.strl_ctx_sync.argtypes = [C.c_void_p]
    L.strl_ctx_set_opts.argtypes = [C.c_void_p, C.POINTER(Opts)]
    L.strl_ctx_set_genome.argtypes = [C.c_void_p, C.POINTER(CGenomeStr)]
    L.strl_ctx_enable_timing.argtypes = [C.c_void_p, C.c_int]
    L.strl_ctx_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_double * 3), C.POINTER(C.c_uint64)]
    L.strl_ctx_kernel_times_detail.argtypes = [C.c_void_p, C.POINTER(C.c_double * 8), C.POINTER(C.c_uint64)]
    L.strl_soa_from_records.argtypes = [C.POINTER(CRecords)] + [C.c_void_p] * 6 + [C.POINTER(C.c_uint32)]
    L.strl_score_reads.argtypes = [C.c_void_p, C.POINTER(CReadSoa), C.c_void_p, C.c_void_p, C.c_uint64,
                                   C.POINTER(C.c_uint64), C.POINTER(ScoreStats)]
    L.strl_index_chrom.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
    L.strl_index_regions.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                     C.POINTER(C.c_uint64)]
    L.strl_pair_reads.argtypes = [C.POINTER(CRecords), C.POINTER(Opts), C.c_void_p, C.c_void_p, C.c_uint64, C.c_int64,
                                  C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.strl_qname_hash.argtypes = [C.POINTER(CRecords), C.c_void_p]
    L.strl_extract.argtypes = [C.c_void_p, C.POINTER(CRecords), C.c_int64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                               C.POINTER(ScoreStats)]
    L.strl_cluster.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_int32, C.c_uint16, C.c_uint16,
                               C.c_uint16, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64,
                               C.POINTER(C.c_uint64), C.POINTER(ClusterStats)]
    L.strl_cluster_replay.argtypes = [C.c_void_p]
    L.strl_frag_median.argtypes = [C.c_void_p, C.c_double]
    L.strl_bin_write.argtypes = [C.c_char_p, C.c_float, C.c_uint8, C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_uint64,
                                 C.c_void_p, C.c_char_p]
    L.strl_bin_read.argtypes = [C.c_char_p, C.POINTER(BinInfo), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.strl_bounds_row.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_char_p]
    L.strl_cluster_members.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.strl_spanners.argtypes = [C.POINTER(CRecords), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint8, C.c_void_p, C.c_uint64,
                                C.POINTER(SpanSummary)]
    L.strl_genotype.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(CallOpts),
                                C.c_double, C.c_void_p]
    L.strl_calls_finish.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    L.strl_unplaced_order.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    L.strl_call_row.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_char_p]
    L.strl_score_read_host.argtypes = [C.c_char_p, C.c_int32, C.c_double, C.POINTER(C.c_uint32)]
    L.strl_canonical_repeat.argtypes = [C.c_char_p, C.c_char_p]
    L.strl_canonical_repeat.restype = None
    L.strl_group_order.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.strl_assign_reads_loci.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_assign_reads_loci_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_assign_info_last.argtypes = [C.c_void_p, C.POINTER(AssignInfo)]
    L.strl_extract_device.argtypes = [C.c_void_p, C.POINTER(CReadSoa), C.POINTER(CPairSoa), C.c_int64, C.c_uint64, C.c_uint64]
    L.strl_treads_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(ScoreStats)]
    L.strl_ctx_pair_times.argtypes = [C.c_void_p, C.POINTER(C.c_double * 5)]
    if hasattr(L, "strl_score_queue_probe"):     # (likewise)
        L.strl_score_queue_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    if hasattr(L, "strl_pair_items_probe"):      # (STRL_LIB may name a build from before the entry point)
        L.strl_pair_items_probe.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.strl_cluster_resident.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int, C.c_uint32, C.c_int32, C.c_uint16, C.c_uint16, C.c_uint16,
                                        C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                        C.POINTER(ClusterStats)]
    L.strl_ctx_set_treads.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_ctx_tail_stream.argtypes = [C.c_void_p]
    L.strl_ctx_tail_stream.restype = C.c_void_p
    L.strl_cluster_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                       C.POINTER(ClusterStats)]
    L.strl_extract_begin.argtypes = [C.c_void_p, C.c_uint64]
    L.strl_extract_add.argtypes = [C.c_void_p, C.POINTER(CReadSoa), C.POINTER(CPairSoa)]
    L.strl_extract_finish.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64]
    L.strl_pair_rule.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Opts), C.c_uint32, C.POINTER(C.c_int)]
    L.strl_pair_rules_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Opts), C.c_void_p]
    L.strl_bounds_bare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint16, C.c_uint16, C.c_uint16, C.c_void_p, C.POINTER(C.c_int)]
    L.strl_ctx_treads_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)]
    L.strl_cluster_gathered.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int32, C.c_int, C.c_uint32,
                                        C.c_int32, C.c_uint16, C.c_uint16, C.c_uint16, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p,
                                        C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(ClusterStats)]
    L.strl_inflate_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    L.strl_ctx_inflate_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.strl_bgzf_deflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint32)]
    L.strl_bgzf_deflate_host.argtypes = L.strl_bgzf_deflate.argtypes[1:]
    L.strl_bgzf_deflate_mode.argtypes = [C.c_void_p, C.c_int] + L.strl_bgzf_deflate.argtypes[1:]
    L.strl_bgzf_deflate_host_mode.argtypes = [C.c_int] + L.strl_bgzf_deflate.argtypes[1:]
    L.strl_bamsort_deflate_mode.argtypes = [C.c_void_p, C.c_int]
    L.strl_bgzf_deflate_bound.argtypes = [C.c_uint64, C.c_uint32]
    L.strl_bgzf_deflate_bound.restype = C.c_uint64
    L.strl_ctx_deflate_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.strl_regions_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                     C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.strl_evidence_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint8, C.c_void_p,
                                        C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.strl_regions_evidence.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_uint32, C.c_int32, C.c_void_p, C.c_uint8, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_double)]
    L.strl_pull_select.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                   C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p,
                                   C.POINTER(C.c_double)]
    L.strl_pull_mates.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_double)]
    L.strl_pull_select_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.strl_pull_counts_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_pull_mates_host.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.strl_pull_order.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    L.strl_front_begin.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64]
    L.strl_front_push.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_int)]
    L.strl_front_finish.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.strl_front_trim_next.argtypes = [C.c_void_p, C.c_uint32]
    L.strl_front_tail_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.strl_ctx_blocking_waits.argtypes = [C.c_void_p, C.c_int]
    L.strl_ctxs_extract_gather.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_front_fragwords.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.strl_front_tids.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.strl_front_qnames.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.strl_bamindex_begin.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64]
    L.strl_bamindex_reserve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    L.strl_bamindex_push.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
    L.strl_bamindex_finish.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(BamindexInfo)]
    L.strl_bamindex_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_bamindex_end.argtypes = [C.c_void_p]
    L.strl_bamsort_begin.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64]
    L.strl_bamsort_reserve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    L.strl_bamsort_push.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.strl_bamsort_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BamsortInfo)]
    L.strl_bamsort_fetch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.strl_bamsort_fetch_bgzf.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.strl_bamsort_order.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_bamsort_info_now.argtypes = [C.c_void_p, C.POINTER(BamsortInfo)]
    L.strl_bamsort_end.argtypes = [C.c_void_p]
    L.strl_bamsort_key.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)]
    L.strl_bamsort_key_bits.argtypes = [C.c_int32]
    L.strl_bamsort_header.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.strl_bamsort_index.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(BamindexInfo)]
    L.strl_bamsort_index_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_bamsort_voff.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.strl_bamsort_members.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.strl_bamsort_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_bamsort_begin_windowed.argtypes = [C.c_void_p, C.c_int32, C.c_uint64]
    L.strl_bamsort_window_limit.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.strl_bamsort_window_begin.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.strl_bamsort_window_push.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.strl_bamsort_window_end.argtypes = [C.c_void_p]
    L.strl_bamsort_window_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.strl_bamsort_sam_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64]
    L.strl_bamsort_sam_reserve.argtypes = [C.c_void_p, C.c_uint64]
    L.strl_bamsort_push_sam.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_bamsort_sam_info.argtypes = [C.c_void_p, C.POINTER(BamsortSamFigures)]
    L.strl_bamsort_markdup_mode.argtypes = [C.c_void_p, C.c_int]
    L.strl_bamsort_markdup.argtypes = [C.c_void_p, C.POINTER(MarkdupInfo)]
    L.strl_markdup_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(MarkdupInfo)]
    L.strl_bamsort_fastq_mode.argtypes = [C.c_void_p, C.c_int]
    L.strl_bamsort_fastq.argtypes = [C.c_void_p, C.POINTER(FastqOpts), C.POINTER(FastqInfo)]
    L.strl_bamsort_fastq_fetch.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    L.strl_bamsort_fastq_info_now.argtypes = [C.c_void_p, C.POINTER(FastqInfo)]
    L.strl_fastq_host.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(FastqOpts), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(FastqInfo)]
    L.strl_sam_encode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.strl_sam_header.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    L.strl_bamsort_window_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.strl_sweep_begin.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint8]
    L.strl_sweep_reserve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    L.strl_view_begin.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(ViewOpts)]
    L.strl_view_reserve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    L.strl_view_push.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.strl_view_finish.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(ViewInfo)]
    L.strl_view_end.argtypes = [C.c_void_p]
    L.strl_view_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(ViewOpts), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(ViewInfo)]
    L.strl_view_records_at.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(ViewOpts), C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(ViewInfo)]
    L.strl_view_count_only.argtypes = [C.c_void_p, C.c_int]
    L.strl_view_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(ViewOpts), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(ViewInfo)]
    L.strl_sweep_push.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
    L.strl_sweep_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SweepInfo)]
    L.strl_sweep_end.argtypes = [C.c_void_p]
    L.strl_front_index_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.strl_bamindex_begin_csi.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32]
    L.strl_front_index_begin_csi.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32]
    L.strl_front_index_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
    L.strl_front_index_finish.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(BamindexInfo)]
    L.strl_pinned_alloc.argtypes = [C.c_uint64]
    L.strl_pinned_alloc.restype = C.c_void_p
    L.strl_pinned_free.argtypes = [C.c_void_p]
    L.strl_comm_unique_id.argtypes = [C.c_void_p]
    L.strl_ctx_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.strl_ctxs_comm_init.argtypes = [C.c_void_p, C.c_int]
    L.strl_ctx_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.strl_cluster_exchange.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int32, C.c_int, C.c_uint32, C.c_int32, C.c_uint16, C.c_uint16, C.c_uint16,
                                        C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(ClusterStats)]
    L.strl_ctxs_cluster_exchange.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_int32, C.c_int, C.c_uint32, C.c_int32, C.c_uint16, C.c_uint16, C.c_uint16]
    L.strl_exchange_treads.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.strl_pair_rows.argtypes = [C.POINTER(CRecords)] + [C.c_void_p] * 5
    L.strl_ctx_cluster_times.argtypes = [C.c_void_p, C.POINTER(C.c_double * 3)]
    L.strl_sort_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int]
    L.strl_sort_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_int,
                                  C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint64)]
    L.strl_outliers_row_medians.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int]
    L.strl_outliers_huber.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.strl_outliers_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.strl_outliers_order.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int]
    _LIB = L
    return L


REGION_DTYPE = np.dtype([("start", "<u8"), ("stop", "<u8"), ("unit", "S8")])


def index_regions(seq, words, window=100, step=60):
    """host half of strling index: merge + trim the scored windows (strl_index_regions)"""
    L = load()
    words = np.ascontiguousarray(words, np.uint32)
    cap = len(words) + 1
    out = np.zeros(cap, REGION_DTYPE)
    n = C.c_uint64(0)
    _check(L.strl_index_regions(seq, len(seq), words.ctypes.data, len(words), window, step, out.ctypes.data, cap, C.byref(n)))
    return [(int(r["start"]), int(r["stop"]), r["unit"].decode()) for r in out[:n.value]]


def _check(rc):
    if rc != 0:
        e = StrlingError(f"strling_amd error {rc}: {load().strl_last_error().decode()}")
        e.code = rc
        raise e


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class _RecView:
    def __init__(self, rec: RecordBatch):
        k = dict(tid=np.ascontiguousarray(rec.tid, np.int32), pos=np.ascontiguousarray(rec.pos, np.int32),
                 mtid=np.ascontiguousarray(rec.mtid, np.int32), mpos=np.ascontiguousarray(rec.mpos, np.int32),
                 flag=np.ascontiguousarray(rec.flag, np.uint16), mapq=np.ascontiguousarray(rec.mapq, np.uint8),
                 cigar_off=np.ascontiguousarray(rec.cigar_off, np.uint32),
                 cigar=np.ascontiguousarray(np.append(rec.cigar, 0), np.uint32),
                 seq_off=np.ascontiguousarray(rec.seq_off, np.uint64), l_seq=np.ascontiguousarray(rec.l_seq, np.int32),
                 seq4=np.ascontiguousarray(rec.seq4, np.uint8), qname_off=np.ascontiguousarray(rec.qname_off, np.uint64),
                 qnames=np.frombuffer(bytes(rec.qnames) + b"\0", dtype=np.uint8))
        self.keep = k
        self.n = int(k["tid"].size)
        self.c = CRecords(self.n, *[k[f].ctypes.data for f in ("tid", "pos", "mtid", "mpos", "flag", "mapq", "cigar_off",
                                                               "cigar", "seq_off", "l_seq", "seq4", "qname_off", "qnames")])


class Soa:
    """Host numpy SoA batch (the layout the kernels consume)."""

    def __init__(self, rec: RecordBatch):
        L = load()
        rv = _RecView(rec)
        n = rv.n
        self.rv = rv
        self.n = n
        self.end = np.zeros(n, np.int32)
        self.seq_off = np.zeros(n, np.uint32)
        self.l_seq = np.zeros(n, np.uint16)
        self.clip_l = np.zeros(n, np.uint16)
        self.clip_r = np.zeros(n, np.uint16)
        self.cig = np.zeros(n, np.uint8)
        mx = C.c_uint32(0)
        _check(L.strl_soa_from_records(C.byref(rv.c), self.end.ctypes.data, self.seq_off.ctypes.data, self.l_seq.ctypes.data,
                                       self.clip_l.ctypes.data, self.clip_r.ctypes.data, self.cig.ctypes.data, C.byref(mx)))
        self.max_l_seq = mx.value
        self.tid, self.pos, self.mapq, self.seq4 = rv.keep["tid"], rv.keep["pos"], rv.keep["mapq"], rv.keep["seq4"]

    def pair_rows(self):
        """the 32-byte rows + qname hashes the pair logic reads (strl_pair_rows, strl_qname_hash) -> (rows, qhash)"""
        rows = np.zeros(max(self.n, 1), PAIR_REC_DTYPE)
        _check(load().strl_pair_rows(C.byref(self.rv.c), _ptr(self.end), _ptr(self.clip_l), _ptr(self.clip_r), _ptr(self.cig), rows.ctypes.data))
        qh = np.zeros(max(self.n, 1), np.uint64)
        _check(load().strl_qname_hash(C.byref(self.rv.c), qh.ctypes.data))
        return rows[:self.n], qh[:self.n]

    def meta_rows(self):
        """strl_read_meta rows (16 B per read: seq_off | l_seq, clip_l | clip_r, cig, mapq | pad) for strl_read_soa.meta"""
        m = np.zeros((max(self.n, 1), 4), np.uint32)
        m[:self.n, 0] = self.seq_off
        m[:self.n, 1] = self.l_seq.astype(np.uint32) | (self.clip_l.astype(np.uint32) << 16)
        m[:self.n, 2] = self.clip_r.astype(np.uint32) | (self.cig.astype(np.uint32) << 16) | (self.mapq.astype(np.uint32) << 24)
        return m[:self.n]

    def c_struct(self):
        return CReadSoa(self.n, _ptr(self.tid), _ptr(self.pos), _ptr(self.end), _ptr(self.seq_off), _ptr(self.l_seq),
                        _ptr(self.clip_l), _ptr(self.clip_r), _ptr(self.mapq), _ptr(self.cig), self.seq4.ctypes.data,
                        self.seq4.size, self.max_l_seq, MEM_HOST)


class Context:
    """One context per GPU (strl_ctx)."""

    def __init__(self, device=0):
        self.L = load()
        h = C.c_void_p()
        _check(self.L.strl_ctx_create(device, C.byref(h)))
        self.h = h
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            self.L.strl_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return self.L.strl_ctx_stream(self.h)

    def sync(self):
        _check(self.L.strl_ctx_sync(self.h))

    def enable_timing(self, on=True):
        _check(self.L.strl_ctx_enable_timing(self.h, int(on)))

    def kernel_times(self):
        """-> ((ms_classify, ms_score, ms_soft) summed, n_launches) since enable_timing(True)"""
        ms = (C.c_double * 3)()
        n = C.c_uint64(0)
        _check(self.L.strl_ctx_kernel_times(self.h, C.byref(ms), C.byref(n)))
        return tuple(ms), n.value

    KERNEL_NAMES = ["classify_kernel", "score_kernel<whole,A>", "compact_kernel<whole>", "score_kernel<whole,B>", "soft_compact_kernel",
                    "score_kernel<segment,A>", "compact_kernel<segment>", "score_kernel<segment,B>"]

    def kernel_times_detail(self):
        """-> ({launch name: ms summed}, n) since enable_timing(True): one entry per kernel launch of a scoring pass"""
        ms = (C.c_double * 8)()
        n = C.c_uint64(0)
        _check(self.L.strl_ctx_kernel_times_detail(self.h, C.byref(ms), C.byref(n)))
        return dict(zip(self.KERNEL_NAMES, list(ms))), n.value

    def set_opts(self, proportion_repeat=0.8, min_mapq=40, median_fragment_length=0):
        self.opts = Opts(median_fragment_length, proportion_repeat, min_mapq)
        _check(self.L.strl_ctx_set_opts(self.h, C.byref(self.opts)))

    def set_genome(self, g: GenomeStr):
        if g is None:
            _check(self.L.strl_ctx_set_genome(self.h, None))
            return
        has = np.ascontiguousarray(g.has_chrom, np.uint8)
        off = np.ascontiguousarray(g.iv_off, np.int64)
        st = np.ascontiguousarray(g.iv_start, np.int32)
        en = np.ascontiguousarray(g.iv_stop, np.int32)
        cg = CGenomeStr(int(g.n_tid), has.ctypes.data, off.ctypes.data, _ptr(st), _ptr(en))
        _check(self.L.strl_ctx_set_genome(self.h, C.byref(cg)))

    # ---- scorer --------------------------------------------------------------------------------
    def score_reads(self, rec_or_soa):
        """-> (whole uint32[n], soft SOFT_DTYPE[m] sorted by read_side, ScoreStats)"""
        soa = rec_or_soa if isinstance(rec_or_soa, Soa) else Soa(rec_or_soa)
        n = soa.n
        whole = np.zeros(max(n, 1), np.uint32)
        soft = np.zeros(2 * n + 1, SOFT_DTYPE)
        ns = C.c_uint64(0)
        st = ScoreStats()
        cs = soa.c_struct()
        _check(self.L.strl_score_reads(self.h, C.byref(cs), whole.ctypes.data, soft.ctypes.data, 2 * n, C.byref(ns), C.byref(st)))
        return whole[:n], soft[:ns.value].copy(), st

    def score_device(self, cs: CReadSoa, whole_ptr, soft_ptr, soft_cap, sync=False):
        """Device-resident batch (pointers from torch tensors). Asynchronous unless sync."""
        if sync:
            ns = C.c_uint64(0)
            st = ScoreStats()
            _check(self.L.strl_score_reads(self.h, C.byref(cs), whole_ptr, soft_ptr, soft_cap, C.byref(ns), C.byref(st)))
            return ns.value, st
        _check(self.L.strl_score_reads(self.h, C.byref(cs), whole_ptr, soft_ptr, soft_cap, None, None))
        return None

    def index_chrom(self, seq, window=100, step=60):
        """packed get_repeat word of every window of a chromosome (strling index, genome_strs.nim:61-92)"""
        if isinstance(seq, str):
            seq = seq.encode()
        nw = C.c_uint64(0)
        _check(self.L.strl_index_chrom(self.h, seq, len(seq), window, step, None, C.byref(nw)))
        words = np.zeros(max(1, nw.value), np.uint32)
        _check(self.L.strl_index_chrom(self.h, seq, len(seq), window, step, words.ctypes.data, C.byref(nw)))
        return words[:nw.value]

    def index_regions(self, seq, window=100, step=60):
        """the (start, stop, unit) rows `strling index` writes for one chromosome (genome_strs.nim:61-92, :137)"""
        if isinstance(seq, str):
            seq = seq.encode()
        return index_regions(seq, self.index_chrom(seq, window, step), window, step)

    def sort_pairs(self, keys, vals, bit_lo=0, bits=64, n_max=None):
        """stable LSD radix sort of (uint64 key, uint32 value) pairs on the device (strl_sort_pairs) -> (keys, vals)"""
        k = np.ascontiguousarray(keys, np.uint64).copy()
        v = np.ascontiguousarray(vals, np.uint32).copy()
        _check(self.L.strl_sort_pairs(self.h, _ptr(k), _ptr(v), k.size, k.size if n_max is None else n_max, bit_lo, bits))
        return k, v

    def sort_probe(self, keys, vals, alt_keys, alt_vals, d_n, n_max, stages, scratch_skew=0, scratch_delta=0, poison=0, layout_bits=None):
        """radix_sort_pairs as the device pipelines call it (strl_sort_probe, test-only): four arrays of `cap` elements for the two
        buffer pairs, *d_n = d_n whatever n_max <= cap is, stages = [(bit_lo, bits, tables_zeroed), ...] chained on one poisoned
        scratch without a sync.  layout_bits = b: nothing is launched, only the table layout of a b-bit sort is reported.
        -> (keys, vals, alt_keys, alt_vals after, dict(result_in_alt, rc[stage], tables_off, tables_bytes, guard_bad))"""
        a = [np.ascontiguousarray(x, t).copy() for x, t in ((keys, np.uint64), (vals, np.uint32), (alt_keys, np.uint64), (alt_vals, np.uint32))]
        cap = a[0].size
        assert all(x.size == cap for x in a)
        n_stages = 0 if layout_bits is not None else len(stages)
        st = np.ascontiguousarray([(0, layout_bits, 0)] if layout_bits is not None else stages, np.int32).reshape(-1, 3)
        assert st.shape[0] == max(n_stages, 1)
        rc = np.zeros(st.shape[0], np.int32)
        in_alt, off, tb, bad = C.c_int(0), C.c_int64(0), C.c_uint64(0), C.c_uint64(0)
        _check(self.L.strl_sort_probe(self.h, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), cap, int(d_n), int(n_max), st.ctypes.data, n_stages,
                                      int(scratch_skew), int(scratch_delta), int(poison), C.byref(in_alt), rc.ctypes.data, C.byref(off), C.byref(tb),
                                      C.byref(bad)))
        return a[0], a[1], a[2], a[3], dict(result_in_alt=bool(in_alt.value), rc=[int(x) for x in rc[:n_stages]], tables_off=off.value,
                                            tables_bytes=tb.value, guard_bad=bad.value)


    # ---- the outlier stage (strling-outliers.py; csrc/outliers.hip): host arrays in and out

    def outliers_row_medians(self, x, keep=None):
        """per-row medians of a (rows, cols) float64 matrix, NaN skipped -> (m_all, m_kept, m_filled); keep: per-column mask
        (strl_outliers_row_medians: the depth medians of :247, :281-282, :296)"""
        x = np.ascontiguousarray(x, np.float64)
        r, c = x.shape
        k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        out = [np.empty(r, np.float64) for _ in range(3)]
        _check(self.L.strl_outliers_row_medians(self.h, _ptr(x), r, c, _ptr(k), *[o.ctypes.data for o in out], MEM_HOST))
        return tuple(out)

    def outliers_huber(self, x):
        """hubers_est (:115-136) of every row -> (mu, sd, method) with method 'Huber' / 'MAD' (strl_outliers_huber)"""
        x = np.ascontiguousarray(x, np.float64)
        r, c = x.shape
        mu, sd, m = np.empty(r, np.float64), np.empty(r, np.float64), np.empty(r, np.uint8)
        _check(self.L.strl_outliers_huber(self.h, _ptr(x), r, c, mu.ctypes.data, sd.ctypes.data, m.ctypes.data, MEM_HOST))
        return mu, sd, np.where(m == 0, "Huber", "MAD")

    def outliers_scores(self, x, mu, sd, null_x=None, null_mu=None, null_sd=None):
        """z, p, p_adj (:138-141, :359-404) of a (loci, samples) matrix; null_*: control-only rows that count in BH only
        (strl_outliers_scores)"""
        x = np.ascontiguousarray(x, np.float64)
        r, c = x.shape
        mu, sd = np.ascontiguousarray(mu, np.float64), np.ascontiguousarray(sd, np.float64)
        nx = None if null_x is None else np.ascontiguousarray(null_x, np.float64)
        nm = np.ascontiguousarray(null_mu if null_mu is not None else [], np.float64)
        ns = np.ascontiguousarray(null_sd if null_sd is not None else [], np.float64)
        z, p, q = (np.empty((r, c), np.float64) for _ in range(3))
        _check(self.L.strl_outliers_scores(self.h, _ptr(x), _ptr(mu), _ptr(sd), r, c, _ptr(nx), _ptr(nm), _ptr(ns), nm.size,
                                           z.ctypes.data, p.ctypes.data, q.ctypes.data, MEM_HOST))
        return z, p, q

    def outliers_order(self, outlier, allele2):
        """STRs.tsv row order (:451) over two (loci, samples) matrices -> row-major cell indices (strl_outliers_order)"""
        z = np.ascontiguousarray(outlier, np.float64)
        a = np.ascontiguousarray(allele2, np.float64)
        r, c = z.shape
        o = np.empty(r * c, np.uint32)
        _check(self.L.strl_outliers_order(self.h, _ptr(z), _ptr(a), r, c, o.ctypes.data, MEM_HOST))
        return o

    def extract_device(self, cs: CReadSoa, cp: CPairSoa, n_tail, item_cap=0, tread_cap=0):
        """scoring + pair logic of one batch, asynchronous for device-resident batches (strl_extract_device)"""
        _check(self.L.strl_extract_device(self.h, C.byref(cs), C.byref(cp), n_tail, item_cap, tread_cap))

    def extract_chunks(self, chunks, n_tail, hint=0):
        """chunked form: chunks = iterable of (CReadSoa, CPairSoa) in file order (strl_extract_begin / _add / _finish)"""
        _check(self.L.strl_extract_begin(self.h, hint))
        for cs, cp in chunks:
            _check(self.L.strl_extract_add(self.h, C.byref(cs), C.byref(cp)))
        _check(self.L.strl_extract_finish(self.h, n_tail, 0, 0))

    def treads_fetch(self, want=True):
        """-> (treads of the last extract_device call in .bin order, ScoreStats)"""
        no = C.c_uint64(0)
        st = ScoreStats()
        _check(self.L.strl_treads_fetch(self.h, None, 0, C.byref(no), C.byref(st)))
        out = np.zeros(max(1, no.value), TREAD_DTYPE)
        if want and no.value:
            _check(self.L.strl_treads_fetch(self.h, out.ctypes.data, out.size, C.byref(no), None))
        return out[:no.value], st

    def score_queue_ids(self, cap):
        """the read ids the skip-predicate pass queued in the context's last scoring pass, in queue order, after a sync
        (strl_score_queue_probe, test-only); `cap`: the batch's reads -> (ids, their number)"""
        out = np.zeros(max(1, int(cap)), np.uint32)
        n = C.c_uint64(0)
        _check(self.L.strl_score_queue_probe(self.h, out.ctypes.data, int(cap), C.byref(n)))
        return out[:min(int(n.value), int(cap))], int(n.value)

    def pair_items(self):
        """join items of the context's last pair pass, after a sync (strl_pair_items_probe, test-only): the reads the probe let
        through the Bloom bitmap plus the hot soft-clip records, clamped to the pass' item capacity"""
        n = C.c_uint64(0)
        _check(self.L.strl_pair_items_probe(self.h, C.byref(n)))
        return n.value

    def pair_times(self):
        ms = (C.c_double * 5)()
        _check(self.L.strl_ctx_pair_times(self.h, C.byref(ms)))
        return dict(zip(["pair_soft_items_kernel", "pair_probe_kernel", "pair_join_sort", "pair_groups_kernel", "pair_order"], list(ms)))

    # ---- extract (score + pair) -----------------------------------------------------------------
    def extract(self, rec: RecordBatch, n_tail=-1):
        rv = _RecView(rec)
        cap = max(1024, rv.n // 4)
        while True:
            out = np.zeros(cap, TREAD_DTYPE)
            no = C.c_uint64(0)
            st = ScoreStats()
            rc = self.L.strl_extract(self.h, C.byref(rv.c), n_tail, out.ctypes.data, cap, C.byref(no), C.byref(st))
            if rc == -4 and no.value > cap:
                cap = int(no.value)
                continue
            _check(rc)
            return out[:no.value].copy(), st

    def pair_reads(self, rec: RecordBatch, whole, soft, n_tail=-1):
        rv = _RecView(rec)
        whole = np.ascontiguousarray(whole, np.uint32)
        soft = np.ascontiguousarray(soft, SOFT_DTYPE)
        cap = max(1024, rv.n // 4)
        while True:
            out = np.zeros(cap, TREAD_DTYPE)
            no = C.c_uint64(0)
            rc = self.L.strl_pair_reads(C.byref(rv.c), C.byref(self.opts), whole.ctypes.data, _ptr(soft), soft.size, n_tail,
                                        out.ctypes.data, cap, C.byref(no))
            if rc == -4 and no.value > cap:
                cap = int(no.value)
                continue
            _check(rc)
            return out[:no.value].copy()

    # ---- cluster --------------------------------------------------------------------------------
    def cluster(self, treads, mode, window, min_support=5, min_clip=0, min_clip_total=0, max_clip_dist=200):
        t = np.ascontiguousarray(treads, TREAD_DTYPE)
        cap = max(64, t.size)
        out = np.zeros(cap, BOUNDS_DTYPE)
        unpl = np.zeros(8192, UNPLACED_DTYPE)
        no, nu = C.c_uint64(0), C.c_uint64(0)
        st = ClusterStats()
        _check(self.L.strl_cluster(self.h, _ptr(t), t.size, mode, window, min_support, min_clip, min_clip_total, max_clip_dist,
                                   out.ctypes.data, cap, C.byref(no), unpl.ctypes.data, unpl.size, C.byref(nu), C.byref(st)))
        return out[:no.value].copy(), unpl[:nu.value].copy(), st

    def set_treads(self, treads):
        """make a host array of treads the context's resident treads, as extract_device would have left them
        (strl_ctx_set_treads): what cluster_resident clusters next"""
        t = np.ascontiguousarray(treads, TREAD_DTYPE)
        _check(self.L.strl_ctx_set_treads(self.h, _ptr(t), t.size))

    def cluster_resident(self, n_tid, window, min_support=5, min_clip=0, min_clip_total=0, max_clip_dist=200, pos_bits=0, fetch=True,
                         cap=None):
        """cluster the treads the last extract_device call left on the device (strl_cluster_resident, call mode).
        fetch=False only enqueues the kernels."""
        if not fetch:
            _check(self.L.strl_cluster_resident(self.h, MODE_CALL, n_tid, pos_bits, window, min_support, min_clip, min_clip_total,
                                                max_clip_dist, None, 0, None, None, 0, None, None))
            return None
        cap = cap or 1 << 16
        while True:
            out = np.zeros(cap, BOUNDS_DTYPE)
            unpl = np.zeros(8192, UNPLACED_DTYPE)
            no, nu = C.c_uint64(0), C.c_uint64(0)
            st = ClusterStats()
            rc = self.L.strl_cluster_resident(self.h, MODE_CALL, n_tid, pos_bits, window, min_support, min_clip, min_clip_total,
                                              max_clip_dist, out.ctypes.data, cap, C.byref(no), unpl.ctypes.data, unpl.size,
                                              C.byref(nu), C.byref(st))
            if rc == -4 and no.value > cap:
                cap = int(no.value)
                continue
            _check(rc)
            return out[:no.value].copy(), unpl[:nu.value].copy(), st

    def cluster_collect(self, cap=None):
        """results of the last cluster_resident(fetch=False) -- which ran on the context's side stream, overlapping whatever
        was enqueued after it (strl_cluster_collect) -> (bounds, unplaced, stats)"""
        cap = cap or 1 << 16
        while True:
            out = np.zeros(cap, BOUNDS_DTYPE)
            unpl = np.zeros(8192, UNPLACED_DTYPE)
            no, nu = C.c_uint64(0), C.c_uint64(0)
            st = ClusterStats()
            rc = self.L.strl_cluster_collect(self.h, out.ctypes.data, cap, C.byref(no), unpl.ctypes.data, unpl.size, C.byref(nu), C.byref(st))
            if rc == -4 and no.value > cap:
                cap = int(no.value)
                continue
            _check(rc)
            return out[:no.value].copy(), unpl[:nu.value].copy(), st

    def bounds_bare(self, positions, splits, max_clip_dist, min_clip=0, min_clip_total=0):
        """bounds() + gate of one bare cluster (strl_bounds_bare) -> (bounds record, good)"""
        p = np.ascontiguousarray(positions, np.uint32)
        sp = np.ascontiguousarray(splits, np.uint8)
        out = np.zeros(1, BOUNDS_DTYPE)
        good = C.c_int(0)
        _check(self.L.strl_bounds_bare(self.h, p.ctypes.data, sp.ctypes.data, p.size, min_clip, min_clip_total, max_clip_dist, out.ctypes.data, C.byref(good)))
        return out[0], bool(good.value)

    def regions_fetch(self, streams, sizes, regions, crcs=None, cap=None, layout=False):
        """strl_regions_fetch: `streams` / `sizes` = raw DEFLATE payloads + ISIZE of BGZF blocks; regions = list of
        (first_block, n_blocks, in_block, tid, beg, end) -> list of (record bytes, status); layout=True: that list, out_off and
        out_len.  cap = the bytes of `out` (default: what the header says always suffices); a StrlingError of STRL_ERR_CAPACITY
        carries the bytes needed (out_off[0]) as `.needed`"""
        comp = np.frombuffer(b"".join(streams) + b"\0" * 8, np.uint8)
        clen = np.array([len(x) for x in streams], np.uint32)
        coff = np.zeros(len(streams), np.uint64)
        coff[1:] = np.cumsum(clen[:-1], dtype=np.uint64)
        isz = np.asarray(sizes, np.uint32)
        req = np.zeros(len(regions), REGION_REQ_DTYPE)
        for k, r in enumerate(regions):
            req[k] = tuple(r)
        if cap is None:
            cap = sum(int(isz[r[0]:r[0] + r[1]].sum()) + 32 for r in regions) + 64
        out = np.zeros(max(1, cap), np.uint8)
        off = np.zeros(len(regions), np.uint64)
        ln = np.zeros(len(regions), np.uint64)
        st = np.zeros(len(regions), np.uint8)
        crc = None if crcs is None else np.asarray(crcs, np.uint32)
        try:
            _check(self.L.strl_regions_fetch(self.h, comp.ctypes.data, int(clen.sum()), _ptr(coff), _ptr(clen), _ptr(isz), None if crc is None else _ptr(crc), len(streams),
                                             req.ctypes.data, len(regions), out.ctypes.data, cap, _ptr(off), _ptr(ln), _ptr(st)))
        except StrlingError as e:
            if e.code == -4 and len(regions):
                e.needed = int(off[0])
            raise
        got = [(out[int(o):int(o) + int(n)].tobytes(), int(x)) for o, n, x in zip(off, ln, st)]
        return (got, off, ln) if layout else got

    def _evidence_call(self, n, call, cap):
        """the support / summary / status buffers of the evidence entry points, grown once if `cap` proves short"""
        while True:
            sup = np.zeros(max(1, cap), SUPPORT_DTYPE)
            off = np.zeros(n + 1, np.uint64)
            sm = np.zeros(max(1, n), SPAN_SUMMARY_DTYPE)
            st = np.zeros(max(1, n), np.uint8)
            rc = call(sup, cap, off, sm, st)
            if rc == -4 and int(off[n]) > cap:
                cap = int(off[n])
                continue
            _check(rc)
            return [(sup[int(off[r]):int(off[r + 1])].copy(), int(sm["median_depth"][r]), np.float32(sm["expected_spanners"][r]), int(st[r])) for r in range(n)]

    def evidence_records(self, regions, bounds, window, frag, min_mapq=20):
        """strl_evidence_records: regions = list of bytes (block_size-prefixed BAM records, what regions_fetch returns), bounds =
        one BOUNDS_DTYPE record per region -> list of (support array, median_depth, expected_spanners, status); status 2 = passed
        on to spanners()"""
        n = len(regions)
        raw = b"".join(regions)
        buf = np.frombuffer(raw + b"\0" * 8, np.uint8)
        ln = np.array([len(x) for x in regions], np.uint64)
        off = np.zeros(n, np.uint64)
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
        bb = np.ascontiguousarray(bounds, BOUNDS_DTYPE).reshape(n)
        frag = np.ascontiguousarray(frag, np.uint32)

        def call(sup, cap, soff, sm, st):
            return self.L.strl_evidence_records(self.h, buf.ctypes.data, _ptr(off), _ptr(ln), bb.ctypes.data, n, window, frag.ctypes.data, min_mapq,
                                                sup.ctypes.data, cap, _ptr(soff), sm.ctypes.data, _ptr(st))
        return self._evidence_call(n, call, len(raw) // 128 + 64 * n + 64)

    def regions_evidence(self, streams, sizes, regions, bounds, window, frag, min_mapq=20, crcs=None):
        """strl_regions_evidence: regions_fetch's arguments plus one bound per region -> list of (support array, median_depth,
        expected_spanners, status); status 1 = the blocks end before the query does, 2 = passed on to spanners()"""
        comp = np.frombuffer(b"".join(streams) + b"\0" * 8, np.uint8)
        clen = np.array([len(x) for x in streams], np.uint32)
        coff = np.zeros(len(streams), np.uint64)
        coff[1:] = np.cumsum(clen[:-1], dtype=np.uint64)
        isz = np.asarray(sizes, np.uint32)
        n = len(regions)
        req = np.zeros(n, REGION_REQ_DTYPE)
        for k, r in enumerate(regions):
            req[k] = tuple(r)
        bb = np.ascontiguousarray(bounds, BOUNDS_DTYPE).reshape(n)
        frag = np.ascontiguousarray(frag, np.uint32)
        crc = None if crcs is None else np.asarray(crcs, np.uint32)
        ms = C.c_double(0)

        def call(sup, cap, soff, sm, st):
            return self.L.strl_regions_evidence(self.h, comp.ctypes.data, int(clen.sum()), _ptr(coff), _ptr(clen), _ptr(isz), None if crc is None else _ptr(crc),
                                                len(streams), req.ctypes.data, bb.ctypes.data, n, window, frag.ctypes.data, min_mapq, sup.ctypes.data, cap,
                                                _ptr(soff), sm.ctypes.data, _ptr(st), C.byref(ms))
        return self._evidence_call(n, call, sum(int(isz[r[0]:r[0] + r[1]].sum()) for r in regions) // 128 + 64 * n + 64)

    def _pull_blocks(self, streams, sizes, regions, crcs):
        comp = np.frombuffer(b"".join(streams) + b"\0" * 8, np.uint8)
        clen = np.array([len(x) for x in streams], np.uint32)
        coff = np.zeros(len(streams), np.uint64)
        coff[1:] = np.cumsum(clen[:-1], dtype=np.uint64)
        isz = np.asarray(sizes, np.uint32)
        req = np.zeros(len(regions), REGION_REQ_DTYPE)
        for k, r in enumerate(regions):
            req[k] = tuple(r)
        crc = None if crcs is None else np.asarray(crcs, np.uint32)
        return comp, clen, coff, isz, req, crc

    def pull_select(self, streams, sizes, regions, tiles, crcs=None):
        """strl_pull_select: regions_fetch's `streams` / `sizes` / `regions` (one per tile) plus tiles = PULL_TILE_DTYPE records ->
        (rows, tile_rows, record bytes, status per tile, kernel ms); rows[tile_rows[t]:tile_rows[t + 1]] are tile t's kept
        records in file order, rows["off"] indexes the bytes, rows["count"] = kept records of the call with the same qname"""
        comp, clen, coff, isz, req, crc = self._pull_blocks(streams, sizes, regions, crcs)
        n = len(regions)
        tl = np.ascontiguousarray(tiles, PULL_TILE_DTYPE).reshape(n)
        tot = int(isz.sum())
        rows = np.zeros(tot // 36 + n + 1, PULL_ROW_DTYPE)
        out = np.zeros(2 * tot + 64, np.uint8)
        tile_rows = np.zeros(n + 1, np.uint64)
        st = np.zeros(max(1, n), np.uint8)
        nr, nb, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        _check(self.L.strl_pull_select(self.h, comp.ctypes.data, int(clen.sum()), _ptr(coff), _ptr(clen), _ptr(isz), None if crc is None else _ptr(crc), len(streams),
                                       req.ctypes.data, tl.ctypes.data, n, rows.ctypes.data, rows.size, C.byref(nr), _ptr(tile_rows), out.ctypes.data, out.size,
                                       C.byref(nb), _ptr(st), C.byref(ms)))
        return rows[:nr.value].copy(), tile_rows, out[:nb.value].tobytes(), st[:n], ms.value

    def pull_mates(self, streams, sizes, regions, win_off, reqs, names, crcs=None):
        """strl_pull_mates: one region per window, window w holding reqs[win_off[w]:win_off[w + 1]] (PULL_REQ_DTYPE, names in
        `names`) -> (rows, record bytes, status per window, kernel ms); rows[k] answers reqs[k] (found = 0: no mate)"""
        comp, clen, coff, isz, req, crc = self._pull_blocks(streams, sizes, regions, crcs)
        n = len(regions)
        wo = np.ascontiguousarray(win_off, np.uint32)
        rq = np.ascontiguousarray(reqs, PULL_REQ_DTYPE)
        nm = np.frombuffer(bytes(names) + b"\0" * 8, np.uint8)
        rows = np.zeros(max(1, rq.size), PULL_ROW_DTYPE)
        out = np.zeros(2 * int(isz.sum()) + 64, np.uint8)
        st = np.zeros(max(1, n), np.uint8)
        nb, ms = C.c_uint64(0), C.c_double(0)
        _check(self.L.strl_pull_mates(self.h, comp.ctypes.data, int(clen.sum()), _ptr(coff), _ptr(clen), _ptr(isz), None if crc is None else _ptr(crc), len(streams),
                                      req.ctypes.data, _ptr(wo), n, rq.ctypes.data, nm.ctypes.data, len(names), rows.ctypes.data, out.ctypes.data, out.size,
                                      C.byref(nb), _ptr(st), C.byref(ms)))
        return rows[:rq.size].copy(), out[:nb.value].tobytes(), st[:n], ms.value

    def inflate_blocks(self, streams, sizes):
        """raw DEFLATE streams (list of bytes) with their inflated sizes -> list of inflated bytes (strl_inflate_blocks)"""
        comp = np.frombuffer(b"".join(streams) + b"\0" * 8, np.uint8)
        clen = np.array([len(s) for s in streams], np.uint32)
        coff = np.zeros(len(streams), np.uint64)
        coff[1:] = np.cumsum(clen[:-1], dtype=np.uint64)
        isz = np.asarray(sizes, np.uint32)
        out = np.zeros(int(isz.sum()) + 16, np.uint8)
        _check(self.L.strl_inflate_blocks(self.h, comp.ctypes.data, int(clen.sum()), _ptr(coff), _ptr(clen), _ptr(isz), len(streams), out.ctypes.data, out.size))
        res, o = [], 0
        for n in isz:
            res.append(out[o:o + int(n)].tobytes())
            o += int(n)
        return res

    # ---- extract with the BAM front end on the device ---------------------------------------------
    @staticmethod
    def _bam_blocks(path):
        """the host side of the device front end in Python: BGZF block table (payload offset, payload length, isize, crc), the
        header (inflated here) -> dict(data, blocks, block_off = file offset of each block of the table, n_ref, targets, text, b0 = the block the first record
        starts in, first_off, header_raw = the header's inflated bytes)"""
        import struct, zlib
        data = np.fromfile(path, np.uint8)
        raw = data.tobytes()
        blocks, block_off, o = [], [], 0
        while o < len(raw):
            xlen = struct.unpack_from("<H", raw, o + 10)[0]
            bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
            isz = struct.unpack_from("<I", raw, o + bsize - 4)[0]
            if isz:
                blocks.append((o + 12 + xlen, bsize - 12 - xlen - 8, isz, struct.unpack_from("<I", raw, o + bsize - 8)[0]))
                block_off.append(o)
            o += bsize
        hdr, k = b"", 0

        def need(nbytes):
            nonlocal hdr, k
            while len(hdr) < nbytes and k < len(blocks):
                po, pl = blocks[k][:2]
                hdr += zlib.decompress(raw[po:po + pl], -15)
                k += 1
            if len(hdr) < nbytes:
                raise StrlingError("truncated BAM header")
        need(12)
        assert hdr[:4] == b"BAM\1"
        l_text = struct.unpack_from("<i", hdr, 4)[0]
        need(12 + l_text)
        text = hdr[8:8 + l_text].decode()
        n_ref = struct.unpack_from("<i", hdr, 8 + l_text)[0]
        at, targets = 12 + l_text, []
        for _ in range(n_ref):
            need(at + 4)
            ln = struct.unpack_from("<i", hdr, at)[0]
            need(at + 8 + ln)
            targets.append((hdr[at + 4:at + 4 + ln - 1].decode(), struct.unpack_from("<i", hdr, at + 4 + ln)[0]))
            at += 8 + ln
        cum, b0 = 0, 0                                        # the block the first record starts in
        while b0 < len(blocks) and cum + blocks[b0][2] <= at:
            cum += blocks[b0][2]
            b0 += 1
        return dict(data=data, raw=raw, blocks=blocks, block_off=block_off, n_ref=n_ref, targets=targets, text=text, b0=b0, first_off=at - cum, header_raw=hdr[:at])

    def _front_push_blocks(self, B, c0, c1, chunk_blocks, check_crc, trim=0, index=False, no_offsets_at=None):
        """blocks [c0, c1) of the table through strl_front_push in chunks; trim = inflated bytes at the end of the LAST block that
        are not this context's (strl_front_trim_next before the last chunk) -> the chunk summaries that came back.
        index: every chunk's file offsets go to strl_front_index_blocks first (but not those of push number no_offsets_at)"""
        done = (FrontChunk * 2)()
        nd = C.c_int(0)
        chunks, keep = [], []
        data, blocks = B["data"], B["blocks"]
        for s0 in range(c0, c1, chunk_blocks):
            cb = blocks[s0:min(c1, s0 + chunk_blocks)]
            lo, hi = cb[0][0], cb[-1][0] + cb[-1][1]
            comp = np.ascontiguousarray(data[lo:hi])
            coff = np.array([b[0] - lo for b in cb], np.uint64)
            clen = np.array([b[1] for b in cb], np.uint32)
            isz = np.array([b[2] for b in cb], np.uint32)
            crc = np.array([b[3] for b in cb], np.uint32)
            keep.append((comp, coff, clen, isz, crc))           # pageable memory: the copy is staged by the runtime
            if trim and s0 + chunk_blocks >= c1:
                _check(self.L.strl_front_trim_next(self.h, trim))
            if index and (s0 - c0) // chunk_blocks != no_offsets_at:
                boff = np.array(B["block_off"][s0:min(c1, s0 + chunk_blocks)], np.uint64)
                _check(self.L.strl_front_index_blocks(self.h, _ptr(boff), hi + 8, len(cb)))
            _check(self.L.strl_front_push(self.h, comp.ctypes.data, comp.size, _ptr(coff), _ptr(clen), _ptr(isz), _ptr(crc) if check_crc else None, len(cb), done, C.byref(nd)))
            chunks += [_front_chunk(done[i]) for i in range(nd.value)]
            keep = keep[-3:]
        _check(self.L.strl_front_finish(self.h, done, C.byref(nd)))
        chunks += [_front_chunk(done[i]) for i in range(nd.value)]
        return chunks

    def _front_results(self, B, chunks):
        """pair logic over everything this context holds + the treads, their names, the fragment words"""
        n_ref = B["n_ref"]
        n_rec = sum(c["n_records"] for c in chunks)
        n_tail = 0
        for c in chunks:                                      # trailing run of unplaced records over the whole file
            n_tail = c["n_records"] - 1 - c["last_placed"] if c["last_placed"] >= 0 else n_tail + c["n_records"]
        _check(self.L.strl_extract_finish(self.h, n_tail, 3 * n_rec + 16, 8 * n_rec + 16))
        no = C.c_uint64(0)
        _check(self.L.strl_treads_fetch(self.h, None, 0, C.byref(no), None))
        out = np.zeros(max(1, no.value), TREAD_DTYPE)
        _check(self.L.strl_treads_fetch(self.h, out.ctypes.data, out.size, C.byref(no), None))
        out = out[:no.value]
        ids = np.ascontiguousarray(out["qname_id"], np.int64)
        qoff = np.zeros(ids.size + 1, np.uint64)
        needb = C.c_uint64(0)
        buf = np.zeros(max(16, 256 * ids.size), np.uint8)
        _check(self.L.strl_front_qnames(self.h, _ptr(ids), ids.size, _ptr(qoff), buf.ctypes.data, buf.size, C.byref(needb)))
        names = [buf[int(qoff[i]):int(qoff[i + 1])].tobytes() for i in range(ids.size)]
        fw = np.zeros(max(1, n_rec), np.uint32)
        _check(self.L.strl_front_fragwords(self.h, 0, n_rec, fw.ctypes.data))
        seen = np.zeros(max(1, n_ref), np.uint8)
        _check(self.L.strl_front_tids(self.h, seen.ctypes.data, n_ref))
        return dict(treads=out, qnames=names, fragwords=fw[:n_rec], chunks=chunks, n_records=n_rec, n_tail=n_tail, targets=B["targets"], header=B["text"],
                    tids_seen=seen[:n_ref])

    def extract_bam_device(self, path, chunk_blocks=16384, n_reads_hint=0, check_crc=True):
        """`strling extract`'s read loop over a BAM FILE with inflate, record scan and parse on the device
        (strl_front_begin / _push / _finish + strl_extract_finish).  The host side here only walks BGZF block headers.
        -> dict(treads, qnames, fragwords, chunks, n_records, n_tail, targets, header)"""
        B = self._bam_blocks(path)
        _check(self.L.strl_front_begin(self.h, B["n_ref"], B["first_off"], n_reads_hint))
        chunks = self._front_push_blocks(B, B["b0"], len(B["blocks"]), chunk_blocks, check_crc)
        return self._front_results(B, chunks)

    def extract_bam_device_indexed(self, path, chunk_blocks=16384, runs0=0, n_reads_hint=0, check_crc=True, no_offsets_at=None, csi=None):
        """extract_bam_device with the .bai built in the same pass (strl_front_index_begin / _blocks / _finish; `strling extract
        --write-index`).  runs0: initial capacity of the run table.  csi = (min_shift, depth): the uncompressed CSI payload instead
        (strl_front_index_begin_csi; depth None or < 0 = samtools' rule).  -> (extract_bam_device's dict, bytes of the .bai or None,
        dict(n_records, n_no_coor, n_runs, n_chunks) or None, None or (status, message) of the index's refusal)"""
        B = self._bam_blocks(path)
        l_ref = np.array([t[1] for t in B["targets"]], np.int32)
        _check(self.L.strl_front_begin(self.h, B["n_ref"], B["first_off"], n_reads_hint))
        try:
            if csi is None:
                _check(self.L.strl_front_index_begin(self.h, _ptr(l_ref) if l_ref.size else None, runs0))
            else:
                _check(self.L.strl_front_index_begin_csi(self.h, _ptr(l_ref) if l_ref.size else None, runs0, int(csi[0]), -1 if csi[1] is None else int(csi[1])))
            chunks = self._front_push_blocks(B, B["b0"], len(B["blocks"]), chunk_blocks, check_crc, index=True, no_offsets_at=no_offsets_at)
            nbytes = C.c_uint64(0)
            info = BamindexInfo()
            rc = self.L.strl_front_index_finish(self.h, C.byref(nbytes), C.byref(info))
            bai, inf, refused = None, None, None
            if rc:
                refused = (rc, self.L.strl_last_error().decode())
            else:
                out = np.zeros(max(1, nbytes.value), np.uint8)
                _check(self.L.strl_bamindex_fetch(self.h, out.ctypes.data, out.size))
                bai, inf = out[:nbytes.value].tobytes(), {k: int(getattr(info, k)) for k, _ in BamindexInfo._fields_}
            res = self._front_results(B, chunks)
        finally:
            self.L.strl_bamindex_end(self.h)
        return res, bai, inf, refused

    def bamindex(self, path, chunk_blocks=16384, check_crc=True, csi=None):
        """the .bai of a coordinate-sorted BAM FILE built on the device (strl_bamindex_begin / _push / _finish / _fetch; what
        `samtools index` writes).  csi = (min_shift, depth): the CSI index instead (strl_bamindex_begin_csi; depth None or < 0 =
        samtools' rule), as its UNCOMPRESSED payload -- a .csi file is that in BGZF blocks (bamio.bgzf_bytes).
        -> (bytes of the .bai / of the CSI payload, dict(n_records, n_no_coor, n_runs, n_chunks))"""
        B = self._bam_blocks(path)
        l_ref = np.array([t[1] for t in B["targets"]], np.int32)
        if csi is None:
            _check(self.L.strl_bamindex_begin(self.h, B["n_ref"], _ptr(l_ref) if l_ref.size else None, B["first_off"]))
        else:
            _check(self.L.strl_bamindex_begin_csi(self.h, B["n_ref"], _ptr(l_ref) if l_ref.size else None, B["first_off"], int(csi[0]), -1 if csi[1] is None else int(csi[1])))
        try:
            data, blocks, keep = B["data"], B["blocks"], []
            for s0 in range(B["b0"], len(blocks), chunk_blocks):
                cb = blocks[s0:s0 + chunk_blocks]
                lo, hi = cb[0][0], cb[-1][0] + cb[-1][1]
                comp = np.ascontiguousarray(data[lo:hi])
                coff = np.array([b[0] - lo for b in cb], np.uint64)
                clen = np.array([b[1] for b in cb], np.uint32)
                isz = np.array([b[2] for b in cb], np.uint32)
                crc = np.array([b[3] for b in cb], np.uint32)
                boff = np.array(B["block_off"][s0:s0 + chunk_blocks], np.uint64)
                keep = (keep + [(comp, coff, clen, isz, crc, boff)])[-3:]      # pageable memory: the copy is staged by the runtime
                _check(self.L.strl_bamindex_push(self.h, comp.ctypes.data, comp.size, _ptr(coff), _ptr(clen), _ptr(isz), _ptr(crc) if check_crc else None,
                                                 _ptr(boff), hi + 8, len(cb)))
            nbytes = C.c_uint64(0)
            info = BamindexInfo()
            _check(self.L.strl_bamindex_finish(self.h, C.byref(nbytes), C.byref(info)))
            out = np.zeros(max(1, nbytes.value), np.uint8)
            _check(self.L.strl_bamindex_fetch(self.h, out.ctypes.data, out.size))
        finally:
            self.L.strl_bamindex_end(self.h)
        return out[:nbytes.value].tobytes(), {k: int(getattr(info, k)) for k, _ in BamindexInfo._fields_}

    # ---- `strling sort` on the device (strl_bamsort_*): the ABI's steps one by one, and the whole sort of a file
    def bamsort_begin(self, n_ref, first_off, arena_limit_bytes=0):
        _check(self.L.strl_bamsort_begin(self.h, int(n_ref), int(first_off), int(arena_limit_bytes)))

    def bamsort_reserve(self, max_blocks, max_comp_bytes):
        _check(self.L.strl_bamsort_reserve(self.h, int(max_blocks), int(max_comp_bytes)))

    def bamsort_push(self, comp, coff, clen, isize, crc=None):
        """one chunk of BGZF blocks: comp uint8 (pageable memory: the runtime stages the copy), coff uint64 / clen / isize / crc uint32 per block"""
        _check(self.L.strl_bamsort_push(self.h, comp.ctypes.data, comp.size, _ptr(coff), _ptr(clen), _ptr(isize), _ptr(crc) if crc is not None else None, len(coff)))

    def bamsort_finish(self, header):
        """header: the output's header bytes (bamsort_header) -> dict of strl_bamsort_info"""
        h = np.frombuffer(bytes(header), np.uint8)
        info = BamsortInfo()
        _check(self.L.strl_bamsort_finish(self.h, _ptr(h), h.size, C.byref(info)))
        return {k: getattr(info, k) for k, _ in BamsortInfo._fields_}

    def bamsort_info(self):
        info = BamsortInfo()
        _check(self.L.strl_bamsort_info_now(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in BamsortInfo._fields_}

    def bamsort_fetch(self, off, nbytes):
        out = np.zeros(max(1, nbytes), np.uint8)
        _check(self.L.strl_bamsort_fetch(self.h, int(off), int(nbytes), out.ctypes.data))
        return out[:nbytes].tobytes()

    def bamsort_fetch_bgzf(self, off, nbytes):
        """-> (BGZF members of the stream's bytes [off, off + nbytes) from the device compressor, members stored)"""
        out = np.zeros(max(1, bgzf_deflate_bound(nbytes)), np.uint8)
        nb, stored = C.c_uint64(0), C.c_uint32(0)
        _check(self.L.strl_bamsort_fetch_bgzf(self.h, int(off), int(nbytes), out.ctypes.data, out.size, C.byref(nb), C.byref(stored)))
        return out[:nb.value].tobytes(), stored.value

    def bamsort_order(self, n):
        perm = np.zeros(max(1, n), np.uint32)
        _check(self.L.strl_bamsort_order(self.h, perm.ctypes.data, n))
        return perm[:n]

    def bamsort_index(self, member_off, l_ref, csi=None):
        """the index of the finished sort's output from what the sort still holds (strl_bamsort_index / _index_fetch), after the last
        fetch and before bamsort_end.  member_off: the file offset of every member the stream was written as (0xFF00 bytes each),
        the EOF block's last; l_ref: the references' lengths; csi = (min_shift, depth) as bamindex's
        -> (bytes of the .bai / of the CSI payload, dict(n_records, n_no_coor, n_runs, n_chunks))"""
        m = np.ascontiguousarray(member_off, np.uint64)
        lr = np.ascontiguousarray(list(l_ref) + [0], np.int32)
        nbytes, info = C.c_uint64(0), BamindexInfo()
        ms, dp = (-1, -1) if csi is None else (int(csi[0]), -1 if csi[1] is None else int(csi[1]))
        _check(self.L.strl_bamsort_index(self.h, _ptr(lr), ms, dp, _ptr(m) if m.size else None, max(int(m.size), 1) - 1, C.byref(nbytes), C.byref(info)))
        out = np.zeros(max(1, nbytes.value), np.uint8)
        _check(self.L.strl_bamsort_index_fetch(self.h, out.ctypes.data, out.size))
        return out[:nbytes.value].tobytes(), {k: int(getattr(info, k)) for k, _ in BamindexInfo._fields_}

    def bamsort_end(self):
        self.L.strl_bamsort_end(self.h)

    # ---- `strling sort --markdup` (strl_bamsort_markdup_mode / strl_bamsort_markdup): flag 0x400 on the resident records; the reference
    # drops records that carry it (collect.nim:140)
    def bamsort_markdup_mode(self, on=True):
        """behind bamsort_begin / bamsort_sam_begin and before the first push: the arena's limit leaves room for the step"""
        _check(self.L.strl_bamsort_markdup_mode(self.h, 1 if on else 0))

    def bamsort_markdup(self):
        """behind bamsort_finish and before the first fetch, once -> dict of strl_markdup_info"""
        info = MarkdupInfo()
        _check(self.L.strl_bamsort_markdup(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in MarkdupInfo._fields_}

    # ---- `strling fastq` (strl_bamsort_fastq_mode / _fastq / _fastq_fetch): the resident records as FASTQ text
    def bamsort_fastq_mode(self, on=True):
        """behind bamsort_begin / bamsort_sam_begin and before the first push; not together with bamsort_markdup_mode"""
        _check(self.L.strl_bamsort_fastq_mode(self.h, 1 if on else 0))

    def bamsort_fastq(self, **opts):
        """behind bamsort_finish, once: the join and the layout.  opts: filter, suffix, default_qual, interleaved, singles
        -> dict of strl_fastq_info (stream_bytes = the lengths of p1, p2 and s)"""
        o, info = _fastq_opts(**opts), FastqInfo()
        _check(self.L.strl_bamsort_fastq(self.h, C.byref(o), C.byref(info)))
        return _fastq_info(info)

    def bamsort_fastq_fetch(self, stream, lo, nbytes, canary=0):
        """bytes [lo, lo + nbytes) of stream 0 (p1), 1 (p2) or 2 (s).  canary > 0 (tests): that many guard bytes on either side of
        the destination, checked to be untouched"""
        out = np.full(max(1, nbytes) + 2 * canary, 0xA5, np.uint8)
        _check(self.L.strl_bamsort_fastq_fetch(self.h, int(stream), int(lo), int(nbytes), out.ctypes.data + canary))
        if canary and not ((out[:canary] == 0xA5).all() and (out[canary + nbytes:][-canary:] == 0xA5).all()):
            raise AssertionError("strl_bamsort_fastq_fetch wrote outside its destination")
        return out[canary:canary + nbytes].tobytes()

    def bamsort_fastq_info(self):
        info = FastqInfo()
        _check(self.L.strl_bamsort_fastq_info_now(self.h, C.byref(info)))
        return _fastq_info(info)

    def bamsort_probe(self, lens, base, lo, hi):
        """test-only (strl_bamsort_probe): the layout and the piece search over caller-given lengths and a 64-bit base
        -> (off uint64[n + 1], (first, end) of the touched records, parts uint64[touched, 3] = source skip, destination, bytes)"""
        l = np.ascontiguousarray(lens, np.uint32)
        off = np.zeros(l.size + 1, np.uint64)
        rng = np.zeros(2, np.uint64)
        parts = np.zeros((max(1, l.size), 3), np.uint64)
        _check(self.L.strl_bamsort_probe(self.h, _ptr(l), l.size, int(base), int(lo), int(hi), off.ctypes.data, rng.ctypes.data, parts.ctypes.data, l.size))
        a, b = int(rng[0]), int(rng[1])
        return off, (a, b), parts[:b - a]

    # ---- SAM text as the sort's input (strl_bamsort_sam_begin / _sam_reserve / _push_sam): encoded to BAM records on the device
    def bamsort_sam_begin(self, names, arena_limit_bytes=0):
        """names: the @SQ names in order (str or bytes)"""
        nm, off = _sam_names(names)
        _check(self.L.strl_bamsort_sam_begin(self.h, _ptr(nm), off.ctypes.data, len(off) - 1, int(arena_limit_bytes)))

    def bamsort_sam_reserve(self, max_text_bytes):
        _check(self.L.strl_bamsort_sam_reserve(self.h, int(max_text_bytes)))

    def bamsort_push_sam(self, text):
        """one chunk of whole alignment lines, the last byte a newline"""
        t = np.frombuffer(bytes(text), np.uint8)
        _check(self.L.strl_bamsort_push_sam(self.h, _ptr(t), t.size))

    def bamsort_sam_info(self):
        f = BamsortSamFigures()
        _check(self.L.strl_bamsort_sam_info(self.h, C.byref(f)))
        return {k: getattr(f, k) for k, _ in BamsortSamFigures._fields_}

    def bamsort_sam(self, text, chunk_bytes=1 << 20, keep_open=False):
        """SAM TEXT (header lines and alignment lines) coordinate-sorted on the device -> (the output stream, strl_bamsort_info as a
        dict with the SAM figures added, the permutation).  Chunks of whole lines of at most chunk_bytes, a longer line alone."""
        text = bytes(text)
        raw, names, _ = sam_header(text)
        l_text = int.from_bytes(raw[4:8], "little")
        body = text[l_text:]
        if body and not body.endswith(b"\n"):
            body += b"\n"
        chunks, at = [], 0
        while at < len(body):
            cut = body.rfind(b"\n", at, at + chunk_bytes)
            cut = body.index(b"\n", at) if cut < 0 else cut
            chunks.append(body[at:cut + 1])
            at = cut + 1
        self.bamsort_sam_begin(names)
        try:
            self.bamsort_sam_reserve(max([len(c) for c in chunks] + [1]))
            for c in chunks:
                self.bamsort_push_sam(c)
            info = self.bamsort_finish(bamsort_header(raw))
            info.update(self.bamsort_sam_info())
            stream = self.bamsort_fetch(0, info["stream_bytes"])
            perm = self.bamsort_order(info["n_records"])
        except Exception:
            self.bamsort_end()
            raise
        if not keep_open:
            self.bamsort_end()
        return stream, info, perm

    # ---- `strling sort --windowed` (strl_bamsort_begin_windowed / _window_*): a file larger than device memory, in passes
    def bamsort_begin_windowed(self, n_ref, first_off):
        _check(self.L.strl_bamsort_begin_windowed(self.h, int(n_ref), int(first_off)))

    def bamsort_window_limit(self):
        """the largest window of the stream the device can hold now, in bytes"""
        n = C.c_uint64(0)
        _check(self.L.strl_bamsort_window_limit(self.h, C.byref(n)))
        return n.value

    def bamsort_window_begin(self, lo, hi):
        _check(self.L.strl_bamsort_window_begin(self.h, int(lo), int(hi)))

    def bamsort_window_push(self, comp, coff, clen, isize, crc=None):
        """one chunk of the same file again, as bamsort_push takes it"""
        _check(self.L.strl_bamsort_window_push(self.h, comp.ctypes.data, comp.size, _ptr(coff), _ptr(clen), _ptr(isize), _ptr(crc) if crc is not None else None, len(coff)))

    def bamsort_window_end(self):
        _check(self.L.strl_bamsort_window_end(self.h))

    def bamsort_window_probe(self, lens, perm, base, lo, hi):
        """test-only (strl_bamsort_window_probe): the layout, the inversion of the permutation and the scatter's part arithmetic over
        caller-given lengths (by input ordinal), perm[rank] = ordinal and a 64-bit base
        -> (dest uint64[n] by ordinal, parts uint64[n, 3] = source skip, destination, bytes of each ordinal's part inside [lo, hi))"""
        l = np.ascontiguousarray(lens, np.uint32)
        p = np.ascontiguousarray(perm, np.uint32)
        assert l.size == p.size
        dest = np.zeros(max(1, l.size), np.uint64)
        parts = np.zeros((max(1, l.size), 3), np.uint64)
        _check(self.L.strl_bamsort_window_probe(self.h, _ptr(l) if l.size else None, _ptr(p) if p.size else None, l.size, int(base), int(lo), int(hi), dest.ctypes.data,
                                                parts.ctypes.data))
        return dest[:l.size], parts[:l.size]

    @staticmethod
    def _bam_chunks(B, chunk_blocks):
        """the blocks of a file (_bam_blocks) in chunks of chunk_blocks, as a push takes them (pageable memory: the runtime stages the copy)"""
        data, blocks = B["data"], B["blocks"]
        for s0 in range(B["b0"], len(blocks), chunk_blocks):
            cb = blocks[s0:s0 + chunk_blocks]
            lo, hi = cb[0][0], cb[-1][0] + cb[-1][1]
            yield (np.ascontiguousarray(data[lo:hi]), np.array([b[0] - lo for b in cb], np.uint64), np.array([b[1] for b in cb], np.uint32),
                   np.array([b[2] for b in cb], np.uint32), np.array([b[3] for b in cb], np.uint32))

    def bamsort_windowed(self, path, window_bytes, chunk_blocks=16384, piece_bytes=0xFF00, again=None, keep_open=False):
        """a BAM FILE coordinate-sorted on the device in windows of the output stream (bamsort_window_plan(stream, window_bytes,
        piece_bytes)): pass 0 over the file, then the file once more per window, every window fetched whole
        -> (the output stream, strl_bamsort_info as a dict with "windows" and "window_bytes" added).
        again (tests): the file the windows' passes read instead of `path` -- a changed input between passes is refused.
        keep_open: the sort is left on the context with its last window current (bamsort_end ends it)"""
        B = self._bam_blocks(path)
        B2 = B if again is None else self._bam_blocks(again)
        header = bamsort_header(B["header_raw"])
        self.bamsort_begin_windowed(B["n_ref"], B["first_off"])
        try:
            keep = []
            for ch in self._bam_chunks(B, chunk_blocks):
                keep = (keep + [ch])[-3:]
                self.bamsort_push(*ch)
            info = self.bamsort_finish(header)
            W, P = bamsort_window_plan(info["stream_bytes"], window_bytes, piece_bytes)
            out = []
            for w in range(P):
                lo, hi = w * W, min(info["stream_bytes"], (w + 1) * W)
                self.bamsort_window_begin(lo, hi)
                for ch in self._bam_chunks(B2, chunk_blocks):
                    keep = (keep + [ch])[-3:]
                    self.bamsort_window_push(*ch)
                self.bamsort_window_end()
                out.append(self.bamsort_fetch(lo, hi - lo))
            info = dict(self.bamsort_info(), windows=P, window_bytes=W)
        except Exception:
            self.bamsort_end()
            raise
        if not keep_open:
            self.bamsort_end()
        return b"".join(out), info

    def bamsort(self, path, chunk_blocks=16384, check_crc=True, arena_limit_bytes=0, keep_open=False, index=None, markdup=False):
        """a BAM FILE coordinate-sorted on the device -> (the output stream: header || records in sorted order, strl_bamsort_info as a
        dict, the permutation).  keep_open: the sort is left on the context for further fetches (bamsort_end ends it).
        index = "bai" or ("csi", min_shift, depth): the stream is also deflated here (the compressor's host twin, members of 0xFF00
        bytes, the EOF block) and indexed from the sort (bamsort_index) -> a fourth item (the file's bytes, the index's bytes, its
        info); a refusal of the index raises, with the sort ended unless keep_open.
        markdup: flag 0x400 decided on the device before the stream is fetched (bamsort_markdup); info["markdup"] = its dict."""
        B = self._bam_blocks(path)
        header = bamsort_header(B["header_raw"])
        self.bamsort_begin(B["n_ref"], B["first_off"], arena_limit_bytes)
        try:
            if markdup:
                self.bamsort_markdup_mode(True)
            data, blocks, keep = B["data"], B["blocks"], []
            for s0 in range(B["b0"], len(blocks), chunk_blocks):
                cb = blocks[s0:s0 + chunk_blocks]
                lo, hi = cb[0][0], cb[-1][0] + cb[-1][1]
                comp = np.ascontiguousarray(data[lo:hi])
                coff = np.array([b[0] - lo for b in cb], np.uint64)
                clen = np.array([b[1] for b in cb], np.uint32)
                isz = np.array([b[2] for b in cb], np.uint32)
                crc = np.array([b[3] for b in cb], np.uint32)
                keep = (keep + [(comp, coff, clen, isz, crc)])[-3:]      # pageable memory: the copy is staged by the runtime
                self.bamsort_push(comp, coff, clen, isz, crc if check_crc else None)
            info = self.bamsort_finish(header)
            if markdup:
                info["markdup"] = self.bamsort_markdup()
            stream = self.bamsort_fetch(0, info["stream_bytes"])
            perm = self.bamsort_order(info["n_records"])
        except Exception:
            self.bamsort_end()
            raise
        extra = ()
        if index is not None:
            try:
                body = bgzf_deflate_host(stream)[0]
                member_off = bamsort_members(body, 0) + [len(body)]
                got, idx_info = self.bamsort_index(member_off, [t[1] for t in B["targets"]], None if index == "bai" else (index[1], index[2] if len(index) > 2 else None))
                extra = ((body + _BGZF_EOF, got, idx_info),)
            except Exception:
                if not keep_open:
                    self.bamsort_end()
                raise
        if not keep_open:
            self.bamsort_end()
        return (stream, info, perm) + extra

    def sweep(self, path, bounds, window, frag, min_mapq=20, chunk_blocks=16384, check_crc=True):
        """the evidence of every bound from one pass over a coordinate-sorted BAM FILE (strl_sweep_begin / _push / _finish):
        bounds = BOUNDS_DTYPE records in any order -> (list of (support array, median_depth, expected_spanners, status) in that
        order, dict of strl_sweep_info); status 0 = answered, 1 = seam / never closed, 2 = passed on to spanners()"""
        B = self._bam_blocks(path)
        bb = np.ascontiguousarray(bounds, BOUNDS_DTYPE).reshape(-1)
        n = bb.size
        frag = np.ascontiguousarray(frag, np.uint32)
        _check(self.L.strl_sweep_begin(self.h, B["n_ref"], B["first_off"], bb.ctypes.data if n else None, n, window, frag.ctypes.data, min_mapq))
        try:
            data, blocks, keep = B["data"], B["blocks"], []
            for s0 in range(B["b0"], len(blocks), chunk_blocks):
                cb = blocks[s0:s0 + chunk_blocks]
                lo, hi = cb[0][0], cb[-1][0] + cb[-1][1]
                comp = np.ascontiguousarray(data[lo:hi])
                coff = np.array([b[0] - lo for b in cb], np.uint64)
                clen = np.array([b[1] for b in cb], np.uint32)
                isz = np.array([b[2] for b in cb], np.uint32)
                crc = np.array([b[3] for b in cb], np.uint32)
                keep = (keep + [(comp, coff, clen, isz, crc)])[-3:]      # pageable memory: the copy is staged by the runtime
                _check(self.L.strl_sweep_push(self.h, comp.ctypes.data, comp.size, _ptr(coff), _ptr(clen), _ptr(isz), _ptr(crc) if check_crc else None,
                                              len(cb), int(s0 + chunk_blocks >= len(blocks))))
            info = SweepInfo()

            def call(sup, cap, soff, sm, st):
                return self.L.strl_sweep_finish(self.h, sup.ctypes.data, cap, _ptr(soff), sm.ctypes.data, _ptr(st), C.byref(info))
            res = self._evidence_call(n, call, 64 * n + 64)
        finally:
            self.L.strl_sweep_end(self.h)
        return res, {k: getattr(info, k) for k, _ in SweepInfo._fields_}

    def view(self, path, chunk_blocks=16384, check_crc=True, **opts):
        """the records of a BAM FILE as SAM text (strl_view_begin / _push / _finish; csrc/view.hip): opts as strl_view_opts ->
        (the alignment lines as bytes, dict of strl_view_info)"""
        B = self._bam_blocks(path)
        names, off = _sam_names([t[0] for t in B["targets"]])
        names = np.concatenate([names, np.zeros(1, np.uint8)])
        o = _view_opts(**opts)
        _check(self.L.strl_view_begin(self.h, B["n_ref"], B["first_off"], names.ctypes.data, off.ctypes.data, C.byref(o)))
        out, info = [], ViewInfo()
        try:
            data, blocks, keep = B["data"], B["blocks"], []
            text, nb = C.c_void_p(), C.c_uint64(0)
            for s0 in range(B["b0"], len(blocks), chunk_blocks):
                cb = blocks[s0:s0 + chunk_blocks]
                lo, hi = cb[0][0], cb[-1][0] + cb[-1][1]
                comp = np.ascontiguousarray(data[lo:hi])
                coff = np.array([b[0] - lo for b in cb], np.uint64)
                clen = np.array([b[1] for b in cb], np.uint32)
                isz = np.array([b[2] for b in cb], np.uint32)
                crc = np.array([b[3] for b in cb], np.uint32)
                keep = (keep + [(comp, coff, clen, isz, crc)])[-3:]      # pageable memory: the copy is staged by the runtime
                _check(self.L.strl_view_push(self.h, comp.ctypes.data, comp.size, _ptr(coff), _ptr(clen), _ptr(isz), _ptr(crc) if check_crc else None, len(cb),
                                             C.byref(text), C.byref(nb)))
                if nb.value:
                    out.append(C.string_at(text.value, nb.value))
            _check(self.L.strl_view_finish(self.h, C.byref(text), C.byref(nb), C.byref(info)))
            if nb.value:
                out.append(C.string_at(text.value, nb.value))
        finally:
            self.L.strl_view_end(self.h)
        return b"".join(out), _view_info(info)

    def view_records(self, records, names, cap=None, guard=0, **opts):
        """records back to back in host memory, each with its block_size word, as SAM text through the device's two kernels
        (strl_view_records).  names: the references' names in order.  cap: the room given (default: what is needed); guard: bytes
        of 0xA5 on both sides of the room, returned as they are found afterwards -> (text, dict of strl_view_info[, before, behind])"""
        src = np.frombuffer(bytes(records), np.uint8)
        nm, off = _sam_names(names)
        nm = np.concatenate([nm, np.zeros(1, np.uint8)])
        o, info, need = _view_opts(**opts), ViewInfo(), C.c_uint64(0)
        ptr = _ptr(src) if src.size else None
        if cap is None:
            rc = self.L.strl_view_records(self.h, ptr, src.size, nm.ctypes.data, off.ctypes.data, len(names), C.byref(o), None, 0, C.byref(need), C.byref(info))
            if rc not in (0, -4):
                _check(rc)
            cap = need.value
        buf = np.full(int(cap) + 2 * guard + 1, 0xA5, np.uint8)
        _check(self.L.strl_view_records(self.h, ptr, src.size, nm.ctypes.data, off.ctypes.data, len(names), C.byref(o), buf.ctypes.data + guard, int(cap), C.byref(need), C.byref(info)))
        text = buf[guard:guard + need.value].tobytes()
        if guard:
            return text, _view_info(info), buf[:guard].tobytes(), buf[guard + need.value:guard + need.value + guard].tobytes()
        return text, _view_info(info)

    def bgzf_deflate(self, data, block=0xFF00, out=None, mode=None):
        """bytes -> (BGZF members back to back, without the EOF block; csize uint32[members]; members that went out stored), on the
        device (strl_bgzf_deflate).  mode = "fast" (the default's rule and bytes) or "dense" (strl_bgzf_deflate_mode)"""
        if mode is None:
            return _bgzf_deflate(lambda *a: self.L.strl_bgzf_deflate(self.h, *a), data, block, out)
        m = _deflate_mode(mode)
        return _bgzf_deflate(lambda *a: self.L.strl_bgzf_deflate_mode(self.h, m, *a), data, block, out)

    def deflate_ms(self):
        """kernel time (ms) of the last bgzf_deflate call"""
        ms = C.c_double(0)
        _check(self.L.strl_ctx_deflate_ms(self.h, C.byref(ms)))
        return ms.value

    def inflate_ms(self):
        """kernel time (ms) of the last inflate_blocks call"""
        ms = C.c_double(0)
        _check(self.L.strl_ctx_inflate_ms(self.h, C.byref(ms)))
        return ms.value

    def cluster_times(self):
        ms = (C.c_double * 3)()
        _check(self.L.strl_ctx_cluster_times(self.h, C.byref(ms)))
        return dict(zip(["cluster_keys_sort_groups", "cluster_sweep", "cluster_bounds"], list(ms)))

    def tail_stream(self):
        """hipStream_t (as an int) the tail of the last extract_device call runs on (strl_ctx_tail_stream)"""
        return int(self.L.strl_ctx_tail_stream(self.h) or 0)

    def treads_device(self):
        """(device pointer of the resident treads, capacity in treads, device pointer of their uint32 count)"""
        p, cap, cnt = C.c_void_p(), C.c_uint64(0), C.c_void_p()
        _check(self.L.strl_ctx_treads_device(self.h, C.byref(p), C.byref(cap), C.byref(cnt)))
        return p.value, cap.value, cnt.value

    def cluster_gathered(self, gathered_ptr, counts_ptr, world, pad, rank, n_tid, window, min_support=5, min_clip=0, min_clip_total=0,
                         max_clip_dist=200, pos_bits=0, mode=MODE_CALL, fetch=True):
        """this rank's share of an all-gathered tread set (strl_cluster_gathered); fetch=False only enqueues the kernels"""
        if not fetch:
            _check(self.L.strl_cluster_gathered(self.h, gathered_ptr, counts_ptr, world, pad, rank, mode, n_tid, pos_bits, window, min_support,
                                                min_clip, min_clip_total, max_clip_dist, None, 0, None, None, 0, None, None))
            return None
        cap = 1 << 16
        while True:
            out = np.zeros(cap, BOUNDS_DTYPE)
            unpl = np.zeros(8192, UNPLACED_DTYPE)
            no, nu = C.c_uint64(0), C.c_uint64(0)
            st = ClusterStats()
            rc = self.L.strl_cluster_gathered(self.h, gathered_ptr, counts_ptr, world, pad, rank, mode, n_tid, pos_bits, window, min_support,
                                              min_clip, min_clip_total, max_clip_dist, out.ctypes.data, cap, C.byref(no), unpl.ctypes.data,
                                              unpl.size, C.byref(nu), C.byref(st))
            if rc == -4 and no.value > cap:
                cap = int(no.value)
                continue
            _check(rc)
            return out[:no.value].copy(), unpl[:nu.value].copy(), st

    # ---- the exchange step inside the library (comm.hip: RCCL over xGMI / device copies) ---------
    def comm_init(self, world, rank, unique_id=None):
        """one process per GPU: join the RCCL communicator `unique_id` (bytes from comm_unique_id() on rank 0) names"""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id) if unique_id is not None else None
        _check(self.L.strl_ctx_comm_init(self.h, world, rank, buf))

    def comm_info(self):
        w, r, u = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(self.L.strl_ctx_comm_info(self.h, C.byref(w), C.byref(r), C.byref(u)))
        return w.value, r.value, bool(u.value)

    def cluster_exchange(self, pad, n_tid, window, min_support=5, min_clip=0, min_clip_total=0, max_clip_dist=200, pos_bits=0, mode=MODE_CALL, fetch=True):
        """all-gather of the resident treads over the context's communicator + clustering of my (tid, unit) groups
        (strl_cluster_exchange); fetch=False only enqueues"""
        if not fetch:
            _check(self.L.strl_cluster_exchange(self.h, pad, mode, n_tid, pos_bits, window, min_support, min_clip, min_clip_total, max_clip_dist,
                                                None, 0, None, None, 0, None, None))
            return None
        cap = 1 << 16
        while True:
            out = np.zeros(cap, BOUNDS_DTYPE)
            unpl = np.zeros(8192, UNPLACED_DTYPE)
            no, nu = C.c_uint64(0), C.c_uint64(0)
            st = ClusterStats()
            rc = self.L.strl_cluster_exchange(self.h, pad, mode, n_tid, pos_bits, window, min_support, min_clip, min_clip_total, max_clip_dist,
                                              out.ctypes.data, cap, C.byref(no), unpl.ctypes.data, unpl.size, C.byref(nu), C.byref(st))
            if rc == -4 and no.value > cap:
                cap = int(no.value)
                continue
            _check(rc)
            return out[:no.value].copy(), unpl[:nu.value].copy(), st

    def exchange_treads(self):
        """all ranks' treads of the last exchange, (rank, .bin) order"""
        n = C.c_uint64(0)
        _check(self.L.strl_exchange_treads(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), TREAD_DTYPE)
        _check(self.L.strl_exchange_treads(self.h, out.ctypes.data, out.size, C.byref(n)))
        return out[:n.value]

    def cluster_collect(self, cap=1 << 16):
        """rows of the last (asynchronous) clustering pass of this context (strl_cluster_collect)"""
        while True:
            out = np.zeros(cap, BOUNDS_DTYPE)
            unpl = np.zeros(8192, UNPLACED_DTYPE)
            no, nu = C.c_uint64(0), C.c_uint64(0)
            st = ClusterStats()
            rc = self.L.strl_cluster_collect(self.h, out.ctypes.data, cap, C.byref(no), unpl.ctypes.data, unpl.size, C.byref(nu), C.byref(st))
            if rc == -4 and no.value > cap:
                cap = int(no.value)
                continue
            _check(rc)
            return out[:no.value].copy(), unpl[:nu.value].copy(), st

    def cluster_members(self, n_bounds):
        """indices (into the tread array of the last cluster() call) of every returned bound's reads, cluster order"""
        off = np.zeros(n_bounds + 1, np.uint64)
        nm = C.c_uint64(0)
        _check(self.L.strl_cluster_members(self.h, off.ctypes.data, None, 0, C.byref(nm)))
        mem = np.zeros(max(1, nm.value), np.uint32)
        _check(self.L.strl_cluster_members(self.h, off.ctypes.data, mem.ctypes.data, mem.size, C.byref(nm)))
        return off, mem[:nm.value]

    def cluster_replay(self):
        """device side of the last cluster() call again, asynchronously (bench)"""
        _check(self.L.strl_cluster_replay(self.h))


def extract_bam_shares(ctxs, path, chunk_blocks=16384, check_crc=True, cut_shift=0):
    """the file in len(ctxs) contiguous shares, one per context (the CLI's `extract --gpus N`): every share begins at a record
    start -- found here by walking the inflated file; the CLI takes them from the .bai --, ends where the next begins
    (strl_front_trim_next on its last chunk, strl_front_tail_bytes == 0 afterwards), the per-read state is gathered on the
    first context (strl_ctxs_extract_gather), which then runs the pair logic.  cut_shift != 0 moves every cut that many bytes
    off its record start: what a stale index does.  -> (result of the first context as extract_bam_device, tail bytes per share)"""
    import struct, zlib
    c0 = ctxs[0]
    B = c0._bam_blocks(path)
    blocks, raw = B["blocks"], B["raw"]
    infl = b"".join(zlib.decompress(raw[po:po + pl], -15) for po, pl, _, _ in blocks)
    ustart = np.concatenate([[0], np.cumsum([b[2] for b in blocks])]).astype(np.int64)
    q = int(ustart[B["b0"]]) + B["first_off"]
    starts = []
    while q + 4 <= len(infl):
        starts.append(q)
        q += 4 + struct.unpack_from("<i", infl, q)[0]
    G = len(ctxs)
    cuts = [starts[0]] + [starts[len(starts) * g // G] + cut_shift for g in range(1, G)] + [None]
    owners, counts, tails = [], [], []
    for g, ctx in enumerate(ctxs):
        a = cuts[g]
        ba = int(np.searchsorted(ustart, a, side="right")) - 1
        _check(ctx.L.strl_ctx_blocking_waits(ctx.h, 1))
        _check(ctx.L.strl_front_begin(ctx.h, B["n_ref"], a - int(ustart[ba]), 0))
        if cuts[g + 1] is None:
            be, trim = len(blocks), 0
        else:
            e = cuts[g + 1]
            bl = int(np.searchsorted(ustart, e, side="right")) - 1
            uo = e - int(ustart[bl])
            be, trim = (bl + 1, blocks[bl][2] - uo) if uo else (bl, 0)
        chunks = ctx._front_push_blocks(B, ba, be, chunk_blocks, check_crc, trim=trim)
        t = C.c_uint32(0)
        _check(ctx.L.strl_front_tail_bytes(ctx.h, C.byref(t)))
        tails.append(int(t.value))
        owners += [g] * len(chunks)
        counts += [c["n_records"] for c in chunks]
        if g == 0:
            all_chunks = list(chunks)
        else:
            all_chunks += chunks
    if any(tails[:-1]):
        return None, tails
    arr = (C.c_void_p * G)(*[c.h for c in ctxs])
    ow, cn = np.array(owners, np.uint32), np.array(counts, np.uint64)
    _check(c0.L.strl_ctxs_extract_gather(arr, G, _ptr(ow), _ptr(cn), len(owners)))
    return c0._front_results(B, all_chunks), tails


def comm_unique_id():
    """128 bytes that name a new RCCL communicator (rank 0 makes them, every rank passes them to Context.comm_init)"""
    L = load()
    buf = (C.c_uint8 * 128)()
    _check(L.strl_comm_unique_id(buf))
    return bytes(buf)


def group_comm_init(ctxs):
    """one process, several contexts: RCCL when they sit on different devices, ordered device copies when they share one"""
    L = load()
    arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    _check(L.strl_ctxs_comm_init(arr, len(ctxs)))


def group_cluster_exchange(ctxs, n_tid, window, min_support=5, min_clip=0, min_clip_total=0, max_clip_dist=200, pos_bits=0, mode=MODE_CALL, pad=0):
    """the exchange step for all contexts of a one-process group (strl_ctxs_cluster_exchange); rows: Context.cluster_collect"""
    L = load()
    arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    _check(L.strl_ctxs_cluster_exchange(arr, len(ctxs), pad, mode, n_tid, pos_bits, window, min_support, min_clip, min_clip_total, max_clip_dist))


def qname_hash(rec):
    """uint64 hash of every record's qname (strl_qname_hash)"""
    rv = _RecView(rec)
    out = np.zeros(max(rv.n, 1), np.uint64)
    _check(load().strl_qname_hash(C.byref(rv.c), out.ctypes.data))
    return out[:rv.n]


def pair_reads(rec, opts, whole, soft, n_tail=-1):
    """strl_pair_reads without a device context (host state machine only). opts = (p, min_mapq, median_fragment_length)"""
    L = load()
    rv = _RecView(rec)
    o = Opts(int(opts[2]), float(opts[0]), int(opts[1]))
    whole = np.ascontiguousarray(whole, np.uint32)
    soft = np.ascontiguousarray(soft, SOFT_DTYPE)
    cap = max(1024, rv.n // 4)
    while True:
        out = np.zeros(cap, TREAD_DTYPE)
        no = C.c_uint64(0)
        rc = L.strl_pair_reads(C.byref(rv.c), C.byref(o), _ptr(whole), _ptr(soft), soft.size, n_tail, out.ctypes.data, cap, C.byref(no))
        if rc == -4 and no.value > cap:
            cap = int(no.value)
            continue
        _check(rc)
        return out[:no.value].copy()


def pair_rule(ctx, op, A, B, opts, B_position=0):
    """one pair rule on single treads (strl_pair_rule): ctx = a Context (device code) or None (host twin).
    op 0 adjust_by, 1 unplaced_pair, 2 canonical_repeat; opts = (p, min_mapq, median_fragment_length) -> (result, A after)"""
    a = np.ascontiguousarray(A, TREAD_DTYPE).reshape(1).copy()
    b = np.ascontiguousarray(B, TREAD_DTYPE).reshape(1).copy()
    o = Opts(int(opts[2]), float(opts[0]), int(opts[1]))
    res = C.c_int(0)
    _check(load().strl_pair_rule(ctx.h if ctx is not None else None, op, a.ctypes.data, b.ctypes.data, C.byref(o), int(B_position), C.byref(res)))
    return res.value, a[0]


def pair_rules(ctx, op, A, B, opts, B_position=None):
    """n cases of one pair rule: arrays of treads A, B and of B_position.  ctx = a Context: ONE launch of the device functions,
    one lane per case (strl_pair_rules_device, test-only); ctx = None: the host twins, case by case (strl_pair_rule).
    -> (results int32[n], A after)"""
    a = np.ascontiguousarray(A, TREAD_DTYPE).copy()
    b = np.ascontiguousarray(B, TREAD_DTYPE)
    n = a.size
    assert b.size == n
    bp = np.zeros(n, np.uint32) if B_position is None else np.ascontiguousarray(B_position, np.uint32)
    assert bp.size == n
    o = Opts(int(opts[2]), float(opts[0]), int(opts[1]))
    res = np.zeros(n, np.int32)
    L = load()
    if ctx is not None:
        _check(L.strl_pair_rules_device(ctx.h, op, _ptr(a), _ptr(b), _ptr(bp), n, C.byref(o), _ptr(res)))
        return res, a
    r = C.c_int(0)
    pa, pb, sz = a.ctypes.data, b.ctypes.data, TREAD_DTYPE.itemsize
    for i in range(n):
        _check(L.strl_pair_rule(None, op, pa + i * sz, pb + i * sz, C.byref(o), int(bp[i]), C.byref(r)))
        res[i] = r.value
    return res, a


def bamsort_key(rec20, n_ref):
    """the sort key of a record from its first 20 bytes behind block_size (strl_bamsort_key; csrc/bamsort_core.h)"""
    b = np.frombuffer(bytes(rec20[:20]), np.uint8)
    if b.size != 20:
        raise ValueError("20 bytes of a record are needed")
    key = C.c_uint64(0)
    _check(load().strl_bamsort_key(b.ctypes.data, int(n_ref), C.byref(key)))
    return key.value


def markdup_host(records):
    """the rule of `strling sort --markdup` without a device (strl_markdup_host; csrc/markdup_core.h): records = BAM records back to
    back in input order, each with its block_size word -> (the flag word every record leaves with, dict of the five counts)"""
    src = np.frombuffer(bytes(records), np.uint8)
    n = C.c_uint64(0)
    info = MarkdupInfo()
    flags = np.zeros(max(src.size // 36, 1), np.uint16)
    _check(load().strl_markdup_host(_ptr(src) if src.size else None, src.size, flags.ctypes.data, flags.size, C.byref(n), C.byref(info)))
    return flags[:n.value].copy(), {k: int(getattr(info, k)) for k, _ in MarkdupInfo._fields_[:5]}


def fastq_host(records, **opts):
    """the rule of `strling fastq` without a device (strl_fastq_host; csrc/fastq_core.h): records = BAM records back to back in input
    order, each with its block_size word; opts as Context.bamsort_fastq's -> ([p1, p2, s] as bytes, dict of the six counts)"""
    src = np.frombuffer(bytes(records), np.uint8)
    o, info = _fastq_opts(**opts), FastqInfo()
    L = load()
    ptr = _ptr(src) if src.size else None
    rc = L.strl_fastq_host(ptr, src.size, C.byref(o), None, (C.c_uint64 * 3)(0, 0, 0), C.byref(info))
    if rc not in (0, -4):
        _check(rc)
    bufs = [np.zeros(max(1, int(n)), np.uint8) for n in info.stream_bytes]
    _check(L.strl_fastq_host(ptr, src.size, C.byref(o), (C.c_void_p * 3)(*[b.ctypes.data for b in bufs]), (C.c_uint64 * 3)(*[b.size for b in bufs]), C.byref(info)))
    return [b[:int(n)].tobytes() for b, n in zip(bufs, info.stream_bytes)], {k: int(getattr(info, k)) for k, _ in FastqInfo._fields_[:6]}


def view_host(records, names, cap=None, **opts):
    """the rule of `strling view` without a device (strl_view_host; csrc/view_core.h): records = BAM records back to back, each with
    its block_size word; names: the references' names in order; opts as strl_view_opts -> (text, dict of strl_view_info).  cap: the
    room given (default: what is needed); too little is a StrlingError of code -4 whose `need` holds the bytes needed"""
    src = np.frombuffer(bytes(records), np.uint8)
    nm, off = _sam_names(names)
    nm = np.concatenate([nm, np.zeros(1, np.uint8)])
    o, info, need = _view_opts(**opts), ViewInfo(), C.c_uint64(0)
    L = load()
    ptr = _ptr(src) if src.size else None
    if cap is None:
        rc = L.strl_view_host(ptr, src.size, nm.ctypes.data, off.ctypes.data, len(names), C.byref(o), None, 0, C.byref(need), C.byref(info))
        if rc not in (0, -4):
            _check(rc)
        cap = need.value
    buf = np.zeros(int(cap) + 1, np.uint8)
    rc = L.strl_view_host(ptr, src.size, nm.ctypes.data, off.ctypes.data, len(names), C.byref(o), buf.ctypes.data, int(cap), C.byref(need), C.byref(info))
    if rc == -4:
        e = StrlingError(L.strl_last_error().decode())
        e.code, e.need = -4, need.value
        raise e
    _check(rc)
    return buf[:need.value].tobytes(), _view_info(info)


def bamsort_key_bits(n_ref):
    return int(load().strl_bamsort_key_bits(int(n_ref)))


def bamsort_header(raw):
    """the header bytes of `strling sort`'s output from the input's inflated bytes (which may go on behind the header): strl_bamsort_header"""
    src = np.frombuffer(bytes(raw), np.uint8)
    n = C.c_uint64(0)
    rc = load().strl_bamsort_header(_ptr(src), src.size, None, 0, C.byref(n))
    if rc not in (0, -4):
        _check(rc)
    out = np.zeros(max(1, n.value), np.uint8)
    _check(load().strl_bamsort_header(_ptr(src), src.size, out.ctypes.data, out.size, C.byref(n)))
    return out[:n.value].tobytes()


def _sam_names(names):
    nb = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    off = np.zeros(len(nb) + 1, np.uint32)
    off[1:] = np.cumsum([len(n) for n in nb], dtype=np.int64)
    return np.frombuffer(b"".join(nb), np.uint8), off


def sam_encode(line, names):
    """one SAM alignment line -> its BAM record with the block_size word, by the rule's host function (strl_sam_encode;
    csrc/sam_core.h).  names: the @SQ names in order.  A refusal is a StrlingError of code -6 with "FIELD: words"."""
    src = np.frombuffer(bytes(line), np.uint8)
    nm, off = _sam_names(names)
    n = C.c_uint64(0)
    out = np.zeros(2 * src.size + 64, np.uint8)
    _check(load().strl_sam_encode(_ptr(src), src.size, _ptr(nm), off.ctypes.data, len(off) - 1, out.ctypes.data, out.size, C.byref(n)))
    return out[:n.value].tobytes()


def sam_header(text):
    """the leading @ lines of SAM text -> (the BAM header they stand for, the @SQ names, their lengths) (strl_sam_header)"""
    src = np.frombuffer(bytes(text), np.uint8)
    n, n_ref = C.c_uint64(0), C.c_int32(0)
    rc = load().strl_sam_header(_ptr(src), src.size, None, 0, C.byref(n), C.byref(n_ref))
    if rc not in (0, -4):
        _check(rc)
    out = np.zeros(max(1, n.value), np.uint8)
    _check(load().strl_sam_header(_ptr(src), src.size, out.ctypes.data, out.size, C.byref(n), C.byref(n_ref)))
    raw = out[:n.value].tobytes()
    at = 12 + int.from_bytes(raw[4:8], "little")
    names, lens = [], []
    for _ in range(n_ref.value):
        l = int.from_bytes(raw[at:at + 4], "little")
        names.append(raw[at + 4:at + 4 + l - 1].decode())
        lens.append(int.from_bytes(raw[at + 4 + l:at + 8 + l], "little"))
        at += 8 + l
    return raw, names, lens


def bgzf_deflate_bound(n, block=0xFF00):
    """the output bytes that always suffice for bgzf_deflate of n bytes (strl_bgzf_deflate_bound)"""
    return int(load().strl_bgzf_deflate_bound(n, block))


def _bgzf_deflate(call, data, block, out):
    """`out`: a caller's uint8 array to write into (tests of the capacity rule and of what is left untouched); default = the bound"""
    src = np.frombuffer(bytes(data), np.uint8)
    if out is None:
        out = np.empty(bgzf_deflate_bound(src.size, block) if 1 <= block <= 0xFF00 else 0, np.uint8)
    csize = np.zeros((src.size + block - 1) // block if block > 0 else 0, np.uint32)
    nb, stored = C.c_uint64(0), C.c_uint32(0)
    _check(call(_ptr(src), src.size, block, out.ctypes.data, out.size, C.byref(nb), _ptr(csize), C.byref(stored)))
    return out[:nb.value].tobytes(), csize, stored.value


_BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bamsort_members(data, file_off=0):
    """the file offset of every BGZF member in `data`, which lies at file_off in its file (strl_bamsort_members: the walk `strling
    sort --write-index` runs over the bytes it writes)"""
    src = np.frombuffer(bytes(data), np.uint8)
    out = np.zeros(len(src) // 26 + 1, np.uint64)
    n = C.c_uint64(0)
    _check(load().strl_bamsort_members(_ptr(src) if src.size else None, src.size, int(file_off), out.ctypes.data, out.size, C.byref(n)))
    return [int(x) for x in out[:n.value]]


def bamsort_window_plan(stream_bytes, limit_bytes, piece_bytes=0xFF00):
    """the windows of `strling sort --windowed` (strl_bamsort_window_plan; csrc/bamsort_core.h) -> (window_bytes, n_windows):
    window_bytes = max(piece_bytes, limit_bytes // piece_bytes * piece_bytes), n_windows = ceil(stream_bytes / window_bytes)"""
    w, n = C.c_uint64(0), C.c_uint64(0)
    _check(load().strl_bamsort_window_plan(int(stream_bytes), int(limit_bytes), int(piece_bytes), C.byref(w), C.byref(n)))
    return w.value, n.value


def bamsort_voff(member_off, stream_bytes, s):
    """the virtual offset of stream offset s of a sort's output (strl_bamsort_voff; csrc/bamsort_core.h): member_off = the file offset
    of every member of 0xFF00 bytes, the EOF block's last"""
    m = np.ascontiguousarray(member_off, np.uint64)
    v = C.c_uint64(0)
    _check(load().strl_bamsort_voff(_ptr(m) if m.size else None, max(int(m.size), 1) - 1, int(stream_bytes), int(s), C.byref(v)))
    return int(v.value)


DEFLATE_MODES = {"fast": 0, "dense": 1}        # STRL_DEFLATE_FAST, STRL_DEFLATE_DENSE


def _deflate_mode(mode):
    """the C value of a mode's name; an integer goes through as it is (the library refuses what it does not know)"""
    if isinstance(mode, str):
        if mode not in DEFLATE_MODES:
            raise ValueError(f"bgzf_deflate: mode must be one of {sorted(DEFLATE_MODES)}, not {mode!r}")
        return DEFLATE_MODES[mode]
    return int(mode)


def bgzf_deflate_host(data, block=0xFF00, out=None, mode=None):
    """Context.bgzf_deflate without a device: the same rule on the calling thread, the same bytes (strl_bgzf_deflate_host;
    with a mode, "fast" or "dense", strl_bgzf_deflate_host_mode)"""
    if mode is None:
        return _bgzf_deflate(load().strl_bgzf_deflate_host, data, block, out)
    m = _deflate_mode(mode)
    return _bgzf_deflate(lambda *a: load().strl_bgzf_deflate_host_mode(m, *a), data, block, out)


def pull_select_host(raw, tile, base_off=0):
    """strl_pull_select_host: the rows a tile (PULL_TILE_DTYPE record) keeps of block_size-prefixed records `raw`, in order"""
    L = load()
    buf = np.frombuffer(bytes(raw) + b"\0" * 8, np.uint8)
    tl = np.ascontiguousarray(tile, PULL_TILE_DTYPE).reshape(1)
    rows = np.zeros(len(raw) // 36 + 1, PULL_ROW_DTYPE)
    n = C.c_uint64(0)
    _check(L.strl_pull_select_host(buf.ctypes.data, len(raw), tl.ctypes.data, base_off, rows.ctypes.data, rows.size, C.byref(n)))
    return rows[:n.value].copy()


def pull_counts_host(raw, rows):
    """strl_pull_counts_host: rows with `count` = rows of the same qname bytes (rows["off"] index `raw`)"""
    L = load()
    buf = np.frombuffer(bytes(raw) + b"\0" * 8, np.uint8)
    rows = np.ascontiguousarray(rows, PULL_ROW_DTYPE).copy()
    _check(L.strl_pull_counts_host(buf.ctypes.data, rows.ctypes.data, rows.size))
    return rows


def pull_mates_host(raw, reqs, names, tid=-1, use_interval=True, base_off=0):
    """strl_pull_mates_host: one row per request (PULL_REQ_DTYPE), found = 0 where no record of `raw` meets its rule"""
    L = load()
    buf = np.frombuffer(bytes(raw) + b"\0" * 8, np.uint8)
    rq = np.ascontiguousarray(reqs, PULL_REQ_DTYPE)
    nm = np.frombuffer(bytes(names) + b"\0" * 8, np.uint8)
    rows = np.zeros(max(1, rq.size), PULL_ROW_DTYPE)
    _check(L.strl_pull_mates_host(buf.ctypes.data, len(raw), int(bool(use_interval)), tid, rq.ctypes.data, rq.size, nm.ctypes.data, base_off, rows.ctypes.data))
    return rows[:rq.size]


def pull_order(rows):
    """strl_pull_order: the stable order of the rows by (tid, pos) as signed integers"""
    L = load()
    rows = np.ascontiguousarray(rows, PULL_ROW_DTYPE)
    order = np.zeros(rows.size, np.uint32)
    _check(L.strl_pull_order(rows.ctypes.data, rows.size, order.ctypes.data))
    return order


def _noop():
    pass


def frag_median(frag, pct=0.5):
    frag = np.ascontiguousarray(frag, np.uint32)
    return load().strl_frag_median(frag.ctypes.data, pct)


GROUP_KEY_DTYPE = np.dtype([("tid", "<i4"), ("repeat", "S8")])


def group_order(treads, mode):
    """[(tid, unit bytes)] of the (tid, unit) groups in the reference's Table iteration order (strl_group_order)"""
    L = load()
    t = np.ascontiguousarray(treads, TREAD_DTYPE)
    ng = C.c_uint64(0)
    _check(L.strl_group_order(_ptr(t), t.size, mode, None, 0, C.byref(ng)))
    out = np.zeros(max(1, ng.value), GROUP_KEY_DTYPE)
    _check(L.strl_group_order(_ptr(t), t.size, mode, out.ctypes.data, out.size, C.byref(ng)))
    return [(int(k["tid"]), bytes(k["repeat"])) for k in out[:ng.value]]


def assign_reads_loci(treads, loci, mode):
    """assign_reads_locus (callclusters.nim:14-50) for every locus in order.  Returns (treads with taken ones marked,
    loci with recounted reads, [index arrays of the reads each locus received])."""
    L = load()
    t = np.ascontiguousarray(treads, TREAD_DTYPE).copy()
    lo = np.ascontiguousarray(loci, LOCUS_DTYPE).copy()
    off = np.zeros(lo.size + 1, np.uint64)
    idx = np.zeros(max(1, t.size), np.uint32)
    _check(L.strl_assign_reads_loci(t.ctypes.data, t.size, mode, lo.ctypes.data, lo.size, off.ctypes.data, idx.ctypes.data, idx.size))
    return t, lo, [idx[int(off[j]):int(off[j + 1])].copy() for j in range(lo.size)]


def assign_reads_loci_device(ctx, treads, loci, mode, cap=None):
    """assign_reads_loci on the device (strl_assign_reads_loci_device): the same three results.  cap: entries the assigned
    array may take (default: one per tread, which always suffices)"""
    t = np.ascontiguousarray(treads, TREAD_DTYPE).copy()
    lo = np.ascontiguousarray(loci, LOCUS_DTYPE).copy()
    off = np.zeros(lo.size + 1, np.uint64)
    idx = np.zeros(max(1, t.size if cap is None else cap), np.uint32)
    _check(ctx.L.strl_assign_reads_loci_device(ctx.h, _ptr(t), t.size, mode, _ptr(lo), lo.size, off.ctypes.data, idx.ctypes.data,
                                               idx.size if cap is None else cap))
    return t, lo, [idx[int(off[j]):int(off[j + 1])].copy() for j in range(lo.size)]


def assign_info_last(ctx):
    """figures of the context's last assign_reads_loci_device call -> AssignInfo"""
    info = AssignInfo()
    _check(ctx.L.strl_assign_info_last(ctx.h, C.byref(info)))
    return info


def spanners(rec: RecordBatch, bound, window, frag, min_mapq=20):
    """collect.nim:132-182 over the records of `rec` -> (support array, median_depth, expected_spanners)"""
    L = load()
    rv = _RecView(rec)
    isz = np.ascontiguousarray(rec.isize if rec.isize is not None else np.zeros(rec.n), np.int32)
    frag = np.ascontiguousarray(frag, np.uint32)
    bb = np.ascontiguousarray(bound, BOUNDS_DTYPE).reshape(1)
    cap = 2 * rv.n + 16
    out = np.zeros(cap, SUPPORT_DTYPE)
    sm = SpanSummary()
    _check(L.strl_spanners(C.byref(rv.c), isz.ctypes.data, bb.ctypes.data, window, frag.ctypes.data, min_mapq, out.ctypes.data, cap, C.byref(sm)))
    return out[:sm.n_support].copy(), sm.median_depth, sm.expected_spanners


def genotype(bound, members, qname_off, qnames, supports, depth, median_fragment_length, min_support=5, min_clip=0, min_clip_total=0):
    L = load()
    bb = np.ascontiguousarray(bound, BOUNDS_DTYPE).reshape(1)
    m = np.ascontiguousarray(members, TREAD_DTYPE)
    sp = np.ascontiguousarray(supports, SUPPORT_DTYPE)
    qo = np.ascontiguousarray(qname_off, np.uint64)
    qn = np.frombuffer(bytes(qnames) + b"\0", dtype=np.uint8)
    out = np.zeros(1, CALL_DTYPE)
    o = CallOpts(median_fragment_length, min_support, min_clip, min_clip_total)
    _check(L.strl_genotype(bb.ctypes.data, m.ctypes.data, m.size, qo.ctypes.data, qn.ctypes.data, sp.ctypes.data, sp.size, C.byref(o), float(depth),
                           out.ctypes.data))
    return out[0]


def calls_finish(calls, unplaced):
    """percentiles + output order (call.nim:38-48,264-276) -> (calls, order)"""
    L = load()
    c = np.ascontiguousarray(calls, CALL_DTYPE).copy()
    u = np.ascontiguousarray(unplaced, UNPLACED_DTYPE)
    order = np.zeros(max(1, c.size), np.uint64)
    _check(L.strl_calls_finish(c.ctypes.data, c.size, u.ctypes.data, u.size, order.ctypes.data))
    return c, order[:c.size]


def call_row(call, chrom):
    buf = C.create_string_buffer(1024)
    cc = np.ascontiguousarray(call, CALL_DTYPE).reshape(1)
    load().strl_call_row(buf, 1024, cc.ctypes.data, chrom.encode())
    return buf.value.decode()


def bounds_row(b, chrom):
    buf = C.create_string_buffer(512)
    bb = np.ascontiguousarray(b, BOUNDS_DTYPE).reshape(1)
    load().strl_bounds_row(buf, 512, bb.ctypes.data, chrom.encode())
    return buf.value.decode()


def bin_write(path, proportion_repeat, min_mapq, frag, sam_header, treads, qname_off, qnames):
    t = np.ascontiguousarray(treads, TREAD_DTYPE)
    frag = np.ascontiguousarray(frag, np.uint32)
    qo = np.ascontiguousarray(qname_off, np.uint64)
    hdr = sam_header.encode() if isinstance(sam_header, str) else sam_header
    _check(load().strl_bin_write(path.encode(), proportion_repeat, min_mapq, frag.ctypes.data, hdr, len(hdr), _ptr(t), t.size,
                                 qo.ctypes.data, bytes(qnames) + b"\0"))


def bin_read(path):
    L = load()
    info = BinInfo()
    _check(L.strl_bin_read(path.encode(), C.byref(info), None, None, None, None))
    hdr = C.create_string_buffer(max(1, info.header_len))
    t = np.zeros(max(1, info.n_reads), TREAD_DTYPE)
    qo = np.zeros(info.n_reads + 1, np.uint64)
    qn = C.create_string_buffer(max(1, int(info.qnames_bytes)))
    _check(L.strl_bin_read(path.encode(), C.byref(info), hdr, t.ctypes.data, qo.ctypes.data, qn))
    return dict(proportion_repeat=info.proportion_repeat, min_mapq=info.min_mapq, frag=np.array(info.frag, np.uint32),
                header=hdr.raw[:info.header_len].decode(), treads=t[:info.n_reads].copy(), qname_off=qo,
                qnames=qn.raw[:int(info.qnames_bytes)])
