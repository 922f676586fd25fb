"""Buffer-level Python face of the hg_* C ABI (include/hypergrep_amd.h) for text already resident in HBM.

Used by bench.py, the GPU parity tests and multi-GPU shard drivers.  Device memory is handed over as raw
pointers (e.g. `torch.Tensor.data_ptr()`); no torch types cross into the native library.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from hypergrep_amd import utils

DEFAULT_FLAGS = utils.HS_FLAG_DOTALL | utils.HS_FLAG_MULTILINE | utils.HS_FLAG_SINGLEMATCH
# Report where each match starts (Scanner.hit_starts); not with SINGLEMATCH.  See include/hypergrep_amd.h for the contract.
HS_FLAG_SOM_LEFTMOST = 256
# Logical combinations of other expressions' report ids, and reports that only feed combinations (include/hypergrep_amd.h).
HS_FLAG_COMBINATION = utils.HS_FLAG_COMBINATION
HS_FLAG_QUIET = utils.HS_FLAG_QUIET
HG_ID_INVERT = utils.HG_ID_INVERT  # the id of an inverted scan's records (Scanner.scan(invert=True)): no expression
HG_ID_CONTEXT = utils.HG_ID_CONTEXT  # the ids of Scanner.context()'s records: a context piece, a tail candidate (scan(tail=True))
HG_ID_CONTEXT_TAIL = utils.HG_ID_CONTEXT_TAIL
HG_CONTEXT_TAIL = 1  # hg_context_t.flags
# Scanner.gather (hg_gather_lines): the flags, the kinds of an entry, and the output bytes one workgroup of the copy pass writes
HG_LINES_CONTEXT, HG_LINES_TERMINATE, HG_LINES_NUMBER, HG_LINES_SEPARATOR = 1, 2, 4, 8
HG_LINE_MATCH, HG_LINE_CONTEXT, HG_LINE_TAIL = 0, 1, 2
HG_GATHER_TILE = 16384
# Scanner.count (hg_count_records): the flags, the bins a workgroup counts in LDS, and the records one workgroup takes
HG_COUNTS_ACCUMULATE, HG_COUNTS_PER_SEGMENT = 1, 2
HG_COUNTS_LDS_BINS = 4096
HG_COUNTS_RUN = 16384
# Scanner.gather_parts (hg_gather_parts): the flags, the bits of an entry's kind, and the longest marker
HG_PARTS_NUMBER, HG_PARTS_BYTE_OFFSET, HG_PARTS_TERMINATE, HG_PARTS_LINE = 1, 2, 4, 8
HG_PART_FIRST, HG_PART_LAST = 1, 2
HG_PARTS_MARK_MAX = 16


class HgHit(ctypes.Structure):
    _fields_ = [("line_number", ctypes.c_uint64), ("id", ctypes.c_uint32), ("to", ctypes.c_uint32)]


class HgHitAux(ctypes.Structure):
    _fields_ = [("start", ctypes.c_uint64), ("len", ctypes.c_uint32), ("pattern", ctypes.c_uint32)]


class HgScanResult(ctypes.Structure):
    _fields_ = [
        ("n_hits", ctypes.c_uint64), ("n_lines", ctypes.c_uint64), ("n_candidates", ctypes.c_uint64),
        ("n_raw_hits", ctypes.c_uint64), ("d_hits", ctypes.c_void_p), ("d_aux", ctypes.c_void_p),
        ("ms_stream", ctypes.c_float), ("ms_total", ctypes.c_float), ("reruns", ctypes.c_uint32), ("stream_launches", ctypes.c_uint32),
        ("joiner_tiles", ctypes.c_uint64), ("joiner_launches", ctypes.c_uint32), ("invert_us", ctypes.c_uint32),
    ]


class HgContext(ctypes.Structure):
    _fields_ = [("before", ctypes.c_uint32), ("after", ctypes.c_uint32), ("carry_after", ctypes.c_uint64), ("flags", ctypes.c_uint32)]


class HgContextResult(ctypes.Structure):
    _fields_ = [("n_context", ctypes.c_uint64), ("n_tail", ctypes.c_uint64), ("owed_after", ctypes.c_uint64), ("d_ctx_hits", ctypes.c_void_p),
                ("d_ctx_aux", ctypes.c_void_p), ("context_us", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class HgPart(ctypes.Structure):
    _fields_ = [("line_number", ctypes.c_uint64), ("from_", ctypes.c_uint32), ("to", ctypes.c_uint32)]


class HgPartsResult(ctypes.Structure):
    _fields_ = [("n_parts", ctypes.c_uint64), ("d_parts", ctypes.c_void_p), ("d_part_pattern", ctypes.c_void_p), ("parts_us", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class HgSegments(ctypes.Structure):
    _fields_ = [("d_seg_start", ctypes.c_void_p), ("d_seg_end", ctypes.c_void_p), ("n_seg", ctypes.c_uint32), ("max_per_segment", ctypes.c_uint64)]


class HgSegmentResult(ctypes.Structure):
    _fields_ = [("d_record_segment", ctypes.c_void_p), ("d_first_record", ctypes.c_void_p), ("d_n_lines", ctypes.c_void_p), ("d_n_selected", ctypes.c_void_p),
                ("segments_us", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class HgSegmentPartsResult(ctypes.Structure):
    _fields_ = [("d_part_segment", ctypes.c_void_p), ("d_first_part", ctypes.c_void_p)]


class HgLinesResult(ctypes.Structure):
    _fields_ = [("n_entries", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64), ("d_bytes", ctypes.c_void_p), ("d_entry_off", ctypes.c_void_p),
                ("d_line_number", ctypes.c_void_p), ("d_kind", ctypes.c_void_p), ("d_segment", ctypes.c_void_p), ("d_first_entry", ctypes.c_void_p),
                ("gather_us", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class HgPartLinesParams(ctypes.Structure):  # sizeof 56
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("byte_base", ctypes.c_uint64), ("mark_on_len", ctypes.c_uint32),
                ("mark_off_len", ctypes.c_uint32), ("mark_on", ctypes.c_uint8 * 16), ("mark_off", ctypes.c_uint8 * 16)]


class HgPartLinesResult(ctypes.Structure):  # sizeof 80
    _fields_ = [("n_entries", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64), ("d_bytes", ctypes.c_void_p), ("d_entry_off", ctypes.c_void_p),
                ("d_line_number", ctypes.c_void_p), ("d_kind", ctypes.c_void_p), ("d_pattern", ctypes.c_void_p), ("d_segment", ctypes.c_void_p),
                ("d_first_entry", ctypes.c_void_p), ("gather_us", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


HG_VALUES_BY_PATTERN = 1


class HgValuesParams(ctypes.Structure):  # sizeof 16
    _fields_ = [("flags", ctypes.c_uint32), ("hash_bits", ctypes.c_uint32), ("table_log2", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class HgValuesResult(ctypes.Structure):  # sizeof 88
    _fields_ = [("n_values", ctypes.c_uint64), ("n_parts", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64), ("d_bytes", ctypes.c_void_p), ("d_off", ctypes.c_void_p),
                ("d_count", ctypes.c_void_p), ("d_first", ctypes.c_void_p), ("d_pattern", ctypes.c_void_p), ("d_line_number", ctypes.c_void_p),
                ("d_segment", ctypes.c_void_p), ("table_log2", ctypes.c_uint32), ("values_us", ctypes.c_uint32)]


HG_RANK_BY_PATTERN = 1
HG_RANK_PER_SEGMENT = 2
HG_ACC_BY_PATTERN = 1
HG_ACC_RESET = 2
HG_ACC_ORDER_FIRST = 1


class HgAccParams(ctypes.Structure):  # sizeof 16
    _fields_ = [("flags", ctypes.c_uint32), ("hash_bits", ctypes.c_uint32), ("table_log2", ctypes.c_uint32), ("store_log2", ctypes.c_uint32)]


class HgAccResult(ctypes.Structure):  # sizeof 56
    _fields_ = [("n_distinct", ctypes.c_uint64), ("n_added", ctypes.c_uint64), ("n_groups", ctypes.c_uint64), ("n_parts", ctypes.c_uint64), ("n_parts_total", ctypes.c_uint64),
                ("n_bytes", ctypes.c_uint64), ("store_log2", ctypes.c_uint32), ("acc_us", ctypes.c_uint32)]


class HgAccRankResult(ctypes.Structure):  # sizeof 88
    _fields_ = [("n_values", ctypes.c_uint64), ("n_distinct", ctypes.c_uint64), ("n_parts", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64), ("d_bytes", ctypes.c_void_p),
                ("d_off", ctypes.c_void_p), ("d_count", ctypes.c_void_p), ("d_first", ctypes.c_void_p), ("d_pattern", ctypes.c_void_p), ("d_line_number", ctypes.c_void_p),
                ("store_log2", ctypes.c_uint32), ("rank_us", ctypes.c_uint32)]


class HgRankParams(ctypes.Structure):  # sizeof 24
    _fields_ = [("flags", ctypes.c_uint32), ("hash_bits", ctypes.c_uint32), ("table_log2", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("top", ctypes.c_uint64)]


class HgRankResult(ctypes.Structure):  # sizeof 128
    _fields_ = [("n_values", ctypes.c_uint64), ("n_distinct", ctypes.c_uint64), ("n_parts", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64), ("d_bytes", ctypes.c_void_p),
                ("d_off", ctypes.c_void_p), ("d_count", ctypes.c_void_p), ("d_first", ctypes.c_void_p), ("d_pattern", ctypes.c_void_p), ("d_line_number", ctypes.c_void_p),
                ("d_segment", ctypes.c_void_p), ("d_first_value", ctypes.c_void_p), ("d_seg_distinct", ctypes.c_void_p), ("d_seg_parts", ctypes.c_void_p),
                ("n_seg", ctypes.c_uint32), ("table_log2", ctypes.c_uint32), ("rank_us", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class HgCountsResult(ctypes.Structure):
    _fields_ = [("n_bins", ctypes.c_uint32), ("n_seg", ctypes.c_uint32), ("n_records", ctypes.c_uint64), ("d_ids", ctypes.c_void_p),
                ("d_n_lines", ctypes.c_void_p), ("d_n_reports", ctypes.c_void_p), ("d_seg_lines", ctypes.c_void_p), ("d_seg_reports", ctypes.c_void_p),
                ("counts_us", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class HgFinalizeInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("path", "fin_shift", "fin_nb", "fin_cap", "id_bits", "to_bits", "early_buckets", "early_beside_stream",
                                               "scan_blocks", "left_bucketed", "n_fill", "reserved")]


FIN_PATHS = ("none", "bucketed", "compact_packed", "compact_wide")  # hg_finalize_info_t.path


class HgDbInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("n_patterns", "n_literal_anchored", "n_always_on", "n_factors", "n_windows",
                                               "fold_mask", "max_state_words", "table_bytes", "byte_windows")]


class HgSynthSpec(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("first_block", ctypes.c_uint64), ("hit_per_million", ctypes.c_uint32),
                ("n_needles", ctypes.c_uint32), ("needles", ctypes.c_char_p), ("needle_off", ctypes.POINTER(ctypes.c_uint32))]


SYNTH_BLOCK = 16000

_configured = False


def lib() -> ctypes.CDLL:
    global _configured
    l = utils._get_hyperscanner_lib()  # pylint: disable=protected-access
    if not _configured:
        l.hg_db_compile.restype = ctypes.c_int
        l.hg_db_compile.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                    ctypes.c_uint, ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_size_t]
        l.hg_db_compile_ext.restype = ctypes.c_int
        l.hg_db_compile_ext.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                        ctypes.POINTER(ctypes.POINTER(utils.ExprExt)), ctypes.c_uint, ctypes.POINTER(ctypes.c_void_p),
                                        ctypes.c_char_p, ctypes.c_size_t]
        l.hg_db_release.argtypes = [ctypes.c_void_p]
        l.hg_db_tune.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        l.hg_db_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(HgDbInfo)]
        l.hg_scanner_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_size_t]
        l.hg_scanner_destroy.argtypes = [ctypes.c_void_p]
        l.hg_scanner_error.restype = ctypes.c_char_p
        l.hg_scanner_error.argtypes = [ctypes.c_void_p]
        l.hg_scan_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.POINTER(HgScanResult)]
        if hasattr(l, "hg_scan_device_invert"):  # (absent from a build before the inverted match: HG_LIB comparisons with an older library)
            l.hg_scan_device_invert.argtypes = l.hg_scan_device.argtypes
        if hasattr(l, "hg_scan_device_context"):  # (absent from a build before the context lines)
            l.hg_scan_device_context.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p,
                                                 ctypes.POINTER(HgContext), ctypes.c_int, ctypes.POINTER(HgScanResult), ctypes.POINTER(HgContextResult)]
            l.hg_copy_context.argtypes = [ctypes.c_void_p, ctypes.POINTER(HgHit), ctypes.POINTER(HgHitAux), ctypes.c_uint64]
            l.hg_copy_context_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        if hasattr(l, "hg_scan_device_segments"):  # (absent from a build before the segment stage)
            l.hg_scan_device_segments.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(HgSegments),
                                                  ctypes.c_int, ctypes.POINTER(HgScanResult), ctypes.POINTER(HgSegmentResult)]
            if hasattr(l, "hg_scan_device_segments_context"):  # (absent from a build before the per-file context stage)
                l.hg_scan_device_segments_context.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(HgSegments),
                                                              ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(HgScanResult), ctypes.POINTER(HgSegmentResult),
                                                              ctypes.POINTER(HgContextResult)]
                l.hg_copy_segment_context.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]
            if hasattr(l, "hg_scan_device_segments_parts"):  # (absent from a build before the per-file parts stage)
                l.hg_scan_device_segments_parts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(HgSegments),
                                                            ctypes.POINTER(HgScanResult), ctypes.POINTER(HgSegmentResult), ctypes.POINTER(HgPartsResult),
                                                            ctypes.POINTER(HgSegmentPartsResult)]
                l.hg_copy_segment_parts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]
            l.hg_copy_segments.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint64)]
        if hasattr(l, "hg_scan_device_parts"):  # (absent from a build before the matched parts)
            l.hg_scan_device_parts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p,
                                               ctypes.POINTER(HgScanResult), ctypes.POINTER(HgPartsResult)]
            l.hg_copy_parts.argtypes = [ctypes.c_void_p, ctypes.POINTER(HgPart), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64]
            l.hg_copy_parts_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        if hasattr(l, "hg_gather_lines"):  # (absent from a build before the gather stage)
            p8, p32, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
            l.hg_gather_lines.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(HgLinesResult)]
            l.hg_copy_lines.argtypes = [ctypes.c_void_p, p8, ctypes.c_uint64, p64, p64, p32, p32, ctypes.c_uint64]
            l.hg_copy_lines_first.argtypes = [ctypes.c_void_p, p64]
            l.hg_copy_lines_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        if hasattr(l, "hg_count_records"):  # (absent from a build before the counts stage)
            p32, p64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
            l.hg_count_records.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(HgCountsResult)]
            l.hg_copy_counts.argtypes = [ctypes.c_void_p, p32, p64, p64, ctypes.c_uint32]
            l.hg_copy_segment_counts.argtypes = [ctypes.c_void_p, p32, p32, ctypes.c_uint32, ctypes.c_uint32]
            l.hg_db_report_ids.argtypes = [ctypes.c_void_p, p32, ctypes.c_uint32, p32]
        if hasattr(l, "hg_gather_parts"):  # (absent from a build before the parts gather)
            p8, p32, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
            l.hg_gather_parts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HgPartLinesParams), ctypes.c_void_p,
                                          ctypes.POINTER(HgPartLinesResult)]
            l.hg_copy_part_lines.argtypes = [ctypes.c_void_p, p8, ctypes.c_uint64, p64, p64, p32, p32, p32, ctypes.c_uint64]
            l.hg_copy_part_lines_first.argtypes = [ctypes.c_void_p, p64]
            l.hg_copy_part_lines_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        if hasattr(l, "hg_count_values"):  # (absent from a build before the values stage)
            p8, p32, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
            l.hg_count_values.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HgValuesParams), ctypes.c_void_p, ctypes.POINTER(HgValuesResult)]
            l.hg_copy_values.argtypes = [ctypes.c_void_p, p8, ctypes.c_uint64, p64, p64, p64, p32, p64, p32, ctypes.c_uint64]
            l.hg_copy_values_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        if hasattr(l, "hg_rank_values"):  # (absent from a build before the rank stage)
            p8, p32, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
            l.hg_rank_values.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HgRankParams), ctypes.c_void_p, ctypes.POINTER(HgRankResult)]
            l.hg_copy_ranked_values.argtypes = [ctypes.c_void_p, p8, ctypes.c_uint64, p64, p64, p64, p32, p64, p32, ctypes.c_uint64]
            l.hg_copy_ranked_segments.argtypes = [ctypes.c_void_p, p64, p64, p64]
            l.hg_copy_ranked_values_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        if hasattr(l, "hg_accumulate_values"):  # (absent from a build before the value store)
            p8, p32, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
            l.hg_accumulate_values.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HgAccParams), ctypes.c_void_p, ctypes.POINTER(HgAccResult)]
            l.hg_rank_accumulated.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(HgAccRankResult)]
            l.hg_copy_accumulated.argtypes = [ctypes.c_void_p, p8, ctypes.c_uint64, p64, p64, p64, p32, p64, ctypes.c_uint64]
            l.hg_copy_accumulated_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
            l.hg_reset_accumulated.argtypes = [ctypes.c_void_p]
        l.hg_copy_hits.argtypes = [ctypes.c_void_p, ctypes.POINTER(HgHit), ctypes.POINTER(HgHitAux), ctypes.c_uint64]
        l.hg_copy_hits_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        l.hg_copy_hit_starts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64]
        l.hg_copy_hit_starts_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        l.hg_synth_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HgSynthSpec), ctypes.c_int, ctypes.c_void_p]
        l.hg_synth_host.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(HgSynthSpec)]
        l.hg_debug_alloc_guarded.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]
        l.hg_debug_free_guarded.argtypes = [ctypes.c_void_p]
        l.hg_debug_free_guarded.restype = None
        l.hg_debug_upload.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64]
        l.hg_debug_download.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64]
        l.hg_debug_finalize_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(HgFinalizeInfo), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32]
        l.hg_faceb_next_device.argtypes = [ctypes.c_int]
        l.hg_faceb_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
        l.hg_faceb_stats.restype = None
        _configured = True
    return l


class CompileError(ValueError):
    """A pattern was rejected by the compiler (what check_compatibility reports as 4)."""


class DeviceError(RuntimeError):
    """HIP failure or no usable GPU.  There is no CPU fallback."""


class Database:
    """Compiled pattern set (host side)."""

    def __init__(self, patterns, flags=None, ids=None, ext=None):
        """ext: one utils.ExprExt (extended parameters: approximate matching, offset bounds, min_length) or None per pattern."""
        pa, fa, ia = utils.prepare_patterns(list(patterns), flags=list(flags or ()), ids=list(ids or ()))
        self._h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        if ext is None:
            rc = lib().hg_db_compile(pa, fa, ia, len(pa), ctypes.byref(self._h), err, 512)
        else:
            ea = utils.ext_array(ext, len(pa))
            rc = lib().hg_db_compile_ext(pa, fa, ia, ea, len(pa), ctypes.byref(self._h), err, 512)
        if rc != 0:
            raise CompileError(err.value.decode(errors="replace"))

    def tune(self, sample: bytes) -> None:
        """Re-select prefilter windows from a text sample (call before creating a Scanner); results never change."""
        if lib().hg_db_tune(self._h, sample, len(sample)) != 0:
            raise CompileError("hg_db_tune failed")

    def info(self) -> dict:
        out = HgDbInfo()
        lib().hg_db_info(self._h, ctypes.byref(out))
        return {n: getattr(out, n) for n, _ in HgDbInfo._fields_}

    def report_ids(self):
        """The bins of Scanner.count(): the distinct report ids of the set, ascending, as a uint32 numpy array (needs no GPU)."""
        import numpy as np

        n = ctypes.c_uint32()
        if lib().hg_db_report_ids(self._h, None, 0, ctypes.byref(n)) != 0:
            raise ValueError("hg_db_report_ids failed")
        out = np.zeros(n.value, dtype=np.uint32)
        lib().hg_db_report_ids(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n.value, ctypes.byref(n))
        return out

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # (module globals are gone at interpreter shutdown)
            lib().hg_db_release(self._h)
            self._h = None


@dataclass
class ScanStats:
    n_hits: int
    n_lines: int
    n_candidates: int
    n_raw_hits: int
    ms_stream: float
    ms_total: float
    reruns: int
    stream_launches: int = 1
    joiner_launches: int = 0
    joiner_tiles: int = 0
    invert_us: int = 0  # inverted scans: the invert stage alone, microseconds
    n_context: int = 0  # scans with context: the records of Scanner.context() (context and tail pieces)
    owed_after: int = 0  # ... the after-context pieces still owed past the buffer's end (the next buffer's carry_after)
    n_tail: int = 0  # ... the tail records among n_context
    context_us: int = 0  # ... the context stage alone, microseconds
    segments_us: int = 0  # scans with segments: the segment stage alone, microseconds
    n_parts: int = 0  # scans with parts: the records of Scanner.parts()
    parts_us: int = 0  # ... the parts stage alone, microseconds


@dataclass
class GatherStats:
    n_entries: int  # distinct (segment, line) of the gathered records
    n_bytes: int  # bytes of all entries
    gather_us: int  # the gather stage alone, microseconds


@dataclass
class PartLinesStats:
    n_entries: int  # one per part
    n_bytes: int  # bytes of all entries
    gather_us: int  # the parts gather alone, microseconds


@dataclass
class ValueStats:
    n_values: int  # distinct values (groups)
    n_parts: int  # parts of the scan
    n_bytes: int  # bytes of all distinct values
    values_us: int  # the values stage alone, microseconds


@dataclass
class RankStats:
    n_values: int  # kept rows
    n_distinct: int  # groups before the cut
    n_parts: int  # parts of the scan
    n_bytes: int  # bytes of the kept rows' values
    rank_us: int  # the rank stage alone, microseconds


@dataclass
class AccStats:
    n_distinct: int  # distinct values in the store after the call
    n_added: int  # of them new with this call
    n_groups: int  # this call's groups
    n_parts: int  # this call's parts
    n_parts_total: int  # parts accumulated since the last reset
    n_bytes: int  # bytes of the store's values
    store_log2: int  # the store's table
    acc_us: int  # the call alone, microseconds


@dataclass
class AccRankStats:
    n_values: int  # kept rows
    n_distinct: int  # groups before the cut
    n_parts: int  # parts accumulated since the last reset
    n_bytes: int  # bytes of the kept rows' values
    rank_us: int  # the ranking alone, microseconds


@dataclass
class CountStats:
    n_bins: int  # distinct report ids of the database
    n_records: int  # records this call counted
    counts_us: int  # the counts stage alone, microseconds
    n_seg: int = 0  # rows of segment_counts() (0 without per_segment)


class Scanner:
    """Database + workspace resident on one GPU."""

    def __init__(self, db: Database, device: int = 0):
        self.db = db
        self._h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        self._device = device
        rc = lib().hg_scanner_create(db._h, device, ctypes.byref(self._h), err, 512)
        if rc != 0:
            raise DeviceError(f"hg_scanner_create failed ({rc}): {err.value.decode(errors='replace')}")
        self._last = HgScanResult()
        self._last_ctx = HgContextResult()
        self._last_parts = HgPartsResult()
        self._last_seg = None  # (HgSegmentResult, n_seg) of the last scan, if it had segments
        self._last_segment_parts = False  # the last scan was one with segment_parts
        self._last_lines = None  # HgLinesResult of the last gather, None after a scan
        self._last_counts = None  # HgCountsResult of the last count
        self._last_part_lines = None  # (HgPartLinesResult, whole_line) of the last parts gather, None after a scan
        self._last_values = None  # HgValuesResult of the last value count, None after a scan
        self._last_rank = None  # HgRankResult of the last ranking, None after a scan
        self._last_acc_rank = None  # HgAccRankResult of the value store's last ranking, None after an accumulate or a reset (scans leave it)
        self._seg_arena = None

    def _place_segments(self, starts, ends):
        """The two offset lists as device arrays (one guarded allocation of the scanner's, grown when needed)."""
        import struct

        n = len(starts)
        if len(ends) != n:
            raise ValueError("segments: as many ends as starts")
        blob = struct.pack(f"<{2 * n}Q", *starts, *ends)
        if self._seg_arena is None or self._seg_arena.capacity < len(blob):
            if self._seg_arena is not None:
                self._seg_arena.free()
            self._seg_arena = GuardedArena(max(2 * len(blob), 1 << 16), self._device)
        ptr = self._seg_arena.place(blob)
        return ptr, ptr + 8 * n, n

    def scan(self, d_text: int, nbytes: int, buffer_size: int = 262140, line_base: int = 0, stream: int = 0, invert: bool = False,
             context: tuple[int, int] | None = None, carry_after: int = 0, tail: bool = False, segments=None, max_per_segment: int = 0, parts: bool = False,
             segment_parts: bool = False) -> ScanStats:
        """invert: the result is the line pieces without any report (grep -v; hg_scan_device_invert): n_hits of them, and
        hits() gives (line_number, HG_ID_INVERT, 0, start, len) per piece in line order.
        context = (before, after): grep -B / -A in line pieces (hg_scan_device_context).  hits() is what it is without context;
        context() gives the pieces around them.  carry_after: the owed_after of the previous buffer of a chain; tail: also
        deliver the last `before` pieces that are neither match nor context, as HG_ID_CONTEXT_TAIL records.
        With segments, context is per file (hg_scan_device_segments_context): context() gives every file's context pieces as a
        scan of the file alone would, file after file, and segment_context() says which are whose; carry_after, tail and
        line_base are refused, because nothing chains across files.
        segments = (starts, ends): the text holds many files one after the other (hg_scan_device_segments has the packing
        rule); two sequences of offsets, or (d_starts, d_ends, n) for arrays already on the device.  hits() then gives every
        file's records as a scan of the file alone would, file after file, and segments() says which are whose.
        max_per_segment: keep a file's records up to the line on which their count reaches it (0: all).
        parts: the plain scan with the matched parts of every line that has a hit (grep -o over all expressions;
        hg_scan_device_parts has the definition).  hits() is what it is without; parts() gives the parts.  Not combined with
        invert, context or segments (ValueError), and ValueError with the reason for a database the stage is not offered for.
        segment_parts: with segments, the matched parts per file (hg_scan_device_segments_parts): hits() and segments() are what
        they are without; parts() gives every file's parts as scan(parts=True) of the file alone would, restricted to the lines
        the file keeps, file after file, and segment_parts() says which are whose.  It needs segments and is not combined with
        invert, context, carry_after, tail, line_base or parts (ValueError)."""
        if parts and (invert or context is not None or carry_after or tail or segments is not None):
            raise ValueError("parts: not combined with invert, context or segments (with segments: segment_parts=True)")
        if segment_parts and segments is None:
            raise ValueError("segment_parts: needs segments")
        if segment_parts and (invert or context is not None or carry_after or tail or line_base or parts):
            raise ValueError("segment_parts: not combined with invert, context, carry_after, tail, line_base or parts")
        res = HgScanResult()
        pres = HgPartsResult()
        cres = HgContextResult()
        sres = HgSegmentResult()
        self._last_lines = None
        self._last_part_lines = None
        self._last_values = None
        self._last_rank = None
        self._last_seg = None
        self._last_segment_parts = False
        if segments is not None:
            if carry_after or tail or line_base:
                raise ValueError("segments: carry_after, tail and line_base are not supported (nothing chains across files)")
            d_starts, d_ends, n_seg = segments if len(segments) == 3 else self._place_segments(*segments)
            seg = HgSegments(d_starts, d_ends, n_seg, max_per_segment)
            if segment_parts:
                name = "hg_scan_device_segments_parts"
                spres = HgSegmentPartsResult()
                rc = lib().hg_scan_device_segments_parts(self._h, ctypes.c_void_p(d_text), nbytes, buffer_size, ctypes.c_void_p(stream), ctypes.byref(seg), ctypes.byref(res),
                                                         ctypes.byref(sres), ctypes.byref(pres), ctypes.byref(spres))
            elif context is not None:
                before, after = context
                name = "hg_scan_device_segments_context"
                rc = lib().hg_scan_device_segments_context(self._h, ctypes.c_void_p(d_text), nbytes, buffer_size, ctypes.c_void_p(stream), ctypes.byref(seg), before, after,
                                                           1 if invert else 0, ctypes.byref(res), ctypes.byref(sres), ctypes.byref(cres))
            else:
                name = "hg_scan_device_segments"
                rc = lib().hg_scan_device_segments(self._h, ctypes.c_void_p(d_text), nbytes, buffer_size, ctypes.c_void_p(stream), ctypes.byref(seg), 1 if invert else 0,
                                                   ctypes.byref(res), ctypes.byref(sres))
            if rc == -1:  # HG_ERR_ARG: nothing was scanned
                self._last = HgScanResult()
                self._last_ctx = HgContextResult()
                self._last_parts = HgPartsResult()
                raise ValueError(f"{name}: {lib().hg_scanner_error(self._h).decode(errors='replace')}")
            if rc == 0:
                self._last_seg = (sres, n_seg)
                self._last_segment_parts = segment_parts
        elif context is not None or carry_after or tail:
            before, after = context or (0, 0)
            name = "hg_scan_device_context"
            ctx = HgContext(before, after, carry_after, HG_CONTEXT_TAIL if tail else 0)
            rc = lib().hg_scan_device_context(self._h, ctypes.c_void_p(d_text), nbytes, buffer_size, line_base, ctypes.c_void_p(stream), ctypes.byref(ctx),
                                              1 if invert else 0, ctypes.byref(res), ctypes.byref(cres))
        elif parts:
            name = "hg_scan_device_parts"
            rc = lib().hg_scan_device_parts(self._h, ctypes.c_void_p(d_text), nbytes, buffer_size, line_base, ctypes.c_void_p(stream), ctypes.byref(res), ctypes.byref(pres))
            if rc == -1:  # HG_ERR_ARG: nothing was scanned
                self._last = HgScanResult()
                self._last_parts = HgPartsResult()
                raise ValueError(f"{name}: {lib().hg_scanner_error(self._h).decode(errors='replace')}")
        else:
            name = "hg_scan_device_invert" if invert else "hg_scan_device"
            rc = getattr(lib(), name)(self._h, ctypes.c_void_p(d_text), nbytes, buffer_size, line_base, ctypes.c_void_p(stream), ctypes.byref(res))
        if rc != 0:
            raise DeviceError(f"{name} failed ({rc}): {lib().hg_scanner_error(self._h).decode(errors='replace')}")
        self._last = res
        self._last_ctx = cres
        self._last_parts = pres
        return ScanStats(res.n_hits, res.n_lines, res.n_candidates, res.n_raw_hits, res.ms_stream, res.ms_total, res.reruns, res.stream_launches, res.joiner_launches, res.joiner_tiles,
                         res.invert_us, cres.n_context, cres.owed_after, cres.n_tail, cres.context_us, sres.segments_us, pres.n_parts, pres.parts_us)

    def segments(self):
        """The per-file arrays of the last scan with segments, as uint64 / uint32 numpy arrays: a dict with record_segment (one
        per record of hits()), first_record (n + 1: file s owns hits()[first_record[s]:first_record[s + 1]]), n_lines and
        n_selected (n each)."""
        import numpy as np

        if self._last_seg is None:
            raise ValueError("the last scan had no segments")
        _, n_seg = self._last_seg
        out = {"record_segment": np.zeros(self._last.n_hits, dtype=np.uint32), "first_record": np.zeros(n_seg + 1, dtype=np.uint64),
               "n_lines": np.zeros(n_seg, dtype=np.uint64), "n_selected": np.zeros(n_seg, dtype=np.uint64)}
        p64 = ctypes.POINTER(ctypes.c_uint64)
        rc = lib().hg_copy_segments(self._h, out["record_segment"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), out["first_record"].ctypes.data_as(p64),
                                    out["n_lines"].ctypes.data_as(p64), out["n_selected"].ctypes.data_as(p64))
        if rc != 0:
            raise DeviceError(f"hg_copy_segments failed ({rc})")
        return out

    def segment_context(self):
        """Whose the context records of the last scan with segments and context are, as numpy arrays: a dict with
        context_segment (uint32, one per record of context()) and first_context (uint64, n + 1: file s owns
        context()[first_context[s]:first_context[s + 1]]).  ValueError after a scan of any other kind."""
        import numpy as np

        if self._last_seg is None:
            raise ValueError("the last scan had no segments")
        _, n_seg = self._last_seg
        out = {"context_segment": np.zeros(self._last_ctx.n_context, dtype=np.uint32), "first_context": np.zeros(n_seg + 1, dtype=np.uint64)}
        rc = lib().hg_copy_segment_context(self._h, out["context_segment"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                           out["first_context"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
        if rc == -1:
            raise ValueError("the last scan had segments without context")
        if rc != 0:
            raise DeviceError(f"hg_copy_segment_context failed ({rc})")
        return out

    def segment_parts(self):
        """Whose the parts of the last scan with segments and segment_parts are, as numpy arrays: a dict with part_segment
        (uint32, one per record of parts()) and first_part (uint64, n + 1: file s owns parts()[first_part[s]:first_part[s + 1]]).
        ValueError after a scan of any other kind."""
        import numpy as np

        if self._last_seg is None or not self._last_segment_parts:
            raise ValueError("the last scan was not one with segments and segment_parts")
        _, n_seg = self._last_seg
        out = {"part_segment": np.zeros(self._last_parts.n_parts, dtype=np.uint32), "first_part": np.zeros(n_seg + 1, dtype=np.uint64)}
        rc = lib().hg_copy_segment_parts(self._h, out["part_segment"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                         out["first_part"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
        if rc == -1:
            raise ValueError("the last scan was not one with segments and segment_parts")
        if rc != 0:
            raise DeviceError(f"hg_copy_segment_parts failed ({rc})")
        return out

    def gather(self, d_text: int, nbytes: int, context: bool = False, terminate: bool = False, number: bool = False, separator: bool = False,
               stream: int = 0) -> GatherStats:
        """The lines themselves (hg_gather_lines): the scanned bytes of every line piece the last scan left a record for, one
        entry per distinct (file, line) in the records' order, gathered on the GPU into one device buffer.  d_text and nbytes
        must be the last scan's.  context: merge the last scan's context (and tail) pieces in, in line order; terminate: every
        entry ends in a newline; number: every entry begins with its 1-based line number and ':' (match) or '-' (context, tail);
        separator: "--\n" between entries that are not neighbours (another file, or a gap in the line numbers).
        lines(), lines_arrays() and copy_lines_to() give the result; hits(), context(), segments() ... are unchanged by it.
        ValueError with the reason when there is no scan to gather from, or d_text / nbytes are not the last scan's."""
        flags = (HG_LINES_CONTEXT if context else 0) | (HG_LINES_TERMINATE if terminate else 0) | (HG_LINES_NUMBER if number else 0) | (HG_LINES_SEPARATOR if separator else 0)
        return self._gather(d_text, nbytes, flags, stream)

    def _gather(self, d_text: int, nbytes: int, flags: int, stream: int = 0) -> GatherStats:
        res = HgLinesResult()
        self._last_lines = None
        rc = lib().hg_gather_lines(self._h, ctypes.c_void_p(d_text), nbytes, flags, ctypes.c_void_p(stream), ctypes.byref(res))
        if rc == -1:  # HG_ERR_ARG: nothing was launched
            raise ValueError(lib().hg_scanner_error(self._h).decode(errors="replace"))
        if rc != 0:
            raise DeviceError(f"hg_gather_lines failed ({rc}): {lib().hg_scanner_error(self._h).decode(errors='replace')}")
        self._last_lines = res
        return GatherStats(res.n_entries, res.n_bytes, res.gather_us)

    def lines_arrays(self):
        """The last gather as a dict: bytes (the blob), and numpy arrays entry_off (uint64, n + 1: entry j is
        bytes[entry_off[j]:entry_off[j + 1]]), line_number (uint64), kind (uint32, HG_LINE_*), and after a scan with segments
        segment (uint32) and first_entry (uint64, files + 1), else None.  ValueError without a gather since the last scan."""
        import numpy as np

        g = self._last_lines
        if g is None:
            raise ValueError("no gather since the last scan")
        n = g.n_entries
        blob = np.zeros(max(g.n_bytes, 1), dtype=np.uint8)
        out = {"entry_off": np.zeros(n + 1, dtype=np.uint64), "line_number": np.zeros(n, dtype=np.uint64), "kind": np.zeros(n, dtype=np.uint32),
               "segment": np.zeros(n, dtype=np.uint32) if g.d_segment else None, "first_entry": None}
        p8, p32, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        rc = lib().hg_copy_lines(self._h, blob.ctypes.data_as(p8), g.n_bytes, out["entry_off"].ctypes.data_as(p64), out["line_number"].ctypes.data_as(p64),
                                 out["kind"].ctypes.data_as(p32), out["segment"].ctypes.data_as(p32) if g.d_segment else None, n)
        if rc != 0:
            raise DeviceError(f"hg_copy_lines failed ({rc})")
        if g.d_first_entry:
            _, n_seg = self._last_seg
            out["first_entry"] = np.zeros(n_seg + 1, dtype=np.uint64)
            rc = lib().hg_copy_lines_first(self._h, out["first_entry"].ctypes.data_as(p64))
            if rc != 0:
                raise DeviceError(f"hg_copy_lines_first failed ({rc})")
        out["bytes"] = blob[:g.n_bytes].tobytes()
        return out

    def lines(self):
        """The last gather's entries as a list of bytes, in order."""
        a = self.lines_arrays()
        off = a["entry_off"].tolist()
        return [a["bytes"][off[j]:off[j + 1]] for j in range(len(off) - 1)]

    def copy_lines_to(self, d_dst: int, max_bytes: int, stream: int = 0) -> int:
        """Async device-to-device copy of the last gather's bytes (the first max_bytes of them); returns the number copied."""
        if self._last_lines is None:
            raise ValueError("no gather since the last scan")
        n = min(max_bytes, self._last_lines.n_bytes)
        rc = lib().hg_copy_lines_device(self._h, ctypes.c_void_p(d_dst), n, ctypes.c_void_p(stream))
        if rc != 0:
            raise DeviceError(f"hg_copy_lines_device failed ({rc})")
        return n

    def gather_parts(self, d_text: int, nbytes: int, number: bool = False, byte_offset: bool = False, terminate: bool = False, whole_line: bool = False,
                     mark: tuple[bytes, bytes] = (b"", b""), byte_base: int = 0, stream: int = 0) -> PartLinesStats:
        """The matched parts themselves (hg_gather_parts): after scan(parts=True) or scan(segment_parts=True), the bytes of every
        part, one entry per part in the parts' order, gathered on the GPU into one device buffer.  d_text and nbytes must be
        the last scan's.  number: the 1-based line number and ':' in front; byte_offset: the byte offset (byte_base + the part's
        offset in the text; file-relative after a scan with segments, where byte_base must be 0) and ':' in front; terminate:
        every entry ends in a newline (grep -o -n -b).  whole_line: the whole matching line instead, its parts between the two
        byte strings of `mark` (at most 16 bytes each; grep --color), number and byte_offset (the line's) once per line.
        part_lines(), part_lines_arrays() and copy_part_lines_to() give the result; hits(), parts(), lines(), counts() ... are
        unchanged by it.  ValueError with the reason when there are no parts to gather: no scan yet, a scan without parts,
        d_text / nbytes not the last scan's, a mark too long, byte_base after segments."""
        flags = (HG_PARTS_NUMBER if number else 0) | (HG_PARTS_BYTE_OFFSET if byte_offset else 0) | (HG_PARTS_TERMINATE if terminate else 0) | (HG_PARTS_LINE if whole_line else 0)
        return self._gather_parts(d_text, nbytes, flags, mark, byte_base, stream)

    def _gather_parts(self, d_text: int, nbytes: int, flags: int, mark=(b"", b""), byte_base: int = 0, stream: int = 0, mark_lens=None) -> PartLinesStats:
        on, off = bytes(mark[0]), bytes(mark[1])
        params = HgPartLinesParams(flags=flags, byte_base=byte_base, mark_on_len=len(on), mark_off_len=len(off))
        if mark_lens is not None:  # (the tests: lengths the bytes do not have)
            params.mark_on_len, params.mark_off_len = mark_lens
        ctypes.memmove(params.mark_on, on, min(len(on), 16))
        ctypes.memmove(params.mark_off, off, min(len(off), 16))
        res = HgPartLinesResult()
        self._last_part_lines = None
        rc = lib().hg_gather_parts(self._h, ctypes.c_void_p(d_text), nbytes, ctypes.byref(params), ctypes.c_void_p(stream), ctypes.byref(res))
        if rc == -1:  # HG_ERR_ARG: nothing was launched
            raise ValueError(lib().hg_scanner_error(self._h).decode(errors="replace"))
        if rc != 0:
            raise DeviceError(f"hg_gather_parts failed ({rc}): {lib().hg_scanner_error(self._h).decode(errors='replace')}")
        self._last_part_lines = (res, bool(flags & HG_PARTS_LINE))
        return PartLinesStats(res.n_entries, res.n_bytes, res.gather_us)

    def part_lines_arrays(self):
        """The last parts gather as a dict: bytes (the blob), and numpy arrays entry_off (uint64, n + 1: entry j is
        bytes[entry_off[j]:entry_off[j + 1]]), line_number (uint64), kind (uint32, HG_PART_FIRST | HG_PART_LAST), pattern
        (uint32, the expression index), and after a scan with segments segment (uint32) and first_entry (uint64, files + 1),
        else None.  ValueError without a parts gather since the last scan."""
        import numpy as np

        if self._last_part_lines is None:
            raise ValueError("no parts gather since the last scan")
        g = self._last_part_lines[0]
        n = g.n_entries
        blob = np.zeros(max(g.n_bytes, 1), dtype=np.uint8)
        out = {"entry_off": np.zeros(n + 1, dtype=np.uint64), "line_number": np.zeros(n, dtype=np.uint64), "kind": np.zeros(n, dtype=np.uint32),
               "pattern": np.zeros(n, dtype=np.uint32), "segment": np.zeros(n, dtype=np.uint32) if g.d_segment else None, "first_entry": None}
        p8, p32, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        rc = lib().hg_copy_part_lines(self._h, blob.ctypes.data_as(p8), g.n_bytes, out["entry_off"].ctypes.data_as(p64), out["line_number"].ctypes.data_as(p64),
                                      out["kind"].ctypes.data_as(p32), out["pattern"].ctypes.data_as(p32), out["segment"].ctypes.data_as(p32) if g.d_segment else None, n)
        if rc != 0:
            raise DeviceError(f"hg_copy_part_lines failed ({rc})")
        if g.d_first_entry:
            _, n_seg = self._last_seg
            out["first_entry"] = np.zeros(n_seg + 1, dtype=np.uint64)
            rc = lib().hg_copy_part_lines_first(self._h, out["first_entry"].ctypes.data_as(p64))
            if rc != 0:
                raise DeviceError(f"hg_copy_part_lines_first failed ({rc})")
        out["bytes"] = blob[:g.n_bytes].tobytes()
        return out

    def part_lines(self):
        """The last parts gather as a list of bytes, in order: one per part, or with whole_line one per line (the entries of
        a line joined)."""
        a = self.part_lines_arrays()
        off = a["entry_off"].tolist()
        if not self._last_part_lines[1]:
            return [a["bytes"][off[j]:off[j + 1]] for j in range(len(off) - 1)]
        firsts = [j for j, k in enumerate(a["kind"].tolist()) if k & HG_PART_FIRST] + [len(off) - 1]
        return [a["bytes"][off[lo]:off[hi]] for lo, hi in zip(firsts, firsts[1:])]

    def copy_part_lines_to(self, d_dst: int, max_bytes: int, stream: int = 0) -> int:
        """Async device-to-device copy of the last parts gather's bytes (the first max_bytes of them); returns the number copied."""
        if self._last_part_lines is None:
            raise ValueError("no parts gather since the last scan")
        n = min(max_bytes, self._last_part_lines[0].n_bytes)
        rc = lib().hg_copy_part_lines_device(self._h, ctypes.c_void_p(d_dst), n, ctypes.c_void_p(stream))
        if rc != 0:
            raise DeviceError(f"hg_copy_part_lines_device failed ({rc})")
        return n

    def count_values(self, d_text: int, nbytes: int, by_pattern: bool = False, stream: int = 0, hash_bits: int = 0, table_log2: int = 0) -> ValueStats:
        """Distinct matched parts and how often each occurs (hg_count_values; grep -o | sort | uniq -c): after scan(parts=True) or
        scan(segment_parts=True), the parts grouped by their bytes on the GPU (by_pattern: by expression index and bytes).
        d_text and nbytes must be the last scan's.  Groups come in the order of their first part; files are never part of the
        key.  hash_bits (1 .. 64, 0: 64) and table_log2 (0: from the number of parts; else 2 ** table_log2 must exceed it) are
        knobs for tests: fewer hash bits or a nearly full table give the same result, slower.  values(), values_arrays() and
        copy_values_to() give the result; hits(), parts(), part_lines(), counts() ... are unchanged by it.  ValueError with
        the reason when nothing was launched: no scan yet, a scan without parts, d_text / nbytes not the last scan's, a knob
        out of range."""
        params = HgValuesParams(flags=HG_VALUES_BY_PATTERN if by_pattern else 0, hash_bits=hash_bits, table_log2=table_log2)
        return self._count_values(d_text, nbytes, params, stream)

    def _count_values(self, d_text: int, nbytes: int, params, stream: int = 0) -> ValueStats:
        res = HgValuesResult()
        self._last_values = None
        rc = lib().hg_count_values(self._h, ctypes.c_void_p(d_text), nbytes, ctypes.byref(params) if params is not None else None, ctypes.c_void_p(stream), ctypes.byref(res))
        if rc == -1:  # HG_ERR_ARG: nothing was launched
            raise ValueError(lib().hg_scanner_error(self._h).decode(errors="replace"))
        if rc != 0:
            raise DeviceError(f"hg_count_values failed ({rc}): {lib().hg_scanner_error(self._h).decode(errors='replace')}")
        self._last_values = res
        return ValueStats(res.n_values, res.n_parts, res.n_bytes, res.values_us)

    def values_arrays(self):
        """The last value count as a dict: bytes (the blob), and numpy arrays off (uint64, n + 1: value j is
        bytes[off[j]:off[j + 1]]), count (uint64), first (uint64, the smallest part index, ascending), pattern (uint32),
        line_number (uint64) and, after a scan with segments, segment (uint32), else None.  ValueError without a value count
        since the last scan."""
        import numpy as np

        g = self._last_values
        if g is None:
            raise ValueError("no value count since the last scan")
        n = g.n_values
        blob = np.zeros(max(g.n_bytes, 1), dtype=np.uint8)
        out = {"off": np.zeros(n + 1, dtype=np.uint64), "count": np.zeros(n, dtype=np.uint64), "first": np.zeros(n, dtype=np.uint64), "pattern": np.zeros(n, dtype=np.uint32),
               "line_number": np.zeros(n, dtype=np.uint64), "segment": np.zeros(n, dtype=np.uint32) if g.d_segment else None}
        p8, p32, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        rc = lib().hg_copy_values(self._h, blob.ctypes.data_as(p8), g.n_bytes, out["off"].ctypes.data_as(p64), out["count"].ctypes.data_as(p64), out["first"].ctypes.data_as(p64),
                                  out["pattern"].ctypes.data_as(p32), out["line_number"].ctypes.data_as(p64), out["segment"].ctypes.data_as(p32) if g.d_segment else None, n)
        if rc != 0:
            raise DeviceError(f"hg_copy_values failed ({rc})")
        out["bytes"] = blob[:g.n_bytes].tobytes()
        return out

    def values(self):
        """The last value count as a list of (value_bytes, count, pattern, line_number), in the order of the values' first parts."""
        a = self.values_arrays()
        off = a["off"].tolist()
        return [(a["bytes"][off[j]:off[j + 1]], int(c), int(p), int(l)) for j, (c, p, l) in enumerate(zip(a["count"], a["pattern"], a["line_number"]))]

    def copy_values_to(self, d_dst: int, max_bytes: int, stream: int = 0) -> int:
        """Async device-to-device copy of the last value count's bytes (the first max_bytes of them); returns the number copied."""
        if self._last_values is None:
            raise ValueError("no value count since the last scan")
        n = min(max_bytes, self._last_values.n_bytes)
        rc = lib().hg_copy_values_device(self._h, ctypes.c_void_p(d_dst), n, ctypes.c_void_p(stream))
        if rc != 0:
            raise DeviceError(f"hg_copy_values_device failed ({rc})")
        return n

    def rank_values(self, d_text: int, nbytes: int, top: int = 0, per_segment: bool = False, by_pattern: bool = False, stream: int = 0, hash_bits: int = 0,
                    table_log2: int = 0) -> RankStats:
        """The matched values ranked by count and cut to the `top` most frequent on the GPU (hg_rank_values; grep -o | sort | uniq -c |
        sort -rn | head): after scan(parts=True) or scan(segment_parts=True), the parts grouped by their bytes (by_pattern: by
        expression index and bytes; per_segment: additionally by file, so that equal values in two files are two groups),
        ordered by segment (per_segment only), descending count, then first occurrence, and cut to the first `top` groups of the
        scan, or of every file with per_segment (top=0: no cut).  Only the kept rows' bytes are gathered.  d_text and nbytes
        must be the last scan's; hash_bits and table_log2 are count_values()' knobs.  ranked_values(), ranked_values_arrays(),
        ranked_segments() and copy_ranked_values_to() give the result; hits(), parts(), values(), counts(), lines() ... are
        unchanged by it.  ValueError with the reason when nothing was launched: what count_values() refuses, or per_segment
        after a scan without segments."""
        if top < 0:
            raise ValueError("top must not be negative")
        params = HgRankParams(flags=(HG_RANK_BY_PATTERN if by_pattern else 0) | (HG_RANK_PER_SEGMENT if per_segment else 0), hash_bits=hash_bits, table_log2=table_log2, top=top)
        return self._rank_values(d_text, nbytes, params, stream)

    def _rank_values(self, d_text: int, nbytes: int, params, stream: int = 0) -> RankStats:
        res = HgRankResult()
        self._last_rank = None
        rc = lib().hg_rank_values(self._h, ctypes.c_void_p(d_text), nbytes, ctypes.byref(params) if params is not None else None, ctypes.c_void_p(stream), ctypes.byref(res))
        if rc == -1:  # HG_ERR_ARG: nothing was launched
            raise ValueError(lib().hg_scanner_error(self._h).decode(errors="replace"))
        if rc != 0:
            raise DeviceError(f"hg_rank_values failed ({rc}): {lib().hg_scanner_error(self._h).decode(errors='replace')}")
        self._last_rank = res
        return RankStats(res.n_values, res.n_distinct, res.n_parts, res.n_bytes, res.rank_us)

    def ranked_values_arrays(self):
        """The last ranking as a dict: bytes (the blob), and numpy arrays off (uint64, n + 1: row j is bytes[off[j]:off[j + 1]]),
        count (uint64), first (uint64, the smallest part index), pattern (uint32), line_number (uint64) and, after a scan with
        segments, segment (uint32), else None.  ValueError without a ranking since the last scan."""
        import numpy as np

        g = self._last_rank
        if g is None:
            raise ValueError("no ranking since the last scan")
        n = g.n_values
        blob = np.zeros(max(g.n_bytes, 1), dtype=np.uint8)
        out = {"off": np.zeros(n + 1, dtype=np.uint64), "count": np.zeros(n, dtype=np.uint64), "first": np.zeros(n, dtype=np.uint64), "pattern": np.zeros(n, dtype=np.uint32),
               "line_number": np.zeros(n, dtype=np.uint64), "segment": np.zeros(n, dtype=np.uint32) if g.d_segment else None}
        p8, p32, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        rc = lib().hg_copy_ranked_values(self._h, blob.ctypes.data_as(p8), g.n_bytes, out["off"].ctypes.data_as(p64), out["count"].ctypes.data_as(p64),
                                         out["first"].ctypes.data_as(p64), out["pattern"].ctypes.data_as(p32), out["line_number"].ctypes.data_as(p64),
                                         out["segment"].ctypes.data_as(p32) if g.d_segment else None, n)
        if rc != 0:
            raise DeviceError(f"hg_copy_ranked_values failed ({rc})")
        out["bytes"] = blob[:g.n_bytes].tobytes()
        return out

    def ranked_values(self):
        """The last ranking as a list of (value_bytes, count, pattern, line_number), with the segment as a fifth element after a
        scan with segments, in the ranking's order."""
        a = self.ranked_values_arrays()
        off = a["off"].tolist()
        rows = [(a["bytes"][off[j]:off[j + 1]], int(c), int(p), int(l)) for j, (c, p, l) in enumerate(zip(a["count"], a["pattern"], a["line_number"]))]
        if a["segment"] is not None:
            rows = [r + (int(s),) for r, s in zip(rows, a["segment"])]
        return rows

    def ranked_segments(self):
        """The per-file arrays of the last ranking with per_segment=True as a dict of numpy uint64 arrays: first_value (n_seg + 1:
        file s owns rows first_value[s] .. first_value[s + 1]), seg_distinct and seg_parts (n_seg: the file's distinct values
        and its counted parts before the cut).  ValueError otherwise."""
        import numpy as np

        g = self._last_rank
        if g is None or not g.d_first_value:
            raise ValueError("no ranking with per_segment=True since the last scan")
        out = {"first_value": np.zeros(g.n_seg + 1, dtype=np.uint64), "seg_distinct": np.zeros(g.n_seg, dtype=np.uint64), "seg_parts": np.zeros(g.n_seg, dtype=np.uint64)}
        p64 = ctypes.POINTER(ctypes.c_uint64)
        rc = lib().hg_copy_ranked_segments(self._h, out["first_value"].ctypes.data_as(p64), out["seg_distinct"].ctypes.data_as(p64), out["seg_parts"].ctypes.data_as(p64))
        if rc != 0:
            raise DeviceError(f"hg_copy_ranked_segments failed ({rc})")
        return out

    def copy_ranked_values_to(self, d_dst: int, max_bytes: int, stream: int = 0) -> int:
        """Async device-to-device copy of the last ranking's bytes (the first max_bytes of them); returns the number copied."""
        if self._last_rank is None:
            raise ValueError("no ranking since the last scan")
        n = min(max_bytes, self._last_rank.n_bytes)
        rc = lib().hg_copy_ranked_values_device(self._h, ctypes.c_void_p(d_dst), n, ctypes.c_void_p(stream))
        if rc != 0:
            raise DeviceError(f"hg_copy_ranked_values_device failed ({rc})")
        return n

    def accumulate_values(self, d_text: int, nbytes: int, by_pattern: bool = False, reset: bool = False, stream: int = 0, hash_bits: int = 0, table_log2: int = 0,
                          store_log2: int = 0) -> AccStats:
        """Add the matched parts of the last scan with parts to the scanner's value store (hg_accumulate_values): a device-resident
        table of distinct values that survives scans, so that a text that arrives in many buffers (scanned in order, line_base
        chained) is grouped as the whole text would be.  by_pattern: the expression index is part of the key; reset: empty the
        store first.  by_pattern and hash_bits are fixed when a store begins.  hash_bits and table_log2 are count_values()' knobs
        for the call's own grouping; store_log2 fixes the store's table size (0: it grows on its own), for tests.
        rank_accumulated() orders and cuts the store; hits(), parts(), values(), ranked_values() ... are unchanged by it.
        ValueError with the reason when nothing was launched (what count_values() refuses; a changed by_pattern or hash_bits
        without reset); a DeviceError (-2: out of memory, an explicit store_log2 too small) leaves the store as it was."""
        params = HgAccParams(flags=(HG_ACC_BY_PATTERN if by_pattern else 0) | (HG_ACC_RESET if reset else 0), hash_bits=hash_bits, table_log2=table_log2, store_log2=store_log2)
        return self._accumulate_values(d_text, nbytes, params, stream)

    def _accumulate_values(self, d_text: int, nbytes: int, params, stream: int = 0) -> AccStats:
        res = HgAccResult()
        rc = lib().hg_accumulate_values(self._h, ctypes.c_void_p(d_text), nbytes, ctypes.byref(params) if params is not None else None, ctypes.c_void_p(stream), ctypes.byref(res))
        if rc == -1:  # HG_ERR_ARG: nothing was launched
            raise ValueError(lib().hg_scanner_error(self._h).decode(errors="replace"))
        if rc != 0:
            err = DeviceError(f"hg_accumulate_values failed ({rc}): {lib().hg_scanner_error(self._h).decode(errors='replace')}")
            err.rc = rc
            raise err
        self._last_acc_rank = None
        return AccStats(res.n_distinct, res.n_added, res.n_groups, res.n_parts, res.n_parts_total, res.n_bytes, res.store_log2, res.acc_us)

    def rank_accumulated(self, top: int = 0, order_first: bool = False, stream: int = 0) -> AccRankStats:
        """Order the value store by descending count, then first occurrence (order_first: by first occurrence only) and keep the
        first `top` groups (0: all) on the GPU (hg_rank_accumulated); only the kept rows' bytes are gathered.
        accumulated_values(), accumulated_values_arrays() and copy_accumulated_to() give the result, which stays valid until the
        next accumulate_values(), rank_accumulated() or reset_accumulated().  ValueError without an accumulation since the
        last reset."""
        if top < 0:
            raise ValueError("top must not be negative")
        res = HgAccRankResult()
        self._last_acc_rank = None
        rc = lib().hg_rank_accumulated(self._h, top, HG_ACC_ORDER_FIRST if order_first else 0, ctypes.c_void_p(stream), ctypes.byref(res))
        if rc == -1:
            raise ValueError(lib().hg_scanner_error(self._h).decode(errors="replace"))
        if rc != 0:
            raise DeviceError(f"hg_rank_accumulated failed ({rc}): {lib().hg_scanner_error(self._h).decode(errors='replace')}")
        self._last_acc_rank = res
        return AccRankStats(res.n_values, res.n_distinct, res.n_parts, res.n_bytes, res.rank_us)

    def accumulated_values_arrays(self):
        """The value store's last ranking as a dict: bytes (the blob), and numpy arrays off (uint64, n + 1: row j is
        bytes[off[j]:off[j + 1]]), count (uint64), first (uint64, the smallest ordinal: the parts of the earlier calls plus the
        part's index in its call), pattern (uint32) and line_number (uint64).  ValueError without a ranking since the last
        accumulate_values() or reset_accumulated()."""
        import numpy as np

        g = self._last_acc_rank
        if g is None:
            raise ValueError("no ranking of the value store since the last accumulation")
        n = g.n_values
        blob = np.zeros(max(g.n_bytes, 1), dtype=np.uint8)
        out = {"off": np.zeros(n + 1, dtype=np.uint64), "count": np.zeros(n, dtype=np.uint64), "first": np.zeros(n, dtype=np.uint64), "pattern": np.zeros(n, dtype=np.uint32),
               "line_number": np.zeros(n, dtype=np.uint64)}
        p8, p32, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        rc = lib().hg_copy_accumulated(self._h, blob.ctypes.data_as(p8), g.n_bytes, out["off"].ctypes.data_as(p64), out["count"].ctypes.data_as(p64),
                                       out["first"].ctypes.data_as(p64), out["pattern"].ctypes.data_as(p32), out["line_number"].ctypes.data_as(p64), n)
        if rc != 0:
            raise DeviceError(f"hg_copy_accumulated failed ({rc})")
        out["bytes"] = blob[:g.n_bytes].tobytes()
        return out

    def accumulated_values(self):
        """The value store's last ranking as a list of (value_bytes, count, pattern, line_number), in the ranking's order."""
        a = self.accumulated_values_arrays()
        off = a["off"].tolist()
        return [(a["bytes"][off[j]:off[j + 1]], int(c), int(p), int(l)) for j, (c, p, l) in enumerate(zip(a["count"], a["pattern"], a["line_number"]))]

    def copy_accumulated_to(self, d_dst: int, max_bytes: int, stream: int = 0) -> int:
        """Async device-to-device copy of the last ranking's bytes (the first max_bytes of them); returns the number copied."""
        if self._last_acc_rank is None:
            raise ValueError("no ranking of the value store since the last accumulation")
        n = min(max_bytes, self._last_acc_rank.n_bytes)
        rc = lib().hg_copy_accumulated_device(self._h, ctypes.c_void_p(d_dst), n, ctypes.c_void_p(stream))
        if rc != 0:
            raise DeviceError(f"hg_copy_accumulated_device failed ({rc})")
        return n

    def reset_accumulated(self) -> None:
        """Empty the value store (hg_reset_accumulated)."""
        self._last_acc_rank = None
        if lib().hg_reset_accumulated(self._h) != 0:
            raise DeviceError("hg_reset_accumulated failed")

    def count(self, accumulate: bool = False, per_segment: bool = False, stream: int = 0) -> CountStats:
        """Counts per report id (hg_count_records) of the last scan's records (hits(), or the surviving records of a scan with
        segments; context and parts are ignored), computed on the GPU: for every distinct report id of the database the
        records with it and the distinct (file, line) among them.  accumulate: add to the totals already on the scanner (the
        buffers of a chained scan); per_segment: after a scan with segments, also the per-file matrices of segment_counts().
        counts(), counts_arrays() and segment_counts() give the result; hits(), lines() ... are unchanged by it.  DeviceError
        with the reason when there is nothing to count: no scan yet, an inverted scan, per_segment without segments."""
        res = HgCountsResult()
        self._last_counts = None
        flags = (HG_COUNTS_ACCUMULATE if accumulate else 0) | (HG_COUNTS_PER_SEGMENT if per_segment else 0)
        rc = lib().hg_count_records(self._h, flags, ctypes.c_void_p(stream), ctypes.byref(res))
        if rc != 0:
            raise DeviceError(f"hg_count_records failed ({rc}): {lib().hg_scanner_error(self._h).decode(errors='replace')}")
        self._last_counts = res
        return CountStats(res.n_bins, res.n_records, res.counts_us, res.n_seg)

    def counts_arrays(self):
        """The last count as numpy arrays (ids uint32 ascending, n_lines uint64, n_reports uint64), one value per bin."""
        import numpy as np

        c = self._last_counts
        if c is None:
            raise ValueError("no count on this scanner")
        ids, n_lines, n_reports = np.zeros(c.n_bins, dtype=np.uint32), np.zeros(c.n_bins, dtype=np.uint64), np.zeros(c.n_bins, dtype=np.uint64)
        p64 = ctypes.POINTER(ctypes.c_uint64)
        rc = lib().hg_copy_counts(self._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n_lines.ctypes.data_as(p64), n_reports.ctypes.data_as(p64), c.n_bins)
        if rc != 0:
            raise DeviceError(f"hg_copy_counts failed ({rc})")
        return ids, n_lines, n_reports

    def counts(self):
        """The last count as {id: (n_lines, n_reports)}, every bin of the database (zeroes included)."""
        ids, n_lines, n_reports = self.counts_arrays()
        return {int(i): (int(l), int(r)) for i, l, r in zip(ids, n_lines, n_reports)}

    def segment_counts(self):
        """The per-file matrices of the last count(per_segment=True): (lines, reports), uint32 numpy arrays of shape
        (n_seg, n_bins); the columns are the bins of counts_arrays()."""
        import numpy as np

        c = self._last_counts
        if c is None or not c.d_seg_lines:
            raise ValueError("no count with per_segment since the last scan")
        lines, reports = np.zeros((c.n_seg, c.n_bins), dtype=np.uint32), np.zeros((c.n_seg, c.n_bins), dtype=np.uint32)
        p32 = ctypes.POINTER(ctypes.c_uint32)
        rc = lib().hg_copy_segment_counts(self._h, lines.ctypes.data_as(p32), reports.ctypes.data_as(p32), 0, c.n_seg)
        if rc != 0:
            raise DeviceError(f"hg_copy_segment_counts failed ({rc}): {lib().hg_scanner_error(self._h).decode(errors='replace')}")
        return lines, reports

    def context(self, limit: int | None = None):
        """Last scan's context records as a list of (line_number, HG_ID_CONTEXT | HG_ID_CONTEXT_TAIL, 0, start, len), in line
        order; empty after a scan without context."""
        n = self._last_ctx.n_context if limit is None else min(limit, self._last_ctx.n_context)
        if not n:
            return []
        hits = (HgHit * n)()
        aux = (HgHitAux * n)()
        rc = lib().hg_copy_context(self._h, hits, aux, n)
        if rc != 0:
            raise DeviceError(f"hg_copy_context failed ({rc})")
        return [(hits[i].line_number, hits[i].id, hits[i].to, aux[i].start, aux[i].len) for i in range(n)]

    def parts(self, limit: int | None = None):
        """Last scan's matched parts as a list of (line_number, from, to, pattern), ordered by (line_number, from): the bytes
        [from, to) of the line's scanned bytes, and the index of the expression; empty after a scan without parts."""
        n = self._last_parts.n_parts if limit is None else min(limit, self._last_parts.n_parts)
        if not n:
            return []
        recs = (HgPart * n)()
        pattern = (ctypes.c_uint32 * n)()
        rc = lib().hg_copy_parts(self._h, recs, pattern, n)
        if rc != 0:
            raise DeviceError(f"hg_copy_parts failed ({rc})")
        return [(recs[i].line_number, recs[i].from_, recs[i].to, pattern[i]) for i in range(n)]

    def copy_parts_to(self, d_dst: int, limit: int, stream: int = 0) -> int:
        """Device-to-device copy of up to `limit` part records (16 B each: line_number, from, to) into d_dst; returns the count."""
        n = min(limit, self._last_parts.n_parts)
        rc = lib().hg_copy_parts_device(self._h, ctypes.c_void_p(d_dst), n, ctypes.c_void_p(stream))
        if rc != 0:
            raise DeviceError(f"hg_copy_parts_device failed ({rc})")
        return n

    @property
    def d_hits(self) -> int:
        """Device pointer of the last scan's hit records (16 B each)."""
        return self._last.d_hits or 0

    def hits(self, limit: int | None = None):
        """Last scan's hits as a list of (line_number, id, to, start, len)."""
        n = self._last.n_hits if limit is None else min(limit, self._last.n_hits)
        if not n:
            return []
        hits = (HgHit * n)()
        aux = (HgHitAux * n)()
        rc = lib().hg_copy_hits(self._h, hits, aux, n)
        if rc != 0:
            raise DeviceError(f"hg_copy_hits failed ({rc})")
        return [(hits[i].line_number, hits[i].id, hits[i].to, aux[i].start, aux[i].len) for i in range(n)]

    def _hit_records(self):
        """Last scan's hit and aux records as two numpy structured arrays (the layouts of hg_hit_t and hg_hit_aux_t)."""
        import numpy as np

        n = self._last.n_hits
        hits = np.zeros(n, dtype=[("line_number", "<u8"), ("id", "<u4"), ("to", "<u4")])
        aux = np.zeros(n, dtype=[("start", "<u8"), ("len", "<u4"), ("pattern", "<u4")])
        if n:
            rc = lib().hg_copy_hits(self._h, hits.ctypes.data_as(ctypes.POINTER(HgHit)), aux.ctypes.data_as(ctypes.POINTER(HgHitAux)), n)
            if rc != 0:
                raise DeviceError(f"hg_copy_hits failed ({rc})")
        return hits, aux

    def hits_array(self):
        """Last scan's hits as a uint64 numpy array [n_hits, 5], the columns of hits(), without one Python tuple per hit."""
        import numpy as np

        hits, aux = self._hit_records()
        return np.stack([hits["line_number"], hits["id"], hits["to"], aux["start"], aux["len"]], axis=1).astype(np.uint64)

    def hit_patterns(self):
        """The expression index (hg_hit_aux_t.pattern) of each of the last scan's hits, in the order of hits(), as a uint32 numpy array."""
        return self._hit_records()[1]["pattern"].copy()

    def finalize_info(self, fill: bool = False) -> dict:
        """What the finalize stage of the last pass did (hg_debug_finalize_info): path (one of FIN_PATHS), fin_shift, fin_nb,
        fin_cap, id_bits, to_bits, early_buckets, early_beside_stream, scan_blocks, left_bucketed; with fill=True also "fill", the raw reports of
        every bucket as a uint32 numpy array (empty unless the pass was bucketed), read from the device now."""
        import numpy as np

        info = HgFinalizeInfo()
        rc = lib().hg_debug_finalize_info(self._h, ctypes.byref(info), None, 0)
        levels = np.zeros(info.fin_nb if fill and rc == 0 else 0, dtype=np.uint32)
        if rc == 0 and fill and len(levels):
            rc = lib().hg_debug_finalize_info(self._h, ctypes.byref(info), levels.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(levels))
        if rc != 0:
            raise DeviceError(f"hg_debug_finalize_info failed ({rc})")
        out = {n: getattr(info, n) for n, _ in HgFinalizeInfo._fields_ if n not in ("n_fill", "reserved")}
        out["path"] = FIN_PATHS[info.path]
        out["left_bucketed"] = bool(info.left_bucketed)
        if fill:
            out["fill"] = levels[:info.n_fill]
        return out

    def copy_hits_to(self, d_dst: int, limit: int, stream: int = 0) -> int:
        """Async device-to-device copy of the last scan's hit records (16 B each); returns the number copied."""
        n = min(limit, self._last.n_hits)
        rc = lib().hg_copy_hits_device(self._h, ctypes.c_void_p(d_dst), n, ctypes.c_void_p(stream))
        if rc != 0:
            raise DeviceError(f"hg_copy_hits_device failed ({rc})")
        return n

    def hit_starts(self, limit: int | None = None):
        """Start of match of the last scan's hits as a uint32 numpy array, in the order of hits(), with the origin of `to`
        (offsets inside the scanned bytes): the leftmost start for expressions compiled with HS_FLAG_SOM_LEFTMOST, 0 for the
        others."""
        import numpy as np

        n = self._last.n_hits if limit is None else min(limit, self._last.n_hits)
        out = np.zeros(n, dtype=np.uint32)
        if n:
            rc = lib().hg_copy_hit_starts(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n)
            if rc != 0:
                raise DeviceError(f"hg_copy_hit_starts failed ({rc})")
        return out

    def copy_hit_starts_to(self, d_dst: int, limit: int, stream: int = 0) -> int:
        """Async device-to-device copy of the last scan's hit starts (4 B each); returns the number copied."""
        n = min(limit, self._last.n_hits)
        rc = lib().hg_copy_hit_starts_device(self._h, ctypes.c_void_p(d_dst), n, ctypes.c_void_p(stream))
        if rc != 0:
            raise DeviceError(f"hg_copy_hit_starts_device failed ({rc})")
        return n

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # (module globals are gone at interpreter shutdown)
            lib().hg_scanner_destroy(self._h)
            self._h = None
            if getattr(self, "_seg_arena", None) is not None:
                self._seg_arena.free()
                self._seg_arena = None


def _spec(seed: int, first_block: int, hit_per_million: int, needles):
    blob = b"".join(needles)
    offs = [0]
    for n in needles:
        offs.append(offs[-1] + len(n))
    off_arr = (ctypes.c_uint32 * len(offs))(*offs)
    spec = HgSynthSpec(seed, first_block, hit_per_million, len(needles), blob, off_arr)
    return spec, (blob, off_arr)


def synth_device(d_text: int, nbytes: int, seed: int, needles, hit_per_million: int, first_block: int = 0, device: int = 0, stream: int = 0) -> None:
    """Fill nbytes of device memory with the deterministic synthetic log (see csrc/hg_synth.h)."""
    spec, _keep = _spec(seed, first_block, hit_per_million, needles)
    rc = lib().hg_synth_device(ctypes.c_void_p(d_text), nbytes, ctypes.byref(spec), device, ctypes.c_void_p(stream))
    if rc != 0:
        raise DeviceError(f"hg_synth_device failed ({rc})")


def synth_host(nbytes: int, seed: int, needles, hit_per_million: int, first_block: int = 0) -> bytes:
    """The same bytes produced on the host (needs no GPU)."""
    spec, _keep = _spec(seed, first_block, hit_per_million, needles)
    buf = ctypes.create_string_buffer(nbytes)
    rc = lib().hg_synth_host(buf, nbytes, ctypes.byref(spec))
    if rc != 0:
        raise RuntimeError(f"hg_synth_host failed ({rc})")
    return buf.raw


class GuardedArena:
    """Device memory whose END is followed by unmapped address space (hg_debug_alloc_guarded).  place(data) puts the bytes
    so that they end (rounded up to 16) exactly at that edge and returns the device pointer: a kernel that reads past the
    text faults instead of passing silently.  One arena serves many texts — it is mapped once (re-mapping the same
    addresses per text showed stale reads on this stack)."""

    def __init__(self, capacity: int, device: int = 0):
        self.capacity = (max(capacity, 16) + 15) & ~15
        self._ptr = ctypes.c_void_p()
        self._guard = ctypes.c_void_p()
        rc = lib().hg_debug_alloc_guarded(self.capacity, device, ctypes.byref(self._ptr), ctypes.byref(self._guard))
        if rc != 0:
            raise DeviceError(f"hg_debug_alloc_guarded failed ({rc})")

    def place(self, data: bytes) -> int:
        usable = (len(data) + 15) & ~15
        if usable > self.capacity:
            raise ValueError("text larger than the arena")
        ptr = self._ptr.value + self.capacity - usable
        if data and lib().hg_debug_upload(ctypes.c_void_p(ptr), data, len(data)) != 0:
            raise DeviceError("hg_debug_upload failed")
        return ptr

    def tail(self, nbytes: int) -> bytes:
        """The bytes between the end of a text of `nbytes` placed last and the edge (whatever the memory held before)."""
        n = ((nbytes + 15) & ~15) - nbytes
        out = ctypes.create_string_buffer(max(n, 1))
        if n and lib().hg_debug_download(out, ctypes.c_void_p(self._ptr.value + self.capacity - n), n) != 0:
            raise DeviceError("hg_debug_download failed")
        return out.raw[:n]

    def free(self) -> None:
        if getattr(self, "_guard", None):
            lib().hg_debug_free_guarded(self._guard)
            self._guard = None

    def __del__(self):
        if lib is not None:
            self.free()


def faceb_stats() -> dict:
    """Counters of the file API's caches (hg_faceb_stats)."""
    out = (ctypes.c_uint64 * 8)()
    lib().hg_faceb_stats(out)
    names = ("db_cache_hits", "db_cache_misses", "db_cache_entries", "tunes", "contexts_created", "contexts_reused", "contexts_rebound", "contexts_alive")
    return dict(zip(names, (int(v) for v in out)))


def faceb_next_device(ndev: int) -> int:
    return lib().hg_faceb_next_device(ndev)


# ------------------------------------------------------------------------------------------------ stream mode ------
HS_MODE_BLOCK, HS_MODE_STREAM = 1, 2
HS_MODE_SOM_HORIZON_LARGE, HS_MODE_SOM_HORIZON_MEDIUM, HS_MODE_SOM_HORIZON_SMALL = 1 << 24, 1 << 25, 1 << 26
HS_OFFSET_PAST_HORIZON = (1 << 64) - 1
SOM_HORIZONS = {"large": HS_MODE_SOM_HORIZON_LARGE, "medium": HS_MODE_SOM_HORIZON_MEDIUM, "small": HS_MODE_SOM_HORIZON_SMALL}
HS_SUCCESS, HS_INVALID, HS_NOMEM, HS_SCAN_TERMINATED, HS_COMPILER_ERROR, HS_DB_MODE_ERROR = 0, -1, -2, -3, -4, -7
HG_STREAM_ITEM_LAST = 1


class HsCompileError(ctypes.Structure):
    _fields_ = [("message", ctypes.c_char_p), ("expression", ctypes.c_int)]


MATCH_EVENT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_void_p)
STREAM_EVENT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_void_p)
_face_a_configured = False


def face_a() -> ctypes.CDLL:
    """The library with Face A's prototypes (hs_*: block and stream mode, hg_scan_stream_batch, hg_scan_blocks)."""
    global _face_a_configured
    l = lib()
    if not _face_a_configured:
        vp, u = ctypes.c_void_p, ctypes.c_uint
        l.hs_compile_ext_multi.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(u), ctypes.POINTER(u), ctypes.POINTER(ctypes.POINTER(utils.ExprExt)),
                                           u, u, vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.POINTER(HsCompileError))]
        l.hs_free_compile_error.argtypes = [ctypes.POINTER(HsCompileError)]
        l.hs_free_database.argtypes = [vp]
        l.hs_alloc_scratch.argtypes = [vp, ctypes.POINTER(vp)]
        l.hs_free_scratch.argtypes = [vp]
        l.hs_scan.argtypes = [vp, ctypes.c_char_p, u, u, vp, MATCH_EVENT, vp]
        l.hs_open_stream.argtypes = [vp, u, ctypes.POINTER(vp)]
        l.hs_scan_stream.argtypes = [vp, ctypes.c_char_p, u, u, vp, MATCH_EVENT, vp]
        l.hs_close_stream.argtypes = [vp, vp, MATCH_EVENT, vp]
        l.hs_reset_stream.argtypes = [vp, u, vp, MATCH_EVENT, vp]
        l.hs_copy_stream.argtypes = [ctypes.POINTER(vp), vp]
        l.hs_stream_size.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
        l.hg_scan_stream_batch.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(u), ctypes.POINTER(u), u, vp, STREAM_EVENT, vp]
        if hasattr(l, "hg_scan_blocks"):  # (absent from a build before the batched block scan: tools/block_batch_bench.py --lib)
            l.hg_scan_blocks.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(u), u, vp, STREAM_EVENT, vp]
        _face_a_configured = True
    return l


def hs_compile(patterns, flags=None, ids=None, ext=None, mode: int = HS_MODE_STREAM):
    """hs_compile_ext_multi: (database handle, None) or (None, (message, expression index))."""
    pa, fa, ia = utils.prepare_patterns(list(patterns), flags=list(flags or ()), ids=list(ids or ()))
    ea = utils.ext_array(ext, len(pa)) if ext is not None else None
    h = ctypes.c_void_p()
    err = ctypes.POINTER(HsCompileError)()
    rc = face_a().hs_compile_ext_multi(pa, fa, ia, ea, len(pa), mode, None, ctypes.byref(h), ctypes.byref(err))
    if rc == HS_SUCCESS:
        return h, None
    msg = (err.contents.message.decode(errors="replace"), err.contents.expression) if err else ("", -1)
    face_a().hs_free_compile_error(err)
    return None, msg


class StreamDatabase:
    """Expressions compiled for stream mode (hs_compile_ext_multi with HS_MODE_STREAM; include/hypergrep_amd.h has the
    contract).  It owns ONE scratch, so a StreamDatabase and its streams must not be used from several threads at once.
    som_horizon: None, or "large" / "medium" / "small" (HS_MODE_SOM_HORIZON_*: start of match for the expressions with
    HS_FLAG_SOM_LEFTMOST); with a horizon, reports are (id, from, to) triples, else (id, to) pairs."""

    def __init__(self, patterns, flags=None, ids=None, ext=None, device: int | None = None, som_horizon: str | None = None):
        if som_horizon is not None and som_horizon not in SOM_HORIZONS:
            raise ValueError(f"som_horizon must be None or one of {sorted(SOM_HORIZONS)}")
        self.som = som_horizon is not None
        h, err = hs_compile(patterns, flags, ids, ext, HS_MODE_STREAM | (SOM_HORIZONS[som_horizon] if self.som else 0))
        if err:
            raise CompileError(err[0])
        self._h = h
        self._scratch = ctypes.c_void_p()
        if face_a().hs_alloc_scratch(self._h, ctypes.byref(self._scratch)) != HS_SUCCESS:
            raise DeviceError("hs_alloc_scratch failed")

    def open(self) -> "Stream":
        return Stream(self)

    def stream_size(self) -> int:
        n = ctypes.c_size_t()
        if face_a().hs_stream_size(self._h, ctypes.byref(n)) != HS_SUCCESS:
            raise DeviceError("hs_stream_size failed")
        return n.value

    def scan_streams(self, items, last=None):
        """items: [(Stream, bytes)], each stream at most once; last: one bool per item (end of that stream's data: its
        end-of-data reports, then a reset).  One hg_scan_stream_batch call; [[(id, to)] per item] ((id, from, to) with a
        horizon)."""
        items = list(items)
        n = len(items)
        out = [[] for _ in range(n)]
        if n == 0:
            return out
        som = self.som

        def on_event(item, rid, frm, to, _flags, _ctx):
            out[item].append((rid, frm, to) if som else (rid, to))
            return 0

        cb = STREAM_EVENT(on_event)
        streams = (ctypes.c_void_p * n)(*[s._require() for s, _ in items])
        datas = (ctypes.c_char_p * n)(*[bytes(d) for _, d in items])
        lengths = (ctypes.c_uint * n)(*[len(d) for _, d in items])
        flags = (ctypes.c_uint * n)(*[HG_STREAM_ITEM_LAST if (last and last[i]) else 0 for i in range(n)])
        rc = face_a().hg_scan_stream_batch(streams, datas, lengths, flags, n, self._scratch, cb, None)
        if rc not in (HS_SUCCESS, HS_SCAN_TERMINATED):
            raise DeviceError(f"hg_scan_stream_batch returned {rc}")
        return out

    def __del__(self):
        if lib is None:
            return
        if getattr(self, "_scratch", None):
            face_a().hs_free_scratch(self._scratch)
            self._scratch = None
        if getattr(self, "_h", None):
            face_a().hs_free_database(self._h)
            self._h = None


class BlockDatabase:
    """Expressions compiled for block mode (hs_compile_ext_multi with HS_MODE_BLOCK) with ONE scratch, so it must not be used
    from several threads at once.  scan(data) is hs_scan; scan_blocks(items) is hg_scan_blocks: many independent buffers in
    one call, each scanned as a block of its own (include/hypergrep_amd.h, batched block scan).  Reports are (id, to) pairs,
    (id, from, to) triples when the set has HS_FLAG_SOM_LEFTMOST expressions.  device: None or the GPU's index; hs_alloc_scratch
    reads it from HYPERGREP_DEVICE, so an index is put there for the allocation (and the variable restored)."""

    def __init__(self, patterns, flags=None, ids=None, ext=None, device: int | None = None):
        pats = list(patterns)
        fl = list(flags or ())
        self.som = any(f & HS_FLAG_SOM_LEFTMOST for f in fl)
        h, err = hs_compile(pats, fl, ids, ext, HS_MODE_BLOCK)
        if err:
            raise CompileError(err[0])
        self._h = h
        self._scratch = ctypes.c_void_p()
        import os

        before = os.environ.get("HYPERGREP_DEVICE")
        if device is not None:
            os.environ["HYPERGREP_DEVICE"] = str(int(device))
        try:
            rc = face_a().hs_alloc_scratch(self._h, ctypes.byref(self._scratch))
        finally:
            if device is not None:
                if before is None:
                    del os.environ["HYPERGREP_DEVICE"]
                else:
                    os.environ["HYPERGREP_DEVICE"] = before
        if rc != HS_SUCCESS:
            raise DeviceError("hs_alloc_scratch failed")

    def scan(self, data: bytes):
        """hs_scan of one buffer: its reports in (to, id) order."""
        out = []
        som = self.som

        def on_event(rid, frm, to, _flags, _ctx):
            out.append((rid, frm, to) if som else (rid, to))
            return 0

        rc = face_a().hs_scan(self._h, bytes(data), len(data), 0, self._scratch, MATCH_EVENT(on_event), None)
        if rc not in (HS_SUCCESS, HS_SCAN_TERMINATED):
            raise DeviceError(f"hs_scan returned {rc}")
        return out

    def scan_blocks(self, items):
        """One hg_scan_blocks call over items (bytes each): [reports of item i, as scan(items[i]) gives them]."""
        items = [bytes(d) for d in items]
        n = len(items)
        out = [[] for _ in range(n)]
        if n == 0:
            return out
        som = self.som

        def on_event(item, rid, frm, to, _flags, _ctx):
            out[item].append((rid, frm, to) if som else (rid, to))
            return 0

        datas = (ctypes.c_char_p * n)(*items)
        lengths = (ctypes.c_uint * n)(*[len(d) for d in items])
        rc = face_a().hg_scan_blocks(self._h, datas, lengths, n, self._scratch, STREAM_EVENT(on_event), None)
        if rc not in (HS_SUCCESS, HS_SCAN_TERMINATED):
            raise DeviceError(f"hg_scan_blocks returned {rc}")
        return out

    def __del__(self):
        if lib is None:
            return
        if getattr(self, "_scratch", None):
            face_a().hs_free_scratch(self._scratch)
            self._scratch = None
        if getattr(self, "_h", None):
            face_a().hs_free_database(self._h)
            self._h = None


class Stream:
    """One open stream of a StreamDatabase: scan() takes the next write, close() ends the data."""

    def __init__(self, db: StreamDatabase, handle=None):
        self.db = db
        self._h = handle
        if handle is None:
            self._h = ctypes.c_void_p()
            if face_a().hs_open_stream(db._h, 0, ctypes.byref(self._h)) != HS_SUCCESS:
                raise DeviceError("hs_open_stream failed")

    def _require(self):
        if not self._h:
            raise ValueError("stream is closed")
        return self._h

    def _call(self, fn, *args):
        out = []
        som = self.db.som

        def on_event(rid, frm, to, _flags, _ctx):
            out.append((rid, frm, to) if som else (rid, to))
            return 0

        rc = fn(*args, MATCH_EVENT(on_event), None)
        if rc not in (HS_SUCCESS, HS_SCAN_TERMINATED):
            raise DeviceError(f"{fn.__name__} returned {rc}")
        return out

    def scan(self, data: bytes):
        """The next write: [(id, to)] delivered by it (to = stream offset; (id, from, to) with a horizon)."""
        return self._call(face_a().hs_scan_stream, self._require(), bytes(data), len(data), 0, self.db._scratch)

    def reset(self):
        """The end-of-data reports, then the stream is as freshly opened."""
        return self._call(face_a().hs_reset_stream, self._require(), 0, self.db._scratch)

    def copy(self) -> "Stream":
        h = ctypes.c_void_p()
        if face_a().hs_copy_stream(ctypes.byref(h), self._require()) != HS_SUCCESS:
            raise DeviceError("hs_copy_stream failed")
        return Stream(self.db, h)

    def close(self):
        """The end-of-data reports; the stream is freed."""
        out = self._call(face_a().hs_close_stream, self._require(), self.db._scratch)
        self._h = None
        return out

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            face_a().hs_close_stream(self._h, None, MATCH_EVENT(), None)
            self._h = None
