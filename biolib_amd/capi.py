"""ctypes binding of the C ABI in include/biolib_amd.h (biolib_amd/lib/libbiolib_amd.so).

There is no CPU fallback: if the HIP library is missing or no gfx950 device is visible,
loading / context creation raises.  (Build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C biolib_amd/csrc`.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BIOLIB_AMD_LIB", os.path.join(_HERE, "lib", "libbiolib_amd.so"))  # override: A/B builds only

BL_OK, BL_ERR_INVALID, BL_ERR_HIP, BL_ERR_OOM, BL_ERR_CAPACITY, BL_ERR_NO_DEVICE, BL_ERR_INTERNAL, BL_ERR_IO = 0, -1, -2, -3, -4, -5, -6, -7
FLAG_CANONICAL, FLAG_DROP_LAST, FLAG_SYNC = 1, 2, 4

# every symbol include/biolib_amd.h declares (tests check the library exports exactly these)
SYMBOLS = [
    "bl_last_error", "bl_version", "bl_device_count", "bl_ctx_create", "bl_ctx_destroy", "bl_ctx_set_stream", "bl_ctx_use_own_streams", "bl_ctx_sync",
    "bl_batch_upload", "bl_batch_upload_reads", "bl_batch_from_device", "bl_batch_synth", "bl_batch_destroy", "bl_batch_n_bases", "bl_batch_n_seqs",
    "bl_batch_device_bases", "bl_batch_download", "bl_batch_set_origin", "bl_batch_origin", "bl_scan_kmers", "bl_scan_minimizers", "bl_scan_hash_sample", "bl_scan_super_kmers", "bl_scan_super_kmer_records", "bl_scan_syncmers", "bl_sort_unique_u64", "bl_jaccard_sorted_u64", "bl_partition_u64", "bl_sort_u64", "bl_count_sorted_u64", "bl_probe_hbm", "bl_clock_probe_start", "bl_clock_probe_finish", "bl_ctx_set_lanes", "bl_pack_super_kmers", "bl_count_super_kmers", "bl_partition_records", "bl_expand_super_kmers",
    "bl_ctx_last_scan_ms", "bl_ctx_set_exact_windows", "bl_ctx_set_option", "bl_ctx_kernel_timing", "bl_ctx_kernel_time", "bl_ctx_mark", "bl_ctx_mark_times", "bl_ctx_last_scan_kernels", "bl_scan_kernel_names", "bl_reader_open", "bl_reader_open_threads", "bl_reader_kind", "bl_reader_next_text", "bl_reader_next_batch_device", "bl_reader_close", "bl_reader_next_record",
    "bl_reader_next_batch", "bl_reader_last_batch", "bl_reader_last_name", "bl_batch_from_text", "bl_run_file_name", "bl_write_run_u64", "bl_write_vector_u64", "bl_file_count_u64", "bl_read_file_u64_host", "bl_read_file_u64", "bl_merge_runs_u64", "bl_count_allreduce",
    "bl_device_alloc", "bl_device_free", "bl_copy_to_host", "bl_copy_to_device", "bl_hash64_u64", "bl_bgzf_walk", "bl_bgzf_inflate", "bl_host_alloc", "bl_host_free", "bl_reader_open_shard", "bl_reader_shard_range",
    "bl_scan_kmers128", "bl_scan_hash_sample128", "bl_hash64_u128", "bl_scan_syncmers128", "bl_scan_minimizers128",
    "bl_scan_super_kmer_records128", "bl_pack_super_kmers128", "bl_partition_records128", "bl_expand_super_kmers128", "bl_count_super_kmers128",
    "bl_sort_u128", "bl_sort_unique_u128", "bl_count_sorted_u128", "bl_jaccard_sorted_u128", "bl_partition_u128",
    "bl_write_run_u128", "bl_write_vector_u128", "bl_file_count_u128", "bl_read_file_u128_host", "bl_read_file_u128", "bl_merge_runs_u128",
    "bl_table_build_u64", "bl_table_build_u128", "bl_table_destroy", "bl_table_info", "bl_table_arrays", "bl_table_lookup_u64", "bl_table_lookup_u128",
    "bl_table_histogram", "bl_scan_kmer_counts", "bl_scan_read_counts", "bl_table_combine", "bl_table_filter",
    "bl_select_read_counts", "bl_batch_select", "bl_read_spans", "bl_scan_read_edits", "bl_batch_apply_edits",
    "bl_table_adjacency", "bl_table_unitigs", "bl_unitig_links", "bl_unitigs_format_gfa", "bl_unitigs_mark", "bl_table_remove_unitigs",
    "bl_text_index_build", "bl_text_index_info", "bl_text_index_offsets", "bl_text_index_destroy", "bl_reader_next_batch_device_indexed", "bl_batch_format",
    "bl_text_write", "bl_bgzf_bound", "bl_bgzf_deflate", "bl_text_write_bgzf",
    "bl_scan_read_steps", "bl_link_support", "bl_steps_format_gaf",
    "bl_scan_read_quality", "bl_spans_intersect",
    "bl_scan_read_adapters",
    "bl_scan_read_duplicates",
]


class BiolibError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"biolib_amd error {code}: {msg}")
        self.code = code


class Result(C.Structure):
    _fields_ = [("count", C.c_uint64), ("xor_value", C.c_uint64), ("xor_hash", C.c_uint64), ("xor_pos", C.c_uint64),
                ("aux", C.c_uint64), ("status", C.c_int32), ("redone", C.c_int32)]

    def as_dict(self):
        return dict(count=int(self.count), xor_value=int(self.xor_value), xor_hash=int(self.xor_hash), xor_pos=int(self.xor_pos),
                    aux=int(self.aux), status=int(self.status))


class ReadCountsRecord(C.Structure):
    """bl_read_counts: one per sequence (48 bytes)"""
    _fields_ = [("n_kmers", C.c_uint32), ("n_found", C.c_uint32), ("n_solid", C.c_uint32), ("min_count", C.c_uint32), ("max_count", C.c_uint32),
                ("reserved", C.c_uint32), ("sum_counts", C.c_uint64), ("weak_begin", C.c_uint64), ("weak_end", C.c_uint64)]


READ_COUNTS_INIT, READ_COUNTS_ACCUMULATE = 0, 1
SELECT_KEEP_EMPTY = 1
BGZF_NO_EOF = 1
TRIM_NONE, TRIM_PREFIX, TRIM_SUFFIX, TRIM_LONGER = 0, 1, 2, 3


class SpanRule(C.Structure):
    """bl_span_rule: how bl_read_spans turns a read's bl_read_counts record into a span (48 bytes)"""
    _fields_ = [("trim", C.c_uint32), ("k", C.c_uint32), ("min_len", C.c_uint64), ("min_kmers", C.c_uint32), ("solid_min_num", C.c_uint32),
                ("solid_min_den", C.c_uint32), ("solid_max_num", C.c_uint32), ("solid_max_den", C.c_uint32), ("stat_lo", C.c_uint32),
                ("stat_hi", C.c_uint32), ("reserved", C.c_uint32)]


class Edit(C.Structure):
    """bl_edit: one substitution (16 bytes)"""
    _fields_ = [("pos", C.c_uint64), ("from_", C.c_uint8), ("to", C.c_uint8), ("support", C.c_uint8), ("anchor", C.c_uint8), ("reserved", C.c_uint32)]


# the same 16 bytes as a numpy record
EDIT_DTYPE = [("pos", "<u8"), ("from", "u1"), ("to", "u1"), ("support", "u1"), ("anchor", "u1"), ("reserved", "<u4")]


class EditStats(C.Structure):
    """bl_edit_stats"""
    _fields_ = [(name, C.c_uint64) for name in ("n_runs", "n_edits", "n_ambiguous", "n_no_base", "n_misfit", "n_low_support")] + [("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


class TableStats(C.Structure):
    """bl_table_stats"""
    _fields_ = [(name, C.c_uint64) for name in ("n_a_only", "n_b_only", "n_both", "n_out", "sum_min", "sum_max", "sum_out", "reserved")]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


class GraphStats(C.Structure):
    """bl_graph_stats"""
    _fields_ = [(name, C.c_uint64) for name in ("n_keys", "n_arcs", "n_isolated", "n_dead_end_sides", "n_branch_sides", "n_linked_sides", "n_unitigs",
                                                "n_cycles", "longest_unitig")] + [("reserved", C.c_uint64 * 3)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


FORMAT_FASTA, FORMAT_FASTQ = 0, 1
FORMAT_SKIP_EMPTY, FORMAT_TAG_LENGTH = 1, 2
# the 16-byte record of bl_text_index_info as a numpy record
TEXT_RECORD_DTYPE = [("name_begin", "<u8"), ("name_len", "<u4"), ("qual_delta", "<u4")]


class FormatRule(C.Structure):
    """bl_format_rule (64 bytes)"""
    _fields_ = [("format", C.c_uint32), ("flags", C.c_uint32), ("line_width", C.c_uint32), ("quality_fill", C.c_uint32), ("name_prefix", C.c_char * 16),
                ("first_number", C.c_uint64), ("tag_label", C.c_char * 16), ("reserved", C.c_uint64)]


QFAIL_MIN_LEN, QFAIL_MAX_LEN, QFAIL_AMBIGUOUS, QFAIL_LOW, QFAIL_MEAN, QFAIL_EE = 1, 2, 4, 8, 16, 32
SPANS_PAIRED = 1
# bl_read_quality as a numpy record (48 bytes)
READ_QUALITY_DTYPE = [("begin", "<u8"), ("end", "<u8"), ("sum", "<u8"), ("ee", "<u8"), ("n_low", "<u4"), ("n_ambiguous", "<u4"), ("q_min", "u1"),
                      ("q_max", "u1"), ("failed", "<u2"), ("reserved", "<u4")]


class QualityRule(C.Structure):
    """bl_quality_rule (80 bytes)"""
    _fields_ = [(name, C.c_uint32) for name in ("phred_base", "quality_fill", "front_q", "back_q", "maxsum_front_q", "maxsum_back_q", "window_len",
                                                "window_q", "low_q", "low_max_num", "low_max_den", "mean_q", "max_ambiguous", "reserved")] + \
               [(name, C.c_uint64) for name in ("min_len", "max_len", "max_ee")]


class QualityStats(C.Structure):
    """bl_quality_stats"""
    _fields_ = [(name, C.c_uint64) for name in ("n_reads", "n_reads_kept", "n_bases", "n_bases_kept", "n_too_short", "n_too_long", "n_ambiguous",
                                                "n_low", "n_mean", "n_ee")] + [("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


ADAPT_POLY_BEFORE, ADAPT_PAIR, ADAPT_ADAPTER, ADAPT_POLY_AFTER, ADAPT_TOO_SHORT, ADAPT_PAIR_SKIPPED = 1, 2, 4, 8, 16, 32
ADAPTERS_PAIRED = 1
MAX_ADAPTERS, ADAPTER_MAX_LEN, ADAPTER_PAIR_MAX_LEN = 8, 64, 512
# bl_read_adapters as a numpy record (32 bytes)
READ_ADAPTERS_DTYPE = [("begin", "<u8"), ("end", "<u8"), ("match_pos", "<u4"), ("insert", "<u4"), ("adapter", "<u2"), ("overlap", "u1"), ("mismatches", "u1"),
                       ("pair_mismatches", "<u2"), ("cut", "u1"), ("reserved", "u1")]


class AdapterRule(C.Structure):
    """bl_adapter_rule (616 bytes)"""
    _fields_ = [("flags", C.c_uint32), ("n_adapters", C.c_uint32), ("adapter_len", C.c_uint32 * MAX_ADAPTERS),
                ("adapters", (C.c_char * ADAPTER_MAX_LEN) * MAX_ADAPTERS)] + \
               [(name, C.c_uint32) for name in ("min_overlap", "error_num", "error_den", "pair_min_overlap", "pair_error_num", "pair_error_den", "pair_max_diff",
                                                "poly_before", "poly_after", "poly_min_len", "poly_per", "poly_max_mismatch", "reserved")] + \
               [("min_len", C.c_uint64)]


class AdapterStats(C.Structure):
    """bl_adapter_stats"""
    _fields_ = [(name, C.c_uint64) for name in ("n_reads", "n_reads_cut", "n_reads_kept", "n_bases", "n_bases_kept", "n_poly_before", "n_pair", "n_adapter",
                                                "n_poly_after", "n_too_short", "n_pair_skipped")] + \
               [("per_adapter", C.c_uint64 * MAX_ADAPTERS), ("reserved", C.c_uint64 * 5)]

    def as_dict(self):
        d = {name: int(getattr(self, name)) for name, _ in self._fields_ if name not in ("reserved", "per_adapter")}
        d["per_adapter"] = [int(x) for x in self.per_adapter]
        return d


DEDUP_PAIRED, DEDUP_CANONICAL = 1, 2
DUP_DUPLICATE, DUP_EMPTY, DUP_REVERSED = 1, 2, 4
# bl_read_duplicate as a numpy record (16 bytes, one per unit)
READ_DUPLICATE_DTYPE = [("first", "<u4"), ("kept", "<u4"), ("copies", "<u4"), ("flags", "<u4")]


class DedupRule(C.Structure):
    """bl_dedup_rule (32 bytes)"""
    _fields_ = [("flags", C.c_uint32), ("hash_bits", C.c_uint32), ("prefix_len", C.c_uint64), ("seed", C.c_uint64), ("reserved", C.c_uint64)]


class DedupStats(C.Structure):
    """bl_dedup_stats"""
    _fields_ = [(name, C.c_uint64) for name in ("n_units", "n_empty", "n_classes", "n_duplicates", "n_reversed", "largest_class", "n_reads_kept",
                                                "n_bases_kept")] + \
               [("class_hist", C.c_uint64 * 16), ("n_mixed_groups", C.c_uint64), ("rounds", C.c_uint64), ("reserved", C.c_uint64 * 6)]

    def as_dict(self):
        d = {name: int(getattr(self, name)) for name, _ in self._fields_ if name not in ("reserved", "class_hist")}
        d["class_hist"] = [int(x) for x in self.class_hist]
        return d


LINK_NONE = 0xFFFFFFFF
# bl_unitig_node as a numpy record
UNITIG_NODE_DTYPE = [("unitig", "<u4"), ("rank_flip", "<u4")]

LINKS_ONCE = 1
GFA_NO_HEADER = 1
# bl_unitig_link as a numpy record: (unitig << 1) | orientation, 0 for + and 1 for -
UNITIG_LINK_DTYPE = [("from", "<u4"), ("to", "<u4")]


class LinkStats(C.Structure):
    """bl_link_stats"""
    _fields_ = [(name, C.c_uint64) for name in ("n_ends", "n_links", "n_self_reverse", "n_dead_ends", "n_branch_ends")] + [("reserved", C.c_uint64 * 3)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


class GfaRule(C.Structure):
    """bl_gfa_rule (40 bytes)"""
    _fields_ = [("flags", C.c_uint32), ("k", C.c_uint32), ("name_prefix", C.c_char * 16), ("first_number", C.c_uint64), ("reserved", C.c_uint64)]


STEP_LINKED, STEP_CONTINUED = 1, 2
# bl_read_step as a numpy record (32 bytes)
READ_STEP_DTYPE = [("pos", "<u8"), ("seq", "<u8"), ("end", "<u4"), ("offset", "<u4"), ("n_kmers", "<u4"), ("flags", "<u4")]


class StepStats(C.Structure):
    """bl_step_stats"""
    _fields_ = [(name, C.c_uint64) for name in ("n_valid", "n_found", "n_steps", "n_chains", "n_linked", "longest_step")] + [("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


class SupportStats(C.Structure):
    """bl_support_stats"""
    _fields_ = [("n_transitions", C.c_uint64), ("n_unmatched", C.c_uint64), ("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


class GafRule(C.Structure):
    """bl_gaf_rule (64 bytes)"""
    _fields_ = [("flags", C.c_uint32), ("k", C.c_uint32), ("read_prefix", C.c_char * 16), ("segment_prefix", C.c_char * 16),
                ("read_first_number", C.c_uint64), ("segment_first_number", C.c_uint64), ("reserved", C.c_uint64)]


CLEAN_TIPS, CLEAN_ISOLATED, CLEAN_BUBBLES = 1, 2, 4
MARK_KEEP, MARK_TIP, MARK_ISOLATED, MARK_BUBBLE = 0, 1, 2, 3


class CleanRule(C.Structure):
    """bl_clean_rule (56 bytes)"""
    _fields_ = [("flags", C.c_uint32), ("k", C.c_uint32)] + [(name, C.c_uint64) for name in ("max_tip_keys", "max_isolated_keys", "max_isolated_mean",
                                                                                             "max_bubble_keys", "max_bubble_diff", "reserved")]


class CleanStats(C.Structure):
    """bl_clean_stats"""
    _fields_ = [(name, C.c_uint64) for name in ("n_unitigs", "n_tips", "n_isolated", "n_bubbles", "n_keys_marked", "count_sum_marked")] + [("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


TABLE_UNION, TABLE_INTERSECT, TABLE_SUBTRACT, TABLE_COUNT_SUBTRACT = 0, 1, 2, 3
COUNT_SUM, COUNT_MIN, COUNT_MAX, COUNT_LEFT, COUNT_RIGHT = 0, 1, 2, 3, 4

_lib = None


def lib():
    """Load the HIP library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build the HIP extension first (__graft_entry__.build()); "
                          "biolib_amd has no CPU fallback")
    # torch's ROCm wheel bundles its own libamdhip64/libhsa-runtime64 (same SONAMEs as /opt/rocm's).
    # Import torch first so that ONE HIP runtime serves both torch (device memory, streams, RCCL) and
    # this library; loading ours first brings in a second runtime and device enumeration then fails.
    import torch  # noqa: F401

    L = C.CDLL(LIB_PATH)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.bl_last_error.restype = C.c_char_p
    L.bl_version.restype = C.c_int
    L.bl_device_count.argtypes = [C.POINTER(C.c_int)]
    L.bl_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.bl_ctx_destroy.argtypes = [vp]
    L.bl_ctx_set_stream.argtypes = [vp, vp]
    L.bl_ctx_use_own_streams.argtypes = [vp]
    L.bl_ctx_sync.argtypes = [vp]
    L.bl_batch_upload.argtypes = [vp, vp, u64, vp, u64, C.POINTER(vp)]
    L.bl_batch_from_device.argtypes = [vp, vp, u64, vp, u64, u64, C.POINTER(vp)]
    L.bl_batch_synth.argtypes = [vp, u64, u64, u64, C.POINTER(vp)]
    L.bl_batch_destroy.argtypes = [vp]
    L.bl_batch_n_bases.restype = u64
    L.bl_batch_n_bases.argtypes = [vp]
    L.bl_batch_n_seqs.restype = u64
    L.bl_batch_n_seqs.argtypes = [vp]
    L.bl_batch_device_bases.restype = vp
    L.bl_batch_device_bases.argtypes = [vp]
    L.bl_batch_download.argtypes = [vp, u64, u64, vp]
    L.bl_batch_set_origin.argtypes = [vp, u64]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_batch_origin"):  # (an A/B build of an older revision may lack it)
        L.bl_batch_origin.argtypes = [vp]
        L.bl_batch_origin.restype = u64
    L.bl_batch_upload_reads.argtypes = [vp, vp, u64, u64, C.POINTER(vp)]
    L.bl_scan_kmers.argtypes = [vp, vp, u64, u64, u32, u64, u32, vp, vp, vp, C.POINTER(Result)]
    L.bl_scan_minimizers.argtypes = [vp, vp, u64, u64, u32, u32, u64, u32, vp, vp, vp, u64, C.POINTER(Result)]
    L.bl_scan_hash_sample.argtypes = [vp, vp, u64, u64, u32, u64, u64, u32, vp, vp, vp, u64, C.POINTER(Result)]
    L.bl_sort_unique_u64.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.bl_pack_super_kmers.argtypes = [vp, vp, vp, vp, vp, u64, u32, u32, vp]
    L.bl_count_super_kmers.argtypes = [vp, vp, u64, u32, u32, u64, u32, vp, vp, u64, C.POINTER(u64)]
    L.bl_partition_records.argtypes = [vp, vp, vp, u64, u32, vp, vp]
    L.bl_expand_super_kmers.argtypes = [vp, vp, u64, u32, u32, vp, u64, C.POINTER(u64)]
    L.bl_ctx_set_lanes.argtypes = [vp, C.c_int]
    L.bl_probe_hbm.argtypes = [vp, u64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.bl_clock_probe_start.argtypes = [vp, u32, C.POINTER(vp)]
    L.bl_clock_probe_finish.argtypes = [vp, C.POINTER(C.c_double)]
    L.bl_sort_u64.argtypes = [vp, vp, u64]
    for suffix in ("u64", "u128"):  # the key-list calls whose signature does not depend on the key's width
        for name, argtypes in (("jaccard_sorted", [vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]),
                               ("partition", [vp, vp, u64, u32, u64, vp, vp]),
                               ("count_sorted", [vp, vp, u64, vp, vp, C.POINTER(u64)]),
                               ("write_run", [vp, vp, u64, C.c_char_p]),
                               ("write_vector", [vp, vp, u64, C.c_char_p]),
                               ("file_count", [C.c_char_p, C.c_int, C.POINTER(u64)]),
                               ("read_file", [vp, C.c_char_p, C.c_int, vp, u64, C.POINTER(u64)]),
                               ("merge_runs", [vp, C.POINTER(C.c_char_p), u32, vp, u64, C.POINTER(u64)])):
            getattr(L, f"bl_{name}_{suffix}").argtypes = argtypes
        getattr(L, f"bl_read_file_{suffix}_host").argtypes = [C.c_char_p, C.c_int, vp, u64, C.POINTER(u64)]
    L.bl_scan_super_kmers.argtypes = [vp, vp, u64, u64, u32, u32, u64, u32, vp, vp, vp, vp, vp, u64, C.POINTER(Result)]
    L.bl_scan_super_kmer_records.argtypes = [vp, vp, u64, u64, u32, u32, u64, u32, vp, vp, u64, C.POINTER(Result)]
    L.bl_scan_syncmers.argtypes = [vp, vp, u64, u64, u32, u32, u32, u32, u64, u32, vp, u64, C.POINTER(Result)]
    L.bl_ctx_last_scan_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.bl_ctx_set_exact_windows.argtypes = [vp, C.c_int]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_ctx_set_option"):
        L.bl_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_ctx_last_scan_kernels"):  # (an A/B build of an older revision lacks them)
        L.bl_ctx_last_scan_kernels.argtypes = [vp, C.c_char_p, u64, C.POINTER(u64)]
        L.bl_scan_kernel_names.argtypes = [C.c_char_p, u64, C.POINTER(u64)]
    L.bl_ctx_kernel_timing.argtypes = [vp, C.c_int]
    L.bl_ctx_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64)]
    L.bl_ctx_mark.argtypes = [vp]
    L.bl_ctx_mark_times.argtypes = [vp, C.POINTER(C.c_double), u32, C.POINTER(u32)]
    L.bl_reader_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.bl_reader_close.argtypes = [vp]
    L.bl_reader_open_threads.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.bl_reader_kind.restype = C.c_char_p
    L.bl_reader_kind.argtypes = [vp]
    L.bl_reader_next_text.argtypes = [vp, u64, C.POINTER(vp), C.POINTER(u64)]
    L.bl_reader_next_batch_device.argtypes = [vp, vp, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.bl_count_allreduce.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(u64), C.c_int]
    L.bl_reader_next_record.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(u64)]
    L.bl_reader_next_batch.argtypes = [vp, vp, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.bl_reader_last_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.bl_reader_last_name.restype = C.c_char_p
    L.bl_reader_last_name.argtypes = [vp, u64]
    L.bl_batch_from_text.argtypes = [vp, vp, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.bl_run_file_name.argtypes = [C.c_char_p, C.c_char_p, u64, C.c_char_p, u64]
    L.bl_device_alloc.argtypes = [vp, u64, C.POINTER(vp)]
    L.bl_device_free.argtypes = [vp, vp]
    L.bl_copy_to_host.argtypes = [vp, vp, vp, u64]
    L.bl_copy_to_device.argtypes = [vp, vp, vp, u64]
    L.bl_reader_open_shard.argtypes = [C.c_char_p, u32, u32, C.POINTER(vp)]
    L.bl_reader_shard_range.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.bl_host_alloc.argtypes = [vp, u64, C.POINTER(vp)]
    L.bl_host_free.argtypes = [vp, vp]
    L.bl_bgzf_walk.argtypes = [vp, u64, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.bl_bgzf_inflate.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp]
    L.bl_hash64_u64.restype = u64
    L.bl_hash64_u64.argtypes = [u64, u64]
    L.bl_scan_kmers128.argtypes = [vp, vp, u64, u64, u32, u64, u32, vp, vp, vp, C.POINTER(Result)]
    L.bl_scan_hash_sample128.argtypes = [vp, vp, u64, u64, u32, u64, u64, u32, vp, vp, vp, u64, C.POINTER(Result)]
    L.bl_scan_syncmers128.argtypes = [vp, vp, u64, u64, u32, u32, u32, u32, u64, u32, vp, u64, C.POINTER(Result)]
    L.bl_scan_minimizers128.argtypes = [vp, vp, u64, u64, u32, u32, u64, u32, vp, vp, vp, u64, C.POINTER(Result)]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_scan_super_kmer_records128"):  # (an A/B build of an older revision lacks it)
        L.bl_scan_super_kmer_records128.argtypes = [vp, vp, u64, u64, u32, u32, u64, u32, vp, vp, u64, C.POINTER(Result)]
    L.bl_pack_super_kmers128.argtypes = [vp, vp, vp, vp, vp, u64, u32, u32, vp]
    L.bl_partition_records128.argtypes = [vp, vp, vp, u64, u32, vp, vp]
    L.bl_expand_super_kmers128.argtypes = [vp, vp, u64, u32, u32, vp, u64, C.POINTER(u64)]
    L.bl_count_super_kmers128.argtypes = [vp, vp, u64, u32, u32, u64, u32, vp, vp, u64, C.POINTER(u64)]
    L.bl_sort_u128.argtypes = [vp, vp, u64, u32]
    L.bl_sort_unique_u128.argtypes = [vp, vp, u64, u32, C.POINTER(u64)]
    L.bl_hash64_u128.restype = u64
    L.bl_hash64_u128.argtypes = [u64, u64, u64]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_table_build_u64"):  # (an A/B build of an older revision lacks them)
        L.bl_table_build_u64.argtypes = [vp, vp, vp, u64, u32, C.POINTER(vp)]
        L.bl_table_build_u128.argtypes = [vp, vp, vp, u64, u32, C.POINTER(vp)]
        L.bl_table_destroy.argtypes = [vp]
        L.bl_table_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
        L.bl_table_arrays.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.bl_table_lookup_u64.argtypes = [vp, vp, vp, u64, vp]
        L.bl_table_lookup_u128.argtypes = [vp, vp, vp, u64, vp]
        L.bl_table_histogram.argtypes = [vp, vp, vp, u32]
        L.bl_scan_kmer_counts.argtypes = [vp, vp, u64, u64, u32, u32, vp, vp, vp, C.POINTER(Result)]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_scan_read_counts"):
        L.bl_scan_read_counts.argtypes = [vp, vp, u64, u64, u32, u32, vp, u32, vp, u32, vp, C.POINTER(Result)]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_table_combine"):
        L.bl_table_combine.argtypes = [vp, vp, vp, u32, u32, u32, u32, C.POINTER(vp), C.POINTER(TableStats)]
        L.bl_table_filter.argtypes = [vp, vp, u32, u32, C.POINTER(vp)]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_select_read_counts"):
        L.bl_select_read_counts.argtypes = [vp, vp, u64, u64, vp, vp, vp, C.POINTER(u32), C.POINTER(u32), u32, vp, vp]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_batch_select"):
        L.bl_batch_select.argtypes = [vp, vp, vp, vp, u32, C.POINTER(vp), vp, vp, C.POINTER(u64), C.POINTER(u64)]
        L.bl_read_spans.argtypes = [vp, vp, vp, vp, vp, C.POINTER(SpanRule), vp]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_scan_read_edits"):
        L.bl_scan_read_edits.argtypes = [vp, vp, u64, u64, u32, u32, vp, u32, u32, vp, u64, C.POINTER(EditStats)]
        L.bl_batch_apply_edits.argtypes = [vp, vp, vp, u64, C.POINTER(vp)]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_table_adjacency"):
        L.bl_table_adjacency.argtypes = [vp, vp, u32, vp, vp, C.POINTER(GraphStats)]
        L.bl_table_unitigs.argtypes = [vp, vp, u32, C.POINTER(vp), vp, vp, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(GraphStats)]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_unitig_links"):
        L.bl_unitig_links.argtypes = [vp, vp, u32, vp, vp, u64, u32, vp, vp, u64, C.POINTER(u64), C.POINTER(LinkStats)]
        L.bl_unitigs_format_gfa.argtypes = [vp, vp, vp, u64, vp, vp, u64, C.POINTER(GfaRule), vp, u64, C.POINTER(u64)]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_unitigs_mark"):
        L.bl_unitigs_mark.argtypes = [vp, vp, vp, u64, vp, vp, u64, C.POINTER(CleanRule), vp, C.POINTER(CleanStats)]
        L.bl_table_remove_unitigs.argtypes = [vp, vp, vp, vp, u64, C.POINTER(vp), C.POINTER(u64)]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_batch_format"):
        L.bl_text_index_build.argtypes = [vp, vp, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
        L.bl_text_index_info.argtypes = [vp, C.POINTER(u64), C.POINTER(C.c_int), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp)]
        L.bl_text_index_offsets.argtypes = [vp]
        L.bl_text_index_offsets.restype = vp
        L.bl_text_index_destroy.argtypes = [vp]
        L.bl_reader_next_batch_device_indexed.argtypes = [vp, vp, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
        L.bl_batch_format.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.POINTER(FormatRule), vp, u64, C.POINTER(u64), C.POINTER(u64)]
        L.bl_text_write.argtypes = [vp, vp, u64, C.c_char_p, C.c_int]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_bgzf_deflate"):
        L.bl_bgzf_bound.argtypes = [u64, C.c_uint32]
        L.bl_bgzf_bound.restype = u64
        L.bl_bgzf_deflate.argtypes = [vp, vp, u64, C.c_uint32, vp, u64, C.POINTER(u64), vp, C.POINTER(u64)]
        L.bl_text_write_bgzf.argtypes = [vp, vp, u64, C.c_char_p, C.c_int, C.c_uint32]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_scan_read_steps"):
        L.bl_scan_read_steps.argtypes = [vp, vp, u64, u64, u32, u32, vp, vp, vp, u64, vp, vp, u64, C.POINTER(StepStats)]
        L.bl_link_support.argtypes = [vp, vp, u64, vp, vp, u64, u64, vp, C.POINTER(SupportStats)]
        L.bl_steps_format_gaf.argtypes = [vp, vp, vp, vp, u64, vp, u64, C.POINTER(GafRule), vp, u64, C.POINTER(u64)]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_scan_read_quality"):
        L.bl_scan_read_quality.argtypes = [vp, vp, vp, C.POINTER(QualityRule), vp, vp, C.POINTER(QualityStats)]
        L.bl_spans_intersect.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_scan_read_adapters"):
        L.bl_scan_read_adapters.argtypes = [vp, vp, vp, vp, C.POINTER(AdapterRule), vp, vp, C.POINTER(AdapterStats)]
    if "BIOLIB_AMD_LIB" not in os.environ or hasattr(L, "bl_scan_read_duplicates"):
        L.bl_scan_read_duplicates.argtypes = [vp, vp, vp, vp, vp, C.POINTER(DedupRule), vp, vp, C.POINTER(DedupStats)]
    _lib = L
    return L


def check(rc):
    if rc != BL_OK:
        raise BiolibError(rc, lib().bl_last_error().decode(errors="replace"))
    return rc
