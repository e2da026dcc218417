"""ctypes binding of the C ABI declared in include/tkv_amq.h (libtkv_amq.so).

This is the only way the Python host side reaches the filter kernels.  There is no CPU
fallback: if the library is missing or no GPU is visible, device entry points raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _build

OK = 0
INVALID_ARGUMENT = 3
RESOURCE_EXHAUSTED = 8
INTERNAL = 13
UNAVAILABLE = 14

BLOOM = 0
VQF = 1

STATUS_NAMES = {OK: "OK", INVALID_ARGUMENT: "InvalidArgument",
                RESOURCE_EXHAUSTED: "ResourceExhausted", INTERNAL: "Internal",
                UNAVAILABLE: "Unavailable"}


class TkvAmqError(RuntimeError):
    """A non-OK status from libtkv_amq (mirrors batt::Status propagation)."""

    def __init__(self, status: int, what: str):
        super().__init__(f"{what}: {STATUS_NAMES.get(status, status)}")
        self.status = status


class Segment(ctypes.Structure):
    """tkv_amq_segment (64 bytes)."""
    _fields_ = [
        ("out_offset", ctypes.c_uint64),
        ("n_blocks", ctypes.c_uint32),
        ("hash_count", ctypes.c_uint16),
        ("tag_bits", ctypes.c_uint8),
        ("hash_val_shift", ctypes.c_uint8),
        ("mod_magic", ctypes.c_uint64),
        ("key_begin", ctypes.c_uint64),
        ("src_page_id", ctypes.c_uint64),
        ("block_base", ctypes.c_uint64),
        ("n_keys", ctypes.c_uint32),
        ("payload_bytes", ctypes.c_uint32),
        ("bits_per_key", ctypes.c_uint32),
        ("page_flags", ctypes.c_uint32),
    ]


assert ctypes.sizeof(Segment) == 64

SEGMENT_DTYPE = np.dtype([
    ("out_offset", "<u8"), ("n_blocks", "<u4"), ("hash_count", "<u2"), ("tag_bits", "u1"),
    ("hash_val_shift", "u1"), ("mod_magic", "<u8"), ("key_begin", "<u8"), ("src_page_id", "<u8"),
    ("block_base", "<u8"), ("n_keys", "<u4"), ("payload_bytes", "<u4"), ("bits_per_key", "<u4"),
    ("page_flags", "<u4")])
PAGE_IMAGE = 0x1  # TKV_AMQ_PAGE_IMAGE


class ProbeOpts(ctypes.Structure):
    """tkv_amq_probe_opts (device pointers, any may be NULL)."""
    _fields_ = [("d_query_page_id", ctypes.c_void_p), ("d_truth", ctypes.c_void_p),
                ("d_metrics", ctypes.c_void_p)]


# tkv_amq_probe_metrics: KeyQuery::Metrics counters (tree/key_query.hpp:36-60), u64 each
PROBE_METRICS_FIELDS = ("total_filter_query_count", "no_filter_page_count",
                        "page_id_mismatch_count", "filter_reject_count", "filter_positive_count",
                        "filter_false_positive_count")
assert SEGMENT_DTYPE.itemsize == 64

# every symbol include/tkv_amq.h declares
EXPORTS = [
    "tkv_amq_version", "tkv_amq_status_string", "tkv_amq_device_count",
    "tkv_amq_filter_bits_per_key", "tkv_amq_vqf_load_factor", "tkv_amq_vqf_required_size",
    "tkv_amq_vqf_nslots_for_size", "tkv_amq_plan", "tkv_amq_build", "tkv_amq_build_check",
    "tkv_amq_probe", "tkv_amq_vqf_hash", "tkv_amq_vqf_probe_hashed", "tkv_amq_gen_keys16",
    "tkv_amq_bloom_query_stride", "tkv_amq_bloom_hash", "tkv_amq_bloom_probe_hashed",
    "tkv_amq_stage_keys", "tkv_amq_leaf_data_size", "tkv_amq_expected_items_per_leaf",
    "tkv_amq_filter_page_size_log2", "tkv_amq_plan_pages", "tkv_amq_probe_ex",
    "tkv_amq_vqf_probe_hashed_ex", "tkv_amq_bloom_probe_hashed_ex",
    "tkv_amq_bloom_route_ws_bytes", "tkv_amq_bloom_route", "tkv_amq_bloom_build_range_ws_bytes",
    "tkv_amq_bloom_build_range", "tkv_amq_bloom_route_records_ws_bytes", "tkv_amq_bloom_route_records",
    "tkv_amq_bloom_build_range_records_ws_bytes", "tkv_amq_bloom_build_range_records",
    "tkv_amq_bloom_route_records_ex", "tkv_amq_bloom_tile_blocks", "tkv_amq_bloom_range_max_tiles",
    "tkv_amq_bloom_route_plan", "tkv_amq_bloom_route_blocks", "tkv_amq_bloom_build_part_blocks",
    "tkv_amq_bloom_blocks_lost", "tkv_amq_build_ex",
    "tkv_amq_bloom_records_per_key", "tkv_amq_bloom_route_records_any_ws_bytes",
    "tkv_amq_bloom_route_records_any",
    "tkv_amq_path_probe_ws_bytes", "tkv_amq_path_probe",
    "tkv_amq_open_filters", "tkv_amq_scan_filters_ws_bytes", "tkv_amq_scan_filters",
    "tkv_amq_build_route",
    "tkv_amq_verify_members_ws_bytes", "tkv_amq_verify_members",
    "tkv_amq_find_keys",
    "tkv_amq_walk_paths_ws_bytes", "tkv_amq_walk_paths",
    "tkv_amq_get_keys",
    "tkv_amq_get_values", "tkv_amq_gather_values",
    "tkv_amq_merge_leaves_ws_bytes", "tkv_amq_merge_leaves", "tkv_amq_merge_values_bound",
    "tkv_amq_gather_merged_ws_bytes", "tkv_amq_gather_merged",
    "tkv_amq_merge_levels_ws_bytes", "tkv_amq_merge_levels", "tkv_amq_merge_levels_values_bound",
    "tkv_amq_gather_levels_ws_bytes", "tkv_amq_gather_levels",
]

# tkv_amq_build_route: TKV_AMQ_ROUTE_* (a Bloom batch's route, or a VQF batch's decide stage),
# TKV_AMQ_PLACE_* (VQF place stage), TKV_AMQ_LEAF_* (tkv_amq_build_ex's leaves)
ROUTE_SPLIT, ROUTE_WINDOW, ROUTE_LDS, ROUTE_TILED_KEYS, ROUTE_TILED_RECORDS, ROUTE_ATOMICS = range(6)
ROUTE_VQF_BIG_U8, ROUTE_VQF_BIG_GLOBAL, ROUTE_VQF_RING_PLACE, ROUTE_VQF_RING_PLACE2, ROUTE_VQF_RING, \
    ROUTE_VQF_DECIDE = range(16, 22)
PLACE_NONE, PLACE_FUSED512, PLACE_FUSED256, PLACE_SCATTER = range(4)
LEAF_BATCH, LEAF_MULTI, LEAF_TILED_KEYS, LEAF_TILED_RECORDS, LEAF_ATOMICS, LEAF_NONE = range(6)


class BuildRoute(ctypes.Structure):
    """struct tkv_amq_build_route (40 bytes)."""
    _fields_ = [("route", ctypes.c_uint32), ("place", ctypes.c_uint32), ("parts", ctypes.c_uint32),
                ("windows", ctypes.c_uint32), ("threads", ctypes.c_uint32),
                ("located", ctypes.c_uint32), ("ws_bytes", ctypes.c_uint64),
                ("lds_bytes", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


assert ctypes.sizeof(BuildRoute) == 40

# tkv_amq_open_filters' per-filter codes (TKV_AMQ_OPEN_*)
OPEN_OK, OPEN_BAD_MAGIC, OPEN_WRONG_KIND, OPEN_BAD_GEOMETRY, OPEN_OUT_OF_BOUNDS, OPEN_MISALIGNED, \
    OPEN_BAD_PAGE = range(7)
OPEN_STATUS_NAMES = ("OK", "BadMagic", "WrongKind", "BadGeometry", "OutOfBounds", "Misaligned",
                     "BadPage")

# tkv_amq_filter_stats (32 bytes)
FILTER_STATS_DTYPE = np.dtype([
    ("occupied", "<u8"), ("header_items", "<u8"), ("full_blocks", "<u4"), ("empty_blocks", "<u4"),
    ("max_block", "<u4"), ("bad_blocks", "<u4")])
assert FILTER_STATS_DTYPE.itemsize == 32

# tkv_amq_member_check (16 bytes) and its flags (TKV_AMQ_VERIFY_*)
MEMBER_CHECK_DTYPE = np.dtype([("first_missing", "<u8"), ("missing", "<u4"), ("flags", "<u4")])
assert MEMBER_CHECK_DTYPE.itemsize == 16
VERIFY_NO_FILTER, VERIFY_ID_MISMATCH = 0x1, 0x2
NONE_MISSING = (1 << 64) - 1  # first_missing of a leaf whose keys all pass

# tkv_amq_find_result (16 bytes), tkv_amq_find_counts (32 bytes), TKV_AMQ_FIND_ALL and the
# per-candidate states (TKV_AMQ_CAND_*)
FIND_RESULT_DTYPE = np.dtype([("key_index", "<u8"), ("leaf", "<u4"), ("cand", "<u4")])
assert FIND_RESULT_DTYPE.itemsize == 16
FIND_COUNTS_FIELDS = ("leaf_search_count", "found_count", "absent_count", "unsearchable_count")
FIND_COUNTS_DTYPE = np.dtype([(n, "<u8") for n in FIND_COUNTS_FIELDS])
assert FIND_COUNTS_DTYPE.itemsize == 32
FIND_ALL = 0x1
CAND_ABSENT, CAND_FOUND, CAND_NOT_SEARCHED, CAND_UNSEARCHABLE = range(4)
NOT_FOUND = (1 << 64) - 1  # key_index of a query whose key no searched candidate holds
NO_LEAF = 0xFFFFFFFF       # its leaf and cand

# tkv_amq_get_result (16 bytes), tkv_amq_get_counts (48 bytes) and TKV_AMQ_GET_CHECK_PAGE_ID
GET_RESULT_DTYPE = np.dtype([("key_index", "<u8"), ("leaf", "<u4"), ("where", "<u4")])
assert GET_RESULT_DTYPE.itemsize == 16
GET_COUNTS_FIELDS = ("visit_count", "leaf_search_count", "found_count", "absent_count",
                     "unsearchable_count", "flushed_count")
GET_COUNTS_DTYPE = np.dtype([(n, "<u8") for n in GET_COUNTS_FIELDS])
assert GET_COUNTS_DTYPE.itemsize == 48
GET_CHECK_PAGE_ID = 0x1
NO_WHERE = 0xFFFFFFFF      # `where` of a query that found nothing

# tkv_amq_value_result (32 bytes), tkv_amq_value_counts (64 bytes), the ops of a packed value
# (TKV_AMQ_OP_*) and the result flags (TKV_AMQ_VALUE_*)
VALUE_RESULT_DTYPE = np.dtype([("key_index", "<u8"), ("last_index", "<u8"), ("leaf", "<u4"), ("where", "<u4"),
                               ("i32", "<i4"), ("op", "u1"), ("flags", "u1"), ("n_items", "<u2")])
assert VALUE_RESULT_DTYPE.itemsize == 32
VALUE_COUNTS_FIELDS = GET_COUNTS_FIELDS + ("item_count", "bad_combine_count")
VALUE_COUNTS_DTYPE = np.dtype([(n, "<u8") for n in VALUE_COUNTS_FIELDS])
assert VALUE_COUNTS_DTYPE.itemsize == 64
OP_DELETE, OP_NOOP, OP_WRITE, OP_ADD_I32, OP_PAGE_SLICE = range(5)
OP_NONE = 0xFF             # `op` of a lookup that took no item
VALUE_COMBINED, VALUE_BAD_COMBINE = 0x1, 0x2

# tkv_amq_merge_leaves: its flag (TKV_AMQ_MERGE_DECAY_TO_ITEMS), tkv_amq_merge_item (16 bytes),
# tkv_amq_merge_counts (56 bytes) and the run bit of a record's src
MERGE_DECAY_TO_ITEMS = 0x1
MERGE_ITEM_DTYPE = np.dtype([("src", "<u8"), ("i32", "<i4"), ("op", "u1"), ("flags", "u1"), ("reserved", "<u2")])
assert MERGE_ITEM_DTYPE.itemsize == 16
MERGE_COUNTS_FIELDS = ("newer_count", "older_count", "pair_count", "combined_count", "bad_combine_count",
                       "dropped_count", "out_count")
MERGE_COUNTS_DTYPE = np.dtype([(n, "<u8") for n in MERGE_COUNTS_FIELDS])
assert MERGE_COUNTS_DTYPE.itemsize == 56
MERGE_SRC_OLDER = 1 << 63
# tkv_amq_merge_levels: the runs of one call at most, and where a record's src holds its run
MERGE_MAX_RUNS = 8
LEVELS_SRC_SHIFT = 56


class MergeRun(ctypes.Structure):
    """tkv_amq_merge_run (64 bytes): one side of a merge, a host struct of device pointers."""
    _fields_ = [("keys", ctypes.c_void_p), ("key_offsets", ctypes.c_void_p), ("values", ctypes.c_void_p),
                ("value_offsets", ctypes.c_void_p), ("d_begin", ctypes.c_void_p),
                ("n_items", ctypes.c_uint64), ("values_bytes", ctypes.c_uint64),
                ("key_stride", ctypes.c_uint32), ("value_stride", ctypes.c_uint32)]


assert ctypes.sizeof(MergeRun) == 64


# tkv_amq_walk_paths: the flat tree (tkv_amq_tree_node / _segment / _child) and its limits
class TreeNode(ctypes.Structure):
    """tkv_amq_tree_node (32 bytes)."""
    _fields_ = [("pivot_key_begin", ctypes.c_uint32), ("seg_begin", ctypes.c_uint32),
                ("child_begin", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
                ("pivot_count", ctypes.c_uint8), ("height", ctypes.c_uint8),
                ("level_count", ctypes.c_uint8), ("reserved1", ctypes.c_uint8),
                ("level_start", ctypes.c_uint8 * 8), ("reserved2", ctypes.c_uint32)]


class TreeSegment(ctypes.Structure):
    """tkv_amq_tree_segment (32 bytes)."""
    _fields_ = [("leaf_page_id", ctypes.c_uint64), ("active_pivots", ctypes.c_uint64),
                ("flushed_pivots", ctypes.c_uint64), ("leaf", ctypes.c_uint32),
                ("flushed_begin", ctypes.c_uint32)]


class TreeChild(ctypes.Structure):
    """tkv_amq_tree_child (16 bytes)."""
    _fields_ = [("page_id", ctypes.c_uint64), ("index", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


assert (ctypes.sizeof(TreeNode), ctypes.sizeof(TreeSegment), ctypes.sizeof(TreeChild)) == (32, 32, 16)
TREE_NODE_DTYPE = np.dtype([
    ("pivot_key_begin", "<u4"), ("seg_begin", "<u4"), ("child_begin", "<u4"), ("reserved0", "<u4"),
    ("pivot_count", "u1"), ("height", "u1"), ("level_count", "u1"), ("reserved1", "u1"),
    ("level_start", "u1", (8,)), ("reserved2", "<u4")])
TREE_SEGMENT_DTYPE = np.dtype([
    ("leaf_page_id", "<u8"), ("active_pivots", "<u8"), ("flushed_pivots", "<u8"), ("leaf", "<u4"),
    ("flushed_begin", "<u4")])
TREE_CHILD_DTYPE = np.dtype([("page_id", "<u8"), ("index", "<u4"), ("reserved", "<u4")])
assert (TREE_NODE_DTYPE.itemsize, TREE_SEGMENT_DTYPE.itemsize, TREE_CHILD_DTYPE.itemsize) == (32, 32, 16)
WALK_MAX_DEPTH = 16      # TKV_AMQ_WALK_MAX_DEPTH
WALK_LEAF_LEVEL = 0xFF   # TKV_AMQ_WALK_LEAF_LEVEL: d_path_where's level byte of a child-leaf entry
# PackedNodePage's limits (tree/packed_node_page.hpp:42-223), which TreeIndex validates
TREE_MAX_PIVOTS, TREE_MAX_SEGMENTS, TREE_MAX_LEVELS = 64, 63, 7


class RoutePlan(ctypes.Structure):
    """tkv_amq_route_plan: the pipelined hash-range build's parts, route workgroups and block
    layout (include/tkv_amq.h)."""
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "n_tiles", "n_parts", "parts_per_rank", "part_tiles", "world", "n_chunks", "route_wgs",
        "region_cap", "ovf_cap", "hash_count")] + [(n, ctypes.c_uint64) for n in (
        "chunk_keys", "block_bytes", "counts_off", "ovf_n_off", "regions_off", "ovf_off",
        "route_ws_bytes", "part_ws_bytes", "part_bytes", "n_blocks")]


assert ctypes.sizeof(RoutePlan) == 120

# tkv_amq_key_view (libstdc++ std::string_view layout)
KEY_VIEW_DTYPE = np.dtype([("size", "<u8"), ("data", "<u8")])

_lib = None


def experiment_lib():
    """TKV_AMQ_LIB names an experiment build of the library (kernel A/B timing).  It is taken
    only together with TKV_AMQ_EXPERIMENT=1, so a stray variable cannot put an experiment
    library behind the tests, smoke() or the bench."""
    path = os.environ.get("TKV_AMQ_LIB")
    if not path:
        return None
    if os.environ.get("TKV_AMQ_EXPERIMENT") != "1":
        raise RuntimeError("TKV_AMQ_LIB is set but TKV_AMQ_EXPERIMENT is not 1: experiment "
                           "libraries are loaded only on purpose")
    return path


def lib(build_if_missing: bool = True):
    """Load libtkv_amq.so (building it in-tree if absent and hipcc is available)."""
    global _lib
    if _lib is not None:
        return _lib
    path = experiment_lib() or _build.LIB
    if not os.path.exists(path):
        if not build_if_missing:
            raise RuntimeError(f"libtkv_amq.so not built ({path}); run __graft_entry__.build()")
        _build.build()
    L = ctypes.CDLL(path)
    u64, u32, i32, vp, dbl = (ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p,
                              ctypes.c_double)
    L.tkv_amq_version.restype = ctypes.c_char_p
    L.tkv_amq_version.argtypes = []
    L.tkv_amq_status_string.restype = ctypes.c_char_p
    L.tkv_amq_status_string.argtypes = [i32]
    L.tkv_amq_device_count.restype = i32
    L.tkv_amq_device_count.argtypes = []
    L.tkv_amq_filter_bits_per_key.restype = u64
    L.tkv_amq_filter_bits_per_key.argtypes = [i32, u64]
    L.tkv_amq_vqf_load_factor.restype = dbl
    L.tkv_amq_vqf_load_factor.argtypes = [i32, u64]
    L.tkv_amq_vqf_required_size.restype = u64
    L.tkv_amq_vqf_required_size.argtypes = [i32, u64]
    L.tkv_amq_vqf_nslots_for_size.restype = u64
    L.tkv_amq_vqf_nslots_for_size.argtypes = [i32, u64]
    L.tkv_amq_plan.restype = i32
    L.tkv_amq_plan.argtypes = [i32, vp, vp, u32, u32, u64, u64, vp,
                               ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u32)]
    L.tkv_amq_build.restype = i32
    L.tkv_amq_build.argtypes = [i32, vp, vp, u32, u64, vp, u32, u32, vp, vp, u64, vp]
    if hasattr(L, "tkv_amq_build_ex"):
        L.tkv_amq_build_ex.restype = i32
        L.tkv_amq_build_ex.argtypes = [i32, vp, vp, u32, u64, vp, vp, u32, u32, vp, vp, u64, vp]
    L.tkv_amq_build_check.restype = i32
    L.tkv_amq_build_check.argtypes = [i32, vp, u64, vp]
    L.tkv_amq_probe.restype = i32
    L.tkv_amq_probe.argtypes = [i32, vp, vp, u32, vp, vp, u32, u64, vp, vp, vp]
    L.tkv_amq_vqf_hash.restype = i32
    L.tkv_amq_vqf_hash.argtypes = [vp, vp, u32, u64, vp, vp]
    L.tkv_amq_vqf_probe_hashed.restype = i32
    L.tkv_amq_vqf_probe_hashed.argtypes = [vp, vp, u32, vp, vp, u64, vp, vp, vp]
    L.tkv_amq_bloom_query_stride.restype = u32
    L.tkv_amq_bloom_query_stride.argtypes = [u32]
    L.tkv_amq_bloom_hash.restype = i32
    L.tkv_amq_bloom_hash.argtypes = [vp, vp, u32, u64, u32, vp, vp]
    L.tkv_amq_bloom_probe_hashed.restype = i32
    L.tkv_amq_bloom_probe_hashed.argtypes = [vp, vp, u32, vp, u32, vp, u64, vp, vp, vp]
    L.tkv_amq_gen_keys16.restype = i32
    L.tkv_amq_gen_keys16.argtypes = [u64, u64, u64, vp, vp]
    L.tkv_amq_stage_keys.restype = i32
    L.tkv_amq_stage_keys.argtypes = [vp, u64, u64, u32, vp, u64, vp, i32]
    if path != _build.LIB and not hasattr(L, "tkv_amq_probe_ex"):
        _lib = L  # an older experiment build (A/B timing): the round-1 entry points only
        return L
    L.tkv_amq_leaf_data_size.restype = u64
    L.tkv_amq_leaf_data_size.argtypes = [u64]
    L.tkv_amq_expected_items_per_leaf.restype = u64
    L.tkv_amq_expected_items_per_leaf.argtypes = [u64, u32, u32]
    L.tkv_amq_filter_page_size_log2.restype = u32
    L.tkv_amq_filter_page_size_log2.argtypes = [i32, u64, u32, u32, u64]
    L.tkv_amq_plan_pages.restype = i32
    L.tkv_amq_plan_pages.argtypes = [i32, vp, vp, u32, u32, u32, vp,
                                     ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u32)]
    popts = ctypes.POINTER(ProbeOpts)
    L.tkv_amq_probe_ex.restype = i32
    L.tkv_amq_probe_ex.argtypes = [i32, vp, vp, u32, vp, vp, u32, u64, vp, vp, popts, vp]
    L.tkv_amq_vqf_probe_hashed_ex.restype = i32
    L.tkv_amq_vqf_probe_hashed_ex.argtypes = [vp, vp, u32, vp, vp, u64, vp, vp, popts, vp]
    L.tkv_amq_bloom_probe_hashed_ex.restype = i32
    L.tkv_amq_bloom_probe_hashed_ex.argtypes = [vp, vp, u32, vp, u32, vp, u64, vp, vp, popts, vp]
    if hasattr(L, "tkv_amq_path_probe"):
        L.tkv_amq_path_probe_ws_bytes.restype = u64
        L.tkv_amq_path_probe_ws_bytes.argtypes = [u64, u64]
        L.tkv_amq_path_probe.restype = i32
        L.tkv_amq_path_probe.argtypes = [i32, vp, vp, u32, vp, vp, u32, u64, vp, vp, u64, vp, vp, vp,
                                         vp, popts, vp, u64, vp]
    if hasattr(L, "tkv_amq_open_filters"):
        L.tkv_amq_open_filters.restype = i32
        L.tkv_amq_open_filters.argtypes = [i32, vp, u64, vp, u64, u32, u32, vp, vp, vp, vp]
        L.tkv_amq_scan_filters_ws_bytes.restype = u64
        L.tkv_amq_scan_filters_ws_bytes.argtypes = [u32]
        L.tkv_amq_scan_filters.restype = i32
        L.tkv_amq_scan_filters.argtypes = [i32, vp, vp, u32, vp, vp, u64, vp]
    if hasattr(L, "tkv_amq_verify_members"):
        L.tkv_amq_verify_members_ws_bytes.restype = u64
        L.tkv_amq_verify_members_ws_bytes.argtypes = [u32]
        L.tkv_amq_verify_members.restype = i32
        L.tkv_amq_verify_members.argtypes = [i32, vp, vp, u32, u32, vp, vp, u32, u64, vp, vp, vp, vp, u64, vp]
    if hasattr(L, "tkv_amq_find_keys"):
        L.tkv_amq_find_keys.restype = i32
        L.tkv_amq_find_keys.argtypes = [i32, vp, vp, u32, vp, vp, u32, u64, vp, vp, vp, u64, vp, vp, u32,
                                        u64, vp, u32, vp, vp, popts, vp, vp]
    if hasattr(L, "tkv_amq_walk_paths"):
        L.tkv_amq_walk_paths_ws_bytes.restype = u64
        L.tkv_amq_walk_paths_ws_bytes.argtypes = [u64]
        L.tkv_amq_walk_paths.restype = i32
        L.tkv_amq_walk_paths.argtypes = [vp, u64, vp, u64, vp, u64, vp, u64, vp, vp, u32, u64, vp, vp, u32,
                                         u64, vp, vp, vp, vp, vp, u64, vp, vp, u64, vp]
    if hasattr(L, "tkv_amq_get_keys"):
        L.tkv_amq_get_keys.restype = i32
        L.tkv_amq_get_keys.argtypes = [i32, vp, vp, u32,
                                       vp, u64, vp, u64, vp, u64, vp, u64, vp, vp, u32, u64,
                                       vp, vp, u32, u64,
                                       vp, vp, u32, u64, vp,
                                       u32, vp, vp, vp, vp, vp]
    if hasattr(L, "tkv_amq_get_values"):
        L.tkv_amq_get_values.restype = i32
        L.tkv_amq_get_values.argtypes = [i32, vp, vp, u32,
                                         vp, u64, vp, u64, vp, u64, vp, u64, vp, vp, u32, u64,
                                         vp, vp, u32, u64,
                                         vp, vp, u32, u64, vp,
                                         vp, vp, u32, u64,
                                         u32, vp, vp, vp, vp, vp]
    if hasattr(L, "tkv_amq_gather_values"):
        L.tkv_amq_gather_values.restype = i32
        L.tkv_amq_gather_values.argtypes = [vp, u64, vp, vp, u32, u64, u64, vp, u32, vp, vp]
    if hasattr(L, "tkv_amq_merge_leaves"):
        prun = ctypes.POINTER(MergeRun)
        L.tkv_amq_merge_leaves_ws_bytes.restype = u64
        L.tkv_amq_merge_leaves_ws_bytes.argtypes = [u64, u64, u64]
        L.tkv_amq_merge_leaves.restype = i32
        L.tkv_amq_merge_leaves.argtypes = [prun, prun, u64, u32, vp, vp, u64, vp, vp, vp, u64, vp]
        L.tkv_amq_merge_values_bound.restype = u64
        L.tkv_amq_merge_values_bound.argtypes = [u64, u64, u64]
        L.tkv_amq_gather_merged_ws_bytes.restype = u64
        L.tkv_amq_gather_merged_ws_bytes.argtypes = [u64]
        L.tkv_amq_gather_merged.restype = i32
        L.tkv_amq_gather_merged.argtypes = [vp, vp, u64, u64, prun, prun, vp, u32, vp, u64, vp, vp, u64, vp,
                                            vp, u64, vp]
    if hasattr(L, "tkv_amq_merge_levels"):
        prun = ctypes.POINTER(MergeRun)
        L.tkv_amq_merge_levels_ws_bytes.restype = u64
        L.tkv_amq_merge_levels_ws_bytes.argtypes = [u64, u32, u64]
        L.tkv_amq_merge_levels.restype = i32
        L.tkv_amq_merge_levels.argtypes = [prun, u32, u64, u32, vp, vp, u64, vp, vp, vp, u64, vp]
        L.tkv_amq_merge_levels_values_bound.restype = u64
        L.tkv_amq_merge_levels_values_bound.argtypes = [u64, u64]
        L.tkv_amq_gather_levels_ws_bytes.restype = u64
        L.tkv_amq_gather_levels_ws_bytes.argtypes = [u64]
        L.tkv_amq_gather_levels.restype = i32
        L.tkv_amq_gather_levels.argtypes = [vp, vp, u64, u64, prun, u32, vp, u32, vp, u64, vp, vp, u64, vp,
                                            vp, u64, vp]
    if hasattr(L, "tkv_amq_bloom_route"):
        L.tkv_amq_bloom_route_ws_bytes.restype = u64
        L.tkv_amq_bloom_route_ws_bytes.argtypes = [u64, u32]
        L.tkv_amq_bloom_route.restype = i32
        L.tkv_amq_bloom_route.argtypes = [vp, u64, vp, u32, u32, vp, vp, vp, u64, vp]
        L.tkv_amq_bloom_build_range_ws_bytes.restype = u64
        L.tkv_amq_bloom_build_range_ws_bytes.argtypes = [u64, u32, u32]
        L.tkv_amq_bloom_build_range.restype = i32
        L.tkv_amq_bloom_build_range.argtypes = [vp, u64, vp, u32, u32, u32, vp, vp, u64, vp]
        L.tkv_amq_bloom_route_records_ws_bytes.restype = u64
        L.tkv_amq_bloom_route_records_ws_bytes.argtypes = [u64, u32]
        L.tkv_amq_bloom_route_records.restype = i32
        L.tkv_amq_bloom_route_records.argtypes = [vp, u64, vp, u32, u32, u32, vp, vp, vp, u64, vp]
        L.tkv_amq_bloom_route_records_ex.restype = i32
        L.tkv_amq_bloom_route_records_ex.argtypes = [vp, u32, u64, vp, u32, u32, u32, vp, vp, vp, u64, vp]
        L.tkv_amq_bloom_build_range_records_ws_bytes.restype = u64
        L.tkv_amq_bloom_build_range_records_ws_bytes.argtypes = [u64, u32, u32]
        L.tkv_amq_bloom_build_range_records.restype = i32
        L.tkv_amq_bloom_build_range_records.argtypes = [vp, u64, vp, u32, u32, u32, u32, vp, vp, u64, vp]
    if hasattr(L, "tkv_amq_bloom_route_records_any"):
        L.tkv_amq_bloom_records_per_key.restype = u32
        L.tkv_amq_bloom_records_per_key.argtypes = [u32]
        L.tkv_amq_bloom_route_records_any_ws_bytes.restype = u64
        L.tkv_amq_bloom_route_records_any_ws_bytes.argtypes = [u64, u32, u32]
        L.tkv_amq_bloom_route_records_any.restype = i32
        L.tkv_amq_bloom_route_records_any.argtypes = [vp, vp, u32, u64, vp, u32, u32, u32, vp, vp, vp, u64, vp]
    if hasattr(L, "tkv_amq_bloom_route_plan"):
        prp = ctypes.POINTER(RoutePlan)
        L.tkv_amq_bloom_route_plan.restype = i32
        L.tkv_amq_bloom_route_plan.argtypes = [u64, u32, u32, u32, u32, prp]
        L.tkv_amq_bloom_route_blocks.restype = i32
        L.tkv_amq_bloom_route_blocks.argtypes = [vp, u32, u64, vp, prp, vp, u64, vp, u64, vp]
        L.tkv_amq_bloom_build_part_blocks.restype = i32
        L.tkv_amq_bloom_build_part_blocks.argtypes = [vp, u32, vp, prp, u32, vp, vp, u64, vp]
        L.tkv_amq_bloom_blocks_lost.restype = i32
        L.tkv_amq_bloom_blocks_lost.argtypes = [vp, u32, prp, vp]
    if hasattr(L, "tkv_amq_build_route"):
        L.tkv_amq_build_route.restype = i32
        L.tkv_amq_build_route.argtypes = [i32, u32, i32, i32, u32, u64, u32, vp, i32, u64,
                                          ctypes.POINTER(BuildRoute), vp]
    if hasattr(L, "tkv_amq_bloom_tile_blocks"):
        L.tkv_amq_bloom_tile_blocks.restype = u32
        L.tkv_amq_bloom_tile_blocks.argtypes = []
        L.tkv_amq_bloom_range_max_tiles.restype = u32
        L.tkv_amq_bloom_range_max_tiles.argtypes = [i32]
    _lib = L
    return L


def check(status: int, what: str) -> None:
    if status != OK:
        raise TkvAmqError(status, what)


def version() -> str:
    return lib().tkv_amq_version().decode()
