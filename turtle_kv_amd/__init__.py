"""turtle_kv_amd -- MI355X-native AMQ filter engine for TurtleKV's per-leaf Bloom / VQF
build-and-probe path.  Compute runs in HIP kernels (libtkv_amq.so); this
package is the host-side mirror of the reference's filter API."""
from . import abi
from .abi import BLOOM, VQF, TkvAmqError
from .filters import (BoolStatus, FilterPage, FilterPlan, KeyBatch, KeyQuery, PackedVqfFilter,
                      build_all_filters, build_bloom_filter_for_leaf, build_filter_for_leaf_in_job,
                      build_quotient_filter_for_leaf, filter_bits_per_key, gen_keys16,
                      bloom_query_hashes, bloom_probe_hashed, HostFilterPipeline,
                      plan_filters, probe_filters, vqf_filter_load_factor, vqf_hash_val,
                      vqf_nslots_for_size, vqf_probe_hashed, vqf_required_size, key_views,
                      stage_keys, BloomFilterMetrics, QuotientFilterMetrics,
                      plan_filter_stats, record_filter_metrics, TreeOptions, plan_filter_pages,
                      page_header_fields, ProbeMetrics, KeyQueryMetrics, probe_paths,
                      PathProbeResult, path_probe_workspace_bytes, OpenedFilters, open_filters,
                      open_filters_device, scan_filters, scan_filters_device,
                      scan_filters_workspace_bytes, filter_fill, verify_members,
                      verify_members_device, verify_members_workspace_bytes, find_keys,
                      find_keys_device, FindResult, FindCounts, TreeIndex, WalkResult, walk_paths,
                      walk_paths_device, walk_paths_workspace_bytes, get_keys, get_keys_device,
                      GetResult, GetCounts, get_values, get_values_device, gather_values_device,
                      ValueResult, ValueCounts, merge_leaves, merge_leaves_device,
                      gather_merged_device, merge_run, merge_leaves_workspace_bytes,
                      gather_merged_workspace_bytes, merge_values_bound, MergeResult, MergeCounts)

__all__ = [
    "abi", "BLOOM", "VQF", "TkvAmqError", "BoolStatus", "FilterPage", "FilterPlan", "KeyBatch",
    "KeyQuery", "PackedVqfFilter", "build_all_filters", "build_bloom_filter_for_leaf",
    "build_filter_for_leaf_in_job", "build_quotient_filter_for_leaf", "filter_bits_per_key",
    "gen_keys16", "plan_filters", "probe_filters", "vqf_filter_load_factor", "vqf_hash_val",
    "vqf_nslots_for_size", "vqf_probe_hashed", "vqf_required_size", "bloom_query_hashes",
    "bloom_probe_hashed", "HostFilterPipeline", "key_views", "stage_keys",
    "BloomFilterMetrics", "QuotientFilterMetrics", "plan_filter_stats", "record_filter_metrics",
    "TreeOptions", "plan_filter_pages", "page_header_fields", "ProbeMetrics", "KeyQueryMetrics",
    "probe_paths", "PathProbeResult", "path_probe_workspace_bytes", "OpenedFilters",
    "open_filters", "open_filters_device", "scan_filters", "scan_filters_device",
    "scan_filters_workspace_bytes", "filter_fill", "verify_members", "verify_members_device",
    "verify_members_workspace_bytes", "find_keys", "find_keys_device", "FindResult", "FindCounts",
    "TreeIndex", "WalkResult", "walk_paths", "walk_paths_device", "walk_paths_workspace_bytes",
    "get_keys", "get_keys_device", "GetResult", "GetCounts",
    "get_values", "get_values_device", "gather_values_device", "ValueResult", "ValueCounts",
    "merge_leaves", "merge_leaves_device", "gather_merged_device", "merge_run",
    "merge_leaves_workspace_bytes", "gather_merged_workspace_bytes", "merge_values_bound", "MergeResult",
    "MergeCounts",
]
