// turtle_kv_amd/filter_builder.hpp -- C++ host mirror of TurtleKV's filter API over the
// tkv_amq C ABI (libtkv_amq.so, HIP/gfx950).  Header-only, C++17.
//
// Reference interface (mathworks/turtle_kv, src/turtle_kv/...) -> this header:
//   vqf_hash_val                          vqf_filter_page_view.hpp:32-35   (device: vqf_hash_val_batch)
//   vqf_filter_load_factor<TAG_BITS>      vqf_filter_page_view.hpp:39-59   vqf_filter_load_factor<T>
//   PackedVqfFilter                       vqf_filter_page_view.hpp:63-131  PackedVqfFilter (layout)
//   TreeOptions::filter_bits_per_key      tree/tree_options.hpp:155-164    filter_bits_per_key
//   build_bloom_filter_for_leaf           tree/filter_builder.hpp:109-152  build_bloom_filter_for_leaf
//   build_quotient_filter_for_leaf        tree/filter_builder.hpp:221-301  build_quotient_filter_for_leaf
//   build_filter_for_leaf_in_job          tree/filter_builder.hpp:307-331  build_filter_for_leaf_in_job
//   TreeSerializeContext::build_all_pages tree/tree_serialize_context.cpp:62-115 (filter half)
//                                                                          FilterBatchBuilder
//   KeyQuery::reject_page                 tree/key_query.hpp:149-247       KeyQuery::reject_page
//   KeyQuery::Metrics                     tree/key_query.hpp:36-60         KeyQuery::Metrics
//   TreeOptions (filter sizing)           tree/tree_options.hpp:149-258    TreeOptions
//   FilterPageAlloc page image            tree/filter_builder.hpp:58-105,231-237,293-296
//                                                                          FilterBatchBuilder::plan_pages
//   reject_page's read of a loaded page   tree/key_query.hpp:149-247, vqf_filter_page_view.hpp:96-100
//                                                                          open_filter_pages, scan_filters
//   find_pivot_containing / find_key      tree/algo/nodes.hpp:48-71,158-187, tree/algo/segmented_levels.hpp:340-369
//                                                                          TreeIndex, KeyQuery::walk_paths
//   NodeAlgorithms::find_key, no combine  tree/algo/nodes.hpp:158-187, tree/algo/segments.hpp:166-206
//                                                                          TreeIndex::get_host, KeyQuery::get_keys
//   ... with combine_in_place             core/value_view.hpp:316-361, core/packed_key_value.hpp:18-23
//                                                                          TreeIndex::get_values_host, KeyQuery::get_values
//   {BatchUpdate} + {PackedLeafPage}      tree/subtree.cpp:170-231, core/algo/merge_compact_edits.hpp:26-148
//                                                                          merge_leaves
//   InMemoryNode::push_levels_to_merge    tree/in_memory_node.cpp:827-866, merge_compact_edits over K levels
//                                                                          merge_levels
//
// The single-leaf functions take the leaf's keys as host string views (the reference's
// `items` range of EditView keys, tombstones included) and fill a host page payload
// buffer, staging through the device.  The batched FilterBatchBuilder works on
// device-resident keys and is the fast path.  There is no CPU implementation here: every
// filter byte is computed by the HIP kernels.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <optional>
#include <string>
#include <string_view>
#include <thread>
#include <utility>
#include <vector>

#include "../tkv_amq.h"

namespace turtle_kv_amd {

using u8 = std::uint8_t;
using u16 = std::uint16_t;
using u32 = std::uint32_t;
using u64 = std::uint64_t;
using usize = std::size_t;

// ---------------------------------------------------------------------------------------
// Status (batt::Status numbering)
// ---------------------------------------------------------------------------------------
struct Status {
  int code = TKV_AMQ_OK;
  std::string what;
  bool ok() const { return code == TKV_AMQ_OK; }
  static Status from(int c, const char* w) { return Status{c, c == TKV_AMQ_OK ? "" : w}; }
  std::string to_string() const
  {
    return std::string(tkv_amq_status_string(code)) + (what.empty() ? "" : ": " + what);
  }
};
inline Status OkStatus() { return Status{}; }

#define TKV_AMQ_REQUIRE_OK(expr)          \
  do {                                    \
    ::turtle_kv_amd::Status s_ = (expr);  \
    if (!s_.ok()) return s_;              \
  } while (0)

// ---------------------------------------------------------------------------------------
// constants and sizing (config.hpp:20-24, vqf_filter_page_view.hpp:26-28)
// ---------------------------------------------------------------------------------------
enum class FilterKind : int { kBloom = TKV_AMQ_BLOOM, kQuotient = TKV_AMQ_VQF };
inline constexpr FilterKind kDefaultFilterKind = FilterKind::kQuotient;  // TURTLE_KV_USE_QUOTIENT_FILTER 1
inline constexpr u64 kVqfHashSeed = 0x9d0924dc03e79a75ull;
inline constexpr usize kMinQuotientFilterBitsPerKey = 12;
inline constexpr double kMaxQuotientFilterLoadFactor = 0.85;
inline constexpr u16 kDefaultFilterBitsPerKey = 12;
inline constexpr usize kPackedPageHeaderSize = 64;

template <int TAG_BITS>
inline double vqf_filter_load_factor(usize bits_per_key)
{
  static_assert(TAG_BITS == 8 || TAG_BITS == 16, "TAG_BITS must be 8 or 16");
  return tkv_amq_vqf_load_factor(TAG_BITS, bits_per_key);
}

inline usize filter_bits_per_key(std::optional<u16> requested,
                                 FilterKind kind = kDefaultFilterKind)
{
  return (usize)tkv_amq_filter_bits_per_key((int)kind, requested.value_or(kDefaultFilterBitsPerKey));
}

// The filter part of TreeOptions (tree/tree_options.hpp:43-395): bits per key with the VQF
// clamp, and the filter page size from the leaf size and key/value size hints.  `kind` stands
// for the compile-time filter switch (config.hpp:20-24).
class TreeOptions
{
 public:
  static constexpr u32 kDefaultKeySizeHint = 24;     // :58
  static constexpr u32 kDefaultValueSizeHint = 100;  // :59

  explicit TreeOptions(FilterKind kind = kDefaultFilterKind) : kind_{kind} {}
  static TreeOptions with_default_values(FilterKind kind = kDefaultFilterKind) { return TreeOptions{kind}; }

  u64 leaf_size() const { return u64{1} << leaf_size_log2_; }
  TreeOptions& set_leaf_size_log2(u8 size_log2) { leaf_size_log2_ = size_log2; return *this; }
  usize leaf_data_size() const { return (usize)tkv_amq_leaf_data_size(leaf_size()); }

  TreeOptions& set_filter_bits_per_key(std::optional<u16> bpk) { filter_bits_per_key_ = bpk; return *this; }
  usize filter_bits_per_key() const { return turtle_kv_amd::filter_bits_per_key(filter_bits_per_key_, kind_); }

  TreeOptions& set_key_size_hint(u32 n) { key_size_hint_ = n; return *this; }
  TreeOptions& set_value_size_hint(u32 n) { value_size_hint_ = n; return *this; }
  u32 key_size_hint() const { return key_size_hint_; }
  u32 value_size_hint() const { return value_size_hint_; }
  usize expected_items_per_leaf() const
  {
    return (usize)tkv_amq_expected_items_per_leaf(leaf_size(), key_size_hint_, value_size_hint_);
  }

  TreeOptions& set_filter_page_size_log2(u8 size_log2) { filter_page_size_log2_ = size_log2; return *this; }
  u32 filter_page_size_log2() const
  {
    if (filter_page_size_log2_) return *filter_page_size_log2_;
    return tkv_amq_filter_page_size_log2((int)kind_, leaf_size(), key_size_hint_, value_size_hint_,
                                         filter_bits_per_key_.value_or(kDefaultFilterBitsPerKey));
  }
  u64 filter_page_size() const { return u64{1} << filter_page_size_log2(); }
  // the payload the filter builders size against: the page minus the llfs PackedPageHeader
  u64 filter_page_payload_size() const { return filter_page_size() - kPackedPageHeaderSize; }

 private:
  FilterKind kind_;
  u8 leaf_size_log2_ = 21;  // 2 MiB (tree_options.cpp:20-21)
  std::optional<u16> filter_bits_per_key_;
  std::optional<u8> filter_page_size_log2_;
  u32 key_size_hint_ = kDefaultKeySizeHint;
  u32 value_size_hint_ = kDefaultValueSizeHint;
};

// payload capacity of the default TreeOptions' filter page at this bits/key
inline u64 default_filter_page_payload_size(usize bits_per_key, FilterKind kind)
{
  return TreeOptions{kind}.set_filter_bits_per_key((u16)bits_per_key).filter_page_payload_size();
}

// vqf_metadata + PackedVqfFilter on-page layout (little-endian)
struct VqfMetadata {
  u64 total_size_in_bytes;
  u64 key_remainder_bits;
  u64 range;
  u64 nblocks;
  u64 nelts;
  u64 nslots;
};
struct PackedVqfFilter {
  static constexpr u64 kMagic = 0x16015305e0f43a7dull;
  u64 magic;
  u64 src_page_id;
  u64 hash_seed;
  u64 hash_mask;
  VqfMetadata metadata;
};
static_assert(sizeof(PackedVqfFilter) == 32 + sizeof(VqfMetadata), "vqf_filter_page_view.hpp:128");

struct PackedBloomFilterPage {
  static constexpr u64 kMagic = 0xca6f49a0f3f8a4b0ull;
  u64 magic;
  u64 bit_count;
  u64 src_page_id;
  u64 xxh3_checksum;
  u64 word_count;
  u32 block_count;
  u16 hash_count;
  u8 layout;  // 2 = kBlocked512
  u8 reserved0;
  u64 item_count;
  u64 reserved1;
};
static_assert(sizeof(PackedBloomFilterPage) == 64, "tkv-amq v1 Bloom header");

// ---------------------------------------------------------------------------------------
// device buffer helper (RAII)
// ---------------------------------------------------------------------------------------
class DeviceBuffer
{
 public:
  DeviceBuffer() = default;
  explicit DeviceBuffer(usize n) { resize(n); }
  ~DeviceBuffer() { reset(); }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_{o.p_}, n_{o.n_} { o.p_ = nullptr; o.n_ = 0; }

  bool resize(usize n)
  {
    if (n <= n_) return true;
    reset();
    if (hipMalloc(&p_, n ? n : 1) != hipSuccess) { p_ = nullptr; return false; }
    n_ = n;
    return true;
  }
  void reset()
  {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  template <typename T = u8>
  T* get() const { return static_cast<T*>(p_); }
  usize size() const { return n_; }

 private:
  void* p_ = nullptr;
  usize n_ = 0;
};

// ---------------------------------------------------------------------------------------
// FilterBatchBuilder: every leaf filter of one build_all_pages queue in one device call
// ---------------------------------------------------------------------------------------
class FilterBatchBuilder
{
 public:
  FilterBatchBuilder(FilterKind kind, usize bits_per_key, u64 page_payload_bytes,
                     u64 out_stride = 0)
      : kind_{kind}, bpk_{bits_per_key}, cap_{page_payload_bytes}, stride_{out_stride}
  {
  }

  // Whole filter pages of 2^page_size_log2 bytes, leaf s at s << log2: the PackedPageHeader
  // fields the builders set, then the payload (tkv_amq_plan_pages).
  static FilterBatchBuilder pages(FilterKind kind, usize bits_per_key, u32 page_size_log2)
  {
    FilterBatchBuilder b{kind, bits_per_key, (u64{1} << page_size_log2) - kPackedPageHeaderSize,
                         u64{1} << page_size_log2};
    b.page_log2_ = page_size_log2;
    return b;
  }

  // Queue one leaf whose keys occupy the next n_keys slots of the device key array.
  u32 add_leaf(u64 leaf_page_id, u64 n_keys)
  {
    counts_.push_back(n_keys);
    page_ids_.push_back(leaf_page_id);
    return (u32)(counts_.size() - 1);
  }

  Status plan()
  {
    segs_.resize(counts_.size());
    const int st =
        page_log2_ ? tkv_amq_plan_pages((int)kind_, counts_.data(), page_ids_.data(), (u32)counts_.size(),
                                        (u32)bpk_, page_log2_, segs_.data(), &total_out_, &ws_bytes_,
                                        &max_blocks_)
                   : tkv_amq_plan((int)kind_, counts_.data(), page_ids_.data(), (u32)counts_.size(),
                                  (u32)bpk_, cap_, stride_, segs_.data(), &total_out_, &ws_bytes_,
                                  &max_blocks_);
    if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_plan");
    if (!d_segs_.resize(segs_.size() * sizeof(tkv_amq_segment)) || !d_ws_.resize(ws_bytes_))
      return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
    if (hipMemcpy(d_segs_.get(), segs_.data(), segs_.size() * sizeof(tkv_amq_segment),
                  hipMemcpyHostToDevice) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy plan");
    planned_ = true;
    return OkStatus();
  }

  // Device keys: fixed length (d_key_offsets == nullptr, key_stride bytes each) or
  // variable length (d_key_offsets[n+1]).  Asynchronous on `stream`; call check().
  Status build_all(const u8* d_keys, u32 key_stride, const u64* d_key_offsets, u8* d_out,
                   hipStream_t stream = nullptr)
  {
    if (!planned_) TKV_AMQ_REQUIRE_OK(plan());
    u64 n = 0;
    for (u64 c : counts_) n += c;
    // (_ex with the host plan: in a Bloom batch, leaves of 16- or 24-byte keys past 5 LDS
    // windows -- other key shapes past 16 -- take the tiled build, up to 40 per launch)
    return Status::from(tkv_amq_build_ex((int)kind_, d_keys, d_key_offsets, key_stride, n,
                                         d_segs_.get<tkv_amq_segment>(), segs_.data(), (u32)segs_.size(),
                                         max_blocks_, d_out, d_ws_.get(), ws_bytes_, stream),
                        "tkv_amq_build_ex");
  }

  Status check(hipStream_t stream = nullptr) const
  {
    return Status::from(tkv_amq_build_check((int)kind_, d_ws_.get(), ws_bytes_, stream),
                        "vqf_insert (filter_builder.hpp:211)");
  }

  Status probe(const u8* d_filters, const u8* d_queries, u32 query_stride,
               const u64* d_query_offsets, u64 n_queries, const u32* d_query_leaf, u8* d_result,
               hipStream_t stream = nullptr) const
  {
    return Status::from(tkv_amq_probe((int)kind_, d_filters, d_segs_.get<tkv_amq_segment>(),
                                      (u32)segs_.size(), d_queries, d_query_offsets, query_stride,
                                      n_queries, d_query_leaf, d_result, stream),
                        "tkv_amq_probe");
  }

  // After build_all (same keys, the built d_out): does every leaf's filter hold every key of
  // the leaf?  Per leaf the tkv_amq_member_check (missing != 0: do not commit that leaf's filter
  // page).  Synchronises `stream`; defined below verify_members.
  Status verify(const u8* d_keys, u32 key_stride, const u64* d_key_offsets, const u8* d_out,
                std::vector<tkv_amq_member_check>& out, hipStream_t stream = nullptr) const;

  const std::vector<tkv_amq_segment>& segments() const { return segs_; }
  u64 total_out_bytes() const { return total_out_; }
  const tkv_amq_segment* device_segments() const { return d_segs_.get<tkv_amq_segment>(); }

 private:
  FilterKind kind_;
  usize bpk_;
  u64 cap_, stride_;
  std::vector<u64> counts_, page_ids_;
  std::vector<tkv_amq_segment> segs_;
  u64 total_out_ = 0, ws_bytes_ = 0;
  u32 max_blocks_ = 0;
  u32 page_log2_ = 0;
  bool planned_ = false;
  DeviceBuffer d_segs_, d_ws_;
};

// ---------------------------------------------------------------------------------------
// open built filter pages without a plan, and scan their fill (tkv_amq_open_filters,
// tkv_amq_scan_filters): a store restarting on a checkpoint has filter bytes and no plan
// ---------------------------------------------------------------------------------------
// Where filter s lives in the device buffer -- exactly one of: d_offsets[s] (device array),
// s * stride, or the page s << page_size_log2 (FilterBatchBuilder::pages' layout).
struct FilterLocation {
  const u64* d_offsets = nullptr;
  u64 stride = 0;
  u32 page_size_log2 = 0;
};

// The segments the device reconstructed from the filter bytes (host copy and the device copy
// the probes take), each filter's TKV_AMQ_OPEN_* code and the count of each code.  A filter
// that failed is a "no filter" segment: every probe answers 1 (kUnknown) for it.  The segments
// serve the probes and scan_filters; building into them is not supported.
struct OpenedFilterPages {
  std::vector<tkv_amq_segment> segments;
  std::vector<u32> status;
  u32 summary[7] = {0, 0, 0, 0, 0, 0, 0};
  DeviceBuffer d_segments;

  bool all_ok() const { return summary[TKV_AMQ_OPEN_OK] == status.size(); }
  const tkv_amq_segment* device_segments() const { return d_segments.get<tkv_amq_segment>(); }
};

// Synchronises `stream` (the segments and codes are copied back).
inline Status open_filter_pages(FilterKind kind, const u8* d_filters, u64 total_bytes,
                                const FilterLocation& where, u32 n_filters, OpenedFilterPages& out,
                                hipStream_t stream = nullptr)
{
  out.segments.assign(n_filters, tkv_amq_segment{});
  out.status.assign(n_filters, 0);
  if (tkv_amq_device_count() == 0) {
    // nothing can be allocated: the entry point's own answer (InvalidArgument for a bad call,
    // else Unavailable); it launches nothing, so host stand-ins serve as its output buffers
    tkv_amq_segment g{};
    u32 w[7];
    return Status::from(tkv_amq_open_filters((int)kind, d_filters, total_bytes, where.d_offsets, where.stride,
                                             where.page_size_log2, n_filters, &g, w, w, stream),
                        "tkv_amq_open_filters");
  }
  DeviceBuffer d_status, d_summary;
  if (!out.d_segments.resize(sizeof(tkv_amq_segment) * n_filters) || !d_status.resize(4 * usize{n_filters}) ||
      !d_summary.resize(sizeof(out.summary)))
    return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
  const int st = tkv_amq_open_filters((int)kind, d_filters, total_bytes, where.d_offsets, where.stride,
                                      where.page_size_log2, n_filters, out.d_segments.get<tkv_amq_segment>(),
                                      d_status.get<u32>(), d_summary.get<u32>(), stream);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_open_filters");
  if (hipMemcpyAsync(out.segments.data(), out.d_segments.get(), sizeof(tkv_amq_segment) * n_filters,
                     hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(out.status.data(), d_status.get(), 4 * usize{n_filters}, hipMemcpyDeviceToHost, stream) !=
          hipSuccess ||
      hipMemcpyAsync(out.summary, d_summary.get(), sizeof(out.summary), hipMemcpyDeviceToHost, stream) !=
          hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy opened segments");
  return OkStatus();
}

// One read-only pass over every filter's blocks (plan segments or opened ones): set bits /
// occupied slots, the header's item count, full / empty blocks, the fullest block, and the VQF
// blocks that break a block invariant.  Synchronises `stream`.
inline Status scan_filters(FilterKind kind, const u8* d_filters, const tkv_amq_segment* d_segs, u32 n_segs,
                           std::vector<tkv_amq_filter_stats>& out, hipStream_t stream = nullptr)
{
  out.assign(n_segs, tkv_amq_filter_stats{});
  const u64 ws_bytes = tkv_amq_scan_filters_ws_bytes(n_segs);
  if (tkv_amq_device_count() == 0)
    return Status::from(n_segs && (!d_filters || !d_segs) ? TKV_AMQ_INVALID_ARGUMENT : TKV_AMQ_UNAVAILABLE,
                        "tkv_amq_scan_filters");
  DeviceBuffer d_stats, d_ws;
  if (!d_stats.resize(sizeof(tkv_amq_filter_stats) * usize{n_segs}) || !d_ws.resize(ws_bytes))
    return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
  const int st = tkv_amq_scan_filters((int)kind, d_filters, d_segs, n_segs, d_stats.get<tkv_amq_filter_stats>(),
                                      d_ws.get(), ws_bytes, stream);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_scan_filters");
  if (hipMemcpyAsync(out.data(), d_stats.get(), sizeof(tkv_amq_filter_stats) * usize{n_segs},
                     hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy stats");
  return OkStatus();
}

// Does every key of every leaf pass its own filter (tkv_amq_verify_members)?  One leaf-major
// device pass over the filters (plan segments or opened ones) and their keys; per leaf the count
// of keys the filter rejects -- what tkv_amq_probe would answer 0 for -- the smallest such key
// index and the TKV_AMQ_VERIFY_* flags.  Leaf s holds keys [d_key_begin[s], d_key_begin[s+1])
// (device, n_segs + 1 entries: the form for opened segments) or, with d_key_begin == nullptr, the
// segment's own [key_begin, key_begin + n_keys).  max_seg_blocks: the LDS sizing hint (the
// plan's, or 0).  total_missing (may be nullptr): the sum.  Synchronises `stream`.
inline Status verify_members(FilterKind kind, const u8* d_filters, const tkv_amq_segment* d_segs, u32 n_segs,
                             u32 max_seg_blocks, const u8* d_keys, u32 key_stride, const u64* d_key_offsets,
                             u64 n_keys, const u64* d_key_begin, std::vector<tkv_amq_member_check>& out,
                             u64* total_missing = nullptr, hipStream_t stream = nullptr)
{
  out.assign(n_segs, tkv_amq_member_check{~u64{0}, 0, 0});
  if (total_missing) *total_missing = 0;
  const u64 ws_bytes = tkv_amq_verify_members_ws_bytes(n_segs);
  if (tkv_amq_device_count() == 0) {
    // nothing can be allocated: the entry point's own answer (InvalidArgument for a bad call,
    // else Unavailable); it launches nothing, so aligned host stand-ins serve as its buffers
    alignas(16) tkv_amq_member_check r{};
    return Status::from(tkv_amq_verify_members((int)kind, d_filters, d_segs, n_segs, max_seg_blocks, d_keys,
                                               d_key_offsets, key_stride, n_keys, d_key_begin, &r, nullptr, &r,
                                               ws_bytes, stream),
                        "tkv_amq_verify_members");
  }
  DeviceBuffer d_result, d_total, d_ws;
  if (!d_result.resize(sizeof(tkv_amq_member_check) * usize{n_segs}) || !d_total.resize(sizeof(u64)) ||
      !d_ws.resize(ws_bytes))
    return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
  const int st = tkv_amq_verify_members((int)kind, d_filters, d_segs, n_segs, max_seg_blocks, d_keys,
                                        d_key_offsets, key_stride, n_keys, d_key_begin,
                                        d_result.get<tkv_amq_member_check>(), d_total.get<u64>(), d_ws.get(),
                                        ws_bytes, stream);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_verify_members");
  u64 total = 0;
  if (hipMemcpyAsync(out.data(), d_result.get(), sizeof(tkv_amq_member_check) * usize{n_segs},
                     hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(&total, d_total.get(), sizeof(u64), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy member checks");
  if (total_missing) *total_missing = total;
  return OkStatus();
}

inline Status FilterBatchBuilder::verify(const u8* d_keys, u32 key_stride, const u64* d_key_offsets, const u8* d_out,
                                         std::vector<tkv_amq_member_check>& out, hipStream_t stream) const
{
  if (!planned_) return Status::from(TKV_AMQ_INVALID_ARGUMENT, "FilterBatchBuilder::verify before plan()");
  u64 n = 0;
  for (u64 c : counts_) n += c;
  return verify_members(kind_, d_out, d_segs_.get<tkv_amq_segment>(), (u32)segs_.size(), max_blocks_, d_keys,
                        key_stride, d_key_offsets, n, nullptr, out, nullptr, stream);
}

// occupied / capacity of one scanned filter: set bits over 512 * n_blocks (Bloom), occupied tag
// slots over n_blocks * slots (VQF); 0 without a filter
inline double filter_fill(const tkv_amq_segment& seg, const tkv_amq_filter_stats& st)
{
  const double per = seg.hash_count ? 512.0 : seg.tag_bits == 8 ? 48.0 : seg.tag_bits == 16 ? 28.0 : 0.0;
  const double cap = per * (double)seg.n_blocks;
  return cap > 0 ? (double)st.occupied / cap : 0.0;
}

// ---------------------------------------------------------------------------------------
// single-leaf entry points (host keys -> host page payload)
// ---------------------------------------------------------------------------------------
namespace detail {

// std::string_view is read in place as tkv_amq_key_view when the layouts agree (libstdc++:
// {size, data}); otherwise the views are copied into tkv_amq_key_view records first.
inline bool string_view_is_key_view()
{
  static_assert(sizeof(std::string_view) == sizeof(tkv_amq_key_view), "string_view size");
  const char probe[2] = {'a', 0};
  const std::string_view sv(probe, 1);
  tkv_amq_key_view kv;
  std::memcpy(&kv, &sv, sizeof(kv));
  return kv.size == 1 && kv.data == reinterpret_cast<const u8*>(probe);
}

inline Status stage_keys(const std::vector<std::string_view>& items, DeviceBuffer& d_keys,
                         DeviceBuffer& d_offs, bool& fixed, u32& stride)
{
  const usize n = items.size();
  fixed = n > 0;
  stride = n ? (u32)items[0].size() : 16;
  u64 total = 0;
  for (usize i = 0; i < n; ++i) {
    total += items[i].size();
    fixed = fixed && items[i].size() == stride;
  }
  if (fixed && stride == 0) fixed = false;
  std::vector<tkv_amq_key_view> copied;
  const void* views = items.data();
  if (!string_view_is_key_view()) {
    copied.resize(n);
    for (usize i = 0; i < n; ++i)
      copied[i] = tkv_amq_key_view{items[i].size(), reinterpret_cast<const u8*>(items[i].data())};
    views = copied.data();
  }
  // tkv_amq_stage_keys: the host gather (the EditView key range -> one contiguous buffer)
  std::vector<u64> offs(n + 1, 0);
  std::vector<u8> blob(total ? total : 1);
  const int st = tkv_amq_stage_keys(views, sizeof(tkv_amq_key_view), n, fixed ? stride : 0,
                                    blob.data(), blob.size(), fixed ? nullptr : offs.data(), 0);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_stage_keys");
  if (!d_keys.resize(blob.size()) || !d_offs.resize(offs.size() * 8))
    return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
  if (hipMemcpy(d_keys.get(), blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_offs.get(), offs.data(), offs.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy keys");
  return OkStatus();
}

// Per-thread scratch for the single-leaf entry points, which the reference calls once per
// leaf from its worker threads (tree/tree_serialize_context.cpp:71-75): a stream of the
// thread's own and grow-only device / pinned host buffers, so a call makes no hipMalloc /
// hipFree (hipFree synchronises the whole device, which would serialise the workers) and
// only waits for its own stream.
struct LeafScratch {
  hipStream_t stream = nullptr;
  DeviceBuffer d_keys, d_offs, d_segs, d_ws, d_out;
  u8* h_keys = nullptr;
  usize h_keys_cap = 0;
  u64* h_offs = nullptr;
  usize h_offs_cap = 0;
  u8* h_io = nullptr;  // pinned: [segment 64 B][status 4 B .. 64 B][payload]
  usize h_io_cap = 0;
  std::vector<tkv_amq_key_view> views;

  ~LeafScratch()
  {
    if (h_keys) (void)hipHostFree(h_keys);
    if (h_offs) (void)hipHostFree(h_offs);
    if (h_io) (void)hipHostFree(h_io);
    if (stream) (void)hipStreamDestroy(stream);
  }
  bool ensure_stream() { return stream || hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess; }
  template <typename T>
  static bool grow_pinned(T*& p, usize& cap, usize n)
  {
    if (n <= cap) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)) != hipSuccess) return false;
    cap = n;
    return true;
  }
};

inline LeafScratch& leaf_scratch()
{
  thread_local LeafScratch s;
  return s;
}

inline Status build_one(FilterKind kind, usize bpk, u64 leaf_page_id,
                        const std::vector<std::string_view>& items,
                        std::vector<u8>& page_payload, u64 page_payload_bytes)
{
  if (bpk == 0) return OkStatus();  // filter_builder.hpp:115-117, :227-229
  if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");
  LeafScratch& sc = leaf_scratch();
  if (!sc.ensure_stream()) return Status::from(TKV_AMQ_INTERNAL, "hipStreamCreate");
  const u64 n = items.size();
  tkv_amq_segment seg{};
  u64 total_out = 0, ws_bytes = 0;
  u32 max_blocks = 0;
  int st = tkv_amq_plan((int)kind, &n, &leaf_page_id, 1, (u32)bpk, page_payload_bytes, 0, &seg,
                        &total_out, &ws_bytes, &max_blocks);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_plan");

  // stage the keys (the EditView key range) into pinned memory: one fixed stride if every key
  // has the same length, else bytes + offsets
  u64 bytes = 0;
  bool fixed = n > 0;
  const u32 stride = n ? (u32)items[0].size() : 16;
  for (const auto& k : items) {
    bytes += k.size();
    fixed = fixed && k.size() == stride;
  }
  fixed = fixed && stride != 0;
  const void* views = items.data();
  if (!string_view_is_key_view()) {
    sc.views.resize(n);
    for (u64 i = 0; i < n; ++i)
      sc.views[i] = tkv_amq_key_view{items[i].size(), reinterpret_cast<const u8*>(items[i].data())};
    views = sc.views.data();
  }
  if (!LeafScratch::grow_pinned(sc.h_keys, sc.h_keys_cap, bytes ? bytes : 1) ||
      !LeafScratch::grow_pinned(sc.h_offs, sc.h_offs_cap, n + 1))
    return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipHostMalloc");
  st = tkv_amq_stage_keys(views, sizeof(tkv_amq_key_view), n, fixed ? stride : 0, sc.h_keys,
                          sc.h_keys_cap, fixed ? nullptr : sc.h_offs, 1);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_stage_keys");
  if (!sc.d_keys.resize(bytes ? bytes : 1) || !sc.d_offs.resize(8 * (n + 1)) ||
      !sc.d_segs.resize(sizeof(seg)) || !sc.d_ws.resize(ws_bytes) || !sc.d_out.resize(total_out) ||
      !LeafScratch::grow_pinned(sc.h_io, sc.h_io_cap, 128 + (usize)seg.payload_bytes))
    return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
  // everything below is asynchronous on the thread's stream, from and to pinned memory, with
  // one synchronisation at the end (the VQF failure word comes back with the payload)
  std::memcpy(sc.h_io, &seg, sizeof(seg));
  u32* h_status = reinterpret_cast<u32*>(sc.h_io + 64);
  *h_status = 0;
  u8* h_payload = sc.h_io + 128;
  hipStream_t s = sc.stream;
  const u32 used = seg.payload_bytes;
  if (hipMemcpyAsync(sc.d_keys.get(), sc.h_keys, bytes, hipMemcpyHostToDevice, s) != hipSuccess ||
      (!fixed && hipMemcpyAsync(sc.d_offs.get(), sc.h_offs, 8 * (n + 1), hipMemcpyHostToDevice, s) != hipSuccess) ||
      hipMemcpyAsync(sc.d_segs.get(), sc.h_io, sizeof(seg), hipMemcpyHostToDevice, s) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemcpyAsync keys");
  st = tkv_amq_build((int)kind, sc.d_keys.get(), fixed ? nullptr : sc.d_offs.get<u64>(),
                     fixed ? stride : 0, n, sc.d_segs.get<tkv_amq_segment>(), 1, max_blocks,
                     sc.d_out.get(), sc.d_ws.get(), ws_bytes, s);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_build");
  if (hipMemcpyAsync(h_payload, sc.d_out.get(), used, hipMemcpyDeviceToHost, s) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemcpyAsync payload");
  // (the leaf's nelts word: its failure flags, tkv_amq.h)
  if ((kind == FilterKind::kQuotient && ws_bytes >= TKV_AMQ_VQF_NELTS_OFFSET + 4 &&
       hipMemcpyAsync(h_status, sc.d_ws.get<u8>() + TKV_AMQ_VQF_NELTS_OFFSET, 4, hipMemcpyDeviceToHost,
                      s) != hipSuccess) ||
      hipStreamSynchronize(s) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipStreamSynchronize");
  if (*h_status & TKV_AMQ_VQF_FLAG_WORKSPACE) return Status::from(TKV_AMQ_INVALID_ARGUMENT, "workspace");
  if (*h_status & TKV_AMQ_VQF_FLAG_OVERFLOW)
    return Status::from(TKV_AMQ_INTERNAL, "vqf_insert (filter_builder.hpp:211)");
  page_payload.assign(page_payload_bytes ? page_payload_bytes : used, 0);
  std::memcpy(page_payload.data(), h_payload, used);
  return OkStatus();
}

}  // namespace detail

inline Status build_bloom_filter_for_leaf(usize filter_bits_per_key, u64 leaf_page_id,
                                          const std::vector<std::string_view>& items,
                                          std::vector<u8>& page_payload,
                                          u64 page_payload_bytes = 0)
{
  return detail::build_one(FilterKind::kBloom, filter_bits_per_key, leaf_page_id, items,
                           page_payload, page_payload_bytes);
}

inline Status build_quotient_filter_for_leaf(usize filter_bits_per_key, u64 leaf_page_id,
                                             const std::vector<std::string_view>& items,
                                             std::vector<u8>& page_payload,
                                             u64 page_payload_bytes)
{
  return detail::build_one(FilterKind::kQuotient, filter_bits_per_key, leaf_page_id, items,
                           page_payload, page_payload_bytes);
}

// Like the reference: a failed build is logged by the caller and the leaf gets no filter
// (filter_builder.hpp:323-325); the returned Status carries the reason.
// page_payload_bytes 0: the default TreeOptions' filter page payload at this bits/key
// (TreeOptions::filter_page_size(), tree/tree_options.hpp:177-220; 32,704 bytes at 12 bits/key)
inline Status build_filter_for_leaf_in_job(usize filter_bits_per_key, u64 leaf_page_id,
                                           const std::vector<std::string_view>& items,
                                           std::vector<u8>& page_payload,
                                           u64 page_payload_bytes = 0,
                                           FilterKind kind = kDefaultFilterKind)
{
  page_payload.clear();
  if (page_payload_bytes == 0 && filter_bits_per_key != 0)
    page_payload_bytes = default_filter_page_payload_size(filter_bits_per_key, kind);
  Status s = kind == FilterKind::kBloom
                 ? build_bloom_filter_for_leaf(filter_bits_per_key, leaf_page_id, items,
                                               page_payload, page_payload_bytes)
                 : build_quotient_filter_for_leaf(filter_bits_per_key, leaf_page_id, items,
                                                  page_payload, page_payload_bytes);
  if (!s.ok()) page_payload.clear();
  return s;
}

// ---------------------------------------------------------------------------------------
// LeafBatcher: the reference's per-leaf call pattern, built in batches
// ---------------------------------------------------------------------------------------
// build_all_pages runs build_filter_for_leaf_in_job once per leaf on its worker threads
// (tree/tree_serialize_context.cpp:71-75).  One GPU call per leaf pays a copy in, a build, a
// copy out and a synchronisation for one leaf.  LeafBatcher keeps that call site and batches
// the calls that arrive together:
//   - a call reserves its leaf's place in the open batch's pinned arena (keys, offsets) and
//     stages its keys there itself, in parallel with the other callers;
//   - the call that opened the batch (its leader) closes it after `linger`, or as soon as
//     the batch holds its share of the callers (below) or the arena is full, and the next call
//     opens another batch, which fills while this one is on the GPU;
//   - the leader waits for every member's keys, then builds the batch on its thread's stream:
//     one copy of the arena in, one plan, one build, one copy of the pages out;
//   - each caller copies its own page out of the batch's pinned output.
// A batch's share of the callers: the callers inside build() divided by `batches_in_flight`
// (at least 2, at most `max_batch`), so that several small batches run at once, each on its
// own stream, rather than one large one while the next collects.
// A batch holds leaves of one kind, bits/key, page size and key stride (0 = variable length);
// other calls open their own batch.  A leaf larger than the arena is built on its own.  If a
// batch's VQF build reports an insert failure, its leaves are rebuilt one by one so that only
// the failing leaf goes without a filter (filter_builder.hpp:323-325).
//
// Compile-time overrides for tools/leaf_bench.cpp sweeps (profiles/r06/leaf_sweep/, leaf_spin/):
// how long a member polls before it sleeps (16 VQF callers 1,046 Mkeys/s at 300 us, 930 at
// 200, ~750-860 at 0-100 or 400), and how many poll at once (16 / 32 VQF callers 942 / 1,272
// at 4, 878 / 1,105 at 8, 977 / 1,095 at 16; 2-6 within noise, sweep4)
#ifndef TKV_LEAF_SPIN_US
#define TKV_LEAF_SPIN_US 300
#endif
#ifndef TKV_LEAF_MAX_SPINNERS
#define TKV_LEAF_MAX_SPINNERS 4
#endif

class LeafBatcher
{
 public:
  struct Options {
    usize max_batch;  // leaves per batch at most
    std::chrono::microseconds linger;
    usize arena_bytes;  // pinned key bytes per batch (and as many bytes of offsets)
    usize batches_in_flight = 5;  // a batch closes at (callers in build()) / this many leaves
  };

  // (a batch collects callers for up to 60 us.  16 callers of 16K-key leaves, median of three
  // processes of five passes each, profiles/r06/leaf_sweep/: fixed batches of 3 leaves VQF
  // 1,046 Mkeys/s (members spinning 300 us), 4: 979, 5: 930, 8: 750-860, 16: 650-710; Bloom
  // 1,367-1,389 at 3, 1,259-1,279 at 4, 930-1,002 at 8.  32 callers at a fixed 3 fell to
  // 466-912 (VQF): hence a share of the callers, 16 / 5 -> 3, 32 / 5 -> 6.  With one wake-up
  // per batch instead of one for every waiting caller, 32 VQF callers run at 1,015-1,363
  // instead of swinging between ~450 and ~1,200; profiles/r06/leaf_default/, leaf_spin/)
  LeafBatcher() : LeafBatcher(Options{16, std::chrono::microseconds{60}, usize{8} << 20}) {}
  explicit LeafBatcher(Options o) : opt_{o}
  {
    if (opt_.max_batch == 0) opt_.max_batch = 1;
    if (opt_.batches_in_flight == 0) opt_.batches_in_flight = 1;
  }
  LeafBatcher(const LeafBatcher&) = delete;
  LeafBatcher& operator=(const LeafBatcher&) = delete;
  ~LeafBatcher()
  {
    for (Batch* b : all_) destroy(b);
  }

  Status build(FilterKind kind, usize bpk, u64 leaf_page_id, const std::vector<std::string_view>& items,
               std::vector<u8>& page_payload, u64 page_payload_bytes)
  {
    if (bpk == 0) {  // filter_builder.hpp:115-117, :227-229
      page_payload.clear();
      return OkStatus();
    }
    if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");
    const u64 n = items.size();
    u64 bytes = 0;
    bool fixed = n > 0;
    const u32 len0 = n ? (u32)items[0].size() : 0;
    for (const auto& k : items) {
      bytes += k.size();
      fixed = fixed && k.size() == len0;
    }
    const u32 stride = fixed && len0 ? len0 : 0;
    if (bytes > opt_.arena_bytes || n + 1 > key_cap()) {
      Status st = detail::build_one(kind, bpk, leaf_page_id, items, page_payload, page_payload_bytes);
      if (!st.ok()) page_payload.clear();
      return st;
    }

    Req r{&items, leaf_page_id, n, bytes};
    std::unique_lock<std::mutex> lk{mu_};
    ++active_;
    Batch* b = nullptr;
    bool leader = false;
    for (;;) {
      for (Batch* o : open_)
        if (o->kind == kind && o->bpk == bpk && o->cap == page_payload_bytes && o->stride == stride) b = o;
      if (b && (b->bytes + bytes > opt_.arena_bytes || b->n + n + 1 > key_cap())) {
        close(b);
        b = nullptr;
      }
      if (b || !free_.empty()) break;
      // a new batch's pinned arenas, stream and device buffers, allocated outside the lock
      lk.unlock();
      Batch* nb = create();
      lk.lock();
      if (!nb) {
        --active_;
        lk.unlock();
        Status st = detail::build_one(kind, bpk, leaf_page_id, items, page_payload, page_payload_bytes);
        if (!st.ok()) page_payload.clear();
        return st;
      }
      all_.push_back(nb);
      free_.push_back(nb);
    }
    if (!b) {
      leader = true;
      b = free_.back();
      free_.pop_back();
      b->kind = kind;
      b->bpk = bpk;
      b->cap = page_payload_bytes;
      b->stride = stride;
      open_.push_back(b);
    }
    r.key_off = b->n;
    r.byte_off = b->bytes;
    b->n += n;
    b->bytes += bytes;
    b->reqs.push_back(&r);
    ++b->users;
    if (b->reqs.size() >= batch_share()) close(b);
    lk.unlock();

    Status staged = stage(r, *b);
    // this leaf's keys (and offsets) to the device now, on the batch's stream: the copies of
    // the members overlap the collection window and each other's staging, so the leader's
    // build waits only for the last of them (round 6; they were one copy after the batch closed)
    // (a leaf whose staging failed copies too: its zero-length offsets keep the batch valid)
    if (n) {
      const Status c = copy_in(r, *b);
      if (staged.ok()) staged = c;
    }

    lk.lock();
    ++b->staged;
    b->cv.notify_all();
    if (leader) {
      const auto deadline = std::chrono::steady_clock::now() + opt_.linger;
      // no lingering once every caller inside build() has joined this batch (one thread alone
      // never waits)
      b->cv.wait_until(lk, deadline, [&] { return b->closed || b->reqs.size() >= active_; });
      if (!b->closed) close(b);
      b->cv.wait(lk, [&] { return b->staged == b->reqs.size(); });
      lk.unlock();
      run(*b);
      lk.lock();
      for (Req* q : b->reqs) {
        q->done = true;
        q->done_flag.store(true, std::memory_order_release);
      }
      b->cv.notify_all();
    } else {
      // a member first polls its flag (yielding) for about a batch's device time, then sleeps:
      // a condition-variable wake-up costs tens of microseconds on a busy host, about as long
      // as the batch's kernel.  At most kMaxSpinners poll at once (more callers than CPUs:
      // the pollers would take the CPUs the others stage their keys on)
      lk.unlock();
      if (spinners_.fetch_add(1, std::memory_order_relaxed) < kMaxSpinners) {
        const auto spin_until = std::chrono::steady_clock::now() + std::chrono::microseconds{kSpinUs};
        while (!r.done_flag.load(std::memory_order_acquire) && std::chrono::steady_clock::now() < spin_until)
          std::this_thread::yield();
      }
      spinners_.fetch_sub(1, std::memory_order_relaxed);
      lk.lock();
      b->cv.wait(lk, [&] { return r.done; });
    }
    lk.unlock();

    // this leaf's page, from the batch's pinned output (or the per-leaf rebuild)
    Status st = staged.ok() ? r.st : staged;
    if (st.ok() && r.page) {
      page_payload.assign(page_payload_bytes ? page_payload_bytes : r.page_bytes, 0);
      std::memcpy(page_payload.data(), r.page, r.page_bytes);
    } else if (st.ok() && r.rebuilt) {
      page_payload.swap(r.rebuilt_page);
    } else {
      page_payload.clear();
    }
    lk.lock();
    if (--b->users == 0) release(b);
    --active_;
    for (Batch* o : open_) o->cv.notify_all();  // (their leaders' linger ends at every caller joined)
    return st;
  }

 private:
  struct Req {
    const std::vector<std::string_view>* items;
    u64 page_id;
    u64 n, bytes;
    u64 key_off = 0, byte_off = 0;  // this leaf's place in the batch arena
    Status st{};
    const u8* page = nullptr;  // into the batch's pinned output
    u64 page_bytes = 0;
    bool rebuilt = false;
    std::vector<u8> rebuilt_page;
    bool done = false;                 // under mu_
    std::atomic<bool> done_flag{false};  // the same, for the members' polling
  };

  static constexpr int kSpinUs = TKV_LEAF_SPIN_US;
  static constexpr int kMaxSpinners = TKV_LEAF_MAX_SPINNERS;

  struct Batch {
    FilterKind kind{};
    usize bpk = 0;
    u64 cap = 0;
    u32 stride = 0;
    u8* h_keys = nullptr;   // [arena_bytes + seg_area()]: the keys, then the segments (one copy in)
    u64* h_offs = nullptr;  // [arena_bytes / 8]
    u8* h_io = nullptr;     // [segments][status 64 B][pages]
    usize h_io_cap = 0;
    hipStream_t stream = nullptr;
    DeviceBuffer d_keys, d_offs, d_out;  // d_keys: keys then segments; d_out: pages then workspace
    u64 n = 0, bytes = 0;
    usize staged = 0, users = 0;
    bool closed = false;
    std::vector<Req*> reqs;
    std::condition_variable cv;  // this batch's leader and members wait here (under mu_)
  };

  usize key_cap() const { return opt_.arena_bytes / 8; }

  // under mu_: the leaves a batch closes at (Options::batches_in_flight)
  usize batch_share() const
  {
    const usize share = active_ / opt_.batches_in_flight;
    return std::min(opt_.max_batch, std::max<usize>(share, 2));
  }

  // under mu_
  void close(Batch* b)
  {
    b->closed = true;
    for (usize i = 0; i < open_.size(); ++i)
      if (open_[i] == b) {
        open_.erase(open_.begin() + i);
        break;
      }
    b->cv.notify_all();
  }

  // the segments after the batch's keys in the same buffers (256-byte aligned)
  usize seg_area() const { return 256 + opt_.max_batch * sizeof(tkv_amq_segment); }
  static u64 align256(u64 x) { return (x + 255) & ~u64{255}; }

  Batch* create()
  {
    Batch* b = new Batch;
    if (hipHostMalloc(reinterpret_cast<void**>(&b->h_keys), opt_.arena_bytes + seg_area()) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&b->h_offs), 8 * key_cap() + 8) != hipSuccess ||
        hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess ||
        !b->d_keys.resize(opt_.arena_bytes + seg_area()) || !b->d_offs.resize(8 * key_cap() + 8)) {
      destroy(b);
      return nullptr;
    }
    return b;
  }

  static void destroy(Batch* b)
  {
    if (b->h_keys) (void)hipHostFree(b->h_keys);
    if (b->h_offs) (void)hipHostFree(b->h_offs);
    if (b->h_io) (void)hipHostFree(b->h_io);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
  }

  // grow-only, with headroom, so that steady state allocates nothing
  static bool reserve_device(DeviceBuffer& d, usize n) { return n <= d.size() || d.resize(n + n / 2); }

  void release(Batch* b)
  {
    b->reqs.clear();
    b->n = b->bytes = 0;
    b->staged = 0;
    b->closed = false;
    free_.push_back(b);
  }

  // the caller's keys into its reserved place in the arena; variable-length offsets are
  // staged leaf-relative into the thread's pinned scratch, then rebased into the arena
  static Status stage(const Req& r, Batch& b)
  {
    const auto& items = *r.items;
    const void* views = items.data();
    detail::LeafScratch& sc = detail::leaf_scratch();
    if (!detail::string_view_is_key_view()) {
      sc.views.resize(r.n);
      for (u64 i = 0; i < r.n; ++i)
        sc.views[i] = tkv_amq_key_view{items[i].size(), reinterpret_cast<const u8*>(items[i].data())};
      views = sc.views.data();
    }
    if (r.n == 0) return OkStatus();
    if (b.stride) {
      const int st = tkv_amq_stage_keys(views, sizeof(tkv_amq_key_view), r.n, b.stride,
                                        b.h_keys + r.byte_off, r.bytes, nullptr, 1);
      return st == TKV_AMQ_OK ? OkStatus() : Status::from(st, "tkv_amq_stage_keys");
    }
    u64* dst = b.h_offs + r.key_off;
    // on failure this leaf's slice of the batch offsets must not keep an earlier batch's
    // values (the batch is built anyway): zero-length keys at the leaf's own byte offset
    auto fail = [&](int code, const char* what) {
      for (u64 j = 0; j < r.n; ++j) dst[j] = r.byte_off;
      return Status::from(code, what);
    };
    if (!detail::LeafScratch::grow_pinned(sc.h_offs, sc.h_offs_cap, r.n + 1))
      return fail(TKV_AMQ_RESOURCE_EXHAUSTED, "hipHostMalloc");
    const int st = tkv_amq_stage_keys(views, sizeof(tkv_amq_key_view), r.n, 0, b.h_keys + r.byte_off,
                                      r.bytes, sc.h_offs, 1);
    if (st != TKV_AMQ_OK) return fail(st, "tkv_amq_stage_keys");
    for (u64 j = 0; j < r.n; ++j) dst[j] = sc.h_offs[j] + r.byte_off;
    return OkStatus();
  }

  // a member's staged keys (and its offsets) to the batch's device buffers, on its stream
  static Status copy_in(const Req& r, Batch& b)
  {
    if (hipMemcpyAsync(b.d_keys.get<u8>() + r.byte_off, b.h_keys + r.byte_off, r.bytes, hipMemcpyHostToDevice,
                       b.stream) != hipSuccess ||
        (b.stride == 0 && hipMemcpyAsync(b.d_offs.get<u8>() + 8 * r.key_off, b.h_offs + r.key_off, 8 * r.n,
                                         hipMemcpyHostToDevice, b.stream) != hipSuccess))
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpyAsync keys");
    return OkStatus();
  }

  // on the leader's thread: every member staged, nothing else touches the batch
  void run(Batch& b)
  {
    Status st = build_batch(b);
    if (!st.ok() && b.reqs.size() > 1 && st.code == TKV_AMQ_INTERNAL) {
      for (Req* q : b.reqs) {
        q->st = detail::build_one(b.kind, b.bpk, q->page_id, *q->items, q->rebuilt_page, b.cap);
        q->rebuilt = q->st.ok();
      }
    } else {
      for (Req* q : b.reqs) q->st = st;
    }
  }

  Status build_batch(Batch& b)
  {
    const usize n_segs = b.reqs.size();
    std::vector<u64> counts(n_segs), ids(n_segs);
    for (usize i = 0; i < n_segs; ++i) {
      counts[i] = b.reqs[i]->n;
      ids[i] = b.reqs[i]->page_id;
    }
    std::vector<tkv_amq_segment> segs(n_segs);
    u64 total_out = 0, ws_bytes = 0;
    u32 max_blocks = 0;
    int st = tkv_amq_plan((int)b.kind, counts.data(), ids.data(), (u32)n_segs, (u32)b.bpk, b.cap, 0,
                          segs.data(), &total_out, &ws_bytes, &max_blocks);
    if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_plan");
    const usize seg_bytes = n_segs * sizeof(tkv_amq_segment);
    // one copy out: the pages, then (VQF) the workspace header up to the leaves' nelts words,
    // the workspace placed after the pages in one device buffer
    const u64 ws_off = align256(total_out);
    const bool flags_out = b.kind == FilterKind::kQuotient && ws_bytes >= TKV_AMQ_VQF_NELTS_OFFSET + 4 * n_segs;
    const u64 out_bytes = flags_out ? ws_off + TKV_AMQ_VQF_NELTS_OFFSET + 4 * n_segs : total_out;
    const usize io_bytes = seg_bytes + out_bytes;
    if (!detail::LeafScratch::grow_pinned(b.h_io, b.h_io_cap, io_bytes <= b.h_io_cap ? io_bytes : io_bytes + io_bytes / 2))
      return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipHostMalloc");
    const u64 n = b.n, bytes = b.bytes;
    if (!reserve_device(b.d_out, ws_off + ws_bytes)) return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
    std::memcpy(b.h_io, segs.data(), seg_bytes);  // the host plan (tkv_amq_build_ex's h_segs)
    u8* h_out = b.h_io + seg_bytes;
    // the members copied their keys in (copy_in); the segments follow at the next 256-byte
    // boundary, and the offsets' closing entry
    const u64 seg_off = align256(bytes);
    std::memcpy(b.h_keys + seg_off, segs.data(), seg_bytes);
    if (b.stride == 0) b.h_offs[n] = bytes;
    hipStream_t s = b.stream;
    if (hipMemcpyAsync(b.d_keys.get<u8>() + seg_off, b.h_keys + seg_off, seg_bytes, hipMemcpyHostToDevice, s) !=
            hipSuccess ||
        (b.stride == 0 && hipMemcpyAsync(b.d_offs.get<u8>() + 8 * n, b.h_offs + n, 8, hipMemcpyHostToDevice, s) !=
                              hipSuccess))
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpyAsync segments");
    u8* d_ws = b.d_out.get<u8>() + ws_off;
    st = tkv_amq_build_ex((int)b.kind, b.d_keys.get(), b.stride ? nullptr : b.d_offs.get<u64>(), b.stride, n,
                          reinterpret_cast<const tkv_amq_segment*>(b.d_keys.get<u8>() + seg_off),
                          reinterpret_cast<const tkv_amq_segment*>(b.h_io), (u32)n_segs, max_blocks, b.d_out.get(),
                          ws_bytes ? d_ws : nullptr, ws_bytes, s);
    if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_build_ex");
    if (hipMemcpyAsync(h_out, b.d_out.get(), out_bytes, hipMemcpyDeviceToHost, s) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpyAsync pages");
    // (polled, yielding: a blocking synchronisation sleeps until an interrupt wakes it)
    hipError_t q;
    while ((q = hipStreamQuery(s)) == hipErrorNotReady) std::this_thread::yield();
    if (q != hipSuccess) return Status::from(TKV_AMQ_INTERNAL, "hipStreamQuery");
    u32 flags = 0;
    if (flags_out) {
      const u32* h_flags = reinterpret_cast<const u32*>(h_out + ws_off + TKV_AMQ_VQF_NELTS_OFFSET);
      for (usize i = 0; i < n_segs; ++i) flags |= h_flags[i];
    }
    if (flags & TKV_AMQ_VQF_FLAG_WORKSPACE) return Status::from(TKV_AMQ_INVALID_ARGUMENT, "workspace");
    if (flags & TKV_AMQ_VQF_FLAG_OVERFLOW)
      return Status::from(TKV_AMQ_INTERNAL, "vqf_insert (filter_builder.hpp:211)");
    for (usize i = 0; i < n_segs; ++i) {
      b.reqs[i]->page = h_out + segs[i].out_offset;
      b.reqs[i]->page_bytes = segs[i].payload_bytes;
    }
    return OkStatus();
  }

  Options opt_;
  std::mutex mu_;
  std::atomic<int> spinners_{0};
  std::vector<Batch*> open_, free_, all_;
  usize active_ = 0;  // callers inside build() past their size check
};

// build_filter_for_leaf_in_job through a process-wide LeafBatcher: the reference's per-leaf
// call site, built in batches across the worker threads that call it concurrently.  The
// batcher is never destroyed, so no pinned memory is freed after the HIP runtime shuts down.
inline Status build_filter_for_leaf_in_job_batched(usize filter_bits_per_key, u64 leaf_page_id,
                                                   const std::vector<std::string_view>& items,
                                                   std::vector<u8>& page_payload,
                                                   u64 page_payload_bytes = 0,
                                                   FilterKind kind = kDefaultFilterKind)
{
  if (page_payload_bytes == 0 && filter_bits_per_key != 0)
    page_payload_bytes = default_filter_page_payload_size(filter_bits_per_key, kind);
  static LeafBatcher* batcher = new LeafBatcher;
  return batcher->build(kind, filter_bits_per_key, leaf_page_id, items, page_payload, page_payload_bytes);
}

// ---------------------------------------------------------------------------------------
// KeyQuery::reject_page for a batch of point queries against one filter page payload
// ---------------------------------------------------------------------------------------
enum class BoolStatus : int { kFalse = 0, kTrue = 1, kUnknown = 2 };

// FastCountMetric<u64>
// ---------------------------------------------------------------------------------------
// TreeIndex: the flat tree tkv_amq_walk_paths descends (find_pivot_containing, tree/algo/
// nodes.hpp:48-71; find_key, :158-187; for_each_active_segment_in, tree/algo/
// segmented_levels.hpp:340-369; the shapes of PackedNodePage, tree/packed_node_page.hpp:42-223)
// ---------------------------------------------------------------------------------------
// The CSR list a walk produces: key i's entries are [begin[i], begin[i+1]) of every array.
struct TreePaths {
  std::vector<u32> begin, leaf, flushed;
  std::vector<u64> page_id;
  std::vector<u16> where;  // depth << 8 | level; level TKV_AMQ_WALK_LEAF_LEVEL: the child leaf

  void clear(usize n_keys)
  {
    begin.assign(n_keys + 1, 0);
    leaf.clear();
    flushed.clear();
    page_id.clear();
    where.clear();
  }
};

class TreeIndex
{
 public:
  static constexpr usize kMaxPivots = 64, kMaxSegments = 63, kMaxLevels = 7;  // (the reference's page: 6 levels)

  struct Segment {
    u32 leaf = 0;            // the leaf's segment index in the filter plan
    u64 page_id = 0;
    u64 active_pivots = 0;
    std::vector<std::pair<u32, u32>> flushed;  // (pivot, flushed item upper bound)
  };
  struct Leaf {
    u32 leaf = 0;
    u64 page_id = 0;
  };
  // A node owns pivot_count + 1 keys and one child per pivot: `children` (nodes) or `leaves`,
  // never both.  levels: the update buffer, newest first.
  struct Node {
    std::vector<std::string> pivot_keys;
    std::vector<std::vector<Segment>> levels;
    std::vector<Node> children;
    std::vector<Leaf> leaves;
    u64 page_id = 0;
  };

  // Validates the PackedNodePage limits and flattens the description breadth first (node 0 is
  // the root).
  static Status build(const Node& root, TreeIndex& out)
  {
    out.reset();
    int height = 0;
    TKV_AMQ_REQUIRE_OK(validate(root, height));
    if (height > (int)TKV_AMQ_WALK_MAX_DEPTH) return Status::from(TKV_AMQ_INVALID_ARGUMENT, "tree height");
    std::vector<std::pair<const Node*, int>> order{{&root, height}};
    for (usize at = 0; at < order.size(); ++at)
      for (const Node& c : order[at].first->children) order.push_back({&c, order[at].second - 1});
    usize next_child_node = 1;
    for (const auto& [n, h] : order) {
      tkv_amq_tree_node f{};
      const usize pivots = n->children.empty() ? n->leaves.size() : n->children.size();
      f.pivot_key_begin = (u32)out.pivot_keys_.size();
      f.seg_begin = (u32)out.segments_.size();
      f.child_begin = (u32)out.children_.size();
      f.pivot_count = (u8)pivots;
      f.height = (u8)h;
      f.level_count = (u8)n->levels.size();
      usize start = 0;
      for (usize l = 0; l < 8; ++l) {
        f.level_start[l] = (u8)start;
        if (l < n->levels.size()) start += n->levels[l].size();
      }
      for (const auto& k : n->pivot_keys) out.pivot_keys_.push_back(k);
      for (const Node& c : n->children) out.children_.push_back(tkv_amq_tree_child{c.page_id, (u32)next_child_node++, 0});
      for (const Leaf& c : n->leaves) out.children_.push_back(tkv_amq_tree_child{c.page_id, c.leaf, 0});
      for (const auto& level : n->levels) {
        for (const Segment& s : level) {
          tkv_amq_tree_segment g{};
          g.leaf_page_id = s.page_id;
          g.active_pivots = s.active_pivots;
          g.leaf = s.leaf;
          g.flushed_begin = (u32)out.flushed_bounds_.size();
          auto fl = s.flushed;
          std::sort(fl.begin(), fl.end());  // bounds are stored in pivot order (bit_rank)
          for (const auto& [p, bound] : fl) {
            g.flushed_pivots |= u64{1} << p;
            out.flushed_bounds_.push_back(bound);
          }
          out.segments_.push_back(g);
        }
      }
      out.nodes_.push_back(f);
    }
    return OkStatus();
  }

  // A tree that is flat already (read back from a file, say).  Nothing is validated: the walks
  // clamp every index.
  static void from_flat(std::vector<tkv_amq_tree_node> nodes, std::vector<tkv_amq_tree_segment> segments,
                        std::vector<tkv_amq_tree_child> children, std::vector<u32> flushed_bounds,
                        std::vector<std::string> pivot_keys, TreeIndex& out)
  {
    out.reset();
    out.nodes_ = std::move(nodes);
    out.segments_ = std::move(segments);
    out.children_ = std::move(children);
    out.flushed_bounds_ = std::move(flushed_bounds);
    out.pivot_keys_ = std::move(pivot_keys);
  }

  const std::vector<tkv_amq_tree_node>& nodes() const { return nodes_; }
  const std::vector<tkv_amq_tree_segment>& segments() const { return segments_; }
  const std::vector<tkv_amq_tree_child>& children() const { return children_; }
  const std::vector<u32>& flushed_bounds() const { return flushed_bounds_; }
  const std::vector<std::string>& pivot_keys() const { return pivot_keys_; }

  // The same walk on the host, written with std::upper_bound: the comparator of the tests and
  // the CPU baseline.  It applies the clamps of tkv_amq_walk_paths, so it answers for any flat
  // tree.  n_threads > 1 splits the keys into contiguous ranges.
  void walk_host(const std::vector<std::string_view>& keys, TreePaths& out, unsigned n_threads = 1) const
  {
    const usize n = keys.size();
    out.clear(n);
    if (n_threads < 1) n_threads = 1;
    if (n_threads > n) n_threads = n ? (unsigned)n : 1;
    std::vector<std::string_view> pk(pivot_keys_.begin(), pivot_keys_.end());
    std::vector<TreePaths> part(n_threads);
    std::vector<std::thread> pool;
    auto work = [&](unsigned t) {
      const usize b = n * t / n_threads, e = n * (t + 1) / n_threads;
      TreePaths& o = part[t];
      o.begin.assign(e - b + 1, 0);
      for (usize i = b; i < e; ++i) {
        walk_one(pk, keys[i], o);
        o.begin[i - b + 1] = (u32)o.leaf.size();
      }
    };
    for (unsigned t = 1; t < n_threads; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    for (unsigned t = 0; t < n_threads; ++t) {
      const usize b = n * t / n_threads, base = out.leaf.size();
      const TreePaths& o = part[t];
      for (usize j = 1; j < o.begin.size(); ++j) out.begin[b + j] = (u32)(base + o.begin[j]);
      out.leaf.insert(out.leaf.end(), o.leaf.begin(), o.leaf.end());
      out.flushed.insert(out.flushed.end(), o.flushed.begin(), o.flushed.end());
      out.page_id.insert(out.page_id.end(), o.page_id.begin(), o.page_id.end());
      out.where.insert(out.where.end(), o.where.begin(), o.where.end());
    }
  }

  // The whole point lookup on the host (what tkv_amq_get_keys computes, include/tkv_amq.h): the
  // entries of walk_host in order; maybe(leaf, key) stands for the leaf's filter (false: the filter
  // rejects) and defaults to "always maybe", which gives the same results as any filter without
  // false negatives; a leaf that may hold the key is searched with std::lower_bound over
  // leaf_keys [key_begin[leaf], key_begin[leaf + 1]) (a leaf at or past key_begin.size() - 1
  // cannot be searched); a key found below the entry's flushed bound leaves the level; the first
  // key found at or above it ends the lookup.  visits (optional): the entries each key visited.
  template <class Maybe>
  void get_host(const std::vector<std::string_view>& keys, const std::vector<std::string_view>& leaf_keys,
                const std::vector<u64>& key_begin, std::vector<tkv_amq_get_result>& out, Maybe&& maybe,
                std::vector<u32>* visits = nullptr) const
  {
    out.assign(keys.size(), tkv_amq_get_result{~u64{0}, ~u32{0}, ~u32{0}});
    if (visits) visits->assign(keys.size(), 0);
    std::vector<std::string_view> pk(pivot_keys_.begin(), pivot_keys_.end());
    const usize n_leaves = key_begin.empty() ? 0 : key_begin.size() - 1;
    TreePaths o;
    for (usize i = 0; i < keys.size(); ++i) {
      o.clear(0);
      walk_one(pk, keys[i], o);
      u32 left = ~u32{0}, n_visits = 0;  // the level that was left (a `where`), if any
      for (usize e = 0; e < o.leaf.size(); ++e) {
        if (o.where[e] == left) continue;
        ++n_visits;
        const u32 leaf = o.leaf[e];
        if (!maybe(leaf, keys[i]) || leaf >= n_leaves) continue;
        const u64 b0 = std::min<u64>(key_begin[leaf], leaf_keys.size());
        const u64 e0 = std::max<u64>(std::min<u64>(key_begin[leaf + 1], leaf_keys.size()), b0);
        const u64 b = (u64)(std::lower_bound(leaf_keys.begin() + b0, leaf_keys.begin() + e0, keys[i]) - leaf_keys.begin());
        if (b == e0 || leaf_keys[b] != keys[i]) continue;
        if (b - b0 < o.flushed[e]) {
          left = o.where[e];
          continue;
        }
        out[i] = tkv_amq_get_result{b, leaf, o.where[e]};
        break;
      }
      if (visits) (*visits)[i] = n_visits;
    }
  }
  void get_host(const std::vector<std::string_view>& keys, const std::vector<std::string_view>& leaf_keys,
                const std::vector<u64>& key_begin, std::vector<tkv_amq_get_result>& out) const
  {
    get_host(keys, leaf_keys, key_begin, out, [](u32, std::string_view) { return true; });
  }

  // as_i32() of a packed value's data (include/tkv_amq.h): 0 bytes: 0; 1..3: the sign-extended
  // little-endian integer; 4 and more: the first four bytes.
  static u32 value_i32(std::string_view data)
  {
    const usize m = std::min<usize>(data.size(), 4);
    u32 x = 0;
    for (usize j = 0; j < m; ++j) x |= (u32)(u8)data[j] << (8 * j);
    if (m == 0 || m == 4) return x;
    const u32 sign = u32{1} << (8 * m - 1);
    return (x ^ sign) - sign;  // (modulo 2^32: the sign extension)
  }

  // The point lookup with values on the host (what tkv_amq_get_values computes, include/tkv_amq.h):
  // get_host's visits, with every found item taken instead -- leaf_values[i] is the packed value
  // of leaf key i (an op byte, then the data; an empty value reads as NOOP) -- and folded into the
  // lookup's value: the first item is the value; a pending ADD_I32 takes a WRITE (the sum, as a
  // WRITE), a DELETE (a WRITE of the accumulator) or another ADD_I32 (summed, still pending; sums
  // wrap modulo 2^32); anything else is a bad combination, which leaves the value unchanged and ends
  // the lookup if the item is the first taken at its depth (the child leaf is a depth of its own).
  // A value that is no pending ADD ends the lookup; a pending ADD leaves the level.  maybe, visits:
  // as get_host's.  counts (optional): item_count, found_count and bad_combine_count are set.
  template <class Maybe>
  void get_values_host(const std::vector<std::string_view>& keys, const std::vector<std::string_view>& leaf_keys,
                       const std::vector<std::string_view>& leaf_values, const std::vector<u64>& key_begin,
                       std::vector<tkv_amq_value_result>& out, Maybe&& maybe, std::vector<u32>* visits = nullptr,
                       tkv_amq_value_counts* counts = nullptr) const
  {
    const tkv_amq_value_result none{~u64{0}, ~u64{0}, ~u32{0}, ~u32{0}, 0, (u8)TKV_AMQ_OP_NONE, 0, 0};
    out.assign(keys.size(), none);
    if (visits) visits->assign(keys.size(), 0);
    if (counts) *counts = tkv_amq_value_counts{};
    std::vector<std::string_view> pk(pivot_keys_.begin(), pivot_keys_.end());
    const usize n_leaves = key_begin.empty() ? 0 : key_begin.size() - 1;
    TreePaths o;
    for (usize i = 0; i < keys.size(); ++i) {
      o.clear(0);
      walk_one(pk, keys[i], o);
      tkv_amq_value_result r = none;
      u32 left = ~u32{0}, n_visits = 0, acc = 0, n_items = 0, last_depth = ~u32{0};
      for (usize e = 0; e < o.leaf.size(); ++e) {
        if (o.where[e] == left) continue;
        ++n_visits;
        const u32 leaf = o.leaf[e];
        if (!maybe(leaf, keys[i]) || leaf >= n_leaves) continue;
        const u64 b0 = std::min<u64>(key_begin[leaf], leaf_keys.size());
        const u64 e0 = std::max<u64>(std::min<u64>(key_begin[leaf + 1], leaf_keys.size()), b0);
        const u64 b = (u64)(std::lower_bound(leaf_keys.begin() + b0, leaf_keys.begin() + e0, keys[i]) - leaf_keys.begin());
        if (b == e0 || leaf_keys[b] != keys[i]) continue;
        left = o.where[e];  // flushed or taken: either way the level is left (or the lookup ends)
        if (b - b0 < o.flushed[e]) continue;
        const std::string_view value = b < leaf_values.size() ? leaf_values[b] : std::string_view{};
        const u32 op = value.empty() ? TKV_AMQ_OP_NOOP : (u8)value[0];
        const u32 x = value.empty() ? 0 : value_i32(value.substr(1));
        const u32 depth = o.where[e] >> 8;
        const bool first_here = (o.where[e] & 0xffu) == TKV_AMQ_WALK_LEAF_LEVEL || depth != last_depth;
        last_depth = depth;
        r.last_index = b;
        ++n_items;
        if (counts) ++counts->item_count;
        bool stop = true;
        if (n_items == 1) {
          r.key_index = b;
          r.leaf = leaf;
          r.where = o.where[e];
          r.op = (u8)op;
          if (op == TKV_AMQ_OP_ADD_I32) {
            acc = x;
            stop = false;
          }
        } else if (op == TKV_AMQ_OP_WRITE || op == TKV_AMQ_OP_DELETE) {
          acc += op == TKV_AMQ_OP_WRITE ? x : 0;
          r.op = (u8)TKV_AMQ_OP_WRITE;
          r.flags |= TKV_AMQ_VALUE_COMBINED;
        } else if (op == TKV_AMQ_OP_ADD_I32) {
          acc += x;
          r.flags |= TKV_AMQ_VALUE_COMBINED;
          stop = false;
        } else {
          r.flags |= TKV_AMQ_VALUE_BAD_COMBINE;
          if (counts) ++counts->bad_combine_count;
          stop = first_here;
        }
        if (stop) break;
      }
      r.i32 = (int32_t)acc;
      r.n_items = (uint16_t)std::min<u32>(n_items, 0xffff);
      if (counts && n_items) ++counts->found_count;
      out[i] = r;
      if (visits) (*visits)[i] = n_visits;
    }
  }
  void get_values_host(const std::vector<std::string_view>& keys, const std::vector<std::string_view>& leaf_keys,
                       const std::vector<std::string_view>& leaf_values, const std::vector<u64>& key_begin,
                       std::vector<tkv_amq_value_result>& out) const
  {
    get_values_host(keys, leaf_keys, leaf_values, key_begin, out, [](u32, std::string_view) { return true; });
  }

  // The flat arrays on the device, uploaded once (pivot keys fixed-stride if they share a length).
  Status upload()
  {
    if (uploaded_) return OkStatus();
    if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");
    std::vector<std::string_view> pk(pivot_keys_.begin(), pivot_keys_.end());
    TKV_AMQ_REQUIRE_OK(detail::stage_keys(pk, d_keys_, d_key_offs_, keys_fixed_, key_stride_));
    auto put = [](DeviceBuffer& d, const void* p, usize bytes) {
      return d.resize(bytes) && (bytes == 0 || hipMemcpy(d.get(), p, bytes, hipMemcpyHostToDevice) == hipSuccess);
    };
    if (!put(d_nodes_, nodes_.data(), nodes_.size() * sizeof(tkv_amq_tree_node)) ||
        !put(d_segments_, segments_.data(), segments_.size() * sizeof(tkv_amq_tree_segment)) ||
        !put(d_children_, children_.data(), children_.size() * sizeof(tkv_amq_tree_child)) ||
        !put(d_bounds_, flushed_bounds_.data(), flushed_bounds_.size() * 4))
      return Status::from(TKV_AMQ_INTERNAL, "tree upload");
    uploaded_ = true;
    return OkStatus();
  }

  // tkv_amq_walk_paths over the uploaded tree (upload() first); every pointer is a device pointer
  int walk_device(const u8* d_queries, const u64* d_query_offsets, u32 query_stride, u64 n_queries,
                  u32* d_path_begin, u32* d_path_leaf, u64* d_path_page_id, u32* d_path_flushed, u16* d_path_where,
                  u64 path_capacity, u64* d_needed, void* d_workspace, u64 workspace_bytes,
                  hipStream_t stream = nullptr) const
  {
    return tkv_amq_walk_paths(d_nodes_.get<tkv_amq_tree_node>(), nodes_.size(),
                              d_segments_.get<tkv_amq_tree_segment>(), segments_.size(),
                              d_children_.get<tkv_amq_tree_child>(), children_.size(), d_bounds_.get<u32>(),
                              flushed_bounds_.size(), d_keys_.get(), keys_fixed_ ? nullptr : d_key_offs_.get<u64>(),
                              keys_fixed_ ? key_stride_ : 0, pivot_keys_.size(), d_queries, d_query_offsets,
                              query_stride, n_queries, d_path_begin, d_path_leaf, d_path_page_id, d_path_flushed,
                              d_path_where, path_capacity, d_needed, d_workspace, workspace_bytes, stream);
  }

  // tkv_amq_get_keys over the uploaded tree (upload() first); every pointer is a device pointer
  int get_device(int kind, const u8* d_filters, const tkv_amq_segment* d_segs, u32 n_segs, const u8* d_queries,
                 const u64* d_query_offsets, u32 query_stride, u64 n_queries, const u8* d_leaf_keys,
                 const u64* d_leaf_key_offsets, u32 leaf_key_stride, u64 n_leaf_keys, const u64* d_key_begin,
                 u32 flags, tkv_amq_get_result* d_result, u32* d_query_visits, tkv_amq_probe_metrics* d_metrics,
                 tkv_amq_get_counts* d_counts, hipStream_t stream = nullptr) const
  {
    return tkv_amq_get_keys(kind, d_filters, d_segs, n_segs, d_nodes_.get<tkv_amq_tree_node>(), nodes_.size(),
                            d_segments_.get<tkv_amq_tree_segment>(), segments_.size(),
                            d_children_.get<tkv_amq_tree_child>(), children_.size(), d_bounds_.get<u32>(),
                            flushed_bounds_.size(), d_keys_.get(), keys_fixed_ ? nullptr : d_key_offs_.get<u64>(),
                            keys_fixed_ ? key_stride_ : 0, pivot_keys_.size(), d_queries, d_query_offsets,
                            query_stride, n_queries, d_leaf_keys, d_leaf_key_offsets, leaf_key_stride, n_leaf_keys,
                            d_key_begin, flags, d_result, d_query_visits, d_metrics, d_counts, stream);
  }

  // tkv_amq_get_values over the uploaded tree (upload() first); every pointer is a device pointer
  int get_values_device(int kind, const u8* d_filters, const tkv_amq_segment* d_segs, u32 n_segs, const u8* d_queries,
                        const u64* d_query_offsets, u32 query_stride, u64 n_queries, const u8* d_leaf_keys,
                        const u64* d_leaf_key_offsets, u32 leaf_key_stride, u64 n_leaf_keys, const u64* d_key_begin,
                        const u8* d_leaf_values, const u64* d_leaf_value_offsets, u32 leaf_value_stride,
                        u64 leaf_values_bytes, u32 flags, tkv_amq_value_result* d_result, u32* d_query_visits,
                        tkv_amq_probe_metrics* d_metrics, tkv_amq_value_counts* d_counts,
                        hipStream_t stream = nullptr) const
  {
    return tkv_amq_get_values(kind, d_filters, d_segs, n_segs, d_nodes_.get<tkv_amq_tree_node>(), nodes_.size(),
                              d_segments_.get<tkv_amq_tree_segment>(), segments_.size(),
                              d_children_.get<tkv_amq_tree_child>(), children_.size(), d_bounds_.get<u32>(),
                              flushed_bounds_.size(), d_keys_.get(), keys_fixed_ ? nullptr : d_key_offs_.get<u64>(),
                              keys_fixed_ ? key_stride_ : 0, pivot_keys_.size(), d_queries, d_query_offsets,
                              query_stride, n_queries, d_leaf_keys, d_leaf_key_offsets, leaf_key_stride, n_leaf_keys,
                              d_key_begin, d_leaf_values, d_leaf_value_offsets, leaf_value_stride, leaf_values_bytes,
                              flags, d_result, d_query_visits, d_metrics, d_counts, stream);
  }

 private:
  static Status validate(const Node& n, int& height)
  {
    const auto bad = [](const char* w) { return Status::from(TKV_AMQ_INVALID_ARGUMENT, w); };
    if (!n.children.empty() && !n.leaves.empty()) return bad("a node's children are all nodes or all leaves");
    const usize pivots = n.children.empty() ? n.leaves.size() : n.children.size();
    if (pivots < 1 || pivots > kMaxPivots) return bad("a node has 1..64 pivots");
    if (n.pivot_keys.size() != pivots + 1) return bad("a node of p pivots owns p + 1 pivot keys");
    if (n.levels.size() > kMaxLevels) return bad("a node has at most 7 levels");
    usize n_seg = 0;
    for (const auto& level : n.levels) {
      n_seg += level.size();
      for (const Segment& s : level) {
        if (pivots < 64 && (s.active_pivots >> pivots)) return bad("a segment names a pivot the node does not have");
        for (const auto& f : s.flushed)
          if (f.first >= pivots) return bad("a segment names a pivot the node does not have");
      }
    }
    if (n_seg > kMaxSegments) return bad("a node has at most 63 segments");
    height = 1;
    for (usize i = 0; i < n.children.size(); ++i) {
      int h = 0;
      TKV_AMQ_REQUIRE_OK(validate(n.children[i], h));
      if (i && h + 1 != height) return bad("a node's children have one height");
      height = h + 1;
    }
    return OkStatus();
  }

  void walk_one(const std::vector<std::string_view>& pk, std::string_view q, TreePaths& o) const
  {
    u32 ni = 0;
    for (u32 depth = 0; depth < TKV_AMQ_WALK_MAX_DEPTH; ++depth) {
      if (ni >= nodes_.size()) return;
      const tkv_amq_tree_node& nd = nodes_[ni];
      if (nd.pivot_count == 0 || nd.pivot_count > 64) return;
      // the interior keys k1..k(p-1); those past the list do not exist
      const usize first = std::min<usize>((usize)nd.pivot_key_begin + 1, pk.size());
      const usize last = std::min<usize>(first + nd.pivot_count - 1, pk.size());
      const u32 p = (u32)(std::upper_bound(pk.begin() + first, pk.begin() + last, q) - (pk.begin() + first));
      const usize levels = std::min<usize>(nd.level_count, 7);
      for (usize l = 0; l < levels; ++l) {
        const usize sb = std::min<usize>((usize)nd.seg_begin + nd.level_start[l], segments_.size());
        const usize se = std::min<usize>((usize)nd.seg_begin + nd.level_start[l + 1], segments_.size());
        for (usize s = sb; s < se; ++s) {
          const tkv_amq_tree_segment& g = segments_[s];
          if (!((g.active_pivots >> p) & 1)) continue;
          u32 bound = 0;
          if ((g.flushed_pivots >> p) & 1) {
            const usize at = (usize)g.flushed_begin + (usize)__builtin_popcountll(g.flushed_pivots & ((u64{1} << p) - 1));
            if (at < flushed_bounds_.size()) bound = flushed_bounds_[at];
          }
          push(o, g.leaf, g.leaf_page_id, bound, (u16)(depth << 8 | l));
        }
      }
      const usize c = (usize)nd.child_begin + p;
      if (c >= children_.size()) return;
      if (nd.height <= 1) {
        push(o, children_[c].index, children_[c].page_id, 0, (u16)(depth << 8 | TKV_AMQ_WALK_LEAF_LEVEL));
        return;
      }
      ni = children_[c].index;
    }
  }

  void reset()
  {
    nodes_.clear();
    segments_.clear();
    children_.clear();
    flushed_bounds_.clear();
    pivot_keys_.clear();
    uploaded_ = false;
  }

  static void push(TreePaths& o, u32 leaf, u64 page_id, u32 flushed, u16 where)
  {
    o.leaf.push_back(leaf);
    o.page_id.push_back(page_id);
    o.flushed.push_back(flushed);
    o.where.push_back(where);
  }

  std::vector<tkv_amq_tree_node> nodes_;
  std::vector<tkv_amq_tree_segment> segments_;
  std::vector<tkv_amq_tree_child> children_;
  std::vector<u32> flushed_bounds_;
  std::vector<std::string> pivot_keys_;
  DeviceBuffer d_nodes_, d_segments_, d_children_, d_bounds_, d_keys_, d_key_offs_;
  bool uploaded_ = false, keys_fixed_ = false;
  u32 key_stride_ = 0;
};

struct CountMetric {
  std::atomic<u64> value{0};
  void add(u64 n) { value.fetch_add(n, std::memory_order_relaxed); }
  u64 get() const { return value.load(std::memory_order_relaxed); }
};

class KeyQuery
{
 public:
  // KeyQuery::Metrics, the filter counters (tree/key_query.hpp:36-60).  reject_page updates
  // total / no-filter / load-failed / page-id-mismatch / reject (:154,157,183,210,231,243);
  // positive / false positive are the caller's leaf search's (key_query.cpp:41,77):
  // reject_page counts them when the caller passes the ground truth.
  struct Metrics {
    CountMetric total_filter_query_count;
    CountMetric no_filter_page_count;
    CountMetric filter_page_load_failed_count;
    CountMetric page_id_mismatch_count;
    CountMetric filter_reject_count;
    CountMetric filter_positive_count;
    CountMetric filter_false_positive_count;

    double filter_false_positive_rate() const noexcept
    {
      const double positives = (double)filter_positive_count.get();
      if (positives == 0) return -1;
      return (double)filter_false_positive_count.get() / positives;
    }
  };

  static Metrics& metrics()
  {
    static Metrics metrics_;
    return metrics_;
  }

  explicit KeyQuery(std::vector<std::string_view> keys) : keys_{std::move(keys)} {}

  // per key: kTrue = definitely absent; kFalse = maybe present; kUnknown = no filter or the
  // filter belongs to another page (key_query.hpp:156-159, 207-212, 227-232).
  // truth (optional, one per key: 1 = the key is in the leaf) feeds the positive /
  // false-positive counters the reference's leaf search keeps (key_query.cpp:41,77).
  Status reject_page(u64 page_id_to_reject, const std::vector<u8>* filter_payload,
                     FilterKind kind, std::vector<BoolStatus>& out,
                     const std::vector<u8>* truth = nullptr)
  {
    Metrics& m = metrics();
    const u64 n = keys_.size();
    out.assign(n, BoolStatus::kUnknown);
    m.total_filter_query_count.add(n);
    if (!filter_payload) {
      m.no_filter_page_count.add(n);
      return OkStatus();
    }
    if (filter_payload->size() < 64) {  // cannot be read as a filter page: cannot reject
      m.filter_page_load_failed_count.add(n);
      return OkStatus();
    }
    u64 magic, src;
    std::memcpy(&magic, filter_payload->data(), 8);
    std::memcpy(&src, filter_payload->data() + (kind == FilterKind::kBloom ? 16 : 8), 8);
    const u64 want = kind == FilterKind::kBloom ? PackedBloomFilterPage::kMagic : PackedVqfFilter::kMagic;
    if (magic != want) return Status::from(TKV_AMQ_INTERNAL, "filter page magic");
    if (src != page_id_to_reject) {
      m.page_id_mismatch_count.add(n);
      return OkStatus();
    }
    if (keys_.empty()) return OkStatus();
    if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");

    // single-segment plan whose payload sits at offset 0 of the staged page
    tkv_amq_segment seg{};
    if (kind == FilterKind::kBloom) {
      PackedBloomFilterPage h;
      std::memcpy(&h, filter_payload->data(), sizeof(h));
      seg.n_blocks = h.block_count;
      seg.hash_count = h.hash_count;
    } else {
      if (filter_payload->size() < sizeof(PackedVqfFilter)) {
        m.filter_page_load_failed_count.add(n);
        return OkStatus();
      }
      PackedVqfFilter h;
      std::memcpy(&h, filter_payload->data(), sizeof(h));
      const u64 tb = h.metadata.key_remainder_bits;
      if ((tb != 8 && tb != 16) || h.metadata.nblocks == 0 || h.hash_mask == 0)
        return Status::from(TKV_AMQ_INTERNAL, "PackedVqfFilter metadata");
      // hash_mask = ~0 << hash_val_shift (filter_builder.hpp:187): truncated leaves answer
      // "maybe" for every hash with a low bit set (vqf_filter_page_view.hpp:115-117)
      const u32 shift = (u32)__builtin_ctzll(h.hash_mask);
      if (h.hash_mask != (~u64{0} << shift)) return Status::from(TKV_AMQ_INTERNAL, "hash_mask");
      const u64 buckets = tb == 8 ? 80 : 36;
      seg.n_blocks = (u32)h.metadata.nblocks;
      seg.tag_bits = (u8)tb;
      seg.hash_val_shift = (u8)shift;
      seg.mod_magic = ~0ull / (h.metadata.nblocks * buckets);
    }
    seg.out_offset = 0;
    DeviceBuffer d_keys, d_offs, d_page, d_seg, d_leaf, d_res;
    if (!d_page.resize(filter_payload->size()) || !d_seg.resize(sizeof(seg)) ||
        !d_leaf.resize(4 * n) || !d_res.resize(n))
      return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
    bool fixed = false;
    u32 stride = 16;
    TKV_AMQ_REQUIRE_OK(detail::stage_keys(keys_, d_keys, d_offs, fixed, stride));
    if (hipMemcpy(d_page.get(), filter_payload->data(), filter_payload->size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_seg.get(), &seg, sizeof(seg), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_leaf.get(), 0, 4 * n) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy page");
    const int st = tkv_amq_probe((int)kind, d_page.get(), d_seg.get<tkv_amq_segment>(), 1,
                                 d_keys.get(), fixed ? nullptr : d_offs.get<u64>(),
                                 fixed ? stride : 0, n, d_leaf.get<u32>(), d_res.get(), nullptr);
    if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_probe");
    std::vector<u8> res(n);
    if (hipMemcpy(res.data(), d_res.get(), res.size(), hipMemcpyDeviceToHost) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy result");
    u64 rejects = 0, fps = 0;
    for (usize i = 0; i < res.size(); ++i) {
      out[i] = res[i] ? BoolStatus::kFalse : BoolStatus::kTrue;
      rejects += res[i] == 0;
      if (truth && i < truth->size()) fps += res[i] != 0 && (*truth)[i] == 0;
    }
    m.filter_reject_count.add(rejects);
    m.filter_positive_count.add(n - rejects);
    if (truth) m.filter_false_positive_count.add(fps);
    return OkStatus();
  }

  // The batch form of a point lookup's walk (tree/algo/nodes.hpp:158-187,
  // tree/algo/segmented_levels.hpp:358-369, key_query.cpp:27-80): key i would visit the leaves
  // path_leaf[path_begin[i] .. path_begin[i+1]) -- indices into `segs`, newest level first --
  // and reject_page is asked of each.  Every key is hashed once (tkv_amq_path_probe).
  //  d_filters, d_segs, segs   the device filter array with its device and host segments, as a
  //                            FilterBatchBuilder leaves them (device_segments(), segments())
  //  cand_begin, cand_leaf     (out) key i's leaves still to search, in path order:
  //                            cand_leaf[cand_begin[i] .. cand_begin[i+1])
  //  truth                     optional, one per ENTRY (1 = the key is in that leaf)
  // Counts one filter query per entry in metrics(), classified as reject_page classifies it.
  Status candidate_leaves(FilterKind kind, const u8* d_filters, const tkv_amq_segment* d_segs,
                          const std::vector<tkv_amq_segment>& segs, const std::vector<u32>& path_begin,
                          const std::vector<u32>& path_leaf, std::vector<u32>& cand_begin,
                          std::vector<u32>& cand_leaf, const std::vector<u8>* truth = nullptr)
  {
    const u64 n = keys_.size(), n_entries = path_leaf.size();
    cand_begin.assign(n + 1, 0);
    cand_leaf.clear();
    if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");
    if (path_begin.size() != n + 1 || (truth && truth->size() != n_entries))
      return Status::from(TKV_AMQ_INVALID_ARGUMENT, "path lists");
    if (n == 0) return OkStatus();
    const u64 ws_bytes = tkv_amq_path_probe_ws_bytes(n, n_entries);
    if (ws_bytes == 0) return Status::from(TKV_AMQ_INVALID_ARGUMENT, "path lists");
    DeviceBuffer d_keys, d_offs, d_begin, d_leaf, d_cbegin, d_cleaf, d_truth, d_metrics, d_ws;
    if (!d_begin.resize(4 * (n + 1)) || !d_leaf.resize(4 * n_entries) || !d_cbegin.resize(4 * (n + 1)) ||
        !d_cleaf.resize(4 * n_entries) || !d_metrics.resize(sizeof(tkv_amq_probe_metrics)) ||
        !d_ws.resize(ws_bytes) || (truth && !d_truth.resize(n_entries)))
      return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
    bool fixed = false;
    u32 stride = 16;
    TKV_AMQ_REQUIRE_OK(detail::stage_keys(keys_, d_keys, d_offs, fixed, stride));
    if (hipMemcpy(d_begin.get(), path_begin.data(), 4 * (n + 1), hipMemcpyHostToDevice) != hipSuccess ||
        (n_entries && hipMemcpy(d_leaf.get(), path_leaf.data(), 4 * n_entries, hipMemcpyHostToDevice) != hipSuccess) ||
        (truth && n_entries &&
         hipMemcpy(d_truth.get(), truth->data(), n_entries, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemset(d_metrics.get(), 0, sizeof(tkv_amq_probe_metrics)) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy path lists");
    const tkv_amq_probe_opts opts{nullptr, truth ? d_truth.get() : nullptr,
                                  d_metrics.get<tkv_amq_probe_metrics>()};
    const int st = tkv_amq_path_probe((int)kind, d_filters, d_segs, (u32)segs.size(), d_keys.get(),
                                      fixed ? nullptr : d_offs.get<u64>(), fixed ? stride : 0, n,
                                      d_begin.get<u32>(), d_leaf.get<u32>(), n_entries, nullptr,
                                      d_cbegin.get<u32>(), d_cleaf.get<u32>(), nullptr, &opts, d_ws.get(),
                                      ws_bytes, nullptr);
    if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_path_probe");
    tkv_amq_probe_metrics pm{};
    // (blocking copies on the null stream: they wait for the probe)
    if (hipMemcpy(cand_begin.data(), d_cbegin.get(), 4 * (n + 1), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&pm, d_metrics.get(), sizeof(pm), hipMemcpyDeviceToHost) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy candidates");
    cand_leaf.resize(cand_begin[n]);
    if (!cand_leaf.empty() &&
        hipMemcpy(cand_leaf.data(), d_cleaf.get(), 4 * cand_leaf.size(), hipMemcpyDeviceToHost) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy candidates");
    Metrics& m = metrics();
    m.total_filter_query_count.add(pm.total_filter_query_count);
    m.no_filter_page_count.add(pm.no_filter_page_count);
    m.page_id_mismatch_count.add(pm.page_id_mismatch_count);
    m.filter_reject_count.add(pm.filter_reject_count);
    m.filter_positive_count.add(pm.filter_positive_count);
    if (truth) m.filter_false_positive_count.add(pm.filter_false_positive_count);
    return OkStatus();
  }

  // The descent in front of candidate_leaves (tkv_amq_walk_paths): every key's ordered list of
  // leaves over `tree`, with page ids, flushed item upper bounds and (depth, level) per entry --
  // what TreeIndex::walk_host computes on the host.  out.begin / out.leaf are candidate_leaves'
  // path_begin / path_leaf.  Synchronises: the walk runs once with capacity 0 to learn the total,
  // then again with exactly that capacity.
  Status walk_paths(TreeIndex& tree, TreePaths& out)
  {
    const u64 n = keys_.size();
    out.clear(n);
    if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");
    if (n == 0) return OkStatus();
    TKV_AMQ_REQUIRE_OK(tree.upload());
    const u64 ws_bytes = tkv_amq_walk_paths_ws_bytes(n);
    if (ws_bytes == 0) return Status::from(TKV_AMQ_INVALID_ARGUMENT, "too many keys");
    DeviceBuffer d_keys, d_offs, d_begin, d_needed, d_ws, d_leaf, d_page, d_flushed, d_where;
    if (!d_begin.resize(4 * (n + 1)) || !d_needed.resize(8) || !d_ws.resize(ws_bytes))
      return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
    bool fixed = false;
    u32 stride = 16;
    TKV_AMQ_REQUIRE_OK(detail::stage_keys(keys_, d_keys, d_offs, fixed, stride));
    const u64* offs = fixed ? nullptr : d_offs.get<u64>();
    int st = tree.walk_device(d_keys.get(), offs, fixed ? stride : 0, n, d_begin.get<u32>(), nullptr, nullptr,
                              nullptr, nullptr, 0, d_needed.get<u64>(), d_ws.get(), ws_bytes);
    if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_walk_paths");
    u64 total = 0;
    // (blocking copies on the null stream: they wait for the walk)
    if (hipMemcpy(&total, d_needed.get(), 8, hipMemcpyDeviceToHost) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy total");
    if (total > 0xffffffffull) return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "more than 2^32 entries");
    if (!d_leaf.resize(4 * total) || !d_page.resize(8 * total) || !d_flushed.resize(4 * total) ||
        !d_where.resize(2 * total))
      return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
    st = tree.walk_device(d_keys.get(), offs, fixed ? stride : 0, n, d_begin.get<u32>(), d_leaf.get<u32>(),
                          d_page.get<u64>(), d_flushed.get<u32>(), d_where.get<u16>(), total, d_needed.get<u64>(),
                          d_ws.get(), ws_bytes);
    if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_walk_paths");
    out.leaf.resize(total);
    out.page_id.resize(total);
    out.flushed.resize(total);
    out.where.resize(total);
    if (hipMemcpy(out.begin.data(), d_begin.get(), 4 * (n + 1), hipMemcpyDeviceToHost) != hipSuccess ||
        (total && (hipMemcpy(out.leaf.data(), d_leaf.get(), 4 * total, hipMemcpyDeviceToHost) != hipSuccess ||
                   hipMemcpy(out.page_id.data(), d_page.get(), 8 * total, hipMemcpyDeviceToHost) != hipSuccess ||
                   hipMemcpy(out.flushed.data(), d_flushed.get(), 4 * total, hipMemcpyDeviceToHost) != hipSuccess ||
                   hipMemcpy(out.where.data(), d_where.get(), 2 * total, hipMemcpyDeviceToHost) != hipSuccess)))
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy paths");
    return OkStatus();
  }

  // The search candidate_leaves leaves to its caller (find_key_in_leaf_impl, key_query.cpp:27-80,
  // 299-327): key i's candidates cand_leaf[cand_begin[i] .. cand_begin[i+1]) are searched in
  // order -- a lower bound over the leaf's sorted keys, an equality test -- and the walk ends at
  // the first leaf that holds the key (tkv_amq_find_keys).
  //  d_filters, d_segs, segs   as for candidate_leaves
  //  cand_begin, cand_leaf     candidate_leaves' output (or any CSR list of leaves)
  //  d_leaf_keys, ...          the leaves' keys on the device, in the key forms of the build
  //                            (d_leaf_key_offsets != nullptr: variable length); leaf s owns
  //                            keys [segs[s].key_begin, + segs[s].n_keys), each leaf ascending
  //  out                       (out) per key: the found key's global index, its leaf and the
  //                            candidate's position; ~0 / 0xffffffff if no candidate holds it
  // Adds the device's count of searched candidates that a filter had let through without the
  // key to metrics().filter_false_positive_count: no host truth is needed.
  Status find_in_leaves(FilterKind kind, const u8* d_filters, const tkv_amq_segment* d_segs,
                        const std::vector<tkv_amq_segment>& segs, const std::vector<u32>& cand_begin,
                        const std::vector<u32>& cand_leaf, const u8* d_leaf_keys, const u64* d_leaf_key_offsets,
                        u32 leaf_key_stride, u64 n_leaf_keys, std::vector<tkv_amq_find_result>& out)
  {
    const u64 n = keys_.size(), n_cand = cand_leaf.size();
    out.assign(n, tkv_amq_find_result{~u64{0}, ~u32{0}, ~u32{0}});
    if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");
    if (cand_begin.size() != n + 1) return Status::from(TKV_AMQ_INVALID_ARGUMENT, "candidate lists");
    if (n == 0) return OkStatus();
    DeviceBuffer d_keys, d_offs, d_begin, d_leaf, d_result, d_metrics;
    if (!d_begin.resize(4 * (n + 1)) || !d_leaf.resize(4 * n_cand) ||
        !d_result.resize(sizeof(tkv_amq_find_result) * n) || !d_metrics.resize(sizeof(tkv_amq_probe_metrics)))
      return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
    bool fixed = false;
    u32 stride = 16;
    TKV_AMQ_REQUIRE_OK(detail::stage_keys(keys_, d_keys, d_offs, fixed, stride));
    if (hipMemcpy(d_begin.get(), cand_begin.data(), 4 * (n + 1), hipMemcpyHostToDevice) != hipSuccess ||
        (n_cand && hipMemcpy(d_leaf.get(), cand_leaf.data(), 4 * n_cand, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemset(d_metrics.get(), 0, sizeof(tkv_amq_probe_metrics)) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy candidate lists");
    const tkv_amq_probe_opts opts{nullptr, nullptr, d_metrics.get<tkv_amq_probe_metrics>()};
    const int st = tkv_amq_find_keys((int)kind, d_filters, d_segs, (u32)segs.size(), d_keys.get(),
                                     fixed ? nullptr : d_offs.get<u64>(), fixed ? stride : 0, n,
                                     d_begin.get<u32>(), d_leaf.get<u32>(), nullptr, n_cand, d_leaf_keys,
                                     d_leaf_key_offsets, leaf_key_stride, n_leaf_keys, nullptr, 0,
                                     d_result.get<tkv_amq_find_result>(), nullptr, &opts, nullptr, nullptr);
    if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_find_keys");
    tkv_amq_probe_metrics pm{};
    // (blocking copies on the null stream: they wait for the search)
    if (hipMemcpy(out.data(), d_result.get(), sizeof(tkv_amq_find_result) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&pm, d_metrics.get(), sizeof(pm), hipMemcpyDeviceToHost) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy found keys");
    metrics().filter_false_positive_count.add(pm.filter_false_positive_count);
    return OkStatus();
  }

  // The whole lookup in one call (tkv_amq_get_keys): walk_paths, candidate_leaves and
  // find_in_leaves fused, in the reference's order and with its flushed-bound rule -- what
  // TreeIndex::get_host computes on the host.  No path is materialised, and nothing below a hit
  // is visited or counted.
  //  d_filters, d_segs, segs   as for candidate_leaves
  //  d_leaf_keys, ...          as for find_in_leaves
  //  check_page_ids            compare each filter's stored page id with the tree's id of the leaf
  //  out                       (out) per key: the found key's global index, its leaf and
  //                            depth << 8 | level of the entry that held it; ~0 / 0xffffffff if none
  //  counts                    (out, optional) the lookup's own tallies
  // Adds every visit to metrics(), classified as reject_page classifies it, the false positives
  // included: no host truth is needed.
  Status get_keys(FilterKind kind, const u8* d_filters, const tkv_amq_segment* d_segs,
                  const std::vector<tkv_amq_segment>& segs, TreeIndex& tree, const u8* d_leaf_keys,
                  const u64* d_leaf_key_offsets, u32 leaf_key_stride, u64 n_leaf_keys, bool check_page_ids,
                  std::vector<tkv_amq_get_result>& out, tkv_amq_get_counts* counts = nullptr)
  {
    const u64 n = keys_.size();
    out.assign(n, tkv_amq_get_result{~u64{0}, ~u32{0}, ~u32{0}});
    if (counts) *counts = tkv_amq_get_counts{};
    if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");
    if (n == 0) return OkStatus();
    TKV_AMQ_REQUIRE_OK(tree.upload());
    DeviceBuffer d_keys, d_offs, d_result, d_tallies;
    constexpr usize kMetricsBytes = sizeof(tkv_amq_probe_metrics);
    if (!d_result.resize(sizeof(tkv_amq_get_result) * n) || !d_tallies.resize(kMetricsBytes + sizeof(tkv_amq_get_counts)))
      return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
    bool fixed = false;
    u32 stride = 16;
    TKV_AMQ_REQUIRE_OK(detail::stage_keys(keys_, d_keys, d_offs, fixed, stride));
    if (hipMemset(d_tallies.get(), 0, kMetricsBytes + sizeof(tkv_amq_get_counts)) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemset counters");
    auto* d_metrics = d_tallies.get<tkv_amq_probe_metrics>();
    auto* d_counts = reinterpret_cast<tkv_amq_get_counts*>(d_tallies.get() + kMetricsBytes);
    const int st = tree.get_device((int)kind, d_filters, d_segs, (u32)segs.size(), d_keys.get(),
                                   fixed ? nullptr : d_offs.get<u64>(), fixed ? stride : 0, n, d_leaf_keys,
                                   d_leaf_key_offsets, leaf_key_stride, n_leaf_keys, nullptr,
                                   check_page_ids ? TKV_AMQ_GET_CHECK_PAGE_ID : 0u,
                                   d_result.get<tkv_amq_get_result>(), nullptr, d_metrics, d_counts);
    if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_get_keys");
    tkv_amq_probe_metrics pm{};
    tkv_amq_get_counts gc{};
    // (blocking copies on the null stream: they wait for the lookup)
    if (hipMemcpy(out.data(), d_result.get(), sizeof(tkv_amq_get_result) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&pm, d_metrics, sizeof(pm), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&gc, d_counts, sizeof(gc), hipMemcpyDeviceToHost) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy found keys");
    if (counts) *counts = gc;
    Metrics& m = metrics();
    m.total_filter_query_count.add(pm.total_filter_query_count);
    m.no_filter_page_count.add(pm.no_filter_page_count);
    m.page_id_mismatch_count.add(pm.page_id_mismatch_count);
    m.filter_reject_count.add(pm.filter_reject_count);
    m.filter_positive_count.add(pm.filter_positive_count);
    m.filter_false_positive_count.add(pm.filter_false_positive_count);
    return OkStatus();
  }

  // The lookup from keys to resolved values in one call (tkv_amq_get_values): get_keys with the
  // value rule of the reference's find_key -- every found item's packed value folded as
  // combine_in_place folds it, ADD_I32 deltas summed through the older levels and the child until a
  // WRITE or a DELETE resolves them -- what TreeIndex::get_values_host computes on the host.
  //  d_leaf_values, ...        the leaves' packed values, parallel to the leaf keys: offsets
  //                            (n_leaf_keys + 1) or a fixed stride, and the buffer's size
  //  out                       (out) per key: the tkv_amq_value_result record
  //  slots, lengths, out_stride (out, optional; out_stride > 0) tkv_amq_gather_values behind the
  //                            lookup: slots[i * out_stride ..] holds the first min(length,
  //                            out_stride) bytes of key i's value, lengths[i] its full length
  // Adds every visit to metrics(), as get_keys does.
  Status get_values(FilterKind kind, const u8* d_filters, const tkv_amq_segment* d_segs,
                    const std::vector<tkv_amq_segment>& segs, TreeIndex& tree, const u8* d_leaf_keys,
                    const u64* d_leaf_key_offsets, u32 leaf_key_stride, u64 n_leaf_keys, const u8* d_leaf_values,
                    const u64* d_leaf_value_offsets, u32 leaf_value_stride, u64 leaf_values_bytes,
                    bool check_page_ids, std::vector<tkv_amq_value_result>& out,
                    tkv_amq_value_counts* counts = nullptr, std::vector<u8>* slots = nullptr,
                    std::vector<u32>* lengths = nullptr, u32 out_stride = 0)
  {
    const u64 n = keys_.size();
    out.assign(n, tkv_amq_value_result{~u64{0}, ~u64{0}, ~u32{0}, ~u32{0}, 0, (u8)TKV_AMQ_OP_NONE, 0, 0});
    if (counts) *counts = tkv_amq_value_counts{};
    const bool gather = slots && lengths && out_stride;
    if (gather) {
      slots->assign(n * out_stride, 0);
      lengths->assign(n, 0);
    }
    if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");
    if (n == 0) return OkStatus();
    TKV_AMQ_REQUIRE_OK(tree.upload());
    DeviceBuffer d_keys, d_offs, d_result, d_tallies, d_slots, d_lengths;
    constexpr usize kMetricsBytes = sizeof(tkv_amq_probe_metrics);
    if (!d_result.resize(sizeof(tkv_amq_value_result) * n) ||
        !d_tallies.resize(kMetricsBytes + sizeof(tkv_amq_value_counts)) ||
        (gather && (!d_slots.resize(n * out_stride) || !d_lengths.resize(4 * n))))
      return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
    bool fixed = false;
    u32 stride = 16;
    TKV_AMQ_REQUIRE_OK(detail::stage_keys(keys_, d_keys, d_offs, fixed, stride));
    if (hipMemset(d_tallies.get(), 0, kMetricsBytes + sizeof(tkv_amq_value_counts)) != hipSuccess ||
        (gather && hipMemset(d_slots.get(), 0, n * out_stride) != hipSuccess))
      return Status::from(TKV_AMQ_INTERNAL, "hipMemset counters");
    auto* d_metrics = d_tallies.get<tkv_amq_probe_metrics>();
    auto* d_counts = reinterpret_cast<tkv_amq_value_counts*>(d_tallies.get() + kMetricsBytes);
    int st = tree.get_values_device((int)kind, d_filters, d_segs, (u32)segs.size(), d_keys.get(),
                                    fixed ? nullptr : d_offs.get<u64>(), fixed ? stride : 0, n, d_leaf_keys,
                                    d_leaf_key_offsets, leaf_key_stride, n_leaf_keys, nullptr, d_leaf_values,
                                    d_leaf_value_offsets, leaf_value_stride, leaf_values_bytes,
                                    check_page_ids ? TKV_AMQ_GET_CHECK_PAGE_ID : 0u,
                                    d_result.get<tkv_amq_value_result>(), nullptr, d_metrics, d_counts);
    if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_get_values");
    if (gather) {
      st = tkv_amq_gather_values(d_result.get<tkv_amq_value_result>(), n, d_leaf_values, d_leaf_value_offsets,
                                 leaf_value_stride, leaf_values_bytes, n_leaf_keys, d_slots.get(), out_stride,
                                 d_lengths.get<u32>(), nullptr);
      if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_gather_values");
    }
    tkv_amq_probe_metrics pm{};
    tkv_amq_value_counts vc{};
    // (blocking copies on the null stream: they wait for the lookup and the gather)
    if (hipMemcpy(out.data(), d_result.get(), sizeof(tkv_amq_value_result) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&pm, d_metrics, sizeof(pm), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&vc, d_counts, sizeof(vc), hipMemcpyDeviceToHost) != hipSuccess ||
        (gather && (hipMemcpy(slots->data(), d_slots.get(), n * out_stride, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(lengths->data(), d_lengths.get(), 4 * n, hipMemcpyDeviceToHost) != hipSuccess)))
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy values");
    if (counts) *counts = vc;
    Metrics& m = metrics();
    m.total_filter_query_count.add(pm.total_filter_query_count);
    m.no_filter_page_count.add(pm.no_filter_page_count);
    m.page_id_mismatch_count.add(pm.page_id_mismatch_count);
    m.filter_reject_count.add(pm.filter_reject_count);
    m.filter_positive_count.add(pm.filter_positive_count);
    m.filter_false_positive_count.add(pm.filter_false_positive_count);
    return OkStatus();
  }

 private:
  std::vector<std::string_view> keys_;
};

// ---------------------------------------------------------------------------------------
// leaf update: {BatchUpdate} + {PackedLeafPage} => leaf (tree/subtree.cpp:170-191, 211-231) for a
// batch of leaves, on the device (tkv_amq_merge_leaves, tkv_amq_gather_merged)
// ---------------------------------------------------------------------------------------
// The merged leaves, device-resident: what FilterBatchBuilder, KeyQuery::verify_members and
// KeyQuery::get_values take as leaf keys, leaf values and key_begin.
struct MergedLeaves {
  DeviceBuffer items;          // tkv_amq_merge_item [n_items]
  DeviceBuffer out_begin;      // u64 [n_jobs + 1]
  DeviceBuffer keys, key_offsets;      // key_stride > 0: fixed slots, key_offsets unused; else u64 [n_items + 1]
  DeviceBuffer values, value_offsets;  // packed values and u64 [n_items + 1]
  u32 key_stride = 0;
  std::vector<u64> begin;      // out_begin on the host: leaf j holds items [begin[j], begin[j + 1])
  u64 n_items = 0, key_bytes = 0, value_bytes = 0;
  tkv_amq_merge_counts counts{};
};

// Job j merges the update's items newer.d_begin[j .. j + 1) over the leaf's items older.d_begin[j .. j + 1),
// each run strictly ascending: the newer item of a key stands, an ADD_I32 is folded with the older
// item, and with decay_to_items tombstones and no-ops are dropped (a leaf keeps them:
// ResultSet<decay_to_items = false>, tree/in_memory_leaf.hpp:35).  The outputs are sized from the
// inputs, so nothing is truncated; the counts and out_begin are copied back.
inline Status merge_leaves(const tkv_amq_merge_run& newer, const tkv_amq_merge_run& older, u64 n_jobs,
                           bool decay_to_items, MergedLeaves& out)
{
  out.begin.assign(1, 0);
  out.n_items = out.key_bytes = out.value_bytes = 0;
  out.counts = tkv_amq_merge_counts{};
  const u64 ws_bytes = tkv_amq_merge_leaves_ws_bytes(n_jobs, newer.n_items, older.n_items);
  if (ws_bytes == 0) return Status::from(TKV_AMQ_INVALID_ARGUMENT, "merge_leaves: too many jobs or items");
  if ((!newer.key_offsets && !newer.key_stride) || (!older.key_offsets && !older.key_stride) ||
      (!newer.value_offsets && !newer.value_stride) || (!older.value_offsets && !older.value_stride))
    return Status::from(TKV_AMQ_INVALID_ARGUMENT, "merge_leaves: a fixed form with stride 0");
  if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");
  const u64 cap = newer.n_items + older.n_items;
  const bool fixed = !newer.key_offsets && !older.key_offsets && newer.key_stride == older.key_stride;
  out.key_stride = fixed ? newer.key_stride : 0;
  auto key_bytes_of = [](const tkv_amq_merge_run& r, u64& bytes) {
    bytes = r.n_items * r.key_stride;
    if (!r.key_offsets || r.n_items == 0) return true;
    return hipMemcpy(&bytes, r.key_offsets + r.n_items, 8, hipMemcpyDeviceToHost) == hipSuccess;
  };
  u64 nk = 0, ok = 0;
  if (!key_bytes_of(newer, nk) || !key_bytes_of(older, ok)) return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy key offsets");
  const u64 k_cap = nk + ok;
  const u64 v_cap = tkv_amq_merge_values_bound(newer.values_bytes, older.values_bytes, newer.n_items);
  const u64 gather_ws = tkv_amq_gather_merged_ws_bytes(cap);
  DeviceBuffer ws, tallies;
  if (!ws.resize(std::max(ws_bytes, gather_ws)) || !tallies.resize(sizeof(tkv_amq_merge_counts)) ||
      !out.items.resize(sizeof(tkv_amq_merge_item) * cap) || !out.out_begin.resize(8 * (n_jobs + 1)) ||
      !out.keys.resize(k_cap) || (!fixed && !out.key_offsets.resize(8 * (cap + 1))) || !out.values.resize(v_cap) ||
      !out.value_offsets.resize(8 * (cap + 1)))
    return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
  if (hipMemset(tallies.get(), 0, sizeof(tkv_amq_merge_counts)) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemset counters");
  int st = tkv_amq_merge_leaves(&newer, &older, n_jobs, decay_to_items ? TKV_AMQ_MERGE_DECAY_TO_ITEMS : 0u,
                                out.out_begin.get<u64>(), out.items.get<tkv_amq_merge_item>(), cap, nullptr,
                                tallies.get<tkv_amq_merge_counts>(), ws.get(), ws.size(), nullptr);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_merge_leaves");
  st = tkv_amq_gather_merged(out.items.get<tkv_amq_merge_item>(), out.out_begin.get<u64>(), n_jobs, cap, &newer,
                             &older, out.keys.get(), out.key_stride, fixed ? nullptr : out.key_offsets.get<u64>(),
                             k_cap, out.values.get(), out.value_offsets.get<u64>(), v_cap, nullptr, ws.get(),
                             ws.size(), nullptr);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_gather_merged");
  out.begin.assign(n_jobs + 1, 0);
  // (blocking copies on the null stream: they wait for the merge and the gather)
  if (hipMemcpy(out.begin.data(), out.out_begin.get(), 8 * (n_jobs + 1), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&out.counts, tallies.get(), sizeof(out.counts), hipMemcpyDeviceToHost) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy merge results");
  out.n_items = out.begin.back();
  out.key_bytes = out.n_items * out.key_stride;
  if ((!fixed && hipMemcpy(&out.key_bytes, out.key_offsets.get<u64>() + out.n_items, 8, hipMemcpyDeviceToHost) != hipSuccess) ||
      hipMemcpy(&out.value_bytes, out.value_offsets.get<u64>() + out.n_items, 8, hipMemcpyDeviceToHost) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy merge sizes");
  return OkStatus();
}

// ---------------------------------------------------------------------------------------
// node merge: merge_compact_edits over the K levels InMemoryNode::push_levels_to_merge pushes
// (tree/in_memory_node.cpp:827-866; core/algo/merge_compact_edits.hpp:26-148), for a batch of key
// ranges, on the device (tkv_amq_merge_levels, tkv_amq_gather_levels)
// ---------------------------------------------------------------------------------------
// Job j merges items runs[s].d_begin[j .. j + 1) of every run s, runs[0] the newest, each strictly
// ascending: the newest item of a key stands, an ADD_I32 is folded through the older items of its key
// while it stays one, and with decay_to_items tombstones and no-ops are dropped.  The counterpart of
// merge_leaves: the outputs are sized from the inputs, the counts and out_begin are copied back.
inline Status merge_levels(const tkv_amq_merge_run* runs, u32 n_runs, u64 n_jobs, bool decay_to_items,
                           MergedLeaves& out)
{
  out.begin.assign(1, 0);
  out.n_items = out.key_bytes = out.value_bytes = 0;
  out.counts = tkv_amq_merge_counts{};
  if (!runs || n_runs == 0 || n_runs > TKV_AMQ_MERGE_MAX_RUNS)
    return Status::from(TKV_AMQ_INVALID_ARGUMENT, "merge_levels: 1 to 8 runs");
  u64 cap = 0, values_bytes = 0;
  bool fixed = true;
  for (u32 s = 0; s < n_runs; ++s) {
    const tkv_amq_merge_run& r = runs[s];
    if ((!r.key_offsets && !r.key_stride) || (!r.value_offsets && !r.value_stride))
      return Status::from(TKV_AMQ_INVALID_ARGUMENT, "merge_levels: a fixed form with stride 0");
    if (r.n_items > 0xffffffffull) return Status::from(TKV_AMQ_INVALID_ARGUMENT, "merge_levels: too many items");
    cap += r.n_items;
    values_bytes += r.values_bytes;
    fixed = fixed && !r.key_offsets && r.key_stride == runs[0].key_stride;
  }
  const u64 ws_bytes = tkv_amq_merge_levels_ws_bytes(n_jobs, n_runs, cap);
  if (ws_bytes == 0) return Status::from(TKV_AMQ_INVALID_ARGUMENT, "merge_levels: too many jobs or items");
  if (tkv_amq_device_count() == 0) return Status::from(TKV_AMQ_UNAVAILABLE, "no HIP device");
  out.key_stride = fixed ? runs[0].key_stride : 0;
  u64 k_cap = 0;
  for (u32 s = 0; s < n_runs; ++s) {
    const tkv_amq_merge_run& r = runs[s];
    u64 bytes = r.n_items * r.key_stride;
    if (r.key_offsets && r.n_items &&
        hipMemcpy(&bytes, r.key_offsets + r.n_items, 8, hipMemcpyDeviceToHost) != hipSuccess)
      return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy key offsets");
    k_cap += bytes;
  }
  const u64 v_cap = tkv_amq_merge_levels_values_bound(values_bytes, cap - runs[n_runs - 1].n_items);
  const u64 gather_ws = tkv_amq_gather_levels_ws_bytes(cap);
  DeviceBuffer ws, tallies;
  if (!ws.resize(std::max(ws_bytes, gather_ws)) || !tallies.resize(sizeof(tkv_amq_merge_counts)) ||
      !out.items.resize(sizeof(tkv_amq_merge_item) * cap) || !out.out_begin.resize(8 * (n_jobs + 1)) ||
      !out.keys.resize(k_cap) || (!fixed && !out.key_offsets.resize(8 * (cap + 1))) || !out.values.resize(v_cap) ||
      !out.value_offsets.resize(8 * (cap + 1)))
    return Status::from(TKV_AMQ_RESOURCE_EXHAUSTED, "hipMalloc");
  if (hipMemset(tallies.get(), 0, sizeof(tkv_amq_merge_counts)) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemset counters");
  int st = tkv_amq_merge_levels(runs, n_runs, n_jobs, decay_to_items ? TKV_AMQ_MERGE_DECAY_TO_ITEMS : 0u,
                                out.out_begin.get<u64>(), out.items.get<tkv_amq_merge_item>(), cap, nullptr,
                                tallies.get<tkv_amq_merge_counts>(), ws.get(), ws.size(), nullptr);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_merge_levels");
  st = tkv_amq_gather_levels(out.items.get<tkv_amq_merge_item>(), out.out_begin.get<u64>(), n_jobs, cap, runs, n_runs,
                             out.keys.get(), out.key_stride, fixed ? nullptr : out.key_offsets.get<u64>(), k_cap,
                             out.values.get(), out.value_offsets.get<u64>(), v_cap, nullptr, ws.get(), ws.size(),
                             nullptr);
  if (st != TKV_AMQ_OK) return Status::from(st, "tkv_amq_gather_levels");
  out.begin.assign(n_jobs + 1, 0);
  // (blocking copies on the null stream: they wait for the merge and the gather)
  if (hipMemcpy(out.begin.data(), out.out_begin.get(), 8 * (n_jobs + 1), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&out.counts, tallies.get(), sizeof(out.counts), hipMemcpyDeviceToHost) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy merge results");
  out.n_items = out.begin.back();
  out.key_bytes = out.n_items * out.key_stride;
  if ((!fixed && hipMemcpy(&out.key_bytes, out.key_offsets.get<u64>() + out.n_items, 8, hipMemcpyDeviceToHost) != hipSuccess) ||
      hipMemcpy(&out.value_bytes, out.value_offsets.get<u64>() + out.n_items, 8, hipMemcpyDeviceToHost) != hipSuccess)
    return Status::from(TKV_AMQ_INTERNAL, "hipMemcpy merge sizes");
  return OkStatus();
}

}  // namespace turtle_kv_amd
