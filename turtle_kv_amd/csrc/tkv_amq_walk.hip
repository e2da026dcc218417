// tkv_amq_walk.hip -- the tree descent in front of the path probe: tkv_amq_walk_paths.
//
//   walk_count_kernel  one lane per query (workgroup tiles of 256, grid-stride).  The lane descends
//                      from node 0: per node a branch-free upper bound over the interior pivot keys
//                      (find_pivot_containing, tree/algo/nodes.hpp:48-71), then the active_pivots
//                      bit sets of the node's segments, level by level (find_key, :158-187;
//                      for_each_active_segment_in, tree/algo/segmented_levels.hpp:340-369), then
//                      child p.  It counts the entries, keeps the pivot of every depth in the
//                      workspace (6 bits x 16 depths) and leaves the tile's exclusive prefix in
//                      path_begin and the tile's total in the workspace.
//   scan_totals<u64>   (tkv_amq_scan.h) one workgroup: the tiles' totals to 64-bit exclusive
//                      prefixes; the total.
//   walk_write_kernel  the same descent with the pivots read back: no key is compared again, only
//                      nodes, bit sets and children are re-read; entries go to their positions.
//
// Both descents are one function (walk_tree, tkv_amq_tree_walk.h: shared with tkv_amq_get_keys) with
// the pivot source and the entry sink as arguments, so the two passes cannot disagree about a
// path.  A tree over thousands of leaves is about a hundred nodes: it stays in L2, every step is
// a dependent L2 read, and the throughput comes from waves in flight.
// Every index is checked against its array before the read, so a malformed tree gives a defined
// answer.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "tkv_amq.h"
#include "tkv_amq_device.h"
#include "tkv_amq_scan.h"
#include "tkv_amq_tree_walk.h"

namespace tkv {
namespace {

constexpr uint32_t kWalkThreads = 256;
// the tile loop's workgroups at most: one round of a full machine (256 CUs x 8 workgroups)
constexpr uint32_t kWalkMaxGrid = 2048;
// tile totals a thread of the totals scan takes per pass (tests/test_gpu_walk.py sizes the batch
// that needs a second pass from it)
constexpr uint32_t kWalkScanPerThread = 4;
constexpr uint32_t kWalkTrailSplit = 10;  // depths 0..9 in the trail's low word, 10..15 in the high

static_assert(kWalkThreads == kBlockScanThreads && kWalkScanPerThread == kScanTotalsPerThread,
              "a tile is one block scan; scan_totals' span");
static_assert(TKV_AMQ_WALK_MAX_DEPTH == 16, "the trail holds 16 pivots of 6 bits");

// (the tree, TreeArgs, comes first: the layout the kernels had before the descent was shared)
struct WalkArgs : TreeArgs {
  const uint8_t* q;
  const uint64_t* qoffs;
  uint32_t qstride;
  uint32_t n_queries;
  uint32_t n_tiles;
  uint32_t capacity;
  uint32_t* path_begin;
  uint32_t* path_leaf;
  uint64_t* path_page_id;
  uint32_t* path_flushed;
  uint16_t* path_where;
  uint64_t* needed;
  ulonglong2* trail;     // [n_queries]
  uint64_t* tile_total;  // [n_tiles]: totals, then their exclusive prefixes
};

// The pivots of one walk, 6 bits per depth.
struct Trail {
  uint64_t lo = 0, hi = 0;
  __device__ inline void put(uint32_t depth, uint32_t p)
  {
    if (depth < kWalkTrailSplit) lo |= (uint64_t)p << (6 * depth);
    else hi |= (uint64_t)p << (6 * (depth - kWalkTrailSplit));
  }
  __device__ inline uint32_t get(uint32_t depth) const
  {
    const uint64_t w = depth < kWalkTrailSplit ? lo >> (6 * depth) : hi >> (6 * (depth - kWalkTrailSplit));
    return (uint32_t)w & 63u;
  }
};

// exclusive scan of v over the workgroup's 256 threads; *total = the sum.  s: 4 words of LDS.
// The scheme of block_exclusive_scan (tkv_amq_scan.h) with the barriers placed differently.  Kept
// for walk_count_kernel: with the shared scan one of the walk's four timed rows had its median
// 0.008 ms above the previous code's range (profiles/read_side_shared/README.md).
__device__ inline uint32_t walk_block_scan(uint32_t v, uint32_t* s, uint32_t* total)
{
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  __syncthreads();  // (the previous use of s is over)
  if (lane == 63) s[wave] = x;
  __syncthreads();
  uint32_t base = 0, sum = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWalkThreads / 64; ++w) {
    const uint32_t t = s[w];
    if (w < wave) base += t;
    sum += t;
  }
  *total = sum;
  return base + x - v;
}

template <int MODE>
__global__ __launch_bounds__(kWalkThreads) void walk_count_kernel(WalkArgs a)
{
  __shared__ uint32_t s_scan[kWalkThreads / 64];
  for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const uint64_t i = (uint64_t)t * kWalkThreads + threadIdx.x;
    const bool live = i < a.n_queries;
    uint32_t cnt = 0;
    if (live) {
      const OrderedQuery<MODE> q(KeyArray{a.q, a.qoffs, a.qstride}, i);
      Trail trail;
      walk_tree(
          a,
          [&](uint32_t depth, uint32_t key_begin, uint32_t pivot_count) {
            const uint32_t p = find_pivot<MODE>(a, q, key_begin, pivot_count);
            trail.put(depth, p);
            return p;
          },
          [&](uint32_t, uint32_t, uint32_t) {
            ++cnt;
            return kWalkContinue;
          },
          [&](uint32_t, uint64_t, uint32_t) { ++cnt; });
      a.trail[i] = ulonglong2{trail.lo, trail.hi};
    }
    uint32_t total;
    const uint32_t pre = walk_block_scan(cnt, s_scan, &total);
    if (live) a.path_begin[i] = pre;
    if (threadIdx.x == 0) a.tile_total[t] = total;
  }
}

__global__ __launch_bounds__(kWalkThreads) void walk_write_kernel(WalkArgs a)
{
  for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const uint64_t i = (uint64_t)t * kWalkThreads + threadIdx.x;
    if (i >= a.n_queries) continue;
    uint64_t pos = a.tile_total[t] + a.path_begin[i];
    a.path_begin[i] = (uint32_t)min(pos, (uint64_t)a.capacity);
    if (pos >= a.capacity) continue;  // (every entry of this query lies past the capacity)
    const ulonglong2 tv = a.trail[i];
    Trail trail;
    trail.lo = tv.x;
    trail.hi = tv.y;
    auto put = [&](uint32_t leaf, uint64_t page_id, uint32_t flushed, uint32_t where) {
      if (pos < a.capacity) {
        a.path_leaf[pos] = leaf;
        if (a.path_page_id) a.path_page_id[pos] = page_id;
        if (a.path_flushed) a.path_flushed[pos] = flushed;
        if (a.path_where) a.path_where[pos] = (uint16_t)where;
      }
      ++pos;
    };
    walk_tree(
        a, [&](uint32_t depth, uint32_t, uint32_t) { return trail.get(depth); },
        [&](uint32_t s, uint32_t p, uint32_t where) {
          uint32_t leaf, bound;
          uint64_t page_id;
          segment_entry(a, s, p, a.path_flushed != nullptr, leaf, page_id, bound);
          put(leaf, page_id, bound, where);
          return kWalkContinue;
        },
        [&](uint32_t index, uint64_t page_id, uint32_t where) { put(index, page_id, 0u, where); });
  }
}

struct WalkWsLayout {
  uint64_t n_tiles, totals_off, trail_off, bytes;
};

inline WalkWsLayout walk_ws_layout(uint64_t n_queries)
{
  WalkWsLayout l;
  l.n_tiles = (n_queries + kWalkThreads - 1) / kWalkThreads;
  l.trail_off = 16;
  l.totals_off = l.trail_off + 16 * n_queries;
  l.bytes = l.totals_off + (8 * l.n_tiles + 15) / 16 * 16;
  return l;
}

}  // namespace
}  // namespace tkv

using namespace tkv;

extern "C" {

uint64_t tkv_amq_walk_paths_ws_bytes(uint64_t n_queries)
{
  if (n_queries > 0xffffffffull) return 0;
  return walk_ws_layout(n_queries).bytes;
}

int tkv_amq_walk_paths(const tkv_amq_tree_node* nodes, uint64_t n_nodes, const tkv_amq_tree_segment* segments,
                       uint64_t n_segments, const tkv_amq_tree_child* children, uint64_t n_children,
                       const uint32_t* d_flushed_bounds, uint64_t n_flushed_bounds, const uint8_t* pivot_keys,
                       const uint64_t* pivot_key_offsets, uint32_t pivot_key_stride, uint64_t n_pivot_keys,
                       const uint8_t* queries, const uint64_t* query_offsets, uint32_t query_stride,
                       uint64_t n_queries, uint32_t* d_path_begin, uint32_t* d_path_leaf,
                       uint64_t* d_path_page_id, uint32_t* d_path_flushed, uint16_t* d_path_where,
                       uint64_t path_capacity, uint64_t* d_needed, void* d_workspace, uint64_t workspace_bytes,
                       void* stream)
{
  // (the arguments are judged first, so a bad call is InvalidArgument with or without a device)
  constexpr uint64_t kMax = 0xffffffffull;
  if (n_nodes > kMax || n_segments > kMax || n_children > kMax || n_flushed_bounds > kMax ||
      n_pivot_keys > kMax || n_queries > kMax || path_capacity > kMax)
    return TKV_AMQ_INVALID_ARGUMENT;
  if ((n_nodes && !nodes) || (n_segments && !segments) || (n_children && !children) ||
      (n_flushed_bounds && !d_flushed_bounds) || (n_pivot_keys && !pivot_keys))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (n_queries && (!queries || !d_path_begin || !d_workspace)) return TKV_AMQ_INVALID_ARGUMENT;
  if (path_capacity && !d_path_leaf) return TKV_AMQ_INVALID_ARGUMENT;
  if ((!pivot_key_offsets && !pivot_key_stride) || (!query_offsets && !query_stride))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (((reinterpret_cast<uintptr_t>(nodes) | reinterpret_cast<uintptr_t>(segments) |
        reinterpret_cast<uintptr_t>(children) | reinterpret_cast<uintptr_t>(d_workspace)) & 15) ||
      (reinterpret_cast<uintptr_t>(d_needed) & 7))
    return TKV_AMQ_INVALID_ARGUMENT;
  const WalkWsLayout l = walk_ws_layout(n_queries);
  if (n_queries && workspace_bytes < l.bytes) return TKV_AMQ_INVALID_ARGUMENT;
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(kWalkThreads);
  if (n_queries == 0) {
    if (d_path_begin || d_needed) {
      hipLaunchKernelGGL(scan_totals<uint64_t>, dim3(1), block, 0, s, static_cast<uint64_t*>(nullptr), 0u,
                         d_path_begin, 0u, d_needed);
      return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
    }
    return TKV_AMQ_OK;
  }
  uint8_t* ws = static_cast<uint8_t*>(d_workspace);
  WalkArgs a;
  a.nodes = nodes;
  a.segs = segments;
  a.children = children;
  a.bounds = d_flushed_bounds;
  a.n_nodes = (uint32_t)n_nodes;
  a.n_segs = (uint32_t)n_segments;
  a.n_children = (uint32_t)n_children;
  a.n_bounds = (uint32_t)n_flushed_bounds;
  a.pk = pivot_keys;
  a.pkoffs = pivot_key_offsets;
  a.pkstride = pivot_key_stride;
  a.n_pk = (uint32_t)n_pivot_keys;
  a.q = queries;
  a.qoffs = query_offsets;
  a.qstride = query_stride;
  a.n_queries = (uint32_t)n_queries;
  a.n_tiles = (uint32_t)l.n_tiles;
  a.capacity = (uint32_t)path_capacity;
  a.path_begin = d_path_begin;
  a.path_leaf = d_path_leaf;
  a.path_page_id = d_path_page_id;
  a.path_flushed = d_path_flushed;
  a.path_where = d_path_where;
  a.needed = d_needed;
  a.trail = reinterpret_cast<ulonglong2*>(ws + l.trail_off);
  a.tile_total = reinterpret_cast<uint64_t*>(ws + l.totals_off);
  const int mode = key_order_mode(KeyArray{queries, query_offsets, query_stride},
                                  KeyArray{pivot_keys, pivot_key_offsets, pivot_key_stride});
  const dim3 grid(a.n_tiles < kWalkMaxGrid ? a.n_tiles : kWalkMaxGrid);
  if (mode == kOrder16) hipLaunchKernelGGL(walk_count_kernel<kOrder16>, grid, block, 0, s, a);
  else if (mode == kOrder24) hipLaunchKernelGGL(walk_count_kernel<kOrder24>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(walk_count_kernel<kOrderAny>, grid, block, 0, s, a);
  hipLaunchKernelGGL(scan_totals<uint64_t>, dim3(1), block, 0, s, a.tile_total, a.n_tiles,
                     d_path_begin + a.n_queries, a.capacity, d_needed);
  hipLaunchKernelGGL(walk_write_kernel, grid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

}  // extern "C"
