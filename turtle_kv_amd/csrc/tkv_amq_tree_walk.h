// tkv_amq_tree_walk.h -- one lookup's descent through the flat tree, once: what the path walk
// (tkv_amq_walk.hip: tkv_amq_walk_paths) and the fused lookup (tkv_amq_kernels.hip:
// tkv_amq_get_keys) agree on.
//
// Per node a branch-free upper bound over the interior pivot keys (find_pivot_containing,
// tree/algo/nodes.hpp:48-71), then the active_pivots bit sets of the node's segments, level by
// level (find_key, :158-187; for_each_active_segment_in, tree/algo/segmented_levels.hpp:340-369),
// then child p.  Every index is checked against its array before the read, so a malformed tree
// gives a defined answer (the rules are listed at tkv_amq_walk_paths in tkv_amq.h).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "tkv_amq.h"
#include "tkv_amq_device.h"

namespace tkv {

static_assert(sizeof(tkv_amq_tree_node) == 32 && sizeof(tkv_amq_tree_segment) == 32 &&
                  sizeof(tkv_amq_tree_child) == 16,
              "tree records");

// the tree as the entry points take it
struct TreeArgs {
  const tkv_amq_tree_node* nodes;
  const tkv_amq_tree_segment* segs;
  const tkv_amq_tree_child* children;
  const uint32_t* bounds;
  uint32_t n_nodes, n_segs, n_children, n_bounds;
  const uint8_t* pk;
  const uint64_t* pkoffs;
  uint32_t pkstride;
  uint32_t n_pk;
};

// The pivot of the query in a node that owns keys k0..kp from `key_begin`: the number of interior
// keys k1..k(p-1) that are <= the query (std::upper_bound over them).  k0 and kp are never read;
// interior keys at or past n_pk do not exist.
template <int MODE>
__device__ inline uint32_t find_pivot(const TreeArgs& a, const OrderedQuery<MODE>& q, uint32_t key_begin,
                                      uint32_t pivot_count)
{
  const uint64_t first = (uint64_t)key_begin + 1;
  const uint64_t have = first < a.n_pk ? a.n_pk - first : 0;
  uint32_t len = pivot_count - 1;
  len = have < len ? (uint32_t)have : len;
  // lanes in nodes of equal fan-out take the same trip count (at most 6)
  const KeyArray pk{a.pk, a.pkoffs, a.pkstride};
  return (uint32_t)(bound(first, len, [&](uint64_t k) { return q.less_equal(pk, k); }) - first);
}

// What a segment entry tells the descent to do next: go on with the level's next segment, leave
// the level (its remaining segments are skipped: the reference's kBreak, tree/algo/
// segments.hpp:185-200), or end the walk.
enum WalkStep : uint32_t { kWalkContinue = 0, kWalkLeaveLevel = 1, kWalkStop = 2 };

// Segment s as an entry for pivot p: its leaf, the leaf's page id and, if want_bound, the flushed
// item upper bound for p (0 if bit p of flushed_pivots is clear or the index lies past n_bounds).
__device__ inline void segment_entry(const TreeArgs& a, uint32_t s, uint32_t p, bool want_bound, uint32_t& leaf,
                                     uint64_t& page_id, uint32_t& flushed_bound)
{
  const uint4* sp = reinterpret_cast<const uint4*>(a.segs + s);
  const uint4 s0 = sp[0], s1 = sp[1];  // {leaf_page_id, active}, {flushed, leaf, flushed_begin}
  const uint64_t flushed = mk64(s1.x, s1.y);
  uint32_t bound = 0;
  if (want_bound && ((flushed >> p) & 1u)) {
    // bit_rank: the set bits of flushed_pivots below p
    const uint64_t at = (uint64_t)s1.w + (uint32_t)__popcll(flushed & ((1ull << p) - 1));
    if (at < a.n_bounds) bound = a.bounds[at];
  }
  leaf = s1.z;
  page_id = mk64(s0.x, s0.y);
  flushed_bound = bound;
}

// One query's descent.  pivot(depth, key_begin, pivot_count) names the pivot; entry(seg index, p,
// where) is called for every segment active for it and answers with a WalkStep; leaf(index, page
// id, where) is called for the child leaf, where the walk ends.
template <class Pivot, class Entry, class Leaf>
__device__ inline void walk_tree(const TreeArgs& a, Pivot&& pivot, Entry&& entry, Leaf&& leaf)
{
  uint32_t ni = 0;
  for (uint32_t depth = 0; depth < TKV_AMQ_WALK_MAX_DEPTH; ++depth) {
    if (ni >= a.n_nodes) return;
    const uint4* np = reinterpret_cast<const uint4*>(a.nodes + ni);
    const uint4 n0 = np[0], n1 = np[1];  // {pivot_key_begin, seg_begin, child_begin, -}, {counts, level_start, -}
    const uint32_t pivot_count = n1.x & 0xffu, height = (n1.x >> 8) & 0xffu;
    const uint32_t level_count = min((n1.x >> 16) & 0xffu, 7u);
    if (pivot_count == 0 || pivot_count > 64) return;
    const uint32_t p = pivot(depth, n0.x, pivot_count);
    const uint64_t bit = 1ull << p;
    const uint64_t level_start = mk64(n1.y, n1.z);
    for (uint32_t l = 0; l < level_count; ++l) {
      // (64-bit sums cannot wrap; a decreasing level_start gives end <= begin: an empty level)
      const uint64_t lb = (uint64_t)n0.y + ((level_start >> (8 * l)) & 0xffu);
      const uint64_t le = (uint64_t)n0.y + ((level_start >> (8 * l + 8)) & 0xffu);
      const uint32_t sb = (uint32_t)min(lb, (uint64_t)a.n_segs), se = (uint32_t)min(le, (uint64_t)a.n_segs);
      for (uint32_t s = sb; s < se; ++s)
        if (a.segs[s].active_pivots & bit) {
          const WalkStep step = entry(s, p, (depth << 8) | l);
          if (step == kWalkStop) return;
          if (step == kWalkLeaveLevel) break;
        }
    }
    const uint64_t c = (uint64_t)n0.z + p;
    if (c >= a.n_children) return;
    const uint4 ch = *reinterpret_cast<const uint4*>(a.children + c);  // {page_id, index, -}
    if (height <= 1) {
      leaf(ch.z, mk64(ch.x, ch.y), (depth << 8) | TKV_AMQ_WALK_LEAF_LEVEL);
      return;
    }
    ni = ch.z;
  }
}

}  // namespace tkv
