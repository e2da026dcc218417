// tkv_amq_find.hip -- the leaf search behind the filters: tkv_amq_find_keys.
//
//   find_keys_kernel  one lane per query (grid-stride).  The lane walks its query's candidates in
//                     path order; per candidate a branch-free lower bound over the leaf's sorted
//                     keys (find_key_in_leaf_impl, tree/key_query.cpp:299-327), an equality test,
//                     and -- unless TKV_AMQ_FIND_ALL -- the walk ends at the first leaf that holds
//                     the key (tree/algo/nodes.hpp:165-187).  A searched candidate without the key
//                     whose reject_page class is "checked" is a filter false positive
//                     (key_query.cpp:76-78); the class comes from the helpers the probes use
//                     (load_probe_desc, page_id_matches).
//
// The workload has about one candidate per query that exists and about none for one that does
// not, so a lane per query needs no second pass for the early exit and no atomics on an output; a
// query with hundreds of candidates is serial in its lane.  Every search step is one dependent
// random read: the kernel is bound by latency, and its throughput comes from waves in flight
// (DESIGN.md section 14).  Keys are compared as big-endian words, so an unsigned integer compare
// is memcmp: the query is held that way in registers (16- and 24-byte fast modes); any other
// shape is compared from memory, 8 bytes at a time where both keys have them, then 4, then
// bytes, then the lengths -- never past a key's end.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "tkv_amq.h"
#include "tkv_amq_device.h"

namespace tkv {
namespace {

constexpr uint32_t kFindThreads = 256;
// the grid-stride loop's workgroups at most: two rounds of a full machine (256 CUs x 8
// workgroups), so the counters take at most 16,384 waves' atomics each, spread over the run
constexpr uint32_t kFindMaxGrid = 4096;

struct FindArgs {
  const uint8_t* filters;
  const tkv_amq_segment* segs;
  uint32_t n_segs;
  uint32_t id_off;  // the payload's src_page_id: PackedBloomFilterPage @16, PackedVqfFilter @8
  int kind;
  uint32_t flags;
  const uint8_t* q;
  const uint64_t* qoffs;
  uint32_t qstride;
  uint32_t n_queries;
  const uint32_t* cand_begin;
  const uint32_t* cand_leaf;
  const uint32_t* cand_entry;
  uint32_t n_cand;
  uint32_t kstride;
  const uint8_t* keys;
  const uint64_t* koffs;
  uint64_t n_keys;
  const uint64_t* key_begin;
  tkv_amq_find_result* result;
  uint8_t* state;
  const uint64_t* page_ids;
  tkv_amq_probe_metrics* metrics;
  tkv_amq_find_counts* counts;
};

// reject_page's class of (candidate at `pos`, leaf), as the probes compute it: is it kChecked?
__device__ inline bool find_checked(const FindArgs& a, uint32_t leaf, uint32_t pos)
{
  const ProbeDesc d = load_probe_desc(a.segs, leaf, a.n_segs);
  uint32_t cls = (a.kind == TKV_AMQ_BLOOM ? d.hash_count : d.tag_bits) == 0 ? kNoFilter : kChecked;
  if (cls == kChecked && a.page_ids != nullptr &&
      !page_id_matches(a.filters + d.out_offset, a.id_off, a.page_ids, a.cand_entry[pos]))
    cls = kIdMismatch;
  return cls == kChecked;
}

template <int MODE>
__global__ __launch_bounds__(kFindThreads) void find_keys_kernel(FindArgs a)
{
  uint32_t n_search = 0, n_found = 0, n_absent = 0, n_unsearchable = 0, n_false_pos = 0;
  const bool all = (a.flags & TKV_AMQ_FIND_ALL) != 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kFindThreads + threadIdx.x; i < a.n_queries;
       i += (uint64_t)gridDim.x * kFindThreads) {
    // positions [cb, ce) of query i: both ends clamped to n_cand, end < begin reads as empty
    const uint32_t cb = min(a.cand_begin[i], a.n_cand);
    uint32_t ce = min(a.cand_begin[i + 1], a.n_cand);
    if (ce < cb) ce = cb;
    uint64_t r_key = ~0ull;
    uint32_t r_leaf = ~0u, r_cand = ~0u;
    if (cb < ce) {  // (a query without candidates does not load its key)
      const KeyArray ks{a.keys, a.koffs, a.kstride};
      const OrderedQuery<MODE> q(KeyArray{a.q, a.qoffs, a.qstride}, i);
      bool done = false;
      for (uint32_t pos = cb; pos < ce; ++pos) {
        uint32_t st = TKV_AMQ_CAND_NOT_SEARCHED;
        if (!done || all) {
          const uint32_t leaf = a.cand_leaf[pos];
          if (leaf >= a.n_segs) {
            st = TKV_AMQ_CAND_UNSEARCHABLE;
            ++n_unsearchable;
          } else {
            uint64_t b, e;
            leaf_key_range(a.key_begin, a.segs, leaf, a.n_keys, b, e);
            // the lower bound: lanes with leaves of equal size take the same trip count
            b = bound(b, e - b, [&](uint64_t k) { return q.less(ks, k); });
            const bool hit = b < e && q.equal(ks, b);
            ++n_search;
            if (hit) {
              st = TKV_AMQ_CAND_FOUND;
              if (!done) {
                r_key = b;
                r_leaf = leaf;
                r_cand = pos;
                done = true;
                ++n_found;
              }
            } else {
              st = TKV_AMQ_CAND_ABSENT;
              ++n_absent;
              if (a.metrics && find_checked(a, leaf, pos)) ++n_false_pos;
            }
          }
        }
        if (a.state) a.state[pos] = (uint8_t)st;
        else if (done && !all) break;
      }
    }
    *reinterpret_cast<ulonglong2*>(a.result + i) = ulonglong2{r_key, mk64(r_leaf, r_cand)};
  }
  // one atomic per non-zero counter per wave
  const uint32_t v[5] = {wave_sum(n_search), wave_sum(n_found), wave_sum(n_absent), wave_sum(n_unsearchable),
                         wave_sum(n_false_pos)};
  if (__lane_id() == 0) {
    if (a.counts) {
      unsigned long long* c = reinterpret_cast<unsigned long long*>(a.counts);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (v[j]) atomicAdd(&c[j], (unsigned long long)v[j]);
    }
    if (a.metrics && v[4])
      atomicAdd(reinterpret_cast<unsigned long long*>(&a.metrics->filter_false_positive_count),
                (unsigned long long)v[4]);
  }
}

}  // namespace
}  // namespace tkv

using namespace tkv;

extern "C" {

int tkv_amq_find_keys(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                      const uint8_t* queries, const uint64_t* query_offsets, uint32_t query_stride,
                      uint64_t n_queries, const uint32_t* d_cand_begin, const uint32_t* d_cand_leaf,
                      const uint32_t* d_cand_entry, uint64_t n_cand, const uint8_t* leaf_keys,
                      const uint64_t* leaf_key_offsets, uint32_t leaf_key_stride, uint64_t n_leaf_keys,
                      const uint64_t* d_key_begin, uint32_t flags, tkv_amq_find_result* d_result,
                      uint8_t* d_cand_state, const tkv_amq_probe_opts* opts, tkv_amq_find_counts* d_counts,
                      void* stream)
{
  // (the arguments are judged first, so a bad call is InvalidArgument with or without a device)
  if (kind != TKV_AMQ_BLOOM && kind != TKV_AMQ_VQF) return TKV_AMQ_INVALID_ARGUMENT;
  if (flags & ~TKV_AMQ_FIND_ALL) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_queries > 0xffffffffull || n_cand > 0xffffffffull) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_queries && (!d_cand_begin || !d_result || !queries)) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_cand && !d_cand_leaf) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_segs && !d_segs) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_leaf_keys && !leaf_keys) return TKV_AMQ_INVALID_ARGUMENT;
  if ((!query_offsets && !query_stride) || (!leaf_key_offsets && !leaf_key_stride))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (opts && opts->d_query_page_id && (!d_cand_entry || !d_filters)) return TKV_AMQ_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(d_result) & 15) || (reinterpret_cast<uintptr_t>(d_counts) & 7))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n_queries == 0) return TKV_AMQ_OK;
  FindArgs a;
  a.filters = d_filters;
  a.segs = d_segs;
  a.n_segs = n_segs;
  a.id_off = src_page_id_offset(kind);
  a.kind = kind;
  a.flags = flags;
  a.q = queries;
  a.qoffs = query_offsets;
  a.qstride = query_stride;
  a.n_queries = (uint32_t)n_queries;
  a.cand_begin = d_cand_begin;
  a.cand_leaf = d_cand_leaf;
  a.cand_entry = d_cand_entry;
  a.n_cand = (uint32_t)n_cand;
  a.kstride = leaf_key_stride;
  a.keys = leaf_keys;
  a.koffs = leaf_key_offsets;
  a.n_keys = n_leaf_keys;
  a.key_begin = d_key_begin;
  a.result = d_result;
  a.state = d_cand_state;
  a.page_ids = opts ? opts->d_query_page_id : nullptr;
  a.metrics = opts ? opts->d_metrics : nullptr;
  a.counts = d_counts;
  const int mode = key_order_mode(KeyArray{queries, query_offsets, query_stride},
                                  KeyArray{leaf_keys, leaf_key_offsets, leaf_key_stride});
  const uint64_t wgs = (n_queries + kFindThreads - 1) / kFindThreads;
  const dim3 grid((uint32_t)(wgs < kFindMaxGrid ? wgs : kFindMaxGrid)), block(kFindThreads);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == kOrder16) hipLaunchKernelGGL(find_keys_kernel<kOrder16>, grid, block, 0, s, a);
  else if (mode == kOrder24) hipLaunchKernelGGL(find_keys_kernel<kOrder24>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(find_keys_kernel<kOrderAny>, grid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

}  // extern "C"
