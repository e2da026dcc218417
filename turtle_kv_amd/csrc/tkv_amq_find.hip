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

// kFind16: both sides fixed 16-byte keys, 16-byte aligned; kFind24: both fixed 24-byte keys,
// 8-byte aligned; kFindAny: everything else (other strides, offsets on either side, misaligned)
enum FindMode : int { kFind16 = 0, kFind24 = 1, kFindAny = 2 };

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

// The query of one lane, and its comparison with leaf key `i`.
template <int MODE>
struct FindQuery;

template <>
struct FindQuery<kFind16> {
  uint64_t w0, w1;
  __device__ inline FindQuery(const FindArgs& a, uint64_t i)
  {
    const uint4 v = *reinterpret_cast<const uint4*>(a.q + 16 * i);
    w0 = be64(v.x, v.y);
    w1 = be64(v.z, v.w);
  }
  // one global_load_dwordx4, two u64 compares
  __device__ inline void load(const FindArgs& a, uint64_t i, uint64_t& k0, uint64_t& k1) const
  {
    const uint4 v = *reinterpret_cast<const uint4*>(a.keys + 16 * i);
    k0 = be64(v.x, v.y);
    k1 = be64(v.z, v.w);
  }
  __device__ inline bool less(const FindArgs& a, uint64_t i) const
  {
    uint64_t k0, k1;
    load(a, i, k0, k1);
    return k0 < w0 || (k0 == w0 && k1 < w1);
  }
  __device__ inline bool equal(const FindArgs& a, uint64_t i) const
  {
    uint64_t k0, k1;
    load(a, i, k0, k1);
    return k0 == w0 && k1 == w1;
  }
};

template <>
struct FindQuery<kFind24> {
  uint64_t w0, w1, w2;
  __device__ inline FindQuery(const FindArgs& a, uint64_t i)
  {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(a.q + 24 * i);
    w0 = __builtin_bswap64(p[0]);
    w1 = __builtin_bswap64(p[1]);
    w2 = __builtin_bswap64(p[2]);
  }
  __device__ inline bool less(const FindArgs& a, uint64_t i) const
  {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(a.keys + 24 * i);
    const uint64_t k0 = __builtin_bswap64(p[0]), k1 = __builtin_bswap64(p[1]), k2 = __builtin_bswap64(p[2]);
    return k0 < w0 || (k0 == w0 && (k1 < w1 || (k1 == w1 && k2 < w2)));
  }
  __device__ inline bool equal(const FindArgs& a, uint64_t i) const
  {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(a.keys + 24 * i);
    return __builtin_bswap64(p[0]) == w0 && __builtin_bswap64(p[1]) == w1 && __builtin_bswap64(p[2]) == w2;
  }
};

template <>
struct FindQuery<kFindAny> {
  const uint8_t* p;
  uint32_t len;
  __device__ inline FindQuery(const FindArgs& a, uint64_t i)
  {
    if (a.qoffs) {
      const uint64_t b = a.qoffs[i];
      p = a.q + b;
      len = (uint32_t)(a.qoffs[i + 1] - b);
    } else {
      p = a.q + i * a.qstride;
      len = a.qstride;
    }
  }
  __device__ inline int compare(const FindArgs& a, uint64_t i) const
  {
    const uint8_t* k;
    uint32_t klen;
    if (a.koffs) {
      const uint64_t b = a.koffs[i];
      k = a.keys + b;
      klen = (uint32_t)(a.koffs[i + 1] - b);
    } else {
      k = a.keys + i * a.kstride;
      klen = a.kstride;
    }
    return key_compare(k, klen, p, len);
  }
  __device__ inline bool less(const FindArgs& a, uint64_t i) const { return compare(a, i) < 0; }
  __device__ inline bool equal(const FindArgs& a, uint64_t i) const { return compare(a, i) == 0; }
};

// keys [b, e) of leaf `leaf` (< n_segs): both ends clamped to n_keys, end < begin reads as empty
__device__ inline void leaf_range(const FindArgs& a, uint32_t leaf, uint64_t& b, uint64_t& e)
{
  if (a.key_begin) {
    b = a.key_begin[leaf];
    e = a.key_begin[leaf + 1];
  } else {
    b = a.segs[leaf].key_begin;
    e = b + a.segs[leaf].n_keys;
    if (e < b) e = ~0ull;
  }
  b = b < a.n_keys ? b : a.n_keys;
  e = e < a.n_keys ? e : a.n_keys;
  if (e < b) e = b;
}

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
      const FindQuery<MODE> q(a, i);
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
            leaf_range(a, leaf, b, e);
            // branch-free lower bound: lanes with leaves of equal size take the same trip count
            uint64_t len = e - b;
            while (len > 1) {
              const uint64_t half = len >> 1;
              b += q.less(a, b + half - 1) ? half : 0;
              len -= half;
            }
            if (len == 1) b += q.less(a, b) ? 1 : 0;
            const bool hit = b < e && q.equal(a, b);
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
  a.id_off = kind == TKV_AMQ_BLOOM ? 16u : 8u;
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
  // the fast modes, chosen as the build chooses them
  const bool fixed = !query_offsets && !leaf_key_offsets && query_stride == leaf_key_stride;
  const uintptr_t both = reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(leaf_keys);
  const int mode = fixed && query_stride == 16 && !(both & 15) ? kFind16
                   : fixed && query_stride == 24 && !(both & 7) ? kFind24
                                                                : kFindAny;
  const uint64_t wgs = (n_queries + kFindThreads - 1) / kFindThreads;
  const dim3 grid((uint32_t)(wgs < kFindMaxGrid ? wgs : kFindMaxGrid)), block(kFindThreads);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == kFind16) hipLaunchKernelGGL(find_keys_kernel<kFind16>, grid, block, 0, s, a);
  else if (mode == kFind24) hipLaunchKernelGGL(find_keys_kernel<kFind24>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(find_keys_kernel<kFindAny>, grid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

}  // extern "C"
