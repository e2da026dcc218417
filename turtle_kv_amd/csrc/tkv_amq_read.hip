// tkv_amq_read.hip -- the read side over built filters: the pair probes, the path probe and the
// point lookups, with their C entry points.  (tkv_amq_find.hip, tkv_amq_walk.hip and
// tkv_amq_open_scan.hip are the other read-side units; the membership audit, tkv_amq_verify.h, is
// compiled with the builds.)
//
//   bloom_probe / vqf_probe      one lane per (query, leaf) pair: tkv_amq_probe[_ex] (DESIGN.md
//                                sections 4 and 5)
//   vqf_hash_kernel + vqf_probe_hashed, bloom_hash_kernel + bloom_probe_hashed
//                                each query hashed once for many leaves: tkv_amq_vqf_hash,
//                                tkv_amq_bloom_hash, tkv_amq_*_probe_hashed[_ex]
//   path_probe_kernel, scan_totals<u32> (tkv_amq_scan.h), path_scatter
//                                one lane per query walks its CSR list of leaves and the surviving
//                                leaves are compacted: tkv_amq_path_probe (section 11)
//   get_keys_kernel              descent, filter tests and leaf searches in one lane:
//                                tkv_amq_get_keys (section 16)
//   get_values_kernel, gather_values_kernel
//                                the same descent with find_key's value rule, and the values'
//                                bytes: tkv_amq_get_values, tkv_amq_gather_values (section 17)
//
// The filter tests themselves (one per kind, shared with the membership audit) are in
// tkv_amq_probe.h, the hashers in tkv_amq_hash.h, the descent in tkv_amq_tree_walk.h.
#include <hip/hip_runtime.h>

#include <type_traits>

#include <stdint.h>

#include "tkv_amq.h"
#include "tkv_amq_device.h"
#include "tkv_amq_hash.h"
#include "tkv_amq_launch.h"
#include "tkv_amq_probe.h"
#include "tkv_amq_scan.h"
#include "tkv_amq_tree_walk.h"
#include "tkv_amq_value.h"

namespace tkv {

// ---------------------------------------------------------------------------------------
// Pair probes: one lane per (query, leaf)
// ---------------------------------------------------------------------------------------
// kOpts = false: one lane per query (the plain probe).  kOpts = true (tkv_amq_probe_ex): a
// grid-stride loop over a bounded grid with the page-id check and the metrics tallies.
template <int MODE, bool kOpts>
__global__ __launch_bounds__(256) void bloom_probe(const uint8_t* __restrict__ filters,
                                                   const tkv_amq_segment* __restrict__ segs, uint32_t n_segs,
                                                   const uint8_t* __restrict__ q,
                                                   const uint64_t* __restrict__ qoffs,
                                                   uint32_t stride, uint64_t n,
                                                   const uint32_t* __restrict__ qseg,
                                                   uint8_t* __restrict__ result, tkv_amq_probe_opts opts)
{
  __shared__ uint4 s_blk[256 * kProbeSlotWords / 4];
  uint4* slot = s_blk + threadIdx.x * (kProbeSlotWords / 4);
  if constexpr (!kOpts) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = bloom_probe_item<MODE, false>(filters, segs, n_segs, q, qoffs, stride, i,
                                                     __builtin_nontemporal_load(qseg + i), slot, nullptr);
    __builtin_nontemporal_store((uint8_t)(r & 1u), result + i);
  } else {
    ProbeTally t;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
      const uint32_t r = bloom_probe_item<MODE, true>(filters, segs, n_segs, q, qoffs, stride, i,
                                                      qseg[i], slot, opts.d_query_page_id);
      result[i] = (uint8_t)(r & 1u);
      t.add(r, opts.d_truth, i);
    }
    flush_tally(t, opts.d_metrics, opts.d_truth != nullptr);
  }
}

template <int MODE, bool kOpts>
__global__ __launch_bounds__(256) void vqf_probe(const uint8_t* __restrict__ filters,
                                                 const tkv_amq_segment* __restrict__ segs, uint32_t n_segs,
                                                 const uint8_t* __restrict__ q,
                                                 const uint64_t* __restrict__ qoffs, uint32_t stride,
                                                 uint64_t n, const uint32_t* __restrict__ qseg,
                                                 uint8_t* __restrict__ result, tkv_amq_probe_opts opts)
{
  if constexpr (!kOpts) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = vqf_query_hash<MODE>(q, qoffs, stride, i);
    __builtin_nontemporal_store(
        (uint8_t)(vqf_probe_one<false>(filters, segs, n_segs, __builtin_nontemporal_load(qseg + i), h) & 1u),
        result + i);
  } else {
    ProbeTally t;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
      const uint32_t r = vqf_probe_one<true>(filters, segs, n_segs, qseg[i],
                                             vqf_query_hash<MODE>(q, qoffs, stride, i), opts.d_query_page_id, i);
      result[i] = (uint8_t)(r & 1u);
      t.add(r, opts.d_truth, i);
    }
    flush_tally(t, opts.d_metrics, opts.d_truth != nullptr);
  }
}

template <bool kOpts>
__global__ __launch_bounds__(256) void vqf_probe_hashed(const uint8_t* __restrict__ filters,
                                                        const tkv_amq_segment* __restrict__ segs, uint32_t n_segs,
                                                        const uint64_t* __restrict__ hashes,
                                                        const uint32_t* __restrict__ pair_query,
                                                        uint64_t n, const uint32_t* __restrict__ qseg,
                                                        uint8_t* __restrict__ result, tkv_amq_probe_opts opts)
{
  ProbeTally t;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t qi = pair_query ? pair_query[i] : i;
    const uint32_t r = vqf_probe_one<kOpts>(filters, segs, n_segs, qseg[i], hashes[qi],
                                            opts.d_query_page_id, i);
    result[i] = (uint8_t)(r & 1u);
    if constexpr (kOpts) t.add(r, opts.d_truth, i);
    else break;
  }
  if constexpr (kOpts) flush_tally(t, opts.d_metrics, opts.d_truth != nullptr);
}

// ---- Bloom query hash cache (BloomFilterQuery<KeyView>) ----
__host__ __device__ inline uint32_t bloom_query_stride(uint32_t k_max)
{
  return (8 + 2 * (k_max > 1 ? k_max - 1 : 0) + 15) & ~15u;
}

template <int MODE>
__global__ __launch_bounds__(256) void bloom_hash_kernel(const uint8_t* __restrict__ q,
                                                         const uint64_t* __restrict__ qoffs,
                                                         uint32_t stride, uint64_t n, uint32_t k_max,
                                                         uint8_t* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint8_t* rec = out + i * bloom_query_stride(k_max);
  uint16_t* bits = reinterpret_cast<uint16_t*>(rec + 8);
  if constexpr (MODE == kKey16) {
    const Bloom16 x(load_nt16(q + 16 * i));
    *reinterpret_cast<uint64_t*>(rec) = x.h0();
    for (uint32_t j = 1; j < k_max; ++j) bits[j - 1] = (uint16_t)(x.bit(j) & kBloomBitMask);
  } else {
    uint32_t len;
    const uint8_t* p = key_at<MODE>(q, qoffs, stride, i, len);
    if (len < 32) {
      const BloomShort x(p, len);
      *reinterpret_cast<uint64_t*>(rec) = x.h0();
      for (uint32_t j = 1; j < k_max; ++j) bits[j - 1] = (uint16_t)(x.bit(j) & kBloomBitMask);
    } else {
      const BloomLong x{p, len};
      *reinterpret_cast<uint64_t*>(rec) = x.h0();
      for (uint32_t j = 1; j < k_max; ++j) bits[j - 1] = (uint16_t)(x.bit(j) & kBloomBitMask);
    }
  }
}

template <bool kOpts>
__global__ __launch_bounds__(256) void bloom_probe_hashed(const uint8_t* __restrict__ filters,
                                                          const tkv_amq_segment* __restrict__ segs, uint32_t n_segs,
                                                          const uint8_t* __restrict__ qrec,
                                                          uint32_t k_max,
                                                          const uint32_t* __restrict__ pair_query,
                                                          uint64_t n, const uint32_t* __restrict__ qseg,
                                                          uint8_t* __restrict__ result, tkv_amq_probe_opts opts)
{
  __shared__ uint4 s_blk[256 * kProbeSlotWords / 4];
  uint4* slot = s_blk + threadIdx.x * (kProbeSlotWords / 4);
  const uint32_t* slot32 = reinterpret_cast<const uint32_t*>(slot);
  ProbeTally t;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    // qseg[i] and pair_query[i], then the descriptor and the query record, are independent
    // loads issued side by side; only the block load waits for both
    const uint32_t sidx = qseg[i];
    const uint64_t qi = pair_query ? pair_query[i] : i;
    const uint8_t* rec = qrec + qi * bloom_query_stride(k_max);
    const ProbeDesc d = load_probe_desc(segs, sidx, n_segs);
    const uint64_t h0 = *reinterpret_cast<const uint64_t*>(rec);
    uint32_t r;
    // a filter whose hash_count exceeds the cached k_max cannot be tested: cannot reject
    if (d.hash_count == 0 || d.hash_count > k_max) {
      r = 1u | (kNoFilter << 1);
    } else if (kOpts && !page_id_matches(filters + d.out_offset, src_page_id_offset(TKV_AMQ_BLOOM), opts.d_query_page_id, i)) {
      r = 1u | (kIdMismatch << 1);
    } else {
      const uint16_t* bits = reinterpret_cast<const uint16_t*>(rec + 8);
      const uint4* blk = reinterpret_cast<const uint4*>(filters + d.out_offset + kBloomHeader +
                                                        64 * bloom_block(h0, d.n_blocks));
      const uint4 b0 = blk[0], b1 = blk[1], b2 = blk[2], b3 = blk[3];
      slot[0] = b0;
      slot[1] = b1;
      slot[2] = b2;
      slot[3] = b3;
      uint32_t bit = (uint32_t)h0 & kBloomBitMask;
      uint32_t ok = slot32[bit >> 5] >> (bit & 31);
      for (uint32_t j = 1; j < d.hash_count; ++j) {
        bit = bits[j - 1];  // (cached masked)
        ok &= slot32[bit >> 5] >> (bit & 31);
      }
      r = (ok & 1u) | (kChecked << 1);
    }
    result[i] = (uint8_t)(r & 1u);
    if constexpr (kOpts) t.add(r, opts.d_truth, i);
    else break;
  }
  if constexpr (kOpts) flush_tally(t, opts.d_metrics, opts.d_truth != nullptr);
}

template <int MODE>
__global__ __launch_bounds__(256) void vqf_hash_kernel(const uint8_t* __restrict__ q,
                                                       const uint64_t* __restrict__ qoffs,
                                                       uint32_t stride, uint64_t n,
                                                       uint64_t* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if constexpr (MODE == kKey16) {
    const uint4 kv = reinterpret_cast<const uint4*>(q)[i];
    const Xxh16 x((uint64_t)kv.x | ((uint64_t)kv.y << 32), (uint64_t)kv.z | ((uint64_t)kv.w << 32));
    out[i] = x.finish(xxh16_rhinit(kVqfHashSeed));
  } else {
    out[i] = hash_key<MODE>(q, qoffs, stride, i, kVqfHashSeed);
  }
}

// ---------------------------------------------------------------------------------------
// Path probe (tkv_amq_path_probe): one lane per query walks its CSR list of leaves
// ---------------------------------------------------------------------------------------
// Three launches, no atomics on an output position:
//   path_probe_kernel   lane i hashes query i once (the seed-independent rounds stay in
//                       registers), tests the filter of every entry of its path, keeps the
//                       answers of its first kPathMaskEntries entries as a bit mask (later
//                       entries only as bytes), and counts its candidates; the workgroup scans
//                       its 256 counts (block_exclusive_scan): cand_begin[i] <- prefix inside the workgroup,
//                       wg_total[w] <- the workgroup's sum
//   scan_totals<u32>    (tkv_amq_scan.h) one workgroup: exclusive scan of wg_total in passes of
//                       kScanTotalsSpan; cand_begin[n_queries] <- the total, at most n_entries
//                       (more candidates than entries: only paths that share entries)
//   path_scatter        lane i again: cand_begin[i] += wg_total[w], then its candidates in path
//                       order from the mask (answer bytes past kPathMaskEntries)
// The mask is the query's own, so two paths that share entries (possible only when path_begin
// is not monotone) cannot disturb each other's candidates.
constexpr uint32_t kPathMaskEntries = 32;

struct PathArgs {
  const uint8_t* filters;
  const tkv_amq_segment* segs;
  uint32_t n_segs;
  const uint8_t* q;
  const uint64_t* qoffs;
  uint32_t stride;
  uint32_t n_queries;
  const uint32_t* path_begin;
  const uint32_t* path_leaf;
  uint32_t n_entries;
  uint32_t every_answer;  // 1: `answers` is the caller's d_entry_result, every entry is written
  uint8_t* answers;       // d_entry_result, or the workspace's bytes for entries past the mask
  uint32_t* mask;         // workspace: [n_queries]
  uint32_t* wg_total;     // workspace: [n_wgs]
  uint32_t* cand_begin;
  uint32_t* cand_leaf;
  uint32_t* cand_entry;
  uint32_t n_wgs;
};

// entries [b, e) of query i: both ends clamped to n_entries, end < begin reads as empty
__device__ inline void path_range(const PathArgs& a, uint64_t i, uint32_t& b, uint32_t& e)
{
  b = min(a.path_begin[i], a.n_entries);
  e = min(a.path_begin[i + 1], a.n_entries);
  if (e < b) e = b;
}

// one lane's walk: its answers so far
struct PathWalk {
  uint32_t mask = 0;
  uint32_t cnt = 0;
  template <bool kOpts>
  __device__ inline void record(const PathArgs& a, const tkv_amq_probe_opts& opts, ProbeTally& t,
                                uint32_t r, uint32_t j, uint32_t ent)
  {
    const uint32_t bit = r & 1u;
    if (j < kPathMaskEntries) mask |= bit << j;
    if (a.every_answer || j >= kPathMaskEntries) a.answers[ent] = (uint8_t)bit;
    cnt += bit;
    if constexpr (kOpts) t.add(r, opts.d_truth, ent);
  }
};

// Occupancy: the plain 16-byte-key forms ask for 8 waves per SIMD (64 VGPRs), what the pair
// probes run at.  VQF meets it (57 VGPRs); Bloom stops at 66 VGPRs, 7 waves (the block's 16
// registers beside the unpacked indices): DESIGN.md section 11.  The forms with options do
// not ask (held to 64 VGPRs, the VQF one spilled five registers to scratch).  Independent
// random lines in flight come from the waves, as in the pair probes.
template <int KIND, int MODE, bool kOpts>
__global__ __launch_bounds__(256, (MODE == kKey16 && !kOpts ? 8 : 4)) void path_probe_kernel(
    PathArgs a, tkv_amq_probe_opts opts)
{
  // Bloom: the lane's block slot (16-byte keys) or its cache of bit indices (keys of 32 bytes
  // and more, whose XXH64 has no seed-independent part)
  __shared__ uint4 s_blk[KIND == TKV_AMQ_BLOOM ? 256 * kProbeSlotWords / 4 : 1];
  __shared__ uint32_t s_scan[4];
  const uint32_t tid = threadIdx.x;
  uint4* slot = s_blk + (KIND == TKV_AMQ_BLOOM ? tid * (kProbeSlotWords / 4) : 0u);
  ProbeTally t;
  // without options the grid has one workgroup per 256 queries (no loop: the scan's addresses
  // would be kept in registers across it); with options it is bounded and strides
  uint32_t w = blockIdx.x;
  do {
    const uint64_t i = (uint64_t)w * 256 + tid;
    const bool live = i < a.n_queries;
    uint32_t b = 0, e = 0;
    if (live) path_range(a, i, b, e);
    PathWalk wk;
    if (b < e) {
      // the next entry's leaf index (Bloom, 16-byte keys: its descriptor too) is read while
      // this entry is tested
      uint32_t leaf = a.path_leaf[b];
      if constexpr (KIND == TKV_AMQ_VQF) {
        const uint64_t h = vqf_query_hash<MODE>(a.q, a.qoffs, a.stride, i);
        for (uint32_t ent = b; ent < e; ++ent) {
          const uint32_t leaf1 = ent + 1 < e ? a.path_leaf[ent + 1] : 0u;
          const uint32_t r = vqf_probe_one<kOpts>(a.filters, a.segs, a.n_segs, leaf, h,
                                                  opts.d_query_page_id, ent);
          wk.record<kOpts>(a, opts, t, r, ent - b, ent);
          leaf = leaf1;
        }
      } else if constexpr (MODE == kKey16) {
        const uint4 kv = load_nt16(a.q + 16 * i);
        const Bloom16 x(kv);
        const uint64_t h0 = x.h0();
        const BloomBits16 bits(x);
        bloom_entry16_park(x, slot);
        BloomEntry16 cur = bloom_entry16_fetch<kOpts>(a.filters, a.segs, a.n_segs, leaf, h0,
                                                      opts.d_query_page_id, b);
        for (uint32_t ent = b; ent < e; ++ent) {
          BloomEntry16 nxt = cur;
          if (ent + 1 < e)
            nxt = bloom_entry16_fetch<kOpts>(a.filters, a.segs, a.n_segs, a.path_leaf[ent + 1], h0,
                                             opts.d_query_page_id, ent + 1);
          const uint32_t r = bloom_entry16_test(h0, bits, cur, slot);
          wk.record<kOpts>(a, opts, t, r, ent - b, ent);
          cur = nxt;
        }
      } else {
        with_bloom_key_at<MODE>(a.q, a.qoffs, a.stride, i, [&](const auto& x) {
          const uint64_t h0 = x.h0();
          BloomBitSource<std::decay_t<decltype(x)>> bit_of{x, reinterpret_cast<uint16_t*>(slot)};
          for (uint32_t ent = b; ent < e; ++ent) {
            const uint32_t leaf1 = ent + 1 < e ? a.path_leaf[ent + 1] : 0u;
            const uint32_t r = bloom_entry_test<kOpts>(a.filters, a.segs, a.n_segs, leaf, h0,
                                                       opts.d_query_page_id, ent, bit_of);
            wk.record<kOpts>(a, opts, t, r, ent - b, ent);
            leaf = leaf1;
          }
        });
      }
    }
    if (live) a.mask[i] = wk.mask;
    uint32_t total;
    const uint32_t pre = block_exclusive_scan<uint32_t>(wk.cnt, s_scan, &total);
    if (live) a.cand_begin[i] = pre;
    if (tid == 0) a.wg_total[w] = total;
    w += gridDim.x;
  } while (kOpts && w < a.n_wgs);
  if constexpr (kOpts) flush_tally(t, opts.d_metrics, opts.d_truth != nullptr);
}

// Lane i writes query i's candidates in path order.  Positions at or past n_entries (the
// capacity) can come up only when paths share entries; those candidates are dropped and the
// offsets stop at n_entries, so nothing is written out of range.
__global__ __launch_bounds__(256) void path_scatter(PathArgs a)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_queries) return;
  uint32_t b, e;
  path_range(a, i, b, e);
  uint32_t pos = a.cand_begin[i] + a.wg_total[blockIdx.x];
  a.cand_begin[i] = min(pos, a.n_entries);
  uint32_t m = a.mask[i];
  while (m) {
    const uint32_t j = (uint32_t)__builtin_ctz(m);
    m &= m - 1;
    if (pos < a.n_entries) {
      a.cand_leaf[pos] = a.path_leaf[b + j];
      if (a.cand_entry) a.cand_entry[pos] = b + j;
    }
    ++pos;
  }
  if (e - b > kPathMaskEntries) {
    for (uint32_t ent = b + kPathMaskEntries; ent < e; ++ent) {
      if (a.answers[ent] == 0) continue;
      if (pos < a.n_entries) {
        a.cand_leaf[pos] = a.path_leaf[ent];
        if (a.cand_entry) a.cand_entry[pos] = ent;
      }
      ++pos;
    }
  }
}

// ---------------------------------------------------------------------------------------
// Fused point lookup (tkv_amq_get_keys): descent, filter tests and leaf searches in one lane
// ---------------------------------------------------------------------------------------
// One lane per query (workgroup tiles of 256, a bounded grid striding over them).  The lane runs
// the reference's find_key (tree/algo/nodes.hpp:158-187) as the reference orders it: walk_tree
// names the entries; each entry is one filter test with the path probe's helpers and, if the
// filter says maybe, one lower bound over the leaf's keys (find_keys_kernel's); the entry's answer
// steers the descent: FOUND ends the lookup, found below the segment's flushed item upper bound
// leaves the level (tree/algo/segments.hpp:166-206), anything else goes on.  No path is written
// and nothing below a hit is visited.  The key is hashed once, before the descent; the ordered
// form of the query (OrderedQuery) serves the pivots and the leaves.
constexpr uint32_t kGetThreads = 256;
// the tile loop's workgroups at most: one round of a full machine (256 CUs x 8 workgroups), as the
// walk's (tests/test_gpu_get.py sizes the batch that needs a second round from it)
constexpr uint32_t kGetMaxGrid = 2048;

struct GetArgs : TreeArgs {
  const uint8_t* filters;
  const tkv_amq_segment* segs_plan;
  uint32_t n_plan;
  uint32_t check_id;
  const uint8_t* q;
  const uint64_t* qoffs;
  uint32_t qstride;
  uint32_t n_queries;
  const uint8_t* keys;
  const uint64_t* koffs;
  uint32_t kstride;
  uint32_t n_tiles;
  uint64_t n_keys;
  const uint64_t* key_begin;
  tkv_amq_get_result* result;
  uint32_t* visits;
  tkv_amq_probe_metrics* metrics;
  tkv_amq_get_counts* counts;
};

// One lane's counts.  Two are not kept, they follow from the others once the wave has summed
// them: a visit is rejected unless it is one of the other three classes, and a visit that
// answered "maybe" and is not unsearchable, found or flushed was absent.
// what a visit came to
enum GetOutcome : uint32_t { kGetRejected = 0, kGetUnsearchable, kGetAbsent, kGetFlushed, kGetFound };

struct GetTally {
  uint32_t total = 0, no_filter = 0, mismatch = 0, positive = 0, false_pos = 0;
  uint32_t found = 0, unsearchable = 0, flushed = 0;
  // r: result bit | class << 1.  One add per counter, no branch: spelled as increments on the
  // visit's branches the compiler merged them into one increment through a pointer, and the tally
  // lived in scratch.
  __device__ inline void add(uint32_t r, uint32_t outcome)
  {
    const uint32_t cls = r >> 1;
    no_filter += cls == kNoFilter;
    mismatch += cls == kIdMismatch;
    positive += r == (1u | (kChecked << 1));
    false_pos += (cls == kChecked) & (outcome == kGetAbsent);
    found += outcome == kGetFound;
    unsearchable += outcome == kGetUnsearchable;
    flushed += outcome == kGetFlushed;
  }
};

__device__ inline void flush_get_tally(const GetTally& t, tkv_amq_probe_metrics* m, tkv_amq_get_counts* c)
{
  const uint32_t total = wave_sum(t.total), no_filter = wave_sum(t.no_filter), mismatch = wave_sum(t.mismatch),
                 positive = wave_sum(t.positive), false_pos = wave_sum(t.false_pos), found = wave_sum(t.found),
                 unsearchable = wave_sum(t.unsearchable), flushed = wave_sum(t.flushed);
  if (__lane_id() != 0) return;
  const uint32_t maybe = no_filter + mismatch + positive;
  const uint32_t absent = maybe - unsearchable - found - flushed;
  // one atomic per non-zero counter per wave
  if (m) {
    const uint32_t v[6] = {total, no_filter, mismatch, total - maybe, positive, false_pos};
    unsigned long long* d = reinterpret_cast<unsigned long long*>(m);
#pragma unroll
    for (int j = 0; j < 6; ++j)
      if (v[j]) atomicAdd(&d[j], (unsigned long long)v[j]);
  }
  if (c) {
    const uint32_t v[6] = {total, maybe - unsearchable, found, absent, unsearchable, flushed};
    unsigned long long* d = reinterpret_cast<unsigned long long*>(c);
#pragma unroll
    for (int j = 0; j < 6; ++j)
      if (v[j]) atomicAdd(&d[j], (unsigned long long)v[j]);
  }
}

// What a lookup does with a found item is its Rule.  tkv_amq_get_keys': the first item found is
// the result and ends the lookup; nothing is folded.  (GetValuesRule, below, folds: its take() folds
// the item into the rule's state and says whether it is the lookup's first, step() is what the
// descent does after it, write() stores the query's result.)
struct GetKeysRule {
  using Args = GetArgs;
  using Tally = GetTally;
  static constexpr bool kFolds = false;
};

// The descent of query i with test(leaf, page id) -> result bit | class << 1 as its filter test.
template <int ORDER, typename Rule = GetKeysRule, typename Test>
__device__ inline void get_one(const typename Rule::Args& a, uint64_t i, typename Rule::Tally& t, Test&& test)
{
  const OrderedQuery<ORDER> q(KeyArray{a.q, a.qoffs, a.qstride}, i);
  const KeyArray ks{a.keys, a.koffs, a.kstride};
  uint64_t r_key = ~0ull;
  uint32_t r_leaf = ~0u, r_where = ~0u, n_visits = 0;
  [[maybe_unused]] Rule rule;
  // (always inlined, at both of its sites: as a function it would hold the lookup's state on the
  // stack.  The child leaf's site is where the lanes of a level tree meet again, so the second
  // copy costs code and no divergence.)
  auto visit = [&](uint32_t leaf, uint64_t page_id, uint32_t flushed_bound, uint32_t where)
                   __attribute__((always_inline)) {
    ++n_visits;
    // (a leaf outside the plan is "no filter", as load_probe_desc reads it: no segment is loaded)
    const bool in_plan = leaf < a.n_plan;
    const uint32_t r = in_plan ? test(leaf, PageIdIs{page_id, a.check_id != 0}) : 1u | (kNoFilter << 1);
    uint32_t outcome = kGetRejected;
    if (r & 1u) {
      outcome = kGetUnsearchable;
      if (in_plan) {
        uint64_t b0, e;
        leaf_key_range(a.key_begin, a.segs_plan, leaf, a.n_keys, b0, e);
        // the lower bound: lanes with leaves of equal size take the same trip count
        const uint64_t b = bound(b0, e - b0, [&](uint64_t k) { return q.less(ks, k); });
        outcome = kGetAbsent;
        if (b < e && q.equal(ks, b)) {
          // below the bound the item "has been flushed from this segment": the level is left
          outcome = b - b0 < flushed_bound ? kGetFlushed : kGetFound;
          if constexpr (Rule::kFolds) {
            if (outcome == kGetFound && rule.take(a, t, b, where)) {
              r_key = b;
              r_leaf = leaf;
              r_where = where;
            }
          } else {
            if (outcome == kGetFound) {
              r_key = b;
              r_leaf = leaf;
              r_where = where;
            }
          }
        }
      }
    }
    t.add(r, outcome);
    if constexpr (Rule::kFolds)
      return outcome == kGetFound ? rule.step() : outcome == kGetFlushed ? kWalkLeaveLevel : kWalkContinue;
    else
      return outcome == kGetFound ? kWalkStop : outcome == kGetFlushed ? kWalkLeaveLevel : kWalkContinue;
  };
  walk_tree(
      a, [&](uint32_t, uint32_t key_begin, uint32_t pivot_count) { return find_pivot<ORDER>(a, q, key_begin, pivot_count); },
      [&](uint32_t s, uint32_t p, uint32_t where) {
        uint32_t leaf, flushed_bound;
        uint64_t page_id;
        segment_entry(a, s, p, true, leaf, page_id, flushed_bound);
        return visit(leaf, page_id, flushed_bound, where);
      },
      [&](uint32_t index, uint64_t page_id, uint32_t where) { visit(index, page_id, 0u, where); });
  t.total += n_visits;
  if constexpr (Rule::kFolds)
    rule.write(a, i, t, r_key, r_leaf, r_where);
  else
    *reinterpret_cast<ulonglong2*>(a.result + i) = ulonglong2{r_key, mk64(r_leaf, r_where)};
  if (a.visits) a.visits[i] = n_visits;
}

// ORDER: the key order's mode over the three key sides (tkv_amq_key_order.h); HASH: the hash's
// mode of the query side, as the path probe chooses it.
template <int KIND, int ORDER, int HASH, typename Rule = GetKeysRule>
__device__ inline void get_keys_tiles(const typename Rule::Args& a)
{
  // Bloom: the lane's block slot (16-byte keys) or its cache of bit indices (32 bytes and more)
  __shared__ uint4 s_blk[KIND == TKV_AMQ_BLOOM ? kGetThreads * kProbeSlotWords / 4 : 1];
  uint4* slot = s_blk + (KIND == TKV_AMQ_BLOOM ? threadIdx.x * (kProbeSlotWords / 4) : 0u);
  typename Rule::Tally t;
  for (uint32_t w = blockIdx.x; w < a.n_tiles; w += gridDim.x) {
    const uint64_t i = (uint64_t)w * kGetThreads + threadIdx.x;
    if (i >= a.n_queries) continue;
    if constexpr (KIND == TKV_AMQ_VQF) {
      const uint64_t h = vqf_query_hash<HASH>(a.q, a.qoffs, a.qstride, i);
      get_one<ORDER, Rule>(a, i, t, [&](uint32_t leaf, const PageIdIs& id) {
        return vqf_probe_one<true>(a.filters, a.segs_plan, a.n_plan, leaf, h, id);
      });
    } else if constexpr (HASH == kKey16) {
      const uint4 kv = load_nt16(a.q + 16 * i);
      const Bloom16 x(kv);
      const uint64_t h0 = x.h0();
      const BloomBits16 bits(x);
      bloom_entry16_park(x, slot);
      get_one<ORDER, Rule>(a, i, t, [&](uint32_t leaf, const PageIdIs& id) {
        return bloom_entry16_test(h0, bits, bloom_entry16_fetch<true>(a.filters, a.segs_plan, a.n_plan, leaf, h0, id, 0u), slot);
      });
    } else {
      with_bloom_key_at<HASH>(a.q, a.qoffs, a.qstride, i, [&](const auto& x) {
        const uint64_t h0 = x.h0();
        BloomBitSource<std::decay_t<decltype(x)>> bit_of{x, reinterpret_cast<uint16_t*>(slot)};
        get_one<ORDER, Rule>(a, i, t, [&](uint32_t leaf, const PageIdIs& id) {
          return bloom_entry_test<true>(a.filters, a.segs_plan, a.n_plan, leaf, h0, id, 0u, bit_of);
        });
      });
    }
  }
  if constexpr (Rule::kFolds)
    flush_value_tally(t, a.metrics, a.vcounts);
  else
    flush_get_tally(t, a.metrics, a.counts);
}

// Occupancy: every step of a lookup is a dependent read, so the throughput comes from waves in
// flight, and the lane holds the hash state, the ordered query, the descent and eight tallies:
// 96-140 VGPRs, 3-5 waves per SIMD, no scratch.  No form asks for more
// waves: the compiler would meet the request by spilling registers to scratch.
template <int KIND, int ORDER, int HASH>
__global__ __launch_bounds__(kGetThreads) void get_keys_kernel(GetArgs a)
{
  get_keys_tiles<KIND, ORDER, HASH>(a);
}

// ---------------------------------------------------------------------------------------
// Point lookup with values (tkv_amq_get_values): the same descent with find_key's value rule
// ---------------------------------------------------------------------------------------
// The visit is get_keys' (get_one, with GetValuesRule as its Rule); what differs is what FOUND does: the item's packed value
// (op byte, data) is folded into the lane's value as combine_in_place folds it
// (core/value_view.hpp:316-361) and the descent goes on while an ADD_I32 is pending.
struct ValueArgs : GetArgs {
  ValueArray v;
  tkv_amq_value_result* vresult;
  tkv_amq_value_counts* vcounts;
};

struct ValueTally : GetTally {
  uint32_t valued = 0, bad = 0;  // (GetTally::found counts the items taken)
};

__device__ inline void flush_value_tally(const ValueTally& t, tkv_amq_probe_metrics* m, tkv_amq_value_counts* c)
{
  const uint32_t total = wave_sum(t.total), no_filter = wave_sum(t.no_filter), mismatch = wave_sum(t.mismatch),
                 positive = wave_sum(t.positive), false_pos = wave_sum(t.false_pos), items = wave_sum(t.found),
                 unsearchable = wave_sum(t.unsearchable), flushed = wave_sum(t.flushed),
                 valued = wave_sum(t.valued), bad = wave_sum(t.bad);
  if (__lane_id() != 0) return;
  const uint32_t maybe = no_filter + mismatch + positive;
  const uint32_t absent = maybe - unsearchable - items - flushed;
  // one atomic per non-zero counter per wave
  if (m) {
    const uint32_t v[6] = {total, no_filter, mismatch, total - maybe, positive, false_pos};
    unsigned long long* d = reinterpret_cast<unsigned long long*>(m);
#pragma unroll
    for (int j = 0; j < 6; ++j)
      if (v[j]) atomicAdd(&d[j], (unsigned long long)v[j]);
  }
  if (c) {
    const uint32_t v[8] = {total, maybe - unsearchable, valued, absent, unsearchable, flushed, items, bad};
    unsigned long long* d = reinterpret_cast<unsigned long long*>(c);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (v[j]) atomicAdd(&d[j], (unsigned long long)v[j]);
  }
}

// tkv_amq_get_values' rule: the lane's value -- its op, the accumulator of a pending or resolved ADD,
// flags, the items taken, the last one's index and depth (a bad combination on a node's first item is
// the node's whole answer) -- and the step the last fold chose.
struct GetValuesRule {
  using Args = ValueArgs;
  using Tally = ValueTally;
  static constexpr bool kFolds = true;
  uint64_t r_last = ~0ull;
  uint32_t op = TKV_AMQ_OP_NONE, acc = 0, flags = 0, n_items = 0, last_depth = ~0u;
  WalkStep next = kWalkStop;
  // folds item b, found at `where`; true if it is the lookup's first (the result's key_index)
  __device__ inline bool take(const Args& a, Tally& t, uint64_t b, uint32_t where)
  {
    uint64_t vb, ve;
    value_range(a.v, b, vb, ve);
    const uint32_t item_op = ve > vb ? a.v.values[vb] : TKV_AMQ_OP_NOOP;  // (an empty value is a NOOP)
    const uint32_t item_i32 = ve > vb ? value_i32(a.v.values + vb + 1, ve - vb - 1) : 0u;
    const uint32_t depth = where >> 8;
    // (the child leaf is a depth of its own)
    const bool first_here = (where & 0xffu) == TKV_AMQ_WALK_LEAF_LEVEL || depth != last_depth;
    last_depth = depth;
    r_last = b;
    ++n_items;
    next = kWalkStop;
    if (n_items == 1) {
      op = item_op;
      if (item_op == TKV_AMQ_OP_ADD_I32) {
        acc = item_i32;
        next = kWalkLeaveLevel;
      }
    } else if (item_op == TKV_AMQ_OP_WRITE || item_op == TKV_AMQ_OP_DELETE) {
      // (the lookup is here only with an ADD pending)
      acc += item_op == TKV_AMQ_OP_WRITE ? item_i32 : 0u;
      op = TKV_AMQ_OP_WRITE;
      flags |= TKV_AMQ_VALUE_COMBINED;
    } else if (item_op == TKV_AMQ_OP_ADD_I32) {
      acc += item_i32;
      flags |= TKV_AMQ_VALUE_COMBINED;
      next = kWalkLeaveLevel;
    } else {
      flags |= TKV_AMQ_VALUE_BAD_COMBINE;
      ++t.bad;
      next = first_here ? kWalkStop : kWalkLeaveLevel;
    }
    return n_items == 1;
  }
  __device__ inline WalkStep step() const { return next; }
  __device__ inline void write(const Args& a, uint64_t i, Tally& t, uint64_t r_key, uint32_t r_leaf,
                               uint32_t r_where) const
  {
    t.valued += n_items != 0;
    uint4* out = reinterpret_cast<uint4*>(a.vresult + i);
    out[0] = uint4{(uint32_t)r_key, (uint32_t)(r_key >> 32), (uint32_t)r_last, (uint32_t)(r_last >> 32)};
    out[1] = uint4{r_leaf, r_where, acc, op | (flags << 8) | (min(n_items, 0xffffu) << 16)};
  }
};

// Occupancy: as get_keys_kernel, plus the value's state: no form asks for more waves, none uses
// scratch (DESIGN.md section 17 has the table).
template <int KIND, int ORDER, int HASH>
__global__ __launch_bounds__(kGetThreads) void get_values_kernel(ValueArgs a)
{
  get_keys_tiles<KIND, ORDER, HASH, GetValuesRule>(a);
}

// tkv_amq_gather_values: sixteen lanes per value, eight bytes per lane and step.  A value of the
// reference's default shape (about 100 data bytes behind an op byte, at any byte address) is one
// step: the sixteen lanes read one or two consecutive 128-byte lines and a wave writes four
// consecutive slots.  One lane per value would walk 64 distant lines per instruction; one wave per
// value would leave a third of its lanes idle at a byte each.
constexpr uint32_t kGatherLanes = 16, kGatherThreads = 256, kGatherPerBlock = kGatherThreads / kGatherLanes;

struct GatherArgs {
  const tkv_amq_value_result* result;
  uint64_t n_queries, n_keys;
  ValueArray v;
  uint8_t* out;
  uint32_t out_stride;
  uint32_t* len;
};

__global__ __launch_bounds__(kGatherThreads) void gather_values_kernel(GatherArgs a)
{
  const uint64_t i = (uint64_t)blockIdx.x * kGatherPerBlock + threadIdx.x / kGatherLanes;
  const uint32_t sub = threadIdx.x % kGatherLanes;
  if (i >= a.n_queries) return;
  const uint4* rp = reinterpret_cast<const uint4*>(a.result + i);
  const uint4 r0 = rp[0], r1 = rp[1];  // {key_index, last_index}, {leaf, where, i32, op | flags | n_items}
  const uint64_t key = mk64(r0.x, r0.y);
  const uint32_t op = r1.w & 0xffu, flags = (r1.w >> 8) & 0xffu;
  uint64_t len = 0;
  const uint8_t* src = nullptr;  // null: the record's own i32
  if (key < a.n_keys) {
    if (flags & TKV_AMQ_VALUE_COMBINED) {
      len = 4;
    } else if (op != TKV_AMQ_OP_DELETE) {
      uint64_t vb, ve;
      value_range(a.v, key, vb, ve);
      if (ve > vb) {
        len = ve - vb - 1;
        src = a.v.values + vb + 1;
      }
    }
  }
  if (sub == 0) a.len[i] = len > 0xffffffffull ? 0xffffffffu : (uint32_t)len;
  const uint32_t n = len < a.out_stride ? (uint32_t)len : a.out_stride;
  uint8_t* dst = a.out + i * a.out_stride;
  if (!src) {
    // (n <= 4: the integer, little-endian, by lane 0)
    if (sub == 0)
      for (uint32_t j = 0; j < n; ++j) dst[j] = (uint8_t)(r1.z >> (8 * j));
    return;
  }
  for (uint32_t o = 8 * sub; o < n; o += 8 * kGatherLanes) {
    if (o + 8 <= n && (reinterpret_cast<uintptr_t>(dst + o) & 7) == 0) {
      *reinterpret_cast<uint64_t*>(dst + o) = ld64_unaligned(src + o);
    } else {
      const uint32_t m = n - o < 8 ? n - o : 8;
      for (uint32_t j = 0; j < m; ++j) dst[o + j] = src[o + j];
    }
  }
}

}  // namespace tkv

// =======================================================================================
// host side: the C ABI of the probes and the lookups
// =======================================================================================
using namespace tkv;

extern "C" {

int tkv_amq_probe(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                  uint32_t n_segs, const uint8_t* q, const uint64_t* qoffs, uint32_t stride,
                  uint64_t n, const uint32_t* d_qseg, uint8_t* d_result, void* stream)
{
  return tkv_amq_probe_ex(kind, d_filters, d_segs, n_segs, q, qoffs, stride, n, d_qseg, d_result,
                          nullptr, stream);
}

int tkv_amq_probe_ex(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                     uint32_t n_segs, const uint8_t* q, const uint64_t* qoffs, uint32_t stride,
                     uint64_t n, const uint32_t* d_qseg, uint8_t* d_result,
                     const tkv_amq_probe_opts* opts, void* stream)
{
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n == 0) return TKV_AMQ_OK;
  if (!d_filters || !d_segs || !q || !d_qseg || !d_result || n_segs == 0 || (!qoffs && !stride))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (kind != TKV_AMQ_BLOOM && kind != TKV_AMQ_VQF) return TKV_AMQ_INVALID_ARGUMENT;
  const hipStream_t s = as_stream(stream);
  const int mode = key_mode(qoffs, stride);
  if (mode == kKey16 && (reinterpret_cast<uintptr_t>(q) & 15)) return TKV_AMQ_INVALID_ARGUMENT;
  const tkv_amq_probe_opts o = probe_opts(opts);
  const bool ex = probe_opts_used(o);
  const dim3 grid(probe_grid(n, ex)), block(256);
  with_key_mode(mode, [&](auto M) {
    with_flag(ex, [&](auto X) {
      constexpr int MODE = decltype(M)::value;
      constexpr bool kOpts = decltype(X)::value;
      if (kind == TKV_AMQ_BLOOM)
        hipLaunchKernelGGL((bloom_probe<MODE, kOpts>), grid, block, 0, s, d_filters, d_segs, n_segs, q, qoffs, stride, n,
                           d_qseg, d_result, o);
      else
        hipLaunchKernelGGL((vqf_probe<MODE, kOpts>), grid, block, 0, s, d_filters, d_segs, n_segs, q, qoffs, stride, n,
                           d_qseg, d_result, o);
    });
  });
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

int tkv_amq_vqf_hash(const uint8_t* q, const uint64_t* qoffs, uint32_t stride, uint64_t n,
                     uint64_t* d_hash, void* stream)
{
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n == 0) return TKV_AMQ_OK;
  if (!q || !d_hash || (!qoffs && !stride)) return TKV_AMQ_INVALID_ARGUMENT;
  const hipStream_t s = as_stream(stream);
  const int mode = key_mode(qoffs, stride);
  if (mode == kKey16 && (reinterpret_cast<uintptr_t>(q) & 15)) return TKV_AMQ_INVALID_ARGUMENT;
  const dim3 grid((uint32_t)div_up(n, 256)), block(256);
  with_key_mode(mode, [&](auto M) {
    hipLaunchKernelGGL(vqf_hash_kernel<decltype(M)::value>, grid, block, 0, s, q, qoffs, stride, n, d_hash);
  });
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

int tkv_amq_vqf_probe_hashed(const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                             uint32_t n_segs, const uint64_t* d_hash, const uint32_t* d_pair_query,
                             uint64_t n, const uint32_t* d_qseg, uint8_t* d_result, void* stream)
{
  return tkv_amq_vqf_probe_hashed_ex(d_filters, d_segs, n_segs, d_hash, d_pair_query, n, d_qseg,
                                     d_result, nullptr, stream);
}

int tkv_amq_vqf_probe_hashed_ex(const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                                uint32_t n_segs, const uint64_t* d_hash,
                                const uint32_t* d_pair_query, uint64_t n, const uint32_t* d_qseg,
                                uint8_t* d_result, const tkv_amq_probe_opts* opts, void* stream)
{
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n == 0) return TKV_AMQ_OK;
  if (!d_filters || !d_segs || !d_hash || !d_qseg || !d_result || n_segs == 0)
    return TKV_AMQ_INVALID_ARGUMENT;
  const tkv_amq_probe_opts o = probe_opts(opts);
  const bool ex = probe_opts_used(o);
  if (ex)
    hipLaunchKernelGGL(vqf_probe_hashed<true>, dim3(probe_grid(n, true)), dim3(256), 0,
                       as_stream(stream), d_filters, d_segs, n_segs, d_hash, d_pair_query, n, d_qseg,
                       d_result, o);
  else
    hipLaunchKernelGGL(vqf_probe_hashed<false>, dim3(probe_grid(n, false)), dim3(256), 0,
                       as_stream(stream), d_filters, d_segs, n_segs, d_hash, d_pair_query, n, d_qseg,
                       d_result, o);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

uint32_t tkv_amq_bloom_query_stride(uint32_t k_max) { return bloom_query_stride(k_max); }

int tkv_amq_bloom_hash(const uint8_t* q, const uint64_t* qoffs, uint32_t stride, uint64_t n,
                       uint32_t k_max, uint8_t* d_query, void* stream)
{
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n == 0) return TKV_AMQ_OK;
  if (!q || !d_query || (!qoffs && !stride) || k_max == 0 || k_max > kMaxBloomHashes)
    return TKV_AMQ_INVALID_ARGUMENT;
  const hipStream_t s = as_stream(stream);
  const int mode = key_mode(qoffs, stride);
  if (mode == kKey16 && (reinterpret_cast<uintptr_t>(q) & 15)) return TKV_AMQ_INVALID_ARGUMENT;
  const dim3 grid((uint32_t)div_up(n, 256)), block(256);
  with_key_mode(mode, [&](auto M) {
    hipLaunchKernelGGL(bloom_hash_kernel<decltype(M)::value>, grid, block, 0, s, q, qoffs, stride, n, k_max, d_query);
  });
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

int tkv_amq_bloom_probe_hashed(const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                               uint32_t n_segs, const uint8_t* d_query, uint32_t k_max,
                               const uint32_t* d_pair_query, uint64_t n, const uint32_t* d_qseg,
                               uint8_t* d_result, void* stream)
{
  return tkv_amq_bloom_probe_hashed_ex(d_filters, d_segs, n_segs, d_query, k_max, d_pair_query, n,
                                       d_qseg, d_result, nullptr, stream);
}

int tkv_amq_bloom_probe_hashed_ex(const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                                  uint32_t n_segs, const uint8_t* d_query, uint32_t k_max,
                                  const uint32_t* d_pair_query, uint64_t n, const uint32_t* d_qseg,
                                  uint8_t* d_result, const tkv_amq_probe_opts* opts, void* stream)
{
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n == 0) return TKV_AMQ_OK;
  if (!d_filters || !d_segs || !d_query || !d_qseg || !d_result || n_segs == 0 || k_max == 0 ||
      k_max > kMaxBloomHashes)
    return TKV_AMQ_INVALID_ARGUMENT;
  const tkv_amq_probe_opts o = probe_opts(opts);
  const bool ex = probe_opts_used(o);
  if (ex)
    hipLaunchKernelGGL(bloom_probe_hashed<true>, dim3(probe_grid(n, true)), dim3(256), 0,
                       as_stream(stream), d_filters, d_segs, n_segs, d_query, k_max, d_pair_query, n,
                       d_qseg, d_result, o);
  else
    hipLaunchKernelGGL(bloom_probe_hashed<false>, dim3(probe_grid(n, false)), dim3(256), 0,
                       as_stream(stream), d_filters, d_segs, n_segs, d_query, k_max, d_pair_query, n,
                       d_qseg, d_result, o);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

// Path probe workspace: a 16-byte header (reserved), the workgroup totals, one answer mask
// per query, one answer byte per entry (used when the caller passes no d_entry_result).
struct PathWsLayout {
  uint64_t n_wgs, totals_off, mask_off, answers_off, bytes;
};

static PathWsLayout path_ws_layout(uint64_t n_queries, uint64_t n_entries)
{
  PathWsLayout l;
  l.n_wgs = div_up(n_queries, 256);
  l.totals_off = 16;
  l.mask_off = l.totals_off + div_up(4 * l.n_wgs, 16) * 16;
  l.answers_off = l.mask_off + div_up(4 * n_queries, 16) * 16;
  l.bytes = l.answers_off + div_up(n_entries, 16) * 16;
  return l;
}

uint64_t tkv_amq_path_probe_ws_bytes(uint64_t n_queries, uint64_t n_entries)
{
  if (n_queries > 0xffffffffull || n_entries > 0xffffffffull) return 0;
  return path_ws_layout(n_queries, n_entries).bytes;
}

int tkv_amq_path_probe(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                       const uint8_t* q, const uint64_t* qoffs, uint32_t stride, uint64_t n_queries,
                       const uint32_t* d_path_begin, const uint32_t* d_path_leaf, uint64_t n_entries,
                       uint8_t* d_entry_result, uint32_t* d_cand_begin, uint32_t* d_cand_leaf,
                       uint32_t* d_cand_entry, const tkv_amq_probe_opts* opts, void* d_ws,
                       uint64_t ws_bytes, void* stream)
{
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (kind != TKV_AMQ_BLOOM && kind != TKV_AMQ_VQF) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_queries > 0xffffffffull || n_entries > 0xffffffffull) return TKV_AMQ_INVALID_ARGUMENT;
  const hipStream_t s = as_stream(stream);
  if (n_queries == 0) {
    if (d_cand_begin) {
      hipLaunchKernelGGL(scan_totals<uint32_t>, dim3(1), dim3(256), 0, s, static_cast<uint32_t*>(nullptr), 0u,
                         d_cand_begin, 0u, static_cast<uint64_t*>(nullptr));
      return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
    }
    return TKV_AMQ_OK;
  }
  if (!q || !d_path_begin || !d_cand_begin || (!qoffs && !stride)) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_entries && (!d_filters || !d_segs || n_segs == 0 || !d_path_leaf || !d_cand_leaf))
    return TKV_AMQ_INVALID_ARGUMENT;
  const PathWsLayout l = path_ws_layout(n_queries, n_entries);
  if (!d_ws || ws_bytes < l.bytes || (reinterpret_cast<uintptr_t>(d_ws) & 15))
    return TKV_AMQ_INVALID_ARGUMENT;
  const int mode = key_mode(qoffs, stride);
  if (mode == kKey16 && (reinterpret_cast<uintptr_t>(q) & 15)) return TKV_AMQ_INVALID_ARGUMENT;
  const tkv_amq_probe_opts o = probe_opts(opts);
  const bool ex = probe_opts_used(o);
  uint8_t* ws = static_cast<uint8_t*>(d_ws);
  PathArgs a;
  a.filters = d_filters;
  a.segs = d_segs;
  a.n_segs = n_segs;
  a.q = q;
  a.qoffs = qoffs;
  a.stride = stride;
  a.n_queries = (uint32_t)n_queries;
  a.path_begin = d_path_begin;
  a.path_leaf = d_path_leaf;
  a.n_entries = (uint32_t)n_entries;
  a.every_answer = d_entry_result ? 1u : 0u;
  a.answers = d_entry_result ? d_entry_result : ws + l.answers_off;
  a.mask = reinterpret_cast<uint32_t*>(ws + l.mask_off);
  a.wg_total = reinterpret_cast<uint32_t*>(ws + l.totals_off);
  a.cand_begin = d_cand_begin;
  a.cand_leaf = d_cand_leaf;
  a.cand_entry = d_cand_entry;
  a.n_wgs = (uint32_t)l.n_wgs;
  // with options: a bounded grid, so the metrics take one atomic per counter per wave (as
  // probe_grid does for the pair probes)
  const dim3 grid(ex && a.n_wgs > 8192u ? 8192u : a.n_wgs), block(256);
  with_key_mode(mode, [&](auto M) {
    with_flag(ex, [&](auto X) {
      constexpr int MODE = decltype(M)::value;
      constexpr bool kOpts = decltype(X)::value;
      if (kind == TKV_AMQ_BLOOM)
        hipLaunchKernelGGL((path_probe_kernel<TKV_AMQ_BLOOM, MODE, kOpts>), grid, block, 0, s, a, o);
      else
        hipLaunchKernelGGL((path_probe_kernel<TKV_AMQ_VQF, MODE, kOpts>), grid, block, 0, s, a, o);
    });
  });
  hipLaunchKernelGGL(scan_totals<uint32_t>, dim3(1), dim3(256), 0, s, a.wg_total, a.n_wgs,
                     d_cand_begin + a.n_queries, a.n_entries, static_cast<uint64_t*>(nullptr));
  hipLaunchKernelGGL(path_scatter, dim3(a.n_wgs), block, 0, s, a);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

// The argument checks of tkv_amq_get_keys and tkv_amq_get_values, everything but the result pointer's
// own (judged first, so a bad call is InvalidArgument with or without a device), and the launch's
// arguments filled from them.  `order`: one order for the pivots and the leaves.
static int get_prepare(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                       const tkv_amq_tree_node* nodes, uint64_t n_nodes, const tkv_amq_tree_segment* segments,
                       uint64_t n_segments, const tkv_amq_tree_child* children, uint64_t n_children,
                       const uint32_t* d_flushed_bounds, uint64_t n_flushed_bounds, const uint8_t* pivot_keys,
                       const uint64_t* pivot_key_offsets, uint32_t pivot_key_stride, uint64_t n_pivot_keys,
                       const uint8_t* queries, const uint64_t* query_offsets, uint32_t query_stride,
                       uint64_t n_queries, const uint8_t* leaf_keys, const uint64_t* leaf_key_offsets,
                       uint32_t leaf_key_stride, uint64_t n_leaf_keys, const uint64_t* d_key_begin, uint32_t flags,
                       const void* d_result, uint32_t* d_query_visits, tkv_amq_probe_metrics* d_metrics,
                       const void* d_counts, GetArgs& a, int& order, int& hash_mode)
{
  constexpr uint64_t kMax = 0xffffffffull;
  if (kind != TKV_AMQ_BLOOM && kind != TKV_AMQ_VQF) return TKV_AMQ_INVALID_ARGUMENT;
  if (flags & ~TKV_AMQ_GET_CHECK_PAGE_ID) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_nodes > kMax || n_segments > kMax || n_children > kMax || n_flushed_bounds > kMax ||
      n_pivot_keys > kMax || n_queries > kMax)
    return TKV_AMQ_INVALID_ARGUMENT;
  if ((n_nodes && !nodes) || (n_segments && !segments) || (n_children && !children) ||
      (n_flushed_bounds && !d_flushed_bounds) || (n_pivot_keys && !pivot_keys) || (n_leaf_keys && !leaf_keys))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (n_segs && (!d_segs || !d_filters)) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_queries && (!queries || !d_result)) return TKV_AMQ_INVALID_ARGUMENT;
  if ((!pivot_key_offsets && !pivot_key_stride) || (!query_offsets && !query_stride) ||
      (!leaf_key_offsets && !leaf_key_stride))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (((reinterpret_cast<uintptr_t>(nodes) | reinterpret_cast<uintptr_t>(segments) |
        reinterpret_cast<uintptr_t>(children) | reinterpret_cast<uintptr_t>(d_result)) & 15) ||
      ((reinterpret_cast<uintptr_t>(d_metrics) | reinterpret_cast<uintptr_t>(d_counts)) & 7) ||
      (reinterpret_cast<uintptr_t>(d_query_visits) & 3))
    return TKV_AMQ_INVALID_ARGUMENT;
  // the hash's mode is the path probe's, with its rule for 16-byte queries
  hash_mode = key_mode(query_offsets, query_stride);
  if (hash_mode == kKey16 && (reinterpret_cast<uintptr_t>(queries) & 15)) return TKV_AMQ_INVALID_ARGUMENT;
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
  a.filters = d_filters;
  a.segs_plan = d_segs;
  a.n_plan = n_segs;
  a.check_id = (flags & TKV_AMQ_GET_CHECK_PAGE_ID) ? 1u : 0u;
  a.q = queries;
  a.qoffs = query_offsets;
  a.qstride = query_stride;
  a.n_queries = (uint32_t)n_queries;
  a.keys = leaf_keys;
  a.koffs = leaf_key_offsets;
  a.kstride = leaf_key_stride;
  a.n_tiles = (uint32_t)div_up(n_queries, kGetThreads);
  a.n_keys = n_leaf_keys;
  a.key_begin = d_key_begin;
  a.result = nullptr;
  a.visits = d_query_visits;
  a.metrics = d_metrics;
  a.counts = nullptr;
  // a fast mode only if all three sides have its shape
  const KeyArray qa{queries, query_offsets, query_stride};
  const int op = key_order_mode(qa, KeyArray{pivot_keys, pivot_key_offsets, pivot_key_stride});
  const int ol = key_order_mode(qa, KeyArray{leaf_keys, leaf_key_offsets, leaf_key_stride});
  order = op == ol ? op : (int)kOrderAny;
  return TKV_AMQ_OK;
}

// launch(KIND, ORDER, HASH as integral constants) for the form the key shapes choose
extern "C++" template <typename Launch>
static void with_get_form(int kind, int order, int hash_mode, Launch&& launch)
{
  auto pick = [&](auto K) {
    if (order == kOrder16) {
      launch(K, KeyModeC<kOrder16>{}, KeyModeC<kKey16>{});
    } else if (order == kOrder24) {
      launch(K, KeyModeC<kOrder24>{}, KeyModeC<kKeyFixed>{});
    } else {
      with_key_mode(hash_mode, [&](auto M) { launch(K, KeyModeC<kOrderAny>{}, M); });
    }
  };
  if (kind == TKV_AMQ_BLOOM) pick(KeyModeC<TKV_AMQ_BLOOM>{});
  else pick(KeyModeC<TKV_AMQ_VQF>{});
}

int tkv_amq_get_keys(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                     const tkv_amq_tree_node* nodes, uint64_t n_nodes, const tkv_amq_tree_segment* segments,
                     uint64_t n_segments, const tkv_amq_tree_child* children, uint64_t n_children,
                     const uint32_t* d_flushed_bounds, uint64_t n_flushed_bounds, const uint8_t* pivot_keys,
                     const uint64_t* pivot_key_offsets, uint32_t pivot_key_stride, uint64_t n_pivot_keys,
                     const uint8_t* queries, const uint64_t* query_offsets, uint32_t query_stride,
                     uint64_t n_queries, const uint8_t* leaf_keys, const uint64_t* leaf_key_offsets,
                     uint32_t leaf_key_stride, uint64_t n_leaf_keys, const uint64_t* d_key_begin, uint32_t flags,
                     tkv_amq_get_result* d_result, uint32_t* d_query_visits, tkv_amq_probe_metrics* d_metrics,
                     tkv_amq_get_counts* d_counts, void* stream)
{
  GetArgs a;
  int order, hash_mode;
  const int st = get_prepare(kind, d_filters, d_segs, n_segs, nodes, n_nodes, segments, n_segments, children,
                             n_children, d_flushed_bounds, n_flushed_bounds, pivot_keys, pivot_key_offsets,
                             pivot_key_stride, n_pivot_keys, queries, query_offsets, query_stride, n_queries,
                             leaf_keys, leaf_key_offsets, leaf_key_stride, n_leaf_keys, d_key_begin, flags, d_result,
                             d_query_visits, d_metrics, d_counts, a, order, hash_mode);
  if (st != TKV_AMQ_OK) return st;
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n_queries == 0) return TKV_AMQ_OK;
  a.result = d_result;
  a.counts = d_counts;
  const dim3 grid(a.n_tiles < kGetMaxGrid ? a.n_tiles : kGetMaxGrid), block(kGetThreads);
  const hipStream_t s = as_stream(stream);
  with_get_form(kind, order, hash_mode, [&](auto K, auto O, auto H) {
    hipLaunchKernelGGL((get_keys_kernel<decltype(K)::value, decltype(O)::value, decltype(H)::value>), grid, block, 0,
                       s, a);
  });
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

// the checks the two value entry points share
static bool value_array_ok(const uint8_t* leaf_values, const uint64_t* leaf_value_offsets, uint32_t leaf_value_stride,
                           uint64_t leaf_values_bytes, uint64_t n_leaf_keys)
{
  if (n_leaf_keys && leaf_values_bytes && !leaf_values) return false;
  return !(n_leaf_keys && !leaf_value_offsets && !leaf_value_stride);
}

int tkv_amq_get_values(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                       const tkv_amq_tree_node* nodes, uint64_t n_nodes, const tkv_amq_tree_segment* segments,
                       uint64_t n_segments, const tkv_amq_tree_child* children, uint64_t n_children,
                       const uint32_t* d_flushed_bounds, uint64_t n_flushed_bounds, const uint8_t* pivot_keys,
                       const uint64_t* pivot_key_offsets, uint32_t pivot_key_stride, uint64_t n_pivot_keys,
                       const uint8_t* queries, const uint64_t* query_offsets, uint32_t query_stride,
                       uint64_t n_queries, const uint8_t* leaf_keys, const uint64_t* leaf_key_offsets,
                       uint32_t leaf_key_stride, uint64_t n_leaf_keys, const uint64_t* d_key_begin,
                       const uint8_t* leaf_values, const uint64_t* leaf_value_offsets, uint32_t leaf_value_stride,
                       uint64_t leaf_values_bytes, uint32_t flags, tkv_amq_value_result* d_result,
                       uint32_t* d_query_visits, tkv_amq_probe_metrics* d_metrics, tkv_amq_value_counts* d_counts,
                       void* stream)
{
  ValueArgs a;
  int order, hash_mode;
  const int st = get_prepare(kind, d_filters, d_segs, n_segs, nodes, n_nodes, segments, n_segments, children,
                             n_children, d_flushed_bounds, n_flushed_bounds, pivot_keys, pivot_key_offsets,
                             pivot_key_stride, n_pivot_keys, queries, query_offsets, query_stride, n_queries,
                             leaf_keys, leaf_key_offsets, leaf_key_stride, n_leaf_keys, d_key_begin, flags, d_result,
                             d_query_visits, d_metrics, d_counts, a, order, hash_mode);
  if (st != TKV_AMQ_OK) return st;
  if (!value_array_ok(leaf_values, leaf_value_offsets, leaf_value_stride, leaf_values_bytes, n_leaf_keys))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n_queries == 0) return TKV_AMQ_OK;
  a.v = ValueArray{leaf_values, leaf_value_offsets, leaf_value_stride, leaf_values_bytes};
  a.vresult = d_result;
  a.vcounts = d_counts;
  const dim3 grid(a.n_tiles < kGetMaxGrid ? a.n_tiles : kGetMaxGrid), block(kGetThreads);
  const hipStream_t s = as_stream(stream);
  with_get_form(kind, order, hash_mode, [&](auto K, auto O, auto H) {
    hipLaunchKernelGGL((get_values_kernel<decltype(K)::value, decltype(O)::value, decltype(H)::value>), grid, block,
                       0, s, a);
  });
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

int tkv_amq_gather_values(const tkv_amq_value_result* d_result, uint64_t n_queries, const uint8_t* leaf_values,
                          const uint64_t* leaf_value_offsets, uint32_t leaf_value_stride, uint64_t leaf_values_bytes,
                          uint64_t n_leaf_keys, uint8_t* d_out, uint32_t out_stride, uint32_t* d_value_len,
                          void* stream)
{
  if (n_queries > 0xffffffffull) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_queries && (!d_result || !d_value_len || (out_stride && !d_out))) return TKV_AMQ_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(d_result) & 15) || (reinterpret_cast<uintptr_t>(d_value_len) & 3))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (!value_array_ok(leaf_values, leaf_value_offsets, leaf_value_stride, leaf_values_bytes, n_leaf_keys))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n_queries == 0) return TKV_AMQ_OK;
  GatherArgs a;
  a.result = d_result;
  a.n_queries = n_queries;
  a.n_keys = n_leaf_keys;
  a.v = ValueArray{leaf_values, leaf_value_offsets, leaf_value_stride, leaf_values_bytes};
  a.out = d_out;
  a.out_stride = out_stride;
  a.len = d_value_len;
  hipLaunchKernelGGL(gather_values_kernel, dim3((uint32_t)div_up(n_queries, kGatherPerBlock)), dim3(kGatherThreads), 0,
                     as_stream(stream), a);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

}  // extern "C"
