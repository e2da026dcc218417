// tkv_amq_verify.h -- tkv_amq_verify_members: does every key of every leaf pass its own filter?
// Included at the end of tkv_amq_kernels.hip; it is not a translation unit of its own.  It uses
// the hashers and the bit ladder of tkv_amq_hash.h, the block tests of tkv_amq_probe.h
// (bloom_block_test, vqf_present_at), div_up and as_stream of tkv_amq_launch.h,
// prefix_inclusive_u64 of tkv_amq_scan.h, and of the build unit itself the VQF build's key
// buffer and hash (VqfKeyBuf, vqf_key_hash), with_build_key_mode, launch_lds_cap and the leaf LDS
// budgets, which is why it is compiled there.  DESIGN.md section 13.
//
//   verify_init     one lane per leaf: the clamped key range, the flags (no filter, the payload's
//                   src_page_id against the segment's), the result zeroed, the leaf's unit count
//   prefix_inclusive_u64 (tkv_amq_scan.h)
//                   one workgroup: the unit counts' inclusive prefix, in the workspace
//   verify_members_kernel
//                   one workgroup per unit (up to chunk_keys consecutive keys of one leaf, found
//                   through the prefix).  The leaf's blocks are copied into LDS with 16-byte
//                   loads when they fit what the launch allocated, and the unit's keys are loaded
//                   (ahead, nontemporal, for the 16- and 24-byte modes), hashed by the builds'
//                   hasher types and TESTED against the image: k ds_read_b32 per Bloom key, the
//                   primary and, if needed, the alternate block's metadata and tag window per VQF
//                   key.  Rejects are counted per lane, summed over the wave, and a wave that saw
//                   one adds to its leaf with integer atomics.  A leaf whose blocks do not fit
//                   runs the same loop with the block reads from global memory.
#pragma once

namespace tkv {

struct VerifyArgs {
  const uint8_t* filters;
  const tkv_amq_segment* segs;
  const uint8_t* keys;
  const uint64_t* offs;
  const uint64_t* key_begin;  // CSR [n_segs + 1], or NULL: the segments' key_begin / n_keys
  tkv_amq_member_check* result;
  unsigned long long* total;  // or NULL
  uint64_t* pre;              // [n_segs + 1]: pre[s] = units before leaf s
  uint64_t n_keys;
  uint32_t n_segs, stride;
  uint32_t chunk_keys;  // keys per unit
  uint32_t lds_blocks;  // the blocks the launch's dynamic LDS holds
};

TKV_INLINE bool verify_has_filter(int kind, const tkv_amq_segment& g)
{
  return g.n_blocks != 0 && (kind == TKV_AMQ_BLOOM ? g.hash_count != 0 : g.tag_bits != 0);
}

__global__ __launch_bounds__(256) void verify_init(int kind, VerifyArgs a)
{
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s == 0) {
    if (a.pre) a.pre[0] = 0;
    if (a.total) *a.total = 0;
  }
  if (s >= a.n_segs) return;
  const tkv_amq_segment g = a.segs[s];
  uint32_t flags = TKV_AMQ_VERIFY_NO_FILTER;
  uint64_t units = 0;
  if (verify_has_filter(kind, g)) {
    // the 8 bytes page_id_matches reads
    const uint64_t id = *reinterpret_cast<const uint64_t*>(a.filters + g.out_offset + src_page_id_offset(kind));
    flags = id != g.src_page_id ? TKV_AMQ_VERIFY_ID_MISMATCH : 0u;
    uint64_t b, e;
    segment_key_range(a.key_begin, &g, s, a.n_keys, b, e);
    units = (e - b + a.chunk_keys - 1) / a.chunk_keys;
  }
  // first_missing = ~0 | missing = 0, flags
  *reinterpret_cast<ulonglong2*>(a.result + s) = ulonglong2{~0ull, (uint64_t)flags << 32};
  a.pre[s + 1] = units;
}

// Where a leaf's blocks are read from.  words(b): block b as 16 words; bytes(): block 0.
struct VerifyLdsBlocks {
  uint32_t base;  // LDS byte address of block 0
  TKV_INLINE const lds_u32_t* words(uint32_t block) const
  {
    return reinterpret_cast<const lds_u32_t*>((uintptr_t)(base + (block << 6)));
  }
  TKV_INLINE lds_bytes_t bytes() const { return reinterpret_cast<lds_bytes_t>((uintptr_t)base); }
};

struct VerifyGlobalBlocks {
  const uint8_t* base;
  TKV_INLINE const uint32_t* words(uint32_t block) const
  {
    return reinterpret_cast<const uint32_t*>(base + 64ull * block);
  }
  TKV_INLINE const uint8_t* bytes() const { return base; }
};

struct VerifyLeaf {  // what the key loop needs of the segment
  uint32_t nb, k, tag_bits;
  uint64_t mask, magic;  // VQF: hash_mask, mod_magic
};

// A key loaded ahead of its test (16- and 24-byte modes: VqfKeyBuf's registers; other shapes
// are read where they are hashed)
struct VerifyNoBuf {};
template <int MODE>
using VerifyKeyBuf = std::conditional_t<MODE == kKey16 || MODE == kKey24, VqfKeyBuf<MODE>, VerifyNoBuf>;

template <int MODE>
TKV_INLINE void verify_load_key(const uint8_t* __restrict__ keys, uint64_t i, VerifyKeyBuf<MODE>& kb)
{
  if constexpr (MODE == kKey16) {
    kb.v = load_nt16(keys + 16 * i);
  } else if constexpr (MODE == kKey24) {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(keys) + 3 * i;
#pragma unroll
    for (int w = 0; w < 3; ++w) kb.w[w] = __builtin_nontemporal_load(p + w);
  }
}

template <int K, typename Blocks, typename H>
TKV_INLINE uint32_t verify_bloom_key(const Blocks& m, const VerifyLeaf& lf, const H& x)
{
  const uint64_t h0 = x.h0();
  return bloom_block_test<K>(x, h0, m.words((uint32_t)bloom_block(h0, lf.nb)), lf.k);
}

// 1: tkv_amq_probe would answer 1 for (key i, this leaf)
template <int KIND, int MODE, int K, typename Blocks>
TKV_INLINE uint32_t verify_key_present(const VerifyArgs& a, const VerifyLeaf& lf, const Blocks& m, uint64_t i,
                                       const VerifyKeyBuf<MODE>& kb)
{
  if constexpr (KIND == TKV_AMQ_BLOOM) {
    if constexpr (MODE == kKey16) {
      return verify_bloom_key<K>(m, lf, Bloom16(kb.v));
    } else if constexpr (MODE == kKey24) {
      return verify_bloom_key<K>(m, lf, BloomFixed<24>(kb.w));
    } else {
      return with_bloom_key_at<MODE>(a.keys, a.offs, a.stride, i,
                                     [&](const auto& x) { return verify_bloom_key<K>(m, lf, x); });
    }
  } else {
    uint64_t h;
    if constexpr (MODE == kKey16 || MODE == kKey24) h = vqf_key_hash<MODE>(a.keys, a.offs, a.stride, i, kb);
    else h = hash_key<MODE>(a.keys, a.offs, a.stride, i, kVqfHashSeed);
    if ((h & lf.mask) != h) return 1u;  // dropped by hash_val_shift: always "maybe"
    return lf.tag_bits == 8 ? (uint32_t)vqf_present_at<8>(m.bytes(), lf.nb, lf.magic, h)
                            : (uint32_t)vqf_present_at<16>(m.bytes(), lf.nb, lf.magic, h);
  }
}

// Keys [kb0, ke) of one leaf against its blocks: full chunks of NT * U keys without guards, the
// tail guarded (as the builds' leaf loops).  A lane meets its keys in rising order, so its first
// reject is its smallest.
template <int KIND, int MODE, uint32_t NT, int K, typename Blocks>
TKV_INLINE void verify_unit(const VerifyArgs& a, const VerifyLeaf& lf, const Blocks& m, uint64_t kb0, uint64_t ke,
                            uint32_t& miss, uint64_t& first)
{
  constexpr int U = MODE == kKey16 ? 4 : MODE == kKey24 ? 2 : 1;
  constexpr uint32_t C = NT * U;
  const uint32_t tid = threadIdx.x;
  uint64_t base = kb0;
  for (; ke - base >= C; base += C) {
    VerifyKeyBuf<MODE> kb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) verify_load_key<MODE>(a.keys, base + u * NT + tid, kb[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = base + u * NT + tid;
      if (!verify_key_present<KIND, MODE, K>(a, lf, m, i, kb[u]) && miss++ == 0) first = i;
      __builtin_amdgcn_sched_barrier(0);  // one key at a time, as in bloom_keys16_lds (register count)
    }
  }
  if (base < ke) {
    VerifyKeyBuf<MODE> kb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = base + u * NT + tid;
      verify_load_key<MODE>(a.keys, i < ke ? i : ke - 1, kb[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = base + u * NT + tid;
      if (i < ke && !verify_key_present<KIND, MODE, K>(a, lf, m, i, kb[u]) && miss++ == 0) first = i;
    }
  }
}

// the leaf of unit u: the last s with pre[s] <= u (it has pre[s + 1] > u: leaves without a unit
// are skipped).  Equal leaves put it at u * n_segs / total, which is tried first.
TKV_INLINE uint32_t verify_find_leaf(const uint64_t* __restrict__ pre, uint32_t n_segs, uint64_t u, uint64_t total)
{
  if (total <= 0xffffffffull) {
    const uint32_t g = (uint32_t)(u * n_segs / total);
    if (pre[g] <= u && u < pre[g + 1]) return g;
  }
  uint32_t lo = 0, hi = n_segs;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pre[mid] <= u) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <int KIND, int MODE, uint32_t NT>
__global__ __launch_bounds__(NT) void verify_members_kernel(VerifyArgs a)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t s_vimg[];
  const uint64_t total = a.pre[a.n_segs];
  const uint32_t tid = threadIdx.x;
  // (the grid covers every unit of disjoint leaves; overlapping CSR ranges loop)
  for (uint64_t u = blockIdx.x; u < total; u += gridDim.x) {
    const uint32_t s = verify_find_leaf(a.pre, a.n_segs, u, total);
    const tkv_amq_segment g = a.segs[s];
    uint64_t b, e;
    segment_key_range(a.key_begin, &g, s, a.n_keys, b, e);
    const uint64_t kb0 = b + (u - a.pre[s]) * a.chunk_keys;
    const uint64_t ke = e - kb0 < a.chunk_keys ? e : kb0 + a.chunk_keys;
    VerifyLeaf lf;
    lf.nb = g.n_blocks;
    lf.k = g.hash_count;
    lf.tag_bits = g.tag_bits;
    lf.mask = ~0ull << g.hash_val_shift;
    lf.magic = g.mod_magic;
    const uint8_t* blocks =
        a.filters + g.out_offset + (KIND == TKV_AMQ_BLOOM ? kBloomHeader : kVqfHeader + kVqfMetadata);
    uint32_t miss = 0;
    uint64_t first = ~0ull;
    if (lf.nb <= a.lds_blocks) {
      const uint4* src = reinterpret_cast<const uint4*>(blocks);
      uint4* dst = reinterpret_cast<uint4*>(s_vimg);
      for (uint32_t i = tid; i < 4 * lf.nb; i += NT) dst[i] = src[i];
      __syncthreads();
      const VerifyLdsBlocks m{lds_addr(s_vimg)};
      if (KIND == TKV_AMQ_BLOOM && lf.k == 7) verify_unit<KIND, MODE, NT, 7>(a, lf, m, kb0, ke, miss, first);
      else if (KIND == TKV_AMQ_BLOOM && lf.k == 8) verify_unit<KIND, MODE, NT, 8>(a, lf, m, kb0, ke, miss, first);
      else verify_unit<KIND, MODE, NT, 0>(a, lf, m, kb0, ke, miss, first);
      __syncthreads();  // (the next unit's copy overwrites the image)
    } else {
      verify_unit<KIND, MODE, NT, 0>(a, lf, VerifyGlobalBlocks{blocks}, kb0, ke, miss, first);
    }
    // one set of atomics per wave, and only from a wave that saw a reject
    const uint32_t wave_miss = wave_sum(miss);
    if (wave_miss != 0) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = __shfl_xor(first, o, 64);
        first = other < first ? other : first;
      }
      if (__lane_id() == 0) {
        tkv_amq_member_check* r = a.result + s;
        atomicAdd(&r->missing, wave_miss);
        atomicMin(reinterpret_cast<unsigned long long*>(&r->first_missing), (unsigned long long)first);
        if (a.total) atomicAdd(a.total, (unsigned long long)wave_miss);
      }
    }
  }
}

}  // namespace tkv

namespace {

// Keys per unit, from the batch's size alone: about kVerifyTargetUnits units over the batch (eight
// workgroups for each of 256 CUs), at least kVerifyMinChunk keys each (two full 16-byte-key chunks
// of a 256-thread workgroup), in multiples of 1,024 keys.  6,104 leaves of 16K keys: 49,152, one
// unit per leaf; one leaf of 3M keys: 2,048, 1,465 units.
constexpr uint64_t kVerifyTargetUnits = 2048;
constexpr uint64_t kVerifyMinChunk = 2048;

inline uint32_t verify_chunk_keys(uint64_t n_keys, uint32_t n_segs)
{
  (void)n_segs;  // (leaves add units, never remove them: the key count alone sizes the chunk)
  uint64_t c = div_up(n_keys, kVerifyTargetUnits);
  if (c < kVerifyMinChunk) c = kVerifyMinChunk;
  if (c > (1ull << 30)) c = 1ull << 30;
  return (uint32_t)(div_up(c, 1024) * 1024);
}

constexpr uint64_t kVerifyWsHeader = 16;
constexpr uint64_t kVerifyMaxGrid = 1ull << 24;

inline uint64_t verify_ws_bytes(uint32_t n_segs)
{
  return kVerifyWsHeader + div_up(((uint64_t)n_segs + 1) * 8, 16) * 16;
}

template <int KIND, int MODE>
void launch_verify(uint32_t grid, size_t lds, hipStream_t s, const VerifyArgs& a)
{
  // images past kBloomWideLds take 1024-thread workgroups, as the LDS build's do
  if (lds > kBloomWideLds)
    launch_lds_cap<&verify_members_kernel<KIND, MODE, 1024>>(kBloomLeafLdsBudget, dim3(grid), dim3(1024), lds, s, a);
  else
    hipLaunchKernelGGL((verify_members_kernel<KIND, MODE, 256>), dim3(grid), dim3(256), lds, s, a);
}

}  // namespace

extern "C" {

uint64_t tkv_amq_verify_members_ws_bytes(uint32_t n_segs) { return verify_ws_bytes(n_segs); }

int tkv_amq_verify_members(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                           uint32_t max_seg_blocks, const uint8_t* keys, const uint64_t* key_offsets,
                           uint32_t key_stride, uint64_t n_keys, const uint64_t* d_key_begin,
                           tkv_amq_member_check* d_result, uint64_t* d_total_missing, void* d_workspace,
                           uint64_t workspace_bytes, void* stream)
{
  // (the arguments are judged first, so a bad call is InvalidArgument with or without a device)
  if (kind != TKV_AMQ_BLOOM && kind != TKV_AMQ_VQF) return TKV_AMQ_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(d_filters) & 15) || (reinterpret_cast<uintptr_t>(d_result) & 15) ||
      (reinterpret_cast<uintptr_t>(d_total_missing) & 7))
    return TKV_AMQ_INVALID_ARGUMENT;
  const int bmode = build_key_mode(keys, key_offsets, key_stride);
  if (n_segs) {
    if (!d_filters || !d_segs || !d_result || !d_workspace || (n_keys && !keys)) return TKV_AMQ_INVALID_ARGUMENT;
    if (!key_offsets && key_stride == 0) return TKV_AMQ_INVALID_ARGUMENT;
    if (workspace_bytes < verify_ws_bytes(n_segs) || (reinterpret_cast<uintptr_t>(d_workspace) & 15))
      return TKV_AMQ_INVALID_ARGUMENT;
    // (16-byte keys load as one 16-byte word, as tkv_amq_build takes them)
    if (bmode == kKey16 && (reinterpret_cast<uintptr_t>(keys) & 15)) return TKV_AMQ_INVALID_ARGUMENT;
  }
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n_segs == 0 && !d_total_missing) return TKV_AMQ_OK;
  const hipStream_t s = as_stream(stream);
  VerifyArgs a;
  a.filters = d_filters;
  a.segs = d_segs;
  a.keys = keys;
  a.offs = key_offsets;
  a.key_begin = d_key_begin;
  a.result = d_result;
  a.total = reinterpret_cast<unsigned long long*>(d_total_missing);
  a.pre = n_segs ? reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_workspace) + kVerifyWsHeader) : nullptr;
  a.n_keys = n_keys;
  a.n_segs = n_segs;
  a.stride = key_stride;
  a.chunk_keys = verify_chunk_keys(n_keys, n_segs);
  // the hint sizes the image; 0 (unknown) and a hint past the leaf budget allocate the budget
  const uint64_t want = 64ull * max_seg_blocks;
  const size_t lds = want != 0 && want <= kBloomLeafLdsBudget ? (size_t)want : (size_t)kBloomLeafLdsBudget;
  a.lds_blocks = (uint32_t)(lds / 64);
  hipLaunchKernelGGL(verify_init, dim3(n_segs ? (n_segs + 255u) / 256u : 1u), dim3(256), 0, s, kind, a);
  if (n_segs == 0) return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
  hipLaunchKernelGGL(prefix_inclusive_u64<kPrefixThreads>, dim3(1), dim3(kPrefixThreads), 0, s, a.pre + 1, n_segs);
  if (n_keys != 0) {
    const uint64_t units = div_up(n_keys, a.chunk_keys) + n_segs;
    const uint32_t grid = (uint32_t)(units < kVerifyMaxGrid ? units : kVerifyMaxGrid);
    with_build_key_mode(bmode, [&](auto M) {
      constexpr int MODE = decltype(M)::value;
      if (kind == TKV_AMQ_BLOOM) launch_verify<TKV_AMQ_BLOOM, MODE>(grid, lds, s, a);
      else launch_verify<TKV_AMQ_VQF, MODE>(grid, lds, s, a);
    });
  }
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

}  // extern "C"
