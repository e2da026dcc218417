// tkv_amq_probe.h -- one filter test per kind, for any caller (device only; DESIGN.md sections
// 3.2, 5 and 11).
//
//   Bloom   probe_block16, bloom_probe_item: a 16-byte key's block staged in the lane's LDS slot;
//           bloom_block_test: the same answer from a block the caller holds (tkv_amq_verify.h);
//           ProbeTally, flush_tally: the KeyQuery::Metrics classes of a lane, summed per wave
//   VQF     Vqf<T>: the block geometry (the builds size their kernels with it too); ld_*: a block
//           in global memory or in LDS; VqfBucketRef .. vqf_present_at, vqf_probe_one: is_present;
//           vqf_query_hash: a query's one hash
//   Path    BloomEntry16, BloomBits16, BloomBitSource, bloom_entry_test: a query hashed once and
//           tested against every filter on its way (the path probe, tkv_amq_get_keys / _values)
//
// Included by tkv_amq_read.hip (every probe and lookup kernel) and by tkv_amq_kernels.hip (Vqf<T>
// for the VQF builds; bloom_block_test and vqf_present_at for tkv_amq_verify.h).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include <stdint.h>

#include "tkv_amq.h"
#include "tkv_amq_device.h"
#include "tkv_amq_hash.h"

namespace tkv {

// ---------------------------------------------------------------------------------------
// Bloom probe
// ---------------------------------------------------------------------------------------
// (ProbeDesc, load_probe_desc, ProbeClass, page_id_matches and wave_sum live in tkv_amq_device.h:
// tkv_amq_find.hip classifies its candidates with them too)

// One lane per (query, leaf).  The 64-byte filter block is fetched with four 16-byte loads
// (instead of k divergent 8-byte loads) and staged in a per-lane LDS slot; the k bit tests
// are then LDS reads.  Stride 20 dwords keeps the slots 16-byte aligned and spreads banks.
constexpr uint32_t kProbeSlotWords = 20;

// The block's four 16-byte loads are issued first and the remaining k-1 bit indices are
// hashed while they are in flight; only then is the block staged in the lane's LDS slot.
template <int K>
__device__ inline uint32_t probe_block16(const Bloom16& x, uint64_t h0, const uint4* blk, uint4* slot,
                                         uint32_t k_rt = K)
{
  const uint4 b0 = blk[0], b1 = blk[1], b2 = blk[2], b3 = blk[3];
  const uint32_t* slot32 = reinterpret_cast<const uint32_t*>(slot);
  uint32_t ok = 1;
  if constexpr (K > 0) {
    uint32_t bit[K];
    bit[0] = (uint32_t)h0 & kBloomBitMask;
    bloom_ladder<K>(x, K, [&](uint32_t j, uint32_t b) { bit[j] = b & kBloomBitMask; });
    slot[0] = b0;
    slot[1] = b1;
    slot[2] = b2;
    slot[3] = b3;
#pragma unroll
    for (int j = 0; j < K; ++j) ok &= slot32[bit[j] >> 5] >> (bit[j] & 31);
  } else {
    slot[0] = b0;
    slot[1] = b1;
    slot[2] = b2;
    slot[3] = b3;
    uint32_t b = (uint32_t)h0 & kBloomBitMask;
    ok &= slot32[b >> 5] >> (b & 31);
    for (uint32_t j = 1; j < k_rt; ++j) {
      b = x.bit(j) & kBloomBitMask;
      ok &= slot32[b >> 5] >> (b & 31);
    }
  }
  return ok;
}

// probe_block16's test in pointer form, for a caller that knows its leaf per workgroup and holds
// the filter's blocks itself (tkv_amq_verify_members): `blk` is the key's 64-byte block as 16
// words -- W = const lds_u32_t* for an image in LDS (each bit test one ds_read_b32, no staging
// slot), const uint32_t* for global memory -- and any hasher serves.  The same answer as
// probe_block16 / bloom_probe_item: the AND of the k bits.  K as in bloom_ladder.
template <int K, typename H, typename W>
TKV_INLINE uint32_t bloom_block_test(const H& x, uint64_t h0, W blk, uint32_t k)
{
  const uint32_t b0 = (uint32_t)h0;
  uint32_t ok = blk[(b0 >> 5) & 15u] >> (b0 & 31);
  bloom_ladder<K>(x, k, [&](uint32_t, uint32_t b) { ok &= blk[(b >> 5) & 15u] >> (b & 31); });
  return ok & 1u;
}

// KeyQuery::Metrics tallies of one lane (tkv_amq_probe_ex): per query, the class of its
// reject_page answer (tree/key_query.hpp:149-247).  Reduced over the wave with shuffles and
// added to the caller's counters with one atomic per counter per wave.
struct ProbeTally {
  uint32_t total = 0, no_filter = 0, mismatch = 0, reject = 0, positive = 0, false_pos = 0;
  // r: result bit (1 = maybe present) | class << 1
  __device__ inline void add(uint32_t r, const uint8_t* truth, uint64_t i)
  {
    const uint32_t cls = r >> 1;
    ++total;
    no_filter += cls == kNoFilter;
    mismatch += cls == kIdMismatch;
    const bool checked = cls == kChecked;
    reject += checked && !(r & 1u);
    const bool pos = checked && (r & 1u);
    positive += pos;
    if (pos && truth) false_pos += truth[i] == 0;
  }
};

__device__ inline void flush_tally(const ProbeTally& t, tkv_amq_probe_metrics* m, bool has_truth)
{
  const uint32_t v[6] = {wave_sum(t.total), wave_sum(t.no_filter), wave_sum(t.mismatch),
                         wave_sum(t.reject), wave_sum(t.positive), wave_sum(t.false_pos)};
  if (__lane_id() == 0 && m) {
    unsigned long long* c = reinterpret_cast<unsigned long long*>(m);
    if (v[0]) atomicAdd(&c[0], (unsigned long long)v[0]);
    if (v[1]) atomicAdd(&c[1], (unsigned long long)v[1]);
    if (v[2]) atomicAdd(&c[2], (unsigned long long)v[2]);
    if (v[3]) atomicAdd(&c[3], (unsigned long long)v[3]);
    if (v[4]) atomicAdd(&c[4], (unsigned long long)v[4]);
    if (has_truth && v[5]) atomicAdd(&c[5], (unsigned long long)v[5]);
  }
}

// One Bloom (query, leaf) test: result bit | class << 1 (the class only with kOpts).  Without
// kOpts the control flow is the plain probe's: no early exit, so the key load is issued
// side by side with the segment index and descriptor loads (an early "no filter" return
// made the compiler sink it behind them: 11% slower).
template <int MODE, bool kOpts>
__device__ inline uint32_t bloom_probe_item(const uint8_t* __restrict__ filters,
                                            const tkv_amq_segment* __restrict__ segs, uint32_t n_segs,
                                            const uint8_t* __restrict__ q,
                                            const uint64_t* __restrict__ qoffs, uint32_t stride,
                                            uint64_t i, uint32_t sidx, uint4* slot,
                                            const uint64_t* page_ids)
{
  uint32_t ok = 1;
  if constexpr (MODE == kKey16) {
    // the key load, the descriptor and the first hash do not depend on the "has a filter"
    // test, so they are issued before it: one dependent chain qseg -> descriptor -> block
    const uint4 kv = load_nt16(q + 16 * i);
    const ProbeDesc d = load_probe_desc(segs, sidx, n_segs);
    const Bloom16 x(kv);
    const uint64_t h0 = x.h0();
    const uint4* blk = reinterpret_cast<const uint4*>(filters + d.out_offset + kBloomHeader +
                                                      64 * bloom_block(h0, d.n_blocks));
    // hash_count 0: no filter page => reject_page returns kUnknown => cannot reject
    uint32_t cls = d.hash_count == 0 ? kNoFilter : kChecked;
    if constexpr (kOpts) {
      if (cls == kChecked && !page_id_matches(filters + d.out_offset, src_page_id_offset(TKV_AMQ_BLOOM), page_ids, i)) cls = kIdMismatch;
    }
    if (!kOpts || cls == kChecked) {
      if (d.hash_count == 7) ok = probe_block16<7>(x, h0, blk, slot);
      else if (d.hash_count == 8) ok = probe_block16<8>(x, h0, blk, slot);
      else if (d.hash_count != 0) ok = probe_block16<0>(x, h0, blk, slot, d.hash_count);
    }
    return (ok & 1u) | (cls << 1);
  } else {
    const ProbeDesc d = load_probe_desc(segs, sidx, n_segs);
    if (d.hash_count == 0) return 1u | (kNoFilter << 1);
    if (!page_id_matches(filters + d.out_offset, src_page_id_offset(TKV_AMQ_BLOOM), page_ids, i)) return 1u | (kIdMismatch << 1);
    const uint8_t* words = filters + d.out_offset + kBloomHeader;
    uint32_t len;
    const uint8_t* p = key_at<MODE>(q, qoffs, stride, i, len);
    if (len < 32) {  // seed-independent lane rounds shared by the k hashes
      const BloomShort x(p, len);
      const uint64_t h0 = x.h0();
      const uint64_t* blk = reinterpret_cast<const uint64_t*>(words + 64 * bloom_block(h0, d.n_blocks));
      uint32_t b = (uint32_t)h0 & kBloomBitMask;
      ok &= (uint32_t)(blk[b >> 6] >> (b & 63));
      for (uint32_t j = 1; j < d.hash_count; ++j) {
        b = x.bit(j) & kBloomBitMask;
        ok &= (uint32_t)(blk[b >> 6] >> (b & 63));
      }
    } else {
      const BloomLong x{p, len};
      const uint64_t h0 = x.h0();
      const uint64_t* blk = reinterpret_cast<const uint64_t*>(words + 64 * bloom_block(h0, d.n_blocks));
      uint32_t b = (uint32_t)h0 & kBloomBitMask;
      ok &= (uint32_t)(blk[b >> 6] >> (b & 63));
      for (uint32_t j = 1; j < d.hash_count; ++j) {
        b = x.bit(j) & kBloomBitMask;
        ok &= (uint32_t)(blk[b >> 6] >> (b & 63));
      }
    }
  }
  return (ok & 1u) | (kChecked << 1);
}

// ---------------------------------------------------------------------------------------
// VQF constants (tkv-amq v1)
// ---------------------------------------------------------------------------------------
template <int T>
struct Vqf;
template <>
struct Vqf<8> {
  static constexpr uint32_t kSlots = 48, kBuckets = 80, kThreshold = 37, kMdBytes = 16;
  static constexpr uint32_t kOffsetBits = 7;
  using Entry = uint16_t;  // (bucket offset << 8) | tag
};
template <>
struct Vqf<16> {
  static constexpr uint32_t kSlots = 28, kBuckets = 36, kThreshold = 22, kMdBytes = 8;
  static constexpr uint32_t kOffsetBits = 6;
  using Entry = uint32_t;  // (bucket offset << 16) | tag
};
// kThreshold: the reference-side vqf consults the alternate block only when the primary's
// metadata popcount is below CHECK_ALT (92 / 43), i.e. when its count >= kThreshold.

// ---------------------------------------------------------------------------------------
// VQF probe (PackedVqfFilter::is_present, vqf_filter_page_view.hpp:113-125)
// ---------------------------------------------------------------------------------------
// The block pointer is a type parameter: BP = const uint8_t* reads a filter in global memory (the
// probes), BP = lds_bytes_t one staged in LDS (tkv_amq_verify_members: its loads are ds_read,
// not flat).  ld_as<V>(p): the scalar V at p in p's address space; ld_u64x2 / ld_win16: a block's
// 16 metadata bytes, and a bucket's 16-byte tag window (4-byte aligned: one load from global
// memory, as the probes always read it; four words from LDS, which the compiler pairs).
typedef const __attribute__((address_space(3))) uint8_t* lds_bytes_t;
typedef uint64_t u64x2_t __attribute__((ext_vector_type(2)));
template <typename V>
TKV_INLINE V ld_as(const uint8_t* p) { return *reinterpret_cast<const V*>(p); }
template <typename V>
TKV_INLINE V ld_as(lds_bytes_t p) { return *reinterpret_cast<const __attribute__((address_space(3))) V*>(p); }
TKV_INLINE ulonglong2 ld_u64x2(const uint8_t* p) { return *reinterpret_cast<const ulonglong2*>(p); }
TKV_INLINE ulonglong2 ld_u64x2(lds_bytes_t p)
{
  const u64x2_t v = ld_as<u64x2_t>(p);
  return ulonglong2{v.x, v.y};
}
TKV_INLINE uint4 ld_win16(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }
TKV_INLINE uint4 ld_win16(lds_bytes_t p)
{
  return uint4{ld_as<uint32_t>(p), ld_as<uint32_t>(p + 4), ld_as<uint32_t>(p + 8), ld_as<uint32_t>(p + 12)};
}

template <int T, typename BP = const uint8_t*>
struct VqfBucketRef {
  BP bp;            // the 64-byte block
  uint32_t o;       // bucket offset inside it
  uint64_t lo, hi;  // block metadata
};

template <int T, typename BP>
__device__ inline VqfBucketRef<T, BP> vqf_bucket_ref(BP blocks, uint32_t idx)
{
  using C = Vqf<T>;
  VqfBucketRef<T, BP> r;
  const uint32_t blk = idx / C::kBuckets;
  r.o = idx - blk * C::kBuckets;
  if constexpr (std::is_same_v<BP, lds_bytes_t>) r.bp = blocks + (blk << 6);
  else r.bp = blocks + (uint64_t)blk * 64;
  if constexpr (T == 8) {
    const ulonglong2 md = ld_u64x2(r.bp);
    r.lo = md.x;
    r.hi = md.y;
  } else {
    r.lo = ld_as<uint64_t>(r.bp);
    r.hi = 0;
  }
  return r;
}

// exact per-byte / per-halfword equality mask (high bit of each lane set where x's lane is 0)
__device__ inline uint32_t zero_bytes(uint32_t x)
{
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
__device__ inline uint32_t zero_halves(uint32_t x)
{
  return ~(((x & 0x7fff7fffu) + 0x7fff7fffu) | x | 0x7fff7fffu);
}

// Tags of bucket o are slots [start, end).  One 16-byte load of the tag area starting at the
// dword that holds slot `start` covers the bucket in almost every case (a bucket holds ~0.6
// tags on average); longer buckets finish with a per-slot loop.
template <int T, typename BP>
__device__ inline bool vqf_bucket_has(const VqfBucketRef<T, BP>& r, uint32_t tag)
{
  using C = Vqf<T>;
  const int o = (int)r.o;
  // metadata without an (o+1)-th set bit (a damaged block: every block the builds write has
  // at least kBuckets) holds no bucket o, as the CPU oracle's select reads it: absent
  if (__popcll(r.lo) + __popcll(r.hi) <= o) return false;
  const int start = o == 0 ? 0 : select128(r.lo, r.hi, o - 1) - (o - 1);
  const int end = select128(r.lo, r.hi, o) - o;
  if (end <= start) return false;
  constexpr int kPer = 4 / (T / 8);                     // slots per dword: 4 / 2
  const int d0 = start / kPer;                          // first dword of the window
  const int last_dword = (C::kSlots * (T / 8)) / 4 - 1; // 11 / 13
  const int d = d0 + 3 <= last_dword ? d0 : last_dword - 3;
  const uint4 w = ld_win16(r.bp + C::kMdBytes + 4 * d);
  const int s0 = start - d * kPer, s1 = end - d * kPer;  // window-relative slot range
  const uint32_t rep = T == 8 ? tag * 0x01010101u : tag * 0x00010001u;
  uint32_t m[4];
  const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = T == 8 ? zero_bytes(wv[i] ^ rep) : zero_halves(wv[i] ^ rep);
  // pack one bit per slot: slot j of the window <-> bit j
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (T == 8) {
      const uint32_t b4 = ((m[i] >> 7) & 1u) | ((m[i] >> 14) & 2u) | ((m[i] >> 21) & 4u) | ((m[i] >> 28) & 8u);
      bits |= b4 << (4 * i);
    } else {
      const uint32_t b2 = ((m[i] >> 15) & 1u) | ((m[i] >> 30) & 2u);
      bits |= b2 << (2 * i);
    }
  }
  constexpr int kWin = 4 * kPer;  // 16 / 8 slots
  const int hi_in = s1 < kWin ? s1 : kWin;
  const uint32_t range = (hi_in > s0 ? ((1u << (hi_in - s0)) - 1u) : 0u) << s0;
  bool hit = (bits & range) != 0;
  for (int p = d * kPer + kWin; p < end; ++p) {  // rare: bucket runs past the window
    uint32_t tv;
    if constexpr (T == 8) tv = r.bp[C::kMdBytes + p];
    else tv = ld_as<uint16_t>(r.bp + C::kMdBytes + 2 * p);
    hit |= tv == tag;
  }
  return hit;
}

// is_present over the blocks at `blocks` (global memory or an LDS image, see VqfBucketRef)
template <int T, typename BP>
__device__ inline bool vqf_present_at(BP blocks, uint32_t n_blocks, uint64_t magic, uint64_t h)
{
  using C = Vqf<T>;
  const uint64_t R = (uint64_t)n_blocks * C::kBuckets;
  const uint32_t tag = (uint32_t)(h & ((1ull << T) - 1));
  const uint32_t pi = (uint32_t)mod_by_magic(h >> T, R, magic);
  const uint32_t ai = (uint32_t)mod_by_magic((h ^ ((uint64_t)tag * kVqfAltMul)) >> T, R, magic);
  // primary bucket first; only the lanes that did not find the tag there read the alternate
  // block (vqf_is_present's order, vqf_filter_page_view.hpp:120-124; loading both blocks up
  // front measured slower)
  if (vqf_bucket_has<T>(vqf_bucket_ref<T>(blocks, pi), tag)) return true;
  return vqf_bucket_has<T>(vqf_bucket_ref<T>(blocks, ai), tag);
}

template <int T>
__device__ inline bool vqf_present(const uint8_t* payload, uint32_t n_blocks, uint64_t magic,
                                   uint64_t h)
{
  return vqf_present_at<T>(payload + kVqfHeader + kVqfMetadata, n_blocks, magic, h);
}

// One VQF (hash, leaf) test: result bit | class << 1.  Ids: where the page id to compare comes
// from, the probes' array indexed by i or the fused lookup's PageIdIs (page_id_matches).
// (always inlined: out of line it was a real call in every probe kernel, with a stack frame)
template <bool kOpts, typename Ids = const uint64_t*>
__device__ __attribute__((always_inline)) inline uint32_t vqf_probe_one(const uint8_t* filters, const tkv_amq_segment* segs,
                                         uint32_t n_segs, uint32_t s, uint64_t h,
                                         Ids page_ids = nullptr, uint64_t i = 0)
{
  const ProbeDesc d = load_probe_desc(segs, s, n_segs);
  if (d.tag_bits == 0) return 1u | (kNoFilter << 1);  // no filter: cannot reject
  const uint8_t* payload = filters + d.out_offset;
  if constexpr (kOpts) {
    if (!page_id_matches(payload, src_page_id_offset(TKV_AMQ_VQF), page_ids, i)) return 1u | (kIdMismatch << 1);
  }
  const uint64_t mask = ~0ull << d.hash_val_shift;  // == PackedVqfFilter::hash_mask
  // dropped hash values are always "maybe" (:115-117)
  if ((h & mask) != h) return 1u | (kChecked << 1);
  const uint64_t magic = segs[s].mod_magic;
  const bool p = d.tag_bits == 8 ? vqf_present<8>(payload, d.n_blocks, magic, h)
                                 : vqf_present<16>(payload, d.n_blocks, magic, h);
  return (uint32_t)p | (kChecked << 1);
}

template <int MODE>
__device__ inline uint64_t vqf_query_hash(const uint8_t* __restrict__ q, const uint64_t* __restrict__ qoffs,
                                          uint32_t stride, uint64_t i)
{
  if constexpr (MODE == kKey16) {
    const uint4 kv = load_nt16(q + 16 * i);
    const Xxh16 x((uint64_t)kv.x | ((uint64_t)kv.y << 32), (uint64_t)kv.z | ((uint64_t)kv.w << 32));
    return x.finish(xxh16_rhinit(kVqfHashSeed));
  } else {
    return hash_key<MODE>(q, qoffs, stride, i, kVqfHashSeed);
  }
}

// ---------------------------------------------------------------------------------------
// Path-probe helpers: one query against every filter on its way
// ---------------------------------------------------------------------------------------
// A 16-byte key's Bloom test in two halves, so that the next entry's descriptor (and, with
// options, its filter's page id) is in flight while this entry's block is loaded and tested:
// fetch = descriptor, class, block address; test = the block's loads and bit tests.
// (Measured on 200M entries: 4.49 ms with the descriptor fetched ahead, 4.66 without, at the
// same 66 VGPRs.  Loading the next block ahead as well held two blocks in registers: 108
// VGPRs, 4 waves.)
struct BloomEntry16 {
  const uint4* blk;
  uint32_t k_cls;  // hash_count | class << 16
  __device__ inline uint32_t k() const { return k_cls & 0xffffu; }
  __device__ inline uint32_t cls() const { return k_cls >> 16; }
};

template <bool kOpts, typename Ids>
__device__ inline BloomEntry16 bloom_entry16_fetch(const uint8_t* __restrict__ filters,
                                                   const tkv_amq_segment* __restrict__ segs,
                                                   uint32_t n_segs, uint32_t leaf, uint64_t h0,
                                                   Ids page_ids, uint32_t ent)
{
  BloomEntry16 f;
  const ProbeDesc d = load_probe_desc(segs, leaf, n_segs);
  uint32_t cls = d.hash_count == 0 ? kNoFilter : kChecked;
  if constexpr (kOpts) {
    if (cls == kChecked && !page_id_matches(filters + d.out_offset, src_page_id_offset(TKV_AMQ_BLOOM), page_ids, ent)) cls = kIdMismatch;
  }
  f.k_cls = d.hash_count | (cls << 16);
  f.blk = reinterpret_cast<const uint4*>(filters + d.out_offset + kBloomHeader +
                                         64 * bloom_block(h0, d.n_blocks));
  return f;
}

// Bit indices 1..7 of a 16-byte key (what hash_count <= 8 needs, i.e. up to 12 bits per key),
// finished once per query and packed 9 bits each into three registers; a filter with more
// hashes finishes indices 8.. again from the shared lane rounds (finish_lo9), per entry.
struct BloomBits16 {
  uint32_t w[3];
  __device__ inline explicit BloomBits16(const Bloom16& x)
  {
    w[0] = w[1] = w[2] = 0;
#pragma unroll
    for (int j = 1; j < 8; ++j)
      w[(j - 1) / 3] |= (x.bit(j) & kBloomBitMask) << (9 * ((j - 1) % 3));
  }
  // `zero` is 0 at run time, but comes from the entry, so that the unpacking stays in the loop
  // over the path: hoisted out of it, every index is held as an LDS address and a shift, two
  // registers each, and the kernel drops to 6 waves per SIMD
  template <int J>
  __device__ inline uint32_t get(uint32_t zero) const
  {
    return (w[(J - 1) / 3] >> (9 * ((J - 1) % 3) + zero)) & 511u;
  }
};

template <int J>
__device__ inline uint32_t bloom_bits16_and(const BloomBits16& bits, const uint32_t* slot32, uint32_t k,
                                            uint32_t zero, uint32_t ok)
{
  if constexpr (J < 8) {
    const uint32_t bit = bits.get<J>(zero);
    const uint32_t v = slot32[bit >> 5] >> (bit & 31);
    return bloom_bits16_and<J + 1>(bits, slot32, k, zero, ok & ((uint32_t)J < k ? v : 1u));
  } else {
    return ok;
  }
}

// the block test of probe_block16 (four 16-byte loads staged in the lane's LDS slot, the bit
// tests LDS reads) with the cached indices.  The hash state a filter of more than 8 hashes
// needs waits in the slot's four padding words (kProbeSlotWords = 20: 16 of block, 4 spare),
// not in registers.
__device__ inline void bloom_entry16_park(const Xxh16& x, uint4* slot)
{
  slot[4] = uint4{(uint32_t)x.rk1, (uint32_t)(x.rk1 >> 32), (uint32_t)x.k2, (uint32_t)(x.k2 >> 32)};
}

__device__ inline uint32_t bloom_entry16_test(uint64_t h0, const BloomBits16& bits,
                                              const BloomEntry16& f, uint4* slot)
{
  uint32_t ok = 1;
  if (f.cls() == kChecked) {
    const uint4 b0 = f.blk[0], b1 = f.blk[1], b2 = f.blk[2], b3 = f.blk[3];
    const uint32_t* slot32 = reinterpret_cast<const uint32_t*>(slot);
    slot[0] = b0;
    slot[1] = b1;
    slot[2] = b2;
    slot[3] = b3;
    const uint32_t k = f.k();
    uint32_t bit = (uint32_t)h0 & kBloomBitMask;
    // (class < 4 and hash_count < 65536: bit 31 of k_cls is never set)
    ok = bloom_bits16_and<1>(bits, slot32, k, f.k_cls >> 31, slot32[bit >> 5] >> (bit & 31));
    if (k > 8) {
      const uint4 xs = slot[4];
      Bloom16 x;
      x.rk1 = (uint64_t)xs.x | ((uint64_t)xs.y << 32);
      x.k2 = (uint64_t)xs.z | ((uint64_t)xs.w << 32);
      for (uint32_t j = 8; j < k; ++j) {
        bit = x.bit(j) & kBloomBitMask;
        ok &= slot32[bit >> 5] >> (bit & 31);
      }
    }
  }
  return (ok & 1u) | (f.cls() << 1);
}

// Keys of other shapes: the bit index of hash j of one query, for every filter on its way.
// Under 32 bytes the seed-independent lane rounds are shared by every hash of every filter.  A
// longer key's every hash reads the whole key: bit index j is computed when the first filter with
// more than j hashes comes by, and kept in the lane's LDS slot (`cache`).
template <typename H>
struct BloomBitSource {
  const H& x;
  uint16_t* cache;
  uint32_t have = 1;
  __device__ inline uint32_t operator()(uint32_t j, [[maybe_unused]] uint32_t k)
  {
    if constexpr (kBloomShared<H>) {
      return x.bit(j) & kBloomBitMask;
    } else {
      for (const uint32_t want = min(k, kMaxBloomHashes); have < want; ++have)
        cache[have] = (uint16_t)(x.bit(have) & kBloomBitMask);
      return (uint32_t)cache[min(j, kMaxBloomHashes - 1)];
    }
  }
};

// bloom_probe_item's test with the bit index of hash j supplied by the caller (a BloomBitSource).
template <bool kOpts, typename Ids, typename BitFn>
__device__ inline uint32_t bloom_entry_test(const uint8_t* __restrict__ filters,
                                            const tkv_amq_segment* __restrict__ segs, uint32_t n_segs,
                                            uint32_t leaf, uint64_t h0, Ids page_ids,
                                            uint32_t ent, BitFn&& bit_of)
{
  const ProbeDesc d = load_probe_desc(segs, leaf, n_segs);
  if (d.hash_count == 0) return 1u | (kNoFilter << 1);
  if constexpr (kOpts) {
    if (!page_id_matches(filters + d.out_offset, src_page_id_offset(TKV_AMQ_BLOOM), page_ids, ent)) return 1u | (kIdMismatch << 1);
  }
  const uint64_t* blk = reinterpret_cast<const uint64_t*>(filters + d.out_offset + kBloomHeader +
                                                          64 * bloom_block(h0, d.n_blocks));
  uint32_t b = (uint32_t)h0 & kBloomBitMask;
  uint32_t ok = (uint32_t)(blk[b >> 6] >> (b & 63));
  for (uint32_t j = 1; j < d.hash_count; ++j) {
    b = bit_of(j, d.hash_count);
    ok &= (uint32_t)(blk[b >> 6] >> (b & 63));
  }
  return (ok & 1u) | (kChecked << 1);
}

}  // namespace tkv
