// tkv_amq_hash.h -- the key shapes and the Bloom hashers that the builds and the probes share
// (device only; DESIGN.md sections 3.1 and 4).
//
//   c_bloom                 the seed table every Bloom hasher reads
//   KeyMode, key_at, hash_key, load_nt16
//                           a key array's shape, key i's bytes and its XXH64
//   Bloom16 / BloomFixed<L> / BloomShort / BloomLong
//                           one hasher per key shape: h0() and bit(j)
//   bloom_ladder, bloom_fill_bits, bloom_h0_at, with_bloom_key_at
//                           the one loop over a key's hashes, and the short / long dispatch
//
// Included by tkv_amq_probe.h and tkv_amq_launch.h, and so by tkv_amq_kernels.hip (the builds
// and tkv_amq_verify.h) and tkv_amq_read.hip (the probes and the lookups).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include <stdint.h>

#include "tkv_amq_device.h"

namespace tkv {

// ---------------------------------------------------------------------------------------
// constant tables
// ---------------------------------------------------------------------------------------
struct BloomSeeds {
  uint64_t seed[kMaxBloomHashes];
  uint64_t rhinit16[kMaxBloomHashes];  // rotl(seed + P5 + 16, 27), see Xxh16
  uint64_t seed_p5[kMaxBloomHashes];   // seed + P5, see XxhShort
};

constexpr BloomSeeds make_bloom_seeds()
{
  BloomSeeds t{};
  for (uint32_t i = 0; i < kMaxBloomHashes; ++i) {
    t.seed[i] = bloom_seed(i);
    t.rhinit16[i] = xxh16_rhinit(t.seed[i]);
    t.seed_p5[i] = t.seed[i] + kP5;
  }
  return t;
}

// constant-initialised at load: no host upload, so every entry point is graph-capturable
// `inline` (C++17), so that every unit that includes this header sees one table with external
// linkage, as when a single unit defined it.  Linkage decides the code: with internal linkage
// (`static`, with or without `used`) the compiler folds the seeds into the instructions and 83
// of the 169 kernels compile differently (bloom_probe<0,false> 744 -> 675 instructions,
// bloom_build_lds<1,*> 63 -> 70 VGPRs, bloom_probe<1,true> 60 -> 68 VGPRs); `inline` and
// `__attribute__((weak))` change none (profiles/read_unit/README.md).
inline __constant__ BloomSeeds c_bloom = make_bloom_seeds();

// ---------------------------------------------------------------------------------------
// key access
// ---------------------------------------------------------------------------------------
// kKey24: fixed 24-byte keys, 8-byte aligned (Bloom build fast path; other kernels hash them
// through the generic fixed-stride path)
// kKeyLoc: not a key shape -- the small-batch VQF path's located keys (vqf_locate_keys writes
// one 8-byte record per key: vqf_loc_encode), read by vqf_ring_place in place of the keys
enum KeyMode : int { kKey16 = 0, kKeyFixed = 1, kKeyVar = 2, kKey24 = 3, kKeyLoc = 4 };

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// streaming (non-temporal) loads/stores for data touched exactly once, so it does not
// evict reused data (the probe's filter array) from L2 / the Infinity Cache
__device__ inline uint4 load_nt16(const void* p)
{
  const u32x4_t v = __builtin_nontemporal_load(static_cast<const u32x4_t*>(p));
  return uint4{v.x, v.y, v.z, v.w};
}

// key i of a fixed-stride or offset-indexed key array: its bytes and length
template <int MODE>
__device__ inline const uint8_t* key_at(const uint8_t* keys, const uint64_t* offs, uint32_t stride,
                                        uint64_t i, uint32_t& len)
{
  if constexpr (MODE == kKeyFixed || MODE == kKey24) {
    len = stride;
    return keys + i * stride;
  } else {
    const uint64_t b = offs[i];
    len = (uint32_t)(offs[i + 1] - b);
    return keys + b;
  }
}

template <int MODE>
__device__ inline uint64_t hash_key(const uint8_t* keys, const uint64_t* offs, uint32_t stride,
                                    uint64_t i, uint64_t seed)
{
  uint32_t len;
  const uint8_t* p = key_at<MODE>(keys, offs, stride, i, len);
  if (len < 32) return XxhShort(p, len).finish(seed + kP5);
  return xxh64_bytes(p, len, seed);
}

// ---- Bloom hash in device code: the frozen spec, down to bloom_h0_at, and nowhere else ----
// A Bloom hasher is a key shape's XXH64 state paired with its column of the seed table.  h0():
// the 64-bit hash for seed 0 (block = bloom_block(h0, n_blocks), bit 0 = h0 & kBloomBitMask).
// bit(j): a value whose low 9 bits are bit index j; ITS HIGH BITS ARE UNSPECIFIED: lds_set_bit
// ignores them, every other consumer masks with kBloomBitMask where it takes the value.
// kBloomShared: seed-independent work is done once per key, so a compile-time hash count is
// unrolled; a long key always loops.  The helpers are always_inline: a site compiles as code in place.
constexpr uint32_t kBloomBitMask = 511u;
#define TKV_INLINE __device__ __attribute__((always_inline)) inline

TKV_INLINE uint64_t bloom_block(uint64_t h0, uint32_t n_blocks) { return __umul64hi(h0, (uint64_t)n_blocks); }

struct Bloom16 : Xxh16 {  // 16-byte keys
  TKV_INLINE explicit Bloom16(const uint4& v) : Xxh16((uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32)) {}
  TKV_INLINE Bloom16() : Xxh16() {}  // a state moved between lanes or parked: set rk1, k2
  TKV_INLINE uint64_t h0() const { return finish(c_bloom.rhinit16[0]); }
  TKV_INLINE uint32_t bit(uint32_t j) const { return finish_lo9(c_bloom.rhinit16[j]); }
};

template <int L>
struct BloomFixed : XxhFixed<L> {  // L-byte keys, 8-byte aligned
  TKV_INLINE explicit BloomFixed(const uint64_t (&lanes)[L / 8]) : XxhFixed<L>(lanes) {}
  TKV_INLINE BloomFixed() : XxhFixed<L>() {}  // a moved state: set rk0, k[]
  TKV_INLINE uint64_t h0() const { return this->finish(xxh_fixed_rc<L>(c_bloom.seed[0])); }
  TKV_INLINE uint32_t bit(uint32_t j) const { return this->finish_lo9(xxh_fixed_rc<L>(c_bloom.seed[j])); }
};

struct BloomShort : XxhShort {  // any key under 32 bytes
  using XxhShort::XxhShort;
  TKV_INLINE uint64_t h0() const { return finish(c_bloom.seed_p5[0]); }
  TKV_INLINE uint32_t bit(uint32_t j) const { return finish_lo9(c_bloom.seed_p5[j]); }
};

struct BloomLong {  // 32 bytes and more: every hash reads the whole key
  const uint8_t* p;
  uint64_t len;  // (64-bit, as xxh64_bytes takes it)
  TKV_INLINE uint64_t h0() const { return xxh64_bytes(p, len, c_bloom.seed[0]); }
  TKV_INLINE uint32_t bit(uint32_t j) const { return (uint32_t)xxh64_bytes(p, len, c_bloom.seed[j]); }
};

template <typename H>
constexpr bool kBloomShared = !std::is_same_v<H, BloomLong>;

// The one ladder: sink(j, bit(j)) for j = 1 .. k - 1.  K != 0: the hash count at compile time
// (7 / 8, the counts at 10 / 12 bits per key), unrolled; K == 0: the run-time k.
template <int K, typename H, typename Sink>
TKV_INLINE void bloom_ladder(const H& x, uint32_t k, Sink&& sink)
{
  if constexpr (K != 0 && kBloomShared<H>) {
#pragma unroll
    for (uint32_t j = 1; j < (uint32_t)K; ++j) sink(j, x.bit(j));
  } else {
    for (uint32_t j = 1; j < k; ++j) sink(j, x.bit(j));
  }
}

// A record's NB (8, or a wide record's 16) bit indices: hash j below the hash count, else the
// padding, b_0 in the first record and b_8 in the second.  K as in bloom_ladder.
template <int K, int NB, typename H>
TKV_INLINE void bloom_fill_bits(const H& x, uint64_t h0, uint32_t k, uint32_t (&b)[NB])
{
  b[0] = (uint32_t)h0 & kBloomBitMask;
  auto fill = [&](uint32_t j) {
    return (K != 0 ? j < (uint32_t)K : j < k) ? x.bit(j) & kBloomBitMask : b[j <= 8 ? 0 : 8];
  };
  if constexpr (kBloomShared<H>) {
#pragma unroll
    for (uint32_t j = 1; j < (uint32_t)NB; ++j) b[j] = fill(j);
  } else {
    for (uint32_t j = 1; j < (uint32_t)NB; ++j) b[j] = fill(j);
  }
}

// Key i's seed-0 hash as hash_key finishes it: a short key with seed[0] + P5, where BloomShort
// reads seed_p5[0] (the same value; the window build keeps hash_key's instructions).
template <int MODE>
TKV_INLINE uint64_t bloom_h0_at(const uint8_t* keys, const uint64_t* offs, uint32_t stride, uint64_t i)
{ return hash_key<MODE>(keys, offs, stride, i, c_bloom.seed[0]); }

// The short/long dispatch of a generic key shape: f(the hasher that matches key i's length)
template <int MODE, typename F>
TKV_INLINE auto with_bloom_key_at(const uint8_t* keys, const uint64_t* offs, uint32_t stride, uint64_t i, F&& f)
{
  uint32_t len;
  const uint8_t* p = key_at<MODE>(keys, offs, stride, i, len);
  if (len < 32) return f(BloomShort(p, len));
  return f(BloomLong{p, len});
}

}  // namespace tkv
