// tkv_amq_key_order.h -- the order of two keys, once: what the leaf search (tkv_amq_find.hip), the
// tree walk (tkv_amq_walk.hip) and the membership audit (tkv_amq_verify.h) agree on.
//
// Keys order as memcmp does, the shorter key first on a tie (std::string_view's order).  Read as
// big-endian words an unsigned integer compare is memcmp, so a query of a fixed 16 or 24 bytes is
// held that way in registers (OrderedQuery<kOrder16 | kOrder24>); any other shape is compared
// from memory (key_compare): 8 bytes at a time where both keys have them, then 4, then bytes,
// then the lengths -- never past a key's end.
// Plain functions, shared by the kernels, the entry points' mode choice and tests/cpp.
#pragma once

#include <stdint.h>

#include "tkv_amq.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TKV_ORDER_FN __host__ __device__ inline
#else
#define TKV_ORDER_FN inline
#endif

namespace tkv {

// Unaligned global loads: gfx950 (HSA, unaligned access mode) serves a dwordx2 / dword load
// at any byte address; memcpy from a byte pointer compiles to exactly that
// (tools/probe/unaligned_load.hip checks every byte offset on the device).
TKV_ORDER_FN uint64_t ld64_unaligned(const uint8_t* p)
{
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

TKV_ORDER_FN uint32_t ld32_unaligned(const uint8_t* p)
{
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// two little-endian words of a key as one big-endian u64
TKV_ORDER_FN uint64_t be64(uint32_t lo, uint32_t hi) { return __builtin_bswap64(((uint64_t)hi << 32) | lo); }

// memcmp order, then the shorter key first (std::string_view's): < 0, 0, > 0 for k <, ==, > q
TKV_ORDER_FN int key_compare(const uint8_t* k, uint32_t klen, const uint8_t* q, uint32_t qlen)
{
  const uint32_t n = klen < qlen ? klen : qlen;
  uint32_t o = 0;
  for (; o + 8 <= n; o += 8) {
    const uint64_t x = ld64_unaligned(k + o), y = ld64_unaligned(q + o);
    if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
  }
  if (o + 4 <= n) {
    const uint32_t x = ld32_unaligned(k + o), y = ld32_unaligned(q + o);
    if (x != y) return __builtin_bswap32(x) < __builtin_bswap32(y) ? -1 : 1;
    o += 4;
  }
  for (; o < n; ++o) {
    const uint32_t x = k[o], y = q[o];
    if (x != y) return x < y ? -1 : 1;
  }
  return klen < qlen ? -1 : (klen > qlen ? 1 : 0);
}

// An array of keys: offsets form (key i is bytes [offsets[i], offsets[i + 1]) of base) or, with
// offsets == NULL, stride form (key i is the `stride` bytes at base + i * stride).
struct KeyArray {
  const uint8_t* base;
  const uint64_t* offsets;
  uint32_t stride;
  TKV_ORDER_FN void at(uint64_t i, const uint8_t*& p, uint32_t& len) const
  {
    if (offsets) {
      const uint64_t b = offsets[i];
      p = base + b;
      len = (uint32_t)(offsets[i + 1] - b);
    } else {
      p = base + i * stride;
      len = stride;
    }
  }
};

// kOrder16: both sides fixed 16-byte keys, 16-byte aligned; kOrder24: both fixed 24-byte keys,
// 8-byte aligned; kOrderAny: everything else (other strides, offsets on either side, misaligned)
enum KeyOrderMode : int { kOrder16 = 0, kOrder24 = 1, kOrderAny = 2 };

// (host side: the entry points choose the kernel with it; static, so the library exports nothing new)
// Over a table of n >= 1 arrays any of which may be searched for a key of any other: the fixed modes
// only when every one of them qualifies.
static inline KeyOrderMode key_order_mode(const KeyArray* ks, uint32_t n)
{
  bool fixed = true;
  uintptr_t all = 0;
  for (uint32_t i = 0; i < n; ++i) {
    fixed = fixed && !ks[i].offsets && ks[i].stride == ks[0].stride;
    all |= reinterpret_cast<uintptr_t>(ks[i].base);
  }
  return fixed && ks[0].stride == 16 && !(all & 15) ? kOrder16 : fixed && ks[0].stride == 24 && !(all & 7) ? kOrder24 : kOrderAny;
}

static inline KeyOrderMode key_order_mode(const KeyArray& q, const KeyArray& k)
{
  const KeyArray both[2] = {q, k};
  return key_order_mode(both, 2);
}

// The query of one lane (key i of `qs`), and its order against key i of an array of the same mode.
template <int MODE>
struct OrderedQuery;

template <>
struct OrderedQuery<kOrder16> {
#if defined(__HIPCC__) || defined(__CUDACC__)
  typedef uint4 Quad;
#else
  struct alignas(16) Quad { uint32_t x, y, z, w; };
#endif
  uint64_t w0, w1;
  // one global_load_dwordx4, two u64 compares
  TKV_ORDER_FN static void load(const uint8_t* base, uint64_t i, uint64_t& k0, uint64_t& k1)
  {
    const Quad v = *reinterpret_cast<const Quad*>(base + 16 * i);
    k0 = be64(v.x, v.y);
    k1 = be64(v.z, v.w);
  }
  TKV_ORDER_FN OrderedQuery(const KeyArray& qs, uint64_t i) { load(qs.base, i, w0, w1); }
  TKV_ORDER_FN bool less(const KeyArray& ks, uint64_t i) const
  {
    uint64_t k0, k1;
    load(ks.base, i, k0, k1);
    return k0 < w0 || (k0 == w0 && k1 < w1);
  }
  TKV_ORDER_FN bool less_equal(const KeyArray& ks, uint64_t i) const
  {
    uint64_t k0, k1;
    load(ks.base, i, k0, k1);
    return k0 < w0 || (k0 == w0 && k1 <= w1);
  }
  TKV_ORDER_FN bool equal(const KeyArray& ks, uint64_t i) const
  {
    uint64_t k0, k1;
    load(ks.base, i, k0, k1);
    return k0 == w0 && k1 == w1;
  }
};

template <>
struct OrderedQuery<kOrder24> {
  uint64_t w0, w1, w2;
  TKV_ORDER_FN OrderedQuery(const KeyArray& qs, uint64_t i)
  {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(qs.base + 24 * i);
    w0 = __builtin_bswap64(p[0]);
    w1 = __builtin_bswap64(p[1]);
    w2 = __builtin_bswap64(p[2]);
  }
  TKV_ORDER_FN bool less(const KeyArray& ks, uint64_t i) const
  {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(ks.base + 24 * i);
    const uint64_t k0 = __builtin_bswap64(p[0]), k1 = __builtin_bswap64(p[1]), k2 = __builtin_bswap64(p[2]);
    return k0 < w0 || (k0 == w0 && (k1 < w1 || (k1 == w1 && k2 < w2)));
  }
  TKV_ORDER_FN bool less_equal(const KeyArray& ks, uint64_t i) const
  {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(ks.base + 24 * i);
    const uint64_t k0 = __builtin_bswap64(p[0]), k1 = __builtin_bswap64(p[1]), k2 = __builtin_bswap64(p[2]);
    return k0 < w0 || (k0 == w0 && (k1 < w1 || (k1 == w1 && k2 <= w2)));
  }
  TKV_ORDER_FN bool equal(const KeyArray& ks, uint64_t i) const
  {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(ks.base + 24 * i);
    return __builtin_bswap64(p[0]) == w0 && __builtin_bswap64(p[1]) == w1 && __builtin_bswap64(p[2]) == w2;
  }
};

template <>
struct OrderedQuery<kOrderAny> {
  const uint8_t* p;
  uint32_t len;
  TKV_ORDER_FN OrderedQuery(const KeyArray& qs, uint64_t i) { qs.at(i, p, len); }
  TKV_ORDER_FN int compare(const KeyArray& ks, uint64_t i) const
  {
    const uint8_t* k;
    uint32_t klen;
    ks.at(i, k, klen);
    return key_compare(k, klen, p, len);
  }
  TKV_ORDER_FN bool less(const KeyArray& ks, uint64_t i) const { return compare(ks, i) < 0; }
  TKV_ORDER_FN bool less_equal(const KeyArray& ks, uint64_t i) const { return compare(ks, i) <= 0; }
  TKV_ORDER_FN bool equal(const KeyArray& ks, uint64_t i) const { return compare(ks, i) == 0; }
};

// The first index of [first, first + len) at which pred is false; pred must be true on a prefix of
// the range and false after it (less: std::lower_bound; less_equal: std::upper_bound).
// Branch-free: lanes with ranges of equal length take the same trip count.
template <class Len, class Pred>
TKV_ORDER_FN uint64_t bound(uint64_t first, Len len, Pred pred)
{
  uint64_t b = first;
  while (len > 1) {
    const Len half = len >> 1;
    b += pred(b + half - 1) ? half : 0;
    len -= half;
  }
  if (len == 1) b += pred(b) ? 1 : 0;
  return b;
}

// keys [b, e) of leaf `leaf`, whose segment is *g (in the segment array, or a caller's loaded
// copy), from the CSR key_begin [n + 1] or, with key_begin == NULL, from the segment's key_begin /
// n_keys: both ends clamped to n_keys, an end below its begin reads as empty
TKV_ORDER_FN void segment_key_range(const uint64_t* key_begin, const tkv_amq_segment* g, uint32_t leaf,
                                    uint64_t n_keys, uint64_t& b, uint64_t& e)
{
  uint64_t lo, hi;
  if (key_begin) {
    lo = key_begin[leaf];
    hi = key_begin[leaf + 1];
  } else {
    lo = g->key_begin;
    hi = lo + g->n_keys;
    if (hi < lo) hi = ~0ull;
  }
  b = lo < n_keys ? lo : n_keys;
  e = hi < n_keys ? hi : n_keys;
  if (e < b) e = b;
}

// the same with the leaf's segment in its array (leaf < the segment count)
TKV_ORDER_FN void leaf_key_range(const uint64_t* key_begin, const tkv_amq_segment* segs, uint32_t leaf,
                                 uint64_t n_keys, uint64_t& b, uint64_t& e)
{
  segment_key_range(key_begin, segs + leaf, leaf, n_keys, b, e);
}

}  // namespace tkv
