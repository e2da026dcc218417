// tkv_amq_value.h -- a packed value array and how an item's bytes and integer are read from it,
// once: what tkv_amq_get_values / tkv_amq_gather_values (tkv_amq_read.hip) and the leaf merge
// (tkv_amq_merge.hip) agree on.  Device only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tkv {

struct ValueArray {
  const uint8_t* values;
  const uint64_t* offs;  // n_keys + 1 entries, or null: the fixed form
  uint32_t stride;
  uint64_t bytes;
};

// Item i's bytes [b, e), both ends clamped to the buffer, e >= b.
__device__ inline void value_range(const ValueArray& v, uint64_t i, uint64_t& b, uint64_t& e)
{
  if (v.offs) {
    b = min(v.offs[i], v.bytes);
    e = max(min(v.offs[i + 1], v.bytes), b);
  } else {
    // (a product past 2^64 lies past any buffer)
    b = __umul64hi(i, v.stride) ? v.bytes : min(i * v.stride, v.bytes);
    e = v.bytes - b < v.stride ? v.bytes : b + v.stride;
  }
}

// as_i32() of n data bytes at p (core/value_view.hpp:248-262): 0 bytes: 0; 1..3: the sign-extended
// little-endian integer; 4 and more: the first four.  Byte loads: values start at any address and
// an item is read once per hit.
__device__ inline uint32_t value_i32(const uint8_t* p, uint64_t n)
{
  const uint32_t m = n < 4 ? (uint32_t)n : 4u;
  uint32_t x = 0;
  for (uint32_t j = 0; j < m; ++j) x |= (uint32_t)p[j] << (8 * j);
  const uint32_t sh = 32 - 8 * m;
  return m == 0 ? 0u : (uint32_t)((int32_t)(x << sh) >> sh);
}

}  // namespace tkv
