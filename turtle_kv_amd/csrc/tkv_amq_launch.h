// tkv_amq_launch.h -- the host helpers that the entry points of more than one unit use: a key
// array's shape as a run-time and as a compile-time value, the probe options, grid sizes.
//
// Everything here has internal linkage: every unit that includes this header has its own copy, as
// with the kernels of tkv_amq_scan.h.  Included by tkv_amq_kernels.hip and tkv_amq_read.hip; the
// key shapes (KeyMode) come from tkv_amq_hash.h.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include <stdint.h>

#include "tkv_amq.h"
#include "tkv_amq_hash.h"

namespace tkv {
namespace {

inline uint64_t div_up(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// The runtime key shape as a compile-time constant: fn(std::integral_constant<int, MODE>).
// with_key_mode: key_mode's three shapes (probes, hashes); with_build_key_mode: build_key_mode's
// four (kKey24 besides).
template <int M>
using KeyModeC = std::integral_constant<int, M>;

template <typename Fn>
inline void with_key_mode(int mode, Fn&& fn)
{
  if (mode == kKey16) fn(KeyModeC<kKey16>{});
  else if (mode == kKeyFixed) fn(KeyModeC<kKeyFixed>{});
  else fn(KeyModeC<kKeyVar>{});
}

// a launch with or without probe options (the kernels' kOpts)
template <typename Fn>
inline void with_flag(bool on, Fn&& fn)
{
  if (on) fn(std::true_type{});
  else fn(std::false_type{});
}

inline int key_mode_of(bool var, uint32_t stride)
{
  if (var) return kKeyVar;
  return stride == 16 ? kKey16 : kKeyFixed;
}

inline int key_mode(const uint64_t* offs, uint32_t stride) { return key_mode_of(offs != nullptr, stride); }

inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }

inline tkv_amq_probe_opts probe_opts(const tkv_amq_probe_opts* o)
{
  tkv_amq_probe_opts r{nullptr, nullptr, nullptr};
  return o ? *o : r;
}

inline bool probe_opts_used(const tkv_amq_probe_opts& o)
{
  return o.d_query_page_id || o.d_truth || o.d_metrics;
}

// plain probes: one lane per query; with options: a grid-stride loop over a bounded grid, so
// the metrics take one atomic per counter per wave (8 waves per SIMD)
inline uint32_t probe_grid(uint64_t n, bool ex)
{
  const uint64_t g = (n + 255) / 256;
  const uint64_t cap = ex ? 8192 : 0xffffffffull;
  return (uint32_t)(g < cap ? g : cap);
}

}  // namespace
}  // namespace tkv
