// tkv_amq_scan.h -- the prefix sums of the device passes, once (device only).
//
//   block_exclusive_scan<T>  exclusive scan over a 256-thread workgroup: a shuffle scan inside each
//                            wave, the four wave sums through 4 words of LDS, two barriers
//   scan_totals<T>           one workgroup: per-workgroup totals to their exclusive prefixes
//   prefix_inclusive_u64<NT> one workgroup: the inclusive prefix of a u64 array in place
//
// The kernels have internal linkage: every unit of the library that includes this header
// registers and launches a copy of its own.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tkv {

constexpr uint32_t kBlockScanThreads = 256;
constexpr uint32_t kScanTotalsPerThread = 4;
constexpr uint32_t kScanTotalsSpan = kBlockScanThreads * kScanTotalsPerThread;  // totals per scan pass
constexpr uint32_t kPrefixThreads = 1024;  // the workgroup prefix_inclusive_u64 is launched with

// exclusive scan of v over the workgroup's 256 threads; *total = the sum.  s_waves: 4 words of
// LDS, free for the caller's next scan on return.
template <class T>
__device__ inline T block_exclusive_scan(T v, T* s_waves, T* total)
{
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T u = __shfl_up(inc, d, 64);
    if (lane >= (uint32_t)d) inc += u;
  }
  if (lane == 63) s_waves[wave] = inc;
  __syncthreads();
  const T w0 = s_waves[0], w1 = s_waves[1], w2 = s_waves[2], w3 = s_waves[3];
  __syncthreads();  // (s_waves is written again by the caller's next pass)
  *total = w0 + w1 + w2 + w3;
  const T wave_base = (wave > 0 ? w0 : T(0)) + (wave > 1 ? w1 : T(0)) + (wave > 2 ? w2 : T(0));
  return wave_base + inc - v;
}

namespace {

// One workgroup: totals[w] <- the sum of totals[w'] over w' < w, kScanTotalsSpan of them per pass
// with the running base carried over; *offsets_end <- min(total, capacity); *needed <- the total
// (either may be NULL).  n == 0: an empty batch, only the two words are written.
template <class T>
__global__ __launch_bounds__(kBlockScanThreads) void scan_totals(T* __restrict__ totals, uint32_t n,
                                                                 uint32_t* __restrict__ offsets_end,
                                                                 uint32_t capacity, uint64_t* __restrict__ needed)
{
  __shared__ T s[kBlockScanThreads / 64];
  const uint32_t tid = threadIdx.x;
  T base = 0;
  for (uint32_t p0 = 0; p0 < n; p0 += kScanTotalsSpan) {
    T v[kScanTotalsPerThread];
    T sum = 0;
#pragma unroll
    for (uint32_t r = 0; r < kScanTotalsPerThread; ++r) {
      const uint64_t w = (uint64_t)p0 + tid * kScanTotalsPerThread + r;
      v[r] = w < n ? totals[w] : T(0);
      sum += v[r];
    }
    T total;
    T run = base + block_exclusive_scan<T>(sum, s, &total);
#pragma unroll
    for (uint32_t r = 0; r < kScanTotalsPerThread; ++r) {
      const uint64_t w = (uint64_t)p0 + tid * kScanTotalsPerThread + r;
      if (w < n) totals[w] = run;
      run += v[r];
    }
    base += total;
  }
  if (tid == 0) {
    if (offsets_end) *offsets_end = (uint32_t)min((uint64_t)base, (uint64_t)capacity);
    if (needed) *needed = base;
  }
}

// in-place inclusive scan of v[0 .. n) by one workgroup of NT threads: a serial run per thread,
// the runs' sums scanned over the wave with shuffles, the waves' totals through LDS
template <uint32_t NT>
__global__ __launch_bounds__(NT) void prefix_inclusive_u64(uint64_t* __restrict__ v, uint32_t n)
{
  __shared__ uint64_t s_wave[NT / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t per = ((uint64_t)n + NT - 1) / NT;
  const uint64_t b = per * tid < n ? per * tid : n;
  const uint64_t e = b + per < n ? b + per : n;
  uint64_t sum = 0;
  for (uint64_t i = b; i < e; ++i) sum += v[i];
  uint64_t inc = sum;  // inclusive over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t up = __shfl_up(inc, o, 64);
    if ((int)lane >= o) inc += up;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint64_t run = inc - sum;
  for (uint32_t w = 0; w < wave; ++w) run += s_wave[w];
  for (uint64_t i = b; i < e; ++i) {
    run += v[i];
    v[i] = run;
  }
}

}  // namespace
}  // namespace tkv
