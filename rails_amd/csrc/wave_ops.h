// Sums and prefix sums over a 64-lane wave and over a workgroup, shared by topk.hip, collapse.hip, mmr.hip, item_mask.hip, rank.hip and softmax.hip.
// Device-only; no atomics and no LDS of its own: the workgroup forms take their scratch from the caller.
#pragma once
#include <hip/hip_runtime.h>

namespace mol {

// Sum over the wave, returned to every lane (T: int, unsigned int, double).  An xor butterfly with d = 32, 16, ..., 1: every lane ends with
// the same bits, in an order fixed by the lane ids -- the float64 partial sums of scores_lse_sum_kernel depend on that order.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// Maximum over the wave, returned to every lane (T: any type ordered by >; the 64-bit keys of topk_keys.h).  The same butterfly.
template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const T u = __shfl_xor(v, d, 64);
    v = u > v ? u : v;
  }
  return v;
}

// Inclusive prefix sum over the wave in lane order (T: int, unsigned int); lane 63 holds the wave's sum.
template <class T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// Exclusive prefix sum over the workgroup in thread order; `total`: the workgroup's sum.  All NT threads call; `totals` is LDS of NT / 64
// ints.  Write, barrier, read, barrier: the scratch may be reused at once on return.
template <int NT>
__device__ __forceinline__ int block_scan_excl(int v, int* totals, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int inc = wave_scan_incl(v, lane);
  if (lane == 63) totals[wave] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int t = totals[w];
    if (w < wave) base += t;
    total += t;
  }
  __syncthreads();
  return base + inc - v;
}

// The max form of the scan: the maximum of v over the threads BEFORE this one in thread order, `lowest` for thread 0 (and wherever every
// earlier thread holds `lowest`).  The same calling rules and scratch as block_scan_excl.
template <int NT>
__device__ __forceinline__ int block_scan_max_excl(int v, int lowest, int* totals) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o && u > inc) inc = u;
  }
  if (lane == 63) totals[wave] = inc;
  const int before = __shfl_up(inc, 1, 64);      // the wave's lanes below this one
  __syncthreads();
  int base = lane > 0 ? before : lowest;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int t = totals[w];
    if (w < wave && t > base) base = t;
  }
  __syncthreads();
  return base;
}

// Sum over the workgroup, returned to every thread.  All NT threads call; `part` is LDS of NT / 64 ints.  The same sequence as the scan.
template <int NT>
__device__ __forceinline__ int block_sum(int v, int* part) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) s += part[w];
  __syncthreads();
  return s;
}

}  // namespace mol
