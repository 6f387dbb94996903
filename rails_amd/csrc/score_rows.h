// The masked walk over the rows of a (rows, n) fp32 score matrix shared by rank.hip and softmax.hip, and the host helpers of the row kernels.
//
// Grid (column chunks, rows), kRowWalkThreads threads: a workgroup streams its chunk of ONE row -- kRowWalkIters 16-byte loads per thread
// over the aligned middle of the row, the ragged head and tail peeled onto chunk 0 --; grid-y loops over the rows.  With a mask (rows of
// ceil(n / 32) 32-bit words, item_mask.hip) every element arrives with its bit.  No atomics, no fast-math intrinsics, no LDS; every index is
// tested against n before it is used.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mol_kernels.h"

namespace mol {

constexpr int kRowWalkThreads = 256;
constexpr int kRowWalkIters = 4;                                               // 16-byte loads per thread
constexpr int64_t kRowWalkChunkVecs = (int64_t)kRowWalkThreads * kRowWalkIters;      // 1 024 float4 = 4 096 columns per workgroup

// ---- host ----
inline unsigned grid_for(int64_t blocks) { return (unsigned)(blocks < 1 ? 1 : blocks > 65536 ? 65536 : blocks); }
inline int launched() { return hipGetLastError() == hipSuccess ? kOk : kErrLaunch; }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int64_t chunks_of(int64_t n) { return ((n + 3) / 4 + kRowWalkChunkVecs - 1) / kRowWalkChunkVecs; }      // (a row's aligned middle holds at most n / 4 float4)
inline dim3 row_grid(int rows, int64_t n) { return dim3((unsigned)chunks_of(n), (unsigned)(rows < 65535 ? rows : 65535)); }      // (the kernels loop over grid-y)

// the masked or the unmasked instantiation of a row kernel, by whether the call carries mask words
template <class... P, class... A>
inline void launch_masked(const void* words, void (*masked)(P...), void (*plain)(P...), dim3 grid, hipStream_t stream, A... args) {
  hipLaunchKernelGGL(words != nullptr ? masked : plain, grid, dim3(kRowWalkThreads), 0, stream, args...);
}

// ---- device ----
// a row as head + q aligned float4 + tail
struct RowShape {
  int64_t head, q, tail0;
};

__device__ __forceinline__ RowShape row_shape(const float* srow, int64_t n) {
  const int64_t lead = (int64_t)((4u - (unsigned int)(((uintptr_t)srow >> 2) & 3u)) & 3u);
  RowShape s;
  s.head = lead < n ? lead : n;
  s.q = (n - s.head) >> 2;
  s.tail0 = s.head + 4 * s.q;
  return s;
}

// the mask bits of the four columns from x0, for the wave whose first column is xw (256 consecutive columns: at most 9 mask words, one load
// per word, handed to the lanes by shuffles); every lane of the wave calls it
__device__ __forceinline__ unsigned int wave_mask_bits(const unsigned int* mrow, int64_t n_words, int64_t xw, int64_t x0, int lane) {
  const int64_t wi = (xw >> 5) + lane;
  const unsigned int wv = lane < 10 && wi < n_words ? mrow[wi] : 0u;
  const int rel = (int)((x0 >> 5) - (xw >> 5));
  const unsigned int lo = __shfl(wv, rel, 64), hi = __shfl(wv, rel + 1, 64);
  return (unsigned int)((((unsigned long long)hi << 32) | lo) >> (int)(x0 & 31)) & 0xFu;
}

__device__ __forceinline__ bool mask_bit(const unsigned int* mrow, int64_t x) { return ((mrow[x >> 5] >> (int)(x & 31)) & 1u) != 0u; }

// The workgroup's chunk (blockIdx.x) of the row srow[0, n): quad(x0, s, bits) for every aligned float4 s = srow[x0 .. x0 + 3] of the chunk,
// bit i of `bits` set iff column x0 + i is eligible; edge(x, srow[x], eligible) for the head and tail columns, on chunk 0 by threads 0..7.
// All kRowWalkThreads threads call it; mrow / n_words are not read unless MASKED.
template <bool MASKED, class Quad, class Edge>
__device__ __forceinline__ void for_row_chunk(const float* srow, int64_t n, const unsigned int* mrow, int64_t n_words, Quad quad, Edge edge) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RowShape rs = row_shape(srow, n);
  const int64_t v0 = (int64_t)blockIdx.x * kRowWalkChunkVecs;
#pragma unroll
  for (int it = 0; it < kRowWalkIters; ++it) {
    const int64_t vw = v0 + (int64_t)it * kRowWalkThreads + wave * 64;      // the wave's first float4: 256 consecutive columns from xw
    if (vw >= rs.q) break;                                                  // (wave-uniform)
    const int64_t v = vw + lane;
    const int64_t xw = rs.head + 4 * vw, x0 = rs.head + 4 * v;
    const unsigned int bits = MASKED ? wave_mask_bits(mrow, n_words, xw, x0, lane) : 0xFu;
    if (v < rs.q) quad(x0, *reinterpret_cast<const float4*>(srow + x0), bits);
  }
  if (blockIdx.x == 0 && tid < 8) {      // the peeled head (threads 0..3) and tail (threads 4..7): at most 3 columns each
    const int64_t x = tid < 4 ? tid : rs.tail0 + (tid - 4);
    if (tid < 4 ? x < rs.head : x < n) edge(x, srow[x], !MASKED || mask_bit(mrow, x));
  }
}

}  // namespace mol
