// Exact ranks of given items (rails_scores_rank_keys, rails_scores_rank, rails_item_mask_clear_rows).
//
// rank(r, j) = 1 + #{ eligible y : key(r, y) > key(r, target j) } under the selection key of topk_keys.h, so rank - 1 is the index at which the
// target stands in the row's exhaustive top-k list (score descending, then position ascending; +-0, +-inf and NaN payloads by their bits).
//   keys    positions -> the targets' own keys, read from the matrix that is counted; key 0 (below every real key) for a position outside [0, n)
//   count   grid (column chunks, rows): a workgroup streams its slice of ONE score row once for all t targets of the row (the masked row
//           walk of score_rows.h), builds each element's key (0 where its mask bit is clear: such a key exceeds no target's), compares it
//           with the row's t target keys held in LDS and counts per lane in registers (tiers of t as a template parameter: every counter
//           index is a compile-time constant); wave sum (wave_ops.h), LDS sum over the workgroup, then one integer atomic per (workgroup,
//           target).  Integer adds commute: the result is the same bits whatever the arrival order.
//   finish  counts -> ranks: counts + 1 where the target's key is a real one and its own mask bit is set, else 0
// Plain launches on one stream (zero, count, finish); plain C++ with vector stores; every index is tested against n before it is used.
#include <hip/hip_runtime.h>

#include "mol_kernels.h"
#include "score_rows.h"
#include "topk_keys.h"
#include "wave_ops.h"

namespace mol {

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kThreads = kRowWalkThreads;
constexpr u64 kNoTarget = ~0ull;                            // pads a tier's unused key slots: no key exceeds it

// four element keys against the row's T target keys: each target key is read from LDS once (a broadcast read) per call
template <int T>
__device__ __forceinline__ void count_elements(u64 e0, u64 e1, u64 e2, u64 e3, const u64* tk, int (&cnt)[T]) {
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const u64 k = tk[j];
    cnt[j] += (e0 > k ? 1 : 0) + (e1 > k ? 1 : 0) + (e2 > k ? 1 : 0) + (e3 > k ? 1 : 0);
  }
}

}  // namespace

__global__ void scores_rank_keys_kernel(const float* __restrict__ scores, int64_t ld, int64_t n, const int64_t* __restrict__ positions, int64_t total, int t,
                                        u64* __restrict__ keys_out) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = positions[u];
    keys_out[u] = p >= 0 && p < n ? make_key(scores[(u / t) * ld + p], (u32)p) : 0ull;
  }
}

template <int T, bool MASKED>
__global__ void __launch_bounds__(kThreads) scores_rank_kernel(const float* __restrict__ scores, int64_t ld, int rows, int64_t n, const u64* __restrict__ keys,
                                                              int t, const u32* __restrict__ words, int64_t words_row_stride, int64_t n_words,
                                                              int32_t* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) u64 tk[T];
  __shared__ int total[T];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const float* srow = scores + row * ld;
    const u32* mrow = MASKED ? words + row * words_row_stride : nullptr;
    if (tid < T) {
      tk[tid] = tid < t ? keys[row * t + tid] : kNoTarget;
      total[tid] = 0;
    }
    __syncthreads();
    int cnt[T];
#pragma unroll
    for (int j = 0; j < T; ++j) cnt[j] = 0;
    for_row_chunk<MASKED>(
        srow, n, mrow, n_words,
        [&](int64_t x0, float4 s, u32 bits) {
          const u32 p = (u32)x0;
          count_elements<T>((bits & 1u) ? make_key(s.x, p) : 0ull, (bits & 2u) ? make_key(s.y, p + 1) : 0ull, (bits & 4u) ? make_key(s.z, p + 2) : 0ull,
                            (bits & 8u) ? make_key(s.w, p + 3) : 0ull, tk, cnt);
        },
        [&](int64_t x, float s, bool keep) { count_elements<T>(keep ? make_key(s, (u32)x) : 0ull, 0ull, 0ull, 0ull, tk, cnt); });      // (key 0 exceeds no target's)
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const int s = wave_sum(cnt[j]);
      if (lane == 0 && s != 0) atomicAdd(&total[j], s);
    }
    __syncthreads();
    if (tid < t && total[tid] != 0) atomicAdd(counts + row * t + tid, total[tid]);
    __syncthreads();      // (tk / total are rewritten for the next row)
  }
}

// in place: the counts of scores_rank_kernel -> ranks
__global__ void scores_rank_finish_kernel(const u64* __restrict__ keys, int64_t total, int t, int64_t n, const u32* __restrict__ words, int64_t words_row_stride,
                                          int32_t* __restrict__ ranks) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    const u64 key = keys[u];
    const int64_t p = (int64_t)key_pos(key);
    bool ranked = key != 0ull && p < n;
    if (ranked && words != nullptr) ranked = mask_bit(words + (u / t) * words_row_stride, p);
    ranks[u] = ranked ? ranks[u] + 1 : 0;
  }
}

// (named apart from the item_mask_* kernels: tests/test_item_mask_cpu.py pins that family's list)
__global__ void mask_rows_clear_kernel(const int64_t* __restrict__ positions, int64_t total, int64_t m, int64_t n, u32* __restrict__ words,
                                       int64_t words_row_stride) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = positions[u];
    if (p >= 0 && p < n) atomicAnd(words + (u / m) * words_row_stride + (p >> 5), ~(1u << (int)(p & 31)));
  }
}

int scores_rank_keys(const float* scores, int64_t ld, int rows, int64_t n, const int64_t* positions, int t, void* keys_out, hipStream_t stream) {
  const int64_t total = (int64_t)rows * t;
  hipLaunchKernelGGL(scores_rank_keys_kernel, dim3(grid_for((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, scores, ld, n, positions, total, t,
                     (u64*)keys_out);
  return launched();
}

template <int T>
static void launch_count(dim3 grid, const float* scores, int64_t ld, int rows, int64_t n, const u64* keys, int t, const u32* words, int64_t stride,
                         int32_t* counts, hipStream_t stream) {
  launch_masked(words, scores_rank_kernel<T, true>, scores_rank_kernel<T, false>, grid, stream, scores, ld, rows, n, keys, t, words, stride, item_mask_words(n),
                counts);
}

int scores_rank(const float* scores, int64_t ld, int rows, int64_t n, const void* keys, int t, const void* mask_words, int64_t words_row_stride,
                int32_t* ranks_out, hipStream_t stream) {
  const int64_t total = (int64_t)rows * t;
  if (hipMemsetAsync(ranks_out, 0, (size_t)total * sizeof(int32_t), stream) != hipSuccess) return kErrLaunch;
  const dim3 grid = row_grid(rows, n);
  const u64* k = (const u64*)keys;
  const u32* w = (const u32*)mask_words;
  if (t <= 1) launch_count<1>(grid, scores, ld, rows, n, k, t, w, words_row_stride, ranks_out, stream);
  else if (t <= 4) launch_count<4>(grid, scores, ld, rows, n, k, t, w, words_row_stride, ranks_out, stream);
  else if (t <= 16) launch_count<16>(grid, scores, ld, rows, n, k, t, w, words_row_stride, ranks_out, stream);
  else launch_count<64>(grid, scores, ld, rows, n, k, t, w, words_row_stride, ranks_out, stream);
  if (launched() != kOk) return kErrLaunch;
  hipLaunchKernelGGL(scores_rank_finish_kernel, dim3(grid_for((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, k, total, t, n, w,
                     words_row_stride, ranks_out);
  return launched();
}

int item_mask_clear_rows(const int64_t* positions, int rows, int64_t m, int64_t n, void* words, int64_t words_row_stride, hipStream_t stream) {
  const int64_t total = (int64_t)rows * m;
  hipLaunchKernelGGL(mask_rows_clear_kernel, dim3(grid_for((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, positions, total, m, n, (u32*)words,
                     words_row_stride);
  return launched();
}

}  // namespace mol
