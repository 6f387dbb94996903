// Exact ranks of given items (rails_scores_rank_keys, rails_scores_rank, rails_item_mask_clear_rows).
//
// rank(r, j) = 1 + #{ eligible y : key(r, y) > key(r, target j) } under the selection key of topk_keys.h, so rank - 1 is the index at which the
// target stands in the row's exhaustive top-k list (score descending, then position ascending; +-0, +-inf and NaN payloads by their bits).
//   keys    positions -> the targets' own keys, read from the matrix that is counted; key 0 (below every real key) for a position outside [0, n)
//   count   grid (column chunks, rows): a workgroup streams its slice of ONE score row once for all t targets of the row -- 16-byte loads
//           over the aligned middle of the row, the ragged head and tail peeled onto chunk 0 --, builds each element's key (0 where its mask bit
//           is clear: such a key exceeds no target's), compares it with the row's t target keys held in LDS and counts per lane in registers
//           (tiers of t as a template parameter: every counter index is a compile-time constant); wave sum, LDS sum over the workgroup, then
//           one integer atomic per (workgroup, target).  Integer adds commute: the result is the same bits whatever the arrival order.
//   finish  counts -> ranks: counts + 1 where the target's key is a real one and its own mask bit is set, else 0
// Plain launches on one stream (zero, count, finish); plain C++ with vector stores; every index is tested against n before it is used.
#include <hip/hip_runtime.h>

#include "mol_kernels.h"
#include "topk_keys.h"

namespace mol {

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kIters = 4;                                   // 16-byte loads per thread
constexpr int64_t kChunkVecs = (int64_t)kThreads * kIters;  // 1 024 float4 = 4 096 columns per workgroup
constexpr unsigned kMaxGridY = 65535u;
constexpr unsigned kMaxGrid = 1u << 16;
constexpr u64 kNoTarget = ~0ull;                            // pads a tier's unused key slots: no key exceeds it

inline unsigned grid_for(int64_t blocks) { return (unsigned)(blocks < 1 ? 1 : blocks > (int64_t)kMaxGrid ? (int64_t)kMaxGrid : blocks); }

__device__ __forceinline__ int wave_sum(int v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

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
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const float* srow = scores + row * ld;
    const u32* mrow = MASKED ? words + row * words_row_stride : nullptr;
    // the row as head + q aligned float4 + tail
    const int64_t lead = (int64_t)((4u - (u32)(((uintptr_t)srow >> 2) & 3u)) & 3u);
    const int64_t head = lead < n ? lead : n;
    const int64_t q = (n - head) >> 2;
    const int64_t tail0 = head + 4 * q;
    if (tid < T) {
      tk[tid] = tid < t ? keys[row * t + tid] : kNoTarget;
      total[tid] = 0;
    }
    __syncthreads();
    int cnt[T];
#pragma unroll
    for (int j = 0; j < T; ++j) cnt[j] = 0;

    const int64_t v0 = (int64_t)blockIdx.x * kChunkVecs;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int64_t vw = v0 + (int64_t)it * kThreads + wave * 64;      // the wave's first float4: 256 consecutive columns from xw
      if (vw >= q) break;                                              // (wave-uniform)
      const int64_t v = vw + lane;
      const int64_t xw = head + 4 * vw, x0 = head + 4 * v;
      u32 bits = 0xFu;
      if (MASKED) {
        // the wave's 256 columns lie in at most 9 mask words: one load per word, handed to the lanes by shuffles
        const int64_t wi = (xw >> 5) + lane;
        const u32 wv = lane < 10 && wi < n_words ? mrow[wi] : 0u;
        const int rel = (int)((x0 >> 5) - (xw >> 5));
        const u32 lo = __shfl(wv, rel, 64), hi = __shfl(wv, rel + 1, 64);
        bits = (u32)((((u64)hi << 32) | lo) >> (int)(x0 & 31)) & 0xFu;
      }
      if (v < q) {
        const float4 s = *reinterpret_cast<const float4*>(srow + x0);
        const u32 p = (u32)x0;
        count_elements<T>((bits & 1u) ? make_key(s.x, p) : 0ull, (bits & 2u) ? make_key(s.y, p + 1) : 0ull, (bits & 4u) ? make_key(s.z, p + 2) : 0ull,
                          (bits & 8u) ? make_key(s.w, p + 3) : 0ull, tk, cnt);
      }
    }
    if (blockIdx.x == 0 && tid < 8) {      // the peeled head (threads 0..3) and tail (threads 4..7): at most 3 columns each
      const int64_t x = tid < 4 ? tid : tail0 + (tid - 4);
      if (tid < 4 ? x < head : x < n) {
        const bool keep = !MASKED || ((mrow[x >> 5] >> (int)(x & 31)) & 1u) != 0u;
        count_elements<T>(keep ? make_key(srow[x], (u32)x) : 0ull, 0ull, 0ull, 0ull, tk, cnt);      // (key 0 exceeds no target's)
      }
    }
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
    if (ranked && words != nullptr) ranked = ((words[(u / t) * words_row_stride + (p >> 5)] >> (int)(p & 31)) & 1u) != 0u;
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

static inline int launched() { return hipGetLastError() == hipSuccess ? kOk : kErrLaunch; }

int scores_rank_keys(const float* scores, int64_t ld, int rows, int64_t n, const int64_t* positions, int t, void* keys_out, hipStream_t stream) {
  const int64_t total = (int64_t)rows * t;
  hipLaunchKernelGGL(scores_rank_keys_kernel, dim3(grid_for((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, scores, ld, n, positions, total, t,
                     (u64*)keys_out);
  return launched();
}

template <int T>
static void launch_count(dim3 grid, const float* scores, int64_t ld, int rows, int64_t n, const u64* keys, int t, const u32* words, int64_t stride,
                         int32_t* counts, hipStream_t stream) {
  const int64_t n_words = item_mask_words(n);
  if (words != nullptr)
    hipLaunchKernelGGL((scores_rank_kernel<T, true>), grid, dim3(kThreads), 0, stream, scores, ld, rows, n, keys, t, words, stride, n_words, counts);
  else
    hipLaunchKernelGGL((scores_rank_kernel<T, false>), grid, dim3(kThreads), 0, stream, scores, ld, rows, n, keys, t, words, stride, n_words, counts);
}

int scores_rank(const float* scores, int64_t ld, int rows, int64_t n, const void* keys, int t, const void* mask_words, int64_t words_row_stride,
                int32_t* ranks_out, hipStream_t stream) {
  const int64_t total = (int64_t)rows * t;
  if (hipMemsetAsync(ranks_out, 0, (size_t)total * sizeof(int32_t), stream) != hipSuccess) return kErrLaunch;
  const int64_t chunks = ((n + 3) / 4 + kChunkVecs - 1) / kChunkVecs;      // (a row's aligned middle holds at most n / 4 float4)
  const dim3 grid((unsigned)chunks, (unsigned)((unsigned)rows < kMaxGridY ? (unsigned)rows : kMaxGridY));
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
