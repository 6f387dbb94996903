// Softmax over the corpus (rails_scores_lse, rails_scores_log_prob, rails_scores_gumbel).
//
// For row r of a (rows, n) fp32 score matrix, over the row's ELIGIBLE columns (mask bit set; no mask: all of them), with beta = 1 / temperature:
//   y(x) = fl32(x * beta)                          one rounded fp32 multiply
//   Y    = y(M), M the largest eligible x
//   S    = sum over the eligible x of expf(y(x) - Y)
//   lse  = fl32(Y + log S)                         the log, the add and every cross-lane / cross-workgroup sum in float64
//   log_prob(x) = fl32(y(x) - lse)
// Special rows: nothing eligible, or every eligible entry -inf -> lse = -inf; any eligible NaN -> NaN; otherwise any eligible +inf -> +inf
// (and a Y that overflows is the lse); an eligible -inf adds 0.
//   lse      max     grid (column chunks, rows): the largest eligible x of the chunk, or NaN if it holds an eligible NaN (order-independent)
//            rowmax  the chunks' maxima -> M per row (NaN if any is)
//            sum     the same grid, a second read, grouped by COLUMN (quads of four columns from column 0, float4 loads where the row starts
//                    16-byte aligned, four 4-byte loads elsewhere), so that the bits do not depend on the alignment of the row: per thread
//                    an fp32 chain of at most 16 terms (the peeled tail element of chunk 0 is kept apart), then float64: xor butterfly over
//                    the wave, the workgroup's four waves in wave order, one float64 partial per (row, chunk) stored to the workspace
//            finish  a row's partials added in chunk order, lse = fl32(Y + log S)
//            No floating-point atomics and no order that depends on arrival or on the grid: the same bits on every run.
//   log_prob a gather: out[r, j] = fl32(y(scores[r, p]) - lse[r]) for p = positions[r, j] eligible and inside [0, n), else -inf
//   gumbel   out of place: out[r, x] = fl32(y(x) + g(seed, first_row + r, x)) for eligible x, -inf otherwise; g = -logf(-logf(u)),
//            u = ((w >> 9) + 0.5) * 2^-23 (exact in fp32, inside [2^-24, 1 - 2^-24]), w = word 0 of Philox4x32-10 with counter
//            (x, row & 0xFFFFFFFF, row >> 32, 0) and key (seed & 0xFFFFFFFF, seed >> 32): the noise depends on (seed, global row, x) alone
// The order-independent passes (max, gumbel) run on the masked row walk of score_rows.h, which rank.hip shares; the sum keeps a walk of its
// own and takes the constants and mask_bit from there, the wave sum from wave_ops.h.  Plain C++ with vector stores; every index is tested
// against n before it is used.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mol_kernels.h"
#include "score_rows.h"
#include "wave_ops.h"

namespace mol {

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kThreads = kRowWalkThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kIters = kRowWalkIters;      // the fp32 chain of the sum has 4 * kIters = 16 terms

// NaN absorbs, otherwise the larger: commutative and associative, so any order of combination gives the same value
__device__ __forceinline__ float max_or_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

__device__ __forceinline__ float scaled(float x, float beta) { return __fmul_rn(x, beta); }

// word 0 of Philox4x32-10 (Salmon et al., SC'11) for counter (c0, c1, c2, 0) and key (k0, k1)
__device__ __forceinline__ u32 philox4x32_10_word0(u32 c0, u32 c1, u32 c2, u32 k0, u32 k1) {
  u32 c3 = 0u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const u32 hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const u32 hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

__device__ __forceinline__ float gumbel_noise(u32 x, u32 row_lo, u32 row_hi, u32 k0, u32 k1) {
  const u32 w = philox4x32_10_word0(x, row_lo, row_hi, k0, k1);
  const float u = ((float)(w >> 9) + 0.5f) * 0x1p-23f;      // 23 bits + a half: exact
  return -logf(-logf(u));
}

}  // namespace

// pass 1 of the lse: part_max[row * chunks + chunk] = the largest eligible x of the chunk (-inf: none), NaN if an eligible NaN is among them
template <bool MASKED>
__global__ void __launch_bounds__(kThreads) scores_lse_max_kernel(const float* __restrict__ scores, int64_t ld, int rows, int64_t n,
                                                                 const u32* __restrict__ words, int64_t words_row_stride, int64_t n_words,
                                                                 float* __restrict__ part_max) {
  __shared__ float wave_max[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const float* srow = scores + row * ld;
    const u32* mrow = MASKED ? words + row * words_row_stride : nullptr;
    float m = -INFINITY;
    for_row_chunk<MASKED>(
        srow, n, mrow, n_words,
        [&](int64_t, float4 s, u32 bits) {
          if (bits & 1u) m = max_or_nan(m, s.x);
          if (bits & 2u) m = max_or_nan(m, s.y);
          if (bits & 4u) m = max_or_nan(m, s.z);
          if (bits & 8u) m = max_or_nan(m, s.w);
        },
        [&](int64_t, float s, bool keep) {
          if (keep) m = max_or_nan(m, s);
        });
    for (int d = 32; d > 0; d >>= 1) m = max_or_nan(m, __shfl_xor(m, d, 64));
    if (lane == 0) wave_max[wave] = m;
    __syncthreads();
    if (tid == 0) {
      float t = wave_max[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) t = max_or_nan(t, wave_max[w]);
      part_max[row * gridDim.x + blockIdx.x] = t;
    }
    __syncthreads();      // (wave_max is rewritten for the next row)
  }
}

__global__ void scores_lse_rowmax_kernel(const float* __restrict__ part_max, int64_t rows, int64_t chunks, float* __restrict__ row_max) {
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < rows; row += (int64_t)gridDim.x * blockDim.x) {
    float m = -INFINITY;
    for (int64_t c = 0; c < chunks; ++c) m = max_or_nan(m, part_max[row * chunks + c]);
    row_max[row] = m;
  }
}

// pass 2 of the lse: part_sum[row * chunks + chunk] = the chunk's share of S, for the rows whose Y is finite (the others need no sum)
template <bool MASKED>
__global__ void __launch_bounds__(kThreads) scores_lse_sum_kernel(const float* __restrict__ scores, int64_t ld, int rows, int64_t n, float beta,
                                                                 const u32* __restrict__ words, int64_t words_row_stride, int64_t n_words,
                                                                 const float* __restrict__ row_max, double* __restrict__ part_sum) {
  __shared__ double wave_part[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const float Y = scaled(row_max[row], beta);
    if (!(fabsf(Y) <= 3.402823466e+38f)) {      // NaN or +-inf: the finish kernel answers from Y alone (uniform over the workgroup)
      if (tid == 0) part_sum[row * gridDim.x + blockIdx.x] = 0.0;
      continue;
    }
    const float* srow = scores + row * ld;
    const u32* mrow = MASKED ? words + row * words_row_stride : nullptr;
    // The sum is grouped by COLUMN, not by address: q quads of four consecutive columns from column 0, then at most 3 tail columns.  Which
    // terms share a thread's chain, a wave and a chunk is then a function of the column alone, so the bits of the lse do not depend on where
    // the row starts -- a batch slice, whose rows sit at other alignments of a matrix with ld % 4 != 0, reproduces the unsliced call.  A
    // row that starts 16-byte aligned loads its quads as float4, any other as four 4-byte loads: the same values either way.
    const int64_t q = n >> 2;
    const bool aligned = (((uintptr_t)srow) & 15u) == 0u;      // (uniform over the row)
    float acc = 0.0f;      // the fp32 chain: at most 16 terms, each in [0, 1]
    const int64_t v0 = (int64_t)blockIdx.x * kRowWalkChunkVecs;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int64_t vw = v0 + (int64_t)it * kThreads + wave * 64;      // the wave's first quad: 256 columns = 8 whole mask words
      if (vw >= q) break;                                              // (wave-uniform)
      const int64_t v = vw + lane;
      u32 bits = 0xFu;
      if (MASKED) {
        const int64_t wi = (vw >> 3) + lane;
        const u32 wv = lane < 8 && wi < n_words ? mrow[wi] : 0u;
        bits = (__shfl(wv, lane >> 3, 64) >> ((lane & 7) * 4)) & 0xFu;
      }
      if (v < q) {
        const float* at = srow + 4 * v;
        float4 s;
        if (aligned) {
          s = *reinterpret_cast<const float4*>(at);
        } else {
          s.x = at[0];
          s.y = at[1];
          s.z = at[2];
          s.w = at[3];
        }
        if (bits & 1u) acc += expf(scaled(s.x, beta) - Y);
        if (bits & 2u) acc += expf(scaled(s.y, beta) - Y);
        if (bits & 4u) acc += expf(scaled(s.z, beta) - Y);
        if (bits & 8u) acc += expf(scaled(s.w, beta) - Y);
      }
    }
    double part = (double)acc;
    if (blockIdx.x == 0 && tid < 3) {      // the peeled tail, at most 3 columns: one more term, added in float64 so that the chain stays at 16
      const int64_t x = 4 * q + tid;
      if (x < n && (!MASKED || mask_bit(mrow, x))) part += (double)expf(scaled(srow[x], beta) - Y);
    }
    part = wave_sum(part);
    if (lane == 0) wave_part[wave] = part;
    __syncthreads();
    if (tid == 0) {
      double t = wave_part[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) t += wave_part[w];
      part_sum[row * gridDim.x + blockIdx.x] = t;
    }
    __syncthreads();      // (wave_part is rewritten for the next row)
  }
}

__global__ void scores_lse_finish_kernel(const float* __restrict__ row_max, const double* __restrict__ part_sum, int64_t rows, int64_t chunks, float beta,
                                         float* __restrict__ lse_out) {
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < rows; row += (int64_t)gridDim.x * blockDim.x) {
    const float Y = scaled(row_max[row], beta);
    float lse = Y;                                   // NaN, +inf, -inf (nothing eligible, or -inf alone) stand as they are
    if (fabsf(Y) <= 3.402823466e+38f) {
      double s = 0.0;
      for (int64_t c = 0; c < chunks; ++c) s += part_sum[row * chunks + c];
      lse = (float)((double)Y + log(s));
    }
    lse_out[row] = lse;
  }
}

template <bool MASKED>
__global__ void scores_log_prob_kernel(const float* __restrict__ scores, int64_t ld, int64_t n, const int64_t* __restrict__ positions, int64_t total, int64_t t,
                                       float beta, const float* __restrict__ lse, const u32* __restrict__ words, int64_t words_row_stride,
                                       float* __restrict__ out) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = positions[u], row = u / t;
    float v = -INFINITY;
    if (p >= 0 && p < n && (!MASKED || mask_bit(words + row * words_row_stride, p))) v = scaled(scores[row * ld + p], beta) - lse[row];
    out[u] = v;
  }
}

template <bool MASKED>
__global__ void __launch_bounds__(kThreads) scores_gumbel_kernel(const float* __restrict__ scores, int64_t ld, int rows, int64_t n, float beta, u32 k0, u32 k1,
                                                                int64_t first_row, const u32* __restrict__ words, int64_t words_row_stride, int64_t n_words,
                                                                float* __restrict__ out, int64_t out_ld) {
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const float* srow = scores + row * ld;
    float* orow = out + row * out_ld;
    const u32* mrow = MASKED ? words + row * words_row_stride : nullptr;
    const RowShape rs = row_shape(srow, n);
    const bool out_aligned = (((uintptr_t)(orow + rs.head)) & 15u) == 0u;      // (uniform over the row: the body's stores are 16 bytes wide or scalar)
    const u64 grow = (u64)(first_row + row);
    const u32 r_lo = (u32)grow, r_hi = (u32)(grow >> 32);
    for_row_chunk<MASKED>(
        srow, n, mrow, n_words,
        [&](int64_t x0, float4 s, u32 bits) {
          const u32 p = (u32)x0;
          float4 o;
          o.x = (bits & 1u) ? scaled(s.x, beta) + gumbel_noise(p, r_lo, r_hi, k0, k1) : -INFINITY;
          o.y = (bits & 2u) ? scaled(s.y, beta) + gumbel_noise(p + 1, r_lo, r_hi, k0, k1) : -INFINITY;
          o.z = (bits & 4u) ? scaled(s.z, beta) + gumbel_noise(p + 2, r_lo, r_hi, k0, k1) : -INFINITY;
          o.w = (bits & 8u) ? scaled(s.w, beta) + gumbel_noise(p + 3, r_lo, r_hi, k0, k1) : -INFINITY;
          if (out_aligned) {
            *reinterpret_cast<float4*>(orow + x0) = o;
          } else {
            orow[x0] = o.x;
            orow[x0 + 1] = o.y;
            orow[x0 + 2] = o.z;
            orow[x0 + 3] = o.w;
          }
        },
        [&](int64_t x, float s, bool keep) { orow[x] = keep ? scaled(s, beta) + gumbel_noise((u32)x, r_lo, r_hi, k0, k1) : -INFINITY; });
  }
}

// workspace: float64 partial sums (rows * chunks), fp32 partial maxima (rows * chunks), fp32 row maxima (rows), each 256-byte aligned
size_t scores_lse_workspace_bytes(int rows, int64_t n) {
  const size_t cells = (size_t)rows * (size_t)chunks_of(n);
  return align256(cells * sizeof(double)) + align256(cells * sizeof(float)) + align256((size_t)rows * sizeof(float));
}

int scores_lse(const float* scores, int64_t ld, int rows, int64_t n, float beta, const void* mask_words, int64_t words_row_stride, void* workspace,
               float* lse_out, hipStream_t stream) {
  const int64_t chunks = chunks_of(n);
  const size_t cells = (size_t)rows * (size_t)chunks;
  char* ws = (char*)workspace;
  double* part_sum = (double*)ws;
  float* part_max = (float*)(ws + align256(cells * sizeof(double)));
  float* row_max = (float*)(ws + align256(cells * sizeof(double)) + align256(cells * sizeof(float)));
  const dim3 grid = row_grid(rows, n);
  const u32* w = (const u32*)mask_words;
  const int64_t n_words = item_mask_words(n);
  const unsigned row_blocks = grid_for(((int64_t)rows + kThreads - 1) / kThreads);
  launch_masked(w, scores_lse_max_kernel<true>, scores_lse_max_kernel<false>, grid, stream, scores, ld, rows, n, w, words_row_stride, n_words, part_max);
  if (launched() != kOk) return kErrLaunch;
  hipLaunchKernelGGL(scores_lse_rowmax_kernel, dim3(row_blocks), dim3(kThreads), 0, stream, part_max, (int64_t)rows, chunks, row_max);
  if (launched() != kOk) return kErrLaunch;
  launch_masked(w, scores_lse_sum_kernel<true>, scores_lse_sum_kernel<false>, grid, stream, scores, ld, rows, n, beta, w, words_row_stride, n_words, row_max,
                part_sum);
  if (launched() != kOk) return kErrLaunch;
  hipLaunchKernelGGL(scores_lse_finish_kernel, dim3(row_blocks), dim3(kThreads), 0, stream, row_max, part_sum, (int64_t)rows, chunks, beta, lse_out);
  return launched();
}

int scores_log_prob(const float* scores, int64_t ld, int rows, int64_t n, const int64_t* positions, int64_t t, float beta, const float* lse,
                    const void* mask_words, int64_t words_row_stride, float* out, hipStream_t stream) {
  const int64_t total = (int64_t)rows * t;
  const dim3 grid(grid_for((total + kThreads - 1) / kThreads));
  const u32* w = (const u32*)mask_words;
  launch_masked(w, scores_log_prob_kernel<true>, scores_log_prob_kernel<false>, grid, stream, scores, ld, n, positions, total, t, beta, lse, w, words_row_stride,
                out);
  return launched();
}

int scores_gumbel(const float* scores, int64_t ld, int rows, int64_t n, float beta, uint64_t seed, int64_t first_row, const void* mask_words,
                  int64_t words_row_stride, float* out, int64_t out_ld, hipStream_t stream) {
  const dim3 grid = row_grid(rows, n);
  const u32* w = (const u32*)mask_words;
  const int64_t n_words = item_mask_words(n);
  const u32 k0 = (u32)seed, k1 = (u32)(seed >> 32);
  launch_masked(w, scores_gumbel_kernel<true>, scores_gumbel_kernel<false>, grid, stream, scores, ld, rows, n, beta, k0, k1, first_row, w, words_row_stride,
                n_words, out, out_ld);
  return launched();
}

}  // namespace mol
