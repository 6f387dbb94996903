// Range search over a score matrix (rails_scores_range_count / _write / _sort / _decode).
//
// hit(r, x) = eligible(r, x) and v(r, x) >= t[r]  -- an IEEE fp32 compare, false when either side is NaN -- with
//   v = scores[r, x]                               the score form (lse == NULL)
//   v = fl32(fl32(scores[r, x] * beta) - lse[r])   the log-probability form: scores_log_prob_kernel's value, one rounded multiply, no fma
// The result is ragged: row r owns [lims[r], lims[r + 1]) of one key array.  Five kernels, no atomics:
//   count    grid (column chunks, rows), the masked row walk of score_rows.h: hits per (row, slot) -> int32, plain stores.  A row has
//            chunks + 2 slots in POSITION order: [head | chunk 0 .. chunk C - 1 | tail].  for_row_chunk peels the ragged head and tail onto
//            chunk 0, but the tail's columns are the row's last, so both get slots of their own.  Every slot is written on every call.
//   offsets  one workgroup: the exclusive scan of all (row, slot) counts in row-major order -> int64 offsets, lims[rows + 1], counts[rows]
//   write    the same walk; per iteration a prefix scan over the workgroup (iteration, thread, element is position order inside a chunk):
//            make_key(score, position) stored at offset + rank, every store tested against the slot's count and the capacity.  Where the
//            walk disagrees with the count (it cannot, on unchanged inputs) nothing is written out of bounds and the error word is set.
//   sort     one workgroup per row: the row's segment into LDS, zero-padded to a power of two, lds_sort_desc, back
//   decode   key -> (score bits, id)
// Position order out of `write`, selection-key order (score descending, position ascending) out of `sort`; the same bits whatever the
// alignment of a row.  Plain C++ with vector stores; every index is tested before it is used.
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
constexpr int kWaves = kThreads / 64;
constexpr int kScanThreads = kSortThreads;       // the offsets kernel's one workgroup

// the value that meets the threshold; lp: the log-probability form (uniform over the launch)
__device__ __forceinline__ bool passes(float s, bool lp, float beta, float lse, float t) { return (lp ? __fmul_rn(s, beta) - lse : s) >= t; }

__device__ __forceinline__ u32 quad_hits(float4 s, u32 bits, bool lp, float beta, float lse, float t) {
  return bits & ((passes(s.x, lp, beta, lse, t) ? 1u : 0u) | (passes(s.y, lp, beta, lse, t) ? 2u : 0u) | (passes(s.z, lp, beta, lse, t) ? 4u : 0u) |
                 (passes(s.w, lp, beta, lse, t) ? 8u : 0u));
}

struct RangeWorkspace {
  int32_t* counts;      // [rows * slots]
  int64_t* offsets;     // [rows * slots]
  int32_t* error;       // one word: a write pass that disagreed with its count
};

inline size_t range_cells(int rows, int64_t n) { return (size_t)rows * (size_t)(chunks_of(n) + 2); }

inline RangeWorkspace range_workspace(void* workspace, int rows, int64_t n) {
  const size_t cells = range_cells(rows, n);
  char* ws = (char*)workspace;
  RangeWorkspace w;
  w.offsets = (int64_t*)ws;
  w.counts = (int32_t*)(ws + align256(cells * sizeof(int64_t)));
  w.error = (int32_t*)(ws + align256(cells * sizeof(int64_t)) + align256(cells * sizeof(int32_t)));
  return w;
}

}  // namespace

template <bool MASKED>
__global__ void __launch_bounds__(kThreads) scores_range_count_kernel(const float* __restrict__ scores, int64_t ld, int rows, int64_t n,
                                                                     const float* __restrict__ thresholds, float beta, const float* __restrict__ lse,
                                                                     const u32* __restrict__ words, int64_t words_row_stride, int64_t n_words,
                                                                     int32_t* __restrict__ counts) {
  __shared__ int part[kWaves];
  const int tid = threadIdx.x;
  const int64_t slots = (int64_t)gridDim.x + 2;
  const bool lp = lse != nullptr;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const float* srow = scores + row * ld;
    const u32* mrow = MASKED ? words + row * words_row_stride : nullptr;
    const float t = thresholds[row], l = lp ? lse[row] : 0.0f;
    int cnt = 0;
    bool edge_hit = false;
    for_row_chunk<MASKED>(
        srow, n, mrow, n_words, [&](int64_t, float4 s, u32 bits) { cnt += __popc(quad_hits(s, bits, lp, beta, l, t)); },
        [&](int64_t, float s, bool keep) { edge_hit = keep && passes(s, lp, beta, l, t); });
    const u64 edges = __ballot(edge_hit);      // (wave 0 of chunk 0: lanes 0..3 the head, 4..7 the tail)
    const int total = block_sum<kThreads>(cnt, part);
    if (tid == 0) {
      int32_t* crow = counts + row * slots;
      crow[1 + blockIdx.x] = total;
      if (blockIdx.x == 0) {
        crow[0] = __popcll(edges & 0xFull);
        crow[slots - 1] = __popcll(edges & 0xF0ull);
      }
    }
  }
}

// offsets[i] = the sum of counts[0 .. i) over all (row, slot) cells in row-major order; lims[r] = the offset of row r's first slot,
// lims[rows] = the sum of all; row_counts[r] = lims[r + 1] - lims[r].  One workgroup, kScanThreads cells per pass, an int64 carry.
__global__ void __launch_bounds__(kScanThreads) scores_range_offsets_kernel(const int32_t* __restrict__ counts, int64_t rows, int64_t slots,
                                                                           int64_t* __restrict__ offsets, int64_t* __restrict__ lims,
                                                                           int64_t* __restrict__ row_counts, int32_t* __restrict__ error) {
  __shared__ int totals[kScanThreads / 64];
  const int tid = threadIdx.x;
  const int64_t cells = rows * slots;
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < cells; c0 += kScanThreads) {
    const int64_t i = c0 + tid;
    const int v = i < cells ? counts[i] : 0;
    int total;
    const int before = block_scan_excl<kScanThreads>(v, totals, total);
    if (i < cells) {
      offsets[i] = carry + before;
      if (i % slots == 0) lims[i / slots] = carry + before;
    }
    carry += total;
  }
  if (tid == 0) {
    lims[rows] = carry;
    *error = 0;
  }
  __syncthreads();      // (lims, written by this workgroup, read back below)
  for (int64_t r = tid; r < rows; r += kScanThreads) row_counts[r] = lims[r + 1] - lims[r];
}

template <bool MASKED>
__global__ void __launch_bounds__(kThreads) scores_range_write_kernel(const float* __restrict__ scores, int64_t ld, int rows, int64_t n,
                                                                     const float* __restrict__ thresholds, float beta, const float* __restrict__ lse,
                                                                     const u32* __restrict__ words, int64_t words_row_stride, int64_t n_words,
                                                                     const int32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                                     u64* __restrict__ keys_out, int64_t capacity, int32_t* __restrict__ error) {
  __shared__ int totals[kWaves];
  const int tid = threadIdx.x;
  const int64_t slots = (int64_t)gridDim.x + 2;
  const bool lp = lse != nullptr;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const float* srow = scores + row * ld;
    const u32* mrow = MASKED ? words + row * words_row_stride : nullptr;
    const float t = thresholds[row], l = lp ? lse[row] : 0.0f;
    const int64_t cell = row * slots + 1 + blockIdx.x;
    const int expect = counts[cell];
    const int64_t first = offsets[cell];
    const int64_t x_first = row_shape(srow, n).head + 4 * ((int64_t)blockIdx.x * kRowWalkChunkVecs + tid);      // the thread's first column
    // the walk: the thread's quads stay in registers (iteration j of this thread is the j-th call), their hits in four bits each
    float4 val[kRowWalkIters];
#pragma unroll
    for (int i = 0; i < kRowWalkIters; ++i) val[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    u32 hits = 0u;
    int j = 0;
    bool edge_hit = false;
    float edge_score = 0.0f;
    for_row_chunk<MASKED>(
        srow, n, mrow, n_words,
        [&](int64_t, float4 s, u32 bits) {
          hits |= quad_hits(s, bits, lp, beta, l, t) << (4 * j);
#pragma unroll
          for (int i = 0; i < kRowWalkIters; ++i)
            if (i == j) val[i] = s;
          ++j;
        },
        [&](int64_t, float s, bool keep) {
          edge_hit = keep && passes(s, lp, beta, l, t);
          edge_score = s;
        });
    // the head and the tail (chunk 0, lanes 0..3 and 4..7 of wave 0): a hit's rank is the number of hits in the lanes before it
    const u64 edges = __ballot(edge_hit);
    if (blockIdx.x == 0 && tid < 8 && edge_hit) {
      const bool tail = tid >= 4;
      const int64_t ecell = row * slots + (tail ? slots - 1 : 0);
      const u64 group = tail ? (edges >> 4) & 0xFull : edges & 0xFull;
      const int rank = __popcll(group & ((1ull << (tid & 3)) - 1ull));
      const int64_t x = tail ? row_shape(srow, n).tail0 + (tid - 4) : tid;
      const int64_t at = offsets[ecell] + rank;
      if (__popcll(group) == counts[ecell] && at >= 0 && at < capacity) keys_out[at] = make_key(edge_score, (u32)x);
      else *error = 1;      // (every writer stores the same value)
    }
    if (expect == 0) {      // (uniform over the workgroup) most chunks of a selective threshold: no scan
      if (hits != 0u) *error = 1;
      continue;
    }
    int before_it = 0;
#pragma unroll
    for (int it = 0; it < kRowWalkIters; ++it) {
      const u32 h = (hits >> (4 * it)) & 0xFu;
      int total;
      int rank = before_it + block_scan_excl<kThreads>(__popc(h), totals, total);
      const float s[4] = {val[it].x, val[it].y, val[it].z, val[it].w};
      const int64_t x0 = x_first + 4 * (int64_t)it * kThreads;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if ((h >> e) & 1u) {
          const int64_t at = first + rank;
          if (rank < expect && at >= 0 && at < capacity) keys_out[at] = make_key(s[e], (u32)(x0 + e));
          else *error = 1;
          ++rank;
        }
      }
      before_it += total;
    }
    if (tid == 0 && before_it != expect) *error = 1;
  }
}

// Row r's keys[lims[r], lims[r + 1]) sorted descending in place.  A row of fewer than 2 keys, or of more than max_count (what the launch's
// LDS holds), is left as it is.  LDS: npad slots, 3 npad up to 1 024 keys (lds_sort_desc's exchange buffer, as in collapse.hip).
__global__ void __launch_bounds__(kSortThreads) scores_range_sort_kernel(u64* __restrict__ keys, const int64_t* __restrict__ lims, int max_count) {
  extern __shared__ __attribute__((aligned(16))) u64 seg[];
  const int64_t row = blockIdx.x;
  const int64_t begin = lims[row], count64 = lims[row + 1] - begin;
  if (count64 < 2 || count64 > max_count) return;      // (uniform over the workgroup)
  const int count = (int)count64, npad = next_pow2(count, 2);
  for (int i = threadIdx.x; i < npad; i += kSortThreads) seg[i] = i < count ? keys[begin + i] : 0ull;
  __syncthreads();
  lds_sort_desc(seg, npad);      // (ends with a barrier)
  for (int i = threadIdx.x; i < count; i += kSortThreads) keys[begin + i] = seg[i];
}

__global__ void scores_range_decode_kernel(const u64* __restrict__ keys, int64_t total, const int64_t* __restrict__ ids, int64_t n,
                                           float* __restrict__ scores_out, int64_t* __restrict__ ids_out) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    const u64 key = keys[u];
    const int64_t p = (int64_t)key_pos(key);
    scores_out[u] = unorderable(key_score(key));
    ids_out[u] = p < n ? (ids != nullptr ? ids[p] : p) : -1;
  }
}

// workspace: int64 offsets and int32 counts per (row, slot), then the error word, each 256-byte aligned
size_t scores_range_workspace_bytes(int rows, int64_t n) {
  const size_t cells = range_cells(rows, n);
  return align256(cells * sizeof(int64_t)) + align256(cells * sizeof(int32_t)) + 256;
}

int scores_range_count(const float* scores, int64_t ld, int rows, int64_t n, const float* thresholds, float beta, const float* lse, const void* mask_words,
                       int64_t words_row_stride, void* workspace, int64_t* counts_out, int64_t* lims_out, hipStream_t stream) {
  const RangeWorkspace ws = range_workspace(workspace, rows, n);
  const u32* w = (const u32*)mask_words;
  launch_masked(w, scores_range_count_kernel<true>, scores_range_count_kernel<false>, row_grid(rows, n), stream, scores, ld, rows, n, thresholds, beta, lse, w,
                words_row_stride, item_mask_words(n), ws.counts);
  if (launched() != kOk) return kErrLaunch;
  hipLaunchKernelGGL(scores_range_offsets_kernel, dim3(1), dim3(kScanThreads), 0, stream, ws.counts, (int64_t)rows, chunks_of(n) + 2, ws.offsets, lims_out,
                     counts_out, ws.error);
  return launched();
}

int scores_range_write(const float* scores, int64_t ld, int rows, int64_t n, const float* thresholds, float beta, const float* lse, const void* mask_words,
                       int64_t words_row_stride, void* workspace, void* keys_out, int64_t capacity, hipStream_t stream) {
  const RangeWorkspace ws = range_workspace(workspace, rows, n);
  const u32* w = (const u32*)mask_words;
  launch_masked(w, scores_range_write_kernel<true>, scores_range_write_kernel<false>, row_grid(rows, n), stream, scores, ld, rows, n, thresholds, beta, lse, w,
                words_row_stride, item_mask_words(n), ws.counts, ws.offsets, (u64*)keys_out, capacity, ws.error);
  return launched();
}

int scores_range_sort(void* keys, const int64_t* lims, int rows, int max_count, hipStream_t stream) {
  if (max_count < 2) return kOk;
  const int npad = next_pow2(max_count, 2);
  // (a shorter row of the same launch may take the exchange buffer of the sorts up to 1 024 keys)
  const int lds = (npad <= kSortThreads ? 3 * npad : npad > 3 * kSortThreads ? npad : 3 * kSortThreads) * (int)sizeof(u64);
  static DynLdsOnce once;
  if (ensure_dyn_lds(once, reinterpret_cast<const void*>(&scores_range_sort_kernel), kRangeSortMax * (int)sizeof(u64)) != kOk) return kErrLaunch;
  hipLaunchKernelGGL(scores_range_sort_kernel, dim3(rows), dim3(kSortThreads), lds, stream, (u64*)keys, lims, max_count);
  return launched();
}

int scores_range_decode(const void* keys, int64_t total, const int64_t* ids, int64_t n, float* scores_out, int64_t* ids_out, hipStream_t stream) {
  hipLaunchKernelGGL(scores_range_decode_kernel, dim3(grid_for((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, (const u64*)keys, total, ids, n,
                     scores_out, ids_out);
  return launched();
}

}  // namespace mol
