// Query fusion: several sub-query rows per user become one result row (rails_scores_fuse_rows / rails_topk_fuse_lists).
//
// Fused row u owns the sub-query rows [lims[u], lims[u + 1]) of its input.  Two kernels:
//   scores_fuse_rows_kernel   (S, n) fp32 -> (U, n) fp32.  Grid (column chunks, fused rows), grid-y looped as in score_rows.h: a workgroup owns
//                             4 096 columns of ONE output row and reads the segment's rows at those columns, ascending -- a runtime loop over
//                             rows with one accumulator per column in registers.  Every sub-query score is read once, every fused score
//                             written once; no atomics, no LDS, no scratch.
//                               max            the element with the largest orderable(bits) of topk_keys.h: no float compare, so +-0, +-inf
//                                              and NaN payloads fuse as rails_topk ranks them
//                               sum            acc = s[r0]; acc = fl32(acc + s[r])
//                               weighted sum   acc = fl32(w[r0] * s[r0]); acc = fl32(acc + fl32(w[r] * s[r])): two roundings per term, never an fma
//                             The input rows are not mutually aligned unless both bases are 16-byte aligned and both row strides multiples of
//                             4: then 16-byte loads and stores, otherwise the same loop one column per thread.  Every index is tested against n.
//   topk_fuse_lists_kernel    max alone: one workgroup per fused row merges its m sorted lists of k' (score, position) entries.  If x is among
//                             the first k eligible-and-unseen items of F[u, .] and r* the row where x attains its maximum, x is among row r*'s
//                             top (k + w) -- so the lists hold every answer.  Entries sorted in LDS by (position, orderable(score)) descending:
//                             the head of each position run is that position's best; heads become make_key(score, position), the rest key 0; a
//                             second sort puts them in selection order; the first k whose id is not among the row's seen ids are written.
//   lists_union_kernel        the candidate union of the approximate modules' fused calls (rails_lists_union): one workgroup per fused row sorts
//                             its sub-query rows' candidate positions in LDS and writes the distinct ones ascending -- the columns on which the
//                             rows of a segment are scored, so that scores_fuse_rows_kernel fuses aligned columns.
// Plain C++ with vector stores; every index is tested before it is used.
#include <hip/hip_runtime.h>

#include "mol_kernels.h"
#include "ranked_list.h"
#include "score_rows.h"
#include "topk_keys.h"
#include "wave_ops.h"

namespace mol {

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kThreads = kRowWalkThreads;
constexpr int kIters = kRowWalkIters;
constexpr int kListThreads = kSortThreads;

enum : int { kFuseMax = RAILS_FUSE_MAX, kFuseSum = RAILS_FUSE_SUM, kFuseWeighted = 2 };

template <int MODE>
__device__ __forceinline__ float fuse_first(float s, float w) {
  return MODE == kFuseWeighted ? __fmul_rn(w, s) : s;
}
template <int MODE>
__device__ __forceinline__ float fuse_next(float acc, float s, float w) {
  if (MODE == kFuseMax) return orderable(s) > orderable(acc) ? s : acc;
  return __fadd_rn(acc, MODE == kFuseWeighted ? __fmul_rn(w, s) : s);
}

// the segment of fused row u, clamped to the rows the matrix has (an empty one: begin == end)
__device__ __forceinline__ void segment_of(const int64_t* lims, int64_t u, int64_t rows_in, int64_t& begin, int64_t& end) {
  begin = lims[u];
  end = lims[u + 1];
  if (begin < 0) begin = 0;
  if (end > rows_in) end = rows_in;
  if (end < begin) end = begin;
}

}  // namespace

// VEC: scores, out 16-byte aligned, ld and ld_out multiples of 4 -- column 4 v of every row is then 16-byte aligned.
// An empty segment (the host refuses one) writes the identity of its mode: -inf for max, +0 for the sums.
template <bool VEC, int MODE>
__global__ void __launch_bounds__(kThreads) scores_fuse_rows_kernel(const float* __restrict__ scores, int64_t ld, int64_t rows_in, int64_t n,
                                                                   const int64_t* __restrict__ lims, int64_t n_out, const float* __restrict__ weights,
                                                                   float* __restrict__ out, int64_t ld_out, const int32_t* __restrict__ run_if) {
  MOL_RUN_IF(run_if);
  const int tid = threadIdx.x;
  const float empty = MODE == kFuseMax ? -INFINITY : 0.0f;
  for (int64_t u = blockIdx.y; u < n_out; u += gridDim.y) {
    int64_t begin, end;
    segment_of(lims, u, rows_in, begin, end);
    float* orow = out + u * ld_out;
    if (VEC) {
      const int64_t q = n >> 2;                                       // whole float4 of a row
      const int64_t v0 = (int64_t)blockIdx.x * kRowWalkChunkVecs + tid;
      float4 acc[kIters];
#pragma unroll
      for (int it = 0; it < kIters; ++it) acc[it] = make_float4(empty, empty, empty, empty);
      for (int64_t r = begin; r < end; ++r) {                         // (uniform over the workgroup)
        const float* srow = scores + r * ld;
        const float w = MODE == kFuseWeighted ? weights[r] : 1.0f;
#pragma unroll
        for (int it = 0; it < kIters; ++it) {
          const int64_t v = v0 + (int64_t)it * kThreads;
          if (v >= q) continue;
          const float4 s = *reinterpret_cast<const float4*>(srow + 4 * v);
          if (r == begin) {
            acc[it] = make_float4(fuse_first<MODE>(s.x, w), fuse_first<MODE>(s.y, w), fuse_first<MODE>(s.z, w), fuse_first<MODE>(s.w, w));
          } else {
            acc[it].x = fuse_next<MODE>(acc[it].x, s.x, w);
            acc[it].y = fuse_next<MODE>(acc[it].y, s.y, w);
            acc[it].z = fuse_next<MODE>(acc[it].z, s.z, w);
            acc[it].w = fuse_next<MODE>(acc[it].w, s.w, w);
          }
        }
      }
#pragma unroll
      for (int it = 0; it < kIters; ++it) {
        const int64_t v = v0 + (int64_t)it * kThreads;
        if (v < q) *reinterpret_cast<float4*>(orow + 4 * v) = acc[it];
      }
      // the n % 4 last columns of the row, on chunk 0 by threads 0..2
      const int64_t x = 4 * q + tid;
      if (blockIdx.x == 0 && tid < 3 && x < n) {
        float a = empty;
        for (int64_t r = begin; r < end; ++r) {
          const float s = scores[r * ld + x], w = MODE == kFuseWeighted ? weights[r] : 1.0f;
          a = r == begin ? fuse_first<MODE>(s, w) : fuse_next<MODE>(a, s, w);
        }
        orow[x] = a;
      }
    } else {
      const int64_t x0 = (int64_t)blockIdx.x * (4 * kRowWalkChunkVecs) + tid;
      constexpr int kCols = 4 * kIters;                               // columns per thread: the chunk of the 16-byte form
      float acc[kCols];
#pragma unroll
      for (int it = 0; it < kCols; ++it) acc[it] = empty;
      for (int64_t r = begin; r < end; ++r) {
        const float* srow = scores + r * ld;
        const float w = MODE == kFuseWeighted ? weights[r] : 1.0f;
#pragma unroll
        for (int it = 0; it < kCols; ++it) {
          const int64_t x = x0 + (int64_t)it * kThreads;
          if (x >= n) continue;
          const float s = srow[x];
          acc[it] = r == begin ? fuse_first<MODE>(s, w) : fuse_next<MODE>(acc[it], s, w);
        }
      }
#pragma unroll
      for (int it = 0; it < kCols; ++it) {
        const int64_t x = x0 + (int64_t)it * kThreads;
        if (x < n) orow[x] = acc[it];
      }
    }
  }
}

template <bool VEC>
static void launch_fuse_rows(int mode, dim3 grid, hipStream_t stream, const float* scores, int64_t ld, int64_t rows_in, int64_t n, const int64_t* lims,
                             int64_t n_out, const float* weights, float* out, int64_t ld_out, const int32_t* run_if) {
  if (mode == kFuseMax)
    hipLaunchKernelGGL((scores_fuse_rows_kernel<VEC, kFuseMax>), grid, dim3(kThreads), 0, stream, scores, ld, rows_in, n, lims, n_out, weights, out, ld_out, run_if);
  else if (weights == nullptr)
    hipLaunchKernelGGL((scores_fuse_rows_kernel<VEC, kFuseSum>), grid, dim3(kThreads), 0, stream, scores, ld, rows_in, n, lims, n_out, weights, out, ld_out, run_if);
  else
    hipLaunchKernelGGL((scores_fuse_rows_kernel<VEC, kFuseWeighted>), grid, dim3(kThreads), 0, stream, scores, ld, rows_in, n, lims, n_out, weights, out, ld_out,
                       run_if);
}

int scores_fuse_rows(const float* scores, int64_t ld, int64_t rows_in, int64_t n, const int64_t* lims, int64_t n_out, int mode, const float* weights, float* out,
                     int64_t ld_out, const int32_t* run_if, hipStream_t stream) {
  const bool vec = ((((uintptr_t)scores | (uintptr_t)out) & 15u) == 0) && ld % 4 == 0 && ld_out % 4 == 0;
  const dim3 grid((unsigned)((n + 4 * kRowWalkChunkVecs - 1) / (4 * kRowWalkChunkVecs)), (unsigned)(n_out < 65535 ? n_out : 65535));
  if (vec) launch_fuse_rows<true>(mode, grid, stream, scores, ld, rows_in, n, lims, n_out, weights, out, ld_out, run_if);
  else launch_fuse_rows<false>(mode, grid, stream, scores, ld, rows_in, n, lims, n_out, weights, out, ld_out, run_if);
  return launched();
}

// ---- the list merge ------------------------------------------------------------------------------------------------------------------------
// One workgroup of kListThreads per fused row; npad (a power of two >= the largest segment's m * depth, the same for every row of the launch)
// keys in LDS, 3 npad up to 1 024 keys (lds_sort_desc's exchange buffer), then `look` survivor bytes; a tile of seen ids and the scan's wave
// totals are static.  An entry takes part iff its position lies in [0, n_items) and its score is above -inf (what a sub-row with fewer than
// depth eligible items is padded with).
//   sort 1   ((position + 1) << 32) | orderable(score), descending: the entries of one position side by side, the best first
//   heads    make_key(score, position) for the head of every position run, key 0 for everything else
//   sort 2   selection order: score descending, then position ascending
//   filter   the first look = min(npad, k + width) keys hold the first k unseen ones (ids are distinct: a row's seen ids remove at most
//            `width` items); a prefix scan over their survivor flags compacts the first k, the rest of the row is (-1, -inf)
__global__ void __launch_bounds__(kListThreads) topk_fuse_lists_kernel(const float* __restrict__ scores, int64_t ld, const int64_t* __restrict__ positions,
                                                                      int64_t rows_in, int depth, const int64_t* __restrict__ lims, int npad, int sort_slots,
                                                                      int look, int64_t n_items, const int64_t* __restrict__ ids,
                                                                      const int64_t* __restrict__ invalid, int width, int k, int64_t* __restrict__ out_ids,
                                                                      float* __restrict__ out_scores) {
  extern __shared__ __attribute__((aligned(16))) u64 keys[];
  unsigned char* surv = reinterpret_cast<unsigned char*>(keys + sort_slots);      // [look]
  __shared__ int64_t seen[kSeenTile];
  __shared__ int wave_tot[kListThreads / 64];
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x;
  int64_t begin, end;
  segment_of(lims, u, rows_in, begin, end);
  const int64_t count64 = (end - begin) * depth;
  const int count = count64 < npad ? (int)count64 : npad;      // (the host sized npad by the largest segment: never cut on a checked call)

  for (int i = tid; i < npad; i += kListThreads) {
    u64 kv = 0ull;
    if (i < count) {
      const int64_t r = begin + i / depth;
      const int j = i % depth;
      const int64_t p = positions[r * depth + j];
      const float s = scores[r * ld + j];
      if (p >= 0 && p < n_items && s != -INFINITY) kv = ((u64)((u32)p + 1u) << 32) | orderable(s);      // (n_items <= 2^32 - 1; a NaN is a score, not padding)
    }
    keys[i] = kv;
  }
  __syncthreads();
  lds_sort_desc(keys, npad);      // (ends with a barrier)

  constexpr int kPer = 16384 / kListThreads;      // slots per thread at the largest npad
  u64 head[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = tid + j * kListThreads;
    head[j] = 0ull;
    if (i < npad) {
      const u64 kv = keys[i];
      if (kv != 0ull && (i == 0 || (keys[i - 1] >> 32) != (kv >> 32))) head[j] = make_key(unorderable((u32)(kv & 0xFFFFFFFFull)), (u32)(kv >> 32) - 1u);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = tid + j * kListThreads;
    if (i < npad) keys[i] = head[j];
  }
  __syncthreads();
  lds_sort_desc(keys, npad);

  for (int i = tid; i < look; i += kListThreads) surv[i] = keys[i] != 0ull ? 1 : 0;
  drop_seen<kListThreads>(surv, look, [&](int i) { return (int64_t)key_pos(keys[i]); }, ids, invalid + u * width, width, seen);
  __syncthreads();
  emit_first_k<kListThreads>(
      surv, look, k, wave_tot,
      [&](int i, int o) {
        const u64 kv = keys[i];
        const int64_t p = (int64_t)key_pos(kv);
        out_ids[u * k + o] = ids != nullptr ? ids[p] : p;
        out_scores[u * k + o] = unorderable(key_score(kv));
      },
      [&](int e) {
        out_ids[u * k + e] = -1;
        out_scores[u * k + e] = -INFINITY;
      });
}

int topk_fuse_lists(const float* scores, int64_t ld, const int64_t* positions, int64_t rows_in, int depth, const int64_t* lims, int n_out, int max_segment,
                    int64_t n_items, const int64_t* ids, const int64_t* invalid, int width, int k, int64_t* out_ids, float* out_scores, hipStream_t stream) {
  const int64_t entries = (int64_t)max_segment * depth;
  if (entries > kFuseListMaxEntries) { set_error("topk_fuse_lists: %lld entries per fused row beyond %d", (long long)entries, kFuseListMaxEntries); return kErrUnsupported; }
  if (k > kFuseListMaxK) { set_error("topk_fuse_lists: k = %d beyond %d", k, kFuseListMaxK); return kErrUnsupported; }
  if (width > kFuseListMaxSeen) { set_error("topk_fuse_lists: width = %d beyond %d seen ids per row", width, kFuseListMaxSeen); return kErrUnsupported; }
  if (n_items > 0xFFFFFFFFll) { set_error("topk_fuse_lists: positions beyond 2^32 - 2"); return kErrUnsupported; }
  const int npad = next_pow2((int)entries, 64);
  const int sort_slots = npad <= kSortThreads ? 3 * npad : npad;      // lds_sort_desc's exchange buffer
  const int look = npad < k + width ? npad : k + width;
  const int lds = sort_slots * (int)sizeof(u64) + (look + 15) / 16 * 16;
  constexpr int max_lds = kFuseListMaxEntries * (int)sizeof(u64) + (kFuseListMaxK + kFuseListMaxSeen + 15) / 16 * 16;
  static DynLdsOnce once;
  if (ensure_dyn_lds(once, reinterpret_cast<const void*>(&topk_fuse_lists_kernel), max_lds) != kOk) return kErrLaunch;
  hipLaunchKernelGGL(topk_fuse_lists_kernel, dim3(n_out), dim3(kListThreads), lds, stream, scores, ld, positions, rows_in, depth, lims, npad, sort_slots, look,
                     n_items, ids, invalid, width, k, out_ids, out_scores);
  return launched();
}

// ---- the candidate union ---------------------------------------------------------------------------------------------------------------------
// One workgroup of kListThreads per fused row merges the ragged candidate lists of its sub-query rows (W positions each) into one sorted,
// duplicate-free list.  npad keys in LDS as for the list merge, then npad head bytes.  An entry takes part iff its position lies in
// [0, n_items).
//   sort    key 2^32 - position (n_items <= 2^32 - 1: never 0), descending: positions ascending, the copies of one position side by side, the
//           dropped entries (key 0) last
//   heads   the first key of every run of equal positions
//   emit    a prefix scan over the head flags compacts them: out[u, 0 : count) the distinct positions ascending, -1 behind them up to w_out
__global__ void __launch_bounds__(kListThreads) lists_union_kernel(const int64_t* __restrict__ positions, int64_t ld, int width, int64_t rows_in,
                                                                  const int64_t* __restrict__ lims, int npad, int sort_slots, int64_t n_items,
                                                                  int64_t* __restrict__ out, int w_out, int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) u64 keys[];
  unsigned char* head = reinterpret_cast<unsigned char*>(keys + sort_slots);      // [npad]
  __shared__ int wave_tot[kListThreads / 64];
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x;
  int64_t begin, end;
  segment_of(lims, u, rows_in, begin, end);
  const int64_t count64 = (end - begin) * width;
  const int count = count64 < npad ? (int)count64 : npad;      // (the host sized npad by the largest segment: never cut on a checked call)

  for (int i = tid; i < npad; i += kListThreads) {
    u64 kv = 0ull;
    if (i < count) {
      const int64_t p = positions[(begin + i / width) * ld + i % width];
      if (p >= 0 && p < n_items) kv = 0x100000000ull - (u64)p;
    }
    keys[i] = kv;
  }
  __syncthreads();
  lds_sort_desc(keys, npad);      // (ends with a barrier)

  for (int i = tid; i < npad; i += kListThreads) {
    const u64 kv = keys[i];
    head[i] = (kv != 0ull && (i == 0 || keys[i - 1] != kv)) ? 1 : 0;
  }
  __syncthreads();
  int64_t* orow = out + u * (int64_t)w_out;
  const int total = emit_first_k<kListThreads>(
      head, npad, w_out, wave_tot, [&](int i, int o) { orow[o] = (int64_t)(0x100000000ull - keys[i]); }, [&](int e) { orow[e] = -1; });
  if (counts != nullptr && tid == 0) counts[u] = total;
}

int lists_union(const int64_t* positions, int64_t ld, int width, int64_t rows_in, const int64_t* lims, int n_out, int max_segment, int64_t n_items,
                int64_t* out, int w_out, int32_t* counts, hipStream_t stream) {
  const int64_t entries = (int64_t)max_segment * width;
  if (entries > kFuseListMaxEntries) { set_error("lists_union: %lld entries per fused row beyond %d", (long long)entries, kFuseListMaxEntries); return kErrUnsupported; }
  if (n_items > 0xFFFFFFFFll) { set_error("lists_union: n_items = %lld, positions beyond 2^32 - 2", (long long)n_items); return kErrUnsupported; }
  if (w_out < entries) { set_error("lists_union: bad size (w_out = %d below max_segment * width = %lld)", w_out, (long long)entries); return kErrInvalid; }
  const int npad = next_pow2((int)entries, 64);
  const int sort_slots = npad <= kSortThreads ? 3 * npad : npad;      // lds_sort_desc's exchange buffer
  const int lds = sort_slots * (int)sizeof(u64) + npad;
  constexpr int max_lds = kFuseListMaxEntries * (int)sizeof(u64) + kFuseListMaxEntries;
  static DynLdsOnce once;
  if (ensure_dyn_lds(once, reinterpret_cast<const void*>(&lists_union_kernel), max_lds) != kOk) return kErrLaunch;
  hipLaunchKernelGGL(lists_union_kernel, dim3(n_out), dim3(kListThreads), lds, stream, positions, ld, width, rows_in, lims, npad, sort_slots, n_items, out, w_out,
                     counts);
  return launched();
}

}  // namespace mol
