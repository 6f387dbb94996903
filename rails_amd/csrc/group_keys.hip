// Candidate keys of the item-sharded MoLNaiveTopK / MoLCombTopK, global form (rails_amd/sharded.py): the per-group and coarse candidates of
// every rank travel as ONE 64-bit key each -- the scores are bf16 values -- and one launch turns the gathered lists into the global top-k of
// every row, written as THIS rank's local positions (holes elsewhere) straight into the union buffer the rerank reads.
//   key = (order-preserving 16-bit image of the bf16 score) << 48 | (2^48 - 1 - global position)        key 0 = pad
// A larger unsigned key is the better candidate; equal scores order by ascending global position.  The score image is rails_topk's
// (topk_keys.h orderable(): u | sign bit for a clear sign, ~u for a set one) cut to the upper 16 bits of the fp32 word, so +0 > -0,
// +inf above every finite score, a NaN with a clear sign bit above +inf, a NaN with a set sign bit below -inf -- a plain bit-pattern
// order with no special case, exactly as rails_topk ranks the same values.  (include/rails_amd.h rails_group_keys_*)
#include <hip/hip_runtime.h>

#include "mol_kernels.h"
#include "topk_keys.h"

namespace mol {

constexpr int kGroupKeyCap = 16384;          // keys per row in LDS (128 KiB), the limit of rails_merge_candidates
constexpr int kGroupKeyThreads = 256;
constexpr unsigned long long kPosMask = (1ull << 48) - 1ull;

__device__ __forceinline__ unsigned long long group_key(float score, int64_t global_pos) {
  const unsigned int h = __float_as_uint(score) >> 16;
  const unsigned int img = (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
  return ((unsigned long long)img << 48) | (kPosMask - (unsigned long long)global_pos);
}

__global__ __launch_bounds__(kGroupKeyThreads) void group_keys_pack_kernel(const float* __restrict__ scores, const int64_t* __restrict__ positions,
                                                                          int64_t total, int k_local, int64_t offset, int k_slots,
                                                                          unsigned long long* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kGroupKeyThreads + threadIdx.x;
  if (i >= total) return;
  const int64_t row = i / k_slots;
  const int j = (int)(i - row * k_slots);
  unsigned long long kv = 0ull;
  if (j < k_local) {
    const int64_t p = positions[row * k_local + j];
    if (p >= 0) kv = group_key(scores[row * k_local + j], p + offset);
  }
  keys[i] = kv;
}

// One workgroup per row.  The R lists of a row are staged in LDS; list r occupies [r * k, (r + 1) * k).  Every list is descending (a rank's
// own top-k, pads last), so the merged rank of key (r, j) needs no sort: it is j + the number of keys of every other list that precede it
// -- keys greater than it, and for the lists of lower ranks the equal ones too, which makes the order total (ranks are a permutation even
// among pads or the equal keys of overlapping shards).  One binary search per other list, one barrier in all.  A row whose lists are not
// descending (legal for the C entry point, never produced by rails_group_keys_pack over sorted rows) is sorted in LDS instead.
__global__ __launch_bounds__(kGroupKeyThreads) void group_keys_merge_own_kernel(const unsigned long long* __restrict__ gathered, int R,
                                                                               int64_t rank_stride, int k, int npad, int64_t lo, int64_t hi,
                                                                               int64_t* __restrict__ out_global, int64_t* __restrict__ out_local,
                                                                               int64_t out_ld, int64_t out_col, int rows_per_out_row) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long gk_keys[];
  __shared__ int unsorted;
  const int row = blockIdx.x;
  const int count = R * k;
  if (threadIdx.x == 0) unsorted = 0;
  for (int i = threadIdx.x; i < npad; i += kGroupKeyThreads) {
    unsigned long long kv = 0ull;
    if (i < count) {
      const int r = i / k, j = i - r * k;
      kv = gathered[(int64_t)r * rank_stride + (int64_t)row * k + j];
    }
    gk_keys[i] = kv;
  }
  __syncthreads();
  const int64_t local_base = (int64_t)(row / rows_per_out_row) * out_ld + out_col + (int64_t)(row % rows_per_out_row) * k;
  auto emit = [&](unsigned long long kv, int slot) {
    const int64_t pos = kv == 0ull ? (int64_t)-1 : (int64_t)(kPosMask - (kv & kPosMask));
    if (out_global) out_global[(int64_t)row * k + slot] = pos;
    out_local[local_base + slot] = (pos >= lo && pos < hi) ? pos - lo : (int64_t)-1;
  };
  if (sorted_lists_check<kGroupKeyThreads>(gk_keys, count, k, &unsorted)) {
    for (int i = threadIdx.x; i < count; i += kGroupKeyThreads) {
      const int rank = sorted_lists_rank<true>(gk_keys, R, k, i, k);   // an equal key of a lower rank precedes this one
      if (rank < k) emit(gk_keys[i], rank);
    }
    return;
  }
  lds_bitonic_desc<kGroupKeyThreads>(gk_keys, npad);
  for (int j = threadIdx.x; j < k; j += kGroupKeyThreads) emit(gk_keys[j], j);
}

}  // namespace mol

using namespace mol;

extern "C" {

int rails_group_keys_pack(const float* scores, const int64_t* positions, int32_t rows, int32_t k_local, int64_t offset, int64_t n_local,
                          int32_t k_slots, uint64_t* keys, void* stream) {
  if (rows < 0 || k_local < 0 || k_slots < k_local) { set_error("group_keys_pack: bad size (rows %d, k_local %d, k_slots %d)", rows, k_local, k_slots); return kErrInvalid; }
  if (offset < 0 || n_local < 0 || offset > (int64_t)(1ll << 48) || n_local > (int64_t)(1ll << 48) - offset) {
    set_error("group_keys_pack: global positions [%lld, %lld) do not fit 48 bits", (long long)offset, (long long)offset + (long long)n_local);
    return kErrInvalid;
  }
  const int64_t total = (int64_t)rows * k_slots;
  if (total == 0) return kOk;
  if (!keys || (k_local > 0 && (!scores || !positions))) { set_error("group_keys_pack: NULL pointer"); return kErrInvalid; }
  if ((total + kGroupKeyThreads - 1) / kGroupKeyThreads > 0x7FFFFFFFll) { set_error("group_keys_pack: too many keys"); return kErrInvalid; }
  hipLaunchKernelGGL(group_keys_pack_kernel, dim3((unsigned int)((total + kGroupKeyThreads - 1) / kGroupKeyThreads)), dim3(kGroupKeyThreads), 0,
                     (hipStream_t)stream, scores, positions, total, k_local, offset, k_slots, reinterpret_cast<unsigned long long*>(keys));
  if (hipGetLastError() != hipSuccess) { set_error("group_keys_pack: HIP launch failed"); return kErrLaunch; }
  return kOk;
}

int rails_group_keys_supported(int32_t n_ranks, int32_t k) {
  return n_ranks > 0 && k > 0 && (int64_t)n_ranks * k <= kGroupKeyCap ? 1 : 0;
}

int rails_group_keys_merge_own(const uint64_t* gathered, int32_t n_ranks, int64_t rank_stride, int32_t rows, int32_t k, int64_t lo, int64_t hi,
                               int64_t* out_global, int64_t* out_local, int64_t out_ld, int64_t out_col, int32_t rows_per_out_row,
                               void* stream) {
  if (n_ranks <= 0 || rows < 0 || k <= 0 || rows_per_out_row <= 0 || rank_stride < (int64_t)rows * k || out_col < 0 ||
      out_ld < out_col + (int64_t)(rows_per_out_row < rows ? rows_per_out_row : (rows > 0 ? rows : 1)) * k) {
    set_error("group_keys_merge_own: bad size (ranks %d, rows %d, k %d, rank_stride %lld, out_ld %lld, out_col %lld, rows_per_out_row %d)", n_ranks, rows, k,
              (long long)rank_stride, (long long)out_ld, (long long)out_col, rows_per_out_row);
    return kErrInvalid;
  }
  if (!rails_group_keys_supported(n_ranks, k)) {
    set_error("group_keys_merge_own: n_ranks * k = %lld exceeds the in-LDS capacity (%d)", (long long)n_ranks * k, kGroupKeyCap);
    return kErrUnsupported;
  }
  if (rows == 0) return kOk;
  if (!gathered || !out_local) { set_error("group_keys_merge_own: NULL pointer"); return kErrInvalid; }
  static DynLdsOnce once;
  if (ensure_dyn_lds(once, reinterpret_cast<const void*>(&group_keys_merge_own_kernel), kGroupKeyCap * (int)sizeof(unsigned long long)) != kOk) {
    set_error("group_keys_merge_own: cannot reserve LDS");
    return kErrLaunch;
  }
  const int npad = next_pow2(n_ranks * k, 2);
  hipLaunchKernelGGL(group_keys_merge_own_kernel, dim3(rows), dim3(kGroupKeyThreads), npad * sizeof(unsigned long long), (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(gathered), n_ranks, rank_stride, k, npad, lo, hi, out_global, out_local, out_ld,
                     out_col, rows_per_out_row);
  if (hipGetLastError() != hipSuccess) { set_error("group_keys_merge_own: HIP launch failed"); return kErrLaunch; }
  return kOk;
}

}  // extern "C"
