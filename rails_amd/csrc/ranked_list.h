// The tail of a ranked list held by one workgroup, shared by collapse.hip and fuse.hip (the seen-id test alone: topk.hip too): drop the entries
// whose id is among the row's seen ids, write the first k survivors in list order, pad a short row.  Device-only; the LDS is the caller's.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_ops.h"

namespace mol {

constexpr int kSeenTile = 256;      // seen ids held in LDS at a time

// id among the `width` seen ids in LDS?  No early exit: every lane of the wave reads the same words.
template <class T>
__device__ __forceinline__ bool seen_id(const T* seen, int width, T id) {
  bool hit = false;
  for (int w = 0; w < width; ++w) hit |= (seen[w] == id);
  return hit;
}

// Drop the seen: clears surv[i], i < count, wherever the id of entry i's position (pos_of(i); ids == NULL: the position itself) is among
// invalid[0 .. width), the row's seen ids, which pass through `tile` (kSeenTile words of LDS) a tile at a time.  All NT threads call; thread t
// owns the entries t, t + NT, ...  The caller's barrier follows.
template <int NT, class P>
__device__ __forceinline__ void drop_seen(unsigned char* surv, int count, P pos_of, const int64_t* __restrict__ ids,
                                          const int64_t* __restrict__ invalid, int width, int64_t* tile) {
  const int tid = threadIdx.x;
  for (int w0 = 0; w0 < width; w0 += kSeenTile) {
    const int wn = width - w0 < kSeenTile ? width - w0 : kSeenTile;
    __syncthreads();
    if (tid < wn) tile[tid] = invalid[w0 + tid];
    __syncthreads();
    for (int i = tid; i < count; i += NT) {
      if (!surv[i]) continue;
      const int64_t p = pos_of(i);
      if (seen_id(tile, wn, ids != nullptr ? ids[p] : p)) surv[i] = 0;
    }
  }
}

// The first k survivors in list order: a contiguous segment of the list per thread, a prefix scan of the segments' survivor counts, emit(i, o)
// for survivor i at output column o < k, pad(e) for every column e of a short row beyond its last survivor.  -> the row's survivors (all of
// them, not min(., k)).  All NT threads call behind a barrier that orders the writes of surv; wave_tot: NT / 64 ints of LDS.
template <int NT, class E, class Z>
__device__ __forceinline__ int emit_first_k(const unsigned char* surv, int count, int k, int* wave_tot, E emit, Z pad) {
  const int tid = threadIdx.x;
  const int seg = (count + NT - 1) / NT;
  const int s0 = tid * seg < count ? tid * seg : count, s1 = s0 + seg < count ? s0 + seg : count;
  int c = 0;
  for (int i = s0; i < s1; ++i) c += surv[i];
  int total;
  int o = block_scan_excl<NT>(c, wave_tot, total);
  for (int i = s0; i < s1 && o < k; ++i) {
    if (!surv[i]) continue;
    emit(i, o);
    ++o;
  }
  for (int e = total + tid; e < k; e += NT) pad(e);
  return total;
}

}  // namespace mol
