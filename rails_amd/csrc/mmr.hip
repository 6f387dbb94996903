// Diversifying a ranked list by maximal marginal relevance.  One kernel:
//   mmr_walk_kernel   one workgroup per row over a ranked list of `depth` (score, position) entries: the first `pool` eligible entries (collapse's
//                     rule: a position of the corpus, a score above -inf, an id the row has not seen) form the pool, thread c owns pool entry c,
//                     and k dependent steps each pick the unpicked entry with the largest  lam * s[c] - mu * M[c]  (ties: the smaller pool index),
//                     M[c] = max(+0, the largest similarity of c to an entry picked so far) (rails_topk_mmr)
// All arithmetic is fp32, round to nearest, never fused (the library is built with -ffp-contract=off), and the similarity is ONE chain
// acc = acc + a[e] * b[e], e ascending from acc = +0 -- so the result is a function of the inputs alone, bit for bit.  No atomics; every loop
// bound is k, pool, dim or depth.
// Where thread c keeps its vector: in registers for dim <= 64 (three compile-time tiers of 16 / 32 / 64 floats, the tail zero: a product with
// a finite value is +-0 and acc + +-0 = acc, acc never being -0); beyond that in a per-call workspace (rows, dim, pool) it gathers once,
// TRANSPOSED so that the lanes of a wave read neighbouring words in every step.  A thread reads back only what it wrote itself.  The picked
// entry's vector reaches the others through LDS, read from the item table by its position (dim coalesced words).
#include "mol_kernels.h"
#include "ranked_list.h"
#include "score_rows.h"
#include "topk_keys.h"
#include "wave_ops.h"

namespace mol {

constexpr int kMmrThreads = kSortThreads;            // 1024: one thread per pool entry
constexpr int kMmrMaxDepth = 16384;                  // entries of one ranked list (rails_topk_collapse's)
constexpr int kMmrMaxPool = kMmrThreads;
constexpr int kMmrMaxDim = 256;
constexpr int kMmrRegDim = 64;                       // vectors up to this many floats stay in registers
constexpr int kMmrWaves = kMmrThreads / 64;

// ET: the register tier (16 / 32 / 64 floats per thread); 0: the workspace tier.
template <int ET>
__global__ __launch_bounds__(kMmrThreads) void mmr_walk_kernel(const float* __restrict__ scores, int64_t ld, const int64_t* __restrict__ positions,
                                                               int depth, const float* __restrict__ vectors, int64_t n_items, int dim, float lam,
                                                               float mu, int k, int pool, const int64_t* __restrict__ ids,
                                                               const int64_t* __restrict__ invalid, int width, float* ws,
                                                               float* __restrict__ out_scores, int64_t* __restrict__ out_pos,
                                                               int64_t* __restrict__ out_ids, int32_t* __restrict__ out_counts,
                                                               int32_t* __restrict__ out_of_range) {
  __shared__ unsigned char surv[kMmrMaxDepth];        // eligibility of the list's entries
  __shared__ int pool_j[kMmrMaxPool];                 // pool index -> list entry
  __shared__ int64_t seen[kSeenTile];
  __shared__ int wave_tot[kMmrWaves];
  __shared__ unsigned long long wave_best[kMmrWaves];
  __shared__ float ybuf[kMmrMaxDim];                  // the vector of the entry picked last
  constexpr int NV = ET > 0 ? ET : 1;
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* srow = scores + (int64_t)row * ld;
  const int64_t* prow = positions + (int64_t)row * depth;

  // phase 0: eligibility, the seen ids, the first `pool` eligible entries in list order
  for (int j = tid; j < depth; j += kMmrThreads) {
    const int64_t p = prow[j];
    surv[j] = (p >= 0 && p < n_items && srow[j] > -INFINITY) ? 1 : 0;
  }
  drop_seen<kMmrThreads>(surv, depth, [&](int j) { return prow[j]; }, ids, invalid + (int64_t)row * width, width, seen);
  __syncthreads();
  const int total = emit_first_k<kMmrThreads>(surv, depth, pool, wave_tot, [&](int j, int o) { pool_j[o] = j; }, [&](int) {});
  __syncthreads();
  const int P = total < pool ? total : pool;

  // thread c owns pool entry c: its score, its position, its vector (an entry of the pool is eligible, so its position is one of the table)
  const int c = tid;
  bool live = c < P;
  float s = 0.0f, M = 0.0f;
  int64_t p = -1;
  float v[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = 0.0f;
  float* wcol = nullptr;
  if (live) {
    const int j = pool_j[c];
    s = srow[j];
    p = prow[j];
    const float* vr = vectors + p * (int64_t)dim;
    if (ET > 0) {
#pragma unroll
      for (int e = 0; e < NV; ++e)
        if (e < dim) v[e] = vr[e];
    } else {
      wcol = ws + (int64_t)row * dim * pool + c;      // ws[row][e][c]
      for (int e = 0; e < dim; ++e) wcol[(int64_t)e * pool] = vr[e];
    }
  }

  const int kk = k < P ? k : P;
  const int ylen = ET > 0 ? ET : dim;                 // words of ybuf a step reads
  for (int t = 0; t < kk; ++t) {
    if (t > 0 && live) {                                // the similarity to the entry picked last: one chain, e ascending
      float acc = 0.0f;
      if (ET > 0) {
#pragma unroll
        for (int e = 0; e < NV; ++e) acc = acc + v[e] * ybuf[e];
      } else {
        for (int e = 0; e < dim; ++e) acc = acc + wcol[(int64_t)e * pool] * ybuf[e];
      }
      M = fmaxf(M, acc);
    }
    const float val = lam * s - mu * M;
    unsigned long long key = live ? make_key(val, (unsigned int)c) : 0ull;
    key = wave_max(key);
    if ((tid & 63) == 0) wave_best[tid >> 6] = key;
    __syncthreads();
    unsigned long long best = 0ull;
#pragma unroll
    for (int w = 0; w < kMmrWaves; ++w) {
      const unsigned long long o = wave_best[w];
      best = o > best ? o : best;
    }
    const int y = best != 0ull ? (int)key_pos(best) : 0;      // (t < P: an unpicked entry exists and its key is not 0; the test keeps y a pool index regardless)
    if (c == y) {
      live = false;
      out_scores[(int64_t)row * k + t] = s;
      out_pos[(int64_t)row * k + t] = p;
      out_ids[(int64_t)row * k + t] = ids != nullptr ? ids[p] : p;
    }
    if (t + 1 < kk) {
      const float* yr = vectors + prow[pool_j[y]] * (int64_t)dim;
      for (int e = tid; e < ylen; e += kMmrThreads) ybuf[e] = e < dim ? yr[e] : 0.0f;
    }
    __syncthreads();
  }
  for (int e = kk + tid; e < k; e += kMmrThreads) {
    out_scores[(int64_t)row * k + e] = -INFINITY;
    out_pos[(int64_t)row * k + e] = -1;
    out_ids[(int64_t)row * k + e] = -1;
  }
  if (tid == 0) {
    out_counts[row] = P;
    if (P < k) *out_of_range = 1;                       // every writer stores the same value
  }
}

size_t mmr_workspace_bytes(int rows, int pool, int dim) {
  return dim > kMmrRegDim ? sizeof(float) * (size_t)rows * (size_t)dim * (size_t)pool : 0;
}

int topk_mmr(const float* scores, int64_t ld, const int64_t* positions, int rows, int depth, const float* vectors, int64_t n_items, int dim,
             float lam, int k, int pool, const int64_t* ids, const int64_t* invalid, int width, void* ws, size_t ws_bytes, float* out_scores,
             int64_t* out_pos, int64_t* out_ids, int32_t* out_counts, int32_t* out_of_range, hipStream_t stream) {
  if (rows <= 0 || k <= 0) return kOk;
  if (depth < 1 || depth > kMmrMaxDepth) {
    set_error("topk_mmr: depth = %d outside [1, %d]", depth, kMmrMaxDepth);
    return kErrUnsupported;
  }
  if (pool < k || pool > kMmrMaxPool || dim < 1 || dim > kMmrMaxDim) {
    set_error("topk_mmr: need k <= pool <= %d and 1 <= dim <= %d (k = %d, pool = %d, dim = %d)", kMmrMaxPool, kMmrMaxDim, k, pool, dim);
    return kErrUnsupported;
  }
  if (ws_bytes < mmr_workspace_bytes(rows, pool, dim) || (dim > kMmrRegDim && ws == nullptr)) {
    set_error("topk_mmr: workspace of %zu bytes, %zu needed", ws_bytes, mmr_workspace_bytes(rows, pool, dim));
    return kErrInvalid;
  }
  const float mu = 1.0f - lam;
  const dim3 grid(rows), block(kMmrThreads);
#define RAILS_MMR_LAUNCH(ET)                                                                                                                      \
  hipLaunchKernelGGL(mmr_walk_kernel<ET>, grid, block, 0, stream, scores, ld, positions, depth, vectors, n_items, dim, lam, mu, k, pool, ids, invalid, \
                     width, static_cast<float*>(ws), out_scores, out_pos, out_ids, out_counts, out_of_range)
  if (dim <= 16) RAILS_MMR_LAUNCH(16);
  else if (dim <= 32) RAILS_MMR_LAUNCH(32);
  else if (dim <= kMmrRegDim) RAILS_MMR_LAUNCH(64);
  else RAILS_MMR_LAUNCH(0);
#undef RAILS_MMR_LAUNCH
  return launched();
}

}  // namespace mol
