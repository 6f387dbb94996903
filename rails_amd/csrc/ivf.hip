// Inverted-file (IVF-Flat) index over the item components: the native counterpart of MoLNaiveTopK(use_faiss=True)
// (reference rails/indexing/mol_top_k.py:176-239, which builds one faiss.IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT)
// per item group and searches it with nprobe = 1).  One independent index per item group m < P_X:
//
//   training   spherical Lloyd k-means on a sample of the fp16-rounded components (the host draws the sample), every iteration
//              assign (argmax inner product, ties to the lower list) -> stable counting sort of the sample by list -> per-list sums
//              in sample order -> divide -> split empty lists off the largest one (ties to the lower id, +-1/1024 per dimension as
//              FAISS's split does, without its random choice) -> l2-normalise.  No float atomics: the same inputs give the same bits.
//   lists      every item assigned in fp32 from its fp16-rounded values, then a stable counting sort (per-tile histograms, one
//              prefix sum over (list, tile), a scatter) writes per group: fp16 vectors in list order, int32 item positions alongside,
//              nlist + 1 offsets.  Items are read straight from the tile-packed fp32 item index (as component_build_kernel does).
//   search     three launches per slice of the batch: coarse (best lists of every (b, i, m) row by centroid score, continued past
//              nprobe in coarse-score order while the probed lists hold fewer than k items), scan (one workgroup per
//              (m, list, segment): the rows that probe the list find it there, so each probed list is read once per call), merge
//              (the partial top-k of every probe and segment -> k positions per row).  Tie rule everywhere: score desc, position asc.
//   filtered   the same three launches with the hidden set / a per-row tag filter INSIDE them: the filter gathered into list order once
//              (list words beside the positions), the eligible entries counted per (row, group, list); the coarse rule then counts eligible
//              entries, the scan offers eligible entries only -- the result is the plain search of the lists without the others.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "mol_kernels.h"
#include "mol_layout.h"

namespace mol {

namespace {

constexpr int kSortTile = 4096;        // items per histogram tile of the counting sort
constexpr int kMaxNlist = 4096;
constexpr int kMaxProbe = 64;
constexpr int kMaxK = 128;
constexpr int kSliceRows = 1024;       // query rows (b, i) per search slice: the scan's match list lives in LDS
constexpr int kScanUnits = 16384;      // (probe, segment) work units the scan aims for
constexpr int kScanBlocks = 65536;     // cap on the scan grid (most of its blocks find no probe and leave)
constexpr float kSplitEps = 1.0f / 1024.0f;

__device__ __forceinline__ float h2f(unsigned short h) { return (float)__builtin_bit_cast(_Float16, h); }
__device__ __forceinline__ unsigned short f2h(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }

// Four consecutive dims [4c + (d/2) hi, +4) of item `item`, group m, from the tile-packed fp32 index (mol_layout.h fragment order).
__device__ __forceinline__ float4 index_quad(const float* ipack, int64_t item, int PQ, int PX, int d, int m, int q) {
  const int hi = q >= d / 8, c = q - hi * (d / 8);
  const float* tEx = ipack + (item >> 5) * (int64_t)(kTileItems * (PX * d + PQ * PX));
  return *reinterpret_cast<const float4*>(tEx + ex_slot(d, (int)(item & 31), m, c, hi) * 4);
}

// dims 4q .. 4q+3 of the fp16-rounded component, as fp16 bits
__device__ __forceinline__ uint2 index_quad16(const float* ipack, int64_t item, int PQ, int PX, int d, int m, int q) {
  const float4 v = index_quad(ipack, item, PQ, PX, d, m, q);
  return make_uint2((unsigned)f2h(v.x) | ((unsigned)f2h(v.y) << 16), (unsigned)f2h(v.z) | ((unsigned)f2h(v.w) << 16));
}

struct Src {                 // the points of a counting sort / an assignment: a (G, n, d) fp16 table, or the item index
  const unsigned short* x16;
  const float* ipack;
  int PQ, PX;
};

template <int D>
__device__ __forceinline__ void load_point(const Src& src, int m, int64_t n, int64_t p, float* x) {
  if (src.x16) {
    const uint4* r = reinterpret_cast<const uint4*>(src.x16 + ((int64_t)m * n + p) * D);
#pragma unroll
    for (int c = 0; c < D / 8; ++c) {
      const uint4 v = r[c];
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        x[8 * c + 2 * j] = h2f((unsigned short)(w[j] & 0xffff));
        x[8 * c + 2 * j + 1] = h2f((unsigned short)(w[j] >> 16));
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < D / 4; ++q) {
      const uint2 v = index_quad16(src.ipack, p, src.PQ, src.PX, D, m, q);
      x[4 * q] = h2f((unsigned short)(v.x & 0xffff));
      x[4 * q + 1] = h2f((unsigned short)(v.x >> 16));
      x[4 * q + 2] = h2f((unsigned short)(v.y & 0xffff));
      x[4 * q + 3] = h2f((unsigned short)(v.y >> 16));
    }
  }
}

// ---- training / build kernels ---------------------------------------------------------------------------------------------------

// out[m][s][:] = fp16(Ex[pos[s], m, :]), from the fp32-format index or (src16 != NULL) the (PX, n, d) fp16 component table
__global__ void mol_ivf_gather_kernel(const float* __restrict__ ipack, const unsigned short* __restrict__ src16, int64_t n, int PQ, int PX, int d,
                                      const int32_t* __restrict__ pos, int S, unsigned short* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int qn = d / 4;
  if (i >= (int64_t)PX * S * qn) return;
  const int q = (int)(i % qn);
  const int64_t ms = i / qn;
  const int s = (int)(ms % S), m = (int)(ms / S);
  *reinterpret_cast<uint2*>(out + ms * d + 4 * q) =
      src16 ? *reinterpret_cast<const uint2*>(src16 + ((int64_t)m * n + pos[s]) * d + 4 * q) : index_quad16(ipack, pos[s], PQ, PX, d, m, q);
}

// table[m][first + x][:] = fp16(Ex[x, m, :]) for the n items of an fp32-format index (chunk)
__global__ void mol_ivf_components16_kernel(const float* __restrict__ ipack, int64_t n, int PQ, int PX, int d, int64_t n_total, int64_t first,
                                            unsigned short* __restrict__ table) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int qn = d / 4;
  if (i >= n * PX * qn) return;
  const int q = (int)(i % qn);
  const int64_t xm = i / qn;
  const int m = (int)(xm % PX);
  const int64_t x = xm / PX;
  *reinterpret_cast<uint2*>(table + ((int64_t)m * n_total + first + x) * d + 4 * q) = index_quad16(ipack, x, PQ, PX, d, m, q);
}

// centroids[m][l][:] = sample[m][l][:] (l < nlist)
__global__ void mol_ivf_init_kernel(const unsigned short* __restrict__ x16, int S, int d, int nlist, int G, float* __restrict__ cent) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)G * nlist * d) return;
  const int dd = (int)(i % d);
  const int64_t ml = i / d;
  const int l = (int)(ml % nlist), m = (int)(ml / nlist);
  cent[i] = h2f(x16[((int64_t)m * S + l) * d + dd]);
}

// key of one inserted entry of a list edit: (list, position) order, the row of the edit's source in the low bits (positions are unique, so
// the row never decides an order)
constexpr int kEditMax = 16384;        // inserted entries per list edit: one rails_sort_rows_i64 row
__device__ __forceinline__ int64_t edit_key(int list, int64_t pos, int row) { return ((int64_t)list << 45) | ((pos & 0x7fffffffLL) << 14) | (int64_t)row; }

// argmax_l <x_p, c_l> (fp32, dims in order; ties to the lower l) of 256 points of one group per block; the centroids pass through LDS in
// chunks (every lane reads the same centroid: broadcast).  One body, two addressing modes: point p is item p of `src` and its list goes
// to assign[m][p]; or (kIndexed) point p is entry p of a list edit -- item pos[p] of the fp32-format index `src` (src_in_place) or its
// item p -- and edit_key(list, pos[p], p) goes to keys[m][p].
template <int D, bool kIndexed>
__device__ __forceinline__ void ivf_assign_body(const Src& src, int64_t n, const float* __restrict__ cent, int nlist, int32_t* __restrict__ assign,
                                                int src_in_place, const int64_t* __restrict__ pos, int64_t* __restrict__ keys) {
  constexpr int kChunk = 8192 / D;
  __shared__ float4 sc[kChunk * D / 4];
  const int m = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float x[D];
  if (p < n) load_point<D>(src, m, n, kIndexed && src_in_place ? pos[p] : p, x);
  else
    for (int j = 0; j < D; ++j) x[j] = 0.0f;
  float best = -INFINITY;
  int arg = 0;
  const float4* cm = reinterpret_cast<const float4*>(cent + (int64_t)m * nlist * D);
  for (int l0 = 0; l0 < nlist; l0 += kChunk) {
    const int nc = min(kChunk, nlist - l0);
    __syncthreads();
    for (int i = threadIdx.x; i < nc * D / 4; i += 256) sc[i] = cm[(int64_t)l0 * (D / 4) + i];
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
      float acc = 0.0f;
#pragma unroll
      for (int q = 0; q < D / 4; ++q) {
        const float4 v = sc[c * (D / 4) + q];
        acc = fmaf(x[4 * q], v.x, acc);
        acc = fmaf(x[4 * q + 1], v.y, acc);
        acc = fmaf(x[4 * q + 2], v.z, acc);
        acc = fmaf(x[4 * q + 3], v.w, acc);
      }
      if (acc > best) { best = acc; arg = l0 + c; }
    }
  }
  if (p < n) {
    if (kIndexed) keys[(int64_t)m * n + p] = edit_key(arg, pos[p], (int)p);
    else assign[(int64_t)m * n + p] = arg;
  }
}

template <int D>
__global__ __launch_bounds__(256) void mol_ivf_assign_kernel(Src src, int64_t n, const float* __restrict__ cent, int nlist,
                                                             int32_t* __restrict__ assign) {
  ivf_assign_body<D, false>(src, n, cent, nlist, assign, 1, nullptr, nullptr);
}

template <int D>
__global__ __launch_bounds__(256) void mol_ivf_assign_indexed_kernel(Src src, int src_in_place, const int64_t* __restrict__ pos, int64_t m_ins,
                                                                     const float* __restrict__ cent, int nlist, int64_t* __restrict__ keys) {
  ivf_assign_body<D, true>(src, m_ins, cent, nlist, nullptr, src_in_place, pos, keys);
}

// hist[m][l][t] = #{items of tile t in list l}
__global__ __launch_bounds__(256) void mol_ivf_hist_kernel(const int32_t* __restrict__ assign, int64_t n, int nlist, int tiles,
                                                           int32_t* __restrict__ hist) {
  __shared__ int h[kMaxNlist];
  const int m = blockIdx.y, t = blockIdx.x;
  for (int l = threadIdx.x; l < nlist; l += 256) h[l] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)t * kSortTile, hi = min(n, lo + kSortTile);
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) atomicAdd(&h[assign[(int64_t)m * n + i]], 1);   // integer counts: order-free
  __syncthreads();
  for (int l = threadIdx.x; l < nlist; l += 256) hist[((int64_t)m * nlist + l) * tiles + t] = h[l];
}

// exclusive prefix sum of hist[m][.][.] in place; offsets[m][l] = start of list l, offsets[m][nlist] = n
__global__ __launch_bounds__(1024) void mol_ivf_prefix_kernel(int32_t* __restrict__ hist, int nlist, int tiles, int64_t n,
                                                              int32_t* __restrict__ offsets) {
  __shared__ int buf[1024];
  __shared__ int carry;
  const int m = blockIdx.x;
  int32_t* h = hist + (int64_t)m * nlist * tiles;
  const int64_t len = (int64_t)nlist * tiles;
  if (threadIdx.x == 0) carry = 0;
  for (int64_t base = 0; base < len; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const int v = i < len ? h[i] : 0;
    __syncthreads();
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {      // Hillis-Steele inclusive scan
      const int add = threadIdx.x >= (unsigned)o ? buf[threadIdx.x - o] : 0;
      __syncthreads();
      buf[threadIdx.x] += add;
      __syncthreads();
    }
    const int excl = carry + buf[threadIdx.x] - v;
    if (i < len) {
      h[i] = excl;
      if (i % tiles == 0) offsets[(int64_t)m * (nlist + 1) + i / tiles] = excl;
    }
    __syncthreads();
    if (threadIdx.x == 1023) carry += buf[1023];
  }
  if (threadIdx.x == 0) offsets[(int64_t)m * (nlist + 1) + nlist] = (int32_t)n;
}

// Stable scatter: one wave per (tile, group).  Items of a tile go out in index order, 64 at a time; the lanes of one list (peeled by
// ballot) take consecutive slots from the list's running cursor.  order[m][slot] = item; vec16 (optional): its fp16 vector.
template <int D>
__global__ __launch_bounds__(64) void mol_ivf_scatter_kernel(Src src, const int32_t* __restrict__ assign, int64_t n, int nlist, int tiles,
                                                             const int32_t* __restrict__ hist, int32_t* __restrict__ order,
                                                             unsigned short* __restrict__ vec16) {
  __shared__ int cursor[kMaxNlist];
  const int m = blockIdx.y, t = blockIdx.x, lane = threadIdx.x;
  for (int l = lane; l < nlist; l += 64) cursor[l] = hist[((int64_t)m * nlist + l) * tiles + t];
  __syncthreads();
  const int64_t lo = (int64_t)t * kSortTile, hi = min(n, lo + kSortTile);
  for (int64_t i0 = lo; i0 < hi; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool valid = i < hi;
    const int l = valid ? assign[(int64_t)m * n + i] : -1;
    unsigned long long left = __ballot(valid);
    int slot = 0;
    while (left) {
      const int leader = __ffsll((long long)left) - 1;
      const int L = __shfl(l, leader, 64);
      const unsigned long long same = __ballot(valid && l == L);
      int base = 0;
      if (lane == leader) {
        base = cursor[L];
        cursor[L] = base + (int)__popcll(same);
      }
      base = __shfl(base, leader, 64);
      if (valid && l == L) slot = base + (int)__popcll(same & ((1ull << lane) - 1ull));
      left &= ~same;
    }
    if (valid) {
      order[(int64_t)m * n + slot] = (int32_t)i;
      if (vec16) {
        uint2* dst = reinterpret_cast<uint2*>(vec16 + ((int64_t)m * n + slot) * D);
#pragma unroll
        for (int q = 0; q < D / 4; ++q)
          dst[q] = src.x16 ? *reinterpret_cast<const uint2*>(src.x16 + ((int64_t)m * n + i) * D + 4 * q) : index_quad16(src.ipack, i, src.PQ, src.PX, D, m, q);
      }
    }
  }
}

// Per-list means of the sample in sorted (list, sample index) order; sizes[m][l] = member count (float, as FAISS's hassign).
__global__ __launch_bounds__(128) void mol_ivf_mean_kernel(const unsigned short* __restrict__ x16, int S, int d, const int32_t* __restrict__ order,
                                                           const int32_t* __restrict__ offsets, int nlist, float* __restrict__ cent,
                                                           float* __restrict__ sizes) {
  const int l = blockIdx.x, m = blockIdx.y, dd = threadIdx.x;
  const int32_t* off = offsets + (int64_t)m * (nlist + 1);
  const int b = off[l], e = off[l + 1];
  if (dd == 0) sizes[(int64_t)m * nlist + l] = (float)(e - b);
  if (dd >= d || e == b) return;
  float acc = 0.0f;
  for (int j = b; j < e; ++j) acc += h2f(x16[((int64_t)m * S + order[(int64_t)m * S + j]) * d + dd]);
  cent[((int64_t)m * nlist + l) * d + dd] = acc / (float)(e - b);
}

// Empty lists split off the largest (FAISS split_clusters with the largest list instead of a random draw), then every centroid
// is l2-normalised.  One workgroup per group; lists are visited in ascending order.
__global__ __launch_bounds__(256) void mol_ivf_finish_kernel(float* __restrict__ cent, const float* __restrict__ sizes_in, int nlist, int d) {
  __shared__ float sz[kMaxNlist];
  __shared__ float rv[4];
  __shared__ int ri[4];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* c = cent + (int64_t)m * nlist * d;
  for (int l = tid; l < nlist; l += 256) sz[l] = sizes_in[(int64_t)m * nlist + l];
  __syncthreads();
  for (int ci = 0; ci < nlist; ++ci) {
    if (sz[ci] != 0.0f) continue;                          // uniform: sz is read after the last barrier
    float bv = -1.0f;
    int bi = 0;
    for (int l = tid; l < nlist; l += 256)
      if (sz[l] > bv) { bv = sz[l]; bi = l; }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
    __syncthreads();
    int cj = ri[0];
    float vj = rv[0];
    for (int w = 1; w < 4; ++w)
      if (rv[w] > vj || (rv[w] == vj && ri[w] < cj)) { vj = rv[w]; cj = ri[w]; }
    for (int dd = tid; dd < d; dd += 256) {
      const float v = c[(int64_t)cj * d + dd];
      c[(int64_t)ci * d + dd] = (dd & 1) ? v * (1.0f - kSplitEps) : v * (1.0f + kSplitEps);
      c[(int64_t)cj * d + dd] = (dd & 1) ? v * (1.0f + kSplitEps) : v * (1.0f - kSplitEps);
    }
    __syncthreads();
    if (tid == 0) {
      sz[ci] = sz[cj] / 2.0f;
      sz[cj] -= sz[ci];
    }
    __syncthreads();
  }
  for (int l = wave; l < nlist; l += 4) {                 // one wave per centroid: fixed butterfly, so the norm is reproducible
    float* r = c + (int64_t)l * d;
    const float a = lane < d ? r[lane] : 0.0f, b = lane + 64 < d ? r[lane + 64] : 0.0f;
    float ss = fmaf(a, a, b * b);
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float inv = 1.0f / sqrtf(ss);
    if (lane < d) r[lane] = a * inv;
    if (lane + 64 < d) r[lane + 64] = b * inv;
  }
}

// ---- list edit kernels (frozen centroids) ------------------------------------------------------------------------------------------
// The lists after an edit = the kept old entries and the inserted ones, merged in (list, position) order.  A kept old slot s moves to
// K[s] + (inserted entries before it); sorted inserted entry j goes to j + K[s*], s* its lower bound among the old slots of its list.

// number of keys[0..m) below `key` (keys ascending)
__device__ __forceinline__ int keys_below(const int64_t* __restrict__ keys, int m, int64_t key) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// an old entry stays: its position is below n_lim = min(n_old, n_keep) and is not replaced by the edit
__device__ __forceinline__ bool edit_kept(int p, int64_t n_lim, const unsigned char* __restrict__ drop) { return p >= 0 && p < n_lim && drop[p] == 0; }

// drop[p] = 1 for the edit's positions inside the old corpus (drop is zeroed before)
__global__ void mol_ivf_edit_mask_kernel(const int64_t* __restrict__ pos, int m, int64_t n_old, unsigned char* __restrict__ drop) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int64_t p = pos[j];
  if (p >= 0 && p < n_old) drop[p] = 1;
}

// counts[g][t] = kept slots of tile t (kSortTile old slots) of group g
__global__ __launch_bounds__(256) void mol_ivf_edit_count_kernel(const int32_t* __restrict__ old_pos, int64_t n_old, int64_t n_lim,
                                                                 const unsigned char* __restrict__ drop, int tiles, int32_t* __restrict__ counts) {
  __shared__ int wsum[4];
  const int g = blockIdx.y, t = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t lo = (int64_t)t * kSortTile, hi = min(n_old, lo + kSortTile);
  int c = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) c += edit_kept(old_pos[(int64_t)g * n_old + i], n_lim, drop) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) wsum[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[(int64_t)g * tiles + t] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// K[g][s] = kept slots of group g before old slot s (s <= n_old), from the tiles' exclusive prefix sums `base`
__global__ __launch_bounds__(256) void mol_ivf_edit_scan_kernel(const int32_t* __restrict__ old_pos, int64_t n_old, int64_t n_lim,
                                                                const unsigned char* __restrict__ drop, int tiles, const int32_t* __restrict__ base,
                                                                int32_t* __restrict__ K) {
  __shared__ int wcount[4];
  const int g = blockIdx.y, t = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t lo = (int64_t)t * kSortTile, hi = min(n_old, lo + kSortTile);
  int32_t* Kg = K + (int64_t)g * (n_old + 1);
  int carry = base[(int64_t)g * tiles + t];
  for (int64_t i0 = lo; i0 < hi; i0 += 256) {          // (uniform trip count: lo and hi are the block's)
    const int64_t i = i0 + threadIdx.x;
    const bool kept = i < hi && edit_kept(old_pos[(int64_t)g * n_old + i], n_lim, drop);
    const unsigned long long b = __ballot(kept);
    __syncthreads();
    if (lane == 0) wcount[wave] = (int)__popcll(b);
    __syncthreads();
    int before = (int)__popcll(b & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += wcount[w];
      total += wcount[w];
    }
    if (i < hi) Kg[i] = carry + before;
    carry += total;
  }
  if (t == tiles - 1 && threadIdx.x == 0) Kg[n_old] = carry;
}

// Move: block = 256 old slots of one group.  Every kept slot finds its list (the last l with old_off[l] <= s) and its new slot, writes
// its position there; then the block copies the vectors 16 bytes per lane.
template <int D>
__global__ __launch_bounds__(256) void mol_ivf_edit_move_kernel(const unsigned short* __restrict__ old_vec, const int32_t* __restrict__ old_pos,
                                                                const int32_t* __restrict__ old_off, int64_t n_old, int64_t n_lim, int nlist,
                                                                const unsigned char* __restrict__ drop, const int32_t* __restrict__ K,
                                                                const int64_t* __restrict__ keys, int m_ins, unsigned short* __restrict__ new_vec,
                                                                int32_t* __restrict__ new_pos, int64_t n_new) {
  __shared__ int dst[256];
  const int g = blockIdx.y;
  const int64_t s0 = (int64_t)blockIdx.x * 256, s = s0 + threadIdx.x;
  int to = -1;
  if (s < n_old) {
    const int p = old_pos[(int64_t)g * n_old + s];
    if (edit_kept(p, n_lim, drop)) {
      const int32_t* off = old_off + (int64_t)g * (nlist + 1);
      int lo = 0, hi = nlist;                           // off[lo] <= s < off[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= s) lo = mid;
        else hi = mid;
      }
      const int64_t t = (int64_t)K[(int64_t)g * (n_old + 1) + s] + keys_below(keys + (int64_t)g * m_ins, m_ins, edit_key(lo, p, 0));
      if (t < n_new) {                                  // (always, for the n_new of the header's formula)
        to = (int)t;
        new_pos[(int64_t)g * n_new + t] = p;
      }
    }
  }
  dst[threadIdx.x] = to;
  __syncthreads();
  constexpr int C = D / 8;
  const uint4* src = reinterpret_cast<const uint4*>(old_vec) + ((int64_t)g * n_old + s0) * C;
  uint4* out = reinterpret_cast<uint4*>(new_vec) + (int64_t)g * n_new * C;
  for (int i = threadIdx.x; i < 256 * C; i += 256) {
    const int r = i / C, c = i - r * C;
    if (dst[r] >= 0) out[(int64_t)dst[r] * C + c] = src[(int64_t)r * C + c];
  }
}

// Insert: one lane per sorted inserted entry (list, position, row): its position and its fp16 vector, cut from the fp32-format index
// `src` (item `position` when src_in_place, else item `row`), at slot j + K[s*].
template <int D>
__global__ __launch_bounds__(256) void mol_ivf_edit_insert_kernel(const float* __restrict__ src, int src_in_place, int PQ, int PX,
                                                                  const int64_t* __restrict__ keys, int m_ins, const int32_t* __restrict__ old_pos,
                                                                  const int32_t* __restrict__ old_off, int64_t n_old, int nlist,
                                                                  const int32_t* __restrict__ K, unsigned short* __restrict__ new_vec,
                                                                  int32_t* __restrict__ new_pos, int64_t n_new) {
  const int g = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m_ins) return;
  const int64_t key = keys[(int64_t)g * m_ins + j];
  const int l = (int)(key >> 45), row = (int)(key & (kEditMax - 1));
  const int p = (int)((key >> 14) & 0x7fffffffLL);
  if (l < 0 || l >= nlist) return;
  const int32_t* off = old_off + (int64_t)g * (nlist + 1);
  int64_t lo = max(0, off[l]), hi = min(n_old, (int64_t)off[l + 1]);
  while (lo < hi) {                                     // old positions ascend inside a list, dropped entries included
    const int64_t mid = (lo + hi) >> 1;
    if (old_pos[(int64_t)g * n_old + mid] < p) lo = mid + 1;
    else hi = mid;
  }
  const int64_t t = (int64_t)j + K[(int64_t)g * (n_old + 1) + lo];
  if (t >= n_new) return;                               // (never, for the n_new of the header's formula)
  new_pos[(int64_t)g * n_new + t] = p;
  const int64_t item = src_in_place ? p : row;
  uint2* out = reinterpret_cast<uint2*>(new_vec + ((int64_t)g * n_new + t) * D);
#pragma unroll
  for (int q = 0; q < D / 4; ++q) out[q] = index_quad16(src, item, PQ, PX, D, g, q);
}

// new_off[g][l] = kept slots before old list l + inserted entries of lower lists; new_off[g][nlist] = n_new
__global__ void mol_ivf_edit_offsets_kernel(const int32_t* __restrict__ old_off, int nlist, int G, int64_t n_old, const int32_t* __restrict__ K,
                                            const int64_t* __restrict__ keys, int m_ins, int64_t n_new, int32_t* __restrict__ new_off) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G * (nlist + 1)) return;
  const int g = i / (nlist + 1), l = i - g * (nlist + 1);
  if (l == nlist) { new_off[i] = (int32_t)n_new; return; }
  const int64_t s = min(n_old, (int64_t)max(0, old_off[i]));
  new_off[i] = K[(int64_t)g * (n_old + 1) + s] + keys_below(keys + (int64_t)g * m_ins, m_ins, edit_key(l, 0, 0));
}

// ---- search kernels ------------------------------------------------------------------------------------------------------------

// (score, position) order: a before b iff a.s > b.s, or equal scores and a.p < b.p
__device__ __forceinline__ bool before(float as, int ap, float bs, int bp) { return as > bs || (as == bs && ap < bp); }

// A running top-(64 KS) list spread over a wave: lane l holds ranks l (s0, p0) and 64 + l (s1, p1), sorted.
template <int KS>
struct WaveTopK {
  float s0 = -INFINITY, s1 = -INFINITY;
  int p0 = 0x7fffffff, p1 = 0x7fffffff;
  __device__ __forceinline__ void kth(int k, float& ks, int& kp) const {
    const int src = (k - 1) & 63;
    if (KS == 2 && k > 64) { ks = __shfl(s1, src, 64); kp = __shfl(p1, src, 64); }
    else { ks = __shfl(s0, src, 64); kp = __shfl(p0, src, 64); }
  }
  __device__ __forceinline__ void insert(float cs, int cp, int lane) {   // wave-uniform candidate
    int rank = (int)__popcll(__ballot(before(s0, p0, cs, cp)));
    if (KS == 2) rank += (int)__popcll(__ballot(before(s1, p1, cs, cp)));
    const float u0 = __shfl(s0, (lane + 63) & 63, 64);
    const int q0 = __shfl(p0, (lane + 63) & 63, 64);
    if (KS == 2) {
      const float u1 = __shfl(s1, (lane + 63) & 63, 64);
      const int q1 = __shfl(p1, (lane + 63) & 63, 64);
      const int r1 = 64 + lane;
      if (r1 == rank) { s1 = cs; p1 = cp; }
      else if (r1 > rank) { s1 = lane == 0 ? u0 : u1; p1 = lane == 0 ? q0 : q1; }   // rank 64 takes rank 63 (lane 63 of slot 0)
    }
    if (lane == rank) { s0 = cs; p0 = cp; }
    else if (lane > rank) { s0 = u0; p0 = q0; }
  }
  // offer one candidate per lane (valid lanes only)
  __device__ __forceinline__ void offer(bool valid, float s, int p, int k, int lane) {
    float ks;
    int kp;
    kth(k, ks, kp);
    unsigned long long want = __ballot(valid && before(s, p, ks, kp));
    while (want) {
      const int leader = __ffsll((long long)want) - 1;
      want &= want - 1;
      const float cs = __shfl(s, leader, 64);
      const int cp = __shfl(p, leader, 64);
      kth(k, ks, kp);
      if (before(cs, cp, ks, kp)) insert(cs, cp, lane);
    }
  }
};

// Coarse: one workgroup per row (b, i, m).  Scores every centroid, then takes lists best-first until nprobe are taken and they hold at
// least k items (the short-list rule), at most max_probes.  probes[row][r] (-1 beyond), nprob[row].
// kFiltered ("filtered lists"): the rule counts the items the row's filter keeps in a list -- counts[r][m][l], r = 0 for
// a filter shared by the batch (count_rows == 1), else the row's query b = qrow / PQ -- where the plain kernel counts the list's entries.
template <int D, bool kFiltered>
__device__ __forceinline__ void ivf_coarse_body(const float* __restrict__ eq, int G, const float* __restrict__ cent, int nlist,
                                                const int32_t* __restrict__ offsets, int nprobe, int k, int max_probes, int32_t* __restrict__ probes,
                                                int32_t* __restrict__ nprob, int32_t* __restrict__ unfilled, const int32_t* __restrict__ counts,
                                                int count_rows, int PQ) {
  __shared__ float sc[kMaxNlist];
  __shared__ float rv[4];
  __shared__ int ri[4];
  const int row = blockIdx.x, m = row % G, qrow = row / G;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (unfilled && row == 0 && tid == 0) *unfilled = 0;
  const float* q = eq + (int64_t)qrow * D;
  float x[D];
#pragma unroll
  for (int j = 0; j < D; ++j) x[j] = q[j];
  const float* cm = cent + (int64_t)m * nlist * D;
  for (int l = tid; l < nlist; l += 256) {
    const float4* c4 = reinterpret_cast<const float4*>(cm + (int64_t)l * D);
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < D / 4; ++j) {
      const float4 v = c4[j];
      acc = fmaf(x[4 * j], v.x, acc);
      acc = fmaf(x[4 * j + 1], v.y, acc);
      acc = fmaf(x[4 * j + 2], v.z, acc);
      acc = fmaf(x[4 * j + 3], v.w, acc);
    }
    sc[l] = acc != acc ? -INFINITY : acc;       // a NaN query still takes lists (in id order): every row gets k items
  }
  const int32_t* off = kFiltered ? counts + ((int64_t)(count_rows == 1 ? 0 : qrow / PQ) * G + m) * nlist : offsets + (int64_t)m * (nlist + 1);
  int32_t* out = probes + (int64_t)row * max_probes;
  int taken = 0;
  int64_t held = 0;
  __syncthreads();
  while (taken < max_probes) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int l = tid; l < nlist; l += 256) {
      const float v = sc[l];
      if (v > bv || (v == bv && l < bi)) { bv = v; bi = l; }     // a taken list holds NaN and never compares greater
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
    __syncthreads();
    int L = ri[0];
    float vL = rv[0];
    for (int w = 1; w < 4; ++w)
      if (rv[w] > vL || (rv[w] == vL && ri[w] < L)) { vL = rv[w]; L = ri[w]; }
    if (L >= nlist) break;                                 // every list taken (cannot happen with max_probes <= nlist)
    held += kFiltered ? off[L] : off[L + 1] - off[L];
    if (tid == 0) { out[taken] = L; sc[L] = NAN; }
    ++taken;
    __syncthreads();
    if (taken >= nprobe && held >= k) break;
  }
  for (int r = taken + tid; r < max_probes; r += 256) out[r] = -1;
  if (tid == 0) nprob[row] = taken;
}

template <int D>
__global__ __launch_bounds__(256) void mol_ivf_coarse_kernel(const float* __restrict__ eq, int G, const float* __restrict__ cent, int nlist,
                                                             const int32_t* __restrict__ offsets, int nprobe, int k, int max_probes,
                                                             int32_t* __restrict__ probes, int32_t* __restrict__ nprob, int32_t* __restrict__ unfilled) {
  ivf_coarse_body<D, false>(eq, G, cent, nlist, offsets, nprobe, k, max_probes, probes, nprob, unfilled, nullptr, 1, 1);
}

template <int D>
__global__ __launch_bounds__(256) void mol_ivf_coarse_filtered_kernel(const float* __restrict__ eq, int G, const float* __restrict__ cent, int nlist,
                                                                      const int32_t* __restrict__ counts, int count_rows, int PQ, int nprobe, int k,
                                                                      int max_probes, int32_t* __restrict__ probes, int32_t* __restrict__ nprob,
                                                                      int32_t* __restrict__ unfilled) {
  ivf_coarse_body<D, true>(eq, G, cent, nlist, nullptr, nprobe, k, max_probes, probes, nprob, unfilled, counts, count_rows, PQ);
}

// Scan: workgroup (segment, list, group).  Collects the probes of this list (at most one per query row), then each wave runs one
// probe over the segment's items at a time: fp32 dot of the query with the fp16 vectors (dims in order), running top-k.
// part_s / part_p [(row * max_probes + r) * n_seg + seg][k].
// kFiltered: an entry whose word in list_words (the filter in list order, beside `pos`) shares no bit with the allow word of the probe's query
// (allowed[slot / max_probes / G / PQ], wave-uniform) is not offered, and its vector is not read; a segment without an eligible entry leaves
// the sentinels (-inf, 0x7fffffff), which the merge never takes.
template <int D, int KS, bool kFiltered>
__device__ __forceinline__ void ivf_scan_body(const float* __restrict__ eq, int qrows, int G, int nlist, const unsigned short* __restrict__ vec16,
                                              const int32_t* __restrict__ pos, const int32_t* __restrict__ offsets, int64_t n,
                                              const int32_t* __restrict__ probes, int max_probes, int seg_items, int n_seg, int k,
                                              float* __restrict__ part_s, int32_t* __restrict__ part_p, const uint32_t* __restrict__ list_words,
                                              const uint32_t* __restrict__ allowed, int PQ) {
  __shared__ int match[kSliceRows];
  __shared__ int n_match;
  const int seg = blockIdx.x, l = blockIdx.y, m = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* off = offsets + (int64_t)m * (nlist + 1);
  const int lb = off[l], size = off[l + 1] - lb;
  const int s0 = seg * seg_items, s1 = min(size, s0 + seg_items);
  if (s0 >= s1) return;
  if (tid == 0) n_match = 0;
  __syncthreads();
  for (int e = tid; e < qrows * max_probes; e += 256) {
    const int qr = e / max_probes, r = e - qr * max_probes;
    const int slot = (qr * G + m) * max_probes + r;
    if (probes[slot] == l) match[atomicAdd(&n_match, 1)] = slot;   // order of the list is free: every probe writes its own slot
  }
  __syncthreads();
  const int nm = n_match;
  const int64_t base = (int64_t)m * n + lb;
  for (int j = wave; j < nm; j += 4) {
    const int slot = __builtin_amdgcn_readfirstlane(match[j]);
    const float* q = eq + (int64_t)(slot / max_probes / G) * D;
    float x[D];
#pragma unroll
    for (int t = 0; t < D; ++t) x[t] = q[t];
    uint32_t aw = 0;
    if (kFiltered) aw = allowed[slot / max_probes / G / PQ];
    WaveTopK<KS> top;
    for (int i0 = s0; i0 < s1; i0 += 64) {
      const int i = i0 + lane;
      bool valid = i < s1;
      if (kFiltered) valid = valid && (list_words[base + i] & aw) != 0u;
      float acc = 0.0f;
      int p = 0;
      if (valid) {
        const uint4* r = reinterpret_cast<const uint4*>(vec16 + (base + i) * D);
#pragma unroll
        for (int c = 0; c < D / 8; ++c) {
          const uint4 v = r[c];
          const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            acc = fmaf(x[8 * c + 2 * h], h2f((unsigned short)(w[h] & 0xffff)), acc);
            acc = fmaf(x[8 * c + 2 * h + 1], h2f((unsigned short)(w[h] >> 16)), acc);
          }
        }
        p = pos[base + i];
        if (acc != acc) acc = -INFINITY;          // NaN ranks last but still fills the list
      }
      top.offer(valid, acc, p, k, lane);
    }
    const int64_t o = ((int64_t)slot * n_seg + seg) * k;
    if (lane < k) { part_s[o + lane] = top.s0; part_p[o + lane] = top.p0; }
    if (KS == 2 && 64 + lane < k) { part_s[o + 64 + lane] = top.s1; part_p[o + 64 + lane] = top.p1; }
  }
}

template <int D, int KS>
__global__ __launch_bounds__(256) void mol_ivf_scan_kernel(const float* __restrict__ eq, int qrows, int G, int nlist, const unsigned short* __restrict__ vec16,
                                                           const int32_t* __restrict__ pos, const int32_t* __restrict__ offsets, int64_t n,
                                                           const int32_t* __restrict__ probes, int max_probes, int seg_items, int n_seg, int k,
                                                           float* __restrict__ part_s, int32_t* __restrict__ part_p) {
  ivf_scan_body<D, KS, false>(eq, qrows, G, nlist, vec16, pos, offsets, n, probes, max_probes, seg_items, n_seg, k, part_s, part_p, nullptr, nullptr, 1);
}

template <int D, int KS>
__global__ __launch_bounds__(256) void mol_ivf_scan_filtered_kernel(const float* __restrict__ eq, int qrows, int G, int nlist,
                                                                    const unsigned short* __restrict__ vec16, const int32_t* __restrict__ pos,
                                                                    const int32_t* __restrict__ offsets, int64_t n, const int32_t* __restrict__ probes,
                                                                    int max_probes, int seg_items, int n_seg, int k, float* __restrict__ part_s,
                                                                    int32_t* __restrict__ part_p, const uint32_t* __restrict__ list_words,
                                                                    const uint32_t* __restrict__ allowed, int PQ) {
  ivf_scan_body<D, KS, true>(eq, qrows, G, nlist, vec16, pos, offsets, n, probes, max_probes, seg_items, n_seg, k, part_s, part_p, list_words, allowed, PQ);
}

// ---- the filter in list order (filtered lists) ---------------------------------------------------------------------------------------

// list_words[m][slot] = word(pos[m][slot]): the item's effective tag word, or (no tags) all ones for a visible item and 0 for a hidden one
__global__ void mol_ivf_list_words_kernel(const int32_t* __restrict__ pos, int64_t total, int64_t n, const uint32_t* __restrict__ eff,
                                          const uint32_t* __restrict__ visible, uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int p = pos[i];
  uint32_t w = 0u;
  if (p >= 0 && p < n) w = eff ? eff[p] : (((visible[p >> 5] >> (p & 31)) & 1u) ? 0xffffffffu : 0u);
  out[i] = w;
}

// counts[r][m][l] = entries of list l of group m whose word shares a bit with allowed[r].  One workgroup per (list, group); 64 allow words at
// a time sit in LDS, every 64-entry chunk of the list is tested against each (ballot + popcount, the sum kept by the lane of the word's
// index); the four waves' sums meet in LDS.  No atomics.
__global__ __launch_bounds__(256) void mol_ivf_list_counts_kernel(const uint32_t* __restrict__ list_words, const int32_t* __restrict__ offsets, int64_t n,
                                                                  int nlist, int G, const uint32_t* __restrict__ allowed, int R,
                                                                  int32_t* __restrict__ counts) {
  __shared__ uint32_t aw[64];
  __shared__ int wsum[4][64];
  const int l = blockIdx.x, m = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* off = offsets + (int64_t)m * (nlist + 1);
  const int lb = off[l], size = off[l + 1] - lb;
  const uint32_t* lw = list_words + (int64_t)m * n + lb;
  for (int r0 = 0; r0 < R; r0 += 64) {                  // (uniform trip counts: R and size are the block's)
    const int nr = min(64, R - r0);
    __syncthreads();
    if (tid < 64) aw[tid] = tid < nr ? allowed[r0 + tid] : 0u;
    __syncthreads();
    int cnt = 0;
    for (int i0 = wave * 64; i0 < size; i0 += 256) {
      const int i = i0 + lane;
      const uint32_t w = i < size ? lw[i] : 0u;
      for (int j = 0; j < nr; ++j) {
        const int c = (int)__popcll(__ballot((w & aw[j]) != 0u));
        if (lane == j) cnt += c;
      }
    }
    wsum[wave][lane] = cnt;
    __syncthreads();
    if (tid < nr) counts[((int64_t)(r0 + tid) * G + m) * nlist + l] = wsum[0][tid] + wsum[1][tid] + wsum[2][tid] + wsum[3][tid];
  }
}

// Merge: one wave per row; the k best of the row's probes x segments -> out[row][0..k) (int64 positions, best first).
template <int KS>
__global__ __launch_bounds__(256) void mol_ivf_merge_kernel(int rows, int nlist, int G, const int32_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ probes, const int32_t* __restrict__ nprob, int max_probes,
                                                            int seg_items, int n_seg, int k, const float* __restrict__ part_s,
                                                            const int32_t* __restrict__ part_p, int64_t* __restrict__ out, int32_t* __restrict__ unfilled) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int32_t* off = offsets + (int64_t)(row % G) * (nlist + 1);
  WaveTopK<KS> top;
  const int np = nprob[row];
  for (int r = 0; r < np; ++r) {
    const int slot = row * max_probes + r;
    const int l = probes[slot];
    const int size = off[l + 1] - off[l];
    const int ns = min(n_seg, (size + seg_items - 1) / seg_items);
    for (int s = 0; s < ns; ++s) {
      const int64_t o = ((int64_t)slot * n_seg + s) * k;
      const int have = min(k, min(seg_items, size - s * seg_items));
      for (int c = 0; c < have; c += 64) {
        const bool valid = c + lane < have;
        top.offer(valid, valid ? part_s[o + c + lane] : 0.0f, valid ? part_p[o + c + lane] : 0, k, lane);
      }
    }
  }
  // the short-list rule makes the probed lists hold >= k items; a sentinel can only remain after a max_probes below rails_ivf_plan's:
  // it raises *unfilled and is written as position 0, so that no consumer reads outside the corpus
  const bool empty0 = lane < k && top.p0 == 0x7fffffff, empty1 = KS == 2 && 64 + lane < k && top.p1 == 0x7fffffff;
  if (unfilled && __ballot(empty0 || empty1) != 0ull && lane == 0) *unfilled = 1;
  int64_t* o = out + (int64_t)row * k;
  if (lane < k) o[lane] = top.p0 == 0x7fffffff ? 0 : top.p0;
  if (KS == 2 && 64 + lane < k) o[64 + lane] = top.p1 == 0x7fffffff ? 0 : top.p1;
}

bool d_ok(int d) { return d == 32 || d == 64 || d == 128; }

int64_t sort_tiles(int64_t n) { return (n + kSortTile - 1) / kSortTile; }

template <typename F>
int by_d(int d, F&& f) {
  if (d == 32) return f(std::integral_constant<int, 32>{});
  if (d == 64) return f(std::integral_constant<int, 64>{});
  return f(std::integral_constant<int, 128>{});
}

struct SearchGeo {
  int slice_b, qrows, rows, n_seg, seg_items;
};

SearchGeo search_geo(int B, int PQ, int G, int nlist, int nprobe, int max_list) {
  SearchGeo g;
  g.slice_b = std::max(1, std::min(B, kSliceRows / PQ));
  g.qrows = g.slice_b * PQ;
  g.rows = g.qrows * G;
  const int64_t units = (int64_t)g.rows * nprobe;
  int ns = (int)std::max<int64_t>(1, (kScanUnits + units - 1) / units);
  ns = std::min(ns, std::max(1, (max_list + 63) / 64));
  ns = std::min(ns, std::max(1, kScanBlocks / (nlist * G)));
  g.seg_items = std::max(64, ((max_list + ns - 1) / ns + 63) / 64 * 64);
  g.n_seg = std::max(1, (max_list + g.seg_items - 1) / g.seg_items);
  return g;
}

// build workspace: sample16 | assign | hist | order | sample offsets | sizes (each 256-byte aligned)
struct BuildWs {
  unsigned short* x16;
  int32_t *assign, *hist, *order, *soff;
  float* sizes;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t build_ws_layout(int G, int64_t n, int nlist, int S, int d, char* base, BuildWs* w) {
  const int64_t nm = std::max<int64_t>(n, S);
  const size_t sz[6] = {align256((size_t)G * S * d * 2), align256((size_t)G * nm * 4), align256((size_t)G * nlist * sort_tiles(nm) * 4),
                        align256((size_t)G * nm * 4), align256((size_t)G * (nlist + 1) * 4), align256((size_t)G * nlist * 4)};
  size_t o = 0;
  char* p[6];
  for (int i = 0; i < 6; ++i) { p[i] = base ? base + o : nullptr; o += sz[i]; }
  if (w) {
    w->x16 = reinterpret_cast<unsigned short*>(p[0]);
    w->assign = reinterpret_cast<int32_t*>(p[1]);
    w->hist = reinterpret_cast<int32_t*>(p[2]);
    w->order = reinterpret_cast<int32_t*>(p[3]);
    w->soff = reinterpret_cast<int32_t*>(p[4]);
    w->sizes = reinterpret_cast<float*>(p[5]);
  }
  return o;
}

int launch_ok() { return hipGetLastError() == hipSuccess ? kOk : kErrLaunch; }

int assign_points(const Src& src, int G, int64_t n, int d, const float* cent, int nlist, int32_t* assign, hipStream_t st) {
  return by_d(d, [&](auto DC) {
    constexpr int D = decltype(DC)::value;
    hipLaunchKernelGGL(mol_ivf_assign_kernel<D>, dim3((unsigned)((n + 255) / 256), (unsigned)G), dim3(256), 0, st, src, n, cent, nlist, assign);
    return launch_ok();
  });
}

// stable counting sort of n points per group by assign[]: order[m][slot] = point; offsets (G, nlist + 1); vec16: also their vectors
int counting_sort(const Src& src, int G, int64_t n, int d, int nlist, const int32_t* assign, int32_t* hist, int32_t* offsets, int32_t* order,
                  unsigned short* vec16, hipStream_t st) {
  const int tiles = (int)sort_tiles(n);
  hipLaunchKernelGGL(mol_ivf_hist_kernel, dim3((unsigned)tiles, (unsigned)G), dim3(256), 0, st, assign, n, nlist, tiles, hist);
  hipLaunchKernelGGL(mol_ivf_prefix_kernel, dim3((unsigned)G), dim3(1024), 0, st, hist, nlist, tiles, n, offsets);
  by_d(d, [&](auto DC) {
    constexpr int D = decltype(DC)::value;
    hipLaunchKernelGGL(mol_ivf_scatter_kernel<D>, dim3((unsigned)tiles, (unsigned)G), dim3(64), 0, st, src, assign, n, nlist, tiles, hist, order, vec16);
    return kOk;
  });
  return launch_ok();
}

}  // namespace

int ivf_check(const Shape& s, int64_t n, int nlist, bool from_index) {
  if (!d_ok(s.dot_product_dimension)) {
    set_error("ivf: d = %d outside the supported dot_product_dimension in {32, 64, 128}", s.dot_product_dimension);
    return kErrUnsupported;
  }
  if (nlist < 1 || nlist > kMaxNlist) { set_error("ivf: nlist = %d outside [1, %d]", nlist, kMaxNlist); return kErrUnsupported; }
  if (n < nlist) { set_error("ivf: %lld items cannot fill nlist = %d lists (need n_items >= nlist)", (long long)n, nlist); return kErrInvalid; }
  if (n > 0x7fffffffLL) { set_error("ivf: %lld items exceed the int32 positions of the lists", (long long)n); return kErrUnsupported; }
  if (from_index && is_split(s)) { set_error("ivf: needs an fp32-format item index (build one with precision = RAILS_PRECISION_FP32)"); return kErrUnsupported; }
  return kOk;
}

size_t ivf_build_workspace_bytes(const Shape& s, int64_t n, int nlist, int S) {
  return build_ws_layout(s.item_dot_product_groups, n, nlist, S, s.dot_product_dimension, nullptr, nullptr);
}

int ivf_components16(const Shape& s, const float* ipack, int64_t n, void* table, int64_t n_total, int64_t first, hipStream_t st) {
  const int64_t t = n * s.item_dot_product_groups * (s.dot_product_dimension / 4);
  if (t == 0) return kOk;
  hipLaunchKernelGGL(mol_ivf_components16_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, st, ipack, n, s.query_dot_product_groups,
                     s.item_dot_product_groups, s.dot_product_dimension, n_total, first, static_cast<unsigned short*>(table));
  return launch_ok();
}

int ivf_train(const Shape& s, const float* ipack, const void* comp16, int64_t n, const int32_t* sample_pos, int S, int nlist, int iters, int init, float* cent,
              void* ws, size_t ws_bytes, hipStream_t st) {
  const int G = s.item_dot_product_groups, d = s.dot_product_dimension;
  BuildWs w;
  if (build_ws_layout(G, n, nlist, S, d, static_cast<char*>(ws), &w) > ws_bytes) { set_error("ivf_train: workspace too small"); return kErrNoMem; }
  const int64_t g = (int64_t)G * S * (d / 4);
  hipLaunchKernelGGL(mol_ivf_gather_kernel, dim3((unsigned)((g + 255) / 256)), dim3(256), 0, st, ipack, static_cast<const unsigned short*>(comp16), n,
                     s.query_dot_product_groups, G, d, sample_pos, S, w.x16);
  if (init) {
    const int64_t c = (int64_t)G * nlist * d;
    hipLaunchKernelGGL(mol_ivf_init_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, st, w.x16, S, d, nlist, G, cent);
  }
  if (launch_ok() != kOk) return kErrLaunch;
  const Src src{w.x16, nullptr, s.query_dot_product_groups, G};
  for (int it = 0; it < iters; ++it) {
    if (assign_points(src, G, S, d, cent, nlist, w.assign, st) != kOk) return kErrLaunch;
    if (counting_sort(src, G, S, d, nlist, w.assign, w.hist, w.soff, w.order, nullptr, st) != kOk) return kErrLaunch;
    hipLaunchKernelGGL(mol_ivf_mean_kernel, dim3((unsigned)nlist, (unsigned)G), dim3(128), 0, st, w.x16, S, d, w.order, w.soff, nlist, cent, w.sizes);
    hipLaunchKernelGGL(mol_ivf_finish_kernel, dim3((unsigned)G), dim3(256), 0, st, cent, w.sizes, nlist, d);
    if (launch_ok() != kOk) return kErrLaunch;
  }
  return kOk;
}

int ivf_assign(const Shape& s, const float* ipack, const void* comp16, int64_t n, int nlist, const float* cent, int32_t* assign, hipStream_t st) {
  const Src src{static_cast<const unsigned short*>(comp16), ipack, s.query_dot_product_groups, s.item_dot_product_groups};
  return assign_points(src, s.item_dot_product_groups, n, s.dot_product_dimension, cent, nlist, assign, st);
}

int ivf_build_lists(const Shape& s, const float* ipack, const void* comp16, int64_t n, int nlist, const float* cent, void* vectors, int32_t* positions, int32_t* offsets,
                    void* ws, size_t ws_bytes, hipStream_t st) {
  const int G = s.item_dot_product_groups, d = s.dot_product_dimension;
  BuildWs w;
  if (build_ws_layout(G, n, nlist, 0, d, static_cast<char*>(ws), &w) > ws_bytes) { set_error("ivf_build_lists: workspace too small"); return kErrNoMem; }
  const Src src{static_cast<const unsigned short*>(comp16), ipack, s.query_dot_product_groups, G};
  if (assign_points(src, G, n, d, cent, nlist, w.assign, st) != kOk) return kErrLaunch;
  return counting_sort(src, G, n, d, nlist, w.assign, w.hist, offsets, positions, static_cast<unsigned short*>(vectors), st);
}

// edit workspace: drop mask | keys as assigned | keys sorted | K | tile counts | the tile prefix's offsets (each 256-byte aligned)
struct EditWs {
  unsigned char* drop;
  int64_t *keys_in, *keys;
  int32_t *K, *counts, *ends;
};

static size_t edit_ws_layout(int G, int64_t n_old, int m, char* base, EditWs* w) {
  const size_t sz[6] = {align256((size_t)n_old), align256((size_t)G * m * 8), align256((size_t)G * m * 8), align256((size_t)G * (n_old + 1) * 4),
                        align256((size_t)G * sort_tiles(n_old) * 4), align256((size_t)G * 2 * 4)};
  size_t o = 0;
  char* p[6];
  for (int i = 0; i < 6; ++i) { p[i] = base ? base + o : nullptr; o += sz[i]; }
  if (w) {
    w->drop = reinterpret_cast<unsigned char*>(p[0]);
    w->keys_in = reinterpret_cast<int64_t*>(p[1]);
    w->keys = reinterpret_cast<int64_t*>(p[2]);
    w->K = reinterpret_cast<int32_t*>(p[3]);
    w->counts = reinterpret_cast<int32_t*>(p[4]);
    w->ends = reinterpret_cast<int32_t*>(p[5]);
  }
  return o;
}

int ivf_lists_edit_check(const Shape& s, int64_t n_old, int nlist, int64_t m) {
  if (!d_ok(s.dot_product_dimension)) {
    set_error("ivf_lists_edit: d = %d outside the supported dot_product_dimension in {32, 64, 128}", s.dot_product_dimension);
    return kErrUnsupported;
  }
  if (nlist < 1 || nlist > kMaxNlist) { set_error("ivf_lists_edit: nlist = %d outside [1, %d]", nlist, kMaxNlist); return kErrUnsupported; }
  if (m < 0 || m > kEditMax) { set_error("ivf_lists_edit: %lld inserted entries outside [0, %d] (rebuild the lists instead)", (long long)m, kEditMax); return kErrUnsupported; }
  if (n_old < 1 || n_old > 0x7fffffffLL) { set_error("ivf_lists_edit: %lld old entries outside [1, 2^31)", (long long)n_old); return kErrInvalid; }
  return kOk;
}

size_t ivf_lists_edit_workspace_bytes(const Shape& s, int64_t n_old, int m) {
  return edit_ws_layout(s.item_dot_product_groups, n_old, m, nullptr, nullptr);
}

int ivf_lists_edit(const Shape& s, const float* src, int src_in_place, const int64_t* positions, int m, int64_t n_keep, int nlist, const float* cent,
                   const void* old_vectors, const int32_t* old_positions, const int32_t* old_offsets, int64_t n_old, void* new_vectors,
                   int32_t* new_positions, int32_t* new_offsets, int64_t n_new, void* ws, size_t ws_bytes, hipStream_t st) {
  const int G = s.item_dot_product_groups, d = s.dot_product_dimension, PQ = s.query_dot_product_groups;
  EditWs w;
  if (edit_ws_layout(G, n_old, m, static_cast<char*>(ws), &w) > ws_bytes) { set_error("ivf_lists_edit: workspace too small"); return kErrNoMem; }
  const int64_t n_lim = std::min(n_old, std::max<int64_t>(n_keep, 0));
  const int tiles = (int)sort_tiles(n_old);
  const unsigned short* ov = static_cast<const unsigned short*>(old_vectors);
  unsigned short* nv = static_cast<unsigned short*>(new_vectors);
  if (hipMemsetAsync(w.drop, 0, (size_t)n_old, st) != hipSuccess) return kErrLaunch;
  if (m > 0) {
    hipLaunchKernelGGL(mol_ivf_edit_mask_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, positions, m, n_old, w.drop);
    const Src source{nullptr, src, PQ, G};
    by_d(d, [&](auto DC) {
      constexpr int D = decltype(DC)::value;
      hipLaunchKernelGGL(mol_ivf_assign_indexed_kernel<D>, dim3((unsigned)((m + 255) / 256), (unsigned)G), dim3(256), 0, st, source, src_in_place, positions,
                         (int64_t)m, cent, nlist, w.keys_in);
      return kOk;
    });
    if (launch_ok() != kOk) return kErrLaunch;
    const int r = sort_rows_i64(w.keys_in, G, m, w.keys, st);
    if (r != kOk) return r;
  }
  hipLaunchKernelGGL(mol_ivf_edit_count_kernel, dim3((unsigned)tiles, (unsigned)G), dim3(256), 0, st, old_positions, n_old, n_lim, w.drop, tiles, w.counts);
  hipLaunchKernelGGL(mol_ivf_prefix_kernel, dim3((unsigned)G), dim3(1024), 0, st, w.counts, 1, tiles, n_old, w.ends);      // one "list" per group: counts -> tile bases
  hipLaunchKernelGGL(mol_ivf_edit_scan_kernel, dim3((unsigned)tiles, (unsigned)G), dim3(256), 0, st, old_positions, n_old, n_lim, w.drop, tiles, w.counts, w.K);
  by_d(d, [&](auto DC) {
    constexpr int D = decltype(DC)::value;
    hipLaunchKernelGGL(mol_ivf_edit_move_kernel<D>, dim3((unsigned)((n_old + 255) / 256), (unsigned)G), dim3(256), 0, st, ov, old_positions, old_offsets, n_old,
                       n_lim, nlist, w.drop, w.K, w.keys, m, nv, new_positions, n_new);
    if (m > 0)
      hipLaunchKernelGGL(mol_ivf_edit_insert_kernel<D>, dim3((unsigned)((m + 255) / 256), (unsigned)G), dim3(256), 0, st, src, src_in_place, PQ, G, w.keys, m,
                         old_positions, old_offsets, n_old, nlist, w.K, nv, new_positions, n_new);
    return kOk;
  });
  const int no = G * (nlist + 1);
  hipLaunchKernelGGL(mol_ivf_edit_offsets_kernel, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, st, old_offsets, nlist, G, n_old, w.K, w.keys, m, n_new,
                     new_offsets);
  return launch_ok();
}

int ivf_search_check(const Shape& s, int nlist, int nprobe, int max_probes, int max_list, int k, int64_t n) {
  if (!d_ok(s.dot_product_dimension)) {
    set_error("ivf_search: d = %d outside the supported dot_product_dimension in {32, 64, 128}", s.dot_product_dimension);
    return kErrUnsupported;
  }
  if (nlist < 1 || nlist > kMaxNlist) { set_error("ivf_search: nlist = %d outside [1, %d]", nlist, kMaxNlist); return kErrUnsupported; }
  if (nprobe < 1 || nprobe > std::min(kMaxProbe, nlist)) {
    set_error("ivf_search: nprobe = %d outside [1, min(%d, nlist = %d)]", nprobe, kMaxProbe, nlist);
    return kErrUnsupported;
  }
  if (k < 1 || k > kMaxK) { set_error("ivf_search: k_per_group = %d outside [1, %d]", k, kMaxK); return kErrUnsupported; }
  if (k > n) { set_error("ivf_search: selected index k out of range (k = %d > n = %lld)", k, (long long)n); return kErrInvalid; }
  if (max_probes < nprobe || max_probes > nlist) { set_error("ivf_search: max_probes = %d outside [nprobe, nlist]", max_probes); return kErrInvalid; }
  if (max_list < 1 || max_list > n) { set_error("ivf_search: max_list = %d outside [1, n_items]", max_list); return kErrInvalid; }
  return kOk;
}

size_t ivf_search_workspace_bytes(const Shape& s, int B, int nlist, int nprobe, int max_probes, int max_list, int k) {
  const SearchGeo g = search_geo(B, s.query_dot_product_groups, s.item_dot_product_groups, nlist, nprobe, max_list);
  const size_t probes = align256((size_t)g.rows * max_probes * 4), nprob = align256((size_t)g.rows * 4);
  const size_t part = align256((size_t)g.rows * max_probes * g.n_seg * k * 4);
  return probes + nprob + 2 * part;
}

int ivf_search(const Shape& s, const float* eq, int B, const float* cent, const void* vectors, const int32_t* positions, const int32_t* offsets,
               int64_t n, int nlist, int nprobe, int max_probes, int max_list, int k, void* ws, size_t ws_bytes, int64_t* out, int32_t* unfilled,
               hipStream_t st) {
  return ivf_search_filtered(s, eq, B, cent, vectors, positions, offsets, n, nlist, nprobe, max_probes, max_list, k, ws, ws_bytes, out, unfilled, nullptr,
                             nullptr, nullptr, 1, st);
}

// list_words == NULL: the plain search (the three launches of ivf_search, the kernels it always ran).  Else allowed holds one word per batch row
// and counts (count_rows, G, nlist) the eligible entries per list: one row shared by the batch, or one per batch row.
int ivf_search_filtered(const Shape& s, const float* eq, int B, const float* cent, const void* vectors, const int32_t* positions, const int32_t* offsets,
                        int64_t n, int nlist, int nprobe, int max_probes, int max_list, int k, void* ws, size_t ws_bytes, int64_t* out, int32_t* unfilled,
                        const uint32_t* list_words, const uint32_t* allowed, const int32_t* counts, int count_rows, hipStream_t st) {
  const int PQ = s.query_dot_product_groups, G = s.item_dot_product_groups, d = s.dot_product_dimension;
  if (ivf_search_workspace_bytes(s, B, nlist, nprobe, max_probes, max_list, k) > ws_bytes) { set_error("ivf_search: workspace too small"); return kErrNoMem; }
  const SearchGeo g = search_geo(B, PQ, G, nlist, nprobe, max_list);
  char* p = static_cast<char*>(ws);
  int32_t* probes = reinterpret_cast<int32_t*>(p);
  p += align256((size_t)g.rows * max_probes * 4);
  int32_t* nprob = reinterpret_cast<int32_t*>(p);
  p += align256((size_t)g.rows * 4);
  const size_t part = align256((size_t)g.rows * max_probes * g.n_seg * k * 4);
  float* part_s = reinterpret_cast<float*>(p);
  int32_t* part_p = reinterpret_cast<int32_t*>(p + part);
  const unsigned short* v16 = static_cast<const unsigned short*>(vectors);
  for (int b0 = 0; b0 < B; b0 += g.slice_b) {
    const int qrows = std::min(g.slice_b, B - b0) * PQ, rows = qrows * G;
    const float* eqs = eq + (int64_t)b0 * PQ * d;
    int64_t* outs = out + (int64_t)b0 * PQ * G * k;
    by_d(d, [&](auto DC) {
      constexpr int D = decltype(DC)::value;
      const dim3 grid((unsigned)g.n_seg, (unsigned)nlist, (unsigned)G);
      if (list_words) {
        const int32_t* cs = counts + (count_rows == 1 ? 0 : (int64_t)b0 * G * nlist);
        hipLaunchKernelGGL(mol_ivf_coarse_filtered_kernel<D>, dim3((unsigned)rows), dim3(256), 0, st, eqs, G, cent, nlist, cs, count_rows, PQ, nprobe, k,
                           max_probes, probes, nprob, b0 == 0 ? unfilled : nullptr);
        if (k > 64)
          hipLaunchKernelGGL((mol_ivf_scan_filtered_kernel<D, 2>), grid, dim3(256), 0, st, eqs, qrows, G, nlist, v16, positions, offsets, n, probes,
                             max_probes, g.seg_items, g.n_seg, k, part_s, part_p, list_words, allowed + b0, PQ);
        else
          hipLaunchKernelGGL((mol_ivf_scan_filtered_kernel<D, 1>), grid, dim3(256), 0, st, eqs, qrows, G, nlist, v16, positions, offsets, n, probes,
                             max_probes, g.seg_items, g.n_seg, k, part_s, part_p, list_words, allowed + b0, PQ);
        return kOk;
      }
      hipLaunchKernelGGL(mol_ivf_coarse_kernel<D>, dim3((unsigned)rows), dim3(256), 0, st, eqs, G, cent, nlist, offsets, nprobe, k, max_probes, probes, nprob,
                         b0 == 0 ? unfilled : nullptr);
      if (k > 64)
        hipLaunchKernelGGL((mol_ivf_scan_kernel<D, 2>), grid, dim3(256), 0, st, eqs, qrows, G, nlist, v16, positions, offsets, n, probes, max_probes,
                           g.seg_items, g.n_seg, k, part_s, part_p);
      else
        hipLaunchKernelGGL((mol_ivf_scan_kernel<D, 1>), grid, dim3(256), 0, st, eqs, qrows, G, nlist, v16, positions, offsets, n, probes, max_probes,
                           g.seg_items, g.n_seg, k, part_s, part_p);
      return kOk;
    });
    const dim3 mgrid((unsigned)((rows + 3) / 4));
    if (k > 64)
      hipLaunchKernelGGL(mol_ivf_merge_kernel<2>, mgrid, dim3(256), 0, st, rows, nlist, G, offsets, probes, nprob, max_probes, g.seg_items, g.n_seg, k,
                         part_s, part_p, outs, unfilled);
    else
      hipLaunchKernelGGL(mol_ivf_merge_kernel<1>, mgrid, dim3(256), 0, st, rows, nlist, G, offsets, probes, nprob, max_probes, g.seg_items, g.n_seg, k,
                         part_s, part_p, outs, unfilled);
    if (launch_ok() != kOk) return kErrLaunch;
  }
  return kOk;
}

// host: the probe capacity the short-list rule needs (the fewest lists whose sizes reach k, or nprobe) and the largest list
void ivf_plan(const int32_t* offsets, int G, int nlist, int nprobe, int k, int* max_probes, int* max_list) {
  int mp = nprobe, ml = 1;
  std::vector<int> sz(nlist);
  for (int m = 0; m < G; ++m) {
    const int32_t* off = offsets + (int64_t)m * (nlist + 1);
    for (int l = 0; l < nlist; ++l) { sz[l] = off[l + 1] - off[l]; ml = std::max(ml, sz[l]); }
    std::sort(sz.begin(), sz.end());
    int64_t held = 0;
    int need = nlist;
    for (int l = 0; l < nlist; ++l) {
      held += sz[l];
      if (held >= k) { need = l + 1; break; }
    }
    mp = std::max(mp, need);
  }
  *max_probes = std::min(mp, nlist);
  *max_list = ml;
}

int ivf_list_words(const int32_t* positions, int G, int64_t n, const uint32_t* eff, const uint32_t* visible, uint32_t* list_words, hipStream_t st) {
  const int64_t total = (int64_t)G * n;
  hipLaunchKernelGGL(mol_ivf_list_words_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, positions, total, n, eff, visible, list_words);
  return launch_ok();
}

int ivf_list_counts(const uint32_t* list_words, const int32_t* offsets, int G, int64_t n, int nlist, const uint32_t* allowed, int R, int32_t* counts,
                    hipStream_t st) {
  hipLaunchKernelGGL(mol_ivf_list_counts_kernel, dim3((unsigned)nlist, (unsigned)G), dim3(256), 0, st, list_words, offsets, n, nlist, G, allowed, R, counts);
  return launch_ok();
}

// host: ivf_plan's probe capacity over the eligible counts of every (row, group): the fewest lists whose counts reach k (every list where they
// never do), at least nprobe
int ivf_plan_filtered(const int32_t* counts, int R, int G, int nlist, int nprobe, int k) {
  int mp = nprobe;
  std::vector<int> sz(nlist);
  for (int64_t rm = 0; rm < (int64_t)R * G && mp < nlist; ++rm) {
    const int32_t* c = counts + rm * nlist;
    std::copy(c, c + nlist, sz.begin());
    std::sort(sz.begin(), sz.end());
    int64_t held = 0;
    int need = nlist;
    for (int l = 0; l < nlist; ++l) {
      held += sz[l];
      if (held >= k) { need = l + 1; break; }
    }
    mp = std::max(mp, need);
  }
  return std::min(mp, nlist);
}

}  // namespace mol
