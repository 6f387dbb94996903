// Item masks (rails_item_mask_*, rails_scores_mask): a top-k call restricted to a subset of the corpus.
//
// A mask is `rows` bit rows of ceil(n / 32) 32-bit words each: bit i % 32 of word i / 32 is item i (little-endian), the unused high bits
// of a row's last word are ZERO -- every kernel here keeps that invariant and none relies on it for its bounds.
//   pack        bool bytes -> words: one wave ballot per 64 items, lanes 0 and 32 store the two words
//   set         positions -> bits of one zeroed row, a 32-bit atomic OR per position
//   clear       positions -> bits of one row cleared, a 32-bit atomic AND-NOT per position (hide_items)
//   count       per-row popcount, one workgroup per row
//   positions   STABLE compaction of a row's set bits into its ascending position list, in tiles of kTileBits items:
//                 1. per-tile popcounts  2. exclusive scan of a row's tile counts (64-bit, one workgroup per row, looping)
//                 3. every tile writes its positions behind its offset  4. the slots past the row's count are set to 0
//   scores_mask scores[b][x] = fill where bit first_item + x of row b's mask is clear; kept entries are neither read nor written
//   item tags    effective tags, kept counts per allow word, a filter's mask rows, scores[r][x] = fill where item x carries
//               no bit of row r's allow word
// All plain C++ with vector stores, no LDS beyond the 4-word reductions (wave_ops.h), every loop grid-strided with 64-bit indices (rows of 125 M bits).
#include <hip/hip_runtime.h>

#include "mol_kernels.h"
#include "score_rows.h"
#include "wave_ops.h"

namespace mol {

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileWords = kThreads;               // one word per thread
constexpr int64_t kTileBits = 32 * kTileWords;     // 8 192 items per compaction tile

// the word `w` of a row of n bits with the bits at or past n cleared
__device__ __forceinline__ u32 live_bits(u32 word, int64_t w, int64_t n) {
  const int64_t left = n - w * 32;
  return left >= 32 ? word : left <= 0 ? 0u : word & ((1u << (int)left) - 1u);
}

}  // namespace

__global__ void __launch_bounds__(kThreads) item_mask_pack_kernel(const unsigned char* __restrict__ mask, int64_t ld, int rows, int64_t n, int64_t n_words,
                                                                 u32* __restrict__ words) {
  const int64_t chunks = (n + kThreads - 1) / kThreads, total = chunks * rows;
  for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
    const int64_t row = c / chunks, ch = c - row * chunks;
    const int64_t i = ch * kThreads + threadIdx.x;
    const bool set = i < n && mask[row * ld + i] != 0;
    const u64 b = __ballot(set);
    const int lane = threadIdx.x & 63;
    const int64_t w = (ch * kThreads + (threadIdx.x & ~63)) >> 5;      // the first of this wave's two words
    if (lane == 0 && w < n_words) words[row * n_words + w] = (u32)b;
    if (lane == 32 && w + 1 < n_words) words[row * n_words + w + 1] = (u32)(b >> 32);
  }
}

__global__ void item_mask_set_kernel(const int64_t* __restrict__ positions, int64_t m, int64_t n, u32* __restrict__ words) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < m; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = positions[u];
    if (p >= 0 && p < n) atomicOr(words + (p >> 5), 1u << (int)(p & 31));
  }
}

// (named apart from the item_mask_* kernels: tests/test_item_mask_cpu.py pins that family's list)
__global__ void mask_bits_clear_kernel(const int64_t* __restrict__ positions, int64_t m, int64_t n, u32* __restrict__ words) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < m; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = positions[u];
    if (p >= 0 && p < n) atomicAnd(words + (p >> 5), ~(1u << (int)(p & 31)));
  }
}

__global__ void __launch_bounds__(kThreads) item_mask_count_kernel(const u32* __restrict__ words, int64_t n, int64_t n_words, int32_t* __restrict__ counts) {
  __shared__ int part[kWaves];
  const int64_t row = blockIdx.x;
  int c = 0;
  for (int64_t w = threadIdx.x; w < n_words; w += kThreads) c += __popc(live_bits(words[row * n_words + w], w, n));
  c = block_sum<kThreads>(c, part);
  if (threadIdx.x == 0) counts[row] = c;
}

// ws[row * tiles + t] = set bits of tile t of the row
__global__ void __launch_bounds__(kThreads) item_mask_tile_counts_kernel(const u32* __restrict__ words, int rows, int64_t n, int64_t n_words, int64_t tiles,
                                                                        int64_t* __restrict__ ws) {
  __shared__ int part[kWaves];
  const int64_t total = tiles * rows;
  for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
    const int64_t row = c / tiles, t = c - row * tiles;
    const int64_t w = t * kTileWords + threadIdx.x;
    const int bits = w < n_words ? __popc(live_bits(words[row * n_words + w], w, n)) : 0;
    const int s = block_sum<kThreads>(bits, part);
    if (threadIdx.x == 0) ws[c] = s;
  }
}

// in place: a row's tile counts -> their exclusive prefix sums; ws[rows * tiles + row] = the row's total
__global__ void __launch_bounds__(kThreads) item_mask_tile_scan_kernel(int rows, int64_t tiles, int64_t* __restrict__ ws) {
  __shared__ int part[kWaves];
  const int64_t row = blockIdx.x;
  int64_t* counts = ws + row * tiles;
  int64_t running = 0;
  for (int64_t base = 0; base < tiles; base += kThreads) {
    const int64_t t = base + threadIdx.x;
    const int v = t < tiles ? (int)counts[t] : 0;      // at most kTileBits
    int all;
    const int excl = block_scan_excl<kThreads>(v, part, all);
    if (t < tiles) counts[t] = running + excl;
    running += all;
  }
  if (threadIdx.x == 0) ws[(int64_t)rows * tiles + row] = running;
}

__global__ void __launch_bounds__(kThreads) item_mask_tile_write_kernel(const u32* __restrict__ words, int rows, int64_t n, int64_t n_words, int64_t tiles,
                                                                       const int64_t* __restrict__ ws, int64_t* __restrict__ out, int64_t out_ld) {
  __shared__ int part[kWaves];
  const int64_t total = tiles * rows;
  for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
    const int64_t row = c / tiles, t = c - row * tiles;
    const int64_t w = t * kTileWords + threadIdx.x;
    u32 word = w < n_words ? live_bits(words[row * n_words + w], w, n) : 0u;
    int all;
    int64_t slot = ws[c] + block_scan_excl<kThreads>(__popc(word), part, all);
    int64_t* dst = out + row * out_ld;
    while (word) {
      const int bit = __ffs((int)word) - 1;
      if (slot < out_ld) dst[slot] = w * 32 + bit;
      ++slot;
      word &= word - 1;
    }
  }
}

__global__ void item_mask_pad_kernel(int rows, int64_t tiles, const int64_t* __restrict__ ws, int64_t* __restrict__ out, int64_t out_ld) {
  const int64_t total = out_ld * rows;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / out_ld, slot = i - row * out_ld;
    if (slot >= ws[(int64_t)rows * tiles + row]) out[i] = 0;
  }
}

constexpr int kMaskPerThread = 4;

__global__ void __launch_bounds__(kThreads) scores_mask_kernel(float* __restrict__ scores, int64_t ld, int rows, int64_t n, int64_t first_item,
                                                              const u32* __restrict__ words, int64_t words_row_stride, float fill,
                                                              const int32_t* __restrict__ run_if) {
  MOL_RUN_IF(run_if);
  constexpr int64_t kChunk = (int64_t)kThreads * kMaskPerThread;
  const int64_t chunks = (n + kChunk - 1) / kChunk, total = chunks * rows;
  for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
    const int64_t row = c / chunks, ch = c - row * chunks;
    const u32* mrow = words + row * words_row_stride;
    float* srow = scores + row * ld;
#pragma unroll
    for (int j = 0; j < kMaskPerThread; ++j) {
      const int64_t x = ch * kChunk + (int64_t)j * kThreads + threadIdx.x;
      if (x < n) {
        const int64_t bit = first_item + x;
        if (((mrow[bit >> 5] >> (int)(bit & 31)) & 1u) == 0u) srow[x] = fill;
      }
    }
  }
}

// ---- item tags: one 32-bit word of attributes per item; row b of a call may return item x iff eff[x] & allowed[b] != 0.
// (Named apart from the item_mask_* / scores_mask kernels: tests/test_item_mask_cpu.py pins that family's list.)  Plain C++, vector stores,
// grid-strided loops with 64-bit indices; every index is tested against n before it is used.

// eff[i] = tags[i] where bit i of the visibility row is set, else 0: a hidden item carries no attribute
__global__ void __launch_bounds__(kThreads) item_tags_effective_kernel(const u32* __restrict__ tags, const u32* __restrict__ visible, int64_t n,
                                                                      u32* __restrict__ eff) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    eff[i] = ((visible[i >> 5] >> (int)(i & 31)) & 1u) ? tags[i] : 0u;
}

// counts[j] = #{i < n : eff[i] & words[j] != 0}: one workgroup per word (a count is read back once per new word and cached by the caller)
__global__ void __launch_bounds__(kThreads) item_tags_count_kernel(const u32* __restrict__ eff, int64_t n, const u32* __restrict__ words,
                                                                  int32_t* __restrict__ counts) {
  __shared__ int part[kWaves];
  const u32 word = words[blockIdx.x];
  int c = 0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) c += (eff[i] & word) != 0u;
  c = block_sum<kThreads>(c, part);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// the ItemMask rows of a tag filter: bit i of row r = (eff[i] & allowed[r]) != 0, packed with a ballot as item_mask_pack_kernel packs bool bytes
__global__ void __launch_bounds__(kThreads) item_tags_to_mask_kernel(const u32* __restrict__ eff, int64_t n, int64_t n_words, const u32* __restrict__ allowed,
                                                                    int rows, u32* __restrict__ words) {
  const int64_t chunks = (n + kThreads - 1) / kThreads, total = chunks * rows;
  for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
    const int64_t row = c / chunks, ch = c - row * chunks;
    const int64_t i = ch * kThreads + threadIdx.x;
    const bool set = i < n && (eff[i] & allowed[row]) != 0u;
    const u64 b = __ballot(set);
    const int lane = threadIdx.x & 63;
    const int64_t w = (ch * kThreads + (threadIdx.x & ~63)) >> 5;      // the first of this wave's two words
    if (lane == 0 && w < n_words) words[row * n_words + w] = (u32)b;
    if (lane == 32 && w + 1 < n_words) words[row * n_words + w + 1] = (u32)(b >> 32);
  }
}

// scores_mask_kernel's shape with a tag test in place of the mask bit: row r of the matrix belongs to allow word r / rows_per_allowed
__global__ void __launch_bounds__(kThreads) scores_tags_fill_kernel(float* __restrict__ scores, int64_t ld, int rows, int64_t n, int64_t first_item,
                                                                   const u32* __restrict__ eff, const u32* __restrict__ allowed, int rows_per_allowed,
                                                                   float fill, const int32_t* __restrict__ run_if) {
  MOL_RUN_IF(run_if);
  constexpr int64_t kChunk = (int64_t)kThreads * kMaskPerThread;
  const int64_t chunks = (n + kChunk - 1) / kChunk, total = chunks * rows;
  for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
    const int64_t row = c / chunks, ch = c - row * chunks;
    const u32 allow = allowed[row / rows_per_allowed];
    float* srow = scores + row * ld;
#pragma unroll
    for (int j = 0; j < kMaskPerThread; ++j) {
      const int64_t x = ch * kChunk + (int64_t)j * kThreads + threadIdx.x;
      if (x < n && (eff[first_item + x] & allow) == 0u) srow[x] = fill;
    }
  }
}

int item_tags_effective(const void* tags, const void* visible, int64_t n, void* eff, hipStream_t stream) {
  hipLaunchKernelGGL(item_tags_effective_kernel, dim3(grid_for((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, (const u32*)tags, (const u32*)visible,
                     n, (u32*)eff);
  return launched();
}

int item_tags_count(const void* eff, int64_t n, const void* words, int n_words, int32_t* counts, hipStream_t stream) {
  hipLaunchKernelGGL(item_tags_count_kernel, dim3((unsigned)n_words), dim3(kThreads), 0, stream, (const u32*)eff, n, (const u32*)words, counts);
  return launched();
}

int scores_mask_tags(float* scores, int64_t ld, int rows, int64_t n, int64_t first_item, const void* eff, const void* allowed, int rows_per_allowed,
                     float fill, const int32_t* run_if, hipStream_t stream) {
  const int64_t chunks = (n + (int64_t)kThreads * kMaskPerThread - 1) / ((int64_t)kThreads * kMaskPerThread);
  hipLaunchKernelGGL(scores_tags_fill_kernel, dim3(grid_for(chunks * rows)), dim3(kThreads), 0, stream, scores, ld, rows, n, first_item, (const u32*)eff,
                     (const u32*)allowed, rows_per_allowed, fill, run_if);
  return launched();
}

// ---- the eligibility pass of the pair-level calls: scores[r][j] belongs to item pos[r][j]; -inf where the position is
// outside [0, n) or row r may not return the item -- its mask bit clear, no bit of the row's allow word among its effective tags, or its id among
// the row's seen ids (a loop over the row's `width` ids: O(width) per pair, nothing of size n is built).  Where a score is set, the pair's
// extra_len entries of extra_a / extra_b (explain_of's weights and component logits) are zeroed.  One thread per pair, every index tested first.
// (Named apart from the item_mask_* / scores_mask kernels: tests/test_item_mask_cpu.py pins that family's list.)
__global__ void __launch_bounds__(kThreads) pairs_eligible_kernel(float* __restrict__ scores, int64_t ld, int rows, int64_t t, const int64_t* __restrict__ pos,
                                                                 int64_t n, const u32* __restrict__ words, int64_t words_row_stride,
                                                                 const u32* __restrict__ eff, const u32* __restrict__ allowed,
                                                                 const int64_t* __restrict__ invalid, int width, const int64_t* __restrict__ item_ids,
                                                                 float* __restrict__ extra_a, float* __restrict__ extra_b, int extra_len) {
  const int64_t total = (int64_t)rows * t;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / t, j = i - r * t;
    const int64_t p = pos[i];
    bool ok = p >= 0 && p < n;
    if (ok && words) ok = ((words[r * words_row_stride + (p >> 5)] >> (int)(p & 31)) & 1u) != 0u;
    if (ok && eff) ok = (eff[p] & allowed[r]) != 0u;
    if (ok && invalid) {
      const int64_t id = item_ids[p];
      const int64_t* seen = invalid + r * (int64_t)width;
      for (int s = 0; s < width; ++s) ok = ok && seen[s] != id;
    }
    if (ok) continue;
    scores[r * ld + j] = -INFINITY;
    if (extra_a) {
      for (int l = 0; l < extra_len; ++l) {
        extra_a[i * extra_len + l] = 0.0f;
        extra_b[i * extra_len + l] = 0.0f;
      }
    }
  }
}

int scores_at_eligible(float* scores, int64_t ld, int rows, int64_t t, const int64_t* positions, int64_t n, const void* words, int64_t words_row_stride,
                       const void* eff, const void* allowed, const int64_t* invalid_ids, int width, const int64_t* item_ids, float* extra_a, float* extra_b,
                       int extra_len, hipStream_t stream) {
  hipLaunchKernelGGL(pairs_eligible_kernel, dim3(grid_for(((int64_t)rows * t + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, scores, ld, rows, t,
                     positions, n, (const u32*)words, words_row_stride, (const u32*)eff, (const u32*)allowed, invalid_ids, width, item_ids, extra_a, extra_b,
                     extra_len);
  return launched();
}

int64_t item_mask_words(int64_t n) { return (n + 31) / 32; }

int item_mask_count(const void* words, int rows, int64_t n, int32_t* counts, hipStream_t stream) {
  hipLaunchKernelGGL(item_mask_count_kernel, dim3((unsigned)rows), dim3(kThreads), 0, stream, (const u32*)words, n, item_mask_words(n), counts);
  return launched();
}

int item_mask_from_tags(const void* eff, int64_t n, const void* allowed, int rows, void* words, int32_t* counts, hipStream_t stream) {
  const int64_t chunks = (n + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(item_tags_to_mask_kernel, dim3(grid_for(chunks * rows)), dim3(kThreads), 0, stream, (const u32*)eff, n, item_mask_words(n),
                     (const u32*)allowed, rows, (u32*)words);
  if (launched() != kOk) return kErrLaunch;
  return item_mask_count(words, rows, n, counts, stream);
}

int item_mask_pack(const unsigned char* mask, int64_t ld, int rows, int64_t n, void* words, int32_t* counts, hipStream_t stream) {
  const int64_t chunks = (n + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(item_mask_pack_kernel, dim3(grid_for(chunks * rows)), dim3(kThreads), 0, stream, mask, ld, rows, n, item_mask_words(n), (u32*)words);
  if (launched() != kOk) return kErrLaunch;
  return item_mask_count(words, rows, n, counts, stream);
}

int item_mask_set(const int64_t* positions, int64_t m, int64_t n, void* words, hipStream_t stream) {
  hipLaunchKernelGGL(item_mask_set_kernel, dim3(grid_for((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, positions, m, n, (u32*)words);
  return launched();
}

int item_mask_clear(const int64_t* positions, int64_t m, int64_t n, void* words, hipStream_t stream) {
  hipLaunchKernelGGL(mask_bits_clear_kernel, dim3(grid_for((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, positions, m, n, (u32*)words);
  return launched();
}

int64_t item_mask_tile_bits() { return kTileBits; }

size_t item_mask_positions_workspace_bytes(int rows, int64_t n) {
  const int64_t tiles = (item_mask_words(n) + kTileWords - 1) / kTileWords;
  return (size_t)(tiles + 1) * (size_t)rows * sizeof(int64_t);
}

int item_mask_positions(const void* words, int rows, int64_t n, int64_t* out, int64_t out_ld, void* workspace, hipStream_t stream) {
  const int64_t n_words = item_mask_words(n), tiles = (n_words + kTileWords - 1) / kTileWords;
  int64_t* ws = (int64_t*)workspace;
  const u32* w = (const u32*)words;
  hipLaunchKernelGGL(item_mask_tile_counts_kernel, dim3(grid_for(tiles * rows)), dim3(kThreads), 0, stream, w, rows, n, n_words, tiles, ws);
  if (launched() != kOk) return kErrLaunch;
  hipLaunchKernelGGL(item_mask_tile_scan_kernel, dim3((unsigned)rows), dim3(kThreads), 0, stream, rows, tiles, ws);
  if (launched() != kOk) return kErrLaunch;
  if (out_ld == 0) return kOk;
  hipLaunchKernelGGL(item_mask_tile_write_kernel, dim3(grid_for(tiles * rows)), dim3(kThreads), 0, stream, w, rows, n, n_words, tiles, ws, out, out_ld);
  if (launched() != kOk) return kErrLaunch;
  hipLaunchKernelGGL(item_mask_pad_kernel, dim3(grid_for((out_ld * rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, rows, tiles, ws, out, out_ld);
  return launched();
}

int scores_mask(float* scores, int64_t ld, int rows, int64_t n, int64_t first_item, const void* words, int64_t words_row_stride, float fill,
                const int32_t* run_if, hipStream_t stream) {
  const int64_t chunks = (n + (int64_t)kThreads * kMaskPerThread - 1) / ((int64_t)kThreads * kMaskPerThread);
  hipLaunchKernelGGL(scores_mask_kernel, dim3(grid_for(chunks * rows)), dim3(kThreads), 0, stream, scores, ld, rows, n, first_item, (const u32*)words,
                     words_row_stride, fill, run_if);
  return launched();
}

}  // namespace mol
