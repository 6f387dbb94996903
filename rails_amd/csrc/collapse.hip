// Collapsing a ranked list by item group: at most one result per group, or at most m.  Three kernels:
//   collapse_walk_kernel   one workgroup per row over a ranked list of D (score, position) entries in key order: the first k entries whose
//                          group has not occurred earlier in the list, the seen-id filter inside (rails_topk_collapse); its quota form keeps
//                          the first m entries of every group (rails_topk_collapse_quota)
//   group_next_kernel      streams a (rows, n) score matrix: table[row][rank] = max over the group's eligible items of the topk_keys.h key
//                          (rails_scores_group_max) -- the exact fallback where one group owns the head of the ranking; bounded from above
//                          by the previous round's table, round t leaves every group's (t + 1)-th best eligible item
//                          (rails_scores_group_next) -- the fallback of a quota
//   topk_keys_kernel       the k largest keys of every row of that table, by MSD radix selection, decoded (rails_topk_keys)
// The kernels see DENSE group ranks (int32 in [0, G), every ungrouped item a rank of its own), never the callers' sparse keys.
#include "mol_kernels.h"
#include "ranked_list.h"
#include "score_rows.h"
#include "topk_keys.h"
#include "wave_ops.h"

namespace mol {

constexpr int kCollapseThreads = kSortThreads;       // 1024: the in-LDS sorts' workgroup
constexpr int kCollapseMaxDepth = 16384;             // entries of one ranked list: what lds_sort_desc sorts

// ---- the walk ----------------------------------------------------------------------------------------------------
// Entry j of a row is ELIGIBLE iff its position is one of the corpus, its score is above -inf (what the masks write) and its id is not in
// the row's seen set.  An eligible entry SURVIVES iff no eligible entry before it has its group rank.  "First occurrence" is found by a sort,
// not a hash table: the key (rank + 1, ~j) of every eligible entry (0: not eligible, the padding of topk_keys.h) is sorted descending in LDS,
// which puts the entries of one rank side by side with the smallest j first -- the head of every run survives.  A prefix scan over the
// survivor flags in list order compacts the first k.  Deterministic, order-preserving, no probe loops.
// LDS: sort_slots keys | depth survivor bytes (dynamic), one tile of seen ids and the scan's wave totals (static).
// QUOTA: an eligible entry survives iff FEWER THAN max_per_group eligible entries before it have its group rank -- its index within its run
// of the sorted array is below max_per_group.  The run's start is the last run head at or before the slot: every thread takes a contiguous
// segment of the sorted slots, a block-wide max-scan of the segments' last head indices hands it the start of the run that reaches into its
// segment, and it walks the segment once.  No LDS per entry beyond what the plain walk holds; max_per_group = 1 keeps exactly the run heads.
template <bool QUOTA>
__global__ __launch_bounds__(kCollapseThreads) void collapse_walk_kernel(
    const float* __restrict__ scores, int64_t ld, const int64_t* __restrict__ positions, int depth, int npad, int sort_slots,
    const int32_t* __restrict__ ranks, int64_t n_items, const int64_t* __restrict__ ids, const int64_t* __restrict__ invalid, int width, int k,
    int max_per_group, float* __restrict__ out_scores, int64_t* __restrict__ out_pos, int64_t* __restrict__ out_ids,
    int32_t* __restrict__ out_counts, int32_t* __restrict__ out_of_range) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
  unsigned char* surv = reinterpret_cast<unsigned char*>(keys + sort_slots);      // [depth]
  __shared__ int64_t seen[kSeenTile];
  __shared__ int wave_tot[kCollapseThreads / 64];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* srow = scores + (int64_t)row * ld;
  const int64_t* prow = positions + (int64_t)row * depth;

  for (int j = tid; j < depth; j += kCollapseThreads) {
    const int64_t p = prow[j];
    surv[j] = (p >= 0 && p < n_items && srow[j] > -INFINITY) ? 1 : 0;
  }
  drop_seen<kCollapseThreads>(surv, depth, [&](int j) { return prow[j]; }, ids, invalid + (int64_t)row * width, width, seen);
  __syncthreads();
  for (int j = tid; j < npad; j += kCollapseThreads) {
    unsigned long long kv = 0ull;
    if (j < depth && surv[j]) kv = ((unsigned long long)((unsigned int)ranks[prow[j]] + 1u) << 32) | (unsigned int)(~(unsigned int)j);
    keys[j] = kv;
  }
  __syncthreads();
  for (int j = tid; j < depth; j += kCollapseThreads) surv[j] = 0;
  lds_sort_desc(keys, npad);                            // (ends with a barrier)
  if (QUOTA) {
    const int per = npad / kCollapseThreads, i0 = tid * per;      // (npad is a multiple of the workgroup)
    int last_head = -1;
    for (int i = i0; i < i0 + per; ++i) {
      const unsigned long long kv = keys[i];
      if (kv != 0ull && (i == 0 || (keys[i - 1] >> 32) != (kv >> 32))) last_head = i;
    }
    int start = block_scan_max_excl<kCollapseThreads>(last_head, -1, wave_tot);
    for (int i = i0; i < i0 + per; ++i) {
      const unsigned long long kv = keys[i];
      if (kv == 0ull) break;                              // the padding sorts last
      if (i == 0 || (keys[i - 1] >> 32) != (kv >> 32)) start = i;
      if (i - start < max_per_group) surv[~(unsigned int)(kv & 0xFFFFFFFFull)] = 1;
    }
  } else {
    for (int i = tid; i < npad; i += kCollapseThreads) {
      const unsigned long long kv = keys[i];
      if (kv != 0ull && (i == 0 || (keys[i - 1] >> 32) != (kv >> 32))) surv[~(unsigned int)(kv & 0xFFFFFFFFull)] = 1;
    }
  }
  __syncthreads();
  const int total = emit_first_k<kCollapseThreads>(
      surv, depth, k, wave_tot,
      [&](int j, int o) {
        const int64_t p = prow[j];
        out_scores[(int64_t)row * k + o] = srow[j];
        out_pos[(int64_t)row * k + o] = p;
        out_ids[(int64_t)row * k + o] = ids != nullptr ? ids[p] : p;
      },
      [&](int e) {
        out_scores[(int64_t)row * k + e] = -INFINITY;
        out_pos[(int64_t)row * k + e] = -1;
        out_ids[(int64_t)row * k + e] = -1;
      });
  if (tid == 0) {
    out_counts[row] = total;
    if (total < k) *out_of_range = 1;                   // every writer stores the same value
  }
}

// max_per_group == 0: the plain walk (rails_topk_collapse); >= 1: the quota form, a kernel of its own.
int topk_collapse(const float* scores, int64_t ld, const int64_t* positions, int rows, int depth, const int32_t* ranks, int64_t n_items,
                  const int64_t* ids, const int64_t* invalid, int width, int k, int max_per_group, float* out_scores, int64_t* out_pos,
                  int64_t* out_ids, int32_t* out_counts, int32_t* out_of_range, hipStream_t stream) {
  if (rows <= 0 || k <= 0) return kOk;
  if (depth < 1 || depth > kCollapseMaxDepth) {
    set_error("topk_collapse: depth = %d outside [1, %d]", depth, kCollapseMaxDepth);
    return kErrUnsupported;
  }
  const int npad = next_pow2(depth, kSortThreads);
  const int sort_slots = npad <= kSortThreads ? 3 * npad : npad;      // lds_sort_desc's exchange buffer
  const int lds = sort_slots * (int)sizeof(unsigned long long) + (depth + 15) / 16 * 16;
  constexpr int max_lds = kCollapseMaxDepth * ((int)sizeof(unsigned long long) + 1);
  if (max_per_group > 0) {
    static DynLdsOnce once_quota;
    if (ensure_dyn_lds(once_quota, reinterpret_cast<const void*>(&collapse_walk_kernel<true>), max_lds) != kOk) return kErrLaunch;
    hipLaunchKernelGGL(collapse_walk_kernel<true>, dim3(rows), dim3(kCollapseThreads), lds, stream, scores, ld, positions, depth, npad, sort_slots,
                       ranks, n_items, ids, invalid, width, k, max_per_group, out_scores, out_pos, out_ids, out_counts, out_of_range);
    return launched();
  }
  static DynLdsOnce once;
  if (ensure_dyn_lds(once, reinterpret_cast<const void*>(&collapse_walk_kernel<false>), max_lds) != kOk) return kErrLaunch;
  hipLaunchKernelGGL(collapse_walk_kernel<false>, dim3(rows), dim3(kCollapseThreads), lds, stream, scores, ld, positions, depth, npad, sort_slots,
                     ranks, n_items, ids, invalid, width, k, 1, out_scores, out_pos, out_ids, out_counts, out_of_range);
  return launched();
}

// ---- the exact fallback: per-group maxima of a score matrix ---------------------------------------------------------------------------
// table[row][rank[first_item + x]] = max(., make_key(score, first_item + x)) for every FINITE entry x < n of the row whose id is not in the
// row's seen set: afterwards a group's slot holds the key of its best eligible item under (score desc, position asc), 0 where it has none.
// A slot only grows, so an entry whose key does not beat a plain read of its slot is dropped before its id is looked up -- after the first
// few items of a group, most are.  One workgroup per (chunk of kGroupMaxChunk columns, row); the row's seen ids sit in LDS.
// The rounds of a quota's fallback bound the same pass from above: an entry enters table[row][r] only where the previous round's slot
// below[row][r] is non-zero and its key lies BELOW that slot: round t then holds the key of every group's (t + 1)-th best eligible item, 0
// once the group is exhausted.  below == NULL is round 0 (no bound: the group maxima themselves).  The table and the bound take their own
// row strides, so the m rounds of a row lie side by side as one row of m * n_groups keys for topk_keys_kernel.
constexpr int kGroupMaxThreads = 256;
constexpr int kGroupMaxChunk = 4096;
constexpr int kGroupMaxSeen = 4096;      // seen ids per row

__global__ __launch_bounds__(kGroupMaxThreads) void group_next_kernel(const float* __restrict__ scores, int64_t ld, int64_t n, int64_t first_item,
                                                                     const int32_t* __restrict__ ranks, int64_t n_groups,
                                                                     unsigned long long* __restrict__ table, int64_t table_stride,
                                                                     const unsigned long long* __restrict__ below, int64_t below_stride,
                                                                     const int64_t* __restrict__ ids, const int64_t* __restrict__ invalid, int width) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long gm_seen[];      // [width]
  const int row = blockIdx.y, tid = threadIdx.x;
  for (int w = tid; w < width; w += kGroupMaxThreads) gm_seen[w] = (unsigned long long)invalid[(int64_t)row * width + w];
  __syncthreads();
  const int64_t begin = (int64_t)blockIdx.x * kGroupMaxChunk;
  const int64_t end = begin + kGroupMaxChunk < n ? begin + kGroupMaxChunk : n;
  const float* srow = scores + (int64_t)row * ld;
  unsigned long long* trow = table + (int64_t)row * table_stride;
  const unsigned long long* brow = below != nullptr ? below + (int64_t)row * below_stride : nullptr;
  for (int64_t x = begin + tid; x < end; x += kGroupMaxThreads) {
    const float s = srow[x];
    if (!(fabsf(s) < INFINITY)) continue;               // -inf (masked), +inf, NaN
    const int64_t p = first_item + x;
    const int32_t r = ranks[p];
    if (r < 0 || r >= n_groups) continue;
    const unsigned long long kv = make_key(s, (unsigned int)p);
    if (brow != nullptr) {
      const unsigned long long bound = brow[r];        // (the previous round is complete: a plain read)
      if (bound == 0ull || kv >= bound) continue;
    }
    if (kv <= __atomic_load_n(&trow[r], __ATOMIC_RELAXED)) continue;
    if (width > 0) {
      const unsigned long long id = (unsigned long long)(ids != nullptr ? ids[p] : p);
      if (seen_id(gm_seen, width, id)) continue;
    }
    atomicMax(&trow[r], kv);
  }
}

// One pass of the kernel for either entry: `entry`'s limits, its clear of a contiguous table (rails_scores_group_max's clear_table), the launch.
static int group_table_pass(const char* entry, const float* scores, int64_t ld, int rows, int64_t n, int64_t first_item, const int32_t* ranks,
                            int64_t n_groups, unsigned long long* table, int64_t table_stride, bool clear_table, const unsigned long long* below,
                            int64_t below_stride, const int64_t* ids, const int64_t* invalid, int width, hipStream_t stream) {
  if (width > kGroupMaxSeen) { set_error("%s: width = %d beyond %d seen ids per row", entry, width, kGroupMaxSeen); return kErrUnsupported; }
  if (first_item + n > 0xFFFFFFFFll) { set_error("%s: positions beyond 32 bits", entry); return kErrUnsupported; }
  if (rows > 65535) { set_error("%s: more than 65 535 rows", entry); return kErrUnsupported; }
  if (clear_table && hipMemsetAsync(table, 0, sizeof(unsigned long long) * (size_t)rows * (size_t)n_groups, stream) != hipSuccess) return kErrLaunch;
  if (n <= 0) return kOk;
  const unsigned int blocks = (unsigned int)((n + kGroupMaxChunk - 1) / kGroupMaxChunk);
  hipLaunchKernelGGL(group_next_kernel, dim3(blocks, rows), dim3(kGroupMaxThreads), sizeof(unsigned long long) * (size_t)width, stream, scores, ld, n,
                     first_item, ranks, n_groups, table, table_stride, below, below_stride, ids, invalid, width);
  return launched();
}

int scores_group_next(const float* scores, int64_t ld, int rows, int64_t n, int64_t first_item, const int32_t* ranks, int64_t n_groups,
                      unsigned long long* table, int64_t table_stride, const unsigned long long* below, int64_t below_stride, const int64_t* ids,
                      const int64_t* invalid, int width, hipStream_t stream) {
  if (rows <= 0 || n_groups <= 0 || n <= 0) return kOk;
  return group_table_pass("scores_group_next", scores, ld, rows, n, first_item, ranks, n_groups, table, table_stride, false, below, below_stride, ids,
                          invalid, width, stream);
}

// Round 0 on a table of n_groups keys per row; an empty pass (n == 0) still clears.
int scores_group_max(const float* scores, int64_t ld, int rows, int64_t n, int64_t first_item, const int32_t* ranks, int64_t n_groups,
                     unsigned long long* table, int clear_table, const int64_t* ids, const int64_t* invalid, int width, hipStream_t stream) {
  if (rows <= 0 || n_groups <= 0) return kOk;
  return group_table_pass("scores_group_max", scores, ld, rows, n, first_item, ranks, n_groups, table, n_groups, clear_table != 0, nullptr, 0, ids, invalid,
                          width, stream);
}

// ---- top-k of a key table -------------------------------------------------------------------------------------------
// One workgroup per row.  The keys of a row are distinct (a key holds its position), zeros aside, so "the kk largest" (kk = min(k, non-zero
// keys)) is the set of keys >= the kk-th largest, found by MSD radix selection -- eight passes of one byte, a 256-bin LDS histogram of the keys
// that match the prefix so far (sublist_select_kernel's scheme over a row of any length) -- and collected in a ninth pass, sorted in LDS
// (lds_sort_desc) and decoded with the codec of topk_keys.h.
constexpr int kKeysThreads = kSortThreads;
constexpr int kKeysMaxK = 512;

__global__ __launch_bounds__(kKeysThreads) void topk_keys_kernel(const unsigned long long* __restrict__ table, int64_t n_groups, int k,
                                                                const int64_t* __restrict__ ids, float* __restrict__ out_scores,
                                                                int64_t* __restrict__ out_pos, int64_t* __restrict__ out_ids,
                                                                int32_t* __restrict__ out_counts) {
  __shared__ __attribute__((aligned(16))) unsigned long long sel[3 * kKeysThreads];      // the winners + lds_sort_desc's exchange buffer
  __shared__ unsigned int hist[256];
  __shared__ unsigned int nonzero, taken;
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned int s_remaining;
  const int row = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* trow = table + (int64_t)row * n_groups;
  if (tid == 0) { nonzero = 0u; taken = 0u; s_prefix = 0ull; }
  __syncthreads();
  unsigned int nz = 0u;
  for (int64_t g = tid; g < n_groups; g += kKeysThreads) nz += trow[g] != 0ull ? 1u : 0u;
  nz = wave_sum(nz);
  if ((tid & 63) == 0 && nz) atomicAdd(&nonzero, nz);
  __syncthreads();
  const unsigned int kk = nonzero < (unsigned int)k ? nonzero : (unsigned int)k;
  if (tid == 0) s_remaining = kk;
  for (int i = tid; i < kKeysThreads; i += kKeysThreads) sel[i] = 0ull;
  __syncthreads();
  if (kk > 0u) {
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0u;
      __syncthreads();
      const unsigned long long prefix = s_prefix;
      const unsigned long long hi_mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
      for (int64_t g = tid; g < n_groups; g += kKeysThreads) {
        const unsigned long long kv = trow[g];
        if (kv != 0ull && (kv & hi_mask) == prefix) atomicAdd(&hist[(unsigned int)(kv >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {                                   // the byte whose bin holds the remaining-th largest matching key
        unsigned int rem = s_remaining, above = 0u;
        int d = 255;
        for (; d > 0; --d) {
          if (above + hist[d] >= rem) break;
          above += hist[d];
        }
        s_remaining = rem - above;
        s_prefix = prefix | ((unsigned long long)d << shift);
      }
      __syncthreads();
    }
    const unsigned long long threshold = s_prefix;      // the kk-th largest key itself
    for (int64_t g = tid; g < n_groups; g += kKeysThreads) {
      const unsigned long long kv = trow[g];
      if (kv != 0ull && kv >= threshold) {
        const unsigned int slot = atomicAdd(&taken, 1u);
        if (slot < (unsigned int)kKeysThreads) sel[slot] = kv;
      }
    }
    __syncthreads();
    lds_sort_desc(sel, kKeysThreads);
  }
  for (int e = tid; e < k; e += kKeysThreads) {
    const unsigned long long kv = sel[e];
    const bool real = kv != 0ull;
    const int64_t p = real ? (int64_t)key_pos(kv) : -1;
    out_scores[(int64_t)row * k + e] = real ? unorderable(key_score(kv)) : -INFINITY;
    out_pos[(int64_t)row * k + e] = p;
    out_ids[(int64_t)row * k + e] = real ? (ids != nullptr ? ids[p] : p) : -1;
  }
  if (tid == 0) out_counts[row] = (int32_t)nonzero;
}

int topk_keys(const unsigned long long* table, int rows, int64_t n_groups, int k, const int64_t* ids, float* out_scores, int64_t* out_pos,
              int64_t* out_ids, int32_t* out_counts, hipStream_t stream) {
  if (rows <= 0 || k <= 0) return kOk;
  if (k > kKeysMaxK) { set_error("topk_keys: k = %d beyond %d", k, kKeysMaxK); return kErrUnsupported; }
  if (n_groups < 1) { set_error("topk_keys: no groups"); return kErrInvalid; }
  hipLaunchKernelGGL(topk_keys_kernel, dim3(rows), dim3(kKeysThreads), 0, stream, table, n_groups, k, ids, out_scores, out_pos, out_ids, out_counts);
  return launched();
}

}  // namespace mol
