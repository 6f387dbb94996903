// The 64-bit selection key and the in-LDS sorts of the top-k kernels (topk.hip, group_keys.hip, mol_coarse.hip).  Device code, all of it
// forced inline; next_pow2 alone also serves the host.
//
// Every score becomes a 64-bit key  (orderable(score) << 32) | ~position : all keys of a row are distinct, so "the k largest keys" is a
// unique set and its descending order is "score descending, then position ascending" -- the deterministic tie rule that makes
// 1/2/4/8-GPU results identical.  Key 0 lies below every real key (orderable() never returns 0 for a finite / inf score) and is the padding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mol {

constexpr int kSortThreads = 1024;    // workgroup size of block_sort_desc_multi and lds_sort_desc

// the smallest power of two >= v that is also >= at_least (itself a power of two)
__host__ __device__ inline int next_pow2(int v, int at_least = 1) { int p = at_least; while (p < v) p <<= 1; return p; }

// ---- key codec ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int orderable(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unorderable(unsigned int k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ unsigned long long make_key(float score, unsigned int pos) {
  return ((unsigned long long)orderable(score) << 32) | (unsigned int)(~pos);
}
__device__ __forceinline__ unsigned int key_score(unsigned long long kv) { return (unsigned int)(kv >> 32); }   // orderable(score); unorderable() gives the score
__device__ __forceinline__ unsigned int key_pos(unsigned long long kv) { return ~(unsigned int)(kv & 0xFFFFFFFFull); }

// ---- block bitonic sort, one key per thread (npad <= 1024) ----------------------------------------------------
// Thread i holds key i.  Compare-exchange partners at distance < 64 sit in the same wavefront and are exchanged with
// ds_bpermute (no barrier); only the distances >= 64 go through LDS (one barrier each, double-buffered): 3 barriers for
// 256 keys, 10 for 1024, against 36 / 55 barrier-separated LDS passes for the plain loop (~0.4 us each with 16 waves).
// Returns the key of descending rank threadIdx.x.  `buf` needs 2 * npad entries; all threads of the block must call.
__device__ __forceinline__ unsigned long long block_sort_desc(unsigned long long key, int npad, unsigned long long* buf) {
  const int i = threadIdx.x;
  int flip = 0;
  for (int size = 2; size <= npad; size <<= 1) {
    const bool desc = (i & size) == 0;
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      unsigned long long other;
      if (stride >= 64) {
        unsigned long long* b = buf + flip * npad;
        flip ^= 1;
        if (i < npad) b[i] = key;
        __syncthreads();
        other = i < npad ? b[i ^ stride] : 0ull;
      } else {
        other = __shfl_xor(key, stride, 64);
      }
      const bool lower = (i & stride) == 0;
      const bool take_max = lower == desc;
      const unsigned long long mx = key > other ? key : other, mn = key > other ? other : key;
      key = take_max ? mx : mn;
    }
  }
  return key;
}

// ---- more keys than threads: KPT = npad / 1024 keys per thread (npad = 2048 .. 16384) --------------------------------
// Thread t holds the keys of LDS slots [t * KPT, (t + 1) * KPT).  Compare-exchange distances below KPT stay inside the
// thread, distances below 64 * KPT are one ds_bpermute per key inside the wavefront, only the rest go through LDS (two
// barriers each, `keys` itself is the exchange buffer): 10 LDS steps of 78 for 4096 keys, where the plain loop took a
// barrier-separated LDS pass for every step (39 us per 4096-key row).
// In: keys[0, npad) in LDS, visible to all threads.  Out: the same, sorted descending, visible to all threads.
template <int KPT>
__device__ __forceinline__ void block_sort_desc_multi(unsigned long long* keys) {
  constexpr int npad = KPT * kSortThreads;
  const int t = threadIdx.x;
  unsigned long long key[KPT];
#pragma unroll
  for (int j = 0; j < KPT; ++j) key[j] = keys[t * KPT + j];
  for (int size = 2; size <= npad; size <<= 1) {
    for (int stride = size >> 1; stride >= KPT; stride >>= 1) {
      unsigned long long other[KPT];
      if (stride >= 64 * KPT) {
        __syncthreads();                       // every thread is done reading the previous exchange
#pragma unroll
        for (int j = 0; j < KPT; ++j) keys[t * KPT + j] = key[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KPT; ++j) other[j] = keys[(t * KPT + j) ^ stride];
      } else {
#pragma unroll
        for (int j = 0; j < KPT; ++j) other[j] = __shfl_xor(key[j], stride / KPT, 64);
      }
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const int e = t * KPT + j;
        const bool take_max = ((e & stride) == 0) == ((e & size) == 0);
        const unsigned long long mx = key[j] > other[j] ? key[j] : other[j], mn = key[j] > other[j] ? other[j] : key[j];
        key[j] = take_max ? mx : mn;
      }
    }
#pragma unroll
    for (int s = KPT / 2; s > 0; s >>= 1) {
      if (s < size) {
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
          if ((j & s) == 0) {
            const bool desc = (((t * KPT + j) & size) == 0);
            const unsigned long long a = key[j], b = key[j | s];
            const bool sw = (a < b) == desc;
            key[j] = sw ? b : a;
            key[j | s] = sw ? a : b;
          }
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < KPT; ++j) keys[t * KPT + j] = key[j];
  __syncthreads();
}

// ---- block rank (64 <= npad <= 512 keys in LDS, zero-padded, distinct) ------------------------------------------
// A key's descending rank is the number of larger keys.  The 1024 threads split into 1024/npad parts; thread (c, part)
// counts the keys of its slice that exceed key c (broadcast 16-byte LDS reads, no conflicts) and adds the count to
// rank_buf[c].  Two barriers and ~npad^2/2048 LDS reads per thread, against the 36-45 dependent shuffle steps of the
// bitonic network (5.6 us -> ~1.5 us for the ~220 candidates of a k = 200 selection).  Afterwards every thread with
// part 0 holds (key c, rank of key c).
__device__ __forceinline__ void block_rank_desc(const unsigned long long* keys, int npad, unsigned int* rank_buf,
                                                unsigned long long& mine, unsigned int& rank, bool& owner) {
  const int tid = threadIdx.x;
  const int c = tid & (npad - 1), part = tid / npad;
  const int span = npad / ((int)blockDim.x / npad);      // keys per slice (>= 4 for npad >= 64 at 1024 threads)
  if (tid < npad) rank_buf[tid] = 0u;
  __syncthreads();
  mine = keys[c];
  unsigned int cnt = 0;
  const ulonglong2* p = reinterpret_cast<const ulonglong2*>(keys + part * span);
  for (int i = 0; i < span / 2; ++i) {
    const ulonglong2 x = p[i];
    cnt += x.x > mine ? 1u : 0u;
    cnt += x.y > mine ? 1u : 0u;
  }
  if (cnt) atomicAdd(&rank_buf[c], cnt);
  __syncthreads();
  rank = rank_buf[c];
  owner = part == 0;
}

// ---- the plain bitonic network over keys[0, npad) in LDS, NT threads, one barrier per step ---------------------------
// The slow sort: any power of two npad, any workgroup size, no exchange buffer.  In: keys visible to all threads.  Out: sorted
// (DESC: descending), visible to all threads.  All threads of the workgroup call.
template <int NT, bool DESC>
__device__ __forceinline__ void lds_bitonic(unsigned long long* keys, int npad) {
  for (int size = 2; size <= npad; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (npad >> 1); t += NT) {
        const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
        const int hi = lo | stride;
        const bool first = ((lo & size) == 0);
        const unsigned long long a = keys[lo], b = keys[hi];
        if ((DESC ? a < b : a > b) == first) { keys[lo] = b; keys[hi] = a; }
      }
      __syncthreads();
    }
  }
}
template <int NT>
__device__ __forceinline__ void lds_bitonic_desc(unsigned long long* keys, int npad) { lds_bitonic<NT, true>(keys, npad); }
template <int NT>
__device__ __forceinline__ void lds_bitonic_asc(unsigned long long* keys, int npad) { lds_bitonic<NT, false>(keys, npad); }

// ---- the fast sort of keys[0, npad) in LDS, descending, by a workgroup of kSortThreads ------------------------------
// npad is a power of two <= 16384.  npad <= 1024 runs block_sort_desc and needs keys[npad, 3 npad) as its exchange buffer (the
// launch reserves 3 * npad slots); wider rows run block_sort_desc_multi in place.  In: keys visible to all threads.  Out: sorted,
// visible to all threads.  lds_sort_desc_wide is the npad = 2048 .. MAX_KPT * 1024 half on its own, for kernels that
// have no exchange buffer or bound npad lower.
template <int MAX_KPT = 16>
__device__ __forceinline__ void lds_sort_desc_wide(unsigned long long* keys, int npad) {
  if (MAX_KPT == 2 || npad == 2 * kSortThreads) block_sort_desc_multi<2>(keys);
  else if (MAX_KPT == 4 || npad == 4 * kSortThreads) block_sort_desc_multi<4>(keys);
  else if (MAX_KPT == 8 || npad == 8 * kSortThreads) block_sort_desc_multi<8>(keys);
  else block_sort_desc_multi<16>(keys);
}
__device__ __forceinline__ void lds_sort_desc(unsigned long long* keys, int npad) {
  const int tid = threadIdx.x;
  if (npad <= kSortThreads) {   // one key per thread, sorted mostly in registers
    unsigned long long kv = tid < npad ? keys[tid] : 0ull;
    kv = block_sort_desc(kv, npad, keys + npad);
    __syncthreads();
    if (tid < npad) keys[tid] = kv;
    __syncthreads();
  } else {
    lds_sort_desc_wide(keys, npad);
  }
}

// ---- merging R descending lists of k keys without a sort ----------------------------------------------------------
// keys[r * k + j] is entry j of list r.  When every list is descending, the merged rank of key i = (r, j) is j + the number of keys
// of the other lists that precede it: one binary search per other list.  TIES_BY_LIST = false is for distinct keys (a key precedes
// the larger ones only); true also counts the EQUAL keys of the lists o < r, which makes the order total among pads and repeated
// keys.  The search stops once the rank has reached `limit` (such a key is not written); the value returned is then >= limit.
template <bool TIES_BY_LIST>
__device__ __forceinline__ int sorted_lists_rank(const unsigned long long* keys, int R, int k, int i, int limit) {
  const unsigned long long kv = keys[i];
  const int r = i / k, j = i - r * k;
  int rank = j;
  for (int o = 0; o < R && rank < limit; ++o) {
    if (o == r) continue;
    const unsigned long long* list = keys + o * k;   // descending
    int lo = 0, hi = k;
    while (lo < hi) {                                // first index whose key does not precede kv
      const int mid = (lo + hi) >> 1;
      const unsigned long long x = list[mid];
      if (x > kv || (TIES_BY_LIST && o < r && x == kv)) lo = mid + 1; else hi = mid;
    }
    rank += lo;
  }
  return rank;
}
// Whether every list is descending, for the whole workgroup of NT threads (one barrier).  `unsorted` is a shared flag the caller
// zeroed before the barrier that published the keys.
template <int NT>
__device__ __forceinline__ bool sorted_lists_check(const unsigned long long* keys, int count, int k, int* unsorted) {
  bool bad = false;
  for (int i = threadIdx.x; i + 1 < count; i += NT)
    if ((i + 1) % k != 0 && keys[i] < keys[i + 1]) bad = true;
  if (bad) *unsorted = 1;
  __syncthreads();
  return !*unsorted;
}

}  // namespace mol
