// Device-resident item id -> position map (rails_id_map_*): the in-place corpus API addressed by id.
//
// Table: open addressing with linear probing in device memory, `slots` a power of two:
//   int64 keys[slots], then int32 values[slots]                                  (12 bytes per slot)
//   EMPTY  = INT64_MIN      never held a key: a probe ends here
//   ERASED = INT64_MIN + 1  a tombstone: a probe walks over it, an insert does NOT reuse it (the host rebuilds instead)
// Both are reserved: an id equal to either is counted and never stored.  The home slot of an id is mix(id) & (slots - 1), with
// mix the splitmix64 step the synthetic item tables already hash with (mol_index.hip, oracle/mol_oracle.py _splitmix64), on the
// id's 64 bits as an unsigned word, all arithmetic mod 2^64:
//   z = id + 0x9E3779B97F4A7C15
//   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//   z = (z ^ (z >> 27)) * 0x94D049BB133111EB
//   mix(id) = z ^ (z >> 31)
// Every step is invertible (an odd multiplier has an inverse mod 2^64, x ^ (x >> s) is undone by repeating the shift), so mix is a
// bijection of the 64-bit words: ids with a chosen home slot can be constructed, which the tests do.
//
// One thread per id, no LDS.  Every probe loop runs at most `slots` iterations and ends by raising its counter or writing -1: a full or
// damaged table costs time, never a hang.  Which key lands in which slot depends on the order the CAS operations win in -- the contract
// is on lookups, not on the table's bytes.
#include <hip/hip_runtime.h>

#include <limits.h>

#include "mol_kernels.h"

namespace mol {

namespace {

typedef unsigned long long u64;
constexpr u64 kEmpty = 0x8000000000000000ull;    // INT64_MIN
constexpr u64 kErased = 0x8000000000000001ull;   // INT64_MIN + 1

__device__ __forceinline__ u64 id_mix(u64 x) {
  u64 z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ u64 key_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ void count(int32_t* c) { __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

}  // namespace

__global__ void id_map_clear_kernel(u64* __restrict__ keys, int32_t* __restrict__ values, int64_t slots) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (int64_t)gridDim.x * blockDim.x) {
    keys[i] = kEmpty;
    values[i] = 0;
  }
}

// flags[0]: ids already in the table or twice in this call; flags[1]: reserved ids (and positions outside int32); flags[2]: no slot found.
// A slot is claimed by a 64-bit CAS on EMPTY only.  Keys never return to EMPTY, so a slot a thread walked past stays what it was: of two
// threads with one id exactly one claims a slot and the other meets that key (in its load or in the word its failed CAS returns).
__global__ void id_map_insert_kernel(u64* __restrict__ keys, int32_t* __restrict__ values, int64_t slots, const int64_t* __restrict__ ids,
                                     const int64_t* __restrict__ positions, int64_t first, int64_t m, int32_t* __restrict__ flags) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= m) return;
  const u64 id = (u64)ids[u];
  const int64_t pos = positions ? positions[u] : first + u;
  if (id == kEmpty || id == kErased || pos < 0 || pos > (int64_t)INT_MAX) { count(flags + 1); return; }
  const u64 mask = (u64)slots - 1;
  u64 h = id_mix(id) & mask;
  for (int64_t i = 0; i < slots; ++i, h = (h + 1) & mask) {
    u64 k = key_load(keys + h);
    if (k == kEmpty) {
      k = atomicCAS(keys + h, kEmpty, id);
      if (k == kEmpty) { values[h] = (int32_t)pos; return; }
    }
    if (k == id) { count(flags); return; }
  }
  count(flags + 2);
}

// key -> ERASED, by CAS: of two threads erasing one id, one wins and the other walks on to the end of the chain and counts as missing
__global__ void id_map_erase_kernel(u64* __restrict__ keys, int64_t slots, const int64_t* __restrict__ ids, int64_t m, int32_t* __restrict__ missing) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= m) return;
  const u64 id = (u64)ids[u];
  if (id == kEmpty || id == kErased) { count(missing); return; }
  const u64 mask = (u64)slots - 1;
  u64 h = id_mix(id) & mask;
  for (int64_t i = 0; i < slots; ++i, h = (h + 1) & mask) {
    const u64 k = key_load(keys + h);
    if (k == kEmpty) break;
    if (k == id && atomicCAS(keys + h, id, kErased) == id) return;
  }
  count(missing);
}

__global__ void id_map_lookup_kernel(const u64* __restrict__ keys, const int32_t* __restrict__ values, int64_t slots, const int64_t* __restrict__ ids,
                                     int64_t m, int64_t* __restrict__ out) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= m) return;
  const u64 id = (u64)ids[u];
  int64_t found = -1;
  if (id != kEmpty && id != kErased) {
    const u64 mask = (u64)slots - 1;
    u64 h = id_mix(id) & mask;
    for (int64_t i = 0; i < slots; ++i, h = (h + 1) & mask) {
      const u64 k = keys[h];
      if (k == kEmpty) break;
      if (k == id) { found = values[h]; break; }
    }
  }
  out[u] = found;
}

static inline u64* map_keys(void* map) { return reinterpret_cast<u64*>(map); }
static inline int32_t* map_values(void* map, int64_t slots) { return reinterpret_cast<int32_t*>(reinterpret_cast<u64*>(map) + slots); }
static inline unsigned per_id_grid(int64_t m) { return (unsigned)((m + 255) / 256); }

int id_map_clear(void* map, int64_t slots, hipStream_t stream) {
  int64_t blocks = (slots + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(id_map_clear_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, map_keys(map), map_values(map, slots), slots);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int id_map_insert(void* map, int64_t slots, const int64_t* ids, const int64_t* positions, int64_t first, int64_t m, int32_t* flags, hipStream_t stream) {
  hipLaunchKernelGGL(id_map_insert_kernel, dim3(per_id_grid(m)), dim3(256), 0, stream, map_keys(map), map_values(map, slots), slots, ids, positions, first, m,
                     flags);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int id_map_erase(void* map, int64_t slots, const int64_t* ids, int64_t m, int32_t* missing, hipStream_t stream) {
  hipLaunchKernelGGL(id_map_erase_kernel, dim3(per_id_grid(m)), dim3(256), 0, stream, map_keys(map), slots, ids, m, missing);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int id_map_lookup(const void* map, int64_t slots, const int64_t* ids, int64_t m, int64_t* positions_out, hipStream_t stream) {
  hipLaunchKernelGGL(id_map_lookup_kernel, dim3(per_id_grid(m)), dim3(256), 0, stream, reinterpret_cast<const u64*>(map),
                     reinterpret_cast<const int32_t*>(reinterpret_cast<const u64*>(map) + slots), slots, ids, m, positions_out);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace mol
