// HSTU cached incremental decoding, several rows per sequence in one step (rails_hstu_decode_rows): the contiguous run of rows
// [p_b, p_b + m_b) of every sequence re-encoded through every layer against the cached K / V of the rows below them, the cache
// (rails_hstu_decode_layer: v / outputs jagged, q / k padded) gaining those rows in place.  The single-row step (hstu_decode_kernel in
// hstu.hip, one workgroup per sequence, the whole stack in one launch) is untouched; this is the batch-wide route beside it, in which
// a layer's weights are read once per 32 work rows instead of once per sequence.
//
// A WORK ROW is a (sequence, position) pair in one of B * M fixed slots (M = max_rows): slot r = b * M + t is active iff sequence b
// is valid and t < m_b, and stands for position p_b + t.  m_b = counts[b] (M when there is no count array) clamped on the device into
// [1, min(M, len_b - p_b)].  The scheme is kvdec.hip's (the staging loop is written out in both files, the LayerNorm statistics
// of a staged row are encoder_device.h's row_ln_stats): a row tile resolves its 32 slots into an LDS table once (sequence, position,
// jagged row; -1 for an idle slot); an idle slot stages zeros and writes nothing, and its attention workgroup exits before its
// first barrier.  A row's arithmetic depends on neither its slot nor M, so one step over m rows is bit for bit m steps of one row.
//
// hsturows_scan_kernel derives, from the lengths alone, each sequence's jagged offset (an exclusive prefix sum) and its row count into
// the workspace; a sequence whose length lies outside [1, seq_len], which follows a length outside [0, seq_len], whose start lies
// outside [0, length) or whose rows fall outside cache_rows gets offset -1: every one of its slots is idle and its out row is NaN
// (hstu_decode_kernel's policy).  No caller-supplied offset addresses a write.
//
// Per layer three launches over ALL work rows of the batch (3 * n_blocks + 2 launches per step):
//   hsturows_gemm_kernel<0> y = act(LN(x) W_uvqk) for 32 work rows x 64 output columns per workgroup (layer 0: x = [id != 0] (emb *
//                           sqrt(D) + pos_emb[p]) folded in; column tile 0 keeps x); u to the workspace, v into the cache's jagged
//                           row off_b + p, q / k into the padded caches at (b, p)
//   hsturows_attn_kernel   one workgroup per (work row, head): a_h = sum_{j <= p} silu(q_h . k_hj + pos_w[N-1+j-p] +
//                          ts_w[bucket(ts[min(p+1, N-1)] - ts[j])]) / N v_hj, keys from the padded k cache, values from the jagged v rows
//                          (row p's own k / v were written by the launch in front); the bucket is a binary search over the
//                          thresholds staged in LDS
//   hsturows_gemm_kernel<1> x <- (u * LN(a)) W_o^T + b_o + x, also into the cache's outputs[off_b + p]: the next layer's input
// then hsturows_post_kernel: normalize_row (encoder_device.h, the prefill's postprocessor) on the last layer's outputs row at
// len_b - 1 (fresh when the run reaches it, the cached row otherwise).  A layer's attention of row p + 1 needs that layer's fresh k / v of row p: the projection
// launch in front of it, on the same stream, wrote them; each row's own key limit j <= p keeps the new rows causal among themselves.
//
// The row GEMMs are plain fmaf tiles (a lane per output column, eight rows per wave broadcast from LDS, four partial sums k mod 4
// added in a fixed tree), not MFMA: a step has B * M rows, a handful to a few hundred, so the launches are bound by their latency
// and by streaming the weights, not by arithmetic, and the fmaf tile keeps the summation order spelled out.  fp32 throughout,
// -ffp-contract=off, no atomics, no grid-wide barrier, no scratch.
#include <hip/hip_runtime.h>
#include <math.h>

#include "encoder_device.h"
#include "mol_kernels.h"
#include "mol_layout.h"

namespace mol {

namespace {

constexpr int kRowsThreads = 256;
constexpr int kRowsWaves = kRowsThreads / 64;
constexpr int kRowsCols = 64;              // output columns per workgroup: one per lane
constexpr int kRowsTile = 32;              // work rows per workgroup
constexpr int kRowsPerWave = kRowsTile / kRowsWaves;
constexpr int kRowsMaxDim = 1024;          // D and H * dv: the staged A tile is kRowsTile x K floats (128 KiB at the limit)
constexpr int kRowsMaxHead = 32;           // dqk, dv
constexpr int kRowsMaxBuckets = 255;
constexpr int kRowsKBatch0 = 32;           // weights of a lane's column loaded ahead of their FMAs: the uvqk projection (one per load)
constexpr int kRowsKBatch1 = 64;           // ... and the output projection (four per load)
constexpr int kRowsScanThreads = 1024;
constexpr int kRowsMaxGridY = 65535;
constexpr int64_t kRowsMaxSlots = RAILS_HSTU_DECODE_MAX_ROWS;
static_assert(kRowsTile == kTileRows && kRowsThreads == kTileThreads, "the staging loop is written out here and in kvdec.hip for one geometry");
static_assert(kRowsMaxSlots == (int64_t)kRowsMaxGridY * kRowsTile, "rails_amd.h states the grid limit");
static_assert(kRowsMaxSlots * kRowsThreads < (1LL << 32), "the attention grid has its work rows on x");

struct RowsLayer {                    // mirrors rails_hstu_decode_layer
  const float* uvqk; const float* o_w; const float* o_b; const float* ts_w; const float* pos_w;
  float* v; float* q; float* k; float* outputs;
};
static_assert(sizeof(RowsLayer) == sizeof(rails_hstu_decode_layer), "RowsLayer mirrors rails_hstu_decode_layer field for field");

struct RowsArgs {
  const float* emb; const int64_t* ids; const int64_t* positions; const int64_t* counts; const int64_t* lengths; const int64_t* ts;
  const int64_t* thresholds; const float* pos_emb; const RowsLayer* layers;
  int blk, first, n_blocks;
  int B, N, M; int64_t R; int64_t cache_rows; int D, H, dqk, dv, num_buckets, act, mode;
  float eps;
  long long* seq_off;                 // (B) jagged offset of the sequence, -1: left alone
  int* seq_m;                         // (B) rows of the run
  float* x; float* u; float* att;     // work rows: (R, D), (R, H dv), (R, H dv)
  float* out;
};

struct Slot { int b, p; long long row; };   // sequence, position (-1: idle) and jagged row of a work-row slot

__device__ __forceinline__ Slot rows_slot(const RowsArgs& a, int64_t r) {
  const int b = (int)(r / a.M), t = (int)(r - (int64_t)b * a.M);
  const long long off = a.seq_off[b];
  if (off < 0 || t >= a.seq_m[b]) return Slot{b, -1, -1};
  const int p = (int)a.positions[b] + t;     // in [0, len): the scan checked the start and clamped the count
  return Slot{b, p, off + p};
}

// One workgroup.  Chunks of kRowsScanThreads sequences: an inclusive scan of the lengths (and an OR-scan of "a length outside
// [0, N]") by wave shuffles and one LDS pass over the wave totals, the carry kept by every thread.
__global__ __launch_bounds__(kRowsScanThreads) void hsturows_scan_kernel(RowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rows_smem[];
  long long* tot = reinterpret_cast<long long*>(rows_smem);      // [waves]
  int* badw = reinterpret_cast<int*>(tot + kRowsScanThreads / 64);   // [waves]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long carry = 0;
  int carry_bad = 0;
  for (int b0 = 0; b0 < a.B; b0 += kRowsScanThreads) {
    const int b = b0 + tid;
    const long long len = b < a.B ? a.lengths[b] : 0;
    const int bad = len < 0 || len > a.N;
    long long s = len;
    int sb = bad;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long t = __shfl_up(s, o, 64);
      const int tb = __shfl_up(sb, o, 64);
      if (lane >= o) { s += t; sb |= tb; }
    }
    if (lane == 63) { tot[wave] = s; badw[wave] = sb; }
    __syncthreads();
    long long before = carry, all = carry;
    int bad_before = carry_bad, bad_all = carry_bad;
    for (int w = 0; w < kRowsScanThreads / 64; ++w) {
      if (w < wave) { before += tot[w]; bad_before |= badw[w]; }
      all += tot[w];
      bad_all |= badw[w];
    }
    const int below = __shfl_up(sb, 1, 64);                      // the inclusive flag of the lane below: this lane's exclusive one
    if (b < a.B) {
      const long long off = before + s - len;                    // exclusive
      const int pre = bad_before | (lane > 0 ? below : 0);       // a length before this one outside [0, N]: the offset means nothing
      const long long p = a.positions[b];
      const bool ok = !pre && len >= 1 && len <= a.N && p >= 0 && p < len && off + len <= a.cache_rows;
      long long m = 1;
      if (ok) {
        const long long cap = len - p < a.M ? len - p : a.M;
        const long long c = a.counts ? a.counts[b] : (long long)a.M;
        m = c < 1 ? 1 : c > cap ? cap : c;
      }
      a.seq_off[b] = ok ? off : -1;
      a.seq_m[b] = (int)m;
    }
    carry = all;
    carry_bad = bad_all;
    __syncthreads();
  }
}

// The slot table of a row tile, then its A rows.  LDS: A [kRowsTile][ks] (ks = K rounded up to 4, zero-padded), mean / rstd
// [kRowsTile], slot sequence / position [kRowsTile] (ints), slot jagged row [kRowsTile] (64-bit).
struct RowsLds {
  float* As; float* mean_s; float* rstd_s; int* slot_b; int* slot_p; long long* slot_row;
};

__device__ __forceinline__ RowsLds rows_lds(unsigned char* smem, int ks) {
  RowsLds l;
  l.As = reinterpret_cast<float*>(smem);
  l.mean_s = l.As + kRowsTile * ks;
  l.rstd_s = l.mean_s + kRowsTile;
  l.slot_b = reinterpret_cast<int*>(l.rstd_s + kRowsTile);
  l.slot_p = l.slot_b + kRowsTile;
  l.slot_row = reinterpret_cast<long long*>(l.slot_p + kRowsTile);   // 16-byte aligned: ks % 4 == 0
  return l;
}

static size_t rows_lds_bytes(int K) { return sizeof(float) * ((size_t)kRowsTile * ((K + 3) & ~3) + 4 * kRowsTile) + sizeof(long long) * kRowsTile; }

__device__ __forceinline__ void rows_resolve(const RowsArgs& a, const RowsLds& l, int64_t r0, int nr) {
  if (threadIdx.x < kRowsTile) {
    Slot s{-1, -1, -1};
    if ((int)threadIdx.x < nr) s = rows_slot(a, r0 + threadIdx.x);
    l.slot_b[threadIdx.x] = s.b;
    l.slot_p[threadIdx.x] = s.p;
    l.slot_row[threadIdx.x] = s.row;
  }
  __syncthreads();
}

// LayerNorm statistics of each staged row (row_ln_stats), a wave per row
__device__ __forceinline__ void rows_stats(const RowsLds& l, int K, int ks, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < kRowsTile; r += kRowsWaves) row_ln_stats(l.As + r * ks, K, eps, l.mean_s + r, l.rstd_s + r, lane);
  __syncthreads();
}

// MODE 0: the uvqk projection (A = LN(x), W given as (K, n_cols)); MODE 1: the output projection (A = u * LN(a), W as (n_cols, K),
// torch Linear; its rows are read 16 bytes at a time where K and the layer's pointer allow, which changes no sum).
// grid (column tiles, row tiles).
template <int MODE>
__global__ __launch_bounds__(kRowsThreads) void hsturows_gemm_kernel(RowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rows_smem[];
  const int D = a.D, N = a.N, HV = a.H * a.dv, HQ = a.H * a.dqk;
  const int K = MODE == 0 ? D : HV;
  const int n_cols = MODE == 0 ? 2 * (HV + HQ) : D;
  const int ks = (K + 3) & ~3;
  const RowsLds l = rows_lds(rows_smem, ks);
  float* As = l.As;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t r0 = (int64_t)blockIdx.y * kRowsTile;
  const int nr = a.R - r0 < kRowsTile ? (int)(a.R - r0) : kRowsTile;
  const RowsLayer L = a.layers[a.blk];
  rows_resolve(a, l, r0, nr);
  auto live = [&](int r) -> bool { return l.slot_p[r] >= 0; };   // idle slots and tile rows past the last slot: -1

  // ---- stage the A rows (zeros past K and in idle slots), then the LayerNorm statistics of each row, a wave per row
  const float emb_scale = sqrtf((float)D);
  auto load = [&](int i) -> float {
    const int r = i / ks, k = i - r * ks;
    if (k >= K || !live(r)) return 0.0f;
    if (MODE == 1) return a.att[(r0 + r) * HV + k];
    if (!a.first) return a.x[(r0 + r) * D + k];
    const int64_t prow = (int64_t)l.slot_b[r] * N + l.slot_p[r];   // x = [id != 0] (emb * sqrt(D) + pos_emb[p])
    return a.ids[prow] != 0 ? a.emb[prow * D + k] * emb_scale + a.pos_emb[(int64_t)l.slot_p[r] * D + k] : 0.0f;
  };
  for (int i0 = tid; i0 < kRowsTile * ks; i0 += kStageBatch * kRowsThreads) {   // the loop of kvdec.hip's kv_rows_kernel, written out there too
    float v[kStageBatch];
#pragma unroll
    for (int u = 0; u < kStageBatch; ++u) v[u] = i0 + u * kRowsThreads < kRowsTile * ks ? load(i0 + u * kRowsThreads) : 0.0f;
#pragma unroll
    for (int u = 0; u < kStageBatch; ++u)
      if (i0 + u * kRowsThreads < kRowsTile * ks) As[i0 + u * kRowsThreads] = v[u];
  }
  __syncthreads();
  rows_stats(l, K, ks, a.eps);
  // ---- normalise in place: LN(x) (column tile 0 of layer 0 keeps x itself), or u * LN(a)
  for (int i = tid; i < kRowsTile * ks; i += kRowsThreads) {
    const int r = i / ks, k = i - r * ks;
    if (k < K) {
      const float raw = As[i];
      float y = (raw - l.mean_s[r]) * l.rstd_s[r];
      if (MODE == 0) {
        if (a.first && blockIdx.x == 0 && live(r)) a.x[(r0 + r) * D + k] = raw;
      } else if (live(r)) {
        y *= a.u[(r0 + r) * HV + k];
      }
      As[i] = y;
    }
  }
  __syncthreads();

  const int col = blockIdx.x * kRowsCols + lane;
  if (col >= n_cols) return;   // no barrier follows
  const int rw = wave * kRowsPerWave;   // this wave's rows of the tile
  if (rw >= nr) return;
  float acc[kRowsPerWave][4];
#pragma unroll
  for (int j = 0; j < kRowsPerWave; ++j) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0f;
  const bool V4 = MODE == 1 && (K & 3) == 0 && (reinterpret_cast<uintptr_t>(L.o_w) & 15) == 0;   // uniform
  constexpr int kRowsKBatch = MODE == 0 ? kRowsKBatch0 : kRowsKBatch1;
  for (int k0 = 0; k0 < K; k0 += kRowsKBatch) {   // kRowsKBatch weights of this lane's column in flight, then their FMAs
    float wv[kRowsKBatch];
    if (MODE == 0) {                              // (K, n_cols): a wave reads 64 adjacent columns of one k per load
#pragma unroll
      for (int u = 0; u < kRowsKBatch; ++u) wv[u] = k0 + u < K ? L.uvqk[(int64_t)(k0 + u) * n_cols + col] : 0.0f;
    } else {                                      // (n_cols, K): a lane reads its own row, 16 bytes per load where aligned
      const float* wr = L.o_w + (int64_t)col * K;
#pragma unroll
      for (int u = 0; u < kRowsKBatch; u += 4) {
        const int k = k0 + u;
        if (V4) {
          const float4 w4 = k < K ? *reinterpret_cast<const float4*>(wr + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          wv[u] = w4.x; wv[u + 1] = w4.y; wv[u + 2] = w4.z; wv[u + 3] = w4.w;
        } else {
          wv[u] = k < K ? wr[k] : 0.0f;
          wv[u + 1] = k + 1 < K ? wr[k + 1] : 0.0f;
          wv[u + 2] = k + 2 < K ? wr[k + 2] : 0.0f;
          wv[u + 3] = k + 3 < K ? wr[k + 3] : 0.0f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kRowsKBatch; u += 4) {
      const int k = k0 + u;
      if (k >= K) break;   // uniform; the A rows are zero-padded to a multiple of 4 only
#pragma unroll
      for (int j = 0; j < kRowsPerWave; ++j) {
        const float4 x4 = *reinterpret_cast<const float4*>(As + (rw + j) * ks + k);   // the same address in every lane: a broadcast
        acc[j][0] = __builtin_fmaf(x4.x, wv[u], acc[j][0]);
        acc[j][1] = __builtin_fmaf(x4.y, wv[u + 1], acc[j][1]);
        acc[j][2] = __builtin_fmaf(x4.z, wv[u + 2], acc[j][2]);
        acc[j][3] = __builtin_fmaf(x4.w, wv[u + 3], acc[j][3]);
      }
    }
  }
  const float bc = MODE == 1 ? L.o_b[col] : 0.0f;
#pragma unroll
  for (int j = 0; j < kRowsPerWave; ++j) {
    if (rw + j >= nr) break;
    if (!live(rw + j)) continue;   // an idle slot writes nothing, neither work rows nor the cache
    const int64_t r = r0 + rw + j;
    float v = (acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3]);
    if (MODE == 0) {
      if (a.act == 1) v = silu_fast(v);
      const int64_t prow = (int64_t)l.slot_b[rw + j] * N + l.slot_p[rw + j];
      if (col < HV) a.u[r * HV + col] = v;
      else if (col < 2 * HV) L.v[l.slot_row[rw + j] * HV + col - HV] = v;
      else if (col < 2 * HV + HQ) L.q[prow * HQ + col - 2 * HV] = v;
      else L.k[prow * HQ + col - 2 * HV - HQ] = v;
    } else {
      v = v + bc + a.x[r * D + col];
      a.x[r * D + col] = v;
      L.outputs[l.slot_row[rw + j] * D + col] = v;
    }
  }
}

// grid (work rows, heads), 4 waves.  Keys go in chunks of kRowsThreads.  Per chunk: a thread per key j <= p computes the key's weight
// (its k row straight from the padded cache, 16 bytes per load where dqk and the layer's pointer allow, which changes no sum) into
// LDS; then thread (slice, d) = (tid / 32, tid % 32) adds the weighted values of keys slice, slice + 8, ... of the chunk for output
// dimension d (a jagged v row read by 32 adjacent lanes, four rows in flight).  The eight slices are added in a fixed tree at the
// end.  The order depends on p alone.
// LDS: thresholds [num_buckets] (64-bit), q [kRowsMaxHead], weights [kRowsThreads], the slices' sums [kRowsSlices][kRowsMaxHead].
constexpr int kRowsSlices = kRowsThreads / kRowsMaxHead;
static_assert(kRowsSlices == 8, "the fixed tree below adds eight slices");

__global__ __launch_bounds__(kRowsThreads) void hsturows_attn_kernel(RowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rows_smem[];
  const int64_t r = blockIdx.x;
  const int head = blockIdx.y;
  const Slot s = rows_slot(a, r);
  if (s.p < 0) return;   // uniform: before any barrier
  const int N = a.N, dqk = a.dqk, dv = a.dv, HV = a.H * dv, HQ = a.H * dqk;
  long long* thr = reinterpret_cast<long long*>(rows_smem);
  float* qs = reinterpret_cast<float*>(thr + ((a.num_buckets + 1) & ~1));
  float* wj = qs + kRowsMaxHead;
  float* part = wj + kRowsThreads;
  const int tid = threadIdx.x;
  const RowsLayer L = a.layers[a.blk];
  const bool biased = a.ts != nullptr && L.ts_w != nullptr;
  const int p = s.p, b = s.b;
  if (biased)
    for (int i = tid; i < a.num_buckets; i += kRowsThreads) thr[i] = a.thresholds[i];
  if (tid < kRowsMaxHead) qs[tid] = tid < dqk ? L.q[((int64_t)b * N + p) * HQ + head * dqk + tid] : 0.0f;
  __syncthreads();
  float qv[kRowsMaxHead];
#pragma unroll
  for (int d = 0; d < kRowsMaxHead; ++d) qv[d] = qs[d];
  const float inv_n = 1.0f / (float)N;
  const long long tq = biased ? a.ts[(int64_t)b * N + (p + 1 < N ? p + 1 : N - 1)] : 0;
  const long long off = s.row - p;
  const bool k4 = (dqk & 3) == 0 && (reinterpret_cast<uintptr_t>(L.k) & 15) == 0;   // uniform; every k row of a head is then 16-byte aligned
  const int d = tid & (kRowsMaxHead - 1), slice = tid / kRowsMaxHead;
  float acc = 0.0f;
  for (int j0 = 0; j0 <= p; j0 += kRowsThreads) {
    const int j = j0 + tid;
    float w = 0.0f;
    if (j <= p) {
      const float* kr = L.k + ((int64_t)b * N + j) * HQ + head * dqk;
      float sc = 0.0f;
      if (k4) {
#pragma unroll
        for (int e = 0; e < kRowsMaxHead; e += 4) {
          if (e < dqk) {
            const float4 k = *reinterpret_cast<const float4*>(kr + e);
            sc = __builtin_fmaf(qv[e], k.x, sc);
            sc = __builtin_fmaf(qv[e + 1], k.y, sc);
            sc = __builtin_fmaf(qv[e + 2], k.z, sc);
            sc = __builtin_fmaf(qv[e + 3], k.w, sc);
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < kRowsMaxHead; ++e)
          if (e < dqk) sc = __builtin_fmaf(qv[e], kr[e], sc);
      }
      if (biased) {
        long long dt = tq - a.ts[(int64_t)b * N + j];
        if (dt < 0) dt = -dt;
        int lo = 0, hi = a.num_buckets;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (thr[mid] <= dt) lo = mid + 1; else hi = mid;
        }
        sc += L.pos_w[N - 1 + j - p] + L.ts_w[lo];
      }
      w = silu_fast(sc) * inv_n;
    }
    wj[tid] = w;
    __syncthreads();
    const int n = p + 1 - j0 < kRowsThreads ? p + 1 - j0 : kRowsThreads;   // keys of this chunk
    if (d < dv) {
      const float* vb = L.v + (off + j0) * HV + head * dv + d;
      for (int i = slice; i < n; i += 4 * kRowsSlices) {
        float vv[4], ww[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int iu = i + u * kRowsSlices;
          vv[u] = iu < n ? vb[(int64_t)iu * HV] : 0.0f;
          ww[u] = iu < n ? wj[iu] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (i + u * kRowsSlices < n) acc = __builtin_fmaf(ww[u], vv[u], acc);
      }
    }
    __syncthreads();
  }
  part[slice * kRowsMaxHead + d] = acc;
  __syncthreads();
  if (tid < dv) {
    const float* c = part + tid;
    const float o = ((c[0] + c[kRowsMaxHead]) + (c[2 * kRowsMaxHead] + c[3 * kRowsMaxHead])) +
                    ((c[4 * kRowsMaxHead] + c[5 * kRowsMaxHead]) + (c[6 * kRowsMaxHead] + c[7 * kRowsMaxHead]));
    a.att[r * HV + head * dv + tid] = o;
  }
}

// the postprocessor of sequence b (one wave): normalize_row, as the prefill's rows_normalize_kernel, on the last layer's outputs row
// at len - 1; NaN for a sequence left alone
__global__ __launch_bounds__(64) void hsturows_post_kernel(RowsArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, D = a.D;
  float* o = a.out + (int64_t)b * D;
  const long long off = a.seq_off[b];
  if (off < 0) {
    for (int k = lane; k < D; k += 64) o[k] = __builtin_nanf("");
    return;
  }
  normalize_row(a.layers[a.n_blocks - 1].outputs + (off + a.lengths[b] - 1) * D, D, a.mode, a.eps, o, lane);
}

template <int MODE>
int launch_gemm(const RowsArgs& a, int K, int n_cols, hipStream_t stream) {
  static DynLdsOnce once;
  if (ensure_dyn_lds(once, reinterpret_cast<const void*>(&hsturows_gemm_kernel<MODE>), (int)rows_lds_bytes(kRowsMaxDim)) != kOk) return kErrLaunch;
  const dim3 grid((n_cols + kRowsCols - 1) / kRowsCols, (unsigned)((a.R + kRowsTile - 1) / kRowsTile));
  hipLaunchKernelGGL((hsturows_gemm_kernel<MODE>), grid, dim3(kRowsThreads), rows_lds_bytes(K), stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace

bool hstu_decode_rows_supported(int N, int D, int H, int dqk, int dv, int num_buckets) {
  if (N < 1 || D < 1 || D > kRowsMaxDim || H < 1 || dqk < 1 || dqk > kRowsMaxHead || dv < 1 || dv > kRowsMaxHead) return false;
  if (num_buckets < 0 || num_buckets > kRowsMaxBuckets) return false;
  return (int64_t)H * dv <= kRowsMaxDim && H <= kRowsMaxGridY;
}

// the sequence table (64-bit offsets, then 32-bit counts) in front of the work rows; one float of slack to align the table
int64_t hstu_decode_rows_workspace_floats(int64_t R, int B, int D, int H, int dv) {
  return 2 + 3 * (int64_t)B + (B & 1) + R * ((int64_t)D + 2 * (int64_t)H * dv);
}

int hstu_decode_rows(const float* emb, const int64_t* ids, const int64_t* positions, const int64_t* counts, int M, const int64_t* lengths,
                     const int64_t* ts, const int64_t* thresholds, const float* pos_emb, const void* layers, int n_blocks, int B, int N,
                     int64_t cache_rows, int D, int H, int dqk, int dv, int num_buckets, int act, int mode, float eps, float* work, float* out,
                     hipStream_t stream) {
  if (B == 0) return kOk;
  if (!hstu_decode_rows_supported(N, D, H, dqk, dv, num_buckets)) { set_error("hstu_decode_rows: geometry not supported"); return kErrUnsupported; }
  if (M < 1 || (int64_t)B * M > kRowsMaxSlots) { set_error("hstu_decode_rows: batch %d x max_rows %d work rows", B, M); return kErrUnsupported; }
  RowsArgs a{};
  a.emb = emb; a.ids = ids; a.positions = positions; a.counts = counts; a.lengths = lengths; a.ts = ts; a.thresholds = thresholds;
  a.pos_emb = pos_emb; a.layers = static_cast<const RowsLayer*>(layers); a.n_blocks = n_blocks;
  a.B = B; a.N = N; a.M = M; a.R = (int64_t)B * M; a.cache_rows = cache_rows; a.D = D; a.H = H; a.dqk = dqk; a.dv = dv;
  a.num_buckets = ts ? num_buckets : 0; a.act = act; a.mode = mode; a.eps = eps; a.out = out;
  const int HV = H * dv;
  unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(work) + 7) & ~(uintptr_t)7);
  a.seq_off = reinterpret_cast<long long*>(base);
  a.seq_m = reinterpret_cast<int*>(a.seq_off + B);
  a.x = reinterpret_cast<float*>(a.seq_m + B + (B & 1));
  a.u = a.x + a.R * D;
  a.att = a.u + a.R * HV;
  hipLaunchKernelGGL(hsturows_scan_kernel, dim3(1), dim3(kRowsScanThreads), (kRowsScanThreads / 64) * (sizeof(long long) + sizeof(int)), stream, a);
  if (hipGetLastError() != hipSuccess) return kErrLaunch;
  const size_t attn_lds = sizeof(long long) * ((a.num_buckets + 1) & ~1) + sizeof(float) * (kRowsMaxHead + kRowsThreads + kRowsSlices * kRowsMaxHead);
  for (int i = 0; i < n_blocks; ++i) {
    a.blk = i;
    a.first = i == 0;
    int r = launch_gemm<0>(a, D, 2 * H * (dqk + dv), stream);
    if (r != kOk) return r;
    hipLaunchKernelGGL(hsturows_attn_kernel, dim3((unsigned)a.R, H), dim3(kRowsThreads), attn_lds, stream, a);
    if (hipGetLastError() != hipSuccess) return kErrLaunch;
    if ((r = launch_gemm<1>(a, HV, D, stream)) != kOk) return r;
  }
  hipLaunchKernelGGL(hsturows_post_kernel, dim3(B), dim3(64), 0, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace mol
