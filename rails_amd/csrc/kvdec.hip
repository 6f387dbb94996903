// SASRec cached incremental decoding (rails_sasrec_decode[_rows]): the last m_b rows of every sequence, p = lengths[b] - m_b ..
// lengths[b] - 1 (one row, m_b = 1, in rails_sasrec_decode), re-encoded through every block against the key / value rows below them
// held in a per-block cache (batch, seq_len, dim), which gains those rows in place.
//
// A WORK ROW is a (sequence, position) pair in one of B * M fixed slots (M = max_new): slot r = b * M + t is active iff t < m_b and
// stands for position p_r = lengths[b] - m_b + t (dec_row).  m_b = counts[b] (M when there is no count array), clamped on the device
// into [1, min(M, lengths[b])] like the lengths themselves.  An inactive slot stages zeros and writes nothing; its attention workgroup
// exits at once.  All new k / v rows of a block are written by the launch in front of that block's attention launch, and each row's own
// key limit j <= p_r keeps the new rows causal among themselves.  A row's arithmetic does not depend on its slot, so one step over m
// rows is bit for bit m single-row steps.
//
// One body per kernel, two instances of each.  Over KvDecArgs: the single-row step, one row per sequence (work row b is sequence b
// at lengths[b] - 1; attention grid (heads, sequences)), which keeps the argument block and the launch grids it had before the slot
// scheme and compiles to the code it had then (profiles/decode_one_body_isa.txt).  Over KvSlotArgs: the slot scheme, used when
// max_new > 1 (or the batch is beyond the 65 535 of the single-row attention grid's y); each row tile first resolves its 32 slots
// into an LDS table (sequence, position or -1), once, which staging, stores and epilogue read.  The instances differ in where a
// tile row finds its sequence and position (seq_of / pos_of, `if constexpr (SLOTS)`) and in nothing else; each body stands in its
// __global__ kernel with the argument block by value, since a shared device function that takes the block by reference is what
// costs the single-row step 2-3 %.
//
// SASRec's attention is strictly causal and its only other mask is the per-row id mask, so row p of every block depends on rows
// 0..p of that block's input alone: the cached K / V of the rows below p are exactly what a full encode would compute there, and
// the step equals encode() of the updated sequence up to fp32 summation order.  One block, for the row alone (sasrec.hip's header):
//   Q = LN(x, 1e-8);  q = Q W_q^T + b_q;  [k | v] = x W_kv^T + b_kv  -> cache row p
//   a = softmax(q k_j^T / sqrt(hd)) v_j over j = 0..p per head (k_p / v_p: the fresh row just written)
//   y = Q + a W_o^T + b_o;  z = LN(y, 1e-8);  x = (act(z W_1^T + b_1) W_2^T + b_2 + z) * (id != 0)
//
// Route: per block five launches over ALL rows of the batch, each row GEMM splitting its output columns across
// workgroups (64 columns each) so that a weight is read once per 32 rows, never once per sequence:
//   kv_rows_kernel<0>  LN1 + the in-projection (block 0: the embedding / position preprocessor first); q to the work rows, k / v
//                      into cache row p; column tile 0 also stores Q (and block 0's x)
//   kv_attn_kernel     one workgroup per (work row, head): scores of keys 0..p, softmax, the weighted sum of values
//   kv_rows_kernel<1>  y = Q + a W_o^T + b_o
//   kv_rows_kernel<2>  z = LN2(y) in LDS, h = act(z W_1^T + b_1); column tile 0 stores z
//   kv_rows_kernel<3>  x = (h W_2^T + b_2 + z) * (id != 0)
// then kvdec_post_kernel / kvslot_post_kernel: the LayerNorm / l2-norm postprocessor (normalize_row) of the last block's row of
// every sequence.  5 * n_blocks + 1 launches per step.  The LayerNorm statistics of a staged row are encoder_device.h's
// row_ln_stats, shared with hstu_rows.hip; the staging loop is written out in both files.
//
// Numerics as sasrec.hip (-ffp-contract=off, explicit fmaf): a dot product keeps four partial sums (k mod 4) and adds them in a
// fixed tree; the softmax pre-scales q by 1 / sqrt(hd) and runs on v_exp_f32 of log2-scaled scores.  No grid-wide barrier.
#include <hip/hip_runtime.h>
#include <math.h>

#include "encoder_device.h"
#include "mol_kernels.h"
#include "mol_layout.h"

namespace mol {

constexpr float kDecLnEps = 1e-8f;     // F.layer_norm(..., eps=1e-8) inside every block
constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / 64;
constexpr int kDecCols = 64;           // output columns per workgroup: one per lane
constexpr int kDecRows = 32;           // batch rows per workgroup
constexpr int kDecRowsPerWave = kDecRows / kDecWaves;
constexpr int kDecMaxSeq = 2048;       // LDS score buffer of the attention kernel
constexpr int kDecMaxDim = 1024;       // D and F: the staged A tile is kDecRows x K floats (128 KiB at the limit)
constexpr int kDecKBatch = 64;         // weights of a lane's row loaded ahead of their FMAs (16 float4)
constexpr int kDecVBatch = 8;          // value rows in flight per lane in the attention's weighted sum
constexpr int kDecMaxGridY = 65535;
// work rows of one step: the row kernels put 32-slot tiles on grid.y; the slot attention kernel has its rows on grid.x (heads, at
// most kDecMaxDim, on grid.y), where HIP wants grid.x * block size below 2^32
constexpr int64_t kDecMaxSlots = RAILS_SASREC_DECODE_MAX_ROWS;
static_assert(kDecRows == kTileRows && kDecThreads == kTileThreads, "the staging loop is written out here and in hstu_rows.hip for one geometry");
static_assert(kDecMaxSlots == (int64_t)kDecMaxGridY * kDecRows, "rails_amd.h states the grid limit");
static_assert(kDecMaxSlots * kDecThreads < (1LL << 32) && kDecMaxDim <= kDecMaxGridY, "the slot attention grid (work rows, heads)");

struct KvDecArgs {                     // the single-row step's block: work row b is sequence b at lengths[b] - 1
  const float* emb; const int64_t* ids; const int64_t* lengths; const float* pos_emb;   // (B, N, D), (B, N), (B), (>= N, D)
  int B, N, D, H, F, act, first;
  const float* w; const float* bias;   // this launch's weight (n_cols, K) and bias (n_cols)
  float* kc; float* vc;                // this block's cache, (B, N, D)
  float* x; float* qn; float* q; float* att; float* y; float* z; float* h;   // work rows: (B, D) each, h (B, F)
};

struct KvSlotArgs : KvDecArgs {        // the slot scheme's additions, behind the single-row step's block
  const int64_t* counts;               // (B) new rows per sequence, or null: M each
  int M, R;                            // R = B * M work-row slots
};

__device__ __forceinline__ int dec_pos(const int64_t* lengths, int b, int N) {
  const int64_t len = lengths[b];
  return len < 1 ? 0 : len > N ? N - 1 : (int)len - 1;   // the host validates or clamps; never a row outside the cache
}

struct DecRow { int b, p; bool active; };   // the sequence and position of a work-row slot

__device__ __forceinline__ DecRow dec_row(const KvSlotArgs& a, int r) {
  const int b = r / a.M, t = r - b * a.M;
  const int len = dec_pos(a.lengths, b, a.N) + 1;
  const int cap = a.M < len ? a.M : len;
  const int64_t c = a.counts ? a.counts[b] : (int64_t)a.M;
  const int m = c < 1 ? 1 : c > cap ? cap : (int)c;   // the same policy as dec_pos
  return DecRow{b, len - m + t, t < m};
}

// C[r][col] = sum_k A[r][k] W[col][k] for the rows of a tile and one column per lane.  MODE: 0 in-projection (A = x; the q columns
// read (x - mean) * rstd, the k / v columns x itself), 1 out-projection (A = a), 2 FFN 1 (A = LN2(y)), 3 FFN 2 (A = h).
// grid (column tiles, row tiles); LDS: A [kDecRows][ks] (ks = K rounded up to 4, zero-padded), then mean / rstd [kDecRows], then
// (SLOTS) the tile's slot table: sequence and position [kDecRows] each, position -1 for an inactive slot.
// The body stands in the kernel, its argument block by value: behind a reference to the block the single-row instances compile to
// other code.  seq_of / pos_of are all that tells a single-row tile row from a slot.
template <int MODE, bool V4, bool SLOTS, class Args>
__global__ __launch_bounds__(kDecThreads) void kv_rows_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const int D = a.D, N = a.N;
  const int K = MODE == 3 ? a.F : D;
  const int n_cols = MODE == 0 ? 3 * D : MODE == 2 ? a.F : D;
  const int ks = (K + 3) & ~3;
  float* As = dsm;
  float* mean_s = As + kDecRows * ks;
  float* rstd_s = mean_s + kDecRows;
  [[maybe_unused]] int* slot_b = reinterpret_cast<int*>(rstd_s + kDecRows);
  [[maybe_unused]] int* slot_p = slot_b + kDecRows;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r0 = blockIdx.y * kDecRows;
  int rows;
  if constexpr (SLOTS) rows = a.R;
  else rows = a.B;
  const int nr = rows - r0 < kDecRows ? rows - r0 : kDecRows;
  const float emb_scale = sqrtf((float)D);
  if constexpr (SLOTS) {
    if (tid < kDecRows) {   // the tile's slots, resolved once
      int b = -1, p = -1;
      if (tid < nr) {
        const DecRow w = dec_row(a, r0 + tid);
        b = w.b;
        p = w.active ? w.p : -1;
      }
      slot_b[tid] = b;
      slot_p[tid] = p;
    }
    __syncthreads();
  }
  // of tile row r < nr, work row w = r0 + r: does it stand for a row at all, and for which sequence and position (of a live row)
  auto live = [&](int r) -> bool { if constexpr (SLOTS) return slot_p[r] >= 0; else return true; };
  auto seq_of = [&](int r, int w) -> int { if constexpr (SLOTS) return slot_b[r]; else return w; };
  auto pos_of = [&](int r, int w) -> int { if constexpr (SLOTS) return slot_p[r]; else return dec_pos(a.lengths, w, N); };

  // ---- stage the A rows (zeros past K, past the last row and in inactive slots)
  auto load = [&](int i) -> float {
    const int r = i / ks, k = i - r * ks;
    if (r >= nr || k >= K) return 0.0f;
    if (!live(r)) return 0.0f;
    const int b = r0 + r;
    if (MODE == 0) {
      if (!a.first) return a.x[(int64_t)b * D + k];
      const int s = seq_of(r, b), p = pos_of(r, b);   // x = (emb * sqrt(D) + pos_emb[p]) * (id != 0), as rails_hstu_preprocess
      return a.ids[(int64_t)s * N + p] != 0 ? a.emb[((int64_t)s * N + p) * D + k] * emb_scale + a.pos_emb[(int64_t)p * D + k] : 0.0f;
    }
    if (MODE == 1) return a.att[(int64_t)b * D + k];
    if (MODE == 2) return a.y[(int64_t)b * D + k];
    return a.h[(int64_t)b * a.F + k];
  };
  // kStageBatch global loads in flight per thread, then their stores.  Written out here and in hstu_rows.hip's hsturows_gemm_kernel:
  // behind any shared helper the single-row instances <1> and <3> stop being the code they were
  for (int i0 = tid; i0 < kDecRows * ks; i0 += kStageBatch * kDecThreads) {
    float v[kStageBatch];
#pragma unroll
    for (int u = 0; u < kStageBatch; ++u) v[u] = i0 + u * kDecThreads < kDecRows * ks ? load(i0 + u * kDecThreads) : 0.0f;
#pragma unroll
    for (int u = 0; u < kStageBatch; ++u)
      if (i0 + u * kDecThreads < kDecRows * ks) As[i0 + u * kDecThreads] = v[u];
  }
  __syncthreads();
  if (MODE == 0 || MODE == 2) {   // LayerNorm statistics of each row, a wave per row
    for (int r = wave; r < kDecRows; r += kDecWaves) row_ln_stats(As + r * ks, K, kDecLnEps, mean_s + r, rstd_s + r, lane);
    __syncthreads();
  }
  if (MODE == 2) {   // z = LN(y) in place; column tile 0 keeps z for the FFN 2 residual
    for (int i = tid; i < kDecRows * ks; i += kDecThreads) {
      const int r = i / ks, k = i - r * ks;
      if (k < K) {
        const float zv = (As[i] - mean_s[r]) * rstd_s[r];
        As[i] = zv;
        if (blockIdx.x == 0 && r < nr && live(r)) a.z[(int64_t)(r0 + r) * D + k] = zv;
      }
    }
    __syncthreads();
  }
  if (MODE == 0 && blockIdx.x == 0) {   // Q for the out-projection residual (and block 0's x, which no later kernel recomputes)
    for (int i = tid; i < nr * ks; i += kDecThreads) {
      const int r = i / ks, k = i - r * ks;
      if (k < K && live(r)) {
        a.qn[(int64_t)(r0 + r) * D + k] = (As[i] - mean_s[r]) * rstd_s[r];
        if (a.first) a.x[(int64_t)(r0 + r) * D + k] = As[i];
      }
    }
  }

  const int col = blockIdx.x * kDecCols + lane;
  if (col >= n_cols) return;   // no barrier follows
  const int rw = wave * kDecRowsPerWave;   // this wave's rows of the tile
  if (rw >= nr) return;
  const float* wr = a.w + (int64_t)col * K;
  float mu[kDecRowsPerWave], sc[kDecRowsPerWave];   // in-projection: the q columns normalise x on the fly, k / v take it as is
#pragma unroll
  for (int j = 0; j < kDecRowsPerWave; ++j) {
    const bool qcol = MODE == 0 && col < D;
    mu[j] = qcol ? mean_s[rw + j] : 0.0f;
    sc[j] = qcol ? rstd_s[rw + j] : 1.0f;
  }
  float acc[kDecRowsPerWave][4];
#pragma unroll
  for (int j = 0; j < kDecRowsPerWave; ++j) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0f;
  for (int k0 = 0; k0 < K; k0 += kDecKBatch) {   // kDecKBatch weights of this lane's row in flight, then their FMAs
    float4 wv[kDecKBatch / 4];
#pragma unroll
    for (int u = 0; u < kDecKBatch / 4; ++u) {
      const int k = k0 + 4 * u;
      if (V4) {
        wv[u] = k < K ? *reinterpret_cast<const float4*>(wr + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      } else {
        wv[u].x = k < K ? wr[k] : 0.0f;
        wv[u].y = k + 1 < K ? wr[k + 1] : 0.0f;
        wv[u].z = k + 2 < K ? wr[k + 2] : 0.0f;
        wv[u].w = k + 3 < K ? wr[k + 3] : 0.0f;
      }
    }
#pragma unroll
    for (int u = 0; u < kDecKBatch / 4; ++u) {
      const int k = k0 + 4 * u;
      if (k >= K) break;   // uniform; the A rows are zero-padded to a multiple of 4 only
      const float4 w4 = wv[u];
#pragma unroll
      for (int j = 0; j < kDecRowsPerWave; ++j) {
        float4 x4 = *reinterpret_cast<const float4*>(As + (rw + j) * ks + k);   // the same address in every lane: a broadcast
        if (MODE == 0) {
          x4.x = (x4.x - mu[j]) * sc[j];   // (x - 0) * 1 == x exactly on the k / v columns
          x4.y = (x4.y - mu[j]) * sc[j];
          x4.z = (x4.z - mu[j]) * sc[j];
          x4.w = (x4.w - mu[j]) * sc[j];
        }
        acc[j][0] = __builtin_fmaf(x4.x, w4.x, acc[j][0]);
        acc[j][1] = __builtin_fmaf(x4.y, w4.y, acc[j][1]);
        acc[j][2] = __builtin_fmaf(x4.z, w4.z, acc[j][2]);
        acc[j][3] = __builtin_fmaf(x4.w, w4.w, acc[j][3]);
      }
    }
  }
  const float bc = a.bias[col];
#pragma unroll
  for (int j = 0; j < kDecRowsPerWave; ++j) {
    if (rw + j >= nr) break;
    if (!live(rw + j)) continue;   // an inactive slot writes nothing, neither work rows nor the cache
    const int b = r0 + rw + j;
    const float v = ((acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3])) + bc;
    if (MODE == 0) {
      if (col < D) {
        a.q[(int64_t)b * D + col] = v;
      } else {
        const int64_t crow = ((int64_t)seq_of(rw + j, b) * N + pos_of(rw + j, b)) * D;
        if (col < 2 * D) a.kc[crow + col - D] = v;
        else a.vc[crow + col - 2 * D] = v;
      }
    } else if (MODE == 1) {
      a.y[(int64_t)b * D + col] = v + a.qn[(int64_t)b * D + col];
    } else if (MODE == 2) {
      a.h[(int64_t)b * a.F + col] = ffn_act(v, a.act);
    } else {
      const float o = v + a.z[(int64_t)b * D + col];
      const int p = pos_of(rw + j, b);
      a.x[(int64_t)b * D + col] = a.ids[(int64_t)seq_of(rw + j, b) * N + p] != 0 ? o : 0.0f;
    }
  }
}

// One workgroup (4 waves) per (work row `row`, head): sequence b at position p.  Grid (heads, sequences) for the single-row step,
// (work rows, heads) for the slot scheme, where an inactive slot's workgroup exits at once.  Scores: a thread per key j <= p (the key
// row straight from the cache, HD-unrolled with four partial sums), kept in LDS; the block's maximum and denominator by wave sums;
// the output: a wave per key residue mod 4, a lane per output dimension (value rows read coalesced, 8 in flight), two partial sums
// per lane, the four waves summed in a fixed order.  The body stands in the kernel, as in kv_rows_kernel.
template <int HD, bool SLOTS, class Args>
__global__ __launch_bounds__(kDecThreads) void kv_attn_kernel(Args a) {
  __shared__ float sc[kDecMaxSeq];
  __shared__ float qs[HD];
  __shared__ float red[kDecWaves];
  __shared__ float part[kDecWaves][HD];
  const int head = SLOTS ? blockIdx.y : blockIdx.x, row = SLOTS ? blockIdx.x : blockIdx.y;
  const int N = a.N, D = a.D, hd = D / a.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b = row, p;
  if constexpr (SLOTS) {
    const DecRow w = dec_row(a, row);
    if (!w.active) return;   // uniform: before any barrier
    b = w.b;
    p = w.p;
  } else {
    p = dec_pos(a.lengths, b, N);
  }
  const float scale = 1.0f / sqrtf((float)hd);
  if (tid < HD) qs[tid] = tid < hd ? a.q[(int64_t)row * D + head * hd + tid] * scale : 0.0f;
  __syncthreads();
  const float* kbase = a.kc + (int64_t)b * N * D + head * hd;
  const float* vbase = a.vc + (int64_t)b * N * D + head * hd;
  float mx = -INFINITY;
  for (int j = tid; j <= p; j += kDecThreads) {
    const float* kr = kbase + (int64_t)j * D;
    float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int d = 0; d < HD; ++d)
      if (d < hd) s4[d & 3] = __builtin_fmaf(qs[d], kr[d], s4[d & 3]);
    const float s = ((s4[0] + s4[1]) + (s4[2] + s4[3])) * kLog2e;
    sc[j] = s;
    mx = fmaxf(mx, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));   // finite: key 0 exists
  float l = 0.0f;
  for (int j = tid; j <= p; j += kDecThreads) {
    const float e = __builtin_amdgcn_exp2f(sc[j] - mx);
    sc[j] = e;
    l += e;
  }
  l = wave_sum(l);
  __syncthreads();   // every red[] read above, every sc[] weight written
  if (lane == 0) red[wave] = l;
  __syncthreads();
  const float denom = (red[0] + red[1]) + (red[2] + red[3]);
  float o0 = 0.0f, o1 = 0.0f;
  if (lane < hd) {
    for (int j0 = wave; j0 <= p; j0 += kDecVBatch * kDecWaves) {
      float vv[kDecVBatch];
#pragma unroll
      for (int u = 0; u < kDecVBatch; ++u) {
        const int j = j0 + u * kDecWaves;
        vv[u] = j <= p ? vbase[(int64_t)j * D + lane] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kDecVBatch; ++u) {
        const int j = j0 + u * kDecWaves;
        if (j <= p) {
          if (u & 1) o1 = __builtin_fmaf(sc[j], vv[u], o1);
          else o0 = __builtin_fmaf(sc[j], vv[u], o0);
        }
      }
    }
  }
  if (lane < HD) part[wave][lane] = o0 + o1;
  __syncthreads();
  if (tid < hd) {
    const float o = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    a.att[(int64_t)row * D + head * hd + tid] = o / denom;
  }
}

// the postprocessor (normalize_row, one wave) of sequence b's last new row: work row b of the single-row step ...
__global__ __launch_bounds__(64) void kvdec_post_kernel(const float* x, int D, int mode, float eps, float* out) {
  const int b = blockIdx.x;
  normalize_row(x + (int64_t)b * D, D, mode, eps, out + (int64_t)b * D, threadIdx.x);
}

// ... and slot b * M + m_b - 1 of the slot scheme
__global__ __launch_bounds__(64) void kvslot_post_kernel(KvSlotArgs a, int mode, float eps, float* out) {
  const int b = blockIdx.x, D = a.D;
  const int last = dec_pos(a.lengths, b, a.N) - dec_row(a, b * a.M).p;   // m_b - 1
  normalize_row(a.x + ((int64_t)b * a.M + last) * D, D, mode, eps, out + (int64_t)b * D, threadIdx.x);
}

static int work_rows(const KvDecArgs& a) { return a.B; }
static int work_rows(const KvSlotArgs& a) { return a.R; }

static size_t kvdec_rows_lds(int K, bool slots) {
  return sizeof(float) * ((size_t)kDecRows * ((K + 3) & ~3) + (slots ? 4 : 2) * kDecRows);
}

bool sasrec_decode_supported(int N, int D, int H, int F) {
  if (N < 1 || N > kDecMaxSeq || D < 1 || D > kDecMaxDim || F < 1 || F > kDecMaxDim || H < 1 || D % H != 0) return false;
  return D / H <= 64;
}

int64_t sasrec_decode_workspace_floats(int B, int D, int F) { return (int64_t)B * (6 * (int64_t)D + F); }

template <int MODE, bool SLOTS, class Args>
static int launch_rows(const Args& a, int K, int n_cols, hipStream_t stream) {
  const bool v4 = K % 4 == 0;
  void (*const fn)(Args) = v4 ? &kv_rows_kernel<MODE, true, SLOTS, Args> : &kv_rows_kernel<MODE, false, SLOTS, Args>;
  static DynLdsOnce once[2];
  if (ensure_dyn_lds(once[v4 ? 1 : 0], reinterpret_cast<const void*>(fn), (int)kvdec_rows_lds(kDecMaxDim, SLOTS)) != kOk) return kErrLaunch;
  const dim3 grid((n_cols + kDecCols - 1) / kDecCols, (work_rows(a) + kDecRows - 1) / kDecRows);
  hipLaunchKernelGGL(fn, grid, dim3(kDecThreads), kvdec_rows_lds(K, SLOTS), stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// the 5 * n_blocks + 1 launches of one step
template <bool SLOTS, class Args>
static int decode_blocks(Args& a, const rails_sasrec_decode_layer* layers, int n_blocks, int mode, float eps, float* out, hipStream_t stream) {
  const int D = a.D, H = a.H, F = a.F, hd = D / H;
  for (int i = 0; i < n_blocks; ++i) {
    const rails_sasrec_decode_layer& L = layers[i];
    a.first = i == 0;
    a.kc = L.k; a.vc = L.v;
    a.w = L.in_proj_weight; a.bias = L.in_proj_bias;
    int r = launch_rows<0, SLOTS>(a, D, 3 * D, stream);
    if (r != kOk) return r;
    const dim3 agrid = SLOTS ? dim3(work_rows(a), H) : dim3(H, work_rows(a));
    if (hd <= 16) hipLaunchKernelGGL((kv_attn_kernel<16, SLOTS, Args>), agrid, dim3(kDecThreads), 0, stream, a);
    else if (hd <= 32) hipLaunchKernelGGL((kv_attn_kernel<32, SLOTS, Args>), agrid, dim3(kDecThreads), 0, stream, a);
    else hipLaunchKernelGGL((kv_attn_kernel<64, SLOTS, Args>), agrid, dim3(kDecThreads), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return kErrLaunch;
    a.w = L.out_proj_weight; a.bias = L.out_proj_bias;
    if ((r = launch_rows<1, SLOTS>(a, D, D, stream)) != kOk) return r;
    a.w = L.conv1_weight; a.bias = L.conv1_bias;
    if ((r = launch_rows<2, SLOTS>(a, D, F, stream)) != kOk) return r;
    a.w = L.conv2_weight; a.bias = L.conv2_bias;
    if ((r = launch_rows<3, SLOTS>(a, F, D, stream)) != kOk) return r;
  }
  if constexpr (SLOTS) hipLaunchKernelGGL(kvslot_post_kernel, dim3(a.B), dim3(64), 0, stream, a, mode, eps, out);
  else hipLaunchKernelGGL(kvdec_post_kernel, dim3(a.B), dim3(64), 0, stream, static_cast<const float*>(a.x), D, mode, eps, out);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int sasrec_decode(const float* emb, const int64_t* ids, const int64_t* lengths, const int64_t* counts, int M, const float* pos_emb,
                  const rails_sasrec_decode_layer* layers, int n_blocks, int B, int N, int D, int H, int F, int act, int mode, float eps,
                  float* work, float* out, hipStream_t stream) {
  if (B == 0) return kOk;
  if (!sasrec_decode_supported(N, D, H, F)) { set_error("sasrec_decode: geometry not supported"); return kErrUnsupported; }
  if (M < 1 || M > N) { set_error("sasrec_decode: max_new %d outside [1, seq_len %d]", M, N); return kErrUnsupported; }
  if ((int64_t)B * M > kDecMaxSlots) {
    set_error("sasrec_decode: batch %d x max_new %d = %lld work rows, more than the %lld of one launch grid", B, M, (long long)B * M,
              (long long)kDecMaxSlots);
    return kErrUnsupported;
  }
  KvSlotArgs a{};
  a.emb = emb; a.ids = ids; a.lengths = lengths; a.pos_emb = pos_emb;
  a.B = B; a.N = N; a.D = D; a.H = H; a.F = F; a.act = act;
  a.counts = counts; a.M = M; a.R = B * M;
  const int64_t bd = (int64_t)a.R * D;
  a.x = work; a.qn = work + bd; a.q = work + 2 * bd; a.att = work + 3 * bd; a.y = work + 4 * bd; a.z = work + 5 * bd; a.h = work + 6 * bd;
  // one row per sequence: the single-row kernels (a count array can only say 1); their attention grid has the batch on y
  if (M == 1 && B <= kDecMaxGridY) return decode_blocks<false>(static_cast<KvDecArgs&>(a), layers, n_blocks, mode, eps, out, stream);
  return decode_blocks<true>(a, layers, n_blocks, mode, eps, out, stream);
}

}  // namespace mol
