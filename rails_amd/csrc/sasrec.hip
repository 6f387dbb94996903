// SASRec query encoder, eval path: causal softmax multi-head attention and a fused single-launch encoder for short sequences.
//
// Reference: modeling/sequential/sasrec.py -- SASRec._run_one_layer (:190-215) with torch.nn.MultiheadAttention (batch_first,
// bool causal attn_mask, dropout off) and StandardAttentionFF (:42-76); the preprocessor input_features_preprocessors.py:75-92
// (the mask is `ids != 0` only); the postprocessors output_postprocessors.py:38-85.  One block, with m = (ids != 0):
//   Q = LN(x, 1e-8);  [q | k | v] = [Q | x | x] W_in^T + b_in       (query from Q, key / value from the UN-normalised x)
//   a = softmax_causal(q k^T / sqrt(hd)) v per head                  (keys j <= i, ALL of them: the id mask hides no key)
//   y = Q + a W_o^T + b_o;  z = LN(y, 1e-8);  x = (act(z W_1^T + b_1) W_2^T + b_2 + z) * m
// The per-layer route chains rails_rows_layer_norm, rails_gemm_f32 / rails_gemm_f32_id_masked and sasrec_attention_kernel;
// sasrec_fused_kernel runs all of it in one launch.
//
// Kernels (fp32 throughout):
//   sasrec_attention_kernel  one wave per (64 queries, head, sequence), one query per lane: q and the output row in registers,
//                            key / value rows staged in LDS 64 at a time (every lane reads the same row: broadcasts), an online
//                            softmax over groups of 16 keys (one rescale per group).
//   sasrec_fused_kernel      the whole encoder for seq_len <= 64, dim <= 128, ffn_dim <= 128: one workgroup per sequence, the
//                            residual stream and every activation in LDS (<= 133 KiB), all blocks back to back.
#include <hip/hip_runtime.h>
#include <math.h>

#include "encoder_device.h"
#include "mol_kernels.h"
#include "mol_layout.h"

namespace mol {

typedef float sf32x16 __attribute__((ext_vector_type(16)));

constexpr float kBlockLnEps = 1e-8f;   // F.layer_norm(..., eps=1e-8) inside every block (sasrec.py:195-212)
constexpr int kKeyGroup = 16;          // keys per online-softmax rescale

// The online softmax of ONE query over a run of keys held in LDS (rows of `ks` floats; K at Ks, V at Vs).  q is pre-scaled by
// 1 / sqrt(hd) (torch scales q before q k^T); keys j0 + t for t < n_keys, of which those with j0 + t > qi are masked out.
// State: running maximum m (log2-scaled), denominator l, unnormalised output o.  exp via v_exp_f32 (2^x, ~1 ulp) of a
// non-positive argument.  Key groups that are entirely masked for this lane leave the state unchanged (p = 0, alpha = 1).
template <int HD>
__device__ __forceinline__ void softmax_keys(const float* Ks, const float* Vs, int ks, int j0, int n_keys, int qi, const float (&q)[HD],
                                             float (&o)[HD], float& m, float& l) {
  for (int t0 = 0; t0 < n_keys; t0 += kKeyGroup) {
    float s[kKeyGroup];
    float gm = -INFINITY;
#pragma unroll
    for (int u = 0; u < kKeyGroup; ++u) {
      const int t = t0 + u;
      const float* kr = Ks + (t < n_keys ? t : 0) * ks;
      float acc = 0.0f;
#pragma unroll
      for (int d = 0; d < HD; d += 4) {
        const float4 k4 = *reinterpret_cast<const float4*>(kr + d);
        acc = __builtin_fmaf(q[d], k4.x, acc);
        acc = __builtin_fmaf(q[d + 1], k4.y, acc);
        acc = __builtin_fmaf(q[d + 2], k4.z, acc);
        acc = __builtin_fmaf(q[d + 3], k4.w, acc);
      }
      // acc is q . k over hd dims: the lanes d >= hd of q are zero
      s[u] = (t < n_keys && j0 + t <= qi) ? acc * kLog2e : -INFINITY;
      gm = fmaxf(gm, s[u]);
    }
    const float mn = fmaxf(m, gm);                 // finite: the first group of every query holds key 0 <= qi
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    l *= alpha;
#pragma unroll
    for (int d = 0; d < HD; ++d) o[d] *= alpha;
#pragma unroll
    for (int u = 0; u < kKeyGroup; ++u) {
      const float p = __builtin_amdgcn_exp2f(s[u] - mn);   // 0 for masked keys
      l += p;
      const int t = t0 + u;
      const float* vr = Vs + (t < n_keys ? t : 0) * ks;
#pragma unroll
      for (int d = 0; d < HD; d += 4) {
        const float4 v4 = *reinterpret_cast<const float4*>(vr + d);
        o[d] = __builtin_fmaf(p, v4.x, o[d]);
        o[d + 1] = __builtin_fmaf(p, v4.y, o[d + 1]);
        o[d + 2] = __builtin_fmaf(p, v4.z, o[d + 2]);
        o[d + 3] = __builtin_fmaf(p, v4.w, o[d + 3]);
      }
    }
  }
}

struct SasAttnArgs {
  const float* qkv; int64_t ld;        // (B * N, ld) rows [q | k | v], each heads * hd wide
  int B, N, H, hd;
  float* out;                          // (B * N, heads * hd)
};

constexpr int kAttnTile = 64;          // queries per wave, and keys per LDS stage

// grid (query tiles of 64, heads, sequences), one wave.  LDS: K and V of 64 keys, rows HD floats (16-byte aligned, zero past hd).
template <int HD>
__global__ __launch_bounds__(64) void sasrec_attention_kernel(SasAttnArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[kAttnTile * HD], Vs[kAttnTile * HD];
  const int lane = threadIdx.x;
  const int qt = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int N = a.N, hd = a.hd, D = a.H * a.hd;
  const float* base = a.qkv + (int64_t)b * N * a.ld;
  const int qrow = qt * kAttnTile + lane;
  const int qi = qrow < N ? qrow : N - 1;          // clamped: lanes past N compute a valid row and store nothing
  const float scale = 1.0f / sqrtf((float)hd);
  float q[HD], o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) {
    const float v = base[(int64_t)qi * a.ld + head * hd + (d < hd ? d : 0)];
    q[d] = d < hd ? v * scale : 0.0f;
    o[d] = 0.0f;
  }
  float m = -INFINITY, l = 0.0f;
  const int last = (qt + 1) * kAttnTile < N ? (qt + 1) * kAttnTile : N;   // keys [0, last): the causal triangle of this tile
  for (int j0 = 0; j0 < last; j0 += kAttnTile) {
    const int nk = last - j0 < kAttnTile ? last - j0 : kAttnTile;
    __syncthreads();                                // the previous stage has been read by every lane
    for (int e = lane; e < kAttnTile * HD; e += 64) {
      const int r = e / HD, d = e - r * HD;
      float kv = 0.0f, vv = 0.0f;
      if (r < nk && d < hd) {
        const float* row = base + (int64_t)(j0 + r) * a.ld + head * hd + d;
        kv = row[D];
        vv = row[2 * D];
      }
      Ks[e] = kv;
      Vs[e] = vv;
    }
    __syncthreads();
    softmax_keys<HD>(Ks, Vs, HD, j0, nk, qi, q, o, m, l);
  }
  if (qrow >= N) return;
  const float inv = 1.0f / l;
  float* orow = a.out + ((int64_t)b * N + qrow) * D + head * hd;
#pragma unroll
  for (int d = 0; d < HD; ++d)
    if (d < hd) orow[d] = o[d] * inv;
}

int sasrec_attention(const float* qkv, int64_t ld, int B, int N, int H, int hd, float* out, hipStream_t stream) {
  if (B == 0 || N == 0) return kOk;
  if (hd < 1 || hd > 64) { set_error("sasrec_attention: head_dim = %d (supported: 1..64)", hd); return kErrUnsupported; }
  SasAttnArgs a{qkv, ld, B, N, H, hd, out};
  const dim3 grid((N + kAttnTile - 1) / kAttnTile, H, B);
  if (hd <= 16) hipLaunchKernelGGL(sasrec_attention_kernel<16>, grid, dim3(64), 0, stream, a);
  else if (hd <= 32) hipLaunchKernelGGL(sasrec_attention_kernel<32>, grid, dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(sasrec_attention_kernel<64>, grid, dim3(64), 0, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// ---------------------------------------------------------------------------------------------
// Fused encoder for short sequences.  One workgroup (4 waves) per sequence; LDS:
//   X  [64][D + 1]              residual stream; after the projections y = Q + a W_o^T + b_o, then z = LN(y), then the block output
//   T  [64][max(3D, F) + 1]     [q | k | v]; the attention output overwrites q (a lane owns its query's q row of its head and holds it
//                               in registers); then act(z W_1^T + b_1)
//   mean / rstd [64] each       LN1 statistics of X: Q = (X - mean) * rstd is formed where it is read (q projection, residual of y)
// Per block: stats | GEMM [q | k | v] | attention | GEMM o (+ Q) | LN2 | GEMM ffn1 (+act) | GEMM ffn2 (+z, * m).  Rows >= N hold zeros.
// ---------------------------------------------------------------------------------------------
struct SasFusedLayer {
  const float* in_w; const float* in_b; const float* out_w; const float* out_b;
  const float* w1; const float* b1; const float* w2; const float* b2;
};

static_assert(sizeof(SasFusedLayer) == sizeof(rails_sasrec_layer), "SasFusedLayer mirrors rails_sasrec_layer field for field");

struct SasFusedArgs {
  const float* emb; const int64_t* ids; const int64_t* lengths; const float* pos_emb;
  const SasFusedLayer* layers; int n_blocks;
  int B, N, D, H, F, act, mode;
  float eps;       // postprocessor eps
  float* out;      // (B, D)
};

constexpr int kSasThreads = 256;   // one wave per SIMD: a lane may use the whole register file (q, o in registers at hd 64)
constexpr int kSasWaves = kSasThreads / 64;
constexpr int kSasRows = 64;
constexpr int kSasMaxDim = 128;   // D and F

// C (64 x n_cols) = A (64 x K) W^T, W a torch Linear / Conv1d(k=1) weight (n_cols, K); v_mfma_f32_32x32x2_f32, one wave per 32 x 32
// tile.  aop(row, k) yields the A operand (k < K); epi(row, col, acc) consumes a finished element (col < n_cols).
template <class AOp, class Epi>
__device__ __forceinline__ void fused_gemm(int K, int n_cols, const float* __restrict__ W, int wave, int lane, AOp aop, Epi epi) {
  const int x = lane & 31, h = lane >> 5;
  const int tn = (n_cols + 31) / 32;
  for (int t = wave; t < 2 * tn; t += kSasWaves) {
    const int mt = t / tn, nt = t - mt * tn;
    const int col = nt * 32 + x;
    const float* wr = W + (int64_t)(col < n_cols ? col : n_cols - 1) * K;
    sf32x16 acc = {0};
    for (int k0 = 0; k0 < K; k0 += 64) {      // 32 K-steps of two k per batch of weight loads
      float bw[32];
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        const int k = k0 + 2 * s + h;
        const float w = wr[k < K ? k : K - 1];
        bw[s] = k < K ? w : 0.0f;
      }
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        const int k = k0 + 2 * s + h;
        if (k0 + 2 * s < K) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k < K ? aop(mt * 32 + x, k) : 0.0f, bw[s], acc, 0, 0, 0);
      }
    }
    if (col < n_cols) {
#pragma unroll
      for (int r = 0; r < 16; ++r) epi(mt * 32 + acc_row(r, h), col, acc[r]);
    }
  }
}

// mean and 1 / sqrt(var + eps) of the 64 rows of src (dim wide): a wave takes 64 / kSasWaves rows, kRowLanes lanes per row
constexpr int kRowLanes = 64 / (kSasRows / kSasWaves);
__device__ __forceinline__ void fused_row_stats(const float* src, int ss, int dim, float eps, float* mean_s, float* rstd_s, int wave,
                                                int lane) {
  const int row = wave * (kSasRows / kSasWaves) + lane / kRowLanes, sub = lane % kRowLanes;
  float sm = 0.0f;
  for (int k = sub; k < dim; k += kRowLanes) sm += src[row * ss + k];
#pragma unroll
  for (int o = kRowLanes / 2; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
  const float mean = sm / (float)dim;
  float vr = 0.0f;
  for (int k = sub; k < dim; k += kRowLanes) { const float c = src[row * ss + k] - mean; vr = __builtin_fmaf(c, c, vr); }
#pragma unroll
  for (int o = kRowLanes / 2; o > 0; o >>= 1) vr += __shfl_xor(vr, o, 64);
  if (sub == 0) { mean_s[row] = mean; rstd_s[row] = 1.0f / sqrtf(vr / (float)dim + eps); }
}

template <int HD>
__device__ __forceinline__ void fused_attention(float* T, int TS, int N, int H, int hd, int wave, int lane) {
  const int D = H * hd;
  const float scale = 1.0f / sqrtf((float)hd);
  for (int head = wave; head < H; head += kSasWaves) {
    const int qi = lane < N ? lane : N - 1;
    float* qrow = T + qi * TS + head * hd;
    float q[HD], o[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      q[d] = d < hd ? qrow[d < hd ? d : 0] * scale : 0.0f;
      o[d] = 0.0f;
    }
    float m = -INFINITY, l = 0.0f;
    // K / V rows straight from LDS (stride TS: not 16-byte aligned, so scalar reads; every lane reads the same row)
    for (int t0 = 0; t0 < N; t0 += kKeyGroup) {
      float s[kKeyGroup];
      float gm = -INFINITY;
#pragma unroll
      for (int u = 0; u < kKeyGroup; ++u) {
        const int j = t0 + u;
        const float* kr = T + (j < N ? j : 0) * TS + D + head * hd;
        float acc = 0.0f;
#pragma unroll
        for (int d = 0; d < HD; ++d) acc = __builtin_fmaf(q[d], kr[d < hd ? d : 0], acc);   // q[d] = 0 for d >= hd
        s[u] = (j < N && j <= qi) ? acc * kLog2e : -INFINITY;
        gm = fmaxf(gm, s[u]);
      }
      const float mn = fmaxf(m, gm);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      m = mn;
      l *= alpha;
#pragma unroll
      for (int d = 0; d < HD; ++d) o[d] *= alpha;
#pragma unroll
      for (int u = 0; u < kKeyGroup; ++u) {
        const float p = __builtin_amdgcn_exp2f(s[u] - mn);
        l += p;
        const int j = t0 + u;
        const float* vr = T + (j < N ? j : 0) * TS + 2 * D + head * hd;
#pragma unroll
        for (int d = 0; d < HD; ++d) o[d] = __builtin_fmaf(p, vr[d < hd ? d : 0], o[d]);
      }
    }
    const float inv = 1.0f / l;
    if (lane < N) {
#pragma unroll
      for (int d = 0; d < HD; ++d)
        if (d < hd) qrow[d] = o[d] * inv;          // over this lane's own q row of this head: nobody else reads it
    }
  }
}

template <int HD>
__global__ __launch_bounds__(kSasThreads) void sasrec_fused_kernel(SasFusedArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ssm[];
  const int N = a.N, D = a.D, F = a.F;
  const int hd = D / a.H;
  const int XS = D + 1, TS = (3 * D > F ? 3 * D : F) + 1;
  float* X = ssm;                          // [64][XS]
  float* T = X + kSasRows * XS;            // [64][TS]
  float* mean_s = T + kSasRows * TS;       // [64]
  float* rstd_s = mean_s + kSasRows;       // [64]
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t* ids = a.ids + (int64_t)b * N;
  const float scale = sqrtf((float)D);

  // ---- x = (emb * sqrt(D) + pos_emb[n]) * (id != 0); rows >= N zero
  for (int i = tid; i < kSasRows * D; i += kSasThreads) {
    const int n = i / D, dd = i - n * D;
    float v = 0.0f;
    if (n < N && ids[n] != 0) v = a.emb[((int64_t)b * N + n) * D + dd] * scale + a.pos_emb[(int64_t)n * D + dd];
    X[n * XS + dd] = v;
  }
  __syncthreads();

  for (int blk = 0; blk < a.n_blocks; ++blk) {
    const SasFusedLayer L = a.layers[blk];
    // ---- LN1 statistics
    fused_row_stats(X, XS, D, kBlockLnEps, mean_s, rstd_s, wave, lane);
    __syncthreads();
    // ---- [q | k | v] = [Q | X | X] W_in^T + b_in  (rows >= N: zero)
    fused_gemm(D, D, L.in_w, wave, lane,
               [&](int r, int k) { return (X[r * XS + k] - mean_s[r]) * rstd_s[r]; },
               [&](int r, int c, float v) { T[r * TS + c] = r < N ? v + L.in_b[c] : 0.0f; });
    fused_gemm(D, 2 * D, L.in_w + (int64_t)D * D, wave, lane,
               [&](int r, int k) { return X[r * XS + k]; },
               [&](int r, int c, float v) { T[r * TS + D + c] = r < N ? v + L.in_b[D + c] : 0.0f; });
    __syncthreads();
    // ---- attention: T[i][:D] = softmax_causal(q k^T / sqrt(hd)) v
    fused_attention<HD>(T, TS, N, a.H, hd, wave, lane);
    __syncthreads();
    // ---- y = Q + a W_o^T + b_o  -> X (each element reads its own residual, then overwrites it)
    fused_gemm(D, D, L.out_w, wave, lane,
               [&](int r, int k) { return T[r * TS + k]; },
               [&](int r, int c, float v) {
                 const float y = (v + L.out_b[c]) + (X[r * XS + c] - mean_s[r]) * rstd_s[r];
                 X[r * XS + c] = r < N ? y : 0.0f;
               });
    __syncthreads();
    // ---- z = LN(y) in place
    fused_row_stats(X, XS, D, kBlockLnEps, mean_s, rstd_s, wave, lane);
    __syncthreads();
    for (int i = tid; i < kSasRows * D; i += kSasThreads) {
      const int n = i / D, dd = i - n * D;
      X[n * XS + dd] = (X[n * XS + dd] - mean_s[n]) * rstd_s[n];
    }
    __syncthreads();
    // ---- h = act(z W_1^T + b_1) -> T
    fused_gemm(D, F, L.w1, wave, lane,
               [&](int r, int k) { return X[r * XS + k]; },
               [&](int r, int c, float v) { T[r * TS + c] = ffn_act(v + L.b1[c], a.act); });
    __syncthreads();
    // ---- x = (h W_2^T + b_2 + z) * (id != 0)
    fused_gemm(F, D, L.w2, wave, lane,
               [&](int r, int k) { return T[r * TS + k]; },
               [&](int r, int c, float v) {
                 const float y = (v + L.b2[c]) + X[r * XS + c];
                 X[r * XS + c] = (r < N && ids[r] != 0) ? y : 0.0f;
               });
    __syncthreads();
  }
  // ---- postprocessor on row len - 1
  if (wave == 0) {
    const int64_t len = a.lengths[b];
    const int row = len < 1 ? 0 : len > N ? N - 1 : (int)len - 1;   // the host validates or clamps; never a row outside X
    const float* xr = X + row * XS;
    if (a.mode == 0) {
      float sm = 0.0f;
      for (int k = lane; k < D; k += 64) sm += xr[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
      const float mean = sm / (float)D;
      float vr = 0.0f;
      for (int k = lane; k < D; k += 64) { const float c = xr[k] - mean; vr = __builtin_fmaf(c, c, vr); }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) vr += __shfl_xor(vr, o, 64);
      const float rstd = 1.0f / sqrtf(vr / (float)D + a.eps);
      for (int k = lane; k < D; k += 64) a.out[(int64_t)b * D + k] = (xr[k] - mean) * rstd;
    } else {
      float vr = 0.0f;
      for (int k = lane; k < D; k += 64) vr = __builtin_fmaf(xr[k], xr[k], vr);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) vr += __shfl_xor(vr, o, 64);
      const float nrm = fmaxf(sqrtf(vr), a.eps);
      for (int k = lane; k < D; k += 64) a.out[(int64_t)b * D + k] = xr[k] / nrm;
    }
  }
}

static size_t sasrec_fused_lds(int D, int F) {
  const int XS = D + 1, TS = (3 * D > F ? 3 * D : F) + 1;
  return sizeof(float) * ((size_t)kSasRows * (XS + TS) + 2 * kSasRows);
}

bool sasrec_fused_supported(int N, int D, int H, int F) {
  if (N < 1 || N > kSasRows || D < 1 || D > kSasMaxDim || F < 1 || F > kSasMaxDim || H < 1 || D % H != 0) return false;
  if (D / H > 64) return false;
  return sasrec_fused_lds(D, F) <= 150 * 1024;
}

int sasrec_encode_fused(const float* emb, const int64_t* ids, const int64_t* lengths, const float* pos_emb, const void* layers, int n_blocks,
                        int B, int N, int D, int H, int F, int act, int mode, float eps, float* out, hipStream_t stream) {
  if (B == 0) return kOk;
  if (!sasrec_fused_supported(N, D, H, F)) { set_error("sasrec_encode_fused: geometry not supported"); return kErrUnsupported; }
  const size_t lds = sasrec_fused_lds(D, F);
  SasFusedArgs a{emb, ids, lengths, pos_emb, static_cast<const SasFusedLayer*>(layers), n_blocks, B, N, D, H, F, act, mode, eps, out};
  const int hd = D / H;
  const void* fn = hd <= 16 ? reinterpret_cast<const void*>(&sasrec_fused_kernel<16>)
                 : hd <= 32 ? reinterpret_cast<const void*>(&sasrec_fused_kernel<32>)
                            : reinterpret_cast<const void*>(&sasrec_fused_kernel<64>);
  static DynLdsOnce once[3];   // one opt-in per instantiation
  if (ensure_dyn_lds(once[hd <= 16 ? 0 : hd <= 32 ? 1 : 2], fn, 150 * 1024) != kOk) return kErrLaunch;
  if (hd <= 16) hipLaunchKernelGGL(sasrec_fused_kernel<16>, dim3(B), dim3(kSasThreads), lds, stream, a);
  else if (hd <= 32) hipLaunchKernelGGL(sasrec_fused_kernel<32>, dim3(B), dim3(kSasThreads), lds, stream, a);
  else hipLaunchKernelGGL(sasrec_fused_kernel<64>, dim3(B), dim3(kSasThreads), lds, stream, a);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

}  // namespace mol
