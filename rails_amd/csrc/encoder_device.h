// Device helpers shared by the encoder kernels (hstu.hip, hstu_rows.hip, sasrec.hip, kvdec.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/rails_amd.h"

namespace mol {

// silu on the hardware transcendentals (v_exp_f32 = 2^x, v_rcp_f32; ~1 ulp each) instead of expf + an IEEE division (~50
// instructions per element: the attention kernels were VALU-bound on it); the scoring kernel does the same.
__device__ __forceinline__ float silu_fast(float v) {
  return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v));
}

__device__ __forceinline__ float relu(float v) { return v > 0.0f ? v : 0.0f; }

// GELU (erf), as torch.nn.GELU()
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// the FFN activation of SASRec: RAILS_ACT_RELU, otherwise GELU (the codes of rails_gemm_f32's act)
__device__ __forceinline__ float ffn_act(float v, int act) {
  if (act == RAILS_ACT_RELU) return relu(v);
  return gelu_erf(v);
}

// sum over the 64 lanes of a wave
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The postprocessor of one row by one wave: LayerNorm without affine (mode 0; two passes, biased variance) or x / max(||x||, eps)
// (mode 1).  The only copy: the prefill (rows_normalize_kernel) and every decode step end in it, so a row gives the same bits on
// every route.
__device__ __forceinline__ void normalize_row(const float* xr, int D, int mode, float eps, float* out_row, int lane) {
  if (mode == 0) {
    float sm = 0.0f;
    for (int k = lane; k < D; k += 64) sm += xr[k];
    const float mean = wave_sum(sm) / (float)D;
    float vr = 0.0f;
    for (int k = lane; k < D; k += 64) { const float c = xr[k] - mean; vr = __builtin_fmaf(c, c, vr); }
    const float rstd = 1.0f / sqrtf(wave_sum(vr) / (float)D + eps);
    for (int k = lane; k < D; k += 64) out_row[k] = (xr[k] - mean) * rstd;
  } else {
    float vr = 0.0f;
    for (int k = lane; k < D; k += 64) vr = __builtin_fmaf(xr[k], xr[k], vr);
    const float nrm = fmaxf(sqrtf(wave_sum(vr)), eps);
    for (int k = lane; k < D; k += 64) out_row[k] = xr[k] / nrm;
  }
}

// ---- the staged A tile of the decoders' row GEMMs (kvdec.hip, hstu_rows.hip): rows x ks floats in LDS.
// The staging loop itself (kStageBatch loads of every thread issued, then their stores) is written out in both kernels: behind a
// helper, the whole loop or one turn of it, the single-row SASRec row kernels compile to other code than they had.
constexpr int kStageBatch = 8;   // global loads in flight per thread while the tile is staged
constexpr int kTileRows = 32;    // rows of a staged tile and threads of its workgroup: both files static_assert their own names to these
constexpr int kTileThreads = 256;

// One turn of `for (r = wave; r < rows; r += waves)`, a loop that stays in the kernel for the same reason: the LayerNorm
// statistics of one staged row by one wave (no affine, biased variance, two-pass); lane 0 stores them.  The caller's barrier follows the loop.
__device__ __forceinline__ void row_ln_stats(const float* row, int K, float eps, float* mean_o, float* rstd_o, int lane) {
  float sm = 0.0f;
  for (int k = lane; k < K; k += 64) sm += row[k];
  const float mean = wave_sum(sm) / (float)K;
  float vr = 0.0f;
  for (int k = lane; k < K; k += 64) { const float c = row[k] - mean; vr = __builtin_fmaf(c, c, vr); }
  vr = wave_sum(vr);
  if (lane == 0) { *mean_o = mean; *rstd_o = 1.0f / sqrtf(vr / (float)K + eps); }
}

}  // namespace mol
