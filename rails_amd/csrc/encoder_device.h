// Device helpers shared by the encoder kernels (hstu.hip, sasrec.hip, kvdec.hip).
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

}  // namespace mol
