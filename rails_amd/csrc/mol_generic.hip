// Shape-generic fp32 Mixture-of-Logits scoring for gfx950: steps 5-8 of the reference's eval-mode MoLSimilarity.forward
// (rails/similarities/mol/similarity_fn.py:389-413) for ANY (P_Q, P_X, d, H) inside the envelope of mol_generic.h, with the
// shape as a launch argument.  Used only where no fused kernel exists (or when the route is forced): it is slower than those.
//
// A wave scores one query against a tile of 32 items; items sit on the MFMA column axis (lane & 31) as in the fused kernels.
//   GEMM1   per item group m and block of 32 query groups: acc[p][x] = sum_k Eq[b][p][k]/tau * Ex[x][m][k], k zero-padded to a
//           multiple of 8; the cross logits go to LDS as cl[l = p P_X + m][x] (the store does the (p, m) -> l permutation),
//           rows L .. Lp of that buffer stay zero
//   gate    per block t of 32 hidden units: hid = silu(b1 + W1[t] cl), cl read back from LDS as the B operand; the accumulator of
//           that MFMA IS the B operand of the next one (register r of both lane halves = hidden units 32 t + row(r, 0 / 1)), so
//           gqi[v] += W2[v][t] hid chains in registers, one accumulator tile per 32 logits (TL = Lp / 32, the only template axis)
//   mix     g = gq gi + gqi, w = silu(g) (or the plain sum), softmax over the L real logits, out = sum pi cl / clamp(sum pi, 1e-6)
// Pair-gate weights are read in A-operand order (mol_generic.h): from LDS when both matrices fit next to the cl buffers
// (RES = true, staged once per workgroup, workgroups are persistent), else streamed from L2 one K-slice of 16 B per lane at a time.
//
// One arithmetic per pair: every contraction visits k in ascending order of its zero-padded axis, the softmax sums run in
// ascending l per lane half and the two halves are added last (a commutative add), and nothing depends on the lane, the wave,
// the batch, N, or on whether the pair came from a shared index, per-row candidates or positions of the shared index (the indexed
// mode: the item row of a lane comes from a 64-bit position load at the head of the unit): same bits everywhere.
// fp32 throughout, precise expf and true divisions.
//
// The explaining instantiations (EXP; rails_mol_generic_explain*, per-row candidates and the indexed mode) also store what the mixture is
// made of: per pair the L cross logits cl and the L mixture weights pi = (e / den) / clamp(sum e / den, 1e-6), (B, T, L) row-major.  The
// logit is the same code as everywhere else; cl and pi leave through the wave's own cl buffer (emit_tile), whole 256-byte runs at a time.
#include <hip/hip_runtime.h>

#include "mol_generic.h"
#include "mol_layout.h"

namespace mol {

typedef float gf32x16 __attribute__((ext_vector_type(16)));

constexpr int kGenThreads = 256;         // 4 waves, one tile of 32 items each
constexpr int kGenWaves = kGenThreads / 64;
constexpr int kGenBlockItems = 32 * kGenWaves;

struct GenKernelArgs {
  GenericScoreArgs a;
  int PQ, PX, dp, L, Lq, TH, combine_none;
  int64_t item_floats, query_floats;
  int64_t blocks_per_row, units;
};

__device__ __forceinline__ gf32x16 mfma4(const float4 a, const float4 b, gf32x16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c, 0, 0, 0);
  return c;
}

__device__ __forceinline__ float silu_exact(float v) { return v / (1.0f + expf(-v)); }

// cl buffer of a wave: logit l of item x at ((l >> 2) * 32 + x) * 4 + (l & 3): four consecutive logits of an item are one float4
__device__ __forceinline__ int cl_at(int l, int x) { return ((l >> 2) * 32 + x) * 4 + (l & 3); }

// The wave's cl-shaped buffer holds a value per (l, item): float4 (l >> 2) of item x at slot x ^ ((l >> 2) & 7) of its row of 32 (stage_at).
// The `nv` first items of the tile are consecutive pairs of one query row, so their L-vectors are ONE run of nv * L floats at dst: lane i of
// a store instruction writes float f = 64 j + i of it -- 256 contiguous bytes per instruction, whatever L is.  The XOR spreads the 8 float4
// rows that 32 consecutive l of one item touch over all 32 banks of the dword read.
__device__ __forceinline__ int stage_at(int l4, int x) { return l4 * 32 + (x ^ (l4 & 7)); }

__device__ __forceinline__ void emit_tile(const float* buf, float* dst, int nv, int L, int lane) {
  const int total = nv * L;
  for (int f = lane; f < total; f += 64) {
    const int item = f / L, l = f - item * L;
    dst[f] = buf[stage_at(l >> 2, item) * 4 + (l & 3)];
  }
}

// orders this wave's LDS writes before its reads of other lanes' slots (the buffer is the wave's own: no workgroup barrier is needed)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// IDX: the indexed mode (candidates scored in place on the shared index) -- an instantiation of its own, so that the dense and per-row
// launches keep their registers; the item row address and the count test are all that differs.
// EXP: the explaining mode, an instantiation of its own for the same reason; the store stage behind the logit is all it adds.
template <int TL, bool RES, bool IDX = false, bool EXP = false>
__global__ __launch_bounds__(kGenThreads) void mol_generic_score_kernel(GenKernelArgs k) {
  MOL_RUN_IF(k.a.run_if);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int Lp = 32 * TL;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, x = lane & 31, hi = lane >> 5;
  const int PQ = k.PQ, PX = k.PX, dp = k.dp, L = k.L, TH = k.TH, Hp = 32 * k.TH;
  float* cl = smem + wave * (Lp * 32);
  const float4* cl4 = reinterpret_cast<const float4*>(cl);
  const float4* w1g = reinterpret_cast<const float4*>(k.a.wpack);
  const float4* w2g = w1g + (Hp * Lp) / 4;
  const float* b1 = k.a.wpack + 2 * Hp * Lp;
  const float* b2 = b1 + Hp;
  float4* wl = reinterpret_cast<float4*>(smem + kGenWaves * Lp * 32);   // RES: W1 then W2, as in the pack
  if constexpr (RES) {
    for (int i = threadIdx.x; i < (2 * Hp * Lp) / 4; i += kGenThreads) wl[i] = w1g[i];
  }
  for (int i = lane; i < Lp * 32; i += 64) cl[i] = 0.0f;   // rows L .. Lp are never written again
  __syncthreads();
  auto w1 = [&](int i) -> float4 { if constexpr (RES) return wl[i]; else return w1g[i]; };
  auto w2 = [&](int i) -> float4 { if constexpr (RES) return wl[(Hp * Lp) / 4 + i]; else return w2g[i]; };

  for (int64_t u = blockIdx.x; u < k.units; u += gridDim.x) {
    const int b = (int)(u % k.a.B);
    const int64_t xi = (u / k.a.B) * kGenBlockItems + wave * 32 + x;
    bool valid = xi < k.a.n_items;
    bool live = true;                                          // false: this wave's tile is past the row's count -- it only keeps the unit's barriers
    int64_t row;
    if constexpr (IDX) {
      // this lane's item: one 64-bit load ahead of GEMM1, clamped into the index (a slot past the row's end reads the last slot's)
      const int64_t cnt = k.a.cand_count ? (int64_t)k.a.cand_count[b] : k.a.n_items;
      live = __builtin_amdgcn_readfirstlane((int)(xi - x < cnt)) != 0;      // (the same for the whole wave: a scalar branch, EXEC stays full)
      const int64_t p = k.a.cand_pos[(int64_t)b * k.a.n_items + (valid ? xi : k.a.n_items - 1)];
      row = p < 0 ? 0 : (p < k.a.index_items ? p : k.a.index_items - 1);
      valid = valid && xi < cnt;
    } else {
      row = (k.a.per_row ? (int64_t)b * k.a.n_items : 0) + (valid ? xi : k.a.n_items - 1);   // clamped: always a real row
    }
    const float* irow = k.a.ipack + row * k.item_floats;
    const float* qrow = k.a.qpack + (int64_t)b * k.query_floats;

    if (live) {
      // ---- GEMM1 -> cl in LDS
      for (int p0 = 0; p0 < PQ; p0 += 32) {
        const int p = p0 + x;                                  // this lane's A row
        const float* arow = qrow + (p < PQ ? p : PQ - 1) * dp + 4 * hi;
        for (int m = 0; m < PX; ++m) {
          const float* brow = irow + m * dp + 4 * hi;
          gf32x16 acc = {0};
          for (int c = 0; c < dp; c += 8) {
            float4 av = *reinterpret_cast<const float4*>(arow + c);
            const float4 bv = *reinterpret_cast<const float4*>(brow + c);
            if (p >= PQ) av = make_float4(0.f, 0.f, 0.f, 0.f);
            acc = mfma4(av, bv, acc);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int pr = p0 + acc_row(r, hi);
            if (pr < PQ) cl[cl_at(pr * PX + m, x)] = acc[r];
          }
        }
      }
    }
    __syncthreads();

    if (live) {
      // ---- pair gate: gqi = W2 silu(W1 cl + b1) + b2
      gf32x16 out[TL];
#pragma unroll
      for (int v = 0; v < TL; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[v][r] = b2[32 * v + acc_row(r, hi)];
      for (int t = 0; t < TH; ++t) {
        gf32x16 h;
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = b1[32 * t + acc_row(r, hi)];
#pragma unroll
        for (int c = 0; c < Lp / 8; ++c) h = mfma4(w1((t * (Lp / 8) + c) * 64 + lane), cl4[(2 * c + hi) * 32 + x], h);
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = silu_exact(h[r]);
#pragma unroll
        for (int v = 0; v < TL; ++v)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float4 hv = make_float4(h[4 * g], h[4 * g + 1], h[4 * g + 2], h[4 * g + 3]);
            out[v] = mfma4(w2(((t * TL + v) * 4 + g) * 64 + lane), hv, out[v]);
          }
      }

      // ---- combine + softmax mixture: this lane holds logits l = 32 v + 8 g + 4 hi + j of item x
      const float* gq = qrow + PQ * dp;
      const float* gi = irow + PX * dp;
      float mx = -INFINITY;
#pragma unroll
      for (int v = 0; v < TL; ++v)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int l0 = 32 * v + 8 * g + 4 * hi;
          const int lc = l0 < k.Lq ? l0 : 0;                    // Lq is a multiple of 4: a float4 inside the row
          const float4 q4 = *reinterpret_cast<const float4*>(gq + lc);
          const float4 i4 = *reinterpret_cast<const float4*>(gi + lc);
          const float qv[4] = {q4.x, q4.y, q4.z, q4.w}, iv[4] = {i4.x, i4.y, i4.z, i4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float gqi = out[v][4 * g + j];
            float w;
            if (k.combine_none) w = (qv[j] + iv[j]) + gqi;
            else w = silu_exact(__builtin_fmaf(qv[j], iv[j], gqi));
            out[v][4 * g + j] = w;
            if (l0 + j < L) mx = fmaxf(mx, w);
          }
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float den = 0.0f, num = 0.0f;
#pragma unroll
      for (int v = 0; v < TL; ++v)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int l0 = 32 * v + 8 * g + 4 * hi;
          const float4 c4 = cl4[(8 * v + 2 * g + hi) * 32 + x];
          const float cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float e = l0 + j < L ? expf(out[v][4 * g + j] - mx) : 0.0f;
            den += e;
            num = __builtin_fmaf(e, cv[j], num);
          }
        }
      den += __shfl_xor(den, 32, 64);
      num += __shfl_xor(num, 32, 64);
      // pi = e / den, then the eval-time renormalisation pi / clamp(sum pi, 1e-6) (similarity_fn.py:42-46)
      const float rden = 1.0f / den;
      const float res = (num * rden) / fmaxf(den * rden, 1e-6f);
      if (valid && hi == 0) k.a.logits[(int64_t)b * k.a.ld + xi] = res;
      if constexpr (EXP) {
        // the tile's valid items are its first nv slots (valid is a prefix of x): pairs b * n_items + (xi - x) .. + nv of the outputs
        // (the explaining launches take no per-row counts: mol_generic.h)
        const int64_t left = k.a.n_items - (xi - x);
        const int nv = left >= 32 ? 32 : left > 0 ? (int)left : 0;
        const int64_t pair0 = ((int64_t)b * k.a.n_items + (xi - x)) * L;
        float4* st4 = reinterpret_cast<float4*>(cl);
        // cl: every lane moves its own float4s to their staged slots (a permutation inside a row of 32: read, then write), rows L .. Lp stay zero
#pragma unroll
        for (int v = 0; v < TL; ++v) {
          const int r0 = 8 * v + hi;
          const float4 c0 = cl4[r0 * 32 + x], c1 = cl4[(r0 + 2) * 32 + x], c2 = cl4[(r0 + 4) * 32 + x], c3 = cl4[(r0 + 6) * 32 + x];
          wave_lds_fence();
          st4[stage_at(r0, x)] = c0;
          st4[stage_at(r0 + 2, x)] = c1;
          st4[stage_at(r0 + 4, x)] = c2;
          st4[stage_at(r0 + 6, x)] = c3;
        }
        wave_lds_fence();
        emit_tile(cl, k.a.cl_out + pair0, nv, L, lane);
        wave_lds_fence();
        // pi over the same slots: e recomputed from w (the same bits as in the sums above), 0 in the padded logits
        const float rnorm = fmaxf(den * rden, 1e-6f);
#pragma unroll
        for (int v = 0; v < TL; ++v)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int l0 = 32 * v + 8 * g + 4 * hi;
            auto pi_of = [&](int j) { return l0 + j < L ? (expf(out[v][4 * g + j] - mx) * rden) / rnorm : 0.0f; };
            st4[stage_at(8 * v + 2 * g + hi, x)] = make_float4(pi_of(0), pi_of(1), pi_of(2), pi_of(3));
          }
        wave_lds_fence();
        emit_tile(cl, k.a.pi_out + pair0, nv, L, lane);
        // (the next unit's GEMM1 rewrites every l < L of every item; what is left past L is zeros)
      }
    }
    __syncthreads();   // the next unit's GEMM1 overwrites cl
  }
}

// ---- packs ----------------------------------------------------------------------------------------------------------------
// W1f[t][c][lane][j]    = W1[32 t + (lane & 31)][8 c + 4 (lane >> 5) + j]                     (t < TH, c < Lp / 8)
// W2f[t][v][g][lane][j] = W2[32 v + (lane & 31)][32 t + row(4 g + j, lane >> 5)]              (v < TL, g < 4)
__global__ void mol_generic_pack_gate_kernel(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                             const float* __restrict__ b2, float* __restrict__ out, int L, int H, int Lp, int Hp) {
  const int TL = Lp / 32, HL = Hp * Lp, total = 2 * HL + Hp + Lp;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    float v = 0.0f;
    if (i < HL) {
      const int j = i & 3, lane = (i >> 2) & 63, blk = i >> 8;
      const int c = blk % (Lp / 8), t = blk / (Lp / 8);
      const int hrow = 32 * t + (lane & 31), l = 8 * c + 4 * (lane >> 5) + j;
      if (hrow < H && l < L) v = w1[hrow * L + l];
    } else if (i < 2 * HL) {
      const int q = i - HL;
      const int j = q & 3, lane = (q >> 2) & 63, blk = q >> 8;
      const int g = blk & 3, tv = (blk >> 2) % TL, t = (blk >> 2) / TL;
      const int l = 32 * tv + (lane & 31), hcol = 32 * t + acc_row(4 * g + j, lane >> 5);
      if (l < L && hcol < H) v = w2[l * H + hcol];
    } else if (i < 2 * HL + Hp) {
      const int q = i - 2 * HL;
      if (q < H) v = b1[q];
    } else {
      const int q = i - 2 * HL - Hp;
      if (q < L) v = b2[q];
    }
    out[i] = v;
  }
}

int generic_pack_gate_weights(const Shape& s, const Weights& w, float* wpack, hipStream_t stream) {
  const int total = (int)gen_gate_pack_floats(s);
  hipLaunchKernelGGL(mol_generic_pack_gate_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, w.gqi_w1, w.gqi_b1, w.gqi_w2, w.gqi_b2,
                     wpack, num_logits(s), s.gating_qi_hidden_dim, gen_lp(s), gen_hp(s));
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

__global__ void mol_generic_index_unpack_kernel(const float* __restrict__ ipack, int64_t n, int PX, int d, int dp, int L, int64_t item_floats,
                                                float* __restrict__ ex, float* __restrict__ gi) {
  const int per = PX * d + L;
  const int64_t total = n * per;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t item = i / per;
    const int c = (int)(i - item * per);
    const float* row = ipack + item * item_floats;
    if (c < PX * d) {
      if (ex) ex[item * PX * d + c] = row[(c / d) * dp + c % d];
    } else if (gi) {
      gi[item * L + (c - PX * d)] = row[PX * dp + (c - PX * d)];
    }
  }
}

int generic_index_unpack(const Shape& s, const float* ipack, int64_t n, float* ex, float* gi, hipStream_t stream) {
  if (n <= 0) return kOk;
  const int PX = s.item_dot_product_groups, d = s.dot_product_dimension, L = num_logits(s);
  int64_t blocks = (n * (PX * d + L) + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(mol_generic_index_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, ipack, n, PX, d, gen_dp(s), L,
                     gen_item_floats(s), ex, gi);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// Eq for the bf16 scans of the padded table width (mol_generic.h gen_table_width): a copy, the columns d .. width zeros
__global__ void mol_generic_eq_pad_kernel(const float* __restrict__ eq, int64_t rows, int d, int width, float* __restrict__ out) {
  const int64_t total = rows * width;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / width;
    const int c = (int)(i - r * width);
    out[i] = c < d ? eq[r * d + c] : 0.0f;
  }
}

int generic_eq_pad(const Shape& s, const float* eq, int64_t rows, float* out, hipStream_t stream) {
  const int width = gen_table_width(s);
  if (rows <= 0 || width <= 0) return kOk;
  int64_t blocks = (rows * width + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(mol_generic_eq_pad_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, eq, rows, s.dot_product_dimension, width, out);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// ---- launch ---------------------------------------------------------------------------------------------------------------
constexpr size_t kGenMaxLds = 160 * 1024;

template <int TL, bool RES, bool IDX, bool EXP>
static int launch_generic(const GenKernelArgs& k, size_t lds, int grid, hipStream_t stream) {
  static DynLdsOnce once;
  auto* fn = &mol_generic_score_kernel<TL, RES, IDX, EXP>;
  // the bytes depend on the shape (L, and H when the weights are resident), not on the instantiation alone: opt in to the route's maximum
  if (ensure_dyn_lds(once, reinterpret_cast<const void*>(fn), (int)kGenMaxLds) != kOk) return kErrLaunch;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kGenThreads), lds, stream, k);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

template <int TL>
static int launch_generic_tl(const GenKernelArgs& k, bool res, size_t lds, int grid, hipStream_t stream) {
  if (k.a.cl_out) {      // the explaining instantiations: per-row candidates or the indexed mode
    if (k.a.cand_pos) return res ? launch_generic<TL, true, true, true>(k, lds, grid, stream) : launch_generic<TL, false, true, true>(k, lds, grid, stream);
    return res ? launch_generic<TL, true, false, true>(k, lds, grid, stream) : launch_generic<TL, false, false, true>(k, lds, grid, stream);
  }
  if (k.a.cand_pos) return res ? launch_generic<TL, true, true, false>(k, lds, grid, stream) : launch_generic<TL, false, true, false>(k, lds, grid, stream);
  return res ? launch_generic<TL, true, false, false>(k, lds, grid, stream) : launch_generic<TL, false, false, false>(k, lds, grid, stream);
}

int generic_score(const Shape& s, const GenericScoreArgs& a, int n_cu, hipStream_t stream) {
  GenKernelArgs k;
  k.a = a;
  k.PQ = s.query_dot_product_groups; k.PX = s.item_dot_product_groups; k.dp = gen_dp(s); k.L = num_logits(s); k.Lq = gen_lq(s);
  k.TH = gen_hp(s) / 32; k.combine_none = s.gating_combination == RAILS_COMBINE_NONE ? 1 : 0;
  k.item_floats = gen_item_floats(s); k.query_floats = gen_query_floats(s);
  k.blocks_per_row = (a.n_items + kGenBlockItems - 1) / kGenBlockItems;
  k.units = k.blocks_per_row * a.B;
  if (k.units <= 0) return kOk;
  const int Lp = gen_lp(s), Hp = gen_hp(s), TL = Lp / 32;
  const size_t cl_bytes = sizeof(float) * (size_t)kGenWaves * Lp * 32, w_bytes = sizeof(float) * 2 * (size_t)Hp * Lp;
  const bool res = cl_bytes + w_bytes <= kGenMaxLds;    // both weight matrices next to the cl buffers, else streamed
  const size_t lds = cl_bytes + (res ? w_bytes : 0);
  const int64_t max_grid = (int64_t)n_cu * (lds <= kGenMaxLds / 2 ? 2 : 1);
  const int grid = (int)(k.units < max_grid ? k.units : max_grid);
  switch (TL) {
    case 1: return launch_generic_tl<1>(k, res, lds, grid, stream);
    case 2: return launch_generic_tl<2>(k, res, lds, grid, stream);
    case 3: return launch_generic_tl<3>(k, res, lds, grid, stream);
    case 4: return launch_generic_tl<4>(k, res, lds, grid, stream);
    case 5: return launch_generic_tl<5>(k, res, lds, grid, stream);
    case 6: return launch_generic_tl<6>(k, res, lds, grid, stream);
    case 7: return launch_generic_tl<7>(k, res, lds, grid, stream);
    case 8: return launch_generic_tl<8>(k, res, lds, grid, stream);
  }
  set_error("generic scoring route: P_Q * P_X = %d > %d", k.L, kGenericMaxL);
  return kErrUnsupported;
}

}  // namespace mol
