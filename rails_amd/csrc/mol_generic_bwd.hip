// Backward of the shape-generic fp32 pair stage (mol_generic.hip) for per-row candidates: gradients of sum(dY * logits) with respect to
// the query pack (Eq, gq), the candidate pack (Ex, gi) and the pair-gate weights (W1, b1, W2, b2), in eval-mode arithmetic.  DESIGN 3.23.
//
// mol_generic_bwd_kernel: a workgroup owns a query row b, its waves take the row's tiles of 32 candidates in turn (wave w: tiles w, w + W, ..).
// Per tile the wave recomputes the forward as mol_generic_score_kernel does (GEMM1 into its cl buffer, the gate per block of 32 hidden units
// on v_mfma_f32_32x32x2_f32) and runs the chain
//   dw = pi (dY cl - dY y), dg = dw silu'(g), dgi = dg gq, dgq += dg gi            (lane-local: logits l = 32 v + 8 g + 4 hi + j of item x)
//   per hidden block t: h recomputed, da = W2^T dg (dg read from LDS as the B operand), dh = da silu'(h),
//                       dcl += W1^T dh (the accumulator of the da product IS the B operand, as hid is in the forward)
//   dEx[m] = sum_p dcl[p, m] Eq[p] / tau (B operand dcl from LDS, A operand the query pack), dEq[p] += sum_m sum_x dcl[p, m][x] Ex[x][m]
// dEq and dgq are accumulated over the row's tiles (in registers up to 96 logits, in the wave's LDS beyond), summed over the wave's lanes and the workgroup's waves in a fixed order, and
// written once: no atomics, and no dependence on the grid (a row is never split).
//
// Weight gradients go through a workspace of a fixed number of pairs (rows of cl, a, dh, dg, pair-major): the host runs the rows in
// chunks; per chunk mol_generic_bwd_contract_kernel contracts the chunk over its pairs, one wave per 32 x 32 tile of dW1 / dW2 (and per block
// of db1 / db2) and per fixed run of kBwdSplitPairs pairs, and mol_generic_bwd_reduce_kernel adds the runs in ascending order to the result.
#include <hip/hip_runtime.h>

#include "mol_generic.h"
#include "mol_layout.h"

namespace mol {
namespace {

typedef float bf32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ bf32x16 mfma1(float a, float b, bf32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ bf32x16 mfma4(const float4 a, const float4 b, bf32x16 c) {
  c = mfma1(a.x, b.x, c);
  c = mfma1(a.y, b.y, c);
  c = mfma1(a.z, b.z, c);
  c = mfma1(a.w, b.w, c);
  return c;
}

// logit l of item x in a wave's cl-shaped buffer (mol_generic.hip cl_at): four consecutive logits of an item are one float4
__device__ __forceinline__ int cl_at(int l, int x) { return ((l >> 2) * 32 + x) * 4 + (l & 3); }

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// silu(v) and silu'(v) = s (1 + v (1 - s)), s = sigmoid(v)
__device__ __forceinline__ void silu_grad(float v, float& val, float& grad) {
  const float s = 1.0f / (1.0f + expf(-v));
  val = v * s;
  grad = s * (1.0f + v * (1.0f - s));
}

struct BwdKernelArgs {
  const float *wpack, *wtpack, *qpack, *ipack, *dy;
  float *d_qpack, *d_ipack;                     // each may be NULL: not wanted
  float *ws_cl, *ws_a, *ws_dh, *ws_dg;          // all NULL: no weight gradients
  int64_t ld_dy, X, item_floats, query_floats, xp32;
  int row0, nrows;
  int PQ, PX, dp, L, Lq, TH, combine_none, nq, nkb, wave_floats, dq_off, vec_off;
  float inv_tau;
};

template <int TL>
__global__ __launch_bounds__(256) void mol_generic_bwd_kernel(BwdKernelArgs k) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int Lp = 32 * TL;
  // From 128 logits on, out[TL] and the row's accumulators no longer fit the register file together: dgq (per lane, a third cl-shaped
  // buffer) and the dEq tiles (raw accumulator layout) are then kept in the wave's LDS and updated per tile.
  constexpr bool kLdsAcc = TL >= 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, x = lane & 31, hi = lane >> 5;
  const int PQ = k.PQ, PX = k.PX, dp = k.dp, L = k.L, TH = k.TH, Hp = 32 * k.TH;
  float* cl = smem + wave * k.wave_floats;       // the cross logits of the tile
  float* dgb = cl + Lp * 32;                     // silu'(g), then dg, then dcl: the same layout
  const float4* cl4 = reinterpret_cast<const float4*>(cl);
  float4* dg4 = reinterpret_cast<float4*>(dgb);
  float4* dgq4 = reinterpret_cast<float4*>(dgb + Lp * 32);   // kLdsAcc only
  float* dqb = cl + k.dq_off;                                  // kLdsAcc only
  const float4* w1g = reinterpret_cast<const float4*>(k.wpack);
  const float4* w2g = w1g + (Hp * Lp) / 4;
  const float* b1 = k.wpack + 2 * Hp * Lp;
  const float* b2 = b1 + Hp;
  const float4* w2tg = reinterpret_cast<const float4*>(k.wtpack);   // W2^T in W1's order, then W1^T in W2's order
  const float4* w1tg = w2tg + (Hp * Lp) / 4;
  const int64_t ntiles = (k.X + 31) / 32;
  const bool want_w = k.ws_cl != nullptr;

  for (int rb = blockIdx.x; rb < k.nrows; rb += gridDim.x) {
    const int b = k.row0 + rb;
    const float* qrow = k.qpack + (int64_t)b * k.query_floats;
    const float* gq = qrow + PQ * dp;
    for (int i = lane; i < Lp * 32; i += 64) cl[i] = 0.0f;   // rows L .. Lp stay zero over the row's tiles
    wave_lds_fence();
    bf32x16 dq[kLdsAcc ? 1 : 4];
    bf32x16 dgq[kLdsAcc ? 1 : TL];
    if constexpr (kLdsAcc) {
      for (int i = lane; i < Lp * 32; i += 64) dgb[Lp * 32 + i] = 0.0f;
      for (int i = lane; i < k.nq * 1024; i += 64) dqb[i] = 0.0f;
      wave_lds_fence();
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[i][r] = 0.0f;
#pragma unroll
      for (int v = 0; v < TL; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) dgq[v][r] = 0.0f;
    }

    for (int64_t tile = wave; tile < ntiles; tile += nw) {
      const int64_t xi = tile * 32 + x;
      const bool valid = xi < k.X;
      const int64_t row = (int64_t)b * k.X + (valid ? xi : k.X - 1);           // clamped: always a real row
      const float* irow = k.ipack + row * k.item_floats;
      const float* gi = irow + PX * dp;
      const float dyv = valid ? k.dy[(int64_t)b * k.ld_dy + xi] : 0.0f;        // a slot past the row's end: every gradient of it is 0
      const int64_t wsrow = (int64_t)rb * k.xp32 + xi;                         // this pair's row of the chunk workspace
      // (opaque to the optimiser: the clamped gate offsets below are then computed where they are used, not hoisted out of the tile loop
      // into a register pair per group of four logits)
      int Lq_t = k.Lq;
      asm volatile("" : "+s"(Lq_t));

      // ---- GEMM1 -> cl in LDS (as the forward)
      for (int p0 = 0; p0 < PQ; p0 += 32) {
        const int p = p0 + x;
        const float* arow = qrow + (p < PQ ? p : PQ - 1) * dp + 4 * hi;
        for (int m = 0; m < PX; ++m) {
          const float* brow = irow + m * dp + 4 * hi;
          bf32x16 acc = {0};
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
      wave_lds_fence();

      // ---- pair gate, forward: gqi = W2 silu(W1 cl + b1) + b2
      bf32x16 out[TL];
#pragma unroll
      for (int v = 0; v < TL; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[v][r] = b2[32 * v + acc_row(r, hi)];
      for (int t = 0; t < TH; ++t) {
        bf32x16 h;
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = b1[32 * t + acc_row(r, hi)];
#pragma unroll 4
        for (int c = 0; c < Lp / 8; ++c) h = mfma4(w1g[(t * (Lp / 8) + c) * 64 + lane], cl4[(2 * c + hi) * 32 + x], h);
#pragma unroll
        for (int r = 0; r < 16; ++r) { float a, gr; silu_grad(h[r], a, gr); h[r] = a; }
#pragma unroll
        for (int v = 0; v < TL; ++v)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float4 hv = make_float4(h[4 * g], h[4 * g + 1], h[4 * g + 2], h[4 * g + 3]);
            out[v] = mfma4(w2g[((t * TL + v) * 4 + g) * 64 + lane], hv, out[v]);
          }
      }

      // (the lane's position, opaque to the optimiser from here to the gate's backward: the per-group LDS slots and compares are
      // then formed in place from one base instead of being hoisted, one register each, out of the tile loop)
      int xs = x, his = hi;
      asm volatile("" : "+v"(xs), "+v"(his));
      // ---- combine: w and silu'(g); this lane holds logits l = 32 v + 8 g + 4 hi + j of item x, and slot (8 v + 2 g + his) * 32 + xs of dg4
      float mx = -INFINITY;
#pragma unroll
      for (int v = 0; v < TL; ++v)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int l0 = 32 * v + 8 * g + 4 * his;
          const int lc = l0 < Lq_t ? l0 : 0;
          const float4 q4 = *reinterpret_cast<const float4*>(gq + lc);
          const float4 i4 = *reinterpret_cast<const float4*>(gi + lc);
          const float qv[4] = {q4.x, q4.y, q4.z, q4.w}, iv[4] = {i4.x, i4.y, i4.z, i4.w};
          float sg[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float gqi = out[v][4 * g + j];
            float w;
            if (k.combine_none) { w = (qv[j] + iv[j]) + gqi; sg[j] = 1.0f; }
            else silu_grad(__builtin_fmaf(qv[j], iv[j], gqi), w, sg[j]);
            out[v][4 * g + j] = w;
            if (l0 + j < L) mx = fmaxf(mx, w);
          }
          dg4[(8 * v + 2 * g + his) * 32 + xs] = make_float4(sg[0], sg[1], sg[2], sg[3]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float den = 0.0f, num = 0.0f;
#pragma unroll
      for (int v = 0; v < TL; ++v)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int l0 = 32 * v + 8 * g + 4 * his;
          const float4 c4 = cl4[(8 * v + 2 * g + his) * 32 + xs];
          const float cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float e = l0 + j < L ? expf(out[v][4 * g + j] - mx) : 0.0f;
            out[v][4 * g + j] = e;
            den += e;
            num = __builtin_fmaf(e, cv[j], num);
          }
        }
      den += __shfl_xor(den, 32, 64);
      num += __shfl_xor(num, 32, 64);
      const float rden = 1.0f / den;
      const float s = dyv * (num * rden);                     // sum_l pi dpi = dY y

      // ---- dw, dg (to LDS), dgi (stored), dgq (accumulated); out becomes the direct term dY pi of dcl
#pragma unroll
      for (int v = 0; v < TL; ++v)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int l0 = 32 * v + 8 * g + 4 * his;
          const int lc = l0 < Lq_t ? l0 : 0;
          const int slot = (8 * v + 2 * g + his) * 32 + xs;
          const float4 q4 = *reinterpret_cast<const float4*>(gq + lc);
          const float4 i4 = *reinterpret_cast<const float4*>(gi + lc);
          const float4 c4 = cl4[slot];
          const float4 s4 = dg4[slot];
          const float qv[4] = {q4.x, q4.y, q4.z, q4.w}, iv[4] = {i4.x, i4.y, i4.z, i4.w};
          const float cv[4] = {c4.x, c4.y, c4.z, c4.w}, sv[4] = {s4.x, s4.y, s4.z, s4.w};
          float dgv[4], dgiv[4], acc4[4];
          if constexpr (kLdsAcc) {
            const float4 a4 = dgq4[slot];
            acc4[0] = a4.x; acc4[1] = a4.y; acc4[2] = a4.z; acc4[3] = a4.w;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc4[j] = dgq[v][4 * g + j];
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float pi = out[v][4 * g + j] * rden;
            const float dw = pi * (dyv * cv[j] - s);
            const float dg = dw * sv[j];
            dgv[j] = dg;
            if (k.combine_none) { dgiv[j] = dg; acc4[j] += dg; }
            else { dgiv[j] = dg * qv[j]; acc4[j] = __builtin_fmaf(dg, iv[j], acc4[j]); }
            out[v][4 * g + j] = dyv * pi;
          }
          if constexpr (kLdsAcc) {
            dgq4[slot] = make_float4(acc4[0], acc4[1], acc4[2], acc4[3]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) dgq[v][4 * g + j] = acc4[j];
          }
          const float4 dg_4 = make_float4(dgv[0], dgv[1], dgv[2], dgv[3]);
          dg4[slot] = dg_4;
          if (k.d_ipack && valid && l0 < Lq_t)
            *reinterpret_cast<float4*>(k.d_ipack + row * k.item_floats + PX * dp + l0) = make_float4(dgiv[0], dgiv[1], dgiv[2], dgiv[3]);
          if (want_w) {
            *reinterpret_cast<float4*>(k.ws_dg + wsrow * Lp + l0) = dg_4;
            *reinterpret_cast<float4*>(k.ws_cl + wsrow * Lp + l0) = c4;
          }
        }
      wave_lds_fence();

      // ---- pair gate, backward, per hidden block: h again, da = W2^T dg, dh = da silu'(h), dcl += W1^T dh
      for (int t = 0; t < TH; ++t) {
        bf32x16 h, da = {0};
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = b1[32 * t + acc_row(r, hi)];
#pragma unroll 4
        for (int c = 0; c < Lp / 8; ++c) h = mfma4(w1g[(t * (Lp / 8) + c) * 64 + lane], cl4[(2 * c + hi) * 32 + x], h);
#pragma unroll 4
        for (int c = 0; c < Lp / 8; ++c) da = mfma4(w2tg[(t * (Lp / 8) + c) * 64 + lane], dg4[(2 * c + hi) * 32 + x], da);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float a, gr;
          silu_grad(h[r], a, gr);
          h[r] = a;
          da[r] = da[r] * gr;                                  // dh
        }
        if (want_w) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int64_t at = wsrow * Hp + 32 * t + 8 * g + 4 * hi;
            *reinterpret_cast<float4*>(k.ws_a + at) = make_float4(h[4 * g], h[4 * g + 1], h[4 * g + 2], h[4 * g + 3]);
            *reinterpret_cast<float4*>(k.ws_dh + at) = make_float4(da[4 * g], da[4 * g + 1], da[4 * g + 2], da[4 * g + 3]);
          }
        }
#pragma unroll
        for (int v = 0; v < TL; ++v)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float4 dv = make_float4(da[4 * g], da[4 * g + 1], da[4 * g + 2], da[4 * g + 3]);
            out[v] = mfma4(w1tg[((t * TL + v) * 4 + g) * 64 + lane], dv, out[v]);
          }
      }

      // ---- dcl -> LDS (every lane its own slots), then the two products with the component embeddings
      wave_lds_fence();
#pragma unroll
      for (int v = 0; v < TL; ++v)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          dg4[(8 * v + 2 * g + hi) * 32 + x] = make_float4(out[v][4 * g], out[v][4 * g + 1], out[v][4 * g + 2], out[v][4 * g + 3]);
      wave_lds_fence();

      if (k.d_ipack) {
        // dEx[x][m][kk] = sum_p dcl[p PX + m][x] (Eq[p][kk] / tau): rows kk, columns x, two p per MFMA
        float* drow = k.d_ipack + row * k.item_floats;
        for (int m = 0; m < PX; ++m)
          for (int kb = 0; kb < dp; kb += 32) {
            bf32x16 acc = {0};
            for (int p0 = 0; p0 < PQ; p0 += 2) {
              const int p = p0 + hi;
              const bool in = p < PQ;
              const float av = in && kb + x < dp ? qrow[p * dp + kb + x] : 0.0f;
              const float bv = in ? dgb[cl_at(p * PX + m, x)] : 0.0f;
              acc = mfma1(av, bv, acc);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int kk = kb + 8 * g + 4 * hi;              // dp is a multiple of 8: the float4 is inside the group or past it
              if (valid && kk < dp)
                *reinterpret_cast<float4*>(drow + m * dp + kk) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
            }
          }
      }
      if (k.d_qpack) {
        // dEq[p][kk] += sum_m sum_x dcl[p PX + m][x] Ex[x][m][kk]: rows p, columns kk, two items per MFMA
        const int64_t last = k.X - 1 - tile * 32;              // the tile's last real slot (>= 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (i < k.nq) {
            const int pb = i / k.nkb, kb = 32 * (i - pb * k.nkb);
            const int p = 32 * pb + x;
            bf32x16 acc;
            if constexpr (kLdsAcc) {
#pragma unroll
              for (int r = 0; r < 16; ++r) acc[r] = dqb[i * 1024 + r * 64 + lane];
            } else {
              acc = dq[i];
            }
            for (int m = 0; m < PX; ++m)
              for (int s2 = 0; s2 < 32; s2 += 2) {
                const int xx = s2 + hi;
                const int64_t r2 = (int64_t)b * k.X + tile * 32 + (xx < last ? xx : last);
                const float av = p < PQ ? dgb[cl_at(p * PX + m, xx)] : 0.0f;
                const float bv = kb + x < dp ? k.ipack[r2 * k.item_floats + m * dp + kb + x] : 0.0f;
                acc = mfma1(av, bv, acc);
              }
            if constexpr (kLdsAcc) {
#pragma unroll
              for (int r = 0; r < 16; ++r) dqb[i * 1024 + r * 64 + lane] = acc[r];
            } else {
              dq[i] = acc;
            }
          }
        }
      }
      wave_lds_fence();   // the next tile's GEMM1 and combine overwrite both buffers
    }

    if (k.d_qpack) {
      // the row's sums: over the lanes (dgq), then over the waves in ascending order
      __syncthreads();                                         // every wave is done with its buffers
      float* red = smem + wave * k.wave_floats;
      if constexpr (!kLdsAcc) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < k.nq)
#pragma unroll
            for (int r = 0; r < 16; ++r) red[k.dq_off + i * 1024 + r * 64 + lane] = dq[i][r];
      }
#pragma unroll
      for (int v = 0; v < TL; ++v)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float val[4];
          if constexpr (kLdsAcc) {
            const float4 a4 = dgq4[(8 * v + 2 * g + hi) * 32 + x];
            val[0] = a4.x; val[1] = a4.y; val[2] = a4.z; val[3] = a4.w;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) val[j] = dgq[v][4 * g + j];
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float t = val[j];
            t += __shfl_xor(t, 1, 64);
            t += __shfl_xor(t, 2, 64);
            t += __shfl_xor(t, 4, 64);
            t += __shfl_xor(t, 8, 64);
            t += __shfl_xor(t, 16, 64);
            if (x == 0) red[k.vec_off + 32 * v + 8 * g + 4 * hi + j] = t;   // (cl is free: the row's tiles are done)
          }
        }
      __syncthreads();
      float* dqrow = k.d_qpack + (int64_t)b * k.query_floats;
      for (int idx = threadIdx.x; idx < k.nq * 1024; idx += blockDim.x) {
        const int i = idx >> 10, r = (idx >> 6) & 15, ln = idx & 63;
        const int pb = i / k.nkb, kb = 32 * (i - pb * k.nkb);
        const int p = 32 * pb + acc_row(r, ln >> 5), kk = kb + (ln & 31);
        if (p < PQ && kk < dp) {
          float sum = 0.0f;
          for (int w = 0; w < nw; ++w) sum += smem[w * k.wave_floats + k.dq_off + idx];
          dqrow[p * dp + kk] = sum * k.inv_tau;
        }
      }
      for (int l = threadIdx.x; l < k.Lq; l += blockDim.x) {
        float sum = 0.0f;
        for (int w = 0; w < nw; ++w) sum += smem[w * k.wave_floats + k.vec_off + l];
        dqrow[PQ * dp + l] = sum;
      }
      __syncthreads();                                         // the next row zeroes the buffers
    }
  }
}

// ---- weight gradients: contraction of a chunk of the workspace over its pairs ---------------------------------------------
constexpr int kBwdSplitPairs = 256;     // a fixed run of pairs per partial: the partition does not depend on the grid or the device

struct ContractArgs {
  const float *cl, *a, *dh, *dg;
  float* part;
  int64_t np;                           // pairs of the chunk, a multiple of 32
  int Lp, Hp, TH, TLt;
};

// tiles: TH * TLt of dW1 (rows h, columns l), TLt * TH of dW2 (rows l, columns h), TH of db1, TLt of db2 (every column the same sum)
__global__ __launch_bounds__(64) void mol_generic_bwd_contract_kernel(ContractArgs k) {
  const int lane = threadIdx.x, x = lane & 31, hi = lane >> 5;
  const int tile = blockIdx.x, nW = k.TH * k.TLt, ntile = gridDim.x;
  const float *A, *Bm = nullptr;
  int lda, ldb = 0, ao, bo = 0;
  if (tile < nW) { A = k.dh; lda = k.Hp; ao = 32 * (tile / k.TLt); Bm = k.cl; ldb = k.Lp; bo = 32 * (tile % k.TLt); }
  else if (tile < 2 * nW) { const int q = tile - nW; A = k.dg; lda = k.Lp; ao = 32 * (q / k.TH); Bm = k.a; ldb = k.Hp; bo = 32 * (q % k.TH); }
  else if (tile < 2 * nW + k.TH) { A = k.dh; lda = k.Hp; ao = 32 * (tile - 2 * nW); }
  else { A = k.dg; lda = k.Lp; ao = 32 * (tile - 2 * nW - k.TH); }
  const int64_t p0 = (int64_t)blockIdx.y * kBwdSplitPairs;
  const int64_t p1 = p0 + kBwdSplitPairs < k.np ? p0 + kBwdSplitPairs : k.np;
  bf32x16 acc = {0};
  for (int64_t p = p0; p < p1; p += 2) {
    const int64_t pr = p + hi;
    const float av = A[pr * lda + ao + x];
    const float bv = Bm ? Bm[pr * ldb + bo + x] : 1.0f;
    acc = mfma1(av, bv, acc);
  }
  float* dst = k.part + ((int64_t)blockIdx.y * ntile + tile) * 1024;
#pragma unroll
  for (int r = 0; r < 16; ++r) dst[r * 64 + lane] = acc[r];
}

struct ReduceArgs {
  const float* part;
  float *dw1, *db1, *dw2, *db2;
  int L, H, TH, TLt, nk, accumulate;
};

// element (i, j) of a 32 x 32 accumulator tile: register (i & 3) + 4 (i >> 3) of lane j + 32 ((i >> 2) & 1)
__device__ __forceinline__ int tile_at(int i, int j) { return ((i & 3) + 4 * (i >> 3)) * 64 + j + 32 * ((i >> 2) & 1); }

__global__ void mol_generic_bwd_reduce_kernel(ReduceArgs k) {
  const int HL = k.H * k.L, total = 2 * HL + k.H + k.L, nW = k.TH * k.TLt, ntile = 2 * nW + k.TH + k.TLt;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    int tile, at;
    float* dst;
    if (e < HL) { const int h = e / k.L, l = e - h * k.L; tile = (h >> 5) * k.TLt + (l >> 5); at = tile_at(h & 31, l & 31); dst = k.dw1 + e; }
    else if (e < 2 * HL) { const int q = e - HL, l = q / k.H, h = q - l * k.H; tile = nW + (l >> 5) * k.TH + (h >> 5); at = tile_at(l & 31, h & 31); dst = k.dw2 + q; }
    else if (e < 2 * HL + k.H) { const int h = e - 2 * HL; tile = 2 * nW + (h >> 5); at = tile_at(h & 31, 0); dst = k.db1 + h; }
    else { const int l = e - 2 * HL - k.H; tile = 2 * nW + k.TH + (l >> 5); at = tile_at(l & 31, 0); dst = k.db2 + l; }
    float sum = 0.0f;
    for (int s = 0; s < k.nk; ++s) sum += k.part[((int64_t)s * ntile + tile) * 1024 + at];
    *dst = k.accumulate ? *dst + sum : sum;
  }
}

// W2^T in W1's A-operand order, then W1^T in W2's (mol_generic.hip mol_generic_pack_gate_kernel with the two matrices transposed and swapped):
// W2Tf[t][c][lane][j]    = W2[8 c + 4 (lane >> 5) + j][32 t + (lane & 31)]                     (t < TH, c < Lp / 8)
// W1Tf[t][v][g][lane][j] = W1[32 t + row(4 g + j, lane >> 5)][32 v + (lane & 31)]              (v < TL, g < 4)
__global__ void mol_generic_bwd_pack_gate_kernel(const float* __restrict__ w1, const float* __restrict__ w2, float* __restrict__ out, int L, int H,
                                               int Lp, int Hp) {
  const int TL = Lp / 32, HL = Hp * Lp;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * HL; i += gridDim.x * blockDim.x) {
    float v = 0.0f;
    if (i < HL) {
      const int j = i & 3, lane = (i >> 2) & 63, blk = i >> 8;
      const int c = blk % (Lp / 8), t = blk / (Lp / 8);
      const int hrow = 32 * t + (lane & 31), l = 8 * c + 4 * (lane >> 5) + j;
      if (hrow < H && l < L) v = w2[l * H + hrow];
    } else {
      const int q = i - HL;
      const int j = q & 3, lane = (q >> 2) & 63, blk = q >> 8;
      const int g = blk & 3, tv = (blk >> 2) % TL, t = (blk >> 2) / TL;
      const int l = 32 * tv + (lane & 31), hcol = 32 * t + acc_row(4 * g + j, lane >> 5);
      if (l < L && hcol < H) v = w1[hcol * L + l];
    }
    out[i] = v;
  }
}

constexpr size_t kBwdMaxLds = 160 * 1024;

template <int TL>
int launch_bwd(const BwdKernelArgs& k, int threads, size_t lds, int grid, hipStream_t stream) {
  static DynLdsOnce once;
  auto* fn = &mol_generic_bwd_kernel<TL>;
  if (ensure_dyn_lds(once, reinterpret_cast<const void*>(fn), (int)kBwdMaxLds) != kOk) return kErrLaunch;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(threads), lds, stream, k);
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int bwd_nq(const Shape& s) { return ((s.query_dot_product_groups + 31) / 32) * (gen_dp(s) / 32 + (gen_dp(s) % 32 ? 1 : 0)); }
int64_t bwd_tiles(const Shape& s) { const int64_t th = gen_hp(s) / 32, tl = gen_lp(s) / 32; return 2 * th * tl + th + tl; }
int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

}  // namespace

int generic_pack_gate_weights_t(const Shape& s, const Weights& w, float* wtpack, hipStream_t stream) {
  const int total = (int)gen_gate_pack_t_floats(s);
  hipLaunchKernelGGL(mol_generic_bwd_pack_gate_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, w.gqi_w1, w.gqi_w2, wtpack, num_logits(s),
                     s.gating_qi_hidden_dim, gen_lp(s), gen_hp(s));
  return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

bool generic_backward_supported(const Shape& s) {
  if (bwd_nq(s) > kGenericBwdMaxQTiles) {
    set_error("the generic route's backward keeps dEq in %d accumulator tiles of 32 x 32: ceil(P_Q / 32) * ceil(d / 32) <= %d, got %d",
              kGenericBwdMaxQTiles, kGenericBwdMaxQTiles, bwd_nq(s));
    return false;
  }
  return true;
}

// chunk_pairs pairs of cl, a, dh, dg rows, then the partials of the chunk's runs
size_t generic_backward_workspace_floats(const Shape& s, int64_t chunk_pairs) {
  const int64_t cp = round_up(chunk_pairs, kBwdSplitPairs);
  return (size_t)(cp * 2 * (gen_lp(s) + gen_hp(s)) + (cp / kBwdSplitPairs) * bwd_tiles(s) * 1024);
}

int generic_pair_backward(const Shape& s, const GenericBackwardArgs& a, int n_cu, hipStream_t stream) {
  if (!generic_backward_supported(s)) return kErrUnsupported;
  const int Lp = gen_lp(s), Hp = gen_hp(s), TL = Lp / 32;
  BwdKernelArgs k{};
  k.wpack = a.wpack; k.wtpack = a.wtpack; k.qpack = a.qpack; k.ipack = a.ipack; k.dy = a.dy; k.ld_dy = a.ld_dy;
  k.d_qpack = a.d_qpack; k.d_ipack = a.d_ipack;
  k.X = a.n_cand; k.xp32 = round_up(a.n_cand, 32);
  k.item_floats = gen_item_floats(s); k.query_floats = gen_query_floats(s);
  k.PQ = s.query_dot_product_groups; k.PX = s.item_dot_product_groups; k.dp = gen_dp(s); k.L = num_logits(s); k.Lq = gen_lq(s);
  k.TH = Hp / 32; k.combine_none = s.gating_combination == RAILS_COMBINE_NONE ? 1 : 0;
  k.nkb = (k.dp + 31) / 32; k.nq = bwd_nq(s);
  k.inv_tau = 1.0f / s.temperature;
  if (TL >= 4) {          // three cl-shaped buffers (cl; dg / dcl; the dgq accumulators), then the dEq tiles; the dgq row sums reuse cl
    k.wave_floats = 3 * Lp * 32 + k.nq * 1024; k.dq_off = 3 * Lp * 32; k.vec_off = 0;
  } else {                // two buffers; at the end of a row the dEq tiles and the dgq row sums are laid over them
    const int reduce_floats = k.nq * 1024 + Lp;
    k.wave_floats = 2 * Lp * 32 > reduce_floats ? 2 * Lp * 32 : reduce_floats; k.dq_off = 0; k.vec_off = k.nq * 1024;
  }
  const int fit = (int)(kBwdMaxLds / (sizeof(float) * k.wave_floats));
  const int waves = fit >= 4 ? 4 : fit;                          // 112 KB per wave at TL = 8 with four dEq tiles: one wave
  const size_t lds = sizeof(float) * (size_t)waves * k.wave_floats;
  const int per_cu = lds <= kBwdMaxLds / 2 ? 2 : 1;

  const bool want_w = a.dw1 != nullptr;
  const int64_t cp = round_up(a.chunk_pairs, kBwdSplitPairs);
  int64_t chunk_rows = a.B;
  float* part = nullptr;
  if (want_w) {
    if (k.xp32 > cp) {
      set_error("generic_pair_backward: a row of %lld candidates does not fit the weight-gradient chunk of %lld pairs", (long long)a.n_cand, (long long)cp);
      return kErrInvalid;
    }
    chunk_rows = cp / k.xp32;
    k.ws_cl = a.workspace; k.ws_dg = k.ws_cl + cp * Lp; k.ws_a = k.ws_dg + cp * Lp; k.ws_dh = k.ws_a + cp * Hp;
    part = k.ws_dh + cp * Hp;
  }
  for (int64_t r0 = 0; r0 < a.B; r0 += chunk_rows) {
    k.row0 = (int)r0;
    k.nrows = (int)(a.B - r0 < chunk_rows ? a.B - r0 : chunk_rows);
    const int64_t max_grid = (int64_t)n_cu * per_cu;
    const int grid = (int)(k.nrows < max_grid ? k.nrows : max_grid);
    int r = kErrUnsupported;
    switch (TL) {
      case 1: r = launch_bwd<1>(k, 64 * waves, lds, grid, stream); break;
      case 2: r = launch_bwd<2>(k, 64 * waves, lds, grid, stream); break;
      case 3: r = launch_bwd<3>(k, 64 * waves, lds, grid, stream); break;
      case 4: r = launch_bwd<4>(k, 64 * waves, lds, grid, stream); break;
      case 5: r = launch_bwd<5>(k, 64 * waves, lds, grid, stream); break;
      case 6: r = launch_bwd<6>(k, 64 * waves, lds, grid, stream); break;
      case 7: r = launch_bwd<7>(k, 64 * waves, lds, grid, stream); break;
      case 8: r = launch_bwd<8>(k, 64 * waves, lds, grid, stream); break;
    }
    if (r != kOk) return r;
    if (want_w) {
      ContractArgs c{};
      c.cl = k.ws_cl; c.a = k.ws_a; c.dh = k.ws_dh; c.dg = k.ws_dg; c.part = part;
      c.np = k.nrows * k.xp32; c.Lp = Lp; c.Hp = Hp; c.TH = Hp / 32; c.TLt = TL;
      const int nk = (int)((c.np + kBwdSplitPairs - 1) / kBwdSplitPairs);
      hipLaunchKernelGGL(mol_generic_bwd_contract_kernel, dim3((unsigned)bwd_tiles(s), (unsigned)nk), dim3(64), 0, stream, c);
      if (hipGetLastError() != hipSuccess) return kErrLaunch;
      ReduceArgs d{};
      d.part = part; d.dw1 = a.dw1; d.db1 = a.db1; d.dw2 = a.dw2; d.db2 = a.db2;
      d.L = k.L; d.H = s.gating_qi_hidden_dim; d.TH = Hp / 32; d.TLt = TL; d.nk = nk; d.accumulate = r0 > 0 ? 1 : 0;
      const int total = 2 * d.H * d.L + d.H + d.L;
      hipLaunchKernelGGL(mol_generic_bwd_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, d);
      if (hipGetLastError() != hipSuccess) return kErrLaunch;
    }
  }
  return kOk;
}

}  // namespace mol
