"""Float64 restatement of the MoL hot path (oracle/mol_oracle.py steps 1-8), every function returning (value, per-element bound).

The bound is an a-priori bound on |fp32 kernel - exact value of the same operation on the same fp32 inputs|, built from float64
absolute sums with u = 2^-24 in the running-error style of tests/test_hstu_kernels_gpu.py.  Each stage takes the fp32 inputs the
kernel under test actually read, so one check covers one kernel:

  prologue64  q, user ids, fp32 weights                 -> Eq, gq   (mol_query.hip: per-query, split and batched routes)
  index64     X, fp32 weights                           -> Ex, gi   (mol_index.hip: index_build_kernel)
  score64     the engine's own plain Eq, Ex, gq, gi     -> logits   (every fp32 scoring shell: mol_score_fp32_unit.h,
              and the fp32 pair-gate weights                         mol_score_small.hip, mol_score_wsplit.h)
  gate_combine64, glu64                                             (rails_mol_gate_combine, rails_glu_f32)

Arithmetic model (rails_amd/f16x3_bound.py H1-H4): MFMA / fmaf chains of n terms lose at most gamma(n) of their absolute sum; exp2 and
rcp of the scoring kernels are within 1 ulp (2 u); expf is within 1 ulp, erff within 2 ulp, sqrtf and true divisions are correctly
rounded (the TUs are built without fast-math).  In the prologue, the index build and the stand-alone units, errors are carried forward
through silu / gelu with their Lipschitz constants and through the softmax with the mixture sensitivity of f16x3_bound.py.  The
scoring bound (score64) instead weights each intermediate's own rounding bound with the pair's exact sensitivity of the logit to it
(a float64 reverse pass): the |W|-summed worst case of the forward propagation is 100-1000 times the observed error once the gate
MLP's 64-256 logits and 128 hidden units are chained.

`mut` arguments apply the bug classes the CPU meta-tests of tests/test_mol_kernels_gpu.py check the bars against.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24
# Bound constants (each <= 8), one line of justification each:
C_DOT = 1.01    # fmaf / MFMA chain of n terms: |err| <= C_DOT u (n + k) sum|terms|, gamma_n <= 1.01 n u (fp32 MFMA is a chain of round-to-
                # nearest fmaf, f16x3_bound.py H1); k counts the other roundings of the value: 1 for the bias add of a dense layer, 3 in the
                # scoring GEMMs for the packs (Eq / tau; -log2e W1, -log2e b1; prescaled b2) and the bias
C_SUM = 1.01    # plain VALU sums of n terms: gamma_n <= 1.01 n u while n u <= 0.01 (Higham, Lemma 3.1)
C_FAST = 2.0    # v_exp_f32 / v_rcp_f32 (pk_sigmoid_arg, the softmax exp2): 1 ulp = 2 u relative each (f16x3_bound.py H3)
C_SILU = 2.0    # t * rcp(1 + exp2(t)): exp2 and rcp 2 u each, three plain roundings and the rounded argument (u |t|): rel <= C_SILU u (4 + |z|)
C_EXPF = 4.0    # v / (1 + expf(-v)) (precise silu of the prologue / index build / gate_combine): expf 1 ulp (2 u), the add and the division
C_ERF = 6.0     # 1 + erff(z / sqrt 2): erff 2 ulp (<= 2 u absolute, |erf| <= 1) plus the add (2 u absolute, result < 2), with margin
C_NORM = 4.0    # sqrtf, the division by the clamped norm and the final rounding: relative error <= C_NORM u of the normalised value
C_MIX = 8.0     # the mixture's rcp(den), num * rden, den * rden, the renormalising division and the two lane-half additions: <= 8 u relative
SILU_LIP = 1.1  # sup |silu'| = 1.0998 (f16x3_bound.py LIP)
GELU_LIP = 1.13  # sup |gelu'| = 1.1289
LN2 = math.log(2.0)
TINY = 1e-30    # absolute floor: flushed subnormals and exp2 underflow to 0 (H4)
C_LIN = 0.05    # score64's first-order propagation: margin for the second-order remainder (|dw|^2 spread, products of two roundings)


def f32(x: float) -> float:
    """The fp32 value of a Python float (what the kernels read for temperature / eps)."""
    return float(np.float32(x))


def _d(t):
    return t.detach().to("cpu", torch.float64)


# ----------------------------------------------------------------------------------------------------------------------------
# elementwise pieces
# ----------------------------------------------------------------------------------------------------------------------------
def linear64(x, ex, W, b, nk=True):
    """x @ W^T + b (nk: W is (N, K), a torch Linear weight) or x @ W + b (W is (K, N), a GLU `_w`): an fmaf chain of K terms per output,
    then the bias added (one more rounding) -- the prologue's and the index build's dense layers and the fp32 GEMM of rails_glu_f32."""
    W = _d(W)
    Wt = W.T if nk else W
    K = Wt.shape[0]
    y = x @ Wt
    yabs = x.abs() @ Wt.abs()
    if b is not None:
        b = _d(b).reshape(-1)
        y, yabs = y + b, yabs + b.abs()
    e = C_DOT * U * (K + 1) * yabs
    if ex is not None:
        e = e + ex @ Wt.abs()
    return y, e


def silu_precise64(z, ez):
    s = z * torch.sigmoid(z)
    return s, SILU_LIP * ez + C_EXPF * U * s.abs() + TINY


def silu_fast64(z, ez):
    s = z * torch.sigmoid(z)
    return s, SILU_LIP * ez + C_SILU * U * (4 + z.abs()) * s.abs() + TINY


def gelu64(z, ez, tanh=False):
    if tanh:   # mutation: the tanh approximation instead of erf
        g = 0.5 * z * (1 + torch.tanh(math.sqrt(2 / math.pi) * (z + 0.044715 * z ** 3)))
    else:
        g = 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))
    return g, GELU_LIP * ez + 0.5 * z.abs() * U * (C_ERF + 1.2 * z.abs()) + 2 * U * g.abs() + TINY


def glu64(x, ex, W, b, kind, mut=None):
    """act(x W_l + b_l) * (x W_r + b_r), W the (K, 2F) `_w` (rails/similarities/layers.py:36-43, :66-73)."""
    pre, epre = linear64(x, ex, W, b, nk=False)
    F = pre.shape[-1] // 2
    l, r, el, er = pre[..., :F], pre[..., F:], epre[..., :F], epre[..., F:]
    a, ea = gelu64(l, el, tanh=(mut == "tanh_gelu")) if kind == "geglu" else silu_precise64(l, el)
    h = a * r
    return h, ea * r.abs() + a.abs() * er + ea * er + U * h.abs()


def l2norm64(y, ey, eps, on=True, mut=None):
    """y / clamp(||y||, min=eps) over the last axis; the kernels: an fmaf chain of the d squares, fmaxf(sqrtf(ss), eps), a true division.
    mut: "clamp_sq" (sqrt(max(ss, eps))), "rsqrt_eps" (y * rsqrt(ss + eps))."""
    if not on:
        return y, ey
    d = y.shape[-1]
    ss = (y * y).sum(-1, keepdim=True)
    n = ss.sqrt()
    if mut == "clamp_sq":
        m = torch.clamp(ss, min=eps).sqrt()
    elif mut == "rsqrt_eps":
        m = (ss + eps).sqrt()
    else:
        m = torch.clamp(n, min=eps)
    val = y / m
    dm = (ey * ey).sum(-1, keepdim=True).sqrt() + n * U * (0.5 * C_SUM * (d + 1) + 1)   # the clamp is 1-Lipschitz
    room = m - dm
    e = torch.where(room > 0, ey / m + y.abs() * dm / (m * room.clamp(min=1e-300)), torch.full_like(val, math.inf)) + C_NORM * U * val.abs()
    return val, e


# ----------------------------------------------------------------------------------------------------------------------------
# steps 1 / 4: the query prologue
# ----------------------------------------------------------------------------------------------------------------------------
def prologue64(cfg, w, q, user_ids=None, mut=None):
    """-> ((Eq, bound) (B, P_Q, d), (gq, bound) (B, L)) from the fp32 q and weights (query_embeddings_fns.py:175-254, similarity_utils.py:153-168)."""
    q = _d(q)
    B = q.shape[0]
    pre = "_query_embeddings_fn._query_emb_proj_module."
    n_uid = len(cfg.uid_embedding_hash_sizes)
    G, d = cfg.query_dot_product_groups - n_uid, cfg.dot_product_dimension
    if cfg.query_hidden_dim > 0:
        h, eh = glu64(q, None, w[pre + "1._w"], w[pre + "1._b"], cfg.query_nonlinearity, mut)
        proj, ep = linear64(h, eh, w[pre + "2.weight"], w[pre + "2.bias"])
    else:
        proj, ep = linear64(q, None, w[pre + "1.weight"], w[pre + "1.bias"])
    proj, ep = proj.reshape(B, G, d), ep.reshape(B, G, d)
    if n_uid:
        parts, eparts = [proj], [ep]
        for i, hs in enumerate(cfg.uid_embedding_hash_sizes):
            rows = _d(w[f"_query_embeddings_fn._uid_embeddings_{i}.weight"])[(torch.as_tensor(user_ids).cpu() % hs) + 1]
            parts.append(rows.unsqueeze(1))
            eparts.append(torch.zeros_like(rows).unsqueeze(1))
        proj, ep = torch.cat(parts, 1), torch.cat(eparts, 1)
    eq = l2norm64(proj, ep, f32(cfg.eps), cfg.dot_product_l2_norm, mut)
    L = cfg.num_logits
    if not cfg.gating_query_fn:
        return eq, (torch.zeros(B, L, dtype=torch.float64), torch.zeros(B, L, dtype=torch.float64))
    g = "_gating_fn._query_only_partial_module."
    z, ez = linear64(q, None, w[g + "0.weight"], w[g + "0.bias"])
    hq, ehq = silu_precise64(z, ez)
    return eq, linear64(hq, ehq, w[g + "2.weight"], None)


# ----------------------------------------------------------------------------------------------------------------------------
# steps 2 / 3: the index build
# ----------------------------------------------------------------------------------------------------------------------------
def index64(cfg, w, X, mut=None):
    """-> ((Ex, bound) (N, P_X, d), (gi, bound) (N, L)) from the fp32 items and weights (item_embeddings_fns.py:149-183,
    similarity_utils.py:169-185)."""
    X = _d(X)
    N = X.shape[0]
    pre = "_item_embeddings_fn._item_emb_proj_module."
    if cfg.item_hidden_dim > 0:
        h, eh = glu64(X, None, w[pre + "1._w"], w[pre + "1._b"], cfg.item_nonlinearity, mut)
        proj, ep = linear64(h, eh, w[pre + "2.weight"], w[pre + "2.bias"])
    else:
        proj, ep = linear64(X, None, w[pre + "1.weight"], w[pre + "1.bias"])
    shp = (N, cfg.item_dot_product_groups, cfg.dot_product_dimension)
    ex = l2norm64(proj.reshape(shp), ep.reshape(shp), f32(cfg.eps), cfg.dot_product_l2_norm, mut)
    L = cfg.num_logits
    if not cfg.gating_item_fn:
        return ex, (torch.zeros(N, L, dtype=torch.float64), torch.zeros(N, L, dtype=torch.float64))
    g = "_gating_fn._item_only_partial_module."
    z, ez = linear64(X, None, w[g + "1.weight"], w[g + "1.bias"])
    hi, ehi = silu_precise64(z, ez)
    return ex, linear64(hi, ehi, w[g + "3.weight"], None)


# ----------------------------------------------------------------------------------------------------------------------------
# steps 5-8: the fused scoring kernels
# ----------------------------------------------------------------------------------------------------------------------------
def _dsilu(z):
    sg = torch.sigmoid(z)
    return sg * (1 + z * (1 - sg))


def score64(cfg, w, Eq, Ex, gq, gi, mut=None):
    """Logits of the fp32 scoring kernels from the operands they read.  Eq (B, P_Q, d), gq (B, L); Ex (N, P_X, d), gi (N, L) for a shared
    corpus or (B, N, P_X, d), (B, N, L) for per-row candidates.  -> (B, N) logits and bounds.
    mut: "no_b2" (pair-gate output bias dropped), "silu_gqgi" (w = silu(gq gi) + gqi).

    The bound propagates each stage's own rounding bound with the pair's EXACT sensitivities (a reverse pass through the mixture, the
    combination and the gate MLP in float64), instead of carrying |W|-summed worst cases from layer to layer:
        |out - f(...)| <= (1 + C_LIN) sum_stages sum_i |d out / d x_i| e_i  +  (rounding of the softmax / mixture itself),
    e_i the rounding bound of intermediate x_i from its own inputs (chains: C_DOT u (n + 3) sum|terms|; silu: C_SILU u (4 + |z|) |silu|).
    This is first-order in u: the second-order remainder is below C_LIN of the first-order term while every |dw| stays below 1e-3."""
    Eq, Ex, gq, gi = _d(Eq), _d(Ex), _d(gq), _d(gi)
    B, PQ, d = Eq.shape
    tau = f32(cfg.temperature)
    if Ex.dim() == 3:
        cl = torch.einsum("bpd,nmd->bnpm", Eq, Ex)
        clabs = torch.einsum("bpd,nmd->bnpm", Eq.abs(), Ex.abs())
        gi = gi.unsqueeze(0)
    else:
        cl = torch.einsum("bpd,bnmd->bnpm", Eq, Ex)
        clabs = torch.einsum("bpd,bnmd->bnpm", Eq.abs(), Ex.abs())
    N = cl.shape[1]
    L = cfg.num_logits
    cl, clabs = cl.reshape(B, N, L) / tau, clabs.reshape(B, N, L) / tau
    ecl = C_DOT * U * (d + 3) * clabs                     # GEMM1 chain (d / 2 K-steps of two products) + the Eq / tau pack
    p = "_gating_fn._qi_partial_module."
    H = cfg.gating_qi_hidden_dim
    W1, b1 = _d(w[p + "1.weight"]), _d(w[p + "1.bias"])
    if H > 0:
        W2, b2 = _d(w[p + "3.weight"]), _d(w[p + "3.bias"])
        if mut == "no_b2":
            b2 = torch.zeros_like(b2)
        pre = cl @ W1.T + b1
        epre = C_DOT * U * (L + 3) * (cl.abs() @ W1.abs().T + b1.abs())      # GEMM2 chain + the -log2e W1 / b1 packs
        hid = pre * torch.sigmoid(pre)
        ehid = C_SILU * U * (4 + pre.abs()) * hid.abs() + TINY
        gqi = hid @ W2.T + b2
        egqi = C_DOT * U * (H + 3) * (hid.abs() @ W2.abs().T + b2.abs())     # GEMM3 chain + the prescaled b2
    else:   # one Linear(L, L): its weights in the W1 slot, its bias in the b2 slot
        if mut == "no_b2":
            b1 = torch.zeros_like(b1)
        gqi = cl @ W1.T + b1
        egqi = C_DOT * U * (L + 3) * (cl.abs() @ W1.abs().T + b1.abs())
    gq = gq.unsqueeze(1)
    none = cfg.gating_combination_type == "none"
    if none:
        g = gq + gi + gqi
        eg = C_DOT * U * 3 * (gq.abs() + gi.abs() + gqi.abs())
        wv, ew = g, torch.zeros_like(g)
    else:
        a = gq * gi
        g = a + gqi
        eg = C_DOT * U * 3 * (a.abs() + gqi.abs())        # the -log2e gq pack and the fma
        wv = g * torch.sigmoid(g)
        ew = C_SILU * U * (4 + g.abs()) * wv.abs() + TINY
        if mut == "silu_gqgi":
            wv = a * torch.sigmoid(a) + gqi
    pi = torch.softmax(wv, -1)
    out = (pi * cl).sum(-1)
    dev_c = (cl - out.unsqueeze(-1)).abs()
    # reverse pass: d out / d w_l = pi_l (cl_l - out); through w = silu(g), gqi = W2 hid + b2, hid = silu(pre), pre = W1 cl + b1
    s_w = pi * (cl - out.unsqueeze(-1))
    s_g = s_w if none else s_w * _dsilu(g)
    if H > 0:
        s_hid = s_g @ W2
        s_pre = s_hid * _dsilu(pre)
        s_cl = pi + s_pre @ W1
        lin = (s_pre.abs() * epre).sum(-1) + (s_hid.abs() * ehid).sum(-1)
    else:
        s_cl = pi + s_g @ W1
        lin = torch.zeros_like(out)
    lin = lin + (s_cl.abs() * ecl).sum(-1) + (s_g.abs() * (egqi + eg)).sum(-1) + (s_w.abs() * ew).sum(-1)
    # the softmax itself: exp2 of the rounded exponent (2 u + |d| ln2 u relative per term), the num / den sums, the final divisions
    dexp = math.log2(math.e) * (wv.amax(-1, keepdim=True) - wv)
    mix = (pi * U * (C_FAST + LN2 * dexp + 1) * dev_c).sum(-1) + U * (C_SUM * (L + 2) + C_MIX) * (pi * cl.abs()).sum(-1)
    return out, (1 + C_LIN) * (lin + mix) + TINY


# ----------------------------------------------------------------------------------------------------------------------------
# the stand-alone units
# ----------------------------------------------------------------------------------------------------------------------------
def gate_combine64(y, gqi, gq, gi, X, per_row, glu_silu, renorm, eps):
    """rails_mol_gate_combine (hstu.hip gate_combine_kernel: precise expf, true divisions, a 64-lane fmaf + butterfly mixture).
    y, gqi (rows, L); gq (rows / X, L); gi (X or rows, L); absent parts None."""
    y = _d(y)
    rows, L = y.shape
    b = torch.arange(rows) // X
    parts = []
    if gq is not None:
        parts.append(_d(gq)[b])
    if gi is not None:
        parts.append(_d(gi) if per_row else _d(gi)[torch.arange(rows) % X])
    if gqi is not None:
        parts.append(_d(gqi))
    if glu_silu:
        a = parts[0] * parts[1]
        g = a + parts[2]
        wv, ew = silu_precise64(g, 2 * U * (a.abs() + g.abs()))
    else:
        wv = sum(parts)
        ew = C_SUM * U * len(parts) * sum(t.abs() for t in parts)
    pi = torch.softmax(wv, -1)
    out = (pi * y).sum(-1)
    spread = y.amax(-1) - y.amin(-1)
    dw = ew.amax(-1)
    # expf of (w - max w): 1 ulp plus the rounded argument (u |w - max w| relative); den and sum pi: L-term sums (L / 64 per lane,
    # then a 6-level butterfly); the divisions by den and by the renormalising sum; the fmaf mixture chain of the same depth
    eps_l = U * (C_FAST + (wv.amax(-1, keepdim=True) - wv) + 1)
    dev = (pi * eps_l * (y - out.unsqueeze(-1)).abs()).sum(-1)
    depth = -(-L // 64) + 6
    sums = U * (3 * C_SUM * (depth + 1) + C_MIX) * (pi * y.abs()).sum(-1)
    bound = 1.01 * (dw * spread / 2 * (1 + 2 * dw) + dev) + sums + TINY
    # renormalise: pi / clamp(sum pi, eps) with sum pi = 1 in exact arithmetic -- the identity unless eps > 1, which divides by eps
    # (exactly, for a power of two); the rounded sum and division when the clamp is not taken are in `sums`
    scale = 1.0 / max(1.0, f32(eps)) if renorm else 1.0
    return out * scale, bound * scale


def glu_f32_64(x, W, b, kind):
    """rails_glu_f32: the fp32 GEMM of the pre-activations (K + 2 chain) then act(l) * r."""
    return glu64(_d(x), None, W, b, kind)
