"""References of the differentiable MoLSimilarity.forward.

  stages(cfg, w, q, items, user_ids)   the eval-mode forward of the reference (oracle/mol_oracle.py steps 1-8) as differentiable torch
                                       operations in the dtype of its inputs -- the oracle detaches its inputs and cannot serve
  pair_stage(...)                      steps 5-8 alone, on the pair stage's own inputs (Eq / tau, gq, Ex, gi, pair-gate weights)
  pair_backward64(...)                 numpy analytic backward of the pair stage (float64: the reference; float32: the yardstick of the
                                       per-tensor check); for every output element also A, the same chain with every addend at its
                                       absolute value, n, the number of addends along its nested sums, and F, the absolute error of
                                       the chain-valued factors -- the fp32 kernel is held to 2^-24 ((n + C) A + F) per element
                                       (grad_bound) and per tensor to 8 x the relative L2 error of the float32 chain

`mut` applies the bug classes the CPU meta-tests check the bound against.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
MUTANTS = ("drop_w1t", "drop_sum", "sigmoid_for_silu_grad", "forget_tau", "swap_perm", "forget_db1", "gq_for_gi")


def _glu(x, w, b, kind):
    out = w.shape[1] // 2
    lhs, rhs = torch.split(torch.mm(x, w) + b, [out, out], dim=-1)
    return (F.gelu(lhs) if kind == "geglu" else F.silu(lhs)) * rhs


def _l2norm(x, eps):
    return x / torch.clamp(torch.linalg.norm(x, dim=-1, keepdim=True), min=eps)


def pair_stage(cfg, eq, gq, ex, gi, w1, b1, w2, b2, temperature=None):
    """eq (B, P_Q, d), gq (B, L) or None, ex (B, X, P_X, d), gi (B, X, L) or None -> (B, X) logits.  temperature None: `eq` is Eq / tau
    already (what the kernels read); else the cross logits are divided by it, in the oracle's order of operations."""
    B, X = ex.shape[0], ex.shape[1]
    cl = torch.einsum("bnd,bxmd->bxnm", eq, ex).reshape(B, X, cfg.num_logits)
    if temperature is not None:
        cl = cl / temperature
    gqi = F.linear(F.silu(F.linear(cl, w1, b1)), w2, b2)
    if cfg.gating_combination_type == "glu_silu":
        g = gq.unsqueeze(1) * gi + gqi
        w = g * torch.sigmoid(g)
    else:
        one_sided = [t for t in (None if gq is None else gq.unsqueeze(1), gi) if t is not None]
        w = gqi if not one_sided else (one_sided[0] + gqi if len(one_sided) == 1 else one_sided[0] + one_sided[1] + gqi)
    pi = F.softmax(w, dim=-1)
    if temperature is None or cfg.softmax_dropout_rate > 0.0:
        pi = pi / torch.clamp(pi.sum(-1, keepdim=True), min=1e-6)
    return (pi * cl).sum(-1)


def upstream(cfg, w: Dict[str, torch.Tensor], q, items, user_ids=None):
    """Steps 1-4: q (B, D), items (B, X, D') -> Eq (B, P_Q, d), gq (B, L) | None, Ex (B, X, P_X, d), gi (B, X, L) | None."""
    d = cfg.dot_product_dimension
    pre = "_query_embeddings_fn._query_emb_proj_module."
    if cfg.query_hidden_dim > 0:
        proj = F.linear(_glu(q, w[pre + "1._w"], w[pre + "1._b"], cfg.query_nonlinearity), w[pre + "2.weight"], w[pre + "2.bias"])
    else:
        proj = F.linear(q, w[pre + "1.weight"], w[pre + "1.bias"])
    n_uid = len(cfg.uid_embedding_hash_sizes)
    eq = proj.reshape(q.shape[0], cfg.query_dot_product_groups - n_uid, d)
    if n_uid:
        embs = [F.embedding((user_ids % hs) + 1, w[f"_query_embeddings_fn._uid_embeddings_{i}.weight"]).unsqueeze(1)
                for i, hs in enumerate(cfg.uid_embedding_hash_sizes)]
        eq = torch.cat([eq] + embs, dim=1)
    pre = "_item_embeddings_fn._item_emb_proj_module."
    flat = items.reshape(-1, items.shape[-1])
    if cfg.item_hidden_dim > 0:
        proj = F.linear(_glu(flat, w[pre + "1._w"], w[pre + "1._b"], cfg.item_nonlinearity), w[pre + "2.weight"], w[pre + "2.bias"])
    else:
        proj = F.linear(flat, w[pre + "1.weight"], w[pre + "1.bias"])
    ex = proj.reshape(items.shape[:-1] + (cfg.item_dot_product_groups, d))
    if cfg.dot_product_l2_norm:
        eq, ex = _l2norm(eq, cfg.eps), _l2norm(ex, cfg.eps)
    gq = gi = None
    if cfg.gating_query_fn:
        g = "_gating_fn._query_only_partial_module."
        gq = F.linear(F.silu(F.linear(q, w[g + "0.weight"], w[g + "0.bias"])), w[g + "2.weight"])
    if cfg.gating_item_fn:
        g = "_gating_fn._item_only_partial_module."
        gi = F.linear(F.silu(F.linear(items, w[g + "1.weight"], w[g + "1.bias"])), w[g + "3.weight"])
    return eq, gq, ex, gi


def stages(cfg, w: Dict[str, torch.Tensor], q, items, user_ids=None):
    """The whole eval-mode forward on the per-row branch: q (B, D), items (B, X, D') -> (B, X) logits, differentiable, any float dtype."""
    eq, gq, ex, gi = upstream(cfg, w, q, items, user_ids)
    g = "_gating_fn._qi_partial_module."
    return pair_stage(cfg, eq, gq, ex, gi, w[g + "1.weight"], w[g + "1.bias"], w[g + "3.weight"], w[g + "3.bias"], temperature=cfg.temperature)


def to64(w: Dict[str, torch.Tensor], requires_grad: bool = False) -> Dict[str, torch.Tensor]:
    return {k: v.detach().to("cpu", torch.float64).requires_grad_(requires_grad and v.is_floating_point()) for k, v in w.items()}


# ----------------------------------------------------------------------------------------------------------------------------
# the analytic pair-stage backward
# ----------------------------------------------------------------------------------------------------------------------------
def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def pair_backward64(eqs, gq, ex, gi, w1, b1, w2, b2, dy, inv_tau: float, combine_none: bool, mut: Optional[str] = None, dtype=np.float64):
    """Gradients of sum(dy * logits) of the pair stage, analytically, in `dtype` (float64: the reference; float32: the same chain at the
    kernel's precision, the yardstick of the per-tensor check).  eqs (B, P_Q, d) is Eq / tau AS THE KERNEL READS IT; dEq is the gradient
    of the unscaled Eq (the product with inv_tau), as rails_mol_generic_pair_backward returns it.  gq / gi of an absent gate part are
    zeros.  -> {name: (value, A, n, F)} for dEq, dgq, dEx, dgi, dW1, db1, dW2, db2:
      A   the element's chain with every addend at its absolute value
      n   the number of addends along its nested sums
      F   (units of 2^-24) the absolute error that four factors carry into it.  a = silu(h), silu'(h), silu'(g) and cl are VALUES OF
          CHAINS with cancellation that enter a product directly; their rounding error is that of the chain -- (Lp + 1) S_h with S_h =
          |W1| |cl| + |b1| for h, (Hp + 2) S_g with S_g = |W2| |a| + |b2| + |gq gi| for g, (dp + 1) |Eq / tau| |Ex| for cl -- however small
          the value is: silu(h) near h = 0, silu' at its zero crossing -1.28.  No count of operations relative to the factor covers
          that, so it is added per element: e_a = 1.1 (Lp + 1) S_h (sup silu' = 1.1), e_ap = (Lp + 1) S_h / 2 and e_gp = (Hp + 2) S_g / 2
          (sup |silu''| = 1 / 2), e_cl; each multiplies the VALUE of its cofactor where it occurs (|dw| e_gp in dg, |dg| e_a in dW2,
          |da| e_ap in dh, |dh| e_cl in dW1) and is carried to the later outputs through the absolute values of the weights."""
    eqs, gq, ex, gi, w1, b1, w2, b2, dy = (np.asarray(t, dtype=dtype) for t in (eqs, gq, ex, gi, w1, b1, w2, b2, dy))
    inv_tau = dtype(inv_tau)
    B, PQ, d = eqs.shape
    X, PX = ex.shape[1], ex.shape[2]
    L, H = PQ * PX, w1.shape[0]
    one = dtype(1.0)
    cl = np.einsum("bpk,bxmk->bxpm", eqs, ex).reshape(B, X, L)
    h = cl @ w1.T + b1
    sh = one / (one + np.exp(-h))
    a = h * sh
    ap = sh if mut == "sigmoid_for_silu_grad" else sh * (one + h * (one - sh))
    gqi = a @ w2.T + b2
    gqb = gq[:, None, :]
    if combine_none:
        w = gqb + gi + gqi
        gp = np.ones_like(w)
    else:
        g = gqb * gi + gqi
        sg = one / (one + np.exp(-g))
        w = g * sg
        gp = sg if mut == "sigmoid_for_silu_grad" else sg * (one + g * (one - sg))
    e = np.exp(w - w.max(-1, keepdims=True))
    pi = e / e.sum(-1, keepdims=True)
    dp, Lp, Hp = (d + 7) // 8 * 8, (L + 31) // 32 * 32, (H + 31) // 32 * 32
    aw1, aw2 = np.abs(w1), np.abs(w2)
    s_h = np.abs(cl) @ aw1.T + np.abs(b1)
    e_a, e_ap = 1.1 * (Lp + 1) * s_h, 0.5 * (Lp + 1) * s_h
    e_cl = (dp + 1) * np.einsum("bpk,bxmk->bxpm", np.abs(eqs), np.abs(ex)).reshape(B, X, L)
    e_gp = np.zeros_like(w) if combine_none else 0.5 * (Hp + 2) * (np.abs(a) @ aw2.T + np.abs(b2) + np.abs(gqb * gi))
    dyb = dy[:, :, None]
    dpi, a_dpi = dyb * cl, np.abs(dyb * cl)
    sdot = (pi * dpi).sum(-1, keepdims=True)
    if mut == "drop_sum":
        sdot = 0 * sdot
    dw, a_dw = pi * (dpi - sdot), pi * (a_dpi + (pi * a_dpi).sum(-1, keepdims=True))
    n_dw = L + 3
    dg, a_dg, f_dg = dw * gp, a_dw * np.abs(gp), np.abs(dw) * e_gp
    n_dg = n_dw + 1
    out = {}
    if combine_none:
        out["dgq"] = (dg.sum(1), a_dg.sum(1), X + n_dg, f_dg.sum(1))
        out["dgi"] = (dg, a_dg, n_dg, f_dg)
    else:
        other = gqb if mut == "gq_for_gi" else gi
        out["dgq"] = ((dg * other).sum(1), (a_dg * np.abs(gi)).sum(1), X + n_dg + 1, (f_dg * np.abs(gi)).sum(1))
        out["dgi"] = (dg * gqb, a_dg * np.abs(gqb), n_dg + 1, f_dg * np.abs(gqb))
    out["db2"] = (dg.sum((0, 1)), a_dg.sum((0, 1)), B * X + n_dg, f_dg.sum((0, 1)))
    out["dW2"] = (np.einsum("bxl,bxh->lh", dg, a), np.einsum("bxl,bxh->lh", a_dg, np.abs(a)), B * X + n_dg + 1,
                  np.einsum("bxl,bxh->lh", f_dg, np.abs(a)) + np.einsum("bxl,bxh->lh", np.abs(dg), e_a))
    da, a_da, f_da = dg @ w2, a_dg @ aw2, f_dg @ aw2
    n_dh = L + n_dg + 1
    dh, a_dh, f_dh = da * ap, a_da * np.abs(ap), f_da * np.abs(ap) + np.abs(da) * e_ap
    db1 = dh.sum((0, 1))
    out["db1"] = (0 * db1 if mut == "forget_db1" else db1, a_dh.sum((0, 1)), B * X + n_dh, f_dh.sum((0, 1)))
    out["dW1"] = (np.einsum("bxh,bxl->hl", dh, cl), np.einsum("bxh,bxl->hl", a_dh, np.abs(cl)), B * X + n_dh + 1,
                  np.einsum("bxh,bxl->hl", f_dh, np.abs(cl)) + np.einsum("bxh,bxl->hl", np.abs(dh), e_cl))
    dcl, a_dcl = dyb * pi, np.abs(dyb) * pi
    if mut != "drop_w1t":
        dcl = dcl + dh @ w1
    a_dcl, f_dcl = a_dcl + a_dh @ aw1, f_dh @ aw1
    n_dcl = H + n_dh + 1
    shape = (B, X, PX, PQ) if mut == "swap_perm" else (B, X, PQ, PX)      # swap_perm: dcl read as [m][p] instead of [p][m]
    dclr, a_dclr, f_dclr = (t.reshape(shape).swapaxes(2, 3) if mut == "swap_perm" else t.reshape(shape) for t in (dcl, a_dcl, f_dcl))
    scale = one if mut == "forget_tau" else inv_tau
    out["dEq"] = (np.einsum("bxpm,bxmk->bpk", dclr, ex) * scale, np.einsum("bxpm,bxmk->bpk", a_dclr, np.abs(ex)) * inv_tau, X * PX + n_dcl + 1,
                  np.einsum("bxpm,bxmk->bpk", f_dclr, np.abs(ex)) * inv_tau)
    out["dEx"] = (np.einsum("bxpm,bpk->bxmk", dclr, eqs), np.einsum("bxpm,bpk->bxmk", a_dclr, np.abs(eqs)), PQ + n_dcl,
                  np.einsum("bxpm,bpk->bxmk", f_dclr, np.abs(eqs)))
    return out


def factor_roundings(PQ: int, PX: int, d: int, H: int) -> int:
    """C of the bound 2^-24 (n + C) A: the roundings of the factors of every addend, counted per stage of the
    recomputed forward and of the chain, each taken at unit gain:
      dp + 1   the GEMM1 chain over the zero-padded d and the pack's Eq / tau
      Lp + 1   the W1 chain over the zero-padded L and its bias
      Hp + 1   the W2 chain over the zero-padded H and its bias
      L + 5    the softmax: the subtraction of the maximum, expf (2), the denominator's chain, its reciprocal, the product
      24       silu and silu' of h and of g (expf 2, the add, the division, three products and two adds: 10 each), the fused g, dY cl,
               dY y (2), the difference, the two products of dw and dg"""
    dp, Lp, Hp = (d + 7) // 8 * 8, (PQ * PX + 31) // 32 * 32, (H + 31) // 32 * 32
    return (dp + 1) + (Lp + 1) + (Hp + 1) + (PQ * PX + 5) + 24


def grad_bound(A, n: int, C: int, F=0.0):
    """2^-24 ((n + C) A + F): the issue's bound on the plain A, plus the absolute errors of the chain-valued factors (pair_backward64)."""
    return U * ((n + C) * np.asarray(A, dtype=np.float64) + np.asarray(F, dtype=np.float64))


def rel_l2(v, ref) -> float:
    v, ref = np.asarray(v, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(v - ref) / max(float(np.linalg.norm(ref)), 1e-300))


# ----------------------------------------------------------------------------------------------------------------------------
# inputs: the reference's golden gradients (tools/gen_golden_mol_grad.py) and the kernel-level shapes
# ----------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mol_grad.npz")


def golden_cases():
    """[(name, cfg, weights, arrays, grads)]: arrays q / cand / dY / y (/ user_ids), grads "q", "cand" and "w/<state_dict key>"."""
    from oracle.mol_oracle import MoLConfig

    z = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in z.files})
    out = []
    for name in names:
        d = json.loads(str(z[f"{name}/cfg_json"]))
        d["uid_embedding_hash_sizes"] = tuple(d["uid_embedding_hash_sizes"])
        cfg = MoLConfig(**d)
        get = lambda prefix: {k[len(prefix):]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith(prefix)}
        w, grads = get(f"{name}/w/"), get(f"{name}/grad/")
        arrays = {k: torch.from_numpy(np.asarray(z[f"{name}/{k}"])) for k in ("q", "cand", "dY", "y", "user_ids") if f"{name}/{k}" in z.files}
        out.append((name, cfg, w, arrays, grads))
    return out


def _shape(pq, px, d, h, **kw):
    from oracle.mol_oracle import MoLConfig

    return MoLConfig(32, 24, d, pq, px, query_hidden_dim=48, gating_query_hidden_dim=16, gating_item_hidden_dim=16, gating_qi_hidden_dim=h, **kw)


def kernel_shapes():
    """The smallest shapes at which each axis of the backward kernels can go wrong."""
    return {
        "8x8x32_h128": _shape(8, 8, 32, 128),                 # the headline geometry: TL = 2, nothing padded
        "4x4x64_h128": _shape(4, 4, 64, 128),                 # L = 16 < Lp = 32; two dEq tiles along d
        "12x3x20_h50": _shape(12, 3, 20, 50),                 # d, L and H all padded
        "1x1x64_h128": _shape(1, 1, 64, 128),                 # L = 1: dpi vanishes against its mean, only the direct term is left
        "16x16x8_h32": _shape(16, 16, 8, 32),                 # L = 256, TL = 8: the accumulators in LDS, one wave per workgroup
        "8x16x16_h64": _shape(8, 16, 16, 64),                 # L = 128, TL = 4: the accumulators in LDS, three waves summed at the row's end
        "12x8x8_h32": _shape(12, 8, 8, 32),                   # L = 96, TL = 3: the last register-resident instantiation
        "64x1x16_h64": _shape(64, 1, 16, 64),                 # P_Q = 64: two blocks of query groups in GEMM1 and two dEq tiles along p
        "4x8x32_h512": _shape(4, 8, 32, 512),                 # the widest hidden layer
        "none_4x4x24_h64": _shape(4, 4, 24, 64, gating_combination_type="none", gating_query_fn=False, gating_item_fn=False),
    }


KERNEL_B, KERNEL_X = (1, 3, 33), (1, 31, 32, 33, 130)


def kernel_inputs(cfg, seed: int = 5):
    """weights, q (33, D), items (33, 130, D'), dY (33, 130): one draw per shape; the cases are its leading (B, X) corners."""
    from oracle.mol_oracle import hash_item_table, synthetic_queries, synthetic_weights

    w = synthetic_weights(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    # non-zero biases in the pair gate, so that db1 / db2 paths see them
    for k in list(w):
        if "_qi_partial_module" in k and k.endswith("bias"):
            w[k] = torch.randn(w[k].shape, generator=g) * 0.05
    B, X = max(KERNEL_B), max(KERNEL_X)
    table = torch.from_numpy(hash_item_table(seed + 2, 0, 257, cfg.item_embedding_dim))
    items = table[torch.randint(0, 257, (B, X), generator=g)]
    q = synthetic_queries(cfg, B, seed=seed + 3)
    dy = torch.randn((B, X), generator=g)
    return w, q, items, dy
