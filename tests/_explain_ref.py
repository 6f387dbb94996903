"""Float64 restatement of what explain_of writes: a pair's cross logits cl, its mixture weights pi and the logit
sum_l pi_l cl_l, each with a per-element a-priori bound for the explaining instantiation of mol_generic.hip.  Built on tests/_mol_ref64.py:
its _d, its constants and its arithmetic model (chains of n terms lose at most gamma(n) of their absolute sum; expf within 1 ulp; true
divisions correctly rounded).

  e_cl   score64's ecl: the GEMM1 chain and the Eq / tau pack.
  e_pi   e_w is the bound on the gate value w carried FORWARD through ecl, epre, ehid, egqi and eg (the |W|-summed worst case; the generic
         kernel uses precise expf and true divisions, so the silu constants are C_EXPF's, not C_FAST's).  A perturbation dw of w moves pi_l
         to pi_l exp(dw_l) / sum_j pi_j exp(dw_j), which lies within pi_l exp(+-S_l), S_l = e_w[l] + sum_j pi_j e_w[j] (Jensen); the bound
         takes pi_l expm1(S_l) -- the first-order form |d pi_l| <= pi_l (e_w[l] + sum_j pi_j e_w[j]) without its remainder -- and adds the
         softmax's own roundings: the rounded exponent (u |w_l - max w| relative), expf (C_EXPF u), the L-term sum den, and the reciprocal,
         the two products and the renormalising division (C_MIX u).
  e_out  the same perturbations through out = sum_l pi_l cl_l (d out = sum_l d pi_l (cl_l - out) + sum_l pi_l d cl_l) and the num / den sums.

The forward bound is loose (tests/_mol_ref64.py says 100 - 1000 x for the logits); tests/test_score_of_cpu.py checks that it still
rejects every mutant of the kernel's pair arithmetic by a factor of 10 and prints how far above the reference's own fp32 stages it lies.

`mut` applies the bug classes of that meta-test to the float64 value (not to the bound):
  "transposed"   l = m * P_Q + p instead of p * P_X + m
  "no_tau"       cl without the division by tau
  "silu_gqgi"    w = silu(gq gi) + gqi
"""
from __future__ import annotations

import torch

from tests._mol_ref64 import C_DOT, C_EXPF, C_LIN, C_MIX, C_SUM, SILU_LIP, TINY, U, _d, f32


def explain64(cfg, w, Eq, Ex, gq, gi, mut=None):
    """Eq (B, P_Q, d), gq (B, L); Ex (N, P_X, d), gi (N, L) for a shared corpus or (B, N, P_X, d), (B, N, L) for per-row candidates
    -> ((cl, e_cl), (pi, e_pi), (out, e_out)): cl, pi (B, N, L), out (B, N), float64."""
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
    if mut == "transposed":
        cl, clabs = cl.transpose(2, 3), clabs.transpose(2, 3)
    cl, clabs = cl.reshape(B, N, L), clabs.reshape(B, N, L)
    if mut != "no_tau":
        cl, clabs = cl / tau, clabs / tau
    ecl = C_DOT * U * (d + 3) * clabs
    p = "_gating_fn._qi_partial_module."
    H = cfg.gating_qi_hidden_dim
    assert H > 0, "the generic route needs a hidden-layer pair gate"
    W1, b1, W2, b2 = _d(w[p + "1.weight"]), _d(w[p + "1.bias"]), _d(w[p + "3.weight"]), _d(w[p + "3.bias"])
    pre = cl @ W1.T + b1
    epre = C_DOT * U * (L + 3) * (cl.abs() @ W1.abs().T + b1.abs()) + ecl @ W1.abs().T
    hid = pre * torch.sigmoid(pre)
    ehid = SILU_LIP * epre + C_EXPF * U * hid.abs() + TINY
    gqi = hid @ W2.T + b2
    egqi = C_DOT * U * (H + 3) * (hid.abs() @ W2.abs().T + b2.abs()) + ehid @ W2.abs().T
    gq = gq.unsqueeze(1)
    if cfg.gating_combination_type == "none":
        wv = gq + gi + gqi
        e_w = egqi + C_SUM * U * 3 * (gq.abs() + gi.abs() + gqi.abs())
    else:
        a = gq * gi
        g = a + gqi
        eg = egqi + C_DOT * U * 3 * (a.abs() + gqi.abs())
        wv = g * torch.sigmoid(g)
        e_w = SILU_LIP * eg + C_EXPF * U * wv.abs() + TINY
        if mut == "silu_gqgi":
            wv = a * torch.sigmoid(a) + gqi
    pi = torch.softmax(wv, -1)
    out = (pi * cl).sum(-1)
    S = e_w + (pi * e_w).sum(-1, keepdim=True)
    rel_w = torch.expm1(S)
    gap = wv.amax(-1, keepdim=True) - wv
    term = U * (C_EXPF + gap)                                               # one exponential: the rounded exponent and expf
    rel_own = term + (pi * term).sum(-1, keepdim=True) + U * (C_SUM * (L + 2) + C_MIX)
    e_pi = (1 + C_LIN) * pi * (rel_w + rel_own) + TINY
    dev_c = (cl - out.unsqueeze(-1)).abs()
    e_out = (1 + C_LIN) * ((pi * (rel_w + term) * dev_c).sum(-1) + (pi * ecl).sum(-1) + U * (C_SUM * (L + 2) + C_MIX) * (pi * cl.abs()).sum(-1)) + TINY
    return (cl, ecl + TINY), (pi, e_pi), (out, e_out)


# ---- an fp32 emulation of the kernel's pair arithmetic (the meta-test's subject) and its mutants ---------------------------------------------
def emulate32(cfg, w, Eq, Ex, gq, gi, mut=None, eps=None):
    """The explaining kernel's values in fp32 torch arithmetic (not its bits: torch's sums are not the kernel's chains) -> (cl, pi, out) fp32.
    mut: "transposed", "no_tau", "silu_gqgi" as explain64; "padded_softmax" (the softmax over Lp = L rounded up to 32, the padded w at 0);
    "no_renorm" (the renormalising division dropped; visible with eps forced above 1); "pi_before_den" (pi written before the division by
    den).  The generic kernel's padded axes (tests/test_generic_sweep_cpu.py): "padded_softmax_lq" (the softmax over Lq = L rounded up to 4,
    the width of the gq / gi rows); "q_block" (the last block of 32 query groups, p >= 32 floor((P_Q - 1) / 32), leaves its cl rows zero);
    "d_tail" (GEMM1 stops at k = 8 floor(d / 8)); "hid_tail" (the hidden units from 32 floor(H / 32) on are dropped).
    eps: the clamp of the renormalisation (default 1e-6, the kernel's)."""
    f = torch.float32
    Eq, Ex, gq, gi = (t.detach().to("cpu", f) for t in (Eq, Ex, gq, gi))
    B, PQ, d = Eq.shape
    tau = torch.tensor(cfg.temperature, dtype=f)
    eqs = Eq if mut == "no_tau" else Eq / tau
    if mut == "d_tail":
        eqs, Ex = eqs[..., : d // 8 * 8], Ex[..., : d // 8 * 8]
    if Ex.dim() == 3:
        cl = torch.einsum("bpd,nmd->bnpm", eqs, Ex)
        gi = gi.unsqueeze(0)
    else:
        cl = torch.einsum("bpd,bnmd->bnpm", eqs, Ex)
    N, L = cl.shape[1], cfg.num_logits
    if mut == "q_block":
        cl[:, :, (PQ - 1) // 32 * 32 :, :] = 0
    if mut == "transposed":
        cl = cl.transpose(2, 3)
    cl = cl.reshape(B, N, L)
    p = "_gating_fn._qi_partial_module."
    W1, b1, W2, b2 = (w[p + k].detach().to("cpu", f) for k in ("1.weight", "1.bias", "3.weight", "3.bias"))
    if mut == "hid_tail":
        kept = W1.shape[0] // 32 * 32
        W1, b1, W2 = W1[:kept], b1[:kept], W2[:, :kept]
    pre = cl @ W1.T + b1
    hid = pre / (1 + torch.exp(-pre))
    gqi = hid @ W2.T + b2
    gq = gq.unsqueeze(1)
    if cfg.gating_combination_type == "none":
        wv = (gq + gi) + gqi
    elif mut == "silu_gqgi":
        a = gq * gi
        wv = a / (1 + torch.exp(-a)) + gqi
    else:
        g = gq * gi + gqi
        wv = g / (1 + torch.exp(-g))
    clp = cl
    if mut in ("padded_softmax", "padded_softmax_lq"):
        Lp = (L + 31) // 32 * 32 if mut == "padded_softmax" else (L + 3) // 4 * 4
        wv = torch.nn.functional.pad(wv, (0, Lp - L))
        clp = torch.nn.functional.pad(cl, (0, Lp - L))
    e = torch.exp(wv - wv.amax(-1, keepdim=True))
    den = e.sum(-1, keepdim=True)
    num = (e * clp).sum(-1, keepdim=True)
    rden = 1.0 / den
    clamp = torch.tensor(1e-6 if eps is None else eps, dtype=f)
    norm = torch.maximum(den * rden, clamp)
    if mut == "no_renorm":
        norm = torch.ones_like(norm)
    pi = e if mut == "pi_before_den" else (e * rden) / norm
    out = ((num * rden) / norm).squeeze(-1)
    return cl, pi[..., :L], out

