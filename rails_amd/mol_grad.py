"""Gradients through MoLSimilarity.forward in eval-mode arithmetic.

The (query, item) pair stage -- cross logits, pair gate, combination, softmax mixture -- runs forward and backward in the HIP kernels
of the shape-generic fp32 route (rails_mol_generic_score_candidates / rails_mol_generic_pair_backward); no (B, X, L) or (B, X, H) tensor
exists at any point.  The row-wise stages upstream of it (query / item projection, uid embedding lookup, l2 norm, the query-only and
item-only gate MLPs) are computed by the prologue and index-build kernels in the forward; in the backward they are recomputed as plain
torch operations over the module's parameters (`upstream_stages`, dense layers on rocBLAS) and differentiated by torch.autograd with the
pair stage's (dEq, dgq, dEx, dgi) as cotangents.  The gradient is therefore that of a function that differs from the forward's bits by
the rounding of those row-wise stages only.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .engine import MolShapeSpec


def _glu(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, kind: str) -> torch.Tensor:
    out = w.shape[1] // 2
    lhs, rhs = torch.split(torch.mm(x, w) + b, [out, out], dim=-1)
    return (F.gelu(lhs) if kind == "geglu" else F.silu(lhs)) * rhs


def _l2norm(x: torch.Tensor, eps: float) -> torch.Tensor:
    return x / torch.clamp(torch.linalg.norm(x, dim=-1, keepdim=True), min=eps)


def upstream_stages(spec: MolShapeSpec, w: Dict[str, torch.Tensor], q: Optional[torch.Tensor], items: Optional[torch.Tensor],
                    user_ids: Optional[torch.Tensor] = None):
    """The row-wise stages of the reference's eval-mode forward as differentiable torch operations, in the dtype of their inputs:
    q (B, D) -> Eq (B, P_Q, d), gq (B, L) or None; items (N, D') -> Ex (N, P_X, d), gi (N, L) or None.  A side whose input is None is
    skipped (None, None).  `w` maps the module's state_dict keys to tensors."""
    d = spec.dot_product_dimension
    eq = gq = ex = gi = None
    if q is not None:
        pre = "_query_embeddings_fn._query_emb_proj_module."
        if spec.query_hidden_dim > 0:
            proj = F.linear(_glu(q, w[pre + "1._w"], w[pre + "1._b"], spec.query_nonlinearity), w[pre + "2.weight"], w[pre + "2.bias"])
        else:
            proj = F.linear(q, w[pre + "1.weight"], w[pre + "1.bias"])
        n_uid = len(spec.uid_embedding_hash_sizes)
        eq = proj.reshape(q.shape[0], spec.query_dot_product_groups - n_uid, d)
        if n_uid > 0:
            uid = user_ids.to(device=q.device, dtype=torch.int64).reshape(-1)
            embs = [F.embedding((uid % hs) + 1, w[f"_query_embeddings_fn._uid_embeddings_{i}.weight"]).unsqueeze(1)
                    for i, hs in enumerate(spec.uid_embedding_hash_sizes)]
            eq = torch.cat([eq] + embs, dim=1)
        if spec.dot_product_l2_norm:
            eq = _l2norm(eq, spec.eps)
        if spec.gating_query_fn:
            g = "_gating_fn._query_only_partial_module."
            gq = F.linear(F.silu(F.linear(q, w[g + "0.weight"], w[g + "0.bias"])), w[g + "2.weight"])
    if items is not None:
        pre = "_item_embeddings_fn._item_emb_proj_module."
        if spec.item_hidden_dim > 0:
            proj = F.linear(_glu(items, w[pre + "1._w"], w[pre + "1._b"], spec.item_nonlinearity), w[pre + "2.weight"], w[pre + "2.bias"])
        else:
            proj = F.linear(items, w[pre + "1.weight"], w[pre + "1.bias"])
        ex = proj.reshape(items.shape[0], spec.item_dot_product_groups, d)
        if spec.dot_product_l2_norm:
            ex = _l2norm(ex, spec.eps)
        if spec.gating_item_fn:
            g = "_gating_fn._item_only_partial_module."
            gi = F.linear(F.silu(F.linear(items, w[g + "1.weight"], w[g + "1.bias"])), w[g + "3.weight"])
    return eq, gq, ex, gi


_PAIR_GATE = "_gating_fn._qi_partial_module."
_PAIR_KEYS = (_PAIR_GATE + "1.weight", _PAIR_GATE + "1.bias", _PAIR_GATE + "3.weight", _PAIR_GATE + "3.bias")
_ITEM_SIDE = ("_item_embeddings_fn.", "_gating_fn._item_only_partial_module.")


def _side(key: str) -> int:
    """0: a parameter of the query side, 1: of the item side, 2: of the pair gate."""
    if key.startswith(_PAIR_GATE):
        return 2
    return 1 if key.startswith(_ITEM_SIDE) else 0


class _PairStage(torch.autograd.Function):
    """(q (B, D), items (B, X, D'), *parameters) -> (B, X) fp32 logits; the parameters come in the order of `keys`."""

    @staticmethod
    def forward(ctx, module, keys: Tuple[str, ...], user_ids, q: torch.Tensor, items: torch.Tensor, *params: torch.Tensor):
        eng = module.grad_engine()
        B, X = items.shape[0], items.shape[1]
        qpack, _, _ = eng.query_pack(q.detach(), user_ids)
        cand = eng.build_index(items.detach().reshape(B * X, items.shape[-1]))
        logits = eng.score_candidates(qpack, B, cand, X)
        ctx.engine, ctx.spec, ctx.keys, ctx.user_ids = eng, eng.spec, keys, user_ids
        ctx.packs = (qpack, cand)
        ctx.save_for_backward(q, items, *params)
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, dY: torch.Tensor):
        q, items, *params = ctx.saved_tensors
        keys, spec, eng = ctx.keys, ctx.spec, ctx.engine
        qpack, cand = ctx.packs
        B, X = items.shape[0], items.shape[1]
        wants = ctx.needs_input_grad[3:]                     # (q, items, *params) behind (module, keys, user_ids)
        want_param = dict(zip(keys, wants[2:]))
        need = [wants[0], wants[1], False]
        for key, flag in want_param.items():
            if flag:
                need[_side(key)] = True
        dY = dY if dY.dtype == torch.float32 else dY.float()
        if dY.dim() != 2 or (X > 1 and dY.stride(1) != 1) or (B > 1 and dY.stride(0) < X):
            dY = dY.contiguous()
        dq, di, dw = eng.pair_backward(qpack, B, cand, X, dY, need=tuple(need))
        grads: Dict[str, Optional[torch.Tensor]] = {}
        if dw is not None:
            grads.update(zip(_PAIR_KEYS, dw))

        # the row-wise stages, recomputed from detached leaves and differentiated by torch with the pair stage's cotangents
        PQ, PX, d, L = spec.query_dot_product_groups, spec.item_dot_product_groups, spec.dot_product_dimension, spec.num_logits
        dp = (d + 7) // 8 * 8
        leaves: Dict[str, torch.Tensor] = {}
        w: Dict[str, torch.Tensor] = {}
        for key, p in zip(keys, params):
            t = p.detach().float()
            if want_param[key] and _side(key) != 2:
                t = t.requires_grad_(True)
                leaves[key] = t
            w[key] = t
        q_leaf = items_leaf = None
        if need[0]:
            q_leaf = q.detach().float().requires_grad_(bool(wants[0]))
            if wants[0]:
                leaves["q"] = q_leaf
        if need[1]:
            items_leaf = items.detach().float().reshape(B * X, items.shape[-1]).requires_grad_(bool(wants[1]))
            if wants[1]:
                leaves["items"] = items_leaf
        if leaves:
            with torch.enable_grad():
                eq, gq, ex, gi = upstream_stages(spec, w, q_leaf, items_leaf, ctx.user_ids)
            outs: List[torch.Tensor] = []
            cots: List[torch.Tensor] = []
            if eq is not None and eq.requires_grad:
                outs.append(eq)
                cots.append(dq[:, : PQ * dp].reshape(B, PQ, dp)[:, :, :d])
            if gq is not None and gq.requires_grad:
                outs.append(gq)
                cots.append(dq[:, PQ * dp : PQ * dp + L])
            if ex is not None and ex.requires_grad:
                outs.append(ex)
                cots.append(di[:, : PX * dp].reshape(B * X, PX, dp)[:, :, :d])
            if gi is not None and gi.requires_grad:
                outs.append(gi)
                cots.append(di[:, PX * dp : PX * dp + L])
            names = list(leaves)
            got = torch.autograd.grad(outs, [leaves[n] for n in names], cots, allow_unused=True) if outs else [None] * len(names)
            grads.update(zip(names, got))

        def back(name: str, like: torch.Tensor, wanted: bool):
            g = grads.get(name) if wanted else None
            if g is None:
                return torch.zeros_like(like) if wanted else None      # (a wanted input the function does not depend on)
            return g.reshape(like.shape).to(like.dtype)

        return (None, None, None, back("q", q, wants[0]), back("items", items, wants[1])) + tuple(
            back(key, p, want_param[key]) for key, p in zip(keys, params))


def differentiable_forward(module, query_embeddings: torch.Tensor, item_embeddings: torch.Tensor, user_ids=None) -> torch.Tensor:
    """MoLSimilarity.forward with `differentiable` set: (B, D), (1 / B, X, D') -> (B, X) logits that carry the graph.  The shared-corpus
    branch (1, X, D') runs the per-row kernels over the expanded rows -- B * X item rows are built and scored, and autograd sums the item
    gradient over B."""
    B = query_embeddings.size(0)
    Bp = item_embeddings.shape[0]
    if Bp == 1 and B != 1:
        item_embeddings = item_embeddings.expand(B, -1, -1)
    elif Bp != B:
        raise RuntimeError(f"item_embeddings.shape[0] must be 1 or B={B}, got {Bp}")
    module.grad_engine()                                      # the refusals, before anything is launched
    named = module.state_dict(keep_vars=True)
    keys = tuple(named)
    logits = _PairStage.apply(module, keys, user_ids, query_embeddings, item_embeddings, *(named[k] for k in keys))
    return logits.to(query_embeddings.dtype)
