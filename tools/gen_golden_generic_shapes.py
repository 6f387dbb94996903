#!/usr/bin/env python3
"""Golden vectors for MoL shapes that have NO fused scoring kernel (the generic route's ground): runs the REFERENCE on the CPU
(imported through oracle/gen_golden.py's shim, build container only) and writes tests/golden/generic_shapes.npz.

TEST INFRASTRUCTURE ONLY: arrays in, arrays out; nothing of the reference is copied.
  python tools/gen_golden_generic_shapes.py

Per case: the config JSON, q, X, per-row cand, user ids where the case has a uid table, the reference's logits / row_logits / Eq / Ex
and the state dict (non-zero biases, drawn as oracle/gen_golden_variants.py draws them).  query_hidden_dim and N are kept small so
that the file stays small; the weights are rounded to multiples of 2^-8 (still the reference's own run, on those weights).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as GG  # noqa: E402  (sets up the reference import + shims)
import gen_golden_variants as GV  # noqa: E402  (build(): the reference module with non-zero biases)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from _npz import savez_deterministic  # noqa: E402

from modeling.similarity_utils import create_mol_interaction_module  # noqa: E402  (reference)
from oracle.mol_oracle import MoLConfig, hash_item_table, synthetic_queries  # noqa: E402

# Small everywhere the cases are not about: query_hidden_dim, the query-only / item-only gate widths and the embedding dims.
QH, GH = 16, 16


def _cfg(dq, di, d, pq, px, **kw):
    return MoLConfig(dq, di, d, pq, px, query_hidden_dim=QH, gating_query_hidden_dim=GH, gating_item_hidden_dim=GH, **kw)


CASES = {
    "g_4x4x64": _cfg(32, 32, 64, 4, 4),
    "g_2x2x128_h32": _cfg(32, 32, 128, 2, 2, gating_qi_hidden_dim=32),
    "g_1x1x64": _cfg(32, 32, 64, 1, 1),
    "g_4x8x24_h96": _cfg(32, 24, 24, 4, 8, gating_qi_hidden_dim=96),
    "g_8x8x40": _cfg(32, 32, 40, 8, 8),
    "g_12x3x20_h50_swiglu": _cfg(32, 32, 20, 12, 3, gating_qi_hidden_dim=50, query_nonlinearity="swiglu"),
    "g_16x8x32_h256": _cfg(32, 32, 32, 16, 8, gating_qi_hidden_dim=256),
    "g_32x8x16": _cfg(32, 32, 16, 32, 8),
    "g_8x8x32_h192": _cfg(32, 32, 32, 8, 8, gating_qi_hidden_dim=192),
    "g_uid_4x4x32": _cfg(32, 32, 32, 4, 4, uid_embedding_hash_sizes=(97,)),
    "g_none_4x4x24": _cfg(32, 32, 24, 4, 4, gating_combination_type="none", gating_query_fn=False, gating_item_fn=False),
}
N, B, XC = 37, 6, 12
QUANT = 256.0   # every parameter is rounded to a multiple of 1 / QUANT before the reference runs: the file deflates to a third


def build(cfg: MoLConfig, seed: int):
    if not cfg.uid_embedding_hash_sizes:
        return GV.build(cfg, seed)
    torch.manual_seed(seed)
    mol, _ = create_mol_interaction_module(
        query_embedding_dim=cfg.query_embedding_dim, item_embedding_dim=cfg.item_embedding_dim,
        dot_product_dimension=cfg.dot_product_dimension, query_dot_product_groups=cfg.query_dot_product_groups,
        item_dot_product_groups=cfg.item_dot_product_groups, temperature=cfg.temperature, query_dropout_rate=0.0,
        query_hidden_dim=cfg.query_hidden_dim, item_dropout_rate=0.1, item_hidden_dim=cfg.item_hidden_dim,
        gating_query_hidden_dim=cfg.gating_query_hidden_dim, gating_qi_hidden_dim=cfg.gating_qi_hidden_dim,
        gating_item_hidden_dim=cfg.gating_item_hidden_dim, softmax_dropout_rate=cfg.softmax_dropout_rate, bf16_training=False,
        gating_query_fn=cfg.gating_query_fn, gating_item_fn=cfg.gating_item_fn, query_nonlinearity=cfg.query_nonlinearity,
        item_nonlinearity=cfg.item_nonlinearity, gating_combination_type=cfg.gating_combination_type, eps=cfg.eps,
        uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes), uid_dropout_rate=0.5)
    mol.eval()
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for name, p in mol.named_parameters():
            if name.endswith("bias") or name.endswith("_b"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return mol


def main():
    out = {}
    for i, (name, cfg) in enumerate(CASES.items()):
        mol = build(cfg, 140 + i)
        with torch.no_grad():
            for p in mol.parameters():
                p.copy_(torch.round(p * QUANT) / QUANT)
        X = torch.from_numpy(hash_item_table(130 + i, 0, N, cfg.item_embedding_dim)).unsqueeze(0)
        q = synthetic_queries(cfg, B, seed=150 + i)
        kw = {}
        if cfg.uid_embedding_hash_sizes:
            kw["user_ids"] = torch.tensor([3, 96, 97, 1234567, 0, 55], dtype=torch.int64)
            out[f"{name}/user_ids"] = kw["user_ids"].numpy()
        with torch.inference_mode():
            logits, aux = mol(q, X, **kw)
            assert aux == {}
            eq, _ = mol.get_query_component_embeddings(q, **kw)
            ex, _ = mol.get_item_component_embeddings(X)
            cand = X.squeeze(0)[torch.randint(0, N, (B, XC), generator=torch.Generator().manual_seed(7))]
            rows, _ = mol(q, cand, **kw)
        out[f"{name}/cfg_json"] = np.array(json.dumps(cfg.to_dict()))
        out[f"{name}/q"], out[f"{name}/X"], out[f"{name}/cand"] = q.numpy(), X.numpy(), cand.numpy()
        out[f"{name}/logits"], out[f"{name}/Eq"], out[f"{name}/Ex"], out[f"{name}/row_logits"] = logits.numpy(), eq.numpy(), ex.numpy(), rows.numpy()
        for k, v in mol.state_dict().items():
            out[f"{name}/w/{k}"] = v.detach().numpy()
    path = os.path.join(GG.OUT, "generic_shapes.npz")
    savez_deterministic(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
