"""Loader of tests/golden/generic_shapes.npz (tools/gen_golden_generic_shapes.py: the reference on MoL shapes without a fused kernel)."""
import json
import os

import numpy as np
import torch

from oracle.mol_oracle import MoLConfig

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def generic_cases():
    """(name, cfg, weights, arrays) per case, as tests/_fixtures.variant_cases yields them."""
    z = np.load(os.path.join(GOLDEN, "generic_shapes.npz"))
    for name in sorted({k.split("/")[0] for k in z.files}):
        d = json.loads(str(z[f"{name}/cfg_json"]))
        d["uid_embedding_hash_sizes"] = tuple(d["uid_embedding_hash_sizes"])
        cfg = MoLConfig(**d)
        w = {k[len(name) + 3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "/w/")}
        arrays = {k[len(name) + 1:]: torch.from_numpy(np.asarray(z[k])) for k in z.files
                  if k.startswith(name + "/") and "/w/" not in k and not k.endswith("cfg_json")}
        yield name, cfg, w, arrays


def spec_of(cfg, E):
    """The engine's MolShapeSpec of an oracle MoLConfig."""
    return E.MolShapeSpec(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups, cfg.item_dot_product_groups,
        cfg.query_hidden_dim, cfg.gating_query_hidden_dim if cfg.gating_query_fn else -1, cfg.gating_item_hidden_dim if cfg.gating_item_fn else -1,
        cfg.gating_qi_hidden_dim, query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=tuple(cfg.uid_embedding_hash_sizes),
        dot_product_l2_norm=cfg.dot_product_l2_norm, temperature=cfg.temperature, eps=cfg.eps, item_hidden_dim=cfg.item_hidden_dim,
        item_nonlinearity=cfg.item_nonlinearity, gating_combination_type=cfg.gating_combination_type, gating_query_fn=cfg.gating_query_fn,
        gating_item_fn=cfg.gating_item_fn)
