#!/usr/bin/env python3
"""Golden GRADIENTS of the reference's MoLSimilarity (eval mode, fp32, CPU) for the differentiable forward: runs
the REFERENCE under torch autograd (imported through oracle/gen_golden.py's shim, build container only) and writes
tests/golden/mol_grad.npz.

TEST INFRASTRUCTURE ONLY: arrays in, arrays out; nothing of the reference is copied.
  TORCH_COMPILE_DISABLE=1 python tools/gen_golden_mol_grad.py

Per case: the config JSON, q, the per-row candidates, dY, user ids where the case has a uid table, the reference's y and the gradient
of (y * dY).sum() with respect to q, the candidates and every parameter, next to the state dict.  The weights are rounded to multiples
of 2^-8 as tools/gen_golden_generic_shapes.py rounds them (still the reference's own run, on those weights).
"""
import json
import os
import sys

os.environ.setdefault("TORCH_COMPILE_DISABLE", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden as GG  # noqa: E402  (sets up the reference import + shims)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from _npz import savez_deterministic  # noqa: E402

import gen_golden_generic_shapes as GS  # noqa: E402  (build(): the reference module with non-zero biases; _cfg, QUANT)
from oracle.mol_oracle import hash_item_table, synthetic_queries  # noqa: E402

CASES = {
    "d_8x8x32_geglu": GS._cfg(32, 32, 32, 8, 8),
    "d_uid_4x4x32_swiglu": GS._cfg(32, 32, 32, 4, 4, query_nonlinearity="swiglu", uid_embedding_hash_sizes=(97,)),
    "d_none_4x4x24": GS._cfg(32, 32, 24, 4, 4, gating_combination_type="none", gating_query_fn=False, gating_item_fn=False),
}
N, B, XC = 37, 5, 9


def main():
    out = {}
    for i, (name, cfg) in enumerate(CASES.items()):
        mol = GS.build(cfg, 240 + i)
        with torch.no_grad():
            for p in mol.parameters():
                p.copy_(torch.round(p * GS.QUANT) / GS.QUANT)
        table = torch.from_numpy(hash_item_table(230 + i, 0, N, cfg.item_embedding_dim))
        g = torch.Generator().manual_seed(17 + i)
        cand = table[torch.randint(0, N, (B, XC), generator=g)].clone().requires_grad_(True)
        q = synthetic_queries(cfg, B, seed=250 + i).clone().requires_grad_(True)
        dy = torch.randn((B, XC), generator=g)
        kw = {}
        if cfg.uid_embedding_hash_sizes:
            kw["user_ids"] = torch.tensor([3, 96, 97, 1234567, 0], dtype=torch.int64)
            out[f"{name}/user_ids"] = kw["user_ids"].numpy()
        y, aux = mol(q, cand, **kw)
        assert aux == {} and y.shape == (B, XC)
        names = [k for k, _ in mol.named_parameters()]
        grads = torch.autograd.grad((y * dy).sum(), [q, cand] + [p for _, p in mol.named_parameters()], allow_unused=True)
        out[f"{name}/cfg_json"] = np.array(json.dumps(cfg.to_dict()))
        out[f"{name}/q"], out[f"{name}/cand"], out[f"{name}/dY"], out[f"{name}/y"] = q.detach().numpy(), cand.detach().numpy(), dy.numpy(), y.detach().numpy()
        out[f"{name}/grad/q"], out[f"{name}/grad/cand"] = grads[0].numpy(), grads[1].numpy()
        for k, gr in zip(names, grads[2:]):
            if gr is not None:
                out[f"{name}/grad/w/{k}"] = gr.numpy()
        for k, v in mol.state_dict().items():
            out[f"{name}/w/{k}"] = v.detach().numpy()
    path = os.path.join(GG.OUT, "mol_grad.npz")
    savez_deterministic(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
