#!/usr/bin/env python3
"""Latency of the SASRec query encoder (rails_amd.SASRec.encode, eval path) at the three shipped geometries, B = 32: the fused
single-launch route (where the geometry fits), the per-layer route, and eager torch (torch.nn.MultiheadAttention, Conv1d, layer_norm
with the same weights, on the same GPU) as the baseline.  GPU time between two events around `reps` calls, after warm-up; the median
of `rounds` such rounds, per call.  Prints one JSON line per geometry.

  python tools/sasrec_bench.py [--reps 20] [--rounds 7] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rails_amd import SASRec  # noqa: E402

GEOM = {   # configs/*/sasrec-*.gin: N = max_sequence_length + 1 output position
    "amzn-books": dict(N=51, D=64, blocks=4, heads=4, ffn=64, items=10000),
    "ml-1m": dict(N=201, D=50, blocks=2, heads=1, ffn=50, items=3883),
    "ml-20m": dict(N=201, D=256, blocks=4, heads=4, ffn=256, items=27278),
}


class EagerSASRec(torch.nn.Module):
    """The same encoder in eager torch ops, from the rails_amd module's parameters (the baseline)."""

    def __init__(self, m: SASRec) -> None:
        super().__init__()
        D, H, Fh = m._embedding_dim, m._num_heads, m._ffn_hidden_dim
        self.D, self.m = D, m
        self.mha = torch.nn.ModuleList()
        self.ffn = torch.nn.ModuleList()
        for att, ff in zip(m.attention_layers, m.forward_layers):
            mha = torch.nn.MultiheadAttention(D, H, batch_first=True)
            mha.in_proj_weight.data.copy_(att.in_proj_weight.data)
            mha.in_proj_bias.data.copy_(att.in_proj_bias.data)
            mha.out_proj.weight.data.copy_(att.out_proj.weight.data)
            mha.out_proj.bias.data.copy_(att.out_proj.bias.data)
            self.mha.append(mha)
            c1 = torch.nn.Conv1d(D, Fh, 1)
            c2 = torch.nn.Conv1d(Fh, D, 1)
            c1.load_state_dict(ff._conv1d[0].state_dict())
            c2.load_state_dict(ff._conv1d[3].state_dict())
            self.ffn.append(torch.nn.Sequential(c1, torch.nn.ReLU() if m._ffn_activation_fn == "relu" else torch.nn.GELU(), c2))
        self.register_buffer("mask", m._attn_mask.clone())

    def encode(self, lengths, ids, emb):
        B, N = ids.shape
        valid = (ids != 0).unsqueeze(-1).float()
        x = (emb * self.D ** 0.5 + self.m._input_features_preproc._pos_emb.weight[:N].unsqueeze(0)) * valid
        for mha, ffn in zip(self.mha, self.ffn):
            q = F.layer_norm(x, (self.D,), eps=1e-8)
            a, _ = mha(q, x, x, attn_mask=self.mask[:N, :N])
            z = F.layer_norm(q + a, (self.D,), eps=1e-8)
            x = (ffn(z.transpose(1, 2)).transpose(1, 2) + z) * valid
        x = F.layer_norm(x, (self.D,), eps=1e-6) if self.m._postproc == "layer_norm" else x / x.norm(dim=-1, keepdim=True).clamp(min=1e-6)
        return x[torch.arange(B, device=x.device), lengths - 1]


def time_ms(fn, reps, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / reps)
    per.sort()
    return per[len(per) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = 32
    for name, gm in GEOM.items():
        torch.manual_seed(0)
        N = gm["N"]
        m = SASRec(N - 1, 1, gm["D"], gm["blocks"], gm["heads"], gm["ffn"], "relu", num_items=gm["items"],
                   output_postproc="layer_norm").to(dev).eval()
        eager = EagerSASRec(m).to(dev).eval()
        g = torch.Generator().manual_seed(1)
        lengths = torch.randint(N // 2, N + 1, (B,), generator=g)
        ids = torch.randint(1, gm["items"] + 1, (B, N), generator=g) * (torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1))
        l_d, i_d = lengths.to(dev), ids.to(dev)
        row = {"geometry": name, "B": B, "N": N, "D": gm["D"], "blocks": gm["blocks"], "heads": gm["heads"]}
        with torch.inference_mode():
            emb = m.get_item_embeddings(i_d)
            fits = bool(m._encode_fused(l_d, i_d, emb) is not None)
            m.use_fused_kernel = True
            out_f = m.encode(l_d, i_d, emb, {})
            row["fused_ms"] = time_ms(lambda: m.encode(l_d, i_d, emb, {}), args.reps, args.rounds, args.warmup) if fits else None
            m.use_fused_kernel = False
            out_l = m.encode(l_d, i_d, emb, {})
            row["per_layer_ms"] = time_ms(lambda: m.encode(l_d, i_d, emb, {}), args.reps, args.rounds, args.warmup)
            out_e = eager.encode(l_d, i_d, emb)
            row["torch_eager_ms"] = time_ms(lambda: eager.encode(l_d, i_d, emb), args.reps, args.rounds, args.warmup)
            row["max_abs_diff_vs_eager"] = float(max((out_f - out_e).abs().max(), (out_l - out_e).abs().max()))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
