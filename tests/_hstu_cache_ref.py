"""Restatement of the HSTU encoder's cached incremental decoding (modeling/sequential/hstu.py:144-213, :276-433, :665-803) on the
CPU, in whatever dtype the weights have (float64 for the bars of tests/test_hstu_cache*.py) -- TEST INFRASTRUCTURE ONLY.

prefill(): the states `encode(..., return_cache_states=True)` returns, per layer (v jagged (R, H*dv), padded_q / padded_k (B, N, H*dqk)
with zeros at positions >= length, outputs jagged (R, D)), R = sum of the lengths, and the current embeddings.
decode(): one row per sequence at positions[b] against those states, updating them in place as the reference does, and the
postprocessed last layer's outputs row at lengths - 1.  `bug` injects one of the mistakes a kernel could plausibly make, so that the
tests can show their bars reject it.  `gemv` replaces the summation order of decode()'s two matrix-vector products (chain_gemv: one
sequential chain per output column, the least favourable order a correct kernel could use).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import hstu_oracle as HO

BUGS = ("ts_p", "drop_self", "stale_k", "write_p", "return_p", "no_outputs")
# mistakes of the decode kernel's own matrix-vector products and head loop (tests/test_hstu_decode_kernel.py): the last k term of a
# product dropped, its last output column left at the accumulator's initial value (0), the last head's attention never computed
GEMV_BUGS = ("uvqk_drop_last_k", "uvqk_stale_last_column", "o_drop_last_k", "o_stale_last_column", "skip_head")


def chain_gemv(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x (B, K) @ w (K, C) with every output accumulated as one sequential chain over k in the dtype of the operands."""
    acc = torch.zeros((x.shape[0], w.shape[1]), dtype=x.dtype)
    for k in range(w.shape[0]):
        acc = acc + x[:, k: k + 1] * w[k: k + 1]
    return acc


def _gemv(gemv, x, w, bug, which):
    """x @ w through `gemv` (None: torch's own order), with the `which`_* mistakes of GEMV_BUGS."""
    if bug == which + "_drop_last_k":
        x, w = x[:, :-1], w[:-1]
    y = x @ w if gemv is None else gemv(x, w)
    if bug == which + "_stale_last_column":
        y = y.clone()
        y[:, -1] = 0
    return y


def _postproc(cfg: HO.HSTUConfig, x: torch.Tensor) -> torch.Tensor:
    if cfg.postproc == "l2_norm":
        return x / torch.clamp(torch.linalg.norm(x, dim=-1, keepdim=True), min=cfg.eps)
    return F.layer_norm(x, [x.shape[-1]], eps=cfg.eps)


def _input_rows(cfg, w, ids):
    D = cfg.embedding_dim
    emb = w["_embedding_module._item_emb.weight"][ids]
    x = emb * (D ** 0.5) + w["_input_features_preproc._pos_emb.weight"][: ids.shape[-1]]
    return x * (ids != 0).unsqueeze(-1).to(x.dtype)


def prefill(cfg: HO.HSTUConfig, w: Dict[str, torch.Tensor], lengths: torch.Tensor, ids: torch.Tensor, ts: Optional[torch.Tensor]):
    """-> (current embeddings (B, D), [(v, padded_q, padded_k, outputs)] per layer)."""
    D, H, dqk, dv, N = cfg.embedding_dim, cfg.num_heads, cfg.attention_dim, cfg.linear_dim, cfg.max_sequence_len
    B = ids.shape[0]
    dt = w["_hstu._attention_layers.0._uvqk"].dtype
    valid = torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1)
    x = _input_rows(cfg, w, ids) * valid.unsqueeze(-1).to(dt)
    causal = (torch.arange(N).view(N, 1) >= torch.arange(N).view(1, N)).to(dt)
    states = []
    for l in range(cfg.num_blocks):
        p = f"_hstu._attention_layers.{l}."
        mm = F.silu(F.layer_norm(x, [D], eps=cfg.eps) @ w[p + "_uvqk"]) * valid.unsqueeze(-1).to(dt)
        u, v, q, k = torch.split(mm, [dv * H, dv * H, dqk * H, dqk * H], dim=-1)
        qk = torch.einsum("bnhd,bmhd->bhnm", q.reshape(B, N, H, dqk), k.reshape(B, N, H, dqk))
        if ts is not None:
            qk = qk + HO.rel_bias(cfg, w[p + "_rel_attn_bias._ts_w"], w[p + "_rel_attn_bias._pos_w"], ts).unsqueeze(1)
        qk = F.silu(qk) / N * causal.view(1, 1, N, N)
        a = torch.einsum("bhnm,bmhd->bnhd", qk, v.reshape(B, N, H, dv)).reshape(B, N, H * dv)
        x = (F.linear(u * F.layer_norm(a, [dv * H], eps=cfg.eps), w[p + "_o.weight"], w[p + "_o.bias"]) + x) * valid.unsqueeze(-1).to(dt)
        states.append((v[valid].clone(), q.contiguous().clone(), k.contiguous().clone(), x[valid].clone()))
    cur = _postproc(cfg, x[torch.arange(B), lengths - 1])
    return cur, states


def decode(cfg: HO.HSTUConfig, w: Dict[str, torch.Tensor], lengths: torch.Tensor, ids: torch.Tensor, ts: Optional[torch.Tensor],
           positions: torch.Tensor, states: List[Tuple[torch.Tensor, ...]], bug: Optional[str] = None, gemv=None) -> torch.Tensor:
    """Decode row positions[b] of every sequence against `states` (updated in place) -> current embeddings (B, D)."""
    assert bug is None or bug in BUGS + GEMV_BUGS, bug
    D, H, dqk, dv, N, nb = cfg.embedding_dim, cfg.num_heads, cfg.attention_dim, cfg.linear_dim, cfg.max_sequence_len, cfg.num_buckets
    B = ids.shape[0]
    bidx = torch.arange(B)
    off = torch.cumsum(lengths, 0) - lengths
    rows = off + positions
    wrows = positions if bug == "write_p" else rows
    x = _input_rows(cfg, w, ids)[bidx, positions]                                     # (B, D)
    for l in range(cfg.num_blocks):
        p = f"_hstu._attention_layers.{l}."
        V, Q, K, OUT = states[l]
        mm = F.silu(_gemv(gemv, F.layer_norm(x, [D], eps=cfg.eps), w[p + "_uvqk"], bug, "uvqk"))
        u, v, q, k = torch.split(mm, [dv * H, dv * H, dqk * H, dqk * H], dim=-1)
        k_old = K[bidx, positions].clone()
        V[wrows] = v
        Q[bidx, positions] = q
        K[bidx, positions] = k
        a = torch.zeros((B, H * dv), dtype=x.dtype)
        for b in range(B):
            pb = int(positions[b])
            keys = K[b, : pb + 1].clone()
            if bug == "stale_k":
                keys[pb] = k_old[b]
            vals = V[int(off[b]): int(off[b]) + pb + 1]
            s = torch.einsum("hd,jhd->hj", q[b].view(H, dqk), keys.view(pb + 1, H, dqk))
            if ts is not None:
                j = torch.arange(pb + 1)
                tq = ts[b, pb if bug == "ts_p" else min(pb + 1, N - 1)]
                s = s + (w[p + "_rel_attn_bias._pos_w"][N - 1 + j - pb] + w[p + "_rel_attn_bias._ts_w"][HO.bucketize(tq - ts[b, : pb + 1], nb)]).unsqueeze(0)
            pr = F.silu(s) / N
            if bug == "drop_self":
                pr[:, pb] = 0
            if bug == "skip_head":
                pr[H - 1] = 0
            a[b] = torch.einsum("hj,jhd->hd", pr, vals.view(pb + 1, H, dv)).reshape(H * dv)
        oin = u * F.layer_norm(a, [dv * H], eps=cfg.eps)
        if gemv is None and bug not in ("o_drop_last_k", "o_stale_last_column"):
            x = F.linear(oin, w[p + "_o.weight"], w[p + "_o.bias"]) + x
        else:
            x = _gemv(gemv, oin, w[p + "_o.weight"].t(), bug, "o") + w[p + "_o.bias"] + x
        if bug != "no_outputs":
            OUT[wrows] = x
    last = states[-1][3]
    return _postproc(cfg, x if bug == "return_p" else last[off + lengths - 1])


def clone_states(states):
    return [tuple(t.clone() for t in s) for s in states]


def touched(states, lengths: torch.Tensor, positions: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The cache rows a decode at `positions` writes, per layer, stacked: v / outputs at the jagged rows, q / k at (b, p)."""
    rows = torch.cumsum(lengths, 0) - lengths + positions
    bidx = torch.arange(lengths.numel())
    return {"v": torch.stack([s[0][rows] for s in states]), "q": torch.stack([s[1][bidx, positions] for s in states]),
            "k": torch.stack([s[2][bidx, positions] for s in states]), "outputs": torch.stack([s[3][rows] for s in states])}


# ---- the fixtures of tools/gen_golden_hstu_cache.py ------------------------------------------------------------------------------
import os  # noqa: E402

import numpy as np  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(HO.HSTU_CONFIGS)
TAGS = ("tail", "tail2", "interior", "ts", "nots")
ROWS = ("v", "q", "k", "outputs")


def load(name: str):
    """-> (cfg, float32 weights (those of hstu_<name>.npz), lengths, ids, ts, the cache fixture)."""
    base = np.load(os.path.join(GOLDEN, f"hstu_{name}.npz"))
    z = np.load(os.path.join(GOLDEN, f"hstu_cache_{name}.npz"))
    w = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w/")}
    return (HO.HSTU_CONFIGS[name], w, torch.from_numpy(z["in/past_lengths"]), torch.from_numpy(z["in/past_ids"]),
            torch.from_numpy(z["in/timestamps"]), z)


def scenario(z, tag: str, ts: torch.Tensor):
    """-> (positions, decode ids, decode timestamps or None, prefill timestamps or None) of a fixture scenario."""
    pos = torch.from_numpy(z[f"{tag}/positions"])
    ids = torch.from_numpy(z[f"{tag}/ids"])
    if tag == "nots":
        return pos, ids, None, None
    return pos, ids, (torch.from_numpy(z[f"{tag}/timestamps"]) if f"{tag}/timestamps" in z.files else ts), ts


def expected(name: str, bug: Optional[str] = None, dtype=torch.float64):
    """The fixture scenarios replayed by the restatement: {tag: {"prefill_current", "current", "v", "q", "k", "outputs"}} (and, for
    "interior", "states": the whole cache after the decode)."""
    cfg, w, lengths, ids, ts, z = load(name)
    w = {k: v.to(dtype) for k, v in w.items()}
    out = {}
    states = None
    for tag in TAGS:
        pos, new_ids, new_ts, pre_ts = scenario(z, tag, ts)
        if tag == "tail2":
            pre = out["tail"]["current"]
        else:
            pre, states = prefill(cfg, w, lengths, ids, pre_ts)
        cur = decode(cfg, w, lengths, new_ids, new_ts, pos, states, bug=bug)
        out[tag] = {"prefill_current": pre, "current": cur, **touched(states, lengths, pos)}
        if tag == "interior":
            out[tag]["states"] = clone_states(states)
    return out


def bars(name: str, ref64) -> Dict[str, Dict[str, float]]:
    """Per scenario and quantity: twice the reference's (float32) distance from the float64 restatement, plus 1e-6."""
    z = load(name)[-1]
    return {tag: {q: 2 * float((torch.from_numpy(z[f"{tag}/{q}"]).double() - ref64[tag][q].double()).abs().max()) + 1e-6
                  for q in ("prefill_current", "current") + ROWS} for tag in TAGS}
