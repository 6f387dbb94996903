"""float64 restatement of SASRec's cached incremental decoding for the decode tests, and the chain fixture loader.

The reference has no cache API: a decode step is defined as the encode of the updated sequence at row p = lengths - 1
(tests/_sasrec_ref.encoder64).  `prefill64` and `step64` restate it incrementally -- per block, row p alone against the cached key /
value rows 0..p-1 plus its own fresh k / v, which then replace cache row p -- so the tests can check that the two forms agree and
that the bars reject the mistakes an incremental implementation could make (`bug`, one of BUGS)."""
import os

import numpy as np
import torch

from tests import _sasrec_ref as S

BUGS = ["stale_self_kv", "no_self_key", "extra_key", "no_cache_write", "no_id_mask", "pos_of_p_minus_1", "kv_from_ln"]


def load(name):
    """The SASRec fixture (weights, cfg) plus its append chain: chain/lengths (S, B), chain/ids (S, B, N), chain/out (S, B, D)."""
    f = S.load(name)
    z = np.load(os.path.join(S.GOLDEN, f"sasrec_decode_{name}.npz"))
    f["chain/lengths"] = z["chain/lengths"].astype(np.int64)
    f["chain/ids"] = z["chain/ids"].astype(np.int64)
    f["chain/out"] = z["chain/out"]
    return f


def weights(f, dtype=torch.float64):
    return {k[2:]: torch.from_numpy(v).to(dtype) for k, v in f.items() if k.startswith("w/")}


def _ffn(w, p, z, act):
    h = z @ w[p + "0.weight"][:, :, 0].T + w[p + "0.bias"]
    h = torch.relu(h) if act == "relu" else torch.nn.functional.gelu(h)
    return h @ w[p + "3.weight"][:, :, 0].T + w[p + "3.bias"] + z


def _post(x, postproc):
    if postproc == "layer_norm":
        return S._ln(x, 1e-6)
    return x / torch.clamp(torch.linalg.norm(x, dim=-1, keepdim=True), min=1e-6)


def prefill64(f, lengths, ids):
    """(current (B, D), cache [(k, v) (B, N, D)] per block): encode of the whole sequence, keeping each block's key / value rows."""
    c, w = f["cfg"], weights(f)
    B, N = ids.shape
    D, H = c["D"], c["heads"]
    m = (ids != 0).double().unsqueeze(-1)
    x = (w["_embedding_module._item_emb.weight"][ids] * float(D) ** 0.5 + w["_input_features_preproc._pos_emb.weight"][:N]) * m
    cache = []
    for i in range(c["blocks"]):
        a, p = f"attention_layers.{i}.", f"forward_layers.{i}._conv1d."
        Q = S._ln(x, 1e-8)
        W, bias = w[a + "in_proj_weight"], w[a + "in_proj_bias"]
        kv = x @ W[D:].T + bias[D:]
        cache.append((kv[..., :D].contiguous(), kv[..., D:].contiguous()))
        qkv = torch.cat([Q @ W[:D].T + bias[:D], kv], -1).reshape(B * N, 3 * D)
        att = S.attention64(qkv, B, N, H).reshape(B, N, D)
        z = S._ln(Q + att @ w[a + "out_proj.weight"].T + w[a + "out_proj.bias"], 1e-8)
        x = _ffn(w, p, z, c["act"]) * m
    return _post(x, c["postproc"])[torch.arange(B), lengths - 1], cache


def step64(f, cache, lengths, ids, bug=None):
    """One decode step at p = lengths - 1: (current (B, D), the updated cache).  `cache` is not modified."""
    c, w = f["cfg"], weights(f)
    B, N = ids.shape
    D, H = c["D"], c["heads"]
    hd = D // H
    cache = [(k.clone(), v.clone()) for k, v in cache]
    out = torch.empty((B, D), dtype=torch.float64)
    for b in range(B):
        p = int(lengths[b]) - 1
        idp = int(ids[b, p])
        pp = max(p - 1, 0) if bug == "pos_of_p_minus_1" else p
        mask = 1.0 if (idp != 0 or bug == "no_id_mask") else 0.0
        x = (w["_embedding_module._item_emb.weight"][idp] * float(D) ** 0.5 + w["_input_features_preproc._pos_emb.weight"][pp]) * mask
        for i in range(c["blocks"]):
            a, pf = f"attention_layers.{i}.", f"forward_layers.{i}._conv1d."
            Q = S._ln(x, 1e-8)
            W, bias = w[a + "in_proj_weight"], w[a + "in_proj_bias"]
            q = Q @ W[:D].T + bias[:D]
            kv = (Q if bug == "kv_from_ln" else x) @ W[D:].T + bias[D:]
            kc, vc = cache[i]
            keys, vals = kc[b, :p + 1].clone(), vc[b, :p + 1].clone()
            if bug != "stale_self_kv":
                keys[p], vals[p] = kv[:D], kv[D:]
            if bug == "no_self_key":
                keys, vals = keys[:p], vals[:p]
            if bug == "extra_key" and p + 1 < N:
                keys, vals = torch.cat([keys, kc[b, p + 1:p + 2]]), torch.cat([vals, vc[b, p + 1:p + 2]])
            att = torch.empty(D, dtype=torch.float64)
            for h in range(H):
                sl = slice(h * hd, (h + 1) * hd)
                s = keys[:, sl] @ q[sl] / hd ** 0.5
                att[sl] = torch.softmax(s, 0) @ vals[:, sl] if len(s) else torch.full((hd,), float("nan"), dtype=torch.float64)
            z = S._ln(Q + att @ w[a + "out_proj.weight"].T + w[a + "out_proj.bias"], 1e-8)
            if bug != "no_cache_write":
                kc[b, p], vc[b, p] = kv[:D], kv[D:]
            x = _ffn(w, pf, z, c["act"]) * mask
        out[b] = _post(x, c["postproc"])
    return out, cache


def chain64(f, bug=None):
    """The float64 outputs of the fixture's chain: the prefill's, then one decode step per appended item."""
    L, I = torch.from_numpy(f["chain/lengths"]), torch.from_numpy(f["chain/ids"])
    cur, cache = prefill64(f, L[0], I[0])
    outs = [cur]
    for s in range(1, L.shape[0]):
        cur, cache = step64(f, cache, L[s], I[s], bug=bug)
        outs.append(cur)
    return torch.stack(outs)


def distance(a, b):
    """max |a - b|, a NaN counted as infinitely far."""
    return float(torch.nan_to_num((a.double() - b.double()).abs(), nan=float("inf")).max())
