"""float64 restatement of the reference SASRec encoder (modeling/sequential/sasrec.py, eval) for the SASRec tests, written from
the arithmetic the reference performs, and the fixture loader.  `bug` applies one of the mistakes an implementation could make, so
the tests can check that their tolerances reject it."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GEOMETRIES = ["amzn-books", "amzn-books-gelu", "ml-1m", "ml-20m"]
BUGS = ["kv_from_q", "x_residual", "drop_masked_keys", "no_in_proj_bias", "non_causal", "scale_1_over_hd"]


def from_model(model, lengths, ids, cfg):
    """A fixture-like dict for a module built in a test: its state_dict under `w/`, the inputs, the geometry."""
    f = {"w/" + k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if not k.startswith("_ndp_module")}
    f["in/past_lengths"], f["in/past_ids"], f["cfg"] = lengths.numpy(), ids.numpy(), dict(cfg)
    return f


def load(name):
    z = np.load(os.path.join(GOLDEN, f"sasrec_{name}.npz"))
    f = {k: z[k] for k in z.files if not k.startswith("wstep/")}
    for k in z.files:                # int8 codes on a power-of-two grid: value = code * step, exact in float32
        if k.startswith("wstep/"):
            f["w/" + k[6:]] = (z["w/" + k[6:]].astype(np.float64) * float(z[k])).astype(np.float32)
    msl, mol, D, blocks, heads, ffn, num_items = (int(v) for v in f["meta/geometry"])
    f["cfg"] = dict(max_sequence_len=msl, max_output_len=mol, N=msl + mol, D=D, blocks=blocks, heads=heads, ffn=ffn, num_items=num_items,
                    act=str(f["meta/ffn_activation_fn"]), postproc=str(f["meta/output_postproc"]))
    return f


def _ln(x, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps)


def attention64(qkv, B, N, H, causal=True, scale_pow=0.5, key_mask=None):
    """softmax(q k^T / hd^scale_pow) v per head over rows [q | k | v]; (B * N, 3D) -> (B * N, D), float64."""
    D = qkv.shape[1] // 3
    hd = D // H
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(B, N, H, hd).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / hd ** scale_pow
    allowed = torch.ones((N, N), dtype=torch.bool)
    if causal:
        allowed = torch.tril(allowed)
    allowed = allowed.expand(B, H, N, N)
    if key_mask is not None:   # (B, N): keys allowed; a query whose every key is hidden keeps its own key
        allowed = allowed & key_mask[:, None, None, :]
        allowed = allowed | torch.eye(N, dtype=torch.bool).expand(B, H, N, N)
    s = s.masked_fill(~allowed, float("-inf"))
    p = torch.softmax(s, -1)
    return (p @ v).transpose(1, 2).reshape(B * N, D)


def encoder64(f, bug=None, ids=None, lengths=None, dtype=torch.float64):
    """(sequence (B, N, D), current (B, D)) in float64 (or `dtype`) from the fixture's weights and inputs."""
    c = f["cfg"]
    w = {k[2:]: torch.from_numpy(v).to(dtype) for k, v in f.items() if k.startswith("w/")}
    ids = torch.from_numpy(f["in/past_ids"]) if ids is None else ids
    lengths = torch.from_numpy(f["in/past_lengths"]) if lengths is None else lengths
    B, N = ids.shape
    D, H = c["D"], c["heads"]
    m = (ids != 0).to(dtype).unsqueeze(-1)
    x = (w["_embedding_module._item_emb.weight"][ids] * float(D) ** 0.5 + w["_input_features_preproc._pos_emb.weight"][:N]) * m
    for i in range(c["blocks"]):
        a, p = f"attention_layers.{i}.", f"forward_layers.{i}._conv1d."
        Q = _ln(x, 1e-8)
        W, bias = w[a + "in_proj_weight"], w[a + "in_proj_bias"]
        if bug == "no_in_proj_bias":
            bias = torch.zeros_like(bias)
        kv_src = Q if bug == "kv_from_q" else x
        qkv = torch.cat([Q @ W[:D].T + bias[:D], kv_src @ W[D:].T + bias[D:]], -1).reshape(B * N, 3 * D)
        att = attention64(qkv, B, N, H, causal=bug != "non_causal", scale_pow=1.0 if bug == "scale_1_over_hd" else 0.5,
                          key_mask=(ids != 0) if bug == "drop_masked_keys" else None).reshape(B, N, D)
        y = (x if bug == "x_residual" else Q) + att @ w[a + "out_proj.weight"].T + w[a + "out_proj.bias"]
        z = _ln(y, 1e-8)
        h = z @ w[p + "0.weight"][:, :, 0].T + w[p + "0.bias"]
        h = torch.relu(h) if c["act"] == "relu" else torch.nn.functional.gelu(h)
        x = (h @ w[p + "3.weight"][:, :, 0].T + w[p + "3.bias"] + z) * m
    if c["postproc"] == "layer_norm":
        seq = _ln(x, 1e-6)
    else:
        seq = x / torch.clamp(torch.linalg.norm(x, dim=-1, keepdim=True), min=1e-6)
    cur = seq[torch.arange(B), lengths - 1]
    return seq, cur
