"""The multi-row HSTU cached decode step (rails_hstu_decode_rows, HSTU.encode(..., delta_rows=)) restated from the single-row
restatement -- TEST INFRASTRUCTURE ONLY.

chain(): R.decode (tests/_hstu_cache_ref.py) applied at positions start[b], start[b] + 1, ... in ascending order; sequence b takes part
in the first counts[b] steps and sits out of the others.  `bug` injects one of the mistakes a multi-row kernel could make.
runs(): the runs a case of tests/_hstu_decode_cases.py is tested on.  direct(): the C-ABI test's references and bars, per quantity
    2 * max(d_blocked, d_chain) + 1e-6
with d_blocked / d_chain the distances from the float64 chain of the fp32 chain in torch's summation order and with R.chain_gemv (the
formula of tests/_hstu_decode_cases.py); every chain starts from the float64 prefill rounded to fp32.
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from oracle import hstu_oracle as HO
from tests import _hstu_cache_ref as R
from tests import _hstu_decode_cases as K
from tests.test_hstu_kernels_gpu import gen, timestamps

BUGS = ("stale_prev", "limit_end", "return_last_decoded", "last_row_unwritten", "ts_p")
QUANTITIES = K.QUANTITIES
KINDS = ("uniform1", "uniform2", "ragged", "long")


class Run(NamedTuple):
    lengths: torch.Tensor      # (B,)
    ids: torch.Tensor          # (B, N) the prefill's ids
    new_ids: torch.Tensor      # (B, N) with fresh ids at the run's rows
    ts: torch.Tensor           # (B, N)
    start: torch.Tensor        # (B,) first row of each run
    counts: torch.Tensor       # (B,) rows of each run


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
def _subset(states, lengths, sel):
    off = torch.cumsum(lengths, 0) - lengths
    jag = torch.cat([torch.arange(int(off[b]), int(off[b] + lengths[b])) for b in sel.tolist()])
    return jag, [(v[jag].clone(), q[sel].clone(), k[sel].clone(), o[jag].clone()) for v, q, k, o in states]


def _put_back(states, sub, jag, sel):
    for (v, q, k, o), (sv, sq, sk, so) in zip(states, sub):
        v[jag], q[sel], k[sel], o[jag] = sv, sq, sk, so


def _decode_limit(cfg, w, lengths, ids, ts, positions, kend, states):
    """R.decode with the key limit kend[b] in place of positions[b] (the `limit_end` mistake; kend == positions is R.decode)."""
    D, H, dqk, dv, N, nb = cfg.embedding_dim, cfg.num_heads, cfg.attention_dim, cfg.linear_dim, cfg.max_sequence_len, cfg.num_buckets
    B = ids.shape[0]
    bidx = torch.arange(B)
    off = torch.cumsum(lengths, 0) - lengths
    rows = off + positions
    x = R._input_rows(cfg, w, ids)[bidx, positions]
    for l in range(cfg.num_blocks):
        p = f"_hstu._attention_layers.{l}."
        V, Q, Kc, OUT = states[l]
        mm = F.silu(F.layer_norm(x, [D], eps=cfg.eps) @ w[p + "_uvqk"])
        u, v, q, k = torch.split(mm, [dv * H, dv * H, dqk * H, dqk * H], dim=-1)
        V[rows], Q[bidx, positions], Kc[bidx, positions] = v, q, k
        a = torch.zeros((B, H * dv), dtype=x.dtype)
        for b in range(B):
            pb, ke = int(positions[b]), int(kend[b])
            keys, vals = Kc[b, : ke + 1], V[int(off[b]): int(off[b]) + ke + 1]
            s = torch.einsum("hd,jhd->hj", q[b].view(H, dqk), keys.view(ke + 1, H, dqk))
            if ts is not None:
                j = torch.arange(ke + 1)
                tq = ts[b, min(pb + 1, N - 1)]
                s = s + (w[p + "_rel_attn_bias._pos_w"][N - 1 + j - pb] + w[p + "_rel_attn_bias._ts_w"][HO.bucketize(tq - ts[b, : ke + 1], nb)]).unsqueeze(0)
            a[b] = torch.einsum("hj,jhd->hd", F.silu(s) / N, vals.view(ke + 1, H, dv)).reshape(H * dv)
        x = F.linear(u * F.layer_norm(a, [dv * H], eps=cfg.eps), w[p + "_o.weight"], w[p + "_o.bias"]) + x
        OUT[rows] = x
    return R._postproc(cfg, states[-1][3][off + lengths - 1])


def chain(cfg, w, lengths, ids, ts, start, counts, states, bug: Optional[str] = None, gemv=None):
    """Single-row decodes over every run in ascending order, `states` updated in place -> current embeddings (B, D)."""
    assert bug is None or bug in BUGS, bug
    before = R.clone_states(states) if bug == "stale_prev" else None
    off = torch.cumsum(lengths, 0) - lengths
    cur = None
    for t in range(int(counts.max())):
        sel = (counts > t).nonzero().flatten()
        pos = (start + t)[sel]
        jag, sub = _subset(states, lengths, sel)
        sl, si, st = lengths[sel], ids[sel], (ts[sel] if ts is not None else None)
        if bug == "stale_prev" and t > 0:      # the row below, fresh from the step before, shows its pre-step k / v
            _, old = _subset(before, lengths, sel)
            prev = torch.cumsum(sl, 0) - sl + pos - 1
            fresh = [(s[0][prev].clone(), s[2][torch.arange(len(sel)), pos - 1].clone()) for s in sub]
            for s, o in zip(sub, old):
                s[0][prev] = o[0][prev]
                s[2][torch.arange(len(sel)), pos - 1] = o[2][torch.arange(len(sel)), pos - 1]
        if bug == "limit_end":
            out = _decode_limit(cfg, w, sl, si, st, pos, (start + counts - 1)[sel], sub)
        else:
            out = R.decode(cfg, w, sl, si, st, pos, sub, bug="ts_p" if bug == "ts_p" else "return_p" if bug == "return_last_decoded" else None,
                           gemv=gemv)
        if bug == "stale_prev" and t > 0:
            for s, (fv, fk) in zip(sub, fresh):
                s[0][prev] = fv
                s[2][torch.arange(len(sel)), pos - 1] = fk
        last = counts[sel] == t + 1
        if bug == "last_row_unwritten" and bool(last.any()):
            _, untouched = _subset(states, lengths, sel[last])
            _put_back(states, sub, jag, sel)
            _put_back(states, untouched, _subset(states, lengths, sel[last])[0], sel[last])
        else:
            _put_back(states, sub, jag, sel)
        if bug == "return_last_decoded":
            cur = out.new_zeros((lengths.numel(), out.shape[1])) if cur is None else cur
            cur[sel[last]] = out[last]
    return cur if bug == "return_last_decoded" else R._postproc(cfg, states[-1][3][off + lengths - 1])


def run_rows(lengths, start, counts):
    """(sequence, position) of every row of every run, sequence-major."""
    b = torch.repeat_interleave(torch.arange(lengths.numel()), counts)
    t = torch.arange(int(counts.sum())) - torch.repeat_interleave(torch.cumsum(counts, 0) - counts, counts)
    return b, start[b] + t


def touched(states, lengths, start, counts):
    """The cache rows a step over the runs writes, per layer, stacked: v / outputs at the jagged rows, q / k at (b, p)."""
    b, p = run_rows(lengths, start, counts)
    rows = (torch.cumsum(lengths, 0) - lengths)[b] + p
    return {"v": torch.stack([s[0][rows] for s in states]), "q": torch.stack([s[1][b, p] for s in states]),
            "k": torch.stack([s[2][b, p] for s in states]), "outputs": torch.stack([s[3][rows] for s in states])}


def extend_states(states, old, new):
    """HSTU.extend_cache_states restated: old rows at the new offsets, new rows zero, q / k as they are."""
    off_o, off_n = torch.cumsum(old, 0) - old, torch.cumsum(new, 0) - new
    out = []
    for v, q, k, o in states:
        nv, no = v.new_zeros((int(new.sum()), v.shape[1])), o.new_zeros((int(new.sum()), o.shape[1]))
        for b in range(old.numel()):
            nv[int(off_n[b]): int(off_n[b] + old[b])] = v[int(off_o[b]): int(off_o[b] + old[b])]
            no[int(off_n[b]): int(off_n[b] + old[b])] = o[int(off_o[b]): int(off_o[b] + old[b])]
        out.append((nv, q.clone(), k.clone(), no))
    return out


# ---- the runs of a case ----------------------------------------------------------------------------------------------------------------
def kinds(name: str):
    c = K.CASES[name]
    return tuple(k for k in KINDS if k != "long" or c.N >= 70)


@functools.lru_cache(maxsize=None)
def run(name: str, kind: str, ts_kind: str = "random") -> Run:
    c = K.CASES[name]
    B, N = c.B, c.N
    g = gen(2000 + sum(map(ord, name + kind)))
    lengths = torch.randint(1, N + 1, (B,), generator=g)
    lengths[0], lengths[1] = N, 1
    counts = torch.ones(B, dtype=torch.int64)
    if kind == "uniform2":
        lengths = lengths.clamp(min=2)
        counts[:] = 2
    if kind == "ragged":
        counts = 1 + torch.arange(B) % 3
        if B > 2:
            lengths[2] = max(int(lengths[2]), 3)
            counts[2] = 3                                   # ... with a padding id inside (below)
        if B > 3:
            lengths[3] = max(int(lengths[3]), 2)
        counts = torch.minimum(counts, lengths)
        counts[0], counts[1] = 2, 1                         # an interior run of sequence 0; the whole length-1 sequence
    if kind == "long":
        counts[0] = 33                                      # two 32-slot tiles, keys past 64
    start = lengths - counts
    if kind == "ragged":
        start[0] = 0 if N < 8 else (N - 1) // 2 - 1         # ends below len - 1 (N >= 4 in every case)
        if B > 4:
            start[4], counts[4] = 0, min(2, int(lengths[4]))   # a run starting at 0
    assert bool((start >= 0).all()) and bool((start + counts <= lengths).all()) and bool((counts >= 1).all())
    ids = torch.randint(1, 501, (B, N), generator=g) * (torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1))
    new_ids = ids.clone()
    b, p = run_rows(lengths, start, counts)
    new_ids[b, p] = torch.randint(1, 501, (b.numel(),), generator=g)
    if kind == "ragged" and B > 2:
        new_ids[2, int(start[2]) + 1] = 0
    return Run(lengths, ids, new_ids, timestamps(B, N, g, ts_kind), start, counts)


def ref_ts(name: str, r: Run):
    return r.ts if K.CASES[name].rel_bias else None


def quantities(cur, states, r: Run):
    return {"current": cur, **touched(states, r.lengths, r.start, r.counts)}


class Direct(NamedTuple):
    states32: list
    ref64: dict
    bars: dict
    dist: dict
    states64: list     # the float64 chain's whole cache afterwards


@functools.lru_cache(maxsize=None)
def direct(name: str, kind: str, ts_kind: str = "random") -> Direct:
    _, cfg, w = K.build(name)
    r = run(name, kind, ts_kind)
    ts = ref_ts(name, r)
    w64 = K._f64(w)
    _, st64 = R.prefill(cfg, w64, r.lengths, r.ids, ts)
    states32 = [tuple(t.float() for t in s) for s in st64]

    def go(weights, dtype, **kw):
        st = [tuple(t.to(dtype, copy=True) for t in s) for s in states32]
        return quantities(chain(cfg, weights, r.lengths, r.new_ids, ts, r.start, r.counts, st, **kw), st, r), st

    ref64, after64 = go(w64, torch.float64)
    bars, dist = K._bars(ref64, go(w, torch.float32)[0], go(w, torch.float32, gemv=R.chain_gemv)[0])
    return Direct(states32, ref64, bars, dist, after64)


def mutant(name: str, kind: str, bug: str) -> dict:
    _, cfg, w = K.build(name)
    r = run(name, kind)
    st = [tuple(t.double() for t in s) for s in direct(name, kind).states32]
    return quantities(chain(cfg, K._f64(w), r.lengths, r.new_ids, ref_ts(name, r), r.start, r.counts, st, bug=bug), st, r)


def routed(w, run_fn):
    """The module route's references, built as K.routed builds them: run_fn(weights, gemv=None) -> quantities runs one scenario from
    its own prefill; -> (float64 reference, bars, distances)."""
    ref64 = run_fn(K._f64(w))
    bars, dist = K._bars(ref64, run_fn(w), run_fn(w, gemv=R.chain_gemv))
    return ref64, bars, dist
