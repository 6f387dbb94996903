"""The geometries, batches, float64 references and bars of the HSTU cached-decode kernel's own tests (tests/test_hstu_decode_kernel.py on
the CPU, tests/test_hstu_decode_kernel_gpu.py on the GPU) -- TEST INFRASTRUCTURE ONLY.

hstu_decode_kernel (csrc/hstu.hip) picks its uvqk matrix-vector product by W = 2 H (dqk + dv): four columns per thread in S = 512 / (W / 4)
interleaved k slices when W % 4 == 0 and the weight is 16-byte aligned (S = 1 from W = 2048), otherwise one column per thread with
eight partial sums; a wave walks heads wave, wave + 8, ...; the jagged row offset is a prefix sum over the preceding lengths across the
workgroup; every row loop strides by 512.  CASES holds the smallest geometry on each side of each of those switches.

The bar of a quantity (the current embeddings, or one kind of cache row the decode writes) comes from references alone:
    2 * max(d_blocked, d_chain) + 1e-6
with d_blocked the distance from float64 of the fp32 restatement (tests/_hstu_cache_ref.py) in torch's summation order and d_chain
that of the same restatement with both matrix-vector products accumulated as one sequential fp32 chain per output column, the least
favourable order a correct kernel could use.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import torch

from tests import _hstu_cache_ref as R
from tests.test_hstu_kernels_gpu import gen, module, timestamps

THREADS = 512              # kDecThreads
MAX_DIM = 1024             # kDecMaxDim
MAX_HEAD = 32              # kDecMaxHead
LDS_BYTES = 60 * 1024      # kDecLdsBytes
QUANTITIES = ("current",) + R.ROWS
SCENARIOS = ("tail", "interior")


class Case(NamedTuple):
    B: int
    N: int
    D: int
    blocks: int
    H: int
    dqk: int
    dv: int
    postproc: str
    buckets: int
    rel_bias: bool

    @property
    def W(self):
        return 2 * self.H * (self.dqk + self.dv)


CASES = {
    "scalar_w30": Case(5, 19, 24, 2, 1, 8, 7, "layer_norm", 128, True),          # W = 30: per-column GEMV, no k remainder
    "scalar_w198": Case(5, 70, 50, 2, 3, 16, 17, "l2_norm", 128, True),          # W = 198: per-column GEMV, remainder 2, p > 64
    "one_slice": Case(3, 17, 64, 1, 16, 32, 32, "layer_norm", 128, True),        # W = 2048 -> S = 1, two rounds of heads
    "one_slice_d1024": Case(2, 5, 1024, 1, 16, 32, 32, "layer_norm", 128, True),  # the longest chains of the sliced GEMV
    "heads9": Case(5, 33, 36, 2, 9, 4, 4, "layer_norm", 255, True),              # S = 14, G S = 504, main k loop skipped, 9 heads
    "dqk_ne_dv": Case(5, 130, 48, 2, 3, 31, 7, "l2_norm", 1, True),              # dqk != dv, one bucket, three lane trips over keys
    "d1024": Case(3, 9, 1024, 1, 2, 32, 32, "layer_norm", 128, True),            # every row loop strided, 1024 Wo columns
    "lds_limit": Case(2, 9, 64, 1, 52, 32, 32, "layer_norm", 0, False),          # the largest accepted H at this D
    "b600": Case(600, 4, 8, 1, 2, 2, 2, "layer_norm", 16, True),                 # prefix sum over > 64 and > 512 sequences; S = 128 > D
    "nobias": Case(5, 70, 64, 2, 8, 8, 8, "l2_norm", 128, False),                # ts_w / pos_w NULL
}
TS_KINDS = {name: ("random",) for name in CASES}
TS_KINDS["scalar_w198"] = ("random", "equal", "decreasing", "huge", "thresholds")
RUNS = [(name, kind, scen) for name in CASES for kind in TS_KINDS[name] for scen in SCENARIOS]
# the route hstu_decode_kernel takes for an aligned weight, by the formulas below: ("sliced", S) or ("per-column", 0)
ROUTES = {"scalar_w30": ("per-column", 0), "scalar_w198": ("per-column", 0), "one_slice": ("sliced", 1), "one_slice_d1024": ("sliced", 1),
          "heads9": ("sliced", 14), "dqk_ne_dv": ("sliced", 8), "d1024": ("sliced", 8), "lds_limit": ("sliced", 1), "b600": ("sliced", 128),
          "nobias": ("sliced", 8)}


def run_id(run):
    return "-".join(run)


# ---- the host code's formulas, restated ------------------------------------------------------------------------------------------
def route(W: int, aligned: bool = True):
    if W % 4 or not aligned:
        return "per-column", 0
    G = W // 4
    return "sliced", (1 if G >= THREADS else THREADS // G)


def lds_bytes(D: int, H: int, dqk: int, dv: int, buckets: int) -> int:
    """hstu_decode_lds_bytes: the thresholds, x, LN(x), y, the attention row, the reduction scratch and the k-slice partial sums."""
    W = 2 * H * (dqk + dv)
    return 8 * buckets + 4 * (2 * D + W + H * dv + THREADS // 64 + max(W, 4 * THREADS))


def supported(N: int, D: int, H: int, dqk: int, dv: int, buckets: int) -> bool:
    """rails_hstu_decode_supported."""
    if N < 1 or not 1 <= D <= MAX_DIM or H < 1 or not 1 <= dqk <= MAX_HEAD or not 1 <= dv <= MAX_HEAD or not 0 <= buckets <= 255:
        return False
    return lds_bytes(D, H, dqk, dv, buckets) <= LDS_BYTES


# (N, D, H, dqk, dv, buckets): the accepted side, then the refused side, of every limit
BOUNDARY_PAIRS = {
    "H": ((9, 64, 52, 32, 32, 0), (9, 64, 53, 32, 32, 0)),
    "dqk": ((9, 64, 2, 32, 32, 0), (9, 64, 2, 33, 32, 0)),
    "dv": ((9, 64, 2, 32, 32, 0), (9, 64, 2, 32, 33, 0)),
    "D": ((9, 1024, 2, 32, 32, 0), (9, 1025, 2, 32, 32, 0)),
    "buckets": ((9, 64, 2, 32, 32, 255), (9, 64, 2, 32, 32, 256)),
    "N": ((1, 64, 2, 32, 32, 0), (0, 64, 2, 32, 32, 0)),
}


# ---- modules, batches, references -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(name: str):
    """-> (HSTU module on the CPU, its HSTUConfig, its float32 weights)."""
    c = CASES[name]
    return module(c.N, c.D, c.blocks, c.H, c.dqk, c.dv, c.postproc, num_buckets=c.buckets, rel_bias=c.rel_bias, seed=len(name) + c.D)


class Batch(NamedTuple):
    lengths: torch.Tensor      # (B,)
    ids: torch.Tensor          # (B, N) the prefill's ids
    new_ids: torch.Tensor      # (B, N) with the delta ids at `positions`
    ts: torch.Tensor           # (B, N) timestamps (handed to the kernel in every case; the references of a case without bias ignore them)
    positions: torch.Tensor    # (B,)


@functools.lru_cache(maxsize=None)
def batch(name: str, kind: str, scen: str) -> Batch:
    c = CASES[name]
    g = gen(1000 + sum(map(ord, name)))
    lengths = torch.randint(1, c.N + 1, (c.B,), generator=g)
    lengths[0], lengths[1] = c.N, 1
    ids = torch.randint(1, 501, (c.B, c.N), generator=g) * (torch.arange(c.N).unsqueeze(0) < lengths.unsqueeze(1))
    ts = timestamps(c.B, c.N, g, kind)
    positions = lengths - 1 if scen == "tail" else (lengths - 1) // 2
    new_ids = ids.clone()
    new_ids[torch.arange(c.B), positions] = torch.randint(1, 501, (c.B,), generator=g)
    if c.B >= 3:
        new_ids[2, positions[2]] = 0                      # a padding id at a delta position
    return Batch(lengths, ids, new_ids, ts, positions)


def ref_ts(name: str, b: Batch):
    """The timestamps the references see: None for a stack without relative bias (the kernel then gets NULL ts_w / pos_w)."""
    return b.ts if CASES[name].rel_bias else None


def _f64(w):
    return {k: v.double() for k, v in w.items()}


def _quantities(cur, states, b: Batch):
    return {"current": cur, **R.touched(states, b.lengths, b.positions)}


def _bars(ref64, blocked, chain):
    dist = {q: (float((blocked[q].double() - ref64[q]).abs().max()), float((chain[q].double() - ref64[q]).abs().max())) for q in QUANTITIES}
    return {q: 2 * max(dist[q]) + 1e-6 for q in QUANTITIES}, dist


class Direct(NamedTuple):
    states32: list     # the cache handed to the kernel: the float64 prefill rounded to fp32
    ref64: dict        # float64 decode from exactly those states: {"current", "v", "q", "k", "outputs"}
    bars: dict
    dist: dict         # per quantity (d_blocked, d_chain)


@functools.lru_cache(maxsize=None)
def direct(name: str, kind: str, scen: str) -> Direct:
    """The C-ABI test's references: every decode starts from the float64 prefill's states rounded to fp32."""
    _, cfg, w = build(name)
    b = batch(name, kind, scen)
    ts = ref_ts(name, b)
    _, st64 = R.prefill(cfg, _f64(w), b.lengths, b.ids, ts)
    states32 = [tuple(t.float() for t in s) for s in st64]

    def dec(weights, dtype, **kw):
        st = [tuple(t.to(dtype, copy=True) for t in s) for s in states32]       # decode() updates its states in place
        return _quantities(R.decode(cfg, weights, b.lengths, b.new_ids, ts, b.positions, st, **kw), st, b)

    ref64 = dec(_f64(w), torch.float64)
    bars, dist = _bars(ref64, dec(w, torch.float32), dec(w, torch.float32, gemv=R.chain_gemv))
    return Direct(states32, ref64, bars, dist)


def direct_mutant(name: str, kind: str, scen: str, bug: str) -> dict:
    """The float64 decode of direct() with one mistake injected."""
    _, cfg, w = build(name)
    b = batch(name, kind, scen)
    st = [tuple(t.double() for t in s) for s in direct(name, kind, scen).states32]
    return _quantities(R.decode(cfg, _f64(w), b.lengths, b.new_ids, ref_ts(name, b), b.positions, st, bug=bug), st, b)


class Routed(NamedTuple):
    ref64: dict
    bars: dict
    dist: dict


@functools.lru_cache(maxsize=None)
def routed(name: str, kind: str, scen: str) -> Routed:
    """The module route's references: the float64 reference and both fp32 restatements start from their own prefills."""
    _, cfg, w = build(name)
    b = batch(name, kind, scen)
    ts = ref_ts(name, b)

    def run(weights, **kw):
        _, st = R.prefill(cfg, weights, b.lengths, b.ids, ts)
        return _quantities(R.decode(cfg, weights, b.lengths, b.new_ids, ts, b.positions, st, **kw), st, b)

    ref64 = run(_f64(w))
    bars, dist = _bars(ref64, run(w), run(w, gemv=R.chain_gemv))
    return Routed(ref64, bars, dist)
