"""The shape sweep of the generic scoring route (rails_amd/csrc/mol_generic.hip): shapes that reach every instantiation
mol_generic_score_kernel<TL, RES, ..> a launch can select and every limit of the envelope, two weight sets per shape, synthetic inputs,
and the launch formulas of generic_score restated (tests/test_generic_sweep_cpu.py proves the coverage from them without a device).

  shape      (P_Q, P_X, d, H); L = P_Q P_X, TL = ceil(L / 32); the pair-gate weights are resident in LDS when they fit next to the cl buffers
  "plain"    oracle.mol_oracle.synthetic_weights(cfg, seed)
  "flat"     the same with the pair gate's output layer and the query gate's output layer scaled by 2^-6: the gate values w are then close to
             0, the softmax close to uniform, and a padded logit that entered it with w = 0 takes a visible share of the mass (with plain
             weights the real w are large and the share is below the bars: figures in tests/test_generic_sweep_cpu.py)
"""
import functools

import torch

from oracle import mol_oracle as O
from oracle.mol_oracle import MoLConfig
from tests import _mol_ref64 as R

# (P_Q, P_X, d, H)                what it is there for
SWEEP = (
    (2, 1, 1, 1),               # smallest of everything
    (3, 7, 5, 33),              # L % 4 = 1, d = 5, Hp = 64 for H = 33
    (33, 1, 9, 40),             # second query block of one row
    (7, 9, 3, 300),             # L % 4 = 3, d = 3; streamed
    (40, 2, 20, 50),            # TL 3
    (5, 19, 12, 160),           # TL 3, streamed
    (6, 11, 256, 40),           # d at its limit
    (9, 13, 7, 96),             # LDS exactly 160 KiB
    (9, 13, 7, 97),             # one hidden unit past the boundary: streamed
    (3, 37, 6, 128),            # P_X > 32
    (33, 4, 12, 64),            # LDS exactly 160 KiB
    (33, 4, 12, 512),           # H at its limit
    (13, 13, 7, 31),            # TL 6, H < 32
    (6, 31, 10, 70),            # TL 6, streamed
    (51, 4, 9, 64),             # TL 7
    (51, 5, 9, 64),             # L = 255
    (1, 256, 8, 32),            # P_X = 256
    (256, 1, 8, 1),             # eight query blocks, H = 1
    (16, 16, 256, 512),         # every limit at once
)
KINDS = ("plain", "flat")
FLAT_KEYS = ("_gating_fn._qi_partial_module.3.weight", "_gating_fn._qi_partial_module.3.bias", "_gating_fn._query_only_partial_module.2.weight")
FLAT_SCALE = 2.0 ** -6
B, N, N_CAND = 3, 131, 45      # two 128-item blocks, the second holding 3 items: partial wave tiles and idle waves
PERSISTENT = ((3, 7, 5, 33), (33, 1, 9, 40), (9, 13, 7, 96), (51, 5, 9, 64))      # several units per workgroup (two of them at two workgroups per CU)

# the generic two-pass tables (gen_table_width), one shape per padded width and the width that equals d; NO_TABLE: d = 129, no table at all
TABLE_SHAPES = {"s_4x4x7": (4, 4, 7, 16), "s_4x4x33": (4, 4, 33, 16), "s_4x2x72": (4, 2, 72, 16), "s_2x3x128": (2, 3, 128, 16)}
NO_TABLE = (4, 2, 129, 16)

MAX_LDS = 160 * 1024
BLOCK_ITEMS = 128


def name_of(shape):
    pq, px, d, h = shape
    return f"{pq}x{px}x{d}_h{h}"


def config(shape):
    pq, px, d, h = shape
    return MoLConfig(32, 24, d, pq, px, query_hidden_dim=48, gating_query_hidden_dim=16, gating_item_hidden_dim=16, gating_qi_hidden_dim=h)


@functools.lru_cache(maxsize=None)
def weights(shape, kind):
    """The weight set `kind` of a shape (shared between tests: never written to)."""
    w = O.synthetic_weights(config(shape), seed=1 + SWEEP.index(shape) if shape in SWEEP else 100 + shape[2])
    if kind == "flat":
        for key in FLAT_KEYS:
            w[key] = w[key] * FLAT_SCALE
    else:
        assert kind == "plain"
    return w


def raw_inputs(shape, batch=B, n=N):
    """(q (batch, 32), X (n, 24)) fp32 on the CPU"""
    cfg = config(shape)
    return O.synthetic_queries(cfg, batch, seed=9), torch.from_numpy(O.hash_item_table(3, 0, n, cfg.item_embedding_dim))


@functools.lru_cache(maxsize=None)
def operands(shape, kind):
    """(Eq, Ex, gq, gi) of raw_inputs: the float64 prologue and index build rounded to fp32 (what a device-free test feeds the pair stage)."""
    cfg, w = config(shape), weights(shape, kind)
    q, X = raw_inputs(shape)
    (eq, _), (gq, _) = R.prologue64(cfg, w, q)
    (ex, _), (gi, _) = R.index64(cfg, w, X)
    return eq.float(), ex.float(), gq.float(), gi.float()


# ---- generic_score's launch, restated -------------------------------------------------------------------------------------------------------
def up(x, m):
    return (x + m - 1) // m * m


def launch(shape):
    """The padded axes and the instantiation: dp, Lq, Lp, Hp, TL, res (weights resident in LDS), lds (bytes of the launch)."""
    pq, px, d, h = shape
    L = pq * px
    lp, hp = up(L, 32), up(h, 32)
    cl_bytes, w_bytes = 512 * lp, 8 * hp * lp      # 4 waves x Lp x 32 floats; W1 and W2, Hp x Lp floats each
    res = cl_bytes + w_bytes <= MAX_LDS
    return {"L": L, "dp": up(d, 8), "Lq": up(L, 4), "Lp": lp, "Hp": hp, "TL": lp // 32, "res": res, "lds": cl_bytes + (w_bytes if res else 0)}


def table_width(d):
    """gen_table_width: the bf16 tables' padded width, 0 where there is none"""
    return 32 if d <= 32 else 64 if d <= 64 else 128 if d <= 128 else 0


def units(batch, n):
    return batch * ((n + BLOCK_ITEMS - 1) // BLOCK_ITEMS)


def max_grid(shape, n_cu):
    return n_cu * (2 if launch(shape)["lds"] <= MAX_LDS // 2 else 1)


def grid(shape, batch, n, n_cu):
    return min(units(batch, n), max_grid(shape, n_cu))
