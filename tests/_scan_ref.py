"""Restatement of the bf16 candidate scans (rails_amd/csrc/mol_coarse.hip) and of the key selection behind them (topk_keys.h), in numpy
integers and float64, plus the inputs and the case lists that tests/test_candidate_scans_cpu.py and tests/test_candidate_scans_gpu.py share.

  tables    coarse_table(Ex)    = bf16( bf16( sum_m bf16(Ex[x, m, :]) ) / P_X ), the fp32 sum sequential over m (coarse_table_body)
            component_table(Ex) = bf16(Ex), item-group-major (P_X, N, d)
  queries   coarse_query(Eq, avg)  = bf16( sum_p Eq[b, p, :] )  or  bf16( sum_p Eq / P_Q ), the fp32 sum sequential over p
            component_query(Eq)    = bf16(Eq), row b * P_Q + i
  scores    S = the float64 dot product of the bf16 operands, A = sum |terms|; component rows (b * P_Q + i) * P_X + m
  selection the 64-bit key (orderable(score) << 32) | ~position; "top-k" = the k largest keys: ties by position ascending, no freedom

Two bars:
  * DYADIC inputs.  Eq entries k / 64 (|k| <= 64), table entries j / 128 (|j| <= 128): every operand of the matrix unit is an integer
    multiple of 2^-gq (gq = 6 for summed and component queries, 6 + log2 P_Q for averaged ones) resp. 2^-7 with at most eight
    significant bits, so the products are exact multiples of 2^-(gq + 7), and while sum |terms| < 2^24 * 2^-(gq + 7) every partial sum,
    in any order, is an fp32 number: the fp32 accumulator holds S exactly and the final bf16 rounding is the only rounding of the
    score.  The kernels must then return bf16(S) bit for bit.  No operand is subnormal (the smallest non-zero magnitude is 2^-10).
  * other inputs: admissible(S, A, d) = (bf16(S - e), bf16(S + e)), e = C_DOT u (d + 2) A with the constants of tests/_mol_ref64.py
    (an fp32 chain of d terms loses at most gamma_d of its absolute sum; + 2 for the operand sums that are not exact).  A kernel
    value r passes iff lo <= r <= hi and r is a bf16 number; lo and hi are equal or adjacent bf16 numbers.

`mut` arguments apply the bug classes the CPU file holds both bars against.
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np

from tests._mol_ref64 import C_DOT, U

F32 = np.float32

# name -> (oracle config, P_Q, P_X, d)
SHAPES = {
    "8x8x32": ("amzn-books", 8, 8, 32),
    "8x4x64": ("ml-1m", 8, 4, 64),
    "8x4x128": ("ml-20m", 8, 4, 128),
    "16x16x64": ("synthetic-16x16x64", 16, 16, 64),
}
MUTATIONS = ("trunc", "no_qsum_round", "swap_avg", "swap_groups", "transpose_rows", "ragged_prev", "row32")


# ---- bf16 -----------------------------------------------------------------------------------------------------------------
def bf16_rn(x):
    """bf16_rn of mol_coarse.hip on the uint32 pattern: round to nearest even, NaN kept as is.  fp32 in, fp32 holding bf16 values out."""
    x = np.ascontiguousarray(x, dtype=F32)
    u = x.view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return np.where(nan, u, r).astype(np.uint32).view(F32).reshape(x.shape)


def bf16_trunc(x):
    """the bug class: the low sixteen bits dropped"""
    x = np.ascontiguousarray(x, dtype=F32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32).reshape(x.shape)


def bf16_from_f64(x, trunc: bool = False):
    """The bf16 number nearest to a float64 (ties to even), as fp32 -- one rounding, not float64 -> fp32 -> bf16.  Normal range only."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))          # |m| in [0.5, 1): eight significant bits = m * 256 rounded to an integer
    q = m * 256.0
    with np.errstate(over="ignore"):                          # past the largest bf16 number: inf, as in fp32
        return np.ldexp(np.trunc(q) if trunc else np.rint(q), e - 8).astype(F32)


def is_bf16(x) -> np.ndarray:
    return (np.ascontiguousarray(x, dtype=F32).view(np.uint32) & np.uint32(0xFFFF)) == 0


def _rnd(mut):
    return bf16_trunc if mut == "trunc" else bf16_rn


# ---- tables and queries -----------------------------------------------------------------------------------------------------
def coarse_table(ex, mut: Optional[str] = None):
    """ex (N, P_X, d) fp32 -> (N, d) fp32 holding bf16 values.  mut: "trunc", "table_no_inner" (the inner bf16 rounding dropped)."""
    ex = np.asarray(ex, dtype=F32)
    rnd = _rnd(mut)
    acc = np.zeros((ex.shape[0], ex.shape[2]), dtype=F32)
    for m in range(ex.shape[1]):
        acc = acc + rnd(ex[:, m, :])                            # fp32 adds, m = 0 .. P_X - 1 in order
    inner = acc if mut == "table_no_inner" else rnd(acc)
    return rnd(inner / F32(ex.shape[1]))


def component_table(ex, mut: Optional[str] = None):
    """ex (N, P_X, d) fp32 -> (P_X, N, d) fp32 holding bf16 values"""
    return np.ascontiguousarray(_rnd(mut)(np.asarray(ex, dtype=F32)).transpose(1, 0, 2))


def coarse_query(eq, avg: bool, mut: Optional[str] = None):
    """eq (B, P_Q, d) fp32 -> (B, d).  mut: "trunc", "no_qsum_round", "swap_avg"."""
    eq = np.asarray(eq, dtype=F32)
    if mut == "swap_avg":
        avg = not avg
    acc = np.zeros((eq.shape[0], eq.shape[2]), dtype=F32)
    for p in range(eq.shape[1]):
        acc = acc + eq[:, p, :]
    v = acc / F32(eq.shape[1]) if avg else acc
    return v if mut == "no_qsum_round" else _rnd(mut)(v)


def component_query(eq, mut: Optional[str] = None):
    """eq (B, P_Q, d) fp32 -> (B * P_Q, d), row b * P_Q + i.  mut: "trunc", "transpose_rows" (row r reads (i, b) = divmod(r, B))."""
    eq = np.asarray(eq, dtype=F32)
    q = _rnd(mut)(eq)
    if mut == "transpose_rows":
        q = q.transpose(1, 0, 2)
    return np.ascontiguousarray(q).reshape(eq.shape[0] * eq.shape[1], eq.shape[2])


# ---- scores -----------------------------------------------------------------------------------------------------------------
def dots(q, t, mut: Optional[str] = None, want_abs: bool = True):
    """q (R, d), t (N, d) -> S (R, N) float64 and A = sum |terms| (None unless wanted).  mut: "row32" (query row 32 reads row 0's
    operands), "ragged_prev" (the columns of a ragged last tile of 32 hold the previous tile's scores)."""
    q, t = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if mut == "row32" and q.shape[0] > 32:
        q = q.copy()
        q[32] = q[0]
    s = q @ t.T
    a = np.abs(q) @ np.abs(t).T if want_abs else None
    n, r = s.shape[1], s.shape[1] % 32
    if mut == "ragged_prev" and r and n > 32:
        s[:, n - r:] = s[:, n - r - 32:n - 32]
    return s, a


def coarse_scores(eq, table, avg: bool, mut: Optional[str] = None, want_abs: bool = True):
    """-> (S, A) (B, N) float64: what rails_mol_coarse_score rounds to bf16"""
    return dots(coarse_query(eq, avg, mut), table, mut, want_abs)


def component_scores(eq, table3, mut: Optional[str] = None, want_abs: bool = True):
    """table3 (P_X, N, d) -> (S, A) (B * P_Q * P_X, N) float64, row (b * P_Q + i) * P_X + m.  mut also: "swap_groups" (m <-> m ^ 1)."""
    q = component_query(eq, mut)
    px = table3.shape[0]
    order = [m ^ 1 for m in range(px)] if mut == "swap_groups" else list(range(px))
    parts = [dots(q, table3[m], mut, want_abs) for m in order]
    s = np.stack([p[0] for p in parts], axis=1).reshape(q.shape[0] * px, -1)
    a = np.stack([p[1] for p in parts], axis=1).reshape(q.shape[0] * px, -1) if want_abs else None
    return s, a


def rounded(s, mut: Optional[str] = None):
    """the kernel's output for an accumulator that holds S: bf16(S) as fp32"""
    return bf16_from_f64(s, trunc=mut == "trunc")


def admissible(s, a, d: int):
    """-> (lo, hi), fp32 holding bf16 values, equal or adjacent"""
    e = C_DOT * U * (d + 2) * a
    return bf16_from_f64(s - e), bf16_from_f64(s + e)


def passes(r, lo, hi) -> np.ndarray:
    return (lo <= r) & (r <= hi) & is_bf16(r)


# ---- selection ----------------------------------------------------------------------------------------------------------------
def orderable(scores):
    u = np.ascontiguousarray(scores, dtype=F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unorderable(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def topk_keys(scores, k: int, mut: Optional[str] = None):
    """scores (R, N) fp32 -> (scores (R, k) fp32, positions (R, k) int64): the k largest keys of every row, descending.
    mut: "ties_desc" (the position itself in the low word: ties by position descending)."""
    scores = np.ascontiguousarray(scores, dtype=F32)
    n = scores.shape[1]
    pos = np.arange(n, dtype=np.uint32)
    low = pos if mut == "ties_desc" else ~pos
    keys = (orderable(scores).astype(np.uint64) << np.uint64(32)) | low.astype(np.uint64)[None, :]
    if k < n:
        keys = np.partition(keys, n - k, axis=1)[:, n - k:]
    keys = np.sort(keys, axis=1)[:, ::-1]
    lo32 = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return unorderable((keys >> np.uint64(32)).astype(np.uint32)), (lo32 if mut == "ties_desc" else ~lo32).astype(np.int64)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _rng(*key) -> np.random.Generator:
    return np.random.default_rng([int(v) for v in key])


def assert_exact(q, t, gq: int, gt: int = 7) -> None:
    """The exactness precondition, in int64: q on the 2^-gq grid, t on the 2^-gt grid, both bf16 numbers, and sum |q t| / 2^-(gq + gt) < 2^24
    for every (row, item)."""
    q, t = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(-1, np.shape(t)[-1])
    qi, ti = np.abs(q) * 2.0 ** gq, np.abs(t) * 2.0 ** gt
    assert np.array_equal(qi, np.rint(qi)) and np.array_equal(ti, np.rint(ti)), "operands off their grid"
    assert is_bf16(q.astype(F32)).all() and is_bf16(t.astype(F32)).all()
    assert (qi.astype(np.int64) == qi).all() and (ti.astype(np.int64) == ti).all()
    # the matrix product in float64 is exact here (every entry < 2^53), so its int64 image is the int64 product.  First the bound with
    # the column-wise largest |q| (one row instead of all of them); the full product only where that bound does not settle it.
    worst = (qi.max(axis=0, keepdims=True) @ ti.T).astype(np.int64).max()
    if int(worst) >= (1 << 24):
        worst = (qi @ ti.T).astype(np.int64).max()
    assert int(worst) < (1 << 24), int(worst)


def dyadic_eq(rng, b: int, pq: int, d: int, nonneg: bool = False):
    return (rng.integers(0 if nonneg else -64, 65, size=(b, pq, d)) / 64.0).astype(F32)


def dyadic_rows(rng, n: int, d: int, lo: int = -128, hi: int = 128):
    return (rng.integers(lo, hi + 1, size=(n, d)) / 128.0).astype(F32)


def unit_rows(rng, *shape):
    x = rng.standard_normal(shape)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F32)


class ScoreCase(NamedTuple):
    entry: str      # "coarse" | "component"
    shape: str
    B: int
    N: int

    @property
    def dims(self):
        return SHAPES[self.shape][1:]


def component_batches(shape: str):
    """B with B * P_Q in {8, 40, 256} ({8, 40, 128} at d = 128): less than one query tile, two tiles with a ragged second, the fused limit.
    P_Q = 16 has no such B for 8 and 40: 16 and 48 rows are the same three tilings."""
    _, pq, _, d = SHAPES[shape]
    return (1, 3, 16) if pq == 16 else ((1, 5, 16) if d == 128 else (1, 5, 32))


COARSE_BATCHES = (1, 5, 32, 33, 128)
SCORE_N = (1, 31, 32, 33, 1000)
# a wave takes more than one trip of tiles: the grid is capped at 2 048 / groups workgroups of 4 waves x 2 tiles (d = 32)
MULTI_TRIP = (ScoreCase("coarse", "8x8x32", 3, 600_001), ScoreCase("component", "8x8x32", 1, 70_001))
SCORE_CASES = tuple(ScoreCase("coarse", s, b, n) for s in SHAPES for b in COARSE_BATCHES for n in SCORE_N) + \
    tuple(ScoreCase("component", s, b, n) for s in SHAPES for b in component_batches(s) for n in SCORE_N) + MULTI_TRIP
RANDOM_CASES = tuple(ScoreCase(e, s, 33, 4000) for e in ("coarse", "component") for s in SHAPES)


def applicable(case: ScoreCase, mut: str) -> bool:
    pq, px, _ = case.dims
    rows = case.B if case.entry == "coarse" else case.B * pq
    if mut == "trunc":
        return True
    if mut in ("no_qsum_round", "swap_avg"):
        return case.entry == "coarse"
    if mut == "swap_groups":
        return case.entry == "component"
    if mut == "transpose_rows":
        return case.entry == "component" and case.B > 1
    if mut == "ragged_prev":
        return case.N % 32 != 0 and case.N > 32
    if mut == "row32":
        return rows > 32
    raise ValueError(mut)


def model(case: ScoreCase, eq, table, avg: bool = False, mut: Optional[str] = None, want_abs: bool = False):
    return coarse_scores(eq, table, avg, mut, want_abs) if case.entry == "coarse" else component_scores(eq, table, mut, want_abs)


def modes(case: ScoreCase):
    return (False, True) if case.entry == "coarse" else (False,)


def _dyadic_draw(case: ScoreCase, seed: int):
    pq, px, d = case.dims
    rng = _rng(1, list(SHAPES).index(case.shape), case.entry == "coarse", case.B, case.N, seed)
    eq = dyadic_eq(rng, case.B, pq, d)
    table = dyadic_rows(rng, case.N, d) if case.entry == "coarse" else dyadic_rows(rng, px * case.N, d).reshape(px, case.N, d)
    return eq, table


def check_exact(case: ScoreCase, eq, table) -> None:
    pq = case.dims[0]
    if case.entry == "coarse":
        assert_exact(coarse_query(eq, False), table, 6)
        assert_exact(coarse_query(eq, True), table, 6 + pq.bit_length() - 1)
    else:
        assert_exact(component_query(eq), table, 6)


def is_sharp(case: ScoreCase, eq, table) -> bool:
    """every applicable bug class changes at least one score the exact comparison looks at (in every mode)"""
    for avg in modes(case):
        ref = rounded(model(case, eq, table, avg)[0])
        for mut in MUTATIONS:
            if applicable(case, mut) and np.array_equal(rounded(model(case, eq, table, avg, mut)[0], mut), ref):
                return False
    return True


@functools.lru_cache(maxsize=4)
def dyadic_inputs(case: ScoreCase):
    """Eq (B, P_Q, d) and the table ((N, d) or (P_X, N, d)) of a dyadic case: the first draw on which the comparison is sharp.  A case of a
    single score can hide a bug class by chance (a sum that is a bf16 number survives truncation); the draw is chosen by looking at the
    restatement alone."""
    for seed in range(256):
        eq, table = _dyadic_draw(case, seed)
        if is_sharp(case, eq, table):
            check_exact(case, eq, table)
            return eq, table
    raise AssertionError(f"no sharp draw for {case}")


@functools.lru_cache(maxsize=2)
def random_inputs(case: ScoreCase):
    """unit-norm Gaussian Eq rows and component embeddings; the tables are the restatement's"""
    pq, px, d = case.dims
    rng = _rng(2, list(SHAPES).index(case.shape), case.B, case.N)
    eq, ex = unit_rows(rng, case.B, pq, d), unit_rows(rng, case.N, px, d)
    return eq, (coarse_table(ex) if case.entry == "coarse" else component_table(ex))


# ---- inputs of the fused top-k tests ------------------------------------------------------------------------------------------
COARSE_TOPK_SIZES = ((500, 1), (4000, 100), (30_000, 1000))        # (N, K'): the smallest corpora the fused coarse plan accepts
COMPONENT_TOPK_SIZES = ((1000, 5), (4000, 100), (16_000, 500))    # (N, k_g)
COARSE_TOPK_BATCHES = (1, 33, 128)
SELECT_KINDS = ("dups", "front", "last_class", "few")


def component_topk_batches(shape: str):
    """B with B * P_Q at one query tile and at the fused limit (256 rows, 128 at d = 128)"""
    _, pq, _, d = SHAPES[shape]
    return (32 // pq, (128 if d == 128 else 256) // pq)


class SelectCase(NamedTuple):
    entry: str
    shape: str
    B: int
    N: int
    k: int
    kind: str       # "dups" | "front" | "last_class" | "few"

    @property
    def dims(self):
        return SHAPES[self.shape][1:]


def select_cases():
    """every shape x (N, k) x batch x kind"""
    out = [SelectCase("coarse", s, b, n, k, kind) for kind in SELECT_KINDS for s in SHAPES for n, k in COARSE_TOPK_SIZES for b in COARSE_TOPK_BATCHES]
    out += [SelectCase("component", s, b, n, k, kind) for kind in SELECT_KINDS for s in SHAPES for n, k in COMPONENT_TOPK_SIZES
            for b in component_topk_batches(s)]
    return tuple(out)


def winners_last_class(n: int, k: int) -> np.ndarray:
    """k positions in the last (ragged) tile of 32 and the tiles of its residue class t % 16 only, from the end backwards"""
    assert n % 32 != 0
    tiles = np.arange((n - 1) // 32, -1, -16)
    pos = np.concatenate([np.arange(t * 32, min(t * 32 + 32, n)) for t in tiles])
    assert len(pos) >= k
    return pos[:k]


@functools.lru_cache(maxsize=2)
def select_inputs(case: SelectCase):
    """-> (Eq, table, n).  Dyadic, exact (asserted):
    dups        many distinct values, then the item at the k-th place of a few rows copied to three more positions: ties across the k-th place
    front       non-negative queries; k winner items (entries in [1/2, 1], the others in [-1, 1/4]) at positions 0 .. k - 1
    last_class  the same with the winners in the ragged last tile and its residue class of tiles (n + 1 items where 32 divides n)
    few         every item a copy of one row (of one of two rows from 8 192 items on): all items tied at one or two scores per query"""
    pq, px, d = case.dims
    n = case.N + 1 if case.kind == "last_class" and case.N % 32 == 0 else case.N
    rng = _rng(3, list(SHAPES).index(case.shape), case.entry == "coarse", case.B, case.N, case.k, SELECT_KINDS.index(case.kind))
    g = 1 if case.entry == "coarse" else px
    eq = dyadic_eq(rng, case.B, pq, d, nonneg=case.kind in ("front", "last_class"))
    if case.kind in ("front", "last_class"):
        win = np.arange(case.k) if case.kind == "front" else winners_last_class(n, case.k)
        t = dyadic_rows(rng, g * n, d, -128, 32).reshape(g, n, d)
        t[:, win] = dyadic_rows(rng, g * case.k, d, 64, 128).reshape(g, case.k, d)
    elif case.kind == "few":
        distinct = 1 if n < 8192 else 2      # every score level then holds more items than a candidate list (or, below 4 096 items, than its sub-lists)
        t = dyadic_rows(rng, g * distinct, d).reshape(g, distinct, d)[:, rng.integers(0, distinct, size=n)]
    else:
        t = dyadic_rows(rng, g * n, d).reshape(g, n, d)
        probe = ScoreCase(case.entry, case.shape, min(case.B, 2), n)
        sc = rounded(model(probe, eq[:probe.B], t[0] if g == 1 else t)[0])
        for row in range(min(sc.shape[0], 4)):
            x = int(topk_keys(sc[row:row + 1], case.k)[1][0, -1])
            t[:, rng.choice(n, size=3, replace=False)] = t[:, x:x + 1]
    table = np.ascontiguousarray(t[0] if g == 1 else t)
    check_exact(ScoreCase(case.entry, case.shape, case.B, n), eq, table)
    return eq, table, n


def select_scores(case: SelectCase, eq, table, avg: bool = False):
    """the exact fp32 scores (bf16 values) of a select case, (rows, n)"""
    return rounded(model(ScoreCase(case.entry, case.shape, case.B, table.shape[-2]), eq, table, avg)[0])
