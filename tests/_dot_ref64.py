"""Float64 restatement of the dot-product path (rails_amd/csrc/mips.hip) for tests/test_dot_product_gpu.py: references, the per-pair bound,
the tile layout of engine.MipsIndex in plain torch indexing, and the inputs the cases share.

Bound.  rails_mips_score and rails_dot_rowwise are fp32 FMA chains of length D: v_mfma_f32_32x32x2_f32 is a chain of round-to-nearest fmaf
(tests/test_proved_gpu.py::test_fp32_mfma_is_a_chain_of_fmas), the row-wise kernel is a loop of __builtin_fmaf, and the zero padding of the
MFMA operands (k in [D, Dp), items past N, queries past B) adds exact zeros.  For a chain of D fmaf in any order,

    |got - ref| <= gamma_D * mag,    gamma_D = D u / (1 - D u),  u = 2^-24,  ref = <q, x>,  mag = <|q|, |x|>      (Higham, Lemma 3.1)

with ref and mag taken in float64 (their own error, <= D 2^-53 mag, is nine orders below the bound).  There is no floor term: the inputs
are drawn so that no product or partial sum is subnormal.  products_stay_normal states the condition that is checked: with every non-zero
|q_k x_k| >= 2^-78 each exact product is a multiple of 2^-48 2^-78 = 2^-126, so by induction every partial sum of the chain is, and a
non-zero one is a normal fp32 number.

`mut` applies the bug classes the CPU tests of tests/test_dot_product_gpu.py hold the bound against.
"""
from __future__ import annotations

import torch

from oracle import mol_oracle as O

U = 2.0 ** -24
TILE = 32
MIN_PRODUCT = 2.0 ** -78


def gamma(D: int) -> float:
    return D * U / (1.0 - D * U)


def padded(D: int) -> int:
    return -(-D // 8) * 8


def index_floats(D: int, N: int) -> int:
    """rails_mips_index_floats(D, N), restated."""
    return -(-N // TILE) * TILE * padded(D)


def _d(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", torch.float64)


# ----------------------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------------------
def dot64(q: torch.Tensor, X: torch.Tensor, mut: str = None):
    """q (B, D), X (N, D) fp32 -> (ref (B, N), bound (B, N)) float64.  mut (the value only; the bound stays that of the true operation):
    "drop_last_k"   the last k is not accumulated;
    "half_at_D2"    the item operand's second lane half starts at D / 2 instead of Dp / 2 (the queries' stays right);
    "pad_next_row"  k in [D, Dp) is not zeroed: both operands read on into the first elements of their next row (the last row wraps)."""
    q, X = _d(q), _d(X)
    D = q.shape[1]
    Dp = padded(D)
    bound = gamma(D) * (q.abs() @ X.abs().T)
    if mut is None:
        return q @ X.T, bound
    if mut == "drop_last_k":
        return q[:, : D - 1] @ X[:, : D - 1].T, bound
    if mut == "half_at_D2":
        h = Dp // 2
        qp = torch.zeros(q.shape[0], Dp, dtype=torch.float64)
        qp[:, :D] = q
        Xm = torch.zeros(X.shape[0], Dp, dtype=torch.float64)
        Xm[:, : min(h, D)] = X[:, : min(h, D)]
        n_hi = min(h, D - D // 2)
        Xm[:, h : h + n_hi] = X[:, D // 2 : D // 2 + n_hi]
        return qp @ Xm.T, bound
    if mut == "pad_next_row":
        extra = Dp - D
        return q @ X.T + torch.roll(q, -1, 0)[:, :extra] @ torch.roll(X, -1, 0)[:, :extra].T, bound
    raise ValueError(mut)


def rowwise64(q: torch.Tensor, items: torch.Tensor, mut: str = None):
    """q (Bq, D), items (B_I, X, D), Bq = B_I r -> (ref (Bq, X), bound): <q[bq], items[bq // r][x]>.  mut "mod_bi": items[bq % B_I]."""
    q, items = _d(q), _d(items)
    Bq, D = q.shape
    BI = items.shape[0]
    r = Bq // BI
    rows = torch.arange(Bq)
    own = items[rows // r]
    bound = gamma(D) * torch.einsum("bd,bxd->bx", q.abs(), own.abs())
    src = own if mut is None else items[rows % BI]
    return torch.einsum("bd,bxd->bx", q, src), bound


def products_stay_normal(q: torch.Tensor, X: torch.Tensor) -> bool:
    """Every non-zero product q[b][k] X[x][k] is at least 2^-78 in magnitude (module docstring: then no partial sum is subnormal)."""
    aq, ax = _d(q).abs(), _d(X).abs()
    big = torch.finfo(torch.float64).max
    mq = torch.where(aq > 0, aq, torch.full_like(aq, big)).amin(0)      # per k: the smallest non-zero |q|, |x|
    mx = torch.where(ax > 0, ax, torch.full_like(ax, big)).amin(0)
    return bool(((mq * mx) >= MIN_PRODUCT).all())


# ----------------------------------------------------------------------------------------------------------------------------
# the index layout, and the gather formula, in plain indexing
# ----------------------------------------------------------------------------------------------------------------------------
def _coords(N: int, D: int):
    Dp = padded(D)
    tiles = -(-N // TILE)
    t = torch.arange(tiles).view(-1, 1, 1, 1)
    sc = torch.arange(Dp // 8).view(1, -1, 1, 1)
    lane = torch.arange(64).view(1, 1, -1, 1)
    j = torch.arange(4).view(1, 1, 1, -1)
    item = (TILE * t + (lane & 31)).expand(tiles, Dp // 8, 64, 4)
    k = ((lane >> 5) * (Dp // 2) + 4 * sc + j).expand(tiles, Dp // 8, 64, 4)
    return item, k


def mips_layout(X: torch.Tensor, D: int = None) -> torch.Tensor:
    """The floats of engine.MipsIndex(X).buf: for tile t, sub-chunk sc < Dp / 8, lane < 64 and j < 4 the float at
    ((t Dp / 8 + sc) 64 + lane) 4 + j is X[32 t + (lane & 31)][(lane >> 5) Dp / 2 + 4 sc + j], and zero where the item is at or past N or
    k is at or past D.  Copies: the bits of X (fp32; another dtype as X.float())."""
    X = X.detach().cpu().float()
    N, D = X.shape[0], X.shape[1] if D is None else D
    item, k = _coords(N, D)
    ok = (item < N) & (k < D)
    out = torch.zeros(item.shape, dtype=torch.float32)
    out[ok] = X[item[ok], k[ok]]
    out = out.reshape(-1)
    assert out.numel() == index_floats(D, N)
    return out


def gather_rows(buf: torch.Tensor, N: int, D: int, pos: torch.Tensor) -> torch.Tensor:
    """mips_gather_rows_kernel, restated: rows[u][k] = buf[(p >> 5) 32 Dp + (sc 64 + hi 32 + (p & 31)) 4 + j] with hi = k >= Dp / 2,
    r = k - hi Dp / 2, sc = r >> 2, j = r & 3; zeros for a position outside [0, N)."""
    Dp = padded(D)
    k = torch.arange(D).view(1, -1)
    p = pos.view(-1, 1)
    hi = (k >= Dp // 2).long()
    r = k - hi * (Dp // 2)
    sc, j = r >> 2, r & 3
    inside = (p >= 0) & (p < N)
    pc = torch.where(inside, p, torch.zeros_like(p))
    rows = buf[(pc >> 5) * (TILE * Dp) + (sc * 64 + hi * 32 + (pc & 31)) * 4 + j]
    return torch.where(inside, rows, torch.zeros_like(rows))


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------------
def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def table(N: int, D: int, seed: int, first: int = 0) -> torch.Tensor:
    """Hashed item table, sigma 0.02: every value a multiple of 5.3e-7 (oracle.mol_oracle.hash_item_table)."""
    return torch.from_numpy(O.hash_item_table(seed, first, N, D))


def queries(B: int, D: int, seed: int) -> torch.Tensor:
    """Layer-normed Gaussian rows (what a SASRec encoder hands over); plain Gaussian below D = 8, where a layer norm leaves nothing."""
    q = torch.randn(B, D, generator=gen(seed))
    return torch.nn.functional.layer_norm(q, (D,)) if D >= 8 else q


def score_inputs(B: int, N: int, D: int, kind: str = "plain"):
    """(q, X) of a rails_mips_score case.  "x1e3": both operands scaled by 1e3.  "cancel": the second half of every item row is the
    negation of its first half plus a term of 1e-3 of its size, and the queries repeat their first half: mag stays, ref loses three digits."""
    q, X = queries(B, D, seed=1000 * D + B), table(N, D, seed=D + 7 * N)
    if kind == "x1e3":
        q, X = q * 1e3, X * 1e3
    elif kind == "cancel":
        h = D // 2
        X, q = X.clone(), q.clone()
        X[:, h : 2 * h] = -X[:, :h] + 1e-3 * table(N, h, seed=D + 7 * N + 1)
        q[:, h : 2 * h] = q[:, :h]
    elif kind != "plain":
        raise ValueError(kind)
    return q, X


def rowwise_inputs(BI: int, r: int, X: int, D: int):
    """(q (B_I r, D), items (B_I, X, D)): batch b's items are scaled by 4^b, so that another batch's items never pass for the right ones."""
    q = queries(BI * r, D, seed=BI * 1000 + r * 100 + X + D)
    items = table(BI * X, D, seed=BI + 3 * r + 5 * X + 7 * D).view(BI, X, D) * (4.0 ** torch.arange(BI)).view(BI, 1, 1)
    return q, items


def topk_inputs(B: int, N: int, D: int):
    """(q, X) of the top-k cases: every fourth item (3, 7, 11, ...) is a copy of the row N // 2 + 1 places on (mod N, never itself a copy's
    copy: the source is moved off the 3 (mod 4) class), so every copy ties with its source exactly."""
    q, X = queries(B, D, seed=N + D), table(N, D, seed=N).clone()
    dup = torch.arange(3, N, 4)
    src = (dup + N // 2 + 1) % N
    src = torch.where(src % 4 == 3, (src + 1) % N, src)
    X[dup] = X[src]
    return q, X, dup, src


def topk_rule(ref: torch.Tensor, bound: torch.Tensor, got_pos: torch.Tensor, k: int):
    """The float64 rule a returned set is held to.  ref, bound (B, N) float64, got_pos (B, k) positions.  With eps the largest bound of the
    row and t the k-th largest float64 score: every item scoring above t + 2 eps is returned, no returned item scores below t - 2 eps.
    -> (missing, intruding): how many (row, item) pairs break either half."""
    eps = bound.amax(1, keepdim=True)
    t = torch.sort(ref, dim=1, descending=True).values[:, k - 1 : k]
    returned = torch.zeros_like(ref, dtype=torch.bool)
    returned.scatter_(1, got_pos, True)
    missing = int(((ref > t + 2 * eps) & ~returned).sum())
    intruding = int(((ref < t - 2 * eps) & returned).sum())
    return missing, intruding


def band_share(ref: torch.Tensor, bound: torch.Tensor, k: int):
    """-> (share of the (row, rank) places of the float64 ranking whose score lies within 2 eps of the row's k-th score -- the places the
    rule says nothing about --, share of the rows whose returned SET the rule leaves open: more items in the band than places for them)."""
    eps = bound.amax(1, keepdim=True)
    t = torch.sort(ref, dim=1, descending=True).values[:, k - 1 : k]
    band = (ref - t).abs() <= 2 * eps
    above = (ref > t + 2 * eps).sum(1)
    open_rows = (above + band.sum(1)) > k
    return float(band.double().mean()), float(open_rows.double().mean())
