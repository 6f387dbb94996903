"""MoL kernels (mol_query.hip, mol_index.hip, the fp32 scoring shells, rails_mol_gate_combine, rails_glu_f32) one by one against the
float64 restatement of tests/_mol_ref64.py, on every launch route and on both sides of the lines the host code draws between them.

Every float result is held to a per-element (per-pair) bound built from float64 absolute sums with u = 2^-24; the constants are named at
the top of tests/_mol_ref64.py.  Each stage is checked on the fp32 inputs its kernel read: the prologue on q and the weights, the index
build on X and the weights, the scoring shells on the engine's own plain Eq, Ex, gq and gi.  Copies of the packed index (the row-major
copy, the gathered candidate tiles) are exact.

Routes are decided by geometry (mol_query.hip query_prologue, mol_score.hip use_small_units, mol_score_shell.h choose_variant): each
case states its route from the same formulas, restated below, with n_cu read from the device, and asserts it.  Geometry reaches every
route, so the RAILS_SCORE_VARIANT / RAILS_PROLOGUE overrides are not used.

The CPU tests (unmarked) apply the bug classes a kernel could plausibly have -- the eps clamp on the squared norm, rsqrt(ss + eps), a
tanh GELU, a dropped pair-gate bias, silu(gq gi) + gqi, a padding row's gi or gq -- to the float64 reference at the inputs the GPU cases
use, check that each lands outside its bar, and print whether the fp32-oracle bars of tests/test_gpu_parity.py (LOGIT_TOL on logits,
STAGE_TOL on Eq / Ex) would have let it through.
"""
import dataclasses
import functools

import pytest
import torch

from oracle import mol_oracle as O
from tests import _mol_ref64 as R

LOGIT_TOL = 1e-4   # tests/test_gpu_parity.py: the fp32-oracle bar on logits
STAGE_TOL = 2e-6   # ... and on Eq / Ex
E2E_FLOOR = 1e-6   # end to end: |hip - f64| <= 2 |oracle32 - f64| + E2E_FLOOR (the floor covers pairs where the oracle happens to be exact)

LDS = 160 * 1024
SCORE_WAVES = 8
SMALL_SHAPES = {(4, 64), (4, 128), (8, 32)}        # mol_kernels.h score_small_shape (P_Q = 8, H = 128, fp32)
TUNED = {(8, 4, 64), (8, 4, 128), (8, 8, 32), (16, 16, 64)}
BATCHED_BYTES = 1300 * 1024                         # mol_query.hip kBatchedPrologueBytes
SPLIT_BYTES = 1000 * 1024
EXTRA_SHAPES = [(8, 4, 32, 128), (8, 8, 16, 128), (8, 8, 64, 128), (8, 8, 128, 128), (8, 8, 48, 128), (8, 4, 16, 128), (16, 2, 64, 128),
                (16, 4, 32, 128), (16, 4, 64, 128), (32, 2, 32, 128), (8, 8, 32, 64), (8, 4, 64, 64)]          # MOL_EXTRA_SHAPES
NOHID_SHAPES = [(8, 8, 32), (8, 4, 64), (16, 4, 32)]                                                           # MOL_NOHID_SHAPES


# ----------------------------------------------------------------------------------------------------------------------------
# routes, from the host code's formulas
# ----------------------------------------------------------------------------------------------------------------------------
def prologue_weight_bytes(cfg):
    D, QH, d, PQ = cfg.query_embedding_dim, max(cfg.query_hidden_dim, 0), cfg.dot_product_dimension, cfg.query_dot_product_groups
    Hq, L, n_uid = (cfg.gating_query_hidden_dim if cfg.gating_query_fn else 0), cfg.num_logits, len(cfg.uid_embedding_hash_sizes)
    return 4 * (D * 2 * QH + (PQ - n_uid) * d * QH + Hq * D + L * Hq)


def prologue_route(cfg, B):
    """query_prologue: batched MFMA kernels (p1 / p2 / p3) past 1300 KB of weights per query and 64 queries, the split kernels
    (glu_slice + group) past 1000 KB for at most 64 queries, else the per-query kernel."""
    QH, d, L = max(cfg.query_hidden_dim, 0), cfg.dot_product_dimension, cfg.num_logits
    Hq = cfg.gating_query_hidden_dim if cfg.gating_query_fn else 0
    batched_ok = QH > 0 and cfg.gating_query_fn and QH % 32 == 0 and Hq % 32 == 0 and d % 32 == 0 and L % 32 == 0 and d <= 256
    wb = prologue_weight_bytes(cfg)
    if batched_ok and wb > BATCHED_BYTES and not (QH > 0 and B <= 64):
        return "batched"
    if QH > 0 and B <= 64 and wb > SPLIT_BYTES:
        return "split"
    return "per_query"


def geo(pq, px, d, h):
    L = pq * px
    wpack = (h * L if h > 0 else L * L) + L * h + h + L
    ex, gi = 32 * px * d, 32 * L
    return wpack, ex, gi


def score_route(shape, B, N, n_cu, cand=False):
    """score_launch: wsplit for 16x16x64; the small units (use_small_units); else choose_variant's direct / staged / staged1.
    cand: per-row or indexed candidates (always the independent-wave shells)."""
    pq, px, d, h = shape
    if (pq, px, d) not in TUNED or h != 128:
        return "direct"
    if (pq, px, d) == (16, 16, 64):
        return "wsplit"
    n_groups, n_tiles = -(-B // (32 // pq)), -(-N // 32)
    if not cand and pq == 8 and (px, d) in SMALL_SHAPES:
        if n_tiles * n_groups <= 2 * n_cu or (B <= 2 and n_tiles >= 8 * n_cu):
            return "small"
    wpack, ex, gi = geo(pq, px, d, h)
    staged_fits = 4 * (wpack + 2 * (ex + gi)) <= LDS
    staged1_fits = 4 * (wpack + ex + 2 * gi) <= LDS
    if not cand and n_groups >= SCORE_WAVES:
        if staged_fits and n_tiles >= 8 * n_cu:
            return "staged"
        if staged1_fits:
            return "staged1"
        if staged_fits:
            return "staged"
    return "direct"


def staged1_split(N, n_cu, B, pq):
    """mol_score_staged1_kernel's leftover round: (full rounds, leftover tiles, workgroups per leftover tile)."""
    n_tiles, n_groups = -(-N // 32), -(-B // (32 // pq))
    rounds, left = divmod(n_tiles, n_cu)
    nsub = min(n_cu // left, SCORE_WAVES, n_groups) if left and 2 * left <= n_cu else 1
    return rounds, left, nsub


# ----------------------------------------------------------------------------------------------------------------------------
# configurations and inputs
# ----------------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def config(shape=(8, 8, 32, 128), D=64, Di=64, QH=512, IH=-1, qnl="geglu", inl="geglu", uid=(), tau=0.05, comb="glu_silu", Hq=128, Hi=128):
    pq, px, d, h = shape
    return O.MoLConfig(D, Di, d, pq, px, temperature=tau, query_hidden_dim=QH, item_hidden_dim=IH, gating_query_hidden_dim=Hq,
                       gating_qi_hidden_dim=h, gating_item_hidden_dim=Hi, query_nonlinearity=qnl, item_nonlinearity=inl,
                       uid_embedding_hash_sizes=tuple(uid), gating_combination_type=comb)


PROJ = ("_query_embeddings_fn._query_emb_proj_module.", "_item_embeddings_fn._item_emb_proj_module.")


def weights(cfg, seed, kind="bias", gain=1.0):
    """Synthetic weights with non-zero biases everywhere ("bias"), or with zero projection biases so that scaled rows reach the eps
    clamp of the l2 norm ("eps"; gate biases stay non-zero).  gain scales the three gate output layers (and the pair gate's output bias)
    until w spans > 100: the softmax exp2 underflows for all but a few terms and glu_silu sees large negative g."""
    g = gen(seed + 7)
    w = O.synthetic_weights(cfg, seed=seed, uid_rows=None)
    for k in list(w):
        if k.endswith("bias") or k.endswith("._b"):
            zero = kind == "eps" and k.startswith(PROJ)
            w[k] = torch.zeros_like(w[k]) if zero else torch.randn(w[k].shape, generator=g) * (0.5 if k.endswith("._b") else 0.1)
    for k in ("_gating_fn._qi_partial_module.3.weight", "_gating_fn._qi_partial_module.3.bias", "_gating_fn._query_only_partial_module.2.weight",
              "_gating_fn._item_only_partial_module.3.weight"):
        if k in w:
            w[k] = w[k] * gain
    if kind == "wide":   # GLU pre-activations of O(1 .. 3), where gelu's tails differ from their approximations
        for k in (PROJ[0] + "1._w", PROJ[1] + "1._w"):
            if k in w:
                w[k] = w[k] * 40
    for i, hs in enumerate(cfg.uid_embedding_hash_sizes):   # zeroed rows and rows straddling the eps clamp
        t = w[f"_query_embeddings_fn._uid_embeddings_{i}.weight"]
        t[1:4] = 0.0
        for r, s in zip(range(4, 8), (0.3e-6, 0.8e-6, 1.5e-6, 4e-6)):
            t[r] = t[r] / t[r].norm() * s
    return w


ROW_SCALES = (0.0, 1e-8, 1e-6, 3e-6, 1e-5, 3e-5)   # 3e-5: the hash table's small entries (sigma 0.02) need it to clear eps


def edge_rows(x, scales):
    """The first rows scaled by `scales`: sub-embedding norms from 0 to beyond eps (with zero projection biases)."""
    x = x.clone()
    for i, s in enumerate(scales[: x.shape[0]]):
        x[i] = x[i] * s
    return x


GLU_ITEM_SCALES = (0.0, 1e-3, 0.1, 0.2, 0.3, 1.0)   # a GLU item projection is quadratic near 0 and already ~1e-5 at scale 1


def item_scales(cfg):
    return ROW_SCALES if cfg.item_hidden_dim <= 0 else GLU_ITEM_SCALES


def query_scales(cfg):
    # a GLU query projection is quadratic in q near 0: the square roots of the linear case's scales put its norms around eps
    return ROW_SCALES if cfg.query_hidden_dim <= 0 else tuple(s ** 0.5 for s in ROW_SCALES)


def items(cfg, N, seed, edge=True):
    X = torch.from_numpy(O.hash_item_table(seed, 0, N, cfg.item_embedding_dim))
    return edge_rows(X, item_scales(cfg)) if edge else X


def queries(cfg, B, seed, edge=True):
    q = O.synthetic_queries(cfg, B, seed=seed)
    return edge_rows(q, query_scales(cfg)) if edge else q


def user_ids(cfg, B):
    if not cfg.uid_embedding_hash_sizes:
        return None
    hs = cfg.uid_embedding_hash_sizes[0]
    u = torch.arange(B, dtype=torch.int64) * 37 + 11
    u[:7] = torch.tensor([0, 1, 2, 3, 4, 5, 6])[: min(B, 7)]        # rows 1..7 of the table: zeroed and near-eps rows
    if B > 8:
        u[8] = -5                                                     # python %: a negative id maps to row hs - 5 + 1
        u[-1] = hs - 1
    return u


def columns(N, seed, k=192):
    """Items the float64 reference is evaluated at: both ends (the edge rows, the partial last tile) and a random sample."""
    if N <= 512:
        return torch.arange(N)
    g = gen(seed)
    return torch.unique(torch.cat([torch.arange(64), torch.arange(N - 64, N), torch.randint(64, N - 64, (k,), generator=g)]))


# ----------------------------------------------------------------------------------------------------------------------------
# comparison helpers
# ----------------------------------------------------------------------------------------------------------------------------
RATIOS = {}   # kernel -> worst |got - ref| / bound seen by this module's GPU cases (printed when the module finishes)


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    for k in sorted(RATIOS):
        print(f"[ratio] {k}: {RATIOS[k]:.3f}")


def assert_within(got, ref, bound, what, kernel):
    got = got.detach().double().cpu()
    d = (got - ref).abs()
    bad = ~(d <= bound)
    assert bool(torch.isfinite(bound).all()), f"{what}: infinite bound"
    ratio = float((d / bound.clamp(min=1e-300)).max()) if d.numel() else 0.0
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    if bool(bad.any()):
        idx = tuple(int(t) for t in bad.nonzero()[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at {idx}: got {float(got[idx])!r}, "
                    f"ref {float(ref[idx])!r}, |d| {float(d[idx]):.3e} > bound {float(bound[idx]):.3e}")


def catches(mutated, ref, bound):
    return bool(((mutated - ref).abs() > bound).any())


def old_bar_verdict(name, mutated, ref, tol):
    err = float((mutated - ref).abs().max())
    print(f"[bug class] {name}: max |mutation - f64| = {err:.3e}; the fp32-oracle bar {tol:g} would {'ACCEPT' if err <= tol else 'reject'} it")


def spec_of(cfg):
    from rails_amd import engine as E

    names = {f.name for f in dataclasses.fields(E.MolShapeSpec)}
    return E.MolShapeSpec(**{k: v for k, v in dataclasses.asdict(cfg).items() if k in names})


# ----------------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------------
# prologue: (name, cfg kwargs, B, weight kind, expected route).  Per-query up to 1000 KB of weights per query (QH = 608: 999 424 B), the
# split kernels beyond it for B <= 64 (QH = 640: 1 048 576 B), the batched ones beyond 1300 KB (QH = 832: 1 343 488 B) for B > 64;
# ML-1M's 1 164 288 B: split at B = 64, per-query at B = 65; ML-20M's 3 MB: split at B = 64, batched at B = 65.
ML1M = dict(shape=(8, 4, 64, 128), D=50, Di=50, qnl="swiglu", uid=(6040,))
ML20M = dict(shape=(8, 4, 128, 128), D=256, Di=256, qnl="swiglu", uid=(16384,))
PROLOGUE_CASES = [
    ("qh608-geglu", dict(QH=608), 13, "eps", "per_query"),
    ("qh640-geglu", dict(QH=640), 13, "eps", "split"),
    ("qh640-swiglu-b64", dict(QH=640, qnl="swiglu"), 64, "bias", "split"),
    ("qh640-swiglu-b65", dict(QH=640, qnl="swiglu"), 65, "eps", "per_query"),
    ("qh800-geglu-b65", dict(QH=800), 65, "bias", "per_query"),
    ("qh832-geglu-b65", dict(QH=832), 65, "eps", "batched"),
    ("qh832-swiglu-b64", dict(QH=832, qnl="swiglu"), 64, "eps", "split"),
    ("qh832-swiglu-b97", dict(QH=832, qnl="swiglu"), 97, "bias", "batched"),
    ("qh0-uid", dict(QH=0, uid=(977,)), 30, "eps", "per_query"),
    ("qh0-uid-b65", dict(QH=0, uid=(977,), shape=(8, 4, 64, 128)), 65, "bias", "per_query"),
    ("ml1m-b64", ML1M, 64, "eps", "split"),
    ("ml1m-b65", ML1M, 65, "eps", "per_query"),
    ("ml20m-b64", ML20M, 64, "eps", "split"),
    ("ml20m-b65", ML20M, 65, "eps", "batched"),
    ("books-b3", dict(), 3, "eps", "per_query"),
    ("qh64-geglu-wide", dict(QH=64, D=32), 5, "wide", "per_query"),
]


def prologue_case(case):
    name, kw, B, kind, route = case
    cfg = config(**kw)
    w = weights(cfg, seed=len(name) + B, kind=kind)
    q = queries(cfg, B, seed=B + 3, edge=kind == "eps")
    return cfg, w, q, user_ids(cfg, B), route


# index: (name, cfg kwargs, N).  N = 1, 31, 0 (mod 32), linear and GLU item projections.
INDEX_CASES = [
    ("linear-n1", dict(), 1), ("linear-n31", dict(), 31), ("linear-n97", dict(), 97), ("linear-n256", dict(), 256),
    ("linear-8x4x128-n223", dict(shape=(8, 4, 128, 128), Di=256), 223),
    ("geglu-n33", dict(IH=96), 33), ("geglu-n63", dict(IH=96, Di=50), 63), ("swiglu-n96", dict(IH=64, inl="swiglu"), 96),
    ("swiglu-16x16x64-n161", dict(shape=(16, 16, 64, 128), IH=128, inl="swiglu"), 161),
]


def index_case(case, kind="eps"):
    name, kw, N = case
    cfg = config(**kw)
    w = weights(cfg, seed=N + 5, kind=kind)
    return cfg, w, items(cfg, N, seed=N, edge=kind == "eps")


# scoring: (name, shape, B, N as a function of n_cu, tau, weight kind / gain, combination, expected route)
SCORE_CASES = [
    # small units, trigger (a): at most 2 n_cu big units; one more tile and the direct shell takes over
    ("small-a-8x4x64", (8, 4, 64, 128), 8, (lambda n: 32 * n - 7), 0.05, ("bias", 1.0), "glu_silu", "small"),
    ("direct-past-a-8x4x64", (8, 4, 64, 128), 8, (lambda n: 32 * n + 1), 0.05, ("bias", 1.0), "glu_silu", "direct"),
    ("small-a-8x8x32-sat", (8, 8, 32, 128), 7, (lambda n: 1001), 0.01, ("bias", 30.0), "glu_silu", "small"),
    ("small-a-8x4x128", (8, 4, 128, 128), 5, (lambda n: 700), 1.0, ("bias", 1.0), "glu_silu", "small"),
    # small units, trigger (b): B <= 2 over >= 8 n_cu tiles; one tile fewer is the direct shell
    ("small-b-8x8x32", (8, 8, 32, 128), 1, (lambda n: 32 * 8 * n - 5), 0.05, ("bias", 1.0), "glu_silu", "small"),
    ("direct-below-b-8x8x32", (8, 8, 32, 128), 2, (lambda n: 32 * (8 * n - 1)), 0.05, ("bias", 1.0), "glu_silu", "direct"),
    ("direct-8x8x32-eps", (8, 8, 32, 128), 9, (lambda n: 32 * n - 3), 0.05, ("eps", 1.0), "glu_silu", "direct"),
    # staged (double-buffered) from 8 n_cu tiles with >= 8 query groups; staged1 below it
    ("staged-8x8x32", (8, 8, 32, 128), 33, (lambda n: 32 * 8 * n - 3), 0.05, ("bias", 1.0), "glu_silu", "staged"),
    ("staged1-8x8x32", (8, 8, 32, 128), 33, (lambda n: 32 * (8 * n - 1)), 0.05, ("bias", 8.0), "glu_silu", "staged1"),
    # staged1 (8x4x128 tiles fit LDS once) at r n_cu - 1, r n_cu, r n_cu + 1 tiles: no leftover split / none left / a split leftover round
    ("staged1-r1m1", (8, 4, 128, 128), 30, (lambda n: 32 * (n - 1) - 9), 0.05, ("bias", 1.0), "glu_silu", "staged1"),
    ("staged1-r1", (8, 4, 128, 128), 32, (lambda n: 32 * n), 0.05, ("bias", 1.0), "glu_silu", "staged1"),
    ("staged1-r1p1", (8, 4, 128, 128), 30, (lambda n: 32 * n + 1), 0.01, ("bias", 1.0), "glu_silu", "staged1"),
    ("staged1-r2p1", (8, 4, 128, 128), 29, (lambda n: 32 * (2 * n + 1) - 31), 1.0, ("bias", 20.0), "glu_silu", "staged1"),
    ("staged1-8x4x64", (8, 4, 64, 128), 64, (lambda n: 2000), 0.05, ("bias", 1.0), "glu_silu", "staged1"),
    # the 16x16x64 team kernel
    ("wsplit", (16, 16, 64, 128), 5, (lambda n: 777), 0.05, ("bias", 4.0), "glu_silu", "wsplit"),
    ("wsplit-sat", (16, 16, 64, 128), 7, (lambda n: 301), 0.01, ("bias", 30.0), "glu_silu", "wsplit"),
    # gating_combination_type "none"
    ("none-small", (8, 8, 32, 128), 9, (lambda n: 500), 0.05, ("bias", 1.0), "none", "small"),
    ("none-direct", (8, 4, 64, 128), 6, (lambda n: 32 * n + 33), 0.05, ("bias", 1.0), "none", "direct"),
    ("none-staged1", (8, 4, 128, 128), 30, (lambda n: 32 * n + 1), 0.05, ("bias", 1.0), "none", "staged1"),
    ("none-wsplit", (16, 16, 64, 128), 3, (lambda n: 100), 0.05, ("bias", 1.0), "none", "wsplit"),
]


@functools.lru_cache(maxsize=None)
def score_setup(shape, B, N, tau, kind, gain, comb, edge=True):
    pq, px, d, h = shape
    cfg = config(shape, D=48 + pq, Di=40 + px, QH=256, uid=(101,) if pq == 8 and px == 4 else (), tau=tau, comb=comb)
    w = weights(cfg, seed=pq * 100 + px * 10 + d + B, kind=kind, gain=gain)
    # queries across the eps clamp only with zero projection biases ("eps"), where the clamp is reachable; the prologue cases cover them
    # elsewhere, and in a batch of a few queries they would leave the gates nothing to do
    return cfg, w, queries(cfg, B, seed=B + d, edge=edge and kind == "eps"), items(cfg, N, seed=N % 9973 + 1, edge=edge), user_ids(cfg, B)


# ============================================================================================================================
# CPU: routes, input coverage and the sensitivity of every bar
# ============================================================================================================================
def test_route_formulas_pick_every_route():
    n = 256
    routes = {c[0]: score_route(c[1], c[2], c[3](n), n) for c in SCORE_CASES}
    assert routes == {c[0]: c[7] for c in SCORE_CASES}
    assert [prologue_route(prologue_case(c)[0], c[2]) for c in PROLOGUE_CASES] == [c[4] for c in PROLOGUE_CASES]
    assert [staged1_split(32 * n + k, n, 30, 8) for k in (-32, 0, 1)] == [(0, n - 1, 1), (1, 0, 1), (1, 1, 8)]
    # the prologue thresholds sit where the comments say
    assert [prologue_weight_bytes(config(QH=qh)) for qh in (608, 640, 800, 832)] == [999_424, 1_048_576, 1_294_336, 1_343_488]
    assert prologue_weight_bytes(config(**ML1M)) == 1_164_288


def test_edge_rows_straddle_the_eps_clamp():
    """The scaled rows put sub-embedding norms below and above eps = 1e-6 (no fp32 overflow / subnormal sums), zero rows included."""
    eps = R.f32(1e-6)
    for case in INDEX_CASES:
        cfg, w, X = index_case(case)
        (ex, _), _ = R.index64(cfg, w, X)
        pre = "_item_embeddings_fn._item_emb_proj_module."
        Xd = X.double()
        if cfg.item_hidden_dim > 0:
            h, _ = R.glu64(Xd, None, w[pre + "1._w"], w[pre + "1._b"], cfg.item_nonlinearity)
            proj, _ = R.linear64(h, None, w[pre + "2.weight"], w[pre + "2.bias"])
        else:
            proj, _ = R.linear64(Xd, None, w[pre + "1.weight"], w[pre + "1.bias"])
        norms = proj.reshape(X.shape[0], cfg.item_dot_product_groups, -1).norm(dim=-1)
        if X.shape[0] >= 6:
            assert bool((norms[1:6] < eps).any()) and bool((norms[1:6] > eps).any()), (case[0], norms[:6].amin(1), norms[:6].amax(1))
            assert float(norms[1:6].min()) > 1e-17, case[0]        # fp32 sums of squares stay normal
            assert bool((norms[0] == 0).all())
    for case in PROLOGUE_CASES:
        cfg, w, q, uid, _ = prologue_case(case)
        if case[3] != "eps":
            continue
        (eq, _), _ = R.prologue64(cfg, w, q, uid)
        raw = eq.norm(dim=-1)
        assert bool((raw[0] == 0).all()) and bool((raw[1:6] < 1 - 1e-3).any()), case[0]   # rows of norm < eps are not normalised to 1


def _score_ref_inputs(cfg, w, q, X, uid, cols):
    (Eq, _), (gq, _) = R.prologue64(cfg, w, q, uid)
    (Ex, _), (gi, _) = R.index64(cfg, w, X[cols])
    return Eq, gq, Ex, gi


def test_l2_norm_bars_catch_a_wrong_clamp():
    """The eps clamp on the squared norm and rsqrt(ss + eps), on the index and prologue inputs of the GPU cases."""
    for case in (INDEX_CASES[3], INDEX_CASES[5]):
        cfg, w, X = index_case(case)
        (ref, bound), _ = R.index64(cfg, w, X)
        for mut in ("clamp_sq", "rsqrt_eps"):
            (m, _), _ = R.index64(cfg, w, X, mut=mut)
            assert catches(m, ref, bound), (case[0], mut)
            old_bar_verdict(f"Ex {mut} ({case[0]})", m, ref, STAGE_TOL)
    for case in (PROLOGUE_CASES[0], PROLOGUE_CASES[8]):
        cfg, w, q, uid, _ = prologue_case(case)
        (ref, bound), _ = R.prologue64(cfg, w, q, uid)
        for mut in ("clamp_sq", "rsqrt_eps"):
            (m, _), _ = R.prologue64(cfg, w, q, uid, mut=mut)
            assert catches(m, ref, bound), (case[0], mut)
            old_bar_verdict(f"Eq {mut} ({case[0]})", m, ref, STAGE_TOL)


def test_glu_bars_catch_a_tanh_gelu():
    cfg, w, X = index_case(INDEX_CASES[5], kind="bias")
    (ref, bound), _ = R.index64(cfg, w, X)
    (m, _), _ = R.index64(cfg, w, X, mut="tanh_gelu")
    assert catches(m, ref, bound)
    old_bar_verdict("Ex tanh GELU", m, ref, STAGE_TOL)
    cfg, w, q, uid, _ = prologue_case(PROLOGUE_CASES[-1])
    (ref, bound), _ = R.prologue64(cfg, w, q, uid)
    (m, _), _ = R.prologue64(cfg, w, q, uid, mut="tanh_gelu")
    assert catches(m, ref, bound)
    old_bar_verdict("Eq tanh GELU", m, ref, STAGE_TOL)
    g = gen(3)
    x, W, b = torch.randn(33, 50, generator=g), torch.randn(50, 74, generator=g) * 0.3, torch.randn(74, generator=g)
    ref, bound = R.glu64(x.double(), None, W, b, "geglu")
    assert catches(R.glu64(x.double(), None, W, b, "geglu", mut="tanh_gelu")[0], ref, bound)


def extra_cases():
    """The extra / no-hidden-layer shapes' scoring cases (direct shell): a partial last query group and a partial last tile."""
    out = []
    for shape in EXTRA_SHAPES + [(pq, px, d, 0) for pq, px, d in NOHID_SHAPES]:
        B = 32 // shape[0] + 3
        out.append((f"extra-{'x'.join(map(str, shape))}", shape, B, (lambda n: 333), 0.05, ("bias", 4.0), "glu_silu", "direct"))
        if shape[3] == 0:
            out.append((f"nohid-eps-{'x'.join(map(str, shape[:3]))}", shape, B, (lambda n: 333), 0.01, ("eps", 1.0), "glu_silu", "direct"))
    return out


EXTRA_CASES = extra_cases()
CAND_SHAPES = [(8, 8, 32, 128), (8, 4, 64, 128), (8, 4, 128, 128), (8, 8, 64, 128), (8, 4, 32, 128)]
CAND_B, CAND_N, CAND_K = 11, 1000, 45


def candidate_positions():
    pos = torch.randint(0, CAND_N, (CAND_B, CAND_K), generator=gen(5))
    pos[:, 0] = 0                       # the zero row
    pos[:, 1] = CAND_N - 1              # the last item of the corpus's partial tile
    return pos


def bug_classes(cfg, Eq, Ex, gq, gi, B, n, qt):
    """The mutated logits of every bug class that applies to this geometry: a dropped pair-gate output bias, silu(gq gi) + gqi (glu_silu),
    the last item of a partial tile scored with the padding row's gi (zeros), the last query of a partial group with a padding row's gq."""
    muts = {"no_b2": R.score64(cfg, _W[0], Eq, Ex, gq, gi, mut="no_b2")[0]}
    if cfg.gating_combination_type == "glu_silu":
        muts["silu_gqgi"] = R.score64(cfg, _W[0], Eq, Ex, gq, gi, mut="silu_gqgi")[0]
    if n % 32:
        gi_pad = gi.clone()
        gi_pad[..., -1, :] = 0.0
        muts["pad_gi"] = R.score64(cfg, _W[0], Eq, Ex, gq, gi_pad)[0]
    if B % qt:
        gq_pad = gq.clone()
        gq_pad[-1] = 0.0
        muts["pad_gq"] = R.score64(cfg, _W[0], Eq, Ex, gq_pad, gi)[0]
    return muts


_W = [None]


def _assert_bugs_outside(name, cfg, w, Eq, Ex, gq, gi, B, n, qt):
    _W[0] = w
    ref, bound = R.score64(cfg, w, Eq, Ex, gq, gi)
    print(f"[bar] {name}: per-pair bound median {float(bound.median()):.2e}, max {float(bound.max()):.2e}")
    muts = bug_classes(cfg, Eq, Ex, gq, gi, B, n, qt)
    missed = []
    for mname, m in muts.items():
        old_bar_verdict(f"logits {mname} ({name})", m, ref, LOGIT_TOL)
        if not catches(m, ref, bound):
            missed.append(mname)
    assert not missed, (name, missed)


@pytest.mark.parametrize("case", SCORE_CASES + EXTRA_CASES, ids=lambda c: c[0])
def test_scoring_bars_catch_gate_and_padding_bugs(case):
    """Every bug class that applies to the case's geometry lands outside its bar, on every dense scoring case."""
    name, shape, B, nf, tau, (kind, gain), comb, _ = case
    N = nf(256)
    cfg, w, q, X, uid = score_setup(shape, B, N, tau, kind, gain, comb)
    cols = columns(N, seed=N)
    assert int(cols[-1]) == N - 1                      # the last item (of the partial tile, if any) is among the checked ones
    Eq, gq, Ex, gi = _score_ref_inputs(cfg, w, q, X, uid, cols)
    _assert_bugs_outside(name, cfg, w, Eq, Ex, gq, gi, B, N, 32 // shape[0])


@pytest.mark.parametrize("shape", CAND_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_candidate_bars_catch_gate_and_padding_bugs(shape):
    """The same on the per-row candidates of the candidate shells: 45 candidates per row (a partial last tile), 11 queries."""
    cfg, w, q, X, uid = score_setup(shape, CAND_B, CAND_N, 0.05, "bias", 4.0, "glu_silu")
    (Eq, _), (gq, _) = R.prologue64(cfg, w, q, uid)
    (Ex, _), (gi, _) = R.index64(cfg, w, X)
    pos = candidate_positions()
    _assert_bugs_outside(f"candidates-{shape}", cfg, w, Eq, Ex[pos], gq, gi[pos], CAND_B, CAND_K, 32 // shape[0])


def test_saturated_gates_reach_the_softmax_tails():
    """gain 30: w spans > 100 for some pairs (exp2 underflows for all but a few terms), and g reaches large negative values."""
    case = next(c for c in SCORE_CASES if c[0] == "small-a-8x8x32-sat")
    name, shape, B, nf, tau, (kind, gain), comb, _ = case
    cfg, w, q, X, uid = score_setup(shape, B, nf(256), tau, kind, gain, comb)
    cols = columns(nf(256), seed=1)
    Eq, gq, Ex, gi = _score_ref_inputs(cfg, w, q, X, uid, cols)
    cl = torch.einsum("bpd,nmd->bnpm", Eq, Ex).reshape(B, len(cols), -1) / R.f32(tau)
    p = "_gating_fn._qi_partial_module."
    hid = torch.nn.functional.silu(cl @ w[p + "1.weight"].double().T + w[p + "1.bias"].double())
    g = gq.unsqueeze(1) * gi.unsqueeze(0) + hid @ w[p + "3.weight"].double().T + w[p + "3.bias"].double()
    wv = g * torch.sigmoid(g)
    assert float((wv.amax(-1) - wv.amin(-1)).max()) > 100 and float(g.min()) < -50


# ============================================================================================================================
# GPU
# ============================================================================================================================
@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def n_cu():
    from rails_amd import _lib

    n = int(_lib.load().rails_device_compute_units())
    assert n > 0
    return n


def engine(cfg, w, dev):
    from rails_amd import engine as E

    return E.MolEngine(spec_of(cfg), {k: v.to(dev) for k, v in w.items()}, precision="fp32")


def _dev(t, dev):
    return None if t is None else t.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PROLOGUE_CASES, ids=lambda c: f"{c[0]}-{c[4]}")
def test_query_prologue_matches_float64(dev, case):
    cfg, w, q, uid, route = prologue_case(case)
    assert prologue_route(cfg, q.shape[0]) == route
    eng = engine(cfg, w, dev)
    _, eq, gq = eng.query_pack(q.to(dev), _dev(uid, dev), want_plain=True)
    (ref_eq, b_eq), (ref_gq, b_gq) = R.prologue64(cfg, w, q, uid)
    kernel = {"per_query": "query_prologue_kernel", "split": "query_glu_slice_kernel+query_group_kernel", "batched": "query_p1/p2/p3_kernel"}[route]
    assert_within(eq, ref_eq, b_eq, f"Eq {case[0]} ({route})", kernel)
    assert_within(gq, ref_gq, b_gq, f"gq {case[0]} ({route})", kernel)
    if case[3] == "eps":
        assert bool((eq.cpu()[0] == 0).all()), "a zero query row gives zero components"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["eps", "bias"])
@pytest.mark.parametrize("case", INDEX_CASES, ids=lambda c: c[0])
def test_index_build_matches_float64_and_its_copies_are_exact(dev, case, kind):
    cfg, w, X = index_case(case, kind)
    eng = engine(cfg, w, dev)
    index = eng.build_index(X.to(dev))
    ex, gi = eng.unpack_index(index)
    (ref_ex, b_ex), (ref_gi, b_gi) = R.index64(cfg, w, X)
    assert_within(ex, ref_ex, b_ex, f"Ex {case[0]} {kind}", "index_build_kernel")
    assert_within(gi, ref_gi, b_gi, f"gi {case[0]} {kind}", "index_build_kernel")
    N = X.shape[0]
    # padding rows of the last tile are zeros
    tile_f = index.buf.numel() // -(-N // 32)
    buf = index.buf.cpu().view(-1, tile_f // 4, 4)
    lanes = torch.arange(tile_f // 4) % 32
    last = buf[-1][lanes >= (N - 32 * (buf.shape[0] - 1))]
    assert bool((last == 0).all()), "padding items of the last tile must be zeros"
    # the row-major copy: item i's slot s, half h at rows[i * RP + 2 s + h] (mol_index.hip index_rows_kernel)
    rows = eng.build_index_rows(index).cpu().view(N, -1, 4)
    rp = rows.shape[1]
    i = torch.arange(N).view(N, 1)
    j = torch.arange(rp).view(1, rp)
    src = (i // 32) * (tile_f // 4) + (j // 2) * 64 + (j % 2) * 32 + (i % 32)
    assert torch.equal(rows, buf.view(-1, 4)[src]), "row-major copy"
    # gathered candidate tiles: an exact copy of the chosen items, zeros for padding / out-of-range positions
    g = gen(N)
    pos = torch.randint(0, N, (3, 37), generator=g)
    pos[1, 5] = N            # out of range: treated as padding
    cidx, kp = eng.gather_index(index, pos.to(dev))
    cex, cgi = eng.unpack_index(cidx)
    cex, cgi = cex.cpu().view(3, kp, *ex.shape[1:]), cgi.cpu().view(3, kp, -1)
    ok = pos < N
    assert torch.equal(cex[:, :37][ok], ex.cpu()[pos[ok]]) and torch.equal(cgi[:, :37][ok], gi.cpu()[pos[ok]])
    assert bool((cex[:, :37][~ok] == 0).all()) and bool((cex[:, 37:] == 0).all()) and bool((cgi[:, 37:] == 0).all())


def _score_case(dev, n_cu, case):
    name, shape, B, nf, tau, (kind, gain), comb, route = case
    N = nf(n_cu)
    assert score_route(shape, B, N, n_cu) == route, (name, n_cu)
    cfg, w, q, X, uid = score_setup(shape, B, N, tau, kind, gain, comb)
    eng = engine(cfg, w, dev)
    pack, eq, gq = eng.query_pack(q.to(dev), _dev(uid, dev), want_plain=True)
    index = eng.build_index(X.to(dev))
    ex, gi = eng.unpack_index(index)
    out = eng.score_dense(pack, B, index)
    cols = columns(N, seed=N)
    ref, bound = R.score64(cfg, w, eq, ex[cols.to(dev)], gq, gi[cols.to(dev)])
    kernel = {"small": "mol_score_small_kernel", "direct": "mol_score_direct_kernel", "staged": "mol_score_staged_kernel",
              "staged1": "mol_score_staged1_kernel", "wsplit": "mol_score_wsplit_kernel"}[route]
    assert_within(out[:, cols.to(dev)], ref, bound, f"logits {name} ({route}, N={N}, B={B})", kernel)
    return cfg, w, eng, pack, eq, gq, index, ex, gi


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCORE_CASES, ids=lambda c: f"{c[0]}-{c[7]}")
def test_fp32_scoring_matches_float64(dev, n_cu, case):
    _score_case(dev, n_cu, case)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CAND_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_candidate_scoring_shells_match_float64(dev, n_cu, shape):
    """Per-row candidates: the indexed-candidate direct shell (score_indexed), the row-major one (mol_score_rows_kernel) and the
    gathered per-row tiles (score_candidates), every candidate held to the per-pair bound."""
    B, N, n_cand = CAND_B, CAND_N, CAND_K
    assert score_route(shape, B, N, n_cu, cand=True) == "direct"
    cfg, w, q, X, uid = score_setup(shape, B, N, 0.05, "bias", 4.0, "glu_silu")
    eng = engine(cfg, w, dev)
    pack, eq, gq = eng.query_pack(q.to(dev), _dev(uid, dev), want_plain=True)
    index = eng.build_index(X.to(dev))
    ex, gi = eng.unpack_index(index)
    pos = candidate_positions()
    ref, bound = R.score64(cfg, w, eq, ex.cpu()[pos], gq, gi.cpu()[pos])
    dpos = pos.to(dev)
    assert eng.score_indexed_supported(B, n_cand), "every exact-fp32 direct-shell shape scores indexed candidates"
    assert_within(eng.score_indexed(pack, B, index, dpos), ref, bound, f"score_indexed {shape}", "mol_score_direct_kernel(indexed)")
    if (shape[0], shape[1], shape[2]) in TUNED:
        rows = eng.build_index_rows(index)
        assert_within(eng.score_indexed_rows(pack, B, rows, N, dpos), ref, bound, f"score_indexed_rows {shape}", "mol_score_rows_kernel")
    cidx, kp = eng.gather_index(index, dpos)
    got = eng.score_candidates(pack, B, cidx, kp)
    assert_within(got[:, :n_cand], ref, bound, f"score_candidates {shape}", "mol_score_direct_kernel(per_row)")


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXTRA_CASES, ids=lambda c: c[0])
def test_extra_and_nohid_shapes_match_float64(dev, n_cu, case):
    """Every MOL_EXTRA_SHAPES / MOL_NOHID_SHAPES build (the direct shell), a partial last query group and a partial last tile."""
    _score_case(dev, n_cu, case)


@pytest.mark.gpu
@pytest.mark.parametrize("L,X,per_row", [(32, 1, False), (64, 7, False), (256, 5, True), (1000, 3, False)])
@pytest.mark.parametrize("glu_silu", [True, False])
@pytest.mark.parametrize("renorm,eps", [(False, 1e-6), (True, 1e-6), (True, 2.0)])   # eps = 2 > sum pi: the clamp binds and halves every pi
def test_gate_combine_matches_float64(dev, L, X, per_row, glu_silu, renorm, eps):
    from rails_amd import engine as E

    g = gen(L + X)
    B = 6
    rows = B * X
    y = torch.randn(rows, L, generator=g) * 10
    gqi = torch.randn(rows, L, generator=g) * 3
    gq = torch.randn(B, L, generator=g) * 4
    gi = torch.randn(rows if per_row else X, L, generator=g) * 4
    gqi[0] *= 40                          # a saturated row: w spans hundreds, g very negative
    parts = (gqi, gq, gi) if glu_silu else (gqi, None if L == 64 else gq, gi)
    out, pi = E.gate_combine(y.to(dev), *(_dev(t, dev) for t in parts), X, per_row, glu_silu, renorm, eps, want_probs=True)
    ref, bound = R.gate_combine64(y, parts[0], parts[1], parts[2], X, per_row, glu_silu, renorm, eps)
    assert_within(out, ref, bound, f"gate_combine L={L} X={X} per_row={per_row} glu_silu={glu_silu} renorm={renorm} eps={eps}", "gate_combine_kernel")
    total = 1.0 / max(1.0, eps) if renorm else 1.0
    assert float(pi.sum(-1).double().cpu().sub(total).abs().max()) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("rows,K,F", [(1, 50, 37), (33, 64, 64), (100, 17, 129), (257, 256, 96)])
@pytest.mark.parametrize("kind", ["geglu", "swiglu"])
def test_glu_f32_matches_float64(dev, rows, K, F, kind):
    from rails_amd import _lib
    from rails_amd.engine import _ptr, _stream

    g = gen(rows + K + F)
    x = torch.randn(rows, K, generator=g)
    W = torch.randn(K, 2 * F, generator=g) * K ** -0.5
    b = torch.randn(2 * F, generator=g)
    dx, dW, db = x.to(dev), W.to(dev), b.to(dev)
    scratch = torch.empty(rows * 2 * F, device=dev)
    out = torch.full((rows, F), float("nan"), device=dev)
    kcode = _lib.RAILS_GEGLU if kind == "geglu" else _lib.RAILS_SWIGLU
    _lib.check(_lib.load().rails_glu_f32(_ptr(dx), K, _ptr(dW), _ptr(db), rows, K, F, kcode, _ptr(scratch), _ptr(out), _stream()), "rails_glu_f32")
    ref, bound = R.glu_f32_64(x, W, b, kind)
    assert_within(out, ref, bound, f"glu_f32 rows={rows} K={K} F={F} {kind}", "glu_gate_kernel")


E2E = ["ml-1m", "ml-20m", "amzn-books", "synthetic-16x16x64"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", E2E)
def test_end_to_end_against_float64(dev, name):
    """MoLSimilarity.forward and MoLBruteForceTopK.all_logits at the four BASELINE shapes, held to twice the fp32 oracle's own distance
    from the float64 restatement plus E2E_FLOOR."""
    import rails_amd

    cfg = O.CONFIGS[name]
    w = weights(cfg, seed=11, kind="bias", gain=3.0)
    B, N = 9, 1500
    q = queries(cfg, B, seed=4, edge=False)
    X = items(cfg, N, seed=6, edge=False)
    uid = user_ids(cfg, B)
    kw = {"user_ids": uid} if uid is not None else {}
    (Eq, _), (gq, _) = R.prologue64(cfg, w, q, uid)
    (Ex, _), (gi, _) = R.index64(cfg, w, X)
    ref64, _ = R.score64(cfg, w, Eq, Ex, gq, gi)
    ref32 = O.mol_logits(cfg, w, q, X.unsqueeze(0), uid)
    bar = 2 * float((ref32.double() - ref64).abs().max()) + E2E_FLOOR
    mol, _ = rails_amd.create_mol_interaction_module(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
        cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
        cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
        query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None)
    mol.load_state_dict(w, strict=True)
    mol = mol.to(dev).eval()
    kwd = {k: v.to(dev) for k, v in kw.items()}
    ids = torch.arange(N, dtype=torch.int64).unsqueeze(0) + 1
    with torch.inference_mode():
        fwd, _ = mol(q.to(dev), X.unsqueeze(0).to(dev), **kwd)
        tk = rails_amd.MoLBruteForceTopK(mol, X.unsqueeze(0).to(dev), ids.to(dev))
        al = tk.all_logits(q.to(dev), **kwd)
    for what, got in (("forward", fwd), ("all_logits", al)):
        err = float((got.double().cpu() - ref64).abs().max())
        RATIOS[f"end-to-end {what}"] = max(RATIOS.get(f"end-to-end {what}", 0.0), err / bar)
        assert err <= bar, (name, what, err, bar)
