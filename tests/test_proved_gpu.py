"""The PROVED exact top-k on the GPU: the arithmetic model behind the a-priori bound of rails_amd/f16x3_bound.py measured on the part
(hypotheses H1-H3), |first pass - fp32| against the bound on stressed models, and the module -- first pass on the split-f16 kernels,
fp32 re-scoring, device verdict with the a-priori eps -- against the dense fp32 path, bit for bit, on every BASELINE shape.
Reference call site replaced: rails/indexing/mol_top_k.py:99-130 (MoLBruteForceTopK.forward)."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import rails_amd
from oracle import f16x3_bound as OB
from oracle import mol_oracle as O
from rails_amd import engine as E
from rails_amd import f16x3_bound as FB
from tests._fixtures import Fixture, full_size_inputs
from tests.test_gpu_parity import build_module

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---- H2: one v_mfma_f32_32x32x16_f16 ---------------------------------------------------------------------------------------------
def _f16_families(g):
    """(name, a (n, 32, 16) f16, b (n, 16, 32) f16, c (n, 32, 32) fp32): operand sets that stress the accumulation inside the instruction"""
    n = 64
    rnd = lambda *s: torch.randn(*s, generator=g)
    fam = []
    a, b = rnd(n, 32, 16), rnd(n, 16, 32)
    fam.append(("gaussian, C ~ 1", a, b, rnd(n, 32, 32)))
    fam.append(("gaussian, C ~ 100", a, b, 100 * rnd(n, 32, 32)))
    fam.append(("gaussian, C ~ 1e-3", a, b, 1e-3 * rnd(n, 32, 32)))
    fam.append(("same sign, C = 0", a.abs(), b.abs(), torch.zeros(n, 32, 32)))
    for spread in (4, 8, 11, 13):
        ea = torch.randint(-spread, 1, (n, 32, 16), generator=g).float()
        eb = torch.randint(-spread, 1, (n, 16, 32), generator=g).float()
        fam.append((f"mixed exponents 2^-{2 * spread} .. 1", (1 + torch.rand(n, 32, 16, generator=g)) * 2 ** ea,
                    (1 + torch.rand(n, 16, 32, generator=g)) * 2 ** eb * torch.sign(rnd(n, 16, 32)), 2.0 ** -spread * rnd(n, 32, 32)))
    fam.append(("large C, small products", 2.0 ** -5 * a, 2.0 ** -5 * b, 1024 * (1 + torch.rand(n, 32, 32, generator=g))))
    fam.append(("lo x hi block: |a| ~ 2^-10", 2.0 ** -10 * a, b, 20 * rnd(n, 32, 32)))
    sub = torch.randint(1, 1024, (n, 32, 16), generator=g).float() * 2.0 ** -24        # f16 subnormals
    fam.append(("f16 subnormal operands", sub, 16 * b, torch.zeros(n, 32, 32)))
    half = rnd(n, 32, 8)
    fam.append(("cancelling pairs", torch.cat([half, -half], 2), torch.cat([b[:, :8], b[:, :8]], 1), rnd(n, 32, 32)))
    # built for the datapath: per lane half one product ~ 1 and seven just under 2^-24 of it (cut inside the half) ...
    big = torch.zeros(n, 32, 16); bb = torch.zeros(n, 16, 32)
    big[:] = (2 - 2.0 ** -10) * 2.0 ** -13; bb[:] = (2 - 2.0 ** -10) * 2.0 ** -13          # product = 0.998 x 2^-24
    big[:, :, 0] = 1.0; bb[:, 0, :] = 1.0 + torch.rand(n, 32, generator=g).round(decimals=2)
    big[:, :, 8] = 1.0; bb[:, 8, :] = 1.0 + torch.rand(n, 32, generator=g).round(decimals=2)
    fam.append(("two big products + 14 just under 2^-24 of them", big, bb, torch.zeros(n, 32, 32)))
    # ... and a large C with sixteen products just under 2^-26 of it (cut against the largest addend)
    sm = torch.full((n, 32, 16), (2 - 2.0 ** -10) * 2.0 ** -14); sb = torch.full((n, 16, 32), (2 - 2.0 ** -10) * 2.0 ** -14)   # 0.998 x 2^-26
    fam.append(("C ~ 1 + 16 products just under 2^-26", sm, sb, 1.0 + torch.rand(n, 32, 32, generator=g)))
    fam.append(("C ~ 1 + 16 products just under 2^-24", 2 * sm, sb * 2, 1.0 + torch.rand(n, 32, 32, generator=g)))
    return [(name, x.half(), y.half(), z.float()) for name, x, y, z in fam]


def test_f16_mfma_accumulation_model(dev):
    """H2: D = C + sum_16 a_i b_i + e with |e| <= KC u (|C| + sum |p|) + KP u sum |p| (rails_amd/f16x3_bound.py).  Every operand family --
    random ones, and ones built for the measured datapath (addends cut below 2^-26 of the largest, products below 2^-24 of their
    half's largest) -- must stay below 0.8 of that bound; f16 subnormal operands must be kept."""
    g = torch.Generator().manual_seed(0)
    worst = 0.0
    for name, a, b, c in _f16_families(g):
        d = E.mfma_probe_f16(a.to(dev), b.to(dev), c.to(dev)).cpu().double()
        a64, b64, c64 = a.double(), b.double(), c.double()
        exact = c64 + a64 @ b64                                  # products of f16 are exact in float64, the sum is good to 2^-53
        psum = a64.abs() @ b64.abs()
        bound = U * (FB.KC * (c64.abs() + psum) + FB.KP * psum)
        ratio = float(((d - exact).abs() / bound.clamp_min(1e-300)).max())
        single = float(((d - exact).abs() / (U * (c64.abs() + psum)).clamp_min(1e-300)).max())
        print(f"f16 MFMA  {name:48s} max |e| / bound = {ratio:.3f}   max |e| / (u (|C| + sum |p|)) = {single:.3f}")
        worst = max(worst, ratio)
        if "subnormal" in name:    # flushed operands would lose whole products: an error of the order of the magnitudes themselves
            assert float(d.abs().max()) > 0 and float(((d - exact).abs() / (c64.abs() + psum).clamp_min(1e-300)).max()) < 2.0 ** -20, "f16 subnormal operands are flushed"
    print("f16 MFMA worst |e| / bound", worst, "KC", FB.KC, "KP", FB.KP)
    assert worst <= 0.8


def test_fp32_mfma_is_a_chain_of_fmas(dev):
    """H1 for one instruction: v_mfma_f32_32x32x2_f32 returns C + a0 b0 + a1 b1 within the error of two round-to-nearest fmas, in either order."""
    g = torch.Generator().manual_seed(1)
    n = 64
    worst = 0.0
    for scale_c in (1.0, 1e3, 1e-3, 0.0):
        a, b, c = torch.randn(n, 32, 2, generator=g), torch.randn(n, 2, 32, generator=g), scale_c * torch.randn(n, 32, 32, generator=g)
        d = E.mfma_probe_f32(a.to(dev), b.to(dev), c.to(dev)).cpu().double()
        a64, b64, c64 = a.double(), b.double(), c.double()
        p0, p1 = a64[:, :, 0:1] * b64[:, 0:1, :], a64[:, :, 1:2] * b64[:, 1:2, :]
        exact = c64 + p0 + p1
        # a term is rounded by its own fma and by every later one: the first product twice, the second once, C twice
        bound = 2 * U * (c64.abs() + torch.maximum(p0.abs(), p1.abs())) + U * torch.minimum(p0.abs(), p1.abs())
        r = float(((d - exact).abs() / bound.clamp_min(1e-300)).max())
        worst = max(worst, r)
        # which order?  (informational: the bound charges the larger product the larger factor)
        f01 = ((c64 + p0).float().double() + p1).float().double()
        f10 = ((c64 + p1).float().double() + p0).float().double()
        print(f"fp32 MFMA  C ~ {scale_c:g}: max |e| / bound = {r:.3f};  bits equal to k = 0 then 1: {float((d == f01).double().mean()):.4f}, 1 then 0: {float((d == f10).double().mean()):.4f}")
    assert worst <= 1.0 + 1e-6


def test_scalar_transcendentals_are_one_ulp(dev):
    """H3: v_exp_f32 and v_rcp_f32 within 1 ulp (relative 2 u), and phi(t) = t / (1 + 2^t) as the kernels compute it within gamma(7) |phi|."""
    g = torch.Generator().manual_seed(2)
    x = torch.cat([torch.randn(1 << 16, generator=g) * s for s in (0.1, 1.0, 8.0, 40.0)] + [torch.linspace(-126, 126, 1 << 14)]).clamp(-140.0, 126.0)
    out = E.scalar_probe(x.to(dev)).cpu().double()
    x64 = x.double()
    normal = torch.exp2(x64) >= 2.0 ** -125                       # below the normal range v_exp_f32 returns 0 (H4: an absolute 2^-126, carried as OMEGA)
    assert float((out[0][~normal] - torch.exp2(x64[~normal])).abs().max()) <= 2.0 ** -125
    e_exp = float(((out[0][normal] - torch.exp2(x64[normal])).abs() / torch.exp2(x64[normal])).max())
    nz = x64.abs() > 1e-30
    e_rcp = float(((out[1][nz] - 1 / x64[nz]).abs() * x64[nz].abs()).max())
    phi = x64 / (1 + torch.exp2(x64))
    sel = phi.abs() > 1e-30
    e_phi = float(((out[2][sel] - phi[sel]).abs() / phi[sel].abs()).max())
    print(f"v_exp_f32 max rel err = {e_exp / U:.3f} u   v_rcp_f32 = {e_rcp / U:.3f} u   phi = {e_phi / U:.3f} u  (model: 2, 2, 7)")
    assert e_exp <= 2 * U * 1.001 and e_rcp <= 2 * U * 1.001 and e_phi <= FB.gamma(7)


def test_device_self_check_passes_here_and_gates_the_proved_mode(dev):
    """rails_amd/arith_check.py: the compact re-measurement of H1-H3 that runs once per device before the proved mode binds passes on this
    part with room to spare, is reported by stats(), and a device that failed it gets the dense kernels."""
    from rails_amd import arith_check as AC

    rep = AC.report(dev)
    print("arithmetic self-check:", rep)
    assert rep["ok"] and rep["h1_fp32_mfma_fma_chain"] <= 1.0 + 1e-6 and rep["h2_f16_mfma_kc_kp"] <= 0.8 and rep["h3_exp_rcp_phi"] <= 0.8 and rep["h2_f16_subnormals_kept"]
    cfg = O.CONFIGS["amzn-books"]
    N = 70_000
    X = torch.from_numpy(O.hash_item_table(3, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(N, dtype=torch.int64, device=dev).unsqueeze(0)
    with torch.inference_mode():
        m = build_module(cfg, O.synthetic_weights(cfg, seed=0), dev, None)
        tk = rails_amd.MoLBruteForceTopK(m, X, ids)
        assert tk._bind().exact is not None and tk.stats()["arithmetic_model_on_device"]["ok"] is True
        key = str(torch.device(dev))
        saved = AC._cache[key]
        try:
            AC._cache[key] = {"ok": False, "forced": "by the test"}
            assert rails_amd.MoLBruteForceTopK(m, X, ids)._bind().exact is None
        finally:
            AC._cache[key] = saved


# ---- |first pass - fp32| against the bound, on the kernels -----------------------------------------------------------------------
STRESS = ["gaussian", "outlier", "hot gate", "near overflow", "tiny components"]


def _stressed(cfg, kind: str, seed: int):
    """weights, items: the families of the CPU property test (oracle/f16x3_bound.py stress_case) at kernel scale"""
    w = O.synthetic_weights(cfg, seed=seed, uid_rows=64 if cfg.uid_embedding_hash_sizes else None)
    w, scale_items = OB.stress_weights(w, kind, seed)
    return w, scale_items


@pytest.mark.parametrize("kind", STRESS)
@pytest.mark.parametrize("workload", ["amzn-books", "ml-1m", "ml-20m", "synthetic-16x16x64"])
def test_first_pass_error_stays_below_the_a_priori_bound(dev, workload, kind):
    """max |f16x3 logit - fp32 logit| over B x N pairs <= eps (and the oracle's restatement of the bound equals the product's)."""
    cfg = O.CONFIGS[workload]
    if cfg.uid_embedding_hash_sizes:
        cfg = dataclasses.replace(cfg, uid_embedding_hash_sizes=(63,))
    w, item_scale = _stressed(cfg, kind, seed=5)
    N, B = 40_000, 16
    X = torch.from_numpy(O.hash_item_table(21, 0, N, cfg.item_embedding_dim)) * item_scale
    q = O.synthetic_queries(cfg, B, seed=41)
    kw = {"user_ids": torch.arange(B, dtype=torch.int64, device=dev)} if cfg.uid_embedding_hash_sizes else {}
    p = "_gating_fn._qi_partial_module."
    args = (w[p + "1.weight"], w[p + "1.bias"], w[p + "3.weight"], w[p + "3.bias"], cfg.temperature, cfg.dot_product_dimension,
            cfg.query_dot_product_groups, cfg.item_dot_product_groups)
    bound = FB.first_pass_bound(*args)
    restated = OB.first_pass_bound(*(np.asarray(t) if torch.is_tensor(t) else t for t in args))
    assert bound["eps"] == pytest.approx(restated["eps"], rel=1e-9) or (math.isinf(bound["eps"]) and math.isinf(restated["eps"]))
    with torch.inference_mode():
        try:
            m16 = build_module(cfg, w, dev, "f16x3")
            s16 = rails_amd.MoLBruteForceTopK(m16, X.unsqueeze(0).to(dev), torch.arange(N, device=dev).unsqueeze(0)).all_logits(q.to(dev), **kw)
        except NotImplementedError:
            assert math.isinf(bound["eps"]) or not bound["in_f16_range"] or kind == "near overflow"
            return
        m32 = build_module(cfg, w, dev, "fp32")
        tk32 = rails_amd.MoLBruteForceTopK(m32, X.unsqueeze(0).to(dev), torch.arange(N, device=dev).unsqueeze(0))
        tk32.exact_mode = "dense"
        s32 = tk32.all_logits(q.to(dev), **kw)
    err = float((s16 - s32).abs().max())
    print(f"{workload:20s} {kind:16s} max |s16 - s32| = {err:.3e}   eps = {bound['eps']:.4f}   ratio = {err / bound['eps']:.2e}  gate |t2| <= {bound.get('t2_max', 0):.0f}")
    assert torch.isfinite(s16).all() and torch.isfinite(s32).all()
    assert err <= bound["eps"]


@pytest.mark.parametrize("kind", STRESS)
@pytest.mark.parametrize("workload", ["synthetic-16x16x64", "amzn-books", "ml-20m", "ml-1m"])
def test_upper_first_pass_bounds_every_fp32_logit(dev, workload, kind):
    """rails_mol_score_dense_upper (the team kernel of 16x16x64 and the register-resident f16x3 units of the other BASELINE shapes):
    logit + (ub2 c + ub1) c + ub0 with the product's coefficients is >= the fp32 kernels' logit for EVERY pair; the added term is the
    polynomial of the pair's own largest |cross logit| (checked against the oracle's stage functions on a sample); and it is far below the
    one a-priori eps where the pairs of a corpus sit."""
    cfg = O.CONFIGS[workload]
    if cfg.uid_embedding_hash_sizes:
        cfg = dataclasses.replace(cfg, uid_embedding_hash_sizes=(63,))
    w, item_scale = _stressed(cfg, kind, seed=7)
    N, B = 30_011, 9
    X = torch.from_numpy(O.hash_item_table(23, 0, N, cfg.item_embedding_dim)) * item_scale
    q = O.synthetic_queries(cfg, B, seed=45)
    uid = torch.arange(B, dtype=torch.int64) if cfg.uid_embedding_hash_sizes else None
    kw = {"user_ids": uid.to(dev)} if uid is not None else {}
    p = "_gating_fn._qi_partial_module."
    args = (w[p + "1.weight"], w[p + "1.bias"], w[p + "3.weight"], w[p + "3.bias"], cfg.temperature, cfg.dot_product_dimension,
            cfg.query_dot_product_groups, cfg.item_dot_product_groups)
    res = FB.upper_bound_poly(*args)
    if res["poly"] is None:
        assert math.isinf(FB.first_pass_bound(*args)["eps"])
        return
    ub2, ub1, ub0 = res["poly"]
    ids = torch.arange(N, device=dev).unsqueeze(0)
    with torch.inference_mode():
        try:
            tk16 = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, "f16x3"), X.unsqueeze(0).to(dev), ids)
            eng = tk16._bind()
        except NotImplementedError:
            assert kind == "near overflow"
            return
        assert eng.score_dense_upper_supported()
        qpack, _, _ = eng.query_pack(q.to(dev), kw.get("user_ids"))
        s16 = eng.score_dense(qpack, B, tk16._index)
        up = eng.score_dense_upper(qpack, B, tk16._index, res["poly"])
        tk32 = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, "fp32"), X.unsqueeze(0).to(dev), ids, exact_mode="dense")
        s32 = tk32.all_logits(q.to(dev), **kw)
    assert torch.isfinite(up).all() and torch.isfinite(s32).all()
    assert bool((up >= s32).all()), float((s32 - up).max())
    add = (up - s16).double().cpu()
    assert float(add.min()) >= ub0 * (1 - 1e-6) - 2e-6
    # the added term == P(max |cl|) of the pair: cross logits of a sample from the oracle's stage functions (fp32 torch, ~1e-5 off the kernel's)
    cols = torch.randint(0, N, (64,), generator=torch.Generator().manual_seed(3))
    eq = O.query_component_embeddings(cfg, w, q, uid)
    exm = O.item_component_embeddings(cfg, w, X[cols])
    c = (torch.einsum("bpd,nmd->bnpm", eq, exm) / cfg.temperature).abs().amax((2, 3)).double()
    want = (ub2 * c + ub1) * c + ub0
    assert float((add[:, cols] - want).abs().max()) <= 1e-3 * float(want.max()) + 1e-5
    eps_top = FB.first_pass_bound(*args)["eps"]
    print(f"{workload:20s} {kind:16s} added bound: median {float(add.median()):.4f}  max {float(add.max()):.4f}   one a-priori eps {eps_top:.3f};  min (upper - fp32) = {float((up - s32).min()):.4f}")
    assert float(add.max()) <= eps_top * 1.06 + 1e-4
    if kind == "gaussian":
        assert float(add.median()) <= 0.3 * eps_top


def test_per_pair_bound_keeps_heavier_gate_weights_provable(dev):
    """amzn-books shape with the pair-gate weights scaled x 1.8: one a-priori eps is ~3 logit units (beyond PROVED_MAX_EPS: with it the module
    would bind the dense kernels) -- the default binds the per-pair form instead (the f16x3 units' UPPER build), proves its calls and returns
    the dense fp32 kernels' bits."""
    cfg = O.CONFIGS["amzn-books"]
    N, B, k = 200_000, 16, 200
    X = torch.from_numpy(O.hash_item_table(33, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = (torch.arange(N, dtype=torch.int64, device=dev) * 5 + 1).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=47).to(dev)
    p = "_gating_fn._qi_partial_module."
    w = O.synthetic_weights(cfg, seed=11)
    w[p + "1.weight"] = w[p + "1.weight"] * 1.8
    w[p + "3.weight"] = w[p + "3.weight"] * 1.8
    with torch.inference_mode():
        m = build_module(cfg, w, dev, None)
        tk = rails_amd.MoLBruteForceTopK(m, X, ids)
        eng = tk._bind()
        assert eng.exact is not None and tk._upper_poly() is not None
        r_s, r_i = _dense(m, X, ids)(q, k=k)
        for _ in range(4):
            s, i = tk(q, k=k)
            assert torch.equal(s, r_s) and torch.equal(i, r_i)
        st = tk.stats()
        print("amzn-books x 1.8 gate weights:", {key: st.get(key) for key in ("calls", "proved_calls", "fallbacks", "bound_violations", "kc", "eps_rigorous", "bound_kind")}, "pad", tk._pad_scale)
        assert PROVED_MAX < st["eps_rigorous"] <= rails_amd.MoLBruteForceTopK.PROVED_MAX_EPS_PER_PAIR and st["bound_kind"] == "per-pair upper bound"
        assert st["bound_violations"] == 0 and st["proved_calls"] + st["fallbacks"] == st["calls"] == 4 and st["proved_calls"] >= 2
        inv = ids[0, torch.randint(0, N, (B, 61), device=dev)]
        ci = rails_amd.CandidateIndex(ids, X)
        a = ci.get_top_k_outputs(q, k=120, aux_payloads={}, top_k_module=tk, invalid_ids=inv, truncate_k_prime_to=200)
        b = ci.get_top_k_outputs(q, k=120, aux_payloads={}, top_k_module=_dense(m, X, ids), invalid_ids=inv, truncate_k_prime_to=200)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


PROVED_MAX = 2.0


# ---- the module -------------------------------------------------------------------------------------------------------------------
def _dense(m32, X, ids):
    tk = rails_amd.MoLBruteForceTopK(m32, X, ids)
    tk.exact_mode = "dense"
    return tk


@pytest.mark.parametrize("workload,N,B,k", [("amzn-books", 695762, 32, 200), ("amzn-books", 695762, 32, 2561), ("amzn-books", 100_003, 5, 120),
                                            ("ml-20m", 27278, 32, 200), ("ml-1m", 3883, 32, 200), ("synthetic-16x16x64", 400_000, 32, 200)])
def test_proved_mode_is_the_default_and_equals_dense_fp32(dev, workload, N, B, k):
    """A module of the DEFAULT precision: MoLBruteForceTopK runs the proved mode (split-f16 first pass, a-priori eps) and returns the
    dense fp32 kernels' output bit for bit -- scores, ids, tie order -- with every call proved and no fallback; via forward and via
    CandidateIndex.get_top_k_outputs with the seen-id filter.  C1 / C2 are below SPECULATE_MIN_ITEMS by default (they run dense there):
    here the threshold is lifted so that the proved route itself is exercised at their full N."""
    cfg = O.CONFIGS[workload]
    w = O.synthetic_weights(cfg, seed=0)
    X = torch.from_numpy(O.hash_item_table(1, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = (torch.arange(N, dtype=torch.int64, device=dev) * 3 + 7).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=2).to(dev)
    kw = {"user_ids": torch.arange(1, B + 1, dtype=torch.int64, device=dev)} if cfg.uid_embedding_hash_sizes else {}
    k = min(k, N)
    with torch.inference_mode():
        m = build_module(cfg, w, dev, None)
        r_s, r_i = _dense(m, X, ids)(q, k=k, **kw)
        old = rails_amd.MoLBruteForceTopK.SPECULATE_MIN_ITEMS, rails_amd.MoLBruteForceTopK.PROVED_MIN_PAIRS
        try:
            rails_amd.MoLBruteForceTopK.SPECULATE_MIN_ITEMS = 0
            rails_amd.MoLBruteForceTopK.PROVED_MIN_PAIRS = 0
            tk = rails_amd.MoLBruteForceTopK(m, X, ids)
            assert tk.exact_mode == "proved"
            assert tk._bind().exact is not None, "the proved mode is not the default exact path"
            # 16x16x64: one a-priori eps (3.0 logit units) is beyond PROVED_MAX_EPS -> the first pass writes per-pair upper bounds instead
            per_pair = cfg.num_logits > 64 or N <= rails_amd.MoLBruteForceTopK.PER_PAIR_MAX_ITEMS      # ... and small corpora take them whatever their eps
            assert (tk._upper_poly() is not None) == per_pair
            assert tk._policy.kind == ("upper" if per_pair else "eps")      # (27 278 items: "upper", with the library's own shape query)
            for _ in range(3):
                s, i = tk(q, k=k, **kw)
                assert torch.equal(s, r_s) and torch.equal(i, r_i)
            st = tk.stats()
            print(workload, N, B, k, {key: st.get(key) for key in ("calls", "fallbacks", "proved_calls", "bound_violations", "eps", "eps_rigorous", "guard_max", "kc")}, "kc pad", tk._pad_scale)
            assert st["eps_rigorous_usable"] is True and st["bound_violations"] == 0
            assert (st.get("bound_kind") == "per-pair upper bound") == per_pair
            if workload == "ml-20m":      # one eps cannot prove it (its candidates run to the cap); the per-pair form does, with 512 candidates
                assert st["calls"] == 3 and st["proved_calls"] == 3 and st["fallbacks"] == 0 and st["kc"] == 512
            if N > 65536 and cfg.num_logits <= 64:
                # large corpora of the 8x8x32 shape: a few hundred items lie within eps of the k-th score -> every call is proved
                assert st["calls"] == 3 and st["proved_calls"] == 3 and st["fallbacks"] == 0
                if per_pair:
                    assert st["eps"] == 0.0
                elif k >= rails_amd.MoLBruteForceTopK.PER_PAIR_MIN_K:      # a call for that many results takes per-pair bounds (its verdict runs with eps = 0,
                    assert st["eps"] < 1e-3 and st["kc"] < 2 * k + 64      # raised only by what the two-sided calls before it observed) and ~2 k candidates
                else:
                    assert st["eps"] == pytest.approx(st["eps_rigorous"], rel=1e-4)
            else:
                # ML-1M / ML-20M (most of the corpus lies within eps of the k-th score) and a 400 k-item sub-range of the 256-logit shape (the
                # k-th score sits where scores are dense: ~10 k items can reach it; the full 12.5 M-item shard, where 730-900 can, is
                # tests/test_full_shard_gpu.py): what cannot be proved is redone densely, says so, and the margin grows or the module stops speculating
                assert st["proved_calls"] + st["fallbacks"] + st.get("paused_calls", 0) + st.get("unprovable_calls", 0) + (3 - st["calls"]) >= 3 and st["proved_calls"] <= st["calls"]
            inv = ids[0, torch.randint(0, N, (B, 61), device=dev)]
            kk = min(k, 120)
            ci = rails_amd.CandidateIndex(ids, X)
            a = ci.get_top_k_outputs(q, k=kk, aux_payloads=kw, top_k_module=tk, invalid_ids=inv, truncate_k_prime_to=200)
            b = ci.get_top_k_outputs(q, k=kk, aux_payloads=kw, top_k_module=_dense(m, X, ids), invalid_ids=inv, truncate_k_prime_to=200)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            # the module's own logits stay the fp32 kernels' (the split-f16 engine is internal)
            assert torch.equal(tk.all_logits(q[:2], **{key: v[:2] for key, v in kw.items()}), _dense(m, X, ids).all_logits(q[:2], **{key: v[:2] for key, v in kw.items()}))
        finally:
            rails_amd.MoLBruteForceTopK.SPECULATE_MIN_ITEMS, rails_amd.MoLBruteForceTopK.PROVED_MIN_PAIRS = old


@pytest.mark.parametrize("B", [1, 2, 3])
def test_small_batches_take_the_dense_kernels_with_the_fused_filter(dev, B):
    """Calls with fewer than PROVED_MIN_PAIRS (query, item) pairs of a default-mode module run the dense fp32 kernels -- through forward and
    through get_top_k_outputs, where the seen-id filter stays inside the selection launch -- and return what the dense module returns."""
    cfg = O.CONFIGS["amzn-books"]
    N, k = 90_001, 120
    X = torch.from_numpy(O.hash_item_table(5, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = (torch.arange(N, dtype=torch.int64, device=dev) * 2 + 3).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=12).to(dev)
    with torch.inference_mode():
        m = build_module(cfg, O.synthetic_weights(cfg, seed=0), dev, None)
        tk = rails_amd.MoLBruteForceTopK(m, X, ids)
        assert tk._bind().exact is not None
        dense = _dense(m, X, ids)
        s, i = tk(q, k=k)
        r_s, r_i = dense(q, k=k)
        assert torch.equal(s, r_s) and torch.equal(i, r_i)
        inv = ids[0, torch.randint(0, N, (B, 61), device=dev)]
        inv[:, :7] = r_i[:, :7]                       # some of the best items are "seen"
        ci = rails_amd.CandidateIndex(ids, X)
        fused = tk.forward_filtered(q, 200, inv, k)
        dense_route = not rails_amd.MoLBruteForceTopK.speculation_pays(B, N)
        assert dense_route == (B < 3)
        assert fused is not None      # dense route: inside the dense selection launch; otherwise inside the proved flow's finish launch (round 6)
        a = ci.get_top_k_outputs(q, k=k, aux_payloads={}, top_k_module=tk, invalid_ids=inv, truncate_k_prime_to=200)
        b = ci.get_top_k_outputs(q, k=k, aux_payloads={}, top_k_module=dense, invalid_ids=inv, truncate_k_prime_to=200)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(fused[0], b[0]) and torch.equal(fused[1], b[1])
        st = tk.stats()
        assert (st["calls"] == 0) == dense_route     # below the pair count nothing is speculated; from it on the proved flow runs
        assert st["fallbacks"] == 0 or not dense_route


def test_proved_mode_unprovable_calls_fall_back(dev):
    """What cannot be proved is redone on the dense fp32 kernels, and says so:
      (a) stressed gate weights (x 6): the a-priori bound is several logit units, the candidates cannot cover everything within it
          -> verdicts fail, the device-side fallback returns the dense result, the margin grows;
      (b) a violated guard: query-gate rows beyond gate_guard / max |gi| -> REDO, never proved;
      (c) an observed |first pass - fp32| above the bound (planted on a candidate through the test hook) is a violation of the
          arithmetic model: counted, the call is not proved, the result is still the dense one (the hook's victim is re-scored);
      (d) a module outside the bound's guards (gating_combination "none") does not speculate at all."""
    cfg = O.CONFIGS["amzn-books"]
    N, B, k = 200_000, 8, 100      # (above PER_PAIR_MAX_ITEMS: the one-eps form of the bound, whose verdict arithmetic the cases below are written for)
    assert N > rails_amd.MoLBruteForceTopK.PER_PAIR_MAX_ITEMS
    X = torch.from_numpy(O.hash_item_table(31, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=43).to(dev)
    p = "_gating_fn._qi_partial_module."
    with torch.inference_mode():
        # (a)
        w = O.synthetic_weights(cfg, seed=9)
        w[p + "1.weight"] = w[p + "1.weight"] * 6.0
        w[p + "3.weight"] = w[p + "3.weight"] * 6.0
        m = build_module(cfg, w, dev, None)
        r_s, r_i = _dense(m, X, ids)(q, k=k)
        assert rails_amd.MoLBruteForceTopK(m, X, ids)._bind().exact is None      # eps ~ 33 > PROVED_MAX_EPS: the default does not speculate ...
        old_max = rails_amd.MoLBruteForceTopK.PROVED_MAX_EPS
        rails_amd.MoLBruteForceTopK.PROVED_MAX_EPS = math.inf                    # ... unless told to: every verdict then fails and is redone
        try:
            tk = rails_amd.MoLBruteForceTopK(m, X, ids)
        finally:
            rails_amd.MoLBruteForceTopK.PROVED_MAX_EPS = old_max
        assert tk._bind().exact is not None and tk.stats()["eps_rigorous"] > 5.0
        for _ in range(3):
            s, i = tk(q, k=k)
            assert torch.equal(s, r_s) and torch.equal(i, r_i)
        st = tk.stats()
        print("stressed gate:", {key: st[key] for key in ("calls", "fallbacks", "proved_calls", "eps_rigorous")}, "pad", tk._pad_scale)
        assert st["fallbacks"] >= 1 and st["proved_calls"] == st["calls"] - st["fallbacks"] and tk._pad_scale > 1
        # (b)
        w = O.synthetic_weights(cfg, seed=9)
        m = build_module(cfg, w, dev, None)
        r_s, r_i = _dense(m, X, ids)(q, k=k)
        tk = rails_amd.MoLBruteForceTopK(m, X, ids)
        s, i = tk(q, k=k)
        assert torch.equal(s, r_s) and torch.equal(i, r_i) and tk.stats()["proved_calls"] == 1
        tk._gate_guard_limit = 0.5 * tk.stats()["guard_max"]
        s, i = tk(q, k=k)
        st = tk.stats()
        assert torch.equal(s, r_s) and torch.equal(i, r_i) and st["proved_calls"] == 1 and st["fallbacks"] == 1, st
        # (c)
        tk = rails_amd.MoLBruteForceTopK(m, X, ids)
        victim = (r_i[:, 3] - 1)                         # every row's fourth-best item (ids are positions + 1)
        tk._debug_first_pass_bias = (victim, 1.25)      # they stay candidates (rank 4 of 924, 1.25 logits of margin used up); their first-pass logits are 1.25 off
        s, i = tk(q, k=k)
        s, i = tk(q, k=k)
        st = tk.stats()
        print("planted:", {key: st[key] for key in ("calls", "fallbacks", "proved_calls", "bound_violations", "eps")})
        assert torch.equal(s, r_s) and torch.equal(i, r_i) and st["bound_violations"] >= 1 and st["proved_calls"] == 0
        # (d)
        cfg_n = dataclasses.replace(cfg, gating_combination_type="none")
        wn = O.synthetic_weights(cfg_n, seed=9)
        mol, _ = rails_amd.create_mol_interaction_module(
            cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups, cfg.item_dot_product_groups,
            cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim, cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim,
            cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False, query_nonlinearity=cfg.query_nonlinearity, gating_combination_type="none")
        mol.load_state_dict(wn, strict=True)
        mol = mol.to(dev).eval()
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
        assert tk._bind().exact is None        # dense fp32: nothing to prove
        ref = O.brute_force_topk(cfg_n, wn, q.cpu(), X.cpu(), ids.cpu(), k)
        s, i = tk(q, k=k)
        assert float((s.cpu() - ref[0]).abs().max()) <= 1e-4


def _bit_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal with NaN == NaN (the same bits)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("kind", ["nan_row", "inf_row", "huge_row", "all_tied", "crowded_top"])
def test_proved_route_on_non_finite_and_tied_corpora(dev, kind):
    """The default exact path on corpora the a-priori bound says nothing about (round-5 review, weak 4): item rows with NaN / inf / absurd
    magnitudes, a corpus of identical items, and a top of the ranking more crowded than the candidate lists.  What cannot be proved there
    must come back as the dense fp32 kernels' result, bit for bit (NaN logits included), through forward and through get_top_k_outputs:
      nan_row / inf_row   the item gate of such a row is non-finite -> max |gi| is, the bound's guard limit is zero -> the module never speculates;
      huge_row            a finite row of 1e30: max |gi| is huge, every call violates the gate guard on the device and is redone densely;
      all_tied            every score of a row equals every other: the threshold selection finds no bin that fits -> REDO -> position order;
      crowded_top         3 000 copies of each query's best item: more ties at the top than candidate slots -> REDO."""
    cfg = O.CONFIGS["amzn-books"]
    N, B, k = 120_000, 6, 100
    X = torch.from_numpy(O.hash_item_table(71, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = (torch.arange(N, dtype=torch.int64, device=dev) * 2 + 9).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=19).to(dev)
    with torch.inference_mode():
        m = build_module(cfg, O.synthetic_weights(cfg, seed=0), dev, None)
        if kind == "nan_row":
            X[0, 777] = float("nan")
        elif kind == "inf_row":
            X[0, 4242] = float("inf")
            X[0, 4243, ::2] = float("-inf")
        elif kind == "huge_row":
            X[0, 31_337] = 1.0e30
        elif kind == "all_tied":
            X[0, :] = X[0, 5].clone()
        elif kind == "crowded_top":
            best = _dense(m, X, ids)(q, k=1)[1][:, 0]                # ids = 2 * position + 9
            for b in range(B):
                X[0, 1000 + 3000 * b : 4000 + 3000 * b] = X[0, (int(best[b]) - 9) // 2].clone()
        dense = _dense(m, X, ids)
        r_s, r_i = dense(q, k=k)
        tk = rails_amd.MoLBruteForceTopK(m, X, ids)
        assert tk.exact_mode == "proved"
        for _ in range(3):
            s, i = tk(q, k=k)
            assert _bit_equal(s, r_s) and torch.equal(i, r_i), kind
        st = tk.stats()
        print(kind, {key: st.get(key) for key in ("calls", "proved_calls", "fallbacks", "unprovable_calls", "paused_calls", "bound_violations", "guard_max")})
        assert st["bound_violations"] == 0
        if kind in ("nan_row", "inf_row"):
            assert st["proved_calls"] == 0 and (tk._bind().exact is None or st.get("unprovable_calls", 0) == 3)
        else:
            assert st["proved_calls"] == 0 and st["fallbacks"] + st.get("unprovable_calls", 0) + st.get("paused_calls", 0) >= 1
        inv = ids[0, torch.randint(0, N, (B, 40), device=dev)]
        inv[:, :5] = r_i[:, :5]
        ci = rails_amd.CandidateIndex(ids, X)
        a = ci.get_top_k_outputs(q, k=60, aux_payloads={}, top_k_module=tk, invalid_ids=inv, truncate_k_prime_to=100)
        b = ci.get_top_k_outputs(q, k=60, aux_payloads={}, top_k_module=dense, invalid_ids=inv, truncate_k_prime_to=100)
        assert torch.equal(a[0], b[0]) and _bit_equal(a[1], b[1])
