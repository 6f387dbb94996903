"""GPU: score_of / explain_of.

score_of is held to torch.equal against all_logits gathered -- every exact mode, precision and route the fixtures cover, every restriction,
an edit chain --; explain_of to the reference's own stages (F1/cl, F1/pi of tests/golden/c1 .. c4) and to tests/_explain_ref.explain64 on the
engine's own operands, per element, inside the a-priori bounds of that module and nothing wider.  Corpora: the N = 1 024 fixture tables
(ids 3 i + 1, so that 0, 2 and negative ids are absent) unless stated.

Maximum observed |error| / bound (printed by every stage test; one run on an MI355X; also in DESIGN section 3.22):
  against the reference's stages, component_logits / weights     c1 0.071 / 3.8e-4, c2 0.044 / 1.8e-4, c3 0.21 / 9.2e-4, c4 0.099 / 1.4e-4
  against explain64, component_logits / weights / logits         12x3x20 H = 50   0.109 / 2.1e-3 / 5.6e-4
    (the largest over T = 1, 33, 129)                            1x1x64           0.016 / 0 / 0.015      (pi = 1 exactly)
                                                                 32x8x16          0.18 / 2.6e-4 / 1.1e-4
                                                                 16x8x32 H = 256  0.092 / 3.2e-4 / 7.3e-5
                                                                 none 4x4x24      0.080 / 1.2e-3 / 3.8e-4
  |sum_l weights * component_logits - logits| on fused modules   at most 4.4e-4 of e_out + the fused route's bound
"""
import pytest
import torch

import rails_amd
from rails_amd import engine as E
from tests import _explain_ref as X64
from tests import _mol_ref64 as R
from tests._fixtures import PER_CONFIG, Fixture
from tests._generic_fixtures import generic_cases
from tests.test_generic_route_gpu import build_module

pytestmark = pytest.mark.gpu
NEG_INF = float("-inf")
TS = (1, 31, 32, 33, 128, 129, 517)      # across the 32-item wave tile and the 128-item block of the generic kernel, and the fused kernels' padded tiles
MAKERS = {
    "brute": lambda mol, x, i, **kw: rails_amd.MoLBruteForceTopK(mol, x, i, **kw),
    "avg": lambda mol, x, i: rails_amd.MoLAvgTopK(mol, x, i, avg_top_k=500),
    "naive": lambda mol, x, i: rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=5),
    "comb": lambda mol, x, i: rails_amd.MoLCombTopK(mol, x, i, avg_top_k=200, k_per_group=5),
}
# (module, fixture, route of the MoL module, constructor kwargs[, precision of the MoL module])
ROUTES = {
    "brute-f16x3": ("brute", "c3_books", None, {"exact_mode": "dense"}, "f16x3"),      # through _score_positions' gather route
    "avg-f16x3": ("avg", "c3_books", None, {}, "f16x3"),
    "brute-default": ("brute", "c3_books", None, {}),
    "brute-dense": ("brute", "c3_books", None, {"exact_mode": "dense"}),
    "brute-uid": ("brute", "c1_ml1m", None, {}),
    "brute-ml20m": ("brute", "c2_ml20m", None, {}),
    "brute-16x16x64": ("brute", "c4_16x16x64", None, {}),
    "brute-generic": ("brute", "c1_ml1m", "generic", {}),
    "avg": ("avg", "c3_books", None, {}),
    "naive": ("naive", "c3_books", None, {}),
    "comb": ("comb", "c3_books", None, {}),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def ids_of(n, dev, first=0):
    return torch.arange(first, first + n, dtype=torch.int64, device=dev) * 3 + 1


def rows_of(t, b):
    """b rows of a fixture tensor of 5 or 6 rows (repeated from the top where it has fewer)"""
    return t[torch.arange(b) % t.shape[0]]


def setup(case, dev, b=6, precision=None):
    """-> (tk, fx, q (b, D), kw)"""
    module, name, route, ckw = ROUTES[case][:4]
    precision = precision or (ROUTES[case][4] if len(ROUTES[case]) > 4 else None)
    fx = Fixture(name)
    mol = build_module(fx.cfg, fx.weights, dev, route=route, precision=precision)
    Xt = fx.t("X").to(dev).clone()
    tk = MAKERS[module](mol, Xt, ids_of(Xt.shape[1], dev).unsqueeze(0), **ckw)
    q = rows_of(fx.t("q"), b).to(dev)
    kw = {"user_ids": rows_of(fx.user_ids, b).to(dev)} if fx.user_ids is not None else {}
    return tk, fx, q, kw


def expected(tk, q, pos, kw, invalid=None):
    """all_logits(q, **kw) gathered at pos (on the device), -inf for an absent position and for an item whose id is among the row's invalid ids"""
    full = tk.all_logits(q, **kw)
    n = tk.num_items
    ok = (pos >= 0) & (pos < n)
    at = pos.clamp(0, n - 1)
    want = full.gather(1, at)
    want[~ok] = NEG_INF
    if invalid is not None:
        seen = (tk._ids_flat[at].unsqueeze(-1) == invalid.to(pos.device).unsqueeze(1)).any(-1)
        want[seen] = NEG_INF
    return want


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == torch.float32, (what, got.shape, want.shape)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (what, int((got.view(torch.int32) != want.view(torch.int32)).sum()))


def positions_for(b, t, n, g, absent_row=True):
    """random positions with a repeat inside every row, absent entries (-1, n) and, with absent_row, a last row of absent entries only"""
    pos = torch.randint(0, n, (b, t), generator=g)
    if t >= 3:
        pos[:, t // 2] = pos[:, 0]
        pos[0, 1], pos[-1, 2] = -1, n
    if absent_row and b > 1:
        pos[-1] = torch.where(torch.arange(t) % 2 == 0, torch.tensor(-1), torch.tensor(n + 5))
    return pos


def ids_at(tk, pos):
    """the ids of positions (CPU), absent positions as ids nobody has (0, 2 and negative ones)"""
    n = tk.num_items
    ids = tk._ids_flat.cpu()[pos.clamp(0, n - 1)]
    return torch.where((pos >= 0) & (pos < n), ids, torch.where(pos < 0, torch.tensor(-5), torch.tensor(2)))


# ---- score_of = all_logits gathered ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(ROUTES))
def test_score_of_equals_all_logits_gathered(case, dev):
    tk, fx, q6, kw6 = setup(case, dev)
    g = torch.Generator().manual_seed(61)
    n = tk.num_items
    with torch.inference_mode():
        for b in (1, 6):
            q, kw = q6[:b], {k: v[:b] for k, v in kw6.items()}
            for j, t in enumerate(TS):
                pos = positions_for(b, t, n, g)
                want = expected(tk, q, pos.to(dev), kw)
                ids = ids_at(tk, pos)
                got = tk.score_of(q, ids if j % 2 else ids.to(dev), **kw)      # (ids on the CPU and on the device)
                assert got.device == q.device
                same_bits(got, want, f"{case}: score_of, B = {b}, T = {t}")
                same_bits(tk.score_of_positions(q, pos if j % 2 == 0 else pos.to(dev), **kw), want, f"{case}: score_of_positions, B = {b}, T = {t}")
                assert bool(torch.isinf(want[(pos < 0) | (pos >= n)]).all())
                if b > 1:
                    assert bool((want[-1] == NEG_INF).all()) and bool(torch.isfinite(want[0, :1]).all())
    assert tk.stats()["score_of_calls"] == 4 * len(TS) and tk.stats()["explain_calls"] == 0


def test_split_f16_precisions(dev):
    """'f16x3' scores given positions with the dense pass's bits (the cases above); explain_of is refused there, and both calls where the dense
    pass runs the one-product kernels."""
    pos = torch.zeros((6, 2), dtype=torch.int64, device=dev)
    tk, fx, q, kw = setup("brute-f16x3", dev)
    with pytest.raises(NotImplementedError, match=r"^MoLBruteForceTopK\.explain_of_positions: precision='f16x3'"):      # (the call made is named)
        tk.explain_of_positions(q, pos, **kw)
    tk, fx, q, kw = setup("brute-dense", dev, precision="f16x1")
    for call in ("score_of", "explain_of"):
        with pytest.raises(NotImplementedError, match=rf"^MoLBruteForceTopK\.{call}_positions: precision='f16x1'"):
            getattr(tk, call + "_positions")(q, pos, **kw)


# ---- restrictions ----------------------------------------------------------------------------------------------------------------------------
def restricted_check(tk, q, kw, extra, invalid, g, dev, what):
    """score_of under the call's restriction against the restricted all_logits gathered; the eligible set against rank_of's and log_prob_of's"""
    n, b = tk.num_items, q.shape[0]
    pos = positions_for(b, 70, n, g, absent_row=False).to(dev)
    if invalid is not None:
        pos[:, 5] = tk.positions_of(invalid[:, 0].reshape(-1))      # a seen item among the targets of every row
    want = expected(tk, q, pos, {**kw, **extra}, invalid)
    got = tk.score_of_positions(q, pos, invalid, **kw, **extra)
    same_bits(got, want, what)
    same_bits(tk.score_of(q, ids_at(tk, pos.cpu()), invalid, **kw, **extra), want, what + " (by id)")
    if type(tk)._rank_scores is not None:
        assert torch.equal(tk.rank_of_positions(q, pos, invalid, **kw, **extra) == 0, got == NEG_INF), what
        assert torch.equal(torch.isinf(tk.log_prob_of_positions(q, pos, invalid, **kw, **extra)), torch.isinf(got)), what
    return got


@pytest.mark.parametrize("case", ["brute-default", "brute-generic", "avg"])
def test_restrictions(case, dev):
    tk, fx, q, kw = setup(case, dev)
    g = torch.Generator().manual_seed(62)
    n = tk.num_items
    brute = case.startswith("brute")
    with torch.inference_mode():
        seen = torch.zeros((6, 9), dtype=torch.int64)      # invalid_ids with zero padding: real ids, ids nobody has, zeros behind
        seen[:, :4] = tk._ids_flat.cpu()[torch.randint(0, n, (6, 4), generator=g)]
        seen[:, 4] = 2
        seen = seen.to(dev)
        got = restricted_check(tk, q, kw, {}, seen, g, dev, f"{case}: invalid_ids")
        assert bool((got[:, 5] == NEG_INF).all())
        hidden = torch.randperm(n, generator=g)[: n // 3]
        tk.hide_items(hidden)
        got = restricted_check(tk, q, kw, {}, None, g, dev, f"{case}: hidden")
        assert int((got == NEG_INF).sum()) > 0
        restricted_check(tk, q, kw, {}, seen, g, dev, f"{case}: hidden + invalid_ids")
        tags = torch.randint(0, 16, (n,), generator=g).to(dev)      # (some items carry no tag at all)
        tk.set_item_tags(tags)
        restricted_check(tk, q, kw, {"allowed_tags": 0b0101}, None, g, dev, f"{case}: a shared tag word + hidden")
        restricted_check(tk, q, kw, {"allowed_tags": [1, 2, 4, 8, 3, 12]}, seen, g, dev, f"{case}: a tag word per row + hidden + invalid_ids")
        # one tag word per row across more than 32 rows
        b = 40
        qb = q[torch.arange(b, device=dev) % 6]
        kwb = {k: v[torch.arange(b, device=dev) % 6] for k, v in kw.items()}
        restricted_check(tk, qb, kwb, {"allowed_tags": [1 + (r % 15) for r in range(b)]}, None, g, dev, f"{case}: 40 tag words")
        if brute:
            ragged = torch.rand((6, n), generator=g) < torch.tensor([0.9, 0.5, 0.1, 0.02, 0.3, 0.7]).unsqueeze(1)      # a ragged per-row item_mask=
            mask = E.ItemMask(ragged.to(dev))
            restricted_check(tk, q, kw, {"item_mask": mask}, None, g, dev, f"{case}: ragged item_mask + hidden")
            restricted_check(tk, q, kw, {"item_mask": mask}, seen, g, dev, f"{case}: ragged item_mask + hidden + invalid_ids")
            restricted_check(tk, q, kw, {"item_mask": ragged[0].to(dev)}, seen, g, dev, f"{case}: a shared bool mask + hidden + invalid_ids")
            with pytest.raises(ValueError, match="allowed_tags= and item_mask= in one call"):
                tk.score_of_positions(q, torch.zeros((6, 1), dtype=torch.int64, device=dev), item_mask=mask, allowed_tags=1, **kw)
        else:
            with pytest.raises(NotImplementedError, match="takes no item_mask"):
                tk.score_of_positions(q, torch.zeros((6, 1), dtype=torch.int64, device=dev), item_mask=torch.ones(n, dtype=torch.bool, device=dev), **kw)


@pytest.mark.parametrize("case", ["brute-default", "comb"])
def test_an_edit_chain(case, dev):
    tk, fx, q, kw = setup(case, dev)
    g = torch.Generator().manual_seed(63)
    Xt = fx.t("X")[0].to(dev)
    gone_ids = []

    def check(step):
        n = tk.num_items
        pos = positions_for(6, 70, n, g, absent_row=False)
        ids = ids_at(tk, pos)
        if gone_ids:
            ids[:, 7] = torch.tensor(gone_ids[:1])      # an id that left the corpus is absent
            pos[:, 7] = -1
        want = expected(tk, q, pos.to(dev), kw)
        same_bits(tk.score_of(q, ids, **kw), want, f"{case}: after {step}")

    with torch.inference_mode():
        check("construction")
        at = torch.tensor([0, 31, 32, 1023])
        tk.update_items(at, Xt[torch.tensor([5, 6, 7, 8], device=dev)] * 0.5)
        check("update")
        tk.append_items(Xt[:5] * 0.25, ids_of(5, dev, first=5000))
        check("append")
        rm = torch.tensor([1, 33, tk.num_items - 1])
        gone_ids.extend(tk._ids_flat.cpu()[rm].tolist())
        tk.remove_items(rm)
        check("remove")
        hide = torch.tensor([2, 64, 500])
        tk.hide_items(hide)
        check("hide")
        gone_ids[:0] = tk._ids_flat.cpu()[hide].tolist()
        tk.compact()
        check("compact")


def test_no_dense_pass(dev):
    # 300 007 items: a (32, N) logit matrix would be 38 MB, three orders above every O(B T) buffer of the call, and N is no multiple of a tile
    from oracle import mol_oracle as O
    n, b = 300_007, 32
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=1), dev)
    Xt = torch.from_numpy(O.hash_item_table(7, 0, n, cfg.item_embedding_dim)).to(dev)
    q = O.synthetic_queries(cfg, b, seed=5).to(dev)
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, Xt.unsqueeze(0), ids_of(n, dev).unsqueeze(0))
        pos = torch.randint(0, n, (b, 33), generator=torch.Generator().manual_seed(64)).to(dev)
        tk.score_of(q, tk._ids_flat[pos])      # (binds, builds what the route keeps)
        torch.cuda.synchronize()
        assert not [key for key in tk._scratch if key[0] == "logits"]
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        got = tk.score_of(q, tk._ids_flat[pos])
        explained = tk.explain_of_positions(q, pos)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated(dev) - before
        assert not [key for key in tk._scratch if key[0] == "logits"], "the recycled (B, N) logits buffer exists"
        assert grown < b * n * 4 // 8, grown      # nothing near one (B, N) fp32 matrix was allocated
        same_bits(got, expected(tk, q, pos, {}), "score_of on 300 007 items")
        same_bits(explained.logits, got, "explain_of's logits on 300 007 items")


def test_mips_score_of_is_forwards_score(dev):
    from oracle import mol_oracle as O
    n, b, d = 1024, 6, 50
    g = torch.Generator().manual_seed(65)
    Xt = torch.from_numpy(O.hash_item_table(7, 0, n, d)).to(dev)
    q = (torch.randn(b, d, generator=g) * 0.05).to(dev)
    with torch.inference_mode():
        tk = rails_amd.MIPSBruteForceTopK(Xt.unsqueeze(0), ids_of(n, dev).unsqueeze(0))
        scores, ids = tk(q, k=n)
        by_pos = torch.empty_like(scores).scatter_(1, (ids - 1) // 3, scores.float())      # forward(k = N) re-ordered by id
        for t in (1, 33, 517):
            pos = positions_for(b, t, n, g)
            want = by_pos.gather(1, pos.clamp(0, n - 1).to(dev))
            want[((pos < 0) | (pos >= n)).to(dev)] = NEG_INF
            same_bits(tk.score_of(q, ids_at(tk, pos)), want, f"mips: score_of, T = {t}")
            same_bits(tk.score_of_positions(q, pos.to(dev)), want, f"mips: score_of_positions, T = {t}")
        tk.hide_items(torch.tensor([3, 4]))
        seen = tk._ids_flat[torch.randint(0, n, (b, 3), generator=g).to(dev)]
        pos = positions_for(b, 70, n, g, absent_row=False).to(dev)
        pos[:, 0], pos[:, 1] = 3, tk.positions_of(seen[:, 0])
        mask = E.ItemMask((torch.rand(n, generator=g) < 0.5).to(dev))
        got = tk.score_of_positions(q, pos, seen, item_mask=mask)
        assert torch.equal(tk.rank_of_positions(q, pos, seen, item_mask=mask) == 0, got == NEG_INF) and bool((got[:, :2] == NEG_INF).all())
        kept = got != NEG_INF
        assert torch.equal(got[kept], by_pos.gather(1, pos.clamp(0, n - 1))[kept])      # (positions_for leaves absent entries in the row: clamped for torch's gather)
        with pytest.raises(NotImplementedError, match=r"^MIPSBruteForceTopK\.explain_of: there is no mixture"):
            tk.explain_of(q, ids_at(tk, pos.cpu()))


# ---- explain_of ------------------------------------------------------------------------------------------------------------------------------
def within(got, ref, bound, what):
    err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    worst = float((err / bound).max())
    print(f"{what}: max |err| / bound = {worst:.3g}, max |err| = {float(err.max()):.3g}")
    assert bool((err <= bound).all()), (what, worst)
    return worst


@pytest.mark.parametrize("name", PER_CONFIG)
def test_explain_of_against_the_reference_stages(name, dev):
    """c1 - c4 with the F1 inputs (B = 6, the first 200 items): the kernel's bound plus the reference's own measured distance, per element."""
    case = {"c1_ml1m": "brute-uid", "c2_ml20m": "brute-ml20m", "c3_books": "brute-default", "c4_16x16x64": "brute-16x16x64"}[name]
    tk, fx, q, kw = setup(case, dev, b=Fixture(name).t("q").shape[0])
    n1 = int(fx.z["F1/n"])
    b = q.shape[0]
    pos = torch.arange(n1, device=dev).unsqueeze(0).expand(b, -1).contiguous()
    with torch.inference_mode():
        ex = tk.explain_of_positions(q, pos, **kw)
        same_bits(ex.logits, tk.score_of_positions(q, pos, **kw), f"{name}: explain_of's logits are score_of's")
    PQ, PX, L = fx.cfg.query_dot_product_groups, fx.cfg.item_dot_product_groups, fx.cfg.num_logits
    assert ex.weights.shape == ex.component_logits.shape == (b, n1, PQ, PX) and ex.logits.shape == (b, n1)
    (cl64, ecl), (pi64, epi), _ = X64.explain64(fx.cfg, fx.weights, fx.t("F1/Eq"), fx.t("F1/Ex")[0], fx.t("F1/gq"), fx.t("F1/gi")[0])
    f_cl, f_pi = fx.t("F1/cl").double(), fx.t("F1/pi").double()
    within(ex.component_logits.reshape(b, n1, L), f_cl, ecl + (f_cl - cl64).abs(), f"{name}: component_logits against F1/cl")
    within(ex.weights.reshape(b, n1, L), f_pi, epi + (f_pi - pi64).abs(), f"{name}: weights against F1/pi")


GENERIC = ("g_12x3x20_h50_swiglu", "g_1x1x64", "g_32x8x16", "g_16x8x32_h256", "g_none_4x4x24")


@pytest.mark.parametrize("name", GENERIC)
def test_explain_of_off_the_fused_grid(name, dev):
    """explain64 on the engine's own Eq / Ex / gq / gi; the module is on the generic route, so the explaining launch reads its index in place."""
    _, cfg, w, a = next(c for c in generic_cases() if c[0] == name)
    mol = build_module(cfg, w, dev)
    Xt, q = a["X"].to(dev), a["q"].to(dev)
    n, b = Xt.shape[1], q.shape[0]
    g = torch.Generator().manual_seed(66)
    L = cfg.num_logits
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, Xt, ids_of(n, dev).unsqueeze(0))
        eng = tk._bind()
        assert eng.route == "generic"
        qpack, eq, gq = eng.query_pack(q, None, want_plain=True)
        exi, gi = eng.unpack_index(tk._index)
        (cl64, ecl), (pi64, epi), (out64, eout) = X64.explain64(cfg, w, eq, exi, gq, gi)
        for t in (1, 33, 129):
            pos = positions_for(b, t, n, g)
            ex = tk.explain_of_positions(q, pos.to(dev))
            score = tk.score_of_positions(q, pos.to(dev))
            same_bits(ex.logits, score, f"{name}: explain_of's logits are score_of's, T = {t}")
            ok = (pos >= 0) & (pos < n)
            at = pos.clamp(0, n - 1)
            own, _, _ = eng.explain_indexed(qpack, b, tk._index, at.to(dev))      # what the explaining launch itself writes
            assert torch.equal(own[ok.to(dev)], score[ok.to(dev)]), f"{name}: the explaining instantiation's logit bits, T = {t}"
            rows = torch.arange(b).unsqueeze(1)
            live = ok.unsqueeze(-1).expand(-1, -1, L)
            for what, got, ref, bound in (("component_logits", ex.component_logits, cl64, ecl), ("weights", ex.weights, pi64, epi)):
                got = got.reshape(b, t, L).cpu().double()
                assert bool((got[~live] == 0).all()), f"{name}: {what} of absent pairs"
                r, e = ref[rows, at], bound[rows, at]
                within(torch.where(live, got, r), r, e, f"{name}: {what}, T = {t}")
            r, e = out64[rows, at], eout[rows, at]
            within(torch.where(ok, ex.logits.cpu().double(), r), r, e, f"{name}: logits, T = {t}")
            s = ex.weights.reshape(b, t, L).sum(-1).cpu()
            assert bool(((s - 1).abs()[ok] <= 8 * L * 2.0 ** -24).all()) and bool((s[~ok] == 0).all())
            if L == 1:
                assert bool((ex.weights.reshape(b, t).cpu()[ok] == 1).all())


@pytest.mark.parametrize("case", ["brute-default", "brute-uid", "avg", "brute-generic"])
def test_explain_of_is_consistent_with_score_of(case, dev):
    """logits is score_of's result under the same restriction; on fused modules the mixture of the companion launch reproduces the fused logit to
    the two routes' bounds; weights sum to 1; absent and ineligible pairs hold exact zeros.  T = 1, 33, 129 at B = 1 and 6, a row of absent ids."""
    tk, fx, q6, kw6 = setup(case, dev)
    g = torch.Generator().manual_seed(67)
    n = tk.num_items
    cfg = fx.cfg
    L = cfg.num_logits
    with torch.inference_mode():
        tk.hide_items(torch.randperm(n, generator=g)[:200])
        seen = tk._ids_flat[torch.randint(0, n, (6, 3), generator=g).to(dev)]
        eng, index, _ = tk._pair_scorer()
        _, eq, gq = eng.query_pack(q6, kw6.get("user_ids"), want_plain=True)
        exi, gi = eng.unpack_index(index)
        (_, _), (_, _), (out64, eout) = X64.explain64(cfg, fx.weights, eq, exi, gq, gi)
        _, efused = R.score64(cfg, fx.weights, eq, exi, gq, gi)
        calls = 0
        for b in (1, 6):
            q, kw = q6[:b], {k: v[:b] for k, v in kw6.items()}
            for t in (1, 33, 129):
                pos = positions_for(b, t, n, g)
                ids = ids_at(tk, pos)
                ex = tk.explain_of(q, ids.to(dev), seen[:b], **kw)
                calls += 1
                score = tk.score_of(q, ids, seen[:b], **kw)
                same_bits(ex.logits, score, f"{case}: logits, B = {b}, T = {t}")
                assert ex.weights.shape == ex.component_logits.shape == (b, t, cfg.query_dot_product_groups, cfg.item_dot_product_groups)
                dead = (score == NEG_INF).cpu()
                assert bool(dead[((pos < 0) | (pos >= n))].all()) and (b == 1 or bool(dead[-1].all()))
                wts, cls = ex.weights.reshape(b, t, L).cpu().double(), ex.component_logits.reshape(b, t, L).cpu().double()
                assert bool((wts[dead] == 0).all()) and bool((cls[dead] == 0).all()), f"{case}: exact zeros, B = {b}, T = {t}"
                s = wts.sum(-1)
                assert bool(((s - 1).abs()[~dead] <= 8 * L * 2.0 ** -24).all()), float((s - 1).abs()[~dead].max())
                mix = (wts * cls).sum(-1)
                at = pos.clamp(0, n - 1)
                rows = torch.arange(b).unsqueeze(1)
                bound = eout[rows, at] + efused[rows, at]
                err = (mix - score.cpu().double()).abs()[~dead]
                print(f"{case}: |sum w cl - logits| / bound = {float((err / bound[~dead]).max()):.3g}, B = {b}, T = {t}")
                assert bool((err <= bound[~dead]).all())
                if eng.route == "generic":      # the explaining launch's own logit is score_of's, bit for bit
                    qpack, _, _ = eng.query_pack(q, kw.get("user_ids"))
                    own, _, _ = eng.explain_indexed(qpack, b, index, at.to(dev))
                    assert torch.equal(own[~dead.to(dev)], score[~dead.to(dev)])
    assert tk.stats()["explain_calls"] == calls == 6 and tk.stats()["score_of_calls"] == 6


def test_explain_of_outside_the_generic_envelope_is_refused(dev):
    """A one-Linear pair gate (gating_qi_hidden_dim = -1) has fused fp32 kernels and no generic route: score_of runs, explain_of refuses by name."""
    from tests._fixtures import variant_cases
    case = next((c for c in variant_cases() if c[1].gating_qi_hidden_dim <= 0), None)
    assert case is not None, "tests/golden/variants.npz holds a one-Linear-gate variant"
    name, cfg, w, a = case
    mol = build_module(cfg, w, dev)
    Xt, q = a["X"].to(dev), a["q"].to(dev)
    kw = {"user_ids": a["user_ids"].to(dev)} if "user_ids" in a else {}
    n = Xt.shape[1]
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, Xt, ids_of(n, dev).unsqueeze(0))
        pos = torch.randint(0, n, (q.shape[0], 33), generator=torch.Generator().manual_seed(68)).to(dev)
        same_bits(tk.score_of_positions(q, pos, **kw), expected(tk, q, pos, kw), f"{name}: score_of")
        with pytest.raises(NotImplementedError, match=r"^MoLBruteForceTopK\.explain_of: .*outside its envelope.*hidden layer"):
            tk.explain_of_positions(q, pos, **kw)
