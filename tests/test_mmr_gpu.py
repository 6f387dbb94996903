"""GPU: diversify=lam.  The kernel alone, through engine.topk_mmr, on the seeded inputs of tests/_mmr_ref.py (the inputs the
CPU tests run the mutants on) against that file's numpy walk; then the five modules, each against the same walk over the module's OWN ranked
list -- forward(q, L) taken under _positions_as_ids() with the call's arguments.  Every comparison is on bit patterns: the arithmetic order is
pinned, so there is no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from tests import _mmr_ref as MR
from tests import test_collapse_gpu as CG
from tests import test_index_update_gpu as U
from tests._fixtures import Fixture
from tests.test_generic_route_gpu import build_module

pytestmark = pytest.mark.gpu
N = CG.N
DIM = 24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_inputs(name):
    return MR.build(MR.CASE[name])


@functools.lru_cache(maxsize=None)
def case_expected(name, lam=None):
    case, d = MR.CASE[name], case_inputs(name)
    return MR.walk(d["scores"], d["positions"], d["vectors"], case.lam if lam is None else lam, case.k, case.pool, d["ids"], d["invalid"])


def run_kernel(d, lam, k, pool, dev, rows=slice(None), ids=True):
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    inv = None if d["invalid"] is None else torch.from_numpy(d["invalid"][rows]).to(dev)
    out = E.topk_mmr(torch.from_numpy(d["scores"][rows]).to(dev), torch.from_numpy(d["positions"][rows]).to(dev), torch.from_numpy(d["vectors"]).to(dev),
                     lam, k, pool, torch.from_numpy(d["ids"]).to(dev) if ids else None, inv, word)
    s, p, i, counts = (t.cpu().numpy() for t in out)
    return s.view(np.uint32), p, i, counts, int(word.item())


def assert_same(got, want, what):
    for name, a, b in zip(("scores", "positions", "ids", "counts"), got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name)
    assert got[4] == want[4], (what, "verdict word")


@pytest.mark.parametrize("name", [c.name for c in MR.CASES])
def test_kernel_against_the_reference(name, dev):
    case, d = MR.CASE[name], case_inputs(name)
    got = run_kernel(d, case.lam, case.k, case.pool, dev)
    assert_same(got, case_expected(name), name)
    assert got[0].shape == (case.rows, case.k)


def test_kernel_without_an_id_table(dev):
    """ids == NULL: a position is its own id, for the outputs and for the seen-id test"""
    case, d = MR.CASE["L64-all"], dict(case_inputs("L64-all"))
    d["invalid"] = d["positions"][:, :9].copy()
    want = MR.walk(d["scores"], d["positions"], d["vectors"], case.lam, 1, case.pool, None, d["invalid"])
    got = run_kernel(d, case.lam, 1, case.pool, dev, ids=False)
    assert_same(got, want, "no id table")
    assert np.array_equal(got[1], got[2]) and got[3].tolist() == [55] * 3


def test_short_rows_pad_count_and_leave_the_others_alone(dev):
    case, d = MR.CASE["short-rows"], case_inputs("short-rows")
    s, p, i, counts, word = run_kernel(d, case.lam, case.k, case.pool, dev)
    want = case_expected("short-rows")
    assert_same((s, p, i, counts, word), want, "short rows")
    m = int(counts[1])
    assert word == 1 and m < case.k and counts[0] == counts[2] == case.pool
    neg_inf = np.array([-np.inf], dtype=np.float32).view(np.uint32)[0]
    assert (s[1, m:] == neg_inf).all() and (p[1, m:] == -1).all() and (i[1, m:] == -1).all() and (p[1, :m] >= 0).all()
    for b in (0, 2):      # a row of the batch is what a call of its own returns
        alone = run_kernel(d, case.lam, case.k, case.pool, dev, rows=slice(b, b + 1))
        assert alone[4] == 0 and np.array_equal(alone[0][0], s[b]) and np.array_equal(alone[1][0], p[b]) and np.array_equal(alone[2][0], i[b]), b


@pytest.mark.parametrize("name", ["L2-D1", "L1025-one-hot", "L1025-one-hot-k64", "L5120-seen4096"])
def test_lam_1_is_the_seen_id_filter_of_the_same_list(name, dev):
    """every entry of these lists is eligible by itself and the lists are in key order: the first k unseen entries"""
    case, d = MR.CASE[name], case_inputs(name)
    if name == "L5120-seen4096":      # (the case's sizes with every entry eligible by itself: the seen ids cover the first 3 000 entries)
        d = dict(d)
        rng = np.random.default_rng(5)
        d["scores"] = -np.sort(-rng.standard_normal(d["scores"].shape).astype(np.float32), axis=1)
        d["positions"] = np.stack([rng.permutation(d["n"])[: case.length] for _ in range(case.rows)])
        d["invalid"] = np.concatenate([d["ids"][d["positions"][:, :3000]], np.full((case.rows, 1096), -3)], axis=1)
    got = run_kernel(d, 1.0, case.k, case.pool, dev)
    list_ids = torch.from_numpy(d["ids"][d["positions"]]).to(dev)
    f_ids, f_scores = E.filter_seen_ids(list_ids, torch.from_numpy(d["scores"]).to(dev), torch.from_numpy(d["invalid"]).to(dev), case.k)
    assert got[4] == 0 and np.array_equal(got[2], f_ids.cpu().numpy()) and np.array_equal(got[0], f_scores.cpu().numpy().view(np.uint32)), name
    assert_same(got, MR.walk(d["scores"], d["positions"], d["vectors"], 1.0, case.k, case.pool, d["ids"], d["invalid"]), name)


# ---- the modules --------------------------------------------------------------------------------------------------------------------------
def clustered_vectors(n, g, dim=DIM, clusters=40):
    """items near one of a few centres: the head of a ranking holds near-duplicates, so the re-rank has something to do"""
    centres = torch.randn(clusters, dim, generator=g)
    return centres[torch.randint(0, clusters, (n,), generator=g)] + 0.3 * torch.randn(n, dim, generator=g)


def ranked_list(tk, q, k, kw, width, pool):
    """The list the call walks, by the module's own forward under _positions_as_ids() -> (scores, positions, D)."""
    D = MR.default_pool(k) if pool is None else pool
    if isinstance(tk, (rails_amd.MoLBruteForceTopK, rails_amd.MIPSBruteForceTopK)):
        kw = dict(kw)
        mask = tk._take_item_mask(kw, q.shape[0], k)
        kw["_resolved_mask"] = mask
        bound = tk.num_items if mask is None else mask.kept_min
        length = min(bound, D + width)
    else:
        length = tk._avg_top_k if type(tk) is rails_amd.MoLAvgTopK else k      # (Naive / Comb rank their whole union whatever k is)
    with tk._positions_as_ids():
        s, p = tk(q, k=length, **kw)
    return s.float().cpu().numpy(), p.cpu().numpy(), D


def cand_of(tk):
    return rails_amd.CandidateIndex(ids=tk._ids_flat.reshape(1, -1), embeddings=None)


def check(tk, q, k, kw, what, invalid=None, lam=0.7, pool=None, want_raise=False):
    """One diversified call -- forward, or get_top_k_outputs when there are invalid ids -- against the reference; -> (scores, ids)."""
    width = 0 if invalid is None else invalid.shape[1]
    s, p, D = ranked_list(tk, q, k, kw, width, pool)
    want = MR.walk(s, p, tk.item_vectors.cpu().numpy(), lam, k, D, tk._ids_flat.cpu().numpy(), None if invalid is None else invalid.cpu().numpy())
    call_kw = dict(kw, diversify=lam, **({} if pool is None else {"diversity_pool": pool}))

    def call():
        if invalid is None:
            return tk(q, k=k, **call_kw)
        got_ids, got_scores, _ = cand_of(tk).get_top_k_outputs(q, k, call_kw, tk, invalid)
        return got_scores, got_ids

    if want[4] or want_raise:
        assert want[4] and want_raise, what
        with pytest.raises(RuntimeError, match="selected index k out of range"):
            call()
        return None
    calls = tk.diversity_stats()["calls"]
    scores, ids = call()
    assert tk.diversity_stats()["calls"] == calls + 1, what
    assert scores.shape == (q.shape[0], k) and ids.shape == (q.shape[0], k) and scores.dtype == q.dtype, what
    assert np.array_equal(ids.cpu().numpy(), want[2]), what
    assert np.array_equal(scores.float().cpu().numpy().view(np.uint32), want[0]), what
    return scores, ids


def seen_of(tk, q, kw, dev, width=61):
    """(B, width) invalid ids: the three best items of every row's plain ranking, then ids nobody has"""
    top = tk(q, k=3, **kw)[1][:, :3]      # (Naive / Comb return their whole union whatever k is)
    return torch.cat([top, torch.full((q.shape[0], width - 3), -9, dtype=torch.int64, device=dev)], dim=1)


def plain_outputs(tk, q, k, kw, invalid):
    if invalid is None:
        return tk(q, k=k, **kw)
    ids, scores, _ = cand_of(tk).get_top_k_outputs(q, k, kw, tk, invalid)
    return scores, ids


def the_contract(tk, q, aux, dev, what, ks=(1, 10, 200)):
    """forward and get_top_k_outputs against the reference; diversify=1.0 and orthogonal / zero vectors against the plain call"""
    g = torch.Generator().manual_seed(71)
    n = tk.num_items
    plain = {k: tk(q, k=k, **aux) for k in ks}
    seen = seen_of(tk, q, aux, dev)
    plain_seen = plain_outputs(tk, q, 10, aux, seen)
    tk.set_item_vectors(clustered_vectors(n, g).to(dev), normalize=True)
    assert tk.item_vectors.shape == (n, DIM) and tk.item_vectors.dtype == torch.float32
    changed = False
    for k in ks:
        got = check(tk, q, k, aux, f"{what}: forward, k = {k}")
        changed |= k > 1 and not torch.equal(got[1], plain[k][1])
        U.same(tk(q, k=k, **aux), plain[k], f"{what}: plain call with vectors set, k = {k}")
        U.same(tk(q, k=k, diversify=1.0, **aux), plain[k], f"{what}: diversify=1.0, k = {k}")
    assert changed, "the re-rank changed nothing: the vectors prove nothing"
    got = check(tk, q, 10, aux, f"{what}: seen ids", seen)
    assert not bool((got[1].unsqueeze(2) == seen.unsqueeze(1)).any())
    check(tk, q, 10, aux, f"{what}: seen ids, lam = 0.3, pool = 65", seen, lam=0.3, pool=65)
    check(tk, q, 10, aux, f"{what}: pool = k", None, pool=10)
    U.same(plain_outputs(tk, q, 10, dict(aux, diversify=1.0), seen), plain_seen, f"{what}: diversify=1.0 under seen ids")
    tk.set_item_vectors(torch.zeros(n, 3, device=dev))
    U.same(tk(q, k=10, diversify=0.2, **aux), plain[10], f"{what}: zero vectors")
    U.same(plain_outputs(tk, q, 10, dict(aux, diversify=0.2), seen), plain_seen, f"{what}: zero vectors under seen ids")
    tk.clear_item_vectors()
    assert tk.item_vectors is None
    with pytest.raises(ValueError, match="without vectors"):
        tk(q, k=3, diversify=0.5, **aux)
    U.same(tk(q, k=10, **aux), plain[10], f"{what}: plain call after clear_item_vectors")
    tk.set_item_vectors(clustered_vectors(n, g).to(dev), normalize=True)


def surfaces(tk, q, aux, dev, what, sparse_ok=True):
    """get_top_k_outputs under the seen ids with allowed_tags=, item_mask= (shared and per row; the sparse and the dense strategy) and a hidden set"""
    g = torch.Generator().manual_seed(72)
    n, batch = tk.num_items, q.shape[0]
    tags = (torch.ones(n, dtype=torch.int64) << torch.randint(0, 4, (n,), generator=g)).to(dev)
    tk.set_item_tags(tags)
    allowed = [(0b0111, 0b1010, 0b1111, 0b0001)[b % 4] for b in range(batch)]
    kw = dict(aux, allowed_tags=allowed)
    check(tk, q, 10, kw, what + ": seen ids + allowed_tags", seen_of(tk, q, kw, dev))
    dense_shared = torch.rand(n, generator=g) < 0.6
    sparse_shared = torch.zeros(n, dtype=torch.bool)
    sparse_shared[torch.randperm(n, generator=g)[:1000]] = True
    per_row = torch.rand(batch, n, generator=g) < 0.6
    sparse_rows = torch.rand(batch, n, generator=g) < 0.2
    for name, m in (("dense shared", dense_shared), ("sparse shared", sparse_shared), ("dense per row", per_row), ("sparse per row", sparse_rows)):
        mask = E.ItemMask(m.to(dev))
        kw = dict(aux, item_mask=mask)
        if hasattr(tk, "_masked") and sparse_ok:
            assert tk._masked(tk._bind(), mask, count=False) == name.split()[0], name
        check(tk, q, 10, kw, f"{what}: seen ids + {name} mask", seen_of(tk, q, kw, dev))
    # a mask that keeps exactly k items, one of them seen: the pool is short of k, found through the walk's verdict word
    few = torch.zeros(n, dtype=torch.bool)
    few[torch.randperm(n, generator=g)[:12]] = True
    kw = dict(aux, item_mask=E.ItemMask(few.to(dev)))
    check(tk, q, 12, kw, what + ": twelve kept items", None)
    check(tk, q, 12, kw, what + ": twelve kept items, one seen", seen_of(tk, q, kw, dev, width=4), want_raise=True)
    tk.hide_items(torch.randperm(n, generator=g)[: n // 3])
    check(tk, q, 10, aux, what + ": hidden set", seen_of(tk, q, aux, dev))
    tk.unhide_items(tk.hidden_positions())


@pytest.mark.parametrize("mode", ["dense", "default"])
@pytest.mark.parametrize("batch", [5, 37])
def test_exact_module(batch, mode, dev):
    with torch.inference_mode():
        tk, q, aux, X, ids = CG.setup(dev, batch, **({"exact_mode": "dense"} if mode == "dense" else {}))
        if mode == "dense":
            CG.dense_mode(tk)
        assert tk.item_vectors is None and tk.diversity_stats() == {"calls": 0}
        the_contract(tk, q, aux, dev, f"{mode}, B = {batch}", ks=(1, 10, 200) if batch == 5 else (10,))
        if batch == 5:
            surfaces(tk, q, aux, dev, mode)


@pytest.mark.parametrize("route", sorted(CG.ROUTES))
def test_routes(route, dev):
    with torch.inference_mode():
        spec = dict(CG.ROUTES[route])
        batch = spec.pop("batch", 5)
        tk, q, aux, X, ids = CG.setup(dev, batch, **spec)
        if route == "chunked":
            tk.CHUNK_ITEMS, tk.MAX_LOGIT_BYTES = 1024, batch * 1024 * 4
        if route == "generic g_4x4x64":
            assert tk._bind().route == "generic"
        proved = tk.stats().get("proved_calls", 0)
        the_contract(tk, q, aux, dev, route, ks=(10, 200))
        if route == "proved":      # the ranked top-L came from the proved flow, and its verdicts cleared; then a forced redo ranks the same list
            st = tk.stats()
            assert tk.exact_mode == "proved" and tk._bind().exact is not None
            assert st["proved_calls"] > proved and st["bound_violations"] == 0, st
            seen = seen_of(tk, q, aux, dev)
            want = check(tk, q, 10, aux, "proved: seen ids", seen)
            st = tk.stats()
            tk._gate_guard_limit = 0.5 * st["guard_max"]
            U.same(plain_outputs(tk, q, 10, dict(aux, diversify=0.7), seen), want, "proved: forced redo")
            assert tk.stats()["fallbacks"] == st["fallbacks"] + 1


def test_mips(dev):
    g = torch.Generator().manual_seed(73)
    with torch.inference_mode():
        X = torch.randn(N, 48, generator=g).to(dev)
        ids = U.ids_of(N, dev)
        q = torch.randn(5, 48, generator=g).to(dev)
        tk = rails_amd.MIPSBruteForceTopK(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        the_contract(tk, q, {}, dev, "mips")
        surfaces(tk, q, {}, dev, "mips")


@pytest.mark.parametrize("min_items", [0, 1 << 62])
@pytest.mark.parametrize("kind", sorted(CG.APPROX))
def test_approximate_modules_diversify_their_own_ranking(kind, min_items, dev):
    g = torch.Generator().manual_seed(74)
    with torch.inference_mode():
        fx = Fixture("c3_books")
        mol = build_module(fx.cfg, fx.weights, dev)
        X, ids = U.table(fx.cfg, N, 7, dev), U.ids_of(N, dev)
        q, aux = O.synthetic_queries(fx.cfg, 5, seed=5).to(dev), CG.aux_of(fx.cfg, 5, dev)
        tk = CG.APPROX[kind](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        tk.fused_coarse_min_items = tk.fused_component_min_items = min_items
        plain = tk(q, k=10, **aux)
        seen = seen_of(tk, q, aux, dev)
        plain_seen = plain_outputs(tk, q, 10, aux, seen)
        tk.set_item_vectors(clustered_vectors(N, g).to(dev), normalize=True)
        for k in (1, 10, 200):
            check(tk, q, k, aux, f"{kind}: forward, k = {k}")
        check(tk, q, 10, aux, f"{kind}: seen ids", seen)
        check(tk, q, 10, aux, f"{kind}: seen ids, pool = 65", seen, lam=0.3, pool=65)
        U.same(tk(q, k=10, **aux), plain, f"{kind}: plain call with vectors set")
        got = tk(q, k=10, diversify=1.0, **aux)
        assert torch.equal(got[0][:, :10], plain[0][:, :10]) and torch.equal(got[1][:, :10], plain[1][:, :10]) and got[0].shape == (5, 10), kind
        U.same(plain_outputs(tk, q, 10, dict(aux, diversify=1.0), seen), plain_seen, f"{kind}: diversify=1.0 under seen ids")
        if kind != "naive":      # (MoLNaiveTopK has no submit)
            with pytest.raises(NotImplementedError, match="submit takes no diversify"):
                tk.submit(q, 10, diversify=0.5, **aux)
        if kind == "avg":      # 256 candidates, 61 of them seen: a pool of 195
            wide = torch.cat([tk(q, k=61, **aux)[1]], dim=1)
            check(tk, q, 200, aux, "avg: a pool short of k", wide, pool=200, want_raise=True)


def test_vectors_follow_a_chain_of_edits(dev):
    """update -> append (zero rows, then set by positions) -> remove across a tile boundary -> hide -> compact; after each step item_vectors is the
    table a fresh module is given, and the diversified calls of the two agree."""
    g = torch.Generator().manual_seed(75)
    with torch.inference_mode():
        tk, q, aux, X, ids = CG.setup(dev, 5)
        cfg = Fixture("c3_books").cfg
        mol = tk.mol_module
        vec = clustered_vectors(N, g).to(dev)
        tk.set_item_vectors(vec)
        seen = seen_of(tk, q, aux, dev)

        def agree(step, hidden=None):
            assert torch.equal(tk.item_vectors, vec) and tk.item_vectors.is_contiguous() and tk.num_items == X.shape[0] == vec.shape[0], step
            fresh = rails_amd.MoLBruteForceTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
            fresh.set_item_vectors(vec)
            if hidden is not None:
                fresh.hide_items(hidden)
            kw = dict(aux, diversify=0.6)
            U.same(tk(q, k=50, **kw), fresh(q, k=50, **kw), f"{step}: forward")
            U.same(cand_of(tk).get_top_k_outputs(q, 10, kw, tk, seen)[:2], cand_of(fresh).get_top_k_outputs(q, 10, kw, fresh, seen)[:2], f"{step}: seen ids")
            check(tk, q, 10, aux, f"{step}: against the reference", seen)

        pos = U.positions_for(N, g, extra=100).to(dev)                       # update: the vectors stay
        rows = U.table(cfg, pos.numel(), 21, dev, first=5_000_000)
        tk.update_items(pos, rows)
        X[pos] = rows
        agree("update")
        new_rows, new_ids = U.table(cfg, 40, 22, dev, first=6_000_000), U.ids_of(40, dev, first=N + 1000)      # append: zero rows, then set by positions
        tk.append_items(new_rows, new_ids)
        X, ids, vec = torch.cat([X, new_rows]), torch.cat([ids, new_ids]), torch.cat([vec, torch.zeros(40, DIM, device=dev)])
        agree("append")
        some = torch.arange(N, N + 20)
        given = clustered_vectors(20, g).to(dev)
        tk.set_item_vectors(given, positions=some)
        vec[some.to(dev)] = given
        agree("set_item_vectors(..., positions)")

        def removed(gone):
            nonlocal X, ids, vec
            n = X.shape[0]
            holes, movers = rails_amd.topk_modules.removal_plan(gone.cpu(), n)
            n_new = n - gone.numel()
            X2, ids2, vec2 = X[:n_new].clone(), ids[:n_new].clone(), vec[:n_new].clone()
            X2[holes.to(dev)], ids2[holes.to(dev)], vec2[holes.to(dev)] = X[movers.to(dev)], ids[movers.to(dev)], vec[movers.to(dev)]
            X, ids, vec = X2, ids2, vec2

        n = X.shape[0]
        gone = torch.cat([torch.arange(4090, 4102), torch.randperm(4000, generator=g)[:50], torch.tensor([n - 1, n - 3])])      # remove across a tile boundary
        tk.remove_items(gone)
        removed(gone)
        agree("remove")
        hide = torch.randperm(X.shape[0], generator=g)[:300]                   # hide, then compact
        tk.hide_items(hide)
        agree("hide", hide)
        gone = tk.hidden_positions().cpu()
        tk.compact()
        removed(gone)
        agree("compact")
