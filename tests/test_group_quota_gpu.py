"""GPU: max_per_group=m.  The reference of every module-level case is tests/_quota_ref.py's quota_walk applied to the
module's OWN all_logits(...) of the same call arguments, ordered on the host by (score desc, position asc) in exact integer arithmetic; the
comparison is torch.equal on ids and on scores, every row of every case.  The approximate modules are compared with quota_walk over their own
ranking.  The two new kernels are also driven on their own: the walk on hand-built lists, the fallback's rounds against the numpy round table
of integer keys.  The helpers, sizes and layouts are those of tests/test_collapse_gpu.py."""
import numpy as np
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from tests import _collapse_ref as CR
from tests import _quota_ref as QR
from tests import test_collapse_gpu as C
from tests import test_index_update_gpu as U
from tests._fixtures import Fixture
from tests.test_collapse_gpu import dev  # noqa: F401  (the device fixture)
from tests.test_generic_route_gpu import build_module

pytestmark = pytest.mark.gpu
N = C.N
NEG_INF = float("-inf")
MS = (2, 3)


def cand_of(tk):
    return rails_amd.CandidateIndex(ids=tk._ids_flat.reshape(1, -1), embeddings=None)


def check(tk, q, k, m, kw, what, invalid=None, want_raise=False, via=None):
    """One call with max_per_group=m -- forward, or get_top_k_outputs when there are invalid ids (via="filtered": forward_filtered itself) --
    against the reference; -> (scores, ids)."""
    keys, ids = tk.item_groups.cpu(), tk._ids_flat.cpu()
    want = QR.quota_topk(C.logits_of(tk, q, kw), keys, invalid, ids, k, m)
    call_kw = dict(kw, max_per_group=m)

    def call():
        if via == "filtered":
            got_ids, got_scores = tk.forward_filtered(q, k + invalid.shape[1], invalid, k, **call_kw)
            return got_scores, got_ids
        if invalid is None and via != "outputs":
            return tk(q, k=k, **call_kw)
        got_ids, got_scores, _ = cand_of(tk).get_top_k_outputs(q, k, call_kw, tk, invalid)
        return got_scores, got_ids

    if want is None or want_raise:
        assert want is None, what
        with pytest.raises(RuntimeError, match="out of range"):
            call()
        return None
    scores, got_ids = call()
    assert scores.shape == (q.shape[0], k) and got_ids.shape == (q.shape[0], k), what
    assert torch.equal(got_ids.cpu(), want[1]), what
    assert torch.equal(scores.float().cpu().view(torch.int32), want[0].view(torch.int32)), what
    return scores, got_ids


def both_paths(tk, q, k, m, kw, what, invalid=None):
    """the walk path as the module takes it, then the exact fallback forced (a walk of depth 0 never answers): same expected output"""
    check(tk, q, k, m, kw, what + ", walk", invalid)
    before = tk.collapse_stats()["fallbacks"]
    tk.COLLAPSE_DEPTH_FACTOR = 0
    try:
        check(tk, q, k, m, kw, what + ", forced fallback", invalid)
    finally:
        del tk.COLLAPSE_DEPTH_FACTOR
    assert tk.collapse_stats()["fallbacks"] == before + 1, what


def seen_of(tk, q, kw, dev, m, width=61):
    """(B, width) invalid ids holding, per row, the reference's first four results under the quota -- the best, and mostly the second, members
    of its best groups --, then ids nobody returns"""
    keys, ids = tk.item_groups.cpu(), tk._ids_flat.cpu()
    logits = C.logits_of(tk, q, kw).cpu()
    rows = []
    for b in range(q.shape[0]):
        _, _, top = QR.quota_walk(logits[b], CR.key_order(logits[b]), keys, None, ids, 4, m)
        rows.append(torch.tensor(top + [-7 - j for j in range(width - len(top))], dtype=torch.int64))
    return torch.stack(rows).to(dev)


# ---- the exact modules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "default"])
@pytest.mark.parametrize("batch", [5, 37])
def test_layouts(batch, mode, dev):
    g = torch.Generator().manual_seed(181)
    with torch.inference_mode():
        tk, q, aux, X, ids = C.setup(dev, batch, **({"exact_mode": "dense"} if mode == "dense" else {}))
        if mode == "dense":
            C.dense_mode(tk)
        plain = {k: tk(q, k=k, **aux) for k in (1, 10, 200)}
        keys = C.layout_a(N, g)
        tk.set_item_groups(keys.to(dev))
        for m in MS:
            for k in (1, 10, 200):
                both_paths(tk, q, k, m, aux, f"(a), B = {batch}, k = {k}, m = {m}")
        for k in (1, 10, 200):      # m = 1 is collapse_groups=True, on the launches of collapse_groups=True
            U.same(tk(q, k=k, max_per_group=1, **aux), tk(q, k=k, collapse_groups=True, **aux), f"m = 1, k = {k}")
            U.same(tk(q, k=k, max_per_group=1, collapse_groups=True, **aux), tk(q, k=k, collapse_groups=True, **aux), f"m = 1 with collapse_groups, k = {k}")
            U.same(tk(q, k=k, **aux), plain[k], f"plain call with groups set, k = {k}")
        largest = int(torch.bincount(keys[keys >= 0]).max())      # every group of size <= m: the uncollapsed call
        assert 2 < largest <= E.COLLAPSE_MAX_PER_GROUP
        for k in (10, 200):
            U.same(check(tk, q, k, largest, aux, f"m = the largest group, k = {k}"), plain[k], f"m = the largest group, k = {k}")
        seen = seen_of(tk, q, aux, dev, largest)      # ... and with seen ids the uncollapsed filtered call
        got_s, got_i = check(tk, q, 10, largest, aux, "m = the largest group, seen ids", seen)
        want_i, want_s, _ = cand_of(tk).get_top_k_outputs(q, 10, aux, tk, seen)
        U.same((got_s, got_i), (want_s, want_i), "m = the largest group: get_top_k_outputs with seen ids")
        # m >= k: m_eff = k, nothing among the first k can be excluded
        tk.set_item_groups(torch.zeros(N, dtype=torch.int32, device=dev))
        U.same(check(tk, q, 7, 1000, aux, "k = 7, m = 1000"), tk(q, k=7, **aux), "k = 7, m = 1000: one group, the plain top 7")
        # (d) one group for the whole corpus: exactly m survive
        for m in MS:
            U.same(check(tk, q, m, m, aux, f"(d) k = m = {m}"), tk(q, k=m, **aux), "(d): the top m items")
        fb = tk.collapse_stats()["fallbacks"]
        check(tk, q, 3, 2, aux, "(d) k = 3, m = 2", want_raise=True)
        assert tk.collapse_stats()["fallbacks"] == fb + 1      # raised only after the exact fallback established it
        with pytest.raises(RuntimeError) as e:
            tk(q, k=3, max_per_group=2, **aux)
        assert str(e.value).startswith("selected index k out of range (k=3, n=2: ")
        # (b) everything ungrouped: the plain call
        tk.set_item_groups(torch.full((N,), -1, dtype=torch.int32, device=dev))
        for k in (1, 10, 200):
            U.same(check(tk, q, k, 2, aux, f"(b), k = {k}"), plain[k], f"(b) against the plain call, k = {k}")
        tk.clear_item_groups()
        with pytest.raises(ValueError, match="without groups"):
            tk(q, k=3, max_per_group=2, **aux)
        U.same(tk(q, k=10, **aux), plain[10], "plain call after clear_item_groups")


@pytest.mark.parametrize("m", MS)
def test_a_giant_group_takes_the_first_walk_the_doubling_and_the_fallback(m, dev):
    g = torch.Generator().manual_seed(182)
    with torch.inference_mode():
        tk, q, aux, X, ids = C.setup(dev, 5, exact_mode="dense")
        C.dense_mode(tk)
        tk.set_item_groups(C.layout_c(tk.all_logits(q, **aux)[0], N, g).to(dev))
        for k in (10, 200):      # (k > m: row 0 needs items behind the giant group's 60 % of the ranking)
            answers = []
            s0 = tk.collapse_stats()
            tk.COLLAPSE_DEPTH_FACTOR = 4000 // k   # the first walk sees 4 000 ranked items: 1 500 behind the giant group on row 0
            answers.append(check(tk, q, k, m, aux, f"(c) first walk, k = {k}"))
            s1 = tk.collapse_stats()
            assert (s1["calls"], s1["walk_redos"], s1["fallbacks"]) == (s0["calls"] + 1, s0["walk_redos"], s0["fallbacks"])
            tk.COLLAPSE_DEPTH_FACTOR = 1           # k ranked items, doubled until the walk holds k survivors
            answers.append(check(tk, q, k, m, aux, f"(c) doubling, k = {k}"))
            s2 = tk.collapse_stats()
            assert s2["walk_redos"] > s1["walk_redos"] and s2["fallbacks"] == s1["fallbacks"], (s1, s2)
            tk.COLLAPSE_MAX_DEPTH = 64
            answers.append(check(tk, q, k, m, aux, f"(c) COLLAPSE_MAX_DEPTH = 64, k = {k}"))
            s3 = tk.collapse_stats()
            assert s3["fallbacks"] == s2["fallbacks"] + 1, (s2, s3)
            del tk.COLLAPSE_DEPTH_FACTOR, tk.COLLAPSE_MAX_DEPTH
            for other in answers[1:]:
                U.same(other, answers[0], f"(c) the three paths, k = {k}")
        assert sorted(tk.collapse_stats()) == ["calls", "fallbacks", "walk_redos"]


def test_all_scores_tie(dev):
    """(e) a corpus of identical rows: only the position tie rule decides, on the walk and on the forced fallback"""
    g = torch.Generator().manual_seed(183)
    with torch.inference_mode():
        tk, q, aux, X, ids = C.setup(dev, 5)
        tk.update_items(torch.arange(N), X[:1].expand(N, -1).contiguous())
        logits = tk.all_logits(q, **aux)
        assert bool((logits == logits[:, :1]).all())
        tk.set_item_groups(C.layout_a(N, g).to(dev))
        for m in MS:
            for k in (1, 10, 200):
                both_paths(tk, q, k, m, aux, f"(e) k = {k}, m = {m}")


def surfaces(tk, q, aux, dev, m, what, sparse_ok=True):
    """forward, forward_filtered and get_top_k_outputs under the seen ids, allowed_tags=, item_mask= (shared and per row; the sparse and the dense
    strategy) and a hidden set -- on whichever path the module's constants select."""
    g = torch.Generator().manual_seed(184)
    n, batch = tk.num_items, q.shape[0]
    check(tk, q, 10, m, aux, what + ": forward")
    check(tk, q, 10, m, aux, what + ": get_top_k_outputs without seen ids", via="outputs")
    seen = seen_of(tk, q, aux, dev, m)
    got = check(tk, q, 10, m, aux, what + ": seen ids", seen)
    assert not bool((got[1].unsqueeze(2) == seen.unsqueeze(1)).any())
    U.same(check(tk, q, 10, m, aux, what + ": forward_filtered", seen, via="filtered"), got, what + ": forward_filtered against get_top_k_outputs")
    tags = (torch.ones(n, dtype=torch.int64) << torch.randint(0, 4, (n,), generator=g)).to(dev)
    tk.set_item_tags(tags)
    allowed = [(0b0111, 0b1010, 0b1111, 0b0001)[b % 4] for b in range(batch)]
    kw = dict(aux, allowed_tags=allowed)
    check(tk, q, 10, m, kw, what + ": allowed_tags")
    check(tk, q, 10, m, kw, what + ": seen ids + allowed_tags", seen_of(tk, q, kw, dev, m))
    dense_shared = torch.rand(n, generator=g) < 0.6
    sparse_shared = torch.zeros(n, dtype=torch.bool)
    sparse_shared[torch.randperm(n, generator=g)[:1000]] = True
    per_row = torch.rand(batch, n, generator=g) < 0.6
    sparse_rows = torch.rand(batch, n, generator=g) < 0.2
    for name, bits in (("dense shared", dense_shared), ("sparse shared", sparse_shared), ("dense per row", per_row), ("sparse per row", sparse_rows)):
        mask = E.ItemMask(bits.to(dev))
        kw = dict(aux, item_mask=mask)
        if hasattr(tk, "_masked") and sparse_ok:
            assert tk._masked(tk._bind(), mask, count=False) == name.split()[0], name
        check(tk, q, 10, m, kw, f"{what}: {name} mask")
        check(tk, q, 10, m, kw, f"{what}: seen ids + {name} mask", seen_of(tk, q, kw, dev, m))
    tk.hide_items(torch.randperm(n, generator=g)[: n // 3])
    check(tk, q, 10, m, aux, what + ": hidden set")
    check(tk, q, 10, m, aux, what + ": seen ids + hidden set", seen_of(tk, q, aux, dev, m))
    tk.unhide_items(tk.hidden_positions())


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("mode", ["dense", "default"])
@pytest.mark.parametrize("layout", ["a", "c forced fallback"])
def test_call_surfaces(layout, mode, m, dev):
    g = torch.Generator().manual_seed(185)
    with torch.inference_mode():
        tk, q, aux, X, ids = C.setup(dev, 5, **({"exact_mode": "dense"} if mode == "dense" else {}))
        if mode == "dense":
            C.dense_mode(tk)
        if layout == "a":
            tk.set_item_groups(C.layout_a(N, g).to(dev))
        else:
            tk.set_item_groups(C.layout_c(tk.all_logits(q, **aux)[0], N, g).to(dev))
            tk.COLLAPSE_MAX_DEPTH = 64
        surfaces(tk, q, aux, dev, m, layout)
        if layout != "a":
            assert tk.collapse_stats()["fallbacks"] > 0


@pytest.mark.parametrize("route", sorted(C.ROUTES))
def test_routes(route, dev):
    g = torch.Generator().manual_seed(186)
    with torch.inference_mode():
        spec = dict(C.ROUTES[route])
        batch, n = spec.pop("batch", 5), spec.get("n", N)
        tk, q, aux, X, ids = C.setup(dev, batch, **spec)
        layout = C.layout_a
        if route == "chunked":      # about 200 groups: a table row of m * G * 8 = 5 KB fits the policy of 20 KB four queries at a time, whose scores
            tk.CHUNK_ITEMS, tk.MAX_LOGIT_BYTES = 1024, batch * 1024 * 4      # do not -- five chunks, scored again every round; the fifth query alone is one chunk
            layout = lambda n_items, gen: torch.randint(0, n_items // 20, (n_items,), generator=gen)      # noqa: E731
        if route == "generic g_4x4x64":
            assert tk._bind().route == "generic"
        tk.set_item_groups(layout(n, g).to(dev))
        proved = tk.stats().get("proved_calls", 0)
        for m in MS:
            for k in (1, 10, 200):
                check(tk, q, k, m, aux, f"{route}, k = {k}, m = {m}")
            both_paths(tk, q, 10, m, aux, f"{route}: seen ids, m = {m}", seen_of(tk, q, aux, dev, m))
        if route == "proved":      # the ranked top-D came from the proved flow, and its verdicts cleared
            st = tk.stats()
            assert tk.exact_mode == "proved" and tk._bind().exact is not None
            assert st["proved_calls"] > proved and st["bound_violations"] == 0, st
        keys = layout(n, g)      # (c): one giant group (key 0) owning the top 60 % of row 0's ranking
        keys[keys >= 0] += 1
        keys[CR.key_order(tk.all_logits(q, **aux)[0])[: n * 6 // 10]] = 0
        tk.set_item_groups(keys.to(dev))
        tk.COLLAPSE_MAX_DEPTH = 64
        fb = tk.collapse_stats()["fallbacks"]
        for m in MS:
            check(tk, q, 10, m, aux, f"{route}: (c), forced fallback, m = {m}", seen_of(tk, q, aux, dev, m))
        assert tk.collapse_stats()["fallbacks"] == fb + len(MS)


def test_mips(dev):
    g = torch.Generator().manual_seed(187)
    with torch.inference_mode():
        X = torch.randn(N, 48, generator=g).to(dev)
        ids = U.ids_of(N, dev)
        q = torch.randn(5, 48, generator=g).to(dev)
        tk = rails_amd.MIPSBruteForceTopK(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        plain = tk(q, k=10)
        tk.set_item_groups(C.layout_a(N, g).to(dev))
        for m in MS:
            for k in (1, 10, 200):
                both_paths(tk, q, k, m, {}, f"mips, k = {k}, m = {m}")
            surfaces(tk, q, {}, dev, m, f"mips (a), m = {m}")
        U.same(tk(q, k=10, max_per_group=1), tk(q, k=10, collapse_groups=True), "mips: m = 1")
        U.same(tk(q, k=10), plain, "mips: plain call with groups set")
        tk.set_item_groups(C.layout_c(tk._index.score(q)[0], N, g).to(dev))
        tk.COLLAPSE_MAX_DEPTH = 64
        surfaces(tk, q, {}, dev, 3, "mips (c), forced fallback")
        assert tk.collapse_stats()["fallbacks"] > 0


# ---- the approximate modules ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_items", [0, 1 << 62])
@pytest.mark.parametrize("kind", sorted(C.APPROX))
def test_approximate_modules_apply_the_quota_to_their_own_ranking(kind, min_items, dev):
    g = torch.Generator().manual_seed(188)
    with torch.inference_mode():
        fx = Fixture("c3_books")
        mol = build_module(fx.cfg, fx.weights, dev)
        X, ids = U.table(fx.cfg, N, 7, dev), U.ids_of(N, dev)
        q, aux = O.synthetic_queries(fx.cfg, 5, seed=5).to(dev), C.aux_of(fx.cfg, 5, dev)
        tk = C.APPROX[kind](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        tk.fused_coarse_min_items = tk.fused_component_min_items = min_items
        ranked_s, ranked_i = tk(q, k=256, **aux)      # all candidates, ranked: MoLAvgTopK's avg_top_k; the union whatever k is
        plain = tk(q, k=10, **aux)
        keys = C.layout_a(N, g)
        tk.set_item_groups(keys.to(dev))
        pos_of_id = {int(i): p for p, i in enumerate(ids.cpu().tolist())}

        def want(k, m, invalid):
            rows_s, rows_i = [], []
            for b in range(5):
                s, i = ranked_s[b].float().cpu(), ranked_i[b].cpu()
                real = s != -32767.0      # (a masked duplicate of the union is no candidate)
                order = [pos_of_id[int(x)] for x in i[real].tolist()]
                by_pos = torch.full((N,), NEG_INF)
                by_pos[torch.tensor(order)] = s[real]
                out_s, _, out_i = QR.quota_walk(by_pos, order, keys, None if invalid is None else invalid[b].cpu(), ids.cpu(), k, m)
                if len(out_i) < k:      # fewer than k survivors among this row's candidates: the call raises
                    return None
                rows_s.append(torch.tensor(out_s))
                rows_i.append(torch.tensor(out_i))
            return torch.stack(rows_s), torch.stack(rows_i)

        for m in (2, 3, 40):      # (no limit on m here: 40 is beyond the exact modules')
            for k in (1, 10, 200):
                expected = want(k, m, None)
                if expected is None:
                    with pytest.raises(RuntimeError, match="out of range"):
                        tk(q, k=k, max_per_group=m, **aux)
                    continue
                s, i = tk(q, k=k, max_per_group=m, **aux)
                assert s.shape == (5, k) and torch.equal(i.cpu(), expected[1]) and torch.equal(s.float().cpu(), expected[0]), (kind, k, m)
            assert want(10, m, None) is not None
            seen = torch.cat([want(4, m, None)[1], torch.full((5, 57), -9)], dim=1).to(dev)
            gi, gs, _ = cand_of(tk).get_top_k_outputs(q, 10, dict(aux, max_per_group=m), tk, seen)
            ws, wi = want(10, m, seen)
            assert torch.equal(gi.cpu(), wi) and torch.equal(gs.float().cpu(), ws), (kind, m)
            if kind != "naive":
                s, i = tk.result(tk.submit(q, 10, max_per_group=m, **aux))
                ws, wi = want(10, m, None)
                assert torch.equal(i.cpu(), wi) and torch.equal(s.float().cpu(), ws), (kind, m)
        U.same(tk(q, k=10, max_per_group=1, **aux), tk(q, k=10, collapse_groups=True, **aux), f"{kind}: m = 1")
        U.same(tk(q, k=10, **aux), plain, f"{kind}: plain call with groups set")
        tk.set_item_groups(torch.zeros(N, dtype=torch.int32, device=dev))      # too few survivors among the candidates
        tk(q, k=2, max_per_group=2, **aux)
        with pytest.raises(RuntimeError, match="out of range"):
            tk(q, k=3, max_per_group=2, **aux)
        assert tk.collapse_stats()["fallbacks"] == 0 and tk.collapse_stats()["walk_redos"] == 0


# ---- edits ------------------------------------------------------------------------------------------------------------------------------
def test_groups_follow_a_chain_of_edits(dev):
    """update -> append (new items -1, then keyed by positions) -> remove across a tile boundary -> hide -> by-id remove -> compact; after each
    step the quota call equals a fresh module's of the resulting table, ids and key row, and the reference."""
    g = torch.Generator().manual_seed(189)
    with torch.inference_mode():
        tk, q, aux, X, ids = C.setup(dev, 5)
        cfg = Fixture("c3_books").cfg
        mol = tk.mol_module
        keys = C.layout_a(N, g).to(torch.int32).to(dev)
        tk.set_item_groups(keys)
        seen = seen_of(tk, q, aux, dev, 2)

        def agree(step, hidden=None):
            assert torch.equal(tk.item_groups, keys) and tk.num_items == X.shape[0] == keys.numel(), step
            fresh = rails_amd.MoLBruteForceTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
            fresh.set_item_groups(keys)
            if hidden is not None:
                fresh.hide_items(hidden)
            for m in MS:
                kw = dict(aux, max_per_group=m)
                for k in (10, 200):
                    U.same(tk(q, k=k, **kw), fresh(q, k=k, **kw), f"{step}: forward, k = {k}, m = {m}")
                U.same(cand_of(tk).get_top_k_outputs(q, 10, kw, tk, seen)[:2], cand_of(fresh).get_top_k_outputs(q, 10, kw, fresh, seen)[:2], f"{step}: seen ids")
                check(tk, q, 10, m, aux, f"{step}: against the reference, m = {m}", seen)

        pos = U.positions_for(N, g, extra=100).to(dev)                       # update: the keys stay
        rows = U.table(cfg, pos.numel(), 21, dev, first=5_000_000)
        tk.update_items(pos, rows)
        X[pos] = rows
        agree("update")
        new_rows, new_ids = U.table(cfg, 40, 22, dev, first=6_000_000), U.ids_of(40, dev, first=N + 1000)      # append: -1, then keyed by positions
        tk.append_items(new_rows, new_ids)
        X, ids, keys = torch.cat([X, new_rows]), torch.cat([ids, new_ids]), torch.cat([keys, torch.full((40,), -1, dtype=torch.int32, device=dev)])
        agree("append")
        some = torch.arange(N, N + 20)
        tk.set_item_groups(torch.arange(20, dtype=torch.int64, device=dev) % 3, positions=some)
        keys[some.to(dev)] = (torch.arange(20, device=dev) % 3).to(torch.int32)

        def removed(gone):
            nonlocal X, ids, keys
            n = X.shape[0]
            holes, movers = rails_amd.topk_modules.removal_plan(gone.cpu(), n)
            n_new = n - gone.numel()
            X2, ids2, keys2 = X[:n_new].clone(), ids[:n_new].clone(), keys[:n_new].clone()
            X2[holes.to(dev)], ids2[holes.to(dev)], keys2[holes.to(dev)] = X[movers.to(dev)], ids[movers.to(dev)], keys[movers.to(dev)]
            X, ids, keys = X2, ids2, keys2

        n = X.shape[0]
        gone = torch.cat([torch.arange(4090, 4102), torch.randperm(4000, generator=g)[:50], torch.tensor([n - 1, n - 3])])      # remove across a tile boundary
        tk.remove_items(gone)
        removed(gone)
        agree("remove")
        hide = torch.randperm(X.shape[0], generator=g)[:300]                   # hide
        tk.hide_items(hide)
        agree("hide", hide)
        by_id = ids[torch.randperm(X.shape[0], generator=g)[:30].to(dev)]
        by_id = by_id[~torch.isin(by_id, ids[hide.to(dev)])]                   # by-id remove (of visible items)
        gone = tk.positions_of(by_id).cpu()
        hidden_ids = ids[hide.to(dev)]
        tk.remove_items_by_id(by_id)
        removed(gone)
        agree("remove by id", tk.positions_of(hidden_ids).cpu())
        gone = tk.hidden_positions().cpu()                                     # compact
        tk.compact()
        removed(gone)
        agree("compact")


def test_refusals_come_before_any_launch(dev):
    g = torch.Generator().manual_seed(190)
    with torch.inference_mode():
        fx = Fixture("c3_books")
        mol = build_module(fx.cfg, fx.weights, dev)
        X, ids = U.table(fx.cfg, N, 7, dev), U.ids_of(N, dev)
        q, aux = O.synthetic_queries(fx.cfg, 5, seed=5).to(dev), C.aux_of(fx.cfg, 5, dev)
        tk = rails_amd.MoLBruteForceTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        with pytest.raises(ValueError, match="without groups"):
            tk(q, k=3, max_per_group=2, **aux)
        with pytest.raises(ValueError, match="without groups"):
            cand_of(tk).get_top_k_outputs(q, 3, dict(aux, max_per_group=2), tk, ids[:5].reshape(5, 1))
        keys = C.layout_a(N, g)
        tk.set_item_groups(keys.to(dev))
        calls = tk.collapse_stats()["calls"]
        for bad in (0, True, 2.0, torch.tensor(2, device=dev)):
            with pytest.raises(ValueError, match="Python int"):
                tk(q, k=3, max_per_group=bad, **aux)
        with pytest.raises(ValueError, match="collapse_groups=True means max_per_group=1"):
            tk(q, k=3, max_per_group=2, collapse_groups=True, **aux)
        for call, name in ((lambda: tk.all_logits(q, max_per_group=2, **aux), "all_logits"), (lambda: tk.rank_of(q, ids[:5].reshape(5, 1), max_per_group=2, **aux), "rank_of"),
                           (lambda: C.APPROX["avg"](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0)).topk_ids(q, max_per_group=2, **aux), "topk_ids")):
            with pytest.raises(NotImplementedError, match=name + " takes no max_per_group"):
                call()
        with pytest.raises(NotImplementedError, match="k <= 512"):
            tk(q, k=513, max_per_group=2, **aux)
        with pytest.raises(NotImplementedError, match="<= 32 on the exact modules"):
            tk(q, k=40, max_per_group=33, **aux)
        with pytest.raises(NotImplementedError, match="seen ids"):
            cand_of(tk).get_top_k_outputs(q, 3, dict(aux, max_per_group=2), tk, torch.zeros((5, 4097), dtype=torch.int64, device=dev))
        assert tk.collapse_stats()["calls"] == calls      # (nothing launched)
        tk.clear_item_groups()
        ivf = rails_amd.MoLNaiveTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0), k_per_group=5, use_faiss=True, nlist=8)
        with pytest.raises(NotImplementedError, match="IVF, use_faiss=True. takes no max_per_group"):
            ivf(q, k=3, max_per_group=2, **aux)
        assert ivf._ivf is None      # (nothing was built, nothing launched)
        naive = C.APPROX["naive"](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        naive.set_item_groups(keys.to(dev))
        for call in (naive.local_candidates, C.APPROX["comb"](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0)).coarse_candidates):
            with pytest.raises(NotImplementedError, match="takes no max_per_group"):
                call(q, max_per_group=2, **aux)


# ---- the kernels on their own ---------------------------------------------------------------------------------------------------------------
def walk(scores, positions, ranks, k, m, ids, invalid, dev):
    """rails_topk_collapse_quota (m = None: rails_topk_collapse) -> (scores, positions, ids, counts, verdict word)"""
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = E.topk_collapse(scores.to(dev), positions.to(dev), ranks.to(torch.int32).to(dev), k, None if ids is None else ids.to(dev),
                          None if invalid is None else invalid.to(dev), flag, m)
    return tuple(t.cpu() for t in out) + (int(flag.item()),)


def ranks_with_runs(n, list_positions, sizes, g):
    """(n,) ranks: the entries of the list, taken in a random order, form groups of the sizes given (cycled), so the members of a group are
    scattered over the list; every position outside the list has a rank of its own."""
    depth = list_positions.numel()
    ranks = torch.arange(n, dtype=torch.int64) + depth
    order = list_positions[torch.randperm(depth, generator=g)]
    at, group = 0, 0
    while at < depth:
        size = sizes[group % len(sizes)]
        ranks[order[at : at + size]] = group
        at += size
        group += 1
    return ranks


def expect_walk(scores_row, positions_row, ranks, invalid_row, ids, n, m):
    """the reference over one hand-built list -> every survivor of the list, in order"""
    by_pos = torch.full((n,), NEG_INF)
    inside = (positions_row >= 0) & (positions_row < n)
    by_pos[positions_row[inside]] = scores_row[inside]
    return QR.quota_walk(by_pos, positions_row[inside], ranks, invalid_row, ids, positions_row.numel(), m)


@pytest.mark.parametrize("k", [1, 512])
@pytest.mark.parametrize("depth", [1, 63, 64, 65, 4096, 8192, 16384])      # (8 192 and 16 384: the widest in-LDS sorts, the launch's LDS ceiling)
def test_walk_kernel_on_hand_built_lists(depth, k, dev):
    g = torch.Generator().manual_seed(191)
    n, rows = 20000, 2
    ids = torch.randperm(n, generator=g) * 5 + 2
    first = torch.randperm(n, generator=g)[:depth]
    positions = torch.stack([first, first.flip(0)])      # one set of entries in two orders: the same runs, other members first
    scores = torch.sort(torch.randint(-50, 50, (rows, depth), generator=g).float(), dim=1, descending=True).values      # tied scores abound
    per = max(1, -(-depth // 1024))      # sorted slots per thread of the quota's scan
    case = 0
    promoted = set()      # (m, width) of the one-group cases that reached "the first m members seen, the next m promoted"
    for m in (1, 2, 3, 7, 32):
        layouts = {
            "one group": torch.zeros(n, dtype=torch.int64),
            "all ungrouped": torch.randperm(n, generator=g),
            "runs of m - 1, m, m + 1": ranks_with_runs(n, first, [max(1, m - 1), m, m + 1], g),
            "runs across segments and waves": ranks_with_runs(n, first, [per + 1, 64 * per + 1, 3, 64 * per - 1, 100], g),
        }
        lead = torch.stack([ids[positions[r, : min(depth, m)]] for r in range(rows)])      # the first m entries of the list (one group: its first m members)
        for name, ranks in layouts.items():
            if name == "one group":
                widths = (0, 1, 256, 257)      # every seen width on the layout where the seen entries ARE a group's first members
            else:      # two of the four, rotating: three layouts against four pairs, so every layout meets every width over the m
                widths = ((0, 256), (1, 257), (0, 257), (1, 256))[case % 4]
                case += 1
            for width in widths:
                if width == 0:
                    invalid = None
                elif width == 1:
                    invalid = lead[:, :1]
                else:
                    invalid = torch.cat([lead, torch.full((rows, width - lead.shape[1]), -3, dtype=torch.int64)], dim=1)[:, torch.randperm(width, generator=g)]
                use_ids = None if (invalid is None and name != "one group" and m % 2 == 1) else ids      # ids = NULL: a position is its own id
                s, p, i, counts, flag = walk(scores, positions, ranks, k, m, use_ids, invalid, dev)
                short = False
                for r in range(rows):
                    ws, wp, wi = expect_walk(scores[r], positions[r], ranks, None if invalid is None else invalid[r], use_ids, n, m)
                    assert counts[r] == len(wp), (name, m, width, r, int(counts[r]), len(wp))
                    if name == "one group" and depth >= 2 * m:
                        assert len(wp) == m      # exactly m survive ...
                        if width >= m:           # ... and with the group's first m members seen, the next m are promoted
                            assert wp == positions[r, m : 2 * m].tolist(), (m, width, r)
                            promoted.add((m, width))
                        elif width == 0:
                            assert wp == positions[r, :m].tolist(), (m, r)
                    take = min(k, len(wp))
                    short |= len(wp) < k
                    assert p[r, :take].tolist() == wp[:take] and i[r, :take].tolist() == wi[:take] and s[r, :take].tolist() == ws[:take], (name, m, width, r)
                    assert bool((p[r, take:] == -1).all()) and bool((i[r, take:] == -1).all()) and bool((s[r, take:] == NEG_INF).all()), (name, m, width, r)
                assert flag == int(short), (name, m, width)
                if m == 1:      # the plain walk's outputs, counts and verdict, bit for bit
                    plain = walk(scores, positions, ranks, k, None, use_ids, invalid, dev)
                    assert all(torch.equal(a, b) for a, b in zip(plain[:4], (s, p, i, counts))) and plain[4] == flag, (name, width)
    want_promoted = {(m, w) for m in (1, 2, 3, 7, 32) if depth >= 2 * m for w in (256, 257)} | ({(1, 1)} if depth >= 2 else set())
    assert promoted == want_promoted, (promoted, want_promoted)
    # entries that are not eligible by themselves: a position outside the corpus, a score of -inf -- they neither count nor fill
    if depth >= 63:
        ranks = torch.zeros(n, dtype=torch.int64)
        sc, ps = scores.clone(), positions.clone()
        sc[:, 1], ps[:, 0], ps[:, 3] = NEG_INF, -1, n
        s, p, i, counts, flag = walk(sc, ps, ranks, 1, 3, None, None, dev)
        assert counts.tolist() == [3] * rows and flag == 0 and torch.equal(p[:, 0], ps[:, 2]) and torch.equal(i, p)
        s, p, i, counts, flag = walk(sc, ps, ranks, 512, 3, ids, None, dev)
        assert flag == 1 and torch.equal(p[:, :3], ps[:, [2, 4, 5]]) and torch.equal(i[:, :3], ids[ps[:, [2, 4, 5]]]) and bool((p[:, 3:] == -1).all())


def keys_of_table(table):
    """(rows, m * G) int64 device table -> (rows, m * G) uint64 numpy"""
    return table.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("groups_kind", ["G = 1", "G = N", "groups of ~5"])
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 70001])
def test_group_next_and_topk_keys_against_the_round_table_of_integer_keys(n, groups_kind, dev):
    g = torch.Generator().manual_seed(192)
    rows, top_m = 3, 8
    ranks = {"G = 1": torch.zeros(n, dtype=torch.int32), "G = N": torch.randperm(n, generator=g).to(torch.int32),
             "groups of ~5": torch.randint(0, max(1, n // 5), (n,), generator=g).to(torch.int32)}[groups_kind]
    groups = int(ranks.max()) + 1
    ids = torch.randperm(n, generator=g) * 3 + 1
    scores = torch.randint(-3, 4, (rows, n), generator=g).float()      # small integers: ties abound
    scores[:, torch.randperm(n, generator=g)[: n // 18]] = NEG_INF     # -inf columns
    if n > 64:      # what the eligibility test of the group-maxima kernel sees: +-inf and NaN are skipped, -0 ranks below +0
        special = torch.randperm(n, generator=g)[:12]
        scores[0, special] = torch.tensor([float("inf"), NEG_INF, float("nan"), -0.0, 0.0, -0.0, 0.0, float("inf"), float("nan"), 3e-40, -3e-40, -0.0])
        scores[1, :] = NEG_INF                                         # ... and a row with nothing eligible
    unseen = QR.round_table(scores, ranks, groups, top_m, ids, None)
    # seen ids that hit the best, the second and the third member of some groups, then ids nobody has
    hits = []
    for b in range(rows):
        taken = [int(0xFFFFFFFF - (int(unseen[b, t, r]) & 0xFFFFFFFF)) for t in range(3) for r in range(t, groups, max(1, groups // 7)) if unseen[b, t, r] != 0][:40]
        hits.append(torch.cat([ids[torch.tensor(taken, dtype=torch.int64)], torch.full((61 - len(taken),), -5, dtype=torch.int64)]))
    invalid = torch.stack(hits)
    cuts = (0, n) if n < 4096 else (0, 4096 + 5 if n > 4101 else 4090, n)      # two chunks: a first_item offset that is no multiple of anything
    case = 0
    for inv, model in ((None, unseen), (invalid, QR.round_table(scores, ranks, groups, top_m, ids, invalid))):
        for m in (2, 3, 8):
            ld = n if case % 2 == 0 else n + 5
            case += 1
            padded = torch.full((rows, ld), 7.0)      # (a column beyond n outranks everything: it must not be read)
            padded[:, :n] = scores
            tables = []
            for run in range(2):      # a second run of the same calls gives the same bits
                table = torch.zeros((rows, m * groups), dtype=torch.int64, device=dev)
                for t in range(m):
                    pieces = list(zip(cuts, cuts[1:]))
                    for lo, hi in (pieces if t % 2 == 0 else pieces[::-1]):      # the chunks of a round in any order
                        chunk = padded.to(dev)[:, lo:] if hi == n else padded[:, lo:hi].contiguous().to(dev)
                        E.scores_group_next(chunk[:, : hi - lo], ranks.to(dev), table, groups, t, first_item=lo, ids=ids.to(dev),
                                            invalid_ids=None if inv is None else inv.to(dev))
                tables.append(table)
            assert torch.equal(tables[0], tables[1])
            got = keys_of_table(tables[0]).reshape(rows, m, groups)
            assert np.array_equal(got, model[:, :m]), (groups_kind, n, m, inv is not None)
            if m == 2 and n > 1:      # round 0 is the group-maxima pass
                best = torch.full((rows, groups), -1, dtype=torch.int64, device=dev)
                E.scores_group_max(padded.to(dev)[:, :n], ranks.to(dev), best, ids=ids.to(dev), invalid_ids=None if inv is None else inv.to(dev))
                assert torch.equal(best, tables[0][:, :groups])
            for k in (1, 10, 512):
                s, p, i, counts = (x.cpu() for x in E.topk_keys(tables[0], k, ids.to(dev)))
                assert counts.tolist() == (model[:, :m] != 0).reshape(rows, -1).sum(axis=1).tolist()
                for r, (want_s, want_p) in enumerate(QR.table_topk(model[:, :m], k)):
                    take = len(want_p)
                    assert p[r, :take].tolist() == want_p and i[r, :take].tolist() == ids[want_p].tolist() if take else True
                    assert s[r, :take].view(torch.int32).tolist() == torch.tensor(want_s, dtype=torch.float32).view(torch.int32).tolist() if take else True
                    assert bool((p[r, take:] == -1).all()) and bool((i[r, take:] == -1).all()) and bool((s[r, take:] == NEG_INF).all())
                    # ... and it is the reference walk's answer over the finite scores
                    finite = torch.where(torch.isfinite(scores[r]), scores[r], torch.tensor(NEG_INF))
                    assert want_p == QR.quota_walk(finite, CR.key_order(finite), ranks, None if inv is None else inv[r], ids, k, m)[1]
