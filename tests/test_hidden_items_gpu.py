"""GPU: hidden items.  The contract: a module with hidden set H answers every call as a module FRESHLY CONSTRUCTED from the
visible rows and their ids would -- torch.equal on scores and ids -- on the fused scans (their visible kernels), the materialising route, the
int8 pre-filter, the exact modules' masked strategies, and across corpus edits.  Engine level: the sample scan keeps hidden items out of the
threshold.  Inputs and helpers: those of tests/test_index_update_gpu.py, tests/test_item_mask_gpu.py and tests/test_candidate_scans_gpu.py."""
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from tests import test_candidate_scans_gpu as CS
from tests import test_index_remove_gpu as R
from tests import test_index_update_gpu as U
from tests import test_item_mask_gpu as M

pytestmark = pytest.mark.gpu
N = 4_037             # a ragged last tile of 5 items; the smallest corpora the fused plans accept at K' = 100 are 4 000 items
K_PRIME, K_GROUP = 100, 5
NEG_INF = float("-inf")
FUSED, MATERIALISED = 0, 1 << 62
MAKERS = {
    "avg": lambda mol, x, i: rails_amd.MoLAvgTopK(mol, x, i, avg_top_k=K_PRIME),
    "naive": lambda mol, x, i: rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=K_GROUP),
    "comb": lambda mol, x, i: rails_amd.MoLCombTopK(mol, x, i, avg_top_k=K_PRIME, k_per_group=K_GROUP),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def routed(tk, min_items):
    """Both scans of the module on the fused route (0) or the materialising one (1 << 62)."""
    tk.fused_coarse_min_items = tk.fused_component_min_items = min_items
    return tk


def approx_calls(tk, q, ids, X, aux, seen=None):
    """forward, get_top_k_outputs with a 61-wide seen list and without, submit / result (MoLAvgTopK), all_logits -> their outputs."""
    out = {"forward": tk(q, k=10, **aux)}
    if seen is None:
        seen = out["forward"][1][:, :61].contiguous()
        if seen.shape[1] < 61:
            seen = torch.cat([seen, ids[:61 - seen.shape[1]].reshape(1, -1).expand(q.shape[0], -1)], dim=1).contiguous()
    cand = rails_amd.CandidateIndex(ids=ids.reshape(1, -1), embeddings=X.reshape(1, *X.shape[-2:]))
    out["filtered"] = cand.get_top_k_outputs(q, 30, aux, tk, seen)[:2]
    out["plain"] = cand.get_top_k_outputs(q, 30, aux, tk, None)[:2]
    if isinstance(tk, rails_amd.MoLAvgTopK) and not isinstance(tk, rails_amd.MoLCombTopK):
        h1, h2 = tk.submit(q, 10, **aux), tk.submit(q, K_PRIME, **aux)
        out["submit_a"], out["submit_b"] = tk.result(h1), tk.result(h2)
    return out, seen


def keep_of(tk, n, dev):
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    keep[tk.hidden_positions()] = False
    assert int(keep.sum()) == tk.num_visible == n - tk.num_hidden
    return keep


def equals_fresh_of_visible(tk, make, X, ids, q, aux, what, min_items, dev):
    """tk (hidden set inside) against a module freshly built from its visible rows; the visible columns of all_logits too."""
    keep = keep_of(tk, X.shape[0], dev)
    fresh = routed(make(X[keep].clone().unsqueeze(0), ids[keep].clone().unsqueeze(0)), min_items)
    got, seen = approx_calls(tk, q, ids, X, aux)
    want, _ = approx_calls(fresh, q, ids[keep], X[keep], aux, seen=seen)
    for name in want:
        U.same(got[name], want[name], f"{what}: {name}")
    gone = ids[~keep]
    for name in got:
        res_ids = got[name][0] if name in ("filtered", "plain") else got[name][1]
        assert not bool(torch.isin(res_ids, gone).any()), f"{what}: {name} returned a hidden id"
    return got


def shape_setup(shape, dev, batch):
    cfg = CS.cfg_of(shape)
    mol = CS.module_of(shape)
    uid = CS.user_ids(shape, batch)
    return cfg, mol, ({} if uid is None else {"user_ids": uid}), O.synthetic_queries(cfg, batch, seed=5).to(dev)


def hidden_sets(tk, q, aux, ids, g, dev):
    """name -> how to hide it: (positions, by_id).  The sets of the contract."""
    n = tk.num_items
    returned = torch.unique(tk(q[:2], k=10, **({k: v[:2] for k, v in aux.items()}))[1])       # a filter applied after the selection would return fewer rows
    spare = torch.randperm(n, generator=g)[: 2 * K_PRIME]
    all_but = torch.ones(n, dtype=torch.bool)
    all_but[spare] = False
    return {
        "random 50 %": (torch.randperm(n, generator=g)[: n // 2], False),      # (2 019 of 4 037 stay visible: still the fused route)
        "one whole tile": (torch.arange(64, 96), False),
        "the ragged last tile": (torch.arange((n - 1) // 32 * 32, n), False),
        "the ids an unhidden call returns": (returned, True),
        "all but 2 K'": (torch.nonzero(all_but).reshape(-1).to(dev), False),
    }


@pytest.mark.parametrize("route", ["fused", "materialised"])
@pytest.mark.parametrize("shape", ["8x8x32", "8x4x128"])
@pytest.mark.parametrize("kind", ["avg", "naive", "comb"])
def test_module_equals_a_fresh_module_of_the_visible_rows(kind, shape, route, dev):
    """B = 2: one query tile (16 component rows); B = 33: two query tiles, and 264 component rows -- past the 256-row (128 at d = 128) slice."""
    min_items = FUSED if route == "fused" else MATERIALISED
    g = torch.Generator().manual_seed(41)
    with torch.inference_mode():
        for batch in (2, 33):
            cfg, mol, aux, q = shape_setup(shape, dev, batch)
            make = lambda x, i: MAKERS[kind](mol, x, i)      # noqa: E731
            X, ids = U.table(cfg, N, 7, dev), U.ids_of(N, dev)
            tk = routed(make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), min_items)
            unhidden, _ = approx_calls(tk, q, ids, X, aux)
            if route == "fused":      # the plans accept these sizes: the fused entries answer
                eng, eq = tk._bind(), tk._bind().query_pack(q[:2], aux.get("user_ids", q)[:2] if aux else None, want_plain=True)[1]
                if kind != "naive":
                    assert eng.coarse_topk(eq, tk._table(), False, K_PRIME, with_flag=True) is not None
                if kind != "avg":
                    assert eng.component_topk(eq, tk._component_table(), K_GROUP, torch.zeros(1, dtype=torch.int32, device=dev)) is not None
            for name, (pos, by_id) in hidden_sets(tk, q, aux, ids, g, dev).items():
                what = f"{kind} {shape} {route}, B = {batch}, {name}"
                if by_id:
                    tk.hide_items_by_id(pos)
                    got_pos = tk.positions_of(pos)
                else:
                    tk.hide_items(pos)
                    got_pos = pos.to(dev)
                assert tk.num_hidden == pos.numel() and torch.equal(tk.hidden_positions(), torch.sort(got_pos).values), what
                got = equals_fresh_of_visible(tk, make, X, ids, q, aux, what, min_items, dev)
                if by_id:
                    assert not bool(torch.isin(got["forward"][1][:2, :10], pos).any()), what
                logits = tk.all_logits(q, **aux)
                keep = keep_of(tk, N, dev)
                assert bool((logits[:, ~keep] == NEG_INF).all()) and bool(torch.isfinite(logits[:, keep]).all()), what
                tk.unhide_items(got_pos)
                assert tk.num_hidden == 0 and tk._visible is None and tk.hidden_positions().numel() == 0, what
            again, _ = approx_calls(tk, q, ids, X, aux)
            for name in unhidden:      # unhiding everything restores the original results bit for bit
                U.same(again[name], unhidden[name], f"{kind} {shape} {route}, B = {batch}: {name} after unhiding everything")


@pytest.mark.parametrize("kind", ["avg", "naive", "comb"])
def test_redo_paths_honour_the_hidden_set(kind, dev):
    """All but 2 K' items hidden with the routing rule switched off: the fused scan finds too few finite group maxima, raises its flag, and the
    predicated redo on the device (masked before its selection) answers; with the redo buffer refused, the host reads the verdict and redoes
    the call on the materialising route."""
    g = torch.Generator().manual_seed(42)
    with torch.inference_mode():
        cfg, mol, aux, q = shape_setup("8x8x32", dev, 5)
        make = lambda x, i: MAKERS[kind](mol, x, i)      # noqa: E731
        X, ids = U.table(cfg, N, 7, dev), U.ids_of(N, dev)
        for redo_bytes in (1 << 30, 0):
            tk = routed(make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), FUSED)
            tk.HIDDEN_FUSED_MIN_VISIBLE = 0.0
            if redo_bytes == 0 and kind != "naive":
                tk.DEVICE_REDO_BYTES = 0
            all_but = torch.ones(N, dtype=torch.bool)
            all_but[torch.randperm(N, generator=g)[: 2 * K_PRIME]] = False
            tk.hide_items(torch.nonzero(all_but).reshape(-1))
            assert tk.num_visible == 2 * K_PRIME
            equals_fresh_of_visible(tk, make, X, ids, q, aux, f"{kind}, redo buffer {redo_bytes}", FUSED, dev)


# ---- engine level: the sample scan honours the hidden set ------------------------------------------------------------------------------------
def unit_rows(shape_tuple, seed, dev):
    x = torch.randn(shape_tuple, generator=torch.Generator().manual_seed(seed))
    return (x / x.norm(dim=-1, keepdim=True)).to(dev)


def test_sample_scan_honours_the_hidden_set_coarse(dev):
    """B = 1, 30 011 unit-norm rows, K' = 100: that query's `capacity` best items are hidden.  A sample that ignores the hidden set puts the
    threshold among them, the select scan then finds no visible candidate and the flag goes up."""
    n, kp = 30_011, K_PRIME
    eng = CS.engine("8x8x32")
    spec = eng.spec
    with torch.inference_mode():
        table = unit_rows((n, spec.dot_product_dimension), 1, dev).bfloat16()
        eq = unit_rows((1, spec.query_dot_product_groups, spec.dot_product_dimension), 2, dev)
        cap = E.MolEngine.coarse_topk_capacity(kp, n, 1)
        scores = eng.coarse_scores(eq, table, False)
        best = torch.topk(scores[0], cap).indices
        words, kept = E.visibility_edit(E.visibility_row(n, dev), n, best, False)
        assert kept == n - cap
        mask = E.item_mask_of_words(words, n, kept)
        want = E.topk(E.scores_mask(scores.clone(), mask), kp)
        sc, pos, counts, flag = eng.coarse_topk(eq, table, False, kp, with_flag=True, visible=words)
        assert int(flag.item()) == 0 and kp <= int(counts.min()) and int(counts.max()) <= cap, (int(flag.item()), counts.tolist(), cap)
        U.same((sc, pos), want, "coarse_topk(visible=) against the masked materialised top-K'")
        assert not bool(torch.isin(pos, best).any())
        with pytest.raises(ValueError, match="visible"):
            eng.coarse_topk(eq, table, False, kp, visible=words[:, :-1].contiguous())


def test_sample_scan_honours_the_hidden_set_component(dev):
    """The same for the component entry: row 0's `capacity` best items are hidden (and every row is checked against the masked selection)."""
    n, kg = 30_011, K_PRIME
    eng = CS.engine("8x8x32")
    spec = eng.spec
    with torch.inference_mode():
        table = unit_rows((spec.item_dot_product_groups, n, spec.dot_product_dimension), 3, dev).bfloat16()
        eq = unit_rows((1, spec.query_dot_product_groups, spec.dot_product_dimension), 4, dev)
        cap = eng.component_topk_capacity(1, n, kg)
        scores = eng.component_scores(eq, table)
        best = torch.topk(scores[0], cap).indices
        words, kept = E.visibility_edit(E.visibility_row(n, dev), n, best, False)
        mask = E.item_mask_of_words(words, n, kept)
        want = E.topk(E.scores_mask(scores.clone(), mask), kg)
        flag = torch.ones(1, dtype=torch.int32, device=dev)
        sc, pos, counts = eng.component_topk(eq, table, kg, flag, visible=words)
        assert int(flag.item()) == 0 and kg <= int(counts.min()) and int(counts.max()) <= cap, (int(flag.item()), int(counts.min()), int(counts.max()), cap)
        U.same((sc, pos), want, "component_topk(visible=) against the masked materialised top-k")
        assert not bool(torch.isin(pos, best).any())


@pytest.mark.parametrize("shape", ["8x8x32", "8x4x128"])
def test_visible_scans_answer_without_their_redo(shape, dev):
    """The fused entries themselves at the modules' sizes (N = 4 037; one and two query tiles; the component sample's four- and eight-tile
    blocks): flag 0 -- the redo, which would hide a wrong visible kernel behind a right answer, is not asked for -- counts of VISIBLE candidates
    inside [k, capacity], and the masked materialised selection bit for bit."""
    eng = CS.engine(shape)
    spec = eng.spec
    pq, px, d = spec.query_dot_product_groups, spec.item_dot_product_groups, spec.dot_product_dimension
    g = torch.Generator().manual_seed(47)
    sets = {"random 50 %": torch.randperm(N, generator=g)[: N // 2], "a whole tile and the ragged last one": torch.cat([torch.arange(64, 96), torch.arange(N // 32 * 32, N)]),
            "every fourth item": torch.arange(3, N, 4), "one item": torch.tensor([77])}
    with torch.inference_mode():
        coarse_table = unit_rows((N, d), 5, dev).bfloat16()
        comp_table = unit_rows((px, N, d), 6, dev).bfloat16()
        for name, hide in sets.items():
            words, kept = E.visibility_edit(E.visibility_row(N, dev), N, hide.to(dev), False)
            mask = E.item_mask_of_words(words, N, kept)
            assert kept == N - hide.numel()
            for batch in (2, 33):
                eq = unit_rows((batch, pq, d), 7 + batch, dev)
                for avg in (False, True):
                    want = E.topk(E.scores_mask(eng.coarse_scores(eq, coarse_table, avg), mask), K_PRIME)
                    sc, pos, counts, flag = eng.coarse_topk(eq, coarse_table, avg, K_PRIME, with_flag=True, visible=words)
                    cap = E.MolEngine.coarse_topk_capacity(K_PRIME, N, batch)
                    assert int(flag.item()) == 0 and K_PRIME <= int(counts.min()) and int(counts.max()) <= min(cap, kept), (shape, name, batch, avg, counts.tolist())
                    U.same((sc, pos), want, f"{shape}, {name}, B = {batch}, avg = {avg}: coarse_topk(visible=)")
            for batch in (2, (128 if d >= 128 else 256) // pq):
                eq = unit_rows((batch, pq, d), 9 + batch, dev)
                for kg in (K_GROUP, K_PRIME):
                    want = E.topk(E.scores_mask(eng.component_scores(eq, comp_table), mask), kg)
                    flag = torch.ones(1, dtype=torch.int32, device=dev)
                    sc, pos, counts = eng.component_topk(eq, comp_table, kg, flag, visible=words)
                    cap = eng.component_topk_capacity(batch, N, kg)
                    assert int(flag.item()) == 0 and kg <= int(counts.min()) and int(counts.max()) <= min(cap, kept), (shape, name, batch, kg, int(counts.min()), int(counts.max()))
                    U.same((sc, pos), want, f"{shape}, {name}, B = {batch}, k_g = {kg}: component_topk(visible=)")


def test_item_mask_clear_kernel(dev):
    """rails_item_mask_clear against torch on a ragged row; positions given twice are harmless; the other bits stay."""
    n = 8_192 + 37
    g = torch.Generator().manual_seed(43)
    start = torch.rand(n, generator=g) < 0.7
    m = E.ItemMask(start.to(dev))
    pos = torch.randint(0, n, (3_000,), generator=g)
    words, kept = E.visibility_edit(m.words, n, pos.to(dev), False)
    want = start.clone()
    want[pos] = False
    ref = E.ItemMask(want.to(dev))
    assert torch.equal(words, ref.words) and kept == int(want.sum()) and torch.equal(m.words, E.ItemMask(start.to(dev)).words)
    back, kept2 = E.visibility_edit(words, n, pos.to(dev), True)
    want[pos] = True
    assert torch.equal(back, E.ItemMask(want.to(dev)).words) and kept2 == int(want.sum())


# ---- the int8 pre-filter -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["8x8x32", "8x4x64", "8x4x128"])
def test_int8_prefilter_honours_the_hidden_set(shape, dev):
    g = torch.Generator().manual_seed(44)
    with torch.inference_mode():
        cfg, mol, aux, q = shape_setup(shape, dev, 32)
        X, ids = U.table(cfg, N, 7, dev), U.ids_of(N, dev)
        hide = torch.nonzero(torch.rand(N, generator=g) < 0.5).reshape(-1)
        outs = {}
        for pre in (True, False):
            tk = routed(MAKERS["avg"](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), FUSED)
            tk.PREFILTER_MIN_ITEMS = 0 if pre else 1 << 62
            tk.hide_items(hide)
            outs[pre] = (tk(q, k=K_PRIME, **aux), tk.coarse_candidates(q, **aux))
            assert (tk._coarse_prefilter is not None) == pre
            if pre and cfg.dot_product_dimension <= 64:      # (d = 128 has no visible form of the int8 scan: the bf16 select scan answers)
                assert tk.prefilter_stats()["tested"] > 0
        for a, b in zip(outs[True], outs[False]):
            U.same(a, b, f"{shape}: with the int8 copy against without")
        keep = torch.ones(N, dtype=torch.bool, device=dev)
        keep[hide.to(dev)] = False
        fresh = MAKERS["avg"](mol, X[keep].clone().unsqueeze(0), ids[keep].clone().unsqueeze(0))
        U.same(outs[True][0], fresh(q, k=K_PRIME, **aux), f"{shape}: with the int8 copy against a fresh module")
        # positions are this module's: the visible items keep their order, so they map to the fresh module's through the rank among the visible
        rank = torch.cumsum(keep.to(torch.int64), 0) - 1
        fs, fp = fresh.coarse_candidates(q, **aux)
        U.same((outs[True][1][0], rank[outs[True][1][1]]), (fs, fp), f"{shape}: coarse_candidates")


# ---- the exact modules -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module,route", [("brute", "default"), ("brute", "dense"), ("brute", "f16x3"), ("mips", "mips")])
def test_exact_modules(module, route, dev):
    n = 40_003 if route == "default" else 20_003
    make, X, ids, q, aux = M.setup(module, route, dev, n=n)
    g = torch.Generator().manual_seed(45)
    with torch.inference_mode():
        tk, twin = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        plain = {k: twin(q, k=k, **aux) for k in (10, 200)}
        best = torch.unique(torch.div(plain[10][1][:, 0] - 1, 3, rounding_mode="floor"))       # (ids are 3 * position + 1)
        visible = torch.rand(n, generator=g) < 0.7
        visible[best.cpu()] = False
        other = torch.rand(n, generator=g) < 0.6
        tiny = torch.zeros(n, dtype=torch.bool)
        tiny[torch.randperm(n, generator=g)[:3000]] = True
        tk.hide_items(torch.nonzero(~visible).reshape(-1).to(dev))
        assert tk.num_visible == int(visible.sum())
        keep = visible.to(dev)
        fresh = make(X[keep].clone().unsqueeze(0), ids[keep].clone().unsqueeze(0))
        vis_mask = E.ItemMask(keep)
        for k in (10, 200):
            got = tk(q, k=k, **aux)
            U.same(got, twin(q, k=k, item_mask=vis_mask, **aux), f"{module} {route}: hidden against item_mask=visible on a twin, k = {k}")
            U.same(got, fresh(q, k=k, **aux), f"{module} {route}: hidden against a fresh module, k = {k}")
            assert not bool(torch.isin(got[1], ids[~keep]).any())
        seen = plain[200][1][:, :61].contiguous()
        cand = rails_amd.CandidateIndex(ids=ids.reshape(1, -1), embeddings=X.unsqueeze(0))
        cand_f = rails_amd.CandidateIndex(ids=ids[keep].reshape(1, -1), embeddings=X[keep].unsqueeze(0))
        U.same(cand.get_top_k_outputs(q, 50, aux, tk, seen)[:2], cand_f.get_top_k_outputs(q, 50, aux, fresh, seen)[:2], f"{module} {route}: get_top_k_outputs")
        for name, extra in (("60 %", other), ("3 000 items", tiny)):      # hidden plus item_mask= is the AND of the two (dense and sparse strategies)
            both = E.ItemMask((extra & visible).to(dev))
            mine = E.ItemMask(extra.to(dev))
            for _ in range(2):      # (the second call takes the cached AND)
                U.same(tk(q, k=50, item_mask=mine, **aux), twin(q, k=50, item_mask=both, **aux), f"{module} {route}: hidden AND {name}")
            assert tk._and_mask_cache[0] is mine
        if module == "brute":
            logits = tk.all_logits(q, **aux)
            assert bool((logits[:, ~keep] == NEG_INF).all())
            U.same(logits[:, keep].contiguous(), fresh.all_logits(q, **aux), f"{module} {route}: all_logits")
        with pytest.raises(RuntimeError, match=rf"selected index k out of range \(k={tk.num_visible + 1}, n={tk.num_visible}\)"):
            tk(q, k=tk.num_visible + 1, **aux)
        tk.unhide_items(tk.hidden_positions())
        for k in (10, 200):
            U.same(tk(q, k=k, **aux), plain[k], f"{module} {route}: after unhiding everything, k = {k}")


# ---- edit chains -----------------------------------------------------------------------------------------------------------------------------
def chain_check(tk, make, X, ids, hidden, q, aux, what, dev, mips=False):
    """tk against the reference state (X, ids, hidden bool on the CPU): its hidden set, and its answers against a fresh module of the visible rows."""
    assert tk.num_items == X.shape[0] and tk.num_hidden == int(hidden.sum()), what
    assert torch.equal(tk.hidden_positions().cpu(), torch.nonzero(hidden).reshape(-1)), what
    keep = (~hidden).to(dev)
    fresh = make(X[keep].clone().unsqueeze(0), ids[keep].clone().unsqueeze(0))
    if mips:
        for k in (10, 200):
            U.same(tk(q, k=k), fresh(q, k=k), f"{what}: forward, k = {k}")
        return
    got, seen = approx_calls(tk, q, ids, X, aux)
    want, _ = approx_calls(fresh, q, ids[keep], X[keep], aux, seen=seen)
    for name in want:
        U.same(got[name], want[name], f"{what}: {name}")


@pytest.mark.parametrize("kind", ["avg", "naive", "comb", "brute", "mips"])
def test_edit_chain(kind, dev):
    """hide -> remove_items of other positions -> append_items -> update_items at a hidden position (it stays hidden) -> unhide_items -> compact,
    the module against a fresh module of the visible rows after every step."""
    g = torch.Generator().manual_seed(46)
    n = 4_037
    mips = kind == "mips"
    with torch.inference_mode():
        if mips:
            make, X, ids, q, aux = M.setup("mips", "mips", dev, n=n)
            cfg = O.CONFIGS["amzn-books"]
        else:
            cfg, mol, aux, q = shape_setup("8x8x32", dev, 5)
            make = (lambda x, i: MAKERS[kind](mol, x, i)) if kind != "brute" else (lambda x, i: rails_amd.MoLBruteForceTopK(mol, x, i))      # noqa: E731
            X, ids = U.table(cfg, n, 7, dev), U.ids_of(n, dev)
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        hidden = torch.rand(n, generator=g) < 0.3
        hidden[torch.tensor([0, 31, 32, n - 1, n - 3])] = True      # tail items are hidden: a removal moves hidden movers into holes
        tk.hide_items(torch.nonzero(hidden).reshape(-1))
        chain_check(tk, make, X, ids, hidden, q, aux, f"{kind}: hide", dev, mips)
        # remove other positions (hidden and visible ones, holes and tail)
        gone = R.removal_set(n, g, must=torch.tensor([5, 64, n - 2]))
        X2, ids2, moved = R.after_removal(X, ids, gone)
        h2 = hidden.clone()
        h2[moved[:, 1]] = hidden[moved[:, 0]]
        h2 = h2[: n - gone.numel()]
        U.same(tk.remove_items(gone), moved, f"{kind}: moved")
        chain_check(tk, make, X2, ids2, h2, q, aux, f"{kind}: remove_items", dev, mips)
        # append: the new items are visible
        m = 70
        rows, new_ids = U.table(cfg, m, 99, dev, first=5_000_000), U.ids_of(m, dev, first=1_000_000)
        tk.append_items(rows, new_ids)
        X3, ids3, h3 = torch.cat([X2, rows]), torch.cat([ids2, new_ids]), torch.cat([h2, torch.zeros(m, dtype=torch.bool)])
        chain_check(tk, make, X3, ids3, h3, q, aux, f"{kind}: append_items", dev, mips)
        # update at a hidden and at a visible position: visibility belongs to the position
        at = torch.tensor([int(torch.nonzero(h3)[3]), int(torch.nonzero(~h3)[3])])
        rows = U.table(cfg, 2, 100, dev, first=6_000_000)
        tk.update_items(at, rows)
        X4 = X3.clone()
        X4[at.to(dev)] = rows
        chain_check(tk, make, X4, ids3, h3, q, aux, f"{kind}: update_items", dev, mips)
        # unhide half of the hidden items, by id
        back = torch.nonzero(h3).reshape(-1)[::2]
        tk.unhide_items_by_id(ids3[back.to(dev)])
        h4 = h3.clone()
        h4[back] = False
        chain_check(tk, make, X4, ids3, h4, q, aux, f"{kind}: unhide_items_by_id", dev, mips)
        # compact == remove_items(hidden_positions()) on a twin: every held buffer bit for bit
        twin = make(X4.clone().unsqueeze(0), ids3.clone().unsqueeze(0))
        if not mips:
            approx_calls(twin, q, ids3, X4, aux)      # (every lazily built buffer exists on both)
        hp = tk.hidden_positions()
        U.same(tk.compact(), twin.remove_items(hp), f"{kind}: compact's moved")
        assert tk.num_hidden == 0 and tk._visible is None and tk.hidden_positions().numel() == 0
        if mips:
            U.same((tk._index.buf, tk._ids_flat), (twin._index.buf, twin._ids_flat), "mips: buffers after compact")
        else:
            hg, hw = U.held(tk), U.held(twin)
            assert set(hg) == set(hw)
            for name in hw:
                U.same(hg[name], hw[name], f"{kind}: buffer {name} after compact")
        X5, ids5, _ = R.after_removal(X4, ids3, hp.cpu())
        chain_check(tk, make, X5, ids5, torch.zeros(X5.shape[0], dtype=torch.bool), q, aux, f"{kind}: compact", dev, mips)


def test_hide_between_submit_and_result(dev):
    """A handle outstanding from submit() keeps the corpus it was submitted against."""
    with torch.inference_mode():
        cfg, mol, aux, q = shape_setup("8x8x32", dev, 5)
        X, ids = U.table(cfg, N, 7, dev), U.ids_of(N, dev)
        tk = routed(MAKERS["avg"](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), FUSED)
        tk.DEVICE_REDO_BYTES = 0      # speculative handles on the module's side streams
        want = tk(q, k=10, **aux)
        h = tk.submit(q, 10, **aux)
        tk.hide_items_by_id(torch.unique(want[1]))
        U.same(tk.result(h), want, "submitted before hide_items")
        assert not bool(torch.isin(tk(q, k=10, **aux)[1], torch.unique(want[1])).any())


# ---- validation and refusals -----------------------------------------------------------------------------------------------------------------
def test_validation_and_refusals(dev):
    with torch.inference_mode():
        cfg, mol, aux, q = shape_setup("8x8x32", dev, 5)
        n = 2_000
        X, ids = U.table(cfg, n, 7, dev), U.ids_of(n, dev)
        mods = {k: MAKERS[k](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0)) for k in MAKERS}
        mods["brute"] = rails_amd.MoLBruteForceTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        mods["mips"] = rails_amd.MIPSBruteForceTopK(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        for name, tk in mods.items():
            for bad in (torch.tensor([0, n]), torch.tensor([-1]), torch.tensor([3, 3]), torch.tensor([1, 2], dtype=torch.int32), torch.tensor([[1, 2]]), [1, 2]):
                for fn in (tk.hide_items, tk.unhide_items):
                    with pytest.raises(ValueError):
                        fn(bad)
            for fn in (tk.hide_items_by_id, tk.unhide_items_by_id):
                with pytest.raises(ValueError, match="not in the corpus"):
                    fn(torch.tensor([2, 5], device=dev))           # (ids are 3 * position + 1)
                with pytest.raises(ValueError, match="repeat"):
                    fn(torch.tensor([4, 4], device=dev))
            with pytest.raises(ValueError, match="none of the"):
                tk.hide_items(torch.arange(n))
            assert tk.num_hidden == 0 and tk.num_visible == n and tk._visible is None, name
            tk.hide_items(torch.empty(0, dtype=torch.int64))       # M = 0 is a no-op
            tk.unhide_items(torch.tensor([1, 2]))                   # nothing is hidden: nothing to do
            assert tk._visible is None and tk.compact().shape == (0, 2)
            tk.hide_items(torch.arange(0, n - 50, device=dev))
            tk.hide_items(torch.arange(0, 10))                      # hiding a hidden item again is allowed
            assert (tk.num_hidden, tk.num_visible) == (n - 50, 50), name
            with pytest.raises(ValueError, match="none of the"):
                tk.hide_items(torch.arange(n - 50, n))
            assert tk.num_visible == 50
        # k, avg_top_k, k_per_group beyond num_visible: what a fresh module of that size raises
        for name, k in (("avg", K_PRIME), ("comb", K_PRIME)):
            with pytest.raises(RuntimeError, match=rf"selected index k out of range \(k={k}, n=50\)"):
                mods[name](q, k=10, **aux)
        for name in ("brute", "mips"):
            with pytest.raises(RuntimeError, match=r"selected index k out of range \(k=51, n=50\)"):
                mods[name](q, k=51, **({} if name == "mips" else aux))
        mods["naive"].unhide_items(torch.arange(0, n - 50))
        mods["naive"].hide_items(torch.arange(0, n - 4))
        with pytest.raises(RuntimeError, match=rf"selected index k out of range \(k={K_GROUP}, n=4\)"):
            mods["naive"](q, k=10, **aux)
        # item_mask= on the approximate modules stays refused, hidden set or not
        mask = E.ItemMask(torch.ones(n, dtype=torch.bool, device=dev))
        for name in ("avg", "naive", "comb"):
            with pytest.raises(NotImplementedError, match="item_mask"):
                mods[name](q, k=10, item_mask=mask, **aux)
        # the IVF module, with and without frozen centroids
        for frozen in (False, True):
            ivf = rails_amd.MoLNaiveTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0), k_per_group=5, use_faiss=True, frozen_centroids=frozen)
            for call in (lambda: ivf.hide_items(torch.tensor([1])), lambda: ivf.unhide_items(torch.tensor([1])), lambda: ivf.hide_items_by_id(ids[:1]),
                         lambda: ivf.unhide_items_by_id(ids[:1]), ivf.hidden_positions, ivf.compact):
                with pytest.raises(NotImplementedError, match="MoLNaiveTopK.*IVF"):
                    call()
            assert ivf._visible is None and ivf._ivf is None       # nothing was touched, nothing built
        # the sharded wrappers refuse by name (their methods raise before anything is looked at)
        from rails_amd import sharded

        for cls in (sharded.ShardedMoLBruteForceTopK, sharded.ShardedMoLAvgTopK, sharded.ShardedMoLNaiveTopK, sharded.ShardedMoLCombTopK):
            w = cls.__new__(cls)
            for call in (lambda: w.hide_items(torch.tensor([1])), lambda: w.unhide_items(torch.tensor([1])), lambda: w.hide_items_by_id(ids[:1]),
                         lambda: w.unhide_items_by_id(ids[:1]), w.hidden_positions, w.compact):
                with pytest.raises(NotImplementedError, match=cls.__name__):
                    call()
