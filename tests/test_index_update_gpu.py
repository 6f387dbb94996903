"""GPU: MoLTopKModule.update_items / append_items.  The oracle is a module FRESHLY CONSTRUCTED from the resulting
table, ids and the same mol_module: every held derived buffer torch.equal, and forward / get_top_k_outputs / submit-result / all_logits
torch.equal, on every route and precision the modules support.  Inputs: the synthetic weights, hashed item tables and queries of
oracle.mol_oracle at the C3 (amzn-books) and C4 (16x16x64) shapes, and one generic-route shape of tests/golden/generic_shapes.npz."""
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from tests._generic_fixtures import generic_cases
from tests.test_generic_route_gpu import build_module

pytestmark = pytest.mark.gpu
B = 32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def table(cfg, n, seed, dev, first=0):
    return torch.from_numpy(O.hash_item_table(seed, first, n, cfg.item_embedding_dim)).to(dev)


def ids_of(n, dev, first=0, mul=3):
    return torch.arange(first, first + n, dtype=torch.int64, device=dev) * mul + 1


MAKERS = {
    "brute": lambda mol, x, i, **kw: rails_amd.MoLBruteForceTopK(mol, x, i, **kw),
    "avg": lambda mol, x, i: rails_amd.MoLAvgTopK(mol, x, i, avg_top_k=500),
    "naive": lambda mol, x, i: rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=5),
    "comb": lambda mol, x, i: rails_amd.MoLCombTopK(mol, x, i, avg_top_k=200, k_per_group=5),
}


def held(tk):
    """Every derived buffer the module holds right now, by name."""
    out = {"index": tk._index.buf, "ids": tk._ids_flat, "table": tk._item_embeddings, "item_ids": tk._item_ids.reshape(-1)}
    c = tk._rows_cache
    if c is not None and c[2] is not None:
        out["rows"] = c[2]
    for name in ("_coarse_table", "_comp_table", "_rows32"):
        t = getattr(tk, name, None)
        if t is not None:
            out[name] = t
    pre = getattr(tk, "_coarse_prefilter", None)
    if pre is not None:      # (bytes 32..47 of the header are running statistics of the calls made)
        out["prefilter_head"], out["prefilter_body"] = pre[:32], pre[48:]
    if getattr(tk, "_index32", None) is not None:
        out["index32"] = tk._index32.buf
    return out


def same(a, b, what):
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for j, (x, y) in enumerate(zip(a, b)):
        if x is None and y is None:
            continue
        assert x.shape == y.shape and x.dtype == y.dtype, (what, j, x.shape, y.shape)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (what, j)


def calls(tk, q, ids, X, aux, ks=(10, 200)):
    """The calls of the contract, in one fixed order -> their outputs."""
    out = {}
    for k in ks:
        out[f"forward{k}"] = tk(q, k=k, **aux)
    seen = out[f"forward{ks[-1]}"][1][:, :61].contiguous()
    cand = rails_amd.CandidateIndex(ids=ids.reshape(1, -1), embeddings=X.reshape(1, *X.shape[-2:]))
    out["filtered"] = cand.get_top_k_outputs(q, 50, aux, tk, seen)[:2]
    out["plain"] = cand.get_top_k_outputs(q, 50, aux, tk, None)[:2]
    out["all_logits"] = tk.all_logits(q, **aux)
    if isinstance(tk, rails_amd.MoLAvgTopK) and not isinstance(tk, rails_amd.MoLCombTopK):
        h1, h2 = tk.submit(q, ks[0], **aux), tk.submit(q, ks[-1], **aux)
        out["submit_a"], out["submit_b"] = tk.result(h1), tk.result(h2)
    return out


def equals_fresh(tk, make, X, ids, q, aux, what, ks=(10, 200)):
    """tk, which went through updates, against a module freshly built from the table X (N, D) and ids (N,) -- the same calls on both."""
    fresh = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
    assert tk.num_items == X.shape[0] == fresh.num_items
    got, want = calls(tk, q, ids, X, aux, ks), calls(fresh, q, ids, X, aux, ks)
    for name in want:
        same(got[name], want[name], f"{what}: {name}")
    hg, hw = held(tk), held(fresh)
    assert set(hg) == set(hw), (what, sorted(hg), sorted(hw))
    for name in hw:
        same(hg[name], hw[name], f"{what}: buffer {name}")
    assert type(tk._bind()) is type(fresh._bind()) and tk._bind().precision == fresh._bind().precision and (tk._bind().exact is None) == (fresh._bind().exact is None), what
    return got


def positions_for(n, g, extra=200):
    """0, N - 1, both ends of a tile boundary and a random set, shuffled"""
    fixed = torch.tensor([0, n - 1, 31, 32, (n - 1) // 32 * 32 - 1, (n - 1) // 32 * 32])
    p = torch.unique(torch.cat([fixed, torch.randint(0, n, (extra,), generator=g)]))
    p = p[torch.randperm(p.numel(), generator=g)]
    front = torch.tensor([0, n - 1, 31, 32])          # (the rows planted below go to these)
    return torch.cat([front, p[~torch.isin(p, front)]])


def new_rows(cfg, X, pos, best_pos, seed, dev):
    """Fresh hashed rows for `pos`; the first few are copies of the rows of some queries' best items, so that the updated positions enter results."""
    rows = table(cfg, pos.numel(), seed, dev, first=10_000_000)
    take = min(4, best_pos.numel())
    rows[:take] = X[best_pos[:take]]
    return rows


def route_cases():
    out = []
    for route in ("default", "dense", "f16x3", "c4", "generic"):
        out.append(("brute", route))
    for m in ("avg", "naive", "comb"):
        for route in ("default", "f16x3", "c4"):
            out.append((m, route))
    return out


def setup_route(module, route, dev):
    """-> (cfg, mol, make(x, i), aux)"""
    aux = {}
    if route == "generic":
        name, cfg, w, a = next(c for c in generic_cases() if c[0] == "g_8x8x40")
        mol = build_module(cfg, w, dev)
        assert mol.engine().route == "generic"
        if "user_ids" in a:
            aux = {"user_ids": (torch.arange(B, dtype=torch.int64) * 7919 - 5).to(dev)}
    else:
        cfg = O.CONFIGS["synthetic-16x16x64" if route == "c4" else "amzn-books"]
        mol = build_module(cfg, O.synthetic_weights(cfg, seed=1), dev, precision="f16x3" if route == "f16x3" else None)
    kw = {"exact_mode": "dense"} if route == "dense" else {}
    return cfg, mol, (lambda x, i: MAKERS[module](mol, x, i, **kw)), aux


@pytest.mark.parametrize("module,route", route_cases())
def test_update_equals_a_fresh_module(module, route, dev):
    cfg, mol, make, aux = setup_route(module, route, dev)
    n = 70_001
    g = torch.Generator().manual_seed(11)
    with torch.inference_mode():
        X, ids = table(cfg, n, 7, dev), ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=5).to(dev)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        before = calls(tk, q, ids, X, aux)             # every lazily built buffer exists now
        eng = tk._bind()
        if module == "brute" and route in ("default", "c4"):
            assert eng.exact is not None and tk._index32 is not None, "the proved mode is what this case is about"
            if route == "c4":
                assert tk._policy.poly is not None      # per-pair upper bounds
        pos = positions_for(n, g)
        best = (before["forward10"][1][:, 0] - 1) // 3
        rows = new_rows(cfg, X, pos, best, 21, dev)
        new_ids = ids[pos.to(dev)] + 1_000_000_007
        want_X, want_ids = X.clone(), ids.clone()
        want_X[pos.to(dev)], want_ids[pos.to(dev)] = rows, new_ids
        tk.update_items(pos, rows, new_ids)             # CPU positions
        assert torch.equal(X, want_X) and torch.equal(ids, want_ids), "the borrowed table and ids are written in place"
        after = equals_fresh(tk, make, want_X, want_ids, q, aux, f"{module} {route}")
        assert not (torch.equal(before["forward10"][1], after["forward10"][1]) and torch.equal(before["forward10"][0], after["forward10"][0])), \
            "the update changed nothing"
        assert bool((after["forward10"][1] > 1_000_000_000).any()), "no updated item reached a result"
        # a second update: device positions, (1, M, D) rows, no ids
        pos2 = torch.unique(torch.cat([pos[:50], torch.tensor([n - 2, 33])])).to(dev)
        rows2 = table(cfg, pos2.numel(), 22, dev, first=20_000_000).unsqueeze(0)
        want_X[pos2] = rows2[0]
        tk.update_items(pos2, rows2)
        equals_fresh(tk, make, want_X, want_ids, q, aux, f"{module} {route} second update")


@pytest.mark.parametrize("module", ["avg", "comb"])
def test_update_with_the_fused_scans(module, dev):
    """N = 300 007 puts the fused coarse and component scans in play (fused_coarse_min_items = 262 144); MoLAvgTopK500 / MoLCombTopK5_200."""
    cfg, mol, make, aux = setup_route(module, "default", dev)
    n = 300_007
    g = torch.Generator().manual_seed(12)
    with torch.inference_mode():
        X, ids = table(cfg, n, 8, dev), ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=6).to(dev)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        assert n >= tk.fused_coarse_min_items
        before = calls(tk, q, ids, X, aux)
        pos = positions_for(n, g, extra=1000)
        rows = new_rows(cfg, X, pos, (before["forward10"][1][:, 0] - 1) // 3, 23, dev)
        new_ids = ids[pos.to(dev)] + 1_000_000_007
        tk.update_items(pos.to(dev), rows, new_ids)
        after = equals_fresh(tk, make, X, ids, q, aux, f"{module} fused")
        assert not torch.equal(before["forward10"][1], after["forward10"][1])


@pytest.mark.parametrize("module", ["brute", "avg", "naive", "comb"])
def test_append_equals_a_fresh_module(module, dev):
    cfg, mol, make, aux = setup_route(module, "default", dev)
    n = 70_001
    with torch.inference_mode():
        full, full_ids = table(cfg, n + 95 + 4000, 9, dev), ids_of(n + 95 + 4000, dev)
        q = O.synthetic_queries(cfg, B, seed=7).to(dev)
        X0, ids0 = full[:n].clone(), full_ids[:n].clone()
        tk = make(X0.unsqueeze(0), ids0.unsqueeze(0))
        before = calls(tk, q, ids0, X0, aux)
        lo = n
        for m in (95, 4000):          # a partially filled last tile and a new one, then many tiles
            tk.append_items(full[lo : lo + m], full_ids[lo : lo + m].unsqueeze(0))
            lo += m
            after = equals_fresh(tk, make, full[:lo], full_ids[:lo], q, aux, f"{module} append to {lo}")
        assert X0.shape[0] == n and torch.equal(X0, full[:n]), "after append_items the module owns its table: the caller's is left alone"
        assert after["all_logits"].shape[1] == n + 4095 and before["all_logits"].shape[1] == n


def test_append_across_the_proved_rule(dev):
    """16 000 -> 17 000 items crosses the 16 384-item rule of the default exact mode: dense before, proved after, as a fresh module of each size."""
    cfg, mol, make, aux = setup_route("brute", "default", dev)
    with torch.inference_mode():
        full, full_ids = table(cfg, 17_000, 10, dev), ids_of(17_000, dev)
        q = O.synthetic_queries(cfg, B, seed=8).to(dev)
        tk = make(full[:16_000].clone().unsqueeze(0), full_ids[:16_000].clone().unsqueeze(0))
        equals_fresh(tk, make, full[:16_000], full_ids[:16_000], q, aux, "16 000 items")
        assert tk._bind().exact is None
        tk.append_items(full[16_000:], full_ids[16_000:])
        assert tk._bind().exact is not None and tk._index32 is not None
        equals_fresh(tk, make, full, full_ids, q, aux, "17 000 items")
        st = tk.stats()
        assert st["proved_calls"] + st["fallbacks"] == st["calls"] > 0, st


@pytest.mark.parametrize("module", ["brute", "comb"])
def test_chains_of_updates_and_appends(module, dev):
    cfg, mol, make, aux = setup_route(module, "default", dev)
    n = 40_011
    g = torch.Generator().manual_seed(13)
    with torch.inference_mode():
        X, ids = table(cfg, n, 14, dev), ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=9).to(dev)
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        calls(tk, q, ids, X, aux)
        p1 = positions_for(n, g)
        r1 = table(cfg, p1.numel(), 31, dev, first=30_000_000)
        tk.update_items(p1, r1)
        X[p1.to(dev)] = r1
        extra, extra_ids = table(cfg, 777, 32, dev, first=40_000_000), ids_of(777, dev, first=5_000_000)
        tk.append_items(extra, extra_ids)
        X, ids = torch.cat([X, extra]), torch.cat([ids, extra_ids])
        p2 = torch.cat([p1[:40], torch.tensor([n - 1, n, n + 776, n + 31, n + 32])])       # overlaps the first update and the appended range
        p2 = torch.unique(p2)
        r2 = table(cfg, p2.numel(), 33, dev, first=50_000_000)
        i2 = ids[p2.to(dev)] + 2_000_000_011
        tk.update_items(p2, r2, i2)
        X[p2.to(dev)], ids[p2.to(dev)] = r2, i2
        p3 = torch.tensor([5, n + 5])                    # an update of ids only: the rows as they are
        tk.update_items(p3, X[p3.to(dev)].clone(), torch.tensor([-7, -8], device=dev))
        ids[p3.to(dev)] = torch.tensor([-7, -8], device=dev)
        equals_fresh(tk, make, X, ids, q, aux, f"{module} chain")


@pytest.mark.parametrize("module", ["brute", "avg", "comb"])
def test_update_before_the_first_call_and_between_calls(module, dev):
    cfg, mol, make, aux = setup_route(module, "default", dev)
    n = 70_001
    g = torch.Generator().manual_seed(14)
    with torch.inference_mode():
        X, ids = table(cfg, n, 15, dev), ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=10).to(dev)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        if module != "brute":
            assert tk._coarse_table is None and tk._rows_cache is None       # nothing lazily built yet
        p = positions_for(n, g)
        r = table(cfg, p.numel(), 41, dev, first=60_000_000)
        tk.update_items(p, r)
        if module != "brute":
            assert tk._coarse_table is None and tk._rows_cache is None, "a buffer that was not built stays unbuilt"
        equals_fresh(tk, make, X, ids, q, aux, f"{module} update before the first call")
        tk(q, k=10, **aux)
        p = positions_for(n, g)
        r = table(cfg, p.numel(), 42, dev, first=70_000_000)
        tk.update_items(p, r)
        equals_fresh(tk, make, X, ids, q, aux, f"{module} update between calls")


SMALL_MAKERS = {      # (the MAKERS' candidate counts exceed a corpus of 61 items)
    "brute": lambda mol, x, i: rails_amd.MoLBruteForceTopK(mol, x, i),
    "comb": lambda mol, x, i: rails_amd.MoLCombTopK(mol, x, i, avg_top_k=16, k_per_group=1),
    "mips": lambda mol, x, i: rails_amd.MIPSBruteForceTopK(x, i),
}


@pytest.mark.parametrize("module", ["brute", "comb", "mips"])
def test_the_three_calls_and_a_by_id_call_interleaved(module, dev):
    """One module through append_items, remove_items, upsert_items and update_items in a row -- one code path for all of them -- at sizes
    where every tile count changes: 70 items (two full tiles and a ragged one) -> 101 -> 61 (the removal takes tail positions and cuts a tile
    boundary) -> 67 (half of the upserted ids present, half absent; the id map is live from here on) -> the last tile updated, ids included.
    Every derived buffer is built before the first edit (the first comparison makes every call); a fresh module after each step."""
    from tests import test_index_remove_gpu as R      # (imports this module: not at the top)

    cfg, mol, _, aux = setup_route("brute", "default", dev)
    make = lambda x, i: SMALL_MAKERS[module](mol, x, i)      # noqa: E731
    with torch.inference_mode():
        if module == "mips":
            q = (torch.randn(B, cfg.item_embedding_dim, generator=torch.Generator().manual_seed(15)) * 0.05).to(dev)
            check = lambda what: R.mips_equals_fresh(tk, X, ids, q, what, ks=(5, 10))      # noqa: E731
        else:
            q = O.synthetic_queries(cfg, B, seed=15).to(dev)
            check = lambda what: equals_fresh(tk, make, X, ids, q, aux, f"{module}: {what}", ks=(5, 10))      # noqa: E731
        X, ids = table(cfg, 70, 61, dev), ids_of(70, dev)
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        check("70 items as built")
        if module == "comb":
            assert tk._coarse_table is not None and tk._comp_table is not None and tk._rows_cache[2] is not None
        e, ei = table(cfg, 31, 62, dev, first=1_000), ids_of(31, dev, first=70)
        tk.append_items(e, ei)
        X, ids = torch.cat([X, e]), torch.cat([ids, ei])
        check("appended to 101")
        pos = torch.cat([torch.arange(92, 101), torch.arange(0, 62, 2)])      # the last nine and every other one of the rest: 40
        X, ids, moved = R.after_removal(X, ids, pos)
        assert torch.equal(tk.remove_items(pos), moved) and X.shape[0] == 61
        check("removed to 61")
        at = torch.tensor([3, 60, 31, 32, 0, 17], device=dev)
        absent = ids_of(6, dev, first=5_000)
        rows = table(cfg, 12, 63, dev, first=2_000)
        tk.upsert_items(torch.stack([ids[at], absent], dim=1).reshape(-1), rows)      # present and absent ids alternate
        X[at] = rows[0::2]
        X, ids = torch.cat([X, rows[1::2]]), torch.cat([ids, absent])
        check("upserted to 67")
        p, r, i = torch.tensor([66, 64, 65], device=dev), table(cfg, 3, 64, dev, first=3_000), ids_of(3, dev, first=9_000)
        tk.update_items(p, r, i)
        X[p], ids[p] = r, i
        check("last tile updated")
        assert torch.equal(tk.positions_of(ids), torch.arange(67, device=dev)), "the id map followed every call since the upsert"


def test_append_over_the_engine_threshold_holds_what_a_fresh_module_holds(dev):
    """16 380 + 8 items cross the 16 384-item rule of the default exact mode: append_items looks first, drops what it held under the dense
    engine and builds the proved one's buffers from the table -- the set of held buffers and their bits are a fresh module's."""
    cfg, mol, make, aux = setup_route("brute", "default", dev)
    with torch.inference_mode():
        full, full_ids = table(cfg, 16_388, 18, dev), ids_of(16_388, dev)
        q = O.synthetic_queries(cfg, B, seed=16).to(dev)
        tk = make(full[:16_380].clone().unsqueeze(0), full_ids[:16_380].clone().unsqueeze(0))
        calls(tk, q, full_ids[:16_380], full[:16_380], aux)
        assert tk._bind().exact is None and tk._index32 is None
        tk.append_items(full[16_380:], full_ids[16_380:])
        assert tk._bind().exact is not None and tk._index32 is not None
        equals_fresh(tk, make, full, full_ids, q, aux, "16 388 items")


def test_refusals_and_validation(dev):
    cfg, mol, make, aux = setup_route("brute", "default", dev)
    n, D = 20_000, cfg.item_embedding_dim
    with torch.inference_mode():
        X, ids = table(cfg, n, 16, dev), ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=11).to(dev)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        want = tk(q, k=10)
        snap = {k: v.clone() for k, v in held(tk).items()}
        rows = table(cfg, 3, 43, dev)
        for bad_pos in (torch.tensor([1, 2, 1]), torch.tensor([1, 2, n]), torch.tensor([-1, 2, 3]), torch.tensor([1, 2]), torch.tensor([1, 2, 3], dtype=torch.int32),
                        torch.tensor([1, 2, 1], device=dev)):
            with pytest.raises(ValueError):
                tk.update_items(bad_pos, rows)
        with pytest.raises(ValueError):
            tk.update_items(torch.tensor([1, 2, 3]), rows[:, : D - 1].contiguous())                # wrong D
        with pytest.raises(ValueError):
            tk.update_items(torch.tensor([1, 2, 3]), rows.double())
        with pytest.raises(ValueError):
            tk.update_items(torch.tensor([1, 2, 3]), rows, torch.tensor([1, 2], device=dev))        # ids of another length
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tk.update_items(torch.tensor([1, 2, 3]), rows.cpu())
        with pytest.raises(ValueError):
            tk.append_items(rows[:, : D - 1].contiguous(), torch.tensor([1, 2, 3], device=dev))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tk.append_items(rows.cpu(), torch.tensor([1, 2, 3]))
        tk.update_items(torch.empty(0, dtype=torch.int64), rows[:0])                                # M = 0: a no-op
        tk.append_items(rows[:0], ids[:0])
        for k, v in held(tk).items():
            same(v, snap[k], f"nothing is modified by a refused call: {k}")
        same(tk(q, k=10), want, "after the refused calls")
        # the IVF module: trained on the corpus, refuses and stays as it was
        ivf = rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), k_per_group=5, use_faiss=True)
        first = ivf(q, k=10)
        with pytest.raises(NotImplementedError, match="IVF"):
            ivf.update_items(torch.tensor([1, 2, 3]), rows)
        with pytest.raises(NotImplementedError, match="IVF"):
            ivf.append_items(rows, torch.tensor([1, 2, 3], device=dev))
        same(ivf(q, k=10), first, "the IVF module after the refusals")
        assert ivf.num_items == n and torch.equal(X, snap["table"][0])


@pytest.mark.parametrize("config", ["amzn-books", "synthetic-16x16x64"])       # 8x8x32 and 16x16x64: P_X and d both differ
def test_derived_tables_build_at_an_offset_and_update_equal_the_build(config, dev):
    """The engine and C entry points of the derived buffers directly, N = 70 (two full tiles and a ragged one of 6), fp32 engine: the build
    into a table at an offset -- _derived_table's chunked arm, which the modules only reach from 2^20 items on -- and the update from both
    forms of update_source, against the one-call build, bit for bit."""
    cfg = O.CONFIGS[config]
    n, px, d = 70, cfg.item_dot_product_groups, cfg.dot_product_dimension
    bits = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    eng = build_module(cfg, O.synthetic_weights(cfg, seed=1), dev, precision="fp32").engine()
    assert eng.precision == "fp32" and eng.route != "generic"
    with torch.inference_mode():
        X = table(cfg, n, 17, dev)
        index, head, tail = eng.build_index(X), eng.build_index(X[:64]), eng.build_index(X[64:])
        shape, lib = E.C.byref(eng.shape), eng.lib
        # (a) one call against two calls into one table, the second at item 64
        coarse, comp = eng.build_coarse_table(index), eng.build_component_table(index)
        coarse2 = torch.full((n, d), -1, dtype=torch.int16, device=dev).view(torch.bfloat16)
        comp2 = torch.full((px, n, d), -1, dtype=torch.int16, device=dev).view(torch.bfloat16)
        with E._on_device(dev):
            for part, m, first in ((head, 64, 0), (tail, 6, 64)):
                E._lib.check(lib.rails_mol_component_build(shape, E._ptr(part.buf), m, E._ptr(comp2), n, first, E._stream()), "rails_mol_component_build")
                E._lib.check(lib.rails_mol_coarse_build(shape, E._ptr(part.buf), m, E.C.c_void_p(coarse2.data_ptr() + 2 * first * d), E._stream()),
                             "rails_mol_coarse_build")
        assert torch.equal(bits(comp2), bits(comp)), "component table built in two parts"
        assert torch.equal(bits(coarse2), bits(coarse)), "coarse table built in two parts"
        # (b), (c) every row updated in a fixed shuffled order, from the index in place and from a temporary index of the rows in that order
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).to(dev)
        for what, source in (("in place", (index.buf, 1)), ("temporary index", (eng.build_index(X[perm]).buf, 0))):
            coarse3, comp3 = torch.full_like(bits(coarse), -1).view(torch.bfloat16), torch.full_like(bits(comp), -1).view(torch.bfloat16)
            eng.update_coarse_table(coarse3, perm, source)
            eng.update_component_table(comp3, perm, source)
            assert torch.equal(bits(coarse3), bits(coarse)), f"coarse table updated from the source {what}"
            assert torch.equal(bits(comp3), bits(comp)), f"component table updated from the source {what}"
        # (d) the row-major copy
        rows = eng.build_index_rows(index)
        rows2 = torch.full_like(bits(rows), -1).view(torch.float32)
        eng.update_index_rows(index, rows2, perm)
        assert torch.equal(bits(rows2), bits(rows)), "row-major copy updated at every position"
