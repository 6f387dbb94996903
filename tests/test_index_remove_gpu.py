"""GPU: remove_items on the MoL top-k modules and the in-place corpus API of MIPSBruteForceTopK.  The oracle is, as in
tests/test_index_update_gpu.py (whose helpers are used through the module, U), a module FRESHLY CONSTRUCTED from the resulting table, the resulting
ids and the same mol_module: every held derived buffer torch.equal -- shape, dtype and the padding slots of the last tile included -- and forward /
get_top_k_outputs / submit-result / all_logits torch.equal.  The resulting table is the one rails_amd.topk_modules.removal_plan predicts.

70 001 = 2 187 x 32 + 17: the last tile of that corpus holds 17 items.  The tile-boundary test therefore runs its 1 / 32 / 33 removals from 70 001
items AND from 70 017 = 2 188 x 32 + 1, where they leave the last tile full, full again one tile lower, then part-filled with 31 items."""
import pytest
import torch

import rails_amd
import tests.test_index_update_gpu as U
from oracle import mol_oracle as O
from rails_amd import _lib
from rails_amd import engine as E
from rails_amd.topk_modules import removal_plan

pytestmark = pytest.mark.gpu
B = U.B


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def after_removal(X, ids, pos):
    """The table (N', D) and ids (N',) removal_plan predicts for removing `pos` from X (N, D), ids (N,) -> (X', ids', moved)."""
    n = X.shape[0]
    holes, movers = removal_plan(pos.cpu(), n)
    n_new = n - pos.numel()
    X2, ids2 = X[:n_new].clone(), ids[:n_new].clone()
    X2[holes.to(X.device)], ids2[holes.to(X.device)] = X[movers.to(X.device)], ids[movers.to(X.device)]
    return X2, ids2, torch.stack([movers, holes], dim=1)


def removal_set(n, g, must=(), extra=200):
    """0, 31, 32, N - 1, N - 2 (the tail itself is partly removed), `must` and a random set; shuffled."""
    fixed = torch.tensor([0, 31, 32, n - 1, n - 2])
    p = torch.unique(torch.cat([fixed, torch.as_tensor(must, dtype=torch.int64).reshape(-1).cpu(), torch.randint(0, n, (extra,), generator=g)]))
    return p[torch.randperm(p.numel(), generator=g)]


def result_ids(out):
    """Every id a contract call returned."""
    got = [v[1] for k, v in out.items() if k.startswith("forward") or k.startswith("submit")]
    got += [out["filtered"][0], out["plain"][0]]
    return torch.cat([t.reshape(-1) for t in got])


@pytest.mark.parametrize("module,route", U.route_cases())
def test_remove_equals_a_fresh_module(module, route, dev):
    cfg, mol, make, aux = U.setup_route(module, route, dev)
    n = 70_001
    g = torch.Generator().manual_seed(31)
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 7, dev), U.ids_of(n, dev)
        X0, ids0 = X.clone(), ids.clone()
        q = O.synthetic_queries(cfg, B, seed=5).to(dev)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        before = U.calls(tk, q, ids, X, aux)               # every lazily built buffer exists now
        if module == "brute" and route in ("default", "c4"):
            assert tk._bind().exact is not None and tk._index32 is not None, "the proved mode is what this case is about"
        best = (before["forward10"][1][:4, 0] - 1) // 3    # positions of four queries' best items: removed items were in the results
        pos = removal_set(n, g, must=best)
        assert n - 2 in pos.tolist() and n - 1 in pos.tolist()
        gone = ids[pos.to(dev)]
        assert bool(torch.isin(before["forward10"][1], gone).any())
        want_X, want_ids, want_moved = after_removal(X, ids, pos)
        moved = tk.remove_items(pos)                       # CPU positions
        assert moved.dtype == torch.int64 and not moved.is_cuda and torch.equal(moved, want_moved), "moved is the plan"
        assert n - 2 not in moved[:, 0].tolist(), "a removed tail position is no mover"
        assert torch.equal(X, X0) and torch.equal(ids, ids0), "the caller's tensors are not written"
        after = U.equals_fresh(tk, make, want_X, want_ids, q, aux, f"{module} {route}")
        assert not bool(torch.isin(result_ids(after), gone).any()), "a removed id came back"
        assert after["all_logits"].shape[1] == n - pos.numel()
        # a second removal: device positions, the module's own table by now
        pos2 = removal_set(want_X.shape[0], g, extra=50).to(dev)
        want_X2, want_ids2, want_moved2 = after_removal(want_X, want_ids, pos2)
        assert torch.equal(tk.remove_items(pos2), want_moved2)
        U.equals_fresh(tk, make, want_X2, want_ids2, q, aux, f"{module} {route} second removal")


@pytest.mark.parametrize("n", [70_001, 70_017])
@pytest.mark.parametrize("module,route", [("brute", "default"), ("brute", "generic"), ("comb", "default")])
def test_remove_to_and_across_a_tile_boundary(module, route, n, dev):
    """1, 32 and 33 items in turn.  From 70 017 items the last tile is then full, full again one tile lower, and part-filled with 31 items: the padding
    slots and index_floats must follow (U.same compares shapes, so a buffer of the wrong size fails too)."""
    cfg, mol, make, aux = U.setup_route(module, route, dev)
    g = torch.Generator().manual_seed(32)
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 8, dev), U.ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=6).to(dev)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        U.calls(tk, q, ids, X, aux)
        for m in (1, 32, 33):
            cur = X.shape[0]
            # half from the last two tiles, half from anywhere
            pos = torch.unique(torch.cat([torch.randint(max(0, cur - 64), cur, (m,), generator=g), torch.randint(0, cur, (m,), generator=g)]))
            pos = pos[torch.randperm(pos.numel(), generator=g)][:m]
            X, ids, _ = after_removal(X, ids, pos)
            tk.remove_items(pos)
            if n == 70_017:
                assert X.shape[0] % 32 == {1: 0, 32: 0, 33: 31}[m]
            eng = tk._bind()
            assert tk._index.buf.numel() == eng._fn("index_floats")(E.C.byref(eng.shape), X.shape[0])
            U.equals_fresh(tk, make, X, ids, q, aux, f"{module} {route} {n} minus {m} -> {X.shape[0]}")


def test_remove_across_the_proved_rule(dev):
    """16 484 -> 16 284 items crosses the 16 384-item rule of the default exact mode downwards: proved before, dense after, holding a fresh dense
    module's buffers and nothing more (equals_fresh compares the key sets of `held` and the engine types); then back above it with append_items."""
    cfg, mol, make, aux = U.setup_route("brute", "default", dev)
    n = 16_384 + 100
    g = torch.Generator().manual_seed(33)
    with torch.inference_mode():
        full, full_ids = U.table(cfg, n + 300, 10, dev), U.ids_of(n + 300, dev)
        X, ids = full[:n].clone(), full_ids[:n].clone()
        q = O.synthetic_queries(cfg, B, seed=8).to(dev)
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        before = U.equals_fresh(tk, make, X, ids, q, aux, f"{n} items")
        assert tk._bind().exact is not None and tk._index32 is not None
        pos = removal_set(n, g, must=(before["forward10"][1][:4, 0] - 1) // 3, extra=400)[:200]
        X, ids, _ = after_removal(X, ids, pos)
        tk.remove_items(pos)
        assert X.shape[0] == 16_384 - 100
        assert tk._bind().exact is None and tk._index32 is None and tk._rows32 is None
        U.equals_fresh(tk, make, X, ids, q, aux, "16 284 items")
        tk.append_items(full[n:], full_ids[n:])
        X, ids = torch.cat([X, full[n:]]), torch.cat([ids, full_ids[n:]])
        assert tk._bind().exact is not None and tk._index32 is not None
        U.equals_fresh(tk, make, X, ids, q, aux, "16 584 items")
        st = tk.stats()
        assert st["proved_calls"] + st["fallbacks"] == st["calls"] > 0, st


@pytest.mark.parametrize("module", ["brute", "comb"])
def test_chains_of_updates_appends_and_removes(module, dev):
    cfg, mol, make, aux = U.setup_route(module, "default", dev)
    n = 40_011
    g = torch.Generator().manual_seed(34)
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 14, dev), U.ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=9).to(dev)
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        U.calls(tk, q, ids, X, aux)
        # update
        p = U.positions_for(n, g)
        r = U.table(cfg, p.numel(), 31, dev, first=30_000_000)
        tk.update_items(p, r)
        X[p.to(dev)] = r
        U.equals_fresh(tk, make, X, ids, q, aux, f"{module} chain: update")
        # remove (overlaps the updated positions)
        p = removal_set(X.shape[0], g, must=p[:20])
        X, ids, _ = after_removal(X, ids, p)
        tk.remove_items(p)
        U.equals_fresh(tk, make, X, ids, q, aux, f"{module} chain: remove")
        # append
        extra, extra_ids = U.table(cfg, 777, 32, dev, first=40_000_000), U.ids_of(777, dev, first=5_000_000)
        tk.append_items(extra, extra_ids)
        X, ids = torch.cat([X, extra]), torch.cat([ids, extra_ids])
        U.equals_fresh(tk, make, X, ids, q, aux, f"{module} chain: append")
        # remove (part of the appended range, on the device)
        cur = X.shape[0]
        p = removal_set(cur, g, must=torch.arange(cur - 777, cur - 700)).to(dev)
        X, ids, _ = after_removal(X, ids, p)
        tk.remove_items(p)
        U.equals_fresh(tk, make, X, ids, q, aux, f"{module} chain: second remove")
        # update (rows and ids, the moved positions among them)
        p = U.positions_for(X.shape[0], g)
        r = U.table(cfg, p.numel(), 33, dev, first=50_000_000)
        i = ids[p.to(dev)] + 2_000_000_011
        tk.update_items(p, r, i)
        X[p.to(dev)], ids[p.to(dev)] = r, i
        U.equals_fresh(tk, make, X, ids, q, aux, f"{module} chain: second update")


@pytest.mark.parametrize("module", ["avg", "comb"])
def test_remove_with_the_fused_scans(module, dev):
    """N = 300 007 puts the fused coarse and component scans in play (fused_coarse_min_items = 262 144); a second removal takes the corpus below
    that size, where the module falls back to the materialising scan as a fresh one does."""
    cfg, mol, make, aux = U.setup_route(module, "default", dev)
    n = 300_007
    g = torch.Generator().manual_seed(35)
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 8, dev), U.ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=6).to(dev)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        assert n >= tk.fused_coarse_min_items
        before = U.calls(tk, q, ids, X, aux)
        pos = removal_set(n, g, must=(before["forward10"][1][:4, 0] - 1) // 3, extra=1200)[:1000]
        gone = ids[pos.to(dev)]
        X, ids, _ = after_removal(X, ids, pos)
        tk.remove_items(pos.to(dev))
        assert X.shape[0] == n - 1000 >= tk.fused_coarse_min_items
        after = U.equals_fresh(tk, make, X, ids, q, aux, f"{module} fused")
        assert not bool(torch.isin(result_ids(after), gone).any())
        cur = X.shape[0]
        pos = torch.randperm(cur, generator=g)[: cur - 262_000]
        X, ids, _ = after_removal(X, ids, pos)
        tk.remove_items(pos)
        assert tk.num_items == 262_000 < tk.fused_coarse_min_items
        U.equals_fresh(tk, make, X, ids, q, aux, f"{module} below the fused scans")


def test_remove_before_the_first_call_and_between_submits(dev):
    cfg, mol, make, aux = U.setup_route("avg", "default", dev)
    n = 70_001
    g = torch.Generator().manual_seed(36)
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 15, dev), U.ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=10).to(dev)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        unbuilt = set(U.held(tk))
        assert tk._coarse_table is None and tk._rows_cache is None       # nothing lazily built yet
        pos = removal_set(n, g)
        X, ids, _ = after_removal(X, ids, pos)
        tk.remove_items(pos)
        assert tk._coarse_table is None and tk._rows_cache is None and set(U.held(tk)) == unbuilt, "a buffer that was not built stays unbuilt"
        assert set(U.held(make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0)))) == unbuilt
        U.equals_fresh(tk, make, X, ids, q, aux, "avg removal before the first call")
        # a handle submitted before a removal keeps the result of the corpus it was submitted against
        old = tk(q, k=10, **aux)
        handle = tk.submit(q, 10, **aux)
        pos = removal_set(X.shape[0], g, must=(old[1][:4, 0] - 1) // 3)
        X, ids, _ = after_removal(X, ids, pos)
        tk.remove_items(pos.to(dev))
        U.same(tk.result(handle), old, "the handle submitted before the removal")
        new = tk(q, k=10, **aux)
        assert not torch.equal(new[1], old[1])
        U.equals_fresh(tk, make, X, ids, q, aux, "avg removal between submits")


def mips_equals_fresh(tk, X, ids, q, what, ks=(10, 200)):
    fresh = rails_amd.MIPSBruteForceTopK(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
    assert tk.num_items == X.shape[0]
    U.same(tk._index.buf, fresh._index.buf, f"{what}: index")
    U.same(tk._ids_flat, fresh._ids_flat, f"{what}: ids")
    out = {}
    for k in ks:
        out[k] = tk(q, k=k)
        U.same(out[k], fresh(q, k=k), f"{what}: forward {k}")
    return out


def test_mips_update_append_remove(dev):
    D, n = 64, 70_001
    g = torch.Generator().manual_seed(37)
    rows_of = lambda m, seed, first: torch.from_numpy(O.hash_item_table(seed, first, m, D)).to(dev)      # noqa: E731
    with torch.inference_mode():
        X, ids = rows_of(n, 17, 0), U.ids_of(n, dev)
        q = (torch.randn(B, D, generator=g) * 0.05).to(dev)
        tk = rails_amd.MIPSBruteForceTopK(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        before = mips_equals_fresh(tk, X, ids, q, "mips as built")
        best = (before[10][1][:4, 0] - 1) // 3
        # update
        p = U.positions_for(n, g)
        r = rows_of(p.numel(), 51, 10_000_000)
        r[:4] = X[best] * 1.5                               # the updated positions enter the results
        i = ids[p.to(dev)] + 1_000_000_007
        tk.update_items(p, r, i)
        X[p.to(dev)], ids[p.to(dev)] = r, i
        out = mips_equals_fresh(tk, X, ids, q, "mips update")
        assert bool((out[10][1] > 1_000_000_000).any()), "no updated item reached a result"
        tk.update_items(p[:7].to(dev), r[:7].flip(0).unsqueeze(0))       # device positions, (1, M, D) rows, no ids
        X[p[:7].to(dev)] = r[:7].flip(0)
        mips_equals_fresh(tk, X, ids, q, "mips second update")
        # append: a partially filled last tile and a new one, then many tiles
        for m in (95, 4000):
            e, ei = rows_of(m, 52, 20_000_000 + m), U.ids_of(m, dev, first=5_000_000 + m)
            tk.append_items(e, ei.unsqueeze(0))
            X, ids = torch.cat([X, e]), torch.cat([ids, ei])
            mips_equals_fresh(tk, X, ids, q, f"mips append {m}")
        # remove
        out = mips_equals_fresh(tk, X, ids, q, "mips before the removal")
        pos = removal_set(X.shape[0], g, must=(X @ q.T).argmax(0)[:4])
        gone = ids[pos.to(dev)]
        assert bool(torch.isin(out[10][1], gone).any())
        X, ids, want_moved = after_removal(X, ids, pos)
        assert torch.equal(tk.remove_items(pos), want_moved)
        out = mips_equals_fresh(tk, X, ids, q, "mips remove")
        assert not bool(torch.isin(torch.cat([out[10][1].reshape(-1), out[200][1].reshape(-1)]), gone).any())
        # tile boundaries: down to a full last tile, one more tile, then a part-filled one
        for m in (X.shape[0] % 32, 32, 33):
            pos = torch.randperm(X.shape[0], generator=g)[:m].to(dev)
            X, ids, _ = after_removal(X, ids, pos)
            tk.remove_items(pos)
            assert tk._index.buf.numel() == _lib.load().rails_mips_index_floats(D, X.shape[0])
            mips_equals_fresh(tk, X, ids, q, f"mips remove {m} -> {X.shape[0]}")
        # a short chain
        p = U.positions_for(X.shape[0], g, extra=50)
        r = rows_of(p.numel(), 53, 30_000_000)
        tk.update_items(p, r)
        X[p.to(dev)] = r
        pos = removal_set(X.shape[0], g, extra=30)
        X, ids, _ = after_removal(X, ids, pos)
        tk.remove_items(pos)
        e, ei = rows_of(40, 54, 40_000_000), U.ids_of(40, dev, first=7_000_000)
        tk.append_items(e, ei)
        X, ids = torch.cat([X, e]), torch.cat([ids, ei])
        mips_equals_fresh(tk, X, ids, q, "mips chain")
        # rails_mips_index_update itself: an item whose position lies outside the index is skipped, nothing else changes
        cur = X.shape[0]
        buf = tk._index.buf.clone()
        three = rows_of(3, 55, 50_000_000)
        where = torch.tensor([5, cur, -1], dtype=torch.int64, device=dev)          # cur: the first slot outside the index (padding, or past the buffer)
        rc = _lib.load().rails_mips_index_update(E._ptr(three), 3, D, E._ptr(where), E._ptr(buf), cur, E._stream())
        assert rc == _lib.RAILS_OK
        X5 = X.clone()
        X5[5] = three[0]
        U.same(buf, E.MipsIndex(X5).buf, "a direct call with positions outside the index")
        # validation: nothing is touched
        snap, snap_ids = tk._index.buf.clone(), tk._ids_flat.clone()
        for bad in (torch.tensor([1, 1]), torch.tensor([1, cur]), torch.tensor([-1, 2]), torch.tensor([1, 2], dtype=torch.int32), torch.tensor([[1, 2]]),
                    torch.arange(cur), torch.tensor([3, 3], device=dev)):
            with pytest.raises(ValueError):
                tk.remove_items(bad)
        with pytest.raises(ValueError):
            tk.update_items(torch.tensor([1, 1]), three[:2])
        with pytest.raises(ValueError):
            tk.update_items(torch.tensor([1, 2]), three[:2, : D - 1].contiguous())
        with pytest.raises(ValueError):
            tk.update_items(torch.tensor([1, 2]), three[:2].double())
        with pytest.raises(ValueError):
            tk.append_items(three, torch.tensor([1, 2], device=dev))
        assert tuple(tk.remove_items(torch.empty(0, dtype=torch.int64)).shape) == (0, 2)
        U.same(tk._index.buf, snap, "refused calls: index")
        U.same(tk._ids_flat, snap_ids, "refused calls: ids")


def test_refusals_and_validation(dev):
    cfg, mol, make, aux = U.setup_route("brute", "default", dev)
    n = 20_000
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 16, dev), U.ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=11).to(dev)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        want = tk(q, k=10)
        snap = {k: v.clone() for k, v in U.held(tk).items()}
        for bad in (torch.tensor([1, 2, 1]), torch.tensor([1, 2, n]), torch.tensor([-1, 2, 3]), torch.tensor([1, 2, 3], dtype=torch.int32),
                    torch.tensor([[1, 2, 3]]), torch.tensor(5), torch.arange(n), torch.tensor([1, 2, 1], device=dev), torch.arange(n, device=dev)):
            with pytest.raises(ValueError):
                tk.remove_items(bad)
        with pytest.raises(ValueError):
            tk.remove_items([1, 2, 3])
        moved = tk.remove_items(torch.empty(0, dtype=torch.int64))                                   # M = 0: a no-op
        assert tuple(moved.shape) == (0, 2) and moved.dtype == torch.int64 and not moved.is_cuda
        held = U.held(tk)
        assert set(held) == set(snap)
        for k, v in held.items():
            U.same(v, snap[k], f"nothing is modified by a refused call: {k}")
        assert tk._item_embeddings.data_ptr() == X.data_ptr(), "a refused call does not take the table over"
        U.same(tk(q, k=10), want, "after the refused calls")
        # the IVF module: trained on the corpus, refuses and stays as it was
        ivf = rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), k_per_group=5, use_faiss=True)
        first = ivf(q, k=10)
        with pytest.raises(NotImplementedError, match="IVF"):
            ivf.remove_items(torch.tensor([1, 2, 3]))
        U.same(ivf(q, k=10), first, "the IVF module after the refusal")
        assert ivf.num_items == n and torch.equal(X, snap["table"][0])
        # a call whose k exceeds N' raises what a fresh module of N' items raises
        small = make(X[:40].clone().unsqueeze(0), ids[:40].clone().unsqueeze(0))
        small.remove_items(torch.arange(5, 35))
        fresh = make(X[:10].clone().unsqueeze(0), ids[:10].clone().unsqueeze(0))
        with pytest.raises(Exception) as e_fresh:
            fresh(q, k=11)
        with pytest.raises(type(e_fresh.value)):
            small(q, k=11)
        assert small.num_items == 10
