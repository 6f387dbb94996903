"""GPU: item masks.  The kernels of rails_amd/csrc/item_mask.hip against numpy / torch bit for bit, and the contract of
a masked call on MoLBruteForceTopK (every exact_mode, precision and route) and MIPSBruteForceTopK: it equals the same call on a module FRESHLY
CONSTRUCTED from the kept rows and their ids, torch.equal on scores and ids.  Inputs and helpers: those of tests/test_index_update_gpu.py."""
import numpy as np
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from tests import test_index_update_gpu as U
from tests.test_index_update_gpu import B

pytestmark = pytest.mark.gpu
N = 70_001
TILE = 8192          # items per tile of the compaction kernels (rails_item_mask_tile_items): 32 x the 256 words of one workgroup
SIZES = (1, 31, 32, 33, 63, 64, 65, 4_095, 4_096, 4_097, 3 * 4_096 + 37, TILE - 1, TILE, TILE + 1)
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def patterns(rows, n, g):
    """name -> (rows, n) bool on the CPU"""
    out = {"none": torch.zeros((rows, n), dtype=torch.bool), "all": torch.ones((rows, n), dtype=torch.bool)}
    out["bit 0"] = out["none"].clone()
    out["bit 0"][:, 0] = True
    out["bit n-1"] = out["none"].clone()
    out["bit n-1"][:, n - 1] = True
    out["alternating"] = (torch.arange(n)[None, :] + torch.arange(rows)[:, None]) % 2 == 0
    out["p = 0.5"] = torch.rand((rows, n), generator=g) < 0.5
    out["p = 0.01"] = torch.rand((rows, n), generator=g) < 0.01
    return out


def packed(mask):
    """(rows, n) bool on the CPU -> (rows, ceil(n / 32)) uint32, little-endian bits, zero high bits in the last word (numpy)"""
    rows, n = mask.shape
    by = np.packbits(mask.numpy(), axis=1, bitorder="little")
    pad = (-by.shape[1]) % 4
    by = np.concatenate([by, np.zeros((rows, pad), dtype=np.uint8)], axis=1)
    return np.ascontiguousarray(by).view("<u4").reshape(rows, -1)


def positions_of(mask):
    """(rows, n) bool on the CPU -> (rows, max count) int64: nonzero ascending per row, pad slots 0"""
    rows = mask.shape[0]
    width = int(mask.sum(1).max())
    out = torch.zeros((rows, width), dtype=torch.int64)
    for r in range(rows):
        p = torch.nonzero(mask[r]).reshape(-1)
        out[r, : p.numel()] = p
    return out


@pytest.mark.parametrize("rows", [1, 3])
def test_pack_set_count_positions_against_numpy(rows, dev):
    assert E._lib.load().rails_item_mask_tile_items() == TILE
    g = torch.Generator().manual_seed(100 + rows)
    for n in SIZES:
        for name, mask in patterns(rows, n, g).items():
            what = f"n = {n}, rows = {rows}, {name}"
            m = E.ItemMask(mask.to(dev)) if rows > 1 else E.ItemMask(mask[0].to(dev))
            assert (m.rows, m.n_items, m.shared) == (rows, n, rows == 1) and m.words.shape == (rows, (n + 31) // 32), what
            assert np.array_equal(m.words.cpu().numpy().view(np.uint32), packed(mask)), what
            counts = mask.sum(1).to(torch.int32)
            assert torch.equal(m.counts.cpu(), counts) and (m.kept_min, m.kept_max) == (int(counts.min()), int(counts.max())), what
            want = positions_of(mask)
            got = m.positions()
            assert got.dtype == torch.int64 and got.shape == want.shape and torch.equal(got.cpu(), want), what
            assert m.positions() is got, "computed once"
            again = torch.full_like(m.counts, -1)       # the count entry on its own
            with E._on_device(dev):
                E._lib.check(E._lib.load().rails_item_mask_count(E._ptr(m.words), rows, n, E._ptr(again), E._stream()), "rails_item_mask_count")
            assert torch.equal(again.cpu(), counts), what
            if rows == 1:       # from_positions == ItemMask(bool) of the same set; shuffled positions, some given twice, CPU or device
                p = torch.nonzero(mask[0]).reshape(-1)
                p = torch.cat([p, p[:3]])[torch.randperm(p.numel() + min(3, p.numel()), generator=g)]
                f = E.ItemMask.from_positions(n, p.to(dev) if n % 2 else p, dev)
                assert f.shared and f.n_items == n and torch.equal(f.words, m.words) and torch.equal(f.counts, m.counts), what
                assert (f.kept_min, f.kept_max) == (m.kept_min, m.kept_max) and torch.equal(f.positions(), got), what
    with pytest.raises(ValueError):
        E.ItemMask.from_positions(10, torch.tensor([3, 10]), dev)
    with pytest.raises(ValueError):
        E.ItemMask.from_positions(10, torch.tensor([-1]), dev)
    # rows_slice of a per-row mask: the rows' words, counts and positions, no sync; a shared mask is its own slice
    if rows == 3:
        mask = patterns(rows, 4_097, g)["p = 0.01"]
        mask[1, :2000] = True
        m = E.ItemMask(mask.to(dev))
        for cached in (False, True):
            if cached:
                m.positions()
            part = m.rows_slice(1, 3)
            assert part.rows == 2 and not part.shared and torch.equal(part.words, m.words[1:3]) and torch.equal(part.counts, m.counts[1:3])
            assert (part.kept_min, part.kept_max) == (int(mask[1:3].sum(1).min()), int(mask[1:3].sum(1).max()))
            assert torch.equal(part.positions().cpu(), positions_of(mask[1:3]))
            assert torch.equal(m.rows_slice(2, 3).positions().cpu(), positions_of(mask[2:3]))
        assert m.rows_slice(0, 3) is m
        shared = E.ItemMask(mask[0].to(dev))
        assert shared.rows_slice(1, 2) is shared
        slots = m.slot_mask()       # bit j of row r: j < counts[r]
        assert torch.equal(slots.counts, m.counts) and torch.equal(slots.positions().cpu(), positions_of(torch.arange(m.kept_max)[None, :] < mask.sum(1)[:, None]))


def test_scores_mask_against_torch(dev):
    g = torch.Generator().manual_seed(7)
    rows, shift = 3, 32 * 3 + 5
    nan_payload = torch.tensor([0x7FC12345], dtype=torch.int32).view(torch.float32)
    for n in SIZES:
        for name, long_mask in patterns(rows, n + shift, g).items():
            for first in (0, shift):
                for per_row in (False, True):
                    what = f"n = {n}, {name}, first_item = {first}, per row = {per_row}"
                    full = long_mask if first else long_mask[:, :n].contiguous()        # a longer mask for the shifted window
                    if not per_row:
                        full = full[:1]
                    m = E.ItemMask(full.to(dev)) if per_row else E.ItemMask(full[0].to(dev))
                    window = full[:, first : first + n].expand(rows, n)
                    buf = torch.randn((rows, n + 5), generator=g)
                    kept = torch.nonzero(window.reshape(-1)).reshape(-1)
                    if kept.numel() >= 1:       # a NaN with a payload and an inf among the kept entries
                        r, x = divmod(int(kept[0]), n)
                        buf[r, x] = nan_payload[0]
                    if kept.numel() >= 2:
                        r, x = divmod(int(kept[-1]), n)
                        buf[r, x] = float("inf")
                    for fill in ((NEG_INF,) if per_row else (-7.5,)):
                        d = buf.to(dev)
                        before = d.clone()
                        flag = torch.zeros(1, dtype=torch.int32, device=dev)
                        E.scores_mask(d[:, :n], m, first_item=first, fill=fill, run_if=flag)
                        assert torch.equal(d.view(torch.int32), before.view(torch.int32)), what + ": run_if = 0 is a no-op"
                        flag.fill_(1)
                        out = E.scores_mask(d[:, :n], m, first_item=first, fill=fill, run_if=flag if fill == NEG_INF else None)
                        assert out.data_ptr() == d.data_ptr()
                        want = before.view(torch.int32).clone()      # (bit patterns: the kept entries, NaN payload included, are not rewritten)
                        fill_bits = torch.tensor([fill], dtype=torch.float32, device=dev).view(torch.int32)[0]
                        want[:, :n] = torch.where(window.to(dev), want[:, :n], fill_bits)
                        assert torch.equal(d.view(torch.int32), want), what      # kept bits, fills, and the 5 slack columns
    m = E.ItemMask(torch.ones(40, dtype=torch.bool, device=dev))
    s = torch.zeros((3, 30), device=dev)
    with pytest.raises(ValueError):
        E.scores_mask(s, m, first_item=11)                                   # the window leaves the mask
    with pytest.raises(ValueError):
        E.scores_mask(s, E.ItemMask(torch.ones((2, 40), dtype=torch.bool, device=dev)))      # a per-row mask of another row count
    with pytest.raises(ValueError):
        E.scores_mask(s.double(), m)


# ---- the contract ------------------------------------------------------------------------------------------------------------------------
def setup(module, route, dev, n=N):
    """-> (make(x, i), X (n, D), ids (n,), q, aux)"""
    if module == "mips":
        cfg = O.CONFIGS["amzn-books"]
        make = lambda x, i: rails_amd.MIPSBruteForceTopK(x, i)      # noqa: E731
        q = (torch.randn(B, cfg.item_embedding_dim, generator=torch.Generator().manual_seed(15)) * 0.05).to(dev)
        aux = {}
    else:
        cfg, mol, make, aux = U.setup_route(module, route, dev)
        q = O.synthetic_queries(cfg, B, seed=5).to(dev)
    return make, U.table(cfg, n, 7, dev), U.ids_of(n, dev), q, aux


def masked_calls(tk, q, ids, X, aux, mask, seen=None, ks=(10, 200), mask_arg=None):
    """The calls of the contract with item_mask=mask (None: the same calls unmasked, on a fresh module) -> their outputs.  `seen`: the 61-wide
    seen list (default: the head of this module's own forward at ks[-1])."""
    kw = dict(aux) if mask is None else {**aux, "item_mask": mask}
    out = {}
    for j, k in enumerate(ks):
        first = dict(kw, item_mask=mask_arg) if (j == 0 and mask_arg is not None) else kw       # (a bool tensor, packed for the call)
        out[f"forward{k}"] = tk(q, k=k, **first)
    if seen is None:
        seen = out[f"forward{ks[-1]}"][1][:, :61].contiguous()
    cand = rails_amd.CandidateIndex(ids=ids.reshape(1, -1), embeddings=X.reshape(1, *X.shape[-2:]))
    out["filtered"] = cand.get_top_k_outputs(q, 50, kw, tk, seen)[:2]
    out["plain"] = cand.get_top_k_outputs(q, 50, kw, tk, None)[:2]
    if hasattr(tk, "all_logits"):
        out["all_logits"] = tk.all_logits(q, **kw)
    return out, seen


def check_against_fresh(tk, make, X, ids, q, aux, mask_cpu, what, dev, ks=(10, 200), calls=None):
    """mask_cpu (N,) or (B, N) bool: the masked calls on tk against fresh modules of the kept rows -- one per DISTINCT row mask."""
    mask_d = mask_cpu.to(dev)
    m = E.ItemMask(mask_d)
    got, seen = masked_calls(tk, q, ids, X, aux, m, ks=ks, mask_arg=mask_d) if calls is None else calls(m)
    rows2d = mask_cpu.reshape(1, -1).expand(B, -1) if mask_cpu.dim() == 1 else mask_cpu
    groups = {}
    for b in range(B):
        groups.setdefault(rows2d[b].numpy().tobytes(), []).append(b)
    assert len(groups) <= 3
    for key, members in groups.items():
        keep = rows2d[members[0]].to(dev)
        fresh = make(X[keep].clone().unsqueeze(0), ids[keep].clone().unsqueeze(0))
        want, _ = masked_calls(fresh, q, ids[keep], X[keep], aux, None, seen=seen, ks=ks)
        sel = torch.tensor(members, device=dev)
        for name in want:
            if name == "all_logits":
                U.same(got[name][sel][:, keep].contiguous(), want[name][sel].contiguous(), f"{what}: all_logits, kept columns")
                assert bool((got[name][sel][:, ~keep] == NEG_INF).all()), f"{what}: all_logits, cleared columns"
                continue
            U.same(tuple(t[sel] for t in got[name]), tuple(t[sel] for t in want[name]), f"{what}: {name}")
        gone = ids[~keep]
        for name in ("forward10", "forward200", "filtered", "plain"):
            if name in got:
                res_ids = got[name][1] if name.startswith("forward") else got[name][0]
                assert not bool(torch.isin(res_ids[sel], gone).any()), f"{what}: {name} returned a cleared id"
    return got


def the_masks(tk, q, ids, aux, g):
    """The three masks of the contract (CPU bool): 60 % shared with the best item of four queries cleared, 3 000 + 4 positions shared, and a
    per-row mask cycling all-true / 50 % / exactly 200."""
    best = ((tk(q, k=10, **aux)[1][:4, 0] - 1) // 3).cpu()       # (ids are 3 * position + 1)
    m60 = torch.rand(N, generator=g) < 0.6
    m60[best] = False
    m3k = torch.zeros(N, dtype=torch.bool)
    m3k[torch.randperm(N, generator=g)[:3000]] = True
    m3k[torch.tensor([0, 31, 32, N - 1])] = True
    r200 = torch.zeros(N, dtype=torch.bool)
    r200[torch.randperm(N, generator=g)[:200]] = True
    three = [torch.ones(N, dtype=torch.bool), torch.rand(N, generator=g) < 0.5, r200]
    per_row = torch.stack([three[b % 3] for b in range(B)])
    assert int(r200.sum()) == 200 and 3000 <= int(m3k.sum()) <= 3004
    return {"60 %": m60, "3 000 items": m3k, "per row": per_row}, best


@pytest.mark.parametrize("module,route", [("brute", r) for r in ("default", "dense", "f16x3", "c4", "generic")] + [("mips", "mips")])
def test_masked_call_equals_a_fresh_module_of_the_kept_rows(module, route, dev):
    make, X, ids, q, aux = setup(module, route, dev)
    g = torch.Generator().manual_seed(21)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        masks, best = the_masks(tk, q, ids, aux, g)
        unmasked = tk(q, k=10, **aux)
        for name, mask in masks.items():
            got = check_against_fresh(tk, make, X, ids, q, aux, mask, f"{module} {route}, {name}", dev)
            if name == "60 %":      # the cleared best items were in the unmasked result and are gone
                assert bool(torch.isin(ids[best.to(dev)], unmasked[1]).all()) and not bool(torch.isin(got["forward10"][1], ids[best.to(dev)]).any())
        U.same(tk(q, k=10, **aux), unmasked, "the unmasked call after the masked ones")
        if module == "brute":
            st = tk.stats()
            sparse_routes = route in ("default", "dense", "c4")      # fused fp32 scoring of positions: the 3 000-item mask goes sparse there
            assert (st.get("masked_sparse_calls", 0) > 0) == sparse_routes and st.get("masked_dense_calls", 0) > 0, st


def test_ragged_rows_on_the_sparse_strategy(dev):
    """A per-row mask whose rows keep 200 / 3 000 / 1 500 items: kept_max = 3 000 -> sparse, short rows padded (default and dense modes)."""
    g = torch.Generator().manual_seed(22)
    for route in ("default", "dense"):
        make, X, ids, q, aux = setup("brute", route, dev)
        with torch.inference_mode():
            tk = make(X.unsqueeze(0), ids.unsqueeze(0))
            three = []
            for count in (200, 3000, 1500):
                r = torch.zeros(N, dtype=torch.bool)
                r[torch.randperm(N, generator=g)[:count]] = True
                three.append(r)
            three[1][0] = three[2][0] = False        # (position 0 is what the padding slots hold: it must not leak into these rows)
            three[0][0] = True
            check_against_fresh(tk, make, X, ids, q, aux, torch.stack([three[b % 3] for b in range(B)]), f"ragged, {route}", dev)
            st = tk.stats()
            assert st.get("masked_sparse_calls", 0) >= 4 and st.get("masked_dense_calls", 0) == 0, st


def test_both_strategies_agree(dev):
    make, X, ids, q, aux = setup("brute", "default", dev)
    g = torch.Generator().manual_seed(23)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        mask = E.ItemMask(the_masks(tk, q, ids, aux, g)[0]["3 000 items"].to(dev))
        outs = {}
        for cap, key in ((0, "masked_dense_calls"), (16384, "masked_sparse_calls")):
            tk.MASK_SPARSE_MAX = cap
            before = dict(tk.stats())
            outs[cap], _ = masked_calls(tk, q, ids, X, aux, mask)
            after = tk.stats()
            other = "masked_sparse_calls" if cap == 0 else "masked_dense_calls"
            assert after.get(key, 0) >= before.get(key, 0) + 4 and after.get(other, 0) == before.get(other, 0), (cap, before, after)
        for name in outs[0]:
            U.same(outs[0][name], outs[16384][name], f"dense against sparse: {name}")


def test_the_proved_flow_stays_the_proved_flow(dev):
    make, X, ids, q, aux = setup("brute", "default", dev)
    g = torch.Generator().manual_seed(24)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        assert tk._bind().exact is not None and tk._index32 is not None
        m60 = the_masks(tk, q, ids, aux, g)[0]["60 %"]
        keep = m60.to(dev)
        mask = E.ItemMask(keep)
        assert mask.kept_min > tk.MASK_PROVED_MIN_KEPT
        fresh = make(X[keep].clone().unsqueeze(0), ids[keep].clone().unsqueeze(0))
        want = {k: fresh(q, k=k, **aux) for k in (10, 200)}
        before = tk.stats()
        for k in (10, 200, 200):
            U.same(tk(q, k=k, item_mask=mask, **aux), want[k], f"proved, masked, k = {k}")
        st = tk.stats()
        assert st["calls"] == before["calls"] + 3 and st["proved_calls"] + st["fallbacks"] == st["calls"], (before, st)
        assert st["proved_calls"] > before["proved_calls"], "no masked call was proved"
        # a failed verdict (the bound's gate guard violated, as tests/test_proved_gpu.py forces it): the redo is masked too
        tk._gate_guard_limit = 0.5 * st["guard_max"]
        U.same(tk(q, k=200, item_mask=mask, **aux), want[200], "proved, masked, forced redo")
        st2 = tk.stats()
        assert st2["fallbacks"] == st["fallbacks"] + 1 and st2["calls"] == st["calls"] + 1, (st, st2)
        # the audit's reference call is masked alike
        tk3 = make(X.unsqueeze(0), ids.unsqueeze(0))
        tk3.audit_every = 1
        U.same(tk3(q, k=10, item_mask=mask, **aux), want[10], "proved, masked, audited")
        assert tk3.audit_summary()["audited"] == 1 and tk3.audit_summary()["mismatches"] == 0


def test_chunked_and_sliced_arms(dev):
    g = torch.Generator().manual_seed(25)
    forwards = lambda tk, q, ids, X, aux: (lambda m: (masked_calls(tk, q, ids, X, aux, m)))      # noqa: E731
    # the corpus scored in chunks of 8 192 items: each chunk masked at its offset
    make, X, ids, q, aux = setup("brute", "dense", dev)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        masks, _ = the_masks(tk, q, ids, aux, g)
        tk.MAX_LOGIT_BYTES, tk.CHUNK_ITEMS = B * N * 4 - 1, 8192
        for name in ("60 %", "per row"):
            check_against_fresh(tk, make, X, ids, q, aux, masks[name], f"chunked, {name}", dev, calls=forwards(tk, q, ids, X, aux))
    # the batch sliced by rows (8 at a time) under the logit policy: a per-row mask is sliced with it
    make, X, ids, q, aux = setup("brute", "default", dev)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        assert tk._bind().exact is not None
        tk.MAX_LOGIT_BYTES = 8 * N * 4
        for name in ("per row", "60 %"):
            check_against_fresh(tk, make, X, ids, q, aux, masks[name], f"sliced, {name}", dev, calls=forwards(tk, q, ids, X, aux))
        st = tk.stats()
        assert st["calls"] > 0 and st["proved_calls"] + st["fallbacks"] == st["calls"], st      # (the 60 % mask's slices ran the proved flow)


@pytest.mark.parametrize("module", ["brute", "mips"])
def test_mask_of_ids(module, dev):
    from tests import test_index_remove_gpu as R

    make, X, ids, q, aux = setup(module, "default", dev)
    g = torch.Generator().manual_seed(26)
    with torch.inference_mode():
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        pos = torch.unique(torch.cat([torch.randperm(N, generator=g)[:20_000], torch.tensor([0, 31, 32, N - 1, N - 2])]))
        wanted = ids[pos.to(dev)]
        by_id, by_pos = tk.mask_of_ids(wanted[torch.randperm(wanted.numel(), generator=g).to(dev)]), E.ItemMask.from_positions(N, pos, dev)
        assert by_id.shared and by_id.n_items == N and torch.equal(by_id.words, by_pos.words) and torch.equal(by_id.counts, by_pos.counts)
        assert by_id.kept_min == by_id.kept_max == pos.numel()
        with pytest.raises(ValueError, match="not in the corpus"):
            tk.mask_of_ids(torch.tensor([2, 5], device=dev))                  # (ids are 3 * position + 1)
        # a removal that moves rows: the old mask is stale, one rebuilt from the surviving ids serves
        gone = R.removal_set(N, g, must=pos[:50])
        X2, ids2, _ = R.after_removal(X, ids, gone)
        tk.remove_items(gone)
        with pytest.raises(ValueError, match="by position"):
            tk(q, k=10, item_mask=by_id, **aux)
        left = wanted[~torch.isin(wanted, ids[gone.to(dev)])]
        mask2 = tk.mask_of_ids(left)
        keep = torch.isin(ids2, left)
        assert mask2.n_items == N - gone.numel() and mask2.kept_max == int(keep.sum()) == left.numel() < wanted.numel()
        fresh = make(X2[keep].clone().unsqueeze(0), ids2[keep].clone().unsqueeze(0))
        for k in (10, 200):
            U.same(tk(q, k=k, item_mask=mask2, **aux), fresh(q, k=k, **aux), f"{module}: after remove_items, k = {k}")


def test_refusals_and_validation(dev):
    cfg, mol, make, aux = U.setup_route("brute", "default", dev)
    n = 20_000
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 16, dev), U.ids_of(n, dev)
        q = O.synthetic_queries(cfg, B, seed=11).to(dev)
        keep = torch.rand(n, generator=torch.Generator().manual_seed(27)) < 0.5
        mask = E.ItemMask(keep.to(dev))
        others = {"avg": U.MAKERS["avg"](mol, X.unsqueeze(0), ids.unsqueeze(0)), "naive": U.MAKERS["naive"](mol, X.unsqueeze(0), ids.unsqueeze(0)),
                  "comb": U.MAKERS["comb"](mol, X.unsqueeze(0), ids.unsqueeze(0)),
                  "ivf": rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), k_per_group=5, use_faiss=True)}
        cand = rails_amd.CandidateIndex(ids=ids.reshape(1, -1), embeddings=X.unsqueeze(0))
        for name, other in others.items():
            with pytest.raises(NotImplementedError, match="IVF" if name == "ivf" else type(other).__name__):
                other(q, k=10, item_mask=mask)
            with pytest.raises(NotImplementedError, match="item_mask"):
                cand.get_top_k_outputs(q, 10, {"item_mask": mask}, other, ids[:61].reshape(1, -1).expand(B, -1).contiguous())
            with pytest.raises(NotImplementedError, match="item_mask"):
                other.all_logits(q, item_mask=mask)
        with pytest.raises(NotImplementedError, match="item_mask"):
            others["avg"].submit(q, 10, item_mask=mask)
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        want = tk(q, k=10)
        # k beyond the smallest row of the mask: what k > N raises, before any launch
        r200 = torch.zeros(n, dtype=torch.bool)
        r200[torch.randperm(n, generator=torch.Generator().manual_seed(28))[:200]] = True
        per_row = E.ItemMask(torch.stack([r200 if b % 3 == 2 else keep for b in range(B)]).to(dev))
        tk(q, k=200, item_mask=per_row)
        with pytest.raises(RuntimeError, match=r"selected index k out of range \(k=201, n=200\)"):
            tk(q, k=201, item_mask=per_row)
        with pytest.raises(RuntimeError, match="selected index k out of range"):       # k' = 150 + 61 under get_top_k_outputs
            cand.get_top_k_outputs(q, 150, {"item_mask": per_row}, tk, ids[:61].reshape(1, -1).expand(B, -1).contiguous())
        with pytest.raises(ValueError, match="rows"):
            tk(q[:5], k=10, item_mask=per_row)
        with pytest.raises(ValueError, match="rows"):
            tk.all_logits(q[:5], item_mask=per_row)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tk(q, k=10, item_mask=keep)
        with pytest.raises(ValueError):
            tk(q, k=10, item_mask=keep.to(dev).float())
        # a stale mask after append_items
        tk.append_items(U.table(cfg, 3, 43, dev), torch.tensor([-1, -2, -3], device=dev))
        for stale in (mask, keep.to(dev)):
            with pytest.raises(ValueError, match="by position"):
                tk(q, k=10, item_mask=stale)
        U.same(tk(q, k=10, item_mask=E.ItemMask(torch.cat([torch.ones(n, dtype=torch.bool), torch.zeros(3, dtype=torch.bool)]).to(dev))), want,
               "the appended items masked out")
