"""GPU: the hidden set and allowed_tags inside the IVF list scan -- MoLNaiveTopK(use_faiss=True, filtered_lists=True), DESIGN section 3.10.
The contract: row b of a filtered call is torch.equal, in scores and ids, to row b of the same call on the TWIN, an index (a module) built
with the SAME centroids (ivf_centroids=) from the items row b keeps alone -- engine.IvfIndex.search(filter=) against the twin's plain search
mapped through the ids, and the module's calls against the twin module's.  Shapes are those of tests/test_ivf_update_gpu.py (amzn-books in
fp32 and split-f16, 16x16x64 for d = 64); N = 4096 + 37, nlist = 16, B = 5; B = 130 at P_Q = 8 is 1 040 query rows: two search slices."""
import numpy as np
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from rails_amd.topk_modules import removal_plan
from tests import _ivf_ref as R
from tests.test_index_update_gpu import ids_of, same, table
from tests.test_ivf_gpu import NEAR, check_search
from tests.test_ivf_update_gpu import bits, members, setup

pytestmark = pytest.mark.gpu
N, NLIST, B = 4096 + 37, 16, 5
ALL, NEG_INF = 0xFFFFFFFF, float("-inf")
ROW_WORDS = (0b1, 0b110, 0b11000, 0b11100000, 0xFF)      # one word per row of the B = 5 batch, no two alike


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def module(mol, X, ids, k=5, nlist=NLIST, nprobe=1, **kw):
    return rails_amd.MoLNaiveTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0), k_per_group=k, use_faiss=True, nlist=nlist, nprobe=nprobe, **kw)


def queries(cfg, batch, dev):
    return O.synthetic_queries(cfg, batch, seed=3).to(dev)


def tag_layout(n, seed, dev):
    """(n,) int64: one of 8 random single-bit categories per item."""
    return (torch.ones(n, dtype=torch.int64) << torch.randint(0, 8, (n,), generator=torch.Generator().manual_seed(seed))).to(dev)


def random_hidden(n, share, seed, dev):
    hidden = torch.zeros(n, dtype=torch.bool)
    hidden[torch.randperm(n, generator=torch.Generator().manual_seed(seed))[: int(n * share)]] = True
    return hidden.to(dev)


def visibility(hidden):
    """The (1, words) int32 visibility row of a hidden set -- what the module keeps and hands to the search of a hidden-only call."""
    n = hidden.numel()
    return E.visibility_edit(E.visibility_row(n, hidden.device), n, hidden.nonzero().flatten(), False)[0]


def tag_filter(tags64, hidden, words):
    """E.TagFilter as the module resolves it: the effective tags (0 on a hidden item) and each word's kept count."""
    eff64 = torch.where(hidden, torch.zeros_like(tags64), tags64)
    eff = torch.where(eff64 >= 1 << 31, eff64 - (1 << 32), eff64).to(torch.int32)
    return E.TagFilter(eff, tuple(words), tuple(int(((eff64 & w) != 0).sum()) for w in words))


_STATE = {}


def state(route, dev, nlist=NLIST, n=N):
    """-> dict: the module under test (filtered lists, frozen centroids) over a seeded table, its engine, index and centroids."""
    key = (route, nlist, n)
    if key not in _STATE:
        cfg, mol, _ = setup(route, dev)
        X, ids = table(cfg, n, 21, dev), ids_of(n, dev)
        tk = module(mol, X, ids, nlist=nlist, filtered_lists=True, frozen_centroids=True)
        ivf = tk.ivf_index()
        _STATE[key] = dict(cfg=cfg, mol=mol, X=X, ids=ids, tk=tk, eng=tk._bind(), ivf=ivf, C=ivf.centroids.clone())
    return _STATE[key]


def components(st, q):
    return st["eng"].query_pack(q, None, want_plain=True)[1]


def twin_index(st, keep, nlist=NLIST):
    Xk = st["X"][keep]
    return E.IvfIndex(st["eng"], st["eng"].build_index(Xk), nlist=nlist, centroids=st["C"], items=Xk)


def keeps_of(kind, tags, hidden, words, batch, dev):
    """-> [(rows of the batch, the items they keep)], one entry per distinct rule of the filter."""
    if kind == "hidden":
        return [(torch.arange(batch, device=dev), ~hidden)]
    rows = {}
    for b, w in enumerate(words if len(words) > 1 else words * batch):
        rows.setdefault(w, []).append(b)
    return [(torch.tensor(bs, device=dev), ((tags & w) != 0) & ~hidden) for w, bs in rows.items()]


def filters(kind, tags, hidden, batch):
    """-> (the filter IvfIndex.search takes, its allow words)."""
    if kind == "hidden":
        return visibility(hidden), ()
    words = (0b1111,) if kind == "shared" else tuple(ROW_WORDS[b % len(ROW_WORDS)] for b in range(batch))
    return tag_filter(tags, hidden if kind == "per_row" else torch.zeros_like(hidden), words), words


# ---- engine level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hidden", "shared", "per_row"])
@pytest.mark.parametrize("route", ["fp32", "c4"])
def test_search_equals_the_twin_of_the_kept_rows(route, kind, dev):
    """k_per_group = 5 and 70 (the second half of WaveTopK), nprobe = 1 and 4; hidden-only, a shared allow word, one word per row (on a
    hidden set as well).  check=True: the unfilled flag stays down.  At k = 5 on amzn-books also against tests/_ivf_ref.py on the kept rows."""
    with torch.inference_mode():
        st = state(route, dev)
        ivf, ids = st["ivf"], st["ids"]
        eq = components(st, queries(st["cfg"], B, dev))
        tags, hidden = tag_layout(N, 11, dev), random_hidden(N, 0.3, 12, dev)
        filt, words = filters(kind, tags, hidden, B)
        keeps = keeps_of(kind, tags, hidden if kind != "shared" else torch.zeros_like(hidden), words, B, dev)
        assert len(keeps) == (B if kind == "per_row" else 1)
        twins = [twin_index(st, keep) for _, keep in keeps]
        for k in (5, 70):
            for nprobe in (1, 4):
                got = ivf.search(eq, k, nprobe=nprobe, check=True, filter=filt)
                for (sel, keep), twin in zip(keeps, twins):
                    want = twin.search(eq, k, nprobe=nprobe, check=True)
                    assert torch.equal(ids[got[sel]], ids[keep][want[sel]]), (route, kind, k, nprobe)
                    assert bool(keep[got[sel]].all())
                assert not torch.equal(got, ivf.search(eq, k, nprobe=nprobe)), "the filter removed nothing the plain search returns"
                if route == "fp32" and k == 5:
                    reference_on_kept_rows(st, eq, got, keeps, k, nprobe)


def reference_on_kept_rows(st, eq, got, keeps, k, nprobe):
    """tests/_ivf_ref.py (probe_order, search_row through tests/test_ivf_gpu.check_search, tie-aware) over the kept rows alone: their
    components, and the lists the index holds cut down to them, renumbered as the compaction numbers them."""
    ivf, X = st["ivf"], st["X"]
    pos, off = ivf.positions.cpu().long(), ivf.offsets.cpu().long()
    for sel, keep in keeps:
        keep_c = keep.cpu()
        new_no = torch.cumsum(keep_c.long(), 0) - 1

        class Kept:      # (the index as check_search reads it: the same lists, without the entries the rows do not keep)
            groups, centroids = ivf.groups, ivf.centroids
            positions = torch.stack([new_no[pos[g][keep_c[pos[g]]]] for g in range(ivf.groups)])
            offsets = torch.stack([torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(
                torch.repeat_interleave(torch.arange(ivf.nlist), off[g, 1:] - off[g, :-1])[keep_c[pos[g]]], minlength=ivf.nlist), 0)])
                for g in range(ivf.groups)])

        ex16 = st["eng"].unpack_index(st["eng"].build_index(X[keep]), want_gi=False)[0].half().cpu()
        mine = new_no.to(got.device)[got[sel]]
        assert check_search(mine, eq[sel], Kept, ex16, k, nprobe) < 0.2


def test_two_search_slices_read_their_own_allow_words(dev):
    """B = 130 at P_Q = 8: 1 040 query rows against the 1 024 of one search slice.  Rows 128 and 129 carry other words than rows 0 and 1."""
    with torch.inference_mode():
        st = state("fp32", dev)
        ivf, ids = st["ivf"], st["ids"]
        batch = 130
        assert batch * ivf.query_groups > 1024
        eq = components(st, queries(st["cfg"], batch, dev))
        tags, none = tag_layout(N, 11, dev), torch.zeros(N, dtype=torch.bool, device=dev)
        three = (0b111, 0b111000, 0b11000001)
        words = tuple(three[b % 3] for b in range(batch))
        assert words[128] != words[0] and words[129] != words[1]
        filt = tag_filter(tags, none, words)
        got = ivf.search(eq, 5, nprobe=1, check=True, filter=filt)
        for sel, keep in keeps_of("per_row", tags, none, words, batch, dev):
            want = twin_index(st, keep).search(eq, 5, nprobe=1, check=True)
            assert torch.equal(ids[got[sel]], ids[keep][want[sel]])
        # the batch cut in Python to bound the workspace: the same answer from any cut
        small = E.IvfIndex(st["eng"], st["tk"]._index, nlist=NLIST, centroids=st["C"], items=st["X"])
        small.FILTER_WS_CAP = 1 << 16
        assert torch.equal(small.search(eq, 5, nprobe=1, check=True, filter=filt), got)


def first_lists_of_row0(st, eq):
    """The lists of group 0 in the order row (b = 0, i = 0) probes them, with a clear gap between the first three centroid scores."""
    c, off = st["ivf"].centroids.cpu().double().numpy(), st["ivf"].offsets.cpu().numpy().astype(np.int64)
    lists, cs = R.probe_order(eq[0, 0].cpu().double().numpy(), c[0], off[0], NLIST, 1 << 30)
    assert len(lists) == NLIST and cs[0] - cs[1] > NEAR and cs[1] - cs[2] > NEAR and cs[2] - cs[3] > NEAR
    return lists


@pytest.mark.parametrize("kind", ["hidden", "per_row"])
def test_short_list_rule_counts_eligible_items(kind, dev):
    """Every item of the list row 0 probes first is hidden (disallowed), and all but 3 of its second list: at k_per_group = 5 the row goes on
    into its third list, as the twin does whose first list is empty and whose second holds 3.  per_row: only row 0 is starved."""
    with torch.inference_mode():
        st = state("fp32", dev)
        ivf, ids = st["ivf"], st["ids"]
        eq = components(st, queries(st["cfg"], B, dev))
        lists = first_lists_of_row0(st, eq)
        first, second = members(ivf, lists[0]), members(ivf, lists[1])
        assert first.numel() >= 1 and second.numel() > 5 and members(ivf, lists[2]).numel() >= 2
        starved = torch.zeros(N, dtype=torch.bool, device=dev)
        starved[torch.cat([first, second[3:]]).to(dev)] = True
        none = torch.zeros_like(starved)
        if kind == "hidden":
            filt, keeps = visibility(starved), [(torch.arange(B, device=dev), ~starved)]
        else:
            tags = torch.where(starved, 2, 3)
            words = (1, 3, 3, 3, 3)
            filt, keeps = tag_filter(tags, none, words), keeps_of("per_row", tags, none, words, B, dev)
            assert int(keeps[1][1].sum()) == N
        got = ivf.search(eq, 5, nprobe=1, check=True, filter=filt)
        plain = ivf.search(eq, 5, nprobe=1, check=True)
        for sel, keep in keeps:
            want = twin_index(st, keep).search(eq, 5, nprobe=1, check=True)
            assert torch.equal(ids[got[sel]], ids[keep][want[sel]])
        row0 = got.view(B, ivf.query_groups, ivf.groups, 5)[0, 0, 0]
        assert not torch.equal(row0, plain.view(B, ivf.query_groups, ivf.groups, 5)[0, 0, 0]), "the case does not bite"
        third = members(ivf, lists[2])       # the candidates of row 0: the 3 items left of its second list and its third list, nothing else
        assert bool(torch.isin(row0.cpu(), torch.cat([second[:3], third])).all())
        assert int(torch.isin(row0.cpu(), third).sum()) >= 2, "row 0 did not reach its third list"
        if kind == "per_row":      # the other rows keep their first list: the plain search's rows
            assert torch.equal(got[1:], plain[1:])


def test_segments_without_an_eligible_entry(dev):
    """nlist = 2 at B = 1: ~2 000-item lists in segments of 64 entries.  Nine whole segments of the larger list of group 0 (and wherever else
    those items sit in the other groups' lists) hold no eligible entry."""
    with torch.inference_mode():
        st = state("fp32", dev, nlist=2)
        ivf, ids = st["ivf"], st["ids"]
        eq = components(st, queries(st["cfg"], 1, dev))
        slots = members(ivf, int(ivf.list_sizes()[0].argmax()))
        assert slots.numel() > 1024
        hidden = torch.zeros(N, dtype=torch.bool, device=dev)
        hidden[slots[64:640].to(dev)] = True
        for k in (5, 70):
            got = ivf.search(eq, k, nprobe=1, check=True, filter=visibility(hidden))
            want = twin_index(st, ~hidden, nlist=2).search(eq, k, nprobe=1, check=True)
            assert torch.equal(ids[got], ids[~hidden][want]), k
            assert not torch.equal(got, ivf.search(eq, k, nprobe=1))


# ---- module level ---------------------------------------------------------------------------------------------------------------------
def calls(tk, q, ids, X, aux, seen=None):
    """forward, get_top_k_outputs with a 61-wide seen list and without -> their outputs."""
    out = {"forward": tk(q, k=10, **aux)}
    if seen is None:
        seen = out["forward"][1][:, :61].contiguous()
    cand = rails_amd.CandidateIndex(ids=ids.reshape(1, -1), embeddings=X.unsqueeze(0))
    out["filtered"] = cand.get_top_k_outputs(q, 30, aux, tk, seen)[:2]
    out["plain"] = cand.get_top_k_outputs(q, 30, aux, tk, None)[:2]
    return out, seen


def check_module(tk, mol, X, ids, tags, hidden, q, allowed, C, what):
    """tk's calls against one twin module per distinct rule, on the rows that follow the rule; all_logits column by column."""
    dev, batch = X.device, q.shape[0]
    aux = {} if allowed is None else {"allowed_tags": allowed}
    got, seen = calls(tk, q, ids, X, aux)
    logits = tk.all_logits(q, **aux)
    assert torch.equal(bits(tk._ivf.centroids), bits(C)), f"{what}: the centroids were written"
    words = (allowed,) if isinstance(allowed, int) else tuple(allowed or ())
    for sel, keep in keeps_of("hidden" if allowed is None else "per_row", tags, hidden, words, batch, dev):
        fresh = module(mol, X[keep], ids[keep], k=tk._k_per_group, nlist=tk._ivf.nlist, nprobe=tk.nprobe, ivf_centroids=C)
        want, _ = calls(fresh, q, ids[keep], X[keep], {}, seen=seen)
        gone = ids[~keep]
        for name in want:
            same(tuple(t[sel] for t in got[name]), tuple(t[sel] for t in want[name]), f"{what}: {name}")
            res_ids = got[name][0] if name in ("filtered", "plain") else got[name][1]
            assert not bool(torch.isin(res_ids[sel], gone).any()), f"{what}: {name} returned a hidden or disallowed id"
        same(logits[sel][:, keep].contiguous(), fresh.all_logits(q)[sel].contiguous(), f"{what}: all_logits, kept columns")
        assert bool((logits[sel][:, ~keep] == NEG_INF).all()), f"{what}: all_logits, other columns"


@pytest.mark.parametrize("route", ["fp32", "f16x3", "c4"])
def test_module_equals_the_twin_module(route, dev):
    """A hidden set, tags (a shared word, a word per row), both; fp32, split-f16 and d = 64 engines.  Before any of it: the opted-in module
    with nothing hidden and no tags returns what a module without the flag returns."""
    with torch.inference_mode():
        cfg, mol, _ = setup(route, dev)
        X, ids, q = table(cfg, N, 21, dev), ids_of(N, dev), queries(cfg, B, dev)
        tk = module(mol, X, ids, nlist=NLIST, filtered_lists=True)
        plain_tk = module(mol, X, ids, nlist=NLIST)
        C = tk.ivf_index().centroids.clone()
        assert torch.equal(bits(C), bits(plain_tk.ivf_index().centroids))
        base, seen = calls(plain_tk, q, ids, X, {})
        for name, out in calls(tk, q, ids, X, {}, seen=seen)[0].items():
            same(out, base[name], f"{route}: {name} with nothing hidden and no tags")
        assert tk._ivf._list_words is None and not tk._ivf._filter_plans         # a module that never filters pays for nothing
        tags, none = tag_layout(N, 11, dev), torch.zeros(N, dtype=torch.bool, device=dev)
        tk.set_item_tags(tags)
        for name, out in calls(tk, q, ids, X, {}, seen=seen)[0].items():
            same(out, base[name], f"{route}: {name} with tags and no allowed_tags")
        check_module(tk, mol, X, ids, tags, none, q, 0b1111, C, f"{route}: a shared word")
        check_module(tk, mol, X, ids, tags, none, q, list(ROW_WORDS), C, f"{route}: a word per row")
        hidden = random_hidden(N, 0.3, 12, dev)
        tk.hide_items(hidden.nonzero().flatten())
        assert tk.num_hidden == int(hidden.sum()) and tk.num_visible == N - tk.num_hidden
        assert torch.equal(tk.hidden_positions(), hidden.nonzero().flatten())
        check_module(tk, mol, X, ids, tags, hidden, q, None, C, f"{route}: a hidden set")
        if route != "c4":
            check_module(tk, mol, X, ids, tags, hidden, q, [0b11, 0b11, 0b1100, 0b11, 0xF0], C, f"{route}: tags on a hidden set")
        tk.unhide_items_by_id(ids[hidden])
        assert tk.num_hidden == 0
        for name, out in calls(tk, q, ids, X, {}, seen=seen)[0].items():
            same(out, base[name], f"{route}: {name} after unhiding everything")


def test_edit_chain_under_frozen_centroids(dev):
    """hide / update / append / remove / unhide / compact: after every step the module equals its twins of the mirrored table, hidden set and
    tags, the centroids are bit for bit what they were, and no call returns a hidden or disallowed id."""
    with torch.inference_mode():
        cfg, mol, _ = setup("fp32", dev)
        X, ids, q = table(cfg, N, 21, dev), ids_of(N, dev), queries(cfg, B, dev)
        tk = module(mol, X, ids, nlist=NLIST, filtered_lists=True, frozen_centroids=True)
        C = tk.ivf_index().centroids.clone()
        tags = tag_layout(N, 11, dev)
        tk.set_item_tags(tags)
        hidden = torch.zeros(N, dtype=torch.bool, device=dev)
        allowed = [0b111, 0b111, 0b11111000, 0b111, 0b111]
        g = torch.Generator().manual_seed(9)

        def step(what):
            assert tk.num_items == X.shape[0] and tk.num_hidden == int(hidden.sum())
            check_module(tk, mol, X, ids, tags, hidden, q, None, C, f"{what}: hidden set")
            check_module(tk, mol, X, ids, tags, hidden, q, allowed, C, f"{what}: tags")

        # 1. hide
        pos = torch.randperm(N, generator=g)[:900]
        tk.hide_items(pos)
        hidden[pos.to(dev)] = True
        step("hide")
        # 2. update: hidden and visible items alike get new rows (tags and visibility belong to the position)
        pos = torch.cat([pos[:50], torch.randperm(N, generator=g)[:250]]).unique()
        rows = table(cfg, pos.numel(), 77, dev, first=5_000_000)
        tk.update_items(pos.to(dev), rows)
        X = X.clone()
        X[pos.to(dev)] = rows
        step("update")
        # 3. append: untagged and visible
        rows, new_ids = table(cfg, 200, 78, dev, first=6_000_000), ids_of(200, dev, first=N)
        tk.append_items(rows, new_ids)
        X, ids = torch.cat([X, rows]), torch.cat([ids, new_ids])
        tags, hidden = torch.cat([tags, torch.zeros(200, dtype=torch.int64, device=dev)]), torch.cat([hidden, torch.zeros(200, dtype=torch.bool, device=dev)])
        step("append")
        # 4. remove: the holes are filled from the tail, whose tags and visibility move with it
        gone = torch.randperm(X.shape[0], generator=g)[:300]
        tk.remove_items(gone)
        X, ids, tags, hidden = cut(X, gone), cut(ids, gone), cut(tags, gone), cut(hidden, gone)
        step("remove")
        # 5. unhide half of the hidden set, by id
        back = hidden.nonzero().flatten()[::2]
        tk.unhide_items_by_id(ids[back])
        hidden[back] = False
        step("unhide")
        # 6. compact: the hidden items leave for good
        gone = hidden.nonzero().flatten().cpu()
        tk.compact()
        X, ids, tags, hidden = cut(X, gone), cut(ids, gone), cut(tags, gone), cut(hidden, gone)
        assert tk.num_hidden == 0 and not bool(hidden.any()) and tk._visible is None
        step("compact")


def cut(t, gone):
    """The mirror of remove_items on one per-item array: removal_plan's holes take the tail's movers, the tail is cut."""
    holes, movers = removal_plan(gone.cpu(), t.shape[0])
    out = t[: t.shape[0] - gone.numel()].clone()
    out[holes.to(t.device)] = t[movers.to(t.device)]
    return out


# ---- caches, refusals, validation -----------------------------------------------------------------------------------------------------
def test_a_repeated_filter_reads_nothing_back(dev, monkeypatch):
    with torch.inference_mode():
        cfg, mol, _ = setup("fp32", dev)
        X, ids, q = table(cfg, N, 21, dev), ids_of(N, dev), queries(cfg, B, dev)
        tk = module(mol, X, ids, nlist=NLIST, filtered_lists=True)
        tk.set_item_tags(tag_layout(N, 11, dev))
        first = tk(q, k=10, allowed_tags=list(ROW_WORDS))
        ivf = tk._ivf
        words, plans = ivf._list_words, dict(ivf._filter_plans)
        assert words is not None and len(plans) == 1
        plan = next(iter(plans.values()))
        assert plan.count_rows == B and plan.kept == plan.key.kept and (tk.nprobe, 5) in plan.max_probes

        def refuse(*a, **kw):
            raise AssertionError("a repeated filter made new counts")

        monkeypatch.setattr(E, "IvfFilterPlan", refuse)
        monkeypatch.setattr(ivf.lib, "rails_ivf_plan_filtered", refuse, raising=False)
        same(tk(q, k=10, allowed_tags=list(ROW_WORDS)), first, "the same filter again")
        assert ivf._list_words is words and ivf._filter_plans == plans and next(iter(ivf._filter_plans.values())) is plan
        assert ivf.filter_plan(plan.key) is plan and ivf.filter_plan(plan.key).counts is plan.counts
        monkeypatch.undo()
        # another filter of the same tags: new counts beside the old, the same words in list order
        tk(q, k=10, allowed_tags=0b11)
        assert ivf._list_words is words and len(ivf._filter_plans) == 2
        # the hidden set changes: other words, other plans -- and again none for a repeated call
        tk.hide_items(torch.arange(0, N, 3))
        hidden_only = tk(q, k=10)
        assert ivf._list_words is not words and len(ivf._filter_plans) == 1 and next(iter(ivf._filter_plans.values())).key is tk._visible
        words, plans = ivf._list_words, dict(ivf._filter_plans)
        monkeypatch.setattr(E, "IvfFilterPlan", refuse)
        same(tk(q, k=10), hidden_only, "the same hidden set again")
        assert ivf._list_words is words and ivf._filter_plans == plans
        monkeypatch.undo()
        # a hidden set's counts are ONE row shared by the batch, whatever batches came before: another set, then a smaller batch
        tk.hide_items(torch.arange(1, N, 3))
        full = tk(q, k=10)
        assert [p.count_rows for p in ivf._filter_plans.values()] == [1]
        same(tk(q[:3], k=10), tuple(t[:3] for t in full), "a smaller batch after a larger one")


def test_refusals_and_validation(dev):
    with torch.inference_mode():
        cfg, mol, _ = setup("fp32", dev)
        n = 2_000
        X, ids, q = table(cfg, n, 7, dev), ids_of(n, dev), queries(cfg, B, dev)
        with pytest.raises(ValueError, match="filtered_lists=True applies to the IVF index of use_faiss=True only"):
            rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), k_per_group=5, filtered_lists=True)
        # the twin's own refusals, before any search launch: fewer than nlist kept items, fewer than k_per_group
        tk = module(mol, X, ids, k=5, filtered_lists=True)
        tk.hide_items(torch.arange(0, n - 10))
        with pytest.raises(ValueError, match=rf"10 items cannot fill nlist = {NLIST}"):
            tk(q, k=10)
        tk.unhide_items(torch.arange(0, n - 10))
        tags = torch.zeros(n, dtype=torch.int64, device=dev)
        tags[:12], tags[12:] = 1, 2
        tk.set_item_tags(tags)
        with pytest.raises(ValueError, match=rf"12 items cannot fill nlist = {NLIST}"):
            tk(q, k=10, allowed_tags=[2, 2, 1, 2, 2])
        assert tk(q, k=10, allowed_tags=2)[1].shape == (B, 8 * 8 * 5)
        big = module(mol, X, ids, k=70, filtered_lists=True)
        big.hide_items(torch.arange(0, n - 30))
        with pytest.raises(RuntimeError, match=r"selected index k out of range \(k=70, n=30\)"):
            big(q, k=10)
        big.set_item_tags(torch.ones(n, dtype=torch.int64, device=dev))
        with pytest.raises(RuntimeError, match=r"selected index k out of range \(k=70, n=30\)"):
            big(q, k=10, allowed_tags=1)
        # what stays refused with the flag
        mask = E.ItemMask(torch.ones(n, dtype=torch.bool, device=dev))
        with pytest.raises(NotImplementedError, match="item_mask"):
            tk(q, k=10, item_mask=mask)
        with pytest.raises(NotImplementedError, match="item_mask"):
            tk(q, k=10, item_mask=mask, allowed_tags=2)
        with pytest.raises(NotImplementedError, match="MoLNaiveTopK takes no allowed_tags"):
            tk.local_candidates(q, allowed_tags=2)
        # compact is a removal: without frozen centroids it is remove_items' refusal
        tk.hide_items(torch.tensor([3, 4]))
        with pytest.raises(NotImplementedError, match=r"MoLNaiveTopK\.remove_items: the IVF index \(use_faiss=True\) is trained on the corpus"):
            tk.compact()
        assert tk.num_items == n and tk.num_hidden == 2
        # the default module still refuses all of it, frozen or not, and builds nothing
        for frozen in (False, True):
            plain = module(mol, X, ids, frozen_centroids=frozen)
            plain.set_item_tags(tags)
            for call in (lambda: plain.hide_items(torch.tensor([1])), lambda: plain.unhide_items(torch.tensor([1])), lambda: plain.hide_items_by_id(ids[:1]),
                         lambda: plain.unhide_items_by_id(ids[:1]), plain.hidden_positions, plain.compact, lambda: plain(q, k=10, allowed_tags=1),
                         lambda: plain.all_logits(q, allowed_tags=1)):
                with pytest.raises(NotImplementedError, match="MoLNaiveTopK.*IVF"):
                    call()
            assert plain._visible is None and plain._ivf is None
        # a filter of another corpus, or of another batch, is refused by the engine
        ivf = tk.ivf_index()
        eq = tk._bind().query_pack(q, None, want_plain=True)[1]
        with pytest.raises(ValueError, match="filter must be"):
            ivf.search(eq, 5, filter=tag_filter(tags[:-1], torch.zeros(n - 1, dtype=torch.bool, device=dev), (2,)))
        with pytest.raises(ValueError, match="allow words"):
            ivf.search(eq, 5, filter=tag_filter(tags, torch.zeros(n, dtype=torch.bool, device=dev), (2, 2, 2)))
