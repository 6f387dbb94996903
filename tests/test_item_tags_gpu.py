"""GPU: item tags and allowed_tags=.  The contract: row b of a filtered call equals row b of the same call on a module FRESHLY
CONSTRUCTED from the rows that row b may return (tags[x] & allowed[b] != 0, not hidden) and their ids -- torch.equal on scores and ids -- on
MoLAvgTopK, MoLNaiveTopK, MoLCombTopK (forward, get_top_k_outputs, submit / result, topk_ids, all_logits), on the exact modules against the
equivalent per-row item_mask=, and across corpus edits; the tag kernels against torch.  Helpers: those of tests/test_hidden_items_gpu.py,
tests/test_item_mask_gpu.py and tests/test_index_update_gpu.py."""
import pytest
import torch

import rails_amd
from rails_amd import engine as E
from tests import test_hidden_items_gpu as H
from tests import test_index_remove_gpu as R
from tests import test_index_update_gpu as U
from tests import test_item_mask_gpu as M

pytestmark = pytest.mark.gpu
N = H.N                      # 4 037: a ragged last tile of 5 items
K_PRIME, K_GROUP = H.K_PRIME, H.K_GROUP
NEG_INF = float("-inf")
ALL, FIVE, ONE, TILES = 0xFFFFFFFF, 0b11111, 1 << 3, (1 << 8) | (1 << 2)
MIX = (FIVE, ONE, TILES, ALL)        # row b of the mixed batch takes MIX[b % 4]: row 31 (ALL) and row 32 (FIVE), the first of the second query tile, differ


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def tag_layout(n, g):
    """(n,) int64 on the CPU: one of 8 random single-bit categories per item, plus bit 8 on one whole tile (items 64..95) and on the ragged last tile."""
    tags = torch.ones(n, dtype=torch.int64) << torch.randint(0, 8, (n,), generator=g)
    tags[64:96] |= 1 << 8
    tags[(n - 1) // 32 * 32:] |= 1 << 8
    return tags


def words_of(allowed, batch):
    return [allowed] * batch if isinstance(allowed, int) else list(allowed)


def check_filtered(tk, make, X, ids, tags, hidden, q, aux, allowed, what, min_items, dev):
    """tk's calls under allowed_tags=allowed against one fresh module per DISTINCT allow word, on the rows that use the word.  tags (N,) int64 and
    hidden (N,) bool: the reference state, on the device."""
    batch = q.shape[0]
    words = words_of(allowed, batch)
    faux = dict(aux, allowed_tags=allowed)
    got, seen = H.approx_calls(tk, q, ids, X, faux)
    logits = tk.all_logits(q, **faux)
    has_ids = isinstance(tk, rails_amd.MoLAvgTopK)
    coarse_pos = tk.topk_ids(q, **faux) if has_ids else None
    for w in dict.fromkeys(words):
        sel = torch.tensor([b for b in range(batch) if words[b] == w], device=dev)
        keep = ((tags & w) != 0) & ~hidden
        fresh = H.routed(make(X[keep].clone().unsqueeze(0), ids[keep].clone().unsqueeze(0)), min_items)
        want, _ = H.approx_calls(fresh, q, ids[keep], X[keep], aux, seen=seen)
        for name in want:
            U.same(tuple(t[sel] for t in got[name]), tuple(t[sel] for t in want[name]), f"{what}, word {w:#x}: {name}")
        gone = ids[~keep]
        for name in got:
            res_ids = got[name][0] if name in ("filtered", "plain") else got[name][1]
            assert not bool(torch.isin(res_ids[sel], gone).any()), f"{what}, word {w:#x}: {name} returned a disallowed or hidden id"
        if has_ids:
            U.same(ids[coarse_pos[sel]], ids[keep][fresh.topk_ids(q, **aux)[sel]], f"{what}, word {w:#x}: topk_ids")
        U.same(logits[sel][:, keep].contiguous(), fresh.all_logits(q, **aux)[sel].contiguous(), f"{what}, word {w:#x}: all_logits, allowed columns")
        assert bool((logits[sel][:, ~keep] == NEG_INF).all()), f"{what}, word {w:#x}: all_logits, disallowed columns"


@pytest.mark.parametrize("route", ["fused", "materialised"])
@pytest.mark.parametrize("shape", ["8x8x32", "8x4x128"])
@pytest.mark.parametrize("kind", ["avg", "naive", "comb"])
def test_filtered_call_equals_a_fresh_module_of_the_allowed_rows(kind, shape, route, dev):
    """B = 2 and B = 33 (a second query tile; 264 component rows, past the slice); a shared word keeping everything, ~60 %, one category, and a
    different word per row; once more with a random 10 % hidden: the filter and the hidden set AND."""
    min_items = H.FUSED if route == "fused" else H.MATERIALISED
    g = torch.Generator().manual_seed(51)
    with torch.inference_mode():
        for batch in (2, 33):
            cfg, mol, aux, q = H.shape_setup(shape, dev, batch)
            make = lambda x, i: H.MAKERS[kind](mol, x, i)      # noqa: E731
            X, ids = U.table(cfg, N, 7, dev), U.ids_of(N, dev)
            tags = tag_layout(N, g).to(dev)
            tk = H.routed(make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), min_items)
            plain, _ = H.approx_calls(tk, q, ids, X, aux)
            assert tk.item_tags is None
            tk.set_item_tags(tags)
            assert tk.item_tags.dtype == torch.int32 and tk.item_tags.data_ptr() != tags.data_ptr()
            nothing = torch.zeros(N, dtype=torch.bool, device=dev)
            mix = [MIX[b % 4] for b in range(batch)]
            for allowed in (ALL, FIVE, ONE, mix) + ((torch.tensor(mix),) if batch == 2 else ()):
                check_filtered(tk, make, X, ids, tags, nothing, q, aux, allowed, f"{kind} {shape} {route}, B = {batch}", min_items, dev)
            again, _ = H.approx_calls(tk, q, ids, X, aux)
            for name in plain:      # tags change nothing for a call without the argument (an item with word 0 included: none here, see the edit chain)
                U.same(again[name], plain[name], f"{kind} {shape} {route}, B = {batch}: {name} without allowed_tags")
        hide = torch.randperm(N, generator=g)[: N // 10]
        tk.hide_items(hide)
        hidden = torch.zeros(N, dtype=torch.bool, device=dev)
        hidden[hide.to(dev)] = True
        for allowed in (FIVE, mix):
            check_filtered(tk, make, X, ids, tags, hidden, q, aux, allowed, f"{kind} {shape} {route}, B = 33, 10 % hidden", min_items, dev)


# ---- engine level: the tagged scans -------------------------------------------------------------------------------------------------------
def ties_at(masked_scores, k, cap, what):
    """What flag == 0 is relied on for: ties at the k-th place of the materialised masked scores.  bf16 scores of 4 037 unit-norm rows ARE tied
    there -- around the 100th of ~2 000 kept scores about 1.6 items share a bf16 value (2 of 2 rows measured tied at place 100 at 8x4x128, B = 2)
    -- so tie-free inputs do not exist at these sizes.  What a tie can do to a right kernel is push a row's candidate count past the capacity
    (every item tied with the k-th score is at or above any threshold below it) and raise the flag; it cannot change the answer, since both
    selections break ties by position.  So the check is the one the flag depends on: the items at or above the k-th score, the whole tied run
    included, fit the candidate lists -- flag == 0 is then attainable and is asserted.  -> rows tied at place k (reported on failure)."""
    top = E.topk(masked_scores, k + 1)[0]
    kth = top[:, k - 1 : k]
    at_or_above = (masked_scores >= kth).sum(dim=1)
    tied = int((top[:, k - 1] == top[:, k]).sum())
    assert int(at_or_above.max()) <= cap, f"{what}: {int(at_or_above.max())} items at or above the k-th score exceed the {cap} slots ({tied} rows tied at place {k})"
    return tied


def filter_of(tags64, words, dev):
    """An E.TagFilter over the tags (N,) int64 on the CPU for the allow words `words`, as a module would resolve it (no hidden set)."""
    eff = torch.where(tags64 >= 1 << 31, tags64 - (1 << 32), tags64).to(torch.int32).to(dev)
    return E.TagFilter(eff, tuple(words), tuple(int(((tags64 & w) != 0).sum()) for w in words))


@pytest.mark.parametrize("shape", ["8x8x32", "8x4x128"])
def test_tagged_scans_answer_without_their_redo(shape, dev):
    """The fused entries themselves at the modules' sizes (N = 4 037; one and two query tiles; the component sample at 2 and at its 128 query rows),
    under tag layouts in which every row keeps at least half the corpus: flag 0 -- the redo, which would hide a wrong tagged kernel behind a
    right answer, is not asked for --, counts of KEPT candidates inside [k, min(capacity, kept)], and the masked materialised selection bit for
    bit (rails_scores_mask_tags + rails_topk).  Before flag == 0 is relied on, the materialised masked scores are
    checked for what ties at the k-th place could do to it (ties_at)."""
    eng = H.CS.engine(shape)
    spec = eng.spec
    pq, px, d = spec.query_dot_product_groups, spec.item_dot_product_groups, spec.dot_product_dimension
    g = torch.Generator().manual_seed(57)
    order = torch.randperm(N, generator=g)
    half = torch.zeros(N, dtype=torch.int64)
    half[order[: N * 11 // 20]] |= 1                                                                   # bit 0 on a random 55 %, bit 1 on another that overlaps it:
    half[order[N * 9 // 20:]] |= 2                                                                     # every item carries one of them, 10 % both
    stripes = torch.ones(N, dtype=torch.int64) << (torch.arange(N) % 4)                                # bit x % 4: every word of three bits keeps 3 / 4
    stripes[64:96] = 1 << 7                                                                            # one whole tile and the ragged last one carry bit 7 alone
    stripes[N // 32 * 32:] = 1 << 7
    layouts = {"two random halves": (half, (1, 2, 3)), "stripes, a tile and the ragged end apart": (stripes, (0b0111, 0b1110 | 1 << 7, 0b1011, 0xFFFFFFFF))}
    with torch.inference_mode():
        coarse_table = H.unit_rows((N, d), 5, dev).bfloat16()
        comp_table = H.unit_rows((px, N, d), 6, dev).bfloat16()
        for name, (tags64, pool) in layouts.items():
            for batch in (2, 33):
                filt = filter_of(tags64, [pool[b % len(pool)] for b in range(batch)], dev)
                assert filt.kept_min * 2 >= N
                eq = H.unit_rows((batch, pq, d), 7 + batch, dev)
                for avg in (False, True):
                    masked = E.scores_mask_tags(eng.coarse_scores(eq, coarse_table, avg), filt)
                    cap = E.MolEngine.coarse_topk_capacity(K_PRIME, N, batch)
                    ties_at(masked, K_PRIME, cap, f"{shape}, {name}, B = {batch}, avg = {avg}")
                    want = E.topk(masked, K_PRIME)
                    sc, pos, counts, flag = eng.coarse_topk(eq, coarse_table, avg, K_PRIME, with_flag=True, tags=filt)
                    kept = torch.tensor(filt.kept, device=dev)
                    assert int(flag.item()) == 0 and K_PRIME <= int(counts.min()) and bool((counts <= kept.clamp_max(cap)).all()), (shape, name, batch, avg, counts.tolist())
                    U.same((sc, pos), want, f"{shape}, {name}, B = {batch}, avg = {avg}: coarse_topk(tags=)")
            for batch in (2, E.TAGGED_COMPONENT_ROWS // pq):
                filt = filter_of(tags64, [pool[b % len(pool)] for b in range(batch)], dev)
                eq = H.unit_rows((batch, pq, d), 9 + batch, dev)
                for kg in (K_GROUP, K_PRIME):
                    masked = E.scores_mask_tags(eng.component_scores(eq, comp_table), filt)
                    cap = eng.component_topk_capacity(batch, N, kg)
                    ties_at(masked, kg, cap, f"{shape}, {name}, B = {batch}, k_g = {kg}")
                    want = E.topk(masked, kg)
                    flag = torch.ones(1, dtype=torch.int32, device=dev)
                    sc, pos, counts = eng.component_topk(eq, comp_table, kg, flag, tags=filt)
                    kept = torch.tensor(filt.kept, device=dev).repeat_interleave(pq * px)
                    assert int(flag.item()) == 0 and kg <= int(counts.min()) and bool((counts <= kept.clamp_max(cap)).all()), (shape, name, batch, kg, int(counts.min()), int(counts.max()))
                    U.same((sc, pos), want, f"{shape}, {name}, B = {batch}, k_g = {kg}: component_topk(tags=)")
            assert eng.component_topk(H.unit_rows((E.TAGGED_COMPONENT_ROWS // pq + 1, pq, d), 3, dev), comp_table, K_GROUP, torch.ones(1, dtype=torch.int32, device=dev),
                                      tags=filter_of(tags64, [pool[0]], dev)) is None      # past the tagged sample's rows: the caller slices
        with pytest.raises(ValueError, match="tags"):
            eng.coarse_topk(eq[:2], coarse_table, False, K_PRIME, tags=filter_of(tags64[:-1], [1], dev))
        with pytest.raises(ValueError, match="tags"):
            eng.coarse_topk(eq[:2], coarse_table, False, K_PRIME, tags=filter_of(tags64, [1, 1, 1], dev))
        with pytest.raises(ValueError, match="hidden set"):
            eng.coarse_topk(eq[:2], coarse_table, False, K_PRIME, tags=filter_of(tags64, [1], dev), visible=E.visibility_row(N, dev))


@pytest.mark.parametrize("entry", ["coarse", "component"])
def test_sample_scan_is_per_row(entry, dev):
    """N = 30 011, K' = 100, B = 2 with the SAME query in both rows; every item carries bit 0, the query's `capacity` best items bit 1 instead;
    allowed = [0b01, 0b11].  Flag 0 and both rows equal to their masked materialised top-K': row 0 holds none of the best items, row 1 the
    unfiltered result.  A sample that ignores the tags fails row 0; a kernel that applies one row's word to the whole tile fails row 1."""
    n, kp = 30_011, K_PRIME
    eng = H.CS.engine("8x8x32")
    spec = eng.spec
    pq, px, d = spec.query_dot_product_groups, spec.item_dot_product_groups, spec.dot_product_dimension
    with torch.inference_mode():
        one = H.unit_rows((1, pq, d), 2, dev)
        eq = torch.cat([one, one]).contiguous()
        if entry == "coarse":
            table = H.unit_rows((n, d), 1, dev).bfloat16()
            cap = E.MolEngine.coarse_topk_capacity(kp, n, 2)
            scores = eng.coarse_scores(eq, table, False)
        else:
            table = H.unit_rows((px, n, d), 3, dev).bfloat16()
            cap = eng.component_topk_capacity(2, n, kp)
            scores = eng.component_scores(eq, table)
        best = torch.topk(scores[0], cap).indices
        tags64 = torch.ones(n, dtype=torch.int64)
        tags64[best.cpu()] = 2
        filt = filter_of(tags64, [0b01, 0b11], dev)
        want = E.topk(E.scores_mask_tags(scores.clone(), filt), kp)
        plain = E.topk(scores, kp)
        if entry == "coarse":
            sc, pos, counts, flag = eng.coarse_topk(eq, table, False, kp, with_flag=True, tags=filt)
            per_query = 1
        else:
            flag = torch.ones(1, dtype=torch.int32, device=dev)
            sc, pos, counts = eng.component_topk(eq, table, kp, flag, tags=filt)
            per_query = pq * px
        assert int(flag.item()) == 0 and kp <= int(counts.min()) and int(counts.max()) <= cap, (int(flag.item()), int(counts.min()), int(counts.max()), cap)
        U.same((sc, pos), want, f"{entry}_topk(tags=) against the masked materialised top-K'")
        assert not bool(torch.isin(pos[0], best).any())                                   # row 0 (its first component row): none of the best items
        U.same((sc[per_query:], pos[per_query:]), (plain[0][per_query:], plain[1][per_query:]), f"{entry}: row 1 is the unfiltered result")


@pytest.mark.parametrize("shape", ["8x8x32", "8x4x64", "8x4x128"])
def test_int8_prefilter_and_tags(shape, dev):
    """The tagged int8 select scan (d = 32 and 64; at d = 128 the bf16 tagged scan answers) under per-row words.  Engine level: coarse_topk(prefilter=,
    tags=) equals the same call without the int8 copy bit for bit, flag 0, and the copy's header shows that the int8 launch tested its tiles.
    Module level: a MoLAvgTopK that holds the copy answers as one without it and as a fresh module of each word's rows."""
    g = torch.Generator().manual_seed(58)
    with torch.inference_mode():
        cfg, mol, aux, q = H.shape_setup(shape, dev, 33)
        d = cfg.dot_product_dimension
        X, ids = U.table(cfg, N, 7, dev), U.ids_of(N, dev)
        tags64 = tag_layout(N, g)
        tags = tags64.to(dev)
        pool = (FIVE, 0b11110000 | 1 << 8, ALL)
        eng = H.CS.engine(shape)
        table = H.unit_rows((N, d), 5, dev).bfloat16()
        pre = eng.build_coarse_prefilter(table)
        for batch in (2, 33):      # one and two query tiles
            filt = filter_of(tags64, [pool[b % 3] for b in range(batch)], dev)
            eq = H.unit_rows((batch, cfg.query_dot_product_groups, d), 7 + batch, dev)
            for avg in (False, True):
                tested = int(pre[32:48].view(torch.int64)[1])
                sc, pos, counts, flag = eng.coarse_topk(eq, table, avg, K_PRIME, with_flag=True, prefilter=pre, tags=filt)
                ran = int(pre[32:48].view(torch.int64)[1]) > tested
                assert ran == (d <= 64), (shape, batch, avg, ran)       # the int8 launch happened (its statistics moved) exactly where it is built
                bf = eng.coarse_topk(eq, table, avg, K_PRIME, with_flag=True, tags=filt)
                assert int(flag.item()) == 0 == int(bf[3].item())
                U.same((sc, pos, counts), bf[:3], f"{shape}, B = {batch}, avg = {avg}: int8 tagged scan against the bf16 tagged scan")
                U.same((sc, pos), E.topk(E.scores_mask_tags(eng.coarse_scores(eq, table, avg), filt), K_PRIME), f"{shape}, B = {batch}, avg = {avg}: against the masked selection")
        words = [pool[b % 3] for b in range(33)]
        outs = {}
        for held in (True, False):
            tk = H.routed(H.MAKERS["avg"](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), H.FUSED)
            tk.PREFILTER_MIN_ITEMS = 0 if held else 1 << 62
            tk.set_item_tags(tags)
            assert tk.allowed_tags_route(words, 33) == "coarse: fused"
            filtered = tk(q, k=K_PRIME, allowed_tags=words, **aux)
            assert (tk._coarse_prefilter is not None) == held
            if held:
                assert (tk.prefilter_stats()["tested"] > 0) == (d <= 64)
            outs[held] = (filtered, tk(q, k=K_PRIME, **aux))
        for a, b in zip(outs[True], outs[False]):
            U.same(a, b, f"{shape}: with the int8 copy against without")
        for w in dict.fromkeys(words):
            keep = (tags & w) != 0
            sel = torch.tensor([b for b in range(33) if words[b] == w], device=dev)
            fresh = H.MAKERS["avg"](mol, X[keep].clone().unsqueeze(0), ids[keep].clone().unsqueeze(0))(q, k=K_PRIME, **aux)
            U.same(tuple(t[sel] for t in outs[True][0]), tuple(t[sel] for t in fresh), f"{shape}, word {w:#x}: against a fresh module")


@pytest.mark.parametrize("kind", ["avg", "naive", "comb"])
def test_redo_paths_honour_the_filter(kind, dev, monkeypatch):
    """Every row allowed a single small category with the routing rule switched off: the tagged sample finds fewer finite group maxima than the
    plan's rank, the threshold is -inf, the flag goes up -- asserted on the fused entry itself, on the same filter -- and the predicated redo on
    the device (masked by tags before its selection) answers; with the redo buffer refused, the host reads the verdict and redoes the call on
    the materialising route.  Categories: 2 K' items for the coarse scan (256 groups of 4 sampled items, r = 61: ~47 finite maxima); 20 items
    for MoLNaiveTopK's component scan (r = 13: ~5)."""
    g = torch.Generator().manual_seed(59)
    size = 20 if kind == "naive" else 2 * K_PRIME
    with torch.inference_mode():
        cfg, mol, aux, q = H.shape_setup("8x8x32", dev, 5)
        make = lambda x, i: H.MAKERS[kind](mol, x, i)      # noqa: E731
        X, ids = U.table(cfg, N, 7, dev), U.ids_of(N, dev)
        order = torch.randperm(N, generator=g)
        tags = torch.full((N,), 1 << 30, dtype=torch.int64)
        for j in range(3):      # three categories of exactly `size` items
            tags[order[j * size:(j + 1) * size]] = 1 << j
        tags = tags.to(dev)
        nothing = torch.zeros(N, dtype=torch.bool, device=dev)
        allowed = [1, 2, 4, 1, 2]
        for redo_bytes in (1 << 30, 0):
            if redo_bytes == 0:      # (the component scans read the class's figure)
                monkeypatch.setattr(rails_amd.MoLAvgTopK, "DEVICE_REDO_BYTES", 0)
            tk = H.routed(make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), H.FUSED)
            tk.TAGGED_FUSED_MIN_GROUPS = 0.0
            tk.set_item_tags(tags)
            assert "materialised" not in tk.allowed_tags_route(allowed, 5)
            # the fused entry on this very filter raises its flag: the call below is answered by a redo
            filt = tk._take_allowed_tags({"allowed_tags": allowed}, 5, ())
            eng = tk._bind()
            eq = eng.query_pack(q, aux.get("user_ids"), want_plain=True)[1]
            if kind == "naive":
                flag = torch.zeros(1, dtype=torch.int32, device=dev)
                assert eng.component_topk(eq, tk._component_table(), K_GROUP, flag, tags=filt) is not None and int(flag.item()) == 1
            else:
                fused = eng.coarse_topk(eq, tk._table(), kind == "comb", K_PRIME, with_flag=True, tags=filt)
                assert fused is not None and int(fused[3].item()) == 1
            check_filtered(tk, make, X, ids, tags, nothing, q, aux, allowed, f"{kind}, redo buffer {redo_bytes}", H.FUSED, dev)


# ---- the exact modules -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module,route", [("brute", "default"), ("brute", "dense"), ("brute", "f16x3"), ("mips", "mips")])
def test_exact_modules_equal_the_per_row_item_mask(module, route, dev):
    n = 40_003 if route == "default" else 20_003
    make, X, ids, q, aux = M.setup(module, route, dev, n=n)
    g = torch.Generator().manual_seed(52)
    with torch.inference_mode():
        tk, twin = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        tags = tag_layout(n, g).to(dev)
        tk.set_item_tags(tags)
        seen = twin(q, k=200, **aux)[1][:, :61].contiguous()
        three = (FIVE, ONE, ALL)
        for name, allowed in (("one category, shared", ONE), ("60 %, shared", FIVE), ("per row", [three[b % 3] for b in range(M.B)])):
            words = torch.tensor(words_of(allowed, M.B), device=dev)
            mask = E.ItemMask(((tags.unsqueeze(0) & words.unsqueeze(1)) != 0).contiguous())
            got, _ = M.masked_calls(tk, q, ids, X, dict(aux, allowed_tags=allowed), None, seen=seen)
            want, _ = M.masked_calls(twin, q, ids, X, aux, mask, seen=seen)
            for call in want:
                U.same(got[call], want[call], f"{module} {route}, {name}: {call}")
        hide = torch.randperm(n, generator=g)[: n // 10].to(dev)      # the filter ANDs with a hidden set
        tk.hide_items(hide)
        vis = torch.ones(n, dtype=torch.bool, device=dev)
        vis[hide] = False
        mask = E.ItemMask((((tags & FIVE) != 0) & vis).contiguous())
        U.same(tk(q, k=50, allowed_tags=FIVE, **aux), twin(q, k=50, item_mask=mask, **aux), f"{module} {route}: allowed_tags on a hidden set")
        with pytest.raises(ValueError, match="allowed_tags= and item_mask="):
            tk(q, k=10, allowed_tags=FIVE, item_mask=mask, **aux)
        kept = int((((tags & ONE) != 0) & vis).sum())
        with pytest.raises(RuntimeError, match=rf"selected index k out of range \(k={kept + 1}, n={kept}\)"):
            tk(q, k=kept + 1, allowed_tags=ONE, **aux)


# ---- the kernels against torch ---------------------------------------------------------------------------------------------------------------
def test_tag_kernels_against_torch(dev):
    n = 8_192 + 37
    g = torch.Generator().manual_seed(53)
    with torch.inference_mode():
        tags64 = torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64) & torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64)
        tags64[::7] = 0
        tags = torch.where(tags64 >= 1 << 31, tags64 - (1 << 32), tags64).to(torch.int32).to(dev)
        vis_bool = torch.rand(n, generator=g) < 0.8
        vis = E.ItemMask(vis_bool.to(dev))
        eff = E.item_tags_effective(tags, vis.words, n)
        eff64 = torch.where(vis_bool, tags64, torch.zeros_like(tags64))
        assert torch.equal(eff.cpu().to(torch.int64) & 0xFFFFFFFF, eff64)
        words = [1, 1 << 31, 0xFFFFFFFF, 0b1010, 1 << 17]
        assert E.item_tags_counts(eff, words) == [int(((eff64 & w) != 0).sum()) for w in words]
        for rows in ([5], [1 << 31, 3, 0xFFFFFFFF]):
            filt = E.TagFilter(eff, tuple(rows), tuple(int(((eff64 & w) != 0).sum()) for w in rows))
            m = filt.item_mask()
            ref = E.ItemMask(torch.stack([(eff64 & w) != 0 for w in rows]).to(dev))
            assert torch.equal(m.words, ref.words) and torch.equal(m.counts, ref.counts) and m.shared == (len(rows) == 1) and m.kept_min == ref.kept_min
        # rails_scores_mask_tags: three allow words over six rows (two rows per word), a window that starts inside the tags, a leading dimension
        # with slack, NaN payloads in kept entries, the launch predicate
        filt = E.TagFilter(eff, (1 << 31, 3, 0xFFFFFFFF), (1, 1, 1))
        first, width, ld = 33, n - 40, n
        base = torch.randn(6, ld, generator=g).to(dev)
        base[:, 5] = float("nan")
        allow = torch.tensor([1 << 31, 1 << 31, 3, 3, 0xFFFFFFFF, 0xFFFFFFFF]).unsqueeze(1)
        keep = ((eff64[first:first + width].unsqueeze(0) & allow) != 0).to(dev)
        for flag, fill in ((None, NEG_INF), (torch.ones(1, dtype=torch.int32, device=dev), -7.5), (torch.zeros(1, dtype=torch.int32, device=dev), -7.5)):
            s = base.clone()
            E.scores_mask_tags(s[:, :width], filt, first_item=first, fill=fill, run_if=flag)
            want = base.view(torch.int32).clone()
            if flag is None or int(flag) == 1:
                fill_bits = torch.tensor([fill], dtype=torch.float32, device=dev).view(torch.int32)[0]
                want[:, :width] = torch.where(keep, want[:, :width], fill_bits)
            assert torch.equal(s.view(torch.int32), want), (fill, flag)
        with pytest.raises(ValueError):
            E.scores_mask_tags(base[:5], filt)                      # five rows against three words
        with pytest.raises(ValueError):
            E.scores_mask_tags(base[:, :50], filt, first_item=n - 10)      # the window leaves the tags


# ---- edit chains -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["avg", "naive", "comb", "brute", "mips"])
def test_edit_chain(kind, dev):
    """set tags -> append (the new items match nothing until tagged) -> tag them by position -> remove across a tile boundary -> hide -> compact: after
    every step the tag row is the reference's and a filtered call equals a fresh module of the allowed rows."""
    g = torch.Generator().manual_seed(54)
    n = N
    mips = kind == "mips"
    allowed = [FIVE, ONE, TILES, ALL, FIVE]

    def check(tk, X, ids, tags, hidden, what):
        assert tk.num_items == X.shape[0] == tags.numel()
        assert torch.equal(tk.item_tags.to(torch.int64) & 0xFFFFFFFF, tags), what
        if kind in ("brute", "mips"):
            words = torch.tensor(allowed, device=dev)
            mask = E.ItemMask((((tags.unsqueeze(0) & words.unsqueeze(1)) != 0) & ~hidden.unsqueeze(0)).contiguous())
            fresh = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
            U.same(tk(q, k=50, allowed_tags=allowed, **aux), fresh(q, k=50, item_mask=mask, **aux), what)
        else:
            check_filtered(tk, make, X, ids, tags, hidden, q, aux, allowed, what, H.MATERIALISED, dev)

    with torch.inference_mode():
        if mips:
            make, X, ids, q, aux = M.setup("mips", "mips", dev, n=n)
            q = q[:5].contiguous()
            cfg = M.O.CONFIGS["amzn-books"]
        else:
            cfg, mol, aux, q = H.shape_setup("8x8x32", dev, 5)
            make = (lambda x, i: H.MAKERS[kind](mol, x, i)) if kind != "brute" else (lambda x, i: rails_amd.MoLBruteForceTopK(mol, x, i))      # noqa: E731
            X, ids = U.table(cfg, n, 7, dev), U.ids_of(n, dev)
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        tags = tag_layout(n, g).to(dev)
        none = torch.zeros(n, dtype=torch.bool, device=dev)
        tk.set_item_tags(tags)
        check(tk, X, ids, tags, none, f"{kind}: set_item_tags")
        m = 70
        rows, new_ids = U.table(cfg, m, 99, dev, first=5_000_000), U.ids_of(m, dev, first=1_000_000)
        tk.append_items(rows, new_ids)
        X2, ids2 = torch.cat([X, rows]), torch.cat([ids, new_ids])
        tags2 = torch.cat([tags, torch.zeros(m, dtype=torch.int64, device=dev)])
        none2 = torch.zeros(n + m, dtype=torch.bool, device=dev)
        check(tk, X2, ids2, tags2, none2, f"{kind}: append_items")
        unfiltered = tk(q, k=10, **aux)      # an item with word 0 stays visible to a call without the argument
        U.same(unfiltered, make(X2.clone().unsqueeze(0), ids2.clone().unsqueeze(0))(q, k=10, **aux), f"{kind}: unfiltered after append_items")
        at = torch.arange(n, n + m, 2)
        new_tags = torch.full((at.numel(),), (1 << 3) | (1 << 31), dtype=torch.int64, device=dev)
        tk.set_item_tags(new_tags, at)
        tags3 = tags2.clone()
        tags3[at.to(dev)] = new_tags
        check(tk, X2, ids2, tags3, none2, f"{kind}: set_item_tags by position")
        gone = R.removal_set(n + m, g, must=torch.tensor([31, 32, 64, n + m - 2]))
        X4, ids4, moved = R.after_removal(X2, ids2, gone)
        tags4 = tags3.clone()
        tags4[moved[:, 1].to(dev)] = tags3[moved[:, 0].to(dev)]
        tags4 = tags4[: n + m - gone.numel()]
        U.same(tk.remove_items(gone), moved, f"{kind}: moved")
        none4 = torch.zeros(tags4.numel(), dtype=torch.bool, device=dev)
        check(tk, X4, ids4, tags4, none4, f"{kind}: remove_items")
        hide = torch.randperm(tags4.numel(), generator=g)[:400]
        tk.hide_items(hide)
        hidden = none4.clone()
        hidden[hide.to(dev)] = True
        check(tk, X4, ids4, tags4, hidden, f"{kind}: hide_items")
        hp = tk.hidden_positions().cpu()
        X5, ids5, moved = R.after_removal(X4, ids4, hp)
        tags5 = tags4.clone()
        tags5[moved[:, 1].to(dev)] = tags4[moved[:, 0].to(dev)]
        tags5 = tags5[: tags4.numel() - hp.numel()]
        tk.compact()
        check(tk, X5, ids5, tags5, torch.zeros(tags5.numel(), dtype=torch.bool, device=dev), f"{kind}: compact")
        # the hand-off: item_tags goes back into set_item_tags as it is
        other = make(X5.clone().unsqueeze(0), ids5.clone().unsqueeze(0))
        other.set_item_tags(tk.item_tags)
        assert torch.equal(other.item_tags, tk.item_tags) and other.item_tags.data_ptr() != tk.item_tags.data_ptr()


def test_filter_between_submit_and_result(dev):
    """A handle outstanding from submit() keeps the tags it was submitted against; the kept counts are cached until tags, hidden set or size change."""
    with torch.inference_mode():
        cfg, mol, aux, q = H.shape_setup("8x8x32", dev, 5)
        X, ids = U.table(cfg, N, 7, dev), U.ids_of(N, dev)
        tk = H.MAKERS["avg"](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        tags = tag_layout(N, torch.Generator().manual_seed(55)).to(dev)
        tk.set_item_tags(tags)
        want = tk(q, k=10, allowed_tags=FIVE, **aux)
        cache = tk._tag_cache
        assert set(cache[2]) == {FIVE} and tk(q, k=10, allowed_tags=[FIVE] * 5, **aux)[1].shape == (5, 10) and tk._tag_cache is cache and set(cache[2]) == {FIVE}
        h = tk.submit(q, 10, allowed_tags=FIVE, **aux)
        tk.set_item_tags(torch.full((N,), 1 << 9, dtype=torch.int64, device=dev))
        U.same(tk.result(h), want, "submitted before set_item_tags")
        assert tk._tag_cache is None
        with pytest.raises(RuntimeError, match=rf"selected index k out of range \(k={K_PRIME}, n=0\)"):
            tk(q, k=10, allowed_tags=FIVE, **aux)


# ---- validation and refusals -----------------------------------------------------------------------------------------------------------------
def test_validation_and_refusals(dev):
    with torch.inference_mode():
        cfg, mol, aux, q = H.shape_setup("8x8x32", dev, 5)
        n = 2_000
        X, ids = U.table(cfg, n, 7, dev), U.ids_of(n, dev)
        mods = {k: H.MAKERS[k](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0)) for k in H.MAKERS}
        mods["brute"] = rails_amd.MoLBruteForceTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        mods["mips"] = rails_amd.MIPSBruteForceTopK(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        tags = torch.ones(n, dtype=torch.int64, device=dev)
        tags[:50] = 2
        for name, tk in mods.items():
            a = {} if name == "mips" else aux
            with pytest.raises(ValueError, match="without tags"):
                tk(q, k=10, allowed_tags=1, **a)
            for bad in (tags[:-1], tags.float(), tags.reshape(1, -1), tags.cpu(), tags - 2, tags + (1 << 32), list(range(n))):
                with pytest.raises(ValueError):
                    tk.set_item_tags(bad)
            for bad_pos in (torch.tensor([0, n]), torch.tensor([-1, 3]), torch.tensor([3, 3]), torch.tensor([1, 2], dtype=torch.int32), torch.tensor([1, 2, 3])):
                with pytest.raises(ValueError):
                    tk.set_item_tags(tags[:2], bad_pos)
            assert tk.item_tags is None, name
            tk.set_item_tags(torch.tensor([2, 2], device=dev), torch.tensor([7, 9]))      # a subset on a module without tags: every other item at 0
            assert int((tk.item_tags != 0).sum()) == 2 and tk.item_tags[7] == 2 == tk.item_tags[9]
            tk.set_item_tags(tags)
            for bad in (0, -1, 1 << 32, [1, 2, 3], [1, 1, 1, 1, 0], [1, 1, 1, 1, 1 << 32], torch.tensor([1, 2]), torch.ones(5), True, "1", [1.0] * 5):
                with pytest.raises(ValueError):
                    tk(q, k=10, allowed_tags=bad, **a)
            if name != "mips":      # a device tensor is accepted: copied to the host
                assert tk(q, k=10, allowed_tags=torch.ones(5, dtype=torch.int64, device=dev), **a)[1].shape[0] == 5
        for name, k in (("avg", K_PRIME), ("comb", K_PRIME)):      # avg_top_k / k_per_group / k beyond the items some row may return
            with pytest.raises(RuntimeError, match=rf"selected index k out of range \(k={k}, n=50\)"):
                mods[name](q, k=10, allowed_tags=[1, 1, 2, 1, 1], **aux)
        for name in ("brute", "mips"):
            with pytest.raises(RuntimeError, match=r"selected index k out of range \(k=51, n=50\)"):
                mods[name](q, k=51, allowed_tags=[1, 1, 2, 1, 1], **({} if name == "mips" else aux))
        mods["naive"].set_item_tags(torch.tensor([4] * 4, device=dev), torch.arange(4))
        with pytest.raises(RuntimeError, match=rf"selected index k out of range \(k={K_GROUP}, n=4\)"):
            mods["naive"](q, k=10, allowed_tags=4, **aux)
        # item_mask= on the approximate modules stays refused; the sharded hand-offs refuse the filter
        mask = E.ItemMask(torch.ones(n, dtype=torch.bool, device=dev))
        for name in ("avg", "naive", "comb"):
            with pytest.raises(NotImplementedError, match="item_mask"):
                mods[name](q, k=10, item_mask=mask, **aux)
        with pytest.raises(NotImplementedError, match="MoLAvgTopK takes no allowed_tags"):
            mods["avg"].coarse_candidates(q, allowed_tags=1, **aux)
        for name, cls in (("naive", "MoLNaiveTopK"), ("comb", "MoLCombTopK")):
            with pytest.raises(NotImplementedError, match=f"{cls} takes no allowed_tags"):
                mods[name].local_candidates(q, allowed_tags=1, **aux)
        for frozen in (False, True):      # the IVF module, with and without frozen centroids
            ivf = rails_amd.MoLNaiveTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0), k_per_group=5, use_faiss=True, frozen_centroids=frozen)
            ivf.set_item_tags(tags)
            cand = rails_amd.CandidateIndex(ids=ids.reshape(1, -1), embeddings=X.unsqueeze(0))
            for call in (lambda: ivf(q, k=10, allowed_tags=1, **aux), lambda: ivf.all_logits(q, allowed_tags=1, **aux),
                         lambda: cand.get_top_k_outputs(q, 10, dict(aux, allowed_tags=1), ivf, None)):
                with pytest.raises(NotImplementedError, match="MoLNaiveTopK.*IVF"):
                    call()
            assert ivf._ivf is None       # nothing built
