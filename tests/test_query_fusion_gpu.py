"""GPU: query fusion.  The kernels of rails_amd/csrc/fuse.hip against tests/_fuse_ref.py, and the contract of query_lims= on
MoLBruteForceTopK (every exact_mode, precision and route) and MIPSBruteForceTopK: every call means what it means on a module whose all_logits
is the fused matrix.  Every comparison is exact: np.array_equal / torch.equal on bit patterns, positions and ids."""
import numpy as np
import pytest
import torch

import rails_amd
from rails_amd import engine as E
from tests import _fuse_ref as F
from tests import _rank_ref
from tests import test_index_update_gpu as U
from tests import test_item_mask_gpu as M
from tests.test_query_fusion_cpu import SPECIALS
from tests.test_range_gpu import on_device
from tests.test_rank_gpu import PAD_BITS, ROUTES, logit_bits

pytestmark = pytest.mark.gpu
SHAPES = (1, 3, 4, 5, 4_095, 4_096, 4_097, 70_001)
SEGMENTS = (1, 17, 2, 3)                       # sub-query rows per fused row of the kernel tests
NM = 6_007                                     # items of the module tests
LIMS = (0, 1, 3, 6, 11)                        # S = 11 sub-query rows in U = 4 segments of 1, 2, 3 and 5
S, NU = LIMS[-1], len(LIMS) - 1
MODES = (("max", False), ("sum", False), ("sum", True))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits_of(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def same_fusion(got_bits, want_bits, mode):
    """Bit for bit.  The one exception is what IEEE 754 leaves open: the PAYLOAD of a NaN that an addition or a multiplication produces (numpy on
    the host and the device propagate different operands').  Under "sum" a NaN must stand where the reference has one, every other element is
    compared by its bits; "max" moves bits and is compared whole."""
    if mode == "max":
        return np.array_equal(got_bits, want_bits)
    got_nan, want_nan = np.isnan(got_bits.view(np.float32)), np.isnan(want_bits.view(np.float32))
    return np.array_equal(got_nan, want_nan) and np.array_equal(got_bits[~want_nan], want_bits[~want_nan])


def special_rows(rng, rows, n):
    """(rows, n) uint32: gaussians with +-0, +-inf, NaNs of both signs and subnormals strewn in"""
    bits = rng.standard_normal((rows, n)).astype(np.float32).view(np.uint32).copy()
    where = rng.random((rows, n)) < 0.25
    bits[where] = rng.choice(SPECIALS, size=int(where.sum()))
    return bits


# ---- rails_scores_fuse_rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_ld", [0, 5])
def test_scores_fuse_rows_against_the_reference(extra_ld, dev):
    """Every shape at ld = n and at ld = n + 5 behind a lead of 3 elements (the rows of a segment then start at different alignments), segments
    of 1, 17, 2 and 3 rows in one call, the three modes; out contiguous and with a stride of its own."""
    rng = np.random.default_rng(90 + extra_ld)
    lims = np.concatenate([[0], np.cumsum(SEGMENTS)])
    rows = int(lims[-1])
    for n in SHAPES:
        bits = special_rows(rng, rows, n)
        scores = on_device(bits, n + extra_ld, 3 if extra_ld else 0, dev)
        weights = rng.standard_normal(rows).astype(np.float32)
        weights[1], weights[5] = 0.0, -2.5
        for mode, weighted in MODES:
            w = weights if weighted else None
            want = F.fuse(bits.view(np.float32), lims, mode, w).view(np.uint32)
            got = E.scores_fuse_rows(scores, torch.from_numpy(lims).to(dev), mode, None if w is None else torch.from_numpy(w).to(dev))
            assert got.shape == (len(SEGMENTS), n) and got.dtype == torch.float32 and same_fusion(bits_of(got), want, mode), (n, mode, weighted)
            out = on_device(np.full((len(SEGMENTS), n), PAD_BITS, dtype=np.uint32), n + 3, 1, dev)
            back = E.scores_fuse_rows(scores, E.QueryLims(torch.from_numpy(lims), rows, dev), mode, None if w is None else torch.from_numpy(w).to(dev), out=out)
            assert back is out and same_fusion(bits_of(out), want, mode), (n, mode, weighted, "strided out")
            gap = out.as_strided((len(SEGMENTS) - 1, 3), (n + 3, 1), out.storage_offset() + n).contiguous().view(torch.int32)
            assert bool((gap == PAD_BITS).all()), "the gap between the rows of out"
        ones = torch.arange(rows + 1, device=dev)
        for mode in ("max", "sum"):      # the size-1 identity: a copy, NaN payloads included
            assert np.array_equal(bits_of(E.scores_fuse_rows(scores, ones, mode)), bits), (n, mode)


def test_scores_fuse_rows_many_fused_rows(dev):
    """U = 65 537 fused rows of n = 3: more than the grid's y extent, so the loop over it runs; segments of 1 and 2."""
    rng = np.random.default_rng(92)
    fused_rows = 65_537
    sizes = 1 + (np.arange(fused_rows) % 3 == 1)
    lims = np.concatenate([[0], np.cumsum(sizes)])
    bits = special_rows(rng, int(lims[-1]), 3)
    vals = bits.view(np.float32)
    scores = torch.from_numpy(bits.view(np.int32)).to(dev).view(torch.float32)
    two = np.nonzero(sizes == 2)[0]
    for mode in ("max", "sum"):
        want = vals[lims[:-1]].copy()
        a, b = vals[lims[two]], vals[lims[two] + 1]
        with np.errstate(all="ignore"):
            want[two] = np.where(F.orderable(b.view(np.uint32)) > F.orderable(a.view(np.uint32)), b, a) if mode == "max" else (a + b).astype(np.float32)
        assert np.array_equal(want[:50].view(np.uint32), F.fuse(vals[: lims[50]], lims[:51], mode).view(np.uint32))      # (the shortcut is the reference)
        got = E.scores_fuse_rows(scores, torch.from_numpy(lims).to(dev), mode)
        assert same_fusion(bits_of(got), want.view(np.uint32), mode), mode


def test_scores_fuse_rows_predicate_and_refusals(dev):
    rng = np.random.default_rng(93)
    bits = special_rows(rng, 6, 100)
    scores = torch.from_numpy(bits.view(np.int32)).to(dev).view(torch.float32)
    lims = torch.tensor([0, 2, 6], device=dev)
    out = torch.full((2, 100), 7.0, device=dev)
    E.scores_fuse_rows(scores, lims, "max", out=out, run_if=torch.zeros(1, dtype=torch.int32, device=dev))
    assert bool((out == 7.0).all()), "run_if = 0 must leave out untouched"
    E.scores_fuse_rows(scores, lims, "max", out=out, run_if=torch.ones(1, dtype=torch.int32, device=dev))
    assert np.array_equal(bits_of(out), F.fuse(bits.view(np.float32), [0, 2, 6], "max").view(np.uint32))
    with pytest.raises(ValueError, match="overlaps"):
        E.scores_fuse_rows(scores, lims, "max", out=scores[2:4])
    with pytest.raises(ValueError, match='query_weights go with fuse="sum"'):
        E.scores_fuse_rows(scores, lims, "max", torch.ones(6, device=dev))
    with pytest.raises(ValueError, match="must be one of"):
        E.scores_fuse_rows(scores, lims, "mean")
    with pytest.raises(ValueError, match=r"query_lims\[U\] = 6 but there are 5"):
        E.scores_fuse_rows(scores[:5], lims, "max")
    with pytest.raises(ValueError, match="segment 0"):
        E.scores_fuse_rows(scores, torch.tensor([0, 0, 6], device=dev), "max")


# ---- rails_topk_fuse_lists -----------------------------------------------------------------------------------------------------------------
N_LIST = 40_000


def sorted_lists(rng, rows, depth, pools, tie=False):
    """Row r: `depth` distinct positions drawn from pools[r], scores sorted into selection-key order -> (scores, positions)"""
    scores = np.empty((rows, depth), dtype=np.float32)
    pos = np.empty((rows, depth), dtype=np.int64)
    for r in range(rows):
        p = rng.permutation(pools[r])[:depth]
        s = np.full(depth, 1.25, dtype=np.float32) if tie else rng.standard_normal(depth).astype(np.float32).round(1)      # (rounded: ties occur)
        order = np.argsort(~F.keys_of(s, p), kind="stable")
        scores[r], pos[r] = s[order], p[order]
    return scores, pos


def check_lists(scores, pos, lims, k, ids, seen, dev, what):
    want_i, want_s = F.merge_lists(scores, pos, lims, k, ids=ids, invalid_ids=seen)
    got_i, got_s = E.topk_fuse_lists(torch.from_numpy(scores).to(dev), torch.from_numpy(pos).to(dev), torch.tensor(lims, device=dev), k, torch.from_numpy(ids).to(dev),
                                     None if seen is None else torch.from_numpy(seen).to(dev))
    assert got_i.dtype == torch.int64 and got_s.dtype == torch.float32 and got_i.shape == got_s.shape == (len(lims) - 1, k)
    assert np.array_equal(got_i.cpu().numpy(), want_i), f"{what}: ids"
    assert np.array_equal(bits_of(got_s), want_s.view(np.uint32)), f"{what}: score bits"
    return want_i


@pytest.mark.parametrize("m,depth", [(3, 32), (4, 256), (8, 256), (8, 512), (32, 512)])
def test_topk_fuse_lists_against_the_reference(m, depth, dev):
    """One case per tier of the in-LDS sort (m * k' = 96, 1 024, 2 048, 4 096, 16 384).  Three fused rows per call: the full segment, a
    single row, and what is left of 2 m + 1 rows."""
    rng = np.random.default_rng(100 + m + depth)
    ids = (np.arange(N_LIST, dtype=np.int64) * 3 + 1)[rng.permutation(N_LIST)]
    rows = 2 * m + 1
    lims = [0, m, m + 1, rows]
    everything = np.arange(N_LIST)
    w = min(61, depth // 2)
    k = depth - w
    absent = np.broadcast_to(np.arange(1, 601, dtype=np.int64) * 3, (3, 600))      # ids are 1 mod 3: these are nobody's
    # no duplicates: disjoint pools -- every entry a duplicate: one pool of exactly `depth` positions -- overlapping pools
    disjoint = [np.arange(r * depth, (r + 1) * depth) for r in range(rows)]
    one_pool = [np.arange(100, 100 + depth)] * rows
    overlapping = [np.arange(0, 3 * depth)] * rows
    for what, pools, tie in (("no duplicates", disjoint, False), ("every entry a duplicate", one_pool, False), ("overlapping", overlapping, False),
                             ("all ties", overlapping, True), ("all ties, one pool", one_pool, True)):
        scores, pos = sorted_lists(rng, rows, depth, pools, tie)
        top = check_lists(scores, pos, lims, k, ids, None, dev, f"{what}, no seen ids")
        # seen ids: every row's best items (a best copy's item leaves altogether: its other copies must not surface), one nobody has, a repeat
        seen = np.concatenate([top[:, : w - 2], np.full((3, 1), -5), top[:, :1]], axis=1)
        check_lists(scores, pos, lims, k, ids, seen, dev, f"{what}, seen ids")
        if (m, depth) == (8, 256):      # 600 seen ids: every hit in the second tile of 256, a third tile read
            check_lists(scores, pos, lims, k, ids, np.concatenate([absent[:, :300], top[:, : w - 2], absent[:, 300 : 602 - w]], axis=1), dev, f"{what}, 600 seen ids")
    # padding: the tail of every list is (-inf, a real position) or (a score, -1); a position outside the corpus is skipped too
    scores, pos = sorted_lists(rng, rows, depth, overlapping)
    scores[:, depth // 2 :: 2] = -np.inf
    pos[:, depth // 2 + 1 :: 2] = -1
    pos[0, 0] = N_LIST
    check_lists(scores, pos, lims, k, ids, None, dev, "padded lists")
    # fewer than k survivors: (-1, -inf) behind them
    scores, pos = sorted_lists(rng, rows, depth, one_pool)
    seen = ids[np.arange(100, 100 + w)][None].repeat(3, 0)
    got = check_lists(scores, pos, lims, min(512, depth), ids, seen, dev, "fewer than k survivors")
    assert (got[:, depth - w :] == -1).all() and (got[:, : depth - w] >= 0).all()
    if (m, depth) == (8, 256):      # k = 512 against 600 seen ids whose 280 hits (second and third tile) leave every row short of k
        scores, pos = sorted_lists(rng, rows, depth, overlapping)      # (at most 3 * depth = 768 items in a fused row)
        top = check_lists(scores, pos, lims, 512, ids, None, dev, "k = 512, no seen ids")
        got = check_lists(scores, pos, lims, 512, ids, np.concatenate([absent[:, :300], top[:, :280], absent[:, 300:320]], axis=1), dev, "k = 512, 600 seen ids")
        assert (got[:, 768 - 280 :] == -1).all() and (got[:, 0] >= 0).any()


def test_topk_fuse_lists_limits(dev):
    one = torch.zeros((1, 16_385), device=dev)
    pos = torch.zeros((1, 16_385), dtype=torch.int64, device=dev)
    ids = torch.arange(10, device=dev)
    with pytest.raises(NotImplementedError, match="16385 entries"):
        E.topk_fuse_lists(one, pos, torch.tensor([0, 1], device=dev), 5, ids)
    with pytest.raises(NotImplementedError, match="k = 513"):
        E.topk_fuse_lists(one[:, :600], pos[:, :600], torch.tensor([0, 1], device=dev), 513, ids)
    with pytest.raises(NotImplementedError, match="seen ids"):
        E.topk_fuse_lists(one[:, :8], pos[:, :8], torch.tensor([0, 1], device=dev), 5, ids, torch.zeros((1, 4_097), dtype=torch.int64, device=dev))
    assert not E.topk_fuse_lists_supported(1, 16_385, 5, 0, 10) and E.topk_fuse_lists_supported(32, 512, 512, 4_096, (1 << 32) - 1)


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------
def fused_setup(module, route, dev, n=NM):
    make, X, ids, q, aux = M.setup(module, route, dev, n=n)
    return make, X, ids, q[:S].contiguous(), {key: v[:S].contiguous() for key, v in aux.items()}


def fusion_kwargs(mode, weighted, dev, lims=LIMS):
    rng = np.random.default_rng(7)
    w = (rng.standard_normal(lims[-1]).astype(np.float32) * 2) if weighted else None
    kw = {"query_lims": torch.tensor(lims, device=dev), "fuse": mode}
    if weighted:
        kw["query_weights"] = torch.from_numpy(w).to(dev)
    return kw, w


def candidate_index(ids, X):
    return rails_amd.CandidateIndex(ids=ids.reshape(1, -1), embeddings=X.reshape(1, *X.shape[-2:]))


def check_topk(tk, q, aux, kw, fused, eligible, ids, X, k, seen, what):
    """forward (seen None) or get_top_k_outputs against the walk over the fused matrix"""
    want_i, want_s = F.topk_walk(fused, np.broadcast_to(eligible, fused.shape), ids.cpu().numpy(), k, None if seen is None else seen.cpu().numpy())
    if seen is None:
        got_s, got_i = tk(q, k=k, **kw, **aux)
    else:
        got_i, got_s, _ = candidate_index(ids, X).get_top_k_outputs(q, k, {**kw, **aux}, tk, seen)
    assert got_i.shape == got_s.shape == (fused.shape[0], k)
    assert np.array_equal(got_i.cpu().numpy(), want_i), f"{what}: ids"
    assert np.array_equal(bits_of(got_s), want_s.view(np.uint32)), f"{what}: score bits"
    return got_i, got_s


@pytest.mark.parametrize("module,route", ROUTES)
def test_fused_calls_mean_what_they_mean_on_the_fused_matrix(module, route, dev):
    make, X, ids, q, aux = fused_setup(module, route, dev)
    g = torch.Generator().manual_seed(61)
    everything = np.ones((1, NM), dtype=bool)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        plain = logit_bits(tk, q, aux).view(np.float32)
        for mode, weighted in MODES:
            what = f"{module} {route} {mode}{' weighted' if weighted else ''}"
            kw, w = fusion_kwargs(mode, weighted, dev)
            fused = F.fuse(plain, LIMS, mode, w)
            on_dev = torch.from_numpy(fused).to(dev)
            if hasattr(tk, "all_logits"):
                assert np.array_equal(bits_of(tk.all_logits(q, **kw, **aux)), fused.view(np.uint32)), f"{what}: all_logits"
            # forward and get_top_k_outputs; under "max" the list route and the forced matrix route, each counted once
            before = tk.stats()
            top_i, _ = check_topk(tk, q, aux, kw, fused, everything, ids, X, 50, None, f"{what}: forward")
            seen = torch.cat([top_i[:, 2:9], torch.tensor([[2, 5]], device=dev).expand(NU, -1)], dim=1).contiguous()
            filtered = check_topk(tk, q, aux, kw, fused, everything, ids, X, 50, seen, f"{what}: get_top_k_outputs")
            st = tk.stats()
            route_key = "fused_list_calls" if mode == "max" else "fused_matrix_calls"
            assert st[route_key] == before.get(route_key, 0) + 2, (what, before, st)
            if mode == "max":
                tk.FUSE_LIST_MAX_ENTRIES = 0
                forced = check_topk(tk, q, aux, kw, fused, everything, ids, X, 50, seen, f"{what}: the forced matrix route")
                del tk.FUSE_LIST_MAX_ENTRIES
                assert torch.equal(forced[0], filtered[0]) and torch.equal(forced[1], filtered[1])
                st2 = tk.stats()
                assert st2["fused_matrix_calls"] == st.get("fused_matrix_calls", 0) + 1 and st2["fused_list_calls"] == st["fused_list_calls"], (st, st2)
            # rank_of - 1 is the index in the fused exhaustive list
            targets = torch.cat([top_i[:, [0, 7, 49]], ids[torch.randint(0, NM, (NU, 3), generator=g).to(dev)], torch.tensor([[2]], device=dev).expand(NU, -1)], dim=1)
            pos = (targets - 1) // 3
            pos[:, -1] = -1
            want = torch.from_numpy(_rank_ref.ranks(fused.view(np.uint32), np.broadcast_to(everything, fused.shape), pos.cpu().numpy()))
            got = tk.rank_of(q, targets.contiguous(), **kw, **aux)
            assert torch.equal(got.cpu(), want) and got[:, :3].tolist() == [[1, 8, 50]] * NU, f"{what}: rank_of"
            assert torch.equal(tk.rank_of_positions(q, pos.contiguous(), **kw, **aux), got)
            elig = np.ones((NU, NM), dtype=bool)
            np.put_along_axis(elig, ((seen[:, :7] - 1) // 3).cpu().numpy(), False, axis=1)
            want = torch.from_numpy(_rank_ref.ranks(fused.view(np.uint32), elig, pos.cpu().numpy()))
            assert torch.equal(tk.rank_of(q, targets.contiguous(), seen, **kw, **aux).cpu(), want), f"{what}: rank_of with seen ids"
            # the softmax and the range calls equal the engine's passes over the fused matrix
            words = E.item_mask_clear_rows(E.visibility_row(NM, dev).repeat(NU, 1), tk.positions_of(seen.reshape(-1)).view(NU, -1), NM)
            for inv, mask in ((None, None), (seen, words)):
                lse = E.scores_lse(on_dev, mask, 0.7)
                assert torch.equal(tk.log_partition(q, inv, 0.7, **kw, **aux), lse), f"{what}: log_partition"
                assert torch.equal(tk.log_prob_of(q, targets.contiguous(), inv, 0.7, **kw, **aux), E.scores_log_prob(on_dev, pos, lse, mask, 0.7)), f"{what}: log_prob_of"
                thr = torch.from_numpy(np.sort(fused, axis=1)[:, -40].copy()).to(dev)
                assert torch.equal(tk.count_above(q, thr, invalid_ids=inv, **kw, **aux), E.scores_range_count(on_dev, thr, mask)), f"{what}: count_above"
                got = tk.range_search(q, thr, invalid_ids=inv, **kw, **aux)
                want = E.scores_range(on_dev, thr, mask, ids=ids)
                assert all(torch.equal(a, b) for a, b in zip(got, want)), f"{what}: range_search"
                lp = torch.full((NU,), -9.0, device=dev)
                got = tk.range_search(q, min_log_prob=lp, temperature=0.7, invalid_ids=inv, sort=False, **kw, **aux)
                want = E.scores_range(on_dev, lp, mask, 0.7, lse, ids=ids, sort=False)
                assert all(torch.equal(a, b) for a, b in zip(got, want)), f"{what}: range_search by log-probability"


@pytest.mark.parametrize("module,route", ROUTES)
def test_slices_hold_whole_segments_and_change_nothing(module, route, dev):
    """Small MAX_LOGIT_BYTES: the same results from one slice, from slices whose boundary would fall inside a segment if rows were cut, and from
    one slice per fused row; sample_items is reproducible under the change; a segment that cannot fit is refused by name."""
    make, X, ids, q, aux = fused_setup(module, route, dev)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        tk.FUSE_LIST_MAX_ENTRIES = 0      # the matrix route of the top-k is what slices
        for mode, weighted in (("max", False), ("sum", True)):
            kw, _ = fusion_kwargs(mode, weighted, dev)
            seen = tk(q, k=20, **kw, **aux)[1][:, 3:9].contiguous()
            cand = candidate_index(ids, X)

            def calls():
                return {"forward": tk(q, k=30, **kw, **aux), "filtered": cand.get_top_k_outputs(q, 30, {**kw, **aux}, tk, seen)[:2],
                        "rank_of": (tk.rank_of(q, seen, **kw, **aux),), "log_partition": (tk.log_partition(q, seen, **kw, **aux),),
                        "count_above": (tk.count_above(q, 0.0, invalid_ids=seen, **kw, **aux),), "range_search": tk.range_search(q, 0.3, invalid_ids=seen, **kw, **aux),
                        "sample_items": tk.sample_items(q, 8, 1234, 0.9, seen, **kw, **aux)}

            whole = calls()
            assert whole["sample_items"][0].shape == (NU, 8) and not any(bool(torch.isin(whole["sample_items"][0][u], seen[u]).any()) for u in range(NU))
            for budget in (14, 9, 7):      # [(0, 3), (3, 4)]; [(0, 2), (2, 3), (3, 4)]; a slice per fused row (7 = 5 + 2 is what sample_items needs)
                tk.MAX_LOGIT_BYTES = budget * NM * 4
                sliced = calls()
                for name in whole:
                    assert all(torch.equal(a, b) for a, b in zip(sliced[name], whole[name])), f"{module} {route} {mode}: {name} under a budget of {budget} rows"
            tk.MAX_LOGIT_BYTES = 6 * NM * 4
            assert torch.equal(tk.rank_of(q, seen, **kw, **aux), whole["rank_of"][0])      # 5 + 1 rows fit
            with pytest.raises(NotImplementedError, match=type(tk).__name__ + r"\.sample_items: a segment of 5 sub-query rows and its fused rows"):
                tk.sample_items(q, 8, 1234, 0.9, seen, **kw, **aux)
            tk.MAX_LOGIT_BYTES = 5 * NM * 4
            for name, call in (("rank_of", lambda: tk.rank_of(q, seen, **kw, **aux)), ("forward", lambda: tk(q, k=30, **kw, **aux)),
                               ("count_above", lambda: tk.count_above(q, 0.0, **kw, **aux))):
                with pytest.raises(NotImplementedError, match=type(tk).__name__ + rf"\.{name}: a segment of 5 sub-query rows and its fused row of"):
                    call()
            del tk.MAX_LOGIT_BYTES


@pytest.mark.parametrize("module,route", ROUTES)
def test_segments_of_one_row_are_the_plain_call(module, route, dev):
    make, X, ids, q, aux = fused_setup(module, route, dev)
    ones = torch.arange(S + 1, device=dev)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        cand = candidate_index(ids, X)
        seen = tk(q, k=20, **aux)[1][:, 3:9].contiguous()
        targets = tk(q, k=20, **aux)[1][:, ::4].contiguous()

        def calls(kw):
            out = {"forward": tk(q, k=30, **kw, **aux), "filtered": cand.get_top_k_outputs(q, 30, {**kw, **aux}, tk, seen)[:2],
                   "plain": cand.get_top_k_outputs(q, 30, {**kw, **aux}, tk, None)[:2],
                   "rank_of": (tk.rank_of(q, targets, seen, **kw, **aux),), "rank_of_positions": (tk.rank_of_positions(q, (targets - 1) // 3, **kw, **aux),),
                   "log_partition": (tk.log_partition(q, seen, 0.8, **kw, **aux),), "log_prob_of": (tk.log_prob_of(q, targets, seen, 0.8, **kw, **aux),),
                   "log_prob_of_positions": (tk.log_prob_of_positions(q, (targets - 1) // 3, None, 0.8, **kw, **aux),),
                   "sample_items": tk.sample_items(q, 6, 99, 0.8, seen, **kw, **aux), "count_above": (tk.count_above(q, 0.1, invalid_ids=seen, **kw, **aux),),
                   "range_search": tk.range_search(q, 0.1, invalid_ids=seen, **kw, **aux)}
            if hasattr(tk, "all_logits"):
                out["all_logits"] = (tk.all_logits(q, **kw, **aux),)
            return out

        want = calls({})
        for fuse in ({}, {"fuse": "max"}, {"fuse": "sum"}):
            for cap in (None, 0):
                if cap is not None:
                    tk.FUSE_LIST_MAX_ENTRIES = cap
                got = calls({"query_lims": ones, **fuse})
                for name in want:
                    assert all(torch.equal(a, b) for a, b in zip(got[name], want[name])), f"{module} {route} {fuse} cap {cap}: {name}"
                if cap is not None:
                    del tk.FUSE_LIST_MAX_ENTRIES


@pytest.mark.parametrize("module,route", ROUTES)
def test_fused_calls_honour_what_a_fused_row_may_return(module, route, dev):
    """A hidden set, per-fused-row allowed_tags=, a ragged per-fused-row item_mask= and seen ids, on both routes."""
    make, X, ids, q, aux = fused_setup(module, route, dev)
    g = torch.Generator().manual_seed(62)
    with torch.inference_mode():
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        plain = logit_bits(tk, q, aux).view(np.float32)
        best = ((tk(q, k=10, **aux)[1][:, :2] - 1) // 3).reshape(-1).cpu()
        hidden = torch.unique(torch.cat([best, torch.randperm(NM, generator=g)[:500], torch.tensor([0, 31, 32, NM - 1])]))
        vis = torch.ones(NM, dtype=torch.bool)
        vis[hidden] = False
        r200 = torch.zeros(NM, dtype=torch.bool)
        r200[torch.randperm(NM, generator=g)[:200]] = True
        per_row = torch.stack([torch.ones(NM, dtype=torch.bool), torch.rand(NM, generator=g) < 0.5, r200, torch.rand(NM, generator=g) < 0.6])
        tags = torch.randint(0, 8, (NM,), generator=g)
        allowed = [1, 2, 5, 3]
        by_tag = (tags[None, :] & torch.tensor(allowed)[:, None]) != 0
        tk.hide_items(hidden)
        tk.set_item_tags(tags.to(dev))
        for mode, weighted in (("max", False), ("sum", True)):
            kw, w = fusion_kwargs(mode, weighted, dev)
            fused = F.fuse(plain, LIMS, mode, w)
            for cap in ((None, 0) if mode == "max" else (None,)):
                if cap is not None:
                    tk.FUSE_LIST_MAX_ENTRIES = cap
                for what, elig, extra in (("hidden set", vis[None].expand(NU, -1), {}),
                                          ("ragged per-row mask", per_row & vis[None], {"item_mask": E.ItemMask(per_row.to(dev))}),
                                          ("per-row bool mask", per_row & vis[None], {"item_mask": per_row.to(dev)}),
                                          ("per-row allowed_tags", by_tag & vis[None], {"allowed_tags": allowed})):
                    what = f"{module} {route} {mode} cap {cap}: {what}"
                    elig_np = elig.numpy()
                    top_i, _ = check_topk(tk, q, aux, {**kw, **extra}, fused, elig_np, ids, X, 40, None, what)
                    seen = top_i[:, 1:8].contiguous()
                    check_topk(tk, q, aux, {**kw, **extra}, fused, elig_np, ids, X, 40, seen, what + ", seen ids")
                    unseen = elig_np.copy()
                    np.put_along_axis(unseen, ((seen - 1) // 3).cpu().numpy(), False, axis=1)
                    want = torch.from_numpy(_rank_ref.ranks(fused.view(np.uint32), unseen, ((top_i - 1) // 3).cpu().numpy()))
                    assert torch.equal(tk.rank_of(q, top_i.contiguous(), seen, **kw, **extra, **aux).cpu(), want), what + ": rank_of"
                    if hasattr(tk, "all_logits"):
                        masked = np.where(elig_np, fused, np.float32(-np.inf))
                        assert np.array_equal(bits_of(tk.all_logits(q, **kw, **extra, **aux)), masked.view(np.uint32)), what + ": all_logits"
                if cap is not None:
                    del tk.FUSE_LIST_MAX_ENTRIES
        with pytest.raises(ValueError, match="item_mask has 11 rows but the batch has 4"):
            tk(q, k=5, query_lims=torch.tensor(LIMS, device=dev), item_mask=torch.ones((S, NM), dtype=torch.bool, device=dev), **aux)
        with pytest.raises(ValueError, match="allowed_tags has 11 words but the batch has 4"):
            tk(q, k=5, query_lims=torch.tensor(LIMS, device=dev), allowed_tags=[1] * S, **aux)


def test_the_list_route_keeps_the_proved_flow(dev):
    """The default mode on a corpus large enough for the proved flow: the list route runs it on the sub-query rows (calls are counted), a forced
    redo included, and equals the matrix route and the walk over the fused fp32 logits."""
    make, X, ids, q, aux = fused_setup("brute", "default", dev, n=70_001)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        assert tk._bind().exact is not None and tk._index32 is not None
        kw, _ = fusion_kwargs("max", False, dev)
        fused = F.fuse(logit_bits(tk, q, aux).view(np.float32), LIMS, "max")
        everything = np.ones((1, 70_001), dtype=bool)
        before = tk.stats()
        top_i, _ = check_topk(tk, q, aux, kw, fused, everything, ids, X, 100, None, "proved: forward")
        seen = top_i[:, :61].contiguous()
        listed = check_topk(tk, q, aux, kw, fused, everything, ids, X, 100, seen, "proved: get_top_k_outputs")
        st = tk.stats()
        assert st["calls"] == before["calls"] + 2 and st["proved_calls"] + st["fallbacks"] == st["calls"] and st["fused_list_calls"] == 2, (before, st)
        tk._gate_guard_limit = 0.5 * st["guard_max"]      # a failed verdict, as tests/test_proved_gpu.py forces it
        redone = check_topk(tk, q, aux, kw, fused, everything, ids, X, 100, seen, "proved: forced redo")
        st2 = tk.stats()
        assert st2["fallbacks"] == st["fallbacks"] + 1 and st2["calls"] == st["calls"] + 1 and st2["fused_list_calls"] == 3, (st, st2)
        tk.FUSE_LIST_MAX_ENTRIES = 0
        matrix = check_topk(tk, q, aux, kw, fused, everything, ids, X, 100, seen, "the matrix route")
        assert tk.stats()["fused_matrix_calls"] == 1
        for a in (redone, matrix):
            assert torch.equal(a[0], listed[0]) and torch.equal(a[1], listed[1])
        # beyond the list route's limits the matrix route answers with the same bits: k' = 3 400 x 5 rows > 16 384 entries
        del tk.FUSE_LIST_MAX_ENTRIES
        wide = check_topk(tk, q, aux, kw, fused, everything, ids, X, 3_400, None, "k beyond the list route")
        assert tk.stats()["fused_matrix_calls"] == 2 and wide[0].shape == (NU, 3_400)


def test_a_corpus_whose_ids_repeat_takes_the_matrix_route(dev):
    make, X, ids, q, aux = fused_setup("brute", "dense", dev)
    with torch.inference_mode():
        twice = ids.clone()
        twice[5] = twice[4]
        tk = make(X.unsqueeze(0), twice.unsqueeze(0))
        kw, _ = fusion_kwargs("max", False, dev)
        fused = F.fuse(logit_bits(tk, q, aux).view(np.float32), LIMS, "max")
        check_topk(tk, q, aux, kw, fused, np.ones((1, NM), dtype=bool), twice, X, 50, None, "repeated ids")
        assert tk.stats()["fused_matrix_calls"] == 1 and tk.stats()["fused_list_calls"] == 0


@pytest.mark.parametrize("module,route", [("brute", "default"), ("brute", "generic"), ("mips", "mips")])
def test_fused_calls_after_corpus_edits(module, route, dev):
    """update, append and remove between fused calls, with the id map live: the answers of a module freshly built from the resulting corpus,
    on both routes."""
    from tests import test_index_remove_gpu as RM

    make, X, ids, q, aux = fused_setup(module, route, dev)
    cfg = U.O.CONFIGS["amzn-books"] if module == "mips" else U.setup_route(module, route, dev)[0]
    g = torch.Generator().manual_seed(63)
    kw, _ = fusion_kwargs("max", False, dev)
    with torch.inference_mode():
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        top = tk(q, k=10, **kw, **aux)[1]      # (the list route: the id map exists from here on)
        assert tk.stats()["fused_list_calls"] == 1
        X2, ids2 = X.clone(), ids.clone()
        upd = U.positions_for(NM, g)
        rows = U.table(cfg, upd.numel(), 31, dev, first=20_000_000)
        tk.update_items(upd, rows)
        X2[upd.to(dev)] = rows
        tk(q, k=10, **kw, **aux)
        extra = U.table(cfg, 70, 41, dev, first=25_000_000)
        extra[:2] = X[(top[:2, 0] - 1) // 3]      # copies of two fused rows' best items: the appended rows enter the head
        new_ids = torch.arange(-7, -77, -1, device=dev)
        tk.append_items(extra, new_ids)
        X2, ids2 = torch.cat([X2, extra]), torch.cat([ids2, new_ids])
        gone = RM.removal_set(NM + 70, g, must=((top[:, 1] - 1) // 3).cpu())
        tk.remove_items(gone)
        X2, ids2, _ = RM.after_removal(X2, ids2, gone)
        fresh = make(X2.clone().unsqueeze(0), ids2.clone().unsqueeze(0))
        seen = top[:, 2:8].contiguous()
        cand = candidate_index(ids2, X2)
        for cap in (None, 0):
            for m in (tk, fresh):
                if cap is not None:
                    m.FUSE_LIST_MAX_ENTRIES = cap
            for name, call in (("forward", lambda m: m(q, k=60, **kw, **aux)), ("get_top_k_outputs", lambda m: cand.get_top_k_outputs(q, 60, {**kw, **aux}, m, seen)[:2]),
                               ("rank_of", lambda m: (m.rank_of(q, top, seen, **kw, **aux),))):
                assert all(torch.equal(a, b) for a, b in zip(call(tk), call(fresh))), f"{module} {route} cap {cap}: {name} after the edits"
        fused = F.fuse(logit_bits(fresh, q, aux).view(np.float32), LIMS, "max")
        check_topk(tk, q, aux, kw, fused, np.ones((1, fused.shape[1]), dtype=bool), ids2, X2, 60, seen, "after the edits, against the reference")


def test_refusals(dev):
    make, X, ids, q, aux = fused_setup("brute", "dense", dev)
    lims = torch.tensor(LIMS, device=dev)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        for extra in ({"collapse_groups": True}, {"max_per_group": 2}):
            with pytest.raises(NotImplementedError, match="together with query_lims="):
                tk(q, k=5, query_lims=lims, **extra)
            with pytest.raises(NotImplementedError, match="together with query_lims="):
                candidate_index(ids, X).get_top_k_outputs(q, 5, {"query_lims": lims, **extra}, tk, ids[:4].reshape(4, 1).contiguous())
            with pytest.raises(NotImplementedError, match=r"MoLBruteForceTopK\.rank_of takes no (collapse_groups|max_per_group)"):
                tk.rank_of(q, ids[:4].reshape(4, 1).contiguous(), query_lims=lims, **extra)
        with pytest.raises(ValueError, match=r"MoLBruteForceTopK\.forward: fuse= without query_lims="):
            tk(q, k=5, fuse="max")
        with pytest.raises(ValueError, match="query_weights= goes with"):
            tk.rank_of(q, ids[:4].reshape(4, 1).contiguous(), query_lims=lims, query_weights=torch.ones(S, device=dev))
        with pytest.raises(ValueError, match=r"rank_of: target_ids must be \(4, T\)"):
            tk.rank_of(q, ids[:S].reshape(S, 1).contiguous(), query_lims=lims)
        with pytest.raises(ValueError, match=r"invalid_ids must be \(4, "):
            tk.log_partition(q, ids[:S].reshape(S, 1).contiguous(), query_lims=lims)
        with pytest.raises(ValueError, match=r"invalid_ids must be \(4, "):
            candidate_index(ids, X).get_top_k_outputs(q, 5, {"query_lims": lims}, tk, ids[:S].reshape(S, 1).contiguous())
        with pytest.raises(ValueError, match=r"thresholds? .*\(4,\)"):
            tk.count_above(q, torch.zeros(S, device=dev), query_lims=lims)
        for kind in ("avg", "naive", "comb"):
            other = U.MAKERS[kind](tk.mol_module, X.unsqueeze(0), ids.unsqueeze(0))
            with pytest.raises(NotImplementedError, match=type(other).__name__ + r" takes no query_lims"):
                other(q, k=5, query_lims=lims)
            with pytest.raises(NotImplementedError, match=type(other).__name__ + r" takes no query_lims"):
                candidate_index(ids, X).get_top_k_outputs(q, 5, {"query_lims": lims}, other, None)
