"""GPU: query fusion over the candidate union (fuse_candidates = True on MoLAvgTopK / MoLNaiveTopK / MoLCombTopK).
rails_lists_union against np.unique; the modules' fused forward / get_top_k_outputs against the reference walk of
tests/_fuse_candidates_ref.py, whose candidates are read from the module's own plain forward on the sub-query rows and whose scores come from
the module's own rerank_masked / rerank_union_masked on the union.  Every comparison is exact: bit patterns and ids."""
import numpy as np
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from rails_amd import topk_modules as T
from tests import _fuse_candidates_ref as R
from tests import test_hidden_items_gpu as H
from tests import test_index_update_gpu as U
from tests.test_generic_candidates_gpu import candidate_module
from tests.test_generic_candidates_gpu import make as generic_make
from tests.test_item_tags_gpu import FIVE, ONE, TILES, tag_layout

pytestmark = pytest.mark.gpu
LIMS = (0, 1, 3, 6, 11)                        # S = 11 sub-query rows in U = 4 segments of 1, 2, 3 and 5
S, NU = LIMS[-1], len(LIMS) - 1
MODES = (("max", False), ("sum", False), ("sum", True))
N_FUSED, N_SMALL = 300_007, 4_096 + 37
K, W_SEEN = 30, 61
KINDS = ("avg", "naive", "comb")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- rails_lists_union ---------------------------------------------------------------------------------------------------------------------------
def check_union(pos_np, lims_np, n_items, dev, extra_ld=0, w_out=None, what=""):
    rows, width = pos_np.shape
    base = torch.full((rows, width + extra_ld), -7, dtype=torch.int64, device=dev)      # (the gap holds positions that would be dropped anyway: -7)
    base[:, :width] = torch.from_numpy(pos_np).to(dev)
    positions = base[:, :width]
    assert positions.stride(0) == width + extra_ld
    lims = torch.from_numpy(lims_np).to(dev)
    want, want_counts = R.union(pos_np, lims_np, n_items, w_out)
    out = None if w_out is None else torch.full((lims_np.size - 1, w_out), 99, dtype=torch.int64, device=dev)
    got, counts = E.lists_union(positions, lims, n_items, out=out)
    assert out is None or got is out
    assert got.dtype == torch.int64 and counts.dtype == torch.int32 and got.shape == want.shape, what
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts), what
    return want_counts


@pytest.mark.parametrize("extra_ld", [0, 3])
@pytest.mark.parametrize("width", [1, 5, 64, 963])
def test_lists_union_against_the_reference(width, extra_ld, dev):
    """Segments of 1, 2, 3 and 17 rows in one launch (17 x 963 = 16 371 entries: the widest sort), repeated over 3 fused rows each; positions
    drawn from a range narrow enough for duplicates inside a row and across rows, with -1 and positions >= n_items among them; one segment
    that is a single position repeated; ld = W and W + 3."""
    rng = np.random.default_rng(100 + width)
    sizes = np.array([1, 2, 3, 17, 17, 1, 3, 2, 2, 17, 1, 3])
    lims = np.concatenate([[0], np.cumsum(sizes)])
    for n_items in (max(2, width // 2), 50 * width + 7, 1 << 31):
        pos = rng.integers(-1, min(n_items, 40 * width + 40) + 3, size=(int(lims[-1]), width))
        pos[lims[4] : lims[5]] = min(n_items - 1, 12345)      # a segment of 17 rows holding one position
        pos[lims[5]] = -1                                     # a segment with nothing to keep
        counts = check_union(pos, lims, n_items, dev, extra_ld, what=f"W = {width}, n_items = {n_items}")
        assert counts[4] == 1 and counts[5] == 0
    check_union(pos, lims, 1 << 31, dev, extra_ld, w_out=17 * width + 9, what=f"W = {width}, a wider out")


@pytest.mark.parametrize("rows,width", [(1, 64), (16, 64), (1, 1024), (32, 64), (2, 1024), (16, 1024), (1, 16384)])
def test_lists_union_in_every_sort_tier(rows, width, dev):
    """Entry counts of 64, 1 024 (the one-key-per-thread sort), 2 048 (the first in-place tier) and exactly 16 384 (the last), two fused rows."""
    rng = np.random.default_rng(rows * width)
    lims = np.array([0, rows, 2 * rows])
    pos = rng.integers(0, 3 * rows * width, size=(2 * rows, width))
    pos[rows:] = np.arange(rows * width)[::-1].reshape(rows, width) * 5      # all distinct, descending: the count is the entry count
    counts = check_union(pos, lims, (1 << 32) - 1, dev, what=f"{rows} x {width}")
    assert counts[1] == rows * width


def test_lists_union_many_fused_rows_and_one(dev):
    rng = np.random.default_rng(7)
    sizes = 1 + (np.arange(40_000) % 3 == 1)
    lims = np.concatenate([[0], np.cumsum(sizes)])
    check_union(rng.integers(-1, 9, size=(int(lims[-1]), 2)), lims, 8, dev, what="U = 40 000")
    check_union(rng.integers(0, 50, size=(3, 7)), np.array([0, 3]), 50, dev, what="U = 1")


def test_lists_union_refusals(dev):
    pos = torch.zeros((4, 4097), dtype=torch.int64, device=dev)
    with pytest.raises(NotImplementedError, match=r"4 sub-query rows x 4097 candidates = 16388 entries.*16384"):
        E.lists_union(pos, torch.tensor([0, 4], device=dev), 100)
    with pytest.raises(NotImplementedError, match="2\\^32 - 2"):
        E.lists_union(pos[:, :4], torch.tensor([0, 4], device=dev), 1 << 32)
    with pytest.raises(ValueError, match=r"positions must be \(4, W\) int64"):
        E.lists_union(pos[:, :4].to(torch.int32), torch.tensor([0, 4], device=dev), 100)
    with pytest.raises(ValueError, match=r"out must be a contiguous \(1, >= 16\) int64"):
        E.lists_union(pos[:, :4], torch.tensor([0, 4], device=dev), 100, out=torch.empty((1, 15), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match=r"query_lims\[U\] = 3 but there are 4"):
        E.lists_union(pos[:, :4], torch.tensor([0, 3], device=dev), 100)


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------------
def fused_on(tk):
    tk.fuse_candidates = True
    return tk


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def positions_of_ids(ids_flat_np, ids):
    order = np.argsort(ids_flat_np, kind="stable")
    at = np.searchsorted(ids_flat_np[order], ids)
    assert np.array_equal(ids_flat_np[order][at], ids)
    return order[at]


class Reference:
    """What the contract says about one (module, queries, query_lims, allowed_tags): C_u from the module's own plain forward on the sub-query
    rows, s[r, x] from its own rerank on the union.  Computed once, shared by the modes, k and seen ids checked against it."""

    def __init__(self, tk, q, aux, lims, tags=None):
        self.lims = np.asarray(lims, dtype=np.int64)
        self.ids = tk._ids_flat.cpu().numpy()
        own = type(tk).forward is rails_amd.MoLAvgTopK.forward
        rows_of = np.repeat(np.arange(self.lims.size - 1), np.diff(self.lims))
        plain = dict(aux)
        if tags is not None:
            plain["allowed_tags"] = tags if isinstance(tags, int) else [int(tags[u]) for u in rows_of]
        tk.fuse_candidates = False
        _, cand_ids = tk(q, k=tk._avg_top_k if own else 1, **plain)      # Naive / Comb return every candidate's id; Avg does at k = avg_top_k
        tk.fuse_candidates = True
        cand_pos = positions_of_ids(self.ids, cand_ids.cpu().numpy().reshape(-1)).reshape(q.shape[0], -1)
        self.union, self.counts = R.union(cand_pos, self.lims, tk.num_items)
        per_row = torch.from_numpy(self.union[rows_of]).to(q.device)
        rerank = tk.rerank_masked if own else tk.rerank_union_masked
        s, i = (t.cpu().numpy() for t in rerank(q, per_row, per_row.shape[1], **aux))
        self.scores = np.full(per_row.shape, -np.inf, dtype=np.float32)
        for r, u in enumerate(rows_of):
            c = int(self.counts[u])
            assert (i[r] >= 0).sum() == c
            cols = np.searchsorted(self.union[u, :c], positions_of_ids(self.ids, i[r, :c]))
            self.scores[r, cols] = s[r, :c]
        self.rows_of = rows_of

    def walk(self, mode, weights, k, seen=None):
        return R.walk(self.union, self.counts, self.scores, self.lims, mode, weights, self.ids, k, None if seen is None else seen.cpu().numpy())


def fused_calls(tk, X, q, aux, lims, mode, weights, k, seen):
    """forward (seen is None) or get_top_k_outputs -> (ids, scores)"""
    kw = dict(aux, query_lims=lims, fuse=mode)
    if weights is not None:
        kw["query_weights"] = weights
    if seen is None:
        scores, ids = tk(q, k=k, **kw)
        return ids, scores
    cand = rails_amd.CandidateIndex(ids=tk._ids_flat.reshape(1, -1), embeddings=X.reshape(1, *X.shape[-2:]))
    return cand.get_top_k_outputs(q, k, kw, tk, seen)[:2]


def check_against(ref, tk, X, q, aux, mode, weights, k, seen, what, tags=None):
    lims = torch.from_numpy(ref.lims).to(q.device)
    kw = dict(aux) if tags is None else dict(aux, allowed_tags=tags)
    got_i, got_s = fused_calls(tk, X, q, kw, lims, mode, weights, k, seen)
    want_i, want_s = ref.walk(mode, None if weights is None else weights.cpu().numpy(), k, seen)
    assert got_i.shape == (ref.lims.size - 1, k) and got_s.dtype == q.dtype, what
    assert np.array_equal(got_i.cpu().numpy(), want_i), (what, "ids")
    assert np.array_equal(bits(got_s), want_s.view(np.uint32)), (what, "scores")
    return got_i, got_s


def seen_from(ref, tk, X, q, aux, width, g):
    """(U, width) seen ids: the fused "max" call's best items first (every fused row loses its best item), random ids behind them."""
    lims = torch.from_numpy(ref.lims).to(q.device)
    top = fused_calls(tk, X, q, aux, lims, "max", None, min(K, width), None)[0]
    rest = tk._ids_flat[torch.randint(0, tk.num_items, (top.shape[0], width - top.shape[1]), generator=g).to(q.device)]
    return torch.cat([top, rest], dim=1).contiguous()


def all_modes(tk, X, q, aux, lims, what, g, dense=None, tags=None):
    ref = Reference(tk, q, aux, lims, tags)
    kw = dict(aux) if tags is None else dict(aux, allowed_tags=tags)
    seen = seen_from(ref, tk, X, q, kw, W_SEEN, g)
    weights = torch.randn(q.shape[0], generator=g).to(q.device)
    for mode, weighted in MODES:
        w = weights if weighted else None
        got_i, _ = check_against(ref, tk, X, q, aux, mode, w, K, None, f"{what}: forward {mode} {weighted}", tags)
        filt_i, _ = check_against(ref, tk, X, q, aux, mode, w, K, seen, f"{what}: get_top_k_outputs {mode} {weighted}", tags)
        assert not bool((filt_i.unsqueeze(2) == seen.unsqueeze(1)).any()), what      # (row by row: a seen id of another fused row may be returned)
        if mode == "max":
            assert not torch.equal(got_i, filt_i), what      # the seen ids held every row's best item
    if dense is not None:      # the scores the walk fuses are all_logits' bits at the union's positions
        logits = dense.all_logits(q, **aux).cpu().numpy()
        for r, u in enumerate(ref.rows_of):
            c = int(ref.counts[u])
            assert np.array_equal(logits[r, ref.union[u, :c]].view(np.uint32), ref.scores[r, :c].view(np.uint32)), (what, r)
    return ref


def route_setup(kind, route, dev):
    """-> (tk with the switch on, X, q, aux, cfg, mol, make)"""
    if route == "generic":
        cfg, a, mol = candidate_module("g_8x8x40", dev)
        make = lambda x, i: generic_make(kind, mol, x, i)      # noqa: E731
        aux = {"user_ids": (torch.arange(S, dtype=torch.int64) * 7919 - 5).to(dev)} if "user_ids" in a else {}
    else:
        cfg, mol, _, aux = U.setup_route(kind, "f16x3" if route == "f16x3" else "default", dev)
        make = lambda x, i: H.MAKERS[kind](mol, x, i)      # noqa: E731
    n = N_FUSED if route == "fused" else N_SMALL
    X, ids = U.table(cfg, n, 8, dev), U.ids_of(n, dev)
    tk = fused_on(make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0)))
    if route == "materialised":
        H.routed(tk, H.MATERIALISED)
    q = O.synthetic_queries(cfg, S, seed=6).to(dev)
    return tk, X, q, aux, cfg, mol, make


@pytest.mark.parametrize("route", ["fused", "materialised", "f16x3", "generic"])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_calls_equal_the_reference_walk(kind, route, dev):
    """forward and get_top_k_outputs with max, sum and weighted sum on the fused-scan route (N = 300 007), the materialising route
    (N = 4 133, forced), a split-f16 engine and the generic route with generic_candidates = True.  On the fp32 routes the scores are a dense
    MoLBruteForceTopK's all_logits at the same positions."""
    g = torch.Generator().manual_seed(71)
    with torch.inference_mode():
        tk, X, q, aux, cfg, mol, make = route_setup(kind, route, dev)
        eng = tk._bind()
        if route == "fused":
            assert all(tk.num_items >= getattr(tk, name) for name in ("fused_coarse_min_items", "fused_component_min_items") if hasattr(tk, name))
        if route == "f16x3":
            assert eng.precision == "f16x3"
        if route == "generic":
            assert eng.route == "generic"
        dense = None
        if route in ("fused", "materialised"):
            assert eng.precision == "fp32" and eng.route != "generic"
            dense = rails_amd.MoLBruteForceTopK(mol, tk._item_embeddings, tk._item_ids, exact_mode="dense")
        assert tk.stats() == {}
        all_modes(tk, X, q, aux, LIMS, f"{kind} {route}", g, dense)
        assert tk.stats()["fused_candidate_calls"] >= 6


def small_setup(kind, dev, batch=S, min_items=H.MATERIALISED, n=N_SMALL):
    cfg, mol, aux, q = H.shape_setup("8x8x32", dev, batch)
    make = lambda x, i: fused_on(H.routed(H.MAKERS[kind](mol, x, i), min_items))      # noqa: E731
    X, ids = U.table(cfg, n, 7, dev), U.ids_of(n, dev)
    return make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), X, ids, q, aux, cfg, make


@pytest.mark.parametrize("kind", KINDS)
def test_hidden_set_and_allowed_tags_per_fused_row(kind, dev):
    """A random half of the corpus hidden; then allowed_tags= per FUSED row -- a shared word, and a (U,) tensor over 20 fused rows whose 41
    sub-query rows span two query tiles, on both scan routes."""
    g = torch.Generator().manual_seed(72)
    with torch.inference_mode():
        for min_items in (H.FUSED, H.MATERIALISED):
            tk, X, ids, q, aux, cfg, _ = small_setup(kind, dev, batch=41, min_items=min_items)
            sizes = np.array([1, 2, 3] * 6 + [2, 3])
            lims = np.concatenate([[0], np.cumsum(sizes)])
            assert lims[-1] == 41
            hidden = torch.randperm(N_SMALL, generator=g)[: N_SMALL // 2].to(dev)
            tk.hide_items(hidden)
            ref = all_modes(tk, X, q, aux, lims, f"{kind} hidden, min_items {min_items}", g)
            assert not np.isin(ref.union[ref.union >= 0], hidden.cpu().numpy()).any()
            tk.unhide_items(hidden)
            tags = tag_layout(N_SMALL, g).to(dev)
            tk.set_item_tags(tags)
            words = torch.tensor([(FIVE, ONE, TILES | FIVE, 0xFFFFFFFF)[u % 4] for u in range(20)])
            for allowed in (FIVE, words):
                ref = all_modes(tk, X, q, aux, lims, f"{kind} tags, min_items {min_items}", g, tags=allowed)
                per_row = [allowed] * 20 if isinstance(allowed, int) else allowed.tolist()
                for u in range(20):      # every candidate of fused row u carries one of its allowed bits
                    c = ref.union[u, : ref.counts[u]]
                    assert bool(((tags[torch.from_numpy(c).to(dev)] & per_row[u]) != 0).all()), (kind, u)
            with pytest.raises(ValueError, match="allowed_tags has 41 words but the batch has 20"):
                tk(q, k=K, query_lims=torch.from_numpy(lims).to(dev), allowed_tags=[FIVE] * 41, **aux)


@pytest.mark.parametrize("kind", KINDS)
def test_short_rows_wide_seen_lists_and_segments_of_one_row(kind, dev):
    g = torch.Generator().manual_seed(73)
    with torch.inference_mode():
        tk, X, ids, q, aux, cfg, _ = small_setup(kind, dev)
        ones = np.arange(S + 1)
        # segments of one row: the plain call's first k columns (the rows hold k distinct candidates)
        ref = Reference(tk, q, aux, ones)
        tk.fuse_candidates = False
        plain_s, plain_i = tk(q, k=K, **aux)
        tk.fuse_candidates = True
        for mode in ("max", "sum"):
            got_i, got_s = check_against(ref, tk, X, q, aux, mode, None, K, None, f"{kind} segments of one row, {mode}")
            assert torch.equal(got_i, plain_i[:, :K]) and torch.equal(got_s, plain_s[:, :K]), (kind, mode)
        # fewer than k candidates left: seen ids that hold most of every union -> the (-1, -inf) padding
        width = int(ref.counts.max())
        seen = torch.from_numpy(np.where(ref.union[:, :width] >= 0, ref.ids[np.clip(ref.union[:, :width], 0, None)], -5)).to(dev)
        seen[:, ::7] = -5      # every seventh candidate stays
        left = int((ref.counts + 6).min() // 7)
        got_i, got_s = check_against(ref, tk, X, q, aux, "max", None, K, seen.contiguous(), f"{kind} short rows")
        if left < K:
            assert bool((got_i[:, -1] == -1).all()) and bool(torch.isneginf(got_s[:, -1]).all()), kind
        # k + w beyond what the filtered selection launch takes (w > 256): top-(k + w) and the filter as two calls, the same bits
        ref = Reference(tk, q, aux, LIMS)
        wide = seen_from(ref, tk, X, q, aux, 300, g)
        for mode, weighted in MODES:
            w = torch.randn(S, generator=g).to(dev) if weighted else None
            check_against(ref, tk, X, q, aux, mode, w, K, wide, f"{kind} w = 300, {mode}")
            check_against(ref, tk, X, q, aux, mode, w, K, wide[:, :200].contiguous(), f"{kind} w = 200, {mode}")


@pytest.mark.parametrize("kind", KINDS)
def test_after_corpus_edits_equals_a_fresh_module(kind, dev):
    g = torch.Generator().manual_seed(74)
    with torch.inference_mode():
        tk, X, ids, q, aux, cfg, make = small_setup(kind, dev)
        lims = torch.tensor(LIMS, device=dev)
        more = U.table(cfg, 70, 19, dev, first=5_000_000)
        more_ids = U.ids_of(70, dev, first=9_000_000)
        tk(q, k=K, query_lims=lims, **aux)      # (the derived tables exist before the edits)
        tk.append_items(more, more_ids)
        tk.remove_items(torch.randperm(N_SMALL, generator=g)[:200].to(dev))
        fresh = make(tk._item_embeddings.clone(), tk._item_ids.clone().reshape(1, -1))
        assert fresh.num_items == tk.num_items == N_SMALL + 70 - 200
        seen = tk._ids_flat[torch.randint(0, tk.num_items, (NU, W_SEEN), generator=g).to(dev)]
        for mode, weighted in MODES:
            w = torch.randn(S, generator=g).to(dev) if weighted else None
            for sn in (None, seen):
                a = fused_calls(tk, tk._item_embeddings[0], q, aux, lims, mode, w, K, sn)
                b = fused_calls(fresh, fresh._item_embeddings[0], q, aux, lims, mode, w, K, sn)
                U.same(a, b, f"{kind} after append + remove, {mode} {weighted} {sn is None}")
        all_modes(tk, tk._item_embeddings[0], q, aux, LIMS, f"{kind} after edits", g)


@pytest.mark.parametrize("kind", KINDS)
def test_a_forced_redo_of_the_scans_gives_the_same_result(kind, dev, monkeypatch):
    """All but 2 K' items hidden with the routing rule switched off and the device-side redo refused: the fused scans raise their verdict word,
    the host reads it behind the whole fused call and the second attempt runs on the materialising route."""
    g = torch.Generator().manual_seed(75)
    verdicts = []
    real = T._verdicts_clear
    monkeypatch.setattr(T, "_verdicts_clear", lambda pending, module: verdicts.append(real(pending, module)) or verdicts[-1])
    with torch.inference_mode():
        tk, X, ids, q, aux, cfg, _ = small_setup(kind, dev, min_items=H.FUSED, n=H.N)
        twin, _, _, _, _, _, _ = small_setup(kind, dev, min_items=H.MATERIALISED, n=H.N)
        all_but = torch.ones(H.N, dtype=torch.bool)
        all_but[torch.randperm(H.N, generator=g)[: 2 * H.K_PRIME]] = False
        for m in (tk, twin):
            m.hide_items(torch.nonzero(all_but).reshape(-1).to(dev))
        tk.HIDDEN_FUSED_MIN_VISIBLE = 0.0
        tk.DEVICE_REDO_BYTES = 0
        lims = torch.tensor(LIMS, device=dev)
        seen = ids[~all_but.to(dev)][torch.randint(0, 2 * H.K_PRIME, (NU, W_SEEN), generator=g).to(dev)]
        for sn in (None, seen):
            del verdicts[:]
            got = fused_calls(tk, X, q, aux, lims, "sum", None, K, sn)
            if kind != "naive":      # (the component scan of these sizes redoes on the device: no verdict for the host)
                assert verdicts[:2] == [False, True], (kind, verdicts)
            U.same(got, fused_calls(twin, X, q, aux, lims, "sum", None, K, sn), f"{kind} redo")
            assert tk._no_fused is False


def test_refusals(dev):
    with torch.inference_mode():
        tk, X, ids, q, aux, cfg, make = small_setup("avg", dev)
        lims = torch.tensor(LIMS, device=dev)
        with pytest.raises(ValueError, match=r"avg_top_k \(100\) must be larger than k \(101\)"):
            tk(q, k=101, query_lims=lims, **aux)
        for extra in ({"collapse_groups": True}, {"max_per_group": 2}, {"diversify": 0.5}, {"item_mask": torch.ones(N_SMALL, dtype=torch.bool, device=dev)}):
            with pytest.raises(NotImplementedError, match="together with query_lims="):
                tk(q, k=K, query_lims=lims, **extra, **aux)
        for call in (lambda: tk.submit(q, K, query_lims=lims, **aux), lambda: tk.topk_ids(q, query_lims=lims, **aux),
                     lambda: tk.all_logits(q, query_lims=lims, **aux), lambda: tk.coarse_candidates(q, query_lims=lims, **aux)):
            with pytest.raises(NotImplementedError, match=r"MoLAvgTopK(\.\w+)? takes no query_lims"):
                call()
        assert tk.stats() == {}
        tk.fuse_candidates = False      # the parent's refusal, unchanged
        with pytest.raises(NotImplementedError, match=r"^MoLAvgTopK takes no query_lims: fusing several query rows per user is built on the single-device "
                                                      r"MoLBruteForceTopK and MIPSBruteForceTopK \(forward, get_top_k_outputs, all_logits and the streaming "
                                                      r"score calls\) only"):
            tk(q, k=K, query_lims=lims, **aux)
        # a segment over the 16 384-entry limit: 5 rows x 4 000 coarse candidates
        mol = tk._mol_module
        big = fused_on(rails_amd.MoLAvgTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), avg_top_k=4000))
        with pytest.raises(NotImplementedError, match=r"5 sub-query rows x 4000 candidates holds 20000 candidate entries, beyond the 16384"):
            big(q, k=K, query_lims=lims, **aux)
        ivf = rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), k_per_group=5, use_faiss=True, nlist=8)
        with pytest.raises(NotImplementedError, match=r"MoLNaiveTopK \(IVF, use_faiss=True\) takes no fuse_candidates"):
            ivf.fuse_candidates = True
        with pytest.raises(NotImplementedError, match=r"MoLNaiveTopK \(IVF, use_faiss=True\) takes no query_lims"):
            ivf(q, k=K, query_lims=lims, **aux)
