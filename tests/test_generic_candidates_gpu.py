"""The two-pass algorithms on the shape-generic scoring route (MoLSimilarity.generic_candidates = True), on the GPU:

  1. MoLAvgTopK / MoLNaiveTopK / MoLCombTopK construct and answer on a shape without a fused kernel
  2. candidates scored in place on the generic index (rails_mol_generic_score_indexed): the dense kernel's bits
  3. the bf16 tables cut from the generic index: the fused builders' bits on the forced route, the restatement of tests/_scan_ref.py on exact
     inputs, zero pad columns, update == rebuild
  4. the bf16 scans at the padded width: tests/_scan_ref.py fed the UNPADDED values, and fused top-k == materialised scores + key selection
  5. the modules against a plain-torch walk of the reference flow, fed the module's own scan scores and dense logits
  6. get_top_k_outputs, the hidden set, allowed_tags= and the corpus edits through the stack
  7. the sparse item_mask strategy of MoLBruteForceTopK
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rails_amd
from rails_amd import engine as E
from rails_amd import topk_modules as T
from tests import _generic_sweep as G
from tests import _mol_ref64 as R
from tests import _scan_ref as S
from tests.test_candidate_scans_gpu import bits, check_contract, ref_topk, same_bits, table_dev, to_dev
from tests.test_generic_route_gpu import CASES, _forced_cases, build_module, corpus, queries

pytestmark = pytest.mark.gpu

N_SMALL, N_LARGE = 300, 4096 + 37
INDEXED_CASES = ("g_4x4x64",                 # pair-gate weights resident in LDS
                 "g_16x8x32_h256",           # streamed weights
                 "g_12x3x20_h50_swiglu",     # L = 36: no multiple of 32; d = 20: dp = 24
                 "g_1x1x64",                 # odd P_Q
                 "g_8x8x40")
MODULE_CASES = ("g_8x8x40", "g_12x3x20_h50_swiglu")      # table widths 64 and 32
TABLE_CASES = MODULE_CASES + tuple(G.TABLE_SHAPES)      # and synthetic shapes at every width: d = 7 -> 32, 33 -> 64, 72 -> 128, 128 -> 128 (= d)
MASKED = -32767.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def candidate_module(name, dev):
    """-> (cfg, fixture arrays (None for a synthetic shape of tests/_generic_sweep.py), the candidate-capable module)"""
    if name in G.TABLE_SHAPES:
        cfg, w, a = G.config(G.TABLE_SHAPES[name]), G.weights(G.TABLE_SHAPES[name], "plain"), None
    else:
        cfg, w, a = CASES[name]
    mol = build_module(cfg, w, dev)
    mol.generic_candidates = True
    return cfg, a, mol


def make(kind, mol, X, ids):
    if kind == "avg":
        return rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=32)
    if kind == "naive":
        return rails_amd.MoLNaiveTopK(mol, X, ids, k_per_group=2)
    return rails_amd.MoLCombTopK(mol, X, ids, avg_top_k=32, k_per_group=2)


def ids_of(n, dev):
    return (torch.arange(n, dtype=torch.int64, device=dev) * 3 + 7).unsqueeze(0)


def route(tk, fused_scans):
    tk.fused_coarse_min_items = tk.fused_component_min_items = 0 if fused_scans else 1 << 62


# ---- 1. fails without the feature --------------------------------------------------------------------------------------------------
def test_the_two_pass_modules_run_on_a_shape_without_a_fused_kernel(dev):
    cfg, a, mol = candidate_module("g_8x8x40", dev)
    X, ids = corpus(cfg, N_SMALL).unsqueeze(0).to(dev), ids_of(N_SMALL, dev)
    q, kw = queries(cfg, a, 5, dev)
    L = cfg.query_dot_product_groups * cfg.item_dot_product_groups
    with torch.inference_mode():
        eng = mol.engine()
        assert eng.route == "generic" and eng.candidates and eng.score_indexed_supported(4, 64) and eng.table_width == 64
        for kind, width in (("avg", 10), ("naive", 2 * L), ("comb", 2 * L + 32)):
            s, i = make(kind, mol, X, ids)(q, k=10, **kw)
            assert s.shape == i.shape == (5, width), kind
            assert bool(torch.isfinite(s).all()) and bool(((i - 7) % 3 == 0).all()), kind
        # what the route still refuses, by name and before any launch
        with pytest.raises(NotImplementedError, match="use_faiss=True"):
            rails_amd.MoLNaiveTopK(mol, X, ids, k_per_group=2, use_faiss=True, nlist=4)
        tk = make("avg", mol, X, ids)
        with pytest.raises(NotImplementedError, match="generic scoring route"):
            tk.set_item_groups(torch.zeros(N_SMALL, dtype=torch.int64, device=dev))
        index = tk._index
        for call in (lambda: eng.build_index_rows(index), lambda: eng.gather_index(index, torch.zeros((1, 1), dtype=torch.int64, device=dev)),
                     lambda: eng.gate_rows(torch.empty(1, device=dev), 1), lambda: E.IvfIndex(eng, index)):
            with pytest.raises(NotImplementedError, match="generic scoring route"):
                call()
        assert tk._index_rows(eng) is None and eng.build_coarse_prefilter(tk._table()) is None
    mol.generic_candidates = False
    with pytest.raises(NotImplementedError, match="generic_candidates"):
        make("avg", mol, X, ids)


# ---- 2. indexed scoring ----------------------------------------------------------------------------------------------------------------
def _positions(B, K, n, seed):
    """Random positions with repeats; over the slots of each row in turn: position 0, n - 1, two inside the last partial tile, and one
    out-of-range position per row (past the end on even rows, negative on odd ones)."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.randint(0, n, (B, K), generator=g)
    if K > 2:
        pos[:, 2] = pos[:, 1]      # a repeat for certain
    special = [0, n - 1, n - 2, n - n % 32]
    for b in range(B):
        for j, p in enumerate(special):
            if j + 1 < K:
                pos[b, (b + j + 1) % K] = p
        pos[b, b % K] = n + 5 + b if b % 2 == 0 else -3 - b
    return pos


@pytest.mark.parametrize("name", INDEXED_CASES)
def test_indexed_scoring_has_the_dense_kernels_bits(name, dev):
    cfg, a, mol = candidate_module(name, dev)
    for n in (N_SMALL, N_LARGE):      # (the larger corpus puts many tiles between the positions of a row)
        assert n % 32 != 0
        with torch.inference_mode():
            eng = mol.engine()
            index = eng.build_index(corpus(cfg, n).to(dev))
            for B in (1, 5):
                q, kw = queries(cfg, a, B, dev)
                qpack, _, _ = eng.query_pack(q, kw.get("user_ids"))
                dense = eng.score_dense(qpack, B, index)
                for K in (1, 31, 32, 33, 200):
                    pos = _positions(B, K, n, 100 * B + K).to(dev)
                    want = torch.gather(dense, 1, pos.clamp(0, n - 1))      # an out-of-range position equals its clamped neighbour
                    got = eng.score_indexed(qpack, B, index, pos)
                    assert same_bits(got, want), (name, n, B, K, int((bits(got) != bits(want)).sum()))
                    assert same_bits(eng.score_indexed_rows(qpack, B, index.buf, n, pos), want), (name, n, B, K)
                    # counts: the slots below a row's count are written, those above keep the sentinel; ld > n_cand
                    counts = torch.tensor([(0, 1, 33, 128, K)[b % 5] for b in range(B)], dtype=torch.int32).clamp(max=K).to(dev)
                    if B == 1:
                        counts[0] = max(1, K - 1)
                    wide = torch.full((B, K + 9), -7.0, device=dev)
                    eng.score_indexed_rows(qpack, B, index.buf, n, pos, counts=counts, out=wide[:, :K])
                    live = torch.arange(K, device=dev)[None, :] < counts[:, None]
                    assert same_bits(wide[:, :K][live], want[live]) and bool((wide[:, :K][~live] == -7.0).all()) and bool((wide[:, K:] == -7.0).all()), (name, n, B, K)


# ---- 3. tables -------------------------------------------------------------------------------------------------------------------------
def test_tables_of_the_forced_route_equal_the_fused_routes(dev):
    n = 0
    for name, cfg, w, q, X, uid, ref in _forced_cases():
        fused_mol, forced = build_module(cfg, w, dev), build_module(cfg, w, dev, route="generic")
        forced.generic_candidates = True
        with torch.inference_mode():
            ef, eg = fused_mol.engine(), forced.engine()
            assert ef.route == "fused" and eg.route == "generic" and eg.candidates and eg.table_width == cfg.dot_product_dimension, name
            items = X[0].to(dev)
            fi, gi = ef.build_index(items), eg.build_index(items)
            for build in ("build_coarse_table", "build_component_table"):
                tf, tg = getattr(ef, build)(fi), getattr(eg, build)(gi)
                assert tf.shape == tg.shape and torch.equal(tf.view(torch.int16), tg.view(torch.int16)), (name, build)
        n += 1
    assert n == 3 + 4


def exact_index(eng, cfg, ex):
    """A generic index whose Ex is `ex` (N, P_X, d) exactly, written in the layout of mol_generic.h (gi zero): -> MolIndex."""
    n, px, d = ex.shape
    dp, lq = (d + 7) // 8 * 8, (cfg.query_dot_product_groups * px + 3) // 4 * 4
    rows = torch.zeros(((n + 31) // 32 * 32, px * dp + lq), dtype=torch.float32)
    rows[:n, : px * dp].view(n, px, dp)[:, :, :d] = torch.from_numpy(ex)
    assert rows.numel() == eng.lib.rails_mol_generic_index_floats(C.byref(eng.shape), n)
    return E.MolIndex(rows.reshape(-1).to(eng.device), n)


def gen_table_width(d):
    """mol_generic.h gen_table_width, restated: the smallest of 32 / 64 / 128 that holds d, 0 where none does"""
    return next((width for width in (32, 64, 128) if d <= width), 0)


@pytest.mark.parametrize("name", TABLE_CASES)
def test_tables_on_exact_inputs_and_their_update_form(name, dev):
    cfg, a, mol = candidate_module(name, dev)
    px, d = cfg.item_dot_product_groups, cfg.dot_product_dimension
    rng = np.random.default_rng(5)
    with torch.inference_mode():
        eng = mol.engine()
        dt = eng.table_width
        assert eng.route == "generic" and eng.candidates and dt == gen_table_width(d) and dt >= d
        assert dt > d or name == "s_2x3x128"      # (the one case whose width is d itself, on a shape without a fused kernel)
        for n in (N_SMALL, N_LARGE):
            ex = S.dyadic_rows(rng, n * px, d).reshape(n, px, d)      # bf16 numbers: the tables' first rounding is exact, the restatement does the rest
            index = exact_index(eng, cfg, ex)
            coarse, comp = eng.build_coarse_table(index), eng.build_component_table(index)
            assert coarse.shape == (n, dt) and comp.shape == (px, n, dt)
            assert same_bits(coarse[:, :d].float().cpu(), torch.from_numpy(S.coarse_table(ex))), (name, n)
            assert same_bits(comp[:, :, :d].float().cpu(), torch.from_numpy(S.component_table(ex))), (name, n)
            assert bool((coarse[:, d:].view(torch.int16) == 0).all()) and bool((comp[:, :, d:].view(torch.int16) == 0).all()), (name, n)
        # the update form, on a real corpus: rows 0, 31, 32 and N - 1 rewritten == a fresh build of the edited corpus
        n = N_SMALL
        X = corpus(cfg, n).to(dev)
        index = eng.build_index(X)
        coarse, comp = eng.build_coarse_table(index), eng.build_component_table(index)
        pos = torch.tensor([0, 31, 32, n - 1], dtype=torch.int64, device=dev)
        new = corpus(cfg, 4, seed=77).to(dev)
        X2 = X.clone()
        X2[pos] = new
        eng.update_index(index, pos, new)
        src = eng.update_source(index, new)
        eng.update_coarse_table(coarse, pos, src)
        eng.update_component_table(comp, pos, src)
        fresh = eng.build_index(X2)
        assert torch.equal(index.buf, fresh.buf)
        assert torch.equal(coarse.view(torch.int16), eng.build_coarse_table(fresh).view(torch.int16))
        assert torch.equal(comp.view(torch.int16), eng.build_component_table(fresh).view(torch.int16))
        changed = (coarse.view(torch.int16) != eng.build_coarse_table(eng.build_index(X)).view(torch.int16)).any(dim=1).nonzero().flatten()
        assert changed.tolist() == pos.tolist()      # the update wrote something, and nowhere else


# ---- 4. the scans at the padded width --------------------------------------------------------------------------------------------------
def padded_table(table, dt):
    """(.., d) fp32 holding bf16 values -> the (.., dt) bf16 device table with zero pad columns"""
    out = np.zeros(table.shape[:-1] + (dt,), dtype=np.float32)
    out[..., : table.shape[-1]] = table
    return table_dev(out)


def test_no_table_past_d_128_the_two_pass_modules_refuse(dev):
    """d = 129: table_width == 0.  A candidate-capable engine still scores positions in place; the three two-pass modules and the table
    builders refuse by name, at construction."""
    cfg, w = G.config(G.NO_TABLE), G.weights(G.NO_TABLE, "plain")
    assert gen_table_width(cfg.dot_product_dimension) == 0 and gen_table_width(128) == 128
    mol = build_module(cfg, w, dev)
    mol.generic_candidates = True
    X, ids = corpus(cfg, N_SMALL).unsqueeze(0).to(dev), ids_of(N_SMALL, dev)
    with torch.inference_mode():
        eng = mol.engine()
        assert eng.route == "generic" and eng.candidates and eng.table_width == 0
        for kind in ("avg", "naive", "comb"):
            with pytest.raises(NotImplementedError, match=r"dot_product_dimension <= 128 .* got d = 129"):
                make(kind, mol, X, ids)
        index = eng.build_index(X[0])
        for call in (lambda: eng.build_coarse_table(index), lambda: eng.build_component_table(index), lambda: eng.update_source(index, X[0, :1])):
            with pytest.raises(NotImplementedError, match=r"dot_product_dimension <= 128 .* got d = 129"):
                call()
        # what does not need a table runs: positions scored in place carry the dense bits
        q = torch.from_numpy(np.random.default_rng(9).standard_normal((3, cfg.query_embedding_dim)).astype(np.float32)).to(dev)
        qpack, _, _ = eng.query_pack(q, None)
        pos = _positions(3, 45, N_SMALL, 5).to(dev)
        assert same_bits(eng.score_indexed(qpack, 3, index, pos), torch.gather(eng.score_dense(qpack, 3, index), 1, pos.clamp(0, N_SMALL - 1)))


@pytest.mark.parametrize("name", TABLE_CASES)
def test_scan_scores_equal_the_restatement_fed_the_unpadded_values(name, dev):
    cfg, a, mol = candidate_module(name, dev)
    pq, px, d = cfg.query_dot_product_groups, cfg.item_dot_product_groups, cfg.dot_product_dimension
    rng = np.random.default_rng(6)
    with torch.inference_mode():
        eng = mol.engine()
        for B, n in ((1, 33), (5, N_SMALL), (33, 1000)):
            eq = S.dyadic_eq(rng, B, pq, d)
            coarse = S.dyadic_rows(rng, n, d)
            ex = S.dyadic_rows(rng, n * px, d).reshape(n, px, d)
            comp = S.component_table(ex)
            comp_d = eng.build_component_table(exact_index(eng, cfg, ex))      # through the builder: bf16(Ex) is Ex here
            assert same_bits(comp_d[:, :, :d].float().cpu(), torch.from_numpy(comp))
            for avg in (False, True) if pq & (pq - 1) == 0 else (False,):      # (sum / P_Q is dyadic for a power of two only)
                S.assert_exact(S.coarse_query(eq, avg), coarse, 6 + (pq.bit_length() - 1 if avg else 0))
                want = torch.from_numpy(S.rounded(S.coarse_scores(eq, coarse, avg)[0]))
                got = eng.coarse_scores(to_dev(eq), padded_table(coarse, eng.table_width), avg)
                assert same_bits(got.cpu(), want), (name, B, n, avg)
            S.assert_exact(S.component_query(eq), comp, 6)
            want = torch.from_numpy(S.rounded(S.component_scores(eq, comp)[0]))
            assert same_bits(eng.component_scores(to_dev(eq), comp_d).cpu(), want), (name, B, n)


def smallest_fused(fn, lo=1, hi=1 << 20):
    """the smallest n in [lo, hi] with fn(n) != 0, by a doubling walk and a bisection of the first non-zero bracket"""
    n = lo
    while n <= hi and fn(n) == 0:
        n *= 2
    assert n <= hi
    a, b = max(lo, n // 2), n
    while a < b:
        m = (a + b) // 2
        if fn(m) != 0:
            b = m
        else:
            a = m + 1
    return a


def visible_words(n, hidden, dev):
    return E.visibility_edit(E.visibility_row(n, dev), n, hidden.to(dev), False)[0]


@pytest.mark.parametrize("name", MODULE_CASES)
def test_fused_topk_equals_materialised_scores_and_key_selection(name, dev):
    cfg, a, mol = candidate_module(name, dev)
    pq, px = cfg.query_dot_product_groups, cfg.item_dot_product_groups
    B = 5
    with torch.inference_mode():
        eng = mol.engine()
        lib, shape = eng.lib, eng.scan_shape
        q, kw = queries(cfg, a, B, dev)
        _, eq, _ = eng.query_pack(q, kw.get("user_ids"), want_plain=True)
        for entry, k in (("coarse", 16), ("component", 2)):
            ws = lib.rails_mol_coarse_topk_workspace_bytes if entry == "coarse" else lib.rails_mol_component_topk_workspace_bytes
            n = smallest_fused(lambda m: ws(C.byref(shape), B, m, k), lo=k) + 37
            index = eng.build_index(corpus(cfg, n, seed=8).to(dev))
            table = eng.build_coarse_table(index) if entry == "coarse" else eng.build_component_table(index)
            scores = (eng.coarse_scores(eq, table, False) if entry == "coarse" else eng.component_scores(eq, table)).cpu()
            rows, per = scores.shape[0], scores.shape[0] // B
            # unrestricted; a hidden set of a random half; one allow word per query row over two random 55 % halves that overlap in 10 %
            # (every item carries a bit, words 1 and 2 keep 55 %, word 3 everything).  Every row keeps at least half the corpus, which is
            # what hidden_scan_route / tagged_scan_route ask before they expect the fused threshold to hold -- asserted below, so that
            # flag == 0 may be demanded: the redo would hide a wrong restricted kernel behind a right answer.
            order = torch.randperm(n, generator=torch.Generator().manual_seed(31))
            hidden = order[: n // 2].sort().values
            tags = torch.zeros(n, dtype=torch.int64)
            tags[order[: n * 11 // 20]] |= 1
            tags[order[n * 9 // 20:]] |= 2
            words = (1, 2, 3, 1, 2)
            kept_tags = tuple(int(((tags & w) != 0).sum()) for w in words)
            filt = E.TagFilter(tags.to(torch.int32).to(dev), words, kept_tags)
            plan = E.scan_plan(B if entry == "coarse" else rows, n, k, 0 if entry == "coarse" else B * pq)
            assert T.hidden_scan_route(n, n - hidden.numel(), k) == "fused" and T.tagged_scan_route(plan, min(kept_tags), n, k) == "fused", (name, entry, n)
            for what, restr in (("plain", {}), ("visible", {"visible": visible_words(n, hidden, dev)}), ("tags", {"tags": filt})):
                ms = scores.clone()
                kept = torch.full((rows,), n)
                if what == "visible":
                    ms[:, hidden] = float("-inf")
                    kept[:] = n - hidden.numel()
                if what == "tags":
                    keep = (tags[None, :] & torch.tensor(words)[:, None]) != 0      # (B, n)
                    ms[~keep.repeat_interleave(per, dim=0)] = float("-inf")
                    kept = torch.tensor(kept_tags).repeat_interleave(per)
                ref_s, ref_p = ref_topk(lambda r0, r1: ms[r0:r1].numpy(), rows, k)
                if entry == "coarse":
                    out = eng.coarse_topk(eq, table, False, k, with_flag=True, **restr)
                    assert out is not None, (name, n)
                    fs, fp, counts, flag = out
                    cap = eng.coarse_topk_capacity(k, n, B)
                else:
                    flag = torch.ones(1, dtype=torch.int32, device=dev)
                    out = eng.component_topk(eq, table, k, flag, **restr)
                    assert out is not None, (name, n)
                    fs, fp, counts = out
                    cap = eng.component_topk_capacity(B, n, k)
                # what flag == 0 is relied on for (tests/test_item_tags_gpu.py ties_at): the items at or above the k-th masked score, its
                # tied run included, fit the candidate lists
                at_or_above = (ms >= ref_s[:, k - 1 : k]).sum(dim=1)
                assert int(at_or_above.max()) <= cap, (name, entry, what, int(at_or_above.max()), cap)
                counts = counts.cpu()
                print(name, entry, what, "n", n, "flag", int(flag.item()), "counts", int(counts.min()), int(counts.max()), "cap", cap, "kept", int(kept.min()))
                assert int(flag.item()) == 0 and k <= int(counts.min()) and bool((counts <= kept.clamp(max=cap)).all()), (name, entry, what)
                ok = check_contract((fs.cpu(), fp.cpu(), counts, int(flag.item()), cap), ref_s, ref_p, k)
                assert bool(ok.all()), (name, entry, what, int(ok.sum()), rows)      # every row, the filtering ones among them, bit for bit


# ---- 5. the modules --------------------------------------------------------------------------------------------------------------------
def key_topk(scores, k):
    """positions of the k largest (score desc, position asc)"""
    return torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :k]


def rank_by_score_then_position(pos, scores):
    pos, perm = torch.sort(pos, dim=1)
    scores = torch.gather(scores, 1, perm)
    scores, order = torch.sort(scores, dim=1, descending=True, stable=True)
    return scores, torch.gather(pos, 1, order)


def walk(kind, coarse, coarse_avg, comp, dense, B, k):
    """The reference flow (mol_top_k.py:247-287, :351-420, :508-513) in plain torch on the module's own scan scores and dense logits."""
    if kind == "avg":
        cand = key_topk(coarse, 32)
        s, p = rank_by_score_then_position(cand, torch.gather(dense, 1, cand))
        return s[:, :k], p[:, :k]
    lists = [key_topk(comp, 2).reshape(B, -1)]
    if kind == "comb":
        lists.append(key_topk(coarse_avg, 32))
    union = torch.sort(torch.cat(lists, dim=1), dim=1).values
    s = torch.gather(dense, 1, union)
    s[:, 1:][union[:, 1:] == union[:, :-1]] = MASKED
    return rank_by_score_then_position(union, s)


@pytest.mark.parametrize("name", MODULE_CASES)
def test_modules_against_the_reference_flow(name, dev):
    cfg, a, mol = candidate_module(name, dev)
    B, k = 5, 10
    q, kw = queries(cfg, a, B, dev)
    for n in (N_SMALL, N_LARGE):
        X, ids = corpus(cfg, n).unsqueeze(0).to(dev), ids_of(n, dev)
        with torch.inference_mode():
            eng = mol.engine()
            for kind in ("avg", "naive", "comb"):
                tk = make(kind, mol, X, ids)
                qpack, eq, _ = eng.query_pack(q, kw.get("user_ids"), want_plain=True)
                dense = eng.score_dense(qpack, B, tk._index).cpu()
                coarse = coarse_avg = comp = None
                if kind != "naive":
                    coarse, coarse_avg = eng.coarse_scores(eq, tk._table(), False).cpu(), eng.coarse_scores(eq, tk._table(), True).cpu()
                if kind != "avg":
                    comp = eng.component_scores(eq, tk._component_table()).cpu()
                want_s, want_p = walk(kind, coarse, coarse_avg, comp, dense, B, k)
                route(tk, False)
                s, i = tk(q, k=k, **kw)
                pos = ((i - 7) // 3).cpu()
                real = s.cpu() != MASKED
                assert same_bits(s.cpu()[real], torch.gather(dense, 1, pos)[real]), (name, kind, n)      # the dense kernel's bits at the returned ids
                assert same_bits(s.cpu(), want_s) and torch.equal(pos, want_p), (name, kind, n)
                if n == N_LARGE:      # the fused scans (their plans take these sizes) == the materialising route
                    if kind != "naive":
                        assert eng.coarse_topk(eq, tk._table(), False, 32) is not None
                    if kind != "avg":
                        assert eng.component_topk(eq, tk._component_table(), 2, torch.zeros(1, dtype=torch.int32, device=dev)) is not None
                    route(tk, True)
                    fs, fi = tk(q, k=k, **kw)
                    assert same_bits(fs, s) and torch.equal(fi, i), (name, kind)
                    # submit / result is MoLAvgTopK's pair on every route; MoLNaiveTopK and MoLCombTopK answer through the synchronous
                    # two-attempt forward above and have no asynchronous form of their own
                    h = tk.submit(q, k, **kw) if kind == "avg" else None
                    if h is not None:
                        hs, hi = tk.result(h)
                        assert same_bits(hs, s) and torch.equal(hi, i), (name, kind)


def _by_position(scores, ids, n):
    """(B, n) fp32: the score a row returned for each position, NaN where it returned none (masked duplicates dropped)"""
    pos = (ids - 7) // 3
    out = torch.full((scores.shape[0], n + 1), float("nan"), dtype=torch.float64, device=scores.device)
    out.scatter_(1, torch.where(scores == MASKED, torch.full_like(pos, n), pos), scores.double())
    return out[:, :n].cpu()


def test_forced_route_modules_on_the_fused_fixtures(dev):
    """The candidates come from bit-equal tables and bit-equal Eq, so both routes generate the same positions; their final scores differ by
    the two scoring kernels' rounding, inside the sum of their score64 bounds (the bar of test_forced_route_on_fused_shapes)."""
    n = N_SMALL
    done = 0
    for name, cfg, w, q, X_fix, uid, ref in _forced_cases():
        kw = {} if uid is None else {"user_ids": uid.to(dev)}
        q = q.to(dev)
        B = q.shape[0]
        fused_mol, forced = build_module(cfg, w, dev), build_module(cfg, w, dev, route="generic")
        forced.generic_candidates = True
        X, ids = corpus(cfg, n).unsqueeze(0).to(dev), ids_of(n, dev)
        with torch.inference_mode():
            bounds = []
            for m in (fused_mol, forced):
                eng = m.engine()
                _, eq, gq = eng.query_pack(q, kw.get("user_ids"), want_plain=True)
                ex, gi = eng.unpack_index(eng.build_index(X[0]))
                bounds.append(R.score64(cfg, w, eq, ex, gq, gi)[1])
            bound = bounds[0] + bounds[1]
            for kind in ("avg", "naive", "comb"):
                tf, tg = make(kind, fused_mol, X, ids), make(kind, forced, X, ids)
                assert tf._bind().route == "fused" and tg._bind().route == "generic"
                cf = tf.coarse_candidates(q, **kw) if kind == "avg" else tf.local_candidates(q, **kw)
                cg = tg.coarse_candidates(q, **kw) if kind == "avg" else tg.local_candidates(q, **kw)
                for x, y in zip(cf, cg):      # scan scores and positions, best first: equal as lists, hence as sets
                    assert torch.equal(x, y), (name, kind)
                sf, idf = tf(q, k=32, **kw)
                sg, idg = tg(q, k=32, **kw)
                pf, pg = _by_position(sf, idf, n), _by_position(sg, idg, n)
                assert torch.equal(torch.isnan(pf), torch.isnan(pg)), (name, kind)
                have = ~torch.isnan(pf)
                assert bool(((pf - pg).abs()[have] <= bound[have]).all()), (name, kind, float((pf - pg).abs()[have].max()))
        done += 1
    assert done == 3 + 4


# ---- 6. through the stack --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stack_inputs(n):
    cfg, w, a = CASES["g_8x8x40"]
    return corpus(cfg, n, seed=12), torch.from_numpy(np.random.default_rng(13).integers(1, 8, size=n))      # rows, tags (3 bits, never 0)


@pytest.mark.parametrize("kind", ("avg", "naive", "comb"))
def test_seen_ids_hidden_items_and_allowed_tags(kind, dev):
    cfg, a, mol = candidate_module("g_8x8x40", dev)
    n, B, k = N_LARGE, 5, 10
    rows, tags = _stack_inputs(n)
    X, ids = rows.unsqueeze(0).to(dev), ids_of(n, dev)
    q, kw = queries(cfg, a, B, dev)
    with torch.inference_mode():
        for fused_scans in (False, True):
            tk = make(kind, mol, X, ids)
            route(tk, fused_scans)
            # get_top_k_outputs with seen ids == forward + filter_seen_ids
            s, i = tk(q, k=k + 4, **kw)
            seen = i[:, :4].contiguous()
            ci = rails_amd.CandidateIndex(ids=ids, embeddings=X)
            got_i, got_s, _ = ci.get_top_k_outputs(q, k, dict(kw), tk, seen)
            want_i, want_s = E.filter_seen_ids(i, s, seen, k)
            assert torch.equal(got_i, want_i) and same_bits(got_s, want_s), (kind, fused_scans)
            # a hidden set: the module freshly constructed from the visible rows and ids
            hidden = torch.cat([torch.arange(0, n, 7), ((i[0, :3] - 7) // 3).cpu()]).unique()
            tk.hide_items(hidden)
            keep = torch.ones(n, dtype=torch.bool)
            keep[hidden] = False
            twin = make(kind, mol, X[:, keep.to(dev)], ids[:, keep.to(dev)])
            route(twin, fused_scans)
            hs, hi = tk(q, k=k, **kw)
            ts, ti = twin(q, k=k, **kw)
            assert same_bits(hs, ts) and torch.equal(hi, ti), (kind, fused_scans, "hidden")
            tk.unhide_items(hidden)
            # per-row allowed_tags: row b against the fresh module of the items row b may return
            tk.set_item_tags(tags.to(dev))
            words = [1, 2, 4, 3, 1]
            fs, fi = tk(q, k=k, allowed_tags=words, **kw)
            for word in sorted(set(words)):
                keep = ((tags & word) != 0).to(dev)
                twin = make(kind, mol, X[:, keep], ids[:, keep])
                route(twin, fused_scans)
                ts, ti = twin(q, k=k, **kw)
                rows_b = [b for b, v in enumerate(words) if v == word]
                assert same_bits(fs[rows_b], ts[rows_b]) and torch.equal(fi[rows_b], ti[rows_b]), (kind, fused_scans, "tags", word)


@pytest.mark.parametrize("kind", ("avg", "naive", "comb"))
def test_a_chain_of_corpus_edits_equals_a_fresh_module(kind, dev):
    cfg, a, mol = candidate_module("g_8x8x40", dev)
    n, B, k = N_SMALL, 5, 10
    D = cfg.item_embedding_dim
    X, ids = corpus(cfg, n).unsqueeze(0).to(dev), ids_of(n, dev)
    q, kw = queries(cfg, a, B, dev)
    new = corpus(cfg, 64, seed=21).to(dev)
    with torch.inference_mode():
        tk = make(kind, mol, X.clone(), ids.clone())
        tk(q, k=k, **kw)      # every derived buffer is held from here on
        tk.update_items(torch.tensor([0, 31, 32, n - 1]), new[:4])
        tk.append_items(new[4:44], torch.arange(40, dtype=torch.int64, device=dev) + 100_000)      # 300 -> 340: across the tile boundary at 320
        tk.remove_items(torch.tensor([5, 100, 330]))                                              # 337 left: the movers come out of the last tile
        tk.upsert_items(torch.tensor([7 + 3 * 10, 100_001, 200_000, 200_001], device=dev), new[44:48])      # two held ids, two new ones
        assert tk.num_items == 339
        fresh = make(kind, mol, tk._item_embeddings.clone(), tk._item_ids.clone())
        s, i = tk(q, k=k, **kw)
        fs, fi = fresh(q, k=k, **kw)
        assert same_bits(s, fs) and torch.equal(i, fi), kind
        assert torch.equal(tk._index.buf, fresh._index.buf), kind
        if kind != "naive":
            assert tk._coarse_table is not None and torch.equal(tk._coarse_table.view(torch.int16), fresh._table().view(torch.int16)), kind
        if kind != "avg":
            assert tk._comp_table is not None and torch.equal(tk._comp_table.view(torch.int16), fresh._component_table().view(torch.int16)), kind


# ---- 7. the sparse item_mask strategy ---------------------------------------------------------------------------------------------------
def test_sparse_item_mask_strategy_on_a_candidate_capable_engine(dev):
    cfg, a, mol = candidate_module("g_8x8x40", dev)
    plain = build_module(*CASES["g_8x8x40"][:2], dev)
    n, B, k = N_LARGE, 5, 10
    X, ids = corpus(cfg, n).unsqueeze(0).to(dev), ids_of(n, dev)
    q, kw = queries(cfg, a, B, dev)
    g = torch.Generator().manual_seed(3)
    shared = torch.rand(n, generator=g) < 0.1
    per_row = torch.rand(B, n, generator=g) < torch.tensor([0.02, 0.05, 0.1, 0.15, 0.2])[:, None]      # ragged counts
    with torch.inference_mode():
        sparse, dense = rails_amd.MoLBruteForceTopK(mol, X, ids), rails_amd.MoLBruteForceTopK(plain, X, ids)
        for mask in (shared, per_row):
            s, i = sparse(q, k=k, item_mask=mask.to(dev), **kw)
            ds, di = dense(q, k=k, item_mask=mask.to(dev), **kw)
            assert same_bits(s, ds) and torch.equal(i, di)
        assert sparse.rescore_stats.get("masked_sparse_calls") == 2 and not sparse.rescore_stats.get("masked_dense_calls")
        assert dense.rescore_stats.get("masked_dense_calls") == 2 and not dense.rescore_stats.get("masked_sparse_calls")
