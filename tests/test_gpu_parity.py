"""GPU parity: the HIP path (through the C ABI) against the golden vectors and the oracle."""
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from tests._fixtures import PER_CONFIG, Fixture, assert_topk_matches, full_size_inputs, tie_branch_census

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-4   # BASELINE.json north_star: "within 1e-4 on MoL logits"
STAGE_TOL = 2e-6   # unit-norm embeddings / O(1) gates: a few ulp of summation-order noise

SUPPORTED = ["c1_ml1m", "c2_ml20m", "c3_books", "c4_16x16x64"]


PRECISIONS = ["fp32", "f16x3"]   # every scoring test runs on both builds of the fused kernel, against the same vectors and bar


def build_module(cfg, weights, dev, precision=None):
    mol = _build_module(cfg, weights, dev)
    mol.precision = precision
    return mol


def _build_module(cfg, weights, dev):
    mol, _ = rails_amd.create_mol_interaction_module(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
        cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
        cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
        query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None,
    )
    mol.load_state_dict(weights, strict=True)
    return mol.to(dev).eval()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=SUPPORTED)
def fx(request):
    return Fixture(request.param)


@pytest.fixture(scope="module", params=PRECISIONS)
def mol(fx, dev, request):
    return build_module(fx.cfg, fx.weights, dev, request.param)


def kw_dev(fx, dev):
    return {k: v.to(dev) for k, v in fx.kw.items()}


def test_f1_stages(fx, mol, dev):
    n = int(fx.z["F1/n"])
    q, X = fx.t("q").to(dev), fx.t("X")[:, :n].to(dev)
    with torch.inference_mode():
        eq, _ = mol.get_query_component_embeddings(q, **kw_dev(fx, dev))
        ex, _ = mol.get_item_component_embeddings(X)
        eng = mol.engine()
        _, _, gq = eng.query_pack(q, fx.user_ids, want_plain=True) if fx.user_ids is None else eng.query_pack(q, fx.user_ids.to(dev), want_plain=True)
        _, gi = eng.unpack_index(eng.build_index(X[0]), want_ex=False)
        logits, aux = mol(q, X, **kw_dev(fx, dev))
    assert aux == {}
    for name, got, tol in (("Eq", eq, STAGE_TOL), ("Ex", ex, STAGE_TOL), ("gq", gq, 1e-5), ("gi", gi.unsqueeze(0), 1e-5), ("logits", logits, LOGIT_TOL)):
        ref = fx.t("F1/" + name)
        d = float((got.cpu().reshape(ref.shape) - ref).abs().max())
        assert d <= tol, f"{fx.name}:{name} max|d| = {d}"


def test_f2_brute_force_topk(fx, mol, dev):
    X, ids = fx.t("X").to(dev), fx.t("item_ids").to(dev)
    N = X.shape[1]
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
        logits = tk.all_logits(fx.t("q").to(dev), **kw_dev(fx, dev))
        d = float((logits.cpu() - fx.t("F2/all_logits")).abs().max())
        assert d <= LOGIT_TOL, d
        for k in (10, 200, N):
            s, i = tk(fx.t("q").to(dev), k=k, **kw_dev(fx, dev))
            assert s.shape == (fx.t("q").shape[0], k) and i.dtype == torch.int64
            assert_topk_matches(s, i, fx.t(f"F2/k{k}/scores"), fx.t(f"F2/k{k}/ids"), atol=LOGIT_TOL)
        with pytest.raises(RuntimeError):
            tk(fx.t("q").to(dev), k=N + 1, **kw_dev(fx, dev))


@pytest.mark.parametrize("case", ["timing", "accuracy", "backfill", "nofilter"])
def test_f3_candidate_index(fx, mol, dev, case):
    X, ids = fx.t("X").to(dev), fx.t("item_ids").to(dev)
    k = int(fx.z[f"F3/{case}/k"])
    trunc = int(fx.z[f"F3/{case}/truncate"])
    inv = fx.t(f"F3/{case}/invalid_ids").to(dev) if fx.has(f"F3/{case}/invalid_ids") else None
    with torch.inference_mode():
        ci = rails_amd.CandidateIndex(ids=ids, embeddings=X)
        tk = rails_amd.get_top_k_module("MoLBruteForceTopK", type("M", (), {"_ndp_module": mol})(), X, ids)
        r_ids, r_scores, r_emb = ci.get_top_k_outputs(
            query_embeddings=fx.t("q").to(dev), k=k, aux_payloads=kw_dev(fx, dev), top_k_module=tk, invalid_ids=inv,
            return_embeddings=False, truncate_k_prime_to=None if trunc < 0 else trunc)
    assert r_emb is None
    assert_topk_matches(r_scores, r_ids, fx.t(f"F3/{case}/scores"), fx.t(f"F3/{case}/ids"), atol=LOGIT_TOL)


def test_f6_per_row_candidates(fx, mol, dev):
    X = fx.t("X").squeeze(0)
    cand = X[fx.t("F6/cand_idx")].to(dev)   # (B, 48, D): 48 is not a multiple of 32 -> padded tile
    with torch.inference_mode():
        got, _ = mol(fx.t("q").to(dev), cand, **kw_dev(fx, dev))
    d = float((got.cpu() - fx.t("F6/logits")).abs().max())
    assert d <= LOGIT_TOL, d


def test_f5_harness_metrics(dev):
    fx = Fixture("harness")
    mol = build_module(fx.cfg, fx.weights, dev)
    X, ids, q = fx.t("X").to(dev), fx.t("item_ids").to(dev), fx.t("q").to(dev)
    past, target = fx.t("past_ids"), fx.t("target_ids")
    N = X.shape[1]
    with torch.inference_mode():
        ci = rails_amd.CandidateIndex(ids=ids, embeddings=X)
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
        for mode, max_k, trunc in (("accuracy", 2500, None), ("timing", 120, 200)):
            k = min(max_k, N)
            top_ids, top_scores, _ = ci.get_top_k_outputs(q, k, {}, tk, past.to(dev), truncate_k_prime_to=trunc)
            ref_ids = fx.t(f"F5/{mode}/eval_top_k_ids")
            # ids -> ranks -> HR/NDCG/MRR: identical ids give identical metrics
            m = O.eval_metrics(top_ids.cpu(), target, max_k)
            ref_m = O.eval_metrics(ref_ids, target, max_k)
            assert torch.equal(m["rank"], ref_m["rank"])
            for key in ("hr@1", "hr@10", "hr@50", "hr@100"):
                assert torch.equal(m[key], fx.t(f"F5/{mode}/{key}")), key
            assert torch.allclose(m["mrr"].float(), fx.t(f"F5/{mode}/mrr").float(), atol=1e-7)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["full_c1_ml1m", "full_c2_ml20m", "full_c3_books"])
def test_f7_full_size(name, dev, precision):
    """MoLBruteForceTopK's default route against the REFERENCE's own output at the corpora's full sizes.  full_c3_books (round 6): all
    695 762 items of the headline workload -- the default route there is the PROVED flow (split-f16 first pass, fused tail), compared
    here with what rails.indexing.mol_top_k.MoLBruteForceTopK itself returned (oracle/gen_golden.py), not with another HIP kernel."""
    fx = Fixture(name)
    mol = build_module(fx.cfg, fx.weights, dev, precision)
    X, ids = full_size_inputs(fx)
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X.to(dev), ids.to(dev))
        s, i = tk(fx.t("q").to(dev), k=200, **kw_dev(fx, dev))
        logits = tk.all_logits(fx.t("q").to(dev), **kw_dev(fx, dev))
    assert_topk_matches(s, i, fx.t("scores"), fx.t("ids"), atol=LOGIT_TOL)
    # how much of "ids identical modulo ties" rests on the tie rule, at the survey's tolerance (1e-5) and at the one the comparison
    # uses (2e-5 = the measured logit error): a handful of the 6 400 positions differ at all, none outside a run of near-equal
    # reference scores at either tolerance (tools/tie_branch_census.py records the counts: profiles/r04_tie_branch_census.json)
    for tol in (1e-5, 2e-5):
        c = tie_branch_census(i, fx.t("scores"), fx.t("ids"), tol)
        assert c["positions_differing"] <= 0.01 * c["rows"] * c["k"] and c["positions_outside_tie_runs"] == 0, c
    if "logits_first_row" in fx.z:
        assert float((logits[0].cpu() - fx.t("logits_first_row")).abs().max()) <= LOGIT_TOL
    assert float((logits.double().sum(1).cpu() - fx.t("logits_rowsum_f64")).abs().max()) <= LOGIT_TOL * logits.shape[1] * 0.05
    if name == "full_c3_books" and precision == "fp32":
        st = tk.stats()
        print("full_c3_books through the default route:", {key: st.get(key) for key in ("calls", "proved_calls", "fallbacks", "kc", "eps", "eps_rigorous", "bound_kind")})
        assert tk._bind().exact is not None and st["calls"] == 1 and st["proved_calls"] + st["fallbacks"] == 1 and st["bound_violations"] == 0, st      # the proved flow answered (proved, or redone behind its verdict)


# ---- selection kernels on their own ---------------------------------------------------------------
@pytest.mark.parametrize("rows,n,k", [(1, 1, 1), (3, 37, 5), (4, 1000, 1000), (2, 16384, 300), (5, 16385, 200),
                                      (32, 100000, 2711), (1, 3000000, 16384), (7, 70001, 1),
                                      # single-launch register-resident select: every per-thread width and both edges
                                      (3, 1025, 200), (4, 4096, 4096), (2, 8193, 17), (3, 27278, 200), (3, 30000, 1),
                                      (2, 40960, 4096), (2, 40961, 100), (2, 9000, 5000), (2, 3883, 3883),
                                      # two-level (per-chunk winners, then their winners): 2 .. 74 chunks
                                      (4, 695762, 200), (3, 86971, 200), (2, 3000000, 200), (3, 81921, 512),
                                      (2, 3400000, 200), (1, 4500000, 200), (2, 49152, 300), (2, 49153, 300),
                                      # the in-LDS sort at 8 keys per thread (the whole row, 8 192 slots) and at 2 (the radix path's 2 048 candidate slots)
                                      (2, 5000, 4500), (2, 200000, 1500)])
def test_topk_matches_deterministic_rule(dev, rows, n, k):
    g = torch.Generator().manual_seed(rows * 1000003 + n)
    scores = torch.randn((rows, n), generator=g)
    s, i = E.topk(scores.to(dev), k)
    rs, ri = O.select_topk_deterministic(scores, k)
    assert torch.equal(s.cpu(), rs) and torch.equal(i.cpu(), ri)


@pytest.mark.parametrize("n", [5000, 30000, 200000])
def test_topk_with_heavy_ties_is_position_ordered(dev, n):
    g = torch.Generator().manual_seed(n)
    scores = torch.randint(0, 7, (6, n), generator=g).float() - 3.0   # only 7 distinct values
    scores[0] = 0.0                                                     # a constant row
    scores[1, ::3] = float("-inf")
    for k in (1, 50, 4096):
        s, i = E.topk(scores.to(dev), k)
        rs, ri = O.select_topk_deterministic(scores, k)
        assert torch.equal(s.cpu(), rs) and torch.equal(i.cpu(), ri)


@pytest.mark.parametrize("k", [513, 2561, 4096, 6000])
def test_radix_topk_settles_early_or_late(dev, k):
    """The radix path (k' > 512 on long rows) stops resolving the threshold as soon as everything at or above the current bin's lower edge
    fits the sort's next_pow2(k') slots, and hands the sort MORE than k' keys.  Rows built to hit every branch: spread values (settles
    after the first or second pass), the narrow spread of MoL logits, a k'-th score shared by thousands of items (never fits: all passes +
    the tie scan), a tie group that just fits / just does not fit the slots, and -inf padding."""
    n, npad = 200_000, 1 << (k - 1).bit_length()
    g = torch.Generator().manual_seed(k)
    rows = [torch.randn(n, generator=g) * 2.0,
            0.1 + 0.02 * torch.randn(n, generator=g),
            torch.round(torch.randn(n, generator=g) * 2) / 2,
            torch.randn(n, generator=g)]
    for extra in (npad - k, npad - k + 1):           # k-th place inside a tie group of `extra + 2` items, k - 1 items above it
        r = torch.rand(n, generator=g) * 0.5
        perm = torch.randperm(n, generator=g)
        r[perm[: k - 1]] = 2.0 + torch.rand(k - 1, generator=g)
        r[perm[k - 1 : k + 1 + extra]] = 1.0
        rows.append(r)
    rows[3][::7] = float("-inf")
    scores = torch.stack(rows)
    s, i = E.topk(scores.to(dev), k)
    rs, ri = O.select_topk_deterministic(scores, k)
    assert torch.equal(s.cpu(), rs) and torch.equal(i.cpu(), ri)


def test_topk_rows_not_16_byte_aligned(dev):
    g = torch.Generator().manual_seed(9)
    big = torch.randn((3, 90001), generator=g).to(dev)       # odd leading dimension: rows 1, 2 start off 16-byte alignment
    for n in (90001, 30001, 2049):
        view = big[:, 1:n]
        s, i = E.topk(view, 77)
        rs, ri = O.select_topk_deterministic(view.cpu(), 77)
        assert torch.equal(s.cpu(), rs) and torch.equal(i.cpu(), ri)


def test_topk_id_lookup_and_strided_rows(dev):
    g = torch.Generator().manual_seed(5)
    big = torch.randn((4, 50000), generator=g).to(dev)
    view = big[:, :40000]                      # ld > n
    ids = torch.randperm(40000, generator=g).to(dev) + 7
    s, i = E.topk(view, 100, ids=ids)
    rs, ri = O.select_topk_deterministic(view.cpu(), 100)
    assert torch.equal(s.cpu(), rs) and torch.equal(i.cpu(), ids.cpu()[ri])
    per_row = torch.stack([torch.randperm(40000, generator=g) for _ in range(4)]).to(dev)
    s, i = E.topk(view, 100, ids=per_row)
    assert torch.equal(i.cpu(), torch.gather(per_row.cpu(), 1, ri))


@pytest.mark.parametrize("rows,kp,width,k", [(4, 200, 61, 120), (8, 2711, 211, 2500), (3, 25, 30, 20), (2, 10, 1, 10)])
def test_filter_seen_ids_matches_oracle(dev, rows, kp, width, k):
    g = torch.Generator().manual_seed(kp)
    ids = torch.stack([torch.randperm(5 * kp, generator=g)[:kp] + 1 for _ in range(rows)])
    scores = torch.sort(torch.randn((rows, kp), generator=g), dim=1, descending=True)[0]
    inv = torch.zeros((rows, width), dtype=torch.int64)
    for r in range(rows):
        m = min(width, kp - 1) if r % 2 == 0 else width // 2     # even rows: nearly everything is seen -> back-fill
        inv[r, :m] = ids[r, torch.randperm(kp, generator=g)[:m]]
    out_i, out_s = E.filter_seen_ids(ids.to(dev), scores.to(dev), inv.to(dev), k)
    ref_i, ref_s = O.filter_seen_ids(ids, scores, inv, k)
    assert torch.equal(out_i.cpu(), ref_i) and torch.equal(out_s.cpu(), ref_s)


# ---- properties at the full amzn-books size --------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_size_books_properties(dev, precision):
    """N = 695 762, B = 32 (BASELINE.json config 3): the oracle cannot score this in seconds, so check
    (a) a random sample of columns against the oracle, (b) shard-merge == global top-k, (c) idempotence."""
    cfg = O.CONFIGS["amzn-books"]
    w = O.synthetic_weights(cfg, seed=0)
    mol = build_module(cfg, w, dev, precision)
    N, B, k = 695762, 32, 200
    X = torch.from_numpy(O.hash_item_table(1, 0, N, cfg.item_embedding_dim))
    q = O.synthetic_queries(cfg, B)
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X.unsqueeze(0).to(dev), torch.arange(1, N + 1).unsqueeze(0).to(dev))
        logits = tk.all_logits(q.to(dev))
        s, i = tk(q.to(dev), k=k)
        s2, i2 = tk(q.to(dev), k=k)
    assert torch.equal(s, s2) and torch.equal(i, i2)          # deterministic
    assert bool((s[:, :-1] >= s[:, 1:]).all())                # sorted descending
    g = torch.Generator().manual_seed(9)
    cols = torch.cat([torch.randperm(N, generator=g)[:4096], torch.tensor([0, 31, 32, N - 1, N - 2])])
    ref = O.mol_logits(cfg, w, q, X[cols].unsqueeze(0))
    d = float((logits[:, cols.to(dev)].cpu() - ref).abs().max())
    assert d <= LOGIT_TOL, d
    # the returned scores are the logits at the returned positions, and nothing outside beats the k-th
    assert torch.equal(torch.gather(logits, 1, i - 1), s)
    assert bool((logits >= s[:, -1:]).sum(1).ge(k).all()) and bool((logits > s[:, -1:]).sum(1).lt(k).all())
    # sharded evaluation: per-shard top-k merged == global top-k, bit for bit (2/4/8 shards)
    for R in (2, 8):
        bounds = [((N + R - 1) // R) * r for r in range(R)] + [N]
        parts_s, parts_i = [], []
        for r in range(R):
            ps, pi = E.topk(logits[:, bounds[r]:bounds[r + 1]], k)
            parts_s.append(ps)
            parts_i.append(pi + bounds[r] + 1)
        ms, mi = E.topk(torch.cat(parts_s, 1), k, ids=torch.cat(parts_i, 1))
        assert torch.equal(ms, s) and torch.equal(mi, i)


# ---- A10: two-pass approximate top-k (MoLAvgTopK) ---------------------------------------------------
@pytest.mark.parametrize("avg_k", [100, 500])
def test_f4_avg_topk(fx, mol, dev, avg_k):
    X, ids, q = fx.t("X").to(dev), fx.t("item_ids").to(dev), fx.t("q").to(dev)
    kw = kw_dev(fx, dev)
    with torch.inference_mode():
        at = rails_amd.get_top_k_module(f"MoLAvgTopK{avg_k}", type("M", (), {"_ndp_module": mol})(), X, ids)
        eng = at._bind()
        # (a) coarse scores: the bf16 arithmetic of the reference, up to fp32 summation order before the
        #     final bf16 rounding (a different order can move a value by one bf16 ulp = 2^-8 relative)
        _, eq, _ = eng.query_pack(q, kw.get("user_ids"), want_plain=True)
        coarse = eng.coarse_scores(eq, at._table(), average_queries=False).cpu()
        ref = fx.t(f"F4/a{avg_k}/coarse_scores_bf16_as_f32")
        assert torch.equal(coarse.bfloat16().float(), coarse)            # values are bf16-representable
        rel = (coarse - ref).abs() / ref.abs().clamp_min(1e-3)
        assert float((rel > 0).float().mean()) < 0.02 and float(rel.max()) <= 2 ** -7
        # (b) rerank on the reference's own candidate set == the reference's final answer
        cand = fx.t(f"F4/a{avg_k}/coarse_idx_forward").to(dev)
        qpack, _, _ = eng.query_pack(q, kw.get("user_ids"))
        s, i = at.rerank(qpack, q.shape[0], cand, 50)
        assert_topk_matches(s, i, fx.t(f"F4/a{avg_k}/scores"), fx.t(f"F4/a{avg_k}/ids"), atol=LOGIT_TOL)
        # (a') the arithmetic itself is the reference's bf16 mm (exact bf16 products, fp32 accumulate, one rounding to bf16):
        #      on the REFERENCE's own bf16 operands the scores agree except where two fp32 accumulation orders straddle a bf16
        #      rounding boundary (probability ~d * 2^-24 / 2^-9 per entry: a handful of entries in 6 x 1024 at d = 128, each by
        #      one bf16 ulp).  What differs under (a) beyond that is the fp32 stage outputs (<= 2e-6, summation order of the
        #      index build) landing on the other side of a bf16 boundary of an OPERAND.
        ex_ref = O.item_component_embeddings(fx.cfg, fx.weights, fx.t("X").float().squeeze(0)).bfloat16()
        table_ref = (ex_ref.sum(1) / fx.cfg.item_dot_product_groups).contiguous()
        eq_ref = O.query_component_embeddings(fx.cfg, fx.weights, fx.t("q").float(), fx.user_ids)
        on_ref = eng.coarse_scores(eq_ref.to(dev), table_ref.to(dev), average_queries=False).cpu()
        n_diff = int((on_ref != ref).sum())
        assert n_diff <= max(2, ref.numel() // 500), n_diff
        assert float(((on_ref - ref).abs() / ref.abs().clamp_min(1e-3)).max()) <= 2 ** -7
        ours_table = at._table().cpu()
        assert float((ours_table != table_ref).float().mean()) < 0.01
        assert float((ours_table.float() - table_ref.float()).abs().max()) <= 2 ** -8    # one bf16 ulp of a unit-norm component

        def exact_scores(average_queries):   # the reference's coarse pass evaluated on OUR operands (CPU, exact accumulate)
            qs = eq.cpu().sum(1) / (fx.cfg.query_dot_product_groups if average_queries else 1)
            return (qs.bfloat16().double() @ ours_table.double().T).float().bfloat16().float()

        def assert_candidates(idx, scores):   # the K' best, exactly, except that members tied with the K'-th score are free
            for b in range(idx.shape[0]):
                mine = set(idx[b].tolist())
                kth = torch.sort(scores[b], descending=True).values[avg_k - 1]
                assert len(mine) == avg_k
                assert set(torch.nonzero(scores[b] > kth).flatten().tolist()) <= mine <= set(torch.nonzero(scores[b] >= kth).flatten().tolist())

        # (c) end to end: the candidate set is the exact top-K' of the coarse scores (modulo ties at the boundary), and the
        #     final answer is the oracle's rerank of that very set
        _, cand_idx = at._coarse_topk(q, average_queries=False, **kw)
        assert_candidates(cand_idx.cpu(), exact_scores(False))
        s, i = at(q, k=50, **kw)
        es, ei, _ = O.avg_topk(fx.cfg, fx.weights, fx.t("q"), fx.t("X"), fx.t("item_ids"), 50, avg_k, fx.user_ids, coarse_idx=cand_idx.cpu())
        assert_topk_matches(s, i, es, ei, atol=LOGIT_TOL)
        ref_ids = fx.t(f"F4/a{avg_k}/ids")
        # (d) recall against exact brute force is what the method trades (it is low on random-init weights):
        #     ours must match the recall the reference itself gets on the same inputs
        exact = fx.t("F2/k10/ids")
        def recall_of(found):
            return sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(found, exact)) / exact.numel()
        assert abs(recall_of(i.cpu()) - recall_of(ref_ids)) <= 0.1, (recall_of(i.cpu()), recall_of(ref_ids))
        # (e) topk_ids uses the averaged query: same criterion
        assert_candidates(at.topk_ids(q, **kw).cpu(), exact_scores(True))
        with pytest.raises(ValueError, match="must be larger than k"):
            at(q, k=avg_k + 1, **kw)


def planted_weights(cfg, seed, gate_scale):
    """Random-init weights make the averaged dot product of pass 1 nearly uncorrelated with the MoL score (recall ~ 0: there is
    nothing to retrieve).  Scaling the three gate networks' output layers towards zero makes the mixture weights near-uniform, so
    that MoL ~ mean cross logit = the coarse score up to a constant, plus a gate-dependent perturbation: a corpus on which the
    two-pass algorithm has something to find."""
    w = {k: v.clone() for k, v in O.synthetic_weights(cfg, seed=seed).items()}
    for key in ("_gating_fn._query_only_partial_module.2.weight", "_gating_fn._item_only_partial_module.3.weight",
                "_gating_fn._qi_partial_module.3.weight", "_gating_fn._qi_partial_module.3.bias"):
        w[key] = w[key] * gate_scale
    return w


def test_two_pass_recall_on_planted_structure(dev):
    """BASELINE config 5's quality side at 1 M items: on a corpus with planted structure the HIP two-pass returns what the
    oracle's two-pass returns, and that is a real retrieval result (recall@10 against exact brute force well above chance)."""
    cfg = O.CONFIGS["amzn-books"]
    w = planted_weights(cfg, seed=3, gate_scale=0.25)
    mol = build_module(cfg, w, dev)
    N, B, k, avg_k = 1_000_000, 8, 10, 1000
    X = torch.cat([torch.from_numpy(O.hash_item_table(21, s0, 250_000, cfg.item_embedding_dim)) for s0 in range(0, N, 250_000)]).unsqueeze(0)
    ids = torch.arange(1, N + 1, dtype=torch.int64).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=6)
    with torch.inference_mode():
        two = rails_amd.MoLAvgTopK(mol, X.to(dev), ids.to(dev), avg_top_k=avg_k)
        s, i = two(q.to(dev), k=k)
        _, exact = rails_amd.MoLBruteForceTopK(mol, X.to(dev), ids.to(dev))(q.to(dev), k=k)
    os_, oi, _ = O.avg_topk(cfg, w, q, X, ids, k, avg_k)                 # the oracle's own two-pass (its own candidates)
    assert_topk_matches(s, i, os_, oi, atol=LOGIT_TOL)
    recall = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(i.cpu(), exact.cpu())) / exact.numel()
    assert recall >= 0.5, recall


@pytest.mark.parametrize("cfg_name,n,avg_k", [("amzn-books", 300_001, 100), ("amzn-books", 300_001, 1000), ("amzn-books", 700_000, 4000),
                                              ("ml-1m", 280_000, 500), ("ml-20m", 270_000, 200), ("amzn-books", 300_002, 4000)])
def test_fused_coarse_topk_equals_the_materialised_path(dev, cfg_name, n, avg_k):
    """Config 5's coarse pass at scale: scan + threshold select without the (B, N) score matrix.  Same MFMA arithmetic as
    rails_mol_coarse_score, so (scores, positions) must equal coarse_scores + top-K' bit for bit.  The last case (128 queries, K' = 4 000 on
    300 k items: ~1 600 hits per workgroup of the select scan) runs the appends past the workgroup's LDS list of 1 024 (round 6)."""
    cfg = O.CONFIGS[cfg_name]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    X = torch.from_numpy(O.hash_item_table(5, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    B = 128 if n == 300_002 else (32 if cfg_name == "amzn-books" else 19)
    q = O.synthetic_queries(cfg, B, seed=4).to(dev)
    kw = {}
    if len(cfg.uid_embedding_hash_sizes) > 0:
        kw["user_ids"] = torch.arange(B, dtype=torch.int64, device=dev) * 7 + 1
    with torch.inference_mode():
        at = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=avg_k)
        eng = at._bind()
        _, eq, _ = eng.query_pack(q, kw.get("user_ids"), want_plain=True)
        for average in (False, True):
            coarse = eng.coarse_scores(eq, at._table(), average)
            rs, rp = E.topk(coarse, avg_k)
            fs, fp, counts = eng.coarse_topk(eq, at._table(), average, avg_k)
            assert int(counts.min()) >= avg_k and int(counts.max()) <= eng.coarse_topk_capacity(avg_k, at._table().shape[0]), counts
            assert torch.equal(fs, rs) and torch.equal(fp, rp)
            # the int8 pre-filter changes what the streaming pass reads, not what it finds: same candidates, counts, output
            ps, pp, pc = eng.coarse_topk(eq, at._table(), average, avg_k, prefilter=eng.build_coarse_prefilter(at._table()))
            assert torch.equal(ps, rs) and torch.equal(pp, rp) and torch.equal(pc, counts)
        # the module takes the fused path at this size and returns what the materialising path returns
        s1, i1 = at(q, k=50, **kw)
        at.fused_coarse_min_items = 1 << 62
        s2, i2 = at(q, k=50, **kw)
        assert torch.equal(s1, s2) and torch.equal(i1, i2)


@pytest.mark.parametrize("cfg_name,n,B,avg_k", [("amzn-books", 2_200_003, 32, 1000), ("amzn-books", 2_200_003, 70, 300),
                                                ("ml-1m", 1_200_001, 32, 500), ("ml-20m", 600_011, 40, 200)])
def test_fused_coarse_topk_over_several_trips_per_wave(dev, cfg_name, n, B, avg_k):
    """The select scan double-buffers trips of item tiles in registers; only a corpus with more than 2 048 workgroups x 4 waves x
    (4 | 2 | 1 tiles at d = 32 | 64 | 128) tiles makes a wave go round that loop more than once (the last round ragged).  Same
    claim as above at such sizes, for one and for several query tiles: fused == materialised coarse scores + top-K', bit for bit."""
    cfg = O.CONFIGS[cfg_name]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=3), dev)
    X = torch.empty((1, n, cfg.item_embedding_dim), dtype=torch.float32, device=dev)
    for s0 in range(0, n, 500_000):
        m = min(500_000, n - s0)
        X[0, s0 : s0 + m] = torch.from_numpy(O.hash_item_table(9, s0, m, cfg.item_embedding_dim)).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=6).to(dev)
    kw = {}
    if len(cfg.uid_embedding_hash_sizes) > 0:
        kw["user_ids"] = torch.arange(B, dtype=torch.int64, device=dev) * 5 + 2
    with torch.inference_mode():
        at = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=avg_k)
        eng = at._bind()
        _, eq, _ = eng.query_pack(q, kw.get("user_ids"), want_plain=True)
        coarse = eng.coarse_scores(eq, at._table(), True)
        rs, rp = E.topk(coarse, avg_k)
        fs, fp, counts = eng.coarse_topk(eq, at._table(), True, avg_k)
        assert int(counts.min()) >= avg_k and int(counts.max()) <= eng.coarse_topk_capacity(avg_k, at._table().shape[0]), counts
        assert torch.equal(fs, rs) and torch.equal(fp, rp)
        ps, pp, pc = eng.coarse_topk(eq, at._table(), True, avg_k, prefilter=eng.build_coarse_prefilter(at._table()))
        assert torch.equal(ps, rs) and torch.equal(pp, rp) and torch.equal(pc, counts)


def test_fused_coarse_topk_falls_back_on_heavy_ties(dev):
    """A corpus of 300k copies of 40 distinct items: every coarse score is tied thousands of times, the candidate lists
    overflow, and the module must notice (counts) and return the materialising path's answer."""
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    base = torch.from_numpy(O.hash_item_table(6, 0, 40, cfg.item_embedding_dim))
    n = 300_000
    X = base[torch.arange(n) % 40].unsqueeze(0).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, 8, seed=4).to(dev)
    with torch.inference_mode():
        at = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=200)
        eng = at._bind()
        _, eq, _ = eng.query_pack(q, None, want_plain=True)
        _, _, counts = eng.coarse_topk(eq, at._table(), False, 200)
        assert int(counts.max()) > eng.coarse_topk_capacity(200, at._table().shape[0])
        s1, i1 = at(q, k=50)
        at.fused_coarse_min_items = 1 << 62
        s2, i2 = at(q, k=50)
        assert torch.equal(s1, s2) and torch.equal(i1, i2)


def test_avg_topk_submit_then_result_equals_forward(dev):
    """MoLAvgTopK.submit / result (forward in two stages: everything enqueued on the assumption that the fused scan was exact, the
    verdict word read afterwards): two batches submitted before either result is taken give forward's outputs; on the heavy-ties
    corpus the verdict says redo and result() returns the materialising path's answer; the same through ShardedMoLAvgTopK."""
    from rails_amd.sharded import ShardedMoLAvgTopK
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    n = 300_000
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    qa, qb = O.synthetic_queries(cfg, 8, seed=4).to(dev), O.synthetic_queries(cfg, 8, seed=5).to(dev)
    base = torch.from_numpy(O.hash_item_table(6, 0, n, cfg.item_embedding_dim))
    with torch.inference_mode():
        for tied in (False, True):
            X = (base[torch.arange(n) % 40] if tied else base).unsqueeze(0).to(dev)
            for make in (lambda: rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=200), lambda: ShardedMoLAvgTopK(mol, X, ids, n, avg_top_k=200)):
                at = make()
                local = getattr(at, "_local_module", at)
                local.DEVICE_REDO_BYTES = 0                      # as on a full shard: no room for the (B, N) redo buffer, the host reads the verdict
                ha, hb = at.submit(qa, 50), at.submit(qb, 50)
                spec = ha if at is local else ha[3]
                assert spec is not None and spec[0] == "speculative"
                ra, rb = at.result(ha), at.result(hb)
                local.fused_coarse_min_items = 1 << 62          # the materialising path
                wa, wb = at(qa, k=50), at(qb, k=50)
                assert torch.equal(ra[0], wa[0]) and torch.equal(ra[1], wa[1]) and torch.equal(rb[0], wb[0]) and torch.equal(rb[1], wb[1])
                if tied:
                    assert ra[0] is not spec[1]                  # redone, not the speculative tensors


@pytest.mark.parametrize("tied", [False, True])
def test_candidate_unions_with_the_verdict_read_on_the_host(dev, tied, monkeypatch):
    """MoLNaiveTopK / MoLCombTopK where the (rows, N) redo buffer "does not fit" (DEVICE_REDO_BYTES = 0, as on a full shard): the
    fused scans' verdict words are collected while the call is enqueued and read once at its end; on the heavy-ties corpus they say
    redo and the materialising path answers.  Same outputs as with the fused scans switched off."""
    monkeypatch.setattr(rails_amd.MoLAvgTopK, "DEVICE_REDO_BYTES", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    n = 300_000
    base = torch.from_numpy(O.hash_item_table(6, 0, n, cfg.item_embedding_dim))
    X = (base[torch.arange(n) % 40] if tied else base).unsqueeze(0).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, 4, seed=4).to(dev)
    with torch.inference_mode():
        for mod in (rails_amd.MoLNaiveTopK(mol, X, ids, k_per_group=5), rails_amd.MoLCombTopK(mol, X, ids, avg_top_k=200, k_per_group=5)):
            s1, i1 = mod(q, k=50)
            mod.fused_component_min_items = mod.fused_coarse_min_items = 1 << 62
            s2, i2 = mod(q, k=50)
            assert torch.equal(s1, s2) and torch.equal(i1, i2)


@pytest.mark.parametrize("case", ["outlier", "inf", "nan_rows", "zeros", "ties", "tiny_queries", "negative"])
def test_int8_prefilter_never_loses_a_candidate(dev, case, monkeypatch):
    """The int8 pre-filter of the fused coarse top-K' decides which tiles are scored at all, from a rigorous bound on |bf16 dot -
    scaled int8 dot|.  Tables and queries that stress the bound: one item 1 000 x larger than the rest (the single scale crushes every
    other item to zero: the bound must then let every tile through), an inf entry, NaN rows, an all-zero table, a table of 40 distinct
    rows, queries 1e-6 x smaller than the items, all-negative scores.  Always: same (scores, positions, counts) as without it."""
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    n, K = 300_000, 300
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, 9, seed=4).to(dev)
    with torch.inference_mode():
        X = torch.from_numpy(O.hash_item_table(6, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
        at = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=K)
        eng = at._bind()
        _, eq, _ = eng.query_pack(q, None, want_plain=True)
        table = at._table().clone()
        if case == "outlier":
            table[12345] = table[12345] * 1000.0
        elif case == "inf":
            table[777, 3] = float("inf")
        elif case == "nan_rows":
            table[5000:9000] = float("nan")
        elif case == "zeros":
            table.zero_()
        elif case == "ties":
            table = table[torch.arange(n, device=dev) % 40].contiguous()
        elif case == "tiny_queries":
            eq = eq * 1e-6
        elif case == "negative":
            table = -table.abs()
            eq = eq.abs()
        pre = eng.build_coarse_prefilter(table)
        for average in (False, True):
            fs, fp, counts = eng.coarse_topk(eq, table, average, K)
            ps, pp, pc = eng.coarse_topk(eq, table, average, K, prefilter=pre)
            assert torch.equal(pc, counts)                # the same candidates reached the lists
            exact = (counts >= K) & (counts <= eng.coarse_topk_capacity(K, table.shape[0]))      # rows whose lists hold every candidate: defined output
            if case in ("zeros", "ties"):
                assert not bool(exact.any())              # every score tied thousands of times: all rows overflow, the caller redoes them
            else:
                assert bool(exact.all()) or case == "inf", (case, counts)
            rs, rp = E.topk(eng.coarse_scores(eq, table, average), K)
            for b in torch.nonzero(exact).flatten().tolist():
                assert torch.equal(ps[b], rs[b]) and torch.equal(pp[b], rp[b]) and torch.equal(fs[b], rs[b]) and torch.equal(fp[b], rp[b])


def test_int8_prefilter_build_equals_the_cpu_restatement(dev):
    """rails_mol_coarse_prefilter_build against oracle.int8_prefilter_bound's quantisation: the same scale, the same max |x|_1 and
    the same int8 value for every entry of the table (the bound tested on the CPU is the bound of what the kernel built)."""
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    n = 100_003
    X = torch.from_numpy(O.hash_item_table(5, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    with torch.inference_mode():
        at = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=100)
        eng = at._bind()
        table = at._table()
        pre = eng.build_coarse_prefilter(table).cpu()
        hdr = pre[:12].view(torch.float32)
        x = table.cpu().float()
        mx = x.abs().max()
        assert float(hdr[0]) == float(mx / 127.0) and float(hdr[1]) == float(torch.tensor(127.0) / mx)
        assert abs(float(hdr[2]) - float(x.abs().sum(1).max())) <= 1e-5 * float(hdr[2])      # summation order
        want = torch.clamp(torch.round(x * hdr[1]), -127, 127).to(torch.int8)
        got = pre[256:].view(torch.int8).view(n, -1)
        assert torch.equal(got, want)


def test_avg_topk_module_with_the_int8_prefilter(dev, monkeypatch):
    """MoLAvgTopK builds the pre-filter for large tables on its own (PREFILTER_MIN_ITEMS); lowered here: forward with it == forward
    without it == the materialising path, d = 32 / 64 / 128 shapes."""
    # (the last case, d = 128 with B = 128: the int8 scan's LDS image would be 50 688 B, over what a launch gets -- the call must take the
    #  bf16 select scan instead, before anything is enqueued, with the same output; it used to fail after the sample launch)
    for cfg_name, n, B in (("amzn-books", 300_001, 70), ("ml-1m", 280_000, 70), ("ml-20m", 270_000, 70), ("ml-20m", 270_000, 128)):
        cfg = O.CONFIGS[cfg_name]
        mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
        X = torch.from_numpy(O.hash_item_table(5, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
        q = O.synthetic_queries(cfg, B, seed=4).to(dev)
        kw = {"user_ids": torch.arange(B, dtype=torch.int64, device=dev) * 7 + 1} if len(cfg.uid_embedding_hash_sizes) > 0 else {}
        with torch.inference_mode():
            monkeypatch.setattr(rails_amd.MoLAvgTopK, "PREFILTER_MIN_ITEMS", 1)
            a = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=500)
            s1, i1 = a(q, k=50, **kw)
            assert a._prefilter() is not None
            monkeypatch.setattr(rails_amd.MoLAvgTopK, "PREFILTER_MIN_ITEMS", 1 << 62)
            b = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=500)
            s2, i2 = b(q, k=50, **kw)
            assert b._prefilter() is None
            b.fused_coarse_min_items = 1 << 62
            s3, i3 = b(q, k=50, **kw)
            assert torch.equal(s1, s2) and torch.equal(i1, i2) and torch.equal(s1, s3) and torch.equal(i1, i3)


@pytest.mark.parametrize("tied", [False, True])
def test_avg_topk_with_the_filter_enqueued_before_the_verdict_is_read(dev, tied, monkeypatch):
    """CandidateIndex.get_top_k_outputs through MoLAvgTopK.forward_filtered (the seen-id filter enqueued on the speculative output,
    redone if the scan's verdict says so) == forward + filter_seen_ids, on an ordinary corpus and on the heavy-ties one."""
    monkeypatch.setattr(rails_amd.MoLAvgTopK, "DEVICE_REDO_BYTES", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    n = 300_000
    base = torch.from_numpy(O.hash_item_table(6, 0, n, cfg.item_embedding_dim))
    X = (base[torch.arange(n) % 40] if tied else base).unsqueeze(0).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, 8, seed=4).to(dev)
    with torch.inference_mode():
        at = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=200)
        cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
        s0, i0 = at(q, k=60)
        inv = torch.zeros((8, 21), dtype=torch.int64, device=dev)
        inv[:, :10] = i0[:, 5:15]
        got_i, got_s, _ = cand.get_top_k_outputs(q, 40, {}, at, inv)
        want_i, want_s = E.filter_seen_ids(*reversed(at(q, k=61)), inv, 40)
        assert torch.equal(got_i, want_i) and torch.equal(got_s, want_s)
        assert at.forward_filtered(q, 61, inv, 40) is not None
        comb = rails_amd.MoLCombTopK(mol, X, ids, avg_top_k=200, k_per_group=5)
        assert comb.forward_filtered(q, 61, inv, 40) is None       # its forward is its own


def test_avg_topk_many_batches_in_flight_on_alternating_streams(dev, monkeypatch):
    """Forty different batches through submit / result with two or three of them in flight (speculative calls alternate between
    two streams of the module; their workspaces, outputs and verdict words are recycled by the caching allocators): every result
    equals the plain forward of its own batch -- also when the results are taken out of submission order."""
    monkeypatch.setattr(rails_amd.MoLAvgTopK, "DEVICE_REDO_BYTES", 0)
    monkeypatch.setattr(rails_amd.MoLAvgTopK, "PREFILTER_MIN_ITEMS", 1)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    n = 400_000
    X = torch.from_numpy(O.hash_item_table(5, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    with torch.inference_mode():
        at = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=60)
        batches = [O.synthetic_queries(cfg, 3 + (i % 5), seed=100 + i).to(dev) for i in range(40)]
        want = [at(q, k=20) for q in batches]
        handles, got = [], {}
        for i, q in enumerate(batches):
            handles.append((i, at.submit(q.clone(), 20)))       # the clone is dropped right away: the call's stream must keep it alive
            if len(handles) == 3:
                j, h = handles.pop(1 if i % 2 else 0)            # not always the oldest
                got[j] = at.result(h)
            junk = torch.randn(1 << 20, device=dev)              # allocator churn on the caller's stream
            del junk
        for j, h in handles:
            got[j] = at.result(h)
        for i in range(40):
            assert torch.equal(got[i][0], want[i][0]) and torch.equal(got[i][1], want[i][1]), i


def test_avg_topk_drops_a_prefilter_that_filters_nothing(dev, monkeypatch):
    """The select scans count, in the pre-filter's header, the (tile, query tile) blocks that passed the integer bound.  On an
    ordinary table few do and the module keeps the int8 copy; with one item 1 000 x larger than the rest the single scale crushes
    the others, every block passes, and the module drops the copy after its second call -- outputs unchanged throughout."""
    monkeypatch.setattr(rails_amd.MoLAvgTopK, "PREFILTER_MIN_ITEMS", 1)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    n = 300_000
    X = torch.from_numpy(O.hash_item_table(5, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, 4, seed=4).to(dev)     # few queries, small K': ~4 K' B = 800 candidates over 9 375 tiles
    with torch.inference_mode():
        a = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=20)
        outs = [a(q, k=20) for _ in range(4)]
        st = a.prefilter_stats()
        assert st is not None and st["tested"] > 0 and st["fraction"] < 0.35, st
        b = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=20)
        eng = b._bind()
        b._table()[4321] *= 1000.0                                   # an outlier row sets the scale of the whole int8 copy
        b._coarse_prefilter = eng.build_coarse_prefilter(b._table())
        outs_b = [b(q, k=20) for _ in range(4)]
        torch.cuda.synchronize()                                     # the statistics travel to the host behind the launches: no host wait inside forward
        outs_b.append(b(q, k=20))                                    # ... and are looked at by the next call that finds them landed
        assert b._coarse_prefilter is None                           # dropped after the statistics were read
        b2 = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=20)
        b2._table()[4321] *= 1000.0
        b2._coarse_prefilter = None
        want = b2(q, k=20)
        for o in outs_b:
            assert torch.equal(o[0], want[0]) and torch.equal(o[1], want[1])
        for o in outs[1:]:
            assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


def test_fused_coarse_topk_raises_its_flag_exactly_when_a_count_is_out_of_range(dev):
    """ABI 6: rails_mol_coarse_topk reports `out_of_range` from inside its key-selection launch -- 0 on an ordinary corpus (and
    the counts in range), 1 on the heavy-ties corpus (a sub-list overflowed), 1 when fewer than K' candidates reach the threshold
    (a corpus whose best K' scores are -inf cannot happen; an under-filled row is produced with a table of NaN rows instead, whose
    scores never compare >= a threshold): such a row names position 0 with score -inf in its unfilled slots."""
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    n = 300_000
    q = O.synthetic_queries(cfg, 8, seed=4).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    with torch.inference_mode():
        X = torch.from_numpy(O.hash_item_table(6, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
        at = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=200)
        eng = at._bind()
        _, eq, _ = eng.query_pack(q, None, want_plain=True)
        cap = eng.coarse_topk_capacity(200, n)
        for _ in range(2):    # the flag is reset by every call
            _, _, counts, flag = eng.coarse_topk(eq, at._table(), False, 200, with_flag=True)
            assert int(flag.item()) == 0 and int(counts.min()) >= 200 and int(counts.max()) <= cap
            tied = at._table()[torch.arange(n, device=dev) % 40].contiguous()
            _, _, counts, flag = eng.coarse_topk(eq, tied, False, 200, with_flag=True)
            assert int(flag.item()) == 1 and int(counts.max()) > cap
        nan_table = at._table().clone()
        nan_table[1000:] = float("nan")       # 1 000 real items: the sample sees a few of them, the scan collects fewer than K' = 2 000
        fs, fp, counts, flag = eng.coarse_topk(eq, nan_table, False, 2000, with_flag=True)
        assert int(flag.item()) == 1 and int(counts.min()) < 2000
        for b in range(eq.shape[0]):
            c = int(counts[b])
            if c < 2000:
                assert bool((fp[b, c:] == 0).all()) and bool(torch.isinf(fs[b, c:]).all()) and bool((fs[b, c:] < 0).all())
                assert bool((fp[b, :c] < 1000).all())


@pytest.mark.parametrize("rows,n,k", [(32, 1000, 120), (5, 100, 10), (7, 600, 512), (3, 1024, 300), (4, 3000, 200), (2, 4096, 2000), (3, 9000, 100), (1, 513, 513)])
def test_topk_candidates_equals_topk_over_gathered_ids(dev, rows, n, k):
    """rails_topk_candidates (ABI 6; reference mol_top_k.py:371-382 in one launch): top-k of candidate rows with the ids looked
    up THROUGH the candidates' corpus positions == rails_topk with ids = item_ids[positions] (the gathered copy the module made
    before); scores with ties (few distinct values), so the column tie rule shows."""
    g = torch.Generator().manual_seed(rows * 7919 + n)
    corpus = 50_000
    scores = (torch.randint(0, 37, (rows, n), generator=g).float() / 8.0).to(dev)
    pos = torch.randint(0, corpus, (rows, n), generator=g).to(dev)
    item_ids = (torch.arange(corpus, dtype=torch.int64, device=dev) * 3 + 11)
    ws, wi = E.topk(scores, k, ids=item_ids[pos])
    gs, gi = E.topk_candidates(scores, k, pos, item_ids)
    assert torch.equal(gs, ws) and torch.equal(gi, wi)
    gs, gp = E.topk_candidates(scores, k, pos)               # no id table: the corpus positions themselves
    assert torch.equal(gs, ws) and torch.equal(gp, torch.gather(pos, 1, E.topk(scores, k)[1]))


def test_topk_candidates_equals_the_oracle_selection_rule(dev):
    """rails_topk_candidates against the oracle's deterministic rule (score desc, column asc: what the reference's torch.topk +
    torch.gather + item_ids lookup returns modulo its tie order, mol_top_k.py:371-382) on rows with many exact ties."""
    g = torch.Generator().manual_seed(7)
    rows, n, k, corpus = 6, 1000, 120, 30_000
    scores = (torch.randint(0, 25, (rows, n), generator=g).float() / 4.0)
    pos = torch.stack([torch.randperm(corpus, generator=g)[:n] for _ in range(rows)])
    item_ids = torch.arange(corpus, dtype=torch.int64) * 5 + 3
    ws, wcol = O.select_topk_deterministic(scores, k)
    gs, gi = E.topk_candidates(scores.to(dev), k, pos.to(dev), item_ids.to(dev))
    assert torch.equal(gs.cpu(), ws) and torch.equal(gi.cpu(), item_ids[torch.gather(pos, 1, wcol)])


@pytest.mark.parametrize("rows,n,kp,width,k", [(32, 6400, 181, 61, 120), (5, 1025, 300, 100, 200), (7, 4096, 512, 256, 256), (3, 7400, 200, 0, 200), (2, 8192, 130, 10, 120),
                                                 (4, 8000, 1, 0, 1), (6, 3000, 150, 50, 100)])
def test_topk_candidates_filtered_equals_the_two_calls(dev, rows, n, kp, width, k):
    """rails_topk_candidates_filtered (ABI 10): the top-k' of candidate rows with the seen-id filter inside the launch == rails_topk_candidates(k')
    followed by rails_filter_seen_ids -- scores with ties and masked duplicates (-32767.0), seen ids drawn from the winners."""
    g = torch.Generator().manual_seed(rows * 31 + n + kp)
    corpus = 80_000
    scores = (torch.randint(0, 91, (rows, n), generator=g).float() / 8.0)
    scores[:, ::7] = -32767.0                                  # masked duplicates
    pos = torch.sort(torch.randint(0, corpus, (rows, n), generator=g), dim=1).values
    item_ids = torch.arange(corpus, dtype=torch.int64) * 3 + 11
    scores, pos, item_ids = scores.to(dev), pos.to(dev), item_ids.to(dev)
    ws, wi = E.topk_candidates(scores, kp, pos, item_ids)
    inv = torch.cat([wi[:, : width // 2], torch.randint(0, 3 * corpus, (rows, width - width // 2), generator=g).to(dev)], dim=1) if width else torch.zeros((rows, 0), dtype=torch.int64, device=dev)
    assert E.topk_candidates_filterable(n, kp, width, k)
    r_i, r_s = E.filter_seen_ids(wi, ws, inv, k)
    f_i, f_s = E.topk_candidates_filtered(scores, kp, pos, item_ids, inv, k)
    assert torch.equal(f_i, r_i) and torch.equal(f_s, r_s)
    assert not E.topk_candidates_filterable(1024, 100, 10, 50) and not E.topk_candidates_filterable(8193, 100, 10, 50) and not E.topk_candidates_filterable(5000, 513, 10, 50) and not E.topk_candidates_filterable(5000, 300, 257, 30)
    with pytest.raises(RuntimeError):
        E.topk_candidates_filtered(scores[:, :1000], min(kp, 1000), pos[:, :1000], item_ids, inv, min(k, kp, 1000))


@pytest.mark.parametrize("rows,n,kp,width,k,distinct", [(32, 6400, 181, 61, 120, 5000), (5, 1025, 300, 100, 200, 400), (7, 8192, 512, 256, 256, 8192), (3, 7400, 200, 0, 200, 3000),
                                                          (4, 3000, 150, 50, 100, 149), (2, 2000, 100, 20, 80, 100)])
def test_rerank_topk_filtered_equals_the_sorted_form(dev, rows, n, kp, width, k, distinct):
    """rails_rerank_topk_filtered (ABI 10): candidates in any order with duplicates -> the result of the sorted form (rails_sort_rows_i64, scores in
    that order, rails_mask_sorted_duplicates, rails_topk_candidates_filtered) whenever every row holds at least k' distinct positions; the
    out-of-range word is raised exactly when one does not.  A position's score is a function of the position (as in a rerank), with ties
    between positions."""
    g = torch.Generator().manual_seed(rows * 131 + n + kp)
    corpus = 3_000_000_000                                        # positions beyond 2^31
    pool = torch.stack([torch.randperm(200_000, generator=g)[:distinct] for _ in range(rows)]).to(torch.int64) * 14_999 + 7
    assert int(pool.max()) < corpus
    pos = torch.gather(pool, 1, torch.randint(0, distinct, (rows, n), generator=g))
    if distinct >= kp:
        pos[:, :distinct] = pool[:, torch.randperm(distinct, generator=g)]     # every pool entry at least once
    score_of = lambda p: ((p * 7 + 3) % 97).float() / 8.0 - 4.0          # many ties between positions
    item_ids = None
    pos = pos.to(dev)
    scores = score_of(pos)
    inv_src = torch.sort(pos, dim=1).values
    flag = torch.zeros(1, dtype=torch.int32).pin_memory()
    # the sorted form
    sp = E.sort_rows(pos)
    ss = score_of(sp).contiguous()
    E.mask_sorted_duplicates(sp, ss, -32767.0)
    ws, wi = E.topk_candidates(ss, kp, sp, item_ids)
    inv = torch.cat([wi[:, : width // 2], torch.randint(0, corpus, (rows, width - width // 2), generator=g).to(dev)], dim=1) if width else torch.zeros((rows, 0), dtype=torch.int64, device=dev)
    want_i, want_s = E.topk_candidates_filtered(ss, kp, sp, item_ids, inv, k)
    got_i, got_s = E.rerank_topk_filtered(scores, kp, pos, item_ids, inv, k, flag)
    torch.cuda.synchronize()
    n_distinct = min(int(torch.unique(pos[r]).numel()) for r in range(rows))
    assert int(flag[0]) == (1 if n_distinct < kp else 0), (n_distinct, kp)
    if n_distinct >= kp:
        assert torch.equal(got_i, want_i) and torch.equal(got_s, want_s)
        dflag = torch.zeros(1, dtype=torch.int32, device=dev)          # a device word works the same
        g2_i, g2_s = E.rerank_topk_filtered(scores, kp, pos, item_ids, inv, k, dflag)
        assert torch.equal(g2_i, want_i) and torch.equal(g2_s, want_s) and int(dflag.item()) == 0


@pytest.mark.parametrize("n,k", [(300_000, 1000), (695_762, 1600), (120_000, 4096), (60_000, 600)])
def test_predicated_topk_takes_the_two_launch_route_and_equals_the_plain_call(dev, n, k):
    """rails_topk under a launch predicate (the fallback behind a device-side verdict) selects k > 512 of a long row in two launches
    (per-chunk winners through the radix core, then the winners' winners) where the plain call takes the multi-launch radix path:
    predicate 1 -> the plain call's output, ties by position included; predicate 0 -> the outputs are left alone."""
    g = torch.Generator().manual_seed(n + k)
    scores = (torch.randint(0, 3000, (5, n), generator=g).float() / 64.0).to(dev)      # many exact ties around the k-th place
    want_s, want_i = E.topk(scores, k)
    out_s = torch.full((5, k), -7.0, dtype=torch.float32, device=dev)
    out_i = torch.full((5, k), -7, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    E.topk(scores, k, out=(out_s, out_i), run_if=flag)
    assert bool((out_s == -7.0).all()) and bool((out_i == -7).all())
    flag.fill_(1)
    E.topk(scores, k, out=(out_s, out_i), run_if=flag)
    assert torch.equal(out_s, want_s) and torch.equal(out_i, want_i)


@pytest.mark.parametrize("n,k", [(513, 1), (600, 120), (1000, 120), (1024, 512), (777, 512), (1000, 513)])
def test_topk_between_512_and_1024_columns(dev, n, k):
    """Rows of 513 .. 1 024 scores with k <= 512 take the register-resident selection (they were fully sorted before): the same
    (scores, positions) as a stable descending sort, ties and -inf included."""
    g = torch.Generator().manual_seed(n * 31 + k)
    scores = (torch.randint(0, 50, (6, n), generator=g).float() / 4.0)
    scores[0, : n // 2] = float("-inf")
    scores[1] = 1.5
    scores = scores.to(dev)
    vals, order = torch.sort(scores, dim=1, descending=True, stable=True)
    gs, gp = E.topk(scores, k)
    assert torch.equal(gs, vals[:, :k]) and torch.equal(gp, order[:, :k])


@pytest.mark.parametrize("cfg_name,n,k_g", [("amzn-books", 300_001, 5), ("amzn-books", 300_001, 100), ("ml-1m", 280_000, 50)])
def test_fused_component_topk_equals_the_materialised_path(dev, cfg_name, n, k_g):
    """Candidate generation of MoLNaiveTopK / MoLCombTopK at scale: same MFMA arithmetic as rails_mol_component_score, so the
    per-(query group, item group) top-k_g must equal component_scores + top-k bit for bit; and the modules must return the
    same final answer through either path."""
    cfg = O.CONFIGS[cfg_name]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    X = torch.from_numpy(O.hash_item_table(5, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    B = 8
    q = O.synthetic_queries(cfg, B, seed=4).to(dev)
    kw = {}
    if len(cfg.uid_embedding_hash_sizes) > 0:
        kw["user_ids"] = torch.arange(B, dtype=torch.int64, device=dev) * 7 + 1
    with torch.inference_mode():
        nt = rails_amd.MoLNaiveTopK(mol, X, ids, k_per_group=k_g)
        eng = nt._bind()
        _, eq, _ = eng.query_pack(q, kw.get("user_ids"), want_plain=True)
        table = nt._component_table()
        rs, rp = E.topk(eng.component_scores(eq, table), k_g)
        flag = torch.ones(1, dtype=torch.int32, device=dev)       # (zeroed by the call, raised when a count leaves its range)
        fs, fp, counts = eng.component_topk(eq, table, k_g, flag)
        assert int(counts.min()) >= k_g and int(counts.max()) <= eng.component_topk_capacity(B, n, k_g), (int(counts.min()), int(counts.max()))
        assert int(flag) == 0
        assert torch.equal(fs, rs) and torch.equal(fp, rp)
        for mod in (nt, rails_amd.MoLCombTopK(mol, X, ids, k_per_group=k_g, avg_top_k=200)):
            s1, i1 = mod(q, k=50, **kw)
            mod.fused_component_min_items = 1 << 62
            mod.fused_coarse_min_items = 1 << 62
            s2, i2 = mod(q, k=50, **kw)
            assert torch.equal(s1, s2) and torch.equal(i1, i2)


def test_large_batches_through_every_algorithm(dev):
    """B = 300 queries (the eval default is 32): nothing may depend on the batch fitting one LDS-resident query block."""
    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    n, B = 270_000, 300
    X = torch.from_numpy(O.hash_item_table(5, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=4).to(dev)
    model = type("M", (), {"_ndp_module": mol})()
    with torch.inference_mode():
        ref_s, ref_i = rails_amd.get_top_k_module("MoLBruteForceTopK", model, X, ids)(q, k=50)
        for name in ("MoLAvgTopK500", "MoLNaiveTopK10", "MoLCombTopK5_200"):
            mod = rails_amd.get_top_k_module(name, model, X, ids)
            s, i = mod(q, k=50)
            s32, i32 = mod(q[:32], k=50)
            assert s.shape[0] == B and torch.equal(s[:32], s32) and torch.equal(i[:32], i32)   # batch slicing changes nothing
        s, i = rails_amd.get_top_k_module("MoLBruteForceTopK", model, X, ids)(q[:32], k=50)
        assert torch.equal(ref_i[:32], i) and torch.equal(ref_s[:32], s)


def test_sharded_two_pass_composition_on_the_gpu(dev):
    """BASELINE config 5's per-rank work with the HIP kernels: MoLAvgTopK on each of R = 2 contiguous shards, the pack and
    merge kernels around the (here: emulated) all-gather.  Must equal the top-k of the union of the shards' results, and
    ShardedMoLAvgTopK at world size 1 must equal MoLAvgTopK."""
    from rails_amd.sharded import ShardedMoLAvgTopK, shard_bounds

    cfg = O.CONFIGS["amzn-books"]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=2), dev)
    n, B, k, avg_k = 600_000, 16, 100, 500
    X = torch.from_numpy(O.hash_item_table(5, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=4).to(dev)
    with torch.inference_mode():
        msgs, parts = [], []
        for r in range(2):
            lo, hi = shard_bounds(n, 2, r)
            s, i = rails_amd.MoLAvgTopK(mol, X[:, lo:hi], ids[:, lo:hi], avg_top_k=avg_k)(q, k=k)
            parts.append((s, i))
            msgs.append(E.pack_candidates(s, i, k))
        ms, mi = E.merge_candidates(torch.cat(msgs, 0), 2, k, k)
        all_s = torch.cat([p[0] for p in parts], 1).cpu()
        all_i = torch.cat([p[1] for p in parts], 1).cpu()
        es, pos = O.select_topk_deterministic(all_s, k)
        assert torch.equal(ms.cpu(), es) and torch.equal(mi.cpu(), torch.gather(all_i, 1, pos))
        one = ShardedMoLAvgTopK(mol, X, ids, n, avg_top_k=avg_k)
        s1, i1 = one(q, k=k)
        s0, i0 = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=avg_k)(q, k=k)
        assert torch.equal(s1, s0) and torch.equal(i1, i0)


# ---- section 8(f) rank 2: MIPSBruteForceTopK + DotProductSimilarity ------------------------------------
def test_f9_mips_and_dot_product(dev):
    import os

    import numpy as np

    from tests._fixtures import GOLDEN
    from tests.test_oracle_golden import _mips_inputs

    z = np.load(os.path.join(GOLDEN, "mips.npz"))
    T = lambda k: torch.from_numpy(z[k])
    dp = rails_amd.DotProductSimilarity()
    with torch.inference_mode():
        for tag in ("d50", "d64"):                       # D = 50 exercises the K padding to a multiple of 8
            q, X, ids = (t.to(dev) for t in _mips_inputs(z, tag))
            logits, aux = dp(q, X)
            assert aux == {}
            ref = O.dot_product_similarity(q.cpu(), X.cpu())
            assert torch.equal(ref[:2], T(f"{tag}/logits_head"))
            assert float((logits.cpu() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
            tk = rails_amd.get_top_k_module("MIPSBruteForceTopK", None, X, ids)
            for k in (10, 200):
                s, i = tk(q, k=k)
                assert_topk_matches(s, i, T(f"{tag}/k{k}/scores"), T(f"{tag}/k{k}/ids"), atol=1e-4, tie_tol=1e-4)
        for qk, ok in (("rows/q1", "rows/out1"), ("rows/q3", "rows/out3")):
            out, _ = dp(T(qk).to(dev), T("rows/X").to(dev))
            assert float((out.cpu() - T(ok)).abs().max()) <= 1e-5


# ---- section 8(f) rank 1: MoLNaiveTopK + MoLCombTopK ------------------------------------------------------
@pytest.mark.parametrize("cname", ["c1", "c3"])
def test_f10_naive_and_comb(dev, cname):
    import os

    import numpy as np

    from tests._fixtures import GOLDEN
    from tests.test_oracle_golden import _union_case

    z = np.load(os.path.join(GOLDEN, "union.npz"))
    cfg, w, T, uid = _union_case(z, cname)
    mol = build_module(cfg, w, dev)
    holder = type("M", (), {"_ndp_module": mol})()
    q, X, ids = T("q").to(dev), T("X").to(dev), T("item_ids").to(dev)
    kw = {} if uid is None else {"user_ids": uid.to(dev)}
    with torch.inference_mode():
        for name, mname in (("MoLNaiveTopK5", "naive5"), ("MoLCombTopK5_100", "comb5_100")):
            mod = rails_amd.get_top_k_module(name, holder, X, ids)
            ref_s, ref_i = T(f"{mname}/scores"), T(f"{mname}/ids")
            # (a) rerank half, on the candidate union the reference itself built: exact
            eng = mod._bind()
            qpack, _, _ = eng.query_pack(q, kw.get("user_ids"))
            s, i = mod._rerank_union(qpack, q.shape[0], T(f"{mname}/sorted_all_indices").to(dev), True)
            assert_topk_matches(s, i, ref_s, ref_i, atol=LOGIT_TOL)
            # (b) candidate generation: per (query, query group, item group) row the k_g best items by the bf16 component
            #     score, exactly (members tied with the k_g-th score are free) -- checked against the reference's arithmetic
            #     evaluated on OUR bf16 operands; then the end-to-end answer is the oracle's rerank of that very union
            _, eq, _ = eng.query_pack(q, kw.get("user_ids"), want_plain=True)
            kg = mod._k_per_group
            pos = mod._component_topk(eq, kg).cpu().view(q.shape[0], cfg.query_dot_product_groups, cfg.item_dot_product_groups, kg)
            table = mod._component_table().cpu()                       # (P_X, N, d) bf16 (item-group-major)
            sc = torch.einsum("bid,mxd->bimx", eq.cpu().bfloat16().double(), table.double()).float().bfloat16().float()
            for b in range(q.shape[0]):
                for gi_ in range(cfg.query_dot_product_groups):
                    for m in range(cfg.item_dot_product_groups):
                        row, mine = sc[b, gi_, m], set(pos[b, gi_, m].tolist())
                        kth = torch.sort(row, descending=True).values[kg - 1]
                        assert len(mine) == kg
                        assert set(torch.nonzero(row > kth).flatten().tolist()) <= mine <= set(torch.nonzero(row >= kth).flatten().tolist())
            s, i = mod(q, k=10, **kw)
            assert s.shape == ref_s.shape and i.shape == ref_i.shape
            assert bool((s[:, :-1] >= s[:, 1:]).all())
            parts = [mod._component_topk(eq, kg)]
            if mname.startswith("comb"):
                parts.append(mod._coarse_topk_from_eq(eq, average_queries=True))
            union = torch.sort(torch.cat(parts, dim=1), dim=1).values.cpu()
            es, ei = O.union_rerank(cfg, w, T("q"), T("X"), T("item_ids"), union, uid)
            assert_topk_matches(s, i, es, ei, atol=LOGIT_TOL)
            for b in range(q.shape[0]):    # and the retrieval result proper agrees with the reference's own run
                assert len(set(i[b, :10].tolist()) & set(ref_i[b, :10].tolist())) >= 9
        with pytest.raises(NotImplementedError):
            rails_amd.get_top_k_module("MoLNaiveFaissTopK5", holder, X, ids)


@pytest.mark.parametrize("cfg_name,n,method,B", [("amzn-books", 300_007, "MoLNaiveTopK100", 5), ("amzn-books", 300_007, "MoLCombTopK50_500", 3), ("amzn-books", 40_000, "MoLNaiveTopK25", 4),
                                                  ("ml-1m", 3883, "MoLCombTopK50_1000", 6), ("amzn-books", 300_007, "MoLNaiveTopK10", 4)])
def test_naive_and_comb_filter_inside_the_selection_equals_the_full_ranking(dev, monkeypatch, cfg_name, n, method, B):
    """get_top_k_outputs over MoLNaiveTopK / MoLCombTopK (which return ALL their candidates ranked, reference mol_top_k.py:260-293 / :518-551):
    round 6 keeps the filter inside the selection launch and selects only the top k + width -- the same (ids, scores) as ranking every
    candidate and filtering after (indexing/candidate_index.py:149-175), bit for bit, with seen ids taken from the best results; modules whose
    candidate count or k + width is outside the fused launch (Naive10: 640 candidates) compose the two calls as before."""
    cfg = O.CONFIGS[cfg_name]
    w = O.synthetic_weights(cfg, seed=0)
    mol = build_module(cfg, w, dev)
    holder = type("M", (), {"_ndp_module": mol})()
    X = torch.from_numpy(O.hash_item_table(3, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = (torch.arange(n, dtype=torch.int64, device=dev) * 2 + 9).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=4).to(dev)
    kw = {"user_ids": torch.arange(1, B + 1, dtype=torch.int64, device=dev)} if cfg.uid_embedding_hash_sizes else {}
    k, width = 120, 61
    # as at bench scale (32 queries x 695 762 items: a 5.7 GB score matrix), the fused scans' redo is the host's: their verdict word sits in pinned memory
    monkeypatch.setattr(rails_amd.MoLAvgTopK, "DEVICE_REDO_BYTES", 0)
    unsorted_calls = []
    real_rerank = E.rerank_topk_filtered
    monkeypatch.setattr(E, "rerank_topk_filtered", lambda *a, **kw_: (unsorted_calls.append(1), real_rerank(*a, **kw_))[1])
    with torch.inference_mode():
        mod = rails_amd.get_top_k_module(method, holder, X, ids)
        ci = rails_amd.CandidateIndex(ids, X)
        full_s, full_i = mod(q, k=k, **kw)                      # every candidate, ranked
        n_cand = full_i.shape[1]
        inv = torch.cat([full_i[:, :20], full_i[:, 100:110], ids[0, torch.randint(0, n, (B, width - 30), device=dev)]], dim=1)
        mod.NO_FILTER_FUSION = True
        assert mod.forward_filtered(q, 181, inv, k, **kw) is None
        want = ci.get_top_k_outputs(q, k=k, aux_payloads=kw, top_k_module=mod, invalid_ids=inv, truncate_k_prime_to=200)
        r_i, r_s = E.filter_seen_ids(full_i, full_s, inv, k)
        assert torch.equal(want[0], r_i) and torch.equal(want[1], r_s)
        mod.NO_FILTER_FUSION = False
        fused = mod.forward_filtered(q, 181, inv, k, **kw)
        assert (fused is not None) == (n_cand > 1024), n_cand
        got = ci.get_top_k_outputs(q, k=k, aux_payloads=kw, top_k_module=mod, invalid_ids=inv, truncate_k_prime_to=200)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert (len(unsorted_calls) > 0) == (fused is not None and n >= 262144), (len(unsorted_calls), n_cand)
        if fused is not None:
            assert torch.equal(fused[0], want[0]) and torch.equal(fused[1], want[1])
            # the sorted form of the fused tail (the unsorted one runs by default wherever the fused scans ran: n >= 262 144)
            mod.UNSORTED_RERANK = False
            n_u = len(unsorted_calls)
            srt = mod.forward_filtered(q, 181, inv, k, **kw)
            mod.UNSORTED_RERANK = True
            assert torch.equal(srt[0], want[0]) and torch.equal(srt[1], want[1]) and len(unsorted_calls) == n_u
            if n >= 262144:
                # a union with fewer distinct positions than k + width: the unsorted tail raises the scans' verdict word and the call is redone on
                # the sorted form, masked duplicates ranked as the reference ranks them
                calls = []
                real = type(mod)._component_topk

                def few(self, eq, kg, pending=None):
                    out = real(self, eq, kg, pending)
                    calls.append(pending is not None and any(not b.is_cuda for b in pending))
                    return out[:, :50].repeat(1, out.shape[1] // 50 + 1)[:, : out.shape[1]].contiguous()

                type(mod)._component_topk = few
                try:
                    mod.NO_FILTER_FUSION = True
                    want2 = ci.get_top_k_outputs(q, k=k, aux_payloads=kw, top_k_module=mod, invalid_ids=inv, truncate_k_prime_to=200)
                    mod.NO_FILTER_FUSION = False
                    n_before = len(calls)
                    got2 = ci.get_top_k_outputs(q, k=k, aux_payloads=kw, top_k_module=mod, invalid_ids=inv, truncate_k_prime_to=200)
                    if "Naive" in method:
                        assert len(calls) == n_before + 2 and calls[n_before], calls      # speculated once, redone once
                finally:
                    type(mod)._component_topk = real
                assert torch.equal(got2[0], want2[0]) and torch.equal(got2[1], want2[1])


@pytest.mark.parametrize("n", [1, 2, 64, 777, 1024, 1025, 2049, 4097, 8193, 16384])
def test_sort_rows_and_duplicate_mask(dev, n):
    """Rows of 1 .. 1 024 values take the plain network (2 .. 1 024 slots), longer ones the register sort at 2, 4, 8 and 16 keys per thread."""
    g = torch.Generator().manual_seed(1)
    if n != 777:
        idx = torch.randint(-(1 << 40), 1 << 40, (3, n), generator=g)
        idx[:, n // 2] = idx[:, 0]                                         # a repeated value
        assert torch.equal(E.sort_rows(idx.to(dev)).cpu(), torch.sort(idx, dim=1)[0])
        return
    idx = torch.randint(-50, 3000, (7, 777), generator=g)
    out = E.sort_rows(idx.to(dev)).cpu()
    assert torch.equal(out, torch.sort(idx, dim=1)[0])
    scores = torch.randn((7, 777), generator=g)
    dev_scores = scores.to(dev).clone()
    E.mask_sorted_duplicates(out.to(dev), dev_scores, -32767.0)
    valid = torch.cat([torch.ones((7, 1), dtype=torch.bool), out[:, 1:] != out[:, :-1]], 1)
    assert torch.equal(dev_scores.cpu(), torch.where(valid, scores, torch.tensor(-32767.0)))


# ---- robustness -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B", [1, 3, 33, 100])
def test_batch_sizes_cover_padding_and_both_kernels(dev, B, precision):
    """B = 1, 3: partial query group on the direct kernel; B = 33, 100: >= 8 groups -> staged kernel with the group
    loop wrapping (g += 8) and a padded last group."""
    cfg = O.CONFIGS["amzn-books"]
    w = O.synthetic_weights(cfg, seed=5)
    mol = build_module(cfg, w, dev, precision)
    N = 2000 + B
    X = torch.from_numpy(O.hash_item_table(3, 0, N, cfg.item_embedding_dim)).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=B)
    with torch.inference_mode():
        got, _ = mol(q.to(dev), X.to(dev))
    ref = O.mol_logits(cfg, w, q, X)
    assert got.shape == (B, N)
    assert float((got.cpu() - ref).abs().max()) <= LOGIT_TOL


@pytest.mark.parametrize("B", [1, 2, 3, 8, 32, 33])
@pytest.mark.parametrize("cfg_name,N", [("ml-1m", 3883), ("ml-20m", 2777), ("amzn-books", 5009)])
def test_small_unit_kernel_returns_the_bits_of_the_32x32_kernels(dev, monkeypatch, cfg_name, N, B):
    """The small-unit shell (v_mfma_f32_16x16x4_f32, 2 queries x 16 items per wave; mol_score_small.hip) visits the terms of every
    contraction and of the softmax sums in the order the 32x32x2 kernels do: the logits are the same BITS, whichever shell a
    corpus (or a shard of one) is given.  Odd batch sizes leave the second query of the last pair empty; N is not a multiple of 16."""
    cfg = O.CONFIGS[cfg_name]
    w = O.synthetic_weights(cfg, seed=11)
    mol = build_module(cfg, w, dev, "fp32")
    X = torch.from_numpy(O.hash_item_table(7, 0, N, cfg.item_embedding_dim)).to(dev)
    q = O.synthetic_queries(cfg, B, seed=B).to(dev)
    uid = torch.arange(B, dtype=torch.int64, device=dev) * 37 if cfg.uid_embedding_hash_sizes else None
    with torch.inference_mode():
        eng = mol.engine()
        index = eng.build_index(X)
        qpack, _, _ = eng.query_pack(q, uid)
        outs = {}
        for variant in ("7", "1", "0"):   # small units; the independent-wave 32x32x2 shell; whatever the dispatcher picks
            monkeypatch.setenv("RAILS_SCORE_VARIANT", variant)
            outs[variant] = eng.score_dense(qpack, B, index).clone()
        torch.cuda.synchronize()
    assert torch.equal(outs["7"], outs["1"])
    assert torch.equal(outs["7"], outs["0"])
    cols = torch.randperm(N, generator=torch.Generator().manual_seed(B))[:256]
    ref = O.mol_logits(cfg, w, q.cpu(), X[cols.to(dev)].cpu().unsqueeze(0), None if uid is None else uid.cpu())
    assert float((outs["7"][:, cols.to(dev)].cpu() - ref).abs().max()) <= LOGIT_TOL


@pytest.mark.parametrize("seed,first,n,dim", [(1, 0, 1000, 64), (7, 123_456_789, 4097, 50), (3, 999_999_000, 33, 256)])
def test_device_item_table_generator_equals_the_oracle_generator(dev, seed, first, n, dim):
    """rails_hash_item_table draws the synthetic corpora in HBM with the bits of oracle.hash_item_table (integer hash, one exact
    int -> float conversion, one fp32 multiply): any row of any shard can be re-created on a CPU by id."""
    got = E.hash_item_table(seed, first, n, dim, dev).cpu()
    assert torch.equal(got, torch.from_numpy(O.hash_item_table(seed, first, n, dim)))
    rows = torch.tensor([0, n // 2, n - 1])
    assert torch.equal(got[rows], torch.from_numpy(O.hash_item_rows(seed, (rows + first).numpy(), dim)))


@pytest.mark.parametrize("B", [1, 5, 32, 70])
@pytest.mark.parametrize("cfg_name", ["ml-1m", "ml-20m", "amzn-books"])
def test_split_prologue_returns_the_bits_of_the_per_query_kernel(dev, monkeypatch, cfg_name, B):
    """The split prologue (two short launches: GLU slices, then one workgroup per sub-embedding group + one for the gate chain;
    mol_query.hip) computes every column exactly as the per-query kernel does: fragments, plain Eq and gq are the same bits, padding
    rows of the last query group included (B = 5, 70: partial groups)."""
    cfg = O.CONFIGS[cfg_name]
    mol = build_module(cfg, O.synthetic_weights(cfg, seed=13), dev, "fp32")
    q = O.synthetic_queries(cfg, B, seed=40 + B).to(dev)
    uid = (torch.arange(B, dtype=torch.int64, device=dev) * 977) if cfg.uid_embedding_hash_sizes else None
    n_frag = ((B + 3) // 4) * 32 * cfg.dot_product_dimension + B * cfg.query_dot_product_groups * cfg.item_dot_product_groups
    outs = {}
    with torch.inference_mode():
        eng = mol.engine()
        for mode in ("1", "3", "2"):
            monkeypatch.setenv("RAILS_PROLOGUE", mode)
            qpack, eq, gq = eng.query_pack(q, uid, want_plain=True)
            outs[mode] = (qpack[:n_frag].clone(), eq.clone(), gq.clone())
        torch.cuda.synchronize()
    for a, b in zip(outs["1"], outs["3"]):
        assert torch.equal(a, b)
    eq_ref = O.query_component_embeddings(cfg, O.synthetic_weights(cfg, seed=13), q.cpu(), None if uid is None else uid.cpu())
    assert float((outs["3"][1].cpu() - eq_ref).abs().max()) <= STAGE_TOL
    assert float((outs["2"][1] - outs["3"][1]).abs().max()) <= STAGE_TOL      # the batched MFMA kernels sum in another order


def test_seen_id_filters_with_zero_width_history(dev):
    """A workload without history (BASELINE configs 4 and 5: seen-id width 0) hands the filters a (rows, 0) tensor, whose data pointer
    is null: every filtering entry point must treat it as "nothing to remove" -- the first k of the k' winners -- not as a NULL argument
    (the sharded bench of the 16x16x64 shape died on exactly that before round 4)."""
    g = torch.Generator().manual_seed(3)
    rows, n, kp, k = 5, 5000, 200, 120
    scores = torch.randn((rows, n), generator=g).to(dev)
    ids = (torch.arange(n, dtype=torch.int64) * 2 + 1).to(dev)
    inv = torch.zeros((rows, 0), dtype=torch.int64, device=dev)
    s, i = E.topk(scores, kp, ids=ids)
    fi, fs = E.filter_seen_ids(i, s, inv, k)
    assert torch.equal(fi, i[:, :k]) and torch.equal(fs, s[:, :k])
    ti, ts = E.topk_filtered(scores, kp, ids, inv, k)
    assert torch.equal(ti, i[:, :k]) and torch.equal(ts, s[:, :k])
    msg = E.pack_candidates(s, i, kp)
    mi, ms = E.merge_candidates_filtered(msg, 1, kp, kp, inv, k)
    assert torch.equal(mi, i[:, :k]) and torch.equal(ms, s[:, :k])


def test_bf16_module_and_inputs_round_trip(dev):
    """eval_batch.py runs --eval_dtype=bf16 (model and item table cast to bf16): parameters and inputs are
    up-cast, arithmetic stays fp32, outputs come back in the query dtype."""
    fx = Fixture("c3_books")
    mol = build_module(fx.cfg, fx.weights, dev).to(torch.bfloat16)
    q, X, ids = fx.t("q").to(dev).bfloat16(), fx.t("X").to(dev).bfloat16(), fx.t("item_ids").to(dev)
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
        s, i = tk(q, k=20)
        logits = tk.all_logits(q)
    assert s.dtype == torch.bfloat16 and i.dtype == torch.int64 and logits.dtype == torch.float32
    w16 = {k: v.bfloat16().float() for k, v in fx.weights.items()}
    ref = O.mol_logits(fx.cfg, w16, q.float().cpu(), X.float().cpu())
    assert float((logits.cpu() - ref).abs().max()) <= LOGIT_TOL


@pytest.mark.parametrize("precision", PRECISIONS)
def test_f8_against_the_references_own_bf16_run(dev, precision):
    """F8 (tests/golden/bf16_books.npz): eval_batch.py evaluates with model.to(bfloat16) and a bf16 item table.  rails_amd
    keeps such a module's operands as their bf16-rounded values and computes in fp32 / f16x3, so it must (a) equal the
    reference's FP32 arithmetic on those bf16 operands within the 1e-4 bar and (b) stay within the bf16 run's own rounding
    noise of the reference's BF16 run: stated tolerance 0.15 on logits in [-20, 20] (the two reference runs differ by up to
    0.127 here), >= 85 % of the bf16 run's top-200 items retrieved."""
    import numpy as np

    from tests._fixtures import GOLDEN
    import json
    import os

    z = np.load(os.path.join(GOLDEN, "bf16_books.npz"))
    d = json.loads(str(z["cfg_json"]))
    d["uid_embedding_hash_sizes"] = tuple(d["uid_embedding_hash_sizes"])
    cfg = O.MoLConfig(**d)
    w = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    mol = build_module(cfg, w, dev, precision).to(torch.bfloat16)
    mol.precision = precision
    q, X = torch.from_numpy(z["q"]).to(dev).bfloat16(), torch.from_numpy(z["X"]).to(dev).bfloat16()
    ids = torch.arange(X.shape[1], dtype=torch.int64, device=dev).unsqueeze(0)
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
        logits = tk.all_logits(q).cpu()
        _, top = tk(q, k=200)
    assert float((logits - torch.from_numpy(z["logits_fp32_run_on_bf16_operands"])).abs().max()) <= LOGIT_TOL
    assert float((logits - torch.from_numpy(z["logits_bf16_run"])).abs().max()) <= 0.15
    ref_top = torch.from_numpy(z["top200_idx_bf16_run"])
    overlap = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(top.cpu(), ref_top)) / ref_top.numel()
    assert overlap >= 0.85, overlap


def test_index_follows_parameter_updates(dev):
    fx = Fixture("c3_books")
    mol = build_module(fx.cfg, fx.weights, dev)
    q, X, ids = fx.t("q").to(dev), fx.t("X").to(dev), fx.t("item_ids").to(dev)
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
        before = tk.all_logits(q).clone()
    w2 = {k: v.clone() for k, v in fx.weights.items()}
    w2["_item_embeddings_fn._item_emb_proj_module.1.weight"] *= 0.5
    w2["_gating_fn._qi_partial_module.3.bias"] += 0.25
    mol.load_state_dict(w2)                       # in-place update, as train-time eval does between epochs
    with torch.inference_mode():
        after = tk.all_logits(q)
    ref = O.mol_logits(fx.cfg, w2, fx.t("q"), fx.t("X"))
    assert float((after.cpu() - ref).abs().max()) <= LOGIT_TOL
    assert float((after - before).abs().max()) > 1e-3
    # the same for an optimizer-style in-place edit and for a `.data` swap (the engine check walks a cached parameter list)
    name = "_gating_fn._qi_partial_module.1.bias"
    prm = dict(mol.named_parameters())[name]
    with torch.no_grad():
        prm.add_(0.125)
    w2[name] = w2[name] + 0.125
    with torch.inference_mode():
        third = tk.all_logits(q)
    assert float((third.cpu() - O.mol_logits(fx.cfg, w2, fx.t("q"), fx.t("X"))).abs().max()) <= LOGIT_TOL
    prm.data = (prm.data * 2.0).clone()
    w2[name] = w2[name] * 2.0
    with torch.inference_mode():
        fourth = tk.all_logits(q)
    assert float((fourth.cpu() - O.mol_logits(fx.cfg, w2, fx.t("q"), fx.t("X"))).abs().max()) <= LOGIT_TOL
    assert float((fourth - third).abs().max()) > 1e-4
    # load_state_dict INSIDE torch.inference_mode(): the in-place copy bumps no version counter there (bench.py's recall leg reloads
    # planted-structure weights that way; the old engine kept scoring with the previous weights before round 4)
    w5 = {k: v.clone() for k, v in w2.items()}
    w5["_gating_fn._qi_partial_module.3.weight"] *= 0.25
    with torch.inference_mode():
        mol.load_state_dict({k: v.to(dev) for k, v in w5.items()})
        fifth = tk.all_logits(q)
    assert float((fifth.cpu() - O.mol_logits(fx.cfg, w5, fx.t("q"), fx.t("X"))).abs().max()) <= LOGIT_TOL
    assert float((fifth - fourth).abs().max()) > 1e-4


@pytest.mark.parametrize("precision", PRECISIONS)
def test_multi_million_item_corpus(dev, precision):
    """3 M items (3.8 GB index): 64-bit addressing of tiles / logits, radix top-k over a long row."""
    cfg = O.CONFIGS["amzn-books"]
    w = O.synthetic_weights(cfg, seed=6)
    mol = build_module(cfg, w, dev, precision)
    N, B, k = 3_000_001, 4, 500
    X = torch.cat([torch.from_numpy(O.hash_item_table(8, s, min(500_000, N - s), cfg.item_embedding_dim)) for s in range(0, N, 500_000)])
    q = O.synthetic_queries(cfg, B, seed=11)
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X.unsqueeze(0).to(dev), torch.arange(N, dtype=torch.int64).unsqueeze(0).to(dev))
        logits = tk.all_logits(q.to(dev))
        s, i = tk(q.to(dev), k=k)
    cols = torch.tensor([0, 1, 31, 32, 1_048_575, 1_048_576, 2_147_483 , N - 2, N - 1])
    g = torch.Generator().manual_seed(2)
    cols = torch.cat([cols, torch.randint(0, N, (2048,), generator=g)])
    ref = O.mol_logits(cfg, w, q, X[cols].unsqueeze(0))
    assert float((logits[:, cols.to(dev)].cpu() - ref).abs().max()) <= LOGIT_TOL
    rs, ri = O.select_topk_deterministic(logits.cpu(), k)
    assert torch.equal(s.cpu(), rs) and torch.equal(i.cpu(), ri)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_million_item_corpus_16x16x64(dev, precision):
    """BASELINE config 4's shape at 1 M items (a 2.2 GB index, 31 251 tiles): the k-split fp32 kernel and the f16x3 big-L kernel
    over a corpus far beyond the fixture's, XCD-aware unit numbering included; sampled columns against the oracle."""
    cfg = O.CONFIGS["synthetic-16x16x64"]
    w = O.synthetic_weights(cfg, seed=12)
    mol = build_module(cfg, w, dev, precision)
    N, B, k = 1_000_001, 5, 200
    X = torch.cat([torch.from_numpy(O.hash_item_table(13, s0, min(250_000, N - s0), cfg.item_embedding_dim)) for s0 in range(0, N, 250_000)])
    q = O.synthetic_queries(cfg, B, seed=17)
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X.unsqueeze(0).to(dev), torch.arange(N, dtype=torch.int64).unsqueeze(0).to(dev))
        logits = tk.all_logits(q.to(dev))
        s, i = tk(q.to(dev), k=k)
    g = torch.Generator().manual_seed(3)
    cols = torch.cat([torch.tensor([0, 31, 32, 524_287, 524_288, N - 2, N - 1]), torch.randint(0, N, (1024,), generator=g)])
    ref = O.mol_logits(cfg, w, q, X[cols].unsqueeze(0))
    assert float((logits[:, cols.to(dev)].cpu() - ref).abs().max()) <= LOGIT_TOL
    rs, ri = O.select_topk_deterministic(logits.cpu(), k)
    assert torch.equal(s.cpu(), rs) and torch.equal(i.cpu(), ri)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_degenerate_sizes(dev, precision):
    fx = Fixture("c3_books")
    mol = build_module(fx.cfg, fx.weights, dev, precision)
    X, ids = fx.t("X")[:, :1].to(dev), fx.t("item_ids")[:, :1].to(dev)     # a corpus of one item
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
        s, i = tk(fx.t("q")[:1].to(dev), k=1)
    ref = O.mol_logits(fx.cfg, fx.weights, fx.t("q")[:1], fx.t("X")[:, :1])
    assert abs(float(s) - float(ref)) <= LOGIT_TOL and int(i) == int(fx.t("item_ids")[0, 0])


# ---- model variants and shapes beyond the BASELINE configs ---------------------------------------------------------
def _module_for(cfg, w, dev, precision):
    mol, _ = rails_amd.create_mol_interaction_module(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
        cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
        cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
        gating_query_fn=cfg.gating_query_fn, gating_item_fn=cfg.gating_item_fn, query_nonlinearity=cfg.query_nonlinearity,
        item_nonlinearity=cfg.item_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None,
        gating_combination_type=cfg.gating_combination_type)
    mol.load_state_dict(w, strict=True)
    mol = mol.to(dev).eval()
    mol.precision = precision
    return mol


@pytest.mark.parametrize("precision", PRECISIONS)
def test_model_variants_against_the_reference(dev, precision):
    """tests/golden/variants.npz: the reference's outputs for a plain-Linear query projection (8x8x64), a GLU item projection
    (8x4x32), gating_combination_type "none" (16x4x32, both precisions) and a 64-wide pair gate (8x4x64)."""
    from tests._fixtures import variant_cases

    for name, cfg, w, a in variant_cases():
        if cfg.gating_qi_hidden_dim <= 0 and precision != "fp32":     # the pair gate without hidden layer is an exact-fp32 build
            with pytest.raises(NotImplementedError, match="without hidden layer"):
                _module_for(cfg, w, dev, precision).engine()
            continue
        mol = _module_for(cfg, w, dev, precision)
        with torch.inference_mode():
            logits, _ = mol(a["q"].to(dev), a["X"].to(dev))
            rows, _ = mol(a["q"].to(dev), a["cand"].to(dev))
            eq, _ = mol.get_query_component_embeddings(a["q"].to(dev))
            ex, _ = mol.get_item_component_embeddings(a["X"].to(dev))
        assert float((logits.cpu() - a["logits"]).abs().max()) <= LOGIT_TOL, name
        assert float((rows.cpu() - a["row_logits"]).abs().max()) <= LOGIT_TOL, name
        assert float((eq.cpu() - a["Eq"]).abs().max()) <= STAGE_TOL and float((ex.cpu() - a["Ex"]).abs().max()) <= STAGE_TOL, name
    with pytest.raises(NotImplementedError, match="without hidden layer"):      # ... and only for the shapes of MOL_NOHID_SHAPES
        m0, _ = rails_amd.create_mol_interaction_module(64, 64, 16, 8, 8, 0.05, 0.0, 512, 0.1, -1, 128, -1, 128, 0.2, False)
        m0.to(dev).eval().engine()


_FUZZ_SHAPES = [(8, 4, 64, 128), (8, 4, 128, 128), (8, 8, 32, 128), (16, 16, 64, 128),          # the tuned shapes
                (8, 4, 32, 128), (8, 8, 16, 128), (8, 8, 64, 128), (8, 8, 128, 128), (8, 8, 48, 128), (8, 4, 16, 128),
                (16, 2, 64, 128), (16, 4, 32, 128), (16, 4, 64, 128), (32, 2, 32, 128), (8, 8, 32, 64), (8, 4, 64, 64)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", _FUZZ_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_shape_fuzz(dev, shape, precision):
    """Every built (P_Q, P_X, d, H) in both precisions (32 kernels' worth): random dims of the outer layers, a ragged corpus,
    a batch that leaves the last query group partial, shared-corpus and per-row-candidate scoring against the oracle."""
    pq, px, d, h = shape
    g = torch.Generator().manual_seed(pq * 1000 + px * 100 + d + h)
    dq, di = int(torch.randint(24, 96, (1,), generator=g)), int(torch.randint(24, 96, (1,), generator=g))
    cfg = O.MoLConfig(dq, di, d, pq, px, gating_qi_hidden_dim=h, query_hidden_dim=int(torch.randint(1, 5, (1,), generator=g)) * 64,
                      gating_query_hidden_dim=int(torch.randint(1, 4, (1,), generator=g)) * 32,
                      gating_item_hidden_dim=int(torch.randint(1, 4, (1,), generator=g)) * 32,
                      query_nonlinearity=("geglu", "swiglu")[int(torch.randint(0, 2, (1,), generator=g))])
    w = O.synthetic_weights(cfg, seed=pq + px + d)
    for key in list(w):   # non-zero biases
        if key.endswith("bias") or key.endswith("_b"):
            w[key] = torch.randn(w[key].shape, generator=g) * 0.05
    mol = _module_for(cfg, w, dev, precision)
    B, N = int(torch.randint(1, 42, (1,), generator=g)), int(torch.randint(33, 900, (1,), generator=g))
    X = torch.from_numpy(O.hash_item_table(pq + d, 0, N, di)).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=px + h)
    cand = X.squeeze(0)[torch.randint(0, N, (B, 37), generator=g)]
    with torch.inference_mode():
        got, _ = mol(q.to(dev), X.to(dev))
        rows, _ = mol(q.to(dev), cand.to(dev))
    assert float((got.cpu() - O.mol_logits(cfg, w, q, X)).abs().max()) <= LOGIT_TOL
    assert float((rows.cpu() - O.mol_logits(cfg, w, q, cand)).abs().max()) <= LOGIT_TOL


F16X1_TOL = 0.1     # one-product f16 first pass: logits in [-20, 20] within 0.1 (observed <= 4.3e-2 on the full amzn-books corpus)


@pytest.mark.parametrize("shape", _FUZZ_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_one_product_first_pass_is_close_on_every_shape(dev, shape):
    """The "f16-exact" mode hides a wrong first pass behind its fp32 fallback (as lost speed, not as wrong results), so the
    one-product kernels (precision "f16x1": never returned to a caller) are held to the oracle on their own: every built shape,
    dense scoring over a ragged corpus with a partial last query group, |logit - oracle| <= 0.1 and a mean below 0.01."""
    pq, px, d, h = shape
    g = torch.Generator().manual_seed(7 + pq * 1000 + px * 100 + d + h)
    cfg = O.MoLConfig(64, 48, d, pq, px, gating_qi_hidden_dim=h, query_hidden_dim=128, gating_query_hidden_dim=64, gating_item_hidden_dim=32)
    w = O.synthetic_weights(cfg, seed=pq + px + d + 1)
    mol = _module_for(cfg, w, dev, "f16x1")
    B, N = int(torch.randint(1, 42, (1,), generator=g)), int(torch.randint(200, 1500, (1,), generator=g))
    X = torch.from_numpy(O.hash_item_table(pq + d + 1, 0, N, 48)).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=px + h + 1)
    with torch.inference_mode():
        got, _ = mol(q.to(dev), X.to(dev))
    err = (got.cpu() - O.mol_logits(cfg, w, q, X)).abs()
    assert float(err.max()) <= F16X1_TOL and float(err.mean()) <= 0.01, (float(err.max()), float(err.mean()))
    assert float(err.max()) > 1e-4          # it IS the one-product build that ran, not the f16x3 one


# ---- opt-in precision mode "f16x3" --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_ml1m", "c2_ml20m", "c3_books"])
def test_f16x3_mode_holds_the_logit_tolerance(dev, name):
    """The split-f16 gate MLP must meet the same 1e-4 bar as the exact fp32 kernels, on the golden vectors."""
    fx = Fixture(name)
    mol = build_module(fx.cfg, fx.weights, dev)
    mol.precision = "f16x3"
    X, ids, q = fx.t("X").to(dev), fx.t("item_ids").to(dev), fx.t("q").to(dev)
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
        logits = tk.all_logits(q, **kw_dev(fx, dev))
        assert tk._engine.precision == "f16x3"
        d = float((logits.cpu() - fx.t("F2/all_logits")).abs().max())
        assert d <= LOGIT_TOL, d
        s, i = tk(q, k=200, **kw_dev(fx, dev))
        assert_topk_matches(s, i, fx.t("F2/k200/scores"), fx.t("F2/k200/ids"), atol=LOGIT_TOL, tie_tol=1e-4)
        cand = fx.t("X").squeeze(0)[fx.t("F6/cand_idx")].to(dev)
        rows, _ = mol(q, cand, **kw_dev(fx, dev))
        assert float((rows.cpu() - fx.t("F6/logits")).abs().max()) <= LOGIT_TOL


def test_f16x3_softmax_overflow_guard(dev):
    """The f16x3 kernel takes softmax numerators without the maximum subtraction and falls back to the stable form when one
    overflows (gate logits > 88).  Force that with a huge pair-gate output bias on one logit: results must stay finite and
    equal the oracle's (which uses torch's stable softmax)."""
    cfg = O.CONFIGS["amzn-books"]
    w = {k: v.clone() for k, v in O.synthetic_weights(cfg, seed=8).items()}
    # w = g*sigmoid(g) ~ 200 on one logit -> exp overflows fp32 without a shift.  (One, not two: the softmax between two
    # logits of magnitude 200 amplifies the fp32 rounding of g itself beyond 1e-4 in ANY fp32 implementation.)
    w["_gating_fn._qi_partial_module.3.bias"][5] = 200.0
    mol = build_module(cfg, w, dev, "f16x3")
    N, B = 1000, 9
    X = torch.from_numpy(O.hash_item_table(4, 0, N, cfg.item_embedding_dim)).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=3)
    with torch.inference_mode():
        got, _ = mol(q.to(dev), X.to(dev))
    ref = O.mol_logits(cfg, w, q, X)
    assert bool(torch.isfinite(got).all())
    assert float((got.cpu() - ref).abs().max()) <= LOGIT_TOL


def test_pack_and_merge_candidates_equal_the_unsharded_topk(dev):
    """Message pack + merge kernels (the two HIP launches around the single all-gather of the sharded path)."""
    from rails_amd.sharded import pack_candidates, shard_bounds

    g = torch.Generator().manual_seed(3)
    rows, n, k, R = 5, 9000, 300, 4
    scores = torch.randint(0, 50, (rows, n), generator=g).float() / 7.0        # ties across shards
    ids = torch.arange(n, dtype=torch.int64) * 2 + 5
    msgs = []
    for r in range(R):
        lo, hi = shard_bounds(n, R, r)
        s, i = E.topk(scores[:, lo:hi].to(dev), min(k, hi - lo), ids=ids[lo:hi].to(dev))
        m = E.pack_candidates(s, i, k)
        assert torch.equal(m.cpu(), pack_candidates(s.cpu(), i.cpu(), k))       # same wire format as the torch version
        msgs.append(m)
    ms, mi = E.merge_candidates(torch.cat(msgs, 0), R, k, k)
    rs, rpos = O.select_topk_deterministic(scores, k)
    assert torch.equal(ms.cpu(), rs) and torch.equal(mi.cpu(), ids[rpos])
    # k_out < k, and R = 8 lists of 200 (the amzn-books 8-GPU shape)
    ms2, mi2 = E.merge_candidates(torch.cat(msgs, 0), R, k, 120)
    assert torch.equal(ms2.cpu(), rs[:, :120]) and torch.equal(mi2.cpu(), ids[rpos][:, :120])
    # the C entry point also accepts lists that are NOT sorted (takes the bitonic sort): distinct scores, shuffled lists
    sc = torch.rand((3, 8 * 200), generator=g)
    gid = torch.arange(8 * 200, dtype=torch.int64).repeat(3, 1) + 11
    msg_sorted, msg_shuffled = [], []
    for r in range(8):
        blk, bid = sc[:, r * 200:(r + 1) * 200], gid[:, r * 200:(r + 1) * 200]
        o = torch.argsort(blk, dim=1, descending=True)
        msg_sorted.append(pack_candidates(torch.gather(blk, 1, o), torch.gather(bid, 1, o), 200))
        msg_shuffled.append(pack_candidates(blk, bid, 200))
    a_s, a_i = E.merge_candidates(torch.cat(msg_sorted, 0).to(dev), 8, 200, 200)
    b_s, b_i = E.merge_candidates(torch.cat(msg_shuffled, 0).to(dev), 8, 200, 200)
    es, eo = torch.sort(sc, dim=1, descending=True)
    assert torch.equal(a_s.cpu(), es[:, :200]) and torch.equal(a_i.cpu(), torch.gather(gid, 1, eo)[:, :200])
    assert torch.equal(b_s.cpu(), a_s.cpu()) and torch.equal(b_i.cpu(), a_i.cpu())
    # a shard shorter than k pads with (-inf, -1)
    s, i = E.topk(scores[:, :7].to(dev), 7, ids=ids[:7].to(dev))
    m = E.pack_candidates(s, i, 10).cpu()
    assert bool((m[:, 17:] == -1).all()) and bool(torch.isinf(m[:, 7:10].to(torch.int32).view(torch.float32)).all())


# ---- section 8(f) rank 3: the eval harness entry points, against the reference harness's own outputs (F5) -----------
def test_eval_harness_reproduces_the_reference_harness(dev):
    import random

    from rails_amd import eval_harness as H

    fx = Fixture("harness")
    mol = build_module(fx.cfg, fx.weights, dev)
    X, ids, q = fx.t("X").to(dev), fx.t("item_ids"), fx.t("q").to(dev)
    past, target = fx.t("past_ids").to(dev), fx.t("target_ids").to(dev)
    id_to_row = {int(v): j for j, v in enumerate(ids.view(-1).tolist())}

    class StubEncoder:                       # the query encoder is upstream of the path: replay its output
        def encode(self, **kw):
            return q

        def get_item_embeddings(self, item_ids):
            flat = item_ids.reshape(-1).tolist()
            rows = torch.tensor([id_to_row.get(int(v), 0) for v in flat], device=dev)
            return X[0][rows].reshape(item_ids.shape + (X.shape[-1],))

    model = StubEncoder()
    holder = type("M", (), {"_ndp_module": mol})()
    state = H.get_eval_state(model, ids.view(-1).tolist(), None,
                             lambda e, i: rails_amd.get_top_k_module("MoLBruteForceTopK", holder, e, i), dev)
    assert state.candidate_index.num_objects == X.shape[1]
    feats = H.SequentialFeatures(past_lengths=torch.full((q.shape[0],), 61, device=dev), past_ids=past, past_embeddings=None, past_payloads={})
    for mode, timing in (("accuracy", False), ("timing", True)):
        random.seed(1)
        res = H.eval_metrics_v2_from_tensors(state, model, feats, target_ids=target, filter_invalid_ids=True,
                                             include_eval_time=timing, include_eval_top_k_ids=True)
        # k = min(2500, N) returns (nearly) the whole corpus sorted: items whose scores differ by < 1e-5 may swap places,
        # so compare ids position-wise with a small allowance and the metrics (functions of the target's rank) exactly
        same = (res["eval_top_k_ids"].cpu() == fx.t(f"F5/{mode}/eval_top_k_ids")).float().mean()
        assert float(same) >= 0.97, float(same)
        for key in ("hr@1", "hr@5", "hr@10", "hr@50", "hr@100", "hr@200", "hr@500", "hr@1000"):
            assert torch.equal(res[key].cpu(), fx.t(f"F5/{mode}/{key}")), key
        for key in ("ndcg@1", "ndcg@5", "ndcg@10", "ndcg@50", "ndcg@100", "ndcg@200", "mrr"):
            assert torch.allclose(res[key].float().cpu(), fx.t(f"F5/{mode}/{key}").float(), atol=1e-7), key
        if timing:
            assert all(t > 0 for t in res["eval_time"])
    assert abs(float(H._avg(res["hr@10"].float(), 1)) - float(fx.t("F5/timing/hr@10").float().mean())) < 1e-7


GLU_CASES = ["geglu_2d", "swiglu_2d", "geglu_3d", "swiglu_1row"]


@pytest.mark.parametrize("case", GLU_CASES)
def test_glu_layers_standalone_against_the_reference_modules(dev, case):
    """GeGLU / SwiGLU forward on their own (reference layers.py:36-43, :68-74) through rails_glu_f32, against the outputs of the
    reference's modules on the same seeded inputs (tests/golden/glu.npz, oracle/gen_golden_glu.py).  fp32 GEMM with another
    summation order: 2e-6 absolute on outputs of order 1."""
    import os

    import numpy as np

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glu.npz"))
    x, w, b, y = (torch.from_numpy(z[f"{case}.{k}"]) for k in ("x", "w", "b", "y"))
    cls = rails_amd.GeGLU if case.startswith("geglu") else rails_amd.SwiGLU
    m = cls(w.shape[0], w.shape[1] // 2)
    m.load_state_dict({"_w": w, "_b": b})
    m = m.to(dev)
    with torch.inference_mode():
        got = m(x.to(dev))
    assert got.shape == y.shape and got.dtype == y.dtype
    err = float((got.cpu() - y).abs().max())
    assert err <= 2e-6 * max(1.0, float(y.abs().max())), err
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x)


# ---- precision "f16x3-exact": f16x3 candidates, fp32 verification -> the fp32 result bit for bit -------------------------
@pytest.mark.parametrize("workload,N,B,k", [("amzn-books", 695762, 32, 200), ("amzn-books", 100_003, 5, 2561), ("ml-1m", 3649, 8, 120),
                                            ("ml-20m", 26_000, 1, 1), ("amzn-books", 300, 4, 200)])
@pytest.mark.parametrize("mode", ["f16x3-exact", "f16-exact"])
def test_f16x3_exact_equals_the_fp32_path_bit_for_bit(dev, workload, N, B, k, mode):
    """MoLBruteForceTopK in precision "f16x3-exact" / "f16-exact" (one-product first pass) == the same module in fp32: scores, ids and tie order, via forward and via
    CandidateIndex.get_top_k_outputs with the seen-id filter.  The last case (N < k + margin) takes the dense fp32 route."""
    cfg = O.CONFIGS[workload]
    w = O.synthetic_weights(cfg, seed=3)
    X = torch.from_numpy(O.hash_item_table(11, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = (torch.arange(N, dtype=torch.int64, device=dev) * 2 + 5).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=21).to(dev)
    kw = {"user_ids": torch.arange(B, dtype=torch.int64, device=dev)} if cfg.uid_embedding_hash_sizes else {}
    k = min(k, N)
    with torch.inference_mode():
        m32 = build_module(cfg, w, dev, None)
        r_s, r_i = rails_amd.MoLBruteForceTopK(m32, X, ids)(q, k=k, **kw)
        mx = build_module(cfg, w, dev, mode)
        tk = rails_amd.MoLBruteForceTopK(mx, X, ids)
        tk.SPECULATE_MIN_ITEMS = 0          # exercise the speculative route on the small corpora as well
        for _ in range(2):
            s, i = tk(q, k=k, **kw)
            assert torch.equal(s, r_s) and torch.equal(i, r_i)
        if B > 2 and N > 1000:     # a logit budget of two rows: the batch goes through the speculative route in slices
            tk.MAX_LOGIT_BYTES, before = 2 * N * 4, tk.stats()["calls"]
            s, i = tk(q, k=k, **kw)
            assert torch.equal(s, r_s) and torch.equal(i, r_i) and tk.stats()["calls"] == before + (B + 1) // 2
            tk.MAX_LOGIT_BYTES = type(tk).MAX_LOGIT_BYTES
            tk.rescore_stats["calls"] = before
        if N > 1000:
            assert tk.stats()["calls"] == 2 and (tk.rescore_stats["fallbacks"] == 0 or mode == "f16-exact"), tk.rescore_stats
            print(mode, workload, N, B, k, tk.rescore_stats)
            # f16x3-exact runs its verdicts on the A-PRIORI bound (rails_amd/f16x3_bound.py): every cleared call is proved.  The one-product
            # pass has no useful a-priori bound (its operands carry 11 bits): it stays conditional on the monitored eps
            st = tk.stats()
            assert st["eps_rigorous"] >= st["eps_default"] and st["eps_rigorous"] <= 2.0 / cfg.temperature + 1.0
            assert st["eps_rigorous_usable"] is (mode == "f16x3-exact")
            if mode == "f16x3-exact":
                per_pair = st.get("bound_kind") == "per-pair upper bound"       # corpora up to PER_PAIR_MAX_ITEMS: upper bounds per pair, the verdict's eps is 0
                assert per_pair == (N <= rails_amd.MoLBruteForceTopK.PER_PAIR_MAX_ITEMS)
                assert st["proved_calls"] >= 2 - st["fallbacks"] and st["bound_violations"] == 0
                assert st["eps"] == (0.0 if per_pair else pytest.approx(st["eps_rigorous"], rel=1e-4))
        inv = ids[0, torch.randint(0, N, (B, 7), device=dev)]
        kk = min(k, 120)
        ci = rails_amd.CandidateIndex(ids, X)
        a = ci.get_top_k_outputs(q, k=kk, aux_payloads=kw, top_k_module=tk, invalid_ids=inv)
        b = ci.get_top_k_outputs(q, k=kk, aux_payloads=kw, top_k_module=rails_amd.MoLBruteForceTopK(m32, X, ids), invalid_ids=inv)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("mode", ["f16x3-exact", "f16-exact"])
def test_f16x3_exact_ties_and_forced_fallback(dev, mode):
    """Duplicated items tie exactly in fp32 (and may straddle the k-th place): the tie order must still be the dense path's
    (position ascending).  Then the verification is made to fail (eps = inf): the dense fp32 fallback returns the same result."""
    cfg = O.CONFIGS["amzn-books"]
    w = O.synthetic_weights(cfg, seed=4)
    base = torch.from_numpy(O.hash_item_table(12, 0, 2500, cfg.item_embedding_dim))
    X = base.repeat(8, 1).unsqueeze(0).to(dev)              # every item 8 times, 2 500 positions apart
    N = X.shape[1]
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, 16, seed=22).to(dev)
    with torch.inference_mode():
        r_s, r_i = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, None), X, ids)(q, k=204)
        tk = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, mode), X, ids)
        tk.SPECULATE_MIN_ITEMS = 0
        s, i = tk(q, k=204)
        assert torch.equal(s, r_s) and torch.equal(i, r_i)
        assert bool((r_s[:, 0] == r_s[:, 7]).all())           # the ties are real
        before = tk.stats()["fallbacks"]
        if mode == "f16x3-exact":     # the verdicts run on the a-priori bound: make it absurd
            tk._policy = tk._policy._replace(eps=1.0e9)
        else:
            tk.RESCORE_EPS_PER_INV_TEMPERATURE_F16X1 = float("inf")
        s, i = tk(q, k=204)
        assert torch.equal(s, r_s) and torch.equal(i, r_i) and tk.stats()["fallbacks"] == before + 1
        # without the dense fp32 index (memory-tight deployments): the candidates' raw rows are rebuilt instead of gathered
        try:
            rails_amd.MoLBruteForceTopK.KEEP_DENSE_FP32_INDEX = False
            tk2 = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, mode), X, ids)
        finally:
            rails_amd.MoLBruteForceTopK.KEEP_DENSE_FP32_INDEX = None
        assert tk2._index32 is None
        tk2.SPECULATE_MIN_ITEMS = 0
        s, i = tk2(q, k=204)
        assert torch.equal(s, r_s) and torch.equal(i, r_i) and tk2.rescore_stats["calls"] == 1


def test_rescore_select_kernel_against_a_host_restatement(dev):
    """rails_rescore_select on synthetic rows: order (exact desc, position asc) with real ties, id map, and the verdict's
    clauses one by one (margin, candidate mismatch, probe mismatch, NaN)."""
    g = torch.Generator().manual_seed(5)
    rows, n_ranked, n_probe, k, N = 6, 96, 32, 40, 5000
    pos = torch.stack([torch.randperm(N, generator=g)[: n_ranked + n_probe] for _ in range(rows)])
    exact = torch.randn(rows, n_ranked + n_probe, generator=g).mul(3).round(decimals=1)     # many exact ties
    approx_c = exact[:, :n_ranked] + (torch.rand(rows, n_ranked, generator=g) - 0.5) * 1e-4
    dense = torch.zeros(rows, N)
    dense.scatter_(1, pos, exact + (torch.rand(rows, n_ranked + n_probe, generator=g) - 0.5) * 1e-4)
    ids = torch.arange(N) * 7 + 3
    margin, check = 1e-3, 2.5e-4
    # rows: 0 plain ok; 1 margin too small (k-th exact == min approx); 2 one candidate off by 1e-3; 3 one probe off; 4 a NaN; 5 ok
    approx_c[1] = approx_c[1].clamp_min(float(exact[1, :n_ranked].topk(k).values[-1]))
    approx_c[2, 17] += 1e-3
    dense[3, pos[3, n_ranked + 5]] += 1e-3
    exact[4, 3] = float("nan")
    approx_c[0] -= 20.0; dense[0] -= 20.0; approx_c[5] -= 20.0; dense[5] -= 20.0     # rows 0, 5: wide margin ...
    check_big = 25.0                                                                  # ... checked with their own tolerance below
    def run(chk):
        return E.rescore_select(exact.to(dev), approx_c.to(dev), pos.to(dev), ids.to(dev), N, k, margin, chk, approx_dense=dense.to(dev))
    s, i, ok, st = run(check)
    assert ok.cpu().tolist() == [0, 0, 0, 0, 0, 0]           # rows 0 / 5 fail the monitor (shifted by 20), the others by construction
    s, i, ok, st = run(check_big)
    st = st.cpu()
    for r in (1, 2, 3):                                      # row_stats: [largest |exact - approx| incl. probes, k-th exact - min candidate approx]
        e, a = exact[r, :n_ranked], approx_c[r]
        want_err = max(float((e - a).abs().max()), float((exact[r, n_ranked:] - dense[r, pos[r, n_ranked:]]).abs().max()))
        assert abs(float(st[r, 0]) - want_err) <= 1e-6 and abs(float(st[r, 1]) - (float(e.topk(k).values[-1]) - float(a.min()))) <= 1e-6
    assert float(st[4, 0]) == float("inf")                   # a NaN among the exact scores
    assert ok.cpu().tolist() == [1, 0, 1, 1, 0, 1]           # with a loose monitor only the margin (1) and the NaN (4) rows fail
    for r in (0, 2, 3, 5):
        e, p = exact[r, :n_ranked], pos[r, :n_ranked]
        order = sorted(range(n_ranked), key=lambda j: (-float(e[j]), int(p[j])))[:k]
        assert torch.equal(s[r].cpu(), e[order]) and torch.equal(i[r].cpu(), ids[p[order]])
    s2, i2, _, _ = E.rescore_select(exact.to(dev), approx_c.to(dev), pos.to(dev), None, N, k, margin, check_big, approx_dense=dense.to(dev))
    assert torch.equal(i2[5].cpu(), (i[5].cpu() - 3) // 7)    # ids = None -> positions


def test_rescore_select_one_sided_monitors_upper_bounds(dev):
    """one_sided = 1 (the first pass wrote UPPER BOUNDS of the exact scores, rails_mol_score_dense_upper): the error stat is max(0, exact - bound),
    zero while every bound holds however loose it is; margin_eps = 0 is the proof e_k > min candidate bound (strict)."""
    g = torch.Generator().manual_seed(8)
    rows, kc, k, N = 5, 160, 50, 3000
    pos = torch.stack([torch.randperm(N, generator=g)[:kc] for _ in range(rows)])
    exact = torch.randn(rows, kc, generator=g).mul(2)
    upper = exact + torch.rand(rows, kc, generator=g) * 0.8 + 0.05              # loose bounds, all valid
    kth = exact.topk(k).values[:, -1]
    # rows: 0 proved (a gap of 6 below the k-th exact score, so the smallest bound is far below it); 1 margin fails (no candidate bound below
    # e_k); 2 a violated bound (exact above its bound by 0.3); 3 the smallest bound == e_k exactly (strict: not proved); 4 a NaN
    low = exact < kth[:, None]
    exact = torch.where(low, exact - 6.0, exact)
    upper = torch.where(low, upper - 6.0, upper)
    upper[1] = torch.where(low[1], torch.full_like(upper[1], float(kth[1]) + 0.25), upper[1])
    j2 = int(exact[2].argmax())
    upper[2, j2] = exact[2, j2] - 0.3
    upper[3] = torch.where(low[3], torch.full_like(upper[3], float(kth[3])), upper[3])
    exact[4, 7] = float("nan")
    s, i, ok, st = E.rescore_select(exact.to(dev), upper.to(dev), pos.to(dev), None, N, k, 0.0, 0.0, one_sided=True)
    st, ok = st.cpu(), ok.cpu().tolist()
    assert ok == [1, 0, 0, 0, 0]
    assert float(st[0, 0]) == 0.0 and float(st[1, 0]) == 0.0 and float(st[3, 0]) == 0.0            # loose but valid bounds: no error
    assert abs(float(st[2, 0]) - 0.3) <= 1e-6 and float(st[4, 0]) == float("inf")
    assert float(st[0, 1]) > 0.0 and float(st[1, 1]) < 0.0 and float(st[3, 1]) == 0.0
    for r in (0, 1, 2, 3):
        order = sorted(range(kc), key=lambda j: (-float(exact[r, j]), int(pos[r, j])))[:k]
        assert torch.equal(s[r].cpu(), exact[r, order]) and torch.equal(i[r].cpu(), pos[r, order])
    # the two-sided form of the same call counts every loose bound as an error
    _, _, ok2, st2 = E.rescore_select(exact.to(dev), upper.to(dev), pos.to(dev), None, N, k, 0.0, 0.0)
    assert ok2.cpu().tolist() == [0, 0, 0, 0, 0] and float(st2.cpu()[0, 0]) > 0.05


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunked_brute_force_equals_the_one_pass_result(dev, precision):
    """MoLBruteForceTopK never materialises more than MAX_LOGIT_BYTES of logits: above that the corpus is scored in chunks whose
    top-k lists are merged.  Forced here with small limits (ragged last chunk, k larger than the last chunk, duplicated items so
    that equal scores straddle chunk boundaries): must equal the one-pass result bit for bit."""
    cfg = O.CONFIGS["amzn-books"]
    w = O.synthetic_weights(cfg, seed=6)
    base = torch.from_numpy(O.hash_item_table(13, 0, 5000, cfg.item_embedding_dim))
    X = torch.cat([base, base[:3000], base[100:2150]]).unsqueeze(0).to(dev)      # 10 050 items, many exact duplicates
    N = X.shape[1]
    ids = (torch.arange(N, dtype=torch.int64, device=dev) * 3 + 7).unsqueeze(0)
    q = O.synthetic_queries(cfg, 9, seed=23).to(dev)
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, precision), X, ids)
        r_s, r_i = tk(q, k=300)
        tk.MAX_LOGIT_BYTES, tk.CHUNK_ITEMS = 1024, 4096          # chunks of 4096, 4096, 1858 items
        s, i = tk(q, k=300)
        assert torch.equal(s, r_s) and torch.equal(i, r_i)
        tk.CHUNK_ITEMS = 320                                     # 32 chunks, the last one (130 items) shorter than k
        s, i = tk(q, k=300)
        assert torch.equal(s, r_s) and torch.equal(i, r_i)
    with pytest.raises(ValueError, match="tile boundary"):
        tk._index.items(5, 100)


def test_exact_modes_speculate_only_where_it_pays(dev):
    """Policy of the verified fast modes: corpora below SPECULATE_MIN_ITEMS take the dense fp32 kernels at once; a run of failed
    verifications pauses the speculation (dense fp32 for the next 256 calls).  The result is the fp32 result throughout."""
    cfg = O.CONFIGS["amzn-books"]
    w = O.synthetic_weights(cfg, seed=8)
    N = 12_000
    assert N < rails_amd.MoLBruteForceTopK.SPECULATE_MIN_ITEMS
    X = torch.from_numpy(O.hash_item_table(14, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, 4, seed=24).to(dev)
    with torch.inference_mode():
        r_s, r_i = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, None), X, ids)(q, k=50)
        tk = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, "f16-exact"), X, ids)
        s, i = tk(q, k=50)
        assert torch.equal(s, r_s) and torch.equal(i, r_i) and tk.rescore_stats["calls"] == 0      # 12 000 items: dense fp32
        tk.SPECULATE_MIN_ITEMS = 0
        tk.RESCORE_EPS_PER_INV_TEMPERATURE_F16X1 = float("inf")                                     # every verification fails
        for _ in range(20):
            s, i = tk(q, k=50)
            assert torch.equal(s, r_s) and torch.equal(i, r_i)
            tk.stats()      # the verdicts are folded in lazily (no host wait inside forward): bring them in before the next call decides
        assert tk.rescore_stats["calls"] == 16 and tk.rescore_stats["fallbacks"] == 16 and tk.rescore_stats["paused_calls"] == 4


@pytest.mark.parametrize("workload", ["amzn-books", "ml-20m", "ml-1m"])
@pytest.mark.parametrize("B", [1, 7, 32])
def test_query_prologue_both_formats(dev, workload, B):
    """rails_mol_query_prologue_both: the second pack is bit for bit what the other-precision prologue writes (per-query and
    batched implementations, uid embeddings, partial last query group)."""
    cfg = O.CONFIGS[workload]
    w = O.synthetic_weights(cfg, seed=9)
    q = O.synthetic_queries(cfg, B, seed=25).to(dev)
    uid = torch.arange(B, dtype=torch.int64, device=dev) * 13 if cfg.uid_embedding_hash_sizes else None
    with torch.inference_mode():
        e16 = build_module(cfg, w, dev, "f16x3").engine()
        e32 = build_module(cfg, w, dev, None).engine()
        n = e16.lib.rails_mol_query_pack_floats(E.C.byref(e16.shape), B)
        assert n == e32.lib.rails_mol_query_pack_floats(E.C.byref(e32.shape), B)
        a, b = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        e16.query_pack_both(q, uid, a, b)
        r16, _, _ = e16.query_pack(q, uid)
        r32, _, _ = e32.query_pack(q, uid)
        # compare the fragment part (the tail of the pack is the prologue's scratch)
        L = cfg.query_dot_product_groups * cfg.item_dot_product_groups
        qt = 32 // cfg.query_dot_product_groups
        n_frag = (B + qt - 1) // qt * 32 * cfg.dot_product_dimension + B * L
        assert torch.equal(a[:n_frag].view(torch.int32), r16[:n_frag].view(torch.int32))
        assert torch.equal(b[:n_frag].view(torch.int32), r32[:n_frag].view(torch.int32))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_pass_batches_beyond_one_query_tile(dev, precision):
    """B > 32 keeps several query tiles in the coarse scan (one read of the table, query tiles inside): the fused scan, the
    materialising path and the 32-query slices of the same batch must all agree, bit for bit (B = 100: a partial fourth tile)."""
    cfg = O.CONFIGS["amzn-books"]
    w = O.synthetic_weights(cfg, seed=10)
    N, B = 300_017, 100
    X = torch.from_numpy(O.hash_item_table(15, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=26).to(dev)
    with torch.inference_mode():
        at = rails_amd.MoLAvgTopK(build_module(cfg, w, dev, precision), X, ids, avg_top_k=500)
        s, i = at(q, k=100)
        cs, cp = at.coarse_candidates(q)
        parts = [at(q[b0 : b0 + 32], k=100) for b0 in range(0, B, 32)]
        assert torch.equal(s, torch.cat([p[0] for p in parts])) and torch.equal(i, torch.cat([p[1] for p in parts]))
        at._no_fused = True                       # the materialising path: (B, N) coarse scores + rails_topk
        s2, i2 = at(q, k=100)
        cs2, cp2 = at.coarse_candidates(q)
        at._no_fused = False
        assert torch.equal(s, s2) and torch.equal(i, i2) and torch.equal(cs, cs2) and torch.equal(cp, cp2)


@pytest.mark.parametrize("mode", ["f16x3-exact", "f16-exact"])
@pytest.mark.parametrize("gain", [3.0, 10.0])
def test_exact_modes_under_stressed_gate_weights(dev, mode, gain):
    """Pair-gate weights scaled far beyond their initialisation make the first pass's error grow past the calibrated bound: the
    monitor must notice and the fallback must keep the result equal to the fp32 path's (fallbacks are allowed here, wrong
    results are not)."""
    cfg = O.CONFIGS["amzn-books"]
    w = dict(O.synthetic_weights(cfg, seed=11))
    for key in ("_gating_fn._qi_partial_module.1.weight", "_gating_fn._qi_partial_module.3.weight"):
        w[key] = w[key] * gain
    N, B, k = 150_000, 16, 200
    X = torch.from_numpy(O.hash_item_table(16, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=27).to(dev)
    with torch.inference_mode():
        r_s, r_i = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, None), X, ids)(q, k=k)
        tk = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, mode), X, ids)
        for _ in range(6):
            s, i = tk(q, k=k)
            assert torch.equal(s, r_s) and torch.equal(i, r_i)
        print(mode, "gate gain", gain, tk.stats(), "pad scale", tk._pad_scale)
        st = tk.stats()
        if mode == "f16x3-exact":   # a-priori bound (it grows with the square of the gain): what is not proved is redone, and counted as such
            assert st["proved_calls"] + st["fallbacks"] + st.get("paused_calls", 0) + st.get("unprovable_calls", 0) >= 6 and st["bound_violations"] == 0, st
        elif gain <= 3.0:      # the monitored bound calibrates itself: after at most a couple of redone calls the speculation holds
            assert st["fallbacks"] <= 2, tk.rescore_stats


@pytest.mark.parametrize("gain", [2.0, 3.0, 5.0])
def test_f16_kernels_near_the_exp_overflow(dev, gain):
    """Gate logits just under the fp32 exp overflow (pair-gate weights x 3 on this model): the un-shifted softmax sum is still
    finite there, but its product with the cross logits overflows and 1/den is a flushed denormal -- the overflow guard must
    take the stable form before that.  (x 3 produced 1 084 non-finite logits of 2.4 M with the guard at FLT_MAX; x 5 overflows
    the sum itself and was always caught.)  Both f16 builds: finite everywhere and as close to fp32 as their precision allows."""
    cfg = O.CONFIGS["amzn-books"]
    w = dict(O.synthetic_weights(cfg, seed=11))
    for key in ("_gating_fn._qi_partial_module.1.weight", "_gating_fn._qi_partial_module.3.weight"):
        w[key] = w[key] * gain
    N, B = 150_000, 16
    X = torch.from_numpy(O.hash_item_table(16, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=27).to(dev)
    with torch.inference_mode():
        ref = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, None), X, ids).all_logits(q)
        assert bool(torch.isfinite(ref).all())
        for pr, tol in (("f16x3", 2e-4 * gain), ("f16x1", 0.15 * gain)):
            got = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, pr), X, ids).all_logits(q)
            assert bool(torch.isfinite(got).all()), pr
            assert float((got - ref).abs().max()) <= tol, (pr, float((got - ref).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16-exact"])     # the MONITORED mode; the proved mode's counterpart is tests/test_proved_gpu.py::test_proved_mode_unprovable_calls_fall_back
def test_exact_modes_against_planted_first_pass_outliers(dev, mode):
    """What the monitored mode rests on is |first pass - fp32| <= eps for every item OUTSIDE the candidates.  Plant violations: the first
    pass is made to under-score true top-k items by far more than eps (a test hook subtracts from their first-pass logits), so
    they drop out of the candidate set while their exact scores belong in the result.
      (a) outliers among the highest-norm items of the corpus: those are probed on every call -> the error is seen, eps widens
          past the margin, the call falls back, the result is the fp32 path's;
      (b) an outlier nothing probes: the verification cannot see it (the guarantee is conditional on the monitored bound, as the
          docs say) -- the shadow audit does: with audit_every = 1 the mismatch is counted."""
    cfg = O.CONFIGS["amzn-books"]
    w = O.synthetic_weights(cfg, seed=11)
    N, B, k = 120_000, 8, 100
    Xc = torch.from_numpy(O.hash_item_table(16, 0, N, cfg.item_embedding_dim))
    q = O.synthetic_queries(cfg, B, seed=27).to(dev)
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    with torch.inference_mode():
        ref0 = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, None), Xc.unsqueeze(0).to(dev), ids)
        _, top_i = ref0(q, k=k)
        # items that are in the fp32 top-k of row 0 (positions = id - 1)
        victims = (top_i[0, :3] - 1).cpu()
        # (a) make the victims the highest-norm rows of the table (the scores barely move: Ex is l2-normalised, scale 1.02)
        Xa = Xc.clone()
        Xa[victims] *= 1.02 * float(Xc.norm(dim=1).max() / Xc[victims].norm(dim=1).min())
        Xa = Xa.unsqueeze(0).to(dev)
        r_s, r_i = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, None), Xa, ids)(q, k=k)
        tk = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, mode), Xa, ids)
        tk.SPECULATE_MIN_ITEMS = 0
        tk._debug_first_pass_bias = (victims.to(dev), 5.0)
        s, i = tk(q, k=k)
        assert torch.equal(s, r_s) and torch.equal(i, r_i)
        assert tk.stats()["fallbacks"] == 1 and tk.rescore_stats["eps"] > 5.0, tk.rescore_stats
        # (b) an outlier of ordinary norm that no probe covers: only the audit notices
        Xb = Xc.unsqueeze(0).to(dev)
        r_s, r_i = ref0(q, k=k)
        tk = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, mode), Xb, ids)
        tk.SPECULATE_MIN_ITEMS = 0
        tk.audit_every = 1
        s, i = tk(q, k=k)                      # clean call: verified and audited, no mismatch
        assert torch.equal(s, r_s) and torch.equal(i, r_i)
        assert tk.audit_summary()["audited"] == 1 and tk.audit_summary()["mismatches"] == 0
        probed = set(torch.cat(tk._probes(B, N), dim=1).reshape(-1).tolist()) | set(tk._risk_pool[: tk.RISK_ALWAYS].tolist())
        lone = next(int(v) for v in (top_i[0] - 1).tolist() if int(v) not in probed)
        tk._debug_first_pass_bias = (torch.tensor([lone], device=dev), 5.0)
        s, i = tk(q, k=k)
        if tk.stats()["fallbacks"] == 0:   # the planted error went unseen by the verification ...
            assert not torch.equal(i, r_i)
            assert tk.audit_summary()["mismatches"] == 1, tk.rescore_stats   # ... and was caught by the audit
        else:
            assert torch.equal(s, r_s) and torch.equal(i, r_i)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gating_combination_none_at_256_logits(dev, precision):
    """gating_combination_type "none" (reference rails/similarities/mol/similarity_fn.py:187-197) on the 16x16x64 team kernel, both
    precisions, against the oracle (whose "none" branch is pinned on the reference by tests/golden/variants.npz at 16x4x32)."""
    import dataclasses

    cfg = dataclasses.replace(O.CONFIGS["synthetic-16x16x64"], gating_combination_type="none")
    w = O.synthetic_weights(cfg, seed=13)
    N, B = 777, 5
    X = torch.from_numpy(O.hash_item_table(18, 0, N, cfg.item_embedding_dim))
    q = O.synthetic_queries(cfg, B, seed=31)
    ref = O.mol_logits(cfg, w, q, X.unsqueeze(0))
    mol = _module_for(cfg, w, dev, precision)
    with torch.inference_mode():
        got, _ = mol(q.to(dev), X.unsqueeze(0).to(dev))
    assert float((got.cpu() - ref).abs().max()) <= LOGIT_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name", ["ml-1m", "amzn-books"])
def test_gating_combination_none_on_every_fp32_shell(dev, monkeypatch, cfg_name):
    """gating_combination_type "none" (similarity_fn.py:187-197; with and without the query-only / item-only gate parts) through the
    small-unit shell, the independent-wave 32x32x2 shell and the dispatcher's choice: same bits, within 1e-4 of the oracle."""
    import dataclasses

    for has_q, has_i in ((True, True), (False, False)):
        cfg = dataclasses.replace(O.CONFIGS[cfg_name], gating_combination_type="none", gating_query_fn=has_q, gating_item_fn=has_i)
        w = O.synthetic_weights(cfg, seed=17)
        N, B = 1234, 7
        X = torch.from_numpy(O.hash_item_table(19, 0, N, cfg.item_embedding_dim))
        q = O.synthetic_queries(cfg, B, seed=33)
        uid = torch.arange(B, dtype=torch.int64) * 11 if cfg.uid_embedding_hash_sizes else None
        ref = O.mol_logits(cfg, w, q, X.unsqueeze(0), uid)
        mol = _module_for(cfg, w, dev, "fp32")
        outs = {}
        with torch.inference_mode():
            eng = mol.engine()
            index = eng.build_index(X.to(dev))
            qpack, _, _ = eng.query_pack(q.to(dev), None if uid is None else uid.to(dev))
            for variant in ("7", "1", "0"):
                monkeypatch.setenv("RAILS_SCORE_VARIANT", variant)
                outs[variant] = eng.score_dense(qpack, B, index).clone()
        assert torch.equal(outs["7"], outs["1"]) and torch.equal(outs["7"], outs["0"])
        assert float((outs["7"].cpu() - ref).abs().max()) <= LOGIT_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("rows,n,kp,width,k", [(4, 5000, 200, 61, 120), (32, 200_000, 200, 61, 120), (3, 30_000, 512, 211, 300), (2, 3883, 200, 211, 120),
                                               (5, 27_278, 25, 30, 20), (2, 1500, 10, 1, 10), (3, 100_003, 331, 256, 331)])
def test_fused_topk_filter_equals_the_two_kernels(dev, rows, n, kp, width, k):
    """rails_topk_filtered == rails_topk followed by rails_filter_seen_ids, bit for bit: seen ids among the winners (dropped), fewer than
    k unseen winners (back-fill), ties, both the one-launch and the two-level selection."""
    g = torch.Generator().manual_seed(rows * 1000 + kp)
    scores = torch.randn((rows, n), generator=g)
    m = scores[:, 1::7].shape[1]
    scores[:, ::7][:, :m] = scores[:, 1::7]                                  # ties
    scores = scores.to(dev)
    ids = (torch.randperm(n, generator=g) * 3 + 5).to(dev)
    s_ref, i_ref = E.topk(scores, kp, ids=ids)
    for frac in (0.0, 0.3, 0.95):                                            # share of each row's seen-id slots filled with its own winners
        inv = torch.zeros((rows, width), dtype=torch.int64)
        n_fill = min(int(width * frac), kp)
        for r in range(rows):
            sel = torch.randperm(kp, generator=g)[:n_fill]
            inv[r, :n_fill] = i_ref[r].cpu()[sel]
        inv = inv.to(dev)
        assert E.topk_filter_fusable(n, kp, width, k)
        want_i, want_s = E.filter_seen_ids(i_ref, s_ref, inv, k)
        got_i, got_s = E.topk_filtered(scores, kp, ids, inv, k)
        assert torch.equal(got_i, want_i) and torch.equal(got_s, want_s), (frac, int((got_i != want_i).sum()))
    assert not E.topk_filter_fusable(n, 600, width, k) and not E.topk_filter_fusable(500, min(kp, 500), width, min(k, 500))


@pytest.mark.gpu
def test_standalone_module_forwards(fx, mol, dev):
    """The pieces of MoLSimilarity called on their own, against the reference's stage outputs (fixture F1): the embeddings fns, the
    gating fn on materialised cross logits, and the softmax combiner on the reference's gating weights.  (MoLSimilarity.forward never
    materialises these tensors; the stand-alone forwards exist for callers that do.)"""
    n = int(fx.z["F1/n"])
    q, X = fx.t("q").to(dev), fx.t("X")[:, :n].to(dev)
    cl, w, ref = fx.t("F1/cl").to(dev), fx.t("F1/w").to(dev), fx.t("F1/logits")
    with torch.inference_mode():
        eq, aux_q = mol._query_embeddings_fn(q, **kw_dev(fx, dev))
        ex, aux_x = mol._item_embeddings_fn(X)
        out_c, aux_c = mol._gating_fn._normalization_fn(w, cl)
        out_g, aux_g = mol._gating_fn(cl, q, X)
        out_b, _ = mol._gating_fn(cl, q, X.expand(q.shape[0], -1, -1).contiguous())      # per-row item embeddings (B' = B)
    assert aux_q == {} and aux_x == {} and aux_c == {} and aux_g == {}
    assert float((eq.cpu() - fx.t("F1/Eq")).abs().max()) <= STAGE_TOL and float((ex.cpu() - fx.t("F1/Ex")).abs().max()) <= STAGE_TOL
    for name, got in (("combiner", out_c), ("gating fn", out_g), ("gating fn, per-row items", out_b)):
        assert got.shape == ref.shape and float((got.cpu() - ref).abs().max()) <= LOGIT_TOL, (fx.name, name, float((got.cpu() - ref).abs().max()))


# ---- hand-driven kernels on a dense binding --------------------------------------------------------------------------------------
def _dense_case(cfg_name, N, B, dev, precision, seed=31, dup=1):
    cfg = O.CONFIGS[cfg_name]
    w = O.synthetic_weights(cfg, seed=seed)
    base = torch.from_numpy(O.hash_item_table(seed, 0, (N + dup - 1) // dup, cfg.item_embedding_dim))
    X = base.repeat(dup, 1)[:N].unsqueeze(0).to(dev)
    ids = (torch.arange(N, dtype=torch.int64, device=dev) * 5 + 3).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=seed + 1).to(dev)
    kw = {"user_ids": torch.arange(B, dtype=torch.int64, device=dev) * 7 + 1} if cfg.uid_embedding_hash_sizes else {}
    tk = rails_amd.MoLBruteForceTopK(build_module(cfg, w, dev, precision), X, ids, exact_mode="dense")   # the callers drive this engine's kernels by hand
    return cfg, tk, q, kw


@pytest.mark.gpu
@pytest.mark.parametrize("R,rows,k,width,k_out", [(2, 9, 200, 61, 120), (8, 32, 200, 61, 120), (4, 5, 64, 211, 50), (3, 7, 512, 1, 512), (8, 3, 25, 256, 20)])
def test_filtered_merge_equals_merge_then_filter(dev, R, rows, k, width, k_out):
    """rails_merge_candidates_filtered (the seen-id filter inside the shard-merge launch) against rails_merge_candidates +
    rails_filter_seen_ids: sorted per-rank lists with ties across ranks, seen ids hitting 0-100 % of the winners."""
    g = torch.Generator().manual_seed(R * 1000 + rows)
    msgs = []
    for r in range(R):
        s = torch.randint(0, 60, (rows, k), generator=g).float().div(8.0).sort(dim=1, descending=True).values   # many ties, within and across ranks
        i = torch.arange(k, dtype=torch.int64).repeat(rows, 1) * R + r + 1000 * torch.arange(rows, dtype=torch.int64)[:, None]
        msgs.append(E.pack_candidates(s.to(dev), i.to(dev), k))
    gathered = torch.cat(msgs, 0)
    ms, mi = E.merge_candidates(gathered, R, k, k)
    for frac in (0.0, 0.5, 1.0):
        hit = int(width * frac)
        inv = torch.full((rows, width), -7, dtype=torch.int64, device=dev)
        if hit:
            inv[:, :hit] = mi[:, torch.randperm(k, generator=g)[:hit].to(dev)] if hit <= k else mi[:, :1]
        want_i, want_s = E.filter_seen_ids(mi, ms, inv, k_out)
        got_i, got_s = E.merge_candidates_filtered(gathered, R, k, k, inv, k_out)
        assert torch.equal(got_i, want_i) and torch.equal(got_s, want_s)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,N,B,n_cand", [("amzn-books", 50_003, 5, 64), ("amzn-books", 200_000, 33, 352), ("ml-20m", 27_278, 32, 288), ("ml-1m", 3_883, 7, 32),
                                                 ("amzn-books", 50_003, 32, 1000), ("amzn-books", 50_003, 3, 5), ("ml-20m", 27_278, 9, 77)])   # ragged last tile of candidates
def test_indexed_candidate_scoring_equals_gather_then_score(dev, cfg_name, N, B, n_cand):
    """rails_mol_score_indexed (per-row candidates read in place from the shared index) against rails_mol_index_gather +
    rails_mol_score_candidates: the same arithmetic per (query, item) pair, hence the same bits -- duplicates, the first and the
    last item of the corpus (a ragged last tile) included."""
    cfg, tk, q, kw = _dense_case(cfg_name, N, B, dev, None)
    with torch.inference_mode():
        eng = tk._bind()
        assert eng.score_indexed_supported(B, n_cand)
        qpack, _, _ = eng.query_pack(q, kw.get("user_ids"))
        g = torch.Generator().manual_seed(N + B)
        pos = torch.randint(0, N, (B, n_cand), generator=g).to(dev)
        pos[:, 0], pos[:, 1], pos[:, 2] = 0, N - 1, pos[:, 3]
        cand, kp = eng.gather_index(tk._index, pos)
        want = eng.score_candidates(qpack, B, cand, kp)[:, :n_cand]
        got = eng.score_indexed(qpack, B, tk._index, pos)
        assert got.shape == (B, n_cand) and torch.equal(got, want)
        dense = eng.score_dense(qpack, B, tk._index)
        assert torch.equal(got, torch.gather(dense, 1, pos))      # and both are the dense kernel's values at those positions
        # the same candidates read from the ROW-MAJOR copy of the index (rails_mol_index_rows_build / rails_mol_score_indexed_rows): same bits;
        # the copy holds item i's fragment slot s, lane half h as float4 number 2 s + h of row i
        rows = eng.build_index_rows(tk._index)
        tile_f4 = tk._index.buf.numel() // 4 // ((N + 31) // 32)
        rp = tile_f4 // 32
        assert rows.numel() == N * rp * 4
        i = int(pos[0, 3])
        packed = tk._index.buf.view(-1, 4)
        for slot, h in ((0, 0), (1, 1), (tile_f4 // 64 - 1, 1)):
            assert torch.equal(rows.view(-1, 4)[i * rp + 2 * slot + h], packed[(i >> 5) * tile_f4 + slot * 64 + h * 32 + (i & 31)])
        assert torch.equal(eng.score_indexed_rows(qpack, B, rows, N, pos), got)


@pytest.mark.gpu
def test_candidate_unions_beyond_the_lds_sort_capacity(dev):
    """MoLNaiveTopK / MoLCombTopK with more than 16 384 candidates per query (16x16x64 with k_per_group >= 75: the reference "just
    runs", mol_top_k.py:260 / :518).  (a) the large-union route (device torch.sort around the HIP scoring) forced on a small union
    equals the LDS route bit for bit; (b) 256 * 75 = 19 200 candidates run, ranked, with exact MoL scores."""
    cfg = O.CONFIGS["amzn-books"]
    w = O.synthetic_weights(cfg, seed=3)
    N = 20_000
    X = torch.from_numpy(O.hash_item_table(5, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = (torch.arange(N, dtype=torch.int64, device=dev) * 2 + 1).unsqueeze(0)
    q = O.synthetic_queries(cfg, 6, seed=9).to(dev)
    with torch.inference_mode():
        mol = build_module(cfg, w, dev)
        a = rails_amd.MoLNaiveTopK(mol, X, ids, k_per_group=10)
        s0, i0 = a(q, k=50)
        a.UNION_CAP = 64                                   # 640 candidates > 64: the torch.sort route
        s1, i1 = a(q, k=50)
        assert torch.equal(s0, s1) and torch.equal(i0, i1)
        c = rails_amd.MoLCombTopK(mol, X, ids, k_per_group=10, avg_top_k=100)
        s0, i0 = c(q, k=50)
        c.UNION_CAP = 64
        s1, i1 = c(q, k=50)
        assert torch.equal(s0, s1) and torch.equal(i0, i1)
        cfg4 = O.CONFIGS["synthetic-16x16x64"]
        w4 = O.synthetic_weights(cfg4, seed=3)
        X4 = torch.from_numpy(O.hash_item_table(6, 0, N, cfg4.item_embedding_dim)).unsqueeze(0).to(dev)
        q4 = O.synthetic_queries(cfg4, 3, seed=10).to(dev)
        mol4 = build_module(cfg4, w4, dev)
        big = rails_amd.MoLNaiveTopK(mol4, X4, ids, k_per_group=75)      # 19 200 candidates per query
        s, i = big(q4, k=10)
        assert s.shape == (3, 256 * 75) and bool((s[:, :-1] >= s[:, 1:]).all())
        dense = rails_amd.MoLBruteForceTopK(mol4, X4, ids).all_logits(q4)     # the rerank is exact: the head carries the dense kernel's scores
        head = torch.gather(dense, 1, (i[:, :50] - 1) // 2)
        assert float((head - s[:, :50]).abs().max()) <= 2e-5 and bool((s[:, 0] <= dense.max(dim=1).values + 1e-6).all())
