"""The shape-generic fp32 scoring route on the GPU (rails_mol_generic_*, rails_amd/csrc/mol_generic.hip): against the reference's
fixture (tests/golden/generic_shapes.npz), against float64 with the a-priori bounds of tests/_mol_ref64.py, the per-pair
invariances, NaN containment, the top-k modules, the forced route on fused shapes, and the refusals."""
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from tests import _mol_ref64 as R
from tests._fixtures import Fixture, assert_topk_matches, variant_cases
from tests._generic_fixtures import generic_cases, spec_of
from tests.test_gpu_parity import LOGIT_TOL, STAGE_TOL

pytestmark = pytest.mark.gpu

CASES = {name: (cfg, w, a) for name, cfg, w, a in generic_cases()}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def build_module(cfg, weights, dev, route=None, precision=None):
    mol, _ = rails_amd.create_mol_interaction_module(
        query_embedding_dim=cfg.query_embedding_dim, item_embedding_dim=cfg.item_embedding_dim,
        dot_product_dimension=cfg.dot_product_dimension, query_dot_product_groups=cfg.query_dot_product_groups,
        item_dot_product_groups=cfg.item_dot_product_groups, temperature=cfg.temperature, query_dropout_rate=0.0,
        query_hidden_dim=cfg.query_hidden_dim, item_dropout_rate=0.1, item_hidden_dim=cfg.item_hidden_dim,
        gating_query_hidden_dim=cfg.gating_query_hidden_dim, gating_qi_hidden_dim=cfg.gating_qi_hidden_dim,
        gating_item_hidden_dim=cfg.gating_item_hidden_dim, softmax_dropout_rate=cfg.softmax_dropout_rate, bf16_training=False,
        gating_query_fn=cfg.gating_query_fn, gating_item_fn=cfg.gating_item_fn, query_nonlinearity=cfg.query_nonlinearity,
        item_nonlinearity=cfg.item_nonlinearity, gating_combination_type=cfg.gating_combination_type, eps=cfg.eps,
        uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None)
    mol.load_state_dict(weights, strict=True)
    mol = mol.to(dev).eval()
    mol.route, mol.precision = route, precision
    return mol


def kw_of(a, dev, rows=None):
    if "user_ids" not in a:
        return {}
    u = a["user_ids"] if rows is None else a["user_ids"][rows]
    return {"user_ids": u.to(dev)}


def corpus(cfg, n, seed=3):
    return torch.from_numpy(O.hash_item_table(seed, 0, n, cfg.item_embedding_dim))


def queries(cfg, a, B, dev):
    """B queries (and user ids where the case has a uid table) drawn like the fixture's."""
    q = O.synthetic_queries(cfg, B, seed=9).to(dev)
    kw = {"user_ids": (torch.arange(B, dtype=torch.int64) * 7919 - 5).to(dev)} if "user_ids" in a else {}
    return q, kw


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_reference_fixture(name, dev):
    cfg, w, a = CASES[name]
    mol = build_module(cfg, w, dev)
    kw = kw_of(a, dev)
    with torch.inference_mode():
        assert mol.engine().route == "generic"
        logits, aux = mol(a["q"].to(dev), a["X"].to(dev), **kw)
        rows, _ = mol(a["q"].to(dev), a["cand"].to(dev), **kw)
        eq, _ = mol.get_query_component_embeddings(a["q"].to(dev), **kw)
        ex, _ = mol.get_item_component_embeddings(a["X"].to(dev))
    assert aux == {}
    figures = {"logits": float((logits.cpu() - a["logits"]).abs().max()), "rows": float((rows.cpu() - a["row_logits"]).abs().max()),
               "Eq": float((eq.cpu() - a["Eq"]).abs().max()), "Ex": float((ex.cpu() - a["Ex"]).abs().max())}
    print(name, figures)
    assert figures["logits"] <= LOGIT_TOL and figures["rows"] <= LOGIT_TOL, figures
    assert figures["Eq"] <= STAGE_TOL and figures["Ex"] <= STAGE_TOL, figures


def _within(got, ref_and_bound, what):
    ref, bound = ref_and_bound
    err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(what, "max |err| / bound =", worst, "max |err| =", float(err.max()))
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64_with_a_priori_bounds(name, dev):
    """prologue64 / index64 on the fp32 inputs, score64 on the engine's own plain Eq / Ex / gq / gi (dense and per-row)."""
    cfg, w, a = CASES[name]
    mol = build_module(cfg, w, dev)
    q, X, cand = a["q"].to(dev), a["X"][0].to(dev), a["cand"].to(dev)
    uid = a.get("user_ids")
    with torch.inference_mode():
        eng = mol.engine()
        qpack, eq, gq = eng.query_pack(q, None if uid is None else uid.to(dev), want_plain=True)
        index = eng.build_index(X)
        ex, gi = eng.unpack_index(index)
        logits = eng.score_dense(qpack, q.shape[0], index)
        B, XC = cand.shape[:2]
        cindex = eng.build_index(cand.reshape(B * XC, -1))
        cex, cgi = eng.unpack_index(cindex)
        rows = eng.score_candidates(qpack, B, cindex, XC)
    (eq64, gq64) = R.prologue64(cfg, w, a["q"], uid)
    _within(eq, eq64, name + " Eq")
    _within(gq, gq64, name + " gq")
    (ex64, gi64) = R.index64(cfg, w, a["X"][0])
    _within(ex, ex64, name + " Ex")
    _within(gi, gi64, name + " gi")
    _within(logits, R.score64(cfg, w, eq, ex, gq, gi), name + " logits")
    PX, d, L = cfg.item_dot_product_groups, cfg.dot_product_dimension, cfg.num_logits
    _within(rows, R.score64(cfg, w, eq, cex.reshape(B, XC, PX, d), gq, cgi.reshape(B, XC, L)), name + " row logits")


@pytest.mark.parametrize("name", sorted(CASES))
def test_per_pair_invariance(name, dev):
    cfg, w, a = CASES[name]
    mol = build_module(cfg, w, dev)
    N, B = 517, 33
    X = corpus(cfg, N).to(dev)
    q, kw = queries(cfg, a, B, dev)
    uid = kw.get("user_ids")
    with torch.inference_mode():
        eng = mol.engine()
        index = eng.build_index(X)
        qpack, _, _ = eng.query_pack(q, uid)
        full = eng.score_dense(qpack, B, index)
        # batch size and the row's position in the batch
        for lo, hi in ((0, 1), (5, 12), (32, 33), (0, 33)):
            qp, _, _ = eng.query_pack(q[lo:hi], None if uid is None else uid[lo:hi])
            assert torch.equal(eng.score_dense(qp, hi - lo, index), full[lo:hi]), (name, lo, hi)
        # the item's position and N: an index of X[100:300], a view of the full index at a tile boundary, N = 1, a ragged N
        sub = eng.build_index(X[100:300])
        assert torch.equal(eng.score_dense(qpack, B, sub), full[:, 100:300]), name
        assert torch.equal(eng.score_dense(qpack, B, index.items(96, 301)), full[:, 96:301]), name
        assert torch.equal(eng.score_dense(qpack, B, eng.build_index(X[77:78])), full[:, 77:78]), name
        assert torch.equal(eng.score_dense(qpack, B, eng.build_index(X[:131])), full[:, :131]), name
        # per-row candidates against the dense result at the same pairs (through the engine and through the module)
        pos = torch.randint(0, N, (B, 45), generator=torch.Generator().manual_seed(11)).to(dev)
        cand = X[pos]
        cidx = eng.build_index(cand.reshape(B * 45, -1))
        assert torch.equal(eng.score_candidates(qpack, B, cidx, 45), torch.gather(full, 1, pos)), name
        rows, _ = mol(q, cand, **kw)
        assert torch.equal(rows, torch.gather(full, 1, pos)), name
        # ld and the launch predicate
        wide = torch.full((B, N + 9), -7.0, device=dev)
        eng.score_dense(qpack, B, index, out=wide)
        assert torch.equal(wide[:, :N], full) and bool((wide[:, N:] == -7.0).all()), name
        off, on = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
        keep = torch.full((B, N), -7.0, device=dev)
        eng.score_dense(qpack, B, index, out=keep, run_if=off)
        assert bool((keep == -7.0).all()), name
        eng.score_dense(qpack, B, index, out=keep, run_if=on)
        assert torch.equal(keep, full), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_nan_and_inf_stay_in_their_row_and_column(name, dev):
    cfg, w, a = CASES[name]
    mol = build_module(cfg, w, dev)
    N, B = 200, 7
    X = corpus(cfg, N).to(dev)
    q, kw = queries(cfg, a, B, dev)
    with torch.inference_mode():
        base, _ = mol(q, X.unsqueeze(0), **kw)
        q2 = q.clone()
        q2[2, 3], q2[5, 0] = float("nan"), float("inf")
        got, _ = mol(q2, X.unsqueeze(0), **kw)
        ok = torch.ones(B, dtype=torch.bool, device=dev)
        ok[2] = ok[5] = False
        assert torch.equal(got[ok], base[ok]) and not bool(torch.isfinite(got[~ok]).any()), name
        X2 = X.clone()
        X2[37, 1] = float("nan")
        got, _ = mol(q, X2.unsqueeze(0), **kw)
        okc = torch.ones(N, dtype=torch.bool, device=dev)
        okc[37] = False
        assert torch.equal(got[:, okc], base[:, okc]) and bool(torch.isnan(got[:, 37]).all()), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_brute_force_topk_and_seen_id_filter(name, dev):
    cfg, w, a = CASES[name]
    mol = build_module(cfg, w, dev)
    N, B, k = 1000, 5, 10
    X = corpus(cfg, N, seed=4).unsqueeze(0)
    ids = torch.arange(1, N + 1, dtype=torch.int64).unsqueeze(0) * 2
    q, kw = queries(cfg, a, B, torch.device("cpu"))
    uid = kw.get("user_ids")
    ref_s, ref_i, ref_logits = O.brute_force_topk(cfg, w, q, X, ids, k, uid)
    kwd = {key: v.to(dev) for key, v in kw.items()}
    with torch.inference_mode():
        for mode in (None, "dense"):
            tk = rails_amd.MoLBruteForceTopK(mol, X.to(dev), ids.to(dev), exact_mode=mode)
            eng = tk._bind()
            assert eng.route == "generic" and eng.exact is None and eng.precision == "fp32", name
            s, i = tk(q.to(dev), k=k, **kwd)
            assert_topk_matches(s, i, ref_s, ref_i)
            assert float((tk.all_logits(q.to(dev), **kwd).cpu() - ref_logits).abs().max()) <= LOGIT_TOL
        # the chunked dense path (corpora whose (B, N) logits exceed the logit budget): sub-ranges of the index at tile boundaries, same bits
        tk.CHUNK_ITEMS = 256
        cs, cidx = tk._forward_chunked(q.to(dev), k, **kwd)
        assert torch.equal(cs, s) and torch.equal(cidx, i), name
        seen = ref_i[:, :4].clone()                      # every row has seen its four best items
        ci = rails_amd.CandidateIndex(ids=ids.to(dev), embeddings=X.to(dev))
        top_ids, top_scores, _ = ci.get_top_k_outputs(q.to(dev), k, dict(kwd), tk, seen.to(dev))
        kp = O.k_prime(k, seen, N, None)
        rs, ri, _ = O.brute_force_topk(cfg, w, q, X, ids, kp, uid)
        want_i, want_s = O.filter_seen_ids(ri, rs, seen, k)
        assert_topk_matches(top_scores, top_ids, want_s, want_i)
        fused = tk.forward_filtered(q.to(dev), kp, seen.to(dev), k, **kwd)      # None where the filter does not fit the selection launch
        if fused is not None:
            assert_topk_matches(fused[1], fused[0], want_s, want_i)


def _forced_cases():
    for fname in ("c1_ml1m", "c3_books", "c4_16x16x64"):
        fx = Fixture(fname)
        n = int(fx.z["F1/n"])
        yield fname, fx.cfg, fx.weights, fx.t("q"), fx.t("X")[:, :n], fx.kw.get("user_ids"), fx.t("F1/logits")
    for name, cfg, w, a in variant_cases():
        if cfg.gating_qi_hidden_dim > 0:
            yield name, cfg, w, a["q"], a["X"], None, a["logits"]


def test_forced_route_on_fused_shapes(dev):
    """route = "generic" on shapes that have fused kernels: within LOGIT_TOL of the reference's fixtures, and within the sum of the two
    kernels' score64 bounds of the fused route (each from its own operands; the prologue and index values are the same arithmetic)."""
    n = 0
    for name, cfg, w, q, X, uid, ref in _forced_cases():
        kw = {} if uid is None else {"user_ids": uid.to(dev)}
        fused, forced = build_module(cfg, w, dev), build_module(cfg, w, dev, route="generic")
        with torch.inference_mode():
            assert fused.engine().route == "fused" and forced.engine().route == "generic", name
            lf, _ = fused(q.to(dev), X.to(dev), **kw)
            lg, _ = forced(q.to(dev), X.to(dev), **kw)
            bounds = []
            for m in (fused, forced):
                eng = m.engine()
                _, eq, gq = eng.query_pack(q.to(dev), kw.get("user_ids"), want_plain=True)
                ex, gi = eng.unpack_index(eng.build_index(X[0].to(dev)))
                bounds.append(R.score64(cfg, w, eq, ex, gq, gi)[1])
                if m is forced:
                    plain_forced = (eq, ex, gq, gi)
                else:
                    plain_fused = (eq, ex, gq, gi)
        d_ref = float((lg.cpu() - ref).abs().max())
        d_routes = (lg.cpu().double() - lf.cpu().double()).abs()
        print(name, "forced vs fixture", d_ref, "forced vs fused", float(d_routes.max()), "bound", float((bounds[0] + bounds[1]).min()))
        assert d_ref <= LOGIT_TOL, (name, d_ref)
        for x, y in zip(plain_fused, plain_forced):      # Eq, Ex, gq, gi: the fused route's own arithmetic, written in another layout
            assert torch.equal(x, y), name
        assert bool((d_routes <= bounds[0] + bounds[1]).all()), name
        n += 1
    assert n == 3 + 4


def test_refusals(dev):
    cfg, w, a = CASES["g_8x8x40"]
    for precision in ("f16x3", "f16x3-exact"):
        mol = build_module(cfg, w, dev, precision=precision)
        with pytest.raises(NotImplementedError, match="no fused scoring kernel"):
            mol.engine()
    for name, vcfg, vw, va in variant_cases():
        if vcfg.gating_qi_hidden_dim <= 0:
            with pytest.raises(NotImplementedError, match="hidden layer"):       # the generic route does not take it either
                build_module(vcfg, vw, dev, route="generic").engine()
            with pytest.raises(NotImplementedError, match="without hidden layer"):
                build_module(vcfg, vw, dev, precision="f16x3").engine()
    mol = build_module(cfg, w, dev)
    X = corpus(cfg, 300).unsqueeze(0).to(dev)
    ids = torch.arange(300, dtype=torch.int64).unsqueeze(0).to(dev)
    with torch.inference_mode():
        eng = mol.engine()
        assert not eng.score_dense_upper_supported() and not eng.score_indexed_supported(4, 64)
        index = eng.build_index(X[0])
        for call in (lambda: eng.build_index_rows(index), lambda: eng.build_coarse_table(index), lambda: eng.build_component_table(index),
                     lambda: eng.gate_rows(torch.empty(1, device=dev), 1), lambda: eng.query_pack_both(X[0, :2], None, None, None),
                     lambda: eng.score_indexed(None, 1, index, torch.zeros((1, 1), dtype=torch.int64)), lambda: E.IvfIndex(eng, index)):
            with pytest.raises(NotImplementedError, match="generic scoring route"):
                call()
        for make in (lambda: rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=32), lambda: rails_amd.MoLNaiveTopK(mol, X, ids, k_per_group=2),
                     lambda: rails_amd.MoLCombTopK(mol, X, ids, avg_top_k=32, k_per_group=2)):
            with pytest.raises(NotImplementedError, match="generic scoring route"):
                make()
