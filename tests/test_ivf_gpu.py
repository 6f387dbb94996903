"""GPU: the IVF-Flat index behind MoLNaiveTopK(use_faiss=True) (rails_amd/csrc/ivf.hip, engine.IvfIndex) against its CPU restatement
tests/_ivf_ref.py, on seeded synthetic inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import _lib
from rails_amd import engine as E
from tests import _ivf_ref as R
from tests._fixtures import assert_topk_matches

pytestmark = pytest.mark.gpu
BAND = 1e-5        # scores closer than this to the k-th are ties
NEAR = 1e-6        # centroid scores closer than this are near-ties
CONFIGS = {"ml-1m": "ml-1m", "ml-20m": "ml-20m", "amzn-books": "amzn-books", "16x16x64": "synthetic-16x16x64"}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def make_mol(cfg, w, dev):
    mol, _ = rails_amd.create_mol_interaction_module(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
        cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
        cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
        query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None,
    )
    mol.load_state_dict(w, strict=True)
    return mol.to(dev).eval()


_CACHE = {}


def setup(name, n, dev, seed=0):
    """-> (cfg, weights, mol, engine, index, X (N, D) on the device, Ex16 (N, P_X, d) fp16 on the host)."""
    key = (name, n, seed)
    if key not in _CACHE:
        cfg = O.CONFIGS[CONFIGS[name]]
        w = O.synthetic_weights(cfg, seed=seed, uid_rows=None)
        mol = make_mol(cfg, w, dev)
        X = torch.from_numpy(O.hash_item_table(11 + seed, 0, n, cfg.item_embedding_dim)).to(dev)
        eng = mol.engine()
        index = eng.build_index(X)
        ex = eng.unpack_index(index, want_gi=False)[0]
        _CACHE[key] = (cfg, w, mol, eng, index, X, ex.half().cpu())
    return _CACHE[key]


def query_components(mol, eng, cfg, B, seed=5):
    q = O.synthetic_queries(cfg, B, seed=seed).to(eng.device)
    uid = torch.arange(1, B + 1, device=eng.device) if cfg.uid_embedding_hash_sizes else None
    _, eq, _ = eng.query_pack(q, uid, want_plain=True)
    return eq


def check_search(got, eq, ivf, ex16, k, nprobe):
    """Every (b, i, m) row against _ivf_ref.search_row on the same index, tie-aware.  -> share of rows skipped as near-ties."""
    G, PQ = ivf.groups, eq.shape[1]
    got = got.view(eq.shape[0], PQ, G, k).cpu().numpy()
    c = ivf.centroids.cpu().double().numpy()
    pos = ivf.positions.cpu().numpy().astype(np.int64)
    off = ivf.offsets.cpu().numpy().astype(np.int64)
    x = ex16.double().numpy()
    eqn = eq.cpu().double().numpy()
    skipped = rows = 0
    for b in range(eq.shape[0]):
        for i in range(PQ):
            for m in range(G):
                rows += 1
                lists, cs = R.probe_order(eqn[b, i], c[m], off[m], nprobe, k)
                n_taken = len(lists)
                if n_taken < len(cs) and cs[n_taken - 1] - cs[n_taken] < NEAR:
                    skipped += 1
                    continue
                ref_p, ref_s, by_pos = R.search_row(eqn[b, i], x[:, m], c[m], pos[m], off[m], nprobe, k)
                mine = got[b, i, m].tolist()
                assert len(set(mine)) == k, (b, i, m, mine)
                assert all(p in by_pos for p in mine), "a position outside the probed lists"
                kth = ref_s[-1]
                must = {p for p, s in by_pos.items() if s > kth + BAND}
                assert must <= set(mine), (b, i, m)
                assert all(by_pos[p] >= kth - BAND for p in mine), (b, i, m)
                s_mine = np.array([by_pos[p] for p in mine])
                assert (s_mine[:-1] >= s_mine[1:] - BAND).all(), "not best first"
    return skipped / rows


# ---- 1. build invariants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("ml-1m", 3883), ("ml-20m", 20000), ("amzn-books", 30000), ("16x16x64", 12000)])
def test_build_invariants(dev, name, n):
    cfg, w, mol, eng, index, X, ex16 = setup(name, n, dev)
    nlist = 100 if n >= 10000 else 40
    ivf = E.IvfIndex(eng, index, nlist=nlist)
    G = cfg.item_dot_product_groups
    off = ivf.offsets.cpu().long()
    pos = ivf.positions.cpu().long()
    vec = ivf.vectors.cpu()
    c = ivf.centroids.cpu().double()
    assert ivf.centroids.shape == (G, nlist, cfg.dot_product_dimension) and ivf.vectors.dtype == torch.float16
    assert torch.allclose(c.norm(dim=2), torch.ones(G, nlist, dtype=torch.float64), atol=1e-5)
    for m in range(G):
        assert off[m, 0] == 0 and off[m, -1] == n and bool((off[m, 1:] >= off[m, :-1]).all())
        assert torch.equal(torch.sort(pos[m]).values, torch.arange(n))                                   # the lists partition [0, N)
        lists = torch.repeat_interleave(torch.arange(nlist), off[m, 1:] - off[m, :-1])
        same = lists[1:] == lists[:-1]
        assert bool((pos[m, 1:][same] > pos[m, :-1][same]).all())                                        # ascending inside a list
        assert torch.equal(vec[m].view(torch.int16), ex16[pos[m], m].view(torch.int16))                  # bitwise Ex.half()
        a, gap = R.assign(ex16[pos[m], m].double().numpy(), c[m].numpy())
        wrong = (a != lists.numpy()) & (gap >= NEAR)
        assert not wrong.any(), f"group {m}: {int(wrong.sum())} items outside their argmax centroid's list"
    again = E.IvfIndex(eng, index, nlist=nlist)
    for t in ("centroids", "vectors", "positions", "offsets"):
        a, b = getattr(ivf, t), getattr(again, t)
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, b.view(torch.int16) if b.dtype == torch.float16 else b), t


# ---- 2. one Lloyd step -------------------------------------------------------------------------------------------------------
def test_one_lloyd_step_equals_reference(dev):
    cfg, w, mol, eng, index, X, ex16 = setup("amzn-books", 30000, dev)
    n, G, d, nlist = 30000, cfg.item_dot_product_groups, cfg.dot_product_dimension, 64
    g = torch.Generator().manual_seed(3)
    start = torch.nn.functional.normalize(torch.randn(G, nlist, d, generator=g), dim=2)
    start[:, 5] = 0.5 * start[:, 4]    # never the argmax where 4 is positive: an empty list, split off the largest
    cent = start.to(dev).contiguous()
    sample = torch.from_numpy(R.sample_positions(n, nlist, 7)).to(torch.int32).to(dev)
    S = sample.numel()
    shape = eng._fp32_shape
    ws = torch.empty(eng.lib.rails_ivf_build_workspace_bytes(C.byref(shape), n, nlist, S), dtype=torch.uint8, device=dev)
    assign = torch.empty((G, n), dtype=torch.int32, device=dev)
    _lib.check(eng.lib.rails_ivf_assign(C.byref(shape), E._ptr(index.buf), None, n, nlist, E._ptr(cent), E._ptr(assign), E._stream()), "assign")
    _lib.check(eng.lib.rails_ivf_train(C.byref(shape), E._ptr(index.buf), None, n, E._ptr(sample), S, nlist, 1, 0, E._ptr(cent), E._ptr(ws), ws.numel(),
                                       E._stream()), "train")
    got_a, got_c = assign.cpu().numpy(), cent.cpu().double().numpy()
    smp = sample.cpu().long().numpy()
    for m in range(G):
        x = ex16[:, m].double().numpy()
        a, gap = R.assign(x, start[m].double().numpy())
        assert not ((a != got_a[m]) & (gap >= NEAR)).any()
        ref = R.lloyd_step(x[smp], start[m].double().numpy())
        _, sgap = R.assign(x[smp], start[m].double().numpy())
        assert (sgap < NEAR).mean() < 0.01
        if (sgap < NEAR).any():
            continue     # a near-tie sample point may sit in either list
        assert np.abs(got_c[m] - ref).max() < 1e-5, m


# ---- 3. search against the reference on the same index -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["amzn-books", "16x16x64"])
@pytest.mark.parametrize("nprobe", [1, 3])
@pytest.mark.parametrize("k", [5, 100])
def test_search_equals_reference(dev, name, nprobe, k):
    n = 30000 if name == "amzn-books" else 12000
    cfg, w, mol, eng, index, X, ex16 = setup(name, n, dev)
    ivf = E.IvfIndex(eng, index, nlist=100)
    for B in (1, 7, 33, 1024 // cfg.query_dot_product_groups + 1):     # the last one spans two slices of the search (1024 query rows each)
        eq = query_components(mol, eng, cfg, B, seed=B)
        got = ivf.search(eq, k, nprobe=nprobe)
        assert got.shape == (B, cfg.query_dot_product_groups * cfg.item_dot_product_groups * k) and got.dtype == torch.int64
        assert check_search(got, eq, ivf, ex16, k, nprobe) < 0.02


# ---- 4. nprobe = nlist is the exhaustive component top-k ------------------------------------------------------------------------
def test_all_lists_probed_is_exhaustive(dev):
    cfg, w, mol, eng, index, X, ex16 = setup("amzn-books", 30000, dev)
    k, nlist = 10, 16
    ivf = E.IvfIndex(eng, index, nlist=nlist, nprobe=nlist)
    eq = query_components(mol, eng, cfg, 4)
    got = ivf.search(eq, k).view(4, 8, 8, k).cpu()
    sc = torch.einsum("bid,xmd->bimx", eq.cpu().double(), ex16.double())
    for b in range(4):
        for i in range(8):
            for m in range(8):
                row = sc[b, i, m]
                kth = torch.sort(row, descending=True).values[k - 1]
                mine = set(got[b, i, m].tolist())
                assert len(mine) == k
                assert set(torch.nonzero(row > kth + BAND).flatten().tolist()) <= mine <= set(torch.nonzero(row >= kth - BAND).flatten().tolist())


# ---- 5. short lists ---------------------------------------------------------------------------------------------------------
def test_short_lists_continue_in_coarse_order(dev):
    cfg, w, mol, eng, index, X, ex16 = setup("amzn-books", 300, dev)
    k, nlist = 20, 14
    ivf = E.IvfIndex(eng, index, nlist=nlist)
    sizes = ivf.list_sizes()
    assert bool((sizes < k).any()), sizes
    eq = query_components(mol, eng, cfg, 9)
    got = ivf.search(eq, k)
    flat = got.view(-1, k).cpu()
    assert all(len(set(r.tolist())) == k for r in flat) and int(flat.min()) >= 0 and int(flat.max()) < 300
    c, off = ivf.centroids.cpu().double().numpy(), ivf.offsets.cpu().numpy().astype(np.int64)
    continued = sum(len(R.probe_order(q, c[m], off[m], 1, k)[0]) > 1 for q in eq.cpu().double().numpy().reshape(-1, 32) for m in range(8))
    assert continued > 0
    assert check_search(got, eq, ivf, ex16, k, 1) < 0.05


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------
def test_module_end_to_end(dev):
    cfg, w, mol, eng, index, X, ex16 = setup("amzn-books", 30000, dev, seed=1)
    n, kg, B = 30000, 5, 6
    ids = (torch.arange(n, dtype=torch.int64) * 3 + 1).unsqueeze(0).to(dev)
    mod = rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids, k_per_group=kg, use_faiss=True)
    assert mod._use_faiss and mod._ivf is None                 # built lazily
    q = O.synthetic_queries(cfg, B, seed=9).to(dev)
    with torch.inference_mode():
        s, i = mod(q, k=10)
        ivf = mod._ivf
        assert ivf is not None and ivf.nlist == 100 and ivf.nprobe == 1
        _, eq, _ = mod._bind().query_pack(q, None, want_plain=True)
        union = torch.sort(ivf.search(eq, kg), dim=1).values.cpu()
    assert s.shape == (B, 8 * 8 * kg)
    es, ei = O.union_rerank(cfg, w, q.cpu(), X.cpu().unsqueeze(0), ids.cpu(), union)
    assert_topk_matches(s, i, es, ei, atol=1e-4)
    # get_top_k_outputs with seen ids: the fused filter equals ranking everything and filtering after
    inv = i[:, 2:9].clone()
    inv[0, 3] = -5
    ci = rails_amd.CandidateIndex(ids, X.unsqueeze(0))
    with torch.inference_mode():
        got_i, got_s, _ = ci.get_top_k_outputs(q, k=10, aux_payloads={}, top_k_module=mod, invalid_ids=inv)
        full_s, full_i = mod(q, k=17)
    r_i, r_s = E.filter_seen_ids(full_i, full_s, inv, 10)
    assert torch.equal(got_i, r_i) and torch.equal(got_s, r_s)
    # new item-projection weights: a new engine, so a new index
    w2 = {k_: v.clone() for k_, v in mol.state_dict().items()}
    key = "_item_embeddings_fn._item_emb_proj_module.1.weight"
    w2[key] = w2[key].flip(0)
    mol.load_state_dict(w2)
    with torch.inference_mode():
        mod(q, k=10)
    assert mod._ivf is not ivf and not torch.equal(mod._ivf.centroids, ivf.centroids)


# ---- 7. recall on planted clusters ---------------------------------------------------------------------------------------------
def planted(cfg, n=20000, n_proto=300, n_query=16, seed=4):
    """Item embeddings: noisy copies of n_proto prototypes; queries: fresh noisy copies of prototypes."""
    g = torch.Generator().manual_seed(seed)
    proto = torch.randn(n_proto, cfg.item_embedding_dim, generator=g)
    items = proto[torch.randint(0, n_proto, (n,), generator=g)] + 0.25 * torch.randn(n, cfg.item_embedding_dim, generator=g)
    queries = proto[torch.randint(0, n_proto, (n_query,), generator=g)] + 0.25 * torch.randn(n_query, cfg.item_embedding_dim, generator=g)
    return items, queries


RECALL_BAR = 0.70     # tests/_ivf_ref.py on the same data (float64, the oracle's Ex): 0.7014


def test_recall_on_planted_clusters(dev):
    cfg = O.CONFIGS["amzn-books"]
    w = O.synthetic_weights(cfg, seed=0)
    mol = make_mol(cfg, w, dev)
    items, queries = planted(cfg)
    eng = mol.engine()
    index = eng.build_index(items.to(dev))
    ivf = E.IvfIndex(eng, index, nlist=100)
    ex16 = eng.unpack_index(index, want_gi=False)[0].half().cpu()
    qx = eng.unpack_index(eng.build_index(queries.to(dev)), want_gi=False)[0]       # (Q, P_X, d): P_Q = P_X = 8 query rows per query
    got = ivf.search(qx, 5, nprobe=4).view(-1, 8, 8, 5).cpu()
    sc = torch.einsum("bid,xmd->bimx", qx.cpu().double(), ex16.double())
    exact = torch.topk(sc, 5, dim=3).indices
    hits = sum(len(set(got[b, i, m].tolist()) & set(exact[b, i, m].tolist())) for b in range(got.shape[0]) for i in range(8) for m in range(8))
    recall = hits / exact.numel()
    assert recall >= RECALL_BAR - 0.02, recall


# ---- 8. limits ----------------------------------------------------------------------------------------------------------------
def test_limits(dev):
    cfg, w, mol, eng, index, X, ex16 = setup("amzn-books", 300, dev)
    ids = torch.arange(300, dtype=torch.int64, device=dev).unsqueeze(0)
    for kw, what in ((dict(nlist=5000), "nlist"), (dict(nlist=100, nprobe=65), "nprobe"), (dict(nlist=10, nprobe=11), "nprobe"),
                     (dict(nlist=0), "nlist"), (dict(nprobe=0), "nprobe")):
        with pytest.raises(NotImplementedError, match=what):
            rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids, k_per_group=5, use_faiss=True, **kw)
    with pytest.raises(NotImplementedError, match="k_per_group"):
        rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids, k_per_group=129, use_faiss=True, nlist=10)
    with pytest.raises(ValueError, match="nlist"):
        rails_amd.MoLNaiveTopK(mol, X[:50].unsqueeze(0), ids[:, :50], k_per_group=5, use_faiss=True, nlist=100)
    ivf = E.IvfIndex(eng, index, nlist=10)
    eq = query_components(mol, eng, cfg, 2)
    with pytest.raises(NotImplementedError, match="k_per_group"):
        ivf.search(eq, 129)
    with pytest.raises(NotImplementedError, match="nprobe"):
        ivf.search(eq, 5, nprobe=11)
    with pytest.raises(ValueError):
        E.IvfIndex(eng, index.items(0, 5), nlist=10)


# ---- the build from a split-f16 engine, NaN queries, shape checks -----------------------------------------------------------------
def test_split_f16_engine_builds_the_same_index(dev, monkeypatch):
    """A split-f16 engine's index holds Ex to 22 bits only: the components come from temporary fp32-format chunks (here of 4 096 items,
    so that 30 000 items take eight) and give the fp32 engine's index bit for bit."""
    cfg, w, mol, eng, index, X, ex16 = setup("amzn-books", 30000, dev)
    ref = E.IvfIndex(eng, index, nlist=100)
    eng16 = mol.engine(precision="f16x3")
    assert eng16.precision != "fp32"
    monkeypatch.setattr(E.IvfIndex, "COMPONENT_CHUNK", 4096)
    got = E.IvfIndex(eng16, eng16.build_index(X), nlist=100, items=X)
    for t in ("centroids", "positions", "offsets"):
        assert torch.equal(getattr(got, t), getattr(ref, t)), t
    assert torch.equal(got.vectors.view(torch.int16), ref.vectors.view(torch.int16))
    eq = query_components(mol, eng, cfg, 5)
    assert torch.equal(got.search(eq, 5, check=True), ref.search(eq, 5, check=True))


def test_nan_queries_still_fill_every_row_and_shapes_are_checked(dev):
    cfg, w, mol, eng, index, X, ex16 = setup("amzn-books", 30000, dev)
    ivf = E.IvfIndex(eng, index, nlist=100)
    eq = query_components(mol, eng, cfg, 3).clone()
    eq[1, 2, 5] = float("nan")
    for k, nprobe in ((5, 1), (100, 3)):
        got = ivf.search(eq, k, nprobe=nprobe, check=True).view(3, 8, 8, k).cpu()
        for row in got.reshape(-1, k):
            assert len(set(row.tolist())) == k and int(row.min()) >= 0 and int(row.max()) < 30000
        assert check_search(got.view(3, -1)[[0, 2]].to(dev), eq[[0, 2]], ivf, ex16, k, nprobe) < 0.02    # the clean queries are untouched
    with pytest.raises(ValueError, match="eq must be"):
        ivf.search(eq[:, :4], 5)
    with pytest.raises(ValueError, match="eq must be"):
        ivf.search(eq[..., :16], 5)
