"""CPU: the host side of diversify= -- the entry point in header, binding and library under ABI 15 and its checks, none of
which launches; the host functions of the vector table against a numpy model; set_item_vectors' checks; every refusal by name; the reference
walk of tests/_mmr_ref.py on its own; and the injected mistakes, each of which must change the result on the inputs the GPU tests run."""
import os
import re
import types

import numpy as np
import pytest
import torch

from rails_amd import _lib
from rails_amd import engine as E
from rails_amd import topk_modules as T
from tests import _mmr_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the entry point ----------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported_under_abi_15():
    with open(os.path.join(ROOT, "include", "rails_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = _lib.load()
    for name, ret, count in (("rails_topk_mmr", "int", 22), ("rails_topk_mmr_workspace_bytes", "size_t", 3)):
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, f"{name} is not declared in include/rails_amd.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == count
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == count, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define\s+RAILS_ABI_VERSION\s+15\b", header)
    assert _lib.RAILS_ABI_VERSION == 15 and lib.rails_abi_version() == 15
    assert E.MMR_MAX_POOL == 1024 and E.MMR_MAX_DIM == 256 and E.MMR_MAX_MAGNITUDE == 2.0 ** 60
    assert lib.rails_topk_mmr_workspace_bytes(3, 100, 64) == 0 and lib.rails_topk_mmr_workspace_bytes(3, 100, 65) == 3 * 100 * 65 * 4
    src = open(os.path.join(ROOT, "rails_amd", "csrc", "Makefile")).read()
    assert " mmr.hip " in src


def test_entry_point_validates_before_any_launch():
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    lib = _lib.load()
    bad, unsup, ok = _lib.RAILS_EINVAL, _lib.RAILS_ENOTSUP, _lib.RAILS_OK
    # rails_topk_mmr(scores, ld, positions, rows, depth, vectors, n_items, dim, lam, k, pool, ids, invalid_ids, width, workspace, workspace_bytes,
    #                out_scores, out_positions, out_ids, out_counts, out_of_range, stream)
    good = [1, 8, 1, 2, 8, 1, 100, 16, 0.5, 3, 4, None, None, 0, None, 0, 1, 1, 1, 1, 1]
    for lam in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        args = list(good)
        args[8] = lam
        assert lib.rails_topk_mmr(*args, None) == bad and "lam" in _lib.last_error(), lam
    for at, value, code, word in ((9, 5, bad, "beyond pool"), (10, 1025, unsup, "pool"), (7, 0, bad, "dim"), (7, 257, unsup, "dim"),
                                  (13, 4097, unsup, "width"), (3, -1, bad, "negative"), (13, -1, bad, "negative")):
        args = list(good)
        args[at] = value
        if at == 10:
            args[9] = 1025      # (k = pool = 1025: the pool's limit, not k <= pool, refuses)
        if at == 13 and value > 0:
            args[12] = 1
        assert lib.rails_topk_mmr(*args, None) == code and word in _lib.last_error(), (at, value, _lib.last_error())
    for at in (0, 2, 5, 16, 17, 18, 19, 20):
        args = list(good)
        args[at] = None
        assert lib.rails_topk_mmr(*args, None) == bad and "NULL" in _lib.last_error(), at
    args = list(good)
    args[13] = 3      # seen ids without their pointer
    assert lib.rails_topk_mmr(*args, None) == bad and "NULL" in _lib.last_error()
    args = list(good)
    args[1] = 7
    assert lib.rails_topk_mmr(*args, None) == bad and "ld < depth" in _lib.last_error()
    for depth in (0, 16385):
        args = list(good)
        args[1], args[4] = depth, depth
        assert lib.rails_topk_mmr(*args, None) == unsup and "depth" in _lib.last_error()
    args = list(good)
    args[7] = 65      # the workspace tier without its workspace
    assert lib.rails_topk_mmr(*args, None) == bad and "workspace" in _lib.last_error()
    for at in (3, 9):      # nothing to do
        args = list(good)
        args[at] = 0
        assert lib.rails_topk_mmr(*args, None) == ok, at


def test_engine_call_checks_before_the_library():
    s, p, v = torch.zeros(2, 8), torch.zeros((2, 8), dtype=torch.int64), torch.zeros(10, 4)
    word = torch.zeros(1, dtype=torch.int32)
    for lam in (0.0, 1.5, -1.0, float("nan"), True, "0.5", torch.tensor(0.5)):
        with pytest.raises(ValueError, match="lam"):
            E.topk_mmr(s, p, v, lam, 2, 4, None, None, word)
    for k, pool, exc in ((5, 4, ValueError), (0, 4, ValueError), (2, 1025, NotImplementedError)):
        with pytest.raises(exc):
            E.topk_mmr(s, p, v, 0.5, k, pool, None, None, word)
    for vec in (torch.zeros(10, 0), torch.zeros(10, 257)):
        with pytest.raises(NotImplementedError, match="1 <= E <= 256"):
            E.topk_mmr(s, p, vec, 0.5, 2, 4, None, None, word)
    with pytest.raises(ValueError, match="float32"):
        E.topk_mmr(s, p, v.double(), 0.5, 2, 4, None, None, word)
    with pytest.raises(NotImplementedError, match="4096 seen ids"):
        E.topk_mmr(s, p, v, 0.5, 2, 4, None, torch.zeros((2, 4097), dtype=torch.int64), word)
    with pytest.raises(NotImplementedError, match="16384"):
        E.topk_mmr(torch.zeros(2, 16385), torch.zeros((2, 16385), dtype=torch.int64), v, 0.5, 2, 4, None, None, word)


def test_list_similarity():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(30, 7, generator=g)
    pos = torch.stack([torch.randperm(30, generator=g)[:6] for _ in range(4)])
    got = E.list_similarity(pos, v)
    for b in range(4):
        pairs = [float(v[pos[b, i]] @ v[pos[b, j]]) for i in range(6) for j in range(i + 1, 6)]
        assert abs(float(got[b]) - sum(pairs) / len(pairs)) < 1e-5
    assert E.list_similarity(pos[:, :1], v).tolist() == [0.0] * 4


# ---- the vector table under edits: pure host functions -----------------------------------------------------------------------------------
def test_vectors_after_append_and_removal_against_a_numpy_model():
    g = torch.Generator().manual_seed(4)
    n, dim = 50, 5
    table = torch.randn(n, dim, generator=g)
    grown = T.vectors_after_append(table, n, n + 7)
    assert grown.shape == (n + 7, dim) and grown.dtype == torch.float32 and torch.equal(grown[:n], table) and bool((grown[n:] == 0).all())
    assert torch.equal(T.vectors_after_append(table, n, n), table)
    for trial in range(20):
        m = int(torch.randint(1, n - 1, (1,), generator=g))
        gone = torch.randperm(n, generator=g)[:m]
        holes, movers = T.removal_plan(gone, n)
        model = table.numpy()[: n - m].copy()
        model[holes.numpy()] = table.numpy()[movers.numpy()]
        before = table.clone()
        got = T.vectors_after_removal(table, n - m, holes, movers)
        assert np.array_equal(got.numpy(), model) and torch.equal(table, before), trial      # (the table given is not written)
        kept = sorted(set(range(n)) - set(gone.tolist()))
        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, table[kept].tolist())), trial      # exactly the survivors' rows


class Exact(T.MIPSBruteForceTopK):
    """set_item_vectors and _take_diversity read the type, the item count, the id table's device and the vector table: no index is needed."""

    def __init__(self, n=6, vectors=True):
        torch.nn.Module.__init__(self)
        self._index = types.SimpleNamespace(n_items=n, dim=4)
        self._ids_flat = torch.arange(n, dtype=torch.int64)
        self._flag_free = []
        if vectors:
            self.set_item_vectors(torch.eye(n, 4))

    def _join_side_streams(self):
        pass


def test_set_item_vectors():
    g = torch.Generator().manual_seed(5)
    tk = Exact(vectors=False)
    assert tk.item_vectors is None and tk.diversity_stats() == {"calls": 0}
    for bad in (torch.zeros(6), torch.zeros(6, 4, 1), torch.zeros(6, 4, dtype=torch.float64), torch.zeros((6, 4), dtype=torch.int32), [[0.0] * 4] * 6,
                torch.zeros(5, 4), torch.zeros(7, 4), torch.zeros(6, 0), torch.zeros(6, 257)):
        with pytest.raises(ValueError):
            tk.set_item_vectors(bad)
        assert tk.item_vectors is None
    for value in (float("nan"), float("inf"), float("-inf"), 2.0 ** 61, -(2.0 ** 61)):
        v = torch.randn(6, 4, generator=g)
        v[3, 2] = value
        with pytest.raises(ValueError, match="finite with magnitude"):
            tk.set_item_vectors(v)
        assert tk.item_vectors is None
    v = torch.randn(6, 4, generator=g)
    v[0, 0], v[1, 1] = 2.0 ** 60, -(2.0 ** 60)      # the limit itself is taken
    tk.set_item_vectors(v)
    assert torch.equal(tk.item_vectors, v) and tk.item_vectors is not v and tk.item_vectors.is_contiguous()
    tk.set_item_vectors(v.t().contiguous().t())      # a strided argument: the stored table is row-major
    assert torch.equal(tk.item_vectors, v) and tk.item_vectors.is_contiguous()
    tk.set_item_vectors(tk.item_vectors)             # the hand-off is taken back as it is
    assert torch.equal(tk.item_vectors, v)
    assert "_vectors" not in tk.state_dict() and not any("vector" in key for key in tk.state_dict())
    # positions=
    rows = torch.randn(2, 4, generator=g)
    tk.set_item_vectors(rows, positions=torch.tensor([4, 1]))
    want = v.clone()
    want[4], want[1] = rows[0], rows[1]
    assert torch.equal(tk.item_vectors, want)
    for pos in (torch.tensor([1, 1]), torch.tensor([1, 6]), torch.tensor([-1, 2]), torch.tensor([1]), torch.tensor([1.0, 2.0])):
        with pytest.raises(ValueError):
            tk.set_item_vectors(rows, positions=pos)
    with pytest.raises(ValueError, match="entries per item"):
        tk.set_item_vectors(torch.zeros(2, 5), positions=torch.tensor([0, 1]))
    assert torch.equal(tk.item_vectors, want)
    tk.clear_item_vectors()
    assert tk.item_vectors is None
    tk.set_item_vectors(rows, positions=torch.tensor([4, 1]))      # on a module without vectors: every other row zero
    want = torch.zeros(6, 4)
    want[4], want[1] = rows[0], rows[1]
    assert torch.equal(tk.item_vectors, want)
    # normalize=
    v = torch.randn(6, 4, generator=g)
    v[2] = 0
    tk.set_item_vectors(v, normalize=True)
    assert torch.equal(tk.item_vectors, v / torch.linalg.vector_norm(v, dim=1, keepdim=True).clamp_min(1e-12))
    assert bool((tk.item_vectors[2] == 0).all()) and abs(float(tk.item_vectors[0].norm()) - 1.0) < 1e-6


def test_take_diversity():
    tk = Exact()
    for kwargs, want in (({}, None), ({"diversify": None}, None), ({"diversify": 0.5}, (0.5, None)), ({"diversify": 1.0, "diversity_pool": 77}, (1.0, 77)),
                         ({"diversify": 0.25, "diversity_pool": None}, (0.25, None)), ({"diversify": 0.5, "collapse_groups": False}, (0.5, None))):
        kw = dict(kwargs, user_ids=7)
        assert T._asks_diversity(kw) == bool(kwargs)
        assert tk._take_diversity(kw) == want
        assert "diversify" not in kw and "diversity_pool" not in kw and kw["user_ids"] == 7
    for lam in (0.0, -0.1, 1.5, 1, True, "0.5", float("nan"), torch.tensor(0.5), np.float32(0.5)):
        with pytest.raises(ValueError) as e:
            tk._take_diversity({"diversify": lam})
        assert str(e.value) == f"Exact: diversify must be a Python float with 0 < diversify <= 1, got {lam!r}"
    for pool in (0, -3, True, 64.0, "64"):
        with pytest.raises(ValueError) as e:
            tk._take_diversity({"diversify": 0.5, "diversity_pool": pool})
        assert str(e.value) == f"Exact: diversity_pool must be a Python int >= 1, got {pool!r}"
    with pytest.raises(ValueError) as e:
        tk._take_diversity({"diversity_pool": 64})
    assert str(e.value) == "Exact: diversity_pool= without diversify="
    with pytest.raises(ValueError) as e:
        Exact(vectors=False)._take_diversity({"diversify": 0.5})
    assert str(e.value) == "Exact: diversify=0.5 on a module without vectors (set_item_vectors first)"
    for other in ({"collapse_groups": True}, {"max_per_group": 2}):
        with pytest.raises(NotImplementedError) as e:
            tk._take_diversity(dict(other, diversify=0.5))
        assert str(e.value) == "Exact: diversify= together with collapse_groups= / max_per_group= is not built"
    for other in ({"query_lims": torch.tensor([0, 2])}, {"fuse": "max"}, {"query_weights": torch.ones(2)}):
        with pytest.raises(NotImplementedError) as e:
            tk._take_diversity(dict(other, diversify=0.5))
        assert str(e.value) == "Exact: diversify= together with query_lims= is not built"
    assert tk.diversity_stats() == {"calls": 0}


def test_pool_size_and_limits_come_before_any_launch():
    assert [T.diversity_pool_size(k, None, 0, "X") for k in (1, 16, 17, 120, 256, 300, 1024)] == [64, 64, 68, 480, 1024, 1024, 1024]
    assert all(T.diversity_pool_size(k, None, 0, "X") == MR.default_pool(k) for k in range(1, 1025))
    assert T.diversity_pool_size(10, 10, 4096, "X") == 10 and T.diversity_pool_size(10, 1024, 0, "X") == 1024
    for k, pool, width in ((1025, None, 0), (10, 9, 0), (10, 1025, 0), (10, None, 4097)):
        with pytest.raises(NotImplementedError) as e:
            T.diversity_pool_size(k, pool, width, "X")
        assert str(e.value).startswith("X: diversify= takes k <= diversity_pool <= 1024 and up to 4096 seen ids per row") and f"k = {k}," in str(e.value)
    # through the public calls of a module that is never launched: the checks come first, nothing of the (absent) index is touched
    tk, q = Exact(), torch.zeros(2, 4)
    seen = torch.zeros((2, 1), dtype=torch.int64)
    for call in (lambda **kw: tk.forward(q, 3, **kw), lambda **kw: tk.forward_filtered(q, 4, seen, 3, **kw)):
        with pytest.raises(ValueError, match="Python float"):
            call(diversify=0.0)
        with pytest.raises(NotImplementedError, match="k <= diversity_pool <= 1024"):
            call(diversify=0.5, diversity_pool=2)
        with pytest.raises(NotImplementedError, match="together with collapse_groups"):
            call(diversify=0.5, max_per_group=2)
        with pytest.raises(NotImplementedError, match="together with query_lims"):
            call(diversify=0.5, query_lims=torch.tensor([0, 2]))
    with pytest.raises(NotImplementedError, match="width = 4097"):
        tk.forward_filtered(q, 3, torch.zeros((2, 4097), dtype=torch.int64), 3, diversify=0.5)
    with pytest.raises(RuntimeError) as e:
        tk.forward(q, 7, diversify=0.5)
    assert str(e.value) == "selected index k out of range (k=7, n=6)"
    assert tk.diversity_stats() == {"calls": 0}


def test_refusals_by_name():
    class Wrapper:
        pass

    w = Wrapper()
    T.refuse_diversity(w, {})
    T.refuse_diversity(w, {"diversify": None, "diversity_pool": None})
    tail = ": diversifying by maximal marginal relevance is built on the single-device modules' forward, forward_filtered and get_top_k_outputs only"
    with pytest.raises(NotImplementedError) as e:
        T.refuse_diversity(w, {"diversify": 0.5})
    assert str(e.value) == "Wrapper takes no diversify" + tail
    with pytest.raises(NotImplementedError) as e:
        T.refuse_diversity(w, {"diversity_pool": 64}, "submit")
    assert str(e.value) == "Wrapper.submit takes no diversity_pool" + tail
    # the streaming family's entry check, on an exact module
    tk = Exact()
    for what in ("rank_of", "log_partition", "log_prob_of", "sample_items", "count_above", "range_search"):
        with pytest.raises(NotImplementedError) as e:
            tk._refuse_streaming({"diversify": 0.5}, what, None)
        assert str(e.value).startswith(f"Exact.{what} takes no diversify: ")
    # the IVF module and the approximate modules of the generic route
    ivf = types.SimpleNamespace(_use_faiss=True, _call_eng=None, _engine=types.SimpleNamespace(route="fp32"))
    for what in ("diversify", "set_item_vectors"):
        with pytest.raises(NotImplementedError) as e:
            T.MoLNaiveTopK._check_diversifiable(ivf, what)
        assert str(e.value) == (f"MoLNaiveTopK (IVF, use_faiss=True) takes no {what}: diversifying by maximal marginal relevance is not built on the IVF "
                                "index; the exhaustive MoLNaiveTopK takes it")
    generic = types.SimpleNamespace(_use_faiss=False, _call_eng=None, _engine=types.SimpleNamespace(route="generic"))
    for cls in (T.MoLNaiveTopK, T.MoLAvgTopK, T.MoLCombTopK):
        with pytest.raises(NotImplementedError) as e:
            cls._check_diversifiable(generic, "diversify")
        assert str(e.value) == ("SimpleNamespace: diversify is not built on the generic scoring route (generic_candidates = True covers the "
                                "single-device exhaustive algorithms without item vectors); MoLBruteForceTopK diversifies on this route")
    plain = types.SimpleNamespace(_use_faiss=False, _call_eng=None, _engine=types.SimpleNamespace(route="fp32"))
    T.MoLNaiveTopK._check_diversifiable(plain, "diversify")
    # submit and the hand-off calls: the refusal is the first thing they do
    q = torch.zeros(2, 4)
    for cls, call in ((T.MoLAvgTopK, "submit"), (T.MoLAvgTopK, "coarse_candidates"), (T.MoLAvgTopK, "topk_ids"), (T.MoLNaiveTopK, "local_candidates"),
                      (T.MoLBruteForceTopK, "all_logits")):
        class Bare(cls):
            def __init__(self):
                torch.nn.Module.__init__(self)

        args = (q, 3) if call == "submit" else (q,)
        with pytest.raises(NotImplementedError, match=f"Bare.{call} takes no diversify"):
            getattr(Bare(), call)(*args, diversify=0.5)


def test_sharded_wrappers_refuse_by_name():
    from rails_amd import sharded

    class OneRank(sharded.ShardedMoLAvgTopK):
        def __init__(self):      # (no process group: the refusal comes before anything of the wrapper is touched)
            torch.nn.Module.__init__(self)

    q = torch.zeros(2, 4)
    for call in (lambda w: w.forward(q, 3, diversify=0.5), lambda w: w.forward_filtered(q, 4, torch.zeros((2, 1), dtype=torch.int64), 3, diversify=0.5)):
        with pytest.raises(NotImplementedError, match="OneRank takes no diversify"):
            call(OneRank())


# ---- the reference alone ------------------------------------------------------------------------------------------------------------------
def test_lam_1_is_the_filtered_list_order():
    for name in ("L64-all", "L1025-one-hot-k64", "seen-head", "seen-head-E32", "short-rows", "plus-inf", "signed-zeros"):
        case = MR.CASE[name]
        d = MR.build(case)
        for b in range(case.rows):
            inv = None if d["invalid"] is None else d["invalid"][b]
            entries = MR.pool_entries(d["scores"][b], d["positions"][b], d["n"], d["ids"], inv, case.pool)
            keys = (MR.R.orderable(d["scores"][b][entries].view(np.uint32)).astype(np.uint64) << np.uint64(32)) | (~np.arange(len(entries), dtype=np.uint32)).astype(np.uint64)
            order = entries[np.argsort(keys, kind="stable")[::-1]][: case.k]
            s, p, i, P = MR.walk_row(d["scores"][b], d["positions"][b], d["vectors"], 1.0, case.k, case.pool, d["ids"], inv)
            assert P == len(entries) and np.array_equal(p, d["positions"][b][order]) and np.array_equal(s, d["scores"][b][order].view(np.uint32)), (name, b)
            assert np.array_equal(i, d["ids"][p])
            if name not in ("signed-zeros",):      # a list in key order: the first k eligible entries as they stand
                assert np.array_equal(order, entries[: case.k]), (name, b)


def test_orthogonal_and_zero_vectors_give_the_plain_order():
    rng = np.random.default_rng(11)
    n, L = 60, 50
    scores = -np.sort(-rng.standard_normal(L).astype(F32))
    positions = rng.permutation(n)[:L]
    one_hot = np.zeros((n, 64), dtype=F32)
    one_hot[np.arange(n), rng.permutation(64)[:n]] = rng.uniform(0.5, 3.0, n).astype(F32)      # pairwise orthogonal, any length
    for vectors in (one_hot, np.zeros((n, 3), dtype=F32)):
        for lam in (1.0, 0.7, 0.01):
            s, p, _, P = MR.walk_row(scores, positions, vectors, lam, 20, 40)
            assert P == 40 and np.array_equal(p, positions[:20]) and np.array_equal(s, scores[:20].view(np.uint32)), lam


def test_three_items_by_hand():
    """a: 1.0, b: 0.9 (a's duplicate), c: 0.5 (orthogonal).  lam = 0.5: a (0.5); then b = 0.45 - 0.5 = -0.05 against c = 0.25: c, then b.  lam = 0.9:
    b = 0.81 - 0.1 = 0.71 against c = 0.45: the ranking as it is.  A NEGATIVE similarity never rewards: with b = -a, b keeps val = 0.45."""
    scores = np.array([1.0, 0.9, 0.5], dtype=F32)
    positions = np.array([2, 0, 1])
    vectors = np.array([[1, 0], [0, 1], [1, 0]], dtype=F32)      # by position: b, c, a
    assert MR.walk_row(scores, positions, vectors, 0.5, 3, 3)[1].tolist() == [2, 1, 0]
    assert MR.walk_row(scores, positions, vectors, 0.9, 3, 3)[1].tolist() == [2, 0, 1]
    assert MR.walk_row(scores, positions, vectors, 0.5, 2, 3)[1].tolist() == [2, 1]
    assert MR.walk_row(scores, positions, vectors, 0.5, 3, 2)[1].tolist() == [2, 0]      # a pool of two: c is never looked at
    s, p, i, P = MR.walk_row(scores, positions, vectors, 0.5, 3, 3, ids=np.array([10, 11, 12]), invalid=np.array([12, 99]))
    assert P == 2 and p.tolist() == [0, 1] and i.tolist() == [10, 11] and s.view(F32).tolist() == [F32(0.9), F32(0.5)]      # the scores are the items' own
    vectors[0] = [-1, 0]
    assert MR.walk_row(scores, positions, vectors, 0.5, 3, 3)[1].tolist() == [2, 0, 1]
    assert MR.walk_row(scores, positions, vectors, 0.5, 3, 3, mutant="no_clamp")[1].tolist() == [2, 0, 1]
    # ties go to the smaller POOL index, whatever the positions are
    tie = np.array([1.0, 1.0, 1.0], dtype=F32)
    assert MR.walk_row(tie, positions, np.zeros((3, 2), dtype=F32), 0.5, 3, 3)[1].tolist() == [2, 0, 1]
    assert MR.walk_row(tie, positions, np.zeros((3, 2), dtype=F32), 0.5, 3, 3, mutant="ties_by_position")[1].tolist() == [0, 1, 2]


# ---- the injected mistakes ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probes():
    """The reference's outputs on the probe cases, computed once."""
    out = {}
    for case in MR.CASES:
        if case.probe:
            d = MR.build(case)
            out[case.name] = (case, d, MR.walk(d["scores"], d["positions"], d["vectors"], case.lam, case.k, case.pool, d["ids"], d["invalid"]))
    return out


@pytest.mark.parametrize("mutant", MR.MUTANTS)
def test_every_mutant_gives_itself_away_on_the_gpu_tests_inputs(mutant, probes):
    caught = []
    for name, (case, d, want) in probes.items():
        got = MR.walk(d["scores"], d["positions"], d["vectors"], case.lam, case.k, case.pool, d["ids"], d["invalid"], mutant=mutant)
        if not all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4])):
            caught.append(name)
    print(mutant, "caught on", caught)
    assert caught, f"the mutant {mutant} returns the reference's result on every probe case"


def test_the_cases_cover_what_the_issue_lists():
    lengths, pools, dims, rows, widths = (set(getattr(c, f) for c in MR.CASES) for f in ("length", "pool", "dim", "rows", "width"))
    assert {1, 2, 63, 64, 65, 1024, 1025, 5120, 16384} <= lengths and {1, 64, 65, 1024} <= pools and {1, 3, 4, 16, 17, 32, 33, 64, 65, 256} <= dims
    assert {1, 3, 70} <= rows and {0, 1, 256, 257, 4096} <= widths
    assert all(c.k in (1, c.pool) for c in MR.CASES) and any(c.k == c.pool == 1024 for c in MR.CASES)
    assert {"gauss", "equal_scores", "identical_vectors", "one_hot", "negative_sims", "signed_zeros", "subnormals", "plus_inf", "mixed", "short"} <= \
        set(c.family for c in MR.CASES)
    for name in ("mixed",):      # the family that carries -inf, NaN, positions -1 and n, and a seen head
        d = MR.build(MR.CASE["seen-head"])
        assert np.isnan(d["scores"]).any() and np.isneginf(d["scores"]).any() and (d["positions"] == -1).any() and (d["positions"] == d["n"]).any()
        assert (d["invalid"] >= 0).sum() >= 3 * 150
    d = MR.build(MR.CASE["short-rows"])
    assert MR.walk(d["scores"], d["positions"], d["vectors"], 0.7, 64, 64, d["ids"], d["invalid"])[3].tolist()[1] < 64
