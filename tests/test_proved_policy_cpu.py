"""CPU: the two pure functions behind the proved top-k's host decisions.  MoLBruteForceTopK.bound_policy: the form of the bound on
|first pass - fp32| from the pair-gate weights, the shape, the policy corpus size and the library's shape query (which loads without a GPU).
MoLBruteForceTopK.candidate_count: the candidate margin of the proved flow, the monitored flow and the item-sharded proof.  Its expectations follow from the constants in the code (tile = 32, PAD_ONE_EPS = (824, 3), PAD_PER_PAIR = (1848, 1),
PAD_PER_PAIR_SMALL = (312, 1), PER_PAIR_MAX_ITEMS = 196 608, cap 16 384), worked out by hand."""
import math
import os

import pytest

import rails_amd
from rails_amd import MoLBruteForceTopK as TK
from rails_amd import _lib
from rails_amd import f16x3_bound as FB
from oracle import mol_oracle as O

BOOKS = 695_762


@pytest.mark.parametrize("items,k,per_pair,want", [
    (BOOKS, 200, False, 1024),          # 200 + max(824, 600) = 1 024
    (BOOKS, 2561, True, 5152),          # 2 561 + max(1 848, 2 561) = 5 122 -> 161 tiles
    (BOOKS, 2561, False, 10272),        # 2 561 + 3 * 2 561 = 10 244 -> 321 tiles
    (27_278, 200, True, 512),           # a small corpus: 200 + 312
    (12_500_000, 200, True, 2048),      # 200 + 1 848
])
def test_candidate_counts_of_the_proved_flow(items, k, per_pair, want):
    assert TK.candidate_count(k, per_pair, items) == want
    assert want % 32 == 0 and TK.PER_PAIR_MIN_K <= 2561 and TK.PER_PAIR_MAX_ITEMS == 196_608


def test_the_count_doubles_with_the_pad_scale_up_to_the_cap():
    got = [TK.candidate_count(200, False, BOOKS, s) for s in (1, 2, 4, 8, 16, 32)]
    assert got == [1024, 1856, 3520, 6816, 13408, 16384]      # 200 + 824 s, whole tiles, at most 16 384
    assert TK.candidate_count(200, True, 12_500_000, 64) == 16384


def test_the_sharded_split():
    per = math.ceil(1024 / 8)
    want = (per + int(4 * math.sqrt(per)) + 32 + 31) // 32 * 32
    assert want == 224
    assert TK.candidate_count(200, False, -(-BOOKS // 8), 1, world=8, n_local=86_971) == want
    assert TK.candidate_count(200, False, -(-BOOKS // 8), 1, world=8, n_local=100) == 100      # a short shard is all candidates
    assert TK.candidate_count(200, False, -(-BOOKS // 8), 1, world=8, n_local=0) == 1


def test_the_monitored_flow_keeps_rails_topk_on_its_two_launch_path():
    assert TK.candidate_count(200, False, BOOKS, 1, single=True) == 352      # 200 + max(128, 100) -> 11 tiles
    assert TK.candidate_count(200, False, BOOKS, 4, single=True) == 512      # 200 + 512 = 712, but k <= 384 stays at 512
    assert TK.candidate_count(2561, False, BOOKS, 1, single=True) == 3872    # 2 561 + 1 280 = 3 841 -> 121 tiles


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


class _WithUpperBuild:
    """The library with the one query that needs a device (rails_mol_score_dense_upper_supported sizes a dry-run launch by the part's compute
    units, so it answers 0 without a GPU) answered as an MI355X answers it for the shapes below; tests/test_proved_gpu.py asserts the form
    "upper" at 27 278 items with the library's own answer."""

    def __init__(self, lib):
        self._lib = lib

    def rails_mol_score_dense_upper_supported(self, shape):
        return 1

    def __getattr__(self, name):
        return getattr(self._lib, name)


def _books_module(gating_qi_hidden_dim=None):
    cfg = O.CONFIGS["amzn-books"]
    hid = cfg.gating_qi_hidden_dim if gating_qi_hidden_dim is None else gating_qi_hidden_dim
    mol, _ = rails_amd.create_mol_interaction_module(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
        cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
        cfg.gating_query_hidden_dim, hid, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
        query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None)
    if gating_qi_hidden_dim is None:
        mol.load_state_dict(O.synthetic_weights(cfg, seed=0), strict=True)
    return mol.eval()


def test_the_form_of_the_bound(lib):
    mol = _books_module()
    spec = mol.shape_spec()
    on_cpu = TK.bound_policy(mol, spec, lib, BOOKS)      # the library's own answers
    assert on_cpu.kind == "eps" and on_cpu.poly is None
    lib = _WithUpperBuild(lib)
    full = TK.bound_policy(mol, spec, lib, BOOKS)
    assert full.terms["eps"] == on_cpu.terms["eps"]
    assert full.kind == "eps" and full.poly is None and math.isfinite(full.terms["eps"]) and full.terms["eps"] <= TK.PROVED_MAX_EPS
    assert full.any_poly is not None and all(c >= 0.0 for c in full.any_poly)      # the shape has the UPPER build: calls for many results take it
    small = TK.bound_policy(mol, spec, lib, 27_278)
    assert small.kind == "upper" and small.poly is not None and small.poly == small.any_poly and small.terms["eps"] == full.terms["eps"]
    plain = _books_module(gating_qi_hidden_dim=-1)      # the pair gate is one Linear: a guard of the bound fails
    none = TK.bound_policy(plain, plain.shape_spec(), lib, BOOKS)
    assert none.kind is None and none.poly is None and none.any_poly is None and math.isinf(none.terms["eps"])


def test_the_verdict_eps_is_the_bound_rounded_up_to_a_float32(lib):
    import torch

    mol = _books_module()
    lib = _WithUpperBuild(lib)
    full = TK.bound_policy(mol, mol.shape_spec(), lib, BOOKS).with_guard(2.0)
    e = full.terms["eps"]
    assert full.eps > e and full.eps <= e * (1.0 + 2.0 ** -15) and float(torch.tensor(full.eps, dtype=torch.float32)) == full.eps
    assert full.guard_limit == FB.GATE_GUARD / 2.0
    small = TK.bound_policy(mol, mol.shape_spec(), lib, 27_278)
    assert small.with_guard(2.0).eps == 0.0 and math.isinf(small.with_guard(math.inf).eps) and small.with_guard(0.0).guard_limit == 3.0e38


def test_constructing_the_policy_evaluates_the_bound_once(lib, monkeypatch):
    """first_pass_bound is counted where the policy calls it; upper_bound_poly's own evaluations of it along its grid are its business (it
    is counted as one call itself)."""
    calls = {"first": 0, "upper": 0, "inside": False}
    real_first, real_upper = FB.first_pass_bound, FB.upper_bound_poly

    def first(*a, **kw):
        if not calls["inside"]:
            calls["first"] += 1
        return real_first(*a, **kw)

    def upper(*a, **kw):
        calls["upper"] += 1
        calls["inside"] = True
        try:
            return real_upper(*a, **kw)
        finally:
            calls["inside"] = False

    monkeypatch.setattr(FB, "first_pass_bound", first)
    monkeypatch.setattr(FB, "upper_bound_poly", upper)
    mol = _books_module()
    TK.bound_policy(mol, mol.shape_spec(), _WithUpperBuild(lib), BOOKS)
    assert calls["first"] == 1 and calls["upper"] == 1
