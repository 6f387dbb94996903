"""The differentiable MoLSimilarity.forward, device-free: the references of tests/_mol_grad_ref.py against the
oracle, against the reference's own gradients (tests/golden/mol_grad.npz) and against each other; the bound of the GPU test against
seven bug classes; the new C symbols; the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import _lib
from rails_amd import engine as E
from tests import _mol_grad_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = G.golden_cases()
NEW_SYMBOLS = ["rails_mol_generic_pair_backward", "rails_mol_generic_pair_backward_supported", "rails_mol_generic_pair_backward_workspace_bytes",
               "rails_mol_generic_pack_gate_weights_t", "rails_mol_generic_gate_pack_t_floats"]


def test_golden_file_holds_the_three_cases():
    assert [n for n, *_ in GOLDEN] == ["d_8x8x32_geglu", "d_none_4x4x24", "d_uid_4x4x32_swiglu"]
    assert os.path.getsize(G.GOLDEN) < 512 * 1024
    for name, cfg, w, a, grads in GOLDEN:
        assert set(grads) >= {"q", "cand"} and sum(k.startswith("w/") for k in grads) >= 8, name


@pytest.mark.parametrize("case", GOLDEN, ids=[c[0] for c in GOLDEN])
def test_restatement_is_the_oracle_in_fp32(case):
    name, cfg, w, a, _ = case
    y = G.stages(cfg, w, a["q"], a["cand"], a.get("user_ids"))
    assert torch.equal(y, O.mol_logits(cfg, w, a["q"], a["cand"], a.get("user_ids")))
    assert float((y - a["y"]).abs().max()) <= 2e-6       # (the reference's own fp32 run: the bar of the per-row logits elsewhere)


def _autograd(cfg, w, a, dtype):
    """Gradients of (y * dY).sum() of the restatement in `dtype` -> {"q", "cand", "w/<key>"}."""
    ws = {k: v.detach().to(dtype).requires_grad_(v.is_floating_point()) for k, v in w.items()}
    q, cand = a["q"].to(dtype).requires_grad_(True), a["cand"].to(dtype).requires_grad_(True)
    y = G.stages(cfg, ws, q, cand, a.get("user_ids"))
    keys = [k for k, v in ws.items() if v.requires_grad]
    got = torch.autograd.grad((y * a["dY"].to(dtype)).sum(), [q, cand] + [ws[k] for k in keys], allow_unused=True)
    out = {"q": got[0], "cand": got[1]}
    out.update({"w/" + k: g for k, g in zip(keys, got[2:]) if g is not None})
    return out


@pytest.mark.parametrize("case", GOLDEN, ids=[c[0] for c in GOLDEN])
def test_float64_autograd_reproduces_the_reference_gradients(case):
    """The reference ran in fp32: its gradients sit within 4 x the fp32-vs-float64 error of the restatement itself on the same inputs
    (floor: 2^-22 of the tensor's largest magnitude)."""
    name, cfg, w, a, grads = case
    g64, g32 = _autograd(cfg, w, a, torch.float64), _autograd(cfg, w, a, torch.float32)
    assert set(g64) == set(grads), (sorted(set(g64) ^ set(grads)))
    for k, ref in grads.items():
        own = float((g32[k].double() - g64[k]).abs().max())
        tol = max(4.0 * own, 2.0 ** -22 * float(g64[k].abs().max()))
        err = float((ref.double() - g64[k]).abs().max())
        print(name, k, "err", err, "tol", tol)
        assert err <= tol, (name, k, err, tol)


def _pair_inputs(cfg, w, q, items, user_ids=None, dtype=torch.float64):
    """The pair stage's inputs as the kernels read them, from the restatement's upstream stages: Eq / tau, gq, Ex, gi (zeros where a
    gate part is absent) and the pair gate's weights."""
    ws = {k: v.to(dtype) if v.is_floating_point() else v for k, v in w.items()}
    eq, gq, ex, gi = G.upstream(cfg, ws, q.to(dtype), items.to(dtype), user_ids)
    B, X, L = ex.shape[0], ex.shape[1], cfg.num_logits
    gq = torch.zeros((B, L), dtype=dtype) if gq is None else gq
    gi = torch.zeros((B, X, L), dtype=dtype) if gi is None else gi
    g = "_gating_fn._qi_partial_module."
    return eq / cfg.temperature, gq, ex, gi, ws[g + "1.weight"], ws[g + "1.bias"], ws[g + "3.weight"], ws[g + "3.bias"]


SHAPES = G.kernel_shapes()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_analytic_backward_is_float64_autograd_of_the_pair_stage(name):
    cfg = SHAPES[name]
    w, q, items, dy = G.kernel_inputs(cfg)
    B, X = 3, 33
    ins = [t.detach().clone().requires_grad_(True) for t in _pair_inputs(cfg, w, q[:B], items[:B, :X])]
    none = cfg.gating_combination_type == "none"
    y = G.pair_stage(cfg, ins[0], None if none else ins[1], ins[2], None if none else ins[3], *ins[4:])
    wanted = [0, 2, 4, 5, 6, 7] if none else list(range(8))
    got = dict(zip(wanted, torch.autograd.grad((y * dy[:B, :X].double()).sum(), [ins[i] for i in wanted])))
    inv_tau = 1.0 / cfg.temperature
    ref = G.pair_backward64(*[t.detach().numpy() for t in ins], dy[:B, :X].numpy(), inv_tau, none)
    # autograd differentiates with respect to Eq / tau; the analytic dEq is the gradient of the unscaled Eq
    pairs = {"dEq": got[0].numpy() * inv_tau, "dEx": got[2].numpy(), "dW1": got[4].numpy(), "db1": got[5].numpy(), "dW2": got[6].numpy(), "db2": got[7].numpy()}
    if not none:
        pairs.update({"dgq": got[1].numpy(), "dgi": got[3].numpy()})
    for k, v in pairs.items():
        val, A, n, F = ref[k]
        assert val.shape == v.shape == np.shape(A), k
        assert float(np.abs(val - v).max()) <= 1e-12 * max(float(np.abs(v).max()), 1e-300), (name, k)
        assert np.all(np.abs(val) <= A * (1 + 1e-12) + 1e-300) and n > 0, (name, k)


@pytest.mark.parametrize("mut", G.MUTANTS)
def test_the_bound_of_the_gpu_test_discriminates(mut):
    """Each bug class leaves the bound 2^-24 ((n + C) A + F) of tests/test_mol_grad_gpu.py on that test's own inputs (the headline shape; the
    'none' shape for nothing: every mutant here acts on glu_silu too)."""
    cfg = SHAPES["8x8x32_h128"]
    w, q, items, dy = G.kernel_inputs(cfg)
    B, X = 3, 33
    ins = [t.numpy() for t in _pair_inputs(cfg, w, q[:B], items[:B, :X], dtype=torch.float32)]
    inv_tau = float(np.float32(1.0) / np.float32(cfg.temperature))
    Cc = G.factor_roundings(cfg.query_dot_product_groups, cfg.item_dot_product_groups, cfg.dot_product_dimension, cfg.gating_qi_hidden_dim)
    ref = G.pair_backward64(*ins, dy[:B, :X].numpy(), inv_tau, False)
    bad = G.pair_backward64(*ins, dy[:B, :X].numpy(), inv_tau, False, mut=mut)
    worst = {k: float((np.abs(bad[k][0] - ref[k][0]) / np.maximum(G.grad_bound(ref[k][1], ref[k][2], Cc, ref[k][3]), 1e-300)).max()) for k in ref}
    print(mut, worst)
    assert max(worst.values()) > 8.0, (mut, worst)         # far outside, not on the edge (the narrowest: the omitted 1 / tau, 171)


def test_symbols_are_declared_and_bound_under_abi_15():
    text = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert int(re.search(r"#define RAILS_ABI_VERSION (\d+)", text).group(1)) == _lib.RAILS_ABI_VERSION == 15
    lib = _lib.load()
    assert lib.rails_abi_version() == 15
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name


def test_sizes_and_the_envelope_answer_without_a_device():
    lib = _lib.load()
    s = E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, 128).to_c()
    assert lib.rails_mol_generic_pair_backward_supported(C.byref(s)) == 1
    assert lib.rails_mol_generic_gate_pack_t_floats(C.byref(s)) == 2 * 128 * 64
    tiles = 2 * 4 * 2 + 4 + 2
    assert lib.rails_mol_generic_pair_backward_workspace_bytes(C.byref(s), 4096) == 4 * (4096 * 2 * (64 + 128) + 16 * tiles * 1024)
    assert lib.rails_mol_generic_pair_backward_workspace_bytes(C.byref(s), 4097) == 4 * (4352 * 2 * (64 + 128) + 17 * tiles * 1024)
    wide = E.MolShapeSpec(64, 64, 256, 8, 8, 512, 128, 128, 128).to_c()          # 8 tiles of dEq along d
    assert lib.rails_mol_generic_supported(C.byref(wide)) == 1 and lib.rails_mol_generic_pair_backward_supported(C.byref(wide)) == 0
    assert "ceil(P_Q / 32) * ceil(d / 32) <= 4" in _lib.last_error()


def _module(differentiable=True, **kw):
    args = dict(query_embedding_dim=32, item_embedding_dim=24, dot_product_dimension=32, query_dot_product_groups=4, item_dot_product_groups=4,
                temperature=0.05, query_dropout_rate=0.0, query_hidden_dim=48, item_dropout_rate=0.0, item_hidden_dim=-1,
                gating_query_hidden_dim=16, gating_qi_hidden_dim=64, gating_item_hidden_dim=16, softmax_dropout_rate=0.2, bf16_training=False)
    args.update(kw)
    mol, _ = rails_amd.create_mol_interaction_module(**args)
    mol = mol.eval()
    mol.differentiable = differentiable
    return mol


def _call(mol, B=2, X=3):
    q = torch.randn(B, mol._query_embedding_dim, requires_grad=True)
    return mol(q, torch.randn(B, X, mol._item_embedding_dim))


def test_refusals_before_any_launch():
    with pytest.raises(NotImplementedError, match=r"hidden layer.*differentiable"):
        _call(_module(gating_qi_hidden_dim=-1))                                   # a pair gate of one Linear
    with pytest.raises(NotImplementedError, match=r"dot_product_dimension <= 256.*differentiable"):
        _call(_module(dot_product_dimension=264))
    with pytest.raises(NotImplementedError, match=r"gating_qi_hidden_dim <= 512.*differentiable"):
        _call(_module(gating_qi_hidden_dim=520))
    with pytest.raises(NotImplementedError, match=r"ceil\(P_Q / 32\).*differentiable"):
        _call(_module(dot_product_dimension=160))
    mol = _module()
    mol._apply_item_embeddings_fn = False
    with pytest.raises(NotImplementedError, match=r"apply_query_embeddings_fn / apply_item_embeddings_fn = False.*differentiable"):
        _call(mol)
    mol = _module().train()
    with pytest.raises(NotImplementedError, match="eval-mode path only"):         # training mode: exactly as without the switch
        _call(mol)


def test_the_switch_defaults_to_off():
    assert _module(differentiable=False).differentiable is False
    mol, _ = rails_amd.create_mol_interaction_module(
        query_embedding_dim=32, item_embedding_dim=24, dot_product_dimension=32, query_dot_product_groups=4, item_dot_product_groups=4,
        temperature=0.05, query_dropout_rate=0.0, query_hidden_dim=48, item_dropout_rate=0.0, item_hidden_dim=-1, gating_query_hidden_dim=16,
        gating_qi_hidden_dim=64, gating_item_hidden_dim=16, softmax_dropout_rate=0.2, bf16_training=False)
    assert mol.differentiable is False
