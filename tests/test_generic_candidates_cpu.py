"""The candidate entries of the shape-generic scoring route, device-free: the new symbols in the header, the binding and the library, the
table width rule, and the engine cache key of MoLSimilarity.generic_candidates."""
import ctypes as C
import os
import re

import pytest
import torch

import rails_amd
from rails_amd import _lib
from rails_amd import engine as E
from tests._generic_fixtures import generic_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rails_mol_generic_score_indexed", "rails_mol_generic_table_width", "rails_mol_generic_coarse_build", "rails_mol_generic_coarse_update",
               "rails_mol_generic_component_build", "rails_mol_generic_component_update", "rails_mol_generic_eq_pad")


def test_header_binding_and_library_export_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert int(re.search(r"#define RAILS_ABI_VERSION (\d+)", text).group(1)) == _lib.RAILS_ABI_VERSION == 15
    lib = _lib.load()
    assert lib.rails_abi_version() == 15
    raw = C.CDLL(_lib.LIB_PATH)      # the library itself, not the binding's table
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", text), name
        assert name in _lib.PROTOTYPES, name
        assert getattr(raw, name) is not None, name      # (AttributeError where the symbol is not exported)


@pytest.mark.parametrize("d, width", [(16, 32), (20, 32), (40, 64), (64, 64), (96, 128), (160, 0)])
def test_table_width_rule(d, width):
    lib = _lib.load()
    s = E.MolShapeSpec(64, 64, d, 4, 4, 64, 128, 128, 128).to_c()
    assert lib.rails_mol_generic_supported(C.byref(s)) == 1, _lib.last_error()
    assert lib.rails_mol_generic_table_width(C.byref(s)) == width
    if width == 0:
        assert "dot_product_dimension <= 128" in _lib.last_error() and "160" in _lib.last_error()


def _cpu_module(cfg, w):
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
    mol.load_state_dict(w, strict=True)
    return mol.eval()


def test_the_attribute_is_part_of_the_engine_cache_key(monkeypatch):
    """Binding an engine needs a device for one launch only, the gate pack's: with that launch, the device check and the stream lookup stubbed
    out, MoLSimilarity.engine() and MolEngine.__init__ run here as they are, on CPU tensors."""
    import contextlib

    cfg, w = next((cfg, w) for name, cfg, w, a in generic_cases() if name == "g_8x8x40")
    mol = _cpu_module(cfg, w)
    assert mol.generic_candidates is False
    monkeypatch.setattr(E, "_require_device", lambda t, what: None)
    monkeypatch.setattr(E, "_on_device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(E, "_stream", lambda: None)
    made = []
    monkeypatch.setattr(_lib.load(), "rails_mol_generic_pack_gate_weights", lambda *a: made.append(1) or 0)
    plain = mol.engine()
    assert plain.route == "generic" and not plain.candidates and not plain.score_indexed_supported(4, 64)
    assert mol.engine() is plain
    mol.generic_candidates = True
    cand = mol.engine()
    assert cand is not plain and cand.route == "generic" and cand.candidates and cand.score_indexed_supported(4, 64)
    assert cand.table_width == 64 and cand.scan_shape.dot_product_dimension == 64 and cand.shape.dot_product_dimension == 40
    assert mol.engine() is cand
    mol.generic_candidates = False
    again = mol.engine()
    assert again is not cand and not again.candidates and not again.score_indexed_supported(4, 64)
    with pytest.raises(NotImplementedError, match="generic scoring route"):
        again.build_coarse_table(E.MolIndex(torch.empty(0), 0))
    assert len(made) == 3
