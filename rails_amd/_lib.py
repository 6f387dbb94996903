"""ctypes binding of librails_amd.so (the C ABI declared in include/rails_amd.h).

There is no fallback: if the shared library is missing or a call fails, this module raises.
Build it with `python -c "import __graft_entry__ as g; g.build()"` or `make -C rails_amd/csrc`.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# RAILS_AMD_LIBRARY: load another build of the same library (e.g. the parent commit's, for an A/B run in one place)
LIB_PATH = os.environ.get("RAILS_AMD_LIBRARY") or os.path.join(_HERE, "librails_amd.so")

RAILS_ABI_VERSION = 15  # include/rails_amd.h
RAILS_OK = 0
RAILS_EINVAL = -22
RAILS_ENOTSUP = -95
RAILS_ENOMEM = -12
RAILS_ELAUNCH = -5
RAILS_FUSE_MAX = 0
RAILS_FUSE_SUM = 1
RAILS_GEGLU = 0
RAILS_SWIGLU = 1
RAILS_MAX_UID_TABLES = 4
RAILS_PRECISION_FP32 = 0
RAILS_PRECISION_F16X3 = 1
RAILS_PRECISION_F16X1 = 2
RAILS_COMBINE_GLU_SILU = 0
RAILS_COMBINE_NONE = 1
RAILS_ACT_NONE = 0
RAILS_ACT_SILU = 1
RAILS_ACT_RELU = 2
RAILS_ACT_GELU = 3
RAILS_SASREC_DECODE_MAX_ROWS = 65535 * 32
RAILS_HSTU_DECODE_MAX_ROWS = 65535 * 32

_f32p = C.POINTER(C.c_float)


class MolShape(C.Structure):
    _fields_ = [
        ("query_embedding_dim", C.c_int32),
        ("item_embedding_dim", C.c_int32),
        ("dot_product_dimension", C.c_int32),
        ("query_dot_product_groups", C.c_int32),
        ("item_dot_product_groups", C.c_int32),
        ("query_hidden_dim", C.c_int32),
        ("gating_query_hidden_dim", C.c_int32),
        ("gating_item_hidden_dim", C.c_int32),
        ("gating_qi_hidden_dim", C.c_int32),
        ("query_nonlinearity", C.c_int32),
        ("num_uid_tables", C.c_int32),
        ("dot_product_l2_norm", C.c_int32),
        ("temperature", C.c_float),
        ("eps", C.c_float),
        ("precision", C.c_int32),
        ("item_hidden_dim", C.c_int32),
        ("item_nonlinearity", C.c_int32),
        ("gating_combination", C.c_int32),
        ("gating_has_query", C.c_int32),
        ("gating_has_item", C.c_int32),
    ]


class MolWeights(C.Structure):
    _fields_ = [
        ("q_glu_w", C.c_void_p),
        ("q_glu_b", C.c_void_p),
        ("q_proj_w", C.c_void_p),
        ("q_proj_b", C.c_void_p),
        ("uid_table", C.c_void_p * RAILS_MAX_UID_TABLES),
        ("uid_hash_size", C.c_int64 * RAILS_MAX_UID_TABLES),
        ("i_proj_w", C.c_void_p),
        ("i_proj_b", C.c_void_p),
        ("gq_w1", C.c_void_p),
        ("gq_b1", C.c_void_p),
        ("gq_w2", C.c_void_p),
        ("gi_w1", C.c_void_p),
        ("gi_b1", C.c_void_p),
        ("gi_w2", C.c_void_p),
        ("gqi_w1", C.c_void_p),
        ("gqi_b1", C.c_void_p),
        ("gqi_w2", C.c_void_p),
        ("gqi_b2", C.c_void_p),
        ("i_glu_w", C.c_void_p),
        ("i_glu_b", C.c_void_p),
    ]


# the encoders' per-layer pointer tables (rails_hstu_encode_fused, rails_hstu_decode, rails_sasrec_encode_fused, rails_sasrec_decode)
class HstuLayer(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("uvqk", "o_w", "o_b", "ts_w", "pos_w")]


class HstuDecodeLayer(C.Structure):
    _fields_ = HstuLayer._fields_ + [(name, C.c_void_p) for name in ("v", "q", "k", "outputs")]


class SasrecLayer(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("in_proj_weight", "in_proj_bias", "out_proj_weight", "out_proj_bias",
                                                "conv1_weight", "conv1_bias", "conv2_weight", "conv2_bias")]


class SasrecDecodeLayer(C.Structure):
    _fields_ = SasrecLayer._fields_ + [("k", C.c_void_p), ("v", C.c_void_p)]


def layer_table(struct, layers, device=None, cached=None):
    """(key, table): an array of `struct`, one entry per layer, its fields the data pointers of that layer's tensors in declaration
    order (None, or fields past the end of a row: NULL).  device None: a host ctypes array; otherwise a tensor on `device` holding
    its bytes.  `cached`, the (key, table) of an earlier call, is returned as it is while the pointers are the same."""
    key = tuple(tuple(0 if t is None else t.data_ptr() for t in layer) for layer in layers)
    if cached is not None and cached[0] == key:
        return cached
    table = (struct * len(key))(*(struct(*ptrs) for ptrs in key))
    if device is not None:
        import torch
        table = torch.frombuffer(bytearray(table), dtype=torch.uint8).to(device)
    return key, table


# name -> (restype, argtypes): one entry per declaration in include/rails_amd.h
_SHAPE_P = C.POINTER(MolShape)
_WEIGHTS_P = C.POINTER(MolWeights)
PROTOTYPES = {
    "rails_last_error": (C.c_char_p, []),
    "rails_device_compute_units": (C.c_int, []),
    "rails_mol_shape_supported": (C.c_int, [_SHAPE_P]),
    "rails_mol_gate_pack_floats": (C.c_size_t, [_SHAPE_P]),
    "rails_mol_pack_gate_weights": (C.c_int, [_SHAPE_P, _WEIGHTS_P, C.c_void_p, C.c_void_p]),
    "rails_mol_index_floats": (C.c_size_t, [_SHAPE_P, C.c_int64]),
    "rails_mol_index_build": (C.c_int, [_SHAPE_P, _WEIGHTS_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_mol_index_unpack": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_mol_index_gather": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p],
    ),
    "rails_mol_query_pack_floats": (C.c_size_t, [_SHAPE_P, C.c_int32]),
    "rails_mol_query_prologue": (
        C.c_int,
        [_SHAPE_P, _WEIGHTS_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "rails_mol_query_prologue_both": (
        C.c_int,
        [_SHAPE_P, _WEIGHTS_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "rails_mol_score_dense": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    ),
    "rails_mol_index_update": (C.c_int, [_SHAPE_P, _WEIGHTS_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_mol_generic_index_update": (C.c_int, [_SHAPE_P, _WEIGHTS_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_mol_index_rows_update": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_mol_index_clear_tail": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_mol_generic_index_clear_tail": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_mol_coarse_update": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_mol_component_update": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_mol_index_rows_floats": (C.c_size_t, [_SHAPE_P, C.c_int64]),
    "rails_mol_index_rows_build": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_mol_score_indexed_rows": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_merge_candidates_verdict": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_int32, C.c_float,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_candidates_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "rails_candidates_select": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_candidates_finish": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                          C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_mol_score_dense_upper_supported": (C.c_int, [_SHAPE_P]),
    "rails_mol_score_dense_upper": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    ),
    "rails_mol_score_candidates": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p],
    ),
    # the shape-generic fp32 scoring route (same argument lists as the fused counterparts; score_candidates also takes run_if)
    "rails_mol_generic_supported": (C.c_int, [_SHAPE_P]),
    "rails_mol_generic_gate_pack_floats": (C.c_size_t, [_SHAPE_P]),
    "rails_mol_generic_index_floats": (C.c_size_t, [_SHAPE_P, C.c_int64]),
    "rails_mol_generic_query_pack_floats": (C.c_size_t, [_SHAPE_P, C.c_int32]),
    "rails_mol_generic_pack_gate_weights": (C.c_int, [_SHAPE_P, _WEIGHTS_P, C.c_void_p, C.c_void_p]),
    "rails_mol_generic_index_build": (C.c_int, [_SHAPE_P, _WEIGHTS_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_mol_generic_index_unpack": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_mol_generic_query_prologue": (
        C.c_int,
        [_SHAPE_P, _WEIGHTS_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "rails_mol_generic_score_dense": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    ),
    "rails_mol_generic_score_candidates": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    ),
    # the generic route's candidate entries: in-place re-scoring (positions, n_cand, counts), the bf16 tables of the padded width, the Eq pad
    "rails_mol_generic_score_indexed": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    ),
    # the explaining launches (score_of / explain_of): the per-row and the indexed launch with component_logits and weights beside the logits
    "rails_mol_generic_explain": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "rails_mol_generic_explain_indexed": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    # the backward of the per-row-candidates launch (the differentiable MoLSimilarity.forward)
    "rails_mol_generic_pair_backward_supported": (C.c_int, [_SHAPE_P]),
    "rails_mol_generic_gate_pack_t_floats": (C.c_size_t, [_SHAPE_P]),
    "rails_mol_generic_pack_gate_weights_t": (C.c_int, [_SHAPE_P, _WEIGHTS_P, C.c_void_p, C.c_void_p]),
    "rails_mol_generic_pair_backward_workspace_bytes": (C.c_size_t, [_SHAPE_P, C.c_int64]),
    "rails_mol_generic_pair_backward": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_void_p],
    ),
    "rails_mol_generic_table_width": (C.c_int32, [_SHAPE_P]),
    "rails_mol_generic_coarse_build": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_mol_generic_coarse_update": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_mol_generic_component_build": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_mol_generic_component_update": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_mol_generic_eq_pad": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_mips_index_floats": (C.c_size_t, [C.c_int32, C.c_int64]),
    "rails_mips_index_build": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_mips_index_update": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_mips_index_gather_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_mips_index_clear_tail": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "rails_mips_query_ws_floats": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rails_mips_score": (
        C.c_int,
        [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    ),
    "rails_id_map_slots": (C.c_int64, [C.c_int64]),
    "rails_id_map_bytes": (C.c_size_t, [C.c_int64]),
    "rails_id_map_clear": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_id_map_insert": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_id_map_erase": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_id_map_lookup": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_item_mask_words": (C.c_int64, [C.c_int64]),
    "rails_item_mask_tile_items": (C.c_int64, []),
    "rails_item_mask_pack": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_item_mask_set": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_item_mask_clear": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_item_tags_effective": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_item_tags_count": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_item_mask_from_tags": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_scores_mask_tags": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p,
                                         C.c_void_p]),
    "rails_item_mask_count": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_item_mask_positions_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "rails_item_mask_positions": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rails_scores_at_eligible": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rails_mips_score_indexed": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_void_p]),
    "rails_scores_mask": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    "rails_scores_rank_keys": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_scores_rank": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_item_mask_clear_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_scores_lse_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "rails_scores_lse": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rails_scores_log_prob": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_void_p]),
    "rails_scores_gumbel": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_float, C.c_uint64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_int64, C.c_void_p]),
    "rails_scores_range_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "rails_scores_range_count": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_scores_range_write": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_scores_range_sort": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "rails_scores_range_decode": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_scores_fuse_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p]),
    "rails_topk_fuse_lists": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_lists_union": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_void_p]),
    "rails_dot_rowwise": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p],
    ),
    "rails_mol_coarse_table_bytes": (C.c_size_t, [_SHAPE_P, C.c_int64]),
    "rails_mol_coarse_build": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_mol_coarse_topk_workspace_bytes": (C.c_size_t, [_SHAPE_P, C.c_int32, C.c_int64, C.c_int32]),
    "rails_mol_coarse_topk_capacity": (C.c_int32, [C.c_int32, C.c_int64, C.c_int32]),
    "rails_mol_coarse_topk": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                        C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_mol_coarse_topk_visible": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                                C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_mol_coarse_topk_tagged": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                               C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_mol_scan_plan": (C.c_int32, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "rails_mol_coarse_prefilter_bytes": (C.c_size_t, [_SHAPE_P, C.c_int64]),
    "rails_mol_coarse_prefilter_build": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_mol_coarse_score": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    ),
    "rails_mol_component_table_bytes": (C.c_size_t, [_SHAPE_P, C.c_int64]),
    "rails_mol_component_build": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "rails_mol_component_topk_capacity": (C.c_int32, [_SHAPE_P, C.c_int32, C.c_int64, C.c_int32]),
    "rails_mol_component_topk_workspace_bytes": (C.c_size_t, [_SHAPE_P, C.c_int32, C.c_int64, C.c_int32]),
    "rails_mol_component_topk": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_mol_component_topk_visible": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_mol_component_topk_tagged": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_ivf_build_workspace_bytes": (C.c_size_t, [_SHAPE_P, C.c_int64, C.c_int32, C.c_int32]),
    "rails_ivf_components16_build": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "rails_ivf_train": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "rails_ivf_assign": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_ivf_build_lists": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "rails_ivf_lists_edit_workspace_bytes": (C.c_size_t, [_SHAPE_P, C.c_int64, C.c_int32, C.c_int64]),
    "rails_ivf_lists_edit": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rails_ivf_plan": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rails_ivf_search_workspace_bytes": (C.c_size_t, [_SHAPE_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rails_ivf_search": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_ivf_list_words": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_ivf_list_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_ivf_plan_filtered": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "rails_ivf_search_filtered": (C.c_int, [_SHAPE_P, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int32, C.c_void_p]),
    "rails_mol_component_score": (
        C.c_int,
        [_SHAPE_P, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    ),
    "rails_hstu_preprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "rails_rows_layer_norm": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_gemm_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                 C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_glu_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    "rails_hstu_time_buckets": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_hstu_attention": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_hstu_fused_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rails_hstu_encode_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "rails_hstu_decode_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rails_hstu_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_float, C.c_void_p, C.c_void_p]),
    "rails_hstu_decode_rows_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rails_hstu_decode_rows_workspace_floats": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rails_hstu_decode_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_gemm_f32_id_masked": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_sasrec_attention": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_sasrec_fused_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rails_sasrec_encode_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "rails_sasrec_decode_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rails_sasrec_decode_workspace_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rails_sasrec_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_sasrec_decode_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "rails_rows_normalize": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "rails_sort_rows_i64": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_mask_sorted_duplicates": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p],
    ),
    "rails_topk_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32]),
    "rails_topk": (
        C.c_int,
        [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p],
    ),
    "rails_topk_candidates": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_topk_candidates_filtered": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_rerank_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rails_rerank_topk_filtered": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_topk_collapse": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_topk_collapse_quota": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_scores_group_next": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rails_scores_group_max": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_void_p]),
    "rails_topk_keys": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_topk_mmr_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "rails_topk_mmr": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "rails_pack_candidates": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_merge_candidates": (
        C.c_int,
        [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "rails_rescore_select": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_group_keys_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_group_keys_supported": (C.c_int, [C.c_int32, C.c_int32]),
    "rails_group_keys_merge_own": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_int64, C.c_int32, C.c_void_p]),
    "rails_abi_version": (C.c_int, []),
    "rails_hash_item_table": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "rails_mol_gate_combine": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_topk_filter_fusable": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "rails_topk_filtered": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rails_merge_candidates_filtered": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rails_mol_score_indexed_supported": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
    "rails_mol_score_indexed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_range_flag_i32": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_rescore_verdict": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    "rails_margin_stats": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rails_mfma_probe_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_mfma_probe_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rails_scalar_probe_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rails_filter_seen_ids": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
         C.c_void_p],
    ),
}

_lib: Optional[C.CDLL] = None


class RailsAmdError(RuntimeError):
    """A call into librails_amd.so failed (message from rails_last_error())."""


def load() -> C.CDLL:
    """Load librails_amd.so once.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C rails_amd/csrc`). "
            "rails_amd has no CPU or PyTorch fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    got = lib.rails_abi_version()
    if got != RAILS_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} implements ABI version {got}, this binding was written for {RAILS_ABI_VERSION}: rebuild the library "
                          "(the structs of include/rails_amd.h changed size between versions)")
    _lib = lib
    return lib


def last_error() -> str:
    return (load().rails_last_error() or b"").decode("utf-8", "replace")


def check(code: int, what: str) -> None:
    """Turn a RAILS_E* code into the exception the reference raises in the same situation."""
    if code == RAILS_OK:
        return
    msg = f"{what}: {last_error()} (code {code})"
    if code == RAILS_EINVAL:
        raise ValueError(msg)
    if code == RAILS_ENOTSUP:
        raise NotImplementedError(msg)
    if code == RAILS_ENOMEM:
        raise MemoryError(msg)
    raise RailsAmdError(msg)
