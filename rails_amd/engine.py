"""Thin Python driver over the C ABI: owns the packed device buffers, passes raw device pointers.

PyTorch is used for device memory, the current stream and (elsewhere) torch.distributed only; every
floating-point operation of the path runs in the HIP kernels behind librails_amd.so.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib

TILE_ITEMS = 32
PRECISIONS = ("fp32", "f16x3", "f16x3-exact", "f16-exact", "f16x1")
# "f16x3-exact" / "f16-exact": the f16x3 / one-product f16 kernels pick candidates, an fp32 companion engine (`MolEngine.exact`)
# re-scores them, so the brute-force top-k is the fp32 path's result bit for bit (topk_modules.MoLBruteForceTopK).  Every other
# use of such an engine behaves as "f16x3": the packs are the same, only the dense pass of "f16-exact" runs the one-product kernels.
# "f16x1": the one-product kernels as they are (logits ~1e-2 off: measurement and tools only, NOT a parity mode).
_C_PRECISION = {"fp32": _lib.RAILS_PRECISION_FP32, "f16x3": _lib.RAILS_PRECISION_F16X3, "f16x1": _lib.RAILS_PRECISION_F16X1}


def default_precision() -> str:
    """"fp32" (exact fp32 MFMA, the parity path) unless RAILS_PRECISION selects an opt-in mode ("f16x3", "f16x3-exact")."""
    p = os.environ.get("RAILS_PRECISION", "fp32")
    if p not in PRECISIONS:
        raise ValueError(f"RAILS_PRECISION must be one of {PRECISIONS}, got {p!r}")
    return p


@dataclasses.dataclass(frozen=True)
class MolShapeSpec:
    """Hyper-parameters of a MoL module (names as in create_mol_interaction_module,
    reference modeling/similarity_utils.py:42-70)."""

    query_embedding_dim: int
    item_embedding_dim: int
    dot_product_dimension: int
    query_dot_product_groups: int
    item_dot_product_groups: int
    query_hidden_dim: int
    gating_query_hidden_dim: int
    gating_item_hidden_dim: int
    gating_qi_hidden_dim: int
    query_nonlinearity: str = "geglu"
    uid_embedding_hash_sizes: Tuple[int, ...] = ()
    dot_product_l2_norm: bool = True
    temperature: float = 0.05
    eps: float = 1e-6
    item_hidden_dim: int = -1                    # > 0: GLU hidden layer in the item projection
    item_nonlinearity: str = "geglu"
    gating_combination_type: str = "glu_silu"    # "glu_silu" | "none"
    gating_query_fn: bool = True                 # False: no query-only gate part (only with "none")
    gating_item_fn: bool = True                  # False: no item-only gate part (only with "none")

    @property
    def num_logits(self) -> int:
        return self.query_dot_product_groups * self.item_dot_product_groups

    def to_c(self, precision: str = "fp32") -> _lib.MolShape:
        if self.query_nonlinearity not in ("geglu", "swiglu") or self.item_nonlinearity not in ("geglu", "swiglu"):
            raise ValueError(f"Unknown nonlinearity {self.query_nonlinearity} / {self.item_nonlinearity}")
        if self.gating_combination_type not in ("glu_silu", "none"):
            raise ValueError(f"Unknown combination_type {self.gating_combination_type}")
        return _lib.MolShape(
            self.query_embedding_dim, self.item_embedding_dim, self.dot_product_dimension,
            self.query_dot_product_groups, self.item_dot_product_groups, self.query_hidden_dim,
            self.gating_query_hidden_dim, self.gating_item_hidden_dim, self.gating_qi_hidden_dim,
            _lib.RAILS_GEGLU if self.query_nonlinearity == "geglu" else _lib.RAILS_SWIGLU,
            len(self.uid_embedding_hash_sizes), 1 if self.dot_product_l2_norm else 0,
            float(self.temperature), float(self.eps),
            _C_PRECISION[precision],
            int(self.item_hidden_dim), _lib.RAILS_GEGLU if self.item_nonlinearity == "geglu" else _lib.RAILS_SWIGLU,
            _lib.RAILS_COMBINE_NONE if self.gating_combination_type == "none" else _lib.RAILS_COMBINE_GLU_SILU,
            1 if self.gating_query_fn else 0, 1 if self.gating_item_fn else 0,
        )

    def weight_fields(self) -> Dict[str, str]:
        """state_dict key -> field of rails_mol_weights for THIS topology (the module indices inside the
        reference's Sequentials are part of the keys, modeling/similarity_utils.py:88-207)."""
        f: Dict[str, str] = {}
        q = "_query_embeddings_fn._query_emb_proj_module."
        if self.query_hidden_dim > 0:
            f.update({q + "1._w": "q_glu_w", q + "1._b": "q_glu_b", q + "2.weight": "q_proj_w", q + "2.bias": "q_proj_b"})
        else:
            f.update({q + "1.weight": "q_proj_w", q + "1.bias": "q_proj_b"})
        i = "_item_embeddings_fn._item_emb_proj_module."
        if self.item_hidden_dim > 0:
            f.update({i + "1._w": "i_glu_w", i + "1._b": "i_glu_b", i + "2.weight": "i_proj_w", i + "2.bias": "i_proj_b"})
        else:
            f.update({i + "1.weight": "i_proj_w", i + "1.bias": "i_proj_b"})
        if self.gating_query_fn:
            g = "_gating_fn._query_only_partial_module."
            f.update({g + "0.weight": "gq_w1", g + "0.bias": "gq_b1", g + "2.weight": "gq_w2"})
        if self.gating_item_fn:
            g = "_gating_fn._item_only_partial_module."
            f.update({g + "1.weight": "gi_w1", g + "1.bias": "gi_b1", g + "3.weight": "gi_w2"})
        g = "_gating_fn._qi_partial_module."
        if self.gating_qi_hidden_dim > 0:
            f.update({g + "1.weight": "gqi_w1", g + "1.bias": "gqi_b1", g + "3.weight": "gqi_w2", g + "3.bias": "gqi_b2"})
        else:   # Sequential(Dropout, Linear(L, L)): modeling/similarity_utils.py:199-206
            f.update({g + "1.weight": "gqi_w1", g + "1.bias": "gqi_b1"})
        return f


# state_dict key -> field of rails_mol_weights for the shipped topology (MolShapeSpec.weight_fields() covers the variants)
WEIGHT_FIELDS = {
    "_query_embeddings_fn._query_emb_proj_module.1._w": "q_glu_w",
    "_query_embeddings_fn._query_emb_proj_module.1._b": "q_glu_b",
    "_query_embeddings_fn._query_emb_proj_module.2.weight": "q_proj_w",
    "_query_embeddings_fn._query_emb_proj_module.2.bias": "q_proj_b",
    "_item_embeddings_fn._item_emb_proj_module.1.weight": "i_proj_w",
    "_item_embeddings_fn._item_emb_proj_module.1.bias": "i_proj_b",
    "_gating_fn._query_only_partial_module.0.weight": "gq_w1",
    "_gating_fn._query_only_partial_module.0.bias": "gq_b1",
    "_gating_fn._query_only_partial_module.2.weight": "gq_w2",
    "_gating_fn._item_only_partial_module.1.weight": "gi_w1",
    "_gating_fn._item_only_partial_module.1.bias": "gi_b1",
    "_gating_fn._item_only_partial_module.3.weight": "gi_w2",
    "_gating_fn._qi_partial_module.1.weight": "gqi_w1",
    "_gating_fn._qi_partial_module.1.bias": "gqi_b1",
    "_gating_fn._qi_partial_module.3.weight": "gqi_w2",
    "_gating_fn._qi_partial_module.3.bias": "gqi_b2",
}


_cur_dev = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device    # the binding itself: torch.cuda.current_device() adds a lazy-init check (0.7 us, six per step)


def _stream() -> C.c_void_p:
    # raw handle of torch's current stream on the current device (torch.cuda.current_stream() costs ~9 us per call)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(_cur_dev()))


class _on_device:
    """`with _on_device(dev)`: make `dev` the current HIP device for the enclosed launches.  Unlike torch.cuda.device it
    costs nothing when `dev` already is current (the one-process-per-GPU case), which matters for sub-millisecond steps."""

    __slots__ = ("idx", "prev")

    def __init__(self, dev: torch.device):
        self.idx = dev.index if dev.index is not None else _cur_dev()
        self.prev = -1

    def __enter__(self):
        cur = _cur_dev()
        if cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
        return False


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


_EMPTY_INV: Dict[torch.device, torch.Tensor] = {}


def _inv_ptr(invalid_ids: Optional[torch.Tensor]) -> C.c_void_p:
    """Pointer of a (rows, width) seen-id tensor for the entry points that filter.  A zero-WIDTH tensor (a workload without history:
    BASELINE configs 4 and 5) has a null data_ptr, which the C ABI reads as "no filter requested": hand it one never-read word instead,
    so that `width == 0` keeps meaning "filter with nothing to remove" (k of the k' winners, same outputs contract)."""
    if invalid_ids is None or invalid_ids.numel() > 0:
        return _ptr(invalid_ids)
    dev = invalid_ids.device
    if dev not in _EMPTY_INV:
        _EMPTY_INV[dev] = torch.zeros(1, dtype=torch.int64, device=dev)
    return _ptr(_EMPTY_INV[dev])


def _require_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} must live on the GPU: rails_amd runs its path in HIP kernels only and has no CPU fallback "
            f"(got a tensor on {t.device})"
        )


def _f32c(t: torch.Tensor) -> torch.Tensor:
    """fp32 + contiguous view/copy of a device tensor (plumbing: dtype cast, no math)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def resized(t: torch.Tensor, n: int, dim: int = 0, zero: bool = False) -> torch.Tensor:
    """A fresh contiguous copy of `t` with n entries along `dim` (the one resize of the in-place corpus API): the first n when that cuts (or
    keeps) it, else all of `t` with room behind it -- zeros where the buffer has padding a fresh build leaves zero, else unwritten (the caller
    writes every new entry)."""
    old = t.shape[dim]
    if n <= old:
        return t.narrow(dim, 0, n).clone(memory_format=torch.contiguous_format)
    shape = list(t.shape)
    shape[dim] = n
    out = (torch.zeros if zero else torch.empty)(shape, dtype=t.dtype, device=t.device)
    out.narrow(dim, 0, old).copy_(t)
    return out


class MolIndex:
    """Tile-packed item index: Ex (l2-normalised component embeddings) + gi (item gate) per item."""

    def __init__(self, buf: torch.Tensor, n_items: int):
        self.buf = buf
        self.n_items = n_items

    def items(self, lo: int, hi: int) -> "MolIndex":
        """The sub-index of items [lo, hi) as a view (lo must be a tile boundary: tiles are stored back to back)."""
        if lo % TILE_ITEMS != 0 or not 0 <= lo <= hi <= self.n_items:
            raise ValueError(f"sub-index [{lo}, {hi}) must start on a {TILE_ITEMS}-item tile boundary inside [0, {self.n_items}]")
        tiles = (self.n_items + TILE_ITEMS - 1) // TILE_ITEMS
        tile_floats = self.buf.numel() // max(tiles, 1)
        t0, t1 = lo // TILE_ITEMS, (hi + TILE_ITEMS - 1) // TILE_ITEMS
        return MolIndex(self.buf[t0 * tile_floats : t1 * tile_floats], hi - lo)


class MolEngine:
    """One MoL module's weights bound to the HIP kernels."""

    def __init__(self, spec: MolShapeSpec, weights: Dict[str, torch.Tensor], precision: Optional[str] = None, route: Optional[str] = None,
                 generic_candidates: bool = False):
        """route: None -- the fused kernels where rails_mol_shape_supported says so, else the shape-generic fp32 kernels
        (rails_mol_generic_*); "generic" -- the generic kernels whatever the shape.  By shape and precision alone, never by size.
        generic_candidates: on the generic route, the engine is candidate-capable: candidates are scored in place on
        the generic index and the bf16 coarse / component tables are cut from it at the padded width table_width; no effect on the fused route."""
        self.lib = _lib.load()
        self.spec = spec
        precision = precision or default_precision()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
        if route not in (None, "generic"):
            raise ValueError(f"route must be None or 'generic', got {route!r}")
        self.route = "fused"
        self.precision = {"f16x3-exact": "f16x3", "f16-exact": "f16x3", "f16x1": "f16x3"}.get(precision, precision)   # format of the packs
        self.shape = spec.to_c(self.precision)
        if route == "generic":
            if not self.lib.rails_mol_generic_supported(C.byref(self.shape)):
                raise NotImplementedError(_lib.last_error())
            self.route = "generic"
        elif not self.lib.rails_mol_shape_supported(C.byref(self.shape)):
            # the fused check's message stays where it names the reason itself (a hidden-layer-free pair gate, a bad combination);
            # "no fused scoring kernel" is the one the generic route answers
            fused_msg = _lib.last_error()
            if not self.lib.rails_mol_generic_supported(C.byref(self.shape)):
                generic_msg = _lib.last_error()
                raise NotImplementedError(fused_msg if not fused_msg.startswith("no fused scoring kernel") else f"{fused_msg}; {generic_msg}")
            self.route = "generic"
        # candidate-capable: the opt-in of the generic route.  The bf16 scans then run under `scan_shape`, a copy of the shape whose
        # dot_product_dimension is the tables' padded width (32 / 64 / 128; 0: d > 128, no tables -- the candidate modules refuse)
        self.candidates = bool(generic_candidates) and self.route == "generic"
        self.scan_shape = self.shape
        self.table_width = spec.dot_product_dimension
        if self.candidates:
            self.table_width = int(self.lib.rails_mol_generic_table_width(C.byref(self.shape)))
            if self.table_width:
                self.scan_shape = spec.to_c(self.precision)
                self.scan_shape.dot_product_dimension = self.table_width
        self.exact: Optional["MolEngine"] = MolEngine(spec, weights, "fp32") if precision.endswith("-exact") else None
        # the shape the DENSE pass is launched with: the one-product kernels for "f16-exact" / "f16x1" (same packs, lo halves ignored)
        self.dense_precision = "f16x1" if precision in ("f16-exact", "f16x1") else self.precision
        self.dense_shape = spec.to_c(self.dense_precision)
        self._fp32_shape = spec.to_c("fp32")     # for the derived bf16 tables, which are cut from an fp32-format index
        self._keep = []  # fp32 contiguous device tensors the weight struct points into
        w = _lib.MolWeights()
        for key, field in spec.weight_fields().items():
            if key not in weights:
                raise KeyError(f"MoL weight '{key}' is missing")
            t = weights[key]
            _require_device(t, f"weight {key}")
            t = _f32c(t.detach())
            self._keep.append(t)
            setattr(w, field, t.data_ptr())
        for i, hs in enumerate(spec.uid_embedding_hash_sizes):
            key = f"_query_embeddings_fn._uid_embeddings_{i}.weight"
            t = _f32c(weights[key].detach())
            _require_device(t, f"weight {key}")
            if t.shape[0] != hs + 1:
                raise ValueError(f"{key} has {t.shape[0]} rows, expected hash_size + 1 = {hs + 1}")
            self._keep.append(t)
            w.uid_table[i] = t.data_ptr()
            w.uid_hash_size[i] = int(hs)
        self.weights = w
        self.device = self._keep[0].device
        if self.precision == "f16x3":
            self._check_f16_range(weights)
        generic = self.route == "generic"
        n = (self.lib.rails_mol_generic_gate_pack_floats if generic else self.lib.rails_mol_gate_pack_floats)(C.byref(self.shape))
        self.gate_pack = torch.empty(n, dtype=torch.float32, device=self.device)
        with _on_device(self.device):
            if generic:
                _lib.check(self.lib.rails_mol_generic_pack_gate_weights(C.byref(self.shape), C.byref(self.weights), _ptr(self.gate_pack), _stream()),
                           "rails_mol_generic_pack_gate_weights")
                return
            _lib.check(
                self.lib.rails_mol_pack_gate_weights(C.byref(self.shape), C.byref(self.weights), _ptr(self.gate_pack), _stream()),
                "rails_mol_pack_gate_weights",
            )

    def _name(self, name: str) -> str:
        """Name of the entry point `rails_mol_<name>` of this engine's route (also the label of its error messages)."""
        return ("rails_mol_generic_" if self.route == "generic" else "rails_mol_") + name

    def _fn(self, name: str):
        return getattr(self.lib, self._name(name))

    def _fused_only(self, what: str) -> None:
        if self.route == "generic":
            raise NotImplementedError(f"{what} is not built on the generic scoring route")

    def _candidates_only(self, what: str) -> None:
        """The candidate entries: the fused route, or the generic route bound with generic_candidates=True (and d <= 128 where tables are cut)."""
        if self.route == "generic" and not self.candidates:
            raise NotImplementedError(f"{what} is not built on the generic scoring route")

    def _tables_only(self, what: str) -> None:
        self._candidates_only(what)
        if self.table_width == 0:
            raise NotImplementedError(f"{what}: the generic route's bf16 tables take dot_product_dimension <= 128 (the widest bf16 scan), "
                                      f"got d = {self.spec.dot_product_dimension}")

    def _scan_eq(self, eq: torch.Tensor) -> torch.Tensor:
        """Eq as the bf16 scans read it: (B, P_Q, table_width) fp32 contiguous -- the caller's tensor where d is the width already, else a
        zero-padded copy (rails_mol_generic_eq_pad); a tensor of the padded width passes through."""
        eq = _f32c(eq)
        if eq.shape[-1] == self.table_width:
            return eq
        if not self.candidates or eq.shape[-1] != self.spec.dot_product_dimension:
            raise ValueError(f"Eq must be (B, P_Q, {self.spec.dot_product_dimension}), got {tuple(eq.shape)}")
        out = torch.empty(eq.shape[:-1] + (self.table_width,), dtype=torch.float32, device=eq.device)
        with _on_device(eq.device):
            _lib.check(self.lib.rails_mol_generic_eq_pad(C.byref(self.shape), _ptr(eq), eq.numel() // eq.shape[-1], _ptr(out), _stream()), "rails_mol_generic_eq_pad")
        return out

    def _check_f16_range(self, weights: Dict[str, torch.Tensor]) -> None:
        """precision='f16x3' keeps cl, hid and the gate weights as f16 hi + lo.  Small values are safe (f16 subnormals are
        kept by the MFMA: absolute resolution 2^-25); large ones are not (f16 max 65504), so bound the hidden layer for
        |cl| <= 1/temperature (unit-norm components) and refuse weights that could overflow."""
        w1 = weights["_gating_fn._qi_partial_module.1.weight"].detach().float()
        b1 = weights["_gating_fn._qi_partial_module.1.bias"].detach().float()
        w2 = weights["_gating_fn._qi_partial_module.3.weight"].detach().float()
        cl_max = 1.0 / self.spec.temperature * 1.001
        log2e = 1.4426950408889634
        t_max = log2e * (cl_max * float(w1.abs().sum(1).max()) + float(b1.abs().max()))
        limit = 60000.0
        if cl_max >= limit or t_max >= limit or log2e * float(w1.abs().max()) >= limit or float(w2.abs().max()) >= limit:
            raise NotImplementedError("precision='f16x3': pair-gate weights / temperature put an operand outside the f16 range; use fp32")

    # ---- item side ----------------------------------------------------------------------------
    def build_index(self, items: torch.Tensor) -> MolIndex:
        """items: (N, D_i) on the GPU -> tile-packed index (reference: item-side work of
        rails/similarities/mol/similarity_fn.py:378-387 + :170-171, done once)."""
        _require_device(items, "item_embeddings")
        if items.dim() != 2 or items.shape[1] != self.spec.item_embedding_dim:
            raise ValueError(f"item_embeddings must be (N, {self.spec.item_embedding_dim}), got {tuple(items.shape)}")
        items = _f32c(items)
        n = items.shape[0]
        floats = self._fn("index_floats")(C.byref(self.shape), n)
        buf = torch.empty(floats, dtype=torch.float32, device=items.device)
        with _on_device(items.device):
            _lib.check(
                self._fn("index_build")(C.byref(self.shape), C.byref(self.weights), _ptr(items), n, _ptr(buf), _stream()),
                self._name("index_build"),
            )
        return MolIndex(buf, n)

    def unpack_index(self, index: MolIndex, want_ex: bool = True, want_gi: bool = True):
        s = self.spec
        ex = torch.empty((index.n_items, s.item_dot_product_groups, s.dot_product_dimension), dtype=torch.float32, device=index.buf.device) if want_ex else None
        gi = torch.empty((index.n_items, s.num_logits), dtype=torch.float32, device=index.buf.device) if want_gi else None
        with _on_device(index.buf.device):
            _lib.check(
                self._fn("index_unpack")(C.byref(self.shape), _ptr(index.buf), index.n_items, _ptr(ex), _ptr(gi), _stream()),
                self._name("index_unpack"),
            )
        return ex, gi

    def build_index_rows(self, index: MolIndex) -> torch.Tensor:
        """Row-major copy of an exact-fp32 index (include/rails_amd.h rails_mol_index_rows_build): what score_indexed_rows reads candidates from."""
        self._fused_only("the row-major index copy")
        floats = self.lib.rails_mol_index_rows_floats(C.byref(self.shape), index.n_items)
        if floats == 0:
            raise NotImplementedError("the row-major index copy exists for exact-fp32 indexes only")
        rows = torch.empty(floats, dtype=torch.float32, device=index.buf.device)
        with _on_device(index.buf.device):
            _lib.check(self.lib.rails_mol_index_rows_build(C.byref(self.shape), _ptr(index.buf), index.n_items, _ptr(rows), _stream()), "rails_mol_index_rows_build")
        return rows

    # ---- in-place updates (MoLTopKModule.update_items / append_items): every method touches the updated positions' bytes only ----------------
    def update_index(self, index: MolIndex, positions: torch.Tensor, items: torch.Tensor) -> None:
        """items (M, D_i) -> slots positions (M,) int64 on the device, unique and inside [0, index.n_items) (the caller has checked), of `index`
        in its own format (rails_mol_index_update / rails_mol_generic_index_update): the bits build_index gives the updated table."""
        _require_device(items, "item_embeddings")
        if items.dim() != 2 or items.shape[1] != self.spec.item_embedding_dim or positions.shape != (items.shape[0],) or positions.dtype != torch.int64:
            raise ValueError(f"update_index takes (M, {self.spec.item_embedding_dim}) items and (M,) int64 positions, got {tuple(items.shape)} and {tuple(positions.shape)}")
        items, positions = _f32c(items), positions.contiguous()
        with _on_device(index.buf.device):
            _lib.check(self._fn("index_update")(C.byref(self.shape), C.byref(self.weights), _ptr(items), items.shape[0], _ptr(positions), _ptr(index.buf),
                                                index.n_items, _stream()), self._name("index_update"))

    def update_index_rows(self, index: MolIndex, rows: torch.Tensor, positions: torch.Tensor) -> None:
        """The row-major copy's rows at `positions`, from the updated index."""
        positions = positions.contiguous()
        with _on_device(index.buf.device):
            _lib.check(self.lib.rails_mol_index_rows_update(C.byref(self.shape), _ptr(index.buf), index.n_items, _ptr(positions), positions.numel(), _ptr(rows),
                                                            _stream()), "rails_mol_index_rows_update")

    def update_source(self, index: MolIndex, items: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """What the bf16 tables' updates are cut from -> (fp32-format index, read in place?): the (updated) index itself for fp32 engines; in
        f16x3 precision, whose index holds Ex to 22 bits, a temporary fp32-format index of the M updated rows alone (as _derived_table's chunks)."""
        self._tables_only("the coarse / component tables")
        if self.precision == "fp32":      # (the generic route is fp32 only: its tables are always cut from the index in place)
            return index.buf, 1
        items = _f32c(items)
        m = items.shape[0]
        tmp = torch.empty(self.lib.rails_mol_index_floats(C.byref(self._fp32_shape), m), dtype=torch.float32, device=items.device)
        with _on_device(items.device):
            _lib.check(self.lib.rails_mol_index_build(C.byref(self._fp32_shape), C.byref(self.weights), _ptr(items), m, _ptr(tmp), _stream()), "rails_mol_index_build")
        return tmp, 0

    def update_coarse_table(self, table: torch.Tensor, positions: torch.Tensor, source: Tuple[torch.Tensor, int]) -> None:
        """Rows `positions` of a build_coarse_table table from update_source's pair."""
        positions = positions.contiguous()
        with _on_device(table.device):
            if self.route == "generic":
                _lib.check(self.lib.rails_mol_generic_coarse_update(C.byref(self.shape), _ptr(source[0]), _ptr(positions), positions.numel(), _ptr(table),
                                                                    table.shape[0], _stream()), "rails_mol_generic_coarse_update")
                return
            _lib.check(self.lib.rails_mol_coarse_update(C.byref(self._fp32_shape), _ptr(source[0]), source[1], _ptr(positions), positions.numel(), _ptr(table),
                                                        table.shape[0], _stream()), "rails_mol_coarse_update")

    def update_component_table(self, table: torch.Tensor, positions: torch.Tensor, source: Tuple[torch.Tensor, int]) -> None:
        """Rows `positions` of every item group of a build_component_table table (P_X, N, d)."""
        positions = positions.contiguous()
        with _on_device(table.device):
            if self.route == "generic":
                _lib.check(self.lib.rails_mol_generic_component_update(C.byref(self.shape), _ptr(source[0]), _ptr(positions), positions.numel(), _ptr(table),
                                                                       table.shape[1], _stream()), "rails_mol_generic_component_update")
                return
            _lib.check(self.lib.rails_mol_component_update(C.byref(self._fp32_shape), _ptr(source[0]), source[1], _ptr(positions), positions.numel(), _ptr(table),
                                                           table.shape[1], _stream()), "rails_mol_component_update")

    def resize_index(self, index: MolIndex, n_items: int) -> None:
        """`index` resized to n_items items, IN PLACE (the same object: caches keyed on it stay valid): a buffer of index_floats(n_items) with the
        whole tiles copied and zeros beyond them (what the padding slots of a fresh index hold); cut, the slots past n_items of the new last
        tile are set to zero (rails_mol_index_clear_tail).  New slots are filled by update_index."""
        if n_items < 1:
            raise ValueError(f"resize_index: {n_items} items")
        shrinking = n_items < index.n_items
        buf = resized(index.buf, self._fn("index_floats")(C.byref(self.shape), n_items), zero=True)
        if shrinking:
            with _on_device(buf.device):
                _lib.check(self._fn("index_clear_tail")(C.byref(self.shape), _ptr(buf), n_items, _stream()), self._name("index_clear_tail"))
        index.buf, index.n_items = buf, n_items

    def score_indexed_rows(self, qpack: torch.Tensor, batch: int, rows: torch.Tensor, n_items: int, positions: torch.Tensor,
                           counts: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """score_indexed with the candidates read from the row-major copy: whole cache lines per candidate, same bits.
        counts: per-row candidate counts (int32 on the device; candidates_select's): only the first counts[b] logits of row b are written."""
        self._candidates_only("score_indexed_rows")
        if positions.dtype != torch.int64 or positions.device != rows.device or not positions.is_contiguous():
            positions = positions.to(device=rows.device, dtype=torch.int64).contiguous()
        n_cand = positions.shape[1]
        if out is None:
            out = torch.empty((batch, n_cand), dtype=torch.float32, device=rows.device)
        with _on_device(rows.device):
            if self.route == "generic":      # `rows` is the generic index itself: it is row-major already
                _lib.check(
                    self.lib.rails_mol_generic_score_indexed(C.byref(self.shape), _ptr(self.gate_pack), _ptr(qpack), batch, _ptr(rows), n_items, _ptr(positions),
                                                             n_cand, _ptr(counts), _ptr(out), out.stride(0), None, _stream()),
                    "rails_mol_generic_score_indexed",
                )
                return out
            _lib.check(
                self.lib.rails_mol_score_indexed_rows(C.byref(self.shape), _ptr(self.gate_pack), _ptr(qpack), batch, _ptr(rows), n_items, _ptr(positions), n_cand,
                                                      _ptr(out), out.stride(0), _ptr(counts), _stream()),
                "rails_mol_score_indexed_rows",
            )
        return out

    def gather_index(self, index: MolIndex, cand_idx: torch.Tensor) -> Tuple[MolIndex, int]:
        """cand_idx: (rows, K) int64 positions -> per-row tile-packed index, K padded to a multiple of 32."""
        self._fused_only("gather_index")
        _require_device(cand_idx, "candidate indices")
        rows, K = cand_idx.shape
        Kp = (K + TILE_ITEMS - 1) // TILE_ITEMS * TILE_ITEMS
        idx = cand_idx.to(torch.int64)
        if Kp != K:
            idx = torch.nn.functional.pad(idx, (0, Kp - K), value=-1)
        idx = idx.contiguous()
        floats = self.lib.rails_mol_index_floats(C.byref(self.shape), rows * Kp)
        out = torch.empty(floats, dtype=torch.float32, device=idx.device)
        with _on_device(idx.device):
            _lib.check(
                self.lib.rails_mol_index_gather(C.byref(self.shape), _ptr(index.buf), index.n_items, _ptr(idx), rows, Kp, _ptr(out), _stream()),
                "rails_mol_index_gather",
            )
        return MolIndex(out, rows * Kp), Kp

    # ---- query side ---------------------------------------------------------------------------
    def query_pack(self, q: torch.Tensor, user_ids: Optional[torch.Tensor] = None, want_plain: bool = False,
                   out: Optional[torch.Tensor] = None):
        _require_device(q, "query_embeddings")
        if q.dim() != 2 or q.shape[1] != self.spec.query_embedding_dim:
            raise ValueError(f"query_embeddings must be (B, {self.spec.query_embedding_dim}), got {tuple(q.shape)}")
        q = _f32c(q)
        B = q.shape[0]
        uid = None
        if len(self.spec.uid_embedding_hash_sizes) > 0:
            if user_ids is None:
                raise KeyError("user_ids")  # the reference does kwargs["user_ids"] (query_embeddings_fns.py:206)
            uid = user_ids.to(device=q.device, dtype=torch.int64).contiguous()
            if uid.numel() != B:
                # the reference fails in torch.cat on the same mismatch (query_embeddings_fns.py:206-216)
                raise RuntimeError(f"Sizes of tensors must match: user_ids has {tuple(uid.shape)} for a batch of {B} queries")
        n = self._fn("query_pack_floats")(C.byref(self.shape), B)
        pack = out if out is not None and out.numel() == n and out.device == q.device else torch.empty(n, dtype=torch.float32, device=q.device)
        s = self.spec
        eq = torch.empty((B, s.query_dot_product_groups, s.dot_product_dimension), dtype=torch.float32, device=q.device) if want_plain else None
        gq = torch.empty((B, s.num_logits), dtype=torch.float32, device=q.device) if want_plain else None
        with _on_device(q.device):
            _lib.check(
                self._fn("query_prologue")(C.byref(self.shape), C.byref(self.weights), _ptr(q), _ptr(uid), B, _ptr(pack), _ptr(eq), _ptr(gq), _stream()),
                self._name("query_prologue"),
            )
        return pack, eq, gq

    def query_pack_both(self, q: torch.Tensor, user_ids: Optional[torch.Tensor], out: torch.Tensor, out_other: torch.Tensor):
        """One prologue, two packs: `out` in this engine's format, `out_other` in the other one (for the fp32 companion of a
        verified fast mode).  Both must hold rails_mol_query_pack_floats floats."""
        self._fused_only("query_pack_both")
        _require_device(q, "query_embeddings")
        if q.dim() != 2 or q.shape[1] != self.spec.query_embedding_dim:
            raise ValueError(f"query_embeddings must be (B, {self.spec.query_embedding_dim}), got {tuple(q.shape)}")
        q = _f32c(q)
        B = q.shape[0]
        uid = None
        if len(self.spec.uid_embedding_hash_sizes) > 0:
            if user_ids is None:
                raise KeyError("user_ids")
            uid = user_ids.to(device=q.device, dtype=torch.int64).contiguous()
            if uid.numel() != B:
                raise RuntimeError(f"Sizes of tensors must match: user_ids has {tuple(uid.shape)} for a batch of {B} queries")
        n = self.lib.rails_mol_query_pack_floats(C.byref(self.shape), B)
        if out.numel() != n or out_other.numel() != n:
            raise ValueError(f"query packs must hold {n} floats")
        with _on_device(q.device):
            _lib.check(self.lib.rails_mol_query_prologue_both(C.byref(self.shape), C.byref(self.weights), _ptr(q), _ptr(uid), B, _ptr(out),
                                                              _ptr(out_other), _stream()), "rails_mol_query_prologue_both")
        return out, out_other

    def gate_rows(self, qpack: torch.Tensor, batch: int) -> torch.Tensor:
        """The batch's gq' rows (batch * num_logits floats) inside an fp32 query pack: they sit behind the Eq fragments, which take
        32 * d floats per block of 32 / P_Q queries (the verdict kernels check the bound's gate guard on them)."""
        self._fused_only("gate_rows")
        s = self.spec
        off = (batch + 32 // s.query_dot_product_groups - 1) // (32 // s.query_dot_product_groups) * 32 * s.dot_product_dimension
        return qpack[off : off + batch * s.num_logits]

    # ---- scoring ------------------------------------------------------------------------------
    def score_dense(self, qpack: torch.Tensor, batch: int, index: MolIndex, out: Optional[torch.Tensor] = None,
                    run_if: Optional[torch.Tensor] = None) -> torch.Tensor:
        """run_if: launch predicate (an int32 device scalar; see _pred): the launch is a no-op unless it is non-zero on the device."""
        if out is None:
            out = torch.empty((batch, index.n_items), dtype=torch.float32, device=index.buf.device)
        with _on_device(index.buf.device):
            _lib.check(
                self._fn("score_dense")(C.byref(self.dense_shape), _ptr(self.gate_pack), _ptr(qpack), batch, _ptr(index.buf), index.n_items, _ptr(out), out.stride(0), _pred(run_if), _stream()),
                self._name("score_dense"),
            )
        return out

    def score_dense_upper_supported(self) -> bool:
        """True iff this engine's dense precision has the upper-bound first pass (include/rails_amd.h rails_mol_score_dense_upper)."""
        if self.route == "generic":
            return False
        memo = self.__dict__
        if "_upper_ok" not in memo:
            memo["_upper_ok"] = bool(self.lib.rails_mol_score_dense_upper_supported(C.byref(self.dense_shape)))
        return memo["_upper_ok"]

    def score_dense_upper(self, qpack: torch.Tensor, batch: int, index: MolIndex, poly: Tuple[float, float, float], out: Optional[torch.Tensor] = None,
                          run_if: Optional[torch.Tensor] = None) -> torch.Tensor:
        """f16x3 logit + (ub2 c + ub1) c + ub0 per pair, c = the pair's largest |cross logit|: an upper bound of the fp32 logit when `poly` is
        f16x3_bound.upper_bound_poly's (ub2, ub1, ub0)."""
        self._fused_only("the upper-bound first pass")
        if out is None:
            out = torch.empty((batch, index.n_items), dtype=torch.float32, device=index.buf.device)
        with _on_device(index.buf.device):
            _lib.check(
                self.lib.rails_mol_score_dense_upper(C.byref(self.dense_shape), _ptr(self.gate_pack), _ptr(qpack), batch, _ptr(index.buf), index.n_items,
                                                     float(poly[0]), float(poly[1]), float(poly[2]), _ptr(out), out.stride(0), _pred(run_if), _stream()),
                "rails_mol_score_dense_upper",
            )
        return out

    def score_indexed_supported(self, batch: int, n_cand: int) -> bool:
        if self.route == "generic":
            return self.candidates      # (the indexed mode of the generic kernel takes any batch and any n_cand >= 1)
        key = (int(batch), int(n_cand))
        memo = self.__dict__.setdefault("_indexed_ok", {})     # a dry run of the launch per call otherwise: host time of every rerank
        if key not in memo:
            memo[key] = bool(self.lib.rails_mol_score_indexed_supported(C.byref(self.shape), key[0], key[1]))
        return memo[key]

    def score_indexed(self, qpack: torch.Tensor, batch: int, index: MolIndex, positions: torch.Tensor) -> torch.Tensor:
        """(B, n_cand) logits of per-row candidates given as positions of `index` (all inside the index):
        gather_index + score_candidates without the gathered copy (include/rails_amd.h rails_mol_score_indexed)."""
        self._candidates_only("score_indexed")
        if self.route == "generic":
            return self.score_indexed_rows(qpack, batch, index.buf, index.n_items, positions)
        positions = positions.to(device=index.buf.device, dtype=torch.int64).contiguous()
        n_cand = positions.shape[1]
        out = torch.empty((batch, n_cand), dtype=torch.float32, device=index.buf.device)
        with _on_device(index.buf.device):
            _lib.check(
                self.lib.rails_mol_score_indexed(C.byref(self.shape), _ptr(self.gate_pack), _ptr(qpack), batch, _ptr(index.buf), index.n_items, _ptr(positions), n_cand,
                                                 _ptr(out), out.stride(0), _stream()),
                "rails_mol_score_indexed",
            )
        return out

    # ---- pair-level scoring on the generic route (score_of / explain_of) ----------------------------------------------
    def _generic_only(self, what: str) -> None:
        if self.route != "generic":
            raise NotImplementedError(f"{what} is built on the generic scoring route only (MolEngine(..., route='generic'))")

    def score_at_generic(self, qpack: torch.Tensor, batch: int, index: MolIndex, positions: torch.Tensor) -> torch.Tensor:
        """(B, T) logits of per-row positions of a generic index, read in place -- the indexed launch whether or not the engine is
        candidate-capable (the index is row-major on this route; rails_mol_generic_score_indexed clamps the positions into it)."""
        self._generic_only("score_at_generic")
        positions = positions.to(device=index.buf.device, dtype=torch.int64).contiguous()
        t = positions.shape[1]
        out = torch.empty((batch, t), dtype=torch.float32, device=index.buf.device)
        with _on_device(index.buf.device):
            _lib.check(self.lib.rails_mol_generic_score_indexed(C.byref(self.shape), _ptr(self.gate_pack), _ptr(qpack), batch, _ptr(index.buf), index.n_items,
                                                                _ptr(positions), t, None, _ptr(out), out.stride(0), None, _stream()),
                       "rails_mol_generic_score_indexed")
        return out

    def explain_indexed(self, qpack: torch.Tensor, batch: int, index: MolIndex, positions: torch.Tensor):
        """score_at_generic's launch in its explaining instantiation -> (logits (B, T), component_logits (B, T, L), weights (B, T, L)): the
        logits carry score_at_generic's bits (include/rails_amd.h rails_mol_generic_explain_indexed)."""
        self._generic_only("explain_indexed")
        dev = index.buf.device
        positions = positions.to(device=dev, dtype=torch.int64).contiguous()
        t, L = positions.shape[1], self.spec.num_logits
        out = torch.empty((batch, t), dtype=torch.float32, device=dev)
        cl = torch.empty((batch, t, L), dtype=torch.float32, device=dev)
        pi = torch.empty((batch, t, L), dtype=torch.float32, device=dev)
        with _on_device(dev):
            _lib.check(self.lib.rails_mol_generic_explain_indexed(C.byref(self.shape), _ptr(self.gate_pack), _ptr(qpack), batch, _ptr(index.buf), index.n_items,
                                                                  _ptr(positions), t, _ptr(out), out.stride(0), _ptr(cl), _ptr(pi), _stream()),
                       "rails_mol_generic_explain_indexed")
        return out, cl, pi

    def explain_candidates(self, qpack: torch.Tensor, batch: int, cand_index: MolIndex, n_cand: int):
        """explain_indexed for per-row candidates held in a generic index of their own (candidate j of row b is its item b * n_cand + j)."""
        self._generic_only("explain_candidates")
        dev = cand_index.buf.device
        L = self.spec.num_logits
        out = torch.empty((batch, n_cand), dtype=torch.float32, device=dev)
        cl = torch.empty((batch, n_cand, L), dtype=torch.float32, device=dev)
        pi = torch.empty((batch, n_cand, L), dtype=torch.float32, device=dev)
        with _on_device(dev):
            _lib.check(self.lib.rails_mol_generic_explain(C.byref(self.shape), _ptr(self.gate_pack), _ptr(qpack), batch, _ptr(cand_index.buf), n_cand,
                                                          _ptr(out), out.stride(0), _ptr(cl), _ptr(pi), _stream()), "rails_mol_generic_explain")
        return out, cl, pi

    # ---- the backward of score_candidates on the generic route (the differentiable MoLSimilarity.forward) -------------
    GRAD_CHUNK_PAIRS = 16384     # pairs per chunk of the weight-gradient workspace (whole rows; a multiple of 256)

    def pair_backward_supported(self) -> bool:
        """True iff rails_mol_generic_pair_backward takes this engine's shape (the message is in _lib.last_error() otherwise)."""
        return self.route == "generic" and bool(self.lib.rails_mol_generic_pair_backward_supported(C.byref(self.shape)))

    def pair_backward(self, qpack: torch.Tensor, batch: int, cand_index: MolIndex, n_cand: int, dY: torch.Tensor,
                      need: Tuple[bool, bool, bool] = (True, True, True), chunk_pairs: Optional[int] = None):
        """Gradients of sum(dY * score_candidates(qpack, batch, cand_index, n_cand)) -> (d_qpack, d_ipack, (dW1, db1, dW2, db2)):
        d_qpack (batch, query_floats) holds dEq (of the unscaled Eq) and dgq in the query pack's layout, d_ipack (batch * n_cand, item_floats)
        dEx and dgi in the item layout, the last four the pair gate's weight gradients.  need = (query side, item side, weights): an entry
        that is False comes back None and its work is skipped.  dY is (batch, n_cand) fp32 with any row stride.  The weight gradients are
        summed through a workspace of `chunk_pairs` pairs (GRAD_CHUNK_PAIRS by default), whatever batch * n_cand is; a row of more
        candidates than that is refused when they are asked for."""
        self._generic_only("pair_backward")
        if not self.pair_backward_supported():
            raise NotImplementedError(_lib.last_error())
        dev = cand_index.buf.device
        if dY.shape != (batch, n_cand) or dY.dtype != torch.float32 or dY.device != dev or (n_cand > 1 and dY.stride(1) != 1):
            raise ValueError(f"dY must be ({batch}, {n_cand}) fp32 on {dev} with unit column stride, got {tuple(dY.shape)} {dY.dtype} strides {dY.stride()}")
        ld = dY.stride(0) if batch > 1 else n_cand
        if ld < n_cand:
            dY, ld = dY.contiguous(), n_cand
        if "gate_pack_t" not in self.__dict__:
            self.gate_pack_t = torch.empty(self.lib.rails_mol_generic_gate_pack_t_floats(C.byref(self.shape)), dtype=torch.float32, device=self.device)
            with _on_device(self.device):
                _lib.check(self.lib.rails_mol_generic_pack_gate_weights_t(C.byref(self.shape), C.byref(self.weights), _ptr(self.gate_pack_t), _stream()),
                           "rails_mol_generic_pack_gate_weights_t")
        s = self.spec
        qf = self.lib.rails_mol_generic_query_pack_floats(C.byref(self.shape), 1)
        itf = self.lib.rails_mol_generic_index_floats(C.byref(self.shape), 32) // 32
        dq = (torch.zeros if n_cand == 0 else torch.empty)((batch, qf), dtype=torch.float32, device=dev) if need[0] else None      # (no candidates: the launch is skipped)
        di = torch.empty((batch * n_cand, itf), dtype=torch.float32, device=dev) if need[1] else None
        dw = ws = None
        ws_bytes = 0
        chunk = int(chunk_pairs or self.GRAD_CHUNK_PAIRS)
        if need[2]:
            L, H = s.num_logits, s.gating_qi_hidden_dim
            dw = (torch.zeros((H, L), dtype=torch.float32, device=dev), torch.zeros(H, dtype=torch.float32, device=dev),
                  torch.zeros((L, H), dtype=torch.float32, device=dev), torch.zeros(L, dtype=torch.float32, device=dev))
            if (n_cand + 31) // 32 * 32 > (chunk + 255) // 256 * 256:      # a row is never split, and the workspace does not grow with it
                raise NotImplementedError(f"pair_backward: the pair gate's weight gradients take rows of at most chunk_pairs = {chunk} candidates, got {n_cand}")
            ws_bytes = self.lib.rails_mol_generic_pair_backward_workspace_bytes(C.byref(self.shape), chunk)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with _on_device(dev):
            _lib.check(self.lib.rails_mol_generic_pair_backward(
                C.byref(self.shape), _ptr(self.gate_pack), _ptr(self.gate_pack_t), _ptr(qpack), batch, _ptr(cand_index.buf), n_cand, _ptr(dY), ld,
                _ptr(dq), _ptr(di), _ptr(dw[0]) if dw else None, _ptr(dw[1]) if dw else None, _ptr(dw[2]) if dw else None,
                _ptr(dw[3]) if dw else None, _ptr(ws), ws_bytes, chunk, _stream()), "rails_mol_generic_pair_backward")
        return dq, di, dw

    def score_candidates(self, qpack: torch.Tensor, batch: int, cand_index: MolIndex, n_cand_padded: int) -> torch.Tensor:
        out = torch.empty((batch, n_cand_padded), dtype=torch.float32, device=cand_index.buf.device)
        with _on_device(cand_index.buf.device):
            if self.route == "generic":
                _lib.check(self.lib.rails_mol_generic_score_candidates(C.byref(self.shape), _ptr(self.gate_pack), _ptr(qpack), batch, _ptr(cand_index.buf),
                                                                       n_cand_padded, _ptr(out), out.stride(0), None, _stream()),
                           "rails_mol_generic_score_candidates")
                return out
            _lib.check(
                self.lib.rails_mol_score_candidates(C.byref(self.shape), _ptr(self.gate_pack), _ptr(qpack), batch, _ptr(cand_index.buf), n_cand_padded, _ptr(out), out.stride(0), _stream()),
                "rails_mol_score_candidates",
            )
        return out


    # ---- coarse pass of the two-pass approximate top-k ------------------------------------------------
    def _derived_table(self, fn_name: str, row_elems: int, index: MolIndex, items: Optional[torch.Tensor]) -> torch.Tensor:
        """A bf16 table cut from the fp32 Ex of the index.  In f16x3 precision the index only holds Ex to 22 bits, so the
        table is cut from temporary fp32-format index chunks rebuilt from `items` (same values as the fp32 engine's)."""
        self._tables_only("the coarse / component tables")
        n, dev = index.n_items, index.buf.device
        table = torch.empty(n * row_elems, dtype=torch.bfloat16, device=dev)
        grouped = fn_name == "rails_mol_component_build"      # item-group-major table: a chunk of items writes a slice of every group
        if self.route == "generic":      # the generic index is fp32 and row-major: one launch, rows of table_width columns (row_elems counts them)
            fn_name = fn_name.replace("rails_mol_", "rails_mol_generic_")
            with _on_device(dev):
                _lib.check(getattr(self.lib, fn_name)(C.byref(self.shape), _ptr(index.buf), n, _ptr(table), _stream()), fn_name)
            return table
        fn = getattr(self.lib, fn_name)
        with _on_device(dev):
            if self.precision == "fp32":
                if grouped:
                    _lib.check(fn(C.byref(self.shape), _ptr(index.buf), n, _ptr(table), n, 0, _stream()), fn_name)
                else:
                    _lib.check(fn(C.byref(self.shape), _ptr(index.buf), n, _ptr(table), _stream()), fn_name)
            else:
                if items is None:
                    raise ValueError(f"{fn_name}: precision='f16x3' needs the raw item embeddings to cut the bf16 table from")
                items = _f32c(items)
                chunk = 1 << 20   # a multiple of the 32-item tile
                tmp = torch.empty(self.lib.rails_mol_index_floats(C.byref(self._fp32_shape), min(chunk, n)), dtype=torch.float32, device=dev)
                for lo in range(0, n, chunk):
                    m = min(chunk, n - lo)
                    _lib.check(self.lib.rails_mol_index_build(C.byref(self._fp32_shape), C.byref(self.weights), _ptr(items[lo : lo + m]), m, _ptr(tmp), _stream()),
                               "rails_mol_index_build")
                    if grouped:
                        _lib.check(fn(C.byref(self._fp32_shape), _ptr(tmp), m, _ptr(table), n, lo, _stream()), fn_name)
                    else:
                        _lib.check(fn(C.byref(self._fp32_shape), _ptr(tmp), m, C.c_void_p(table.data_ptr() + 2 * lo * row_elems), _stream()), fn_name)
        return table

    def build_coarse_table(self, index: MolIndex, items: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(N, d) bf16 table of P_X-averaged component embeddings (reference mol_top_k.py:321-325); on a candidate-capable generic engine
        (N, table_width), the columns d .. table_width zeros."""
        d = self.table_width
        return self._derived_table("rails_mol_coarse_build", d, index, items).view(index.n_items, d)

    def coarse_scores(self, eq: torch.Tensor, table: torch.Tensor, average_queries: bool, out: Optional[torch.Tensor] = None,
                      run_if: Optional[torch.Tensor] = None) -> torch.Tensor:
        """eq (B, P_Q, d) fp32 -> (B, N) fp32 holding bf16-rounded dot products (reference mol_top_k.py:351-354)."""
        B, n = eq.shape[0], table.shape[0]
        eq = self._scan_eq(eq)
        if out is None:
            out = torch.empty((B, n), dtype=torch.float32, device=table.device)
        with _on_device(table.device):
            _lib.check(
                self.lib.rails_mol_coarse_score(C.byref(self.scan_shape), _ptr(eq), B, 1 if average_queries else 0, _ptr(table), n, _ptr(out), out.stride(0), _pred(run_if), _stream()),
                "rails_mol_coarse_score",
            )
        return out

    def build_coarse_prefilter(self, table: torch.Tensor) -> Optional[torch.Tensor]:
        """The int8 copy of a coarse table that lets coarse_topk's streaming pass read d instead of 2d bytes per item
        (include/rails_amd.h rails_mol_coarse_prefilter_build); None for shapes without one."""
        if self.route == "generic":      # not built for the padded widths of the generic route
            return None
        n = table.shape[0]
        nbytes = self.lib.rails_mol_coarse_prefilter_bytes(C.byref(self.scan_shape), n)
        if nbytes == 0:
            return None
        pre = torch.empty(nbytes, dtype=torch.uint8, device=table.device)
        with _on_device(table.device):
            _lib.check(self.lib.rails_mol_coarse_prefilter_build(C.byref(self.scan_shape), _ptr(table), n, _ptr(pre), _stream()), "rails_mol_coarse_prefilter_build")
        return pre

    def coarse_topk(self, eq: torch.Tensor, table: torch.Tensor, average_queries: bool, k_prime: int, with_flag: bool = False,
                    prefilter: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None, visible: Optional[torch.Tensor] = None,
                    tags: Optional["TagFilter"] = None):
        """Fused coarse scoring + exact top-K' (no (B, N) score matrix).  -> (scores (B, K'), positions (B, K'), counts (B,)
        int32) or None when the sizes are unsupported.  The result is exact iff K' <= counts[b] <= capacity for every b
        (see include/rails_amd.h); the caller checks and falls back to coarse_scores + topk otherwise.  with_flag: a fourth
        element, a device int32 that is 1 iff some count is out of range (written by the call's own launches) -- or `flag`, the caller's own
        int32 word (device or PINNED HOST memory: the kernels store through the device-visible address, no copy is needed to read it).
        prefilter: build_coarse_prefilter(table) -- same outputs, the streaming pass reads the int8 copy.
        visible: the visibility words of a hidden set (one ItemMask row over the n items, bit set = visible): the top-K' of the visible items
        alone, through the scans' visible kernels (rails_mol_coarse_topk_visible); None: rails_mol_coarse_topk, launch for launch.
        tags: a TagFilter (allowed_tags= resolved): row b's top-K' of the items it may return, through the scans' tagged
        kernels (rails_mol_coarse_topk_tagged); its effective tags hold the hidden set, so `visible` is not passed with it."""
        B, n = eq.shape[0], table.shape[0]
        _check_visible_words(visible, n, table.device)
        _check_tag_filter(tags, n, B, table.device, visible)
        memo = self.__dict__.setdefault("_coarse_ws_bytes", {})
        if (B, n, k_prime) not in memo:
            memo[(B, n, k_prime)] = self.lib.rails_mol_coarse_topk_workspace_bytes(C.byref(self.scan_shape), B, n, k_prime)
        ws_bytes = memo[(B, n, k_prime)]
        if ws_bytes == 0:
            return None
        eq = self._scan_eq(eq)
        dev = table.device
        if prefilter is not None:
            # the C side indexes the int8 copy by this call's n and d, and the exactness argument assumes copy and scale belong to THIS
            # table: a buffer of another size or device (a stale copy of a rebuilt table) is refused
            want = memo.get(("prefilter", n))
            if want is None:
                want = memo[("prefilter", n)] = self.lib.rails_mol_coarse_prefilter_bytes(C.byref(self.scan_shape), n)
            if prefilter.device != dev or prefilter.dtype != torch.uint8 or prefilter.numel() != want or not prefilter.is_contiguous():
                raise ValueError(f"coarse_topk: the int8 pre-filter does not belong to this table ({prefilter.numel()} bytes on {prefilter.device}, "
                                 f"expected {want} on {dev}): rebuild it with build_coarse_prefilter(table)")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out_s = torch.empty((B, k_prime), dtype=torch.float32, device=dev)
        out_p = torch.empty((B, k_prime), dtype=torch.int64, device=dev)
        counts = torch.empty((B + 1,), dtype=torch.int32, device=dev)   # [B]: the out-of-range flag
        if flag is None:
            flag = counts[B:]
        elif flag.dtype != torch.int32 or flag.numel() != 1 or not (flag.is_cuda or flag.is_pinned()):
            raise ValueError("coarse_topk: flag must be one int32 on the device or in pinned host memory")
        else:
            with_flag = True
        with _on_device(dev):
            if tags is not None:
                _lib.check(
                    self.lib.rails_mol_coarse_topk_tagged(C.byref(self.scan_shape), _ptr(eq), B, 1 if average_queries else 0, _ptr(table), n, k_prime,
                                                          _ptr(ws), ws_bytes, _ptr(out_s), _ptr(out_p), _ptr(counts), _ptr(flag) if with_flag else None,
                                                          _ptr(prefilter), _ptr(tags.eff), _ptr(tags.allowed_for(B)), _stream()),
                    "rails_mol_coarse_topk_tagged",
                )
            elif visible is None:
                _lib.check(
                    self.lib.rails_mol_coarse_topk(C.byref(self.scan_shape), _ptr(eq), B, 1 if average_queries else 0, _ptr(table), n, k_prime,
                                                   _ptr(ws), ws_bytes, _ptr(out_s), _ptr(out_p), _ptr(counts), _ptr(flag) if with_flag else None, _ptr(prefilter), _stream()),
                    "rails_mol_coarse_topk",
                )
            else:
                _lib.check(
                    self.lib.rails_mol_coarse_topk_visible(C.byref(self.scan_shape), _ptr(eq), B, 1 if average_queries else 0, _ptr(table), n, k_prime,
                                                           _ptr(ws), ws_bytes, _ptr(out_s), _ptr(out_p), _ptr(counts), _ptr(flag) if with_flag else None,
                                                           _ptr(prefilter), _ptr(visible), _stream()),
                    "rails_mol_coarse_topk_visible",
                )
        return (out_s, out_p, counts[:B], flag) if with_flag else (out_s, out_p, counts[:B])

    @staticmethod
    def coarse_topk_capacity(k_prime: int, n_items: Optional[int] = None, batch: int = 32) -> int:
        """candidates per query the fused coarse top-K' can hold (include/rails_amd.h rails_mol_coarse_topk_capacity); without n_items: the
        figure of shard-sized corpora"""
        if n_items is not None:
            return int(_lib.load().rails_mol_coarse_topk_capacity(int(batch), int(n_items), int(k_prime)))
        cap = min(24576, max(4096, 8 * k_prime))
        return (cap + 63) // 64 * 64

    # ---- per-component candidates (MoLNaiveTopK / MoLCombTopK) -----------------------------------------
    def build_component_table(self, index: MolIndex, items: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(P_X, N, d) bf16 component embeddings (reference mol_top_k.py:61-73), item-group-major: the scans stream one group's rows back to back."""
        px, d = self.spec.item_dot_product_groups, self.table_width      # (the padded width on a candidate-capable generic engine, as the coarse table)
        return self._derived_table("rails_mol_component_build", px * d, index, items).view(px, index.n_items, d)

    def component_scores(self, eq: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None,
                         run_if: Optional[torch.Tensor] = None) -> torch.Tensor:
        """eq (B, P_Q, d) -> (B * P_Q * P_X, N) fp32 holding bf16 values, row (b * P_Q + i) * P_X + m."""
        B, n = eq.shape[0], table.shape[1]
        eq = self._scan_eq(eq)
        rows = B * self.spec.query_dot_product_groups * self.spec.item_dot_product_groups
        if out is None:
            out = torch.empty((rows, n), dtype=torch.float32, device=table.device)
        with _on_device(table.device):
            _lib.check(
                self.lib.rails_mol_component_score(C.byref(self.scan_shape), _ptr(eq), B, _ptr(table), n, _ptr(out), out.stride(0), _pred(run_if), _stream()),
                "rails_mol_component_score",
            )
        return out

    def component_topk(self, eq: torch.Tensor, table: torch.Tensor, k_group: int, flag: Optional[torch.Tensor] = None,
                       visible: Optional[torch.Tensor] = None, tags: Optional["TagFilter"] = None):
        """Fused component scoring + exact top-k_group per (b, i, m) row (no (rows, N) score matrix).
        -> (scores (rows, k_group), positions (rows, k_group), counts (rows,) int32) or None when unsupported; exact iff
        k_group <= counts <= component_topk_capacity for every row -- `flag` (an int32 device scalar, zeroed by the call) is raised otherwise.
        visible: as for coarse_topk (rails_mol_component_topk_visible), shared by every row.
        tags: as for coarse_topk (rails_mol_component_topk_tagged), the P_Q * P_X rows of a query share its allow word; at most
        TAGGED_COMPONENT_ROWS query rows (B * P_Q) per call -- None beyond, as for any unsupported size."""
        B, n = eq.shape[0], table.shape[1]
        _check_visible_words(visible, n, table.device)
        _check_tag_filter(tags, n, B, table.device, visible)
        if tags is not None and B * self.spec.query_dot_product_groups > TAGGED_COMPONENT_ROWS:
            return None
        ws_bytes = self.lib.rails_mol_component_topk_workspace_bytes(C.byref(self.scan_shape), B, n, k_group)
        if ws_bytes == 0:
            return None
        eq = self._scan_eq(eq)
        dev = table.device
        rows = B * self.spec.query_dot_product_groups * self.spec.item_dot_product_groups
        memo = self.__dict__.setdefault("_comp_ws", {})          # the workspace is recycled: 30-70 MB of candidate lists per call otherwise
        ws = memo.get(ws_bytes)
        if ws is None or ws.device != dev:
            memo.clear()
            ws = memo[ws_bytes] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out_s = torch.empty((rows, k_group), dtype=torch.float32, device=dev)
        out_p = torch.empty((rows, k_group), dtype=torch.int64, device=dev)
        counts = torch.empty((rows,), dtype=torch.int32, device=dev)
        with _on_device(dev):
            if tags is not None:
                _lib.check(
                    self.lib.rails_mol_component_topk_tagged(C.byref(self.scan_shape), _ptr(eq), B, _ptr(table), n, k_group, _ptr(ws), ws_bytes,
                                                             _ptr(out_s), _ptr(out_p), _ptr(counts), _ptr(flag), _ptr(tags.eff), _ptr(tags.allowed_for(B)),
                                                             _stream()),
                    "rails_mol_component_topk_tagged",
                )
            elif visible is None:
                _lib.check(
                    self.lib.rails_mol_component_topk(C.byref(self.scan_shape), _ptr(eq), B, _ptr(table), n, k_group, _ptr(ws), ws_bytes,
                                                      _ptr(out_s), _ptr(out_p), _ptr(counts), _ptr(flag), _stream()),
                    "rails_mol_component_topk",
                )
            else:
                _lib.check(
                    self.lib.rails_mol_component_topk_visible(C.byref(self.scan_shape), _ptr(eq), B, _ptr(table), n, k_group, _ptr(ws), ws_bytes,
                                                              _ptr(out_s), _ptr(out_p), _ptr(counts), _ptr(flag), _ptr(visible), _stream()),
                    "rails_mol_component_topk_visible",
                )
        return out_s, out_p, counts

    def component_topk_capacity(self, batch: int, n: int, k_group: int) -> int:
        return int(self.lib.rails_mol_component_topk_capacity(C.byref(self.scan_shape), int(batch), int(n), int(k_group)))


def ivf_edited_size(n_old: int, n_keep: int, positions=None, *, m: Optional[int] = None, below: Optional[int] = None) -> int:
    """Entries per group after IvfIndex.edit (include/rails_amd.h rails_ivf_lists_edit): the old lists hold each of 0 .. n_old - 1 once, so
    n_new = min(n_old, n_keep) - #{p in positions : p < min(n_old, n_keep)} + m.  Either `positions` (unique ints: a host tensor, an array
    or a list) or, where they live on the device, their number `m` and the count `below` of those under min(n_old, n_keep)."""
    lim = min(int(n_old), int(n_keep))
    if positions is not None:
        pos = [int(p) for p in (positions.tolist() if hasattr(positions, "tolist") else positions)]
        m, below = len(pos), sum(1 for p in pos if p < lim)
    if m is None or below is None or not 0 <= below <= min(m, lim):
        raise ValueError("ivf_edited_size: give positions, or m and 0 <= below <= min(m, min(n_old, n_keep))")
    return lim - int(below) + int(m)


class IvfFilterPlan:
    """What IvfIndex keeps per filter while the lists and the filter stay what they are: the eligible entries per (row, group, list) on the device
    (`counts`, (count_rows, P_X, nlist) int32 -- rails_ivf_list_counts), their ONE read-back (`counts_host`), the items each row keeps (`kept`,
    host integers) and the probe capacity per (nprobe, k_per_group) (rails_ivf_plan_filtered).  `key` is the filter itself: the TagFilter, or the
    visibility row of a hidden-only call."""

    def __init__(self, key, allowed: torch.Tensor, counts: torch.Tensor):
        self.key, self.allowed, self.counts = key, allowed, counts
        self.count_rows = counts.shape[0]
        self.counts_host = counts.cpu().contiguous()
        self.kept = tuple(int(v) for v in self.counts_host[:, 0, :].sum(dim=1))       # (every group's lists hold every item once)
        self.max_probes: Dict[Tuple[int, int], int] = {}


class IvfIndex:
    """IVF-Flat index over the item components (include/rails_amd.h rails_ivf_*): one index per item group, trained by spherical Lloyd
    k-means on a seeded sample of the fp16-rounded components and searched in three launches -- the native counterpart of the FAISS
    branch of MoLNaiveTopK (reference rails/indexing/mol_top_k.py:176-239).  Where the probed lists hold fewer than k_per_group items the
    search goes on into further lists in centroid-score order (FAISS returns -1 there).  edit() makes the lists follow an in-place change
    of the corpus under FROZEN centroids (FAISS IndexIVFFlat.add / remove_ids): the centroids are never written again."""

    COMPONENT_CHUNK = 1 << 20     # items per temporary fp32-format index chunk where the engine's own index is in a split-f16 format
    EDIT_MAX = 16384              # inserted entries one rails_ivf_lists_edit call takes (one rails_sort_rows_i64 row); beyond: edit() rebuilds the lists
    FILTER_WS_CAP = 256 << 20     # bytes of search workspace a filtered call stays under by slicing its batch (the part buffers grow with max_probes)
    FILTER_PLANS_KEPT = 64        # filters whose counts and plans are kept (a per-row filter's counts hold B * P_X * nlist int32)

    def __init__(self, engine: MolEngine, index: MolIndex, nlist: int = 100, nprobe: int = 1, iters: int = 10, seed: int = 1234,
                 items: Optional[torch.Tensor] = None, centroids: Optional[torch.Tensor] = None):
        """items: the raw (N, D) item embeddings; needed only where `engine` is not an fp32 engine: the fp16 components are then cut from
        temporary fp32-format index chunks of COMPONENT_CHUNK items (the same values as the fp32 engine's), as the component table is.
        centroids: a (P_X, nlist, d) fp32 tensor on the index's device -- the lists are built from a COPY of it and nothing is trained (no
        sample, no Lloyd iterations); ValueError for another shape, dtype or device."""
        engine._fused_only("the IVF-Flat index")
        self.lib = engine.lib
        self._engine, self._index = engine, index
        spec = engine.spec
        self.groups, self.d = spec.item_dot_product_groups, spec.dot_product_dimension
        self.query_groups = spec.query_dot_product_groups
        self.n_items, self.nlist = index.n_items, int(nlist)
        if self.nlist < 1 or self.nlist > 4096:
            raise NotImplementedError(f"IvfIndex: nlist = {self.nlist} outside [1, 4096]")
        self._nprobe = int(nprobe)
        self._check_nprobe(self._nprobe)
        shape = self._shape = engine._fp32_shape
        n, dev = self.n_items, index.buf.device
        if n < self.nlist:
            raise ValueError(f"IvfIndex: {n} items cannot fill nlist = {self.nlist} lists")
        G, d = self.groups, self.d
        if centroids is not None:
            if (not torch.is_tensor(centroids) or tuple(centroids.shape) != (G, self.nlist, d) or centroids.dtype != torch.float32
                    or centroids.device != dev):
                raise ValueError(f"IvfIndex: centroids must be a ({G}, {self.nlist}, {d}) float32 tensor on {dev}")
        if engine.precision != "fp32" and items is None:
            raise ValueError("IvfIndex: a non-fp32 engine needs the raw item embeddings to cut the fp32 components from")
        src_index, comp16 = self._source(items)
        self._vectors = torch.empty((G, n, d), dtype=torch.float16, device=dev)
        self._positions = torch.empty((G, n), dtype=torch.int32, device=dev)
        self._offsets = torch.empty((G, self.nlist + 1), dtype=torch.int32, device=dev)
        if centroids is not None:
            self._centroids = centroids.detach().clone(memory_format=torch.contiguous_format)
            self._build_lists(src_index, comp16)
        else:
            # the sample: a seeded permutation of the items, its first min(N, 256 nlist); the first nlist of it start the centroids
            gen = torch.Generator().manual_seed(int(seed))
            n_sample = min(n, 256 * self.nlist)
            sample = torch.randperm(n, generator=gen)[:n_sample].to(torch.int32).to(dev)
            self._centroids = torch.empty((G, self.nlist, d), dtype=torch.float32, device=dev)
            ws = torch.empty(max(self.lib.rails_ivf_build_workspace_bytes(C.byref(shape), n, self.nlist, n_sample), 1), dtype=torch.uint8, device=dev)
            with _on_device(dev):
                _lib.check(self.lib.rails_ivf_train(C.byref(shape), _ptr(src_index), _ptr(comp16), n, _ptr(sample), n_sample, self.nlist, int(iters), 1,
                                                    _ptr(self._centroids), _ptr(ws), ws.numel(), _stream()), "rails_ivf_train")
            self._build_lists(src_index, comp16, ws)
            del ws
        del comp16
        self._offsets_host = self._offsets.cpu().contiguous()
        self._plans: Dict[Tuple[int, int], Tuple[int, int]] = {}
        self._ws: Optional[torch.Tensor] = None
        self._unfilled = torch.zeros(1, dtype=torch.int32, device=dev)
        # filtered lists: nothing is allocated until a search is given a filter
        self._list_words: Optional[Tuple[torch.Tensor, torch.Tensor]] = None       # (the filter's source array, the words in list order)
        self._filter_plans: Dict[int, IvfFilterPlan] = {}
        self._all_ones: Optional[torch.Tensor] = None                               # the allow word of a hidden-only call, one per batch row

    def _source(self, items: Optional[torch.Tensor]):
        """What the components of the whole corpus are read from -> (fp32-format index buffer, None), or on a split-f16 engine (None, the
        (P_X, N, d) fp16 table cut from temporary fp32-format index chunks of `items`)."""
        engine, index, shape = self._engine, self._index, self._shape
        if engine.precision == "fp32":
            return index.buf, None
        n, dev = index.n_items, index.buf.device
        items = _f32c(items)
        comp16 = torch.empty((self.groups, n, self.d), dtype=torch.float16, device=dev)
        chunk = self.COMPONENT_CHUNK
        tmp = torch.empty(self.lib.rails_mol_index_floats(C.byref(shape), min(chunk, n)), dtype=torch.float32, device=dev)
        with _on_device(dev):
            for lo in range(0, n, chunk):
                m = min(chunk, n - lo)
                _lib.check(self.lib.rails_mol_index_build(C.byref(shape), C.byref(engine.weights), _ptr(items[lo : lo + m]), m, _ptr(tmp), _stream()),
                           "rails_mol_index_build")
                _lib.check(self.lib.rails_ivf_components16_build(C.byref(shape), _ptr(tmp), m, _ptr(comp16), n, lo, _stream()),
                           "rails_ivf_components16_build")
        return None, comp16

    def _build_lists(self, src_index, comp16, ws: Optional[torch.Tensor] = None) -> None:
        """vectors / positions / offsets (allocated for n items) of the n items of the source, by the centroids held."""
        n, dev = self._positions.shape[1], self._centroids.device
        if ws is None:
            ws = torch.empty(max(self.lib.rails_ivf_build_workspace_bytes(C.byref(self._shape), n, self.nlist, 0), 1), dtype=torch.uint8, device=dev)
        with _on_device(dev):
            _lib.check(self.lib.rails_ivf_build_lists(C.byref(self._shape), _ptr(src_index), _ptr(comp16), n, self.nlist, _ptr(self._centroids),
                                                      _ptr(self._vectors), _ptr(self._positions), _ptr(self._offsets), _ptr(ws), ws.numel(), _stream()),
                       "rails_ivf_build_lists")

    def edit(self, positions: torch.Tensor, source: Optional[Tuple[torch.Tensor, int]], n_keep: int, items: Optional[torch.Tensor] = None) -> None:
        """The lists follow an in-place change of the corpus; the centroids stay bit for bit what they were.  Every old entry whose position
        is >= n_keep or in `positions` ((M,) int64 on the device, unique, may be empty) is dropped; one entry per element of `positions` is
        inserted -- its list by the assignment kernel's own body against the frozen centroids, its fp16 vector cut from `source`
        (MolEngine.update_source's pair; None with M = 0).  Afterwards vectors / positions / offsets are what rails_ivf_build_lists writes
        from the resulting corpus with these centroids.  PRECONDITION (MoLTopKModule's hooks keep it): the engine's index this object was
        built from already holds the resulting corpus when edit() is called -- updated, grown or cut -- and `items`, needed on a split-f16
        engine only, is the resulting raw table of as many rows.  The edit kernel reads the inserted items from it; more than EDIT_MAX
        positions do not go through the kernel at all: the lists are rebuilt from that index (`positions`, `source` and `n_keep` are then
        not read), with the same result.  One small read-back: the number of replaced entries and the new offsets."""
        dev = self._centroids.device
        m, n_old, n_keep = int(positions.numel()), self.n_items, int(n_keep)
        lim = min(n_old, n_keep)
        if m and (positions.dtype != torch.int64 or positions.dim() != 1 or positions.device != dev):
            raise ValueError(f"IvfIndex.edit: positions must be an (M,) int64 tensor on {dev}")
        if m > self.EDIT_MAX:
            n_new = self._index.n_items
            if n_new < self.nlist:
                raise ValueError(f"IvfIndex: {n_new} items cannot fill nlist = {self.nlist} lists")
            if self._engine.precision != "fp32" and items is None:
                raise ValueError("IvfIndex.edit: a non-fp32 engine needs the raw item embeddings to rebuild the lists from")
            src_index, comp16 = self._source(items)
            self._vectors = self._positions = None      # (freed before the new ones are allocated)
            self._vectors = torch.empty((self.groups, n_new, self.d), dtype=torch.float16, device=dev)
            self._positions = torch.empty((self.groups, n_new), dtype=torch.int32, device=dev)
            self._build_lists(src_index, comp16)
        else:
            positions = positions.contiguous()
            n_new = ivf_edited_size(n_old, n_keep, m=m, below=int((positions < lim).sum()) if m else 0)
            if n_new < self.nlist:
                raise ValueError(f"IvfIndex: {n_new} items cannot fill nlist = {self.nlist} lists")
            ws_bytes = self.lib.rails_ivf_lists_edit_workspace_bytes(C.byref(self._shape), n_old, self.nlist, m)
            if ws_bytes == 0:
                raise NotImplementedError(f"rails_ivf_lists_edit_workspace_bytes: {_lib.last_error()}")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            vectors = torch.empty((self.groups, n_new, self.d), dtype=torch.float16, device=dev)
            pos_new = torch.empty((self.groups, n_new), dtype=torch.int32, device=dev)
            offsets = torch.empty_like(self._offsets)
            src, in_place = source if m else (None, 1)
            with _on_device(dev):
                _lib.check(self.lib.rails_ivf_lists_edit(C.byref(self._shape), _ptr(src), int(in_place), _ptr(positions) if m else None, m, n_keep, self.nlist,
                                                         _ptr(self._centroids), _ptr(self._vectors), _ptr(self._positions), _ptr(self._offsets), n_old,
                                                         _ptr(vectors), _ptr(pos_new), _ptr(offsets), n_new, _ptr(ws), ws.numel(), _stream()),
                           "rails_ivf_lists_edit")
            self._vectors, self._positions, self._offsets = vectors, pos_new, offsets
        self.n_items = n_new
        self._offsets_host = self._offsets.cpu().contiguous()
        self._plans.clear()
        self._list_words = None       # the words sit beside `positions`: other lists, other words, counts and plans
        self._filter_plans.clear()

    # read-only views of the index (tests and tools)
    centroids = property(lambda self: self._centroids, doc="(P_X, nlist, d) fp32 unit-norm centroids")
    vectors = property(lambda self: self._vectors, doc="(P_X, N, d) fp16 components in list order")
    positions = property(lambda self: self._positions, doc="(P_X, N) int32 item positions alongside `vectors`")
    offsets = property(lambda self: self._offsets, doc="(P_X, nlist + 1) int32 list starts")
    nprobe = property(lambda self: self._nprobe, doc="lists probed per query component when search() is not told otherwise")

    def _check_nprobe(self, nprobe: int) -> None:
        if nprobe < 1 or nprobe > min(64, self.nlist):
            raise NotImplementedError(f"IvfIndex: nprobe = {nprobe} outside [1, min(64, nlist = {self.nlist})]")

    def _plan(self, nprobe: int, k: int) -> Tuple[int, int]:
        key = (nprobe, k)
        p = self._plans.get(key)
        if p is None:
            mp, ml = C.c_int32(0), C.c_int32(0)
            _lib.check(self.lib.rails_ivf_plan(C.byref(self._shape), C.c_void_p(self._offsets_host.data_ptr()), self.nlist, nprobe, k,
                                               C.byref(mp), C.byref(ml)), "rails_ivf_plan")
            p = self._plans[key] = (mp.value, ml.value)
        return p

    # ---- filtered lists: the hidden set / allowed_tags inside the list scan ---------------------------------------------------------------
    def list_words(self, filter) -> torch.Tensor:
        """(P_X, N) int32: the filter in list order, beside `positions` (rails_ivf_list_words: one gather launch) -- the effective tag word of
        every entry for a TagFilter, all ones / 0 for a visible / hidden entry for a visibility row.  Kept until the lists change (edit()) or
        another source array comes: the module makes a new one whenever its hidden set or its tags change, and only then."""
        src = filter.eff if isinstance(filter, TagFilter) else filter
        c = self._list_words
        if c is None or c[0] is not src:
            dev, n = self._centroids.device, self.n_items
            if isinstance(filter, TagFilter):
                ok = filter.n_items == n and src.device == dev
            else:
                ok = (torch.is_tensor(src) and src.dtype == torch.int32 and src.numel() == item_mask_words(n) and src.is_contiguous() and src.device == dev)
            if not ok:
                raise ValueError(f"IvfIndex.search: filter must be a TagFilter over the {n} items on {dev}, or their int32 visibility row")
            words = torch.empty((self.groups, n), dtype=torch.int32, device=dev)
            tagged = isinstance(filter, TagFilter)
            with _on_device(dev):
                _lib.check(self.lib.rails_ivf_list_words(_ptr(self._positions), self.groups, n, _ptr(src) if tagged else None, None if tagged else _ptr(src),
                                                         _ptr(words), _stream()), "rails_ivf_list_words")
            c = self._list_words = (src, words)
            self._filter_plans.clear()
        return c[1]

    def filter_plan(self, filter) -> IvfFilterPlan:
        """The counts of `filter` over the lists as they are: one launch and ONE read-back the first time a filter is seen, nothing afterwards."""
        words = self.list_words(filter)
        p = self._filter_plans.get(id(filter))
        if p is None or p.key is not filter:
            dev = self._centroids.device
            if isinstance(filter, TagFilter):
                allowed = filter.allowed
            else:
                allowed = torch.full((1,), -1, dtype=torch.int32, device=dev)      # one word shared by the batch: one row of counts
            counts = torch.empty((allowed.numel(), self.groups, self.nlist), dtype=torch.int32, device=dev)
            with _on_device(dev):
                _lib.check(self.lib.rails_ivf_list_counts(_ptr(words), _ptr(self._offsets), self.groups, self.n_items, self.nlist, _ptr(allowed),
                                                          allowed.numel(), _ptr(counts), _stream()), "rails_ivf_list_counts")
            if len(self._filter_plans) >= self.FILTER_PLANS_KEPT:
                self._filter_plans.clear()
            p = self._filter_plans[id(filter)] = IvfFilterPlan(filter, allowed, counts)
        return p

    def _filtered_max_probes(self, plan: IvfFilterPlan, nprobe: int, k: int) -> int:
        mp = plan.max_probes.get((nprobe, k))
        if mp is None:
            out = C.c_int32(0)
            _lib.check(self.lib.rails_ivf_plan_filtered(C.c_void_p(plan.counts_host.data_ptr()), plan.count_rows, self.groups, self.nlist, nprobe, k,
                                                        C.byref(out)), "rails_ivf_plan_filtered")
            mp = plan.max_probes[(nprobe, k)] = out.value
        return mp

    def _search_filtered(self, eq: torch.Tensor, k: int, nprobe: int, out: torch.Tensor, filter, check: bool) -> None:
        """The refusals are the twin's own -- an index of the kept items alone -- before any search launch; the batch is cut so that the
        workspace of one call stays under FILTER_WS_CAP."""
        B, dev = eq.shape[0], self._centroids.device
        plan = self.filter_plan(filter)
        if plan.count_rows not in (1, B):
            raise ValueError(f"IvfIndex.search: the filter has {plan.count_rows} allow words, the batch {B} rows")
        kept = min(plan.kept)
        if kept < self.nlist:
            raise ValueError(f"IvfIndex: {kept} items cannot fill nlist = {self.nlist} lists")
        if k > kept:
            raise RuntimeError(f"selected index k out of range (k={k}, n={kept})")
        if B == 0:
            return
        max_probes, max_list = self._filtered_max_probes(plan, nprobe, k), self._plan(nprobe, k)[1]
        if isinstance(filter, TagFilter):
            allowed = filter.allowed_for(B)
        else:
            if self._all_ones is None or self._all_ones.numel() < B:
                self._all_ones = torch.full((B,), -1, dtype=torch.int32, device=dev)
            allowed = self._all_ones
        step = B
        while True:
            ws_bytes = self.lib.rails_ivf_search_workspace_bytes(C.byref(self._shape), step, self.nlist, nprobe, max_probes, max_list, k)
            if ws_bytes == 0:
                raise NotImplementedError(f"rails_ivf_search_workspace_bytes: {_lib.last_error()}")
            if ws_bytes <= self.FILTER_WS_CAP or step == 1:
                break
            step = (step + 1) // 2
        if self._ws is None or self._ws.numel() < ws_bytes:
            self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with _on_device(dev):
            for b0 in range(0, B, step):
                b1 = min(B, b0 + step)
                counts = plan.counts if plan.count_rows == 1 else plan.counts[b0:b1]
                _lib.check(self.lib.rails_ivf_search_filtered(C.byref(self._shape), _ptr(eq[b0:b1]), b1 - b0, _ptr(self._centroids), _ptr(self._vectors),
                                                              _ptr(self._positions), _ptr(self._offsets), self.n_items, self.nlist, nprobe, max_probes,
                                                              max_list, k, _ptr(self._ws), self._ws.numel(), _ptr(out[b0:b1]),
                                                              _ptr(self._unfilled), _ptr(self.list_words(filter)), _ptr(allowed[b0:b1]),
                                                              _ptr(counts), plan.count_rows if plan.count_rows == 1 else b1 - b0, _stream()),
                           "rails_ivf_search_filtered")
                if check and int(self._unfilled.item()) != 0:      # (every call zeroes the word: it is read per slice)
                    raise RuntimeError("IvfIndex.search: some row found fewer than k_per_group items")

    def search(self, eq: torch.Tensor, k_per_group: int, nprobe: Optional[int] = None, out: Optional[torch.Tensor] = None,
               check: bool = False, filter=None) -> torch.Tensor:
        """eq (B, P_Q, d) fp32 query components -> (B, P_Q * P_X * k_per_group) int64 item positions, row-major over (query group,
        item group, rank) as MoLNaiveTopK's exhaustive candidates.  check: wait for the call and raise if some row found fewer than
        k_per_group items (which the probe plan rules out).
        filter: a TagFilter (row b returns only items x with eff[x] & words[b] != 0), or the module's (1, words) int32 visibility row (no row
        returns a hidden item).  Row b then equals, position for position through the kept rows, the plain search of an index built with these
        centroids from the items row b keeps.  ValueError where a row keeps fewer than nlist items, RuntimeError where fewer than k_per_group."""
        nprobe = self._nprobe if nprobe is None else int(nprobe)
        self._check_nprobe(nprobe)
        k = int(k_per_group)
        if k < 1 or k > 128:
            raise NotImplementedError(f"IvfIndex: k_per_group = {k} outside [1, 128]")
        if k > self.n_items:
            raise RuntimeError(f"selected index k out of range (k={k}, n={self.n_items})")
        if eq.dim() != 3 or eq.shape[1] != self.query_groups or eq.shape[2] != self.d:
            raise ValueError(f"IvfIndex.search: eq must be (B, {self.query_groups}, {self.d}), got {tuple(eq.shape)}")
        B = eq.shape[0]
        dev = self._centroids.device
        if eq.device != dev:
            raise ValueError(f"IvfIndex.search: eq is on {eq.device}, the index on {dev}")
        eq = _f32c(eq)
        shape_out = (B, self.query_groups * self.groups * k)
        if out is not None and (tuple(out.shape) != shape_out or out.dtype != torch.int64 or not out.is_contiguous() or out.device != dev):
            raise ValueError(f"IvfIndex.search: out must be a contiguous int64 {shape_out} tensor on {dev}")
        if filter is not None:
            if out is None:
                out = torch.empty(shape_out, dtype=torch.int64, device=dev)
            self._search_filtered(eq, k, nprobe, out, filter, check)
            return out
        max_probes, max_list = self._plan(nprobe, k)
        ws_bytes = self.lib.rails_ivf_search_workspace_bytes(C.byref(self._shape), max(B, 1), self.nlist, nprobe, max_probes, max_list, k)
        if ws_bytes == 0:
            raise NotImplementedError(f"rails_ivf_search_workspace_bytes: {_lib.last_error()}")
        if self._ws is None or self._ws.numel() < ws_bytes:
            self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.empty(shape_out, dtype=torch.int64, device=dev)
        with _on_device(dev):
            _lib.check(self.lib.rails_ivf_search(C.byref(self._shape), _ptr(eq), B, _ptr(self._centroids), _ptr(self._vectors), _ptr(self._positions),
                                                 _ptr(self._offsets), self.n_items, self.nlist, nprobe, max_probes, max_list, k, _ptr(self._ws),
                                                 self._ws.numel(), _ptr(out), _ptr(self._unfilled), _stream()), "rails_ivf_search")
        if check and B > 0 and int(self._unfilled.item()) != 0:
            raise RuntimeError("IvfIndex.search: some row found fewer than k_per_group items")
        return out

    def list_sizes(self) -> torch.Tensor:
        """(P_X, nlist) int64 list sizes (host)."""
        return (self._offsets_host[:, 1:] - self._offsets_host[:, :-1]).to(torch.int64)

def sort_rows(idx: torch.Tensor) -> torch.Tensor:
    """Ascending sort of every row of an int64 (rows, n) tensor, n <= 16384 (torch.sort(dim=1) values)."""
    lib = _lib.load()
    _require_device(idx, "indices")
    idx = idx.to(torch.int64).contiguous()
    out = torch.empty_like(idx)
    with _on_device(idx.device):
        _lib.check(lib.rails_sort_rows_i64(_ptr(idx), idx.shape[0], idx.shape[1], _ptr(out), _stream()), "rails_sort_rows_i64")
    return out


def mask_sorted_duplicates(sorted_idx: torch.Tensor, scores: torch.Tensor, fill: float) -> None:
    """In place: scores[r, j] = fill wherever sorted_idx[r, j] == sorted_idx[r, j - 1]."""
    lib = _lib.load()
    rows, n = sorted_idx.shape
    assert scores.dtype == torch.float32 and scores.stride(1) == 1
    with _on_device(scores.device):
        _lib.check(
            lib.rails_mask_sorted_duplicates(_ptr(sorted_idx), _ptr(scores), scores.stride(0), rows, n, C.c_float(fill), _stream()),
            "rails_mask_sorted_duplicates",
        )


# ---- dot-product (MIPS) scoring ----------------------------------------------------------------
class MipsIndex:
    """Tile-packed fp32 copy of an (N, D) item table for the MFMA dot-product scan."""

    def __init__(self, items: torch.Tensor):
        lib = _lib.load()
        _require_device(items, "item_embeddings")
        items = _f32c(items)
        self.n_items, self.dim = items.shape
        self.buf = torch.empty(lib.rails_mips_index_floats(self.dim, self.n_items), dtype=torch.float32, device=items.device)
        with _on_device(items.device):
            _lib.check(lib.rails_mips_index_build(_ptr(items), self.n_items, self.dim, _ptr(self.buf), _stream()), "rails_mips_index_build")

    # ---- in-place changes (MIPSBruteForceTopK.update_items / append_items / remove_items): the bytes of a fresh build of the changed table ----
    def update(self, positions: torch.Tensor, items: torch.Tensor) -> None:
        """items (M, D) -> slots positions (M,) int64 on the device, unique (rails_mips_index_update: the build's stores, scatter addressing)."""
        _require_device(items, "item_embeddings")
        if items.dim() != 2 or items.shape[1] != self.dim or positions.shape != (items.shape[0],) or positions.dtype != torch.int64:
            raise ValueError(f"update takes (M, {self.dim}) items and (M,) int64 positions, got {tuple(items.shape)} and {tuple(positions.shape)}")
        items, positions = _f32c(items), positions.to(self.buf.device).contiguous()
        with _on_device(self.buf.device):
            _lib.check(_lib.load().rails_mips_index_update(_ptr(items), items.shape[0], self.dim, _ptr(positions), _ptr(self.buf), self.n_items, _stream()),
                       "rails_mips_index_update")

    def rows(self, positions: torch.Tensor) -> torch.Tensor:
        """(M, D) fp32: the items at `positions` as the index holds them (the module keeps no raw table; fp32 copies, so the round trip is exact)."""
        positions = positions.to(self.buf.device).contiguous()
        out = torch.empty((positions.numel(), self.dim), dtype=torch.float32, device=self.buf.device)
        with _on_device(self.buf.device):
            _lib.check(_lib.load().rails_mips_index_gather_rows(_ptr(self.buf), self.n_items, self.dim, _ptr(positions), positions.numel(), _ptr(out), _stream()),
                       "rails_mips_index_gather_rows")
        return out

    def resize(self, n_items: int) -> None:
        """To n_items items, as MolEngine.resize_index: whole tiles copied, zeros beyond them; cut, the slots past n_items of the new last tile
        are set to zero (rails_mips_index_clear_tail).  New slots are filled by update()."""
        if n_items < 1:
            raise ValueError(f"resize: {n_items} items")
        lib = _lib.load()
        shrinking = n_items < self.n_items
        buf = resized(self.buf, lib.rails_mips_index_floats(self.dim, n_items), zero=True)
        if shrinking:
            with _on_device(buf.device):
                _lib.check(lib.rails_mips_index_clear_tail(_ptr(buf), n_items, self.dim, _stream()), "rails_mips_index_clear_tail")
        self.buf, self.n_items = buf, n_items

    def score(self, q: torch.Tensor) -> torch.Tensor:
        """(B, D) -> (B, N) fp32 dot products (reference rails/indexing/mips_top_k.py:72)."""
        lib = _lib.load()
        _require_device(q, "query_embeddings")
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(q.shape)} and {self.dim}x{self.n_items})")
        q = _f32c(q)
        B = q.shape[0]
        ws = torch.empty(lib.rails_mips_query_ws_floats(self.dim, B), dtype=torch.float32, device=q.device)
        out = torch.empty((B, self.n_items), dtype=torch.float32, device=q.device)
        with _on_device(q.device):
            _lib.check(lib.rails_mips_score(_ptr(q), B, self.dim, _ptr(self.buf), self.n_items, _ptr(ws), _ptr(out), out.stride(0), _stream()), "rails_mips_score")
        return out


    def score_at(self, q: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        """(B, D), (B, T) int64 positions -> (B, T) fp32: <q[b], item positions[b, j]> with score()'s bits for that pair, the items read in place
        (rails_mips_score_indexed); a position outside [0, N) is clamped into it -- the caller overwrites such entries."""
        lib = _lib.load()
        _require_device(q, "query_embeddings")
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(q.shape)} and {self.dim}x{self.n_items})")
        q = _f32c(q)
        B = q.shape[0]
        positions = positions.to(device=q.device, dtype=torch.int64).contiguous()
        ws = torch.empty(lib.rails_mips_query_ws_floats(self.dim, B), dtype=torch.float32, device=q.device)
        out = torch.empty((B, positions.shape[1]), dtype=torch.float32, device=q.device)
        with _on_device(q.device):
            _lib.check(lib.rails_mips_score_indexed(_ptr(q), B, self.dim, _ptr(self.buf), self.n_items, _ptr(positions), positions.shape[1], _ptr(ws), _ptr(out),
                                                    out.stride(0), _stream()), "rails_mips_score_indexed")
        return out


# ---- item id -> position map (rails_id_map_*) ---------------------------------------------------
ID_MAP_RESERVED = (-(1 << 63), -(1 << 63) + 1)      # EMPTY and ERASED: no item may carry these ids


def _ids_arg(ids: torch.Tensor, device: torch.device, what: str = "item_ids") -> torch.Tensor:
    if not torch.is_tensor(ids) or ids.dtype != torch.int64 or ids.dim() != 1:
        raise ValueError(f"{what} must be (M,) int64")
    return ids.to(device).contiguous()


def id_map_slots(n_items: int) -> int:
    slots = _lib.load().rails_id_map_slots(n_items)
    if slots < 0:
        _lib.check(int(slots), "rails_id_map_slots")
    return int(slots)


def id_map_new(slots: int, device: torch.device) -> torch.Tensor:
    """An empty table of `slots` slots (int64 keys, then int32 values) as one uint8 tensor."""
    lib = _lib.load()
    table = torch.empty(lib.rails_id_map_bytes(slots), dtype=torch.uint8, device=device)
    with _on_device(table.device):
        _lib.check(lib.rails_id_map_clear(_ptr(table), slots, _stream()), "rails_id_map_clear")
    return table


def id_map_insert(table: torch.Tensor, slots: int, ids: torch.Tensor, positions: Optional[torch.Tensor], first: int, flags: torch.Tensor) -> None:
    """ids (M,) int64 -> positions (M,) int64, or first + u for None; flags (>= 3,) int32 on the device is added to: [0] present already or twice in
    the call, [1] reserved, [2] no slot."""
    ids = _ids_arg(ids, table.device)
    if positions is not None:
        positions = _ids_arg(positions, table.device, "positions")
        if positions.numel() != ids.numel():
            raise ValueError(f"{ids.numel()} ids but {positions.numel()} positions")
    with _on_device(table.device):
        _lib.check(_lib.load().rails_id_map_insert(_ptr(table), slots, _ptr(ids), _ptr(positions), first, ids.numel(), _ptr(flags), _stream()),
                   "rails_id_map_insert")


def id_map_erase(table: torch.Tensor, slots: int, ids: torch.Tensor, missing: torch.Tensor) -> None:
    """The keys of ids (M,) int64 become tombstones; missing (1,) int32 on the device is added to for every absent id."""
    ids = _ids_arg(ids, table.device)
    with _on_device(table.device):
        _lib.check(_lib.load().rails_id_map_erase(_ptr(table), slots, _ptr(ids), ids.numel(), _ptr(missing), _stream()), "rails_id_map_erase")


def id_map_lookup(table: torch.Tensor, slots: int, ids: torch.Tensor) -> torch.Tensor:
    """(M,) int64 positions on the table's device, -1 where the id is absent."""
    ids = _ids_arg(ids, table.device)
    out = torch.empty(ids.numel(), dtype=torch.int64, device=table.device)
    with _on_device(table.device):
        _lib.check(_lib.load().rails_id_map_lookup(_ptr(table), slots, _ptr(ids), ids.numel(), _ptr(out), _stream()), "rails_id_map_lookup")
    return out


class ItemIdMap:
    """The id -> position map of one corpus: the device table, the live and tombstone counts (host integers: upper bounds of the slots in
    use) and four device counters -- [0] duplicates, [1] reserved ids, [2] inserts without a slot, [3] erased ids that were absent.

    Tombstones are never reused, so the slots in use only grow: before any launch that would take live + tombstones + incoming past
    slots / 2, insert builds the table again, at rails_id_map_slots(n) slots, from `ids_flat` -- the ids, in position order, that the map
    is to hold once the call in progress is done (a module passes its own id tensor, written before the map is told).  The kernels' "no
    slot" counter cannot be reached through this class.  insert / erase launch and return; take_flags() reads and clears the counters (one
    sync) and is how a caller learns that the ids it fed were not what the map expected."""

    def __init__(self, device: torch.device):
        self.device = torch.device(device)
        self.table: Optional[torch.Tensor] = None
        self.slots = self.live = self.tombstones = self.rebuilds = 0
        with torch.inference_mode(False):     # (an ordinary tensor: cleared in place from inside and outside inference mode)
            self.flags = torch.zeros(4, dtype=torch.int32, device=self.device)

    def build(self, ids_flat: torch.Tensor) -> None:
        """A fresh table holding ids_flat[p] -> p.  ValueError, naming the count, for ids that repeat or are reserved (the map is then empty)."""
        ids = _ids_arg(ids_flat, self.device, "ids_flat")
        self.slots = id_map_slots(ids.numel())
        self.table = id_map_new(self.slots, self.device)
        self.live, self.tombstones = ids.numel(), 0
        self.flags.zero_()
        id_map_insert(self.table, self.slots, ids, None, 0, self.flags)
        dup, reserved, _, _ = self.take_flags()
        if dup or reserved:
            self.table, self.slots, self.live = None, 0, 0
            raise ValueError(f"the corpus cannot be addressed by id: {dup} of its {ids.numel()} item ids repeat an earlier one and {reserved} are reserved "
                             f"values ({ID_MAP_RESERVED[0]}, {ID_MAP_RESERVED[1]})")

    def rebuild(self, ids_flat: torch.Tensor) -> None:
        """build(), counted: what insert does instead of letting the load pass 1/2."""
        self.rebuilds += 1
        self.build(ids_flat)

    def insert(self, ids: torch.Tensor, positions: torch.Tensor, ids_flat: torch.Tensor) -> None:
        m = ids.numel()
        if self.table is None or self.live + self.tombstones + m > self.slots // 2:
            self.rebuild(ids_flat)      # holds `ids` at `positions` already
            return
        id_map_insert(self.table, self.slots, ids, positions, 0, self.flags)
        self.live += m

    def erase(self, ids: torch.Tensor) -> None:
        m = ids.numel()
        id_map_erase(self.table, self.slots, ids, self.flags[3:])
        self.live -= m
        self.tombstones += m

    def lookup(self, ids: torch.Tensor) -> torch.Tensor:
        return id_map_lookup(self.table, self.slots, ids)

    def take_flags(self) -> Tuple[int, int, int, int]:
        host = self.flags.tolist()      # (one sync)
        if any(host):
            self.flags.zero_()
        return tuple(host)

    def info(self) -> Dict[str, int]:
        return {"slots": self.slots, "live": self.live, "tombstones": self.tombstones, "rebuilds": self.rebuilds}


# ---- item masks (rails_item_mask_*, rails_scores_mask) ---------------------
def item_mask_words(n_items: int) -> int:
    return (int(n_items) + 31) // 32


def check_item_mask(mask_items: int, mask_rows: int, shared: bool, kept_min: int, n_items: int, batch: Optional[int], k: Optional[int]) -> None:
    """The pure checks of a masked call, made before any launch: a mask of `mask_items` items (`mask_rows` rows, shared by the batch or one per
    query row, its smallest row keeping `kept_min`) against a module of `n_items` items, a batch of `batch` rows and a call for k results
    (None: not checked).  ValueError for a mask of another corpus size or another batch; for k beyond the kept items what k > N raises."""
    if mask_items != n_items:
        raise ValueError(f"item_mask covers {mask_items} items but the module holds {n_items}: a mask is by position -- build a new one after "
                         "append_items / remove_items (mask_of_ids does it from ids)")
    if not shared and batch is not None and mask_rows != batch:
        raise ValueError(f"item_mask has {mask_rows} rows but the batch has {batch}")
    if k is not None and k > kept_min:
        raise RuntimeError(f"selected index k out of range (k={k}, n={kept_min})")


class ItemMask:
    """Which items a top-k call may return (item_mask= of MoLBruteForceTopK / MIPSBruteForceTopK): by POSITION, tied to n_items.
      ItemMask(mask)        mask: bool device tensor (N,) -- shared by the batch -- or (B, N) -- one row per query row; True = may be returned
      ItemMask.from_positions(n_items, positions, device)   a shared mask with exactly those positions set
    Holds `words` (rows, ceil(N / 32)) int32 -- bit i % 32 of word i / 32 is item i, the unused high bits of the last word zero --, `counts`
    (rows,) int32 on the device, n_items, rows, shared, and the host integers kept_min / kept_max from ONE read-back at construction: a
    reused mask costs a call no host sync.  positions(): the set positions per row, ascending, computed at first use and kept."""

    def __init__(self, mask: torch.Tensor):
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or mask.dim() not in (1, 2) or mask.shape[-1] < 1 or mask.shape[0] < 1:
            raise ValueError("item_mask must be a bool tensor (N,) or (B, N)")
        _require_device(mask, "item_mask")
        shared = mask.dim() == 1
        m2 = mask.reshape(1, -1) if shared else mask
        rows, n = m2.shape
        if m2.stride(1) != 1 or (rows > 1 and m2.stride(0) < n):
            m2 = m2.contiguous()
        words = torch.empty((rows, item_mask_words(n)), dtype=torch.int32, device=mask.device)
        counts = torch.empty(rows, dtype=torch.int32, device=mask.device)
        with _on_device(mask.device):
            _lib.check(_lib.load().rails_item_mask_pack(_ptr(m2), m2.stride(0) if rows > 1 else n, rows, n, _ptr(words), _ptr(counts), _stream()),
                       "rails_item_mask_pack")
        self._init(words, counts, n, shared, counts.cpu())      # (the one sync)

    def _init(self, words: torch.Tensor, counts: torch.Tensor, n_items: int, shared: bool, counts_host: torch.Tensor) -> None:
        self.words, self.counts, self.n_items, self.shared = words, counts, int(n_items), bool(shared)
        self.rows = words.shape[0]
        self._counts_host = counts_host
        self.kept_min, self.kept_max = int(counts_host.min()), int(counts_host.max())
        self._positions: Optional[torch.Tensor] = None
        self._slots: Optional["ItemMask"] = None
        self._expanded: Optional[torch.Tensor] = None

    @classmethod
    def from_positions(cls, n_items: int, positions, device) -> "ItemMask":
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"item_mask must live on the GPU: rails_amd runs its path in HIP kernels only and has no CPU fallback (got {device})")
        pos = torch.as_tensor(positions)
        if pos.dtype != torch.int64 or pos.dim() != 1:
            raise ValueError("positions must be (M,) int64")
        n_items = int(n_items)
        if n_items < 1:
            raise ValueError(f"a mask of {n_items} items")
        if pos.numel():
            lo, hi = torch.aminmax(pos)      # (a sync when the positions live on the device; the construction reads the count back anyway)
            if int(lo) < 0 or int(hi) >= n_items:
                raise ValueError(f"positions must lie in [0, {n_items})")
        pos = pos.to(device).contiguous()
        lib = _lib.load()
        words = torch.zeros((1, item_mask_words(n_items)), dtype=torch.int32, device=device)
        counts = torch.empty(1, dtype=torch.int32, device=device)
        with _on_device(device):
            _lib.check(lib.rails_item_mask_set(_ptr(pos), pos.numel(), n_items, _ptr(words), _stream()), "rails_item_mask_set")
            _lib.check(lib.rails_item_mask_count(_ptr(words), 1, n_items, _ptr(counts), _stream()), "rails_item_mask_count")
        self = cls.__new__(cls)
        self._init(words, counts, n_items, True, counts.cpu())
        return self

    def check(self, n_items: int, batch: Optional[int] = None, k: Optional[int] = None) -> None:
        check_item_mask(self.n_items, self.rows, self.shared, self.kept_min, n_items, batch, k)

    def positions(self) -> torch.Tensor:
        """(rows, kept_max) int64: each row's set positions ascending, the slots past counts[r] hold 0 (rails_item_mask_positions)."""
        if self._positions is None:
            lib = _lib.load()
            out = torch.empty((self.rows, self.kept_max), dtype=torch.int64, device=self.words.device)
            ws_bytes = lib.rails_item_mask_positions_workspace_bytes(self.rows, self.n_items)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.words.device)
            with _on_device(self.words.device):
                _lib.check(lib.rails_item_mask_positions(_ptr(self.words), self.rows, self.n_items, _ptr(out) if self.kept_max else None, self.kept_max,
                                                         _ptr(ws), ws_bytes, _stream()), "rails_item_mask_positions")
            self._positions = out
        return self._positions

    def positions_for(self, batch: int) -> torch.Tensor:
        """positions() as (batch, kept_max) contiguous rows, one per query row: a shared mask's row repeated (kept for the last batch size)."""
        pos = self.positions()
        if not self.shared or batch == 1:
            return pos
        c = self._expanded
        if c is None or c.shape[0] != batch:
            c = self._expanded = pos.expand(batch, -1).contiguous()
        return c

    def ragged(self) -> bool:
        return self.kept_min != self.kept_max

    def slot_mask(self) -> "ItemMask":
        """The mask of the SLOTS of positions(): bit j of row r is set iff j < counts[r] -- what clears the scores of a ragged row's padding
        slots (rails_scores_mask on the (rows, kept_max) candidate scores).  Built at first use and kept."""
        if self._slots is None:
            self._slots = ItemMask(torch.arange(self.kept_max, device=self.words.device).unsqueeze(0) < self.counts.unsqueeze(1))
        return self._slots

    def rows_slice(self, b0: int, b1: int) -> "ItemMask":
        """The mask of the batch rows b0 .. b1 - 1 (the 4 GiB logit policy slices the batch); a shared mask is its own slice.  No sync."""
        if self.shared:
            return self
        b0, b1 = max(0, int(b0)), min(self.rows, int(b1))
        if b0 >= b1:
            raise ValueError(f"rows_slice: no rows in [{b0}, {b1})")
        if b0 == 0 and b1 == self.rows:
            return self
        part = ItemMask.__new__(ItemMask)
        part._init(self.words[b0:b1], self.counts[b0:b1], self.n_items, False, self._counts_host[b0:b1])
        if self._positions is not None:
            part._positions = self._positions[b0:b1, : part.kept_max].contiguous()
        return part

    def rows_take(self, rows: torch.Tensor) -> "ItemMask":
        """The per-row mask whose row i is this mask's row rows[i] ((M,) int64 on the CPU) -- a fused row's mask repeated over its sub-query
        rows; a shared mask is returned as it is.  No sync."""
        if self.shared:
            return self
        part = ItemMask.__new__(ItemMask)
        on_dev = rows.to(self.words.device)
        part._init(self.words.index_select(0, on_dev), self.counts.index_select(0, on_dev), self.n_items, False, self._counts_host.index_select(0, rows))
        return part


def _check_visible_words(visible: Optional[torch.Tensor], n_items: int, device: torch.device) -> None:
    """The visibility row a scan reads one word per 32-item tile of: exactly the words of n_items, on the table's device -- checked before any launch."""
    if visible is None:
        return
    if (not torch.is_tensor(visible) or visible.dtype != torch.int32 or visible.numel() != item_mask_words(n_items) or not visible.is_contiguous()
            or visible.device != device):
        raise ValueError(f"visible must be the {item_mask_words(n_items)} contiguous int32 mask words of {n_items} items on {device}")


def last_word_mask(n_items: int) -> int:
    """The live bits of the last word of a row of n_items bits, as the int32 that holds them (the unused high bits of a row are zero)."""
    live = n_items - 32 * (item_mask_words(n_items) - 1)
    v = (1 << live) - 1
    return v - (1 << 32) if v >= 1 << 31 else v


def visibility_row(n_items: int, device) -> torch.Tensor:
    """(1, words) int32 on `device`: the row in which every one of n_items items is visible."""
    words = torch.full((1, item_mask_words(n_items)), -1, dtype=torch.int32, device=device)
    words[0, -1] = last_word_mask(n_items)
    return words


def visibility_edit(words: torch.Tensor, n_items: int, positions: torch.Tensor, visible: bool) -> Tuple[torch.Tensor, int]:
    """A COPY of the visibility row `words` with the bits at `positions` (device int64, inside [0, n_items)) set (visible) or cleared (hidden:
    rails_item_mask_clear), and its number of set bits (rails_item_mask_count; the one read-back).  The row given is not written: launches
    already enqueued against it keep what they were submitted against."""
    lib = _lib.load()
    out = words.clone()
    counts = torch.empty(1, dtype=torch.int32, device=words.device)
    fn, name = (lib.rails_item_mask_set, "rails_item_mask_set") if visible else (lib.rails_item_mask_clear, "rails_item_mask_clear")
    with _on_device(words.device):
        _lib.check(fn(_ptr(positions), positions.numel(), n_items, _ptr(out), _stream()), name)
        _lib.check(lib.rails_item_mask_count(_ptr(out), 1, n_items, _ptr(counts), _stream()), "rails_item_mask_count")
    return out, int(counts.cpu()[0])


def visibility_count(words: torch.Tensor, n_items: int) -> int:
    counts = torch.empty(1, dtype=torch.int32, device=words.device)
    with _on_device(words.device):
        _lib.check(_lib.load().rails_item_mask_count(_ptr(words), 1, n_items, _ptr(counts), _stream()), "rails_item_mask_count")
    return int(counts.cpu()[0])


def item_mask_of_words(words: torch.Tensor, n_items: int, kept: int) -> ItemMask:
    """The shared ItemMask over an existing (1, words) row that keeps `kept` items (no launch, no sync)."""
    m = ItemMask.__new__(ItemMask)
    m._init(words, torch.full((1,), kept, dtype=torch.int32, device=words.device), n_items, True, torch.tensor([kept], dtype=torch.int32))
    return m


def item_mask_and(mask: ItemMask, visible: ItemMask) -> ItemMask:
    """mask AND the shared row `visible`, row by row: what a call with item_mask= returns from a module with a hidden set (one sync: the counts)."""
    words = torch.bitwise_and(mask.words, visible.words).contiguous()
    counts = torch.empty(mask.rows, dtype=torch.int32, device=words.device)
    with _on_device(words.device):
        _lib.check(_lib.load().rails_item_mask_count(_ptr(words), mask.rows, mask.n_items, _ptr(counts), _stream()), "rails_item_mask_count")
    m = ItemMask.__new__(ItemMask)
    m._init(words, counts, mask.n_items, mask.shared, counts.cpu())
    return m


def as_item_mask(item_mask) -> ItemMask:
    """item_mask= as given: an ItemMask, or a bool tensor packed for this call (one sync: keep an ItemMask to avoid it)."""
    return item_mask if isinstance(item_mask, ItemMask) else ItemMask(item_mask)


def score_matrix_ld(rows: int, n: int, stride0: int) -> int:
    """The leading dimension the kernels are given for a (rows, n) matrix whose rows lie stride0 elements apart.  The stride of a single row
    (or of none) is whatever the view it was cut from carries, a broadcast 0 or 1 included: such a matrix goes as rows of at least n, which is
    what keeps a one-row slice of a recycled buffer inside its allocation under the kernels' ld >= n rule."""
    return stride0 if rows > 1 else max(n, stride0)


def _score_matrix(t: torch.Tensor, name: str = "scores", error: Optional[str] = None) -> Tuple[int, int, int]:
    """The one check of a (rows, n) fp32 matrix with unit column stride on the GPU -> (rows, n, ld)."""
    _require_device(t, name)
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(error or f"{name} must be (rows, n) fp32 with contiguous rows")
    rows, n = t.shape
    return rows, n, score_matrix_ld(rows, n, t.stride(0))


def _positions_arg(what: str, positions: torch.Tensor, rows: int, device: torch.device, beside: str = "scores", t: str = "t") -> None:
    """The one check of a (rows, t) int64 `positions` argument on the device of the matrix (`beside`) it addresses."""
    if not torch.is_tensor(positions) or positions.dtype != torch.int64 or positions.dim() != 2 or positions.shape[0] != rows:
        raise ValueError(f"{what}: positions must be ({rows}, {t}) int64")
    if positions.device != device:
        raise ValueError(f"{what}: the positions and the {beside} live on different devices")


def _lse_arg(what: str, lse: torch.Tensor, rows: int, device: torch.device) -> torch.Tensor:
    if not torch.is_tensor(lse) or lse.dtype != torch.float32 or lse.shape != (rows,):
        raise ValueError(f"{what}: lse must be ({rows},) fp32")
    if lse.device != device:
        raise ValueError(f"{what}: the lse and the scores live on different devices")
    return lse.contiguous()


def scores_mask(scores: torch.Tensor, mask: ItemMask, first_item: int = 0, fill: float = float("-inf"), run_if: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place: scores[b, x] = fill wherever item first_item + x is not in row b's mask (rails_scores_mask); kept entries are not touched.
    scores (rows, n) fp32 with unit column stride; a per-row mask has one row per row of scores."""
    rows, n, ld = _score_matrix(scores)
    if first_item < 0 or first_item + n > mask.n_items:
        raise ValueError(f"scores_mask: items [{first_item}, {first_item + n}) are not inside a mask of {mask.n_items} items")
    if not mask.shared and mask.rows != rows:
        raise ValueError(f"scores_mask: the mask has {mask.rows} rows but scores has {rows}")
    if mask.words.device != scores.device:
        raise ValueError("scores_mask: the mask and the scores live on different devices")
    with _on_device(scores.device):
        _lib.check(_lib.load().rails_scores_mask(_ptr(scores), ld, rows, n, first_item, _ptr(mask.words),
                                                 0 if mask.shared else mask.words.stride(0), float(fill), _pred(run_if), _stream()), "rails_scores_mask")
    return scores


def scores_at_eligible(scores: torch.Tensor, positions: torch.Tensor, n_items: int, mask: Optional[ItemMask] = None, tags: Optional["TagFilter"] = None,
                       invalid_ids: Optional[torch.Tensor] = None, item_ids: Optional[torch.Tensor] = None,
                       extras: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """In place: scores[r, j] (the score of item positions[r, j] for row r; (rows, t) fp32) = -inf wherever the position lies outside
    [0, n_items) or row r may not return the item -- outside `mask` (shared or one row per row), no bit of the row's allow word of `tags` among
    its effective tags, or its id (`item_ids`, (n_items,) int64) among the row's `invalid_ids` ((rows, W)).  extras: two (rows, t, L) fp32
    arrays zeroed in the same pairs (rails_scores_at_eligible).  One launch, O(rows t (1 + W)); no sync."""
    rows, t, ld = _score_matrix(scores)
    _positions_arg("scores_at_eligible", positions, rows, scores.device)
    if positions.shape[1] != t:
        raise ValueError(f"scores_at_eligible: {t} scores but {positions.shape[1]} positions per row")
    words, stride = None, 0
    if mask is not None:
        if mask.n_items != n_items or (not mask.shared and mask.rows != rows) or mask.words.device != scores.device:
            raise ValueError(f"scores_at_eligible: the mask must cover the {n_items} items on {scores.device} with 1 or {rows} rows")
        words, stride = mask.words, 0 if mask.shared else mask.words.stride(0)
    eff = allowed = None
    if tags is not None:
        _check_tag_filter(tags, n_items, rows, scores.device, None)
        eff, allowed = tags.eff, tags.allowed_for(rows)
    inv, width = None, 0
    if invalid_ids is not None and (not torch.is_tensor(invalid_ids) or invalid_ids.dim() != 2 or invalid_ids.shape[0] != rows):
        raise ValueError(f"scores_at_eligible: invalid_ids must be ({rows}, W) integer ids")
    if invalid_ids is not None and invalid_ids.shape[1] > 0:
        if item_ids is None or item_ids.numel() != n_items:
            raise ValueError(f"scores_at_eligible: invalid_ids need the ids of the {n_items} items beside them")
        inv = invalid_ids.to(device=scores.device, dtype=torch.int64).contiguous()
        width = inv.shape[1]
    ea = eb = None
    length = 0
    if extras is not None:
        ea, eb = extras
        length = ea.shape[-1]
        if ea.shape != (rows, t, length) or eb.shape != ea.shape or not ea.is_contiguous() or not eb.is_contiguous() or ea.dtype != torch.float32 or eb.dtype != torch.float32:
            raise ValueError(f"scores_at_eligible: extras must be two contiguous ({rows}, {t}, L) fp32 arrays")
    if rows == 0 or t == 0:
        return scores
    with _on_device(scores.device):
        _lib.check(_lib.load().rails_scores_at_eligible(_ptr(scores), ld, rows, t, _ptr(positions.contiguous()), n_items, _ptr(words), stride, _ptr(eff),
                                                        _ptr(allowed), _ptr(inv), width, _ptr(item_ids), _ptr(ea), _ptr(eb), length, _stream()),
                   "rails_scores_at_eligible")
    return scores


# ---- exact ranks of given items (rails_scores_rank_keys, rails_scores_rank, rails_item_mask_clear_rows) ---------------------
RANK_MAX_TARGETS = 64      # targets per row and launch (rails_scores_rank); scores_rank slices wider calls


def _row_mask_words(what: str, mask, scores: torch.Tensor) -> Tuple[Optional[int], int]:
    """The mask argument of the streaming passes over a (rows, n) score matrix -- an ItemMask, or its int32 words with one row for all or one
    per row --, checked against `scores` -> (the words' pointer, their row stride: 0 for a shared row); (None, 0): every item is eligible."""
    rows, n = scores.shape
    if mask is None:
        return None, 0
    if isinstance(mask, ItemMask):
        if mask.n_items != n:
            raise ValueError(f"{what}: {n} columns of scores against a mask of {mask.n_items} items")
        mwords = mask.words
    else:      # the words themselves (what item_mask_clear_rows edits: nobody has counted their bits)
        if not torch.is_tensor(mask) or mask.dtype != torch.int32 or mask.dim() != 2 or mask.shape[1] < item_mask_words(n) or (mask.shape[1] > 1 and mask.stride(1) != 1):
            raise ValueError(f"{what}: mask must be an ItemMask or its (rows, >= {item_mask_words(n)}) int32 words")
        mwords = mask
    if mwords.shape[0] not in (1, rows):
        raise ValueError(f"{what}: the mask has {mwords.shape[0]} rows but scores has {rows}")
    if mwords.device != scores.device:
        raise ValueError(f"{what}: the mask and the scores live on different devices")
    return _ptr(mwords), 0 if mwords.shape[0] == 1 else mwords.stride(0)


def _row_pass_args(what: str, scores: torch.Tensor, mask, temperature: Optional[float] = None):
    """The argument checks of every streaming pass over a score matrix (the rank, softmax and range passes) -> (rows, n, ld, mask words
    pointer, their row stride, beta); a pass without a temperature gives None and gets beta = None."""
    rows, n, ld = _score_matrix(scores)
    beta = None if temperature is None else inv_temperature(temperature, what)
    words, stride = _row_mask_words(what, mask, scores)
    if rows > 0 and n < 1:
        raise ValueError(f"{what}: scores has no columns")
    return rows, n, ld, words, stride, beta


def scores_rank(scores: torch.Tensor, positions: torch.Tensor, mask: Optional[ItemMask] = None) -> torch.Tensor:
    """(rows, t) int64: the rank of position positions[r, j] in row r of `scores` ((rows, n) fp32 with unit column stride) among the items of row
    r's `mask` (None: all of them; an ItemMask, or its int32 words with one row for all or one per row) -- 1 + the number of eligible items whose selection key (score descending, then position ascending, on
    the score's bits) is larger, so rank - 1 is the target's index in the row's exhaustive top-k list.  0: not ranked (a position outside
    [0, n), such as the -1 of an unknown id, or a target outside the mask).  Every score is read once per RANK_MAX_TARGETS targets of its
    row; no sync."""
    rows, n, ld, words, stride, _ = _row_pass_args("scores_rank", scores, mask)
    _positions_arg("scores_rank", positions, rows, scores.device)
    t_all = positions.shape[1]
    out = torch.empty((rows, t_all), dtype=torch.int64, device=scores.device)
    if rows == 0 or t_all == 0:
        return out
    lib = _lib.load()
    with _on_device(scores.device):
        for t0 in range(0, t_all, RANK_MAX_TARGETS):
            pos = positions[:, t0 : t0 + RANK_MAX_TARGETS].contiguous()
            t = pos.shape[1]
            keys = torch.empty((rows, t), dtype=torch.int64, device=scores.device)      # (the 64-bit keys; never read as integers here)
            ranks = torch.empty((rows, t), dtype=torch.int32, device=scores.device)
            _lib.check(lib.rails_scores_rank_keys(_ptr(scores), ld, rows, n, _ptr(pos), t, _ptr(keys), _stream()), "rails_scores_rank_keys")
            _lib.check(lib.rails_scores_rank(_ptr(scores), ld, rows, n, _ptr(keys), t, words, stride, _ptr(ranks), _stream()), "rails_scores_rank")
            out[:, t0 : t0 + t] = ranks
    return out


def item_mask_clear_rows(words: torch.Tensor, positions: torch.Tensor, n_items: Optional[int] = None) -> torch.Tensor:
    """In place: row r of `words` ((rows, >= words of n_items) int32 with unit column stride) loses the bits at positions[r, :] ((rows, m) int64);
    positions outside [0, n_items) -- the -1 of an unknown id -- are skipped, repeats are harmless (rails_item_mask_clear_rows).  n_items
    defaults to every bit of a row.  How a row's seen ids leave its mask; no sync."""
    _require_device(words, "words")
    if words.dim() != 2 or words.dtype != torch.int32 or (words.shape[1] > 1 and words.stride(1) != 1):
        raise ValueError("words must be (rows, words) int32 with contiguous rows")
    rows = words.shape[0]
    n = 32 * words.shape[1] if n_items is None else int(n_items)
    if n < 1 or item_mask_words(n) > words.shape[1]:
        raise ValueError(f"item_mask_clear_rows: rows of {words.shape[1]} words do not hold {n} items")
    _positions_arg("item_mask_clear_rows", positions, rows, words.device, "words", "m")
    if rows == 0 or positions.shape[1] == 0:
        return words
    pos = positions.contiguous()
    with _on_device(words.device):
        _lib.check(_lib.load().rails_item_mask_clear_rows(_ptr(pos), rows, pos.shape[1], n, _ptr(words), score_matrix_ld(rows, words.shape[1], words.stride(0)),
                                                          _stream()), "rails_item_mask_clear_rows")
    return words


# ---- softmax over the corpus (rails_scores_lse, rails_scores_log_prob, rails_scores_gumbel) ---------------------------------
def inv_temperature(temperature: float, what: str = "temperature") -> float:
    """beta = fp32(1 / temperature) as the Python float that holds it; ValueError unless temperature is a finite number > 0 whose inverse is
    a finite fp32 > 0."""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError(f"{what}: temperature must be a finite number > 0, got {temperature!r}")
    beta = C.c_float(1.0 / temperature).value      # (one rounding to nearest: numpy.float32(1.0 / temperature))
    if not math.isfinite(beta) or beta <= 0:
        raise ValueError(f"{what}: 1 / temperature is not a finite fp32 > 0 for temperature = {temperature!r}")
    return beta


def scores_lse(scores: torch.Tensor, mask: Optional[ItemMask] = None, temperature: float = 1.0) -> torch.Tensor:
    """(rows,) fp32: log sum exp(scores[r, x] / temperature) over the items x of row r's `mask` (as scores_rank takes it; None: all of them)
    -- the normaliser of softmax(scores / temperature) over what the row may return (rails_scores_lse: two reads of the matrix, the same
    bits on every run).  -inf for a row with nothing eligible (or -inf alone), NaN with an eligible NaN, otherwise +inf with an eligible
    +inf.  No sync."""
    rows, n, ld, words, stride, beta = _row_pass_args("scores_lse", scores, mask, temperature)
    out = torch.empty((rows,), dtype=torch.float32, device=scores.device)
    if rows == 0:
        return out
    lib = _lib.load()
    need = int(lib.rails_scores_lse_workspace_bytes(rows, n))
    ws = torch.empty(need, dtype=torch.uint8, device=scores.device)
    with _on_device(scores.device):
        _lib.check(lib.rails_scores_lse(_ptr(scores), ld, rows, n, beta, words, stride, _ptr(ws), need, _ptr(out), _stream()), "rails_scores_lse")
    return out


def scores_log_prob(scores: torch.Tensor, positions: torch.Tensor, lse: torch.Tensor, mask: Optional[ItemMask] = None,
                    temperature: float = 1.0) -> torch.Tensor:
    """(rows, t) fp32: fl32(fl32(scores[r, p] / temperature) - lse[r]) for p = positions[r, j] -- the log-probability of item p under the
    softmax whose normaliser scores_lse gave for the same mask and temperature --, -inf for a position outside [0, n) or outside row r's
    `mask` (rails_scores_log_prob).  No sync."""
    rows, n, ld, words, stride, beta = _row_pass_args("scores_log_prob", scores, mask, temperature)
    _positions_arg("scores_log_prob", positions, rows, scores.device)
    lse = _lse_arg("scores_log_prob", lse, rows, scores.device)
    t = positions.shape[1]
    out = torch.empty((rows, t), dtype=torch.float32, device=scores.device)
    if rows == 0 or t == 0:
        return out
    pos = positions.contiguous()
    with _on_device(scores.device):
        _lib.check(_lib.load().rails_scores_log_prob(_ptr(scores), ld, rows, n, _ptr(pos), t, beta, _ptr(lse), words, stride, _ptr(out), _stream()),
                   "rails_scores_log_prob")
    return out


def scores_gumbel(scores: torch.Tensor, seed: int, first_row: int = 0, mask: Optional[ItemMask] = None, temperature: float = 1.0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(rows, n) fp32, out of place: scores / temperature + Gumbel noise on the items of row r's `mask`, -inf on the others
    (rails_scores_gumbel).  The top-k of a perturbed row draws k items without replacement from softmax(scores / temperature) over the
    row's eligible items, in draw order.  The noise is a function of (seed, first_row + r, column) alone -- Philox4x32-10 --: slicing a batch
    and passing each slice's first row reproduces the unsliced call.  seed: an int in [0, 2^64).  out: a (rows, n) fp32 tensor with
    contiguous rows that does not overlap `scores`.  No sync."""
    rows, n, ld, words, stride, beta = _row_pass_args("scores_gumbel", scores, mask, temperature)
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"scores_gumbel: seed must be an int in [0, 2^64), got {seed!r}")
    if isinstance(first_row, bool) or not isinstance(first_row, int) or not 0 <= first_row < 1 << 62:
        raise ValueError(f"scores_gumbel: first_row must be an int >= 0, got {first_row!r}")
    refused = f"scores_gumbel: out must be a ({rows}, {n}) fp32 tensor with contiguous rows on the scores' device"
    if out is None:
        out = torch.empty((rows, n), dtype=torch.float32, device=scores.device)
    elif not torch.is_tensor(out) or out.shape != (rows, n) or out.device != scores.device or (rows > 1 and out.stride(0) < n):      # (rows that are written do not overlap)
        raise ValueError(refused)
    out_ld = _score_matrix(out, "out", refused)[2]
    if rows == 0:
        return out
    with _on_device(scores.device):
        _lib.check(_lib.load().rails_scores_gumbel(_ptr(scores), ld, rows, n, beta, seed, first_row, words, stride, _ptr(out), out_ld, _stream()),
                   "rails_scores_gumbel")
    return out


# ---- item tags (rails_item_tags_*, rails_item_mask_from_tags, rails_scores_mask_tags) ---------------------
# ---- range search over a score matrix (rails_scores_range_count / _write / _sort / _decode) ------------------------------
def range_thresholds(what: str, thresholds, rows: int, device) -> torch.Tensor:
    """A call's threshold(s) -> (rows,) fp32 on `device`, converted to fp32 once, on the host side of the call: a Python number for every row
    (NaN and +-inf included), or a (rows,) tensor of a real dtype."""
    if torch.is_tensor(thresholds):
        if thresholds.shape != (rows,) or thresholds.dtype == torch.bool or thresholds.is_complex():
            raise ValueError(f"{what}: a threshold tensor must be ({rows},) real numbers, got {tuple(thresholds.shape)} {thresholds.dtype}")
        return thresholds.to(device=device, dtype=torch.float32).contiguous()
    if isinstance(thresholds, bool) or not isinstance(thresholds, (int, float)):
        raise ValueError(f"{what}: the threshold must be a number or a ({rows},) tensor, got {thresholds!r}")
    return torch.full((rows,), C.c_float(float(thresholds)).value, dtype=torch.float32, device=device)


def _range_count(what: str, scores: torch.Tensor, thresholds, mask, temperature: float, lse: Optional[torch.Tensor]):
    """The checks and the counting pass of scores_range_count / scores_range -> (the write pass' leading arguments, the tensors behind them,
    counts, lims).  The caller of the write pass holds on to the tensors until it has launched: the workspace carries the slots' counts and
    offsets from one pass to the other, and a freed block would be handed to the next allocation."""
    rows, n, ld, words, stride, beta = _row_pass_args(what, scores, mask, temperature)
    if lse is None and beta != 1.0:
        raise ValueError(f"{what}: temperature = {temperature!r} without lse: a score threshold is compared with the raw score")
    if lse is not None:
        lse = _lse_arg(what, lse, rows, scores.device)
    thr = range_thresholds(what, thresholds, rows, scores.device)
    counts = torch.empty((rows,), dtype=torch.int64, device=scores.device)
    lims = torch.zeros((rows + 1,), dtype=torch.int64, device=scores.device)
    if rows == 0:
        return None, None, counts, lims
    lib = _lib.load()
    need = int(lib.rails_scores_range_workspace_bytes(rows, n))
    ws = torch.empty(need, dtype=torch.uint8, device=scores.device)
    args = (_ptr(scores), ld, rows, n, _ptr(thr), beta, _ptr(lse), words, stride, _ptr(ws), need)
    with _on_device(scores.device):
        _lib.check(lib.rails_scores_range_count(*args, _ptr(counts), _ptr(lims), _stream()), "rails_scores_range_count")
    return args, (ws, thr, lse, scores), counts, lims


def scores_range_count(scores: torch.Tensor, thresholds, mask: Optional[ItemMask] = None, temperature: float = 1.0,
                       lse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(rows,) int64: how many items of row r's `mask` (as scores_rank takes it; None: all of them) have v >= thresholds[r], an IEEE fp32
    compare (false with a NaN on either side) -- v = scores[r, x] without `lse`, v = fl32(fl32(scores[r, x] / temperature) - lse[r]) with it
    (scores_log_prob's value for the lse scores_lse gave).  thresholds: a number or a (rows,) tensor.  One read of the matrix; no sync."""
    return _range_count("scores_range_count", scores, thresholds, mask, temperature, lse)[2]


def scores_range(scores: torch.Tensor, thresholds, mask: Optional[ItemMask] = None, temperature: float = 1.0, lse: Optional[torch.Tensor] = None,
                 ids: Optional[torch.Tensor] = None, sort: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(lims (rows + 1,) int64, scores (lims[rows],) fp32, ids (lims[rows],) int64): the items scores_range_count counts, row r's in
    [lims[r], lims[r + 1]) -- the raw scores' bits and ids[position] (the positions themselves without `ids`, a (>= n,) int64 table).
    sort=True: a row in selection-key order (score descending, then position ascending, on the bits), that is the row's exhaustive top-k
    list without the items that miss; a row of more than RANGE_SORT_MAX hits raises ValueError after the count, before anything is written.
    sort=False: position ascending, any count.  Two reads of the matrix, no atomics: the same bits on every run.  ONE sync: lims is read
    back to size the result."""
    if ids is not None:
        if not torch.is_tensor(ids) or ids.dtype != torch.int64 or ids.dim() != 1 or ids.shape[0] < scores.shape[-1] or ids.device != scores.device:
            raise ValueError("scores_range: ids must be a (>= n,) int64 table on the scores' device")
        ids = ids.contiguous()
    args, held, _, lims = _range_count("scores_range", scores, thresholds, mask, temperature, lse)
    rows, dev = scores.shape[0], scores.device
    host = lims.cpu()      # (the call's one sync)
    total = int(host[rows])
    most = int((host[1:] - host[:-1]).max()) if rows > 0 else 0
    if sort and most > RANGE_SORT_MAX:
        row = int(torch.nonzero(host[1:] - host[:-1] == most)[0])      # (the first such row)
        raise ValueError(f"scores_range: row {row} has {most} hits, more than the {RANGE_SORT_MAX} one sorted row takes; "
                         "raise the threshold or call with sort=False (position order, any count)")
    out_scores = torch.empty((total,), dtype=torch.float32, device=dev)
    out_ids = torch.empty((total,), dtype=torch.int64, device=dev)
    if total == 0:
        return lims, out_scores, out_ids
    lib = _lib.load()
    keys = torch.empty((total,), dtype=torch.int64, device=dev)      # (the 64-bit keys; never read as integers here)
    with _on_device(dev):
        _lib.check(lib.rails_scores_range_write(*args, _ptr(keys), total, _stream()), "rails_scores_range_write")
        if sort:
            _lib.check(lib.rails_scores_range_sort(_ptr(keys), _ptr(lims), rows, most, _stream()), "rails_scores_range_sort")
        _lib.check(lib.rails_scores_range_decode(_ptr(keys), total, _ptr(ids), scores.shape[1], _ptr(out_scores), _ptr(out_ids), _stream()),
                   "rails_scores_range_decode")
    del held
    return lims, out_scores, out_ids


# ---- query fusion: several sub-query rows per fused row (rails_scores_fuse_rows, rails_topk_fuse_lists) -------------------
FUSE_MODES = {"max": _lib.RAILS_FUSE_MAX, "sum": _lib.RAILS_FUSE_SUM}
FUSE_LIST_MAX_ENTRIES = 16384      # (score, position) entries of one fused row rails_topk_fuse_lists merges
FUSE_LIST_MAX_K = 512
FUSE_LIST_MAX_SEEN = 4096


def parse_query_lims(lims, rows: int, what: str = "query_lims") -> torch.Tensor:
    """query_lims= as given -> the (U + 1,) int64 tensor on the CPU (the ONE read of a device tensor), checked: FAISS-shaped like
    range_search's lims, lims[0] = 0, lims[U] = rows, strictly increasing.  ValueError names what is wrong."""
    if not torch.is_tensor(lims) or lims.dtype != torch.int64 or lims.dim() != 1 or lims.numel() < 2:
        raise ValueError(f"{what}: query_lims must be a (U + 1,) int64 tensor with U >= 1")
    host = lims.detach().cpu().contiguous()
    if int(host[0]) != 0:
        raise ValueError(f"{what}: query_lims[0] must be 0, got {int(host[0])}")
    if int(host[-1]) != rows:
        raise ValueError(f"{what}: query_lims[U] = {int(host[-1])} but there are {rows} sub-query rows")
    sizes = host[1:] - host[:-1]
    if bool((sizes < 1).any()):
        u = int(torch.nonzero(sizes < 1)[0])
        raise ValueError(f"{what}: query_lims must increase strictly: segment {u} = [{int(host[u])}, {int(host[u + 1])}) is empty")
    return host


class QueryLims:
    """A checked query_lims: `host` (U + 1,) on the CPU, `dev` the same on the device of the scores, fused rows U, sub-query rows S and the
    largest segment.  Built once per call (parse_query_lims' one read); slices of whole segments are cut from the host copy."""

    def __init__(self, lims, rows: int, device, what: str = "query_lims"):
        self.host = parse_query_lims(lims, rows, what)
        self.dev = lims if lims.device == torch.device(device) and lims.is_contiguous() else self.host.to(device)
        self.fused, self.rows = self.host.numel() - 1, rows
        self.max_segment = int((self.host[1:] - self.host[:-1]).max())
        self._rows_of = None

    def rows_slice(self, u0: int, u1: int) -> "QueryLims":
        """The fused rows u0 .. u1 - 1 as a QueryLims of their own over the sub-query rows [host[u0], host[u1])."""
        if u0 == 0 and u1 == self.fused:
            return self
        host = self.host[u0 : u1 + 1] - self.host[u0]
        return QueryLims(host.to(self.dev.device), int(host[-1]), self.dev.device)

    def fused_row_of(self) -> torch.Tensor:
        """(S,) int64 on the CPU: the fused row of every sub-query row (what repeats a per-fused-row argument over its segment)."""
        if self._rows_of is None:
            self._rows_of = torch.repeat_interleave(torch.arange(self.fused, dtype=torch.int64), self.host[1:] - self.host[:-1])
        return self._rows_of


def _query_lims_arg(what: str, lims, rows: int, device) -> QueryLims:
    ql = lims if isinstance(lims, QueryLims) else QueryLims(lims, rows, device, what)
    if ql.rows != rows:
        raise ValueError(f"{what}: query_lims[U] = {ql.rows} but there are {rows} sub-query rows")
    if ql.dev.device != device:
        raise ValueError(f"{what}: the query_lims and the scores live on different devices")
    return ql


def scores_fuse_rows(scores: torch.Tensor, lims, mode: str = "max", weights: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                     run_if: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(U, n) fp32, out of place: row u is the fusion of the rows [lims[u], lims[u + 1]) of `scores` ((S, n) fp32 with unit column stride), taken
    ascending (rails_scores_fuse_rows).  mode "max": per column the element that is largest in the selection key's order (on the bits: +-0,
    +-inf and NaNs as topk ranks them); "sum": acc = s[r0], acc = fl32(acc + s[r]), or with `weights` ((S,) fp32) acc = fl32(w[r0] * s[r0]),
    acc = fl32(acc + fl32(w[r] * s[r])) -- no fma, a numpy float32 loop gives the same bits.  lims: a (U + 1,) int64 tensor (checked on the
    host: one read) or a QueryLims.  out: a (U, n) fp32 tensor with contiguous rows that does not overlap `scores`.  One read of every score,
    one write of every result; no sync beyond the read of lims."""
    rows, n, ld = _score_matrix(scores)
    if mode not in FUSE_MODES:
        raise ValueError(f"scores_fuse_rows: fuse must be one of {sorted(FUSE_MODES)}, got {mode!r}")
    if weights is not None:
        if mode != "sum":
            raise ValueError('scores_fuse_rows: query_weights go with fuse="sum"')
        if not torch.is_tensor(weights) or weights.dtype != torch.float32 or weights.shape != (rows,) or weights.device != scores.device:
            raise ValueError(f"scores_fuse_rows: query_weights must be ({rows},) fp32 on the scores' device")
        weights = weights.contiguous()
    ql = _query_lims_arg("scores_fuse_rows", lims, rows, scores.device)
    if n < 1:
        raise ValueError("scores_fuse_rows: scores has no columns")
    refused = f"scores_fuse_rows: out must be a ({ql.fused}, {n}) fp32 tensor with contiguous rows on the scores' device"
    if out is None:
        out = torch.empty((ql.fused, n), dtype=torch.float32, device=scores.device)
    elif not torch.is_tensor(out) or out.shape != (ql.fused, n) or out.device != scores.device or (ql.fused > 1 and out.stride(0) < n):
        raise ValueError(refused)
    out_ld = _score_matrix(out, "out", refused)[2]
    with _on_device(scores.device):
        _lib.check(_lib.load().rails_scores_fuse_rows(_ptr(scores), ld, rows, n, _ptr(ql.dev), ql.fused, FUSE_MODES[mode], _ptr(weights), _ptr(out), out_ld,
                                                      _pred(run_if), _stream()), "rails_scores_fuse_rows")
    return out


def topk_fuse_lists_supported(max_segment: int, depth: int, k: int, width: int, n_items: int) -> bool:
    """Whether rails_topk_fuse_lists takes these sizes (RAILS_ENOTSUP otherwise)."""
    return max_segment * depth <= FUSE_LIST_MAX_ENTRIES and k <= FUSE_LIST_MAX_K and width <= FUSE_LIST_MAX_SEEN and n_items <= (1 << 32) - 1


def topk_fuse_lists(scores: torch.Tensor, positions: torch.Tensor, lims, k: int, ids: Optional[torch.Tensor], invalid_ids: Optional[torch.Tensor] = None,
                    n_items: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The top k of the "max" fusion from sorted lists (rails_topk_fuse_lists): scores / positions (S, D) -- row r's top-D list in selection-key
    order, positions int64, a short list padded with (-inf, anything) or (anything, -1) -- -> (ids (U, k) int64, scores (U, k) fp32), ids
    first like filter_seen_ids: per fused row the best entry of every position, ranked by the selection key (score descending, then position
    ascending), without the entries whose id (ids[position]; the position itself when ids is None) is among invalid_ids[u] ((U, w)); a
    short row ends in (-1, -inf).  n_items: positions outside [0, n_items) are skipped (default: the length of `ids`).  NotImplementedError
    (nothing launched) beyond FUSE_LIST_MAX_ENTRIES entries per fused row, FUSE_LIST_MAX_K or FUSE_LIST_MAX_SEEN."""
    rows, depth, ld = _score_matrix(scores)
    _positions_arg("topk_fuse_lists", positions, rows, scores.device, t="D")
    if positions.shape[1] != depth:
        raise ValueError("topk_fuse_lists: positions must be (S, D) like scores")
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"topk_fuse_lists: k must be an int >= 1, got {k!r}")
    ql = _query_lims_arg("topk_fuse_lists", lims, rows, scores.device)
    if ids is not None:
        ids = ids.to(device=scores.device, dtype=torch.int64).reshape(-1).contiguous()
    if n_items is None:
        if ids is None:
            raise ValueError("topk_fuse_lists: n_items is needed where there is no ids table")
        n_items = ids.numel()
    if ids is not None and ids.numel() < n_items:
        raise ValueError("topk_fuse_lists: ids has fewer entries than n_items")
    inv, width = _seen_arg(invalid_ids, ql.fused, scores.device)
    out_i = torch.empty((ql.fused, k), dtype=torch.int64, device=scores.device)
    out_s = torch.empty((ql.fused, k), dtype=torch.float32, device=scores.device)
    pos = positions.contiguous()
    with _on_device(scores.device):
        _lib.check(_lib.load().rails_topk_fuse_lists(_ptr(scores), ld, _ptr(pos), rows, depth, _ptr(ql.dev), ql.fused, ql.max_segment, int(n_items), _ptr(ids),
                                                     _ptr(inv), width, k, _ptr(out_i), _ptr(out_s), _stream()), "rails_topk_fuse_lists")
    return out_i, out_s


def lists_union(positions: torch.Tensor, lims, n_items: int, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The union of candidate lists per fused row (rails_lists_union): positions (S, W) int64 with unit column stride -- row r's candidate
    positions, in any order, duplicates allowed -- -> (union (U, W_out) int64, counts (U,) int32): row u holds the distinct positions of its
    segment inside [0, n_items) ascending, -1 behind them.  out: a contiguous (U, W_out) int64 tensor, W_out >= max_segment * W (default:
    exactly that).  One launch; no sync beyond the read of lims.  NotImplementedError (nothing launched) beyond FUSE_LIST_MAX_ENTRIES entries
    per fused row or positions beyond 2^32 - 2."""
    if not torch.is_tensor(positions) or positions.dim() != 2 or positions.shape[1] < 1 or (positions.shape[1] > 1 and positions.stride(1) != 1):
        raise ValueError("lists_union: positions must be (S, W) int64 with W >= 1 and contiguous rows")
    _require_device(positions, "positions")
    rows, width = positions.shape
    _positions_arg("lists_union", positions, rows, positions.device, beside="query_lims", t="W")
    ql = _query_lims_arg("lists_union", lims, rows, positions.device)
    entries = ql.max_segment * width
    if entries > FUSE_LIST_MAX_ENTRIES or n_items > (1 << 32) - 1:
        raise NotImplementedError(f"lists_union: a fused row of {ql.max_segment} sub-query rows x {width} candidates = {entries} entries, {n_items} items: "
                                  f"one workgroup sorts up to {FUSE_LIST_MAX_ENTRIES} entries with positions up to 2^32 - 2")
    if out is None:
        out = torch.empty((ql.fused, entries), dtype=torch.int64, device=positions.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != ql.fused or out.shape[1] < entries
          or out.device != positions.device or not out.is_contiguous()):
        raise ValueError(f"lists_union: out must be a contiguous ({ql.fused}, >= {entries}) int64 tensor on the positions' device")
    counts = torch.empty((ql.fused,), dtype=torch.int32, device=positions.device)
    ld = score_matrix_ld(rows, width, positions.stride(0))
    with _on_device(positions.device):
        _lib.check(_lib.load().rails_lists_union(_ptr(positions), ld, rows, width, _ptr(ql.dev), ql.fused, ql.max_segment, int(n_items), _ptr(out), out.shape[1],
                                                 _ptr(counts), _stream()), "rails_lists_union")
    return out, counts


def tag_word_i32(word: int) -> int:
    """A 32-bit tag word as the int32 that holds its bit pattern."""
    return word - (1 << 32) if word >= 1 << 31 else word


def item_tags_effective(tags: torch.Tensor, visible_words: torch.Tensor, n_items: int) -> torch.Tensor:
    """(N,) int32: tags[i] where bit i of the visibility row is set, 0 where the item is hidden (rails_item_tags_effective) -- the one array
    every tag kernel reads: a hidden item is an item that carries no attribute."""
    eff = torch.empty_like(tags)
    with _on_device(tags.device):
        _lib.check(_lib.load().rails_item_tags_effective(_ptr(tags), _ptr(visible_words), n_items, _ptr(eff), _stream()), "rails_item_tags_effective")
    return eff


def item_tags_counts(eff: torch.Tensor, words: Sequence[int]) -> List[int]:
    """How many items each allow word keeps: counts[j] = #{i : eff[i] & words[j] != 0} (rails_item_tags_count: one launch, ONE read-back)."""
    w = torch.tensor([tag_word_i32(int(v)) for v in words], dtype=torch.int32).to(eff.device)
    counts = torch.empty(len(words), dtype=torch.int32, device=eff.device)
    with _on_device(eff.device):
        _lib.check(_lib.load().rails_item_tags_count(_ptr(eff), eff.numel(), _ptr(w), len(words), _ptr(counts), _stream()), "rails_item_tags_count")
    return [int(c) for c in counts.cpu()]


TAGGED_COMPONENT_ROWS = 128      # query rows (B * P_Q) one rails_mol_component_topk_tagged call takes: four row tiles of running maxima


def scan_plan(rows: int, n_items: int, k: int, comp_rows: int = 0) -> Optional[Tuple[int, int, int, int]]:
    """(stride, r, G, s) of the plan behind the fused coarse top-K' (comp_rows = 0, rows = B) or the fused component top-k (rows = B * P_Q * P_X,
    comp_rows = B * P_Q): every stride-th tile is sampled, the threshold is the r-th largest of G group maxima of about s sampled items each
    (rails_mol_scan_plan; host arithmetic, no device).  None where the sizes have no plan."""
    out = (C.c_int32 * 4)()
    if not _lib.load().rails_mol_scan_plan(int(rows), int(n_items), int(k), int(comp_rows), out):
        return None
    return tuple(int(v) for v in out)


def _check_tag_filter(tags, n_items: int, batch: int, device: torch.device, visible) -> None:
    """The filter a tagged scan reads: the effective tags of exactly n_items items on the table's device, one allow word for the batch or one per
    row, and no visibility row beside it -- checked before any launch."""
    if tags is None:
        return
    if not isinstance(tags, TagFilter) or tags.n_items != n_items or tags.eff.device != device or tags.rows not in (1, batch):
        raise ValueError(f"tags must be a TagFilter over the {n_items} items on {device} with 1 or {batch} allow words")
    if visible is not None:
        raise ValueError("tags and visible in one call: the filter's effective tags already hold the hidden set")


class TagFilter:
    """allowed_tags= of one call, resolved against a module's tags: `words` (one allow word shared by the batch, or one per query row, host
    integers), `kept` (how many items each row may return, host integers), `eff` (the module's effective tags, (N,) int32) and `allowed` (the
    words as int32 on the device).  Row b may return item x iff eff[x] & words[b] != 0.  Built by the module, which caches it per tuple of
    words: a repeated filter costs a call neither a copy nor a sync."""

    def __init__(self, eff: torch.Tensor, words: Tuple[int, ...], kept: Tuple[int, ...], allowed: Optional[torch.Tensor] = None, stamp=None):
        self.eff, self.words, self.kept, self.stamp = eff, tuple(words), tuple(kept), stamp
        self.n_items = eff.numel()
        self.rows = len(self.words)
        self.kept_min = min(self.kept)
        self.allowed = allowed if allowed is not None else torch.tensor([tag_word_i32(w) for w in self.words], dtype=torch.int32).to(eff.device)
        self._mask: Optional[ItemMask] = None
        self._per_row: Optional[torch.Tensor] = None

    def allowed_for(self, batch: int) -> torch.Tensor:
        """The allow words as one int32 per query row of a batch (what the tagged scans read); a shared word is repeated, kept for the last batch size."""
        if self.rows == batch:
            return self.allowed
        c = self._per_row
        if c is None or c.numel() != batch:
            c = self._per_row = self.allowed.expand(batch).contiguous()
        return c

    def rows_slice(self, b0: int, b1: int) -> "TagFilter":
        """The filter of the batch rows b0 .. b1 - 1; a shared word is its own slice."""
        if self.rows == 1:
            return self
        return TagFilter(self.eff, self.words[b0:b1], self.kept[b0:b1], self.allowed[b0:b1], self.stamp)

    def item_mask(self) -> ItemMask:
        """The filter as an ItemMask (rails_item_mask_from_tags: a shared row for one word, else one row per query row) -- what the exact
        modules' masked strategies take.  No sync (the counts are the filter's).  A SHARED word's mask (N / 8 bytes) is built at first use and kept
        with the filter; a per-row filter's (B N / 8 bytes: 500 MB per batch of 32 on a 125 M-item shard, times the filters a module caches) is
        built for the call and let go -- a caller with one steady per-row filter on a large corpus keeps an ItemMask and passes item_mask=."""
        if self._mask is not None:
            return self._mask
        n = self.n_items
        words = torch.empty((self.rows, item_mask_words(n)), dtype=torch.int32, device=self.eff.device)
        counts = torch.empty(self.rows, dtype=torch.int32, device=self.eff.device)
        with _on_device(self.eff.device):
            _lib.check(_lib.load().rails_item_mask_from_tags(_ptr(self.eff), n, _ptr(self.allowed), self.rows, _ptr(words), _ptr(counts), _stream()),
                       "rails_item_mask_from_tags")
        m = ItemMask.__new__(ItemMask)
        m._init(words, counts, n, self.rows == 1, torch.tensor(self.kept, dtype=torch.int32))
        if self.rows == 1:
            self._mask = m
        return m


def scores_mask_tags(scores: torch.Tensor, filt: TagFilter, first_item: int = 0, fill: float = float("-inf"),
                     run_if: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place: scores[r, x] = fill wherever item first_item + x carries no bit of the allow word of row r's query (rails_scores_mask_tags); kept
    entries are neither read nor written.  scores (rows, n) fp32 with unit column stride, rows a multiple of the filter's rows: consecutive
    blocks of rows / filt.rows rows share an allow word (the component matrix has P_Q * P_X rows per query; a shared word covers every row)."""
    rows, n, ld = _score_matrix(scores)
    if first_item < 0 or first_item + n > filt.n_items:
        raise ValueError(f"scores_mask_tags: items [{first_item}, {first_item + n}) are not inside the {filt.n_items} tagged items")
    if rows % filt.rows:
        raise ValueError(f"scores_mask_tags: {rows} rows of scores against {filt.rows} allow words")
    if filt.eff.device != scores.device:
        raise ValueError("scores_mask_tags: the tags and the scores live on different devices")
    with _on_device(scores.device):
        _lib.check(_lib.load().rails_scores_mask_tags(_ptr(scores), ld, rows, n, first_item,
                                                      _ptr(filt.eff), _ptr(filt.allowed), rows // filt.rows, float(fill), _pred(run_if), _stream()),
                   "rails_scores_mask_tags")
    return scores


def dot_rowwise(q: torch.Tensor, items: torch.Tensor) -> torch.Tensor:
    """q (Bq, D), items (B_I, X, D) with Bq a multiple of B_I -> (Bq, X): <q[bq], items[bq // r][x]>."""
    lib = _lib.load()
    _require_device(q, "query_embeddings")
    q, items = _f32c(q), _f32c(items)
    Bq, D = q.shape
    BI, X, _ = items.shape
    out = torch.empty((Bq, X), dtype=torch.float32, device=q.device)
    with _on_device(q.device):
        _lib.check(lib.rails_dot_rowwise(_ptr(q), _ptr(items), Bq, X, D, Bq // BI, _ptr(out), _stream()), "rails_dot_rowwise")
    return out


# ---- shape-independent kernels ----------------------------------------------------------------
def _pred(flag: Optional[torch.Tensor]):
    """Launch predicate argument (include/rails_amd.h `run_if`): None, or an int32 device scalar read by the kernels when they start."""
    if flag is None:
        return None
    if flag.dtype != torch.int32 or not flag.is_cuda or flag.numel() < 1:
        raise ValueError("the launch predicate is an int32 device tensor")
    return _ptr(flag)


TOPK_MAX_K = 16384      # the largest k rails_topk takes (the 64-bit keys one workgroup sorts in LDS)
RANGE_SORT_MAX = TOPK_MAX_K      # hits of one row rails_scores_range_sort takes: the same sort


def topk(scores: torch.Tensor, k: int, ids: Optional[torch.Tensor] = None, sorted: bool = True,
         workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
         run_if: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact top-k of every row of `scores` (rows, n) fp32 on the GPU; ties by position ascending.
    ids: None -> positions; (n,) or (1, n) -> shared id row; (rows, n) -> per-row ids.
    Replaces torch.topk + id gather (reference rails/indexing/mol_top_k.py:123-130)."""
    lib = _lib.load()
    _require_device(scores, "scores")
    if scores.dim() != 2:
        raise ValueError("scores must be (rows, n)")
    if scores.dtype != torch.float32 or scores.stride(1) != 1:
        scores = _f32c(scores)
    rows, n = scores.shape
    if k > n:
        raise RuntimeError(f"selected index k out of range (k={k}, n={n})")  # what torch.topk raises
    stride = 0
    if ids is not None:
        if ids.dtype != torch.int64 or ids.device != scores.device:
            ids = ids.to(device=scores.device, dtype=torch.int64)
        if ids.dim() == 2 and ids.shape[0] == rows and rows > 1:
            ids = ids.contiguous()
            stride = ids.shape[1]
        else:
            ids = ids.reshape(-1).contiguous()
        if ids.shape[-1] < n:
            raise ValueError("ids has fewer entries than scores has columns")
    if out is not None:      # (rows, k) fp32 / int64, contiguous: overwritten (the predicated fallback of the verified modes)
        out_s, out_i = out
        if out_s.shape != (rows, k) or out_i.shape != (rows, k) or out_s.dtype != torch.float32 or out_i.dtype != torch.int64 or not (out_s.is_contiguous() and out_i.is_contiguous()):
            raise ValueError("topk: out must be contiguous (rows, k) fp32 and int64 tensors")
    else:
        out_s = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
        out_i = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    ws_bytes = lib.rails_topk_workspace_bytes(rows, n, k)
    ws = workspace if workspace is not None and workspace.numel() >= ws_bytes and workspace.device == scores.device else torch.empty(ws_bytes, dtype=torch.uint8, device=scores.device)
    with _on_device(scores.device):
        _lib.check(
            lib.rails_topk(_ptr(scores), scores.stride(0), rows, n, k, 1 if sorted else 0, _ptr(ids), stride, _ptr(out_s), _ptr(out_i), _ptr(ws), ws_bytes, _pred(run_if), _stream()),
            "rails_topk",
        )
    return out_s, out_i


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, silu: bool = False) -> torch.Tensor:
    """act(x @ weight.T + bias) for 2-D fp32 x on the GPU through rails_gemm_f32 (fp32 MFMA); `weight` is a torch Linear weight (N, K)."""
    lib = _lib.load()
    _require_device(x, "x")
    x, weight = _f32c(x), _f32c(weight.detach())
    bias = None if bias is None else _f32c(bias.detach())
    M, K = x.shape
    N = weight.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    with _on_device(x.device):
        _lib.check(lib.rails_gemm_f32(_ptr(x), K, _ptr(weight), 1, _ptr(bias), None, 0, M, N, K, 1 if silu else 0, None, 0, _ptr(out), N, _stream()), "rails_gemm_f32")
    return out


def gate_combine(logits: torch.Tensor, pair_part: Optional[torch.Tensor], query_part: Optional[torch.Tensor], item_part: Optional[torch.Tensor],
                 items_per_query: int, item_part_per_row: bool, glu_silu: bool, renormalise: bool, eps: float,
                 want_probs: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """rails_mol_gate_combine: logits / pair_part (rows, L), query_part (rows / X, L), item_part (X or rows, L) -> (out (rows,), pi or None)."""
    lib = _lib.load()
    _require_device(logits, "logits")
    logits = _f32c(logits)
    rows, L = logits.shape
    pair_part = None if pair_part is None else _f32c(pair_part)
    query_part = None if query_part is None else _f32c(query_part)
    item_part = None if item_part is None else _f32c(item_part)
    out = torch.empty((rows,), dtype=torch.float32, device=logits.device)
    probs = torch.empty((rows, L), dtype=torch.float32, device=logits.device) if want_probs else None
    with _on_device(logits.device):
        _lib.check(lib.rails_mol_gate_combine(_ptr(logits), L, _ptr(pair_part), L, _ptr(query_part), _ptr(item_part), rows, items_per_query, L,
                                              1 if item_part_per_row else 0, _lib.RAILS_COMBINE_GLU_SILU if glu_silu else _lib.RAILS_COMBINE_NONE,
                                              1 if renormalise else 0, float(eps), _ptr(out), _ptr(probs), _stream()), "rails_mol_gate_combine")
    return out, probs


def topk_candidates(scores: torch.Tensor, k: int, positions: torch.Tensor, ids: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The final_topk of a candidate rerank in one launch (include/rails_amd.h rails_topk_candidates; reference
    rails/indexing/mol_top_k.py:371-382): top-k of every row of `scores` (rows, n_cand); the id of candidate j of row b is
    ids[positions[b, j]] (ids: the module's flat id row), or positions[b, j] itself without ids."""
    lib = _lib.load()
    _require_device(scores, "scores")
    if scores.dtype != torch.float32 or scores.stride(1) != 1:
        scores = _f32c(scores)
    rows, n = scores.shape
    if k > n:
        raise RuntimeError(f"selected index k out of range (k={k}, n={n})")
    positions = positions.to(device=scores.device, dtype=torch.int64).contiguous()
    if positions.shape != (rows, n):
        raise ValueError("positions must be (rows, n_cand) like scores")
    if ids is not None:
        ids = ids.to(device=scores.device, dtype=torch.int64).reshape(-1).contiguous()
    out_s = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    with _on_device(scores.device):
        _lib.check(lib.rails_topk_candidates(_ptr(scores), scores.stride(0), rows, n, k, _ptr(positions), _ptr(ids), _ptr(out_s), _ptr(out_i), _stream()),
                   "rails_topk_candidates")
    return out_s, out_i


def topk_candidates_filterable(n_cand: int, k_prime: int, width: int, k: int) -> bool:
    """sizes rails_topk_candidates_filtered takes (include/rails_amd.h)"""
    return 1024 < n_cand <= 8192 and 0 < k <= k_prime <= min(n_cand, 512) and 0 <= width <= 256


def topk_candidates_filtered(scores: torch.Tensor, k_prime: int, positions: torch.Tensor, ids: Optional[torch.Tensor], invalid_ids: torch.Tensor,
                             k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """topk_candidates(scores, k_prime, positions, ids) followed by filter_seen_ids(..., invalid_ids, k) in one launch (include/rails_amd.h
    rails_topk_candidates_filtered; reference indexing/candidate_index.py:149-175 over a candidate rerank's output).  -> (out_ids (rows, k),
    out_scores (rows, k)), ids first like filter_seen_ids."""
    lib = _lib.load()
    _require_device(scores, "scores")
    if scores.dtype != torch.float32 or scores.stride(1) != 1:
        scores = _f32c(scores)
    rows, n = scores.shape
    positions = positions.to(device=scores.device, dtype=torch.int64).contiguous()
    if positions.shape != (rows, n):
        raise ValueError("positions must be (rows, n_cand) like scores")
    if ids is not None:
        ids = ids.to(device=scores.device, dtype=torch.int64).reshape(-1).contiguous()
    inv = invalid_ids.to(device=scores.device, dtype=torch.int64).contiguous()
    if inv.dim() != 2 or inv.shape[0] != rows:
        raise ValueError("invalid_ids must be (rows, width)")
    out_i = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    out_s = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
    with _on_device(scores.device):
        _lib.check(lib.rails_topk_candidates_filtered(_ptr(scores), scores.stride(0), rows, n, k_prime, _ptr(positions), _ptr(ids), _ptr(inv), inv.shape[1], k,
                                                      _ptr(out_i), _ptr(out_s), _stream()), "rails_topk_candidates_filtered")
    return out_i, out_s


def rerank_topk_filtered(scores: torch.Tensor, k_prime: int, positions: torch.Tensor, ids: Optional[torch.Tensor], invalid_ids: torch.Tensor, k: int,
                         flag: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The tail of a candidate rerank from UNSORTED candidate positions with duplicates (include/rails_amd.h rails_rerank_topk_filtered): first copy
    of every position, ranked by (score desc, position asc), top k_prime, seen-id filter -> (out_ids (rows, k), out_scores (rows, k)).  `flag`
    (int32, zeroed by the caller; device or pinned host memory) is raised when a row has fewer than k_prime distinct positions -- the outputs are
    then undefined and the caller takes the sorted form."""
    lib = _lib.load()
    _require_device(scores, "scores")
    if scores.dtype != torch.float32 or scores.stride(1) != 1:
        scores = _f32c(scores)
    rows, n = scores.shape
    positions = positions.to(device=scores.device, dtype=torch.int64).contiguous()
    if positions.shape != (rows, n):
        raise ValueError("positions must be (rows, n_cand) like scores")
    if ids is not None:
        ids = ids.to(device=scores.device, dtype=torch.int64).reshape(-1).contiguous()
    inv = invalid_ids.to(device=scores.device, dtype=torch.int64).contiguous()
    if inv.dim() != 2 or inv.shape[0] != rows:
        raise ValueError("invalid_ids must be (rows, width)")
    if flag.dtype != torch.int32 or not (flag.is_cuda or flag.is_pinned()):
        raise ValueError("flag must be an int32 tensor on the device or in pinned host memory")
    need = int(lib.rails_rerank_workspace_bytes(rows, n))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=scores.device)
    out_i = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    out_s = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
    with _on_device(scores.device):
        _lib.check(lib.rails_rerank_topk_filtered(_ptr(scores), scores.stride(0), rows, n, k_prime, _ptr(positions), _ptr(ids), _ptr(inv), inv.shape[1], k,
                                                  _ptr(workspace), workspace.numel() * workspace.element_size(), _ptr(out_i), _ptr(out_s), _ptr(flag), _stream()),
                   "rails_rerank_topk_filtered")
    return out_i, out_s


COLLAPSE_MAX_LIST = 16384      # entries of one ranked list rails_topk_collapse walks
COLLAPSE_MAX_K = 512           # rails_topk_keys' k
COLLAPSE_MAX_SEEN = 4096       # rails_scores_group_max's seen ids per row
COLLAPSE_MAX_PER_GROUP = 32    # results per group on the exact modules: their fallback reads the scores once per unit of it
MMR_MAX_POOL = 1024            # pool entries of rails_topk_mmr: one thread of its workgroup each
MMR_MAX_DIM = 256              # entries of an item vector
MMR_MAX_MAGNITUDE = 2.0 ** 60  # of a vector's entries: no dot product of MMR_MAX_DIM terms overflows


def _seen_arg(invalid_ids: Optional[torch.Tensor], rows: int, device) -> Tuple[Optional[torch.Tensor], int]:
    if invalid_ids is None:
        return None, 0
    inv = invalid_ids.to(device=device, dtype=torch.int64).contiguous()
    if inv.dim() != 2 or inv.shape[0] != rows:
        raise ValueError("invalid_ids must be (rows, width)")
    return (inv, inv.shape[1]) if inv.shape[1] else (None, 0)


def topk_collapse(scores: torch.Tensor, positions: torch.Tensor, ranks: torch.Tensor, k: int, ids: Optional[torch.Tensor],
                  invalid_ids: Optional[torch.Tensor], flag: torch.Tensor, max_per_group: Optional[int] = None):
    """The walk of a collapsed top-k (include/rails_amd.h rails_topk_collapse): scores / positions (rows, D) in key order, ranks the (N,) int32
    dense group ranks -> (scores (rows, k), positions, ids, counts (rows,) int32).  `flag` (int32, zeroed by the caller; device or pinned host
    memory) is raised when a row's list holds fewer than k distinct eligible groups.  max_per_group = m (an int >= 1): the walk with a quota
    (rails_topk_collapse_quota) -- up to m entries of a group are kept, and counts / flag speak of the kept entries; None: the plain walk."""
    if max_per_group is not None and max_per_group < 1:
        raise ValueError("max_per_group must be >= 1")
    lib = _lib.load()
    _require_device(scores, "scores")
    if scores.dtype != torch.float32 or scores.stride(1) != 1:
        scores = _f32c(scores)
    rows, depth = scores.shape
    positions = positions.to(device=scores.device, dtype=torch.int64).contiguous()
    if positions.shape != (rows, depth):
        raise ValueError("positions must be (rows, depth) like scores")
    if ranks.dtype != torch.int32 or ranks.dim() != 1 or ranks.device != scores.device or not ranks.is_contiguous():
        raise ValueError("ranks must be a contiguous (N,) int32 tensor on the scores' device")
    if flag.dtype != torch.int32 or not (flag.is_cuda or flag.is_pinned()):
        raise ValueError("flag must be an int32 tensor on the device or in pinned host memory")
    if ids is not None:
        ids = ids.to(device=scores.device, dtype=torch.int64).reshape(-1).contiguous()
    inv, width = _seen_arg(invalid_ids, rows, scores.device)
    out_s = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
    out_p = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    out_i = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    counts = torch.empty(rows, dtype=torch.int32, device=scores.device)
    lists = (_ptr(scores), scores.stride(0), _ptr(positions), rows, depth, _ptr(ranks), ranks.numel(), _ptr(ids), _ptr(inv), width, k)
    outs = (_ptr(out_s), _ptr(out_p), _ptr(out_i), _ptr(counts), _ptr(flag), _stream())
    with _on_device(scores.device):
        if max_per_group is None:
            _lib.check(lib.rails_topk_collapse(*lists, *outs), "rails_topk_collapse")
        else:
            _lib.check(lib.rails_topk_collapse_quota(*lists, min(int(max_per_group), (1 << 31) - 1), *outs), "rails_topk_collapse_quota")
    return out_s, out_p, out_i, counts


def topk_mmr(scores: torch.Tensor, positions: torch.Tensor, vectors: torch.Tensor, lam: float, k: int, pool: int, ids: Optional[torch.Tensor],
             invalid_ids: Optional[torch.Tensor], word: torch.Tensor):
    """The walk of a diversified top-k (include/rails_amd.h rails_topk_mmr): scores / positions (rows, L), a ranked list per
    row; vectors the (N, E) fp32 item vectors -> (scores (rows, k), positions, ids, counts (rows,) int32) in PICK order -- the scores are the
    picked items' own relevance scores, so a row is not monotone.  The pool is the first `pool` eligible entries of the list (a position of
    the corpus, a score above -inf, an id not among the row's invalid_ids); counts: the pool's size per row; `word` (int32, zeroed by the
    caller; device or pinned host memory) is raised when a row's pool holds fewer than k.  Every argument and limit is checked before the
    launch."""
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 < float(lam) <= 1.0:
        raise ValueError(f"lam must be a Python float with 0 < lam <= 1, got {lam!r}")
    if not 1 <= k <= pool:
        raise ValueError(f"need 1 <= k <= pool, got k = {k}, pool = {pool}")
    if pool > MMR_MAX_POOL:
        raise NotImplementedError(f"pool = {pool} beyond {MMR_MAX_POOL}")
    if vectors.dtype != torch.float32 or vectors.dim() != 2 or not vectors.is_contiguous():
        raise ValueError("vectors must be a contiguous (N, E) float32 tensor")
    n_items, dim = vectors.shape
    if not 1 <= dim <= MMR_MAX_DIM:
        raise NotImplementedError(f"vectors of {dim} entries: 1 <= E <= {MMR_MAX_DIM}")
    if invalid_ids is not None and invalid_ids.dim() == 2 and invalid_ids.shape[1] > COLLAPSE_MAX_SEEN:
        raise NotImplementedError(f"width = {invalid_ids.shape[1]} beyond {COLLAPSE_MAX_SEEN} seen ids per row")
    if scores.dim() != 2 or not 1 <= scores.shape[1] <= COLLAPSE_MAX_LIST:
        raise NotImplementedError(f"scores must be (rows, L) with 1 <= L <= {COLLAPSE_MAX_LIST}")
    lib = _lib.load()
    _require_device(scores, "scores")
    if scores.dtype != torch.float32 or scores.stride(1) != 1:
        scores = _f32c(scores)
    rows, depth = scores.shape
    positions = positions.to(device=scores.device, dtype=torch.int64).contiguous()
    if positions.shape != (rows, depth):
        raise ValueError("positions must be (rows, L) like scores")
    if vectors.device != scores.device:
        raise ValueError("vectors must live on the scores' device")
    if word.dtype != torch.int32 or not (word.is_cuda or word.is_pinned()):
        raise ValueError("word must be an int32 tensor on the device or in pinned host memory")
    if ids is not None:
        ids = ids.to(device=scores.device, dtype=torch.int64).reshape(-1).contiguous()
        if ids.numel() < n_items:
            raise ValueError(f"ids holds {ids.numel()} entries but vectors has {n_items} rows")
    inv, width = _seen_arg(invalid_ids, rows, scores.device)
    need = int(lib.rails_topk_mmr_workspace_bytes(rows, pool, dim))
    workspace = torch.empty(need, dtype=torch.uint8, device=scores.device) if need else None
    out_s = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
    out_p = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    out_i = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
    counts = torch.empty(rows, dtype=torch.int32, device=scores.device)
    with _on_device(scores.device):
        _lib.check(lib.rails_topk_mmr(_ptr(scores), scores.stride(0), _ptr(positions), rows, depth, _ptr(vectors), n_items, dim, float(lam), k, pool,
                                      _ptr(ids), _ptr(inv), width, _ptr(workspace), need, _ptr(out_s), _ptr(out_p), _ptr(out_i), _ptr(counts),
                                      _ptr(word), _stream()), "rails_topk_mmr")
    return out_s, out_p, out_i, counts


def list_similarity(positions: torch.Tensor, vectors: torch.Tensor) -> torch.Tensor:
    """Mean pairwise similarity (dot product of the item vectors) of every returned row: positions (rows, k) int64, vectors (N, E) ->
    (rows,) fp32, the mean over the k (k - 1) / 2 pairs of a row (0 for k < 2).  What tools/mmr_bench.py sets beside the cost of diversify=;
    plain torch ops, a measurement and no part of any result."""
    v = vectors.index_select(0, positions.reshape(-1).to(vectors.device)).reshape(positions.shape[0], positions.shape[1], -1).to(torch.float32)
    k = positions.shape[1]
    if k < 2:
        return torch.zeros(positions.shape[0], dtype=torch.float32, device=vectors.device)
    gram = torch.bmm(v, v.transpose(1, 2))
    off = gram.sum(dim=(1, 2)) - torch.diagonal(gram, dim1=1, dim2=2).sum(dim=1)
    return off / float(k * (k - 1))


def _group_table_args(scores: torch.Tensor, ranks: torch.Tensor, table: torch.Tensor, shape: str, first_item: int, ids: Optional[torch.Tensor],
                      invalid_ids: Optional[torch.Tensor]):
    """The argument check scores_group_max and scores_group_next share -> (rows, n, ids, seen ids, width); shape: the table's, for the message."""
    _require_device(scores, "scores")
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise ValueError("scores must be a (rows, n) float32 matrix with unit column stride")
    rows, n = scores.shape
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[0] != rows or not table.is_contiguous() or table.device != scores.device:
        raise ValueError(f"table must be a contiguous {shape} int64 tensor on the scores' device")
    if ranks.dtype != torch.int32 or ranks.dim() != 1 or ranks.device != scores.device or not ranks.is_contiguous() or ranks.numel() < first_item + n:
        raise ValueError("ranks must be a contiguous int32 tensor of at least first_item + n entries on the scores' device")
    if ids is not None:
        ids = ids.to(device=scores.device, dtype=torch.int64).reshape(-1).contiguous()
    return (rows, n, ids) + _seen_arg(invalid_ids, rows, scores.device)


def scores_group_next(scores: torch.Tensor, ranks: torch.Tensor, table: torch.Tensor, groups: int, round: int, first_item: int = 0,
                      ids: Optional[torch.Tensor] = None, invalid_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place on `table` ((rows, m * groups) int64, the m rounds of a row side by side, ZEROED by the caller): round `round` of the per-group
    best-m of the (rows, n) score matrix whose column x is item first_item + x (include/rails_amd.h rails_scores_group_next).  Round t reads
    round t - 1, which must be complete (every chunk of the corpus); afterwards slot t * groups + r of a row holds the key of rank r's
    (t + 1)-th best eligible item, 0 where it has fewer."""
    lib = _lib.load()
    rows, n, ids, inv, width = _group_table_args(scores, ranks, table, "(rows, m * groups)", first_item, ids, invalid_ids)
    if groups < 1 or table.shape[1] % groups or not 0 <= round < table.shape[1] // groups:
        raise ValueError("table must hold whole rounds of `groups` keys per row, `round` one of them")
    stride = table.shape[1]
    here = C.c_void_p(table.data_ptr() + 8 * round * groups)
    below = C.c_void_p(table.data_ptr() + 8 * (round - 1) * groups if round else 0)
    with _on_device(scores.device):
        _lib.check(lib.rails_scores_group_next(_ptr(scores), scores.stride(0), rows, n, int(first_item), _ptr(ranks), groups, here, stride, below, stride,
                                               _ptr(ids), _ptr(inv), width, _stream()), "rails_scores_group_next")
    return table


def scores_group_max(scores: torch.Tensor, ranks: torch.Tensor, table: torch.Tensor, first_item: int = 0, clear: bool = True,
                     ids: Optional[torch.Tensor] = None, invalid_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place on `table` ((rows, G) int64 holding the 64-bit keys): the per-group maxima of the (rows, n) score matrix whose column x is
    item first_item + x (include/rails_amd.h rails_scores_group_max).  clear: zero the table first."""
    lib = _lib.load()
    rows, n, ids, inv, width = _group_table_args(scores, ranks, table, "(rows, G)", first_item, ids, invalid_ids)
    with _on_device(scores.device):
        _lib.check(lib.rails_scores_group_max(_ptr(scores), scores.stride(0), rows, n, int(first_item), _ptr(ranks), table.shape[1], _ptr(table),
                                              1 if clear else 0, _ptr(ids), _ptr(inv), width, _stream()), "rails_scores_group_max")
    return table


def topk_keys(table: torch.Tensor, k: int, ids: Optional[torch.Tensor] = None):
    """The k largest keys of every row of a group-maxima table, decoded (include/rails_amd.h rails_topk_keys) -> (scores (rows, k), positions,
    ids, counts (rows,) int32: the row's non-zero keys)."""
    lib = _lib.load()
    _require_device(table, "table")
    if table.dtype != torch.int64 or table.dim() != 2 or not table.is_contiguous():
        raise ValueError("table must be a contiguous (rows, G) int64 tensor")
    rows, groups = table.shape
    if ids is not None:
        ids = ids.to(device=table.device, dtype=torch.int64).reshape(-1).contiguous()
    out_s = torch.empty((rows, k), dtype=torch.float32, device=table.device)
    out_p = torch.empty((rows, k), dtype=torch.int64, device=table.device)
    out_i = torch.empty((rows, k), dtype=torch.int64, device=table.device)
    counts = torch.empty(rows, dtype=torch.int32, device=table.device)
    with _on_device(table.device):
        _lib.check(lib.rails_topk_keys(_ptr(table), rows, groups, k, _ptr(ids), _ptr(out_s), _ptr(out_p), _ptr(out_i), _ptr(counts), _stream()),
                   "rails_topk_keys")
    return out_s, out_p, out_i, counts


def topk_filter_fusable(n: int, k_prime: int, width: int, k: int) -> bool:
    return bool(_lib.load().rails_topk_filter_fusable(int(n), int(k_prime), int(width), int(k)))


def topk_filtered(scores: torch.Tensor, k_prime: int, ids: Optional[torch.Tensor], invalid_ids: torch.Tensor, k: int,
                  workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                  run_if: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """topk(scores, k_prime, ids) followed by filter_seen_ids(..., invalid_ids, k), the filter fused into the final selection launch
    (include/rails_amd.h rails_topk_filtered).  -> (out_ids (rows, k), out_scores (rows, k)), ids first like filter_seen_ids."""
    lib = _lib.load()
    _require_device(scores, "scores")
    if scores.dtype != torch.float32 or scores.stride(1) != 1:
        scores = _f32c(scores)
    rows, n = scores.shape
    stride = 0
    if ids is not None:
        if ids.dtype != torch.int64 or ids.device != scores.device:
            ids = ids.to(device=scores.device, dtype=torch.int64)
        if ids.dim() == 2 and ids.shape[0] == rows and rows > 1:
            ids = ids.contiguous()
            stride = ids.shape[1]
        else:
            ids = ids.reshape(-1).contiguous()
    invalid_ids = invalid_ids.to(device=scores.device, dtype=torch.int64).contiguous()
    if out is not None:      # (out_ids, out_scores): overwritten (the predicated fallback of the fused score + select path)
        out_i, out_s = out
        if out_i.shape != (rows, k) or out_s.shape != (rows, k) or out_i.dtype != torch.int64 or out_s.dtype != torch.float32 or not (out_i.is_contiguous() and out_s.is_contiguous()):
            raise ValueError("topk_filtered: out must be contiguous (rows, k) int64 and fp32 tensors")
    else:
        out_i = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
        out_s = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
    ws_bytes = lib.rails_topk_workspace_bytes(rows, n, k_prime)
    ws = workspace if workspace is not None and workspace.numel() >= ws_bytes and workspace.device == scores.device else torch.empty(ws_bytes, dtype=torch.uint8, device=scores.device)
    with _on_device(scores.device):
        _lib.check(lib.rails_topk_filtered(_ptr(scores), scores.stride(0), rows, n, k_prime, _ptr(ids), stride, _inv_ptr(invalid_ids), invalid_ids.shape[1], k,
                                           _ptr(out_i), _ptr(out_s), _ptr(ws), ws_bytes, _pred(run_if), _stream()), "rails_topk_filtered")
    return out_i, out_s


def hash_item_table(seed: int, first_item: int, n_items: int, dim: int, device, sigma: float = 0.02, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n_items, dim) fp32 rows of the synthetic counter-hash item table, drawn on the device: the same bits as
    oracle.mol_oracle.hash_item_table(seed, first_item, n_items, dim, sigma) (include/rails_amd.h rails_hash_item_table)."""
    import math

    import numpy as np

    if out is None:
        out = torch.empty((n_items, dim), dtype=torch.float32, device=device)
    scale = float(np.float32(sigma * math.sqrt(3.0) / 65536.0))
    with _on_device(out.device):
        _lib.check(_lib.load().rails_hash_item_table(seed, first_item, n_items, dim, C.c_float(scale), _ptr(out), _stream()), "rails_hash_item_table")
    return out


def range_flag(values: torch.Tensor, lo: int, hi: int, flag: torch.Tensor) -> None:
    """flag |= any(values < lo or values > hi), on the device (rails_range_flag_i32); `flag` is an int32 device scalar the caller zeroed."""
    lib = _lib.load()
    with _on_device(values.device):
        _lib.check(lib.rails_range_flag_i32(_ptr(values), values.numel(), int(lo), int(hi), _ptr(flag), _stream()), "rails_range_flag_i32")


def rescore_verdict(stats: torch.Tensor, state: torch.Tensor, default_eps: float, safety: float,
                    guard: Optional[torch.Tensor] = None, guard_limit: float = 0.0) -> None:
    """Device-side verdict of a speculative call (rails_rescore_verdict): updates `state` (8 fp32 on the device) in stream order.
    guard: fp32 values (contiguous) whose magnitudes must stay <= guard_limit, else the call is flagged for the redo."""
    lib = _lib.load()
    with _on_device(stats.device):
        _lib.check(lib.rails_rescore_verdict(_ptr(stats), stats.shape[0], float(default_eps), float(safety), _ptr(guard),
                                             0 if guard is None else guard.numel(), float(guard_limit), _ptr(state), _stream()), "rails_rescore_verdict")


def margin_stats(kth_scores: torch.Tensor, col: int, m_max: torch.Tensor, err_max: torch.Tensor) -> torch.Tensor:
    """(rows, >= col + 1) fp32 merged scores, (rows,) fp32, (1,) fp32 -> (rows, 2) row_stats [err_max, kth_scores[:, col] - m_max] (rails_margin_stats)."""
    lib = _lib.load()
    _require_device(kth_scores, "scores")
    rows = kth_scores.shape[0]
    stats = torch.empty((rows, 2), dtype=torch.float32, device=kth_scores.device)
    with _on_device(kth_scores.device):
        _lib.check(lib.rails_margin_stats(_ptr(kth_scores), kth_scores.stride(0), int(col), _ptr(m_max), _ptr(err_max), rows, _ptr(stats), _stream()), "rails_margin_stats")
    return stats


def mfma_probe_f16(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """n x (32 x 16) f16, n x (16 x 32) f16, n x (32 x 32) fp32 -> n x (32 x 32) fp32: one v_mfma_f32_32x32x16_f16 each (rails_mfma_probe_f16)."""
    lib = _lib.load()
    _require_device(a, "a")
    a, b, c = a.to(torch.float16).contiguous(), b.to(torch.float16).contiguous(), _f32c(c)
    n = a.shape[0]
    if tuple(a.shape) != (n, 32, 16) or tuple(b.shape) != (n, 16, 32) or tuple(c.shape) != (n, 32, 32):
        raise ValueError("mfma_probe_f16: a (n, 32, 16), b (n, 16, 32), c (n, 32, 32)")
    d = torch.empty_like(c)
    with _on_device(a.device):
        _lib.check(lib.rails_mfma_probe_f16(_ptr(a), _ptr(b), _ptr(c), _ptr(d), n, _stream()), "rails_mfma_probe_f16")
    return d


def mfma_probe_f32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """n x (32 x 2), n x (2 x 32), n x (32 x 32) fp32 -> n x (32 x 32): one v_mfma_f32_32x32x2_f32 each (rails_mfma_probe_f32)."""
    lib = _lib.load()
    _require_device(a, "a")
    a, b, c = _f32c(a), _f32c(b), _f32c(c)
    n = a.shape[0]
    if tuple(a.shape) != (n, 32, 2) or tuple(b.shape) != (n, 2, 32) or tuple(c.shape) != (n, 32, 32):
        raise ValueError("mfma_probe_f32: a (n, 32, 2), b (n, 2, 32), c (n, 32, 32)")
    d = torch.empty_like(c)
    with _on_device(a.device):
        _lib.check(lib.rails_mfma_probe_f32(_ptr(a), _ptr(b), _ptr(c), _ptr(d), n, _stream()), "rails_mfma_probe_f32")
    return d


def scalar_probe(x: torch.Tensor) -> torch.Tensor:
    """(n,) fp32 -> (3, n): v_exp_f32(x), v_rcp_f32(x), x / (1 + 2^x) as the scoring kernels compute it (rails_scalar_probe_f32)."""
    lib = _lib.load()
    _require_device(x, "x")
    x = _f32c(x).reshape(-1)
    out = torch.empty((3, x.numel()), dtype=torch.float32, device=x.device)
    with _on_device(x.device):
        _lib.check(lib.rails_scalar_probe_f32(_ptr(x), x.numel(), _ptr(out), _stream()), "rails_scalar_probe_f32")
    return out


def rescore_select(exact: torch.Tensor, approx: torch.Tensor, positions: torch.Tensor, ids: Optional[torch.Tensor], n_items: int, k: int,
                   margin_eps: float = float("inf"), check_eps: float = float("inf"),
                   approx_dense: Optional[torch.Tensor] = None, one_sided: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Verified finish of a speculative brute-force top-k (include/rails_amd.h rails_rescore_select): exact (rows, >= n_cand) fp32,
    approx (rows, n_ranked), positions (rows, n_cand >= n_ranked; the tail are probes looked up in approx_dense (rows, n_items))
    -> (scores (rows, k), ids (rows, k), row_ok (rows,) int32 for the given eps, row_stats (rows, 2) fp32 = [max |exact - approx|,
    k-th exact - min candidate approx]).  one_sided: approx are upper bounds of the exact scores; the error stat is max(0, exact - approx)."""
    lib = _lib.load()
    _require_device(exact, "exact scores")
    rows, n_cand = positions.shape
    approx, positions = _f32c(approx), positions.to(torch.int64).contiguous()
    out_s = torch.empty((rows, k), dtype=torch.float32, device=exact.device)
    out_i = torch.empty((rows, k), dtype=torch.int64, device=exact.device)
    ok = torch.empty((rows,), dtype=torch.int32, device=exact.device)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=exact.device)
    with _on_device(exact.device):
        _lib.check(lib.rails_rescore_select(_ptr(exact), exact.stride(0), _ptr(approx), _ptr(approx_dense), 0 if approx_dense is None else approx_dense.stride(0),
                                            _ptr(positions), _ptr(ids), n_items, rows, approx.shape[1], n_cand, k, margin_eps, check_eps, 1 if one_sided else 0,
                                            _ptr(out_s), _ptr(out_i), _ptr(ok), _ptr(stats), _stream()), "rails_rescore_select")
    return out_s, out_i, ok, stats


def candidates_workspace(rows: int, device) -> torch.Tensor:
    """The zeroed workspace of candidates_select / candidates_finish for up to `rows` rows (include/rails_amd.h: zeroed once, every
    select + finish pair leaves it zeroed).  Its first `rows` int32 are the per-row candidate counts between the two calls."""
    n = _lib.load().rails_candidates_workspace_bytes(int(rows))
    return torch.zeros((n + 3) // 4, dtype=torch.int32, device=device)


def candidates_select(scores: torch.Tensor, cap: int, lo: float, hi: float, workspace: torch.Tensor, out_pos: torch.Tensor, out_approx: torch.Tensor) -> None:
    """Threshold selection of at most `cap` candidates per row of `scores` (rows, n) fp32 (rails_candidates_select): positions into
    out_pos (rows, >= cap) int64, their scores into out_approx (rows, >= cap) fp32, counts into workspace[:rows]."""
    lib = _lib.load()
    _require_device(scores, "scores")
    rows, n = scores.shape
    if out_pos.stride(0) != out_approx.stride(0) or out_pos.stride(0) < cap:
        raise ValueError("candidates_select: out_pos / out_approx must share a row stride >= cap")
    with _on_device(scores.device):
        _lib.check(lib.rails_candidates_select(_ptr(scores), scores.stride(0), rows, n, int(cap), float(lo), float(hi), _ptr(workspace), _ptr(out_pos), _ptr(out_approx),
                                               out_pos.stride(0), _stream()), "rails_candidates_select")


def candidates_finish(exact: torch.Tensor, approx: torch.Tensor, positions: torch.Tensor, cap: int, workspace: torch.Tensor, ids: Optional[torch.Tensor], n_items: int,
                      k: int, default_eps: float, safety: float, one_sided: bool, guard: Optional[torch.Tensor], guard_per_row: int, guard_limit: float,
                      state: Optional[torch.Tensor], state_host: Optional[torch.Tensor] = None, seen: Optional[Tuple[torch.Tensor, int]] = None,
                      msg: Optional[torch.Tensor] = None):
    """rails_candidates_finish: sort the rows' candidates by (fp32 score, position), write the top k, the verdict and (seen = (invalid_ids, k_out)) the
    seen-id filter's output -> (scores (rows, k), ids (rows, k), f_ids or None, f_scores or None); with `msg` (rows, 2k + 2) int64 the item-sharded
    message is written instead and nothing is returned."""
    lib = _lib.load()
    rows = exact.shape[0]
    dev = exact.device
    out_s = out_i = f_i = f_s = inv = None
    width = f_k = 0
    if msg is None:
        out_s = torch.empty((rows, k), dtype=torch.float32, device=dev)
        out_i = torch.empty((rows, k), dtype=torch.int64, device=dev)
        if seen is not None:
            inv, f_k = seen
            if inv.dtype != torch.int64 or inv.device != dev or not inv.is_contiguous():
                inv = inv.to(device=dev, dtype=torch.int64).contiguous()
            width = inv.shape[1]
            f_i = torch.empty((rows, f_k), dtype=torch.int64, device=dev)
            f_s = torch.empty((rows, f_k), dtype=torch.float32, device=dev)
    with _on_device(dev):
        _lib.check(lib.rails_candidates_finish(_ptr(exact), exact.stride(0), _ptr(approx), _ptr(positions), positions.stride(0), int(cap), _ptr(workspace), _ptr(ids), int(n_items),
                                               rows, int(k), float(default_eps), float(safety), 1 if one_sided else 0, _ptr(guard), int(guard_per_row), float(guard_limit),
                                               _ptr(out_s), _ptr(out_i), None if inv is None else _inv_ptr(inv), width, int(f_k), _ptr(f_i), _ptr(f_s), _ptr(state),
                                               _ptr(state_host), _ptr(msg), _stream()), "rails_candidates_finish")
    return out_s, out_i, f_i, f_s


def pack_candidates(scores: torch.Tensor, ids: torch.Tensor, k: int) -> torch.Tensor:
    """(rows, k_local) fp32 scores + int64 ids -> (rows, 2k) int64 message (score bits | ids), padded with (-inf, -1)."""
    lib = _lib.load()
    _require_device(scores, "scores")
    rows, kl = scores.shape
    scores, ids = _f32c(scores), ids.to(torch.int64).contiguous()
    msg = torch.empty((rows, 2 * k), dtype=torch.int64, device=scores.device)
    with _on_device(scores.device):
        _lib.check(lib.rails_pack_candidates(_ptr(scores), _ptr(ids), rows, kl, k, _ptr(msg), _stream()), "rails_pack_candidates")
    return msg


def merge_candidates(gathered: torch.Tensor, n_ranks: int, k: int, k_out: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """gathered (n_ranks * rows, 2k) int64 messages in rank order -> exact top-k_out (scores, ids) per row."""
    lib = _lib.load()
    _require_device(gathered, "gathered messages")
    rows = gathered.shape[0] // n_ranks
    gathered = gathered.contiguous()
    out_s = torch.empty((rows, k_out), dtype=torch.float32, device=gathered.device)
    out_i = torch.empty((rows, k_out), dtype=torch.int64, device=gathered.device)
    with _on_device(gathered.device):
        _lib.check(lib.rails_merge_candidates(_ptr(gathered), n_ranks, rows, k, k_out, _ptr(out_s), _ptr(out_i), _stream()), "rails_merge_candidates")
    return out_s, out_i


def group_keys_supported(n_ranks: int, k: int) -> bool:
    """sizes rails_group_keys_merge_own takes (n_ranks * k <= 16384); answers without a device"""
    return bool(_lib.load().rails_group_keys_supported(int(n_ranks), int(k)))


def group_keys_pack(scores: torch.Tensor, positions: torch.Tensor, offset: int, n_local: int, k_slots: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(rows, k_local) bf16-valued fp32 scores + int64 local positions in [0, n_local) -> (rows, k_slots) int64 holding the 64-bit candidate
    keys (score image << 48 | 2^48 - 1 - (position + offset); key 0 pads), one launch (include/rails_amd.h rails_group_keys_pack).
    out: a contiguous int64 tensor of rows * k_slots elements to write into (a slice of a larger message)."""
    lib = _lib.load()
    _require_device(scores, "scores")
    rows, kl = scores.shape
    scores, positions = _f32c(scores), positions.to(torch.int64).contiguous()
    if out is None:
        out = torch.empty((rows, k_slots), dtype=torch.int64, device=scores.device)
    elif out.dtype != torch.int64 or out.numel() != rows * k_slots or not out.is_contiguous() or out.device != scores.device:
        raise ValueError("group_keys_pack: out must be a contiguous int64 tensor of rows * k_slots elements on the scores' device")
    with _on_device(scores.device):
        _lib.check(lib.rails_group_keys_pack(_ptr(scores), _ptr(positions), rows, kl, int(offset), int(n_local), int(k_slots), _ptr(out), _stream()),
                   "rails_group_keys_pack")
    return out


def group_keys_merge_own(gathered: torch.Tensor, n_ranks: int, rows: int, k: int, lo: int, hi: int, out_local: Optional[torch.Tensor] = None,
                         out_col: int = 0, rows_per_out_row: int = 1, want_global: bool = False, rank_stride: Optional[int] = None):
    """gathered: int64 keys of n_ranks ranks in rank order, rank r's (rows, k) block starting at element r * rank_stride (default rows * k)
    -> the global top-k of every row as THIS rank's local positions (position - lo inside [lo, hi), -1 elsewhere and for pads), one launch
    (include/rails_amd.h rails_group_keys_merge_own).  out_local: a contiguous (B, W) int64 union buffer, row b of the keys going to
    out_local[b // rows_per_out_row, out_col + (b % rows_per_out_row) * k : ...]; default a fresh (rows, k).
    -> out_local, or (out_local, global positions (rows, k)) with want_global."""
    lib = _lib.load()
    _require_device(gathered, "gathered keys")
    if gathered.dtype != torch.int64 or not gathered.is_contiguous():
        raise ValueError("group_keys_merge_own: gathered must be a contiguous int64 tensor")
    stride = rows * k if rank_stride is None else int(rank_stride)
    if gathered.numel() < (n_ranks - 1) * stride + rows * k:
        raise ValueError("group_keys_merge_own: gathered is shorter than n_ranks messages")
    dev = gathered.device
    if out_local is None:
        out_local = torch.empty((rows, k), dtype=torch.int64, device=dev)
        out_col, rows_per_out_row = 0, 1
    elif (out_local.dtype != torch.int64 or out_local.dim() != 2 or not out_local.is_contiguous() or out_local.device != dev
          or out_local.shape[0] * rows_per_out_row < rows):
        raise ValueError("group_keys_merge_own: out_local must be a contiguous int64 (ceil(rows / rows_per_out_row), W) tensor on the keys' device")
    out_g = torch.empty((rows, k), dtype=torch.int64, device=dev) if want_global else None
    with _on_device(dev):
        _lib.check(lib.rails_group_keys_merge_own(_ptr(gathered), int(n_ranks), stride, int(rows), int(k), int(lo), int(hi), _ptr(out_g), _ptr(out_local),
                                                  out_local.shape[1], int(out_col), int(rows_per_out_row), _stream()), "rails_group_keys_merge_own")
    return (out_local, out_g) if want_global else out_local


def merge_filter_fusable(k_prime: int, width: int, k: int) -> bool:
    return 0 < k <= k_prime <= 512 and 0 <= width <= 256


def merge_candidates_filtered(gathered: torch.Tensor, n_ranks: int, k: int, k_prime: int, invalid_ids: torch.Tensor, k_out: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """merge_candidates(gathered, n_ranks, k, k_prime) followed by filter_seen_ids(..., invalid_ids, k_out) in one launch
    (include/rails_amd.h rails_merge_candidates_filtered) -> (out_ids (rows, k_out), out_scores (rows, k_out))."""
    lib = _lib.load()
    _require_device(gathered, "gathered messages")
    rows = gathered.shape[0] // n_ranks
    gathered = gathered.contiguous()
    invalid_ids = invalid_ids.to(device=gathered.device, dtype=torch.int64).contiguous()
    out_s = torch.empty((rows, k_out), dtype=torch.float32, device=gathered.device)
    out_i = torch.empty((rows, k_out), dtype=torch.int64, device=gathered.device)
    with _on_device(gathered.device):
        _lib.check(lib.rails_merge_candidates_filtered(_ptr(gathered), n_ranks, rows, k, k_prime, _inv_ptr(invalid_ids), invalid_ids.shape[1], k_out,
                                                       _ptr(out_i), _ptr(out_s), _stream()), "rails_merge_candidates_filtered")
    return out_i, out_s


def merge_candidates_verdict(gathered: torch.Tensor, n_ranks: int, k: int, k_out: int, default_eps: float, safety: float, guard: Optional[torch.Tensor],
                             guard_per_row: int, guard_limit: float, state: torch.Tensor, state_host: Optional[torch.Tensor], call_ws: torch.Tensor,
                             seen: Optional[Tuple[torch.Tensor, int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """gathered (n_ranks * rows, 2k + 2) int64 messages of candidates_finish(msg=...) in rank order -> merged exact top-k_out + the global verdict of the
    item-sharded proved top-k in one launch (include/rails_amd.h rails_merge_candidates_verdict).  -> (scores, ids) (rows, k_out), or with
    seen = (invalid_ids, k_f) the filtered (ids, scores) (rows, k_f)."""
    lib = _lib.load()
    _require_device(gathered, "gathered messages")
    rows = gathered.shape[0] // n_ranks
    gathered = gathered.contiguous()
    dev = gathered.device
    inv, width, f_k = None, 0, 0
    cols = k_out
    if seen is not None:
        inv, f_k = seen
        inv = inv.to(device=dev, dtype=torch.int64).contiguous()
        width, cols = inv.shape[1], f_k
    out_s = torch.empty((rows, cols), dtype=torch.float32, device=dev)
    out_i = torch.empty((rows, cols), dtype=torch.int64, device=dev)
    with _on_device(dev):
        _lib.check(lib.rails_merge_candidates_verdict(_ptr(gathered), n_ranks, rows, int(k), int(k_out), float(default_eps), float(safety), _ptr(guard), int(guard_per_row),
                                                      float(guard_limit), _ptr(state), _ptr(state_host), _ptr(call_ws), None if inv is None else _inv_ptr(inv), width, int(f_k),
                                                      _ptr(out_i), _ptr(out_s), _stream()), "rails_merge_candidates_verdict")
    if seen is not None:
        return out_i, out_s
    return out_s, out_i


def filter_seen_ids(top_ids: torch.Tensor, top_scores: torch.Tensor, invalid_ids: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row-wise seen-id filter (reference indexing/candidate_index.py:154-178) -> (ids (rows,k), scores (rows,k))."""
    lib = _lib.load()
    _require_device(top_ids, "top_k ids")
    rows, kp = top_ids.shape
    top_ids = top_ids.to(torch.int64).contiguous()
    score_dtype = top_scores.dtype
    top_scores = _f32c(top_scores)
    inv = invalid_ids.to(device=top_ids.device, dtype=torch.int64).contiguous()
    out_i = torch.empty((rows, k), dtype=torch.int64, device=top_ids.device)
    out_s = torch.empty((rows, k), dtype=torch.float32, device=top_ids.device)
    with _on_device(top_ids.device):
        _lib.check(
            lib.rails_filter_seen_ids(_ptr(top_ids), _ptr(top_scores), rows, kp, _inv_ptr(inv), inv.shape[1], k, _ptr(out_i), _ptr(out_s), _stream()),
            "rails_filter_seen_ids",
        )
    return out_i, out_s.to(score_dtype)
