"""Host layer shared by the HSTU and SASRec query encoders (hstu.py, sasrec.py): the reference's parameter holders, the parsing of
the two constructor signatures, and the `Encoder` base class (input checks, the length policy and its violation counter, the
row-count contract of a multi-row decode step, fp32 parameter staging, the postprocessor launch)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib
from .engine import _on_device, _ptr, _stream


class LocalEmbeddingModule(torch.nn.Module):
    """Reference modeling/sequential/embedding_modules.py:40-73: `_item_emb.weight` (num_items + 1, D), row 0 = padding."""

    def __init__(self, num_items: int, item_embedding_dim: int) -> None:
        super().__init__()
        self._item_embedding_dim = item_embedding_dim
        self._item_emb = torch.nn.Embedding(num_items + 1, item_embedding_dim, padding_idx=0)
        torch.nn.init.trunc_normal_(self._item_emb.weight, mean=0.0, std=0.02, a=-0.04, b=0.04)

    def debug_str(self) -> str:
        return f"local_emb_d{self._item_embedding_dim}"

    def get_item_embeddings(self, item_ids: torch.Tensor) -> torch.Tensor:
        return self._item_emb(item_ids)

    @property
    def item_embedding_dim(self) -> int:
        return self._item_embedding_dim


class LearnablePositionalEmbeddingInputFeaturesPreprocessor(torch.nn.Module):
    """Reference modeling/sequential/input_features_preprocessors.py:43-92: `_pos_emb.weight` (max_sequence_len, D).  A parameter
    holder here: x = emb * sqrt(D) + pos_emb, masked by id != 0, is evaluated by rails_hstu_preprocess / the fused encoder."""

    def __init__(self, max_sequence_len: int, embedding_dim: int, dropout_rate: float = 0.0) -> None:
        super().__init__()
        self._embedding_dim = embedding_dim
        self._pos_emb = torch.nn.Embedding(max_sequence_len, embedding_dim)
        self._dropout_rate = dropout_rate
        std = (1.0 / embedding_dim) ** 0.5
        torch.nn.init.trunc_normal_(self._pos_emb.weight, mean=0.0, std=std, a=-2 * std, b=2 * std)

    def debug_str(self) -> str:
        return f"posi_d{self._dropout_rate}"

    def forward(self, *args, **kwargs):
        raise NotImplementedError("evaluated inside rails_amd's HSTU encoder kernels")


class _Postproc(torch.nn.Module):
    mode = ""

    def __init__(self, embedding_dim: int, eps: float = 1e-6) -> None:
        super().__init__()
        self._embedding_dim = embedding_dim
        self._eps = eps

    def forward(self, *args, **kwargs):
        raise NotImplementedError("evaluated by rails_rows_normalize / the fused encoder kernel")


class L2NormEmbeddingPostprocessor(_Postproc):
    """Reference modeling/sequential/output_postprocessors.py:37-59."""
    mode = "l2_norm"

    def debug_str(self) -> str:
        return "l2"


class LayerNormEmbeddingPostprocessor(_Postproc):
    """Reference modeling/sequential/output_postprocessors.py:62-85."""
    mode = "layer_norm"

    def debug_str(self) -> str:
        return "ln"


def parse_args(name: str, args: tuple, kwargs: dict, reference_style: bool, reference: tuple, compact: tuple) -> dict:
    """The constructor arguments after the seven leading ones, by name.  `reference` / `compact`: (names, defaults) of the two
    signatures; `reference_style` picks one.  Raises TypeError as a Python signature would."""
    names, defaults = reference if reference_style else compact
    if len(args) > len(names):
        raise TypeError(f"{name}() takes at most {7 + len(names)} positional arguments")
    a = dict(defaults)
    a.update(zip(names, args))
    for key, v in kwargs.items():
        if key not in names:
            raise TypeError(f"{name}() got an unexpected keyword argument '{key}'")
        a[key] = v
    missing = [n for n in names if n not in a]
    if missing:
        raise TypeError(f"{name}() missing required arguments: {missing}")
    return a


class Encoder(torch.nn.Module):
    """What HSTU and SASRec share.  Subclasses set NAME and call Encoder.__init__ before building their layers (the parameter
    holders are initialised first, so the random initialisation keeps its order)."""

    NAME = ""
    STRICT_DEVICE_LENGTHS = False   # True: validate device-resident past_lengths too (one blocking device-to-host read per call)
    _violations: Dict[torch.device, torch.Tensor] = {}   # one process-wide counter per device, whichever encoder counted

    def __init__(self, a: dict, reference_style: bool, seq: int, embedding_dim: int, num_blocks: int, num_heads: int) -> None:
        """`a`: parse_args' result.  Reference style: the caller's holder modules (or any objects with the same attributes)."""
        super().__init__()
        if reference_style:
            emb_mod, pre_mod, post_mod = a["embedding_module"], a["input_features_preproc_module"], a["output_postproc_module"]
            if not hasattr(emb_mod, "_item_emb") or not hasattr(pre_mod, "_pos_emb"):
                raise NotImplementedError(f"{self.NAME} needs a LocalEmbeddingModule-like embedding_module (`_item_emb`) and a "
                                          "LearnablePositionalEmbeddingInputFeaturesPreprocessor-like preprocessor (`_pos_emb`)")
            output_postproc = getattr(post_mod, "mode", None) or {"l2": "l2_norm", "ln": "layer_norm"}.get(post_mod.debug_str())
            eps = float(getattr(post_mod, "_eps", 1e-6))
        else:
            output_postproc, eps = a["output_postproc"], a["eps"]
        if output_postproc not in ("layer_norm", "l2_norm"):
            raise ValueError(f"Unknown output_postproc {output_postproc}")
        self._ndp_module = a["similarity_module"]
        self._embedding_dim = embedding_dim
        self._seq = seq
        self._num_blocks, self._num_heads = num_blocks, num_heads
        self._postproc, self._eps = output_postproc, eps
        if not reference_style:
            emb_mod = LocalEmbeddingModule(a["num_items"], embedding_dim)
            pre_mod = LearnablePositionalEmbeddingInputFeaturesPreprocessor(seq, embedding_dim)
            post_mod = (LayerNormEmbeddingPostprocessor(embedding_dim, eps) if output_postproc == "layer_norm"
                        else L2NormEmbeddingPostprocessor(embedding_dim, eps))
        self._embedding_module, self._input_features_preproc, self._output_postproc = emb_mod, pre_mod, post_mod
        self.use_fused_kernel = True    # short sequences: the whole encoder in one launch (falls back when it does not fit)
        self._fused_ptrs = None         # _lib.layer_table's (key, table) of the last fused launch
        self._decode_ptrs = None        # ... and of the last decode step
        self.register_buffer("_attn_mask", torch.triu(torch.ones((seq, seq), dtype=torch.bool), diagonal=1))

    def get_item_embeddings(self, item_ids: torch.Tensor) -> torch.Tensor:
        return self._embedding_module._item_emb(item_ids)       # a row gather

    # ---- checks -----------------------------------------------------------------------------------------------------
    def _check(self, past_ids, past_embeddings, device: bool = True) -> None:
        """Eval mode, past_ids (B, N) and past_embeddings (B, N, D) with N the model's sequence length, and (device) on the GPU."""
        if self.training:
            raise NotImplementedError(f"rails_amd.{self.NAME} is eval-only: call .eval()")
        B, N = past_ids.shape
        if N != self._seq or past_embeddings.shape != (B, N, self._embedding_dim):
            raise ValueError(f"expected past_ids (B, {self._seq}) and past_embeddings (B, {self._seq}, {self._embedding_dim}), "
                             f"got {tuple(past_ids.shape)} and {tuple(past_embeddings.shape)}")
        if device:
            self._check_device(past_embeddings)

    def _check_device(self, past_embeddings) -> None:
        if not past_embeddings.is_cuda:
            raise RuntimeError(f"rails_amd.{self.NAME} runs on the GPU only (no CPU fallback)")

    # ---- lengths ----------------------------------------------------------------------------------------------------
    def _lengths(self, past_lengths: torch.Tensor, dev, N: int, min_len: int = 1) -> torch.Tensor:
        """int64 lengths on the device, VALIDATED to lie in [min_len, N]: a length beyond the padded width, or an empty history in
        encode() (which indexes row `length - 1`; the reference's flattened gather at offset -1 fails there too, hstu.py:773-781),
        is an upstream data bug and raises instead of returning a plausible embedding of the wrong row.  HSTU.forward() accepts 0
        (an all-padding sequence is all zero rows, as in the reference).  Lengths that arrive on the HOST (the data loader's case)
        are checked there, for free; lengths that are already device tensors are clamped into range on the device instead --
        reading a flag back would be a blocking device-to-host sync on every encode and would rule out stream capture (set
        STRICT_DEVICE_LENGTHS = True on the encoder's class, or on Encoder for both, to pay that sync and raise as for host lengths)."""
        lengths = past_lengths.to(dtype=torch.int64)
        if not lengths.is_cuda or type(self).STRICT_DEVICE_LENGTHS:
            if bool(((lengths < min_len) | (lengths > N)).any()):
                raise ValueError(f"past_lengths must lie in [{min_len}, {N}] (got min {int(lengths.min())}, max {int(lengths.max())})")
            return lengths.to(device=dev).contiguous()
        lengths = lengths.to(device=dev)
        # sync-free, but not silent: out-of-range lengths are counted in a sticky device counter (length_violations() reads it at a
        # moment of the caller's choosing -- end of an eval pass, a stats call), then clamped
        self._count_violations(dev, ((lengths < min_len) | (lengths > N)).sum())
        return lengths.clamp(min=min_len, max=N).contiguous()

    @staticmethod
    def _count_violations(dev, bad: torch.Tensor) -> None:
        # The counter is replaced, not updated in place: a tensor created under torch.inference_mode() is an inference tensor for ever, and an
        # in-place update of it from a later no_grad / grad-mode caller raises.  (The sum below is a tensor of whichever mode the CALLER is in;
        # a value made outside inference mode takes part in inference-mode arithmetic without complaint, the other way round does not -- so the
        # running total is re-made outside inference mode.)  During stream capture the count is skipped: its storage would belong to the graph's pool.
        if not torch.cuda.is_current_stream_capturing():
            with torch.inference_mode(False), torch.no_grad():
                prev = Encoder._violations.get(dev)
                Encoder._violations[dev] = (bad.clone() if prev is None else prev + bad.clone())

    @staticmethod
    def length_violations() -> int:
        """Out-of-range past_lengths (and HSTU delta positions) seen and clamped on the sync-free device path since the process
        started, by either encoder: an upstream data bug when non-zero.  One synchronising read per device."""
        return sum(int(v.item()) for v in Encoder._violations.values())

    # ---- rows of a multi-row decode step ---------------------------------------------------------------------------------
    @staticmethod
    def _parse_row_counts(rows, max_rows, B: int, N: int, names, int_dtypes, upper: str):
        """First half of the row-count contract of a multi-row decode step (SASRec's new_rows / max_new_rows, HSTU's delta_rows /
        max_delta_rows; `names` is that pair, so every message names the caller's arguments) -> (counts, uniform, on_device).
        `max_rows`, when given, is an int in [1, N].  `rows` on the host: an int (uniform True), or B ints as a list or tensor of a
        dtype in `int_dtypes`; they must lie in [1, N] (`upper` words the bound in the message) and come back as an int64 host
        tensor (B,).  A DEVICE tensor needs max_rows, is checked for dtype and shape only and comes back as it is, on_device True:
        M is then max_rows, and what is held against the values, and where violations are counted, is the encoder's.  The encoder
        puts its own checks of host counts between this and _finish_row_counts.  Touches neither a device nor the library."""
        rows_name, max_name = names
        if max_rows is not None and (isinstance(max_rows, bool) or not isinstance(max_rows, int) or not 1 <= max_rows <= N):
            raise ValueError(f"{max_name} must be an int in [1, {N}], got {max_rows!r}")
        if rows is None:
            raise ValueError(f"{max_name} needs {rows_name}=")
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            if max_rows is None:
                raise ValueError(f"{rows_name} on the device needs {max_name}=M (an int): the number of work rows is a host-side launch size")
            if rows.dtype not in int_dtypes or rows.shape != (B,):
                raise ValueError(f"{rows_name} must be an integer tensor of shape ({B},), got {rows.dtype} {tuple(rows.shape)}")
            return rows, False, True
        uniform = isinstance(rows, int) and not isinstance(rows, bool)
        if uniform:
            counts = torch.full((B,), rows, dtype=torch.int64)
        else:
            try:
                counts = torch.as_tensor(rows)
            except (TypeError, ValueError, RuntimeError) as e:
                raise ValueError(f"{rows_name} must be an int, or {B} ints as a list or tensor: {e}") from None
            if counts.dtype not in int_dtypes or counts.shape != (B,):
                raise ValueError(f"{rows_name} must be an integer tensor of shape ({B},), got {counts.dtype} {tuple(counts.shape)}")
            counts = counts.to(torch.int64)
        if B and (int(counts.min()) < 1 or int(counts.max()) > N):
            raise ValueError(f"{rows_name} must lie in [1, {upper}] (got min {int(counts.min())}, max {int(counts.max())}, seq_len {N})")
        return counts, uniform, False

    @staticmethod
    def _finish_row_counts(counts: torch.Tensor, uniform: bool, max_rows, names):
        """Second half, for host counts: `max_rows` must not be less than the largest count -> (counts, M).  M: max_rows, else the
        largest count; counts: None when every sequence has M rows, else the tensor."""
        rows_name, max_name = names
        top = int(counts.max()) if counts.numel() else 1
        if max_rows is not None and max_rows < top:
            raise ValueError(f"{max_name} {max_rows} is less than the largest {rows_name} {top}")
        M = top if max_rows is None else max_rows
        return (None if uniform and M == top else counts), M

    @staticmethod
    def _last_rows(lengths: torch.Tensor, N: int) -> torch.Tensor:
        """Flat row index b * N + lengths[b] - 1 of every sequence's last position."""
        return torch.arange(lengths.shape[0], device=lengths.device, dtype=torch.int64) * N + (lengths - 1)

    # ---- launches ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _f32(dev, keep: list):
        """The staging function of one call's launches: t -> t itself when it already is a contiguous float32 tensor on `dev`,
        otherwise such a copy, appended to `keep`.  The caller holds `keep` until the launches that read the copies are enqueued
        (the caching allocator would otherwise hand the same block to the next conversion before the kernel has run)."""
        def f32(t: torch.Tensor) -> torch.Tensor:
            if t.dtype == torch.float32 and t.device == dev and t.is_contiguous():
                return t
            t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
            keep.append(t)
            return t
        return f32

    @property
    def _postproc_mode(self) -> int:
        return 0 if self._postproc == "layer_norm" else 1   # the C ABI's postproc_mode

    def _normalize(self, x2d: torch.Tensor, rows: Optional[torch.Tensor]) -> torch.Tensor:
        lib = _lib.load()
        n = x2d.shape[0] if rows is None else rows.numel()
        out = torch.empty((n, x2d.shape[1]), dtype=torch.float32, device=x2d.device)
        with _on_device(x2d.device):
            _lib.check(lib.rails_rows_normalize(_ptr(x2d), x2d.stride(0), _ptr(rows) if rows is not None else None, n, x2d.shape[1],
                                                self._postproc_mode, C.c_float(self._eps), _ptr(out), _stream()), "rails_rows_normalize")
        return out
