"""HSTU query encoder, eval path -- the step upstream of the retrieval path.

Mirror of modeling/sequential/hstu.py:HSTU for inference: same constructor arguments that matter at eval time, same
parameter / buffer names (so `load_state_dict` of a reference checkpoint's `module.` entries works unchanged), same
`get_item_embeddings` / `encode` / `forward` signatures.  No fbgemm: the layers run on the padded (B, N, D) tensor with
rows at positions >= length held at zero.  Every floating-point operation runs in the HIP kernels
of csrc/hstu.hip through the C ABI (rails_hstu_preprocess, rails_hstu_time_buckets, rails_rows_layer_norm, rails_gemm_f32,
rails_hstu_attention, rails_rows_normalize); torch only holds the parameters and moves rows (embedding lookup).

Cached incremental decoding (hstu.py:144-213, :276-433, :665-803): `encode` / `generate_user_embeddings` with
`return_cache_states=True` return the reference's per-layer states (v, padded_q, padded_k, outputs); passing them back as `cache`
with `delta_x_offsets = (jagged_rows, positions)` re-encodes one row per sequence against the cached K / V of the others in one
launch of rails_hstu_decode and updates the cache in place.  With `delta_rows=` the same call re-encodes a contiguous run of rows
[position, position + delta_rows) of every sequence in one step of rails_hstu_decode_rows (bit for bit the single-row steps of that
entry at ascending positions); `extend_cache_states` lays a cache out for grown lengths, and its docstring has the append recipe.

Not supported (raises): training mode, `concat_ua`, `normalization="softmax_rel_bias"`, `linear_activation` other than
"silu" / "none", autocast / non-fp32 caches, delta rows of one sequence that are not one contiguous run.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._encoder import (Encoder, L2NormEmbeddingPostprocessor, LayerNormEmbeddingPostprocessor,  # noqa: F401 (re-exported)
                       LearnablePositionalEmbeddingInputFeaturesPreprocessor, LocalEmbeddingModule, parse_args)
from .engine import _on_device, _ptr, _stream

TIMESTAMPS_KEY = "timestamps"
CacheState = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]   # (v, padded_q, padded_k, outputs) of one layer


def _bucket_thresholds(num_buckets: int, max_dt: int = 1 << 62) -> torch.Tensor:
    """thresholds[b - 1] = the smallest |dt| whose bucket floor(log(max(|dt|, 1)) / 0.301) (float32, as hstu.py:611-613
    evaluates it) is >= b.  The attention kernel counts thresholds <= |dt|, which reproduces torch's bucketing exactly."""
    def bucket(x: int) -> int:
        return int((torch.log(torch.tensor([x]).abs().clamp(min=1)) / 0.301).long())
    out = []
    for b in range(1, num_buckets + 1):
        if bucket(max_dt) < b:
            out.append(max_dt + 1)
            continue
        lo, hi = 1, max_dt
        while lo < hi:
            mid = (lo + hi) // 2
            if bucket(mid) >= b:
                hi = mid
            else:
                lo = mid + 1
        out.append(lo)
    return torch.tensor(out, dtype=torch.int64)


class _RelBias(torch.nn.Module):                # RelativeBucketedTimeAndPositionBasedBias (hstu.py:82-138)
    def __init__(self, max_seq_len: int, num_buckets: int) -> None:
        super().__init__()
        self._ts_w = torch.nn.Parameter(torch.empty(num_buckets + 1).normal_(mean=0, std=0.02))
        self._pos_w = torch.nn.Parameter(torch.empty(2 * max_seq_len - 1).normal_(mean=0, std=0.02))


class _Layer(torch.nn.Module):                  # SequentialTransductionUnitJagged (hstu.py:215-437): `_uvqk`, `_o`, `_rel_attn_bias`
    def __init__(self, dim: int, dv: int, dqk: int, heads: int, max_seq_len: int, num_buckets: int, rel_bias: bool) -> None:
        super().__init__()
        self._uvqk = torch.nn.Parameter(torch.empty((dim, dv * 2 * heads + dqk * heads * 2)).normal_(mean=0, std=0.02))
        self._o = torch.nn.Linear(dv * heads, dim)
        torch.nn.init.xavier_uniform_(self._o.weight)
        self._rel_attn_bias = _RelBias(max_seq_len, num_buckets) if rel_bias else None


class _Stack(torch.nn.Module):                  # HSTUJagged: `_attention_layers`
    def __init__(self, layers) -> None:
        super().__init__()
        self._attention_layers = torch.nn.ModuleList(layers)


class HSTU(Encoder):
    """encode(past_lengths (B,), past_ids (B, N), past_embeddings (B, N, D), past_payloads {"timestamps": (B, N)}) -> (B, D).
    N must equal max_sequence_len + max_output_len (what the reference's eval feeds, modeling/sequential/features.py:48-58)."""

    NAME = "HSTU"
    _SIGNATURES = ((["normalization", "linear_config", "linear_activation", "linear_dropout_rate", "attn_dropout_rate", "embedding_module",
                     "similarity_module", "input_features_preproc_module", "output_postproc_module", "enable_relative_attention_bias",
                     "concat_ua", "verbose"], dict(enable_relative_attention_bias=True, concat_ua=False, verbose=True)),
                   (["num_items", "similarity_module", "normalization", "linear_config", "linear_activation", "output_postproc",
                     "enable_relative_attention_bias", "concat_ua", "num_buckets", "eps"],
                    dict(similarity_module=None, normalization="rel_bias", linear_config="uvqk", linear_activation="silu",
                         output_postproc="layer_norm", enable_relative_attention_bias=True, concat_ua=False, num_buckets=128, eps=1e-6)))

    def __init__(self, max_sequence_len: int, max_output_len: int, embedding_dim: int, num_blocks: int, num_heads: int, linear_dim: int,
                 attention_dim: int, *args, **kwargs) -> None:
        """Two signatures:
          the reference's (modeling/sequential/hstu.py:544-565) -- ..., normalization, linear_config, linear_activation,
            linear_dropout_rate, attn_dropout_rate, embedding_module, similarity_module, input_features_preproc_module,
            output_postproc_module, enable_relative_attention_bias=True, concat_ua=False, verbose=True -- with rails_amd's
            LocalEmbeddingModule / LearnablePositionalEmbeddingInputFeaturesPreprocessor / {L2Norm,LayerNorm}EmbeddingPostprocessor
            (or any objects with the same attributes), so encoder_utils.py needs only its imports swapped;
          the compact one -- ..., num_items, similarity_module=None, normalization="rel_bias", linear_config="uvqk",
            linear_activation="silu", output_postproc="layer_norm", enable_relative_attention_bias=True, concat_ua=False,
            num_buckets=128, eps=1e-6."""
        reference_style = "embedding_module" in kwargs or (len(args) > 0 and isinstance(args[0], str))
        a = parse_args("HSTU", args, kwargs, reference_style, *self._SIGNATURES)
        if a["normalization"] not in ("rel_bias", "hstu_rel_bias") or a["linear_config"] != "uvqk" or a["concat_ua"]:
            raise NotImplementedError("only normalization='rel_bias', linear_config='uvqk', concat_ua=False are built")
        if a["linear_activation"] not in ("silu", "none"):
            raise ValueError(f"Unknown linear_activation {a['linear_activation']}")
        seq = max_sequence_len + max_output_len
        super().__init__(a, reference_style, seq, embedding_dim, num_blocks, num_heads)
        self._max_sequence_length = max_sequence_len
        self._dqk, self._dv = attention_dim, linear_dim
        self._linear_activation = a["linear_activation"]
        self._num_buckets = num_buckets = 128 if reference_style else a["num_buckets"]
        self._hstu = _Stack([_Layer(embedding_dim, linear_dim, attention_dim, num_heads, seq, num_buckets, a["enable_relative_attention_bias"])
                             for _ in range(num_blocks)])
        self.register_buffer("_bucket_thresholds", _bucket_thresholds(num_buckets), persistent=False)

    # ---- reference API ------------------------------------------------------------------------------------------
    def forward(self, past_lengths, past_ids, past_embeddings, past_payloads: Dict[str, torch.Tensor], batch_id=None) -> torch.Tensor:
        """(B, N, D) postprocessed sequence embeddings (hstu.py:711-739); rows at positions >= length are zero rows
        normalised, exactly as the reference's zero-padded output."""
        x = self._run_layers(past_lengths, past_ids, past_embeddings, past_payloads, min_len=0)
        B, N, D = x.shape
        return self._normalize(x.view(B * N, D), None).view(B, N, D)

    def encode(self, past_lengths, past_ids, past_embeddings, past_payloads: Dict[str, torch.Tensor], delta_x_offsets=None, cache=None,
               return_cache_states: bool = False, delta_rows=None, max_delta_rows: Optional[int] = None) -> torch.Tensor:
        """(B, D): the postprocessed embedding at position past_lengths - 1 (hstu.py:741-803).
        return_cache_states=True: (current embeddings, per-layer states) -- the per-layer route runs (the fused kernel keeps its
        intermediates in LDS).  delta_x_offsets = (jagged_rows (B,), positions (B,)) with `cache`: re-encode one row per sequence
        (rails_hstu_decode), updating the cache in place; the result is the last layer's cached outputs row at past_lengths - 1, as
        in the reference (a delta at an earlier position leaves it as it was).  A `cache` without delta_x_offsets is ignored.
        delta_rows (with delta_x_offsets and cache): re-encode the run of rows [positions[b], positions[b] + m_b) of every sequence in one
        step (rails_hstu_decode_rows); delta_x_offsets then names the run's first row.  An int m >= 1, or m_b per sequence as a list or
        a tensor (B,); the run must end at or below past_lengths.  Counts on the host are validated there and the step runs
        max(m_b) slots per sequence (max_delta_rows if given; no bit depends on it); counts on the device need max_delta_rows=M, are
        clamped on the device into [1, min(M, length - position)], counted in length_violations(), and never read back.  To APPEND
        rows see extend_cache_states."""
        self._delta_rows_need(delta_rows, max_delta_rows, delta_x_offsets, cache)
        if delta_x_offsets is not None:
            cur, states, _ = self._decode(past_lengths, past_ids, past_embeddings, past_payloads, delta_x_offsets, cache, delta_rows, max_delta_rows)
            return (cur, states) if return_cache_states else cur
        if return_cache_states:
            states = []
            x = self._run_layers(past_lengths, past_ids, past_embeddings, past_payloads, states=states)
            B, N, D = x.shape
            return self._normalize(x.view(B * N, D), self._last_rows(self._lengths(past_lengths, x.device, N), N)), states
        if self.use_fused_kernel:
            out = self._encode_fused(past_lengths, past_ids, past_embeddings, past_payloads)
            if out is not None:
                return out
        x = self._run_layers(past_lengths, past_ids, past_embeddings, past_payloads)
        B, N, D = x.shape
        return self._normalize(x.view(B * N, D), self._last_rows(self._lengths(past_lengths, x.device, N), N))

    def generate_user_embeddings(self, past_lengths, past_ids, past_embeddings, past_payloads: Dict[str, torch.Tensor], delta_x_offsets=None,
                                 cache=None, return_cache_states: bool = False, delta_rows=None,
                                 max_delta_rows: Optional[int] = None) -> Tuple[torch.Tensor, List[CacheState]]:
        """(postprocessed (B, N, D), states) as hstu.py:665-703: the states list is [] unless return_cache_states.  With
        delta_x_offsets and cache the (B, N, D) is the last layer's cached outputs (updated in place) padded and postprocessed;
        delta_rows / max_delta_rows as in encode."""
        self._delta_rows_need(delta_rows, max_delta_rows, delta_x_offsets, cache)
        if delta_x_offsets is None:
            states: Optional[list] = [] if return_cache_states else None
            x = self._run_layers(past_lengths, past_ids, past_embeddings, past_payloads, min_len=0, states=states)
            B, N, D = x.shape
            return self._normalize(x.view(B * N, D), None).view(B, N, D), (states if return_cache_states else [])
        _, states, lengths = self._decode(past_lengths, past_ids, past_embeddings, past_payloads, delta_x_offsets, cache, delta_rows, max_delta_rows)
        B, N = past_ids.shape
        D = self._embedding_dim
        out = states[-1][3]
        dev = out.device
        # the jagged outputs padded to (B, N, D): rows at positions >= length are zero rows (data movement only)
        padded = torch.zeros((B * N, D), dtype=torch.float32, device=dev)
        pos = torch.arange(N, device=dev).unsqueeze(0)
        valid = pos < lengths.unsqueeze(1)
        starts = torch.cumsum(lengths, 0) - lengths
        src = (starts.unsqueeze(1) + pos).clamp(max=max(out.shape[0] - 1, 0))
        padded[valid.view(-1)] = out[src[valid]]
        y = self._normalize(padded, None).view(B, N, D)
        return y, (states if return_cache_states else [])

    def _encode_fused(self, past_lengths, past_ids, past_embeddings, past_payloads) -> Optional[torch.Tensor]:
        """Single-launch encoder for short sequences (rails_hstu_encode_fused): one workgroup per sequence, everything in LDS.
        None when the geometry does not fit (the per-layer kernels then run)."""
        self._check(past_ids, past_embeddings)
        lib = _lib.load()
        B, N = past_ids.shape
        D, H, dqk, dv = self._embedding_dim, self._num_heads, self._dqk, self._dv
        layers = list(self._hstu._attention_layers)
        if self._linear_activation != "silu":
            return None
        if not lib.rails_hstu_fused_supported(N, D, H, dqk, dv, self._num_buckets):
            return None
        dev = past_embeddings.device
        ts = past_payloads.get(TIMESTAMPS_KEY) if past_payloads else None
        has_bias = ts is not None and all(l._rel_attn_bias is not None for l in layers)
        if ts is not None and not has_bias and any(l._rel_attn_bias is not None for l in layers):
            return None        # mixed bias / no-bias layers: leave to the general path
        keep = []              # copies staged to fp32 live until the launch is enqueued
        f32 = self._f32(dev, keep)
        params = [(l._uvqk, l._o.weight, l._o.bias) + ((l._rel_attn_bias._ts_w, l._rel_attn_bias._pos_w) if has_bias else ()) for l in layers]
        self._fused_ptrs = _lib.layer_table(_lib.HstuLayer, [[f32(t) for t in p] for p in params], dev, self._fused_ptrs)
        lengths = self._lengths(past_lengths, dev, N)
        ids = past_ids.to(device=dev, dtype=torch.int64).contiguous()
        emb = f32(past_embeddings)
        pos = f32(self._input_features_preproc._pos_emb.weight)
        out = torch.empty((B, D), dtype=torch.float32, device=dev)
        with _on_device(dev):
            st = _stream()
            buckets = None
            if has_bias:
                ts = ts.to(device=dev, dtype=torch.int64).contiguous()
                buckets = torch.empty((B, N, N), dtype=torch.uint8, device=dev)
                _lib.check(lib.rails_hstu_time_buckets(_ptr(ts), B, N, _ptr(self._bucket_thresholds.to(dev)), self._num_buckets, _ptr(buckets), st),
                           "rails_hstu_time_buckets")
            _lib.check(lib.rails_hstu_encode_fused(_ptr(emb), _ptr(ids), _ptr(lengths), _ptr(buckets) if has_bias else None, _ptr(pos),
                                                   _ptr(self._fused_ptrs[1]), len(layers), B, N, D, H, dqk, dv, self._num_buckets,
                                                   self._postproc_mode, C.c_float(self._eps), _ptr(out), st), "rails_hstu_encode_fused")
        return out

    # ---- HIP path ------------------------------------------------------------------------------------------------
    def _run_layers(self, past_lengths, past_ids, past_embeddings, past_payloads, min_len: int = 1, states: Optional[list] = None) -> torch.Tensor:
        self._check(past_ids, past_embeddings)
        lib = _lib.load()
        dev = past_embeddings.device
        B, N = past_ids.shape
        D, H, dqk, dv = self._embedding_dim, self._num_heads, self._dqk, self._dv
        keep = []   # fp32 copies of non-fp32 parameters must outlive the launches that read them
        f32 = self._f32(dev, keep)
        lengths = self._lengths(past_lengths, dev, N, min_len)
        ids = past_ids.to(device=dev, dtype=torch.int64).contiguous()
        ts = past_payloads.get(TIMESTAMPS_KEY) if past_payloads else None
        if ts is not None:
            ts = ts.to(device=dev, dtype=torch.int64).contiguous()
        emb = f32(past_embeddings)
        M, W = B * N, 2 * H * (dv + dqk)
        x = torch.empty((B, N, D), dtype=torch.float32, device=dev)
        nx = torch.empty((M, D), dtype=torch.float32, device=dev)
        mm = torch.empty((M, W), dtype=torch.float32, device=dev)
        att = torch.empty((M, H * dv), dtype=torch.float32, device=dev)
        oin = torch.empty((M, H * dv), dtype=torch.float32, device=dev)
        thr = self._bucket_thresholds.to(dev)
        if states is not None:   # the reference's cache states: flat indices of the jagged rows (one host read of the lengths)
            lh = lengths.cpu()
            jag = (torch.arange(B).unsqueeze(1) * N + torch.arange(N).unsqueeze(0))[torch.arange(N).unsqueeze(0) < lh.unsqueeze(1)].to(dev)
            HV, HQ = H * dv, H * dqk
        has_bias = ts is not None and any(l._rel_attn_bias is not None for l in self._hstu._attention_layers)
        buckets = torch.empty((B, N, N), dtype=torch.uint8, device=dev) if has_bias else None
        with _on_device(dev):
            st = _stream()
            if has_bias:   # the time buckets depend on neither layer nor head: once per call
                _lib.check(lib.rails_hstu_time_buckets(_ptr(ts), B, N, _ptr(thr), self._num_buckets, _ptr(buckets), st), "rails_hstu_time_buckets")
            _lib.check(lib.rails_hstu_preprocess(_ptr(emb), _ptr(ids), _ptr(lengths), _ptr(f32(self._input_features_preproc._pos_emb.weight)),
                                                 B, N, D, C.c_float(float(D) ** 0.5), _ptr(x), st), "rails_hstu_preprocess")
            for layer in self._hstu._attention_layers:
                x2 = x.view(M, D)
                _lib.check(lib.rails_rows_layer_norm(_ptr(x2), D, M, D, C.c_float(self._eps), None, 0, _ptr(nx), D, st), "rails_rows_layer_norm")
                _lib.check(lib.rails_gemm_f32(_ptr(nx), D, _ptr(f32(layer._uvqk)), 0, None, None, 0, M, W, D,
                                              1 if self._linear_activation == "silu" else 0, _ptr(lengths), N, _ptr(mm), W, st), "rails_gemm_f32")
                rb = layer._rel_attn_bias
                use_bias = ts is not None and rb is not None
                _lib.check(lib.rails_hstu_attention(_ptr(mm), W, B, N, H, dqk, dv, _ptr(lengths), _ptr(buckets) if use_bias else None,
                                                    _ptr(f32(rb._ts_w)) if use_bias else None, _ptr(f32(rb._pos_w)) if use_bias else None,
                                                    self._num_buckets if use_bias else 0, _ptr(att), st),
                           "rails_hstu_attention")
                # o_input = u * LN(attn);  u = the first H*dv columns of mm
                _lib.check(lib.rails_rows_layer_norm(_ptr(att), H * dv, M, H * dv, C.c_float(self._eps), _ptr(mm), W, _ptr(oin), H * dv, st),
                           "rails_rows_layer_norm")
                xn = torch.empty((B, N, D), dtype=torch.float32, device=dev)
                _lib.check(lib.rails_gemm_f32(_ptr(oin), H * dv, _ptr(f32(layer._o.weight)), 1, _ptr(f32(layer._o.bias)), _ptr(x2), D, M, D, H * dv,
                                              0, _ptr(lengths), N, _ptr(xn), D, st), "rails_gemm_f32")
                x = xn
                if states is not None:   # (v jagged, padded_q, padded_k, outputs jagged); mm rows past the lengths are zero
                    states.append((mm[jag, HV: 2 * HV].contiguous(), mm[:, 2 * HV: 2 * HV + HQ].contiguous().view(B, N, HQ),
                                   mm[:, 2 * HV + HQ: 2 * HV + 2 * HQ].contiguous().view(B, N, HQ), xn.view(M, D)[jag]))
        return x

    # ---- cached incremental decoding ------------------------------------------------------------------------------
    def _decode_rows(self, delta_x_offsets, lengths: torch.Tensor, past_lengths: torch.Tensor, dev, B: int, N: int) -> torch.Tensor:
        """The delta positions (B,) int64 on the device.  Host-resident offsets (or STRICT_DEVICE_LENGTHS) are checked: jagged_rows[b]
        must be x_offsets[b] + positions[b] with 0 <= positions[b] < lengths[b].  Device-resident ones are checked on the device without
        a sync: violations are counted in length_violations() and the position is clamped into [0, length).  The kernel derives the
        jagged row from the lengths and the position, so the caller's rows never address a write."""
        if not isinstance(delta_x_offsets, (tuple, list)) or len(delta_x_offsets) != 2:
            raise ValueError("delta_x_offsets must be a pair (jagged_rows (B,), positions (B,))")
        rows_in, pos_in = (torch.as_tensor(t) for t in delta_x_offsets)
        if rows_in.shape != (B,) or pos_in.shape != (B,) or rows_in.dtype not in (torch.int32, torch.int64) or pos_in.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"delta_x_offsets must hold two int32 / int64 tensors of shape ({B},)")
        if not (rows_in.is_cuda and pos_in.is_cuda) or type(self).STRICT_DEVICE_LENGTHS:
            lh, r, p = past_lengths.to(dtype=torch.int64).cpu(), rows_in.to(dtype=torch.int64).cpu(), pos_in.to(dtype=torch.int64).cpu()
            off = torch.cumsum(lh, 0) - lh
            if bool(((p < 0) | (p >= lh)).any()):
                b = int(((p < 0) | (p >= lh)).nonzero()[0])
                raise ValueError(f"delta position {int(p[b])} of sequence {b} is outside [0, {int(lh[b])})")
            if not torch.equal(r, off + p):
                b = int((r != off + p).nonzero()[0])
                raise ValueError(f"delta jagged row {int(r[b])} of sequence {b} is not x_offsets[b] + position = {int(off[b] + p[b])}")
            return p.to(device=dev).contiguous()
        r, p = rows_in.to(device=dev, dtype=torch.int64), pos_in.to(device=dev, dtype=torch.int64)
        off = torch.cumsum(lengths, 0) - lengths
        self._count_violations(dev, ((p < 0) | (p >= lengths) | (r != off + p)).sum())
        return torch.minimum(p.clamp(min=0), lengths - 1).contiguous()

    def _check_cache(self, cache, B: int, N: int, dev, lengths_host: Optional[torch.Tensor]) -> int:
        """Host-side checks of the per-layer states; returns the jagged row count they share."""
        H, dqk, dv, D = self._num_heads, self._dqk, self._dv, self._embedding_dim
        layers = self._hstu._attention_layers
        if cache is None:
            raise ValueError("delta_x_offsets needs the cache states of an earlier call (return_cache_states=True)")
        if not isinstance(cache, (list, tuple)) or len(cache) != len(layers):
            raise ValueError(f"cache must hold one (v, padded_q, padded_k, outputs) state per layer: {len(layers)}, "
                             f"got {len(cache) if isinstance(cache, (list, tuple)) else type(cache).__name__}")
        rows = None
        for i, state in enumerate(cache):
            if not isinstance(state, (list, tuple)) or len(state) != 4:
                raise ValueError(f"cache[{i}] must be a 4-tuple (v, padded_q, padded_k, outputs)")
            for name, t in zip(("v", "padded_q", "padded_k", "outputs"), state):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                    raise ValueError(f"cache[{i}] {name} must be a contiguous float32 tensor on {dev}")
            v, q, k, out = state
            if rows is None:
                rows = v.shape[0] if v.dim() == 2 else -1
            if v.shape != (rows, H * dv) or out.shape != (rows, D):
                raise ValueError(f"cache[{i}]: v {tuple(v.shape)} / outputs {tuple(out.shape)} must be ({rows}, {H * dv}) / ({rows}, {D})")
            for name, t in (("padded_q", q), ("padded_k", k)):
                if t.numel() != B * N * H * dqk or t.shape[-1] != H * dqk:
                    raise ValueError(f"cache[{i}] {name} {tuple(t.shape)} must be ({B}, {N}, {H * dqk})")
        if lengths_host is not None and rows != int(lengths_host.sum()):
            raise ValueError(f"the cache holds {rows} jagged rows, the lengths sum to {int(lengths_host.sum())}")
        if rows < B:
            raise ValueError(f"the cache holds {rows} jagged rows for {B} sequences")
        return rows

    @staticmethod
    def _delta_rows_need(delta_rows, max_delta_rows, delta_x_offsets, cache) -> None:
        if (delta_rows is not None or max_delta_rows is not None) and (delta_x_offsets is None or cache is None):
            raise ValueError("delta_rows / max_delta_rows need delta_x_offsets= and cache=")

    def _delta_counts(self, delta_rows, max_delta_rows, delta_x_offsets, past_lengths, B: int, N: int):
        """(counts, M, checked) of a multi-row step, without touching a device unless the data lives there: counts an int64 tensor (B,)
        (on the host, or the caller's device tensor), or None for M rows of every sequence; checked: the runs were held against the
        lengths here.  Raises for whatever the host can see; the rest is counted and clamped on the device (Encoder._parse_row_counts
        and _finish_row_counts hold the contract SASRec's new_rows shares; the runs against the lengths are this encoder's)."""
        names = ("delta_rows", "max_delta_rows")
        counts, uniform, on_device = self._parse_row_counts(delta_rows, max_delta_rows, B, N, names, (torch.int32, torch.int64),
                                                            "past_lengths - position")
        if on_device:
            return counts, max_delta_rows, False
        counts, M = self._finish_row_counts(counts, uniform, max_delta_rows, names)
        pos = delta_x_offsets[1] if isinstance(delta_x_offsets, (tuple, list)) and len(delta_x_offsets) == 2 else None
        pos = torch.as_tensor(pos) if pos is not None else None
        checked = pos is not None and pos.shape == (B,) and ((not past_lengths.is_cuda and not pos.is_cuda) or type(self).STRICT_DEVICE_LENGTHS)
        if checked:
            lh, p = past_lengths.to(dtype=torch.int64).cpu(), pos.to(dtype=torch.int64).cpu()
            ends = p + (M if counts is None else counts)   # counts None: M rows of every sequence
            if bool((ends > lh).any()):
                b = int((ends > lh).nonzero()[0])
                raise ValueError(f"delta rows [{int(p[b])}, {int(ends[b])}) of sequence {b} end past its length {int(lh[b])}")
        return counts, M, checked

    def extend_cache_states(self, cache, old_lengths, new_lengths) -> List[CacheState]:
        """The states of `cache` (laid out for old_lengths) laid out for new_lengths: every jagged `v` / `outputs` becomes (sum new, .)
        with each sequence's old rows at its new offset and its new rows zero; padded_q / padded_k are the same tensors.  Pure row
        movement, on host lengths.  ValueError unless 1 <= old <= new <= N elementwise and the cache holds sum(old) rows.

        To APPEND len_new - len_old events: extend the cache, then decode the run [len_old - 1, len_new), that is
        delta_x_offsets = (new offsets + len_old - 1, len_old - 1) and delta_rows = len_new - len_old + 1, with the ids, embeddings and
        timestamps of the grown sequences.  The run starts one row BELOW the first new one because the relative bias gives query row p
        the timestamp of row p + 1 (ts[min(p + 1, N - 1)]): row len_old - 1 was encoded against whatever the padding held at
        ts[len_old], so its attention, and with it every deeper k / v of that row, changes when the sequence grows.  Decoded from
        len_old - 1 the step equals a prefill at the new lengths; decoded from len_old it does not wherever timestamps are used."""
        old, new = (torch.as_tensor(t).to(dtype=torch.int64).cpu() for t in (old_lengths, new_lengths))
        N = self._seq
        if old.dim() != 1 or old.shape != new.shape:
            raise ValueError(f"old_lengths {tuple(old.shape)} and new_lengths {tuple(new.shape)} must be two (B,) vectors")
        if bool(((old < 1) | (old > new) | (new > N)).any()):
            b = int(((old < 1) | (old > new) | (new > N)).nonzero()[0])
            raise ValueError(f"sequence {b}: 1 <= old length {int(old[b])} <= new length {int(new[b])} <= {N} does not hold")
        if not isinstance(cache, (list, tuple)) or not all(isinstance(s, (list, tuple)) and len(s) == 4 for s in cache):
            raise ValueError("cache must hold one (v, padded_q, padded_k, outputs) state per layer")
        total_old, total_new = int(old.sum()), int(new.sum())
        for i, (v, _, _, out) in enumerate(cache):
            if v.dim() != 2 or out.dim() != 2 or v.shape[0] != total_old or out.shape[0] != total_old:
                raise ValueError(f"cache[{i}]: v {tuple(v.shape)} / outputs {tuple(out.shape)} must hold the {total_old} rows the old lengths sum to")
        # jagged row of old row j of sequence b under the new lengths
        seq = torch.repeat_interleave(torch.arange(old.numel()), old)
        dst = torch.arange(total_old) + ((torch.cumsum(new, 0) - new) - (torch.cumsum(old, 0) - old))[seq]
        states = []
        for v, q, k, out in cache:
            idx = dst.to(v.device)
            nv = torch.zeros((total_new, v.shape[1]), dtype=v.dtype, device=v.device)
            no = torch.zeros((total_new, out.shape[1]), dtype=out.dtype, device=out.device)
            nv[idx] = v
            no[idx] = out
            states.append((nv, q, k, no))
        return states

    def _decode(self, past_lengths, past_ids, past_embeddings, past_payloads, delta_x_offsets, cache, delta_rows=None, max_delta_rows=None):
        """One rails_hstu_decode launch (one rails_hstu_decode_rows step with delta_rows) -> ((B, D) current embeddings, the cache's
        own states, the device lengths)."""
        multi = delta_rows is not None or max_delta_rows is not None
        counts = None
        if multi:   # whatever the host can refuse is refused before the device and the library are touched
            self._check(past_ids, past_embeddings, device=False)
            counts, M, counts_checked = self._delta_counts(delta_rows, max_delta_rows, delta_x_offsets, past_lengths, *past_ids.shape)
        self._check(past_ids, past_embeddings)
        lib = _lib.load()
        dev = past_embeddings.device
        B, N = past_ids.shape
        D, H, dqk, dv = self._embedding_dim, self._num_heads, self._dqk, self._dv
        if multi:
            if not lib.rails_hstu_decode_rows_supported(N, D, H, dqk, dv, self._num_buckets):
                raise NotImplementedError(f"multi-row cached decoding supports dim <= 1024, dqk <= 32, dv <= 32, heads * dv <= 1024 and <= 255 "
                                          f"buckets (got dim {D}, {H} heads, dqk {dqk}, dv {dv}, {self._num_buckets} buckets)")
            if B * M > _lib.RAILS_HSTU_DECODE_MAX_ROWS:
                raise ValueError(f"a decode step runs at most {_lib.RAILS_HSTU_DECODE_MAX_ROWS} work rows (batch x max delta rows), got {B} x {M}")
        elif not lib.rails_hstu_decode_supported(N, D, H, dqk, dv, self._num_buckets):
            raise NotImplementedError(f"cached decoding supports dim <= 1024, dqk <= 32, dv <= 32 and <= 255 buckets within its LDS bound "
                                      f"(got dim {D}, {H} heads, dqk {dqk}, dv {dv}, {self._num_buckets} buckets)")
        # host-side checks of the cache's row count whenever the lengths or the offsets are on the host (the latter read the lengths anyway)
        host_check = not past_lengths.is_cuda or type(self).STRICT_DEVICE_LENGTHS or not (
            isinstance(delta_x_offsets, (tuple, list)) and all(isinstance(t, torch.Tensor) and t.is_cuda for t in delta_x_offsets))
        lengths = self._lengths(past_lengths, dev, N)
        rows = self._check_cache(cache, B, N, dev, past_lengths.to(dtype=torch.int64).cpu() if host_check else None)
        positions = self._decode_rows(delta_x_offsets, lengths, past_lengths, dev, B, N)
        keep = []
        f32 = self._f32(dev, keep)
        ids = past_ids.to(device=dev, dtype=torch.int64).contiguous()
        emb = f32(past_embeddings)
        ts = past_payloads.get(TIMESTAMPS_KEY) if past_payloads else None
        if ts is not None:
            ts = ts.to(device=dev, dtype=torch.int64).contiguous()
        table = []
        for layer, (v, q, k, out) in zip(self._hstu._attention_layers, cache):
            rb = layer._rel_attn_bias
            bias = (f32(rb._ts_w), f32(rb._pos_w)) if (rb is not None and ts is not None) else (None, None)
            table.append((f32(layer._uvqk), f32(layer._o.weight), f32(layer._o.bias), *bias, v, q, k, out))
        self._decode_ptrs = _lib.layer_table(_lib.HstuDecodeLayer, table, dev, self._decode_ptrs)
        thr = self._bucket_thresholds.to(dev)
        res = torch.empty((B, D), dtype=torch.float32, device=dev)
        if multi:
            if counts is not None or not counts_checked:
                c = torch.full((B,), M, dtype=torch.int64, device=dev) if counts is None else counts.to(device=dev, dtype=torch.int64).contiguous()
                if not counts_checked:   # the scan kernel clamps these; nothing is read back
                    bad = (c < 1) | (c > (lengths - positions).clamp(max=M))
                    if type(self).STRICT_DEVICE_LENGTHS and bool(bad.any()):
                        raise ValueError(f"delta_rows must lie in [1, min(max_delta_rows, past_lengths - position)] (got min {int(c.min())}, max {int(c.max())})")
                    self._count_violations(dev, bad.sum())
                counts = None if counts is None else c
            work = torch.empty(lib.rails_hstu_decode_rows_workspace_floats(B * M, B, D, H, dqk, dv), dtype=torch.float32, device=dev)
            with _on_device(dev):
                _lib.check(lib.rails_hstu_decode_rows(_ptr(emb), _ptr(ids), _ptr(positions), _ptr(counts) if counts is not None else None, M,
                                                      _ptr(lengths), _ptr(ts), _ptr(thr) if ts is not None else None,
                                                      _ptr(f32(self._input_features_preproc._pos_emb.weight)), _ptr(self._decode_ptrs[1]), len(table),
                                                      B, N, rows, D, H, dqk, dv, self._num_buckets, 1 if self._linear_activation == "silu" else 0,
                                                      self._postproc_mode, C.c_float(self._eps), _ptr(work), _ptr(res), _stream()),
                           "rails_hstu_decode_rows")
            return res, [(v, q.view(B, N, H * dqk), k.view(B, N, H * dqk), out) for v, q, k, out in cache], lengths
        with _on_device(dev):
            _lib.check(lib.rails_hstu_decode(_ptr(emb), _ptr(ids), _ptr(positions), _ptr(lengths), _ptr(ts), _ptr(thr) if ts is not None else None,
                                             _ptr(f32(self._input_features_preproc._pos_emb.weight)), _ptr(self._decode_ptrs[1]), len(table), B, N,
                                             rows, D, H, dqk, dv, self._num_buckets, 1 if self._linear_activation == "silu" else 0,
                                             self._postproc_mode, C.c_float(self._eps), _ptr(res), _stream()),
                       "rails_hstu_decode")
        states = [(v, q.view(B, N, H * dqk), k.view(B, N, H * dqk), out) for v, q, k, out in cache]
        return res, states, lengths
