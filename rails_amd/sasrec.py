"""SASRec query encoder, eval path -- the other encoder of the paper's configs (`train_fn.main_module = "SASRec"`).

Mirror of modeling/sequential/sasrec.py:SASRec for inference: the reference's constructor call, its parameter / buffer names
(`attention_layers.{i}.in_proj_weight` ..., `forward_layers.{i}._conv1d.{0,3}.*`, `_attn_mask`), so that `load_state_dict` of a
reference checkpoint works unchanged, and its `get_item_embeddings` / `forward` / `encode` signatures.  Every floating-point
operation runs in the HIP kernels of csrc/sasrec.hip and csrc/hstu.hip through the C ABI (rails_hstu_preprocess,
rails_rows_layer_norm, rails_gemm_f32, rails_sasrec_attention, rails_gemm_f32_id_masked, rails_rows_normalize; or the single-launch
rails_sasrec_encode_fused); torch only holds the parameters and moves rows (embedding lookup).

The reference's quirks are kept: the id mask (ids != 0) is the only mask -- rows past `past_lengths` with a nonzero id are valid
rows of forward(), and a masked position is still a key of every later query (its key / value row is the in-projection bias).

Cached incremental decoding (encode with `cache=`): a prefill with return_cache_states=True also returns every
block's key / value rows; a decode step re-encodes row lengths - 1 of every sequence against them in rails_sasrec_decode (5 launches
per block over the whole batch) and writes that row's k / v into the cache in place.  The attention is strictly causal and the id
mask is per row, so the step equals encode() of the updated sequence up to fp32 summation order.  With `new_rows=` one step
re-encodes the last m_b rows of every sequence (rails_sasrec_decode_rows, the same launches): an append of several events, or an
edit of an interior row.

Not supported (raises): training mode, CPU tensors.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib
from ._encoder import Encoder, parse_args
from .engine import _on_device, _ptr, _stream

BLOCK_LN_EPS = 1e-8     # F.layer_norm(..., eps=1e-8) inside every block (sasrec.py:195-212)
_ACT = {"relu": _lib.RAILS_ACT_RELU, "gelu": _lib.RAILS_ACT_GELU}
_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


class _MultiheadAttention(torch.nn.Module):
    """Parameter holder with torch.nn.MultiheadAttention's state_dict (embed_dim == kdim == vdim, bias, no bias_k / bias_v)."""

    def __init__(self, dim: int, num_heads: int) -> None:
        super().__init__()
        if dim % num_heads != 0:
            raise ValueError(f"embedding_dim {dim} must be divisible by num_heads {num_heads}")
        self.embed_dim, self.num_heads = dim, num_heads
        self.in_proj_weight = torch.nn.Parameter(torch.empty(3 * dim, dim))
        self.in_proj_bias = torch.nn.Parameter(torch.zeros(3 * dim))
        self.out_proj = torch.nn.Linear(dim, dim)
        torch.nn.init.xavier_normal_(self.in_proj_weight)
        torch.nn.init.xavier_normal_(self.out_proj.weight)


class _FeedForward(torch.nn.Module):
    """StandardAttentionFF's parameters: `_conv1d` = [Conv1d(D, F, 1), act, Dropout, Conv1d(F, D, 1), Dropout]."""

    def __init__(self, dim: int, hidden_dim: int, activation_fn: str) -> None:
        super().__init__()
        self._conv1d = torch.nn.Sequential(
            torch.nn.Conv1d(dim, hidden_dim, kernel_size=1),
            torch.nn.GELU() if activation_fn == "gelu" else torch.nn.ReLU(),
            torch.nn.Dropout(p=0.0),
            torch.nn.Conv1d(hidden_dim, dim, kernel_size=1),
            torch.nn.Dropout(p=0.0),
        )


class SASRec(Encoder):
    """encode(past_lengths (B,), past_ids (B, N), past_embeddings (B, N, D), past_payloads) -> (B, D);
    forward(...) -> (B, N, D).  N must equal max_sequence_len + max_output_len."""

    NAME = "SASRec"
    _SIGNATURES = ((["ffn_dropout_rate", "embedding_module", "similarity_module", "input_features_preproc_module", "output_postproc_module",
                     "activation_checkpoint", "verbose"], dict(activation_checkpoint=False, verbose=False)),
                   (["num_items", "similarity_module", "output_postproc", "eps"], dict(similarity_module=None, output_postproc="layer_norm", eps=1e-6)))

    def __init__(self, max_sequence_len: int, max_output_len: int, embedding_dim: int, num_blocks: int, num_heads: int,
                 ffn_hidden_dim: int, ffn_activation_fn: str = "relu", *args, **kwargs) -> None:
        """Two signatures:
          the reference's (modeling/sequential/sasrec.py) -- ..., ffn_activation_fn, ffn_dropout_rate, embedding_module,
            similarity_module, input_features_preproc_module, output_postproc_module, activation_checkpoint=False,
            verbose=False -- with rails_amd's LocalEmbeddingModule / LearnablePositionalEmbeddingInputFeaturesPreprocessor /
            {L2Norm,LayerNorm}EmbeddingPostprocessor (or any objects with the same attributes);
          the compact one -- ..., ffn_activation_fn="relu", num_items, similarity_module=None, output_postproc="layer_norm",
            eps=1e-6."""
        reference_style = "embedding_module" in kwargs or (len(args) >= 2 and isinstance(args[1], torch.nn.Module))
        a = parse_args("SASRec", args, kwargs, reference_style, *self._SIGNATURES)
        if ffn_activation_fn not in _ACT:
            raise ValueError(f"Invalid activation_fn {ffn_activation_fn}")
        seq = max_sequence_len + max_output_len
        super().__init__(a, reference_style, seq, embedding_dim, num_blocks, num_heads)
        self._max_sequence_length = seq
        self._ffn_hidden_dim, self._ffn_activation_fn = ffn_hidden_dim, ffn_activation_fn
        self.attention_layers = torch.nn.ModuleList([_MultiheadAttention(embedding_dim, num_heads) for _ in range(num_blocks)])
        self.forward_layers = torch.nn.ModuleList([_FeedForward(embedding_dim, ffn_hidden_dim, ffn_activation_fn) for _ in range(num_blocks)])

    # ---- reference API ------------------------------------------------------------------------------------------
    def debug_str(self) -> str:
        return (f"SASRec-d{self._embedding_dim}-b{self._num_blocks}-h{self._num_heads}-{self._input_features_preproc.debug_str()}-"
                f"{self._output_postproc.debug_str()}-ffn{self._ffn_hidden_dim}-{self._ffn_activation_fn}")

    def forward(self, past_lengths, past_ids, past_embeddings, past_payloads: Optional[Dict[str, torch.Tensor]] = None,
                batch_id=None) -> torch.Tensor:
        """(B, N, D) postprocessed sequence embeddings (sasrec.py generate_user_embeddings).  Lengths play no part here, as in the
        reference: every position with a nonzero id is a valid row."""
        self._check(past_ids, past_embeddings)
        x = self._run_layers(past_ids, past_embeddings)
        B, N, D = past_embeddings.shape
        return self._normalize(x, None).view(B, N, D)

    def encode(self, past_lengths, past_ids, past_embeddings, past_payloads: Optional[Dict[str, torch.Tensor]] = None, cache=None,
               return_cache_states: bool = False, new_rows=None, max_new_rows: Optional[int] = None):
        """(B, D): the postprocessed embedding at position past_lengths - 1 (modeling/sequential/utils.py:74-90).  Lengths follow
        the encoders' policy (Encoder._lengths): host lengths outside [1, N] raise, device lengths are clamped and
        counted (length_violations()).

        return_cache_states=True without a cache (prefill): (emb, cache) from the per-layer route, emb bitwise that of
        use_fused_kernel=False; cache[i] = (k, v), contiguous float32 (B, N, D): block i's in-projection key / value rows of its input.
        With a cache (decode step): row p = past_lengths - 1 of every sequence is re-encoded through every block against cache rows
        0..p-1 and its k / v written to cache row p in place (rows > p untouched); only past_ids / past_embeddings at row p are read.
        Returns the (B, D) embedding of row p, or (emb, cache) with return_cache_states=True -- the same tensors, updated.

        new_rows (with a cache only): several rows per sequence in the one step (rails_sasrec_decode_rows).  The last m_b rows of
        sequence b, positions past_lengths[b] - m_b .. past_lengths[b] - 1, are re-encoded in order and cache rows
        [len_b - m_b, len_b) written in place; every other cache row keeps its bits, only past_ids / past_embeddings at those rows
        are read, and the result is still the (B, D) embedding at len_b - 1 -- bit for bit that of m_b single-row steps.  Two uses:
          append -- past_lengths grew by m_b since the cache was last written (m_b = past_lengths[b] on an empty cache: a prefill);
          edit from an interior row p -- past_lengths unchanged, new_rows = len_b - p: the rows from the edited one on are re-encoded.
        new_rows is None (one row, the call above), an int m >= 1 (the last m rows of every sequence), or m_b per sequence as a list /
        integer tensor (B,).  Counts on the HOST are validated there (1 <= m_b <= past_lengths[b] when the lengths are on the host
        too; ValueError before anything is launched) and the step runs max(m_b) work-row slots per sequence, or max_new_rows when that
        is given (no bit depends on it).  A DEVICE tensor needs max_new_rows=M, an int: its values are clamped on the device into
        [1, min(M, len_b)] and the out-of-range ones counted in length_violations(), like lengths; nothing is read back unless
        STRICT_DEVICE_LENGTHS is set."""
        if cache is None and (new_rows is not None or max_new_rows is not None):
            raise ValueError("new_rows / max_new_rows select the rows of a decode step: they need cache=")
        if new_rows is None and max_new_rows is not None:
            raise ValueError("max_new_rows sizes a new_rows= step: it needs new_rows=")
        if cache is not None:
            out = self._decode(past_lengths, past_ids, past_embeddings, cache, new_rows, max_new_rows)
            return (out, cache) if return_cache_states else out
        self._check(past_ids, past_embeddings, device=False)
        N = past_ids.shape[1]
        lengths = self._lengths(past_lengths, past_embeddings.device, N)
        self._check_device(past_embeddings)
        if return_cache_states:   # the per-layer route: the fused kernel keeps K / V in LDS
            states = []
            x = self._run_layers(past_ids, past_embeddings, states)
            return self._normalize(x, self._last_rows(lengths, N)), states
        if self.use_fused_kernel:
            out = self._encode_fused(lengths, past_ids, past_embeddings)
            if out is not None:
                return out
        x = self._run_layers(past_ids, past_embeddings)
        return self._normalize(x, self._last_rows(lengths, N))

    # ---- HIP path ------------------------------------------------------------------------------------------------
    def _block_params(self):
        """Per block, in rails_sasrec_layer's order: in_proj_weight, in_proj_bias, out_proj weight / bias, conv1 weight / bias, conv2
        weight / bias (Conv1d weights (out, in, 1) read as (out, in) Linear weights)."""
        for att, ff in zip(self.attention_layers, self.forward_layers):
            c1, c2 = ff._conv1d[0], ff._conv1d[3]
            yield (att.in_proj_weight, att.in_proj_bias, att.out_proj.weight, att.out_proj.bias, c1.weight, c1.bias, c2.weight, c2.bias)

    def _encode_fused(self, lengths, past_ids, past_embeddings) -> Optional[torch.Tensor]:
        """Single-launch encoder (rails_sasrec_encode_fused).  None when the geometry does not fit (the per-layer kernels then run)."""
        lib = _lib.load()
        B, N = past_ids.shape
        D, H, F = self._embedding_dim, self._num_heads, self._ffn_hidden_dim
        if not lib.rails_sasrec_fused_supported(N, D, H, F):
            return None
        dev = past_embeddings.device
        keep = []   # copies staged to fp32 live until the launch is enqueued
        f32 = self._f32(dev, keep)
        self._fused_ptrs = _lib.layer_table(_lib.SasrecLayer, [[f32(t) for t in p] for p in self._block_params()], dev, self._fused_ptrs)
        ids = past_ids.to(device=dev, dtype=torch.int64).contiguous()
        emb = f32(past_embeddings)
        pos = f32(self._input_features_preproc._pos_emb.weight)
        out = torch.empty((B, D), dtype=torch.float32, device=dev)
        with _on_device(dev):
            _lib.check(lib.rails_sasrec_encode_fused(_ptr(emb), _ptr(ids), _ptr(lengths), _ptr(pos), _ptr(self._fused_ptrs[1]), self._num_blocks,
                                                     B, N, D, H, F, _ACT[self._ffn_activation_fn], self._postproc_mode, C.c_float(self._eps),
                                                     _ptr(out), _stream()), "rails_sasrec_encode_fused")
        return out

    def _run_layers(self, past_ids, past_embeddings, states: Optional[list] = None) -> torch.Tensor:
        """The block stack on the (B * N, D) rows; returns the last block's output (before the postprocessor).  `states`: a list
        that receives each block's (k, v) rows as contiguous (B, N, D) copies."""
        lib = _lib.load()
        dev = past_embeddings.device
        B, N = past_ids.shape
        D, H, F = self._embedding_dim, self._num_heads, self._ffn_hidden_dim
        M = B * N
        eps = C.c_float(BLOCK_LN_EPS)
        act = _ACT[self._ffn_activation_fn]
        keep = []   # fp32 copies must outlive the launches that read them
        f32 = self._f32(dev, keep)
        layers = [[f32(t) for t in p] for p in self._block_params()]
        ids = past_ids.to(device=dev, dtype=torch.int64).contiguous()
        emb = f32(past_embeddings)
        pos = f32(self._input_features_preproc._pos_emb.weight)
        full = torch.full((B,), N, dtype=torch.int64, device=dev)   # the mask is ids != 0 alone
        x = torch.empty((M, D), dtype=torch.float32, device=dev)
        qn = torch.empty((M, D), dtype=torch.float32, device=dev)
        qkv = torch.empty((M, 3 * D), dtype=torch.float32, device=dev)
        att = torch.empty((M, D), dtype=torch.float32, device=dev)
        y = torch.empty((M, D), dtype=torch.float32, device=dev)
        hid = torch.empty((M, F), dtype=torch.float32, device=dev)
        with _on_device(dev):
            st = _stream()
            _lib.check(lib.rails_hstu_preprocess(_ptr(emb), _ptr(ids), _ptr(full), _ptr(pos), B, N, D, C.c_float(float(D) ** 0.5), _ptr(x), st),
                       "rails_hstu_preprocess")
            for w_in, b_in, w_o, b_o, w1, b1, w2, b2 in layers:
                # Q = LN(x);  q = Q W_q^T + b_q;  [k | v] = x W_kv^T + b_kv  (no row mask: masked rows are keys too)
                _lib.check(lib.rails_rows_layer_norm(_ptr(x), D, M, D, eps, None, 0, _ptr(qn), D, st), "rails_rows_layer_norm")
                _lib.check(lib.rails_gemm_f32(_ptr(qn), D, _ptr(w_in), 1, _ptr(b_in), None, 0, M, D, D, 0, None, 0, _ptr(qkv), 3 * D, st),
                           "rails_gemm_f32")
                _lib.check(lib.rails_gemm_f32(_ptr(x), D, w_in.data_ptr() + 4 * D * D, 1, b_in.data_ptr() + 4 * D, None, 0, M, 2 * D, D, 0, None, 0,
                                              qkv.data_ptr() + 4 * D, 3 * D, st), "rails_gemm_f32")
                if states is not None:
                    states.append((qkv[:, D:2 * D].reshape(B, N, D).contiguous(), qkv[:, 2 * D:].reshape(B, N, D).contiguous()))
                _lib.check(lib.rails_sasrec_attention(_ptr(qkv), 3 * D, B, N, D, H, _ptr(att), st), "rails_sasrec_attention")
                # y = Q + a W_o^T + b_o;  z = LN(y);  x = (act(z W_1^T + b_1) W_2^T + b_2 + z) * (ids != 0)
                _lib.check(lib.rails_gemm_f32(_ptr(att), D, _ptr(w_o), 1, _ptr(b_o), _ptr(qn), D, M, D, D, 0, None, 0, _ptr(y), D, st), "rails_gemm_f32")
                _lib.check(lib.rails_rows_layer_norm(_ptr(y), D, M, D, eps, None, 0, _ptr(qn), D, st), "rails_rows_layer_norm")
                _lib.check(lib.rails_gemm_f32(_ptr(qn), D, _ptr(w1), 1, _ptr(b1), None, 0, M, F, D, act, None, 0, _ptr(hid), F, st), "rails_gemm_f32")
                _lib.check(lib.rails_gemm_f32_id_masked(_ptr(hid), F, _ptr(w2), 1, _ptr(b2), _ptr(qn), D, M, D, F, 0, _ptr(ids), _ptr(x), D, st),
                           "rails_gemm_f32_id_masked")
        return x

    # ---- cached incremental decoding ------------------------------------------------------------------------------
    def _check_cache(self, cache, B: int, N: int, dev) -> None:
        """Host-side checks of the per-block (k, v) states: no device read."""
        D = self._embedding_dim
        if not isinstance(cache, (list, tuple)) or len(cache) != self._num_blocks:
            raise ValueError(f"cache must hold one (k, v) pair per block: {self._num_blocks}, "
                             f"got {len(cache) if isinstance(cache, (list, tuple)) else type(cache).__name__}")
        for i, state in enumerate(cache):
            if not isinstance(state, (list, tuple)) or len(state) != 2:
                raise ValueError(f"cache[{i}] must be a pair (k, v)")
            for name, t in zip("kv", state):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                    raise ValueError(f"cache[{i}] {name} must be a contiguous float32 tensor on {dev}")
                if t.shape != (B, N, D):
                    raise ValueError(f"cache[{i}] {name} {tuple(t.shape)} must be ({B}, {N}, {D})")

    def _new_rows(self, new_rows, max_new_rows, past_lengths, lengths: torch.Tensor, B: int, N: int):
        """(counts, M) of a multi-row step: counts an int64 device tensor (B,), or None for M rows of every sequence.  `lengths`:
        _lengths' result (on the device, in range).  Counts on the host raise here when out of range; counts on the device are
        counted, the kernels clamp them, and nothing is read back (unless STRICT_DEVICE_LENGTHS)."""
        dev = lengths.device
        strict = type(self).STRICT_DEVICE_LENGTHS
        names = ("new_rows", "max_new_rows")
        counts, uniform, on_device = self._parse_row_counts(new_rows, max_new_rows, B, N, names, _INT_DTYPES, "past_lengths")
        if on_device:
            M = max_new_rows
            counts = counts.to(device=dev, dtype=torch.int64).contiguous()
            bad = (counts < 1) | (counts > lengths.clamp(max=M))
            if strict:
                if bool(bad.any()):
                    raise ValueError(f"new_rows must lie in [1, min(max_new_rows, past_lengths)] (got min {int(counts.min())}, max {int(counts.max())})")
            else:
                self._count_violations(dev, bad.sum())
            return counts, M
        # the lengths host counts are held against: the host's own, device lengths only when strict
        len_h = past_lengths.to(torch.int64) if not past_lengths.is_cuda else lengths.cpu() if strict else None
        if len_h is not None and bool((counts > len_h).any()):
            b = int((counts > len_h).nonzero()[0])
            raise ValueError(f"new_rows must lie in [1, past_lengths]: sequence {b} has {int(counts[b])} new rows and length {int(len_h[b])}")
        counts, M = self._finish_row_counts(counts, uniform, max_new_rows, names)
        if counts is not None:
            counts = counts.to(dev)
        if len_h is None:   # device lengths: a count past a sequence's length is clamped by the kernels, and counted here
            self._count_violations(dev, (lengths < (M if counts is None else counts)).sum())
        return counts, M

    def _decode(self, past_lengths, past_ids, past_embeddings, cache, new_rows=None, max_new_rows: Optional[int] = None) -> torch.Tensor:
        """One decode step (rails_sasrec_decode; rails_sasrec_decode_rows with new_rows) -> (B, D); the cache is updated in place.
        With device-resident lengths (and counts) nothing here reads the device."""
        self._check(past_ids, past_embeddings)
        lib = _lib.load()
        B, N = past_ids.shape
        D, H, F = self._embedding_dim, self._num_heads, self._ffn_hidden_dim
        if not lib.rails_sasrec_decode_supported(N, D, H, F):
            raise NotImplementedError(f"cached decoding supports seq_len <= 2048, embedding_dim and ffn_hidden_dim <= 1024 and head_dim <= 64 "
                                      f"(got seq_len {N}, embedding_dim {D}, {H} heads, ffn_hidden_dim {F})")
        dev = past_embeddings.device
        self._check_cache(cache, B, N, dev)
        lengths = self._lengths(past_lengths, dev, N)
        counts, M = (None, 1) if new_rows is None else self._new_rows(new_rows, max_new_rows, past_lengths, lengths, B, N)
        if B * M > _lib.RAILS_SASREC_DECODE_MAX_ROWS:
            raise NotImplementedError(f"a decode step runs at most {_lib.RAILS_SASREC_DECODE_MAX_ROWS} work rows (batch x max new rows), "
                                      f"got {B} x {M}")
        keep = []   # fp32 copies must outlive the launches that read them
        f32 = self._f32(dev, keep)
        self._decode_ptrs = _lib.layer_table(_lib.SasrecDecodeLayer, [[f32(t) for t in p] + [k, v] for p, (k, v) in zip(self._block_params(), cache)],
                                             None, self._decode_ptrs)   # a HOST array
        ids = past_ids.to(device=dev, dtype=torch.int64).contiguous()
        emb = f32(past_embeddings)
        pos = f32(self._input_features_preproc._pos_emb.weight)
        work = torch.empty(lib.rails_sasrec_decode_workspace_floats(B * M, D, F), dtype=torch.float32, device=dev)
        out = torch.empty((B, D), dtype=torch.float32, device=dev)
        tail = (self._decode_ptrs[1], self._num_blocks, B, N, D, H, F, _ACT[self._ffn_activation_fn], self._postproc_mode, C.c_float(self._eps),
                _ptr(work), _ptr(out))
        with _on_device(dev):
            if new_rows is None:
                _lib.check(lib.rails_sasrec_decode(_ptr(emb), _ptr(ids), _ptr(lengths), _ptr(pos), *tail, _stream()), "rails_sasrec_decode")
            else:
                _lib.check(lib.rails_sasrec_decode_rows(_ptr(emb), _ptr(ids), _ptr(lengths), _ptr(counts) if counts is not None else None, M,
                                                        _ptr(pos), *tail, _stream()), "rails_sasrec_decode_rows")
        return out
