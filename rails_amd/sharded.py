"""Item-sharded MoL top-k (exact, and the two-pass approximate one): one process per GPU, one small all-gather per batch.

The reference has no sharded retrieval (eval is asserted single-GPU, eval_from_checkpoint.py:554-555); this
is the north-star's 8-GPU path.  Its oracle is "equals single-device brute force over the concatenated
corpus", which holds bit for bit because (a) per-pair arithmetic does not depend on the shard and
(b) selection uses the total order (score desc, global position asc) at both levels.

  rank r owns items [r * ceil(N/R), min(N, (r+1) * ceil(N/R)))      (contiguous item-id ranges)
  queries and MoL weights are replicated (KBs); every rank redoes the query prologue
  per batch: local scoring -> local top-k -> ONE all_gather of B*k*16 bytes -> merge R*k -> k on every rank

ShardedMoLAvgTopK (BASELINE config 5: 1 B items 8-way, coarse prefilter + MoL rerank) has the same shape: every rank
runs MoLAvgTopK on its shard -- coarse top-K' of ITS items, full MoL on those, local top-k -- and the merge is the same,
because what is merged are exact MoL scores.  It reranks R*K' candidates in total (K' per shard), a superset-quality
variant of the single-device algorithm with the same K'; it equals it exactly when R = 1.

ShardedMoLAvgTopK(global_k_prime=True) is the single-device algorithm itself on a sharded corpus:
one more all-gather first exchanges every shard's coarse top-K' (coarse score bits | global position), every rank
selects the GLOBAL coarse top-K' with the same total order (score desc, global position asc), reranks only its own
members of it, and the usual merge follows.  Bit-identical to MoLAvgTopK(avg_top_k = K') over the whole corpus.

ShardedMoLNaiveTopK / ShardedMoLCombTopK shard the per-component candidate generators the same two ways: per shard (the single-device
module on every shard, one all-gather) and, with global_candidates=True, the single-device algorithm itself -- the ranks exchange their
per-group (and coarse) candidate lists as 64-bit keys, every rank selects the global lists and reranks its own members of the union.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import contextlib

import torch
import torch.distributed as dist

from . import engine as E
from .topk_modules import MoLAvgTopK, MoLBruteForceTopK, MoLCombTopK, MoLNaiveTopK, TopKModule, _checked_positions, refuse_allowed_tags, refuse_collapse_groups, refuse_diversity, refuse_generic_candidates, refuse_item_mask

_GENERIC_WHY = "the single-device module runs there, and ShardedMoLBruteForceTopK shards the exact pass"

_TAGS_WHY = ("tags belong to the positions of ONE corpus and the sharded wrappers split theirs over the ranks: every rank would have to hold its slice "
             "of the tags and the global candidate counts would have to follow the filter (out of scope, DESIGN section 3.15); the single-device modules take it")
_MASK_WHY = "a mask is by position of ONE corpus and the sharded wrappers split theirs over the ranks (out of scope, DESIGN section 3.13)"
_RANK_WHY = ("the exact rank of an item is built on the single-device MoLBruteForceTopK: a sharded one would be a local count plus one sum all-reduce, "
             "and needs the target's key on every rank (out of scope, DESIGN section 3.17)")
_SOFTMAX_WHY = ("the softmax over the corpus is built on the single-device MoLBruteForceTopK: a sharded one would merge the shards' (max, sum) pairs, "
                "which combine associatively, in one all-gather (out of scope, DESIGN section 3.18)")
_PAIRS_WHY = ("scoring caller-given items is built on the single-device modules: a sharded one would route each pair to the rank that owns the item and "
              "gather the scores (out of scope, DESIGN section 3.22)")
_RANGE_WHY = ("the range search is built on the single-device MoLBruteForceTopK: a sharded one would gather the shards' ragged results and merge each "
              "row's sorted runs (out of scope, DESIGN section 3.19)")


def shard_bounds(n_items: int, world_size: int, rank: int) -> Tuple[int, int]:
    per = (n_items + world_size - 1) // world_size
    lo = min(n_items, rank * per)
    return lo, min(n_items, lo + per)


def route_update_positions(global_positions: torch.Tensor, lo: int, hi: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Global -> local routing of an update on the shard that owns the global positions [lo, hi): -> (local positions, rows), `rows` being the
    indices into the update (its embedding / id rows) that fall inside the shard, in the order given; everything else is another shard's."""
    p = global_positions.reshape(-1).to(torch.int64)
    rows = torch.nonzero((p >= lo) & (p < hi)).reshape(-1)
    return p[rows] - lo, rows


def pack_candidates(scores: torch.Tensor, ids: torch.Tensor, k: int) -> torch.Tensor:
    """(B, k_local) fp32 scores + int64 ids -> one (B, 2k) int64 message (score bits | ids); rows shorter than
    k are padded with -inf / id -1 so every rank sends the same size."""
    B, kl = scores.shape
    if kl < k:
        scores = torch.cat([scores, scores.new_full((B, k - kl), float("-inf"))], 1)
        ids = torch.cat([ids, ids.new_full((B, k - kl), -1)], 1)
    return torch.cat([scores.contiguous().view(torch.int32).to(torch.int64), ids], 1)


def unpack_candidates(msg: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(R, B, 2k) gathered messages -> (B, R*k) scores and ids in shard-major order."""
    R, B, _ = msg.shape
    scores = msg[:, :, :k].to(torch.int32).view(torch.float32)
    ids = msg[:, :, k:]
    return scores.permute(1, 0, 2).reshape(B, R * k).contiguous(), ids.permute(1, 0, 2).reshape(B, R * k).contiguous()


def _hip_merge(scores: torch.Tensor, ids: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return E.topk(scores, k, ids=ids)


class ShardedTopK(TopKModule):
    """forward(query_embeddings, k) -> (scores (B, k), ids (B, k)), identical on every rank: the local module's top-k of
    every shard, merged.  `local_topk` / `merge` default to the HIP kernels; the CPU tests of the collective logic inject
    oracle-backed callables instead (gloo, world_size 2)."""

    EXCHANGE_WITH_ONE_RANK = False

    def _make_local_module(self, mol_module, item_embeddings_shard, item_ids_shard) -> TopKModule:
        raise NotImplementedError

    def __init__(
        self,
        mol_module,
        item_embeddings_shard: Optional[torch.Tensor],
        item_ids_shard: Optional[torch.Tensor],
        n_items_total: int,
        group: Optional[dist.ProcessGroup] = None,
        local_topk: Optional[Callable[..., Tuple[torch.Tensor, torch.Tensor]]] = None,
        merge: Optional[Callable[[torch.Tensor, torch.Tensor, int], Tuple[torch.Tensor, torch.Tensor]]] = None,
    ) -> None:
        super().__init__()
        self._group = group
        self._world = dist.get_world_size(group) if dist.is_initialized() else 1
        # one shard = the local module's own result, no exchange -- unless EXCHANGE_WITH_ONE_RANK (a test setting: a one-GPU box runs the whole
        # exchange path -- RCCL all-gather on the exchange stream, merge, global verdict -- in a process group of one rank)
        self._exchange = self._world > 1 or (self.EXCHANGE_WITH_ONE_RANK and dist.is_initialized())
        self._n_total = n_items_total
        if local_topk is None:
            self._local_module = self._make_local_module(mol_module, item_embeddings_shard, item_ids_shard)
            self._n_local = self._local_module.num_items
            local_topk = lambda q, k, **kw: self._local_module(q, k=k, **kw)  # noqa: E731
            self._local_topk_is_module = True
        else:
            self._local_module = None
            self._n_local = int(item_ids_shard.numel())
            self._local_topk_is_module = False
        self._local_topk = local_topk
        self._merge = merge if merge is not None else _hip_merge

    def forward(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        refuse_item_mask(self, kwargs, _MASK_WHY)
        refuse_allowed_tags(self, kwargs, _TAGS_WHY)
        refuse_collapse_groups(self, kwargs)
        refuse_diversity(self, kwargs)
        with self._inline():     # a plain call has no neighbouring batch to overlap with (MoLAvgTopK.submit)
            return self.result(self.submit(query_embeddings, k, sorted, **kwargs))

    # The exchange (all-gather + merge) runs on the caller's stream.  On a second stream, concurrently with the next batch's scoring, it was
    # measured through the real module in a one-rank nccl group (tools/r06_shard_rccl_probe.py, 8-way shard, profiles/r06_shard_rccl_probe.txt):
    # the two stream hand-overs per step cost more than the overlap gains (0.474 against 0.455 ms for the plain call); with everything on the
    # caller's stream, submit / result two batches ahead keeps the device queue full across the host's look at the verdict with no hand-over.
    _plain_call = False

    def _join_submit(self, device, ready) -> None:
        """result() of an explicit submit() may be called on another stream than the one submit() ran on: wait for its event there
        (a plain call's exchange follows on the very stream of its submit)."""
        if not self._plain_call and ready is not None:
            torch.cuda.current_stream(device).wait_event(ready)

    def _all_gather_rows(self, msg: torch.Tensor) -> torch.Tensor:
        """(B, W) -> (world * B, W), rank-major: concatenated along dim 0, the layout both RCCL and gloo accept for all_gather_into_tensor.
        Device tensors on a gloo group (test setups only) are staged through the host."""
        if msg.is_cuda and dist.get_backend(self._group) == "gloo":
            host = torch.empty((self._world * msg.shape[0], msg.shape[1]), dtype=msg.dtype)
            dist.all_gather_into_tensor(host, msg.cpu(), group=self._group)
            return host.to(msg.device)
        out = torch.empty((self._world * msg.shape[0], msg.shape[1]), dtype=msg.dtype, device=msg.device)
        dist.all_gather_into_tensor(out, msg, group=self._group)
        return out

    @contextlib.contextmanager
    def _inline(self):
        """A plain forward / forward_filtered: there is no neighbouring batch to overlap with, so the local module stays on the caller's stream
        (MoLAvgTopK.inline_calls) and so does the exchange -- every hand-over between streams is an event the GPU waits 5-12 us for (round 6:
        two of them per step on an 8-way shard's 0.44 ms)."""
        local = self._local_module
        saved = self._plain_call
        self._plain_call = True
        try:
            with (local.inline_calls() if hasattr(local, "inline_calls") else contextlib.nullcontext()):
                yield
        finally:
            self._plain_call = saved

    # ---- two-stage form of forward: submit() enqueues this rank's part, result() the exchange ------------------------------
    # A caller that has the next batch at hand calls submit(batch i+1) BEFORE result(batch i): the all-gather and the merge of
    # batch i then run on a second stream while batch i+1's prologue and scoring occupy the first ("overlap
    # it with the next batch's scoring").  Same kernels, same order of arithmetic: the output is bit-equal to forward's.
    def submit(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs):
        """Local scoring + local top-k + pack on the current stream -> handle for result()."""
        refuse_item_mask(self, kwargs, _MASK_WHY)
        refuse_allowed_tags(self, kwargs, _TAGS_WHY)
        refuse_collapse_groups(self, kwargs)
        refuse_diversity(self, kwargs)
        if k > self._n_total:
            raise RuntimeError(f"selected index k out of range (k={k}, n={self._n_total})")
        k_local = min(k, self._n_local)
        local = self._local_module
        spec = None   # a local module with its own submit / result (MoLAvgTopK): its speculative output travels on, verified in result()
        if k_local > 0 and local is not None and hasattr(local, "submit") and self._local_topk_is_module:
            spec = local.submit(query_embeddings, k_local, **kwargs)
            s, ids = spec[1], spec[2]
            if spec[0] == "final":
                spec = None
            elif self._exchange and s.is_cuda and isinstance(spec[-1], torch.cuda.Stream):
                # the local call ran on a stream of its own and the pack below reads its output here: join it now (with one shard
                # nothing reads it before result(), and batches overlap)
                torch.cuda.current_stream(s.device).wait_event(spec[4])
        elif k_local > 0:
            s, ids = self._local_topk(query_embeddings, k_local, **kwargs)
        else:  # an empty shard still takes part in the collective
            B = query_embeddings.size(0)
            s = torch.empty((B, 0), dtype=torch.float32, device=query_embeddings.device)
            ids = torch.empty((B, 0), dtype=torch.int64, device=query_embeddings.device)
        if not self._exchange:
            return ("done", s, ids, spec)
        on_gpu = s.is_cuda and self._merge is _hip_merge
        msg = E.pack_candidates(s, ids, k) if on_gpu else pack_candidates(s.float(), ids, k)
        ready = None
        if msg.is_cuda:
            ready = torch.cuda.Event()
            ready.record()
        return ("pending", msg, ready, k, on_gpu, s.dtype, spec)

    def forward_filtered(self, query_embeddings: torch.Tensor, k_prime: int, invalid_ids: torch.Tensor, k: int, **kwargs):
        """CandidateIndex.get_top_k_outputs' body for the sharded modules: the seen-id filter runs inside the merge launch
        (rails_merge_candidates_filtered) -> (top_k_ids (B, k), top_k_scores (B, k)), or None when the sizes are outside the fused path
        or the merge is not the HIP one (the caller then composes forward + filter_seen_ids: same bits)."""
        refuse_item_mask(self, kwargs, _MASK_WHY)
        refuse_allowed_tags(self, kwargs, _TAGS_WHY)
        refuse_collapse_groups(self, kwargs)
        refuse_diversity(self, kwargs)
        if not self._exchange:
            local = self._local_module
            return local.forward_filtered(query_embeddings, k_prime, invalid_ids, k, **kwargs) if hasattr(local, "forward_filtered") else None
        if not (query_embeddings.is_cuda and self._merge is _hip_merge and E.merge_filter_fusable(k_prime, invalid_ids.shape[1], k)) or k_prime > self._n_total:
            return None
        with self._inline():
            return self.result(self.submit(query_embeddings, k_prime, **kwargs), seen=(invalid_ids, k))

    def result(self, handle, seen=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """All-gather of the per-shard candidates + merge -> (scores, ids), identical on every rank.  On the GPU both run on this
        module's exchange stream, behind the handle's event; the current stream waits for the merge only.
        seen = (invalid_ids, k): the seen-id filter inside the merge launch -> (ids (B, k), scores (B, k)) instead (GPU merge only)."""
        if handle[0] == "done":
            s, ids = handle[1], handle[2]
            if handle[3] is not None:
                s, ids = self._local_module.result(handle[3])     # the verified output (the same tensors unless the call was redone)
            if seen is not None:
                return E.filter_seen_ids(ids, s, seen[0], seen[1])
            return s, ids
        _, msg, ready, k, on_gpu, dtype, spec = handle
        if spec is not None:
            s, ids = self._local_module.result(spec)
            if s is not spec[1]:                                   # redone on the materialising path: pack again
                msg = E.pack_candidates(s, ids, k) if on_gpu else pack_candidates(s.float(), ids, k)
                if msg.is_cuda:
                    ready = torch.cuda.Event()
                    ready.record()
        if seen is not None and not (msg.is_cuda and on_gpu):
            raise RuntimeError("result(seen=...) needs the HIP merge")
        if not msg.is_cuda:
            gathered = self._all_gather_rows(msg)
            all_s, all_ids = unpack_candidates(gathered.view(self._world, msg.shape[0], msg.shape[1]), k)
            ms, mi = self._merge(all_s, all_ids, k)
            return ms.to(dtype), mi
        self._join_submit(msg.device, ready)
        gathered = self._all_gather_rows(msg)
        if on_gpu and seen is not None:   # one kernel: rank-major candidates -> exact top-k -> seen-id filter
            mi, ms = E.merge_candidates_filtered(gathered, self._world, k, k, seen[0], seen[1])
        elif on_gpu:   # one kernel: rank-major candidates -> exact top-k (scores, ids)
            ms, mi = E.merge_candidates(gathered, self._world, k, k)
        else:
            all_s, all_ids = unpack_candidates(gathered.view(self._world, msg.shape[0], msg.shape[1]), k)
            ms, mi = self._merge(all_s, all_ids, k)
        ms = ms.to(dtype)
        if seen is not None:
            return mi, ms
        return ms, mi

    # ---- in-place corpus changes (topk_modules.MoLTopKModule.update_items) ----------------------------------------------------------
    def shard_range(self) -> Tuple[int, int]:
        """[lo, hi): the global positions this rank owns."""
        lo = getattr(self, "_offset", None)
        if lo is None:
            rank = dist.get_rank(self._group) if dist.is_initialized() else 0
            lo = shard_bounds(self._n_total, self._world, rank)[0]
        return int(lo), int(lo) + self._n_local

    def update_items(self, global_positions: torch.Tensor, item_embeddings: torch.Tensor, item_ids: Optional[torch.Tensor] = None) -> None:
        """MoLTopKModule.update_items on an item-sharded corpus, called ALIKE on every rank with GLOBAL positions ((M,) int64, unique, inside
        [0, n_items_total)): each rank applies the positions inside its shard range to its local module (route_update_positions) and ignores the
        rest.  No collective is issued (what the ranks agree on collectively -- the global proof's guard -- is agreed again at the next call)."""
        local = self._local_module
        if local is None or not hasattr(local, "update_items"):
            raise NotImplementedError(f"{type(self).__name__}.update_items needs the HIP local module")
        emb = item_embeddings[0] if torch.is_tensor(item_embeddings) and item_embeddings.dim() == 3 and item_embeddings.shape[0] == 1 else item_embeddings
        if not torch.is_tensor(emb) or emb.dim() != 2:
            raise ValueError("item_embeddings must be (M, D) or (1, M, D)")
        host = _checked_positions(global_positions, emb.shape[0], self._n_total).cpu()
        if item_ids is not None and (not torch.is_tensor(item_ids) or item_ids.numel() != emb.shape[0]):
            raise ValueError(f"item_ids must hold {emb.shape[0]} ids")
        if emb.shape[0] == 0:
            return
        lo, hi = self.shard_range()
        local_pos, rows = route_update_positions(host, lo, hi)
        if rows.numel():
            pick = rows.to(emb.device)
            local.update_items(local_pos, emb.index_select(0, pick), None if item_ids is None else item_ids.reshape(-1).index_select(0, rows.to(item_ids.device)))
        else:
            local._update_rows_arg(emb, None if item_ids is None else item_ids.reshape(-1))       # the same argument errors on every rank
        self._after_local_update()

    def _after_local_update(self) -> None:
        pass

    def append_items(self, item_embeddings: torch.Tensor, item_ids: torch.Tensor) -> None:
        raise NotImplementedError(f"{type(self).__name__}.append_items: growing an item-sharded corpus would move the shard bounds; build the shards again")

    def remove_items(self, positions: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError(f"{type(self).__name__}.remove_items: shrinking an item-sharded corpus would move the shard bounds; build the shards again")

    # ---- exact ranks, the softmax over the corpus, range search (DESIGN sections 3.17 - 3.19): not built on the item-sharded wrappers ----------
    def _refuse_streaming(self, what: str, why: str):
        raise NotImplementedError(f"{type(self).__name__}.{what}: {why}")

    def rank_of(self, query_embeddings: torch.Tensor, target_ids: torch.Tensor, invalid_ids=None, **kwargs):
        self._refuse_streaming("rank_of", _RANK_WHY)

    def rank_of_positions(self, query_embeddings: torch.Tensor, positions: torch.Tensor, invalid_ids=None, **kwargs):
        self._refuse_streaming("rank_of_positions", _RANK_WHY)

    def log_partition(self, query_embeddings: torch.Tensor, invalid_ids=None, temperature: float = 1.0, **kwargs):
        self._refuse_streaming("log_partition", _SOFTMAX_WHY)

    def log_prob_of(self, query_embeddings: torch.Tensor, target_ids: torch.Tensor, invalid_ids=None, temperature: float = 1.0, **kwargs):
        self._refuse_streaming("log_prob_of", _SOFTMAX_WHY)

    def log_prob_of_positions(self, query_embeddings: torch.Tensor, positions: torch.Tensor, invalid_ids=None, temperature: float = 1.0, **kwargs):
        self._refuse_streaming("log_prob_of_positions", _SOFTMAX_WHY)

    def sample_items(self, query_embeddings: torch.Tensor, num_samples: int, seed: int, temperature: float = 1.0, invalid_ids=None, **kwargs):
        self._refuse_streaming("sample_items", _SOFTMAX_WHY)

    def count_above(self, query_embeddings: torch.Tensor, min_score=None, *, min_log_prob=None, temperature: float = 1.0, invalid_ids=None, **kwargs):
        self._refuse_streaming("count_above", _RANGE_WHY)

    def range_search(self, query_embeddings: torch.Tensor, min_score=None, *, min_log_prob=None, temperature: float = 1.0, invalid_ids=None,
                     sort: bool = True, **kwargs):
        self._refuse_streaming("range_search", _RANGE_WHY)

    # ---- score_of / explain_of: not built on the item-sharded wrappers ------------------------------------------------------
    def score_of(self, query_embeddings: torch.Tensor, item_ids: torch.Tensor, invalid_ids=None, **kwargs):
        self._refuse_streaming("score_of", _PAIRS_WHY)

    def score_of_positions(self, query_embeddings: torch.Tensor, positions: torch.Tensor, invalid_ids=None, **kwargs):
        self._refuse_streaming("score_of_positions", _PAIRS_WHY)

    def explain_of(self, query_embeddings: torch.Tensor, item_ids: torch.Tensor, invalid_ids=None, **kwargs):
        self._refuse_streaming("explain_of", _PAIRS_WHY)

    def explain_of_positions(self, query_embeddings: torch.Tensor, positions: torch.Tensor, invalid_ids=None, **kwargs):
        self._refuse_streaming("explain_of_positions", _PAIRS_WHY)

    # ---- hidden items: not built on the item-sharded wrappers -------------------------------------------------------
    def _refuse_hidden(self, what: str):
        raise NotImplementedError(f"{type(self).__name__}.{what}: a hidden set is not built on the item-sharded wrappers (every rank would have to hold its "
                                  "slice of one set, and the global candidate counts would have to follow it); the single-device modules take it")

    def hide_items(self, positions: torch.Tensor) -> None:
        self._refuse_hidden("hide_items")

    def unhide_items(self, positions: torch.Tensor) -> None:
        self._refuse_hidden("unhide_items")

    def hide_items_by_id(self, item_ids: torch.Tensor) -> None:
        self._refuse_hidden("hide_items_by_id")

    def unhide_items_by_id(self, item_ids: torch.Tensor) -> None:
        self._refuse_hidden("unhide_items_by_id")

    def hidden_positions(self) -> torch.Tensor:
        self._refuse_hidden("hidden_positions")

    def compact(self) -> torch.Tensor:
        self._refuse_hidden("compact")

    def set_item_tags(self, tags: torch.Tensor, positions: Optional[torch.Tensor] = None) -> None:
        raise NotImplementedError(f"{type(self).__name__}.set_item_tags: {_TAGS_WHY}")

    @property
    def item_tags(self):
        raise NotImplementedError(f"{type(self).__name__}.item_tags: {_TAGS_WHY}")

    def exchange_info(self) -> dict:
        """What carried the exchange: backend of the process group and its size (bench.py reports it)."""
        if not dist.is_initialized():
            return {"backend": None, "ranks": 1}
        return {"backend": dist.get_backend(self._group), "ranks": dist.get_world_size(self._group)}


class ShardedMoLBruteForceTopK(ShardedTopK):
    """Exact: identical to MoLBruteForceTopK over the whole corpus, bit for bit (see the module docstring).

    GLOBAL PROOF (round 5).  The single-device module's default exact path -- split-f16 first pass, fp32 re-scoring of the candidates, proof
    with the a-priori bound eps on |first pass - fp32| (topk_modules.MoLBruteForceTopK, f16x3_bound.py) -- proved PER SHARD would need
    every shard to cover what lies within eps of ITS OWN k-th score, which sits in a denser part of the score distribution than the whole
    corpus' (8 shards of amzn-books: thousands of candidates per shard and query instead of ~85).  So the proof is made once, globally:
      rank r:  first pass over its shard -> its kc_r best by first-pass score, m_r = the best first-pass score it leaves outside
               -> fp32 re-scoring of the kc_r -> its best k by (fp32 score, position)
      all:     ONE all-gather of (B, 2k + 2) messages -- the rank's top-k, m_r per row and the largest |fp32 - first pass| it saw ride in the
               same message (round 6; rounds 5 used an all-reduce next to the gather and an always-enqueued second gather for the redo)
               -> merge to the global top-k by fp32 score + verdict per row, e_k - max_r m_r > eps, in ONE launch
    Every item of every shard outside the candidates has a first-pass score <= max_r m_r, hence an fp32 score < e_k: the merged top-k IS the
    dense one.  Candidates per rank: the ~kc items within eps of the global k-th score spread evenly over the shards, so kc_r = kc / R +
    4 sqrt(kc / R) + 32 (doubled after a failed verdict, halved again after PAD_DECAY_CALLS proved calls: both decided from the verdicts,
    which every rank sees alike).  A failed verdict (crowded scores, a skewed shard, a violated guard) is the same on every rank -- its
    inputs are the gathered bytes -- and is read by the host from the pinned mirror the merge kernel writes; only then do the ranks run
    the dense fp32 kernels over their shards and a second exchange.  Used when EVERY rank's local module is bound in proved mode (an
    all-reduce at the first call); otherwise the per-shard path above."""

    GLOBAL_PROOF = True
    PAD_DECAY_CALLS = 64          # after this many consecutive proved calls a doubled candidate margin is halved again
    VERDICT_TIMEOUT_S = 120.0

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._gp_collectives = 0      # all-gathers of the global proof issued so far (exchange_info)
        self._gp_reset(None, None)

    def _gp_reset(self, eng, device) -> None:
        """The whole state of the global proof, for one binding of the local module (eng None: not decided yet, no device buffers)."""
        self._gp_engine = eng
        self._gp_on = False
        self._gp_eps: Optional[float] = None
        self._gp_guard_limit: Optional[float] = None
        self._gp_state = self._gp_host = self._gp_host_f = self._gp_host_i = self._gp_call = None
        if eng is not None:
            self._gp_state = torch.zeros(8, dtype=torch.float32, device=device)
            self._gp_host = torch.zeros(8, dtype=torch.float32).pin_memory()
            self._gp_host_f = self._gp_host.numpy()                         # views of the same pinned words: a poll is a plain memory read,
            self._gp_host_i = self._gp_host.view(torch.int32).numpy()       # not a tensor index + conversion (2-3 us each, between the batches)
            self._gp_call = torch.zeros(8 + 4 * 256, dtype=torch.int32, device=device)      # arrival counter + one 16-byte word per row
        self._gp_issued = 0           # verdicts enqueued so far (the host mirror's call counter reaches it when the last one has landed)
        self._gp_pad = 1
        self._gp_streak = 0
        self._gp_stats = {"calls": 0, "fallbacks": 0, "proved_calls": 0, "bound_violations": 0}

    def _after_local_update(self) -> None:
        # the global proof's guard limit comes from max |gi| over every shard: decided again, collectively, at the next call (every rank alike)
        self._gp_reset(None, None)

    def _make_local_module(self, mol_module, item_embeddings_shard, item_ids_shard) -> TopKModule:
        # the size-dependent choices of the proved flow (one eps or per-pair bounds, candidate margins) are made for the SHARD size every rank
        # computes alike -- the last shard may be shorter, and ranks must agree on the form of the bound
        return MoLBruteForceTopK(mol_module, item_embeddings_shard, item_ids_shard, bound_kind_items=-(-self._n_total // max(self._world, 1)))

    # ---- collectives on small tensors (host-staged only on a gloo group: test setups) --------------------------------------------
    def _all_reduce(self, t: torch.Tensor, op) -> torch.Tensor:
        if t.is_cuda and dist.get_backend(self._group) == "gloo":
            h = t.cpu()
            dist.all_reduce(h, op=op, group=self._group)
            return h.to(t.device)
        dist.all_reduce(t, op=op, group=self._group)
        return t

    def _global_proof(self, query_embeddings: torch.Tensor) -> bool:
        """Decided collectively, once per binding of the local module (all ranks reach this at the same call)."""
        local = self._local_module
        if not (self.GLOBAL_PROOF and self._exchange and dist.is_initialized() and isinstance(local, MoLBruteForceTopK) and self._local_topk_is_module
                and self._merge is _hip_merge and query_embeddings.is_cuda):
            return False
        eng = local._bind()
        if self._gp_engine is not eng:
            from . import f16x3_bound as FB

            mine = local.shard_can_speculate()
            flags = torch.tensor([1.0 if mine else 0.0, -(local._gi_abs_max() if mine else 0.0)], dtype=torch.float32, device=query_embeddings.device)
            flags = self._all_reduce(flags, dist.ReduceOp.MIN)          # min of the flags, max of max |gi| (negated)
            self._gp_reset(eng, query_embeddings.device)
            self._gp_on = bool(flags[0].item() > 0.5)
            gi_max = -float(flags[1].item())
            self._gp_guard_limit = min(FB.GATE_GUARD / gi_max, 3.0e38) if gi_max > 0.0 else 3.0e38
            self._gp_eps = local._proved_eps() if self._gp_on else None
        return self._gp_on

    def stats(self) -> dict:
        """Counters of the global proof (calls, proved_calls, fallbacks, bound_violations, kc per rank) merged over the local module's."""
        local = self._local_module
        out = local.stats()
        if self._gp_on:
            out.update(self._gp_stats)
            out["global_proof"] = True
        return out

    def _kc_local(self, k: int) -> int:
        return self._local_module.shard_candidate_count(k, self._gp_pad, self._world)

    def submit(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs):
        refuse_item_mask(self, kwargs, _MASK_WHY)
        refuse_allowed_tags(self, kwargs, _TAGS_WHY)
        refuse_collapse_groups(self, kwargs)
        refuse_diversity(self, kwargs)
        B = query_embeddings.size(0)
        per_shard = -(-self._n_total // max(self._world, 1))
        # (the 4 GiB logit policy: the first pass wants the whole (B, N_shard) matrix -- beyond it every rank alike takes the per-shard path, which chunks)
        if (not self._global_proof(query_embeddings) or not MoLBruteForceTopK.speculation_pays(B, per_shard)
                or B * per_shard * 4 > MoLBruteForceTopK.MAX_LOGIT_BYTES):
            return super().submit(query_embeddings, k, sorted, **kwargs)
        if k > self._n_total:
            raise RuntimeError(f"selected index k out of range (k={k}, n={self._n_total})")
        local = self._local_module
        with local.one_bind():
            kc = self._kc_local(k)
            msg, qpack32 = local.speculate_for_shard(query_embeddings, k, kc, **kwargs)
        ready = None
        if not self._plain_call:      # (a plain call's exchange follows on this very stream; result() of an explicit submit may be called on another)
            ready = torch.cuda.Event()
            ready.record()
        self._gp_stats["kc"] = kc
        return ("gproof", msg, ready, k, qpack32, query_embeddings, kwargs, sorted)

    def result(self, handle, seen=None) -> Tuple[torch.Tensor, torch.Tensor]:
        if handle[0] != "gproof":
            return super().result(handle, seen)
        _, msg, ready, k, qpack32, query_embeddings, kwargs, sorted_ = handle
        local = self._local_module
        sp = local._engine.spec
        B = query_embeddings.size(0)
        gq = local._engine.gate_rows(qpack32, B)
        self._join_submit(msg.device, ready)
        fuse = seen is not None and E.merge_filter_fusable(k, seen[0].shape[1], seen[1])
        if self._gp_call.numel() < 8 + 4 * B:
            self._gp_call = torch.zeros(8 + 4 * B, dtype=torch.int32, device=msg.device)
        # ONE exchange: the (B, 2k + 2) messages carry every rank's top-k, the best first-pass score it left outside its candidates and the
        # largest |fp32 - first pass| it saw; merge, verdict and the seen-id filter are one launch behind it
        gathered = self._all_gather_rows(msg)
        self._gp_collectives += 1
        out = E.merge_candidates_verdict(gathered, self._world, k, k, self._gp_eps, 1.0, gq, sp.num_logits, self._gp_guard_limit, self._gp_state,
                                         self._gp_host, self._gp_call, seen if fuse else None)
        if seen is not None and not fuse:
            out = E.filter_seen_ids(out[1], out[0], seen[0], seen[1])
        self._gp_issued += 1
        # Every rank computes the verdict from the same gathered bytes, so all of them raise or clear REDO alike; the host reads it from the pinned
        # mirror the merge kernel writes (with submit / result pipelining batch i + 1 is already enqueued: the device does not idle) and only a
        # failed verdict -- crowded scores, a skewed shard, a violated guard -- costs more: the dense fp32 kernels over the shards and their
        # own exchange, issued here, by every rank.
        redo = self._gp_wait_verdict()
        st = self._gp_stats
        st["calls"] += 1
        if float(self._gp_host_f[0]) > self._gp_eps:
            st["bound_violations"] += 1
        elif not redo:
            st["proved_calls"] += 1
        st["guard_max"] = float(self._gp_host_f[7])
        if not redo:
            self._gp_streak += 1
            if self._gp_pad > 1 and self._gp_streak >= self.PAD_DECAY_CALLS:
                self._gp_pad //= 2
                self._gp_streak = 0
            if seen is not None:
                return out[0], out[1].to(query_embeddings.dtype)
            return out[0].to(query_embeddings.dtype), out[1]
        st["fallbacks"] += 1
        self._gp_streak = 0
        if self._gp_pad < 64:
            self._gp_pad *= 2
        # the dense fp32 kernels over this shard (the local module's resident fp32 index) and the plain exchange of the per-shard top-k
        k_local = min(k, self._n_local)
        if k_local > 0:
            with local.one_bind():
                s, ids = local._forward_fp32_dense(query_embeddings, k_local, **kwargs)
        else:
            s = torch.empty((B, 0), dtype=torch.float32, device=msg.device)
            ids = torch.empty((B, 0), dtype=torch.int64, device=msg.device)
        msg2 = E.pack_candidates(s.float(), ids, k)
        ready2 = torch.cuda.Event()
        ready2.record()
        return super().result(("pending", msg2, ready2, k, True, query_embeddings.dtype, None), seen)

    def _gp_wait_verdict(self) -> bool:
        """Spin on the pinned mirror's call counter until the verdict enqueued last has landed -> its REDO flag."""
        import time

        h = self._gp_host_f
        want = float(self._gp_issued)
        t0 = None
        n = 0
        while h[5] < want:
            n += 1
            if (n & 1023) == 0:
                if t0 is None:
                    t0 = time.perf_counter()
                elif time.perf_counter() - t0 > self.VERDICT_TIMEOUT_S:
                    raise RuntimeError("the item-sharded verdict did not arrive (a kernel or the exchange failed)")
        return int(self._gp_host_i[1]) != 0

    def exchange_info(self) -> dict:
        info = super().exchange_info()
        info["collectives_per_proved_step"] = 1
        info["collectives_issued"] = self._gp_collectives
        return info

    def forward_filtered(self, query_embeddings: torch.Tensor, k_prime: int, invalid_ids: torch.Tensor, k: int, **kwargs):
        refuse_item_mask(self, kwargs, _MASK_WHY)
        refuse_allowed_tags(self, kwargs, _TAGS_WHY)
        refuse_collapse_groups(self, kwargs)
        refuse_diversity(self, kwargs)
        if self._exchange and self._global_proof(query_embeddings) and MoLBruteForceTopK.speculation_pays(query_embeddings.size(0), -(-self._n_total // self._world)) and k_prime <= self._n_total:
            with self._inline():
                return self.result(self.submit(query_embeddings, k_prime, **kwargs), seen=(invalid_ids, k))
        return super().forward_filtered(query_embeddings, k_prime, invalid_ids, k, **kwargs)


class ShardedMoLAvgTopK(ShardedTopK):
    """Two-pass approximate top-k on an item-sharded corpus (BASELINE config 5): MoLAvgTopK(avg_top_k) per shard, then
    the same single all-gather + merge.  `avg_top_k` is PER SHARD; k <= avg_top_k as in the reference
    (rails/indexing/mol_top_k.py:383-386)."""

    def __init__(self, mol_module, item_embeddings_shard, item_ids_shard, n_items_total: int, avg_top_k: int,
                 global_k_prime: bool = False, shard_offset: Optional[int] = None,
                 coarse_local: Optional[Callable[..., Tuple[torch.Tensor, torch.Tensor]]] = None,
                 rerank_local: Optional[Callable[..., Tuple[torch.Tensor, torch.Tensor]]] = None, **kwargs) -> None:
        """global_k_prime: exchange coarse candidates first so that exactly the global coarse top-K' is reranked (see the module
        docstring); `shard_offset` = global position of this shard's first item (default: the contiguous split of shard_bounds).
        `coarse_local(q, **kw) -> (scores, local positions)` / `rerank_local(q, local positions with -1 holes, k, **kw) ->
        (scores, ids)` default to the HIP module's methods; the CPU test of the collective logic injects oracle callables."""
        self._avg_top_k = avg_top_k
        self._global = global_k_prime
        if coarse_local is not None and "local_topk" not in kwargs:
            kwargs["local_topk"] = lambda q, k, **kw: (_ for _ in ()).throw(RuntimeError("global_k_prime path only"))   # noqa: E731
        super().__init__(mol_module, item_embeddings_shard, item_ids_shard, n_items_total, **kwargs)
        rank = dist.get_rank(self._group) if dist.is_initialized() else 0
        self._offset = shard_offset if shard_offset is not None else shard_bounds(n_items_total, self._world, rank)[0]
        if self._global and self._exchange and shard_offset is not None:
            # ties are broken by the slot in the rank-major concatenation: that is the global position order only when the shards
            # are disjoint position ranges in rank order
            spans = [None] * self._world
            dist.all_gather_object(spans, (int(self._offset), int(self._offset + self._n_local)), group=self._group)
            if any(spans[r][1] > spans[r + 1][0] for r in range(self._world - 1)):
                raise ValueError(f"global_k_prime needs shard ranges that ascend with the rank without overlap, got {spans}")
        self._coarse_local = coarse_local if coarse_local is not None else (lambda q, **kw: self._local_module.coarse_candidates(q, **kw))
        self._rerank_local = rerank_local if rerank_local is not None else (lambda q, idx, k, **kw: self._local_module.rerank_masked(q, idx, k, **kw))

    def _make_local_module(self, mol_module, item_embeddings_shard, item_ids_shard) -> TopKModule:
        refuse_generic_candidates(mol_module, "ShardedMoLAvgTopK", _GENERIC_WHY)
        return MoLAvgTopK(mol_module, item_embeddings_shard, item_ids_shard, avg_top_k=min(self._avg_top_k, int(item_ids_shard.numel())))

    def forward_filtered(self, query_embeddings: torch.Tensor, k_prime: int, invalid_ids: torch.Tensor, k: int, **kwargs):
        refuse_item_mask(self, kwargs, _MASK_WHY)
        refuse_allowed_tags(self, kwargs, _TAGS_WHY)
        refuse_collapse_groups(self, kwargs)
        refuse_diversity(self, kwargs)
        if k_prime > self._avg_top_k or (self._global and self._exchange):
            return None   # forward's own checks / the global-K' exchange: the caller composes forward + filter_seen_ids
        return super().forward_filtered(query_embeddings, k_prime, invalid_ids, k, **kwargs)

    def forward(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        refuse_item_mask(self, kwargs, _MASK_WHY)
        refuse_allowed_tags(self, kwargs, _TAGS_WHY)
        refuse_collapse_groups(self, kwargs)
        refuse_diversity(self, kwargs)
        if k > self._avg_top_k:
            raise ValueError(f"avg_top_k ({self._avg_top_k}) must be larger than k ({k})")
        if not self._global or not self._exchange:
            return super().forward(query_embeddings, k, sorted, **kwargs)
        K = self._avg_top_k
        if K > self._n_total:
            raise RuntimeError(f"selected index k out of range (k={K}, n={self._n_total})")
        B = query_embeddings.size(0)
        dev = query_embeddings.device
        # (1) local coarse top-K' -> message (coarse score bits | GLOBAL position), K' slots, short shards padded with (-inf, -1)
        if self._n_local > 0:
            cs, cpos = self._coarse_local(query_embeddings, **kwargs)
            cpos = cpos + self._offset
        else:
            cs = torch.empty((B, 0), dtype=torch.float32, device=dev)
            cpos = torch.empty((B, 0), dtype=torch.int64, device=dev)
        on_gpu = cs.is_cuda and self._merge is _hip_merge
        msg = E.pack_candidates(cs, cpos, K) if on_gpu else pack_candidates(cs.float(), cpos, K)
        gathered = self._all_gather_rows(msg)
        # (2) the global coarse top-K' (same total order on every rank: score desc, global position asc)
        if on_gpu and self._world * K <= 16384:   # one kernel (its lists are sorted in LDS)
            _, gpos = E.merge_candidates(gathered, self._world, K, K)
        elif on_gpu:                              # long lists: the general top-k over the shard-major concatenation (same tie rule)
            all_s, all_p = unpack_candidates(gathered.view(self._world, B, 2 * K), K)
            _, gpos = E.topk(all_s, K, ids=all_p)
        else:
            all_s, all_p = unpack_candidates(gathered.view(self._world, B, 2 * K), K)
            _, gpos = self._merge(all_s, all_p, K)
        # (3) rerank my members of it (others become holes), local top-k, and the usual exchange of exact MoL scores
        mine = (gpos >= self._offset) & (gpos < self._offset + self._n_local)
        local_idx = torch.where(mine, gpos - self._offset, gpos.new_full((), -1))
        if self._n_local > 0:
            s, ids = self._rerank_local(query_embeddings, local_idx, k, **kwargs)
        else:
            s = torch.full((B, k), float("-inf"), dtype=torch.float32, device=dev)
            ids = torch.full((B, k), -1, dtype=torch.int64, device=dev)
        msg2 = E.pack_candidates(s, ids, k) if on_gpu else pack_candidates(s.float(), ids, k)
        gathered2 = self._all_gather_rows(msg2)
        if on_gpu:
            ms, mi = E.merge_candidates(gathered2, self._world, k, k)
        else:
            all_s, all_i = unpack_candidates(gathered2.view(self._world, B, 2 * k), k)
            ms, mi = self._merge(all_s, all_i, k)
        return ms.to(query_embeddings.dtype), mi


# ---- per-component candidates on an item-sharded corpus ---------------------------------------------------------------------------------
# The component scores and the coarse scores are bf16 values, so one 64-bit key carries a candidate (include/rails_amd.h rails_group_keys_*):
#   bits 63..48  order-preserving image of the bf16 score (h | 0x8000 for a clear sign bit, ~h for a set one: rails_topk's order cut to 16 bits --
#                +0 above -0, NaNs with a clear sign bit above +inf, with a set one below -inf)
#   bits 47..0   2^48 - 1 - global position
# A larger UNSIGNED key is better; equal scores order by ascending position; key 0 pads.  The tensors below hold the keys' bit patterns in int64.
GROUP_KEY_POSITION_BITS = 48
_POS_MASK = (1 << GROUP_KEY_POSITION_BITS) - 1
_SIGN64 = -(1 << 63)


def pack_group_keys(scores: torch.Tensor, positions: torch.Tensor, offset: int, k_slots: int, n_local: Optional[int] = None) -> torch.Tensor:
    """The torch restatement of rails_group_keys_pack: (rows, k_local) bf16-valued fp32 scores + int64 local positions -> (rows, k_slots)
    int64 key bit patterns, padded with key 0 (negative positions pad too).  Global positions of 2^48 or more raise ValueError."""
    rows, kl = scores.shape
    if k_slots < kl:
        raise ValueError(f"pack_group_keys: k_slots ({k_slots}) < k_local ({kl})")
    bound = int(n_local) if n_local is not None else (int(positions.max()) + 1 if positions.numel() else 0)
    if offset < 0 or offset + bound > (1 << GROUP_KEY_POSITION_BITS):
        raise ValueError(f"pack_group_keys: global positions [{offset}, {offset + bound}) do not fit {GROUP_KEY_POSITION_BITS} bits")
    h = (scores.float().contiguous().view(torch.int32).to(torch.int64) >> 16) & 0xFFFF
    img = torch.where((h & 0x8000) != 0, ~h & 0xFFFF, h | 0x8000)
    img = torch.where(img >= 0x8000, img - 0x10000, img)          # the upper 16 bits of a two's-complement word
    keys = img * (1 << GROUP_KEY_POSITION_BITS) + (_POS_MASK - (positions.to(torch.int64) + offset))
    keys = torch.where(positions < 0, torch.zeros_like(keys), keys)
    if kl < k_slots:
        keys = torch.cat([keys, keys.new_zeros((rows, k_slots - kl))], 1)
    return keys


def unpack_group_keys(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """keys (any shape, int64 bit patterns) -> (scores fp32, global positions).  A pad decodes to position -1 and to the score its bits
    spell: the all-ones NaN, which rails_topk ranks below everything, -inf included."""
    img = (keys >> GROUP_KEY_POSITION_BITS) & 0xFFFF
    h = torch.where((img & 0x8000) != 0, img & 0x7FFF, ~img & 0xFFFF)
    scores = ((h << 16) - ((h >> 15) << 32)).to(torch.int32).view(torch.float32)      # (the fp32 word as a two's-complement int32)
    pos = _POS_MASK - (keys & _POS_MASK)
    return scores, torch.where(keys == 0, torch.full_like(pos, -1), pos)


def merge_group_keys_own(keys: torch.Tensor, lo: int, hi: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The torch restatement of rails_group_keys_merge_own: keys (R, rows, k) -> (global positions (rows, k), local positions (rows, k)):
    the k largest unsigned keys of every row, best first; position - lo inside [lo, hi), -1 elsewhere and for pads."""
    R, rows, k = keys.shape
    flat = keys.permute(1, 0, 2).reshape(rows, R * k)
    order = torch.sort(flat ^ _SIGN64, dim=1, descending=True, stable=True).values[:, :k] ^ _SIGN64     # unsigned order through the sign flip
    _, gpos = unpack_group_keys(order)
    return gpos, torch.where((gpos >= lo) & (gpos < hi), gpos - lo, torch.full_like(gpos, -1))


class _ShardedComponentCandidates(ShardedTopK):
    """What ShardedMoLNaiveTopK and ShardedMoLCombTopK share.  forward(q, k) -> (scores, ids) with min(k, W) columns, identical on every rank,
    W = P_Q * P_X * k_per_group [+ avg_top_k] being the union width the single-device module returns.

    Per-shard form (default): every rank runs the single-device module on its shard -- k_per_group (and avg_top_k) candidates PER SHARD --
    keeps the first k columns of its ranking and the usual single all-gather + merge follows: weak scaling, a superset-quality variant that
    equals the single-device module at one rank.
    Global form (global_candidates=True): the single-device algorithm on the sharded corpus.  (1) local candidates with scores, verified (a
    rank whose fused-scan verdict fails redoes ITS scan before it sends: the collectives do not depend on verdicts); (2) ONE all-gather of the
    candidate keys -- Comb's group keys and coarse keys in one message, 8 bytes per candidate; (3) every rank selects the global top-k_per_group
    of every (query group, item group) row (and the global coarse top-K') under (score desc, global position asc) and writes its own members of
    the union as local positions, holes elsewhere (rails_group_keys_merge_own; beyond 16 384 keys per row: unpack + the general top-k);
    (4) rerank of those with full MoL, duplicates masked as on one device; (5) the usual all-gather + merge of the local top-k.  Two collectives
    per step.  The scores equal the first columns of the single-device ranking bit for bit, the ids wherever the score is above the duplicate
    mark -32767.0.  THE MASKED TAIL (columns at -32767.0: second and later copies of a candidate several lists named) carries the ids of those
    copies in ascending global position, rank by rank; it holds the same multiset of ids as the single-device tail, and the same order whenever
    the shards are the contiguous split.

    Out of scope: use_faiss=True (IVF lists are trained per shard: NotImplementedError); submit / result pipelining of the global form (its
    forward is one synchronous chain; the per-shard form has ShardedTopK's); the generic scoring route (refused by the local modules)."""

    def __init__(self, mol_module, item_embeddings_shard, item_ids_shard, n_items_total: int, *, global_candidates: bool, shard_offset: Optional[int],
                 candidates_local, rerank_local, **kwargs) -> None:
        self._global = bool(global_candidates)
        if candidates_local is not None and "local_topk" not in kwargs:
            kwargs["local_topk"] = lambda q, k, **kw: (_ for _ in ()).throw(RuntimeError("global_candidates path only"))   # noqa: E731
        super().__init__(mol_module, item_embeddings_shard, item_ids_shard, n_items_total, **kwargs)
        rank = dist.get_rank(self._group) if dist.is_initialized() else 0
        self._offset = int(shard_offset) if shard_offset is not None else shard_bounds(n_items_total, self._world, rank)[0]
        if self._global and self._exchange and shard_offset is not None:
            # equal scores are ordered by global position, and the final merge breaks ties by rank: one order only for ascending disjoint ranges
            spans = [None] * self._world
            dist.all_gather_object(spans, (self._offset, self._offset + self._n_local), group=self._group)
            if any(spans[r][1] > spans[r + 1][0] for r in range(self._world - 1)):
                raise ValueError(f"global_candidates needs shard ranges that ascend with the rank without overlap, got {spans}")
        if self._local_topk_is_module:        # the module ranks its whole union whatever k is: a shard's top-k are its first columns
            self._local_topk = lambda q, k, **kw: tuple(t[:, :k] for t in self._local_module(q, k=k, **kw))  # noqa: E731
            self._local_topk_is_module = False    # (MoLCombTopK inherits MoLAvgTopK's submit / result, which are not its forward: plain calls only)
        self._candidates_local = candidates_local if candidates_local is not None else (lambda q, **kw: self._local_module.local_candidates(q, **kw))
        self._rerank_local = rerank_local if rerank_local is not None else (lambda q, idx, k, **kw: self._local_module.rerank_union_masked(q, idx, k, **kw))
        self._msg_keys = 0

    # (rows per query of the group lists, k_per_group, K' or 0)
    def _widths(self) -> Tuple[int, int, int]:
        raise NotImplementedError

    def union_width(self) -> int:
        g, kg, kc = self._widths()
        return g * kg + kc

    def _check_k(self, k: int) -> int:
        if k > self._n_total:
            raise RuntimeError(f"selected index k out of range (k={k}, n={self._n_total})")
        return min(k, self.union_width())

    def forward(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        refuse_item_mask(self, kwargs, _MASK_WHY)
        refuse_allowed_tags(self, kwargs, _TAGS_WHY)
        refuse_collapse_groups(self, kwargs)
        refuse_diversity(self, kwargs)
        kk = self._check_k(k)
        if not (self._global and self._exchange):
            if not self._exchange:       # one rank: the module's own ranking
                s, ids = self._local_topk(query_embeddings, kk, **kwargs)
                return s, ids
            return super().forward(query_embeddings, kk, sorted, **kwargs)
        return self._forward_global(query_embeddings, kk, **kwargs)

    def submit(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs):
        refuse_item_mask(self, kwargs, _MASK_WHY)
        refuse_allowed_tags(self, kwargs, _TAGS_WHY)
        refuse_collapse_groups(self, kwargs)
        refuse_diversity(self, kwargs)
        if self._global and self._exchange:
            raise NotImplementedError(f"{type(self).__name__}: submit / result pipelining of the global form is not built; call forward")
        return super().submit(query_embeddings, k, sorted, **kwargs)

    def forward_filtered(self, query_embeddings: torch.Tensor, k_prime: int, invalid_ids: torch.Tensor, k: int, **kwargs):
        refuse_item_mask(self, kwargs, _MASK_WHY)
        refuse_allowed_tags(self, kwargs, _TAGS_WHY)
        refuse_collapse_groups(self, kwargs)
        refuse_diversity(self, kwargs)
        if self._global and self._exchange:
            return None      # the caller composes forward + filter_seen_ids: same bits
        if not self._exchange or k_prime > self.union_width() or k_prime > self._n_total:
            return None
        return super().forward_filtered(query_embeddings, k_prime, invalid_ids, k, **kwargs)

    def _forward_global(self, query_embeddings: torch.Tensor, kk: int, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        g, kg, kc = self._widths()
        B = query_embeddings.size(0)
        dev = query_embeddings.device
        rows = B * g
        W = g * kg + kc
        if kg > self._n_total or kc > self._n_total:
            raise RuntimeError(f"selected index k out of range (k={max(kg, kc)}, n={self._n_total})")
        R, lo, hi = self._world, self._offset, self._offset + self._n_local
        # (1) this shard's candidates with their scores, verified
        if self._n_local > 0:
            cand = self._candidates_local(query_embeddings, **kwargs)
        else:
            ef, ei = torch.empty((rows, 0), dtype=torch.float32, device=dev), torch.empty((rows, 0), dtype=torch.int64, device=dev)
            cand = (ef, ei, ef[:B], ei[:B]) if kc else (ef, ei)
        on_gpu = cand[0].is_cuda and self._merge is _hip_merge
        # (2) ONE message per rank: [rows * k_g group keys | B * K' coarse keys], all-gathered in rank order
        n_keys = rows * kg + B * kc
        self._msg_keys = n_keys
        if on_gpu:
            msg = torch.empty(n_keys, dtype=torch.int64, device=dev)
            E.group_keys_pack(cand[0], cand[1], lo, self._n_local, kg, out=msg[: rows * kg])
            if kc:
                E.group_keys_pack(cand[2], cand[3], lo, self._n_local, kc, out=msg[rows * kg :])
        else:
            parts = [pack_group_keys(cand[0].float(), cand[1], lo, kg, self._n_local).reshape(-1)]
            if kc:
                parts.append(pack_group_keys(cand[2].float(), cand[3], lo, kc, self._n_local).reshape(-1))
            msg = torch.cat(parts)
        gathered = self._all_gather_rows(msg.view(1, n_keys))            # (R, n_keys)
        # (3) the global lists, as this rank's local positions in one (B, W) union buffer
        union = torch.empty((B, W), dtype=torch.int64, device=gathered.device)
        for first, n_rows, kx, col, per_row in ((0, rows, kg, 0, g), (rows * kg, B, kc, g * kg, 1)):
            if kx == 0:
                continue
            block = gathered[:, first : first + n_rows * kx]
            if on_gpu and E.group_keys_supported(R, kx):       # one launch
                E.group_keys_merge_own(gathered.view(-1)[first:], R, n_rows, kx, lo, hi, out_local=union, out_col=col, rows_per_out_row=per_row,
                                       rank_stride=n_keys)
                continue
            if on_gpu:       # long lists: unpack + the general top-k over the rank-major concatenation (same total order)
                sc, gp = unpack_group_keys(block.reshape(R, n_rows, kx).permute(1, 0, 2).reshape(n_rows, R * kx))
                _, gpos = E.topk(sc, kx, ids=gp)
                local = torch.where((gpos >= lo) & (gpos < hi), gpos - lo, gpos.new_full((), -1))
            else:
                _, local = merge_group_keys_own(block.reshape(R, n_rows, kx), lo, hi)
            union[:, col : col + per_row * kx] = local.view(B, per_row * kx)
        # (4) full MoL on my members of the union, (5) the usual exchange of exact scores
        if self._n_local > 0:
            s, ids = self._rerank_local(query_embeddings, union, kk, **kwargs)
        else:
            s = torch.full((B, kk), float("-inf"), dtype=torch.float32, device=dev)
            ids = torch.full((B, kk), -1, dtype=torch.int64, device=dev)
        msg2 = E.pack_candidates(s, ids, kk) if on_gpu else pack_candidates(s.float(), ids, kk)
        with self._inline():
            return self.result(("pending", msg2, None, kk, on_gpu, query_embeddings.dtype, None))

    def exchange_info(self) -> dict:
        info = super().exchange_info()
        glob = self._global and self._exchange
        info["form"] = "global" if self._global else "per-shard"
        info["collectives_per_step"] = 2 if glob else (1 if self._exchange else 0)
        # the global form's first exchange: 8 bytes per candidate slot, (B * P_Q * P_X * k_g [+ B * K']) slots as of the last call
        info["candidate_message_bytes"] = 8 * self._msg_keys if glob else 0
        return info


class ShardedMoLNaiveTopK(_ShardedComponentCandidates):
    """MoLNaiveTopK on an item-sharded corpus; the two forms, the return value and what is out of scope: _ShardedComponentCandidates.
    `candidates_local(q, **kw) -> (group scores, group local positions)`, both (B * P_Q * P_X, <= k_per_group), and
    `rerank_local(q, local positions with -1 holes (B, W), k, **kw) -> (scores, ids)` default to the HIP module's local_candidates /
    rerank_union_masked; the CPU test of the collective logic injects oracle callables (then `groups` = P_Q * P_X must be given)."""

    def __init__(self, mol_module, item_embeddings_shard, item_ids_shard, n_items_total: int, k_per_group: int, global_candidates: bool = False,
                 shard_offset: Optional[int] = None, use_faiss: bool = False, candidates_local=None, rerank_local=None, groups: Optional[int] = None,
                 **kwargs) -> None:
        if use_faiss:
            raise NotImplementedError("ShardedMoLNaiveTopK: use_faiss=True is not built for a sharded corpus (IVF lists are trained per shard)")
        self._k_per_group = int(k_per_group)
        self._groups = int(groups) if groups is not None else mol_module._query_dot_product_groups * mol_module._item_dot_product_groups
        super().__init__(mol_module, item_embeddings_shard, item_ids_shard, n_items_total, global_candidates=global_candidates, shard_offset=shard_offset,
                         candidates_local=candidates_local, rerank_local=rerank_local, **kwargs)

    def _make_local_module(self, mol_module, item_embeddings_shard, item_ids_shard) -> TopKModule:
        refuse_generic_candidates(mol_module, "ShardedMoLNaiveTopK", _GENERIC_WHY)
        return MoLNaiveTopK(mol_module, item_embeddings_shard, item_ids_shard, k_per_group=max(1, min(self._k_per_group, int(item_ids_shard.numel()))))

    def _widths(self) -> Tuple[int, int, int]:
        return self._groups, self._k_per_group, 0


class ShardedMoLCombTopK(_ShardedComponentCandidates):
    """MoLCombTopK on an item-sharded corpus: as ShardedMoLNaiveTopK, with the averaged-query coarse top-`avg_top_k` in the union
    (`candidates_local` -> (group scores, group positions, coarse scores (B, <= K'), coarse positions)); in the global form the group keys and the
    coarse keys travel in one message."""

    def __init__(self, mol_module, item_embeddings_shard, item_ids_shard, n_items_total: int, avg_top_k: int, k_per_group: int,
                 global_candidates: bool = False, shard_offset: Optional[int] = None, candidates_local=None, rerank_local=None,
                 groups: Optional[int] = None, **kwargs) -> None:
        self._k_per_group = int(k_per_group)
        self._avg_top_k = int(avg_top_k)
        self._groups = int(groups) if groups is not None else mol_module._query_dot_product_groups * mol_module._item_dot_product_groups
        super().__init__(mol_module, item_embeddings_shard, item_ids_shard, n_items_total, global_candidates=global_candidates, shard_offset=shard_offset,
                         candidates_local=candidates_local, rerank_local=rerank_local, **kwargs)

    def _make_local_module(self, mol_module, item_embeddings_shard, item_ids_shard) -> TopKModule:
        refuse_generic_candidates(mol_module, "ShardedMoLCombTopK", _GENERIC_WHY)
        n = int(item_ids_shard.numel())
        return MoLCombTopK(mol_module, item_embeddings_shard, item_ids_shard, avg_top_k=max(1, min(self._avg_top_k, n)),
                           k_per_group=max(1, min(self._k_per_group, n)))

    def _widths(self) -> Tuple[int, int, int]:
        return self._groups, self._k_per_group, self._avg_top_k
