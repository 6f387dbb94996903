"""Host-side mirror of the reference's top-k modules and candidate index.

  TopKModule            reference rails/indexing/candidate_index.py:24-42
  MoLBruteForceTopK     reference rails/indexing/mol_top_k.py:84-130   (exact)
  MoLAvgTopK            reference rails/indexing/mol_top_k.py:296-429  (two-pass approximate)
  CandidateIndex        reference indexing/candidate_index.py:30-185
  get_top_k_module      reference indexing/utils_rails.py:25-233

Unlike the reference, which keeps the raw (1, N, D) table and re-projects every item on every call
(mol_top_k.py:118-122), the modules here build the tile-packed item index once at construction
(rebuilt automatically if the MoL module's parameters change) and per call run: query prologue ->
fused scoring -> exact top-k -> id gather, all HIP.
"""
from __future__ import annotations

import abc
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import math

import contextlib

import torch

from . import engine as E
from .mol_module import MoLSimilarity


class TopKModule(torch.nn.Module):
    def __setattr__(self, name, value):
        """Plain Python state (counters, flags, cached engines, handles: a dozen assignments per call) goes straight to the instance dict:
        torch.nn.Module.__setattr__ walks its parameter / buffer / module registries for every assignment (1-2.5 us each -- host time that sits
        between the batches wherever a call ends with the host's look at a verdict).  Tensors, modules and names already registered keep the
        nn.Module path."""
        if not isinstance(value, (torch.Tensor, torch.nn.Module)):
            d = self.__dict__
            if name not in d.get("_parameters", ()) and name not in d.get("_buffers", ()) and name not in d.get("_modules", ()):
                d[name] = value
                return
        super().__setattr__(name, value)

    @abc.abstractmethod
    def forward(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (top_k_scores (B, k), top_k_ids (B, k))."""


def _rows_arg(item_embeddings: torch.Tensor, item_ids: Optional[torch.Tensor], dim: int, dtype: torch.dtype, device: torch.device, ids_dtype: torch.dtype, appending: bool = False):
    """The rows (and ids) argument of update_items / append_items against a table of `dim` columns, `dtype`, on `device` -> ((M, dim) rows, (M,) ids
    or None); ValueError for anything else."""
    if appending and item_ids is None:
        raise ValueError("append_items needs the ids of the new items")
    emb = item_embeddings
    if not torch.is_tensor(emb):
        raise ValueError("item_embeddings must be a tensor")
    if emb.dim() == 3 and emb.shape[0] == 1:
        emb = emb[0]
    if emb.dim() != 2 or emb.shape[1] != dim:
        raise ValueError(f"item_embeddings must be (M, {dim}) or (1, M, {dim}), got {tuple(item_embeddings.shape)}")
    if device.type == "cuda":
        E._require_device(emb, "item_embeddings")
    if emb.device != device or emb.dtype != dtype:
        raise ValueError(f"item_embeddings must be {dtype} on {device}, got {emb.dtype} on {emb.device}")
    ids = None
    if item_ids is not None:
        if (not torch.is_tensor(item_ids) or item_ids.dtype != ids_dtype or item_ids.numel() != emb.shape[0]
                or not (item_ids.dim() == 1 or (item_ids.dim() == 2 and item_ids.shape[0] == 1))):
            raise ValueError(f"item_ids must be ({emb.shape[0]},) or (1, {emb.shape[0]}) {ids_dtype}")
        ids = item_ids.reshape(-1)
    return emb, ids


def _checked_positions(positions: torch.Tensor, m: int, n: int) -> torch.Tensor:
    if not torch.is_tensor(positions) or positions.dtype != torch.int64 or tuple(positions.shape) != (m,):
        raise ValueError(f"positions must be ({m},) int64")
    if m:
        host = positions.cpu()      # (the one sync of a device tensor)
        if int(host.min()) < 0 or int(host.max()) >= n:
            raise ValueError(f"positions must lie in [0, {n})")
        if torch.unique(host).numel() != m:
            raise ValueError("positions must be unique")
    return positions


def _removal_arg(positions: torch.Tensor, n: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """remove_items' positions against n items -> removal_plan's (holes, movers) and `moved`, CPU int64 rows [from, to]."""
    if not torch.is_tensor(positions) or positions.dtype != torch.int64 or positions.dim() != 1:
        raise ValueError("positions must be (M,) int64")
    holes, movers = removal_plan(positions.cpu(), n)      # (the one sync of a device tensor)
    return holes, movers, torch.stack([movers, holes], dim=1)


def _write_ids(item_ids: torch.Tensor, flat: torch.Tensor, pos: torch.Tensor, ids: torch.Tensor) -> None:
    """update_items: `ids` at positions `pos` (on flat's device) of the borrowed id tensor, (1, N) or (N,), and of `flat`, its int64 copy (or that very storage)."""
    own = item_ids[0] if item_ids.dim() == 2 else item_ids
    own.index_copy_(0, pos.to(own.device), ids.to(device=own.device, dtype=own.dtype))
    if flat.data_ptr() != own.data_ptr():
        flat.index_copy_(0, pos, ids.to(device=pos.device, dtype=torch.int64))


def _append_ids(item_ids: torch.Tensor, flat: torch.Tensor, ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """append_items: `ids` behind both -> new ((1, N + M) item_ids, flat)."""
    return (torch.cat([item_ids.reshape(1, -1), ids.reshape(1, -1).to(device=item_ids.device, dtype=item_ids.dtype)], dim=1),
            torch.cat([flat, ids.to(device=flat.device, dtype=torch.int64)]))


def _remove_ids(item_ids: torch.Tensor, flat: torch.Tensor, n_new: int, holes: torch.Tensor, movers: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """remove_items: both cut to n_new, the movers' ids in the holes (both on flat's device) -> new ((1, n_new) item_ids, flat)."""
    own = item_ids.reshape(1, -1)
    ids, new_flat = own[:, :n_new].clone(), flat[:n_new].clone()
    ids[0].index_copy_(0, holes.to(own.device), own[0].index_select(0, movers.to(own.device)))
    new_flat.index_copy_(0, holes, flat.index_select(0, movers))
    return ids, new_flat


def removal_plan(positions: torch.Tensor, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The one rule of remove_items: removing `positions` ((M,) int64 on the CPU, unique, inside [0, n)) from a table of n
    rows leaves N' = n - M rows -- rows 0 .. N' - 1 with the HOLES (the removed positions below N', ascending) filled from the MOVERS (the surviving
    positions at or above N', ascending), the i-th mover's row and id at the i-th hole; nothing else moves.  -> (holes, movers), CPU int64, of one
    length.  Pure host arithmetic in O(M log M): the tail N' .. n - 1 has M positions.  ValueError for a wrong dtype or shape, a position out of
    range, a duplicate, or N' < 1."""
    if not torch.is_tensor(positions) or positions.dtype != torch.int64 or positions.dim() != 1 or positions.is_cuda:
        raise ValueError("positions must be a 1-d int64 tensor on the CPU")
    m = positions.numel()
    _checked_positions(positions, m, n)
    n_new = n - m
    if n_new < 1:
        raise ValueError(f"removing {m} of {n} items would leave none")
    order = torch.sort(positions).values
    tail_kept = torch.ones(m, dtype=torch.bool)
    tail_kept[order[order >= n_new] - n_new] = False
    return order[order < n_new], n_new + torch.nonzero(tail_kept).reshape(-1)


def visibility_after_removal(words: torch.Tensor, n_new: int, holes: torch.Tensor, movers: torch.Tensor) -> torch.Tensor:
    """remove_items on a visibility row: visibility belongs to the position, so the i-th mover's bit -- read BEFORE the cut --
    goes to the i-th hole and the row is cut to the words of n_new items, the unused high bits of its last word zero.  words: (1, W) or (W,) int32
    ItemMask words; holes / movers: removal_plan's, int64 on the words' device.  -> (1, words of n_new) int32.  Pure tensor arithmetic, on
    whichever device the row lives (tested on the CPU against a numpy model): holes are unique, so the per-word sums below are ORs."""
    flat = words.reshape(-1)
    n_words = (int(n_new) + 31) // 32
    moved = (flat.index_select(0, movers >> 5).to(torch.int64) >> (movers & 31)) & 1
    w = flat[:n_words].to(torch.int64) & 0xFFFFFFFF
    hole_bit = torch.ones_like(holes) << (holes & 31)
    cleared = torch.zeros(n_words, dtype=torch.int64, device=flat.device).index_add_(0, holes >> 5, hole_bit)
    filled = torch.zeros(n_words, dtype=torch.int64, device=flat.device).index_add_(0, holes >> 5, hole_bit * moved)
    w = (w & ~cleared) | filled
    live = int(n_new) - 32 * (n_words - 1)
    w[-1] &= (1 << live) - 1
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32).reshape(1, -1)


def visibility_after_append(words: torch.Tensor, n: int, n_new: int) -> torch.Tensor:
    """append_items on a visibility row: the row grown to the words of n_new items, the new items n .. n_new - 1 visible.  Pure tensor arithmetic."""
    n_words = (int(n_new) + 31) // 32
    w = torch.zeros(n_words, dtype=torch.int64, device=words.device)
    w[: words.numel()] = words.reshape(-1).to(torch.int64) & 0xFFFFFFFF
    first = torch.arange(n_words, dtype=torch.int64, device=words.device) * 32
    lo, hi = (n - first).clamp(0, 32), (n_new - first).clamp(0, 32)      # the new items of word j are its bits lo .. hi - 1
    w |= ((torch.ones_like(first) << hi) - 1) & ~((torch.ones_like(first) << lo) - 1)
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32).reshape(1, -1)


def hidden_scan_route(n_items: int, num_visible: int, k: int, min_visible_fraction: float = 0.5) -> str:
    """Which route a candidate scan of a module with a hidden set takes -- pure host arithmetic:
      "fused"         the fused scan over the visible items (the scans' visible kernels), guarded by its count check and redo as ever;
      "materialised"  the scores of every item, the hidden columns set to -inf, the usual selection.
    The fused scan's threshold is the r-th largest of the sample's per-group maxima, and a group whose sampled items are all hidden
    contributes -inf.  The plan of n_items sizes the sample for at least 4 r groups, each of which may hold a single sampled item; with a
    fraction v = num_visible / n_items of the items visible, such a plan keeps ~4 r v finite maxima.  v >= 1/2 leaves 2 r of them -- r to
    spare, sqrt(r) standard deviations of the binomial count -- and the visible sample is then the same 1-in-stride sample of the visible
    corpus that the plan's rank r was chosen for: the threshold sits below the visible k-th score and ~r stride visible items above it, as
    without a hidden set.  Below that fraction the threshold may be -inf or too high on every call, every call would pay the scan AND its
    redo, and the materialising route is taken directly.  (k beyond num_visible has been refused before.)"""
    if num_visible < k:
        raise RuntimeError(f"selected index k out of range (k={k}, n={num_visible})")
    return "fused" if num_visible >= min_visible_fraction * n_items else "materialised"


def tags_after_append(tags: torch.Tensor, n: int, n_new: int) -> torch.Tensor:
    """append_items on a tag row: the (n,) int32 row grown to n_new words, the new items n .. n_new - 1 carrying no
    attribute (0: they match no filtered call until set_item_tags(..., positions) tags them).  Pure tensor arithmetic."""
    out = torch.zeros(int(n_new), dtype=torch.int32, device=tags.device)
    out[:n] = tags[:n]
    return out


def tags_after_removal(tags: torch.Tensor, n_new: int, holes: torch.Tensor, movers: torch.Tensor) -> torch.Tensor:
    """remove_items on a tag row: tags belong to the position, so the i-th mover's word -- read BEFORE the cut -- goes to the i-th hole and the
    row is cut to n_new words.  holes / movers: removal_plan's, int64 on the row's device.  Pure tensor arithmetic (a copy: the row given is
    not written)."""
    out = tags[: int(n_new)].clone()
    if holes.numel():
        out.index_copy_(0, holes, tags.index_select(0, movers))
    return out


def groups_after_append(groups: torch.Tensor, n: int, n_new: int) -> torch.Tensor:
    """append_items on a group-key row: the (n,) int32 row grown to n_new keys, the new items n .. n_new - 1 ungrouped
    (-1: they collapse with nothing until set_item_groups(..., positions) keys them).  Pure tensor arithmetic."""
    out = torch.full((int(n_new),), -1, dtype=torch.int32, device=groups.device)
    out[:n] = groups[:n]
    return out


def groups_after_removal(groups: torch.Tensor, n_new: int, holes: torch.Tensor, movers: torch.Tensor) -> torch.Tensor:
    """remove_items on a group-key row: keys belong to the position, so the i-th mover's key -- read BEFORE the cut -- goes to the i-th hole and
    the row is cut to n_new keys (tags_after_removal's rule; a copy: the row given is not written)."""
    return tags_after_removal(groups, n_new, holes, movers)


def vectors_after_append(vectors: torch.Tensor, n: int, n_new: int) -> torch.Tensor:
    """append_items on an item-vector table: the (n, E) fp32 table grown to n_new rows, the new items n .. n_new - 1
    carrying the zero vector (similar to nothing until set_item_vectors(..., positions) gives them one).  Pure tensor arithmetic."""
    out = torch.zeros((int(n_new), vectors.shape[1]), dtype=torch.float32, device=vectors.device)
    out[:n] = vectors[:n]
    return out


def vectors_after_removal(vectors: torch.Tensor, n_new: int, holes: torch.Tensor, movers: torch.Tensor) -> torch.Tensor:
    """remove_items on an item-vector table: vectors belong to the position, so the i-th mover's row -- read BEFORE the cut -- goes to the i-th
    hole and the table is cut to n_new rows (tags_after_removal's rule on rows; a copy: the table given is not written)."""
    return tags_after_removal(vectors, n_new, holes, movers)


GROUP_KEY_LIMIT = (1 << 31) - 1      # group keys lie in [-1, GROUP_KEY_LIMIT)


def group_ranks(groups: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """The dense ranks the collapse kernels read: groups, an (N,) integer row of keys >= 0 or -1 (ungrouped) ->
    ((N,) int32 ranks in [0, G), G): equal keys get equal ranks, every ungrouped item a rank of its own, so G <= N.  A function of the row
    alone -- the ranks of keyed items follow the order of their keys, the ungrouped ones follow in position order -- so an edit chain and a
    fresh module of the resulting row agree.  Integer plumbing in torch ops, on whichever device the row lives (one sync for G)."""
    g = groups.to(torch.int64)
    surrogate = torch.where(g < 0, GROUP_KEY_LIMIT + torch.arange(g.numel(), dtype=torch.int64, device=g.device), g)
    uniq, inverse = torch.unique(surrogate, return_inverse=True)
    return inverse.to(torch.int32).contiguous(), int(uniq.numel())


def parse_allowed_tags(allowed_tags, batch: int) -> Tuple[int, ...]:
    """allowed_tags= as given -> its allow words as host integers: (word,) for a Python int (shared by the batch), else one per query row from
    a sequence or an integer tensor of shape (batch,) (a device tensor is copied to the host: one sync).  ValueError for anything else, a
    word of 0 (it would match nothing) or one outside 32 bits.  Pure host code."""
    if isinstance(allowed_tags, bool):
        raise ValueError("allowed_tags must be an int, or a sequence / integer tensor of one word per query row")
    if isinstance(allowed_tags, int):
        words = (allowed_tags,)
    else:
        if torch.is_tensor(allowed_tags):
            if allowed_tags.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) or allowed_tags.dim() != 1:
                raise ValueError("allowed_tags must be an int, or a sequence / integer tensor of one word per query row")
            values = allowed_tags.cpu().tolist()
        else:
            try:
                values = list(allowed_tags)
            except TypeError:
                raise ValueError("allowed_tags must be an int, or a sequence / integer tensor of one word per query row") from None
        if any(isinstance(v, bool) or not isinstance(v, int) for v in values):
            raise ValueError("allowed_tags must hold integers")
        if len(values) != batch:
            raise ValueError(f"allowed_tags has {len(values)} words but the batch has {batch} rows")
        words = tuple(values)
    for w in words:
        if w == 0:
            raise ValueError("allowed_tags: a word of 0 allows no item")
        if not 0 < w < 1 << 32:
            raise ValueError(f"allowed_tags: {w} is not a 32-bit word (values lie in [1, 2^32))")
    return words


def tagged_scan_route(plan: Optional[Tuple[int, int, int, int]], kept_min: int, n_items: int, k: int, min_groups: float = 2.0) -> str:
    """Which route a candidate scan under allowed_tags= takes -- pure host arithmetic, beside hidden_scan_route:
      "fused"         the fused scan through its tagged kernels, guarded by its count check and redo as ever;
      "materialised"  the scores of every item, the entries a row may not return set to -inf, the usual selection.
    plan = (stride, r, G, s) of the call (engine.scan_plan; None: the sizes have no fused plan): the threshold is the r-th largest of G
    per-group maxima of s sampled items each.  How many candidates pass the threshold does not depend on the kept fraction -- a row's k best
    kept items fall into the 1-in-stride sample as any k items do --, what a small fraction v = kept_min / n_items breaks is the number of
    FINITE maxima the threshold is ranked from: a group keeps one iff at least one of its s sampled items is kept, 1 - (1 - v)^s of them in
    expectation (items kept at random).  Fused iff the least-kept row of the batch still expects min_groups * r finite maxima:
    G (1 - (1 - v)^s) >= 2 r, r to spare as in hidden_scan_route -- whose v >= 1/2 this is for a plan of G = 4 r groups of one item.  A wrong
    guess costs the redo, never the result.  (k beyond kept_min is what a fresh module of kept_min items raises.)"""
    if kept_min < k:
        raise RuntimeError(f"selected index k out of range (k={k}, n={kept_min})")
    if plan is None:
        return "materialised"
    _, r, groups, per_group = plan
    v = min(1.0, kept_min / float(n_items))
    return "fused" if groups * (1.0 - (1.0 - v) ** per_group) >= min_groups * r else "materialised"


def refuse_allowed_tags(module, kwargs, why: str) -> None:
    """allowed_tags= where it is not built: refused by the class's name, before any launch."""
    if kwargs.get("allowed_tags") is not None:
        raise NotImplementedError(f"{type(module).__name__} takes no allowed_tags: {why}")


def refuse_collapse_groups(module, kwargs, what: Optional[str] = None) -> None:
    """collapse_groups=True where it is not built -- the item-sharded wrappers, the hand-off calls they use, and the calls
    that return no ranked ids (all_logits, topk_ids): refused by the class's name, before any launch.  max_per_group= (the quota of the same
    section) is refused in the same places, by its own name."""
    name = type(module).__name__ + ("" if what is None else "." + what)
    if kwargs.get("collapse_groups"):
        raise NotImplementedError(f"{name} takes no collapse_groups: collapsing by item group is built on the single-device modules' forward, "
                                  "forward_filtered, submit and get_top_k_outputs only")
    if kwargs.get("max_per_group") is not None:
        raise NotImplementedError(f"{name} takes no max_per_group: a quota per item group is built on the single-device modules' forward, "
                                  "forward_filtered, submit and get_top_k_outputs only")


def refuse_diversity(module, kwargs, what: Optional[str] = None) -> None:
    """diversify= / diversity_pool= where the re-rank is not built -- the item-sharded wrappers, submit, the hand-off calls
    (coarse_candidates, local_candidates, topk_ids), all_logits and the streaming score calls: refused by the class's name, before any launch."""
    for given in ("diversify", "diversity_pool"):
        if kwargs.get(given) is not None:
            name = type(module).__name__ + ("" if what is None else "." + what)
            raise NotImplementedError(f"{name} takes no {given}: diversifying by maximal marginal relevance is built on the single-device modules' "
                                      "forward, forward_filtered and get_top_k_outputs only")


_FUSION_KWARGS = ("query_lims", "fuse", "query_weights")


def refuse_query_fusion(module, kwargs, what: Optional[str] = None) -> None:
    """query_lims= / fuse= / query_weights= where query fusion is not built -- the approximate modules (their candidates
    are generated per query row), the item-sharded wrappers, submit / result, topk_ids: refused by the class's name, before any launch."""
    given = [name for name in _FUSION_KWARGS if kwargs.get(name) is not None]
    if given:
        name = type(module).__name__ + (" (IVF, use_faiss=True)" if getattr(module, "_use_faiss", False) else "") + ("" if what is None else "." + what)
        raise NotImplementedError(f"{name} takes no {given[0]}: fusing several query rows per user is built on the single-device MoLBruteForceTopK "
                                  "and MIPSBruteForceTopK (forward, get_top_k_outputs, all_logits and the streaming score calls) only; the exhaustive "
                                  "MoLAvgTopK / MoLNaiveTopK / MoLCombTopK fuse over the union of the rows' candidates in forward and get_top_k_outputs "
                                  "once fuse_candidates = True is set on the instance")


def _tag_ks(module) -> Tuple[int, ...]:
    """The sizes a candidate-generating module selects per row: each must fit the items a filtered row may return."""
    return tuple(k for k in (getattr(module, "_avg_top_k", None), getattr(module, "_k_per_group", None)) if k is not None)


class Restriction(NamedTuple):
    """What a call may return when that is not every item: the module's hidden set or the call's resolved allowed_tags=
    (section 3.15; its effective tags hold the hidden set).  Which of the two it is stays in here.  Built once per call by
    _CorpusEdits._restriction -- None for a call with neither, which runs the unrestricted launches and nothing more."""
    hidden: Optional[E.ItemMask]                # the hidden set as a shared mask over the visibility row; None under a tag filter
    tags: Optional[E.TagFilter]
    count: int                                  # items the least-kept row may return (num_visible, or the filter's kept_min): every k is checked against it

    @classmethod
    def of(cls, hidden: Optional[E.ItemMask], tags: Optional[E.TagFilter]) -> Optional["Restriction"]:
        return None if hidden is None and tags is None else cls(hidden, tags, (hidden if tags is None else tags).kept_min)

    def launch_kwargs(self) -> dict:
        """What a fused scan takes beside its plain arguments: its visible kernels' row, or its tagged kernels' filter -- never both."""
        return {"visible": self.hidden.words} if self.tags is None else {"tags": self.tags}

    def mask(self, scores: torch.Tensor, run_if: Optional[torch.Tensor] = None) -> torch.Tensor:
        """In place: -inf in every entry of a materialised score matrix that its row may not return (the rows of one query share its rule)."""
        if self.tags is None:
            return E.scores_mask(scores, self.hidden, run_if=run_if)
        return E.scores_mask_tags(scores, self.tags, run_if=run_if)

    def rows_slice(self, b0: int, b1: int) -> "Restriction":      # (the batch rows b0 .. b1 - 1; the hidden set is every row's)
        return self if self.tags is None else Restriction.of(None, self.tags.rows_slice(b0, b1))

    def allows_fused(self, module, component: bool, batch: int, n: int, k: int) -> bool:
        """The rule of the restriction's kind on whether a fused scan's sampled threshold is expected to hold (a wrong guess costs the redo)."""
        if self.tags is None:
            return hidden_scan_route(n, self.count, k, module.HIDDEN_FUSED_MIN_VISIBLE) == "fused"
        return tagged_scan_route(module._scan_plan(component, batch, n, k), self.count, n, k, module.TAGGED_FUSED_MIN_GROUPS) == "fused"


def upsert_plan(found: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The host rule of upsert_items: `found` ((M,) int64 on the CPU) is where each given id sits in the corpus, -1 where it is absent ->
    (update_rows, update_positions, append_rows): the rows of the argument that replace the items at update_positions, and the rows that are
    appended -- both in the order given, so the i-th appended row lands at position N + i."""
    present = found >= 0
    rows = torch.arange(found.numel(), dtype=torch.int64)
    return rows[present], found[present], rows[~present]


def _by_id_arg(item_ids: torch.Tensor, what: str) -> torch.Tensor:
    if (not torch.is_tensor(item_ids) or item_ids.is_floating_point() or item_ids.is_complex() or item_ids.dtype == torch.bool
            or not (item_ids.dim() == 1 or (item_ids.dim() == 2 and item_ids.shape[0] == 1))):
        raise ValueError(f"{what}: item_ids must be an (M,) or (1, M) integer tensor")
    return item_ids.reshape(-1).to(torch.int64)


class _ItemsById:
    """The corpus addressed by item id, shared by MoLTopKModule and MIPSBruteForceTopK: a device-resident id -> position
    map (engine.ItemIdMap) in front of update_items / append_items / remove_items, which stay the only code that edits the corpus.  The map is
    built from the module's ids at the first by-id call -- ValueError, naming the count, when two items share an id or one carries a reserved
    value (INT64_MIN, INT64_MIN + 1); the module is then exactly what it was and the by-position calls keep working.  From then on the
    by-position calls keep the map in step (at the price of one small read-back per call); a module that never makes a by-id call never
    builds one.  Out of scope: the sharded wrappers (their ranks own slices of the corpus) and an order-preserving compaction --
    remove_items_by_id fills holes from the tail, as remove_items does."""

    _id_map: Optional[E.ItemIdMap] = None

    def _live_id_map(self) -> E.ItemIdMap:
        m = self._id_map
        if m is None:
            m = E.ItemIdMap(self._ids_flat.device)
            m.build(self._ids_flat)
            self._id_map = m
        return m

    def positions_of(self, item_ids: torch.Tensor) -> torch.Tensor:
        """(M,) int64 on the module's device: the position of each id of `item_ids` ((M,) or (1, M), CPU or device), -1 where the corpus has no
        such item.  Read-only; works on every module, the IVF one included."""
        ids = _by_id_arg(item_ids, "positions_of")
        with torch.inference_mode():
            return self._live_id_map().lookup(ids)

    def _resolved(self, item_ids: torch.Tensor, what: str, absent_ok: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (ids (M,) int64 as given, their positions on the CPU); ValueError for an id given twice or, unless absent_ok, an unknown one."""
        ids = _by_id_arg(item_ids, what)
        found = self.positions_of(ids).cpu()      # (the one sync)
        twice = ids.numel() - torch.unique(ids.cpu()).numel()
        if twice:
            raise ValueError(f"{what}: {twice} of the {ids.numel()} item ids repeat an earlier one")
        unknown = int((found < 0).sum())
        if unknown and not absent_ok:
            raise ValueError(f"{what}: {unknown} of the {ids.numel()} item ids are not in the corpus")
        return ids, found

    def mask_of_ids(self, item_ids: torch.Tensor) -> E.ItemMask:
        """The shared item mask that keeps exactly the items carrying `item_ids` ((M,) or (1, M)), resolved through the live
        id map.  ValueError for an unknown id or an id given twice, as update_items_by_id.  A mask is by position: after remove_items (which moves
        rows) or append_items, ask again."""
        _, found = self._resolved(item_ids, "mask_of_ids")
        return E.ItemMask.from_positions(self.num_items, found, self._ids_flat.device)

    def _take_item_mask(self, kwargs: dict, batch: int, k: Optional[int]) -> Optional[E.ItemMask]:
        """item_mask= of a call, taken OUT of its kwargs: None, or the ItemMask (a bool tensor is packed: one sync) checked against this module,
        the batch and k before any launch (engine.check_item_mask)."""
        if "_resolved_mask" in kwargs:      # a collapsed call resolved its mask once and hands it to every arm it runs
            m = kwargs.pop("_resolved_mask")
            if m is not None:
                m.check(self.num_items, batch, k)
            return m
        m = kwargs.pop("item_mask", None)
        if kwargs.get("allowed_tags") is not None:      # a tag filter becomes the call's mask: the hidden set is inside its tags
            if m is not None:
                raise ValueError("allowed_tags= and item_mask= in one call: combining the two is not built; fold one into the other")
            tagged = self._take_allowed_tags(kwargs, batch, ()).item_mask()
            tagged.check(self.num_items, batch, k)
            return tagged
        kwargs.pop("allowed_tags", None)
        vis = self._visible_mask()
        if m is None:
            if vis is not None:      # the hidden set acts as a shared mask of every call
                vis.check(self.num_items, batch, k)
            return vis
        m = E.as_item_mask(m)
        if vis is None:
            m.check(self.num_items, batch, k)
            return m
        m.check(self.num_items, batch, None)
        c = self._and_mask_cache      # the AND of the two, kept per (mask object, hidden-set version): one sync when it is first built
        if c is None or c[0] is not m or c[1] != self._hidden_version:
            c = self._and_mask_cache = (m, self._hidden_version, E.item_mask_and(m, vis))
        c[2].check(self.num_items, batch, k)
        return c[2]

    def update_items_by_id(self, item_ids: torch.Tensor, item_embeddings: torch.Tensor, new_item_ids: Optional[torch.Tensor] = None) -> None:
        """update_items for the items that carry `item_ids` ((M,) or (1, M)); `new_item_ids`, when given, renames them (two items may swap ids in
        one call).  ValueError before anything is touched for an unknown id or an id given twice, naming how many (one device sync)."""
        self._check_updatable("update_items_by_id")
        _, found = self._resolved(item_ids, "update_items_by_id")
        self.update_items(found, item_embeddings, new_item_ids)

    def remove_items_by_id(self, item_ids: torch.Tensor) -> torch.Tensor:
        """remove_items for the items that carry `item_ids` -> its `moved`.  Positions are not stable under removal (holes are filled from the
        tail, no order-preserving compaction): ask positions_of again afterwards."""
        self._check_updatable("remove_items_by_id")
        _, found = self._resolved(item_ids, "remove_items_by_id")
        return self.remove_items(found)

    def upsert_items(self, item_ids: torch.Tensor, item_embeddings: torch.Tensor) -> None:
        """The items of `item_ids` that the corpus holds are updated in place (update_items); the others are appended in the order given
        (append_items: the module then owns its table and ids).  ValueError before anything is touched for an id given twice."""
        self._check_updatable("upsert_items")
        ids, found = self._resolved(item_ids, "upsert_items", absent_ok=True)
        emb, _ = self._update_rows_arg(item_embeddings, None)
        if emb.shape[0] != ids.numel():
            raise ValueError(f"upsert_items: {ids.numel()} item ids but {emb.shape[0]} rows")
        upd, pos, app = upsert_plan(found)
        if upd.numel():
            self.update_items(pos, emb.index_select(0, upd.to(emb.device)))
        if app.numel():
            self.append_items(emb.index_select(0, app.to(emb.device)), ids.index_select(0, app.to(ids.device)).to(self._item_ids.dtype))

    def _ids_at(self, pos: torch.Tensor) -> Optional[torch.Tensor]:
        """The ids at `pos` (device) for a live map -- read BEFORE a by-position call overwrites or moves them."""
        return None if self._id_map is None else self._ids_flat.index_select(0, pos)

    def _id_map_step(self, gone: Optional[torch.Tensor], ids: Optional[torch.Tensor], pos: Optional[torch.Tensor]) -> None:
        """A live map follows a by-position call: the ids `gone` erased in one launch, then `ids` inserted at `pos` in a second (a batch may
        swap ids between positions).  Called with self._ids_flat already what the call leaves.  An id the map did not expect (a duplicate
        among the new ids, most likely) drops the map: the next by-id call builds it again and raises what a fresh module would."""
        m = self._id_map
        if m is None:
            return
        try:
            if gone is not None and gone.numel():
                m.erase(gone)
            if ids is not None and ids.numel():
                m.insert(ids.to(device=self._ids_flat.device, dtype=torch.int64), pos, self._ids_flat)
            ok = not any(m.take_flags())
        except ValueError:
            ok = False
        if not ok:
            self._id_map = None


def _ids_arg(what: str, name: str, ids: torch.Tensor, batch: int, width: str = "T") -> None:
    if not torch.is_tensor(ids) or ids.dim() != 2 or ids.shape[0] != batch or ids.is_floating_point() or ids.dtype == torch.bool:
        raise ValueError(f"{what}: {name} must be ({batch}, {width}) integer ids")


def _positions_arg(what: str, positions: torch.Tensor, batch: int) -> None:
    if not torch.is_tensor(positions) or positions.dtype != torch.int64 or positions.dim() != 2 or positions.shape[0] != batch:
        raise ValueError(f"{what}: positions must be ({batch}, T) int64")


def _join_slices(parts: list):
    """The per-slice results of a streaming call as the call's: tensors joined along the batch, tuples member by member; a single slice is
    returned as it is."""
    if len(parts) == 1:
        return parts[0]
    return tuple(torch.cat(m, 0) for m in zip(*parts)) if isinstance(parts[0], tuple) else torch.cat(parts, 0)


class Streamed(NamedTuple):
    """What a family of streaming calls says where it refuses."""
    lacking: str                                # what a module without exact scores is told it does not have
    whole: str                                  # why a row's logits are needed whole: the tail of the MAX_LOGIT_BYTES refusal


class Fusion(NamedTuple):
    """The resolved query fusion of a call: the checked query_lims=, fuse= and query_weights= (on the module's device)."""
    lims: E.QueryLims
    mode: str
    weights: Optional[torch.Tensor]

    def rows_slice(self, u0: int, u1: int) -> Tuple[int, int, "Fusion"]:
        """The fused rows u0 .. u1 - 1 -> (their first sub-query row, the row past their last, the fusion of that slice alone)."""
        s0, s1 = int(self.lims.host[u0]), int(self.lims.host[u1])
        return s0, s1, Fusion(self.lims.rows_slice(u0, u1), self.mode, None if self.weights is None else self.weights[s0:s1])


_RANK = Streamed("the exact rank of an item", "a target's key must be read from the matrix that is counted, and corpus chunks are not built")
_SOFTMAX = Streamed("the softmax over every item of the corpus", "the normaliser needs every item of a row, and corpus chunks are not built")
_RANGE = Streamed("a range search over every item of the corpus", "a row is counted and written whole, and corpus chunks are not built")


class _StreamingScores(_ItemsById):
    """The calls that stream over the dense (b, N) logit matrix of a query batch (DESIGN sections 3.17 - 3.19): rank_of, the softmax over the
    corpus and range search.  Built on the exact modules, which supply the one hook, _rank_scores; every other module refuses by name before
    any launch.  All of them share one entry check (_streaming_call) and one host flow (_eligible_rows): the row's eligible set -- the
    items it may return: not hidden, inside the call's item_mask= / allowed_tags=, their ids not among the row's invalid_ids -- as mask words,
    and batch slices of the matrix under the logit policy."""

    MAX_LOGIT_BYTES = 4 << 30      # the logit policy: never more (b, N) logits live than this -- a slice of the batch at a time
    # The hook, _rank_scores(query_embeddings, **kwargs): all_logits' (b, N) fp32 scores for these rows, unmasked (a recycled buffer will do: it
    # is consumed before the next call).  None: the module has no exact scores.
    _rank_scores = None

    @contextlib.contextmanager
    def one_bind(self):
        """One look at the module's parameters for a whole call, on the modules that have parameters."""
        yield

    def _refuse_streaming(self, kwargs: dict, what: str, family: Streamed) -> None:
        """Reads the type and kwargs alone."""
        if type(self)._rank_scores is None:
            raise NotImplementedError(f"{type(self).__name__}.{what}: an approximate module ranks its candidates only; {family.lacking} is "
                                      "built on MoLBruteForceTopK (and MIPSBruteForceTopK) -- ask a MoLBruteForceTopK over the same corpus")
        refuse_collapse_groups(self, kwargs, what)
        refuse_diversity(self, kwargs, what)

    def _streaming_call(self, what: str, family: Streamed, query_embeddings: torch.Tensor, invalid_ids: Optional[torch.Tensor], kwargs: dict,
                        family_check: Optional[Callable[[str], None]] = None, matrices: int = 1, policy_as: Optional[str] = None) -> int:
        """The checks of a streaming call, before any launch -> the rows of a batch slice under the logit policy (`matrices` (b, N) matrices
        live).  In this order: the two refusals, the family's own argument checks (family_check, given the call's full name), invalid_ids,
        the policy's refusal (under the name policy_as, where that is not the call's)."""
        self._refuse_streaming(kwargs, what, family)
        fusion = self._resolve_fusion(kwargs, query_embeddings, what)
        if family_check is not None:
            family_check(f"{type(self).__name__}.{what}")
        N = self.num_items
        if invalid_ids is not None:
            _ids_arg(what, "invalid_ids", invalid_ids, self._result_rows(query_embeddings, kwargs), "S")
        if fusion is not None:
            return self._fused_budget(f"{type(self).__name__}.{policy_as or what}", fusion, matrices, family.whole)
        rows = int(self.MAX_LOGIT_BYTES) // (N * 4 * matrices)
        if rows < 1:
            raise NotImplementedError(f"{type(self).__name__}.{policy_as or what}: {'two rows' if matrices == 2 else 'one row'} of {N} logits exceed"
                                      f"{'' if matrices == 2 else 's'} MAX_LOGIT_BYTES; {family.whole}")
        return rows

    # ---- query fusion: several sub-query rows per result row -----------------------------------------------------------
    # query_lims= ((U + 1,) int64, FAISS-shaped): the sub-query rows [lims[u], lims[u + 1]) of query_embeddings belong to fused row u.  With
    # s[r, x] all_logits' bits for sub-query row r, F[u, x] is their fusion over the segment -- fuse="max": the element largest in the
    # selection key's order; "sum": the fp32 chain acc = fl32(acc + s[r, x]), with query_weights= acc = fl32(acc + fl32(w[r] * s[r, x])) -- and
    # every call means what it means on a module whose all_logits is F: per-row arguments and results are per FUSED row (user_ids alone
    # stays per sub-query row).  Two routes: the matrix route fuses the (S, N) logits into (U, N) (engine.scores_fuse_rows) in front of
    # every streaming call and the dense top-k; the list route ("max" alone) merges the sub-query rows' own top-(k + w) lists
    # (engine.topk_fuse_lists) and so keeps whatever route the module's forward takes.
    FUSE_LIST_MAX_ENTRIES = E.FUSE_LIST_MAX_ENTRIES      # entries (sub-query rows x k') of one fused row the list route merges; 0: always the matrix route

    def _resolve_fusion(self, kwargs: dict, query_embeddings: torch.Tensor, what: str) -> Optional[Fusion]:
        """query_lims= / fuse= / query_weights= of a call, taken OUT of its kwargs and checked before any launch (the one host read of a device
        query_lims) -> the Fusion, left in kwargs["_fusion"] for the calls this one makes; None: the call is not fused."""
        if "_fusion" in kwargs:
            return kwargs["_fusion"]
        lims, mode, weights = kwargs.pop("query_lims", None), kwargs.pop("fuse", None), kwargs.pop("query_weights", None)
        name = f"{type(self).__name__}.{what}"
        if lims is None:
            for given, value in (("fuse", mode), ("query_weights", weights)):
                if value is not None:
                    raise ValueError(f"{name}: {given}= without query_lims=")
            return None
        if kwargs.get("collapse_groups") or kwargs.get("max_per_group") is not None:
            raise NotImplementedError(f"{name}: collapse_groups= / max_per_group= together with query_lims= is not built")
        mode = "max" if mode is None else mode
        if mode not in E.FUSE_MODES:
            raise ValueError(f"{name}: fuse must be one of {sorted(E.FUSE_MODES)}, got {mode!r}")
        S, dev = query_embeddings.size(0), self._ids_flat.device
        if weights is not None:
            if mode != "sum":
                raise ValueError(f'{name}: query_weights= goes with fuse="sum", not with {mode!r}')
            if not torch.is_tensor(weights) or weights.dtype != torch.float32 or weights.shape != (S,):
                raise ValueError(f"{name}: query_weights must be ({S},) fp32, one weight per sub-query row")
            weights = weights.to(dev).contiguous()
        fusion = kwargs["_fusion"] = Fusion(E.QueryLims(lims, S, dev, name), mode, weights)
        return fusion

    @staticmethod
    def _result_rows(query_embeddings: torch.Tensor, kwargs: dict) -> int:
        """The rows of a call's per-row arguments and results: the fused rows of a resolved fusion, else the query rows."""
        fusion = kwargs.get("_fusion")
        return query_embeddings.size(0) if fusion is None else fusion.lims.fused

    def _fused_budget(self, name: str, fusion: Fusion, matrices: int, whole: str) -> int:
        """The matrix rows a slice of a fused call may hold under the logit policy: its sub-query rows plus `matrices` rows per fused row."""
        budget = int(self.MAX_LOGIT_BYTES) // (self.num_items * 4)
        if fusion.lims.max_segment + matrices > budget:
            raise NotImplementedError(f"{name}: a segment of {fusion.lims.max_segment} sub-query rows and its fused row{'s' if matrices > 1 else ''} of "
                                      f"{self.num_items} logits exceed MAX_LOGIT_BYTES; a segment is fused whole, and {whole}")
        return budget

    @staticmethod
    def _slice_plan(batch: int, rows: int, fusion: Optional[Fusion], matrices: int = 1) -> list:
        """The batch slices [(b0, b1), ...] of a streaming call: `rows` query rows at a time; under a fusion whole segments, each fused row
        counting its sub-query rows plus `matrices` rows of its own against the budget `rows` (_fused_budget saw that every segment fits)."""
        if fusion is None:
            return [(b0, min(batch, b0 + rows)) for b0 in range(0, batch, rows)]
        sizes = (fusion.lims.host[1:] - fusion.lims.host[:-1]).tolist()
        plan, u0, held = [], 0, 0
        for u, m in enumerate(sizes):
            if held and held + m + matrices > rows:
                plan.append((u0, u))
                u0, held = u, 0
            held += m + matrices
        plan.append((u0, len(sizes)))
        return plan

    def _fused_slices(self, query_embeddings: torch.Tensor, fusion: Fusion, kwargs: dict, plan: list):
        """(u0, u1, F) per slice of `plan`: the sub-query logits of the slice's segments (_rank_scores: the recycled logits buffer) fused into
        the (u1 - u0, N) head of a second buffer shared by the slices -- consumed before the next step.  A payload of kwargs with one row per
        sub-query row is sliced by query_lims, one with a row per fused row by fused row."""
        S, U = fusion.lims.rows, fusion.lims.fused
        fused = torch.empty((max(u1 - u0 for u0, u1 in plan), self.num_items), dtype=torch.float32, device=self._ids_flat.device)
        for u0, u1 in plan:
            s0, s1, part = fusion.rows_slice(u0, u1)
            kw = {key: (v[s0:s1] if v.shape[0] == S else v[u0:u1] if v.shape[0] == U else v) if torch.is_tensor(v) and v.dim() >= 1 else v
                  for key, v in kwargs.items()}
            scores = self._rank_scores(query_embeddings[s0:s1], **kw)
            yield u0, u1, E.scores_fuse_rows(scores, part.lims, part.mode, part.weights, out=fused[: u1 - u0])

    def _fusion_count(self, key: str) -> None:
        stats = self.__dict__.setdefault("_fusion_stats", {"fused_list_calls": 0, "fused_matrix_calls": 0})
        stats[key] += 1

    def fusion_stats(self) -> dict:
        """Which route answered the fused top-k calls so far (fused_list_calls / fused_matrix_calls); empty before the first one."""
        return dict(self.__dict__.get("_fusion_stats", {}))

    def _segment_kwargs(self, kwargs: dict, fusion: Fusion) -> dict:
        """The kwargs of the list route's call on the sub-query rows: a per-fused-row item_mask= / allowed_tags= repeated over its segment."""
        kw, U = dict(kwargs), fusion.lims.fused
        rows = fusion.lims.fused_row_of()
        m = kw.get("item_mask")
        if isinstance(m, E.ItemMask):
            m.check(self.num_items, U, None)
            kw["item_mask"] = m.rows_take(rows)
        elif torch.is_tensor(m) and m.dim() == 2:
            if m.shape[0] != U:
                raise ValueError(f"item_mask has {m.shape[0]} rows but the batch has {U}")
            kw["item_mask"] = m.index_select(0, rows.to(m.device))
        a = kw.get("allowed_tags")
        if a is not None and not isinstance(a, int):
            words = a.words if isinstance(a, E.TagFilter) else parse_allowed_tags(a, U)
            kw["allowed_tags"] = words[0] if len(words) == 1 else [words[u] for u in rows.tolist()]
        return kw

    def _fused_topk(self, what: str, query_embeddings: torch.Tensor, k_prime: int, seen, fusion: Fusion, kwargs: dict, sorted: bool = True):
        """The top-k of a fused call -> (ids (U, k), scores (U, k) fp32): the k' best items of F per fused row, and with seen = (invalid_ids
        (U, w), k) the first k of them whose id is not among the row's invalid_ids (filter_seen_ids' rule).
        The LIST route ("max", k' = k + w, within engine.topk_fuse_lists' limits, a corpus of distinct ids): this module's own forward on the S
        sub-query rows for k' results and no seen filter -- every route it has, unchanged --, their positions (positions_of), one merge launch.
        If x is among the first k eligible-and-unseen items of fused row u and r* the row where x attains its maximum, every item that beats x
        in row r* beats it in F with the same position in the key, so x is among row r*'s top (k + w).
        The MATRIX route (everything else): fuse, mask, select, a slice of whole segments at a time under the logit policy."""
        kwargs.pop("_fusion", None)
        name = f"{type(self).__name__}.{what}"
        U, S, N = fusion.lims.fused, fusion.lims.rows, self.num_items
        inv, k = seen if seen is not None else (None, k_prime)
        if inv is not None:
            _ids_arg(what, "invalid_ids", inv, U, "w")
        w = 0 if inv is None else inv.shape[1]
        with torch.inference_mode(), self.one_bind():
            id_map = None
            if (fusion.mode == "max" and query_embeddings.dtype == torch.float32 and k_prime == k + w and k_prime <= N
                    and fusion.lims.max_segment * k_prime <= self.FUSE_LIST_MAX_ENTRIES and E.topk_fuse_lists_supported(fusion.lims.max_segment, k_prime, k, w, N)):
                try:
                    id_map = self._live_id_map()
                except ValueError:      # two items share an id (the id map's refusal): no position from an id, the matrix route answers
                    id_map = None
            if id_map is not None:
                scores, ids = self.forward(query_embeddings, k_prime, **self._segment_kwargs(kwargs, fusion))
                positions = id_map.lookup(ids.reshape(-1)).view(S, k_prime)
                self._fusion_count("fused_list_calls")
                return E.topk_fuse_lists(scores, positions, fusion.lims, k, self._ids_flat, inv, n_items=N)
            mask = self._take_item_mask(kwargs, U, k_prime)
            budget = self._fused_budget(name, fusion, 1, "corpus chunks are not built for a fused call")
            if k_prime > N:
                raise RuntimeError(f"selected index k out of range (k={k_prime}, n={N})")
            parts = []
            for u0, u1, fused in self._fused_slices(query_embeddings, fusion, kwargs, self._slice_plan(U, budget, fusion)):
                if mask is not None:
                    E.scores_mask(fused, mask.rows_slice(u0, u1))
                if inv is None:
                    s, i = E.topk(fused, k_prime, ids=self._ids_flat, sorted=sorted)
                    parts.append((i, s))
                elif E.topk_filter_fusable(N, k_prime, w, k):
                    parts.append(E.topk_filtered(fused, k_prime, self._ids_flat, inv[u0:u1], k))
                else:
                    s, i = E.topk(fused, k_prime, ids=self._ids_flat)
                    parts.append(E.filter_seen_ids(i, s, inv[u0:u1], k))
            self._fusion_count("fused_matrix_calls")
            return _join_slices(parts)

    def _fused_all_logits(self, query_embeddings: torch.Tensor, fusion: Fusion, kwargs: dict) -> torch.Tensor:
        """all_logits(query_lims=...): F as (U, N) fp32, -inf outside the call's mask."""
        kwargs.pop("_fusion", None)
        with self.one_bind():
            mask = self._take_item_mask(kwargs, fusion.lims.fused, None)
            fused = E.scores_fuse_rows(self._rank_scores(query_embeddings, **kwargs), fusion.lims, fusion.mode, fusion.weights)
            return fused if mask is None else E.scores_mask(fused, mask)

    @contextlib.contextmanager
    def _eligible_rows(self, query_embeddings: torch.Tensor, invalid_ids: Optional[torch.Tensor], kwargs: dict, rows: int, matrices: int = 1):
        """The host flow of the streaming calls: inside the block (inference mode, one bind) the value is a generator of (b0, b1, scores,
        words) over batch slices of at most `rows` rows -- scores: _rank_scores of the slice (a recycled buffer: consumed before the next
        step), words: the eligible items of these rows as engine.scores_rank takes them (None: every item).  Under a fusion (DESIGN section
        3.20) the rows are fused rows, the slices hold whole segments (_slice_plan; `matrices`: the (b, N) matrices the call holds per fused
        row) and scores is the fused matrix."""
        fusion = kwargs.pop("_fusion", None)
        B, N = self._result_rows(query_embeddings, {"_fusion": fusion}), self.num_items
        with torch.inference_mode(), self.one_bind():
            mask = self._take_item_mask(kwargs, B, None)      # the hidden set, allowed_tags= and item_mask= as one mask (its syncs are the call's only ones)
            words = None if mask is None else mask.words
            if invalid_ids is not None and invalid_ids.shape[1] > 0:
                seen = self.positions_of(invalid_ids.reshape(-1)).view(B, -1)
                # a per-row COPY of the mask (a shared row, or "every item", repeated), from which each row's seen positions are cleared
                if words is None:
                    words = E.visibility_row(N, self._ids_flat.device).repeat(B, 1)
                elif mask.shared:
                    words = words.repeat(B, 1)
                else:
                    words = words.clone(memory_format=torch.contiguous_format)
                E.item_mask_clear_rows(words, seen, N)

            def words_of(b0: int, b1: int):
                return None if words is None else words if words.shape[0] == 1 else words[b0:b1]

            def slices():
                for b0 in range(0, B, rows):
                    b1 = min(B, b0 + rows)
                    kw = {key: (v[b0:b1] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B else v) for key, v in kwargs.items()}
                    yield b0, b1, self._rank_scores(query_embeddings[b0:b1], **kw), words_of(b0, b1)

            def fused_slices():
                for u0, u1, fused in self._fused_slices(query_embeddings, fusion, kwargs, self._slice_plan(B, rows, fusion, matrices)):
                    yield u0, u1, fused, words_of(u0, u1)

            yield slices() if fusion is None else fused_slices()

    # ---- rank_of: the exact rank of given items per query row ---------------------------------------------------------
    # rank(b, x) = 1 + the number of items row b may return whose selection key (score descending, position ascending, on all_logits' bits)
    # exceeds x's: the index of x in the row's exhaustive get_top_k_outputs list, plus one.  0: not ranked -- x is not in the corpus or not
    # in the row's eligible set.
    def rank_of(self, query_embeddings: torch.Tensor, target_ids: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """(B, T) int64: the rank of the item carrying target_ids[b, j] ((B, T) integer ids, resolved through the live id map) for query row b;
        0 where the corpus has no such item or the row may not return it.  invalid_ids (B, S): the row's seen ids, which leave its eligible
        set (ids nobody has are ignored).  kwargs: what all_logits takes (user_ids, item_mask=, allowed_tags=)."""
        self._refuse_streaming(kwargs, "rank_of", _RANK)
        self._resolve_fusion(kwargs, query_embeddings, "rank_of")
        B = self._result_rows(query_embeddings, kwargs)
        _ids_arg("rank_of", "target_ids", target_ids, B)
        positions = self.positions_of(target_ids.reshape(-1)).view(B, -1)
        return self.rank_of_positions(query_embeddings, positions, invalid_ids, **kwargs)

    def rank_of_positions(self, query_embeddings: torch.Tensor, positions: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """rank_of for targets given as corpus POSITIONS ((B, T) int64; one outside [0, N), such as the -1 positions_of gives an unknown id, gets
        rank 0)."""
        rows = self._streaming_call("rank_of_positions", _RANK, query_embeddings, invalid_ids, kwargs, policy_as="rank_of",
                                    family_check=lambda _: _positions_arg("rank_of_positions", positions, self._result_rows(query_embeddings, kwargs)))
        with self._eligible_rows(query_embeddings, invalid_ids, kwargs, rows) as slices:
            positions = positions.to(self._ids_flat.device)
            return _join_slices([E.scores_rank(scores, positions[b0:b1], words) for b0, b1, scores, words in slices])

    # ---- softmax over the corpus: log_partition, log_prob_of, sample_items -------------------------------------------------
    # Over the row's eligible set, with beta = fp32(1 / temperature): log_partition = log sum exp(logit * beta), log_prob_of = logit * beta -
    # log_partition, sample_items = draws without replacement from that softmax (Gumbel top-k).
    def _softmax_call(self, what: str, query_embeddings: torch.Tensor, invalid_ids: Optional[torch.Tensor], temperature: float, kwargs: dict,
                      matrices: int = 1) -> int:
        return self._streaming_call(what, _SOFTMAX, query_embeddings, invalid_ids, kwargs, lambda name: E.inv_temperature(temperature, name), matrices)

    def log_partition(self, query_embeddings: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None, temperature: float = 1.0, **kwargs) -> torch.Tensor:
        """(B,) fp32: log sum exp(logit / temperature) over the items query row b may return -- all_logits' bits, the hidden set, the call's
        item_mask= / allowed_tags= and the row's invalid_ids honoured as rank_of honours them --, the normaliser that turns a score of
        get_top_k_outputs into a log-probability.  -inf for a row that may return nothing.  One dense pass and two reads of its matrix."""
        rows = self._softmax_call("log_partition", query_embeddings, invalid_ids, temperature, kwargs)
        with self._eligible_rows(query_embeddings, invalid_ids, kwargs, rows) as slices:
            return _join_slices([E.scores_lse(scores, words, temperature) for _, _, scores, words in slices])

    def log_prob_of(self, query_embeddings: torch.Tensor, target_ids: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None, temperature: float = 1.0,
                    **kwargs) -> torch.Tensor:
        """(B, T) fp32: the log-probability of the item carrying target_ids[b, j] under softmax(logits / temperature) over the items query row
        b may return: fp32(logit * beta) - log_partition.  -inf where the corpus has no such item or the row may not return it."""
        self._softmax_call("log_prob_of", query_embeddings, invalid_ids, temperature, kwargs)
        B = self._result_rows(query_embeddings, kwargs)
        _ids_arg("log_prob_of", "target_ids", target_ids, B)
        positions = self.positions_of(target_ids.reshape(-1)).view(B, -1)
        return self.log_prob_of_positions(query_embeddings, positions, invalid_ids, temperature, **kwargs)

    def log_prob_of_positions(self, query_embeddings: torch.Tensor, positions: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None,
                              temperature: float = 1.0, **kwargs) -> torch.Tensor:
        """log_prob_of for targets given as corpus POSITIONS ((B, T) int64; one outside [0, N) gets -inf)."""
        rows = self._softmax_call("log_prob_of_positions", query_embeddings, invalid_ids, temperature, kwargs)
        _positions_arg("log_prob_of_positions", positions, self._result_rows(query_embeddings, kwargs))
        with self._eligible_rows(query_embeddings, invalid_ids, kwargs, rows) as slices:
            positions = positions.to(self._ids_flat.device)
            return _join_slices([E.scores_log_prob(scores, positions[b0:b1], E.scores_lse(scores, words, temperature), words, temperature)
                                 for b0, b1, scores, words in slices])

    def sample_items(self, query_embeddings: torch.Tensor, num_samples: int, seed: int, temperature: float = 1.0,
                     invalid_ids: Optional[torch.Tensor] = None, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """(ids (B, S) int64, log_probs (B, S) fp32): S = num_samples items per query row drawn WITHOUT replacement from softmax(logits /
        temperature) over the items the row may return, in draw order, each with its log-probability under that softmax (log_prob_of's
        value; the probability of the FIRST draw).  Gumbel top-k: engine.scores_gumbel, then the exact top-k of the perturbed matrix.  A row
        with fewer than S items of non-zero probability ends in (-1, -inf) entries.  seed: an int in [0, 2^64); the noise of (seed, batch row,
        item position) does not depend on how the logit policy slices the batch.  Two (b, N) matrices live per slice."""
        rows = self._softmax_call("sample_items", query_embeddings, invalid_ids, temperature, kwargs, matrices=2)
        B, N, fusion = self._result_rows(query_embeddings, kwargs), self.num_items, kwargs.get("_fusion")
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or not 1 <= num_samples <= min(N, E.TOPK_MAX_K):
            raise ValueError(f"sample_items: num_samples must be an int in [1, {min(N, E.TOPK_MAX_K)}] (the corpus holds {N} items, the exact top-k "
                             f"takes k <= {E.TOPK_MAX_K}), got {num_samples!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"sample_items: seed must be an int in [0, 2^64), got {seed!r}")
        with self._eligible_rows(query_embeddings, invalid_ids, kwargs, rows, matrices=2) as slices:
            parts = []
            most = max(b1 - b0 for b0, b1 in self._slice_plan(B, rows, fusion, 2))
            perturbed = torch.empty((most, N), dtype=torch.float32, device=self._ids_flat.device)      # the second matrix (the third of a fused call), shared by the slices
            for b0, b1, scores, words in slices:
                noisy = E.scores_gumbel(scores, seed, b0, words, temperature, out=perturbed[: b1 - b0])
                top, pos = E.topk(noisy, num_samples)
                lp = E.scores_log_prob(scores, pos, E.scores_lse(scores, words, temperature), words, temperature)
                drawn = top != float("-inf")      # (a perturbed -inf: an item outside the row's eligible set, or one of probability zero)
                parts.append((torch.where(drawn, self._ids_flat[pos], -1), torch.where(drawn, lp, float("-inf"))))
            return _join_slices(parts)

    # ---- range search: count_above, range_search ---------------------------------------------------------------------------
    # Which items of the row's eligible set meet the row's threshold, and how many: logit >= min_score on all_logits' bits, or log_prob_of's
    # value >= min_log_prob.  An IEEE fp32 compare (NaN on either side: no hit).
    def _range_call(self, what: str, query_embeddings: torch.Tensor, min_score, min_log_prob, temperature: float, invalid_ids: Optional[torch.Tensor],
                    kwargs: dict) -> Tuple[int, torch.Tensor]:
        """The checks of a range call, before any launch -> (the rows of a batch slice under the logit policy, the (B,) fp32 thresholds)."""
        def one_threshold(name: str) -> None:
            if (min_score is None) == (min_log_prob is None):
                raise ValueError(f"{name}: exactly one of min_score= and min_log_prob= is given, got {'both' if min_score is not None else 'neither'}")
            if E.inv_temperature(temperature, name) != 1.0 and min_score is not None:
                raise ValueError(f"{name}: temperature = {temperature!r} with min_score=: a score threshold is compared with the raw logit; "
                                 "temperature goes with min_log_prob=")

        rows = self._streaming_call(what, _RANGE, query_embeddings, invalid_ids, kwargs, one_threshold)
        return rows, E.range_thresholds(f"{type(self).__name__}.{what}", min_score if min_score is not None else min_log_prob,
                                        self._result_rows(query_embeddings, kwargs), self._ids_flat.device)

    def count_above(self, query_embeddings: torch.Tensor, min_score=None, *, min_log_prob=None, temperature: float = 1.0,
                    invalid_ids: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """(B,) int64: how many items query row b may return score at least its threshold -- logit >= min_score on all_logits' bits, or
        log_prob_of's value (at `temperature`) >= min_log_prob; exactly one of the two, a number or a (B,) tensor.  The hidden set, the
        call's item_mask= / allowed_tags= and the row's invalid_ids are honoured as rank_of honours them.  One dense pass and one read of its
        matrix (three in the log-probability form: the normaliser first); no host sync beyond the mask's."""
        rows, thr = self._range_call("count_above", query_embeddings, min_score, min_log_prob, temperature, invalid_ids, kwargs)
        with self._eligible_rows(query_embeddings, invalid_ids, kwargs, rows) as slices:
            return _join_slices([E.scores_range_count(scores, thr[b0:b1], words, temperature,
                                                      None if min_log_prob is None else E.scores_lse(scores, words, temperature))
                                 for b0, b1, scores, words in slices])

    def range_search(self, query_embeddings: torch.Tensor, min_score=None, *, min_log_prob=None, temperature: float = 1.0,
                     invalid_ids: Optional[torch.Tensor] = None, sort: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(lims (B + 1,) int64, scores (lims[B],) fp32, ids (lims[B],) int64): the items count_above counts, row b's in
        [lims[b], lims[b + 1]) with their raw logits.  sort=True: each row in get_top_k_outputs' order (score descending, then position
        ascending) -- that exhaustive ranking without the items that miss; a row of more than engine.RANGE_SORT_MAX hits raises ValueError.
        sort=False: position ascending, any count.  One read-back of lims per batch slice of the logit policy, the call's only sync beyond
        the mask's."""
        rows, thr = self._range_call("range_search", query_embeddings, min_score, min_log_prob, temperature, invalid_ids, kwargs)
        with self._eligible_rows(query_embeddings, invalid_ids, kwargs, rows) as slices:
            parts = []
            for b0, b1, scores, words in slices:
                lse = None if min_log_prob is None else E.scores_lse(scores, words, temperature)
                lims, s, i = E.scores_range(scores, thr[b0:b1], words, temperature, lse, ids=self._ids_flat, sort=sort)
                parts.append((lims if not parts else lims[1:] + parts[-1][0][-1], s, i))      # (cumulative over the slices; a device add, no sync)
            return _join_slices(parts)

    # ---- score_of / explain_of: caller-given items, scored and explained pair by pair -----------------------------------
    # score_of[b, j] is all_logits(q, **kwargs)[b, position of item_ids[b, j]] bit for bit -- -inf where the corpus has no such item or row b may
    # not return it (rank_of's eligible set) -- at O(B T) cost: the positions are scored in place on the index (the hooks below), one
    # eligibility launch follows (engine.scores_at_eligible), and nothing of size N is allocated, read or written.  explain_of adds the
    # mixture behind each score: the L = P_Q P_X cross logits after the division by tau and the weights of the reference's eval-mode combiner.
    # The hooks: _pair_scores(query_embeddings, positions, kwargs) -> (B, T) fp32, all_logits' bits at VALID positions (the flow clamps them);
    # _pair_explained(query_embeddings, positions, kwargs) -> (component_logits, weights), (B, T, L) each.
    _pair_scores = None
    _pair_explained = None

    def _refuse_pair_engine(self, what: str) -> None:
        """The refusals that need the module's engine (the MoL modules: precision, envelope); behind _refuse_pairs, before any launch."""
    _PAIR_ITEM_MASK = True      # item_mask= is taken where all_logits takes it

    def _refuse_pairs(self, kwargs: dict, what: str) -> None:
        """The refusals of the pair-level calls, before any launch; reads the type and kwargs alone."""
        name = f"{type(self).__name__}.{what}"
        if getattr(self, "_use_faiss", False):
            raise NotImplementedError(f"{type(self).__name__} (IVF, use_faiss=True).{what}: the IVF module keeps no index of every item to score "
                                      "positions on; the exhaustive modules over the same corpus take the call")
        if type(self)._pair_scores is None:
            raise NotImplementedError(f"{name}: scoring caller-given items is built on the single-device MoL top-k modules and MIPSBruteForceTopK")
        for given in _FUSION_KWARGS:
            if kwargs.get(given) is not None:
                raise NotImplementedError(f"{name} takes no {given}: a pair-level call scores (query row, item) pairs, and fusing query rows "
                                          "over caller-given items is not built; fuse the returned scores")
        refuse_collapse_groups(self, kwargs, what)
        refuse_diversity(self, kwargs, what)
        if not self._PAIR_ITEM_MASK and kwargs.get("item_mask") is not None:
            raise NotImplementedError(f"{name} takes no item_mask: {type(self).__name__} takes none in any call; MoLBruteForceTopK and "
                                      "MIPSBruteForceTopK take it")
        if what.startswith("explain_of") and type(self)._pair_explained is None:
            raise NotImplementedError(f"{name}: there is no mixture to explain -- {type(self).__name__} scores plain dot products; score_of "
                                      "returns them")

    def _pair_count(self, key: str) -> None:
        stats = self.__dict__.setdefault("_pair_stats", {"score_of_calls": 0, "explain_calls": 0})
        stats[key] += 1

    def pair_stats(self) -> dict:
        """score_of_calls / explain_calls (part of stats()); empty before the first pair-level call."""
        return dict(self.__dict__.get("_pair_stats", {}))

    def _pairs_call(self, what: str, query_embeddings: torch.Tensor, positions: torch.Tensor, invalid_ids: Optional[torch.Tensor], kwargs: dict,
                    explain: bool):
        """The one host flow of the four calls.  positions: (B, T) int64 on the module's device, anything outside [0, N) is absent."""
        B, N = query_embeddings.size(0), self.num_items
        if invalid_ids is not None:
            _ids_arg(what, "invalid_ids", invalid_ids, B, "S")
        with torch.inference_mode(), self.one_bind():
            # the row's eligible set, as rank_of / log_prob_of take it -- but never as a per-row matrix of N bits: a tag filter stays its
            # effective tags and allow words, the seen ids stay ids
            tags = mask = None
            if kwargs.get("allowed_tags") is not None:
                if kwargs.get("item_mask") is not None:
                    raise ValueError("allowed_tags= and item_mask= in one call: combining the two is not built; fold one into the other")
                tags = self._take_allowed_tags(kwargs, B, ())
            else:
                mask = self._take_item_mask(kwargs, B, None)
            valid = positions.clamp(0, N - 1)
            extras = None
            if explain:
                cl, pi = self._pair_explained(query_embeddings, valid, kwargs)
                extras = (pi, cl)
            scores = self._pair_scores(query_embeddings, valid, kwargs)
            E.scores_at_eligible(scores, positions, N, mask, tags, invalid_ids, self._ids_flat, extras)
            self._pair_count("explain_calls" if explain else "score_of_calls")
            if not explain:
                return scores
            s = self.mol_module.shape_spec()
            shape4 = (B, positions.shape[1], s.query_dot_product_groups, s.item_dot_product_groups)
            return Explained(scores, pi.view(shape4), cl.view(shape4))

    def _pairs_by_id(self, what: str, query_embeddings: torch.Tensor, item_ids: torch.Tensor, kwargs: dict) -> torch.Tensor:
        self._refuse_pairs(kwargs, what)
        self._refuse_pair_engine(what)
        B = query_embeddings.size(0)
        _ids_arg(what, "item_ids", item_ids, B)
        if item_ids.shape[1] < 1:
            raise ValueError(f"{what}: item_ids must be ({B}, T) with T >= 1")
        return self.positions_of(item_ids.reshape(-1)).view(B, -1)

    def _pairs_by_position(self, what: str, query_embeddings: torch.Tensor, positions: torch.Tensor, kwargs: dict) -> torch.Tensor:
        self._refuse_pairs(kwargs, what)
        self._refuse_pair_engine(what)
        _positions_arg(what, positions, query_embeddings.size(0))
        if positions.shape[1] < 1:
            raise ValueError(f"{what}: positions must be ({query_embeddings.size(0)}, T) with T >= 1")
        return positions.to(self._ids_flat.device).contiguous()

    def score_of(self, query_embeddings: torch.Tensor, item_ids: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """(B, T) fp32: the score of the item carrying item_ids[b, j] ((B, T) integer ids, CPU or device, repeats allowed, resolved through the
        live id map) for query row b -- all_logits' bits for that pair, -inf where the corpus has no such item or the row may not return it
        (hidden, outside item_mask= / allowed_tags=, its id among the row's invalid_ids).  No dense pass: O(B T).  kwargs: what all_logits
        takes (user_ids, item_mask=, allowed_tags=)."""
        positions = self._pairs_by_id("score_of", query_embeddings, item_ids, kwargs)
        return self._pairs_call("score_of", query_embeddings, positions, invalid_ids, kwargs, False)

    def score_of_positions(self, query_embeddings: torch.Tensor, positions: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """score_of for items given as corpus POSITIONS ((B, T) int64; one outside [0, N), such as the -1 positions_of gives an unknown id, gets -inf)."""
        positions = self._pairs_by_position("score_of_positions", query_embeddings, positions, kwargs)
        return self._pairs_call("score_of_positions", query_embeddings, positions, invalid_ids, kwargs, False)

    def explain_of(self, query_embeddings: torch.Tensor, item_ids: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None, **kwargs) -> "Explained":
        """score_of with the mixture behind each score -> Explained(logits (B, T), weights (B, T, P_Q, P_X), component_logits (B, T, P_Q, P_X)):
        logits is score_of's result for the same call; component_logits[b, j, p, m] the cross logit of query component p and item component m
        after the division by the temperature; weights the mixture weights of the reference's eval-mode combiner (they sum to 1).  Both are 0
        where logits is -inf.  fp32 MoL engines inside the generic route's envelope only."""
        positions = self._pairs_by_id("explain_of", query_embeddings, item_ids, kwargs)
        return self._pairs_call("explain_of", query_embeddings, positions, invalid_ids, kwargs, True)

    def explain_of_positions(self, query_embeddings: torch.Tensor, positions: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None, **kwargs) -> "Explained":
        """explain_of for items given as corpus POSITIONS ((B, T) int64)."""
        positions = self._pairs_by_position("explain_of_positions", query_embeddings, positions, kwargs)
        return self._pairs_call("explain_of_positions", query_embeddings, positions, invalid_ids, kwargs, True)


class Explained(NamedTuple):
    """What explain_of returns."""
    logits: torch.Tensor                        # (B, T) fp32: score_of's result
    weights: torch.Tensor                       # (B, T, P_Q, P_X) fp32: the mixture weights, 0 where logits is -inf
    component_logits: torch.Tensor              # (B, T, P_Q, P_X) fp32: the cross logits after the division by tau, 0 where logits is -inf


IN_PLACE, CONCATENATED, CUT_AND_FILLED = "in place", "concatenated", "cut and filled"


class CorpusEdit(NamedTuple):
    """One in-place change of the corpus -- what update_items / append_items / remove_items hand to _CorpusEdits._apply."""
    n_new: int                                  # items afterwards
    positions: torch.Tensor                     # (M',) int64 on the device: the positions to rewrite; ids that are inserted go to these too
    rows: Optional[torch.Tensor]                # their raw rows; None: the rows at `movers`, read before the write
    how: str                                    # table and ids written IN_PLACE, CONCATENATED, or CUT_AND_FILLED from `movers`
    ids: Optional[torch.Tensor] = None          # ids to insert at `positions`; None: the ids are not edited (the movers' ids, when cut and filled)
    gone: Optional[torch.Tensor] = None         # device positions whose ids a live id map erases first (read before the write)
    movers: Optional[torch.Tensor] = None       # CUT_AND_FILLED: device positions, the i-th of them moves to the i-th of `positions`


class Held(NamedTuple):
    """One derived buffer of a module under a corpus edit: everything the edit flow knows about it.  Functions of (module, engine, ...); a
    module class lists its own in _HELD, next to the code that builds the buffer lazily, and holds those of its bases before them."""
    attrs: Tuple[str, ...]                      # the attributes that hold it (None = not built)
    held: Callable[..., bool]                   # (tk, eng): built, and under this engine?  Not held: the edit leaves it alone -- unbuilt stays unbuilt
    resize: Optional[Callable[..., None]]       # (tk, eng, n_new): to n_new items, with a fresh build's padding; new entries are written by refresh
    refresh: Optional[Callable[..., None]]      # (tk, eng, pos, rows): the entries at device positions `pos`, whose raw rows are `rows`
    drop: Optional[Callable[..., None]]         # (tk): the corpus size chose another engine -- nothing derived under the old one stays
    settle: Optional[Callable[..., None]] = None    # (tk, eng): after the edit, resized or not


class _CorpusEdits(_StreamingScores):
    """The in-place corpus API, shared by MoLTopKModule and MIPSBruteForceTopK: the three calls describe themselves as a
    CorpusEdit and _apply is the one flow that carries it out, over the class's list of held buffers.  After any sequence of the calls the
    module holds what a module freshly constructed from the resulting table and ids holds -- every derived buffer bit for bit -- and answers
    alike.  All three are issued on the current stream, behind everything already enqueued there; the module's own side streams are JOINED
    first: handles outstanding from submit() keep the results of the corpus they were submitted against.
    A module supplies num_items, _row_format, _rows_at and _HELD; one with a raw table _write_table; one with a choice of engines _bind,
    _engine_for_bind, _join_side_streams and _forget_corpus_choices."""

    _HELD: Tuple[Held, ...] = ()
    _upd_source = None

    @classmethod
    def _held_buffers(cls) -> Tuple[Held, ...]:
        """Base classes' buffers first: the order of the launches (the index, its row copy, the fp32 companion and its row copy, the tables
        with the pre-filter behind the coarse one, the IVF lists)."""
        return tuple(h for k in reversed(cls.__mro__) for h in k.__dict__.get("_HELD", ()))

    def update_items(self, positions: torch.Tensor, item_embeddings: torch.Tensor, item_ids: Optional[torch.Tensor] = None) -> None:
        """Replace the items at `positions` ((M,) int64, CPU or device: POSITIONS 0 .. N-1 of this module's corpus, not ids; unique) by the rows of
        `item_embeddings` ((M, D) or (1, M, D), on the module's device, the table's dtype) and, when given, their ids by `item_ids` ((M,) or
        (1, M)).  The rows are written INTO the item table (and the ids into the id tensor) the module borrowed at construction: the caller's
        tensors change too (a module that keeps no raw table writes the ids alone).  Every derived buffer the module holds is then brought up
        to date at those positions only; one not built yet stays unbuilt.  ValueError before any launch for bad shapes / dtypes / positions
        (the uniqueness check costs one device sync when the positions live on the device).  M = 0 is a no-op."""
        self._check_updatable("update_items")
        emb, ids = self._update_rows_arg(item_embeddings, item_ids)
        pos = _checked_positions(positions, emb.shape[0], self.num_items)
        if emb.shape[0]:
            pos = pos.to(self._ids_flat.device)
            self._apply(CorpusEdit(self.num_items, pos, emb, IN_PLACE, ids=ids, gone=None if ids is None else pos))

    def append_items(self, item_embeddings: torch.Tensor, item_ids: torch.Tensor) -> None:
        """Grow the corpus from N to N + M items, the new ones at positions N .. N + M - 1.  Every held buffer is grown with device copies and the
        new range goes through update_items' kernels: no old item is recomputed -- unless the larger corpus makes the module choose another
        engine (the default exact mode turning proved at 16 384 items: what was derived under the old one is dropped and the new engine's
        buffers are built from the table, as for a fresh module).  Everything a fresh module decides from N is decided again for N + M.  From
        this call on the module OWNS its item table and ids (the caller's tensors are no longer written)."""
        self._check_updatable("append_items")
        emb, ids = self._update_rows_arg(item_embeddings, item_ids, appending=True)
        n, m = self.num_items, emb.shape[0]
        if m:
            self._apply(CorpusEdit(n + m, torch.arange(n, n + m, dtype=torch.int64, device=self._ids_flat.device), emb, CONCATENATED, ids=ids))

    def remove_items(self, positions: torch.Tensor) -> torch.Tensor:
        """Shrink the corpus from N to N' = N - M items: the items at `positions` ((M,) int64, CPU or device: POSITIONS, not ids; unique) go, and the
        holes they leave below N' are filled from the tail (removal_plan: O(M) rows move, every other item keeps its position).  -> `moved`, a CPU
        int64 tensor of rows [from, to], for callers that keep positions.  A mover's bytes at its new position are what update_items writes there;
        every held buffer is then cut to what a fresh module of N' items holds, and everything a fresh module decides from N is decided again for
        N' (the default exact mode turns dense below 16 384 items: the module then holds a fresh dense module's buffers and nothing more).  From
        this call on the module OWNS its item table and ids; the caller's tensors are not written.  ValueError before anything is touched (one
        device sync when the positions live on the device).  M = 0 is a no-op."""
        n = self.num_items
        self._check_updatable("remove_items", n - positions.numel() if torch.is_tensor(positions) and positions.dim() == 1 else None)
        holes, movers, moved = _removal_arg(positions, n)
        if positions.numel():
            dev = self._ids_flat.device
            self._apply(CorpusEdit(n - positions.numel(), holes.to(dev), None, CUT_AND_FILLED, gone=positions.to(dev), movers=movers.to(dev)))
        return moved

    # ---- hidden items: a persistent, module-level set of items no call returns ---------------------------------------
    # State: one row of visibility words in the ItemMask layout (bit set = visible, the unused high bits of the last word zero), None while
    # nothing is hidden -- such a module runs exactly the launches of one that never heard of hiding.  A module with hidden set H answers every
    # call as a module freshly constructed from the visible rows and their ids would (scores and ids bit for bit; positions, where a call returns
    # positions, are this module's).  Visibility belongs to the POSITION: update_items leaves it, append_items adds visible items,
    # remove_items moves a mover's bit to its hole (visibility_after_removal).  num_hidden / num_visible are host integers from the one
    # read-back of the hide / unhide / remove call -- a query call never syncs for them.
    _visible: Optional[torch.Tensor] = None
    _num_hidden: int = 0
    _hidden_version: int = 0
    _visible_mask_cache = None
    _and_mask_cache = None

    @property
    def num_hidden(self) -> int:
        return self._num_hidden

    @property
    def num_visible(self) -> int:
        return self.num_items - self._num_hidden

    def hide_items(self, positions: torch.Tensor) -> None:
        """The items at `positions` ((M,) int64, CPU or device: POSITIONS, checked as update_items checks them) are returned by no call from now on,
        until unhide_items; hiding a hidden item again is harmless.  Nothing is moved or copied but the visibility row (N / 8 bytes).  ValueError
        before anything is touched for bad positions, or if no item would stay visible.  M = 0 is a no-op."""
        self._set_visibility(positions, False, "hide_items")

    def unhide_items(self, positions: torch.Tensor) -> None:
        """The items at `positions` are visible again (those that were visible stay so)."""
        self._set_visibility(positions, True, "unhide_items")

    def hide_items_by_id(self, item_ids: torch.Tensor) -> None:
        """hide_items for the items that carry `item_ids`, through the live id map; unknown or repeated ids are refused as in update_items_by_id."""
        self._check_hideable("hide_items_by_id")
        _, found = self._resolved(item_ids, "hide_items_by_id")
        self.hide_items(found)

    def unhide_items_by_id(self, item_ids: torch.Tensor) -> None:
        self._check_hideable("unhide_items_by_id")
        _, found = self._resolved(item_ids, "unhide_items_by_id")
        self.unhide_items(found)

    def hidden_positions(self) -> torch.Tensor:
        """(num_hidden,) int64 on the module's device, ascending: the hand-off of the hidden set (it is not part of state_dict)."""
        self._check_hideable("hidden_positions")
        dev = self._ids_flat.device
        if self._visible is None:
            return torch.empty(0, dtype=torch.int64, device=dev)
        with torch.inference_mode():
            inv = torch.bitwise_not(self._visible)
            inv[0, -1] &= E.last_word_mask(self.num_items)
            return E.item_mask_of_words(inv, self.num_items, self._num_hidden).positions()[0]

    def compact(self) -> torch.Tensor:
        """remove_items(hidden_positions()): the hidden items leave the corpus for good -> remove_items' `moved`.  Afterwards nothing is hidden."""
        self._check_hideable("compact")
        return self.remove_items(self.hidden_positions())

    def _check_hideable(self, what: str) -> None:
        """The refusal point of the hidden set: modules whose candidate generation cannot honour it raise here, before anything is touched."""

    def _set_visibility(self, positions: torch.Tensor, visible: bool, what: str) -> None:
        self._check_hideable(what)
        if not torch.is_tensor(positions) or positions.dim() != 1:
            raise ValueError("positions must be (M,) int64")
        n = self.num_items
        pos = _checked_positions(positions, positions.numel(), n)
        if not pos.numel() or (visible and self._visible is None):
            return
        with torch.inference_mode():
            self._join_side_streams()      # handles outstanding from submit() keep the corpus they were submitted against
            dev = self._ids_flat.device
            words = self._visible if self._visible is not None else E.visibility_row(n, dev)
            words, kept = E.visibility_edit(words, n, pos.to(dev), visible)      # a copy: the row in use is not written
            if kept < 1:
                raise ValueError(f"{what}: hiding these {pos.numel()} positions would leave none of the {n} items visible")
            self._visibility_is(words, n - kept)

    def _visibility_is(self, words: Optional[torch.Tensor], num_hidden: int) -> None:
        """The new state; a row without a hidden item is dropped, so that unhiding everything restores the launches of a module that never hid."""
        self._visible = words if num_hidden else None
        self._num_hidden = int(num_hidden)
        self._hidden_version += 1
        self._visible_mask_cache = self._and_mask_cache = None

    def _visible_mask(self) -> Optional[E.ItemMask]:
        """The hidden set as a shared ItemMask (what rails_scores_mask and the exact modules' masked strategies take); None: nothing hidden."""
        if self._visible is None:
            return None
        m = self._visible_mask_cache
        if m is None:
            m = self._visible_mask_cache = E.item_mask_of_words(self._visible, self.num_items, self.num_visible)
        return m

    def _restriction(self, tags: Optional[E.TagFilter] = None) -> Optional[Restriction]:
        """(the hidden set, the call's resolved allowed_tags=) as the one value the candidate scans and all_logits deal with; None: neither."""
        return Restriction.of(None if tags is not None else self._visible_mask(), tags)

    def _visibility_step(self, e: CorpusEdit, n: int) -> None:
        """The visibility row follows an edit (called by _apply with the movers still where they were)."""
        if self._visible is None:
            return
        if e.how == CONCATENATED:
            self._visibility_is(visibility_after_append(self._visible, n, e.n_new), self._num_hidden)
        elif e.how == CUT_AND_FILLED:
            words = visibility_after_removal(self._visible, e.n_new, e.positions, e.movers)
            self._visibility_is(words, e.n_new - E.visibility_count(words, e.n_new))      # (one read-back, inside the removal)

    # ---- item tags: one 32-bit word of attributes per item, and allowed_tags= on the calls --------------------------------
    # State: an owned (N,) int32 tensor of bit patterns, None until set_item_tags -- such a module runs exactly the launches it ran before.  Bit j
    # set = the item carries attribute j.  A call with allowed_tags= returns, in row b, only items x with tags[x] & allowed[b] != 0 that are
    # not hidden, and equals row b of the same call on a module freshly built from those rows and their ids.  An item with word 0 matches no
    # filtered call and stays visible to unfiltered ones.  Tags belong to the POSITION: update_items leaves them, append_items adds words
    # of 0, remove_items moves a mover's word to its hole (tags_after_append / tags_after_removal).  The kernels read one array, the
    # EFFECTIVE tags (a hidden item's word is 0), cached per (tags, hidden set); the kept count of every distinct allow word is read back once
    # and cached with it, so a repeated filter costs a call no sync.
    _tags: Optional[torch.Tensor] = None
    _tags_version: int = 0
    _tag_cache = None              # (stamp, effective tags, {word: kept count}, {words: TagFilter})
    TAG_FILTERS_KEPT = 64          # resolved filters kept per module (a per-row filter holds B words on the device)

    @property
    def item_tags(self) -> Optional[torch.Tensor]:
        """The (N,) int32 tag words on the module's device (bit patterns: a word with bit 31 set reads negative), or None while no tags are
        set.  The hand-off of the tags -- they are not part of state_dict; set_item_tags takes this tensor back as it is."""
        return self._tags

    def set_item_tags(self, tags: torch.Tensor, positions: Optional[torch.Tensor] = None) -> None:
        """One tag word per item.  tags: (N,) -- every item -- or (M,) with positions ((M,) int64, CPU or device, unique POSITIONS); int64 values
        in [0, 2^32), or int32 taken as the bit patterns themselves (what item_tags returns); on the module's device.  A call with positions on
        a module without tags builds the row with every other item at 0.  ValueError before anything is touched for a wrong shape, dtype,
        device, value or position (the value check of int64 tags and the position check cost one sync each).  The stored tensor is the
        module's own: neither argument is aliased, and a row already handed to enqueued launches is not written."""
        n = self.num_items
        dev = self._ids_flat.device
        if not torch.is_tensor(tags) or tags.dim() != 1 or tags.dtype not in (torch.int32, torch.int64):
            raise ValueError("tags must be an (N,) or (M,) int32 / int64 tensor")
        if tags.device != dev:
            raise ValueError(f"tags must live on the module's device {dev}, got {tags.device}")
        m = tags.numel()
        if positions is None:
            if m != n:
                raise ValueError(f"tags has {m} words but the module holds {n} items (pass positions to tag a subset)")
        else:
            positions = _checked_positions(positions, m, n)
        if tags.dtype == torch.int64 and m:
            lo, hi = torch.aminmax(tags)
            if int(lo) < 0 or int(hi) >= 1 << 32:
                raise ValueError("tags must lie in [0, 2^32)")
        with torch.inference_mode():
            self._join_side_streams()
            if tags.dtype == torch.int64:
                tags = torch.where(tags >= 1 << 31, tags - (1 << 32), tags).to(torch.int32)
            if positions is None:
                row = tags.clone()
            else:
                row = torch.zeros(n, dtype=torch.int32, device=dev) if self._tags is None else self._tags.clone()
                row.index_copy_(0, positions.to(dev), tags)
            self._tags_are(row)

    def _tags_are(self, row: Optional[torch.Tensor]) -> None:
        self._tags = row
        self._tags_version += 1
        self._tag_cache = None

    def _tags_step(self, e: CorpusEdit, n: int) -> None:
        """The tag row follows an edit (called by _apply)."""
        if self._tags is None:
            return
        if e.how == CONCATENATED:
            self._tags_are(tags_after_append(self._tags, n, e.n_new))
        elif e.how == CUT_AND_FILLED:
            self._tags_are(tags_after_removal(self._tags, e.n_new, e.positions, e.movers))

    # ---- item groups: one group key per item, and collapse_groups=True on the calls ------------------------------------
    # State: an owned (N,) int32 row of keys (>= 0, or -1: ungrouped), None until set_item_groups -- such a module runs exactly the launches it
    # ran before.  A call with collapse_groups=True returns, per row, the first k items of the row's ranking (score desc, position asc, over the
    # items the row may return and has not seen) whose key is -1 or differs from the key of every earlier item of that ranking: each group is
    # represented by its best eligible item.  Keys belong to the POSITION and follow edits as tags do (groups_after_append / groups_after_removal).
    # The kernels read the DENSE ranks of the keys (group_ranks), computed once per row and kept.
    # max_per_group=m on the same calls keeps the first m items of each key in place of the first one (m = 1 IS collapse_groups=True).
    _groups: Optional[torch.Tensor] = None
    _group_rank_cache = None       # (ranks (N,) int32, G) of the current row
    COLLAPSE_DEPTH_FACTOR = 2      # the exact modules' first walk looks at this many times k + width ranked items ...
    COLLAPSE_MAX_DEPTH = 4096      # ... and a walk that found too few groups doubles its depth up to this; beyond it the group-maxima pass answers

    @property
    def item_groups(self) -> Optional[torch.Tensor]:
        """The (N,) int32 group keys on the module's device, or None while no groups are set.  The hand-off of the keys -- they are not part of
        state_dict; set_item_groups takes this tensor back as it is."""
        return self._groups

    def set_item_groups(self, groups: torch.Tensor, positions: Optional[torch.Tensor] = None) -> None:
        """One group key per item.  groups: (N,) -- every item -- or (M,) with positions ((M,) int64, CPU or device, unique POSITIONS); int32 or
        int64 values in [-1, 2^31 - 1), -1 = ungrouped; on the module's device.  A call with positions on a module without groups builds the
        row with every other item at -1.  ValueError before anything is touched for a wrong shape, dtype, device, value or position (the
        value check and the position check cost one sync each).  The stored row is the module's own: neither argument is aliased."""
        self._check_collapsible("set_item_groups")
        n = self.num_items
        dev = self._ids_flat.device
        if not torch.is_tensor(groups) or groups.dim() != 1 or groups.dtype not in (torch.int32, torch.int64):
            raise ValueError("groups must be an (N,) or (M,) int32 / int64 tensor")
        if groups.device != dev:
            raise ValueError(f"groups must live on the module's device {dev}, got {groups.device}")
        m = groups.numel()
        if positions is None:
            if m != n:
                raise ValueError(f"groups has {m} keys but the module holds {n} items (pass positions to key a subset)")
        else:
            positions = _checked_positions(positions, m, n)
        if m:
            lo, hi = torch.aminmax(groups)
            if int(lo) < -1 or int(hi) >= GROUP_KEY_LIMIT:
                raise ValueError("groups must lie in [-1, 2^31 - 1)")
        with torch.inference_mode():
            self._join_side_streams()
            keys = groups.to(torch.int32)
            if positions is None:
                row = keys.clone()
            else:
                row = torch.full((n,), -1, dtype=torch.int32, device=dev) if self._groups is None else self._groups.clone()
                row.index_copy_(0, positions.to(dev), keys)
            self._groups_are(row)

    def clear_item_groups(self) -> None:
        """No item carries a group key any more: collapse_groups=True is refused again, every other call is what it was."""
        self._groups_are(None)

    def _groups_are(self, row: Optional[torch.Tensor]) -> None:
        self._groups = row
        self._group_rank_cache = None

    def _groups_step(self, e: CorpusEdit, n: int) -> None:
        """The group-key row follows an edit (called by _apply)."""
        if self._groups is None:
            return
        if e.how == CONCATENATED:
            self._groups_are(groups_after_append(self._groups, n, e.n_new))
        elif e.how == CUT_AND_FILLED:
            self._groups_are(groups_after_removal(self._groups, e.n_new, e.positions, e.movers))

    def _dense_group_ranks(self) -> Tuple[torch.Tensor, int]:
        c = self._group_rank_cache
        if c is None:
            with torch.inference_mode():
                c = self._group_rank_cache = group_ranks(self._groups)
        return c

    def _check_collapsible(self, what: str) -> None:
        """The refusal point of the item groups: modules whose candidate generation cannot honour them raise here, before anything is touched."""

    def _take_collapse(self, kwargs: dict) -> int:
        """collapse_groups= and max_per_group= of a call, taken OUT of its kwargs and checked against this module before any launch -> m, the
        results a group may have (collapse_groups=True: 1); 0: the call is not collapsed."""
        collapse = kwargs.pop("collapse_groups", False)
        m = kwargs.pop("max_per_group", None)
        if m is None:
            if not collapse:
                return 0
            m, what = 1, "collapse_groups"
        else:
            what = "max_per_group"
            if isinstance(m, bool) or not isinstance(m, int) or m < 1:
                raise ValueError(f"{type(self).__name__}: max_per_group must be a Python int >= 1, got {m!r}")
            if collapse and m != 1:
                raise ValueError(f"{type(self).__name__}: collapse_groups=True means max_per_group=1, got max_per_group={m} with it (pass one of the two)")
        if any(kwargs.get(name) is not None for name in _FUSION_KWARGS):      # (the two are not built together)
            raise NotImplementedError(f"{type(self).__name__}: {what}= together with query_lims= is not built: collapse the fused ranking on the caller's side, "
                                      "or fuse without groups")
        self._check_collapsible(what)
        if self._groups is None:
            raise ValueError(f"{type(self).__name__}: {what}={'True' if what == 'collapse_groups' else m} on a module without groups (set_item_groups first)")
        return m

    def collapse_stats(self) -> dict:
        """Which path answered the collapsed calls so far: calls, walk_redos (depth doublings), fallbacks (exact group-maxima passes)."""
        return dict(self.__dict__.setdefault("_collapse_stats", {"calls": 0, "walk_redos": 0, "fallbacks": 0}))

    # ---- item vectors: one fp32 vector per item, and diversify=lam on the calls ------------------------------------------
    # State: an owned contiguous (N, E) fp32 table, None until set_item_vectors -- such a module holds nothing extra and a call without
    # diversify= runs none of this.  A call with diversify=lam re-ranks the head of the row's ranking greedily by maximal marginal relevance
    # (rails_topk_mmr): pick after pick, the item with the largest  lam * score - (1 - lam) * max(0, its largest similarity to a picked item).
    # Vectors belong to the POSITION and follow edits as tags do (vectors_after_append / vectors_after_removal); they are not part of state_dict.
    _vectors: Optional[torch.Tensor] = None

    @property
    def item_vectors(self) -> Optional[torch.Tensor]:
        """The (N, E) fp32 item vectors on the module's device, or None while none are set.  The hand-off of the table -- it is not part of
        state_dict; set_item_vectors takes this tensor back as it is."""
        return self._vectors

    def set_item_vectors(self, vectors: torch.Tensor, positions: Optional[torch.Tensor] = None, normalize: bool = False) -> None:
        """One vector per item, the similarity space of diversify=.  vectors: (N, E) fp32 -- every item -- or (M, E) with positions ((M,) int64,
        CPU or device, unique POSITIONS), 1 <= E <= 256, on the module's device; entries finite with magnitude <= 2^60 (no dot product of 256
        terms overflows).  normalize=True divides each row by max(||row||, 1e-12) here, with torch ops; everything downstream reads the stored
        rows.  A call with positions on a module without vectors builds the table with every other row zero; on a module with vectors E must
        be the table's.  ValueError before anything is touched for a wrong shape, dtype, device, value or position (the value check and the
        position check cost one sync each).  The stored table is the module's own: neither argument is aliased."""
        self._check_diversifiable("set_item_vectors")
        n = self.num_items
        dev = self._ids_flat.device
        if not torch.is_tensor(vectors) or vectors.dim() != 2 or vectors.dtype != torch.float32:
            raise ValueError("vectors must be an (N, E) or (M, E) float32 tensor")
        if vectors.device != dev:
            raise ValueError(f"vectors must live on the module's device {dev}, got {vectors.device}")
        m, dim = vectors.shape
        if not 1 <= dim <= E.MMR_MAX_DIM:
            raise ValueError(f"vectors have {dim} entries per item: 1 <= E <= {E.MMR_MAX_DIM}")
        if positions is None:
            if m != n:
                raise ValueError(f"vectors has {m} rows but the module holds {n} items (pass positions to set a subset)")
        else:
            positions = _checked_positions(positions, m, n)
            if self._vectors is not None and self._vectors.shape[1] != dim:
                raise ValueError(f"vectors have {dim} entries per item but the module's table has {self._vectors.shape[1]}")
        with torch.inference_mode():
            if normalize:
                vectors = vectors / torch.linalg.vector_norm(vectors, dim=1, keepdim=True).clamp_min(1e-12)
            if m and not bool((vectors.abs() <= E.MMR_MAX_MAGNITUDE).all()):      # (NaN and inf fail the comparison: the one read-back)
                raise ValueError("vectors must be finite with magnitude <= 2^60")
            self._join_side_streams()
            if positions is None:
                table = vectors.clone(memory_format=torch.contiguous_format)
            else:
                table = torch.zeros((n, dim), dtype=torch.float32, device=dev) if self._vectors is None else self._vectors.clone()
                table.index_copy_(0, positions.to(dev), vectors)
            self._vectors = table

    def clear_item_vectors(self) -> None:
        """No item carries a vector any more: diversify= is refused again, every other call is what it was."""
        self._vectors = None

    def _vectors_step(self, e: CorpusEdit, n: int) -> None:
        """The vector table follows an edit (called by _apply with the movers still where they were)."""
        if self._vectors is None:
            return
        if e.how == CONCATENATED:
            self._vectors = vectors_after_append(self._vectors, n, e.n_new)
        elif e.how == CUT_AND_FILLED:
            self._vectors = vectors_after_removal(self._vectors, e.n_new, e.positions, e.movers)

    def _check_diversifiable(self, what: str) -> None:
        """The refusal point of the item vectors: modules whose candidate generation cannot honour them raise here, before anything is touched."""

    def _take_diversity(self, kwargs: dict) -> Optional[Tuple[float, Optional[int]]]:
        """diversify= and diversity_pool= of a call, taken OUT of its kwargs and checked against this module before any launch -> (lam, the pool
        size asked for or None); None: the call is not diversified."""
        lam = kwargs.pop("diversify", None)
        pool = kwargs.pop("diversity_pool", None)
        name = type(self).__name__
        if lam is None:
            if pool is not None:
                raise ValueError(f"{name}: diversity_pool= without diversify=")
            return None
        if not isinstance(lam, float) or not 0.0 < lam <= 1.0:
            raise ValueError(f"{name}: diversify must be a Python float with 0 < diversify <= 1, got {lam!r}")
        if pool is not None and (isinstance(pool, bool) or not isinstance(pool, int) or pool < 1):
            raise ValueError(f"{name}: diversity_pool must be a Python int >= 1, got {pool!r}")
        if kwargs.get("collapse_groups") or kwargs.get("max_per_group") is not None:
            raise NotImplementedError(f"{name}: diversify= together with collapse_groups= / max_per_group= is not built")
        if any(kwargs.get(given) is not None for given in _FUSION_KWARGS):
            raise NotImplementedError(f"{name}: diversify= together with query_lims= is not built")
        self._check_diversifiable("diversify")
        if self._vectors is None:
            raise ValueError(f"{name}: diversify={lam!r} on a module without vectors (set_item_vectors first)")
        return lam, pool

    def diversity_stats(self) -> dict:
        """How many diversified calls the module has answered: {"calls": n} (each is one ranked-list call and one walk launch)."""
        return dict(self.__dict__.setdefault("_diversity_stats", {"calls": 0}))

    @contextlib.contextmanager
    def _positions_as_ids(self):
        """Inside this block every call of the module returns POSITIONS where it returns ids: the id table is swapped for 0 .. N - 1, so whichever
        arm ranks the call (the proved flow, the dense kernels, the chunks, the sparse masked strategy, a rerank) hands the collapse walk the
        positions it needs without a second form of each arm.  It works because every arm reads self._ids_flat when it launches, and it is
        module state while it lasts: code that runs inside the block must not keep anything derived from the id table -- build the id map
        (only the by-id calls do, never a query call), cache a gathered id tensor, capture a graph -- and a module is driven by one thread at a
        time, as everywhere else in this file (the scratch buffers and pinned words are per module too).  The block holds one query call and
        nothing else: _collapsed_exact's forward, _collapsed_candidates' submit / result."""
        n = self.num_items
        c = self.__dict__.get("_position_ids")
        if c is None or c.numel() != n or c.device != self._ids_flat.device:
            c = self._position_ids = torch.arange(n, dtype=torch.int64, device=self._ids_flat.device)
        saved = self._ids_flat
        self._ids_flat = c
        try:
            yield
        finally:
            self._ids_flat = saved

    HIDDEN_FUSED_MIN_VISIBLE = 0.5    # hidden_scan_route: the visible fraction below which a scan of a module with a hidden set is materialised directly
    TAGGED_FUSED_MIN_GROUPS = 2.0     # tagged_scan_route: the expected finite group maxima, in units of the plan's rank r, below which a tagged scan is materialised directly

    def allowed_tags_route(self, allowed_tags, batch: int) -> str:
        """The route the candidate scans of a call with this allowed_tags= take, e.g. "coarse: fused" or "component: fused, coarse: materialised"
        (tools/item_tags_bench.py records it per cell); "item mask" on the exact modules, which hand the filter to their masked strategies."""
        restr = self._restriction(self._take_allowed_tags({"allowed_tags": allowed_tags}, batch, ()))
        scans = (("component", True, None if getattr(self, "_use_faiss", False) else getattr(self, "_k_per_group", None)),
                 ("coarse", False, getattr(self, "_avg_top_k", None)))
        parts = [f"{name}: " + ("fused" if all(self._scan_route(component, batch, self.num_items, k, restr)) else "materialised")
                 for name, component, k in scans if k is not None]
        return ", ".join(parts) if parts else "item mask"

    def _scan_route(self, component: bool, batch: int, n: int, k: int, restr: Optional[Restriction]) -> Tuple[bool, bool]:
        """The one route decision of the candidate scans (the component scan, or the coarse one) -> (eligible, allowed).  eligible: the sizes are
        the fused scan's (fused_*_min_items; the fused coarse selection holds K' <= 4096).  allowed: the restriction's rule, hidden_scan_route or
        tagged_scan_route, expects the fused scan's threshold to hold.  Fused iff both; the component scan sizes its slices by `allowed` alone."""
        eligible = n >= self.fused_component_min_items if component else (n >= self.fused_coarse_min_items and k <= 4096)
        return eligible, restr is None or restr.allows_fused(self, component, batch, n, k)

    def _scan_plan(self, component: bool, batch: int, n: int, k: int) -> Optional[Tuple[int, int, int, int]]:
        """E.scan_plan of one scan's call as it will be sliced under a tag filter (host arithmetic, memoised per size)."""
        if component:
            spec = self._bind().spec
            pq, px = spec.query_dot_product_groups, spec.item_dot_product_groups
            b = min(batch, max(1, E.TAGGED_COMPONENT_ROWS // pq))
            key = (b * pq * px, n, k, b * pq)
        else:
            key = (min(batch, 128), n, k, 0)
        memo = self.__dict__.setdefault("_scan_plans", {})
        if key not in memo:
            if len(memo) > 64:
                memo.clear()
            memo[key] = E.scan_plan(*key)
        return memo[key]

    def _check_taggable(self, what: str) -> None:
        """The refusal point of allowed_tags=: modules whose candidate generation cannot honour it raise here, before any launch."""

    def _tag_state(self):
        stamp = (self._tags_version, self._hidden_version, self.num_items)
        c = self._tag_cache
        if c is None or c[0] != stamp:
            eff = self._tags if self._visible is None else E.item_tags_effective(self._tags, self._visible, self.num_items)
            c = self._tag_cache = (stamp, eff, {}, {})
        return c

    def _take_allowed_tags(self, kwargs: dict, batch: int, ks: Tuple[int, ...]) -> Optional[E.TagFilter]:
        """allowed_tags= of a call, taken OUT of its kwargs: None, or the resolved E.TagFilter -- validated against this module, the batch and the
        sizes `ks` the call selects (avg_top_k, k_per_group, k) before any launch.  An E.TagFilter given (a call handing its own filter on) is
        returned as it is while the module's tags, hidden set and size are the ones it was resolved against."""
        a = kwargs.pop("allowed_tags", None)
        if a is None:
            return None
        self._check_taggable("allowed_tags")
        if self._tags is None:
            raise ValueError(f"{type(self).__name__}: allowed_tags= on a module without tags (set_item_tags first)")
        stamp, eff, counts, filters = self._tag_state()
        if isinstance(a, E.TagFilter) and a.stamp == stamp and a.rows in (1, batch):
            filt = a
        else:
            words = a.words if isinstance(a, E.TagFilter) else parse_allowed_tags(a, batch)
            filt = filters.get(words)
            if filt is None:
                new = [w for w in dict.fromkeys(words) if w not in counts]
                if new:      # one launch and one read-back per call that brings new words
                    counts.update(zip(new, E.item_tags_counts(eff, new)))
                if len(filters) >= self.TAG_FILTERS_KEPT:
                    filters.clear()
                filt = filters[words] = E.TagFilter(eff, words, tuple(counts[w] for w in words), stamp=stamp)
        for k in ks:
            if k is not None and k > filt.kept_min:
                raise RuntimeError(f"selected index k out of range (k={k}, n={filt.kept_min})")
        return filt

    def _apply(self, e: CorpusEdit) -> None:
        """The one edit flow.  The ids about to be overwritten or moved are read BEFORE the write; what was decided from the corpus size is
        forgotten BEFORE the engine for n_new items is asked for; resize comes before refresh; a removal without holes refreshes nothing."""
        with torch.inference_mode():
            self._join_side_streams()
            eng = self._bind()
            n, pos, rows, ids = self.num_items, e.positions, e.rows, e.ids
            gone = None if e.gone is None else self._ids_at(e.gone)
            if e.how == CUT_AND_FILLED:
                rows, ids = self._rows_at(e.movers), self._ids_at(e.movers)
                if ids is not None:       # (the movers' ids are erased too, and come back at the holes)
                    gone = torch.cat([gone, ids])
            self._write_table(e, pos, rows)
            if e.how == CUT_AND_FILLED:
                self._item_ids, self._ids_flat = _remove_ids(self._item_ids, self._ids_flat, e.n_new, pos, e.movers)
            elif e.how == CONCATENATED:
                self._item_ids, self._ids_flat = _append_ids(self._item_ids, self._ids_flat, ids)
            elif ids is not None:
                _write_ids(self._item_ids, self._ids_flat, pos, ids)
            if ids is not None:
                self._id_map_step(gone, ids, pos)
            self._visibility_step(e, n)
            self._tags_step(e, n)
            self._groups_step(e, n)
            self._vectors_step(e, n)
            held, resize = self._held_buffers(), e.n_new != n
            if resize:
                self._forget_corpus_choices()
            if not resize or self._engine_for_bind() is eng:
                self._upd_source = None
                for h in held:
                    if resize and h.resize is not None and h.held(self, eng):
                        h.resize(self, eng, e.n_new)
                for h in held:
                    if pos.numel() and h.refresh is not None and h.held(self, eng):
                        h.refresh(self, eng, pos, rows)
                self._upd_source = None
            else:       # another engine for n_new items: its buffers are built from the table, as at construction
                for h in held:
                    if h.drop is not None:
                        h.drop(self)
            if resize:
                self._bind()
            for h in held:
                if h.settle is not None and h.held(self, eng):
                    h.settle(self, eng)

    def _update_rows_arg(self, item_embeddings: torch.Tensor, item_ids: Optional[torch.Tensor], appending: bool = False):
        dim, dtype = self._row_format()
        return _rows_arg(item_embeddings, item_ids, dim, dtype, self._ids_flat.device, self._item_ids.dtype, appending)

    def _check_updatable(self, what: str, n_left: Optional[int] = None) -> None:
        """The single refusal point: modules whose state cannot follow an in-place change (or a removal down to n_left items) raise here,
        before anything is touched."""

    def _write_table(self, e: CorpusEdit, pos: torch.Tensor, rows: torch.Tensor) -> None:
        """The raw item table as the edit leaves it (a module that keeps none: nothing)."""

    def _join_side_streams(self) -> None:
        pass

    def _bind(self):
        return None

    _engine_for_bind = _bind       # (no choice of engines)

    def _forget_corpus_choices(self) -> None:
        """What the module decided from the corpus size, to be decided again (subclasses that decide something)."""


class MoLTopKModule(_CorpusEdits, TopKModule):
    """Common state of the MoL top-k modules (reference mol_top_k.py:29-81): borrows `item_embeddings`
    (1, N, D) and `item_ids` (1, N); owns the packed index."""

    def __init__(self, mol_module: MoLSimilarity, item_embeddings: torch.Tensor, item_ids: torch.Tensor) -> None:
        super().__init__()
        self._mol_module: MoLSimilarity = mol_module
        if item_embeddings.dim() != 3 or item_embeddings.shape[0] != 1:
            raise ValueError(f"item_embeddings must be (1, N, D), got {tuple(item_embeddings.shape)}")
        self._item_embeddings: torch.Tensor = item_embeddings
        self._item_ids: torch.Tensor = item_ids
        self._ids_flat: torch.Tensor = item_ids.reshape(-1).to(device=item_embeddings.device, dtype=torch.int64).contiguous()
        self._engine: Optional[E.MolEngine] = None
        self._call_eng: Optional[E.MolEngine] = None
        self._index: Optional[E.MolIndex] = None
        self._scratch: Dict[tuple, torch.Tensor] = {}   # internal buffers recycled across calls (never returned)
        self._no_fused = False        # True: the fused scans are off (the redo of a call whose scan verdict failed; tests)
        self._flag_free: list = []    # pinned verdict words ready for reuse (_pinned_word)
        self._bind()

    def _buf(self, tag: str, numel: int, dtype: torch.dtype) -> torch.Tensor:
        key = (tag, numel, dtype)
        t = self._scratch.get(key)
        if t is None:
            if len(self._scratch) > 16:
                self._scratch.clear()
            t = torch.empty(numel, dtype=dtype, device=self._item_embeddings.device)
            self._scratch[key] = t
        return t

    @property
    def mol_module(self) -> MoLSimilarity:
        return self._mol_module

    @property
    def num_items(self) -> int:
        return self._item_embeddings.shape[1]

    def _bind(self) -> E.MolEngine:
        if self._call_eng is not None:   # inside one_bind(): the parameters were checked when the call began
            return self._call_eng
        eng = self._engine_for_bind()
        if eng is not self._engine:  # first use, or the module's parameters changed
            self._engine = eng
            self._index = eng.build_index(self._item_embeddings[0])
        return eng

    def _engine_for_bind(self) -> E.MolEngine:
        return self._mol_module.engine()

    @contextlib.contextmanager
    def one_bind(self):
        """One look at the module's parameters for a whole call: `engine()` compares 2 x 48 (pointer, version) pairs, ~10 us, and a
        two-pass call asks for the engine six times -- host time that sits between the batches of a plain loop."""
        outer = self._call_eng
        if outer is None:
            self._call_eng = self._bind()
        try:
            yield
        finally:
            self._call_eng = outer

    # ---- in-place corpus changes (_CorpusEdits): the raw table, and the buffers every MoL module holds ------------------------------------------
    # Per-item index values depend on the item's own row alone (one workgroup computes 32 items with one accumulator per item), so an update
    # recomputes the changed items and nothing else: O(M) bytes per held buffer.  Whole passes over the corpus: the int8 pre-filter (one scale
    # for the whole table: rebuilt from the updated coarse table) and the proved mode's max |gi| (metadata of the bound); a resize also copies
    # what it resizes.
    def _row_format(self) -> Tuple[int, torch.dtype]:
        return self._item_embeddings.shape[2], self._item_embeddings.dtype

    def _rows_at(self, pos: torch.Tensor) -> torch.Tensor:
        return self._item_embeddings[0].index_select(0, pos)

    def _write_table(self, e: CorpusEdit, pos: torch.Tensor, rows: torch.Tensor) -> None:
        if e.how == IN_PLACE:
            self._item_embeddings[0].index_copy_(0, pos, rows)
        elif e.how == CONCATENATED:
            self._item_embeddings = torch.cat([self._item_embeddings, rows.unsqueeze(0)], dim=1)
        else:
            table = self._item_embeddings[:, : e.n_new].clone()
            table[0].index_copy_(0, pos, rows)
            self._item_embeddings = table

    def _join_side_streams(self) -> None:
        if not self._item_embeddings.is_cuda:
            return
        cur = torch.cuda.current_stream(self._item_embeddings.device)
        for side in list(getattr(self, "_side_streams", None) or ()) + [getattr(self, "_audit_stream", None)]:
            if side is not None:
                cur.wait_stream(side)

    def _table_source(self, eng, emb: torch.Tensor):
        """engine.update_source, once per edit (the coarse table, the component table and the IVF lists share it)."""
        if self._upd_source is None:
            self._upd_source = eng.update_source(self._index, emb)
        return self._upd_source

    def _rows_held(self, eng) -> bool:
        c = self._rows_cache
        return c is not None and c[0] is eng and c[1] is self._index

    def _rows_resize(self, eng, n_new: int) -> None:
        rows = self._rows_cache[2]      # None: refused for its size -- decided again at the next rerank, as for a fresh module
        self._rows_cache = None if rows is None else (eng, self._index, E.resized(rows, eng.lib.rails_mol_index_rows_floats(E.C.byref(eng.shape), n_new)))

    def _rows_refresh(self, eng, pos: torch.Tensor, emb: torch.Tensor) -> None:
        if self._rows_cache[2] is not None:
            eng.update_index_rows(self._index, self._rows_cache[2], pos)

    def _rows_drop(self) -> None:
        self._rows_cache = None

    _HELD = (
        Held(("_index",), lambda tk, eng: True, lambda tk, eng, n: eng.resize_index(tk._index, n),
             lambda tk, eng, pos, emb: eng.update_index(tk._index, pos, emb), None),       # (never dropped: _bind builds the new engine's over it)
        Held(("_rows_cache",), _rows_held, _rows_resize, _rows_refresh, _rows_drop),
        Held(("_scratch",), lambda tk, eng: True, lambda tk, eng, n: tk._scratch.clear(), None, lambda tk: tk._scratch.clear()),   # recycled buffers sized by N
    )

    def all_logits(self, query_embeddings: torch.Tensor, **kwargs) -> torch.Tensor:
        """(B, N) fp32 MoL logits against the whole corpus."""
        refuse_collapse_groups(self, kwargs, "all_logits")
        refuse_diversity(self, kwargs, "all_logits")
        refuse_item_mask(self, kwargs)
        tags = self._take_allowed_tags(kwargs, query_embeddings.size(0), ())
        logits = self._raw_logits(query_embeddings, **kwargs)
        restr = self._restriction(tags)      # the columns a row may not return -- disallowed by allowed_tags=, or hidden -- hold -inf
        return logits if restr is None else restr.mask(logits)

    def _raw_logits(self, query_embeddings: torch.Tensor, **kwargs) -> torch.Tensor:
        eng = self._bind()
        qpack, _, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"))
        return eng.score_dense(qpack, query_embeddings.size(0), self._index)

    def _all_logits_scratch(self, query_embeddings: torch.Tensor, _eng=None, _index=None, _tag: str = "qpack", _private: bool = False, **kwargs) -> torch.Tensor:
        """Same, into recycled internal buffers (the result is consumed by the top-k before the next call).  _eng / _index: another engine
        over its own index (the fp32 companion of the exact modes; its pack has its own `_tag`); _private: fresh buffers (the audit's side
        stream must not share the scratch of the call it checks)."""
        eng = _eng if _eng is not None else self._bind()
        index = _index if _index is not None else self._index
        B = query_embeddings.size(0)
        pack = logits = None
        if not _private:
            pack = self._buf(_tag, eng._fn("query_pack_floats")(E.C.byref(eng.shape), B), torch.float32)
            logits = self._buf("logits", B * index.n_items, torch.float32).view(B, index.n_items)
        qpack, _, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"), out=pack)
        return eng.score_dense(qpack, B, index, out=logits)

    def _dense_topk(self, query_embeddings: torch.Tensor, k: int, seen=None, sorted: bool = True, _private: bool = False, _mask=None, **kwargs):
        """Dense fp32 logits into scratch (_all_logits_scratch and its options) + exact top-k -> (scores, ids); with seen = (invalid_ids, k_out)
        the seen-id filter runs inside the selection launch (rails_topk_filtered) -> (ids (B, k_out), scores (B, k_out)).  _mask: the logits
        of the items outside this ItemMask are set to -inf before the selection (the dense strategy of a masked call)."""
        logits = self._all_logits_scratch(query_embeddings, _private=_private, **kwargs)
        if _mask is not None:
            E.scores_mask(logits, _mask)
        ws = None if _private else self._buf("topk_ws", E._lib.load().rails_topk_workspace_bytes(logits.shape[0], logits.shape[1], k), torch.uint8)
        if seen is not None:
            ids, scores = E.topk_filtered(logits, k, self._ids_flat, seen[0], seen[1], workspace=ws)
            return ids, scores.to(query_embeddings.dtype)
        scores, ids = E.topk(logits, k, ids=self._ids_flat, sorted=sorted, workspace=ws)
        return scores.to(query_embeddings.dtype), ids

    @staticmethod
    def _score_positions(eng, qpack: torch.Tensor, batch: int, index, rows, positions: torch.Tensor) -> torch.Tensor:
        """(B, K) full-MoL logits of per-row candidates given as VALID positions of `index`, whichever way is cheapest -- same bits each way.
        fp32 engines read the candidates in place (rails_mol_score_indexed: no gathered copy, one launch; the same bits as gather +
        score_candidates): from `rows`, the row-major copy of the index, where there is one (a candidate's bytes in whole cache lines: half
        the time of the tile-packed reads), else from the tile-packed index (any K: the kernel masks the ragged last tile); the f16 builds,
        which have no indexed instantiation, gather a per-row index of the candidates first (the 256-logit team kernel).
        rows: the copy, None, or a function of the engine that yields one of the two (asked only where the copy can be read)."""
        K = positions.shape[1]
        if eng.score_indexed_supported(batch, K):
            if callable(rows):
                rows = rows(eng)
            if rows is not None:
                return eng.score_indexed_rows(qpack, batch, rows, index.n_items, positions)
            return eng.score_indexed(qpack, batch, index, positions)
        cand, kp = eng.gather_index(index, positions)
        return eng.score_candidates(qpack, batch, cand, kp)[:, :K]

    def _score_at(self, eng, qpack: torch.Tensor, batch: int, positions: torch.Tensor) -> torch.Tensor:
        """_score_positions over this module's own index (the rerank of the approximate algorithms); the row-major copy is built at the
        first call that can read it."""
        return self._score_positions(eng, qpack, batch, self._index, self._index_rows, positions)

    # ---- the hooks of score_of / explain_of ------------------------------------------------------------------------------
    _PAIR_ITEM_MASK = False      # (all_logits refuses item_mask= on the candidate modules; MoLBruteForceTopK takes it)

    def _pair_engine(self):
        """The engine whose dense pass all_logits returns: this module's own."""
        return self._bind()

    def _pair_scorer(self):
        """(_pair_engine, its index, the row-major copy or a function yielding it)."""
        return self._pair_engine(), self._index, self._index_rows

    def _refuse_pair_engine(self, what: str) -> None:
        """What the engine decides, still before any launch of the call: the split-f16 precisions (refuse_pair_precision) and, for explain_of
        on a fused-shape module, a MoL shape outside the generic route's envelope (answered by the library without a device; inside it the
        companion engine is built here, once)."""
        eng = self._pair_engine()
        refuse_pair_precision(self, eng, what)
        if what.startswith("explain_of") and eng.route != "generic":
            try:
                self._mol_module.explain_engine()
            except NotImplementedError as e:
                raise explain_outside_envelope(self, e) from None

    def _pair_scores(self, query_embeddings: torch.Tensor, positions: torch.Tensor, kwargs: dict) -> torch.Tensor:
        eng, index, rows = self._pair_scorer()
        B = query_embeddings.size(0)
        qpack, _, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"))
        if eng.route == "generic":      # (candidate-capable or not: the generic index is read in place)
            return eng.score_at_generic(qpack, B, index, positions)
        return self._score_positions(eng, qpack, B, index, rows, positions)

    def _pair_explained(self, query_embeddings: torch.Tensor, positions: torch.Tensor, kwargs: dict):
        """-> (component_logits (B, T, L), weights (B, T, L)); the explaining launch's own logits are dropped (on the generic route they are
        score_of's bits, which the tests hold the engine's explain_indexed to).  A module on the generic route reads its
        own index in place; a fused-shape module gathers the B T raw rows, builds a per-row generic index of them with its companion engine
        (MoLSimilarity.explain_engine) and launches once -- nothing of size N."""
        eng, index, _ = self._pair_scorer()
        B, T = positions.shape
        user_ids = kwargs.get("user_ids")
        if eng.route == "generic":
            qpack, _, _ = eng.query_pack(query_embeddings, user_ids)
            _, cl, pi = eng.explain_indexed(qpack, B, index, positions)
            return cl, pi
        comp = self._mol_module.explain_engine()      # (inside the envelope: _refuse_pair_engine has asked)
        cand = comp.build_index(self._rows_at(positions.reshape(-1)))
        qpack, _, _ = comp.query_pack(query_embeddings, user_ids)
        _, cl, pi = comp.explain_candidates(qpack, B, cand, T)
        return cl, pi

    RERANK_ROWS_COPY_MAX_BYTES = 8 << 30     # fp32 indexes up to this size get a row-major copy for the candidate re-scoring of the rerank paths (0: never)
    _rows_cache = None

    def _index_rows(self, eng) -> Optional[torch.Tensor]:
        """The row-major copy of this module's fp32 index (rails_mol_index_rows_build), built at the first rerank; None where it does not apply
        (f16 index formats, indexes beyond RERANK_ROWS_COPY_MAX_BYTES -- a 125 M-item shard -- or too little free memory)."""
        c = self._rows_cache
        if c is not None and c[0] is eng and c[1] is self._index:
            return c[2]
        rows = None
        need = self._index.buf.numel() * 4
        # (the generic index is row-major itself: no copy, score_indexed reads it in place)
        if getattr(eng, "precision", None) == "fp32" and getattr(eng, "route", None) != "generic" and self._index.buf.is_cuda and 0 < need <= self.RERANK_ROWS_COPY_MAX_BYTES:
            free, _ = torch.cuda.mem_get_info(self._index.buf.device)
            if free > 2 * need:
                rows = eng.build_index_rows(self._index)
        self._rows_cache = (eng, self._index, rows)
        return rows


def refuse_pair_precision(module, eng, what: str) -> None:
    """score_of / explain_of on an engine of a split-f16 precision, by the class's name and the precision, before any
    launch.  score_of runs on 'f16x3': _score_positions' gather route returns the dense pass's bits there (the same three-product kernels on
    a gathered index; verified on the device, tests/test_score_of_gpu.py).  It is refused where the dense pass runs the one-product kernels
    ('f16x1', 'f16-exact'): the gathered index is scored by the three-product ones, every entry differs, and nothing weaker than all_logits'
    bits is returned.  explain_of needs the fp32 kernels, which alone write the mixture out."""
    if eng.precision == "fp32" or (not what.startswith("explain_of") and eng.dense_precision == "f16x3"):
        return
    why = ("the mixture is written out by the fp32 kernels only" if what.startswith("explain_of") else
           "the dense pass runs the one-product split-f16 kernels and given positions are scored by the three-product ones: not all_logits' bits")
    raise NotImplementedError(f"{type(module).__name__}.{what}: precision={eng.dense_precision!r} -- {why}; a module of precision 'fp32' (or an "
                              "exact mode of MoLBruteForceTopK, whose scores are its fp32 companion's) takes the call")


def explain_outside_envelope(module, err: Exception) -> NotImplementedError:
    """explain_of on a MoL shape the generic scoring route does not take (a pair gate without hidden layer, L > 256, d > 256, H > 512): the
    refusal, by the class's name, with the route's own words."""
    return NotImplementedError(f"{type(module).__name__}.explain_of: the mixture is written out by the shape-generic scoring kernel, and this MoL "
                               f"shape lies outside its envelope ({err})")


def refuse_item_mask(module, kwargs, why: str = "its candidates are generated inside the fused scans, and masking their result afterwards is not the "
                                               "contract of a masked call") -> None:
    """item_mask= is built on the exact modules only: every other module refuses it by name, before any launch.
    query_lims= (section 3.20) is built in the same places and refused in the same places, by its own name."""
    refuse_query_fusion(module, kwargs)
    if kwargs.get("item_mask") is not None:
        name = type(module).__name__ + (" (IVF, use_faiss=True)" if getattr(module, "_use_faiss", False) else "")
        raise NotImplementedError(f"{name} takes no item_mask: {why}; MoLBruteForceTopK and MIPSBruteForceTopK take it")


def mask_strategy(kept_max: int, n_items: int, sparse_max: int, factor: int, positions_scorable: bool) -> str:
    """How a masked call runs, from the largest row count of the mask alone -- pure host arithmetic:
      "sparse"  the kept positions are the candidates: scored in place, ranked by rails_topk_candidates; nothing outside the mask is scored.
                Where at most `sparse_max` items are kept per row (never more than the 16 384 candidates one ranking launch takes), the kept
                items are at most 1 / `factor` of the corpus, and the engine can score positions in place (`positions_scorable`: the fused
                fp32 kernels -- not the generic route, not the split-f16 builds);
      "dense"   everything is scored as without a mask, the cleared entries of the (B, N) matrix are set to -inf, the usual selection follows."""
    if positions_scorable and 1 <= kept_max <= min(int(sparse_max), 16384) and factor * kept_max <= n_items:
        return "sparse"
    return "dense"


def _refuse_generic_route(mol_module: MoLSimilarity, what: str) -> None:
    """The approximate algorithms need the coarse / component tables and the in-place candidate re-scoring, which the generic scoring
    route has on a candidate-capable engine only (MoLSimilarity.generic_candidates = True): refuse otherwise, at
    construction, before any build -- and, on a candidate-capable engine, what the route still lacks, by name."""
    eng = mol_module.engine()
    if eng.route != "generic":
        return
    if not eng.candidates:
        raise NotImplementedError(f"{what} is not built on the generic scoring route (this MoL shape has no fused scoring kernel); "
                                  "MoLBruteForceTopK runs it.  Setting generic_candidates = True on the MoLSimilarity opts in to the "
                                  "two-pass algorithms on this route")
    if eng.table_width == 0:
        raise NotImplementedError(f"{what} on the generic scoring route takes dot_product_dimension <= 128 (the widest bf16 candidate scan), "
                                  f"got d = {eng.spec.dot_product_dimension}; MoLBruteForceTopK runs it")


def refuse_generic_candidates(mol_module: MoLSimilarity, what: str, instead: str) -> None:
    """What the two-pass algorithms still lack on the generic scoring route, a candidate-capable engine included:
    refused by name, before any build or launch."""
    if mol_module.engine().route == "generic":
        raise NotImplementedError(f"{what} is not built on the generic scoring route (generic_candidates = True covers the single-device "
                                  f"exhaustive algorithms); {instead}")


class BoundPolicy(NamedTuple):
    """How one MoLBruteForceTopK bounds |first pass - fp32| under one set of parameters: decided once per engine (MoLBruteForceTopK.bound_policy,
    a pure function of the pair-gate weights, the shape, the policy corpus size and the library's shape queries), read by everything else.
      base          the module's own engine the record belongs to (new parameters -> a new engine -> a new record)
      proved        the default mode's choice for `base`: bind the split-f16 engine (_proved_applies) or stay dense; None: not decided
      terms         f16x3_bound.first_pass_bound's breakdown, {"eps": inf} where a guard of the bound fails; None: not evaluated (yet)
      kind          "eps"    one a-priori eps for every pair, where it is at most PROVED_MAX_EPS;
                    "upper"  a per-pair bound, quadratic in the pair's largest |cross logit|, added to the first-pass logit by the kernel itself
                             (f16x3_bound.upper_bound_poly, rails_mol_score_dense_upper): where one eps is too coarse, or the corpus is small,
                             and the shape has the kernel;
                    None     neither (infinite bound, or too coarse without the kernel): the module runs the dense fp32 kernels
      poly          (ub2, ub1, ub0) when the engine's form is per-pair, else None
      any_poly      the same polynomial when the shape has the UPPER build at all: calls for PER_PAIR_MIN_K results or more take it
      eps_of_c      upper_bound_poly's samples of eps against the largest |cross logit| (reported by rigorous_eps)
      eps           what the verdict compares with (with_guard): 0.0 under per-pair bounds, inf when the bound is; None: no a-priori bound in
                    use (the one-product first pass, the dense modes)
      guard_limit   GATE_GUARD / max |gi| over the corpus: the bound's one data-dependent hypothesis, checked per batch by the verdict"""

    base: object = None
    proved: Optional[bool] = None
    terms: Optional[Dict[str, float]] = None
    kind: Optional[str] = None
    poly: Optional[Tuple[float, float, float]] = None
    any_poly: Optional[Tuple[float, float, float]] = None
    eps_of_c: Optional[Dict[str, float]] = None
    eps: Optional[float] = None
    guard_limit: Optional[float] = None

    def with_guard(self, gi_abs_max: float) -> "BoundPolicy":
        """The record with the verdict's eps and the guard limit filled in, given max |gi| over the corpus.  eps: the a-priori bound rounded UP
        to a float32 (the verdict compares in fp32: gap = fl(e_k - m) > eps, one rounding of relative 2^-24 on a gap of at most 2 / tau --
        covered by the 2^-16 relative slack added here); 0.0 where the first pass writes upper bounds of the fp32 logits (the verdict is
        e_k > m itself -- strict: ties with an outsider are redone); inf when an item gate is not finite."""
        from . import f16x3_bound as FB

        if self.poly is not None:
            eps = 0.0
        else:
            eps32 = torch.tensor(float(self.terms["eps"]) * (1.0 + 2.0 ** -16), dtype=torch.float32)
            eps = float(torch.nextafter(eps32, torch.tensor(float("inf"))))
        limit = min(FB.GATE_GUARD / gi_abs_max, 3.0e38) if gi_abs_max > 0.0 else 3.0e38
        return self._replace(eps=eps if math.isfinite(gi_abs_max) else math.inf, guard_limit=limit)


class MoLBruteForceTopK(MoLTopKModule):
    def __init__(self, mol_module: MoLSimilarity, item_embeddings: torch.Tensor, item_ids: torch.Tensor, exact_mode: Optional[str] = None,
                 bound_kind_items: Optional[int] = None) -> None:
        """exact_mode (not in the reference's signature, rails/indexing/mol_top_k.py:84-97): "proved" | "dense", default EXACT_MODE.
        bound_kind_items: the corpus size the proved flow's size-dependent choices are made for (the item-sharded wrapper passes the shard size
        every rank computes alike); default: this module's own corpus."""
        self.bound_kind_items = bound_kind_items
        if exact_mode not in (None, "proved", "dense"):
            raise ValueError(f"exact_mode must be 'proved' or 'dense', got {exact_mode!r}")
        self._index32: Optional[E.MolIndex] = None          # precision "f16x3-exact": dense fp32 index (candidate gather, fallback)
        self._index32_engine = None
        self.keep_dense_fp32_index: Optional[bool] = self.KEEP_DENSE_FP32_INDEX
        self.rescore_stats = {"calls": 0, "fallbacks": 0, "audited": 0, "mismatches": 0}
        self._probe_pool: Optional[torch.Tensor] = None
        self._ok_host: Optional[torch.Tensor] = None
        self._recent: list = []       # verdicts of the last speculative calls
        self._calib_engine = None
        self._err_seen = 0.0          # largest |first pass - fp32| ever seen on re-scored candidates and probes (reset only with the engine)
        self._risk_pool: Optional[torch.Tensor] = None   # positions of the highest-norm items (probed every call)
        self._risk_rows: Optional[torch.Tensor] = None   # the probe rows the rotation over them produces, precomputed
        self.audit_every: int = int(self.AUDIT_EVERY)    # > 0: every n-th speculative call is also run on the dense fp32 path and compared
        self._audit_stream = None
        self._debug_first_pass_bias = None
        self._verdict_state: Optional[torch.Tensor] = None
        self._state_pending = None
        self._pad_scale = 1           # candidate margin multiplier, doubled when a verification fails
        self._state_direct = False    # True: the verdict state reaches the host through the finish kernel's own stores (no copy, no event)
        self._pause_left = 0
        self.exact_mode: str = exact_mode or self.EXACT_MODE
        self._policy = BoundPolicy()  # the bound on |first pass - fp32| for the current parameters (one record per engine)
        self._gate_guard_limit: Optional[float] = None
        self._ok_event = None
        self._probe_n = -1
        super().__init__(mol_module=mol_module, item_embeddings=item_embeddings, item_ids=item_ids)

    # ---- which arithmetic an exact top-k runs in -----------------------------------------------------------------------------------
    # A module whose MoL precision is the default (fp32) returns the fp32 kernels' bits.  "proved" (the default): the split-f16 kernels
    # pick the candidates, the fp32 kernels re-score them, and the a-priori bound of rails_amd/f16x3_bound.py on |first pass - fp32|
    # proves per call, on the device, that nothing outside the candidates can belong to the result -- the dense fp32 path's output bit for
    # bit at ~2.3 x its speed; a call that cannot be proved (crowded scores, a guard of the bound violated) is redone on the dense fp32
    # kernels behind the verdict.  "dense": the fp32 kernels over the whole corpus, always.  RAILS_EXACT_MODE overrides the default.
    # The proved mode needs both index formats resident (2 x the fp32 index bytes); corpora where that does not fit, corpora below
    # SPECULATE_MIN_ITEMS and modules whose bound is infinite (see the guards in f16x3_bound.py) run "dense".
    EXACT_MODE = __import__("os").environ.get("RAILS_EXACT_MODE", "proved")
    if EXACT_MODE not in ("proved", "dense"):
        raise ValueError(f"RAILS_EXACT_MODE must be 'proved' or 'dense', got {EXACT_MODE!r}")
    PROVED_MAX_EPS = 2.0          # a module whose a-priori bound exceeds this many logit units is not worth a second index: the items within eps of the
                                  # k-th score run into the tens of thousands (16x16x64: eps = 2.9; profiles/r05_proved_candidate_census.json)
    PROVED_MAX_EPS_PER_PAIR = 10.0 # ... up to this eps (at the a-priori |cl| <= 1/tau) the bound is applied PER PAIR instead: the pairs of a corpus sit at a third of
                                  # 1/tau and the bound is quadratic in it (_bound_kind "upper": 16x16x64 at random init, 3.0; trained weights of the other shapes).
                                  # Round 6 (tools/r06_scale_probe.py, amzn-books, pair-gate weights x s): x 3 (eps 8.6) proves 44 / 45 calls at 3 904 candidates,
                                  # 2.78 ms per batch against 6.4 dense; x 4 (eps 15.2) proves none even at 16 384 candidates -- hence 10, not 8
    PAD_ONE_EPS = (824, 3)        # candidates beyond k: max(floor, per_k * k) (doubled after a failed verdict) -- under one eps ...
    PAD_PER_PAIR = (1848, 1)      # ... and under per-pair upper bounds (sized for a 12.5 M-item shard of 16x16x64: 730-900 items can reach the 200-th score;
                                  # amzn-books at k' = 2 561: 5 152 candidates prove every call where one eps needs 10 272)
    # Corpora up to PER_PAIR_MAX_ITEMS items take the per-pair form whatever their one eps is: their first pass is short, so the UPPER build's extra
    # work costs microseconds, and the tighter bound proves with half the candidates (kc = 512 at k' = 200: a cheaper selection, half the re-scoring).
    # amzn-books shape, proved step per-pair / one eps: 20 k items 0.173 / 0.195 ms, 32 k 0.219 / 0.255, 65 k 0.350 / 0.368, 131 k 0.590 / 0.603
    # (695 k: 2.80 / 2.75 -- one eps wins there); ML-20M (27 278 items), which one eps cannot prove at all: 0.179 ms against 0.239 dense.
    PER_PAIR_MAX_ITEMS = 196608
    PAD_PER_PAIR_SMALL = (312, 1)
    bound_kind_items: Optional[int] = None
    # The default mode speculates where the first pass saves more than the verification costs (~70 us of launches): from B x N = 2^18 (query, item)
    # pairs on.  Same-box steps, proved flow / dense fp32 kernels (tools/r06_probe_p.sh): amzn-books 695 762 items B = 1 0.285 / 0.322 ms, 400 k items
    # B = 1 0.198 / 0.211, 200 k B = 1 0.131 / 0.125, B = 2 0.145 / 0.184; ML-20M (27 278 items) B = 2 0.100 / 0.057, B = 8 0.113 / 0.094, B = 16 0.113 / 0.146.
    PROVED_MIN_BATCH = 1
    PROVED_MIN_PAIRS = 1 << 18

    @classmethod
    def speculation_pays(cls, batch: int, n_items: int) -> bool:
        return batch >= cls.PROVED_MIN_BATCH and batch * n_items >= cls.PROVED_MIN_PAIRS

    def _engine_for_bind(self) -> E.MolEngine:
        mol = self._mol_module
        base = mol.engine()
        pol = self._policy
        if pol.base is not base:      # new parameters (or another precision): nothing decided, nothing evaluated yet
            pol = self._policy = BoundPolicy(base=base)
        if self.exact_mode != "proved" or base.precision != "fp32" or base.exact is not None or base.route == "generic":
            return base       # (the generic scoring route has the dense fp32 pass only)
        if pol.proved is None:
            ok = self._proved_applies(base)
            pol = self._policy = self._policy._replace(proved=ok)
        return mol.engine("f16x3-exact", _params_as_checked=True) if pol.proved else base     # (the second look at the same parameters in the same breath)

    def _proved_applies(self, base: E.MolEngine) -> bool:
        spec, N = base.spec, self._item_embeddings.shape[1]
        if N < self.SPECULATE_MIN_ITEMS or N > 0xFFFFFFFF or not self._item_embeddings.is_cuda:
            return False
        if not base.lib.rails_mol_shape_supported(E.C.byref(spec.to_c("f16x3"))):
            return False
        if self._evaluated(spec, base.lib).kind is None:
            return False
        from . import arith_check

        if not arith_check.device_ok(self._item_embeddings.device):     # the bound's hypotheses about the part, re-measured on THIS device (once per process)
            return False
        if self.keep_dense_fp32_index is False:
            return False
        need = base.lib.rails_mol_index_floats(E.C.byref(base.shape), N) * 4
        free, _ = torch.cuda.mem_get_info(self._item_embeddings.device)
        held = self._index.buf.numel() * 4 if self._index is not None else 0     # a rebind: the old index is dropped first
        return free + held > 2 * need + min(32 * N * 4, self.MAX_LOGIT_BYTES) + (1 << 30)

    def _evaluated(self, spec, lib) -> BoundPolicy:
        """The current record with the bound evaluated: f16x3_bound runs here, once per engine (float64 work on weight-sized tensors)."""
        pol = self._policy
        if pol.terms is None:
            pol = self._policy = self.bound_policy(self._mol_module, spec, lib, self._policy_items())._replace(base=pol.base, proved=pol.proved)
        return pol

    @classmethod
    def bound_policy(cls, mol_module, spec, lib, policy_items: int) -> BoundPolicy:
        """rails_amd/f16x3_bound.py for this module's pair-gate weights and the form the proved flow takes from it (BoundPolicy.kind): a pure
        function of the weights, the shape, `policy_items` and the library's query for the UPPER build -- no GPU."""
        from . import f16x3_bound as FB

        terms, args = {"eps": math.inf}, None
        if (spec.dot_product_l2_norm and spec.gating_combination_type == "glu_silu" and spec.gating_qi_hidden_dim > 0
                and spec.gating_query_fn and spec.gating_item_fn):
            lin = [m for m in mol_module._gating_fn._qi_partial_module.modules() if isinstance(m, torch.nn.Linear)]
            if len(lin) == 2:
                b1 = lin[0].bias if lin[0].bias is not None else torch.zeros(lin[0].out_features)
                b2 = lin[1].bias if lin[1].bias is not None else torch.zeros(lin[1].out_features)
                args = (lin[0].weight, b1, lin[1].weight, b2, spec.temperature, spec.dot_product_dimension, spec.query_dot_product_groups,
                        spec.item_dot_product_groups)
                terms = FB.first_pass_bound(*args)
        eps = float(terms.get("eps", math.inf))
        per_pair_ok = eps <= cls.PROVED_MAX_EPS_PER_PAIR and bool(lib.rails_mol_score_dense_upper_supported(E.C.byref(spec.to_c("f16x3"))))
        if per_pair_ok and (eps > cls.PROVED_MAX_EPS or policy_items <= cls.PER_PAIR_MAX_ITEMS):
            kind = "upper"
        else:
            kind = "eps" if eps <= cls.PROVED_MAX_EPS else None
        poly = any_poly = eps_of_c = None
        if kind is not None and per_pair_ok:
            res = FB.upper_bound_poly(*args)
            any_poly, eps_of_c = res["poly"], res.get("eps_of_c")
            poly = any_poly if kind == "upper" else None
        return BoundPolicy(terms=terms, kind=kind, poly=poly, any_poly=any_poly, eps_of_c=eps_of_c)

    def _bound_from_weights(self, spec) -> Dict[str, float]:
        """The bound's term dictionary for this module's pair-gate weights; {"eps": inf} where a guard of the bound fails."""
        return self._evaluated(spec, E._lib.load()).terms

    def _policy_items(self) -> int:
        """The corpus size the size-dependent choices of the proved flow are made for: this module's own, or -- set by the item-sharded wrapper,
        the same on every rank -- the shard size (ranks must agree on the form of the bound)."""
        return int(self.bound_kind_items or self._item_embeddings.shape[1])

    @classmethod
    def candidate_count(cls, k: int, per_pair: bool, policy_items: int, pad_scale: int = 1, world: Optional[int] = None,
                        n_local: Optional[int] = None, single: bool = False) -> int:
        """How many candidates per query a speculative call re-scores: k + a margin (PAD_ONE_EPS / PAD_PER_PAIR / PAD_PER_PAIR_SMALL by the form
        of the bound and the policy corpus size, times `pad_scale`, which failed verdicts double), rounded up to whole tiles, at most 16 384.
          world, n_local   the item-sharded proof: the candidates within eps of the GLOBAL k-th score spread evenly over the shards, so each of
                           `world` ranks takes its share + 4 sqrt(share) + 32, at most its `n_local` items (rails_amd/sharded.py)
          single           the one-product first pass, which has no a-priori bound (the monitored flow; per_pair and policy_items do not
                           apply): k / 2 beyond k, at least 128; up to k = 384 at most 512 -- rails_topk's two-launch path ends there,
                           beyond it a selection costs five reads of the logits"""
        tile = E.TILE_ITEMS
        if single:
            kc = (k + max(128, k // 2) * pad_scale + tile - 1) // tile * tile
            return min(kc, 512) if k <= 384 else kc
        floor, per_k = cls.PAD_ONE_EPS if not per_pair else cls.PAD_PER_PAIR_SMALL if policy_items <= cls.PER_PAIR_MAX_ITEMS else cls.PAD_PER_PAIR
        total = k + max(floor, per_k * k) * pad_scale
        if world is None:
            return min((total + tile - 1) // tile * tile, 16384)
        if n_local is None:
            raise ValueError("candidate_count: world needs n_local")
        per = -(-total // world)
        kc = per + int(4.0 * per ** 0.5) + 32
        return max(1, min((kc + tile - 1) // tile * tile, 16384, n_local))

    def shard_candidate_count(self, k: int, pad_scale: int, world: int) -> int:
        """candidate_count for this module as one of `world` shards (the form of the bound and the margins follow the policy corpus size
        every rank computes alike)."""
        return self.candidate_count(k, self._policy.poly is not None, self._policy_items(), pad_scale, world=world, n_local=self.num_items)

    def _upper_poly(self, k: Optional[int] = None) -> Optional[Tuple[float, float, float]]:
        """(ub2, ub1, ub0) when the bound engine's first pass writes per-pair UPPER BOUNDS of the fp32 logits (BoundPolicy.kind "upper"), else None.
        With k: also for a CALL of an engine whose form is the one eps, when the call wants PER_PAIR_MIN_K results or more -- the candidates a
        large k needs under one eps (k' = 2 561 on amzn-books: 10 272) cost more to re-score and sort than the UPPER build adds to the first pass
        (3.19 -> 2.9 ms per batch); the verdict of such a call runs with eps = 0 on the same state."""
        pol = self._policy
        if pol.poly is not None or k is None or k < self.PER_PAIR_MIN_K:
            return pol.poly
        return pol.any_poly

    PER_PAIR_MIN_K = 1024         # calls for at least this many results take per-pair bounds whatever the engine's form (see _upper_poly)

    def all_logits(self, query_embeddings: torch.Tensor, **kwargs) -> torch.Tensor:
        """(B, N) fp32 MoL logits against the whole corpus -- of the module's OWN precision (the proved mode's internal split-f16
        engine is not the module's precision: its fp32 companion answers).  item_mask=: the columns outside the mask hold -inf.
        query_lims=: the fused matrix, (U, N)."""
        refuse_collapse_groups(self, kwargs, "all_logits")
        refuse_diversity(self, kwargs, "all_logits")
        if (fusion := self._resolve_fusion(kwargs, query_embeddings, "all_logits")) is not None:
            return self._fused_all_logits(query_embeddings, fusion, kwargs)
        eng = self._bind()
        mask = self._take_item_mask(kwargs, query_embeddings.size(0), None)
        if eng.exact is not None and self._mol_module.engine() is not eng:
            ex = eng.exact
            qpack, _, _ = ex.query_pack(query_embeddings, kwargs.get("user_ids"))
            logits = ex.score_dense(qpack, query_embeddings.size(0), self._dense_fp32_index())
        else:
            logits = self._raw_logits(query_embeddings, **kwargs)
        return logits if mask is None else E.scores_mask(logits, mask)      # (a hidden set is part of `mask`: _take_item_mask)

    def _rank_scores(self, query_embeddings: torch.Tensor, **kwargs) -> torch.Tensor:
        """all_logits' scores -- the module's OWN precision: the fp32 companion in the exact modes -- unmasked, in the recycled logits buffer."""
        eng = self._bind()
        if eng.exact is not None and self._mol_module.engine() is not eng:
            return self._all_logits_scratch(query_embeddings, _eng=eng.exact, _index=self._dense_fp32_index(), _tag="qpack32", **kwargs)
        return self._all_logits_scratch(query_embeddings, **kwargs)

    _PAIR_ITEM_MASK = True

    def _pair_engine(self):
        """all_logits' engine: the fp32 companion in the exact modes, the module's own otherwise."""
        eng = self._bind()
        return eng.exact if eng.exact is not None and self._mol_module.engine() is not eng else eng

    def _pair_scorer(self):
        """... and its index: the dense fp32 index in the exact modes (built at first use and kept, as all_logits builds it)."""
        eng = self._pair_engine()
        if eng is not self._bind():
            return eng, self._dense_fp32_index(), self._rows32
        return eng, self._index, self._index_rows

    # ---- item_mask=: a call restricted to a subset of the corpus ------------------------------------------------------
    # The call equals the same call on a module freshly constructed from the kept rows and their ids, bit for bit (scores are per item and
    # position-independent, ties break by position, and the kept items keep their order).  Two strategies, chosen on the host from the mask's
    # largest row count (mask_strategy): SPARSE scores the kept positions alone; DENSE scores everything as without a mask and sets the cleared
    # entries of the (B, N) matrix to -inf before the selection -- on every arm: _dense_topk, the corpus chunks, the proved flow's first pass
    # and its redo.  Rows whose k-th kept score is -inf or NaN tie with cleared entries: the contract is stated for finite scores.
    MASK_SPARSE_MAX = 16384       # rows keeping at most this many items may take the sparse strategy (never more than rails_topk_candidates ranks)
    MASK_SPARSE_FACTOR = 4        # ... when they keep at most 1 / this of the corpus.  Measured (profiles/item_mask.json, B = 32, k' = 261): sparse / dense
                                  # step time 0.44 at N = 32 768 and 0.65 at N = 65 536 with N / 4 kept, 1.02 with N / 3, 1.22 with N / 2: the crossover
                                  # lies at a third of the corpus, 4 is the smallest whole factor at which sparse wins
    MASK_PROVED_MIN_KEPT = 16384  # the proved flow runs masked where every row keeps MORE than this: at least as many as a call has candidates
                                  # (candidate_count's cap), so every selected candidate is a kept item; other masks take the dense fp32 kernels

    def _mask_scorer(self, eng):
        """(engine, index, row-major copy or a function yielding it) that scores corpus positions in place in the module's own fp32 arithmetic --
        _score_positions' arguments -- or None where there is none: the generic route unless its engine is candidate-capable (the index is
        then its own row-major copy), the split-f16 precisions (no indexed instantiation), an exact mode without its resident fp32 index."""
        if eng.route == "generic":
            return (eng, self._index, lambda e: self._index.buf) if eng.candidates else None
        if eng.exact is not None:
            if self._index32 is None or self._index32_engine is not eng.exact:
                return None
            return eng.exact, self._index32, self._rows32
        if eng.precision != "fp32":
            return None
        return eng, self._index, self._index_rows

    def _masked(self, eng, mask: E.ItemMask, count: bool = True) -> str:
        """The strategy of this masked call; counted in rescore_stats (stats()["masked_sparse_calls" / "masked_dense_calls"])."""
        how = mask_strategy(mask.kept_max, self.num_items, self.MASK_SPARSE_MAX, self.MASK_SPARSE_FACTOR, self._mask_scorer(eng) is not None)
        if count:
            key = f"masked_{how}_calls"
            self.rescore_stats[key] = self.rescore_stats.get(key, 0) + 1
        return how

    def _forward_sparse(self, eng, query_embeddings: torch.Tensor, k: int, mask: E.ItemMask, seen, **kwargs):
        """The sparse strategy: the kept positions of every row are its candidates (ItemMask.positions, ascending: the order of a fresh module
        of the kept rows), scored in place by the fp32 kernels (_score_positions: the dense kernels' bits) and ranked by rails_topk_candidates
        (score desc, candidate column asc) -> (scores, ids); seen = (invalid_ids, k_out): the seen-id filter inside that launch where the
        sizes fit, behind it otherwise -> (ids, scores).  A ragged per-row mask pads short rows with position 0: those slots are set to -inf."""
        ex, index, rows = self._mask_scorer(eng)
        B = query_embeddings.size(0)
        pos = mask.positions_for(B)
        K = pos.shape[1]
        qpack, _, _ = ex.query_pack(query_embeddings, kwargs.get("user_ids"))
        if mask.ragged():
            copy = (rows(ex) if callable(rows) else rows) if ex.score_indexed_supported(B, K) else None
            if copy is not None:      # the tiles past a row's count are skipped
                scores = ex.score_indexed_rows(qpack, B, copy, index.n_items, pos, counts=mask.counts)
            else:
                scores = self._score_positions(ex, qpack, B, index, None, pos)
            E.scores_mask(scores, mask.slot_mask())
        else:
            scores = self._score_positions(ex, qpack, B, index, rows, pos)
        if seen is not None:
            invalid_ids, k_out = seen
            if E.topk_candidates_filterable(K, k, invalid_ids.shape[1], k_out):
                ids, s = E.topk_candidates_filtered(scores, k, pos, self._ids_flat, invalid_ids, k_out)
            else:
                s, ids = E.topk_candidates(scores, k, pos, self._ids_flat)
                ids, s = E.filter_seen_ids(ids, s, invalid_ids, k_out)
            return ids, s.to(query_embeddings.dtype)
        s, ids = E.topk_candidates(scores, k, pos, self._ids_flat)
        return s.to(query_embeddings.dtype), ids

    def forward(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """item_mask= (an engine.ItemMask, or a bool tensor (N,) / (B, N) packed for this call): only items inside the mask are returned.
        collapse_groups=True: at most one item per group of set_item_groups.  query_lims= (section 3.20): one result row
        per segment of query rows.  diversify=lam (section 3.21; diversity_pool=D): the head of the ranking re-ranked by maximal marginal relevance
        against set_item_vectors -- k columns in PICK order, each with the item's own score, so a row is not monotone."""
        if _asks_diversity(kwargs) and (div := self._take_diversity(kwargs)) is not None:      # (results in pick order)
            return _diversified_exact(self, query_embeddings, k, None, kwargs, div)
        if (fusion := self._resolve_fusion(kwargs, query_embeddings, "forward")) is not None:
            ids, scores = self._fused_topk("forward", query_embeddings, k, None, fusion, kwargs, sorted)
            return scores.to(query_embeddings.dtype), ids
        if _asks_collapse(kwargs) and (m := self._take_collapse(kwargs)):
            return _collapsed_exact(self, query_embeddings, k, None, kwargs, m)
        eng = self._bind()
        mask = self._take_item_mask(kwargs, query_embeddings.size(0), k)
        if mask is not None:
            if self._masked(eng, mask) == "sparse":
                return self._forward_sparse(eng, query_embeddings, k, mask, None, **kwargs)
            kwargs["_mask"] = mask
        if eng.exact is not None:
            return self._forward_rescored(query_embeddings, k, **kwargs)
        B, N = query_embeddings.size(0), self._index.n_items
        if B * N * 4 > self.MAX_LOGIT_BYTES and k <= self.CHUNK_ITEMS:
            return self._forward_chunked(query_embeddings, k, **kwargs)
        return self._dense_topk(query_embeddings, k, sorted=sorted, **kwargs)

    def forward_filtered(self, query_embeddings: torch.Tensor, k_prime: int, invalid_ids: torch.Tensor, k: int, **kwargs):
        """CandidateIndex.get_top_k_outputs' body for this module: top-k' + id map + seen-id filter with the filter fused into the final
        selection launch (rails_topk_filtered on the dense logits) -> (top_k_ids (B, k), top_k_scores (B, k)),
        or None when the sizes / the precision route are outside the fused path (the caller then composes forward +
        filter_seen_ids: same bits).  collapse_groups=True never returns None: the seen ids go to the collapse walk (a filter behind the
        collapse would drop a group whose best item is seen instead of promoting its next member).  Nor does query_lims= (section 3.20)."""
        if _asks_diversity(kwargs) and (div := self._take_diversity(kwargs)) is not None:      # (never None: the seen ids go to the walk)
            scores, ids = _diversified_exact(self, query_embeddings, k, invalid_ids, kwargs, div)
            return ids, scores
        if (fusion := self._resolve_fusion(kwargs, query_embeddings, "forward_filtered")) is not None:
            ids, scores = self._fused_topk("forward_filtered", query_embeddings, k_prime, (invalid_ids, k), fusion, kwargs)
            return ids, scores.to(query_embeddings.dtype)
        if _asks_collapse(kwargs) and (m := self._take_collapse(kwargs)):
            scores, ids = _collapsed_exact(self, query_embeddings, k, invalid_ids, kwargs, m)
            return ids, scores
        eng = self._bind()
        B, N = query_embeddings.size(0), self._index.n_items
        mask = self._take_item_mask(kwargs, B, k_prime)
        if mask is not None and k <= k_prime and self._masked(eng, mask, count=False) == "sparse":
            self._masked(eng, mask)
            return self._forward_sparse(eng, query_embeddings, k_prime, mask, (invalid_ids, k), **kwargs)
        if B * N * 4 > self.MAX_LOGIT_BYTES or not E.topk_filter_fusable(N, k_prime, invalid_ids.shape[1], k):
            return None
        if mask is not None:
            self._masked(eng, mask)
            kwargs["_mask"] = mask
        ex = eng.exact
        if ex is None:
            return self._dense_topk(query_embeddings, k_prime, seen=(invalid_ids, k), **kwargs)
        if (not self.speculation_pays(B, N) and self._mol_module.engine() is not eng and eng.dense_precision == "f16x3"
                and self._index32 is not None and self._index32_engine is ex):
            # the default mode's small calls (speculation_pays) run the dense fp32 kernels (_forward_rescored): keep the filter fused into their
            # selection launch as the plain fp32 module does
            return self._dense_topk(query_embeddings, k_prime, seen=(invalid_ids, k), _eng=ex, _index=self._index32, _tag="qpack32", **kwargs)
        if not (eng.dense_precision == "f16x3" and k <= k_prime <= N):
            return None
        # the proved flow: the filter runs inside its finish launch (and inside the redo's selection)
        r = self._forward_rescored(query_embeddings, k_prime, _seen=(invalid_ids, k), **kwargs)
        if r[0] == "filtered":
            return r[1], r[2]
        return E.filter_seen_ids(r[1], r[0], invalid_ids, k)

    def _own_score_chunks(self, query_embeddings: torch.Tensor, mask: Optional[E.ItemMask], **kwargs):
        """all_logits' scores -- the module's OWN precision, -inf outside `mask` -- as (first item, (B, n) matrix) pieces: the whole corpus
        where the logit policy lets it be materialised, CHUNK_ITEMS at a time otherwise (the collapse fallback consumes each before the next)."""
        eng = self._bind()
        if eng.exact is not None and self._mol_module.engine() is not eng:
            eng, index = eng.exact, self._dense_fp32_index()
        else:
            index = self._index
        B, N = query_embeddings.size(0), index.n_items
        C = N if B * N * 4 <= self.MAX_LOGIT_BYTES else min(N, self.CHUNK_ITEMS)
        qpack, _, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"))
        for lo in range(0, N, C):
            logits = eng.score_dense(qpack, B, index if C == N else index.items(lo, min(N, lo + C)))
            if mask is not None:
                E.scores_mask(logits, mask, first_item=lo)
            yield lo, logits

    MAX_LOGIT_BYTES = 4 << 30      # larger (B, N) logit matrices are never materialised: the corpus is scored in chunks
    CHUNK_ITEMS = 1 << 23          # 8 Mi items per chunk (a multiple of the tile): 1 GiB of logits at B = 32

    def _forward_chunked(self, query_embeddings: torch.Tensor, k: int, _engine=None, _index=None, _mask=None, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """Exact top-k of a corpus whose (B, N) logits would not fit comfortably (a 125 M-item shard at B = 32 is 16 GB): score
        CHUNK_ITEMS at a time into one recycled buffer, keep each chunk's top-k, merge.  Same result as the one-pass path bit for
        bit: chunks are position ranges in order and every list is sorted (score desc, position asc), so the final top-k over
        the chunk-major concatenation breaks ties by position as well (the item-sharded merge's argument, rails_amd/sharded.py).
        _mask: every chunk's logits are masked at its offset (a chunk may keep fewer than k items: its list then ends in -inf entries, which
        the merge ranks below every kept item of the other chunks)."""
        eng = _engine if _engine is not None else self._bind()
        index = _index if _index is not None else self._index
        B, N, C = query_embeddings.size(0), index.n_items, self.CHUNK_ITEMS
        n_q = eng._fn("query_pack_floats")(E.C.byref(eng.shape), B)
        qpack, _, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"), out=self._buf("qpack", n_q, torch.float32))
        buf = self._buf("logits_chunk", B * min(C, N), torch.float32)
        ws = self._buf("topk_ws", E._lib.load().rails_topk_workspace_bytes(B, min(C, N), min(k, C)), torch.uint8)
        part_s, part_p = [], []
        for lo in range(0, N, C):
            n = min(C, N - lo)
            logits = eng.score_dense(qpack, B, index.items(lo, lo + n), out=buf[: B * n].view(B, n))
            if _mask is not None:
                E.scores_mask(logits, _mask, first_item=lo)
            s, p = E.topk(logits, min(k, n), workspace=ws)
            part_s.append(s)
            part_p.append(p + lo)
        scores, pos = E.topk(torch.cat(part_s, 1), k, ids=torch.cat(part_p, 1))
        return scores.to(query_embeddings.dtype), self._ids_flat[pos]

    # ---- precision "f16x3-exact": speculate with the f16x3 kernels, verify in fp32 ---------------------------------------
    KEEP_DENSE_FP32_INDEX: Optional[bool] = None   # None: when memory allows; True / False: always / never (candidates' rows are rebuilt)
    RESCORE_EPS_PER_INV_TEMPERATURE = 5e-5   # eps = this / temperature: 1e-3 on logits in [-20, 20], 30 x the largest
                                             # |f16x3 - fp32| seen over 22 M pairs (profiles/r02_bench.json fast_path)
    # first pass on the one-product f16 kernels ("f16-exact"): |s16 - s32| up to 4.3e-2 on amzn-books, 1.7e-2 on ML-20M
    # (tools/single_f16_probe.py) -> default eps = 0.15 on logits in [-20, 20], twice the candidate margin of the f16x3 first pass
    RESCORE_EPS_PER_INV_TEMPERATURE_F16X1 = 7.5e-3

    def _forward_rescored(self, query_embeddings: torch.Tensor, k: int, _seen=None, _mask=None, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """The router of the exact modes: the fp32 brute-force result -- same scores, same ids, same tie order -- by the dense fp32 kernels, the
        proved flow (_forward_proved) or the monitored flow (_forward_monitored), a slice of the batch at a time under the 4 GiB logit policy.
        _mask (the dense strategy of a masked call) travels with every arm; the proved flow takes it where every row keeps more than
        MASK_PROVED_MIN_KEPT items, the dense fp32 kernels otherwise (and instead of the monitored flow)."""
        if _mask is not None:
            kwargs["_mask"] = _mask
        eng = self._bind()
        self._absorb_state()
        B, N = query_embeddings.size(0), self._index.n_items
        if k > N:
            raise RuntimeError(f"selected index k out of range (k={k}, n={N})")
        # The bound on |first pass - fp32|: A PRIORI for the f16x3 first pass (rails_amd/f16x3_bound.py: the call is then PROVED to
        # return the dense fp32 result whenever its verdict clears); monitored and empirical for the one-product first pass, whose a-priori
        # bound is vacuous (eps None).  A module whose a-priori bound is infinite (a guard fails) does not speculate.
        eps = self._policy.eps
        upper = None
        if eps is not None:
            if not math.isfinite(eps):
                self.rescore_stats["unprovable_calls"] = self.rescore_stats.get("unprovable_calls", 0) + 1
                return self._forward_fp32_dense(query_embeddings, k, **kwargs)
            if not self.speculation_pays(B, N) and self._mol_module.engine() is not eng:
                # too few (query, item) pairs for the first pass to save what the verification costs (PROVED_MIN_PAIRS) -- the default mode takes
                # the dense kernels there (an explicit "f16x3-exact" precision keeps speculating)
                return self._forward_fp32_dense(query_embeddings, k, **kwargs)
            upper = self._upper_poly(k)       # per-pair upper bounds instead of one eps (then the verdict's eps is 0)
            if upper is not None and self._policy.poly is None:
                eps = 0.0                     # a large-k call of an engine whose own form is the one eps
        # candidates: every item within eps of the k-th score must be among them.  amzn-books, eps = 0.9-1.0: 470-680 items at k = 200,
        # 6 000-7 500 at k = 2 561 (128 queries; profiles/r05_proved_candidate_census.json); rails_topk costs the same 80-90 us from
        # 544 to 1 536 candidates per row of 700 k scores, so the margin starts generous.  A failed verdict doubles it
        # (per-pair upper bounds on a 12.5 M-item shard of 16x16x64: 730-900 items can reach the 200-th score; tools/r05_c4_census.py)
        kc = self.candidate_count(k, upper is not None, self._policy_items(), self._pad_scale, single=eps is None)
        if kc >= N or k == 0 or kc > 16384 or k + E.TILE_ITEMS > kc or N > 0xFFFFFFFF or N < self.SPECULATE_MIN_ITEMS or self._speculation_paused():
            return self._forward_fp32_dense(query_embeddings, k, **kwargs)
        if B * N * 4 > self.MAX_LOGIT_BYTES:      # the 4 GiB logit policy: the speculative pass wants the whole (B, N) first-pass matrix
            rows = self.MAX_LOGIT_BYTES // (N * 4)
            if rows >= 1:                         # ... of a slice of the batch at a time (per-row payloads are sliced with it)
                parts = []
                for b0 in range(0, B, rows):
                    kw = {key: (v[b0 : b0 + rows] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B else v) for key, v in kwargs.items()}
                    if _mask is not None:
                        kw["_mask"] = _mask.rows_slice(b0, b0 + rows)
                    parts.append(self._forward_rescored(query_embeddings[b0 : b0 + rows], k, **kw))
                return torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)
            return self._forward_fp32_dense(query_embeddings, k, **kwargs)   # one row is too long: fp32, in corpus chunks
        proved = eps is not None and self._index32 is not None and self._index32_engine is eng.exact
        if _mask is not None and not (proved and _mask.kept_min > self.MASK_PROVED_MIN_KEPT):
            return self._forward_fp32_dense(query_embeddings, k, **kwargs)
        if proved:
            return self._forward_proved(query_embeddings, k, kc, eps, upper, _seen, **kwargs)
        return self._forward_monitored(query_embeddings, k, kc, eps, upper, **kwargs)

    def _first_pass(self, eng, qpack16: torch.Tensor, B: int, upper, bias: bool = True) -> torch.Tensor:
        """The first pass over the whole index into the recycled (B, N) buffer: upper bounds of the fp32 logits with `upper`, else the
        first-pass logits themselves.  bias: apply the tests' planted error (speculate_for_shard does not)."""
        N = self._index.n_items
        s16 = self._buf("logits", B * N, torch.float32).view(B, N)
        hook = self._first_pass_hook        # measurement only (bench.py: events around the dominant launch, on its stream)
        if hook is not None:
            hook(0)
        if upper is not None:
            eng.score_dense_upper(qpack16, B, self._index, upper, out=s16)
        else:
            eng.score_dense(qpack16, B, self._index, out=s16)
        if hook is not None:
            hook(1)
        if bias and self._debug_first_pass_bias is not None:   # tests only: (positions, delta) -- the first pass is made to under-score these items
            s16[:, self._debug_first_pass_bias[0]] -= self._debug_first_pass_bias[1]
        return s16

    def _query_packs(self, eng, query_embeddings: torch.Tensor, **kwargs):
        """One prologue writes the query pack in both formats: f16 hi/lo for the first pass, fp32 for the re-scoring."""
        n_q = eng.lib.rails_mol_query_pack_floats(E.C.byref(eng.shape), query_embeddings.size(0))
        return eng.query_pack_both(query_embeddings, kwargs.get("user_ids"), self._buf("qpack", n_q, torch.float32), self._buf("qpack32", n_q, torch.float32))

    def _forward_monitored(self, query_embeddings: torch.Tensor, k: int, kc: int, eps_proved: Optional[float], upper, **kwargs):
        """The older speculate / verify flow: what serves the one-product first pass ("f16-exact", eps_proved None) and the f16x3 first pass
        without a resident fp32 index.
          1. first-pass logits s16 over the whole index; the top kc of them are the candidates, m = the smallest candidate's s16.  Every
             other item has s16 <= m.
          2. the candidates are scored by the fp32 kernel from the dense fp32 index (kept next to the first-pass one when memory allows;
             otherwise their raw rows go through the fp32 index build): e32, their exact fp32 logits (the same arithmetic per (query, item)
             pair as the dense fp32 path, hence the same bits).
          3. rails_rescore_select: top-k of e32 by (score desc, corpus position asc) -- the dense path's total order.
        The result is the dense fp32 top-k iff no item outside the candidates can reach the k-th exact score e_k, i.e. iff
        e_k > m + eps where |s16 - s32| <= eps.  Step 3 returns e_k - m per row and the largest |e32 - s16| over the row's candidates, and,
        for the one-product pass, over 64 more items: 32 drawn at random from the whole corpus and 32 of the highest-norm ones; its eps is
        the calibrated default or SAFETY x the largest such error this module has seen, whichever is larger.  A row that does not clear eps
        -> the call is redone on the dense fp32 kernels (and later calls take more candidates)."""
        eng = self._engine
        ex = eng.exact
        B, N = query_embeddings.size(0), self._index.n_items
        single = eps_proved is None
        qpack16, qpack32 = self._query_packs(eng, query_embeddings, **kwargs)
        s16 = self._first_pass(eng, qpack16, B, upper)
        ws = self._buf("topk_ws", E._lib.load().rails_topk_workspace_bytes(B, N, kc), torch.uint8)
        c16, pos = E.topk(s16, kc, workspace=ws)
        # two more tiles per query of probes (random + highest-norm items), re-scored too, so that the MONITORED bound |s16 - s32| <= eps is
        # watched outside the candidates as well (the a-priori bound needs no watching: the candidates' own errors are still compared
        # with it, and one above it is reported as a violation of the arithmetic model)
        if single:
            pos = torch.cat([pos, *self._probes(B, N)], dim=1)
        if self._index32 is not None:
            # read the candidates in place from the fp32 index: one launch less and no gathered copy.  A candidate's 1 280 bytes are 80
            # pieces of 16 bytes in the tile-packed index, each in its own cache line, whoever fetches them -- the gather kernel paid
            # that amplification AND wrote and re-read the copy.  Measured with the GEMM1 lookahead of the independent-wave kernels in
            # (amzn-books, `f16-exact`): k' = 200  B = 8 / 32 / 128: 0.501 / 1.59 / 5.81 -> 0.494 / 1.59 / 5.76 ms; k' = 2561: 0.631 /
            # 1.93 / 6.88 -> 0.610 / 1.835 / 6.55 ms (docs/HISTORY.md section 3.3)
            e32 = self._score_positions(ex, qpack32, B, self._index32, self._rows32, pos)
        else:     # no resident fp32 index: the candidates' raw rows go through the fp32 index build
            cand = ex.build_index(self._item_embeddings[0].index_select(0, pos.reshape(-1)))
            e32 = ex.score_candidates(qpack32, B, cand, pos.shape[1])
        scores, ids, _, stats = E.rescore_select(e32, c16, pos, self._ids_flat, N, k, approx_dense=s16, one_sided=upper is not None)
        self.rescore_stats["calls"] += 1
        self.rescore_stats["kc"] = kc
        if single:
            # The bound eps on |s16 - s32|: never below the calibrated default, and SAFETY x the largest error this module has seen on its
            # candidates and probes (this call included) -- a model whose weights make the first pass coarser widens its own margin
            # instead of failing the monitor forever.  The row passes when its k-th exact score clears the best non-candidate by eps.
            default, safety = self.RESCORE_EPS_PER_INV_TEMPERATURE_F16X1 / eng.spec.temperature, self.SAFETY_F16X1
            guard, guard_limit = None, 0.0
        else:
            # eps = the a-priori bound (safety 1: an observed error above it -- a violation of the model -- still widens the margin); the
            # one data-dependent hypothesis of the bound, max |gq'| max |gi| <= gate_guard, is checked on the batch's gq' rows
            default, safety = eps_proved, 1.0
            guard, guard_limit = eng.gate_rows(qpack32, B), self._gate_guard_limit
        if self._index32 is not None:
            # (the one-product first pass only: with a resident fp32 index the f16x3 pass takes the proved flow)
            # Verdict and fallback ON THE DEVICE: rails_rescore_verdict folds the row stats into the calibration state and writes the
            # REDO flag; the dense fp32 pass and its top-k are enqueued behind it under that flag as their launch predicate (no-ops
            # unless the verification failed) and overwrite (scores, ids).  The host never waits; it looks at a snapshot of the
            # state when the NEXT call starts (statistics, candidate margin, pause logic).
            state = self._state()
            E.rescore_verdict(stats, state, default, safety, guard, guard_limit)
            redo = state.view(torch.int32)[1:2]
            l32 = ex.score_dense(qpack32, B, self._index32, out=self._buf("logits", B * N, torch.float32).view(B, N), run_if=redo)
            E.topk(l32, k, ids=self._ids_flat, workspace=ws, out=(scores, ids), run_if=redo)
            self._state_host.copy_(state, non_blocking=True)
            self._state_event.record()
            self._state_pending = (k, kc, upper is not None)
            self._state_direct = False
        else:
            # no resident fp32 index: the host reads the verdict (one event spin per call)
            err, gap = self._read_stats(stats)
            if err == err and err != float("inf"):
                self._err_seen = max(err, self._err_seen)   # never forgotten: a rare outlier keeps the margin wide until the engine changes
            eps = max(default, safety * self._err_seen)
            good = err == err and err != float("inf") and gap > eps
            if guard is not None and good:      # the bound's data-dependent guard, on the host in this (index-less) variant
                gmax = float(guard.abs().max())
                self.rescore_stats["guard_max"] = max(self.rescore_stats.get("guard_max", 0.0), gmax)
                good = gmax <= guard_limit
            if not single:
                self._count_proved(1 if good else 0)
            self.rescore_stats["eps"] = eps
            self._note_verdict(good, k, kc, upper is not None)
            if not good:
                return self._forward_fp32_dense(query_embeddings, k, **kwargs)
        if self.audit_every > 0 and self.rescore_stats["calls"] % self.audit_every == 0:
            self._audit(query_embeddings, k, scores, ids, **kwargs)
        return scores.to(query_embeddings.dtype), ids

    # ---- the proved flow with the fused tail (round 6) ----------------------------------------------------------------------------
    # first pass -> rails_candidates_select (threshold selection: one histogram + one compaction launch, one launch for short rows) ->
    # fp32 re-scoring of the counted candidates -> rails_candidates_finish (sort, top-k, verdict, seen-id filter, calibration state written
    # to the device AND straight into pinned host memory) -> the dense redo under the verdict's launch predicate: 8-9 launches where the
    # exact-kc selection + separate verdict / filter / state copy took 19 (amzn-books B = 32: 0.19 -> ~0.1 ms behind the first pass).
    _cand = None          # {(B, cap): [workspace, positions, first-pass scores, fp32 scores]}
    _cand_dirty = False

    def _cand_buffers(self, B: int, cap: int):
        """(workspace, positions, first-pass scores, fp32 scores) of a (batch, candidate cap): zero-initialised once (the workspace must be; stale
        positions past a row's count must be valid), kept for the last few shapes (callers that alternate batch sizes do not reallocate)."""
        pool = self._cand
        if pool is None:
            pool = self._cand = {}
        c = pool.get((B, cap))
        if c is None:
            if len(pool) >= 4:
                pool.pop(next(iter(pool)))
            dev = self._item_embeddings.device
            c = pool[(B, cap)] = [E.candidates_workspace(B, dev), torch.zeros((B, cap), dtype=torch.int64, device=dev),
                                  torch.zeros((B, cap), dtype=torch.float32, device=dev), torch.zeros((B, cap), dtype=torch.float32, device=dev)]
        elif self._cand_dirty:       # an exception between select and finish left counts / histograms behind
            for v in pool.values():
                v[0].zero_()
        self._cand_dirty = False
        return c[0], c[1], c[2], c[3]

    def _score_range(self, upper) -> Tuple[float, float]:
        """The a-priori range of the first-pass logits (the histogram's bins): a softmax mixture of cross logits in [-1/tau, 1/tau] (l2-normalised
        components: a guard of the bound) plus, for the UPPER builds, the per-pair bound at the largest |cross logit|.  Scores outside are clamped
        into the end bins -- any monotone bin function is valid, the range only sets the resolution."""
        c = 1.02 / float(self._engine.spec.temperature)
        hi = c + ((upper[0] * c + upper[1]) * c + upper[2] if upper is not None else 0.0)
        return -c, hi

    def _select_and_rescore(self, ex, qpack32: torch.Tensor, B: int, s16: torch.Tensor, cap: int, upper):
        """Threshold selection of at most `cap` candidates per row by first-pass score + their fp32 logits
        -> (workspace with the rows' counts, positions, first-pass scores, fp32 scores)."""
        ws, pos, a16, e32 = self._cand_buffers(B, cap)
        self._cand_dirty = True
        lo, hi = self._score_range(upper)
        E.candidates_select(s16, cap, lo, hi, ws, pos, a16)
        if self._rows32 is not None and ex.score_indexed_supported(B, cap):
            ex.score_indexed_rows(qpack32, B, self._rows32, s16.shape[1], pos, counts=ws, out=e32)
        else:      # every slot (the slots past a row's count hold earlier candidates: valid positions, ignored by the finish)
            e32 = self._score_positions(ex, qpack32, B, self._index32, self._rows32, pos)
        return ws, pos, a16, e32

    def _forward_proved(self, query_embeddings: torch.Tensor, k: int, kc: int, eps_proved: float, upper, seen, _mask=None, **kwargs):
        """_mask (every row keeps more than MASK_PROVED_MIN_KEPT >= kc items): the first-pass matrix -- scores, or upper bounds -- is masked
        before the selection, so every candidate is a kept item (the cleared entries sit in the lowest bin, below the threshold bin), m and
        the verdict are those of the kept corpus and the proof is that of a module built from the kept rows; the redo's dense logits are
        masked under the redo's own launch predicate."""
        eng = self._engine
        ex = eng.exact
        B, N = query_embeddings.size(0), self._index.n_items
        sp = eng.spec
        qpack16, qpack32 = self._query_packs(eng, query_embeddings, **kwargs)
        s16 = self._first_pass(eng, qpack16, B, upper)
        if _mask is not None:
            E.scores_mask(s16, _mask)
        cap = min(kc, N)
        ws, pos, a16, e32 = self._select_and_rescore(ex, qpack32, B, s16, cap, upper)
        guard = eng.gate_rows(qpack32, B)
        state = self._state()
        fuse = seen is not None and k <= 512 and seen[0].shape[1] <= 256 and E.topk_filter_fusable(N, k, seen[0].shape[1], seen[1])
        scores, ids, f_i, f_s = E.candidates_finish(e32, a16, pos, cap, ws, self._ids_flat, N, k, eps_proved, 1.0, upper is not None, guard, sp.num_logits,
                                                    self._gate_guard_limit, state, self._state_host, seen if fuse else None)
        self._cand_dirty = False
        self.rescore_stats["calls"] += 1
        self.rescore_stats["kc"] = kc
        # the redo: the dense fp32 kernels behind the verdict, no-ops unless it failed (the host never waits)
        redo = state.view(torch.int32)[1:2]
        l32 = ex.score_dense(qpack32, B, self._index32, out=s16, run_if=redo)
        if _mask is not None:
            E.scores_mask(l32, _mask, run_if=redo)
        tws = self._buf("topk_ws", E._lib.load().rails_topk_workspace_bytes(B, N, k), torch.uint8)
        if fuse:
            E.topk_filtered(l32, k, self._ids_flat, seen[0], seen[1], workspace=tws, out=(f_i, f_s), run_if=redo)
        else:
            E.topk(l32, k, ids=self._ids_flat, workspace=tws, out=(scores, ids), run_if=redo)
        self._state_pending = (k, kc, upper is not None)
        self._state_direct = True
        if fuse:
            return "filtered", f_i, f_s.to(query_embeddings.dtype)
        if self.audit_every > 0 and self.rescore_stats["calls"] % self.audit_every == 0:
            self._audit(query_embeddings, k, scores, ids, _mask=_mask, **kwargs)      # (the audit's reference call is masked alike)
        return scores.to(query_embeddings.dtype), ids

    # ---- the proved flow split for an item-sharded corpus (rails_amd/sharded.py) --------------------------------------------------
    def shard_can_speculate(self) -> bool:
        """True iff this (local) module is bound in proved mode with both index formats resident: what ShardedMoLBruteForceTopK needs from
        EVERY rank before it runs the global proof."""
        eng = self._bind()
        eps = self._policy.eps
        return eng.exact is not None and eng.dense_precision == "f16x3" and self._index32 is not None and self._index32_engine is eng.exact \
            and eps is not None and math.isfinite(eps)

    def speculate_for_shard(self, query_embeddings: torch.Tensor, k: int, kc: int, **kwargs):
        """The proved flow on THIS shard without a verdict: first pass over the shard, threshold selection of at most kc candidates by first-pass
        score, fp32 re-scoring, the best min(k, #candidates) by (fp32 score, position).
        -> (msg (B, 2k + 2) int64: [k score words | k ids | m | err] per row, the fp32 query pack): m = the smallest first-pass score among the
        candidates -- every item outside them scores below it (-inf when the whole shard is a candidate, +inf when nothing could be selected) --,
        err = the largest |fp32 - first pass| over the row's candidates (inf: a NaN).  The caller proves globally, after ONE all-gather of the
        messages: every item of every shard outside the candidates has s16 <= max over ranks of m, so the merged fp32 top-k is the dense one iff
        its k-th score exceeds that by eps (rails_merge_candidates_verdict)."""
        eng = self._bind()
        ex = eng.exact
        B, N = query_embeddings.size(0), self._index.n_items
        dev = query_embeddings.device
        # an fp32 pack of its own: with submit / result pipelining the verdict of batch i reads its gate rows while batch i + 1's prologue runs
        n_q = eng.lib.rails_mol_query_pack_floats(E.C.byref(eng.shape), B)
        qpack16, qpack32 = eng.query_pack_both(query_embeddings, kwargs.get("user_ids"), self._buf("qpack", n_q, torch.float32),
                                               torch.empty(n_q, dtype=torch.float32, device=dev))
        msg = torch.empty((B, 2 * k + 2), dtype=torch.int64, device=dev)
        if N == 0:      # an empty shard still takes part in the exchange: nothing to offer, nothing left outside
            msg[:, :k] = int(torch.tensor(float("-inf")).view(torch.int32)) & 0xFFFFFFFF
            msg[:, k : 2 * k] = -1
            msg[:, 2 * k] = int(torch.tensor(float("-inf")).view(torch.int32)) & 0xFFFFFFFF
            msg[:, 2 * k + 1] = 0
            return msg, qpack32
        cap = min(max(kc, 1), N)
        upper = self._policy.poly
        # bias=False: the tests' planted first-pass error is NOT applied here -- the sharded forced-failure test plants its failure through the
        # global proof's eps instead
        s16 = self._first_pass(eng, qpack16, B, upper, bias=False)
        ws, pos, a16, e32 = self._select_and_rescore(ex, qpack32, B, s16, cap, upper)
        E.candidates_finish(e32, a16, pos, cap, ws, self._ids_flat, N, k, 0.0, 1.0, upper is not None, None, 0, 0.0, None, None, msg=msg)
        self._cand_dirty = False
        self.rescore_stats["calls"] += 1
        self.rescore_stats["kc"] = kc
        return msg, qpack32

    # ---- in-place corpus changes: the proved mode's companions (built in _bind) ---------------------------------------------------------
    def _index32_held(self, eng) -> bool:
        return eng.exact is not None and self._index32 is not None and self._index32_engine is eng.exact

    def _rows32_resize(self, eng, n_new: int) -> None:
        self._rows32 = E.resized(self._rows32, eng.exact.lib.rails_mol_index_rows_floats(E.C.byref(eng.exact.shape), n_new))

    def _index32_drop(self) -> None:
        self._index32 = self._rows32 = self._index32_engine = None      # (a fresh dense module holds neither; a proved one builds both in _bind)

    def _bound_refresh(self, eng, pos: torch.Tensor, emb: torch.Tensor) -> None:
        """The monitored flow's probes follow the raw rows' norms: drawn again at the next call.  The bound's one corpus-dependent figure,
        GATE_GUARD / max |gi|, as a fresh module reads it at its first bind: one pass over the item-gate rows of the index (N * L floats; an
        old maximum may have belonged to a replaced item) -- under a policy that stands; one forgotten with the corpus size is evaluated,
        guard and all, by the _bind() that ends the edit."""
        self._risk_pool = self._risk_rows = None
        pol = self._policy
        if eng.exact is not None and eng.dense_precision == "f16x3" and pol.eps is not None and pol.terms is not None and math.isfinite(float(pol.terms.get("eps", math.inf))):
            pol = pol.with_guard(self._gi_abs_max())
            self._gate_guard_limit = pol.guard_limit
            self._policy = pol

    _HELD = (
        Held(("_index32",), _index32_held, lambda tk, eng, n: eng.exact.resize_index(tk._index32, n),
             lambda tk, eng, pos, emb: eng.exact.update_index(tk._index32, pos, emb), _index32_drop),
        Held(("_rows32",), lambda tk, eng: tk._index32_held(eng) and tk._rows32 is not None, _rows32_resize,
             lambda tk, eng, pos, emb: eng.exact.update_index_rows(tk._index32, tk._rows32, pos), None),      # (dropped with _index32)
        Held(("_policy", "_gate_guard_limit"), lambda tk, eng: True, None, _bound_refresh, None),
    )

    def _forget_corpus_choices(self) -> None:
        """Proved or dense, the form of the bound, the margins, max |gi|, the probes: all decided or drawn again for the new size (_bind)."""
        self._policy = BoundPolicy()
        self._gate_guard_limit = None
        self._probe_pool = self._risk_pool = self._risk_rows = None

    ROWS_COPY_MAX_BYTES = 8 << 30      # the row-major copy of the fp32 index is kept for indexes up to this size (0: never)
    _rows32 = None

    def _note_verdict(self, good: bool, k: int, kc: int, per_pair: bool) -> None:
        self._recent.append(good)
        if not good:
            self.rescore_stats["fallbacks"] += 1
            # crowded scores or a coarse first pass: more candidates from the next call on, while doubling the margin still yields more of
            # them (candidate_count's caps).  Proved mode: the candidates must cover everything within eps of the k-th score, whatever it
            # takes; the monitored margin stops at four times its start
            proved = self._in_proved_mode()
            if (proved or self._pad_scale < 4) and self.candidate_count(k, per_pair, self._policy_items(), self._pad_scale * 2, single=not proved) > kc:
                self._pad_scale *= 2

    def _state(self) -> torch.Tensor:
        if self._verdict_state is None:
            dev = self._item_embeddings.device
            self._verdict_state = torch.zeros(8, dtype=torch.float32, device=dev)
            self._state_host = torch.zeros(8, dtype=torch.float32).pin_memory()
            self._state_event = torch.cuda.Event()
            self._state_pending = None
            self._state_seen = (0.0, 0.0)     # (calls, redone calls) already folded into rescore_stats
        return self._verdict_state

    def _absorb_state(self, wait: bool = False) -> None:
        """Fold the device verdict of the PREVIOUS call(s) into rescore_stats / the candidate margin / the pause logic.  Non-blocking
        unless `wait` (stats()): a snapshot that has not landed yet is picked up by a later call."""
        if self._verdict_state is None or self._state_pending is None:
            return
        if self._state_direct:
            # the finish kernel writes the state into the pinned host words itself, the call counter last: a snapshot is whole when the
            # counter reads the same before and after it
            if wait:
                torch.cuda.current_stream(self._verdict_state.device).synchronize()
            c0 = float(self._state_host[5])
            h = self._state_host.tolist()
            if h[5] != c0 or (h[5] <= self._state_seen[0] and not wait):
                return
        else:
            if wait:
                self._state_event.synchronize()
            elif not self._state_event.query():
                return
            h = self._state_host
        calls, redone = float(h[5]), float(h[6])
        new_calls = max(0, int(calls - self._state_seen[0]))
        new_redone = min(new_calls, max(0, int(redone - self._state_seen[1])))
        self._state_seen = (calls, redone)
        self._err_seen = max(self._err_seen, float(h[0]))
        self.rescore_stats["eps"] = float(h[2])
        self.rescore_stats["guard_max"] = max(self.rescore_stats.get("guard_max", 0.0), float(h[7]))
        k, kc, per_pair = self._state_pending
        self._state_pending = None
        for i in range(new_calls):
            self._note_verdict(i >= new_redone, k, kc, per_pair)
        if self._in_proved_mode():
            self._count_proved(new_calls - new_redone)

    _first_pass_hook = None

    def _in_proved_mode(self) -> bool:
        return self._policy.eps is not None

    def _proved_eps(self) -> Optional[float]:
        """The eps the verdicts of the bound engine compare with (BoundPolicy.eps); None for the one-product first pass and the dense modes."""
        return self._policy.eps

    def _gi_abs_max(self) -> float:
        """max |gi| over the corpus, from the item-gate rows of the tile-packed index (fp32 in both formats; padding rows are zero).
        Once per index: metadata of the bound, not part of the scoring path."""
        idx = self._index
        tiles = (idx.n_items + E.TILE_ITEMS - 1) // E.TILE_ITEMS
        if tiles == 0:
            return 0.0
        tf = idx.buf.numel() // tiles
        gi_f = E.TILE_ITEMS * self._engine.spec.num_logits
        view = idx.buf.view(tiles, tf)[:, tf - gi_f :]
        parts = [torch.stack(torch.aminmax(view[t0 : t0 + (1 << 18)])) for t0 in range(0, tiles, 1 << 18)]    # chunks of 8 M items; no host wait per chunk
        m = torch.stack(parts)                      # (chunks, 2): per-chunk (min, max); a NaN anywhere propagates
        lo, hi = float(m[:, 0].min()), float(m[:, 1].max())
        if lo != lo or hi != hi:
            return math.inf
        return max(-lo, hi, 0.0)

    def _count_proved(self, n_clear: int) -> None:
        """Calls whose verdict cleared count as PROVED while no observed |first pass - fp32| has exceeded the a-priori bound."""
        eps = self._policy.eps
        if self._err_seen > eps:
            self.rescore_stats["bound_violations"] = self.rescore_stats.get("bound_violations", 0) + 1
            return
        self.rescore_stats["proved_calls"] = self.rescore_stats.get("proved_calls", 0) + max(0, n_clear)

    def stats(self) -> Dict[str, float]:
        """rescore_stats brought up to date with the device-side verdicts and the audit counter (synchronises), plus the a-priori
        bound of rigorous_eps() next to the empirical eps the verdicts use."""
        self._absorb_state(wait=True)
        out = self.audit_summary()
        eng = self._bind()
        if eng.exact is not None:
            out.update(self.rigorous_eps())
        out.update(self.fusion_stats())      # (fused_list_calls / fused_matrix_calls, once a call has been fused: DESIGN section 3.20)
        out.update(self.pair_stats())        # (score_of_calls / explain_calls, once a pair-level call has been made: DESIGN section 3.22)
        return out

    def rigorous_eps(self) -> Dict[str, float]:
        """The A-PRIORI bound on |first pass - fp32 logit| that holds for EVERY (query, item) pair, from the pair-gate weights alone
        (rails_amd/f16x3_bound.py, which states the arithmetic model and the propagation; oracle/f16x3_bound.py restates it and
        tests/test_f16x3_bound_cpu.py checks it against float64 evaluations of both arithmetics).
          eps_rigorous          the bound for this module's first pass: finite for the f16x3 pass of a glu_silu module with a hidden pair-gate
                                layer and l2-normalised components (random-init amzn-books: ~0.7 on logits in [-20, 20], against an observed
                                maximum of 3e-5 -- the bound adds absolute values where the real roundings cancel); infinite otherwise,
                                and for the one-product pass "f16-exact", whose operands carry 11 bits (its bound is the trivial 2 / tau).
          eps_rigorous_usable   True iff the verified top-k of this module RUNS on that bound: the verdicts then compare e_k - m with
                                eps_rigorous itself and a cleared call is proved, not merely monitored.
          eps_default           the calibrated empirical eps of the monitored modes, for comparison."""
        eng = self._bind()
        single = eng.dense_precision == "f16x1"
        inv_tau = 1.0 / float(eng.spec.temperature)
        default = (self.RESCORE_EPS_PER_INV_TEMPERATURE_F16X1 if single else self.RESCORE_EPS_PER_INV_TEMPERATURE) * inv_tau
        if single:
            return {"eps_rigorous": 2.0 * inv_tau, "eps_default": default, "eps_rigorous_usable": False}
        pol = self._evaluated(eng.spec, eng.lib)
        bound = float(pol.terms.get("eps", math.inf))
        out = {"eps_rigorous": bound, "eps_default": default, "eps_rigorous_usable": bool(math.isfinite(bound) and eng.exact is not None),
               "eps_rigorous_terms": {k: v for k, v in pol.terms.items() if k != "eps"}}
        if eng.exact is not None and self._item_embeddings.is_cuda:
            from . import arith_check

            out["arithmetic_model_on_device"] = arith_check.report(self._item_embeddings.device)     # H1-H3 re-measured on this device (worst error / bound)
        if eng.exact is not None and pol.poly is not None:
            # one eps for every pair is too coarse for this shape: the first pass adds a per-pair bound (quadratic in the pair's largest
            # |cross logit|) to its logit and the verdict compares upper bounds with exact scores, eps = 0
            out.update({"bound_kind": "per-pair upper bound", "upper_bound_poly": list(pol.poly), "eps_of_max_abs_cl": pol.eps_of_c})
        return out

    # Shadow audit: every AUDIT_EVERY-th verified call is ALSO run on the dense fp32 path and compared bit for bit; the counts are in
    # rescore_stats["audited" / "mismatches"] (bench.py reports them).  0 = off.  RAILS_AUDIT_EVERY overrides the default.
    AUDIT_EVERY = int(__import__("os").environ.get("RAILS_AUDIT_EVERY", "0"))

    def _audit(self, query_embeddings: torch.Tensor, k: int, scores: torch.Tensor, ids: torch.Tensor, **kwargs) -> None:
        """Dense fp32 top-k of the same batch on a side stream (after the verified result is complete), compared on the device; the
        mismatch count is accumulated in a device counter and read when rescore_stats is next summarised (audit_summary())."""
        cur = torch.cuda.current_stream(query_embeddings.device)
        if self._audit_stream is None:
            self._audit_stream = torch.cuda.Stream(query_embeddings.device)
            self._audit_bad = torch.zeros(1, dtype=torch.int64, device=query_embeddings.device)
        side = self._audit_stream
        side.wait_stream(cur)
        for t in (query_embeddings, scores, ids):
            t.record_stream(side)
        with torch.cuda.stream(side):
            ref_s, ref_i = self._forward_fp32_dense(query_embeddings, k, _private=True, **kwargs)
            bad = (ref_i != ids).any() | (ref_s != scores.to(ref_s.dtype)).any()
            self._audit_bad += bad.to(torch.int64)
        cur.wait_stream(side)     # the recycled scratch buffers of the next call must not race with the audit
        self.rescore_stats["audited"] += 1

    def audit_summary(self) -> Dict[str, int]:
        """rescore_stats with the device-side mismatch counter folded in (one synchronising read)."""
        if self._audit_stream is not None:
            self.rescore_stats["mismatches"] = int(self._audit_bad.item())
        return dict(self.rescore_stats)

    SAFETY_F16X1 = 3.0      # eps >= SAFETY x the running maximum of |s16 - s32| over the re-scored candidates and probes

    # Speculation pays on large corpora only: below SPECULATE_MIN_ITEMS the fixed cost of the verification (~0.1 ms) exceeds what
    # the faster first pass saves (ML-20M, 27 278 items: fp32 step 0.26 ms; amzn-books shape at 16 384 items: 0.19 against 0.21 ms of GPU time,
    # at 20 000: 0.173 with per-pair bounds, at 32 768: 0.219 against 0.343 ms), so the exact modes run the dense fp32 kernels there.
    # It also needs scores that are not crowded around the k-th place: when more than a quarter of the last 16 speculative calls
    # had to be redone, the next 256 calls go straight to the dense fp32 path, then speculation is tried again.
    SPECULATE_MIN_ITEMS = 1 << 14

    def _speculation_paused(self) -> bool:
        if self._pause_left == 0 and len(self._recent) >= 16:
            bad = self._recent.count(False)
            self._recent.clear()
            if bad > 4:
                self._pause_left = 256
        if self._pause_left > 0:
            self._pause_left -= 1
            self.rescore_stats["paused_calls"] = self.rescore_stats.get("paused_calls", 0) + 1
            return True
        return False

    def _read_stats(self, stats: torch.Tensor) -> Tuple[float, float]:
        """(rows, 2) per-row [max |exact - approx|, k-th exact - min candidate approx] -> (largest error, smallest margin) on the
        host: an async copy into pinned memory and a spin on its event.  (A blocking read parks the thread on an interrupt-driven
        wait whose wake-up cost 0.1-0.5 ms per call here; the result is due in microseconds.)"""
        B = stats.shape[0]
        if self._ok_host is None or self._ok_host.shape[0] < B:
            self._ok_host = torch.empty((max(B, 64), 2), dtype=torch.float32).pin_memory()
            self._ok_event = torch.cuda.Event()
        self._ok_host[:B].copy_(stats, non_blocking=True)
        self._ok_event.record()
        while not self._ok_event.query():
            pass
        h = self._ok_host[:B]
        err, gap = float(h[:, 0].max()), float(h[:, 1].min())
        if bool(torch.isnan(h).any()):
            err = float("inf")
        return err, gap

    RISK_POOL = 4096      # highest-norm items of the corpus kept as a probe pool
    RISK_ALWAYS = 16      # ... the top of it is probed on every call

    def _probes(self, B: int, N: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Two (B, 32) blocks of corpus positions re-scored next to the candidates so that |first pass - fp32| is watched OUTSIDE them too:
        32 drawn uniformly from the whole corpus (row block `call mod 64` of a pool drawn once per (B, N)), the RISK_ALWAYS items
        of largest embedding norm on every call, and 16 more rotating through the RISK_POOL highest-norm items -- large inputs make
        large gate pre-activations, which is where a reduced-precision first pass is furthest off."""
        dev = self._item_embeddings.device
        pool = self._probe_pool
        if pool is None or pool.shape[1] != B or self._probe_n != N:
            g = torch.Generator(device=dev).manual_seed(0x5EED)
            pool = self._probe_pool = torch.randint(0, N, (64, B, E.TILE_ITEMS), generator=g, device=dev, dtype=torch.int64)
            self._probe_n = N
            self._risk_pool = None
        if self._risk_pool is None:
            # row norms of the raw item table, in slices (monitoring metadata computed once per corpus; not part of the scoring path)
            X, best_v, best_i = self._item_embeddings[0], None, None
            for lo in range(0, N, 1 << 22):
                nv = torch.linalg.vector_norm(X[lo : lo + (1 << 22)].float(), dim=1)
                kk = min(self.RISK_POOL, nv.numel())
                v, i = torch.topk(nv, kk)
                i = i + lo
                if best_v is not None:
                    v, i = torch.cat([best_v, v]), torch.cat([best_i, i])
                    v, sel = torch.topk(v, min(self.RISK_POOL, v.numel()))
                    i = i[sel]
                best_v, best_i = v, i
            self._risk_pool = best_i.to(torch.int64)
            self._risk_rows = None
        if self._risk_rows is None:
            # every row the rotation can produce, once: (phases, 32) positions = the RISK_ALWAYS items + 16 of the rest, window start
            # (phase * 16) mod len(rest).  Per call the probes are then two views -- no index arithmetic on the device (the arange /
            # add / remainder / index / cat chain of the first version was seven small launches, ~40 us of a 1.7 ms step).
            risk = self._risk_pool
            n_always = min(self.RISK_ALWAYS, risk.numel())
            rest = risk[n_always:] if risk.numel() > n_always else risk
            n_rot = E.TILE_ITEMS - n_always
            m = max(rest.numel(), 1)
            phases = m // math.gcd(m, n_rot)
            idx = (torch.arange(phases, device=dev)[:, None] * n_rot + torch.arange(n_rot, device=dev)[None, :]) % m
            self._risk_rows = torch.cat([risk[:n_always].unsqueeze(0).expand(phases, -1), rest[idx]], dim=1).contiguous()
        call = self.rescore_stats["calls"]
        return pool[call % 64], self._risk_rows[call % self._risk_rows.shape[0]].unsqueeze(0).expand(B, -1)

    def _dense_fp32_index(self) -> E.MolIndex:
        ex = self._engine.exact
        if self._index32 is None or self._index32_engine is not ex:
            self._index32, self._index32_engine = ex.build_index(self._item_embeddings[0]), ex
        return self._index32

    def _forward_fp32_dense(self, query_embeddings: torch.Tensor, k: int, _private: bool = False, _mask=None, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """The exact-fp32 brute force of this module's corpus (fallback of a failed verification, small corpora, the audit).
        Same policies as the plain fp32 module: never more than MAX_LOGIT_BYTES of logits (corpus chunks beyond that), and with
        keep_dense_fp32_index False -- or when _bind declined the second index for lack of memory -- no resident fp32 index either:
        each chunk's index is rebuilt from the raw rows and dropped."""
        ex = self._engine.exact
        B, N = query_embeddings.size(0), self._index.n_items
        have32 = self._index32 is not None and self._index32_engine is ex
        if have32 and B * N * 4 <= self.MAX_LOGIT_BYTES:
            return self._dense_topk(query_embeddings, k, _eng=ex, _index=self._index32, _tag="qpack32", _private=_private, _mask=_mask, **kwargs)
        if have32:
            return self._forward_chunked(query_embeddings, k, _engine=ex, _index=self._index32, _mask=_mask, **kwargs)
        # no resident fp32 index: temporary per-chunk indexes (CHUNK_ITEMS rows at a time), merged like _forward_chunked
        C = min(self.CHUNK_ITEMS, max(1, self.MAX_LOGIT_BYTES // (4 * max(B, 1))))
        C = max(E.TILE_ITEMS, C // E.TILE_ITEMS * E.TILE_ITEMS)
        qpack32, _, _ = ex.query_pack(query_embeddings, kwargs.get("user_ids"))
        part_s, part_p = [], []
        for lo in range(0, N, C):
            n = min(C, N - lo)
            idx = ex.build_index(self._item_embeddings[0, lo : lo + n])
            logits = ex.score_dense(qpack32, B, idx)
            if _mask is not None:
                E.scores_mask(logits, _mask, first_item=lo)
            s_, p_ = E.topk(logits, min(k, n))
            part_s.append(s_)
            part_p.append(p_ + lo)
            del idx
        scores, pos = E.topk(torch.cat(part_s, 1), k, ids=torch.cat(part_p, 1))
        return scores.to(query_embeddings.dtype), self._ids_flat[pos]

    def _bind(self) -> E.MolEngine:
        eng = super()._bind()
        if eng.exact is not None and self._calib_engine is not eng:   # a new engine (other weights or precision): calibrate afresh
            self._calib_engine = eng
            self._err_seen, self._pad_scale, self._pause_left = 0.0, 1, 0
            self._recent.clear()
            self._verdict_state = None
            self._state_pending = None
            if eng.dense_precision == "f16x3":
                self.rescore_stats["proved_calls"] = 0
                self.rescore_stats["bound_violations"] = 0
        if eng.exact is not None and self._policy.eps is None and eng.dense_precision == "f16x3":
            # the bound for this engine, once: its form, the eps handed to the verdict and the device-side guard limit GATE_GUARD / max |gi|
            pol = self._evaluated(eng.spec, eng.lib)
            if math.isfinite(float(pol.terms.get("eps", math.inf))):
                pol = pol.with_guard(self._gi_abs_max())
                self._gate_guard_limit = pol.guard_limit
            else:
                pol = pol._replace(eps=math.inf)
            self._policy = pol
        if eng.exact is not None and self._index32_engine is not eng.exact and self.keep_dense_fp32_index is not False:
            # precision "f16x3-exact": a dense fp32 index next to the f16x3 one makes the candidates a gather (10 us) instead of
            # an index build of their raw rows (160 us), and is the fallback's index.  Same bytes again; skipped (None) when
            # less than twice that is free, or when keep_dense_fp32_index is set to False.
            need = self._index.buf.numel() * 4
            free, _ = torch.cuda.mem_get_info(self._item_embeddings.device)
            self._index32 = None
            self._index32_engine = eng.exact
            if self.keep_dense_fp32_index or free > 2 * need:
                self._index32 = eng.exact.build_index(self._item_embeddings[0])
            # ... and, where the candidates are re-scored in place and a third copy is small change (ROWS_COPY_MAX_BYTES), the same index
            # row-major: a candidate's bytes then come in whole cache lines (score_indexed_rows: 8 x fewer bytes than the tile-packed reads)
            self._rows32 = None
            if (self._index32 is not None and self.ROWS_COPY_MAX_BYTES > 0 and need <= self.ROWS_COPY_MAX_BYTES and eng.exact.score_indexed_supported(32, 1024)):
                free, _ = torch.cuda.mem_get_info(self._item_embeddings.device)
                if free > 2 * need:
                    self._rows32 = eng.exact.build_index_rows(self._index32)
        return eng

def _pinned_word(module) -> torch.Tensor:
    """One int32 in pinned host memory, zeroed on the device by the first launch of the call that takes it.  A word goes back to the module's
    free list only when its verdict has been read (_release_words): a call of many slices, or several batches in flight, never share one."""
    free = module._flag_free
    return free.pop() if free else torch.zeros(1, dtype=torch.int32).pin_memory()


def _release_words(module, words) -> None:
    module._flag_free.extend(words[: max(0, 64 - len(module._flag_free))])


def _verdicts_clear(pending: list, module) -> bool:
    """pending: int32 verdict words of fused scans (1 = a candidate count left its range), read after everything that depends on them is
    enqueued.  They live in PINNED HOST memory (the kernels store through the device-visible address) and are read after a spin on an event -- no
    copy launch, no blocking sync (a blocking read parks the thread on an interrupt whose wake-up costs 20-100 us of idle GPU per batch)."""
    if not pending:
        return True
    if torch.cuda.is_available():
        ev = torch.cuda.Event()
        ev.record()
        while not ev.query():
            pass
    _release_words(module, pending)
    return all(int(b.numpy()[0]) == 0 for b in pending)     # (a plain memory read through the numpy view)


class CandidateScan(NamedTuple):
    """One candidate scan as _speculative_scan runs it: what differs between the coarse scan and the component scans, and nothing else."""
    n: int                                      # items scanned
    k: int                                      # selected per row of the score matrix
    rows_per_query: int                         # rows of the score matrix per batch row
    route: Callable[..., Tuple[bool, bool]]     # (batch, restriction) -> the module's _scan_route for this scan: (eligible, allowed)
    width: Callable[[bool], int]                # (allowed) -> batch rows one call takes: the scans keep the query rows in LDS, wider batches go in slices
    launch: Callable                            # (eq, flag, **Restriction.launch_kwargs()) -> (scores, positions, the verdict word), or None: sizes without a plan
    scores: Callable[..., torch.Tensor]         # (eq, out=None, run_if=None) -> the materialised (rows, n) scores
    redo_buffer: str                            # _buf tag of the recycled (rows, n) matrix of a redo on the device
    redo_on_device: Callable[[int], bool]       # (batch) -> the redo is enqueued behind the fused launch, under its verdict word
    device_flag: Callable[[], Optional[torch.Tensor]]   # the verdict word of a call the host does not defer; None: the launcher's own
    shaped: Callable[..., torch.Tensor]         # (positions, batch) -> the positions as the scan's caller takes them


def _speculative_scan(tk, scan: CandidateScan, eq: torch.Tensor, restr: Optional[Restriction], pending: Optional[list] = None, with_scores: bool = False):
    """The one flow of the candidate scans: eq (B, P_Q, d) -> scan.shaped(positions) (with_scores: -> (scores, positions)), the exact top-k of every
    row among the items `restr` lets it return.  The fused scan (no score matrix: 16 GB per 125 M-item shard at B = 32) is exact iff every row
    collected between k and `capacity` candidates; its launches raise a verdict word otherwise, and one of three things follows:
      the redo ON THE DEVICE: scorer, mask and top-k are enqueued under that word as their launch predicate and overwrite the outputs -- no-ops
        unless a count was out of range, nothing for the host to wait for;
      a DEFERRED verdict (`pending`, a list): the word lives in pinned host memory, where the kernels write it themselves (no copy launch); it is
        appended, the positions are returned at once, and the caller reads it (_verdicts_clear, MoLAvgTopK.result) after it has enqueued all
        that depends on them -- speculate, then verify: the GPU never waits for the host in mid-pipeline;
      else the word is read here (one 4-byte D2H copy), and a failed verdict takes the materialising path of every scan that is not fused."""
    n, k, batch = scan.n, scan.k, eq.shape[0]
    for limit in (n,) if restr is None else (n, restr.count):
        if k > limit:
            raise RuntimeError(f"selected index k out of range (k={k}, n={limit})")
    eligible, allowed = scan.route(batch, restr)
    width = scan.width(allowed)
    if batch > width:
        parts = [_speculative_scan(tk, scan, eq[b0 : b0 + width], None if restr is None else restr.rows_slice(b0, b0 + width), pending, with_scores)
                 for b0 in range(0, batch, width)]
        return (torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)) if with_scores else torch.cat(parts, dim=0)
    if eligible and allowed and not tk._no_fused:
        on_device = scan.redo_on_device(batch)
        # a word goes back to the free list when its verdict has been read -- or here, when no launch took it
        word = _pinned_word(tk) if (not on_device and pending is not None) else None
        fused = scan.launch(eq, scan.device_flag() if word is None else word, **({} if restr is None else restr.launch_kwargs()))
        if fused is None:
            _release_words(tk, () if word is None else (word,))
        else:
            sc, pos, bad = fused
            if on_device:      # (the (rows, n) score buffer is recycled across calls)
                rows = batch * scan.rows_per_query
                scores = scan.scores(eq, out=tk._buf(scan.redo_buffer, rows * n, torch.float32).view(rows, n), run_if=bad)
                if restr is not None:
                    restr.mask(scores, run_if=bad)
                E.topk(scores, k, out=(sc, pos), run_if=bad)
            elif pending is not None:
                pending.append(bad)
            if on_device or pending is not None or int(bad.item()) == 0:
                return (sc, pos) if with_scores else scan.shaped(pos, batch)
    scores = scan.scores(eq)
    if restr is not None:
        restr.mask(scores)
    sc, pos = E.topk(scores, k)
    return (sc, pos) if with_scores else scan.shaped(pos, batch)


class CollapseWalk(NamedTuple):
    """One enqueued walk of a collapsed call: its outputs and the pinned verdict word the host reads behind them."""
    scores: torch.Tensor
    positions: torch.Tensor
    ids: torch.Tensor
    counts: torch.Tensor
    word: torch.Tensor

    def clear(self, tk) -> bool:
        return _verdicts_clear([self.word], tk)


def _collapse_count(tk, key: str) -> None:
    stats = tk.__dict__.setdefault("_collapse_stats", {"calls": 0, "walk_redos": 0, "fallbacks": 0})
    stats[key] += 1


def _asks_collapse(kwargs: dict) -> bool:
    """Does the call name one of the two arguments of section 3.16?  (A call with neither runs none of its code.)"""
    return "collapse_groups" in kwargs or "max_per_group" in kwargs


def _too_few_groups(k: int, counts: torch.Tensor, m: int = 1) -> RuntimeError:
    if m > 1:
        return RuntimeError(f"selected index k out of range (k={k}, n={int(counts.min())}: the eligible items within max_per_group={m} of the row "
                            "with the fewest)")
    return RuntimeError(f"selected index k out of range (k={k}, n={int(counts.min())}: the distinct eligible groups of the row with the fewest)")


def _collapse_walk(tk, scores: torch.Tensor, positions: torch.Tensor, k: int, invalid_ids: Optional[torch.Tensor], m: int = 1) -> CollapseWalk:
    """The one walk launch behind a ranked list of POSITIONS in key order; the seen-id filter runs inside it.  m = 1: rails_topk_collapse;
    m > 1 (at most k: the caller's m_eff): rails_topk_collapse_quota."""
    ranks, _ = tk._dense_group_ranks()
    word = _pinned_word(tk)
    word.zero_()      # (a word on the free list has been read: nothing in flight writes it)
    return CollapseWalk(*E.topk_collapse(scores, positions, ranks, k, tk._ids_flat, invalid_ids, word, None if m == 1 else m), word)


def _collapsed_exact(tk, query_embeddings: torch.Tensor, k: int, invalid_ids: Optional[torch.Tensor], kwargs: dict,
                     m: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """The collapsed call of an exact module -> (scores, ids).  The module's ordinary ranked top-D BY POSITION, through the
    arm it would take anyway with the call's mask / hidden set / tags -- the seen ids are NOT handed to it: a seen item must not represent its
    group, so they go to the walk --, then the walk; a walk that found fewer than k groups doubles D up to COLLAPSE_MAX_DEPTH, and beyond that
    the exact fallback answers: the group maxima of the materialised scores (_collapse_fallback).  Correctness never depends on the depths:
    the first k first-occurrences of the top-D are those of the whole ranking whenever the top-D holds k of them.
    m > 1 (max_per_group=): whether an item is kept depends on the items before it alone, so the argument is the same one; the walk keeps the
    first m_eff = min(m, k) members of a group (beyond k a quota excludes nothing among the first k), the fallback the best m_eff.
    The limits are checked before any launch of the call itself; the size check of the fallback's table needs G, so on a key row whose dense
    ranks are not cached yet it computes them first (group_ranks: torch integer ops, once per set_item_groups or edit) -- work every
    collapsed call on that row needs anyway."""
    width = 0 if invalid_ids is None else invalid_ids.shape[1]
    if k > E.COLLAPSE_MAX_K or width > E.COLLAPSE_MAX_SEEN:      # (the fallback's sizes: it must be there for every call the walks may fail on)
        how = "collapse_groups=True" if m == 1 else f"max_per_group={m}"
        raise NotImplementedError(f"{type(tk).__name__}: {how} takes k <= {E.COLLAPSE_MAX_K} and up to {E.COLLAPSE_MAX_SEEN} seen ids per "
                                  f"row (what its exact group-maxima pass selects and filters), got k = {k}, width = {width}")
    m = min(m, max(k, 1))
    if m > 1:
        if m > E.COLLAPSE_MAX_PER_GROUP:
            raise NotImplementedError(f"{type(tk).__name__}: max_per_group takes min(max_per_group, k) <= {E.COLLAPSE_MAX_PER_GROUP} on the exact modules "
                                      f"(their fallback reads the scores once per result of a group), got {m}")
        row_bytes = m * tk._dense_group_ranks()[1] * 8
        if row_bytes > int(getattr(tk, "MAX_LOGIT_BYTES", 4 << 30)):
            raise NotImplementedError(f"{type(tk).__name__}: max_per_group={m} needs {row_bytes} bytes of group keys per query for its exact fallback, "
                                      f"beyond MAX_LOGIT_BYTES = {int(getattr(tk, 'MAX_LOGIT_BYTES', 4 << 30))}")
    _collapse_count(tk, "calls")
    B, n = query_embeddings.size(0), tk.num_items
    # the call's mask -- item_mask= (a bool tensor is packed here: its one sync), allowed_tags=, the hidden set -- is resolved ONCE; every
    # forward of the loop and the fallback take the resolved ItemMask as it is (_take_item_mask's _resolved_mask)
    kwargs = dict(kwargs)
    mask = tk._take_item_mask(kwargs, B, k)
    kwargs["_resolved_mask"] = mask
    bound = n if mask is None else mask.kept_min
    if k > bound:
        raise RuntimeError(f"selected index k out of range (k={k}, n={bound})")
    depth = min(bound, tk.COLLAPSE_DEPTH_FACTOR * (k + width), E.COLLAPSE_MAX_LIST)
    while depth >= k:
        with tk._positions_as_ids():
            scores, positions = tk.forward(query_embeddings, depth, **dict(kwargs))
        walk = _collapse_walk(tk, scores, positions, k, invalid_ids, m)
        if walk.clear(tk):
            return walk.scores.to(query_embeddings.dtype), walk.ids
        deeper = min(2 * depth, bound, tk.COLLAPSE_MAX_DEPTH, E.COLLAPSE_MAX_LIST)
        if deeper <= depth:
            break
        depth = deeper
        _collapse_count(tk, "walk_redos")
    del kwargs["_resolved_mask"]
    return _collapse_fallback(tk, query_embeddings, k, invalid_ids, mask, kwargs, m)


def _collapse_fallback(tk, query_embeddings: torch.Tensor, k: int, invalid_ids: Optional[torch.Tensor], mask: Optional[E.ItemMask],
                       kw: dict, m: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exact fallback of a collapsed call: dense scores of the module's own precision, the call's mask written into them, their per-group
    best m as 64-bit keys (rails_scores_group_next, per corpus chunk under the logit policy, the seen-id filter inside) and the top-k of the
    (B, m * G) key table (rails_topk_keys) -- a slice of the batch at a time where that table would exceed the same policy.  A row with fewer
    than k non-empty groups is the RuntimeError of a call for more than there is.  mask: the call's resolved mask; kw: its other keyword
    arguments.  (k, m and the seen-id width were checked against the pass's limits by _collapsed_exact, before any launch.)
    Round t of a row lies beside round t - 1 -- every group's (t + 1)-th best eligible item, bounded by the finished round before it; rounds
    outermost, corpus chunks inside.  m = 1 is round 0 alone, the group maxima: one fill and one kernel per chunk.  A corpus of one chunk is
    scored once and read m times, a chunked one is scored again for every round (its pieces share a buffer).  Every key of the table is among
    its group's best m and every item the quota keeps is in it, so its top-k is the answer."""
    _collapse_count(tk, "fallbacks")
    B = query_embeddings.size(0)
    ranks, groups = tk._dense_group_ranks()
    rows = max(1, min(B, int(getattr(tk, "MAX_LOGIT_BYTES", 4 << 30)) // (m * groups * 8)))
    parts = []
    for b0 in range(0, B, rows):
        b1 = min(B, b0 + rows)
        part_kw = {key: (v[b0:b1] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B else v) for key, v in kw.items()}
        part_mask = mask if mask is None or mask.shared else mask.rows_slice(b0, b1)
        part_seen = None if invalid_ids is None else invalid_ids[b0:b1]
        table = torch.zeros((b1 - b0, m * groups), dtype=torch.int64, device=query_embeddings.device)
        only = None      # the one chunk of an unchunked corpus, kept for the later rounds
        for t in range(m):
            pieces = [only] if only is not None else tk._own_score_chunks(query_embeddings[b0:b1], part_mask, **part_kw)
            n_pieces = 0
            for lo, logits in pieces:
                E.scores_group_next(logits, ranks, table, groups, t, first_item=lo, ids=tk._ids_flat, invalid_ids=part_seen)
                n_pieces += 1
            if t == 0 and n_pieces == 1:
                only = (lo, logits)
        del only
        parts.append(E.topk_keys(table, k, tk._ids_flat))
    scores, ids, counts = (torch.cat([p[i] for p in parts], 0) for i in (0, 2, 3))
    if int(counts.min()) < k:      # (the one read-back of the fallback)
        raise _too_few_groups(k, counts, m)
    return scores.to(query_embeddings.dtype), ids


def _collapsed_candidates(tk, query_embeddings: torch.Tensor, k: int, invalid_ids: Optional[torch.Tensor], n_ranked: int, kwargs: dict, m: int = 1):
    """The collapsed call of an approximate module -> a handle for _collapsed_candidates_result.  The walk runs over the module's own ranked
    candidate list -- forward's, by position, in its sorted form, all n_ranked of it -- in place of the final cut to k.  No doubling and no
    fallback: the depth is the list's, and too few distinct groups among the candidates is the RuntimeError.  A list longer than the walk takes
    is refused here, before any launch."""
    n_list = n_ranked if n_ranked else tk._union_width()
    if n_list > E.COLLAPSE_MAX_LIST:
        how = "collapse_groups=True" if m == 1 else f"max_per_group={m}"
        raise NotImplementedError(f"{type(tk).__name__}: {how} walks ranked lists of up to {E.COLLAPSE_MAX_LIST} candidates per query, this "
                                  f"module ranks {n_list}")
    m = min(m, max(k, 1))      # (no limit on m here: these modules have no fallback whose cost grows with it)
    _collapse_count(tk, "calls")
    with tk._positions_as_ids(), getattr(tk, "inline_calls", contextlib.nullcontext)():
        inner = MoLAvgTopK.submit(tk, query_embeddings, n_ranked, **dict(kwargs)) if n_ranked else None
        ranked = inner[1:3] if inner is not None else tk.forward(query_embeddings, k, **dict(kwargs))
    return (tk, inner, _collapse_walk(tk, ranked[0], ranked[1], k, invalid_ids, m), k, invalid_ids, query_embeddings.dtype, m)


def _collapsed_candidates_result(handle) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (scores, ids); owns the redo of the candidate scan (MoLAvgTopK.result's) and the look at the walk's verdict."""
    tk, inner, walk, k, invalid_ids, dtype, m = handle
    if inner is not None:
        with tk._positions_as_ids():
            scores, positions = MoLAvgTopK.result(tk, inner)
        if scores is not inner[1]:      # the scan was redone on the materialising path: walk its list instead
            walk.clear(tk)
            walk = _collapse_walk(tk, scores, positions, k, invalid_ids, m)
    if not walk.clear(tk):
        raise _too_few_groups(k, walk.counts, m)
    return walk.scores.to(dtype), walk.ids


def _generic_takes_no_groups(tk, what: str) -> None:
    """Item groups on the approximate modules of the generic route: the collapse walk has not been tested there, so it is refused by name.
    Read from the engine the module is bound to (the constructor bound one): no look at the model's parameters on this path."""
    if (tk._call_eng or tk._engine).route == "generic":
        raise NotImplementedError(f"{type(tk).__name__}: {what} is not built on the generic scoring route (generic_candidates = True covers the "
                                  "single-device exhaustive algorithms without item groups); MoLBruteForceTopK collapses by item group on this route")


def _generic_takes_no_vectors(tk, what: str) -> None:
    """Item vectors on the approximate modules of the generic route: refused by name, as _generic_takes_no_groups refuses groups there."""
    if (tk._call_eng or tk._engine).route == "generic":
        raise NotImplementedError(f"{type(tk).__name__}: {what} is not built on the generic scoring route (generic_candidates = True covers the "
                                  "single-device exhaustive algorithms without item vectors); MoLBruteForceTopK diversifies on this route")


# ---- diversify=lam: the module's ranked list by position, then one walk launch -- no depth doubling, no fallback ---------
def _asks_diversity(kwargs: dict) -> bool:
    """Does the call name one of the two arguments of section 3.21?  (A call with neither runs none of its code.)"""
    return "diversify" in kwargs or "diversity_pool" in kwargs


def diversity_pool_size(k: int, pool: Optional[int], width: int, name: str) -> int:
    """D of a diversified call, checked before any launch: the pool asked for, else min(1024, max(4 k, 64)); k <= D <= 1024, and the seen ids
    the walk filters are at most COLLAPSE_MAX_SEEN per row.  Pure host arithmetic."""
    D = min(E.MMR_MAX_POOL, max(4 * k, 64)) if pool is None else pool
    if not k <= D <= E.MMR_MAX_POOL or width > E.COLLAPSE_MAX_SEEN:
        raise NotImplementedError(f"{name}: diversify= takes k <= diversity_pool <= {E.MMR_MAX_POOL} and up to {E.COLLAPSE_MAX_SEEN} seen ids per row "
                                  f"(the walk's workgroup holds one pool entry per thread), got k = {k}, diversity_pool = {D}, width = {width}")
    return D


def _pool_too_small(k: int, counts: torch.Tensor) -> RuntimeError:
    return RuntimeError(f"selected index k out of range (k={k}, n={int(counts.min())}: the eligible items of the diversity pool of the row with the fewest)")


def _mmr_walk(tk, scores: torch.Tensor, positions: torch.Tensor, lam: float, k: int, pool: int, invalid_ids: Optional[torch.Tensor]) -> CollapseWalk:
    """The one walk launch behind a ranked list of POSITIONS; the seen-id filter runs inside it (rails_topk_mmr)."""
    word = _pinned_word(tk)
    word.zero_()      # (a word on the free list has been read: nothing in flight writes it)
    return CollapseWalk(*E.topk_mmr(scores, positions, tk._vectors, lam, k, pool, tk._ids_flat, invalid_ids, word), word)


def _diversified_exact(tk, query_embeddings: torch.Tensor, k: int, invalid_ids: Optional[torch.Tensor], kwargs: dict,
                       div: Tuple[float, Optional[int]]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The diversified call of an exact module -> (scores, ids) in PICK order: the scores are the items' own relevance
    scores, so a row is not monotone.  The module's ordinary ranked top-L BY POSITION, L = min(items a row may return, D + width), through the
    arm it would take anyway with the call's mask / hidden set / tags resolved once -- the seen ids are NOT handed to it: they go to the walk,
    whose pool is the first D unseen entries -- then the one walk launch.  A row whose pool holds fewer than k is the RuntimeError of a call
    for more than there is."""
    lam, pool = div
    width = 0 if invalid_ids is None else invalid_ids.shape[1]
    D = diversity_pool_size(k, pool, width, type(tk).__name__)
    B, n = query_embeddings.size(0), tk.num_items
    kwargs = dict(kwargs)
    mask = tk._take_item_mask(kwargs, B, k)
    kwargs["_resolved_mask"] = mask
    bound = n if mask is None else mask.kept_min
    if k > bound:
        raise RuntimeError(f"selected index k out of range (k={k}, n={bound})")
    tk.__dict__.setdefault("_diversity_stats", {"calls": 0})["calls"] += 1
    with tk._positions_as_ids():
        scores, positions = tk.forward(query_embeddings, min(bound, D + width), **kwargs)
    walk = _mmr_walk(tk, scores, positions, lam, k, D, invalid_ids)
    if not walk.clear(tk):
        raise _pool_too_small(k, walk.counts)
    return walk.scores.to(query_embeddings.dtype), walk.ids


def _diversified_candidates(tk, query_embeddings: torch.Tensor, k: int, invalid_ids: Optional[torch.Tensor], n_ranked: int, kwargs: dict,
                            div: Tuple[float, Optional[int]]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The diversified call of an approximate module -> (scores, ids) in PICK order.  The walk runs over the module's own ranked candidate
    list, exactly as _collapsed_candidates takes it -- forward's, by position, all n_ranked of it -- in place of the final cut to k; a scan
    that was redone on the materialising path is walked again.  A list longer than the walk takes is refused before any launch."""
    lam, pool = div
    width = 0 if invalid_ids is None else invalid_ids.shape[1]
    D = diversity_pool_size(k, pool, width, type(tk).__name__)
    n_list = n_ranked if n_ranked else tk._union_width()
    if n_list > E.COLLAPSE_MAX_LIST:
        raise NotImplementedError(f"{type(tk).__name__}: diversify= walks ranked lists of up to {E.COLLAPSE_MAX_LIST} candidates per query, this "
                                  f"module ranks {n_list}")
    tk.__dict__.setdefault("_diversity_stats", {"calls": 0})["calls"] += 1
    with tk._positions_as_ids(), getattr(tk, "inline_calls", contextlib.nullcontext)():
        inner = MoLAvgTopK.submit(tk, query_embeddings, n_ranked, **dict(kwargs)) if n_ranked else None
        ranked = inner[1:3] if inner is not None else tk.forward(query_embeddings, k, **dict(kwargs))
    walk = _mmr_walk(tk, ranked[0], ranked[1], lam, k, D, invalid_ids)      # (outside the block: the walk looks the ids up; enqueued before the host
    if inner is not None:                                                    # looks at the scan's verdict)
        with tk._positions_as_ids():
            scores, positions = MoLAvgTopK.result(tk, inner)
        if scores is not inner[1]:      # the scan was redone on the materialising path: walk its list instead
            walk.clear(tk)
            walk = _mmr_walk(tk, scores, positions, lam, k, D, invalid_ids)
    if not walk.clear(tk):
        raise _pool_too_small(k, walk.counts)
    return walk.scores.to(query_embeddings.dtype), walk.ids


# ---- query fusion over the candidate union: opt-in per instance, fuse_candidates = True -------------------------------------
def _asks_fusion(tk, kwargs: dict) -> bool:
    """Does this call go to _fused_candidates?  The switch is read through the class default, so a bare instance, and every module that was not
    opted in, refuses query_lims= / fuse= / query_weights= by name exactly as before (refuse_query_fusion) and runs none of this code."""
    return bool(tk.fuse_candidates) and any(kwargs.get(name) is not None for name in _FUSION_KWARGS)


def _fused_candidates(tk, what: str, query_embeddings: torch.Tensor, k: int, invalid_ids: Optional[torch.Tensor], kwargs: dict):
    """The fused call of an approximate module -> (scores (U, k) fp32 as the queries' dtype, ids (U, k)).  Fused row u's candidates are the
    union C_u of the candidates the module's own generator yields for the sub-query rows of its segment -- under the hidden set, and under the
    fused row's allowed_tags= repeated over the segment --; every candidate is scored under every row of the segment (_score_at: the rerank's
    bits), the scores are fused (engine.scores_fuse_rows on the aligned columns of the union) and ranked once: the first k of C_u in key order
    (F descending, position ascending) whose id is not among the row's invalid_ids, (-1, -inf) where fewer remain.
    The shape of _ComponentCandidates._ranked: the query pack once, two attempts around the speculative scans.  Beside the scans' launches:
    the union, the expansion to the S rows, the scoring, the fusion, the holes and ids, the selection -- the same number whatever S is -- and
    no host read beyond the scans' verdict.  Everything is checked before any launch."""
    name = f"{type(tk).__name__}.{what}"
    if getattr(tk, "_use_faiss", False):      # (the IVF lists: named by the refusal the module has always raised)
        refuse_query_fusion(tk, kwargs, what)
    fusion = tk._resolve_fusion(kwargs, query_embeddings, what)
    kwargs.pop("_fusion", None)
    for given in ("collapse_groups", "max_per_group", "diversify", "diversity_pool", "item_mask"):
        value = kwargs.pop(given, None)
        if value is not None and value is not False:
            raise NotImplementedError(f"{name}: {given}= together with query_lims= is not built")
    own = type(tk).forward is MoLAvgTopK.forward      # MoLAvgTopK itself: the coarse candidates; else the component union (MoLCombTopK: both)
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"{name}: k must be an int >= 1, got {k!r}")
    if own and k > tk._avg_top_k:
        raise ValueError(f"avg_top_k ({tk._avg_top_k}) must be larger than k ({k})")
    U, S, N = fusion.lims.fused, fusion.lims.rows, tk.num_items
    width = tk._avg_top_k if own else tk._union_width()
    entries = fusion.lims.max_segment * width
    if entries > E.FUSE_LIST_MAX_ENTRIES:
        raise NotImplementedError(f"{name}: a fused row of {fusion.lims.max_segment} sub-query rows x {width} candidates holds {entries} candidate entries, "
                                  f"beyond the {E.FUSE_LIST_MAX_ENTRIES} one workgroup sorts; fuse fewer rows per user")
    if invalid_ids is not None:
        _ids_arg(what, "invalid_ids", invalid_ids, U, "w")
    w = 0 if invalid_ids is None else invalid_ids.shape[1]
    with torch.inference_mode(), tk.one_bind():
        kw = tk._segment_kwargs(kwargs, fusion)      # allowed_tags= per fused row -> per sub-query row
        tags = tk._take_allowed_tags(kw, S, (tk._avg_top_k,) if own else _tag_ks(tk))
        eng = tk._bind()
        qpack, eq, _ = eng.query_pack(query_embeddings, kw.get("user_ids"), want_plain=True)
        dev = tk._ids_flat.device
        rows_of = fusion.lims.fused_row_of().to(dev)
        w_out = max(entries, k + w)      # (k + w columns at the least: the selection then never runs short of entries, holes included)
        neg_inf, no_id = torch.full((), float("-inf"), dtype=torch.float32, device=dev), torch.full((), -1, dtype=torch.int64, device=dev)
        for attempt in range(2):      # speculate on the fused scans, verify after everything is enqueued
            pending: list = []
            if own:
                cand = tk._coarse_topk_from_eq(eq, False, pending, tags=tags)
            else:
                cand = tk._candidates(eq, pending) if tags is None else tk._candidates(eq, pending, tags)
            union, _ = E.lists_union(cand.to(torch.int64), fusion.lims, N, out=torch.empty((U, w_out), dtype=torch.int64, device=dev))
            hole = union < 0
            safe = union.clamp_min(0)      # holes read item 0 and are overwritten below
            scores = tk._score_at(eng, qpack, S, safe.index_select(0, rows_of))
            fused = torch.where(hole, neg_inf, E.scores_fuse_rows(scores, fusion.lims, fusion.mode, fusion.weights))
            ids = torch.where(hole, no_id, tk._ids_flat[safe])
            if invalid_ids is None:
                out_s, out_i = E.topk(fused, k, ids=ids)
            elif E.topk_candidates_filterable(w_out, k + w, w, k):      # (the "positions" are the candidates' ids: no id table behind them)
                out_i, out_s = E.topk_candidates_filtered(fused, k + w, ids, None, invalid_ids, k)
            else:
                top_s, top_i = E.topk(fused, k + w, ids=ids)
                out_i, out_s = E.filter_seen_ids(top_i, top_s, invalid_ids, k)
            if _verdicts_clear(pending, tk):
                break
            tk._no_fused = True
        tk._no_fused = False
    tk.__dict__.setdefault("_fuse_candidate_stats", {"fused_candidate_calls": 0})["fused_candidate_calls"] += 1
    return out_s.to(query_embeddings.dtype), out_i


def _fused_candidate_stats(tk) -> Dict[str, int]:
    """fused_candidate_calls: the calls _fused_candidates answered so far; absent before the first one."""
    return dict(tk.__dict__.get("_fuse_candidate_stats", {}))


class MoLAvgTopK(MoLTopKModule):
    fuse_candidates = False       # True (set on an instance): forward, forward_filtered and get_top_k_outputs take query_lims= / fuse= / query_weights=
                                  # over the union of the sub-query rows' candidates; every other call refuses them as before
    DEVICE_REDO_BYTES = 1 << 30   # materialised score matrices up to this size are kept as the device-side redo buffer of a fused scan;
                                  # beyond it (a 125 M-item shard: 16 GB) the counts are read on the host after the call is enqueued --
    DEVICE_REDO_FREE_FRACTION = 0.0    # > 0: larger buffers too, when they fit this fraction of the free memory.  Measured on a full config-5 shard (16 GB
                                       # buffer, round 5): the dozen predicated no-op launches of the redo (grids sized for 125 M items) cost as much as the
                                       # host's look at the verdict word (0.884 ms per batch either way) and the stream overlap of submit / result is lost
                                       # (0.79 -> 0.85 ms pipelined): off

    REDO_TOPK_TWO_LAUNCHES = 49152 * 24576      # n * K' up to which the predicated redo's top-K' is two launches (rails_topk's two-level plan: chunks of
                                                # <= 49 152 scores, <= 24 576 winners' keys); beyond it the radix route's nine

    def _device_redo_fits(self, nbytes: int, n_items: Optional[int] = None) -> bool:
        """May a (B, N) redo buffer of `nbytes` live on the device?  Decided once per size (the buffer is recycled across calls).
        n_items: the redo also has to be SHORT when it does not run -- every predicated launch of it is a 4.7 us no-op behind each call, and a
        top-K' beyond the two-level plan is nine of them (amzn-books, K' = 4 000: 47 us of a 0.28 ms call); such calls leave the verdict to
        the host (its look costs less than that)."""
        if n_items is not None and n_items * self._avg_top_k > self.REDO_TOPK_TWO_LAUNCHES:
            return False
        if nbytes <= self.DEVICE_REDO_BYTES:
            return True
        if self.DEVICE_REDO_BYTES <= 0 or self.DEVICE_REDO_FREE_FRACTION <= 0.0:     # tests: "as if it did not fit"
            return False
        memo = self._redo_fit_memo
        if nbytes not in memo:
            free, _ = torch.cuda.mem_get_info(self._item_embeddings.device)
            memo[nbytes] = nbytes <= self.DEVICE_REDO_FREE_FRACTION * free
        return memo[nbytes]

    """Two-pass approximate top-k (reference rails/indexing/mol_top_k.py:296-429): a bf16 dot product of the
    P_Q-summed query components against the P_X-averaged item components picks `avg_top_k` candidates per query,
    which are then scored with the full MoL and cut to k.  Spans keep the reference's profiler names."""

    def __init__(self, mol_module: MoLSimilarity, item_embeddings: torch.Tensor, item_ids: torch.Tensor, avg_top_k: int) -> None:
        _refuse_generic_route(mol_module, type(self).__name__)
        super().__init__(mol_module=mol_module, item_embeddings=item_embeddings, item_ids=item_ids)
        self._avg_top_k: int = avg_top_k
        self.fused_coarse_min_items: int = 262144    # below this the (B, N) scores are small and one launch chain shorter
        self._coarse_engine = None
        self._coarse_table = None
        self._coarse_prefilter = None
        self._side_streams = None
        self._side_turn = 0
        self._prefilter_calls = 0                 # scans that looked at the int8 copy (the schedule of its statistics check)
        self._prefilter_pending = None            # (pinned copy of the header's counts, its event) on its way to the host
        self._redo_fit_memo: Dict[int, bool] = {} # _device_redo_fits by buffer size

    def _check_collapsible(self, what: str) -> None:
        _generic_takes_no_groups(self, what)

    def _check_diversifiable(self, what: str) -> None:
        _generic_takes_no_vectors(self, what)

    OVERLAP_BATCHES = True            # submit(): speculative calls alternate between two streams of the module (see submit)
    PREFILTER_MIN_ITEMS = 4_000_000   # the int8 copy of the coarse table pays where the streaming pass is bound by HBM reads

    def _table(self) -> torch.Tensor:
        eng = self._bind()
        if self._coarse_engine is not eng:
            self._coarse_engine = eng
            self._coarse_table = eng.build_coarse_table(self._index, self._item_embeddings[0])
            self._coarse_prefilter = eng.build_coarse_prefilter(self._coarse_table) if self._coarse_table.shape[0] >= self.PREFILTER_MIN_ITEMS else None
        return self._coarse_table

    # ---- in-place corpus changes: the coarse table and its int8 copy ------------------------------------------------------------------
    # The int8 copy has ONE scale for the whole table: rebuilt whole from the edited table (one streaming pass over N rows, the one O(N) step of
    # an update) while N is at the threshold, dropped below it, with its statistics and their check schedule as for a fresh table -- a copy
    # dropped for its statistics comes back.  After a removal that left no holes nothing is refreshed: the copy is then rebuilt as the edit settles.
    def _coarse_held(self, eng) -> bool:
        return self._coarse_engine is eng and self._coarse_table is not None

    def _coarse_resize(self, eng, n_new: int) -> None:
        self._coarse_table, self._coarse_prefilter = E.resized(self._coarse_table, n_new), None

    def _coarse_refresh(self, eng, pos: torch.Tensor, emb: torch.Tensor) -> None:
        eng.update_coarse_table(self._coarse_table, pos, self._table_source(eng, emb))
        self._coarse_prefilter = None
        self._coarse_settle(eng)

    def _coarse_settle(self, eng) -> None:
        if self._coarse_prefilter is None and self._coarse_table.shape[0] >= self.PREFILTER_MIN_ITEMS:
            self._coarse_prefilter = eng.build_coarse_prefilter(self._coarse_table)
        self._prefilter_calls = 0
        self._prefilter_pending = None

    def _coarse_drop(self) -> None:
        self._coarse_engine = self._coarse_table = self._coarse_prefilter = None

    _HELD = (
        Held(("_coarse_table", "_coarse_prefilter"), _coarse_held, _coarse_resize, _coarse_refresh, _coarse_drop, _coarse_settle),
        Held(("_redo_fit_memo",), lambda tk, eng: True, lambda tk, eng, n: tk._redo_fit_memo.clear(), None, lambda tk: tk._redo_fit_memo.clear()),
    )

    PREFILTER_MAX_FIRED = 0.35        # fraction of (tile, query tile) blocks passing the integer bound beyond which the copy is dropped
    PREFILTER_CHECK_CALLS = (2, 64)   # the header's statistics are read (16 bytes, one sync) after this many calls, then every so many

    def _prefilter(self, count: bool = True) -> Optional[torch.Tensor]:
        """The int8 copy of the coarse table (None: not built, or dropped).  count = False: a look that is not a scan (statistics, bench
        probes) and must not advance the check schedule."""
        self._table()
        pre = self._coarse_prefilter
        if pre is not None and count:
            # a table whose one scale is set by a few outliers makes most tiles pass the bound: still exact, but the pass then reads
            # both copies.  The select scans keep (fired, tested) counts in the header; looked at now and then -- WITHOUT a host wait:
            # the 16 bytes are copied to pinned memory behind the launches already enqueued and read by a later call, once the copy
            # has landed (a blocking read here stalled the submit / result pipeline on call 3 and on every 64th call)
            self._prefilter_calls += 1
            pend = self._prefilter_pending
            first, every = self.PREFILTER_CHECK_CALLS
            if pend is not None:
                if pend[1].query():
                    fired, tested = (int(v) for v in pend[0])
                    self._prefilter_pending = None
                    if tested > 0 and fired > self.PREFILTER_MAX_FIRED * tested:
                        self._coarse_prefilter = pre = None
            elif self._prefilter_calls == first + 1 or self._prefilter_calls % every == 0:
                host = torch.empty(2, dtype=torch.int64).pin_memory()
                host.copy_(pre[32:48].view(torch.int64), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self._prefilter_pending = (host, ev)
        return pre

    def prefilter_stats(self) -> Optional[dict]:
        """(tile, query tile) blocks of the int8 select scans so far: how many passed the integer bound, how many were tested."""
        if self._coarse_prefilter is None:
            return None
        fired, tested = (int(v) for v in self._coarse_prefilter[32:48].view(torch.int64).cpu())
        return {"fired": fired, "tested": tested, "fraction": fired / tested if tested else 0.0}

    def _coarse_topk(self, query_embeddings: torch.Tensor, average_queries: bool, pending: Optional[list] = None, **kwargs):
        tags = self._take_allowed_tags(kwargs, query_embeddings.size(0), (self._avg_top_k,))      # (before any launch)
        eng = self._bind()
        table = self._table()
        qpack, eq, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"), want_plain=True)
        return qpack, self._coarse_topk_from_eq(eq, average_queries, pending, tags=tags)

    def _coarse_topk_from_eq(self, eq: torch.Tensor, average_queries: bool, pending: Optional[list] = None, with_scores: bool = False,
                             tags: Optional[E.TagFilter] = None):
        """(B, P_Q, d) query components -> (B, avg_top_k) positions of the coarse top-K', best first
        (with_scores: -> (scores, positions), the bf16 coarse scores as fp32).
        The coarse scan's entry to _speculative_scan, which holds the flow: `pending` (a list) DEFERS the fused scan's verdict to the caller."""
        eng, table, k = self._bind(), self._table(), self._avg_top_k
        n = table.shape[0]

        def launch(eq, flag, **restriction):
            out = eng.coarse_topk(eq, table, average_queries, k, with_flag=True, prefilter=self._prefilter(), flag=flag, **restriction)
            return None if out is None else (out[0], out[1], out[3])

        scan = CandidateScan(
            n=n, k=k, rows_per_query=1, route=lambda batch, restr: self._scan_route(False, batch, n, k, restr),
            width=lambda allowed: 128,      # the scan keeps ceil(B / 32) query tiles in LDS
            launch=launch, scores=lambda eq, out=None, run_if=None: eng.coarse_scores(eq, table, average_queries, out=out, run_if=run_if),
            redo_buffer="coarse_all", redo_on_device=lambda batch: self._device_redo_fits(batch * n * 4, n),
            device_flag=lambda: None,       # the tail of the launch's own counts
            shaped=lambda pos, batch: pos)
        return _speculative_scan(self, scan, eq, self._restriction(tags), pending, with_scores)

    def rerank(self, qpack: torch.Tensor, batch: int, cand_idx: torch.Tensor, k: int):
        """Full MoL on per-row candidates (positions, (B, K')) -> exact top-min(k, K') among them."""
        eng = self._bind()
        scores = self._score_at(eng, qpack, batch, cand_idx)
        return E.topk_candidates(scores, min(k, cand_idx.shape[1]), cand_idx, self._ids_flat)

    def _enqueue(self, query_embeddings: torch.Tensor, k: int, pending: list, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """One pass of forward's launches; the verdict words of the fused scan (int32 in pinned host memory, 1 = redo) are appended to `pending`."""
        # the reference's four profiler spans (mol_top_k.py:350-382), around the launches that do the same work here (entered only
        # under a profiler: a span costs ~9 us of host time, four of them more than the GPU needs for the launches they bracket)
        span = torch.profiler.record_function if torch.autograd._profiler_enabled() else (lambda name: contextlib.nullcontext())
        with span("avg_top_k_scoring"):
            qpack, idx = self._coarse_topk(query_embeddings, average_queries=False, pending=pending, **kwargs)
        eng = self._bind()
        with span("avg_topk_selection"):
            pass    # the reference gathers the candidates' embeddings here; they are read in place by the scoring launch below
        with span("filtered_scoring"):
            cand_scores = self._score_at(eng, qpack, query_embeddings.size(0), idx)
        with span("final_topk"):
            scores, ids = E.topk_candidates(cand_scores, min(k, idx.shape[1]), idx, self._ids_flat)   # top-k + gather + id lookup, one launch
        return scores.to(query_embeddings.dtype), ids

    # ---- two-stage form of forward ---------------------------------------------------------------------------------------------
    # The fused coarse scan is exact unless a candidate count left its range (heavy ties at the threshold), which only the device
    # knows when the launches are enqueued.  forward() = result(submit()): submit enqueues the whole call on that assumption and
    # records an event behind it; result waits for THAT event (not for the stream) to read the scan's verdict word, and redoes
    # the call on the materialising path in the rare other case.  A caller with the next batch at hand calls submit(batch i + 1)
    # before result(batch i): the host's look at the verdict then costs the GPU nothing (bench.py --two-pass reports both rates).
    # The handle submit() returns is OPAQUE: the tensors inside it may still be in flight on a stream of the module's own and are
    # joined to the caller's stream only by result() -- read them through result(), never through the handle, and do not drop a handle
    # without calling result() (ShardedTopK.submit, which needs the scores earlier, waits on the handle's event explicitly).
    def submit(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs):
        refuse_diversity(self, kwargs, "submit")
        if _asks_collapse(kwargs) and (m := self._take_collapse(kwargs)):      # (the walk over the reranked candidates; result owns the redo)
            return ("collapsed", self._collapse_enqueue(query_embeddings, k, None, kwargs, m))
        refuse_item_mask(self, kwargs)
        if kwargs.get("allowed_tags") is not None:      # allowed_tags=, resolved and checked before any launch; the handle and a
            kwargs["allowed_tags"] = self._take_allowed_tags(kwargs, query_embeddings.size(0), (self._avg_top_k,))      # redo carry the resolved filter
        if k > self._avg_top_k:  # the reference raises after doing the work (mol_top_k.py:383-386)
            raise ValueError(f"avg_top_k ({self._avg_top_k}) must be larger than k ({k})")
        # Calls that will be speculative (the (B, N) redo buffer does not fit: large shards) alternate between two streams of the
        # module's own: the latency-bound launches of one batch (prologue, sample, threshold, key selection, rerank: ~0.15 ms of
        # a 0.85 ms call on a 125 M-item shard) then run under the table scan of the neighbouring batch.  The caller's stream joins
        # a call's stream in result().  Calls that share the module's redo buffers (small corpora) stay on the caller's stream.
        side = None
        if self.OVERLAP_BATCHES and query_embeddings.is_cuda and not self._device_redo_fits(query_embeddings.size(0) * self.num_items * 4, self.num_items):
            if self._side_streams is None:
                self._side_streams = [torch.cuda.Stream(query_embeddings.device), torch.cuda.Stream(query_embeddings.device)]
            side = self._side_streams[self._side_turn]
            self._side_turn ^= 1
            side.wait_stream(torch.cuda.current_stream(query_embeddings.device))     # the inputs are ready where the caller stands
            query_embeddings.record_stream(side)
            for v in kwargs.values():          # user_ids and the like: read on the call's stream after the caller may have let go of them
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(side)
        pending: list = []
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()), self.one_bind():
            scores, ids = self._enqueue(query_embeddings, k, pending, **kwargs)
            host = list(pending) or None       # the verdict words, in pinned host memory (written by the scans themselves): nothing to copy
            done = torch.cuda.Event() if (pending or side is not None) else None
            if done is not None:
                done.record()
        if not pending and side is None:
            return ("final", scores, ids)
        return ("speculative", scores, ids, host, done, query_embeddings, k, kwargs, side)

    def _collapse_enqueue(self, query_embeddings: torch.Tensor, k: int, invalid_ids: Optional[torch.Tensor], kwargs: dict, m: int = 1):
        """The collapsed call over this module's own ranked list: MoLAvgTopK's avg_top_k reranked candidates; a subclass with its own forward
        (MoLCombTopK) has that forward rank its union."""
        own = type(self).forward is MoLAvgTopK.forward
        if own and k > self._avg_top_k:
            raise ValueError(f"avg_top_k ({self._avg_top_k}) must be larger than k ({k})")
        return _collapsed_candidates(self, query_embeddings, k, invalid_ids, self._avg_top_k if own else 0, kwargs, m)

    def result(self, handle) -> Tuple[torch.Tensor, torch.Tensor]:
        if handle[0] == "collapsed":
            return _collapsed_candidates_result(handle[1])
        if handle[0] == "final":
            return handle[1], handle[2]
        _, scores, ids, host, done, query_embeddings, k, kwargs, side = handle
        if side is not None:           # the caller's stream takes over the outputs
            cur = torch.cuda.current_stream(scores.device)
            cur.wait_event(done)
            scores.record_stream(cur)
            ids.record_stream(cur)
        redo = False
        if host is not None:
            while not done.query():      # spin: the word is microseconds away, and a blocking wait parks the thread on an interrupt whose
                pass                     # wake-up costs 50-100 us of GPU idle per batch (see MoLBruteForceTopK._read_stats)
            redo = any(int(w.numpy()[0]) != 0 for w in host)
            _release_words(self, host)
        if not redo:
            return scores, ids
        self._no_fused = True      # redo this call on the materialising path
        try:
            return self._enqueue(query_embeddings, k, [], **kwargs)
        finally:
            self._no_fused = False

    def stats(self) -> Dict[str, int]:
        """fused_candidate_calls once a call has been fused over the candidate union (fuse_candidates = True), score_of_calls / explain_calls
        once a pair-level call has been made; empty before."""
        return {**_fused_candidate_stats(self), **self.pair_stats()}

    def _diversified(self, query_embeddings: torch.Tensor, k: int, invalid_ids: Optional[torch.Tensor], kwargs: dict, div):
        """The diversified call over this module's own ranked list: MoLAvgTopK's avg_top_k reranked candidates; a
        subclass with its own forward (MoLCombTopK) has that forward rank its union.  -> (scores, ids) in pick order."""
        own = type(self).forward is MoLAvgTopK.forward
        if own and k > self._avg_top_k:
            raise ValueError(f"avg_top_k ({self._avg_top_k}) must be larger than k ({k})")
        return _diversified_candidates(self, query_embeddings, k, invalid_ids, self._avg_top_k if own else 0, kwargs, div)

    def forward(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """diversify=lam: the avg_top_k reranked candidates re-ranked by maximal marginal relevance -- k columns in PICK
        order, each with the item's own score, so a row is not monotone.  query_lims= (section 3.20; fuse_candidates = True): one result row per
        segment of query rows, over the union of their candidates."""
        if _asks_fusion(self, kwargs):
            return _fused_candidates(self, "forward", query_embeddings, k, None, kwargs)
        if _asks_diversity(kwargs) and (div := self._take_diversity(kwargs)) is not None:
            return self._diversified(query_embeddings, k, None, kwargs, div)
        with self.inline_calls():      # nothing to overlap with: stay on the caller's stream (the hand-over between streams costs ~50 us)
            return self.result(self.submit(query_embeddings, k, sorted, **kwargs))

    def forward_filtered(self, query_embeddings: torch.Tensor, k_prime: int, invalid_ids: torch.Tensor, k: int, **kwargs):
        """CandidateIndex.get_top_k_outputs' body: forward(k_prime) + the seen-id filter, with the filter enqueued BEFORE the host looks
        at the scan's verdict word (it then runs while the host is on its way back) -> (top_k_ids, top_k_scores); None where this
        does not apply (subclasses with their own forward, k_prime beyond K': the caller composes the two calls).  collapse_groups=True never
        returns None: the seen ids go to the collapse walk.  Nor does a fused call (query_lims=, fuse_candidates = True): the seen ids are per
        fused row and filter the one ranking of the union."""
        if _asks_fusion(self, kwargs):
            scores, ids = _fused_candidates(self, "forward_filtered", query_embeddings, k, invalid_ids, kwargs)
            return ids, scores
        if _asks_diversity(kwargs) and (div := self._take_diversity(kwargs)) is not None:      # (never None: the seen ids go to the walk)
            scores, ids = self._diversified(query_embeddings, k, invalid_ids, kwargs, div)
            return ids, scores
        if _asks_collapse(kwargs) and (m := self._take_collapse(kwargs)):
            scores, ids = _collapsed_candidates_result(self._collapse_enqueue(query_embeddings, k, invalid_ids, kwargs, m))
            return ids, scores
        refuse_item_mask(self, kwargs)
        if type(self).forward is not MoLAvgTopK.forward or k_prime > self._avg_top_k or k_prime < k:
            return None
        with self.inline_calls():
            h = self.submit(query_embeddings, k_prime, **kwargs)
        out = E.filter_seen_ids(h[2], h[1], invalid_ids, k)
        scores, ids = self.result(h)
        return out if scores is h[1] else E.filter_seen_ids(ids, scores, invalid_ids, k)

    @contextlib.contextmanager
    def inline_calls(self):
        """submit() inside this block stays on the caller's stream (what a plain forward wants)."""
        saved = self.OVERLAP_BATCHES
        self.OVERLAP_BATCHES = False
        try:
            yield
        finally:
            self.OVERLAP_BATCHES = saved

    def coarse_candidates(self, query_embeddings: torch.Tensor, **kwargs):
        """Pass 1 on this module's items: -> (coarse scores (B, K'), positions (B, K')), best first (ties by position)."""
        refuse_collapse_groups(self, kwargs, "coarse_candidates")
        refuse_diversity(self, kwargs, "coarse_candidates")
        refuse_query_fusion(self, kwargs, "coarse_candidates")
        refuse_allowed_tags(self, kwargs, "coarse_candidates is the item-sharded wrappers' hand-off, and a tag filter is not built on them; forward, submit "
                            "and topk_ids take it")
        eng = self._bind()
        _, eq, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"), want_plain=True)
        return self._coarse_topk_from_eq(eq, False, None, with_scores=True)

    def rerank_masked(self, query_embeddings: torch.Tensor, cand_idx: torch.Tensor, k: int, **kwargs):
        """Pass 2 on a candidate list with holes: positions < 0 are not this module's items; they score -inf and come back
        with id -1.  -> exact top-min(k, K') (scores, ids)."""
        eng = self._bind()
        qpack, _, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"))
        hole = cand_idx < 0
        scores = self._score_at(eng, qpack, query_embeddings.size(0), cand_idx.clamp_min(0))   # holes read item 0 and are overwritten below
        scores = torch.where(hole, scores.new_full((), float("-inf")), scores)
        ids = torch.where(hole, cand_idx.new_full((), -1), self._ids_flat[cand_idx.clamp_min(0)])
        return E.topk(scores, min(k, cand_idx.shape[1]), ids=ids)

    def topk_ids(self, query_embeddings: torch.Tensor, sorted: bool = True, **kwargs) -> torch.Tensor:
        """Coarse candidates only, with the P_Q-averaged query (reference mol_top_k.py:398-429) -> positions."""
        refuse_collapse_groups(self, kwargs, "topk_ids")
        refuse_diversity(self, kwargs, "topk_ids")
        refuse_query_fusion(self, kwargs, "topk_ids")
        return self._coarse_topk(query_embeddings, average_queries=True, **kwargs)[1]


class _ComponentCandidates:
    """Per-component candidate generation, the rerank of the union and the two-attempt forward shared by MoLNaiveTopK and MoLCombTopK, which
    supply _candidates(eq, pending) -> (B, _union_width()) positions.  Mixed in BEFORE the MoL base class: its forward / forward_filtered are
    the modules' own."""

    fuse_candidates = False                # as MoLAvgTopK.fuse_candidates
    fused_component_min_items = 262144     # below this the (B * P_Q * P_X, N) component scores are small and one launch chain shorter
    NO_FILTER_FUSION = False               # tests: True keeps the seen-id filter out of the selection launch

    def __init__(self, **kwargs) -> None:
        super().__init__(**kwargs)
        self._comp_engine = None
        self._comp_table = None

    def forward(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """All the union's candidates ranked, whatever `k` is, as the reference does.  collapse_groups=True: the first k
        of that ranking with at most one item per group of set_item_groups -- k columns.  query_lims= (section 3.20; fuse_candidates = True):
        one result row per segment of query rows, over the union of their candidates -- k columns."""
        if _asks_fusion(self, kwargs):
            return _fused_candidates(self, "forward", query_embeddings, k, None, kwargs)
        if _asks_diversity(kwargs) and (div := self._take_diversity(kwargs)) is not None:      # (k columns in pick order)
            return _diversified_candidates(self, query_embeddings, k, None, 0, kwargs, div)
        if _asks_collapse(kwargs) and (m := self._take_collapse(kwargs)):
            return _collapsed_candidates_result(_collapsed_candidates(self, query_embeddings, k, None, 0, kwargs, m))
        scores, ids = self._ranked(query_embeddings, sorted, None, kwargs)
        return scores.to(query_embeddings.dtype), ids

    def forward_filtered(self, query_embeddings: torch.Tensor, k_prime: int, invalid_ids: torch.Tensor, k: int, **kwargs):
        """CandidateIndex.get_top_k_outputs' body (the module returns all its candidates whatever k_prime is, the filter keeps the first k unseen):
        -> (top_k_ids, top_k_scores), or None where the filter does not fit the selection launch (_filter_inside).  collapse_groups=True never
        returns None: the seen ids go to the collapse walk, over the sorted form of the ranking.  Nor does a fused call (query_lims=,
        fuse_candidates = True)."""
        if _asks_fusion(self, kwargs):
            scores, ids = _fused_candidates(self, "forward_filtered", query_embeddings, k, invalid_ids, kwargs)
            return ids, scores
        if _asks_diversity(kwargs) and (div := self._take_diversity(kwargs)) is not None:      # (never None: the seen ids go to the walk)
            scores, ids = _diversified_candidates(self, query_embeddings, k, invalid_ids, 0, kwargs, div)
            return ids, scores
        refuse_query_fusion(self, kwargs)
        if _asks_collapse(kwargs) and (m := self._take_collapse(kwargs)):
            scores, ids = _collapsed_candidates_result(_collapsed_candidates(self, query_embeddings, k, invalid_ids, 0, kwargs, m))
            return ids, scores
        seen = self._filter_inside(self._union_width(), invalid_ids, k)
        if seen is None:
            return None
        ids, scores = self._ranked(query_embeddings, True, seen, kwargs)
        return ids, scores.to(query_embeddings.dtype)

    def stats(self) -> Dict[str, int]:
        """fused_candidate_calls once a call has been fused over the candidate union (fuse_candidates = True), score_of_calls / explain_calls
        once a pair-level call has been made; empty before."""
        return {**_fused_candidate_stats(self), **self.pair_stats()}

    def _ranked(self, query_embeddings: torch.Tensor, sorted: bool, seen, kwargs):
        refuse_item_mask(self, kwargs)
        tags = self._take_allowed_tags(kwargs, query_embeddings.size(0), _tag_ks(self))      # allowed_tags=, before any launch
        eng = self._bind()
        qpack, eq, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"), want_plain=True)
        for attempt in range(2):     # speculate on the fused scans, verify after everything is enqueued
            pending: list = []
            all_indices = self._candidates(eq, pending) if tags is None else self._candidates(eq, pending, tags)
            out = self._rerank_union(qpack, query_embeddings.size(0), all_indices, sorted, seen, pending)
            if _verdicts_clear(pending, self):
                break
            self._no_fused = True
        self._no_fused = False
        return out

    UNION_CAP = 16384          # candidates per query the rerank sorts and ranks in one workgroup's LDS (rails_sort_rows_i64 / rails_topk)
    UNION_HARD_CAP = 1 << 20   # beyond UNION_CAP (16x16x64 with k_per_group >= 75: 256 * 75 = 19 200) the two integer / float sorts of the
                               # rerank go through torch.sort on the device -- the reference "just runs" there (mol_top_k.py:260, :518);
                               # scoring and duplicate masking stay on the HIP kernels

    def _check_union_size(self, n_candidates: int) -> None:
        if n_candidates > self.UNION_HARD_CAP:
            raise NotImplementedError(
                f"{type(self).__name__}: {n_candidates} candidates per query exceed the rerank capacity of {self.UNION_HARD_CAP} "
                "(P_Q * P_X * k_per_group [+ avg_top_k]); use a smaller k_per_group for this shape")

    def _component_table(self) -> torch.Tensor:
        eng = self._bind()
        if self._comp_engine is not eng:
            self._comp_engine = eng
            self._comp_table = eng.build_component_table(self._index, self._item_embeddings[0])
        return self._comp_table

    # ---- in-place corpus changes: the component table (item-group-major: one row per group and position; a resize re-lays it to group stride n_new)
    def _comp_drop(self) -> None:
        self._comp_engine = self._comp_table = None

    _HELD = (
        Held(("_comp_table",), lambda tk, eng: tk._comp_engine is eng and tk._comp_table is not None,
             lambda tk, eng, n: setattr(tk, "_comp_table", E.resized(tk._comp_table, n, dim=1)),
             lambda tk, eng, pos, emb: eng.update_component_table(tk._comp_table, pos, tk._table_source(eng, emb)), _comp_drop),
    )

    def _component_topk(self, eq: torch.Tensor, k_per_group: int, pending: Optional[list] = None, with_scores: bool = False,
                        tags: Optional[E.TagFilter] = None):
        """-> (B, P_Q * P_X * k_per_group) positions: top k_per_group items of every (query group, item group) pair.
        The component scan's entry to _speculative_scan, which holds the flow: `pending` (a list) DEFERS the fused scan's verdict to the caller.
        with_scores: -> (scores, positions), both (B * P_Q * P_X, k_per_group), best first: the bf16 component scores as fp32."""
        eng, table = self._bind(), self._component_table()      # (P_X, N, d), item-group-major
        n, k = table.shape[1], k_per_group
        pq, px = eng.spec.query_dot_product_groups, eng.spec.item_dot_product_groups
        # the scans keep the fragments of all B * P_Q query rows in LDS and (the fused form) eight row tiles of running maxima in registers (four
        # at d = 128): 256 (128) query rows per call; the tagged sample keeps four row tiles at every d (its eight-tile form would spill)
        plain_rows = 128 if eng.table_width >= 128 else 256      # (the width the scans run at: d, or the generic route's padded width)

        def launch(eq, flag, **restriction):      # (flag: zeroed by the call's first launch)
            out = eng.component_topk(eq, table, k, flag, **restriction)
            return None if out is None else (out[0], out[1], flag)

        scan = CandidateScan(
            n=n, k=k, rows_per_query=pq * px, route=lambda batch, restr: self._scan_route(True, batch, n, k, restr),
            width=lambda allowed: max(1, (E.TAGGED_COMPONENT_ROWS if tags is not None and allowed else plain_rows) // pq),
            launch=launch, scores=lambda eq, out=None, run_if=None: eng.component_scores(eq, table, out=out, run_if=run_if),
            # (the limit is MoLAvgTopK's, read from the class: MoLNaiveTopK is no Avg module; 5.7 GB of scores at amzn-books, B = 32, leave the verdict to the host)
            redo_buffer="component_all", redo_on_device=lambda batch: batch * pq * px * n * 4 <= MoLAvgTopK.DEVICE_REDO_BYTES,
            device_flag=lambda: self._buf("redo_flag_c", 1, torch.int32),
            shaped=lambda pos, batch: pos.view(batch, -1))
        return _speculative_scan(self, scan, eq, self._restriction(tags), pending, with_scores)

    # ---- the two halves of _ranked on their own, for the item-sharded global form (sharded.ShardedMoLNaiveTopK / ShardedMoLCombTopK) -----------
    def _candidates_scored(self, eq: torch.Tensor, pending: list):
        """_candidates with the scores that ranked them: -> (group scores, group positions[, coarse scores, coarse positions])."""
        raise NotImplementedError

    def local_candidates(self, query_embeddings: torch.Tensor, **kwargs):
        """Local candidates with scores: the per-group top-k_per_group of THIS module's items as (scores, positions), both
        (B * P_Q * P_X, k_per_group), best first under (score desc, position asc) -- and for MoLCombTopK the averaged-query coarse top-K'
        (scores, positions), both (B, K'), behind them.  Scores are the scans' bf16 values as fp32.  VERIFIED before it returns: the fused
        scans are enqueued speculatively, their verdict words read once (the one host look of the single-device call), and a failed verdict
        redoes the scans on the materialising path -- what comes back is exact."""
        refuse_collapse_groups(self, kwargs, "local_candidates")
        refuse_diversity(self, kwargs, "local_candidates")
        refuse_query_fusion(self, kwargs, "local_candidates")
        refuse_allowed_tags(self, kwargs, "local_candidates is the item-sharded wrappers' hand-off, and a tag filter is not built on them; forward and "
                            "get_top_k_outputs take it")
        eng = self._bind()
        _, eq, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"), want_plain=True)
        for attempt in range(2):
            pending: list = []
            out = self._candidates_scored(eq, pending)
            if _verdicts_clear(pending, self):
                break
            self._no_fused = True
        self._no_fused = False
        return out

    def rerank_union_masked(self, query_embeddings: torch.Tensor, union_idx: torch.Tensor, k: int, **kwargs):
        """Rerank a union with holes: union_idx (B, W) positions of this module's items, < 0 where a candidate is another shard's.  The same
        chain as _rerank_union -- sort, full MoL, duplicates (the second and later copies of an owned position) masked with -32767.0 -- with
        the holes scoring -inf, carrying id -1 and never counting as a duplicate of anything.  -> the top-min(k, W) (scores fp32, ids), ties by
        position ascending.  No host synchronisation."""
        eng = self._bind()
        qpack, _, _ = eng.query_pack(query_embeddings, kwargs.get("user_ids"))
        W = union_idx.shape[1]
        big = W > self.UNION_CAP
        sorted_idx = torch.sort(union_idx.to(torch.int64), dim=1).values if big else E.sort_rows(union_idx)     # holes first
        hole = sorted_idx < 0
        safe = sorted_idx.clamp_min(0)                  # holes read item 0 and are overwritten below
        scores = self._score_at(eng, qpack, query_embeddings.size(0), safe)
        E.mask_sorted_duplicates(sorted_idx, scores, -32767.0)      # (on the unclamped positions: the first owned item 0 is no copy of a hole)
        scores = torch.where(hole, scores.new_full((), float("-inf")), scores)
        ids = torch.where(hole, sorted_idx.new_full((), -1), self._ids_flat[safe])
        if big and min(k, W) > self.UNION_CAP:
            vals, order = torch.sort(scores, dim=1, descending=True, stable=True)
            return vals[:, : min(k, W)].contiguous(), torch.gather(ids, 1, order)[:, : min(k, W)].contiguous()
        return E.topk(scores, min(k, W), ids=ids)

    def _filter_inside(self, n_candidates: int, invalid_ids: torch.Tensor, k: int):
        """get_top_k_outputs over a module that returns ALL its candidates ranked (masked duplicates last): the first k unseen entries of that
        list are the first k unseen of its top k + width -- at most `width` scored candidates are seen, and a masked duplicate (-32767.0)
        outranks a scored one only where fewer than k + width scored ones exist, in both forms alike.  -> (invalid_ids, k) where
        rails_topk_candidates_filtered takes the sizes, else None (the caller ranks everything and filters after)."""
        if invalid_ids is None or invalid_ids.dim() != 2 or self.NO_FILTER_FUSION:
            return None
        width = invalid_ids.shape[1]
        if not E.topk_candidates_filterable(n_candidates, min(k + width, n_candidates), width, k):
            return None
        return (invalid_ids, k)

    UNSORTED_RERANK = True     # get_top_k_outputs: rank the candidates where the scans left them (rails_rerank_topk_filtered) instead of sorting their positions first

    def _rerank_union(self, qpack: torch.Tensor, batch: int, all_indices: torch.Tensor, sorted: bool, seen=None, pending: Optional[list] = None):
        """sort -> gather -> full MoL -> mask duplicates with -32767.0 -> top-k over ALL candidates
        (the reference overwrites k with the candidate count, mol_top_k.py:260 / :518).
        seen = (invalid_ids, k) (get_top_k_outputs, sizes checked by the caller): instead of the full ranking, the first k unseen entries of it
        -- the top k + width of the candidates with the seen-id filter inside the selection launch -> (ids, scores).  Where the fused scans'
        verdict word is pending anyway (pinned host memory, read by the caller once everything is enqueued), the integer sort goes too: the
        candidates are scored in the order the scans left them and ranked by (score, position) keys, first copy of every position; a row with
        fewer than k + width distinct positions raises the same word and the call is redone on the sorted form."""
        eng = self._bind()
        big = all_indices.shape[1] > self.UNION_CAP
        word = pending[0] if pending else None
        if seen is not None and word is not None and self.UNSORTED_RERANK and not self._no_fused:
            invalid_ids, k_out = seen
            pos = all_indices.to(torch.int64).contiguous()
            scores = self._score_at(eng, qpack, batch, pos)
            ws = self._buf("rerank_keys", pos.numel() * 8, torch.uint8)
            return E.rerank_topk_filtered(scores, min(k_out + invalid_ids.shape[1], pos.shape[1]), pos, self._ids_flat, invalid_ids, k_out, word, ws)
        sorted_idx = torch.sort(all_indices.to(torch.int64), dim=1).values if big else E.sort_rows(all_indices)
        k = sorted_idx.shape[1]
        scores = self._score_at(eng, qpack, batch, sorted_idx)
        E.mask_sorted_duplicates(sorted_idx, scores, -32767.0)
        if seen is not None:
            invalid_ids, k_out = seen
            return E.topk_candidates_filtered(scores, min(k_out + invalid_ids.shape[1], k), sorted_idx, self._ids_flat, invalid_ids, k_out)
        if big:   # full ranking of more than 16 384 candidates: stable descending sort = (score desc, column asc), rails_topk's tie rule
            vals, order = torch.sort(scores, dim=1, descending=True, stable=True)
            return vals, torch.gather(self._ids_flat[sorted_idx], 1, order)
        return E.topk_candidates(scores, k, sorted_idx, self._ids_flat)


class MoLNaiveTopK(_ComponentCandidates, MoLTopKModule):
    """Reference rails/indexing/mol_top_k.py:133-293.  Returns (B, P_Q * P_X * k_per_group) columns whatever `k` is, as the reference does.
    use_faiss=True (the reference's FAISS-GPU branch, :176-239): the per-group candidates come from a native IVF-Flat index
    (engine.IvfIndex) built at the first call -- nlist lists per item group, nprobe of them searched per query component -- instead of the
    exhaustive component scan; nlist / nprobe / iters / seed (keyword-only, not in the reference's signature) default to FAISS's values.
    ivf_centroids: a (P_X, nlist, d) fp32 tensor on the module's device -- the index is built from a copy of it, nothing is trained.
    frozen_centroids=True (use_faiss=True only) opts in to the in-place corpus API: update_items / append_items /
    remove_items and the by-id calls edit the lists under the centroids the index has, which are never written again -- as FAISS's
    IndexIVFFlat.add / remove_ids.  The contract is NOT "equals a freshly constructed module" (a fresh module trains new centroids): after any
    sequence of calls the lists are bit for bit what rails_ivf_build_lists writes from the resulting table with THOSE centroids.  Recall may
    drift as the corpus moves away from them: watch ivf_index().list_sizes(), and construct the module again to retrain.
    filtered_lists=True (use_faiss=True only; independent of frozen_centroids) opts in to the hidden set and the item tags (DESIGN sections
    3.14 and 3.15) INSIDE the list scan: hide_items / unhide_items and their by-id forms, hidden_positions, set_item_tags and allowed_tags= on
    forward, get_top_k_outputs and all_logits; compact() is a removal and needs frozen_centroids=True as well.  Row b of a call equals row b of
    the same call on MoLNaiveTopK(mol, X[keep_b], ids[keep_b], k_per_group, use_faiss=True, ivf_centroids=<these centroids>, ...), keep_b the
    items row b may return; a row that keeps fewer than nlist items is that module's ValueError, fewer than k_per_group its RuntimeError.
    The index keeps one more int32 per list entry (P_X * 4 bytes per item) from the first filtered call on.  item_mask= stays refused."""

    def __init__(self, mol_module: MoLSimilarity, item_embeddings: torch.Tensor, item_ids: torch.Tensor, k_per_group: int, use_faiss: bool = False,
                 *, nlist: int = 100, nprobe: int = 1, iters: int = 10, seed: int = 1234, frozen_centroids: bool = False,
                 ivf_centroids: Optional[torch.Tensor] = None, filtered_lists: bool = False) -> None:
        _refuse_generic_route(mol_module, type(self).__name__)
        if use_faiss:
            refuse_generic_candidates(mol_module, "MoLNaiveTopK: the IVF index (use_faiss=True)", "the exhaustive MoLNaiveTopK runs there")
        super().__init__(mol_module=mol_module, item_embeddings=item_embeddings, item_ids=item_ids)
        self._k_per_group: int = k_per_group
        self._use_faiss: bool = bool(use_faiss)
        self._frozen_centroids: bool = bool(frozen_centroids)
        if self._frozen_centroids and not self._use_faiss:
            raise ValueError("MoLNaiveTopK: frozen_centroids=True applies to the IVF index of use_faiss=True only")
        self._filtered_lists: bool = bool(filtered_lists)
        if self._filtered_lists and not self._use_faiss:
            raise ValueError("MoLNaiveTopK: filtered_lists=True applies to the IVF index of use_faiss=True only")
        self._ivf_args = dict(nlist=int(nlist), nprobe=int(nprobe), iters=int(iters), seed=int(seed))
        self.nprobe: int = int(nprobe)      # lists searched per query component; may be changed between calls (the index stays)
        self._ivf: Optional[E.IvfIndex] = None
        self._ivf_engine = None
        self._check_union_size(mol_module._query_dot_product_groups * mol_module._item_dot_product_groups * k_per_group)
        if self._use_faiss:   # the limits, before any build or launch
            if not 1 <= self._ivf_args["nlist"] <= 4096:
                raise NotImplementedError(f"MoLNaiveTopK: nlist = {nlist} outside [1, 4096]")
            if not 1 <= self._ivf_args["nprobe"] <= min(64, self._ivf_args["nlist"]):
                raise NotImplementedError(f"MoLNaiveTopK: nprobe = {nprobe} outside [1, min(64, nlist)]")
            if not 1 <= k_per_group <= 128:
                raise NotImplementedError(f"MoLNaiveTopK: use_faiss=True takes k_per_group in [1, 128], got {k_per_group}")
            if mol_module._dot_product_dimension not in (32, 64, 128):
                raise NotImplementedError(f"MoLNaiveTopK: use_faiss=True takes dot_product_dimension in {{32, 64, 128}}, got {mol_module._dot_product_dimension}")
            if self.num_items < self._ivf_args["nlist"]:
                raise ValueError(f"MoLNaiveTopK: {self.num_items} items cannot fill nlist = {nlist} lists")
        if ivf_centroids is not None:
            want = (mol_module._item_dot_product_groups, self._ivf_args["nlist"], mol_module._dot_product_dimension)
            if (not torch.is_tensor(ivf_centroids) or tuple(ivf_centroids.shape) != want or ivf_centroids.dtype != torch.float32
                    or ivf_centroids.device != item_embeddings.device):
                raise ValueError(f"MoLNaiveTopK: ivf_centroids must be a {want} float32 tensor on {item_embeddings.device}")
            self._ivf_args["centroids"] = ivf_centroids.detach().clone()      # (the caller's tensor is never aliased)

    def __setattr__(self, name, value):
        if name == "fuse_candidates" and value and getattr(self, "_use_faiss", False):
            raise NotImplementedError("MoLNaiveTopK (IVF, use_faiss=True) takes no fuse_candidates: the candidate union is built on the exhaustive "
                                      "component scan; the exhaustive MoLNaiveTopK takes it")
        super().__setattr__(name, value)

    def _check_updatable(self, what: str, n_left: Optional[int] = None) -> None:
        if self._use_faiss and not self._frozen_centroids:
            raise NotImplementedError(f"MoLNaiveTopK.{what}: the IVF index (use_faiss=True) is trained on the corpus -- its lists and centroids do not follow "
                                      "an in-place change; construct the module again (or with frozen_centroids=True: the lists then follow under the "
                                      "centroids the index has)")
        if self._use_faiss and n_left is not None and 0 < n_left < self._ivf_args["nlist"]:      # (the constructor's refusal; n_left < 1 is removal_plan's)
            raise ValueError(f"MoLNaiveTopK: {n_left} items cannot fill nlist = {self._ivf_args['nlist']} lists")

    def _check_hideable(self, what: str) -> None:
        if self._use_faiss and not getattr(self, "_filtered_lists", False):
            raise NotImplementedError(f"MoLNaiveTopK.{what}: the IVF index (use_faiss=True{', frozen_centroids=True' if self._frozen_centroids else ''}) searches "
                                      "its lists without a visibility test -- a hidden set is not built for it; remove_items (under frozen_centroids=True) "
                                      "deletes for good, and the exhaustive MoLNaiveTopK takes hide_items")

    # ---- in-place corpus changes under frozen centroids: the lists of a held index follow, behind every other buffer -----------------------
    def _ivf_resize(self, eng, n_new: int) -> None:
        if n_new < self._ivf.n_items:       # a pure truncation; growth is a no-op (refresh inserts the positions the old lists do not hold)
            self._ivf.edit(torch.empty(0, dtype=torch.int64, device=self._item_embeddings.device), None, n_keep=n_new)

    def _ivf_refresh(self, eng, pos: torch.Tensor, emb: torch.Tensor) -> None:
        self._ivf.edit(pos, self._table_source(eng, emb), n_keep=self.num_items, items=self._item_embeddings[0])

    def _ivf_drop(self) -> None:
        self._ivf = self._ivf_engine = None

    _HELD = (Held(("_ivf",), lambda tk, eng: tk._ivf is not None and tk._ivf_engine is eng, _ivf_resize, _ivf_refresh, _ivf_drop),)

    def ivf_index(self) -> E.IvfIndex:
        """The IVF index of use_faiss=True, built at first use and rebuilt when _bind() yields a new engine (as _component_table)."""
        eng = self._bind()
        if self._ivf_engine is not eng:
            self._ivf = None      # free the old lists before the new ones are built
            self._ivf = E.IvfIndex(eng, self._index, items=self._item_embeddings[0], **self._ivf_args)
            self._ivf_engine = eng
        return self._ivf

    def _candidates(self, eq: torch.Tensor, pending: list, tags: Optional[E.TagFilter] = None) -> torch.Tensor:
        if self._use_faiss:       # exact by construction over the probed lists: nothing to verify, nothing added to `pending`
            # filtered_lists: the call's tag filter, else the hidden set, goes INTO the list scan (a module without the flag holds neither)
            filt = (tags if tags is not None else self._visible) if self._filtered_lists else None
            return self.ivf_index().search(eq, self._k_per_group, nprobe=self.nprobe, filter=filt)
        # (tags travel as a keyword only when there are any: tests/test_gpu_parity.py swaps _component_topk for a stand-in of the (eq, k, pending) form)
        return self._component_topk(eq, self._k_per_group, pending, **({} if tags is None else {"tags": tags}))

    def _check_collapsible(self, what: str) -> None:
        _generic_takes_no_groups(self, what)
        if self._use_faiss:
            raise NotImplementedError(f"MoLNaiveTopK (IVF, use_faiss=True) takes no {what}: collapsing by item group is not built on the IVF index; the "
                                      "exhaustive MoLNaiveTopK takes it")

    def _check_diversifiable(self, what: str) -> None:
        _generic_takes_no_vectors(self, what)
        if self._use_faiss:
            raise NotImplementedError(f"MoLNaiveTopK (IVF, use_faiss=True) takes no {what}: diversifying by maximal marginal relevance is not built on "
                                      "the IVF index; the exhaustive MoLNaiveTopK takes it")

    def _check_taggable(self, what: str) -> None:
        if self._use_faiss and not getattr(self, "_filtered_lists", False):
            raise NotImplementedError(f"MoLNaiveTopK takes no {what}: the IVF index (use_faiss=True{', frozen_centroids=True' if self._frozen_centroids else ''}) "
                                      "searches its lists without a tag test -- a tag filter is not built for it; the exhaustive MoLNaiveTopK takes it")

    def _candidates_scored(self, eq: torch.Tensor, pending: list):
        if self._use_faiss:
            raise NotImplementedError("MoLNaiveTopK: the IVF lists return no exhaustive per-group ranking to exchange (use_faiss=True)")
        return self._component_topk(eq, self._k_per_group, pending, with_scores=True)

    def _union_width(self) -> int:
        mol = self._mol_module
        return mol._query_dot_product_groups * mol._item_dot_product_groups * self._k_per_group


class MoLCombTopK(_ComponentCandidates, MoLAvgTopK):
    """Reference rails/indexing/mol_top_k.py:432-551: per-component candidates + the averaged-query coarse
    candidates, reranked together.  Returns (B, P_Q * P_X * k_per_group + avg_top_k) columns."""

    def __init__(self, mol_module: MoLSimilarity, item_embeddings: torch.Tensor, item_ids: torch.Tensor, avg_top_k: int, k_per_group: int) -> None:
        super().__init__(mol_module=mol_module, item_embeddings=item_embeddings, item_ids=item_ids, avg_top_k=avg_top_k)
        self._k_per_group: int = k_per_group
        self._check_union_size(mol_module._query_dot_product_groups * mol_module._item_dot_product_groups * k_per_group + avg_top_k)

    def _union_width(self) -> int:
        mol = self._mol_module
        return mol._query_dot_product_groups * mol._item_dot_product_groups * self._k_per_group + self._avg_top_k

    def _candidates(self, eq: torch.Tensor, pending: list, tags: Optional[E.TagFilter] = None) -> torch.Tensor:
        comp = self._component_topk(eq, self._k_per_group, pending, **({} if tags is None else {"tags": tags}))      # (as in MoLNaiveTopK._candidates)
        avg_idx = self._coarse_topk_from_eq(eq, average_queries=True, pending=pending, tags=tags)
        return torch.cat([comp, avg_idx], dim=1)

    def _candidates_scored(self, eq: torch.Tensor, pending: list):
        gs, gp = self._component_topk(eq, self._k_per_group, pending, with_scores=True)
        cs, cp = self._coarse_topk_from_eq(eq, average_queries=True, pending=pending, with_scores=True)
        return gs, gp, cs, cp


class MIPSTopKModule(TopKModule):
    """Reference rails/indexing/mips_top_k.py:23-38."""

    def __init__(self, item_embeddings: torch.Tensor, item_ids: torch.Tensor) -> None:
        super().__init__()
        self._item_embeddings: torch.Tensor = item_embeddings
        self._item_ids: torch.Tensor = item_ids


class MIPSBruteForceTopK(_CorpusEdits, MIPSTopKModule):
    """Dot-product brute force (reference rails/indexing/mips_top_k.py:41-81): MFMA scan + exact top-k, all HIP."""

    def __init__(self, item_embeddings: torch.Tensor, item_ids: torch.Tensor) -> None:
        super().__init__(item_embeddings=item_embeddings, item_ids=item_ids)
        if item_embeddings.dim() != 3 or item_embeddings.shape[0] != 1:
            raise ValueError(f"item_embeddings must be (1, N, D), got {tuple(item_embeddings.shape)}")
        del self._item_embeddings
        self._table_dtype = item_embeddings.dtype      # (what update_items / append_items take; the index holds fp32 copies)
        self._index = E.MipsIndex(item_embeddings[0])
        self._ids_flat = item_ids.reshape(-1).to(device=item_embeddings.device, dtype=torch.int64).contiguous()
        self._flag_free: list = []    # pinned verdict words ready for reuse (_pinned_word: the collapse walk's)

    def forward(self, query_embeddings: torch.Tensor, k: int, sorted: bool = True, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """item_mask= (an engine.ItemMask or a bool tensor (N,) / (B, N)): only items inside the mask are returned -- the
        dense strategy: the score matrix of the items outside it is set to -inf before the selection.  collapse_groups=True (section 3.16): at
        most one item per group of set_item_groups.  query_lims= (section 3.20): one result row per segment of query rows.  diversify=lam (section
        3.21; diversity_pool=D): the head of the ranking re-ranked by maximal marginal relevance against set_item_vectors -- k columns in PICK
        order, each with the item's own score, so a row is not monotone."""
        if _asks_diversity(kwargs) and (div := self._take_diversity(kwargs)) is not None:      # (results in pick order)
            return _diversified_exact(self, query_embeddings, k, None, kwargs, div)
        if (fusion := self._resolve_fusion(kwargs, query_embeddings, "forward")) is not None:
            ids, scores = self._fused_topk("forward", query_embeddings, k, None, fusion, kwargs, sorted)
            return scores.to(query_embeddings.dtype), ids
        if _asks_collapse(kwargs) and (m := self._take_collapse(kwargs)):
            return _collapsed_exact(self, query_embeddings, k, None, kwargs, m)
        mask = self._take_item_mask(kwargs, query_embeddings.size(0), k)
        logits = self._index.score(query_embeddings)
        if mask is not None:
            E.scores_mask(logits, mask)
        scores, ids = E.topk(logits, k, ids=self._ids_flat, sorted=sorted)
        return scores.to(query_embeddings.dtype), ids

    def forward_filtered(self, query_embeddings: torch.Tensor, k_prime: int, invalid_ids: torch.Tensor, k: int, **kwargs):
        """CandidateIndex.get_top_k_outputs' body under collapse_groups=True -> (top_k_ids, top_k_scores): the seen ids go to the collapse walk.
        So under query_lims= (section 3.20): the seen ids are per fused row.  None for every other call (the caller composes forward +
        filter_seen_ids, as it always has)."""
        if _asks_diversity(kwargs) and (div := self._take_diversity(kwargs)) is not None:      # (never None: the seen ids go to the walk)
            scores, ids = _diversified_exact(self, query_embeddings, k, invalid_ids, kwargs, div)
            return ids, scores
        if (fusion := self._resolve_fusion(kwargs, query_embeddings, "forward_filtered")) is not None:
            ids, scores = self._fused_topk("forward_filtered", query_embeddings, k_prime, (invalid_ids, k), fusion, kwargs)
            return ids, scores.to(query_embeddings.dtype)
        if _asks_collapse(kwargs) and (m := self._take_collapse(kwargs)):
            scores, ids = _collapsed_exact(self, query_embeddings, k, invalid_ids, kwargs, m)
            return ids, scores
        return None

    def stats(self) -> Dict[str, int]:
        """Which route answered the fused calls so far (fusion_stats), and score_of_calls once score_of has been called."""
        return {**self.fusion_stats(), **self.pair_stats()}

    def _rank_scores(self, query_embeddings: torch.Tensor, **kwargs) -> torch.Tensor:
        return self._index.score(query_embeddings)

    def _pair_scores(self, query_embeddings: torch.Tensor, positions: torch.Tensor, kwargs: dict) -> torch.Tensor:
        """score_of's hook: the dense scan's MFMA chain per pair, the items fetched by position."""
        return self._index.score_at(query_embeddings, positions)

    def _own_score_chunks(self, query_embeddings: torch.Tensor, mask: Optional[E.ItemMask], **kwargs):
        logits = self._index.score(query_embeddings)
        yield 0, logits if mask is None else E.scores_mask(logits, mask)

    # ---- in-place corpus changes (_CorpusEdits): the MoL modules' three calls -------------------------------------------------------------
    # The module keeps the tile-packed copy and the ids only: after any sequence of the calls _index.buf and _ids_flat are what a fresh module
    # built from the resulting table and ids holds (rails_mips_index_update stores the build's bytes at the positions; no arithmetic).  There
    # is no raw table to write (update_items writes the borrowed ids alone) and no choice of engines.  Rows are fp32 in the index whatever
    # the table's dtype was, so a mover's row read back from it is what a fresh build would convert again.
    @property
    def num_items(self) -> int:
        return self._index.n_items

    def _row_format(self) -> Tuple[int, torch.dtype]:
        return self._index.dim, self._table_dtype

    def _rows_at(self, pos: torch.Tensor) -> torch.Tensor:
        return self._index.rows(pos)

    _HELD = (Held(("_index",), lambda tk, eng: True, lambda tk, eng, n: tk._index.resize(n), lambda tk, eng, pos, emb: tk._index.update(pos, emb), None),)


class CandidateIndex(object):
    """Reference indexing/candidate_index.py:30-185 (`filter_invalid_ids` / `apply_object_filter` are never
    called by any entry point of the reference and are not provided)."""

    def __init__(self, ids: torch.Tensor, embeddings: torch.Tensor, invalid_ids: Optional[torch.Tensor] = None, debug_path: Optional[str] = None) -> None:
        super().__init__()
        self._ids: torch.Tensor = ids
        self._embeddings: torch.Tensor = embeddings
        self._invalid_ids: Optional[torch.Tensor] = invalid_ids
        self._debug_path: Optional[str] = debug_path

    @property
    def ids(self) -> torch.Tensor:
        return self._ids

    @property
    def num_objects(self) -> int:
        return self._ids.size(1)

    @property
    def embeddings(self) -> torch.Tensor:
        return self._embeddings

    def get_top_k_outputs(
        self,
        query_embeddings: torch.Tensor,
        k: int,
        aux_payloads: Dict[str, torch.Tensor],
        top_k_module: TopKModule,
        invalid_ids: Optional[torch.Tensor],
        r: int = 1,
        return_embeddings: bool = False,
        truncate_k_prime_to: Optional[int] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """-> (top_k_ids (B, k), top_k_scores (B, k), None).  Note: ids first, as in the reference."""
        bind = getattr(getattr(top_k_module, "_local_module", top_k_module), "one_bind", None)
        with bind() if bind is not None else contextlib.nullcontext():     # one look at the model's parameters per call (MoLTopKModule.one_bind)
            return self._get_top_k_outputs(query_embeddings, k, aux_payloads, top_k_module, invalid_ids, r, return_embeddings, truncate_k_prime_to)

    def _get_top_k_outputs(self, query_embeddings, k, aux_payloads, top_k_module, invalid_ids, r, return_embeddings, truncate_k_prime_to):
        if return_embeddings:
            # the reference's own branch is broken (undefined `top_k_indices`, candidate_index.py:182)
            raise NotImplementedError("return_embeddings=True is not supported")
        max_num_invalid_ids = invalid_ids.size(1) if invalid_ids is not None else 0
        k_prime = min(k + max_num_invalid_ids, self.num_objects)
        if truncate_k_prime_to is not None:
            k_prime = min(k_prime, truncate_k_prime_to)
        if invalid_ids is not None and k <= k_prime and hasattr(top_k_module, "forward_filtered"):
            fused = top_k_module.forward_filtered(query_embeddings, k_prime, invalid_ids, k, **aux_payloads)
            if fused is not None:
                return fused[0], fused[1], None
        top_k_prime_scores, top_k_prime_ids = top_k_module(query_embeddings=query_embeddings, k=k_prime, **aux_payloads)
        if invalid_ids is not None:
            if top_k_prime_ids.shape[1] < k:
                # the reference fails in .view(-1, k) here
                raise RuntimeError(f"shape '[-1, {k}]' is invalid: only {top_k_prime_ids.shape[1]} candidates per row")
            top_k_ids, top_k_scores = E.filter_seen_ids(top_k_prime_ids, top_k_prime_scores, invalid_ids, k)
        else:
            top_k_scores, top_k_ids = top_k_prime_scores, top_k_prime_ids
        return top_k_ids, top_k_scores, None


_BUILT = {"MoLBruteForceTopK": lambda mol, x, ids: MoLBruteForceTopK(mol_module=mol, item_embeddings=x, item_ids=ids)}
for _k in (5, 10, 25, 50, 75, 100):
    _BUILT[f"MoLNaiveTopK{_k}"] = (lambda kk: lambda mol, x, ids: MoLNaiveTopK(mol_module=mol, item_embeddings=x, item_ids=ids, k_per_group=kk))(_k)
for _kg, _ka in ((1, 100), (1, 500), (5, 100), (5, 200), (5, 500), (10, 100), (10, 500), (50, 500), (50, 1000), (100, 1000)):
    _BUILT[f"MoLCombTopK{_kg}_{_ka}"] = (lambda g, a: lambda mol, x, ids: MoLCombTopK(mol_module=mol, item_embeddings=x, item_ids=ids, avg_top_k=a, k_per_group=g))(_kg, _ka)
_NO_MOL = {"MIPSBruteForceTopK": lambda x, ids: MIPSBruteForceTopK(item_embeddings=x, item_ids=ids)}
for _k in (100, 200, 500, 1000, 2000, 2500, 3000, 4000):
    _BUILT[f"MoLAvgTopK{_k}"] = (lambda kk: lambda mol, x, ids: MoLAvgTopK(mol_module=mol, item_embeddings=x, item_ids=ids, avg_top_k=kk))(_k)
# accepted by the reference's factory, not mapped here yet: the IVF candidate generation itself is MoLNaiveTopK(..., use_faiss=True)
_KNOWN_UNBUILT = ["MoLNaiveFaissTopK5"]


def get_top_k_module(top_k_method: str, model: torch.nn.Module, item_embeddings: torch.Tensor, item_ids: torch.Tensor) -> TopKModule:
    """String -> module factory; `model._ndp_module` is the MoLSimilarity (reference indexing/utils_rails.py:25-233)."""
    if top_k_method in _NO_MOL:
        return _NO_MOL[top_k_method](item_embeddings, item_ids)
    if top_k_method in _BUILT:
        return _BUILT[top_k_method](model._ndp_module, item_embeddings, item_ids)
    if top_k_method in _KNOWN_UNBUILT:
        raise NotImplementedError(f"top_k_method {top_k_method} is not mapped by the factory yet; "
                                  "build MoLNaiveTopK(..., k_per_group=5, use_faiss=True) directly")
    raise ValueError(f"Invalid top-k method {top_k_method}")
