"""The reference of the collapsed top-k, in plain Python / torch, written from the semantics alone:

  order all eligible items of a row by (score descending, position ascending);
  the collapsed top-k is the first k items of that order whose group key is -1 or differs from the key of every earlier item of the order.

An item is eligible iff its score is not -inf (what a mask, a hidden set or a tag filter leave) and its id is not in the row's invalid ids."""
import torch


def key_order(scores: torch.Tensor) -> torch.Tensor:
    """(N,) fp32 scores by position -> the positions ordered by (score desc, position asc), in exact integer arithmetic: the scores' bit
    patterns mapped to integers that order as the floats do, sorted descending by a STABLE sort over the ascending positions."""
    bits = scores.detach().cpu().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    ordered = torch.where(bits >= 1 << 31, 0xFFFFFFFF - bits, bits + (1 << 31))
    return torch.sort(ordered, descending=True, stable=True).indices


def collapse_walk(scores, positions_order, groups, invalid, ids, k):
    """scores (N,) fp32 by position; positions_order: the ranking, a sequence of positions; groups (N,) integer keys (-1: ungrouped); invalid: the
    row's invalid ids (any iterable) or None; ids (N,) by position, or None (a position is its own id); k.
    -> (scores, positions, ids) of the collapsed top-k as Python lists: k entries, fewer where the ranking holds fewer eligible groups."""
    sc = scores.detach().cpu().tolist()
    gr = groups.detach().cpu().tolist()
    idl = None if ids is None else ids.detach().cpu().reshape(-1).tolist()
    seen_ids = set() if invalid is None else set(torch.as_tensor(invalid).reshape(-1).tolist())
    taken = set()
    out_s, out_p, out_i = [], [], []
    for p in torch.as_tensor(positions_order).reshape(-1).tolist():
        if len(out_p) == k:
            break
        if sc[p] == float("-inf"):
            continue
        item_id = p if idl is None else idl[p]
        if item_id in seen_ids:
            continue
        g = gr[p]
        if g >= 0:
            if g in taken:
                continue
            taken.add(g)
        out_s.append(sc[p])
        out_p.append(p)
        out_i.append(item_id)
    return out_s, out_p, out_i


def collapsed_topk(logits, groups, invalid_ids, ids, k):
    """collapse_walk over every row of a (B, N) score matrix, each ordered by key_order -> (scores (B, k) fp32, ids (B, k) int64) on the CPU;
    None where some row has fewer than k eligible groups (the call then raises)."""
    logits = logits.detach().float().cpu()
    rows_s, rows_i = [], []
    for b in range(logits.shape[0]):
        s, _, i = collapse_walk(logits[b], key_order(logits[b]), groups, None if invalid_ids is None else invalid_ids[b].cpu(), ids, k)
        if len(i) < k:
            return None
        rows_s.append(torch.tensor(s, dtype=torch.float32))
        rows_i.append(torch.tensor(i, dtype=torch.int64))
    return torch.stack(rows_s), torch.stack(rows_i)
