"""The reference of max_per_group=m, in plain Python / torch, written from the semantics alone:

  order all eligible items of a row by (score descending, position ascending) -- _collapse_ref.key_order;
  an item SURVIVES iff it is ungrouped (key -1) or fewer than m earlier eligible items of that order carry its group key;
  the result is the first k survivors.

An item is eligible iff its score is not -inf (what a mask, a hidden set or a tag filter leave) and its id is not in the row's invalid ids.
A seen item is not eligible: it neither counts against its group's quota nor fills a slot of it."""
import numpy as np
import torch

from tests._collapse_ref import key_order


def quota_walk(scores, positions_order, groups, invalid, ids, k, m):
    """scores (N,) fp32 by position; positions_order: the ranking, a sequence of positions; groups (N,) integer keys (-1: ungrouped); invalid: the
    row's invalid ids (any iterable) or None; ids (N,) by position, or None (a position is its own id); k; m >= 1.
    -> (scores, positions, ids) of the first k survivors as Python lists: fewer than k entries where the ranking holds fewer survivors."""
    assert m >= 1
    sc = scores.detach().cpu().tolist()
    gr = groups.detach().cpu().tolist()
    idl = None if ids is None else ids.detach().cpu().reshape(-1).tolist()
    seen_ids = set() if invalid is None else set(torch.as_tensor(invalid).reshape(-1).tolist())
    taken = {}
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
            if taken.get(g, 0) >= m:
                continue
            taken[g] = taken.get(g, 0) + 1
        out_s.append(sc[p])
        out_p.append(p)
        out_i.append(item_id)
    return out_s, out_p, out_i


def quota_topk(logits, groups, invalid_ids, ids, k, m):
    """quota_walk over every row of a (B, N) score matrix, each ordered by key_order -> (scores (B, k) fp32, ids (B, k) int64) on the CPU;
    None where some row has fewer than k survivors (the call then raises)."""
    logits = logits.detach().float().cpu()
    rows_s, rows_i = [], []
    for b in range(logits.shape[0]):
        s, _, i = quota_walk(logits[b], key_order(logits[b]), groups, None if invalid_ids is None else invalid_ids[b].cpu(), ids, k, m)
        if len(i) < k:
            return None
        rows_s.append(torch.tensor(s, dtype=torch.float32))
        rows_i.append(torch.tensor(i, dtype=torch.int64))
    return torch.stack(rows_s), torch.stack(rows_i)


# ---- the host model of the fallback's round table --------------------------------------------------------------------------------------
def int_keys(scores, first_item=0):
    """(rows, n) fp32 scores -> the selection keys of topk_keys.h as Python-int objects (an unsigned 64-bit key does not fit int64):
    (orderable(score) << 32) | ~position."""
    s = np.ascontiguousarray(scores.detach().cpu().numpy(), dtype=np.float32)
    bits = s.view(np.uint32).astype(np.uint64)
    ordered = np.where(bits >= np.uint64(1 << 31), np.uint64(0xFFFFFFFF) - bits, bits + np.uint64(1 << 31))
    pos = np.arange(first_item, first_item + s.shape[1], dtype=np.uint64)
    return (ordered << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - pos)[None, :]


def round_table(scores, ranks, n_groups, m, ids=None, invalid=None, first_item=0):
    """The table rails_scores_group_next leaves after m rounds, by numpy: (rows, m, n_groups) uint64, [b, t, r] the key of rank r's (t + 1)-th
    best ELIGIBLE item of row b -- finite score (the eligibility of the group-maxima kernel), id not among the row's invalid ids --, 0 where the
    group has fewer.  ranks: (>= first_item + n,) dense ranks by position; ids by position or None."""
    s = scores.detach().cpu().numpy().astype(np.float32)
    rows, n = s.shape
    keys = int_keys(scores, first_item)
    rk = ranks.detach().cpu().numpy().astype(np.int64)[first_item : first_item + n]
    idn = np.arange(first_item, first_item + n) if ids is None else ids.detach().cpu().numpy().reshape(-1)[first_item : first_item + n]
    table = np.zeros((rows, m, n_groups), dtype=np.uint64)
    for b in range(rows):
        ok = np.isfinite(s[b])
        if invalid is not None:
            ok &= ~np.isin(idn, invalid[b].detach().cpu().numpy())
        cols = np.nonzero(ok)[0]
        cols = cols[np.argsort(keys[b, cols], kind="stable")[::-1]]      # eligible columns, best key first (keys are distinct)
        filled = np.zeros(n_groups, dtype=np.int64)
        for c in cols.tolist():
            r = rk[c]
            if filled[r] < m:
                table[b, filled[r], r] = keys[b, c]
                filled[r] += 1
    return table


def table_topk(table, k):
    """(rows, m, G) uint64 round table -> per row the (score bits as fp32, position) of its k largest non-zero keys, descending."""
    out = []
    for b in range(table.shape[0]):
        flat = table[b].reshape(-1)
        flat = np.sort(flat[flat != 0])[::-1][:k]
        ordered = (flat >> np.uint64(32)).astype(np.uint32)
        bits = np.where(ordered >= np.uint32(1 << 31), ordered - np.uint32(1 << 31), np.uint32(0xFFFFFFFF) - ordered).astype(np.uint32)
        pos = (np.uint64(0xFFFFFFFF) - (flat & np.uint64(0xFFFFFFFF))).astype(np.int64)
        out.append((bits.view(np.float32).tolist(), pos.tolist()))
    return out
