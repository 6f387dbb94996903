"""Plain numpy references of query fusion over the candidate union: the union of ragged candidate lists per fused row,
and the walk over it -- fuse the aligned columns, rank by the selection key, drop the seen ids.  Built on tests/_fuse_ref.py."""
import numpy as np

from tests import _fuse_ref as F


def union(positions, lims, n_items: int, w_out=None):
    """positions (S, W) int64 -> (out (U, w_out) int64, counts (U,) int32): per fused row the distinct positions of its segment inside
    [0, n_items) ascending, -1 behind them -- what rails_lists_union writes.  w_out: max_segment * W unless given."""
    positions = np.asarray(positions, dtype=np.int64)
    lims = F.check_lims(lims, positions.shape[0])
    U = lims.size - 1
    if w_out is None:
        w_out = int(np.diff(lims).max()) * positions.shape[1]
    out = np.full((U, w_out), -1, dtype=np.int64)
    counts = np.zeros(U, dtype=np.int32)
    for u in range(U):
        p = positions[lims[u] : lims[u + 1]].reshape(-1)
        distinct = np.unique(p[(p >= 0) & (p < n_items)])
        counts[u] = distinct.size
        out[u, : distinct.size] = distinct
    return out, counts


def walk(union_pos, counts, scores, lims, mode, weights, ids, k: int, invalid_ids=None):
    """The fused-candidate walk.  union_pos (U, W_out), counts (U,): the union; scores (S, W_out) float32: s[r, j] the score of sub-query row r at
    the position in column j of ITS fused row's union (columns beyond the count are ignored).  -> (ids (U, k) int64, scores (U, k) float32):
    the first k positions of every union in key order (fused score descending, position ascending) whose id is not among the row's
    invalid_ids, a short row padded with (-1, -inf)."""
    lims = F.check_lims(lims, scores.shape[0])
    fused = F.fuse(scores, lims, mode, weights)
    U = lims.size - 1
    out_i = np.full((U, k), -1, dtype=np.int64)
    out_s = np.full((U, k), -np.inf, dtype=np.float32)
    for u in range(U):
        c = int(counts[u])
        cols = np.asarray(union_pos[u, :c], dtype=np.int64)
        order = np.argsort(~F.keys_of(fused[u, :c], cols), kind="stable")      # (positions are distinct: so are the keys)
        seen = set() if invalid_ids is None else set(np.asarray(invalid_ids)[u].tolist())
        picked = [j for j in order.tolist() if int(ids[cols[j]]) not in seen][:k]
        out_i[u, : len(picked)] = ids[cols[picked]]
        out_s[u, : len(picked)] = fused[u, picked]
    return out_i, out_s
