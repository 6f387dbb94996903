"""Plain numpy references of query fusion: the fusion of an (S, n) float32 matrix by segments, and the merge of sorted
(score, position) lists."""
import numpy as np


def orderable(bits: np.ndarray) -> np.ndarray:
    """The codec of rails_amd/csrc/topk_keys.h on uint32 bit patterns: unsigned order = selection order."""
    bits = np.asarray(bits, dtype=np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def keys_of(scores: np.ndarray, positions: np.ndarray) -> np.ndarray:
    """(orderable(score) << 32) | ~position as uint64."""
    bits = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return (orderable(bits).astype(np.uint64) << np.uint64(32)) | (~np.asarray(positions).astype(np.uint32)).astype(np.uint64)


def check_lims(lims, rows: int) -> np.ndarray:
    lims = np.asarray(lims, dtype=np.int64)
    assert lims.ndim == 1 and lims.size >= 2 and lims[0] == 0 and lims[-1] == rows and (np.diff(lims) > 0).all(), lims
    return lims


def fuse(scores: np.ndarray, lims, mode: str = "max", weights=None) -> np.ndarray:
    """(S, n) float32 -> (U, n) float32, bit for bit what rails_scores_fuse_rows writes.  max: per column the element whose orderable bits
    are largest (no float compare).  sum: a float32 chain over the segment's rows ascending; with weights two roundings per term."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    lims = check_lims(lims, scores.shape[0])
    out = np.empty((lims.size - 1, scores.shape[1]), dtype=np.float32)
    if weights is not None:
        assert mode == "sum"
        weights = np.asarray(weights, dtype=np.float32)
    with np.errstate(all="ignore"):
        for u in range(lims.size - 1):
            seg = scores[lims[u] : lims[u + 1]]
            if mode == "max":
                best = np.argmax(orderable(seg.view(np.uint32)), axis=0)      # (equal keys are equal bits)
                out[u] = seg[best, np.arange(seg.shape[1])]
            else:
                assert mode == "sum"
                w = None if weights is None else weights[lims[u] : lims[u + 1]]
                acc = seg[0].copy() if w is None else (w[0] * seg[0]).astype(np.float32)
                for r in range(1, seg.shape[0]):
                    term = seg[r] if w is None else (w[r] * seg[r]).astype(np.float32)
                    acc = (acc + term).astype(np.float32)
                out[u] = acc
    return out


def merge_lists(scores: np.ndarray, positions: np.ndarray, lims, k: int, ids=None, invalid_ids=None, n_items=None):
    """The list merge: per fused row, the entries (position in [0, n_items), score not -inf) deduplicated by position keeping the largest key,
    sorted by key descending, without those whose id is among the row's invalid_ids, the first k -> (ids (U, k) int64, scores (U, k)
    float32), a short row padded with (-1, -inf)."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    positions = np.asarray(positions, dtype=np.int64)
    lims = check_lims(lims, scores.shape[0])
    if n_items is None:
        n_items = len(ids)
    U = lims.size - 1
    out_i = np.full((U, k), -1, dtype=np.int64)
    out_s = np.full((U, k), -np.inf, dtype=np.float32)
    for u in range(U):
        s = scores[lims[u] : lims[u + 1]].reshape(-1)
        p = positions[lims[u] : lims[u + 1]].reshape(-1)
        keep = (p >= 0) & (p < n_items) & ~(s == -np.inf)
        best = {}
        for key, pos, sc in zip(keys_of(s[keep], p[keep]).tolist(), p[keep].tolist(), s[keep]):
            if pos not in best or key > best[pos][0]:
                best[pos] = (key, sc)
        seen = set() if invalid_ids is None else set(np.asarray(invalid_ids)[u].tolist())
        j = 0
        for pos, (key, sc) in sorted(best.items(), key=lambda e: -e[1][0]):
            item = pos if ids is None else int(ids[pos])
            if item in seen:
                continue
            if j == k:
                break
            out_i[u, j], out_s[u, j] = item, sc
            j += 1
    return out_i, out_s


def topk_walk(fused: np.ndarray, eligible: np.ndarray, ids: np.ndarray, k: int, invalid_ids=None):
    """The first k eligible-and-unseen items of every row of a fused matrix in selection-key order -> (ids (U, k), scores (U, k))."""
    U, n = fused.shape
    out_i = np.full((U, k), -1, dtype=np.int64)
    out_s = np.full((U, k), -np.inf, dtype=np.float32)
    for u in range(U):
        cols = np.nonzero(eligible[u])[0]
        order = cols[np.argsort(~keys_of(fused[u, cols], cols), kind="stable")]      # (keys are distinct: descending key order)
        seen = set() if invalid_ids is None else set(np.asarray(invalid_ids)[u].tolist())
        picked = [x for x in order.tolist() if int(ids[x]) not in seen][:k]
        out_i[u, : len(picked)] = ids[picked]
        out_s[u, : len(picked)] = fused[u, picked]
    return out_i, out_s
