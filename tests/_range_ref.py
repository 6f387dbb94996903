"""The range-search contract restated in numpy on tests/_topk_ref.keys.

A row is its uint32 score bit patterns.  Item x of row b is a HIT when it is eligible and v >= t[b] as an IEEE fp32 compare (false with a NaN on
either side), v = the score in the score form, v = fl32(fl32(score * beta) - lse[b]) in the log-probability form -- the lse bits are INPUT here: the
reference of log_partition is tests/_softmax_ref.py, not this file.  The ragged result is FAISS-shaped: lims (B + 1,), and per row the hits'
score bits and positions, in selection-key order (keys descending: score descending, then position ascending, on the bits) or in position order.
"""
from __future__ import annotations

import numpy as np

from tests import _topk_ref as R

F32 = np.float32


def thresholds(t, rows: int) -> np.ndarray:
    """a number or a (rows,) array -> (rows,) fp32, converted once"""
    with np.errstate(over="ignore"):      # (a number beyond fp32 becomes +-inf, as on the device side)
        return np.broadcast_to(np.asarray(t, dtype=F32), (rows,)).copy()


def values(bits: np.ndarray, beta=None, lse=None) -> np.ndarray:
    """what is compared with the threshold: (rows, n) fp32"""
    s = np.ascontiguousarray(bits, dtype=np.uint32).view(F32)
    if lse is None:
        return s
    with np.errstate(all="ignore"):
        y = (s * F32(beta)).astype(F32)                      # one rounded fp32 multiply ...
        return (y - np.asarray(lse, dtype=F32)[:, None]).astype(F32)      # ... then one rounded subtraction: never an fma


def hit_mask(bits: np.ndarray, eligible, t, beta=None, lse=None) -> np.ndarray:
    """(rows, n) bool"""
    bits = np.atleast_2d(bits)
    rows = bits.shape[0]
    with np.errstate(invalid="ignore"):
        passing = values(bits, beta, lse) >= thresholds(t, rows)[:, None]      # (numpy's >= is the IEEE one: False with a NaN)
    return passing & np.broadcast_to(np.asarray(eligible, dtype=bool), bits.shape)


def counts(bits, eligible, t, beta=None, lse=None) -> np.ndarray:
    return hit_mask(bits, eligible, t, beta, lse).sum(axis=1).astype(np.int64)


def ragged(bits, eligible, t, beta=None, lse=None, sort: bool = True, ids=None):
    """-> (lims (rows + 1,) int64, score bits (total,) uint32, ids (total,) int64: positions without an id table)"""
    bits = np.atleast_2d(np.ascontiguousarray(bits, dtype=np.uint32))
    hits = hit_mask(bits, eligible, t, beta, lse)
    lims = np.zeros(bits.shape[0] + 1, dtype=np.int64)
    s_out, p_out = [], []
    for r in range(bits.shape[0]):
        pos = np.flatnonzero(hits[r])
        if sort:
            kv = np.sort(R.keys(bits[r])[pos])[::-1]
            s, pos = R.decode(kv)
            assert np.array_equal(s, bits[r][pos])
        s_out.append(bits[r][pos])
        p_out.append(pos.astype(np.int64))
        lims[r + 1] = lims[r] + pos.shape[0]
    p_all = np.concatenate(p_out) if p_out else np.zeros(0, dtype=np.int64)
    s_all = np.concatenate(s_out) if s_out else np.zeros(0, dtype=np.uint32)
    return lims, s_all.astype(np.uint32), (p_all if ids is None else np.asarray(ids, dtype=np.int64)[p_all])


def threshold_for(bits_row: np.ndarray, eligible_row, count: int) -> np.float32:
    """the fp32 threshold that exactly `count` eligible items of a NaN-free row with distinct values meet: the count-th largest eligible value"""
    v = np.sort(bits_row.view(F32)[np.asarray(eligible_row, dtype=bool)])[::-1]
    return F32(np.inf) if count == 0 else v[count - 1]
