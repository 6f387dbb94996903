"""The contract of rank_of in plain numpy, on the 64-bit selection key of tests/_topk_ref.keys:

    rank(b, x) = 1 + #{ y : eligible[b, y] and key(b, y) > key(b, x) }    if 0 <= x < N and eligible[b, x]
    rank(b, x) = 0                                                         otherwise ("not ranked": a target of -1, an ineligible one)

so rank - 1 is the index at which x stands in the descending sort of the row's eligible keys."""
import numpy as np

from tests import _topk_ref as R


def ranks(bits: np.ndarray, eligible: np.ndarray, targets: np.ndarray) -> np.ndarray:
    """bits (B, N) uint32 score bit patterns, eligible (B, N) bool, targets (B, T) integer positions -> (B, T) int64"""
    bits = np.asarray(bits, dtype=np.uint32)
    eligible = np.asarray(eligible, dtype=bool)
    targets = np.asarray(targets, dtype=np.int64)
    B, N = bits.shape
    assert eligible.shape == (B, N) and targets.ndim == 2 and targets.shape[0] == B
    out = np.zeros(targets.shape, dtype=np.int64)
    for b in range(B):
        kv = R.keys(bits[b])
        kept = np.sort(kv[eligible[b]])      # ascending; all keys of a row are distinct
        for j, x in enumerate(targets[b]):
            if 0 <= x < N and eligible[b, x]:
                out[b, j] = 1 + kept.shape[0] - np.searchsorted(kept, kv[x], side="right")
    return out

