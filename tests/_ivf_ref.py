"""CPU restatement (numpy, float64 on the fp16-rounded components) of the IVF-Flat index behind MoLNaiveTopK(use_faiss=True)
(rails_amd/csrc/ivf.hip, include/rails_amd.h rails_ivf_*): the seeded sample, the spherical Lloyd step with the deterministic split of
empty lists, the list build and the search with the short-list rule.  Ties: the lower list id; top-k by score desc, position asc."""
import numpy as np
import torch

SPLIT_EPS = 1.0 / 1024.0


def sample_positions(n: int, nlist: int, seed: int = 1234) -> np.ndarray:
    gen = torch.Generator().manual_seed(int(seed))
    return torch.randperm(n, generator=gen)[: min(n, 256 * nlist)].numpy().astype(np.int64)


def scores(x: np.ndarray, c: np.ndarray) -> np.ndarray:
    return np.asarray(x, np.float64) @ np.asarray(c, np.float64).T


def assign(x: np.ndarray, c: np.ndarray):
    """-> (argmax list (ties to the lower id), gap between the two best centroid scores)."""
    s = scores(x, c)
    a = np.argmax(s, axis=1)
    if s.shape[1] > 1:
        top2 = -np.partition(-s, 1, axis=1)[:, :2]
        gap = top2[:, 0] - top2[:, 1]
    else:
        gap = np.full(s.shape[0], np.inf)
    return a, gap


def lloyd_step(xs: np.ndarray, c: np.ndarray) -> np.ndarray:
    """One iteration: assign, per-list means, split empty lists off the largest one (ascending, ties to the lower id), normalise."""
    nlist, d = c.shape
    a, _ = assign(xs, c)
    sizes = np.bincount(a, minlength=nlist).astype(np.float64)
    new = np.zeros((nlist, d), np.float64)
    np.add.at(new, a, np.asarray(xs, np.float64))
    nz = sizes > 0
    new[nz] /= sizes[nz, None]
    sign = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    for ci in range(nlist):
        if sizes[ci] != 0:
            continue
        cj = int(np.argmax(sizes))
        v = new[cj].copy()
        new[ci] = v * (1 + sign * SPLIT_EPS)
        new[cj] = v * (1 - sign * SPLIT_EPS)
        sizes[ci] = sizes[cj] / 2
        sizes[cj] -= sizes[ci]
    return new / np.linalg.norm(new, axis=1, keepdims=True)


def train(xs: np.ndarray, nlist: int, iters: int) -> np.ndarray:
    c = np.asarray(xs[:nlist], np.float64)
    for _ in range(iters):
        c = lloyd_step(xs, c)
    return c


def build_lists(x: np.ndarray, c: np.ndarray):
    """-> (positions in list order (stable), offsets (nlist + 1,))."""
    a, _ = assign(x, c)
    order = np.argsort(a, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=c.shape[0]))])
    return order, offsets


def probe_order(q: np.ndarray, c: np.ndarray, offsets: np.ndarray, nprobe: int, k: int):
    """Lists probed for query component q: best centroid scores first, nprobe of them, more while they hold fewer than k items.
    -> (lists, centroid scores sorted desc)."""
    s = scores(q[None], c)[0]
    order = np.lexsort((np.arange(len(s)), -s))
    sizes = np.diff(offsets)
    taken, held = [], 0
    for l in order:
        taken.append(int(l))
        held += int(sizes[l])
        if len(taken) >= nprobe and held >= k:
            break
    return taken, s[order]


def search_row(q: np.ndarray, x16: np.ndarray, c: np.ndarray, order: np.ndarray, offsets: np.ndarray, nprobe: int, k: int):
    """-> (positions (k,), their scores, the candidate set's scores by position) for one (query component, item group)."""
    lists, _ = probe_order(q, c, offsets, nprobe, k)
    cand = np.concatenate([order[offsets[l] : offsets[l + 1]] for l in lists])
    sc = np.asarray(x16[cand], np.float64) @ np.asarray(q, np.float64)
    pick = np.lexsort((cand, -sc))[:k]
    return cand[pick], sc[pick], dict(zip(cand.tolist(), sc.tolist()))
