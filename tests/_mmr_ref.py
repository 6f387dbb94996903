"""The reference of diversify=: a numpy walk that implements the semantics literally -- float32 arrays, one explicit loop
over e for the similarity, the key codec of tests/_topk_ref.py --, the injected mistakes (MUTANTS) the CPU tests hold it against, and the
seeded inputs (CASES, build) that the kernel's GPU tests run: the CPU tests check on these very inputs that every mutant gives itself away."""
from typing import NamedTuple, Optional

import numpy as np

from tests import _topk_ref as R

F32 = np.float32
NEG_INF = F32(-np.inf)
MUTANTS = ("no_clamp", "ties_by_position", "sum_penalties", "pool_before_seen", "dot_f64", "dot_reversed", "val_fma")


def default_pool(k: int) -> int:
    return min(1024, max(4 * k, 64))


def pool_entries(scores, positions, n_items, ids, invalid, pool, mutant=None):
    """The list entries of the pool, in list order: the first `pool` ELIGIBLE entries -- a position in [0, n), a score above -inf (NaN is not),
    an id not among the row's invalid ids."""
    scores, positions = np.asarray(scores, dtype=F32), np.asarray(positions, dtype=np.int64)
    ok = (positions >= 0) & (positions < n_items)
    with np.errstate(invalid="ignore"):
        ok &= scores > NEG_INF
    seen = np.zeros(len(scores), dtype=bool)
    if invalid is not None and len(invalid):
        safe = np.where(ok, positions, 0)
        entry_ids = safe if ids is None else np.asarray(ids, dtype=np.int64)[safe]
        seen = ok & np.isin(entry_ids, np.asarray(invalid, dtype=np.int64))
    if mutant == "pool_before_seen":
        first = np.nonzero(ok)[0][:pool]
        return first[~seen[first]]
    return np.nonzero(ok & ~seen)[0][:pool]


def similarity(V, y, mutant=None):
    """sim(vec[c], vec[y]) for every pool entry c: acc = 0, then acc = acc + a[e] * b[e] for e ascending, every operation rounded to float32."""
    dim = V.shape[1]
    if mutant == "dot_f64":
        acc = np.zeros(V.shape[0], dtype=np.float64)
        for e in range(dim):
            acc = acc + V[:, e].astype(np.float64) * np.float64(V[y, e])
        return acc.astype(F32)
    acc = np.zeros(V.shape[0], dtype=F32)
    for e in (range(dim - 1, -1, -1) if mutant == "dot_reversed" else range(dim)):
        acc = acc + V[:, e] * V[y, e]
    return acc


def walk_row(scores, positions, vectors, lam, k, pool, ids=None, invalid=None, mutant=None):
    """One row -> (score bit patterns uint32[m], positions int64[m], ids int64[m], P) in PICK order, m = min(k, P)."""
    scores, positions = np.asarray(scores, dtype=F32), np.asarray(positions, dtype=np.int64)
    vectors = np.asarray(vectors, dtype=F32)
    entries = pool_entries(scores, positions, vectors.shape[0], ids, invalid, pool, mutant)
    P = len(entries)
    s, pos = scores[entries], positions[entries]
    V = vectors[pos]
    lam32 = F32(lam)
    mu32 = F32(1.0) - lam32
    M = np.zeros(P, dtype=F32)
    first = True
    picked = np.zeros(P, dtype=bool)
    tie = pos if mutant == "ties_by_position" else np.arange(P, dtype=np.int64)
    low = (~tie.astype(np.uint32)).astype(np.uint64)
    order = []
    with np.errstate(all="ignore"):
        for _ in range(min(k, P)):
            if mutant == "val_fma":      # lam * s exact (a float64 holds the product of two float32), one rounding behind the subtraction
                val = (lam32.astype(np.float64) * s.astype(np.float64) - (mu32 * M).astype(np.float64)).astype(F32)
            else:
                val = lam32 * s - mu32 * M
            key = (R.orderable(val.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | low
            key[picked] = 0
            y = int(np.argmax(key))
            picked[y] = True
            order.append(y)
            sim = similarity(V, y, mutant)
            if mutant == "no_clamp":
                M = sim if first else np.fmax(M, sim)
            elif mutant == "sum_penalties":
                M = M + np.fmax(sim, F32(0.0))
            else:
                M = np.fmax(M, sim)
            first = False
    order = np.asarray(order, dtype=np.int64)
    out_pos = pos[order]
    out_ids = out_pos if ids is None else np.asarray(ids, dtype=np.int64)[out_pos]
    return s[order].view(np.uint32), out_pos, out_ids, P


def walk(scores, positions, vectors, lam, k, pool, ids=None, invalid=None, mutant=None):
    """Every row -> (score bits uint32 (rows, k), positions, ids, counts int32 (rows,), verdict word): the kernel's outputs, (-inf, -1, -1)
    behind a short row's picks, the word 1 when some pool holds fewer than k."""
    rows = scores.shape[0]
    out_s = np.full((rows, k), NEG_INF, dtype=F32).view(np.uint32)
    out_p, out_i = np.full((rows, k), -1, dtype=np.int64), np.full((rows, k), -1, dtype=np.int64)
    counts = np.zeros(rows, dtype=np.int32)
    for b in range(rows):
        s, p, i, counts[b] = walk_row(scores[b], positions[b], vectors, lam, k, pool, ids, None if invalid is None else invalid[b], mutant)
        out_s[b, : len(p)], out_p[b, : len(p)], out_i[b, : len(p)] = s, p, i
    return out_s, out_p, out_i, counts, int((counts < k).any())


# ---- the inputs of the kernel's GPU tests -------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    rows: int
    length: int                 # entries of a row's list
    pool: int
    dim: int
    k: int
    family: str
    width: int = 0              # seen ids per row
    lam: float = 0.7
    probe: bool = False         # the CPU tests run the mutants on it


CASES = (
    Case("L1", 1, 1, 1, 1, 1, "gauss"),
    Case("L2-D1", 3, 2, 1, 3, 1, "gauss", width=1),
    Case("L2-D64", 3, 2, 64, 4, 1, "gauss"),
    Case("L63-equal", 3, 63, 64, 16, 1, "equal_scores", probe=True),
    Case("L64-all", 3, 64, 64, 17, 64, "gauss", probe=True),
    Case("L64-equal", 3, 64, 64, 16, 64, "equal_scores", lam=0.5, probe=True),
    Case("L65-rows70", 70, 65, 65, 32, 65, "gauss", lam=0.3),
    Case("L65-identical", 3, 65, 64, 33, 64, "identical_vectors", probe=True),
    Case("L1024-D1024", 1, 1024, 1024, 64, 1024, "gauss"),
    Case("L1025-one-hot", 3, 1025, 1024, 65, 1, "one_hot", width=256),
    Case("L1025-one-hot-k64", 3, 1025, 64, 65, 64, "one_hot", width=256, probe=True),
    Case("L5120-seen4096", 1, 5120, 1024, 3, 1024, "mixed", width=4096),
    Case("L16384-E256", 3, 16384, 1024, 256, 1, "mixed", width=257),
    Case("L16384-D65", 1, 16384, 65, 256, 65, "gauss", probe=True),
    Case("L1024-rows70", 70, 1024, 64, 1, 1, "gauss"),
    Case("negative-E64", 3, 65, 65, 64, 65, "negative_sims", lam=0.5, probe=True),
    Case("negative-E256", 1, 257, 64, 256, 64, "negative_sims", lam=0.5, probe=True),
    Case("signed-zeros", 3, 64, 64, 4, 64, "signed_zeros", probe=True),
    Case("subnormals", 3, 65, 65, 17, 65, "subnormals", probe=True),
    Case("plus-inf", 3, 64, 64, 16, 64, "plus_inf", probe=True),
    Case("near-duplicates", 1, 400, 400, 64, 400, "near_duplicates", lam=0.5, probe=True),
    Case("near-duplicates-E65", 1, 300, 300, 65, 300, "near_duplicates", lam=0.5, probe=True),
    Case("fma-pairs", 1, 201, 201, 128, 201, "fma_pairs", probe=True),
    Case("short-rows", 3, 65, 64, 3, 64, "short", width=1, probe=True),
    Case("seen-head", 3, 1025, 64, 4, 64, "mixed", width=256, probe=True),
    Case("seen-head-E32", 3, 200, 65, 32, 65, "mixed", width=257, probe=True),
)
CASE = {c.name: c for c in CASES}


def _sorted_desc(x):
    return -np.sort(-x, axis=1)


def build(case: Case, seed: int = 0):
    """-> dict(scores (rows, L) float32, positions (rows, L) int64, vectors (N, E) float32, ids (N,) int64, invalid (rows, width) int64 or None,
    n); a function of (case, seed) alone."""
    rng = np.random.default_rng([seed, CASES.index(case)])
    rows, L, dim, fam = case.rows, case.length, case.dim, case.family
    n = max(2 * L, 40) + 7
    ids = rng.permutation(n).astype(np.int64) * 5 + 2
    positions = np.stack([rng.permutation(n)[:L] for _ in range(rows)]).astype(np.int64)
    scores = _sorted_desc(rng.standard_normal((rows, L)).astype(F32))
    vectors = rng.standard_normal((n, dim)).astype(F32)
    head = 0                                                        # list entries whose ids the row has seen
    if fam == "equal_scores":
        scores[:] = F32(1.5)
    elif fam == "identical_vectors":
        vectors[:] = vectors[0]
    elif fam == "one_hot":
        vectors[:] = 0
        vectors[np.arange(n), rng.integers(0, dim, n)] = 1
        head = 40
    elif fam == "negative_sims":                                    # the vertices of a simplex, scaled: every pair has a negative dot product
        n = dim + 1
        assert L <= n
        base = np.eye(n, dim, dtype=np.float64) - 1.0 / (dim + 2.0)
        base[dim] = -1.0 / (dim + 2.0) - 0.5
        vectors = (base * rng.uniform(0.5, 2.0, (n, 1))).astype(F32)
        gram = vectors.astype(np.float64) @ vectors.astype(np.float64).T
        assert (gram[~np.eye(n, dtype=bool)] < -1e-4).all()
        ids = ids[:n]
        positions = np.stack([rng.permutation(n)[:L] for _ in range(rows)]).astype(np.int64)
        scores = _sorted_desc((1.0 + 0.01 * rng.standard_normal((rows, L))).astype(F32))
    elif fam == "signed_zeros":
        scores = np.where(rng.random((rows, L)) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    elif fam == "subnormals":
        bits = rng.integers(1, 1 << 23, (rows, L)).astype(np.uint32) | (rng.integers(0, 2, (rows, L)).astype(np.uint32) << np.uint32(31))
        scores = _sorted_desc(bits.view(F32))
    elif fam == "plus_inf":
        scores[:, : L // 4] = F32(np.inf)
    elif fam == "near_duplicates":                                  # pairs of items one ulp apart in one entry, every score equal: rounding decides
        scores[:] = F32(1.0)
        for a in range(0, n - 1, 2):
            vectors[a + 1] = vectors[a]
            e = rng.integers(0, dim)
            vectors[a + 1, e] = np.nextafter(vectors[a, e], F32(np.inf), dtype=F32)
        positions = np.stack([np.arange(L) for _ in range(rows)]).astype(np.int64)
    elif fam == "fma_pairs":
        # a seed item on axis 0, picked first; then pairs (x on an axis of its own: M stays 0; y on axis 0: M = 1) whose scores make
        # lam * s_x and lam * s_y - mu meet within an ulp or two: only the rounding of val orders a pair
        lam32 = F32(case.lam)
        mu32 = F32(1.0) - lam32
        pairs = (L - 1) // 2
        assert pairs < dim and n >= L
        vectors[:] = 0
        vectors[0, 0] = 1
        sx = np.sort(rng.uniform(1.0, 2.0, pairs)).astype(F32)[::-1]
        sy = ((lam32.astype(np.float64) * sx.astype(np.float64) + np.float64(mu32)) / np.float64(lam32)).astype(F32)
        sy = (sy.view(np.uint32) + rng.integers(-1, 2, pairs).astype(np.uint32)).view(F32)
        row = [F32(100.0)]
        for j in range(pairs):
            vectors[1 + 2 * j, 1 + j] = 1
            vectors[2 + 2 * j, 0] = 1
            row += [sx[j], sy[j]]
        scores = np.tile(np.asarray(row, dtype=F32), (rows, 1))
        positions = np.stack([np.arange(L) for _ in range(rows)]).astype(np.int64)
    elif fam == "short":                                            # row 1 keeps five eligible entries
        scores[1, 5:] = NEG_INF
        head = 1
    elif fam == "mixed":                                            # entries that are not eligible by themselves, and a seen head
        for b in range(rows):
            at = rng.permutation(L)[: max(4, L // 8)]
            q = len(at) // 4
            scores[b, at[:q]] = NEG_INF
            scores[b, at[q: 2 * q]] = F32(np.nan)
            positions[b, at[2 * q: 3 * q]] = -1
            positions[b, at[3 * q:]] = n
        head = min(L, (3 * case.width) // 4)
    invalid = None
    if case.width:
        invalid = (-7 - 5 * np.arange(case.width, dtype=np.int64))[None, :].repeat(rows, axis=0)      # ids nobody has (every id is 2 mod 5)
        for b in range(rows):
            hit = positions[b, :head]
            hit = hit[(hit >= 0) & (hit < n)][: case.width]
            where = rng.permutation(case.width)[: len(hit)]
            invalid[b, where] = ids[hit]
    return dict(scores=scores, positions=positions, vectors=vectors, ids=ids, invalid=invalid, n=n)
