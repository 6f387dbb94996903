"""Restatement of the IVF-Flat index kernels (rails_amd/csrc/ivf.hip, include/rails_amd.h rails_ivf_*) in numpy integers, float64 and
single float32 operations, plus the inputs and the case lists that tests/test_ivf_exact_cpu.py and tests/test_ivf_exact_gpu.py share.

The bar is equality.  The header documents these kernels as deterministic: every score is ONE fp32 accumulator fed by fmaf over the dims in
order (assign, coarse and scan alike), means are summed in sample order, nothing uses float atomics, and the build keeps IEEE `/` and sqrtf.
On the DYADIC grid used here -- fp16 components, fp32 query components and crafted fp32 centroids all integer multiples of 2^-6 of magnitude
<= 2 -- every product is a multiple of 2^-12 and every partial sum of <= 128 of them stays below 2^9 + 1: at most 22 significant bits, so
the fmaf chain is exact in any order and equals the float64 dot product; the sum of <= 4096 sample components stays below 2^13 (19 bits).
The CPU file asserts both for every case.  Where an operand leaves the grid (the centroids after a Lloyd step) the restatement uses
fma32, a correctly rounded fp32 fused multiply-add, in dim order: no double rounding.

  assign        argmax of the fp32 score, ties to the lower list
  build_lists   stable counting sort: offsets (nlist + 1), positions ascending inside a list, the fp16 vectors in list order
  lloyd_step    assign -> sums in sample order (exact here) -> ONE fp32 division by the float count -> empty lists, ascending, each split
                off the largest list (float sizes, ties to the lower id; v * (1 +- 1/1024) by dim parity; sz[ci] = sz[cj] / 2,
                sz[cj] -= sz[ci]) -> normalise: ss = fmaf(a, a, b * b) per lane (a = c[lane], b = c[lane + 64], 0 beyond d), the xor
                butterfly 32 .. 1 in fp32, inv = 1 / sqrtf(ss), c * inv
  train         init copies the first nlist sample rows; `iters` steps
  coarse        centroid scores, NaN -> -inf; lists best first, ties to the lower id, until taken >= nprobe and held >= k, at most
                max_probes; the filtered form counts eligible entries
  search        per row (b, i, m) the k best entries of the probed lists by (score desc, position asc), NaN -> -inf; the filtered form
                offers only entries with word & allowed[b] != 0; fewer than k: `unfilled` raised, the tail slots hold position 0
  plan          max_probes = the most lists any probe order can need: the count of smallest lists (of any group) whose sizes reach k, nlist
                where they never do, at least nprobe; max_list = the largest list (at least 1).  plan_filtered: the same over counts rows

`bug` arguments apply the bug classes the CPU file holds the GPU cases' own inputs against (BUGS).
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

F32, F64 = np.float32, np.float64

# name -> (oracle config, P_Q, P_X, d)
SHAPES = {
    "8x8x32": ("amzn-books", 8, 8, 32),
    "8x4x64": ("ml-1m", 8, 4, 64),
    "8x4x128": ("ml-20m", 8, 4, 128),
    "16x16x64": ("synthetic-16x16x64", 16, 16, 64),
}
SORT_TILE = 4096          # items per histogram tile of the counting sort
MAX_NLIST, MAX_PROBE, MAX_K = 4096, 64, 128
SLICE_ROWS = 1024         # query rows (b, i) per search slice
SPLIT_EPS = F32(1.0 / 1024.0)
EMPTY = 0x7FFFFFFF
BUGS = ("assign_high", "coarse_high", "pos_desc", "unstable", "seg_drop_last", "seg_from_max_list", "rank64", "no_continue",
        "filter_counts_sizes", "nan_kept", "split_last_tied", "no_halve", "parity", "mean_div_first")


def geometry(shape):
    """-> (P_Q, G = P_X, d)"""
    return SHAPES[shape][1:]


# ---- the grid ------------------------------------------------------------------------------------------------------------------
def dyadic(rng, shape, big=0.02):
    """multiples of 2^-6: {-4 .. 4} / 64 with a share `big` of +-2 -- a small range, so that exact ties are plentiful"""
    v = rng.integers(-4, 5, size=shape)
    v = np.where(rng.random(shape) < big, rng.choice(np.array([-128, 128]), size=shape), v)
    return (v / 64.0).astype(F32)


def on_grid(x):
    x = np.asarray(x, F64)
    return bool(np.isfinite(x).all() and (np.abs(x) <= 2).all() and (x * 64 == np.rint(x * 64)).all())


def fma32(x, y, z):
    """fmaf(x, y, z) on finite fp32 arrays, correctly rounded.  The product is exact in float64 (48 bits); the float64 sum s and its
    TwoSum error e give the exact value s + e; s -> fp32 can round a second time only where s is exactly an fp32 midpoint while e != 0,
    and there e decides."""
    x, y, z = (np.asarray(v, F32).astype(F64) for v in (x, y, z))
    p = x * y
    s = p + z
    bb = s - p
    e = (p - (s - bb)) + (z - bb)
    r = s.astype(F32)
    r64 = r.astype(F64)
    d = s - r64
    other = np.nextafter(r, np.where(d > 0, F32(np.inf), F32(-np.inf))).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        mid = (d != 0) & ((s - r64) == (other.astype(F64) - s))
    return np.where(mid & (e > 0), np.maximum(r, other), np.where(mid & (e < 0), np.minimum(r, other), r)).astype(F32)


def chain_scores(x, c):
    """(points, lists) fp32: acc = fmaf(x[j], c[j], acc) over the dims in order, from 0"""
    x, c = np.asarray(x, F32), np.asarray(c, F32)
    acc = np.zeros((x.shape[0], c.shape[0]), F32)
    for j in range(x.shape[1]):
        acc = fma32(x[:, j : j + 1], c[None, :, j], acc)
    return acc


def dot64(x, c):
    """the float64 dot products: on the grid THE fp32 chain's value, whatever the order (the CPU file asserts it)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(x, F64) @ np.asarray(c, F64).T


# ---- assignment and list build ----------------------------------------------------------------------------------------------------
def assign(x, c, exact_chain=False, bug=""):
    """argmax_l <x, c_l> in fp32, ties to the lower list"""
    s = chain_scores(x, c) if exact_chain else dot64(x, c)
    if bug == "assign_high":
        return (s.shape[1] - 1 - np.argmax(s[:, ::-1], axis=1)).astype(np.int32)
    return np.argmax(s, axis=1).astype(np.int32)


def counting_sort(a, nlist, bug=""):
    """-> (order (n,) int32: the points in (list, index) order, offsets (nlist + 1,) int32)"""
    order = np.argsort(a, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int32)
    if bug == "unstable":       # two equal-list items of one tile swapped
        for l in range(nlist):
            lo, hi = offsets[l], offsets[l + 1]
            if hi - lo >= 2 and order[lo] // SORT_TILE == order[lo + 1] // SORT_TILE:
                order[lo], order[lo + 1] = order[lo + 1], order[lo]
                break
    return order, offsets


def build_lists(x16, c, bug=""):
    """x16 (n, d) float16, c (nlist, d) fp32 -> (assign, offsets, positions, vectors as uint16 bits in list order)"""
    a = assign(x16.astype(F32), c, bug=bug)
    order, offsets = counting_sort(a, c.shape[0], bug)
    return a, offsets, order, np.ascontiguousarray(x16[order]).view(np.uint16)


# ---- training -----------------------------------------------------------------------------------------------------------------
def normalise(c):
    c = np.asarray(c, F32)
    L, d = c.shape
    a, b = np.zeros((L, 64), F32), np.zeros((L, 64), F32)
    a[:, : min(d, 64)] = c[:, :64]
    if d > 64:
        b[:, : d - 64] = c[:, 64:]
    ss = fma32(a, a, b * b)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[:, lane ^ o]
    inv = F32(1.0) / np.sqrt(ss)
    out = np.empty_like(c)
    out[:, : min(d, 64)] = (a * inv)[:, : min(d, 64)]
    if d > 64:
        out[:, 64:] = (b * inv)[:, : d - 64]
    return out


def lloyd_step(xs, c, exact_chain=False, bug="", want_sizes=False):
    """xs (S, d) the sample's fp16 values as fp32, c (nlist, d) fp32 -> the centroids after one iteration"""
    xs, c = np.asarray(xs, F32), np.asarray(c, F32)
    L, d = c.shape
    a = assign(xs, c, exact_chain)
    sizes = np.bincount(a, minlength=L).astype(F32)
    new = c.copy()                                   # an empty list keeps its row until the split writes it
    nz = sizes > 0
    if bug == "mean_div_first":
        acc = np.zeros((L, d), F32)
        for s in range(xs.shape[0]):
            acc[a[s]] = acc[a[s]] + xs[s] / sizes[a[s]]
        new[nz] = acc[nz]
    else:
        sums = np.zeros((L, d), F64)
        np.add.at(sums, a, xs.astype(F64))           # exact: multiples of 2^-6 below 2^13
        new[nz] = sums[nz].astype(F32) / sizes[nz, None]
    first_sizes = sizes.copy()
    even = np.arange(d) % 2 == 0
    up, down = F32(1.0) + SPLIT_EPS, F32(1.0) - SPLIT_EPS
    if bug == "parity":
        up, down = down, up
    for ci in range(L):
        if sizes[ci] != 0:
            continue
        tied = np.nonzero(sizes == sizes.max())[0]
        cj = int(tied[-1] if bug == "split_last_tied" else tied[0])
        v = new[cj].copy()
        new[ci] = v * np.where(even, up, down)
        new[cj] = v * np.where(even, down, up)
        if bug != "no_halve":
            sizes[ci] = sizes[cj] / F32(2.0)
            sizes[cj] = sizes[cj] - sizes[ci]
    out = normalise(new)
    return (out, first_sizes) if want_sizes else out


def train(xs, nlist, iters, c0=None):
    """init (c0 None): the first nlist sample rows; then `iters` steps with the correctly rounded fmaf chain"""
    c = np.asarray(xs[:nlist], F32).copy() if c0 is None else np.asarray(c0, F32)
    for _ in range(iters):
        c = lloyd_step(xs, c, exact_chain=True)
    return c


# ---- plans and the scan geometry ----------------------------------------------------------------------------------------------------
def need_lists(sizes, k):
    s = np.cumsum(np.sort(np.asarray(sizes, np.int64)))
    hit = np.nonzero(s >= k)[0]
    return int(hit[0]) + 1 if len(hit) else len(s)


def plan(offsets, nprobe, k):
    """offsets (G, nlist + 1) -> (max_probes, max_list)"""
    sizes = np.diff(np.asarray(offsets, np.int64), axis=1)
    nlist = sizes.shape[1]
    mp = max([min(nprobe, nlist)] + [need_lists(sizes[m], k) for m in range(sizes.shape[0])])
    return min(mp, nlist), max(1, int(sizes.max()))


def plan_filtered(counts, nprobe, k):
    """counts (R, G, nlist) -> max_probes"""
    nlist = counts.shape[-1]
    mp = max([min(nprobe, nlist)] + [need_lists(row, k) for row in counts.reshape(-1, nlist)])
    return min(mp, nlist)


def scan_geometry(B, PQ, G, nlist, nprobe, max_list):
    """(seg_items, n_seg) of the list scan: internal, restated only so that the CPU file can say which cases split their lists into
    64-entry segments (the results do not depend on it)"""
    slice_b = max(1, min(B, SLICE_ROWS // PQ))
    units = slice_b * PQ * G * nprobe
    ns = max(1, -(-16384 // units))
    ns = min(ns, max(1, (max_list + 63) // 64))
    ns = min(ns, max(1, 65536 // (nlist * G)))
    seg = max(64, (-(-max_list // ns) + 63) // 64 * 64)
    return seg, max(1, -(-max_list // seg))


# ---- search -------------------------------------------------------------------------------------------------------------------
class Lists(NamedTuple):
    cent: np.ndarray      # (G, nlist, d) fp32
    vec: np.ndarray       # (G, n, d) float16, list order
    pos: np.ndarray       # (G, n) int32
    off: np.ndarray       # (G, nlist + 1) int32

    @property
    def sizes(self):
        return np.diff(self.off.astype(np.int64), axis=1)

    def list_of_slot(self, m):
        return np.repeat(np.arange(self.off.shape[1] - 1), self.sizes[m])


def list_words(pos, n, eff=None, visible=None):
    """word(position): the effective tag word, or all ones / 0 for a visible / hidden item; 0 outside [0, n)"""
    pos = np.asarray(pos, np.int64)
    ok = (pos >= 0) & (pos < n)
    p = np.where(ok, pos, 0)
    w = eff[p] if eff is not None else np.where((visible[p >> 5] >> (p & 31).astype(np.uint32)) & np.uint32(1), np.uint32(0xFFFFFFFF), np.uint32(0))
    return np.where(ok, w, np.uint32(0)).astype(np.uint32)


def list_counts(ix: Lists, words, allowed):
    """counts[r][m][l] = #{slot of list l of group m: words[m][slot] & allowed[r] != 0}"""
    G, L = ix.off.shape[0], ix.off.shape[1] - 1
    out = np.zeros((len(allowed), G, L), np.int32)
    for m in range(G):
        ok = (words[m][None, :] & np.asarray(allowed, np.uint32)[:, None]) != 0
        lid = ix.list_of_slot(m)
        for l in range(L):
            out[:, m, l] = ok[:, lid == l].sum(axis=1)
    return out


def coarse(eq, ix: Lists, held, nprobe, k, max_probes, bug=""):
    """held (B, G, nlist): what the short-list rule counts per list (sizes, or the eligible counts of the row's query)
    -> probes (B, P_Q, G, max_probes) int32 padded with -1, nprob (B, P_Q, G)"""
    B, PQ, d = eq.shape
    G, L = ix.cent.shape[:2]
    probes = np.full((B, PQ, G, max_probes), -1, np.int32)
    nprob = np.zeros((B, PQ, G), np.int32)
    q = eq.reshape(B * PQ, d)
    ids = np.arange(1, L + 1)
    for m in range(G):
        s = dot64(q, ix.cent[m])
        nan = np.isnan(s)
        s[nan] = -np.inf
        if bug == "coarse_high":
            order = L - 1 - np.argsort(-s[:, ::-1], axis=1, kind="stable")
        else:
            order = np.argsort(-s, axis=1, kind="stable")
        cum = np.cumsum(np.take_along_axis(np.repeat(held[:, m], PQ, axis=0), order, 1), axis=1)
        ok = (ids[None, :] >= nprobe) & (cum >= k)
        t = np.where(ok.any(axis=1), ok.argmax(axis=1) + 1, L)
        if bug == "no_continue":
            t = np.full_like(t, nprobe)
        t = np.minimum(t, max_probes)
        if bug == "nan_kept":                        # a NaN score never compares greater: such a row takes no list
            t = np.where(nan.any(axis=1), 0, t)
        pr = np.where(np.arange(max_probes)[None, :] < t[:, None], order[:, :max_probes], -1)
        probes[:, :, m] = pr.reshape(B, PQ, max_probes)
        nprob[:, :, m] = t.reshape(B, PQ)
    return probes, nprob


def search(ix: Lists, eq, nprobe, k, max_probes, words=None, allowed=None, bug="", seg_items=64, max_list=None):
    """-> (positions (B, P_Q * G * k) int64, unfilled 0 / 1, probes, nprob).  words (G, n) uint32 with allowed (B,) uint32: the filtered form."""
    B, PQ, d = eq.shape
    G, L = ix.cent.shape[:2]
    n = ix.pos.shape[1]
    sizes = ix.sizes
    filtered = words is not None
    held = np.broadcast_to(sizes[None], (B, G, L))
    if filtered:
        counts = list_counts(ix, words, allowed)
        if bug != "filter_counts_sizes":
            held = counts
    probes, nprob = coarse(eq, ix, held, nprobe, k, max_probes, bug)
    q = eq.reshape(B * PQ, d)
    out = np.zeros((B, PQ, G, k), np.int64)
    unfilled = 0
    for m in range(G):
        s = dot64(q, ix.vec[m])
        nan = np.isnan(s)
        s[nan] = -np.inf
        pos = np.broadcast_to(ix.pos[m].astype(np.int64), s.shape)
        order = np.lexsort((-pos if bug == "pos_desc" else pos, -s), axis=1)
        lid = ix.list_of_slot(m)
        pm = np.zeros((B * PQ, L + 1), bool)
        pr = probes[:, :, m].reshape(B * PQ, -1)
        np.put_along_axis(pm, np.where(pr < 0, L, pr), True, axis=1)
        pm = pm[:, :L]
        if bug == "seg_from_max_list":               # a list's scan runs max_list entries on, into the lists behind it
            slot = np.arange(n)
            ext = np.stack([(slot >= ix.off[m, l]) & (slot < min(n, ix.off[m, l] + (max_list if sizes[m, l] else 0))) for l in range(L)])
            ok = (pm.astype(np.int64) @ ext.astype(np.int64)) > 0
        else:
            ok = pm[:, lid]
        if bug == "seg_drop_last":
            j = np.arange(n) - ix.off[m, lid]
            ok = ok & ~((j % seg_items == seg_items - 1) | (j == sizes[m, lid] - 1))[None, :]
        if bug == "nan_kept":
            ok = ok & ~nan
        if filtered:
            ok = ok & np.repeat((words[m][None, :] & np.asarray(allowed, np.uint32)[:, None]) != 0, PQ, axis=0)
        oks = np.take_along_axis(ok, order, 1)
        rank = np.cumsum(oks, axis=1)
        have = np.minimum(rank[:, -1], k)
        first = np.argsort(~(oks & (rank <= k)), axis=1, kind="stable")[:, :k]
        p = ix.pos[m].astype(np.int64)[np.take_along_axis(order, first, 1)]
        p[np.arange(k)[None, :] >= have[:, None]] = 0
        unfilled |= int((have < k).any())
        out[:, :, m] = p.reshape(B, PQ, k)
    return out.reshape(B, PQ * G * k), unfilled, probes, nprob


# the kernel's own flow for ONE row, lane by lane: a running top-(64 KS) list per (probe, segment), then their merge
def wave_topk(parts, k, bug=""):
    """parts: lists of (score, position) in arrival order, each offered 64 at a time -> the list's first k (score, position), sentinels included"""
    cap = 128 if k > 64 else 64
    top = [(-np.inf, EMPTY)] * cap
    before = lambda a, b: a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])
    for chunk in (part[c0 : c0 + 64] for part in parts for c0 in range(0, len(part), 64)):
        want = [e for e in chunk if before(e, top[k - 1])]
        for e in want:
            if not before(e, top[k - 1]):
                continue
            r = sum(before(t, e) for t in top)
            new = top[:r] + [e] + top[r:-1]
            if bug == "rank64" and cap == 128 and r < 64:
                new[64] = top[127]                   # rank 64 takes its own slot's neighbour: rank 63 is lost
            top = new
    return top[:k]


def wave_search_row(ix: Lists, q, m, probe_lists, k, seg_items, bug=""):
    s = dot64(q[None], ix.vec[m])[0]
    s[np.isnan(s)] = -np.inf
    top = []
    for l in probe_lists:
        lo, hi = int(ix.off[m, l]), int(ix.off[m, l + 1])
        for s0 in range(lo, hi, seg_items):
            s1 = min(hi, s0 + seg_items)
            part = wave_topk([[(float(s[i]), int(ix.pos[m, i])) for i in range(s0, s1)]], k, bug)
            top.append(part[: min(k, s1 - s0)])
    merged = wave_topk(top, k, bug)
    return [0 if p == EMPTY else p for _, p in merged]


# ---- the fp32-format item index (mol_layout.h ex_offset), Ex part only -----------------------------------------------------------------
def pack_index(ex, PQ):
    """ex (n, G, d) fp32 -> the tile-packed fp32 index buffer (gi left 0): what the list edit cuts its fp16 vectors from"""
    n, G, d = ex.shape
    tile = 32 * (G * d + PQ * G)
    buf = np.zeros(((n + 31) // 32) * tile, F32)
    item, m, dd = np.meshgrid(np.arange(n), np.arange(G), np.arange(d), indexing="ij")
    hi = dd // (d // 2)
    s = dd - hi * (d // 2)
    slot = (m * (d // 8) + (s >> 2)) * 64 + hi * 32 + (item & 31)
    buf[(item >> 5) * tile + slot * 4 + (s & 3)] = ex
    return buf


# ---- cases ----------------------------------------------------------------------------------------------------------------------
class BuildCase(NamedTuple):
    shape: str
    n: int
    nlist: int
    why: str


BUILD_CASES = (
    BuildCase("8x8x32", 255, 37, "one ragged 256-point block"),
    BuildCase("8x8x32", 256, 256, "nlist = n; one full LDS chunk of 256 centroids"),
    BuildCase("8x8x32", 257, 257, "nlist = n; a second chunk of one centroid; a second point block of one"),
    BuildCase("8x8x32", 4096, 300, "two chunks; one full sort tile"),
    BuildCase("8x8x32", 8193, 600, "three tiles with a tail of one; nlist * tiles = 1800 > 1024: the prefix kernel's carry"),
    BuildCase("8x8x32", 4097, 4096, "the LDS histogram's limit; sixteen chunks"),
    BuildCase("8x8x32", 4097, 1, "nlist = 1; two tiles"),
    BuildCase("8x4x64", 257, 129, "d = 64: a second chunk of one centroid"),
    BuildCase("8x4x64", 4097, 129, "d = 64, two tiles"),
    BuildCase("8x4x64", 255, 1, "nlist = 1"),
    BuildCase("8x4x128", 255, 65, "d = 128: a second chunk of one centroid"),
    BuildCase("8x4x128", 4096, 70, "d = 128, two chunks, one full tile"),
    BuildCase("8x4x128", 8193, 65, "d = 128, three tiles"),
    BuildCase("16x16x64", 256, 129, "sixteen groups"),
    BuildCase("16x16x64", 4097, 20, "sixteen groups, two tiles, one chunk"),
)


def seed_of(*key):
    """a seed that does not depend on the interpreter's string hashing"""
    return sum((i + 1) * sum(str(k).encode()) for i, k in enumerate(key)) % (1 << 31)


@functools.lru_cache(maxsize=4)
def build_inputs(case: BuildCase):
    """-> (x16 (G, n, d) float16, cent (G, nlist, d) fp32).  Some centroids are copies of a lower one in ANOTHER LDS chunk where there is
    one: the copy ties with the original on every point and must never win, so its list stays empty."""
    _, G, d = geometry(case.shape)
    rng = np.random.default_rng(seed_of("build", *case[:3]))
    x = dyadic(rng, (G, case.n, d)).astype(np.float16)
    cent = dyadic(rng, (G, case.nlist, d))
    for j in range(min(8, case.nlist // 4)):
        cent[:, case.nlist - 1 - 2 * j] = cent[:, 3 * j]
    return x, cent


def build_copies(case: BuildCase):
    """(lower, higher) centroid ids of the planted copies"""
    return [(3 * j, case.nlist - 1 - 2 * j) for j in range(min(8, case.nlist // 4))]


class LloydCase(NamedTuple):
    shape: str
    kind: str         # none | several | tied | resplit


LLOYD_NLIST = 24
LLOYD_CASES = tuple(LloydCase(s, k) for s in ("8x8x32", "8x4x64", "8x4x128") for k in ("none", "several", "tied", "resplit"))


def lloyd_sizes(kind, rng):
    L = LLOYD_NLIST
    if kind == "none":
        return rng.integers(1, 60, L)
    if kind == "several":
        sz = rng.integers(1, 60, L)
        sz[[3, 7, 8, 20]] = 0
        return sz
    if kind == "tied":            # 9 and 14 tie for the largest: 9 is split first, then 14
        sz = rng.integers(1, 40, L)
        sz[[5, 11]] = 0
        sz[[9, 14]] = 101
        return sz
    sz = rng.integers(1, 10, L)   # resplit: 4 (41 points) is halved to 20.5 | 20.5 with new list 2, which ties with 4 and, the lower id, is split next
    sz[[2, 6, 10]] = 0
    sz[4] = 41
    return sz


@functools.lru_cache(maxsize=None)
def lloyd_inputs(case: LloydCase):
    """-> (table (G, n, d) float16, sample (S,) int32 positions into it, start (G, nlist, d) fp32, the sizes meant (nlist,))
    Point s of list h has its largest entry, 1 or 2, in dim h, where centroid h has 1: its home list wins by a wide margin."""
    _, G, d = geometry(case.shape)
    rng = np.random.default_rng(seed_of("lloyd", *case))
    sizes = lloyd_sizes(case.kind, rng)
    S, L = int(sizes.sum()), LLOYD_NLIST
    n = S + 50
    home = rng.permutation(np.repeat(np.arange(L), sizes))
    table = (rng.integers(-2, 3, (G, n, d)) / 64.0).astype(F32)
    sample = rng.permutation(n)[:S].astype(np.int32)
    for m in range(G):
        table[m, sample, home] = rng.choice(np.array([1.0, 1.5, 2.0]), S)
    start = (rng.integers(-1, 2, (G, L, d)) / 64.0).astype(F32)
    start[:, np.arange(L), np.arange(L)] = 1.0
    return table.astype(np.float16), sample, start, sizes


TRAIN_SHAPE, TRAIN_S, TRAIN_NLIST = "8x8x32", 512, 16


@functools.lru_cache(maxsize=None)
def train_inputs():
    _, G, d = geometry(TRAIN_SHAPE)
    rng = np.random.default_rng(seed_of("train"))
    table = dyadic(rng, (G, TRAIN_S + 30, d)).astype(np.float16)
    return table, rng.permutation(TRAIN_S + 30)[:TRAIN_S].astype(np.int32)


class EditCase(NamedTuple):
    kind: str         # drop | insert | both | cut
    m: int
    in_place: int


EDIT_SHAPE, EDIT_N, EDIT_NLIST = "8x8x32", 4097, 37
EDIT_CASES = (EditCase("drop", 0, 1), EditCase("insert", 40, 0), EditCase("insert", 40, 1), EditCase("both", 0, 1), EditCase("both", 1, 0),
              EditCase("both", 300, 1), EditCase("both", 300, 0), EditCase("cut", 120, 1))


@functools.lru_cache(maxsize=None)
def edit_base():
    _, G, d = geometry(EDIT_SHAPE)
    rng = np.random.default_rng(seed_of("edit"))
    return dyadic(rng, (G, EDIT_N, d)).astype(np.float16), dyadic(rng, (G, EDIT_NLIST, d))


def edit_inputs(case: EditCase):
    """-> (positions (m,) int64 unsorted, n_keep, n_new, rows (m, G, d) fp32: the new values of the edit's positions)
    drop: the tail cut, nothing inserted; insert: appended items only; both: replaced and appended items; cut: a cut with both."""
    _, G, d = geometry(EDIT_SHAPE)
    rng = np.random.default_rng(seed_of("edit", *case))
    n_keep = {"drop": 4000, "insert": EDIT_N, "both": EDIT_N + 7, "cut": 3000}[case.kind]     # (an n_keep past n_old cuts nothing)
    lim = min(EDIT_N, n_keep)
    replaced = 0 if case.kind == "insert" else case.m - case.m // 3
    pos = np.concatenate([rng.choice(lim, replaced, replace=False), lim + np.arange(case.m - replaced)]).astype(np.int64)
    rng.shuffle(pos)
    return pos, n_keep, lim + case.m - replaced, dyadic(rng, (case.m, G, d))


def edited_table(case: EditCase):
    """the (G, n_new, d) float16 table after the edit"""
    x, _ = edit_base()
    pos, n_keep, n_new, rows = edit_inputs(case)
    out = np.zeros((x.shape[0], n_new, x.shape[2]), np.float16)
    lim = min(EDIT_N, n_keep)
    out[:, :lim] = x[:, :lim]
    if case.m:
        out[:, pos] = rows.transpose(1, 0, 2).astype(np.float16)
    return out


# crafted lists for the search: the sizes are the segment edges at 64 entries per segment; three more lists fix the arrival order of one row
EDGE_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 300)
INDEX_SIZES = {
    "edges": EDGE_SIZES + (300, 300, 200),          # + scores ascending with the slot, descending, all equal
    "sixtyfour": tuple((7 * i * i + 3 * i) % 41 for i in range(64)),
    "short": tuple((5 * i) % 7 for i in range(40)),  # 0 .. 6 entries a list: k = 20 needs many lists
    "small": (5, 70, 0, 130, 64, 20),
    "poison": EDGE_SIZES,                            # "edges" with an fp16 NaN, +inf and -inf entry; its queries hold a NaN
}


@functools.lru_cache(maxsize=None)
def search_index(shape, kind) -> Lists:
    _, G, d = geometry(shape)
    sizes = np.array(INDEX_SIZES[kind])
    L, n = len(sizes), int(sizes.sum())
    rng = np.random.default_rng(seed_of("index", shape, kind))
    cent = dyadic(rng, (G, L, d))
    cent[:, L - 1] = cent[:, 1]                      # tied centroids with lists behind both: the lower list is the earlier probe
    cent[:, 5] = cent[:, 2]
    vec = dyadic(rng, (G, n, d)).astype(np.float16)
    off = np.tile(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), (G, 1))
    lid = np.repeat(np.arange(L), sizes)
    pos = np.empty((G, n), np.int32)
    for m in range(G):
        p = rng.permutation(n)
        pos[m] = p[np.lexsort((p, lid))]             # ascending inside a list, as a build leaves them
    if kind == "edges":
        for l, w in ((9, np.arange(300)), (10, np.arange(300)[::-1]), (11, np.zeros(200, np.int64))):
            lo = off[0, l]
            vec[:, lo : lo + len(w)] = 0
            vec[:, lo : lo + len(w), 0] = ((w // 64 - 2) / 64.0).astype(np.float16)[None]      # with q[0] = 1 and q[1] = 1/64 the score is
            vec[:, lo : lo + len(w), 1] = ((w % 64) / 64.0).astype(np.float16)[None]           # ((w // 64 - 2) * 64 + w % 64) / 4096: w's order
    if kind == "short":                              # with q = 2 e_0 the coarse order is smallest list first: the plan's worst case
        cent[:, np.argsort(sizes, kind="stable"), 0] = ((L - np.arange(L)) / 64.0).astype(F32)[None]
    if kind == "poison":
        for m in range(G):
            vec[m, off[m, 4] + 7, 3] = np.float16(np.nan)
            vec[m, off[m, 6] + 100, 1] = np.float16(np.inf)
            vec[m, off[m, 8] + 64, 2] = np.float16(-np.inf)
    return Lists(cent, vec, pos, off)


@functools.lru_cache(maxsize=None)
def search_queries(shape, kind, B):
    PQ, _, d = geometry(shape)
    rng = np.random.default_rng(seed_of("queries", shape, kind, B))
    eq = dyadic(rng, (B, PQ, d))
    if kind == "edges":
        eq[0, 0] = 0                                  # the arrival-order row: list 9 ascends, 10 descends, 11 ties
        eq[0, 0, 0], eq[0, 0, 1] = 1.0, 1.0 / 64.0
        eq[0, 1] = -eq[0, 0]                          # and reversed
    if kind == "short":
        eq[0, 0] = 0
        eq[0, 0, 0] = 2.0
    if kind == "poison":
        eq[B - 1, 2, 5] = np.nan
    return eq


class SearchCase(NamedTuple):
    shape: str
    kind: str
    B: int
    k: int
    nprobe: int
    below_plan: int = 0        # max_probes passed = the plan's minus this


_ROT = tuple(SHAPES)
SEARCH_CASES = tuple(
    SearchCase(_ROT[(ik + ip) % 4], "edges", 1 if _ROT[(ik + ip) % 4] == "16x16x64" else 2, k, nprobe)
    for ik, k in enumerate((1, 5, 63, 64, 65, 127, 128)) for ip, nprobe in enumerate((1, 3, 12))
) + (
    SearchCase("8x4x64", "sixtyfour", 1, 20, 64),
    SearchCase("8x8x32", "sixtyfour", 2, 128, 64),
    SearchCase("8x8x32", "short", 2, 20, 1), SearchCase("8x8x32", "short", 2, 20, 1, 1),
    SearchCase("8x4x128", "short", 1, 100, 3), SearchCase("8x4x128", "short", 1, 100, 3, 1),
    SearchCase("8x8x32", "small", 129, 5, 2),         # B * P_Q = 1032: a second slice of one query
    SearchCase("16x16x64", "small", 65, 65, 1),       # B * P_Q = 1040
    SearchCase("8x8x32", "poison", 2, 64, 9), SearchCase("8x4x128", "poison", 2, 128, 3), SearchCase("8x4x64", "poison", 3, 5, 1),
)


class FilterCase(NamedTuple):
    shape: str
    B: int
    k: int
    nprobe: int
    per_row: bool


FILTER_CASES = (FilterCase("8x8x32", 3, 5, 1, False), FilterCase("8x8x32", 3, 5, 1, True), FilterCase("8x4x64", 4, 64, 3, True),
                FilterCase("8x4x128", 2, 100, 2, False), FilterCase("16x16x64", 2, 128, 1, True), FilterCase("8x8x32", 5, 20, 12, True),
                FilterCase("8x4x64", 129, 5, 2, True))      # B * P_Q = 1032: the second slice reads its own allow words and counts rows
RARE = np.uint32(1 << 30)      # a tag few items carry: a row that allows only it finds short lists everywhere


@functools.lru_cache(maxsize=None)
def filter_words(shape):
    """-> (eff (n,) uint32 by item position, visible ((n + 31) / 32,) uint32 words).  In every group list 3 (64 entries) and the second
    segment of list 8 (its slots 64 .. 127) hold items without any allowed tag (bit 31 only, which no allow word has)."""
    ix = search_index(shape, "edges")
    n = ix.pos.shape[1]
    rng = np.random.default_rng(seed_of("words", shape))
    eff = (np.uint32(1) << rng.integers(0, 4, n).astype(np.uint32)) | np.where(rng.random(n) < 0.04, RARE, np.uint32(0))
    eff = np.where(rng.random(n) < 0.1, np.uint32(0), eff).astype(np.uint32)
    for m in range(ix.pos.shape[0]):
        for lo, hi in ((ix.off[m, 3], ix.off[m, 4]), (ix.off[m, 8] + 64, ix.off[m, 8] + 128)):
            eff[ix.pos[m, lo:hi]] = np.uint32(1 << 31)
    bits = (eff & np.uint32(0xF)) != 0
    visible = np.zeros((n + 31) // 32, np.uint32)
    np.bitwise_or.at(visible, np.nonzero(bits)[0] >> 5, (np.uint32(1) << (np.nonzero(bits)[0] & 31).astype(np.uint32)))
    return eff, visible


def filter_allowed(case: FilterCase):
    """(B,) uint32: one word for the whole batch, or one per row (a rare-tag row among them)"""
    if not case.per_row:
        return np.full(case.B, 0x5, np.uint32)
    rng = np.random.default_rng(seed_of("allowed", *case))
    a = rng.choice(np.array([0x1, 0x6, 0xF, 0x8], np.uint32), case.B).astype(np.uint32)
    a[case.B - 1] = RARE
    return a
