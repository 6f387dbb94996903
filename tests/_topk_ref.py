"""The exact top-k contract of topk.hip / topk_keys.h restated on bit patterns, in numpy only.

A score is its 32-bit pattern u.  Its key is  (hi << 32) | ~position  with  hi = ~u if the sign bit is set, else u | 0x80000000; the answer of a
selection is the k largest 64-bit keys, descending.  Nothing here is float arithmetic: +0.0 (hi 0x80000000) lies strictly above -0.0
(hi 0x7FFFFFFF), a sign-clear NaN above +inf, a sign-set NaN below -inf.  Shares nothing with oracle.select_topk_deterministic.

EXCLUDED INPUT: the pattern 0xFFFFFFFF (a sign-set NaN with every payload bit set).  Its hi is 0, the padding key of the kernels ("no element
here"); it is not a score.  No row family below produces it (`_checked` asserts that).

Also here: the host dispatch of topk() (`route`), the fast path's thread layout and lower bound (`fast_path_survivors`), the sort a slot count
takes (`emit_branch`), traces of the two radix selections, the row families, the case table the GPU test runs and the CPU test walks, and the
bug classes ("mutants") the CPU test applies to this restatement.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np

# ---- constants copied from rails_amd/csrc/topk.hip and topk_keys.h ---------------------------------------------------------------
kSortCap = 16384            # 64-bit keys one workgroup sorts in LDS (sort_emit_kernel, merge_candidates_kernel)
kSortThreads = 1024         # workgroup of the in-LDS sorts
kRowThreads = 1024          # workgroup of row_select_kernel
kRowMaxK = 4096             # largest k of row_select_kernel
kRowMaxN = 48 * kRowThreads  # largest row (or chunk) one workgroup holds in registers: 49 152
kRowFastK = 512             # largest k of the fast path; also the two-level path's largest k without a launch predicate
kRowCandCap = 4096          # survivors the fast path may hand to its sort (lds_keys)
kLevel2Keys = 24 * kRowThreads   # keys per row the second level holds: 24 576
kHalfChunkRows = 8          # up to this many rows the first level's chunks are kRowMaxN / 2
kRadixWgs = 1024            # workgroups per radix launch
kRadixMinChunk = 8192       # at least this many elements per radix workgroup
kRadixPassShift = (53, 42, 32)   # the three radix passes over the score word: 11 / 11 / 10 bits
kRadixPassBits = (11, 11, 10)
kCompactStage = 2048        # selected keys one compact_kernel workgroup stages in LDS before it walks its chunk a second time
kIndexedMaxN = 8 * kRowThreads   # candidate rows (ids through an index) on row_select_kernel: 512 < n <= 8 192
kFuseMaxK = 512             # k' of the fused seen-id filter
kFuseMaxW = 256             # seen ids per row
VPT_SCORES = (4, 8, 16, 28, 40, 48)
VPT_INDEXED = (4, 8)
VPT_KEYS = (4, 8, 16, 24)
SORT_KINDS = ("block_sort_desc<64", "block_rank_desc", "block_sort_desc", "multi<2>", "multi<4>", "multi<8>", "multi<16>")
EMIT_BRANCHES = ("block_sort_desc<64", "block_rank_desc", "block_sort_desc", "lds_bitonic")
RADIX_SETTLES = ("pass0", "pass1", "pass2", "tie")     # early: pass0 / pass1; late: pass2 / tie (tie_resolve_kernel completes the key)

U32 = np.uint32
U64 = np.uint64
EXCLUDED = 0xFFFFFFFF


def next_pow2(v: int, at_least: int = 1) -> int:
    p = at_least
    while p < v:
        p <<= 1
    return p


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def orderable(bits: np.ndarray) -> np.ndarray:
    u = np.asarray(bits, dtype=U32)
    return np.where((u >> U32(31)).astype(bool), ~u, u | U32(0x80000000)).astype(U32)


def unorderable(hi: np.ndarray) -> np.ndarray:
    h = np.asarray(hi, dtype=U32)
    return np.where((h >> U32(31)).astype(bool), h & U32(0x7FFFFFFF), ~h).astype(U32)


def keys(row_bits: np.ndarray, first_position: int = 0) -> np.ndarray:
    u = np.asarray(row_bits, dtype=U32)
    pos = (np.arange(u.shape[0], dtype=np.int64) + first_position).astype(U32)
    return (orderable(u).astype(U64) << U64(32)) | (~pos).astype(U64)


def decode(kv: np.ndarray):
    """keys -> (score bit patterns uint32, positions int64)"""
    kv = np.asarray(kv, dtype=U64)
    return unorderable((kv >> U64(32)).astype(U32)), (~(kv & U64(0xFFFFFFFF)).astype(U32)).astype(np.int64)


def select(row_bits: np.ndarray, k: int):
    """the k largest keys of the row, descending -> (score bit patterns uint32[k], positions int64[k])"""
    kv = np.sort(keys(row_bits))[::-1][:k]
    return decode(kv)


def filter_seen(ids, scores, invalid, k):
    """The seen-id filter over a row's k' selected candidates, best first, in plain loops: the first k not-seen ones are valid; when fewer than
    k exist the earliest of the others (seen, or beyond the first k) fill up; the output is what was picked, in candidate order."""
    seen = set(int(x) for x in invalid)
    valid = []
    for j in range(len(ids)):
        if int(ids[j]) not in seen and len(valid) < k:
            valid.append(j)
    others = [j for j in range(len(ids)) if j not in set(valid)]
    picked = sorted(valid + others[: k - len(valid)])
    return np.array([ids[j] for j in picked], dtype=np.int64), np.array([scores[j] for j in picked], dtype=U32)


def merged(messages: np.ndarray, R: int, k: int, k_out: int):
    """messages (R, rows, 2k) int64: [k score words | k ids] per rank and row.  Entry (r, j) has position r * k + j; the k_out largest keys of
    every row, descending -> (score bit patterns (rows, k_out), ids (rows, k_out))."""
    messages = np.asarray(messages, dtype=np.int64).reshape(R, -1, 2 * k)
    rows = messages.shape[1]
    out_s = np.zeros((rows, k_out), dtype=U32)
    out_i = np.zeros((rows, k_out), dtype=np.int64)
    for row in range(rows):
        words = np.concatenate([(messages[r, row, :k] & 0xFFFFFFFF).astype(U32) for r in range(R)])
        s, pos = select(words, k_out)
        out_s[row] = s
        for j, p in enumerate(pos):
            out_i[row, j] = messages[int(p) // k, row, k + int(p) % k]
    return out_s, out_i


# ---- the host dispatch of topk() ---------------------------------------------------------------------------------------------------
def sort_kind(npad: int) -> str:
    """the sort of sort_emit_kernel / lds_sort_desc for npad slots (final output)"""
    if 64 <= npad <= 512:
        return "block_rank_desc"
    if npad < 64:
        return "block_sort_desc<64"
    if npad <= kSortThreads:
        return "block_sort_desc"
    return "multi<%d>" % (npad // kSortThreads)


def emit_branch(count: int) -> str:
    """the sort emit_sorted() of row_select_kernel takes for `count` keys (npad = next_pow2(count, 2))"""
    npad = next_pow2(count, 2)
    if 64 <= npad <= 512:
        return "block_rank_desc"
    if npad < 64:
        return "block_sort_desc<64"
    if npad <= kRowThreads:
        return "block_sort_desc"
    return "lds_bitonic"


def _vpt(elements: int, choices) -> int:
    for v in choices:
        if elements <= v * kRowThreads:
            return v
    raise ValueError("row select: %d elements per workgroup" % elements)


def _two_level_plan_at(n, k, max_chunk):
    c = (n + max_chunk - 1) // max_chunk
    if c * k > kLevel2Keys:
        return None
    ln = (n + c - 1) // c
    ln = (ln + 3) // 4 * 4
    if ln > kRowMaxN or ln < k:
        return None
    chunks = (n + ln - 1) // ln
    if n - (chunks - 1) * ln < k:
        return None
    return chunks, ln


def two_level_plan(n, k, rows, max_k):
    if k > max_k:
        return None
    first = kRowMaxN // 2 if rows <= kHalfChunkRows else kRowMaxN
    plan = _two_level_plan_at(n, k, first)
    if plan is None and first != kRowMaxN:
        plan = _two_level_plan_at(n, k, kRowMaxN)
    return plan


def route(rows: int, n: int, k: int, *, fused: bool = False, indexed: bool = False, predicated: bool = False):
    """-> (name, params) as topk() in topk.hip dispatches a call of `rows` rows of n scores"""
    assert 1 <= k <= n and k <= kSortCap and n < (1 << 32)
    if fused and not indexed:
        ok = n > 1024 and k <= kFuseMaxK and (n <= kRowMaxN or two_level_plan(n, k, 1 << 30, kRowFastK) is not None)
        if not ok:
            raise ValueError("the seen-id filter cannot be fused at n = %d, k = %d" % (n, k))
    sort_whole = k > kRowFastK and n <= kSortCap and next_pow2(n) <= next_pow2(k) and not fused
    if not sort_whole and indexed and 512 < n <= kIndexedMaxN and k <= kRowMaxK:
        return "row_select", {"vpt": _vpt(n, VPT_INDEXED), "indexed": True}
    if indexed and n > kSortCap:
        raise ValueError("ids_index needs n <= %d" % kSortCap)
    if indexed and fused:
        raise ValueError("the seen-id filter over candidate rows needs 1024 < n <= %d" % kIndexedMaxN)
    if not sort_whole and (n > 1024 or (n > 512 and k <= kRowFastK and not fused)) and k <= kRowMaxK and not indexed:
        if n <= kRowMaxN:
            return "row_select", {"vpt": _vpt(n, VPT_SCORES), "indexed": False}
        plan = two_level_plan(n, k, rows, kRowMaxK if predicated else kRowFastK)
        if plan is not None:
            chunks, chunk = plan
            return "two_level", {"chunks": chunks, "chunk": chunk, "vpt": _vpt(chunk, VPT_SCORES), "vpt2": _vpt(chunks * k, VPT_KEYS),
                                 "halved": rows <= kHalfChunkRows and chunk <= kRowMaxN // 2}
    if n <= kSortCap:
        npad = next_pow2(n, 2)
        return "sort_whole", {"npad": npad, "sort": sort_kind(npad)}
    npad = next_pow2(k, 2)
    chunks = (kRadixWgs + rows - 1) // rows
    chunks = max(1, min(chunks, (n + kRadixMinChunk - 1) // kRadixMinChunk))
    return "radix", {"chunks": chunks, "chunk": (n + chunks - 1) // chunks, "npad": npad, "sort": sort_kind(npad)}


# ---- row_select_kernel's fast path -------------------------------------------------------------------------------------------------
def owner_thread(index: np.ndarray) -> np.ndarray:
    """SCORES source: thread t owns elements (jv * 1024 + t) * 4 .. + 3"""
    return (np.asarray(index) // 4) % kRowThreads


def fast_path_survivors(row_bits: np.ndarray, k: int, vpt: int, layout: str = "scores"):
    """-> (L, S): the 16-bit lower bound the fast path resolves from the per-thread maxima, four bits per step, and the number of elements
    v >= L it compacts.  `row_bits` is what one workgroup holds (a row, or a chunk); layout "keys": thread t owns keys j * 1024 + t."""
    return _survivors(orderable(row_bits), k, vpt, layout)


def _survivors(hi: np.ndarray, k: int, vpt: int, layout: str):
    n = hi.shape[0]
    assert n <= vpt * kRowThreads
    idx = np.arange(n)
    thread = owner_thread(idx) if layout == "scores" else idx % kRowThreads
    tmax = np.zeros(kRowThreads, dtype=U32)
    np.maximum.at(tmax, thread, hi)
    L = 0
    for shift in (28, 24, 20, 16):
        digit = 0
        for d in range(1, 16):
            if int(np.count_nonzero(tmax >= U32(L | (d << shift)))) >= k:
                digit += 1          # the count is monotone in d: the digit is the number of thresholds that k threads reach
        L |= digit << shift
    return L, int(np.count_nonzero(hi >= U32(L)))


def radix_select_trace(kv: np.ndarray, want: int):
    """radix_select() over a workgroup's keys, eight bits per pass, bytes all keys agree on skipped, stop once every key that still matches is
    wanted -> {"passes", "position_passes", "early": the passes stopped inside the score word, "selected": number of keys selected}"""
    kv = np.asarray(kv, dtype=U64)
    want = min(want, kv.shape[0])
    vor, vand = int(np.bitwise_or.reduce(kv)), int(np.bitwise_and.reduce(kv))
    varying = vor ^ vand
    prefix = fixed = 0
    need, passes, pos_passes, stop_byte = want, 0, 0, -1
    for byte in range(7, -1, -1):
        mask = 0xFF << (8 * byte)
        if varying & mask == 0:
            prefix |= vor & mask
            fixed |= mask
            continue
        act = kv[(kv & U64(fixed)) == U64(prefix)]
        hist = np.bincount(((act >> U64(8 * byte)) & U64(255)).astype(np.int64), minlength=256)
        cum = 0
        for digit in range(255, -1, -1):
            if cum < need <= cum + hist[digit]:
                break
            cum += int(hist[digit])
        prefix |= digit << (8 * byte)
        fixed |= mask
        need -= cum
        passes += 1
        pos_passes += 1 if byte < 4 else 0
        if int(hist[digit]) == need:
            stop_byte = byte
            break
    selected = int(np.count_nonzero((kv & U64(fixed)) >= U64(prefix)))
    return {"passes": passes, "position_passes": pos_passes, "early": stop_byte >= 4, "selected": selected}


def row_select_trace(row_bits: np.ndarray, k: int, vpt: int, first_position: int = 0):
    """what one row_select_kernel workgroup does with its elements -> {"path": "fast" | "overflow" | "large_k", "S", "L", "branch", ...}"""
    if k <= kRowFastK:
        L, S = fast_path_survivors(row_bits, k, vpt)
        if S <= kRowCandCap:
            return {"path": "fast", "L": L, "S": S, "branch": emit_branch(S)}
        t = radix_select_trace(keys(row_bits, first_position), k)
        return dict(t, path="overflow", L=L, S=S, branch=emit_branch(k))
    t = radix_select_trace(keys(row_bits, first_position), k)
    return dict(t, path="large_k", L=None, S=None, branch=emit_branch(k))


def two_level_trace(row_bits: np.ndarray, k: int, p: dict):
    """the two launches on one row: the path every first-level workgroup takes on its chunk, and the path of the second level over the
    chunks * k winners (KEYS source: thread t owns keys j * 1024 + t) -> {"level1": set of paths, "level2": path, "S2": its survivors}"""
    kv = keys(row_bits)
    level1, winners = set(), []
    for c in range(p["chunks"]):
        lo, hi = c * p["chunk"], min((c + 1) * p["chunk"], row_bits.shape[0])
        level1.add(row_select_trace(row_bits[lo:hi], k, p["vpt"], lo)["path"])
        winners.append(np.sort(kv[lo:hi])[::-1][:k])
    lvl1 = np.concatenate(winners)
    if k > kRowFastK:
        return {"level1": level1, "level2": "large_k", "S2": None}
    _, S2 = _survivors((lvl1 >> U64(32)).astype(U32), k, p["vpt2"], "keys")
    return {"level1": level1, "level2": "fast" if S2 <= kRowCandCap else "overflow", "S2": S2}


def radix_trace(row_bits: np.ndarray, k: int, rows: int = 1):
    """the multi-launch radix path on one row: pick_bin_kernel's three passes over the score word -> {"settle", "kept": keys the compaction
    keeps (<= npad), "second_walk": some compact_kernel workgroup holds more than its stage}"""
    n = row_bits.shape[0]
    npad = next_pow2(k, 2)
    kv = keys(row_bits)
    prefix, need, settle = 0, k, "tie"
    for p, (shift, bits) in enumerate(zip(kRadixPassShift, kRadixPassBits)):
        above = shift + bits
        act = kv if above >= 64 else kv[(kv >> U64(above)) == U64(prefix >> above)]
        hist = np.bincount(((act >> U64(shift)) & U64((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)
        cum = 0
        for b in range((1 << bits) - 1, -1, -1):
            if cum + hist[b] >= need:
                break
            cum += int(hist[b])
        c, still = int(hist[b]), need - cum
        prefix |= b << shift
        need = still
        if c == still or k - still + c <= npad:
            settle = "pass%d" % p
            break
    if settle == "tie":       # tie_resolve_kernel: the position of the need-th element, in position order, whose score word is the prefix's
        at = np.flatnonzero((kv >> U64(32)) == U64(prefix >> 32))[need - 1]
        prefix = int(kv[at])
    sel = kv >= U64(prefix)
    chunks = route(rows, n, k)[1]["chunks"] if n > kSortCap else 1
    chunk = (n + chunks - 1) // chunks
    per_chunk = np.add.reduceat(sel.astype(np.int64), np.arange(0, n, chunk))
    return {"settle": settle, "kept": int(sel.sum()), "second_walk": bool(per_chunk.max() > kCompactStage)}


# ---- row families: bit patterns, fixed seeds ---------------------------------------------------------------------------------------
def _checked(bits: np.ndarray) -> np.ndarray:
    bits = np.ascontiguousarray(bits, dtype=U32)
    assert not np.any(bits == U32(EXCLUDED)), "0xFFFFFFFF is not a score"
    return bits


def _f2b(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float32).view(U32)


def _distinct_normals(n: int, rng, transform=lambda x: x) -> np.ndarray:
    """n distinct fp32 values of transform(standard normal), in random order, no zeros"""
    have = np.zeros(0, dtype=U32)
    while have.shape[0] < n:
        x = transform(rng.standard_normal(n + n // 4 + 64).astype(np.float32)).astype(np.float32)
        have = np.unique(np.concatenate([have, _f2b(x[x != 0])]))
    return rng.permutation(have)[:n]


def gauss(n, k, rng):
    return _distinct_normals(n, rng)


def all_negative(n, k, rng):      # the ~u branch of the codec on every element
    return _distinct_normals(n, rng, lambda x: -np.abs(x) - np.float32(1e-3))


def narrow(n, k, rng):
    """distinct values sharing their top 16 bits (rows of up to 49 152; longer rows cannot be distinct inside 2^16 patterns and share the top
    11 bits, the first radix pass' bin, instead)"""
    if n <= kRowMaxN:
        return (U32(0x3DCC0000) | rng.permutation(1 << 16)[:n].astype(U32)).astype(U32)
    return (U32(0x3DC00000) | rng.choice(1 << 21, size=n, replace=False).astype(U32)).astype(U32)


def low_byte(n, k, rng):          # values that differ in the lowest mantissa byte only: the radix passes skip the bytes all keys agree on
    return (U32(0x3F800000) | rng.integers(0, 256, size=n).astype(U32)).astype(U32)


def constant(n, k, rng):
    return np.full(n, 0x3F000000, dtype=U32)


def signed_zeros(n, k, rng):
    """k // 3 small positive values, about k zeros -- alternately -0.0 and +0.0 in position order, -0.0 first -- and small negative values:
    the k-th place lies among the zeros, where +0.0 ranks above every -0.0 whatever its position"""
    out = _distinct_normals(n, rng, lambda x: -np.abs(x) * np.float32(1e-3) - np.float32(1e-6))
    order = rng.permutation(n)
    npos = min(k // 3, max(n - 2, 0))
    out[order[:npos]] = _distinct_normals(npos, rng, lambda x: np.abs(x) * np.float32(1e-3) + np.float32(1e-6)) if npos else out[order[:0]]
    zeros = np.sort(order[npos: npos + max(2, k)])
    out[zeros[0::2]] = U32(0x80000000)
    out[zeros[1::2]] = U32(0x00000000)
    return out


def subnormals(n, k, rng):
    """subnormal values of distinct magnitudes: k // 2 positive ones, the rest negative, so that the k-th place lies among the negative
    subnormals"""
    mag = (rng.choice(0x7FFFFF - 1, size=n, replace=False) + 1).astype(U32)
    sign = np.ones(n, dtype=U32)
    sign[rng.permutation(n)[: k // 2]] = 0
    return mag | (sign << U32(31))


NAN_PATTERNS = (0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7F800001, 0x7FFFFFFF, 0xFFC12345, 0xFF800001, 0xFFFFFFFE,
                0x7F800000, 0xFF800000)     # quiet / signalling NaNs of both signs with payloads, then +inf and -inf


def nans(n, k, rng):
    out = _distinct_normals(n, rng)
    copies = 3 if n >= 64 else 1
    special = np.tile(np.array(NAN_PATTERNS, dtype=U32), copies)[:n]
    out[rng.permutation(n)[: special.shape[0]]] = special
    return out


def ascending(n, k, rng):         # every winner at the end of the row: the last threads of the last float4 run, the ragged tail, the last chunk
    b = _distinct_normals(n, rng)
    return b[np.argsort(orderable(b))]


def descending(n, k, rng):        # every winner at the front: chunk 0, thread 0 onwards
    return ascending(n, k, rng)[::-1].copy()


def one_thread(n, k, rng, where="thread"):
    """the k + 3 largest values sit in as few threads as hold them ("thread"), in the 64 threads of one wave ("wave"), at the very end of the
    row, the last n % 4 elements after the last full float4 first ("tail"), or in one run of consecutive elements in the middle of the row
    ("run": one radix workgroup's chunk holds every winner); everything else lies far below.  All values are distinct."""
    out = _distinct_normals(n, rng, lambda x: x - np.float32(100.0))
    idx = np.arange(n)
    thread = owner_thread(idx)
    if where == "thread":
        order = np.lexsort((idx, (thread - 517) % kRowThreads))
    elif where == "wave":
        order = np.lexsort((idx, thread % 64, ((thread // 64) - 5) % 16))
    elif where == "run":
        order = (idx + n // 2) % n
    else:
        order = idx[::-1]
    m = min(n, k + 3)
    out[order[:m]] = _distinct_normals(m, rng, lambda x: np.abs(x) + np.float32(2.0))
    return out


def planted(n, k, rng, S=64):
    """exactly S elements share the top 16-bit pattern 0x4000 (values in [2, 2.0078)), dealt over min(S, 1024) threads; the rest lies below
    -900; the planted element of the highest position holds the row's maximum.  With k <= min(S, 1024) the fast path resolves
    L = orderable(0x40000000) and compacts exactly these S."""
    assert k <= min(S, kRowThreads)
    out = _distinct_normals(n, rng, lambda x: x - np.float32(1000.0))
    i = np.arange(S)
    t, slot = i % kRowThreads, i // kRowThreads
    pos = ((slot // 4) * kRowThreads + t) * 4 + slot % 4
    assert pos.max() < n
    low = rng.permutation(1 << 16)[:S].astype(U32)
    a, b = int(np.argmax(pos)), int(np.argmax(low))
    low[[a, b]] = low[[b, a]]
    out[pos] = U32(0x40000000) | low
    return out


def tie_at_kth(n, k, rng, extra=0):
    """k - 1 distinct values in [2, 3), a tie group of extra + 2 elements at 1.0 -- the k-th place and the one after it inside the group --
    and values in [0, 0.5) below"""
    g = min(extra + 2, n - (k - 1))
    out = _f2b(rng.random(n).astype(np.float32) * np.float32(0.5))
    perm = rng.permutation(n)
    out[perm[: k - 1]] = U32(0x40000000) | rng.choice(1 << 22, size=k - 1, replace=False).astype(U32)
    out[perm[k - 1: k - 1 + g]] = U32(0x3F800000)
    return out


FAMILIES = {f.__name__: f for f in (gauss, all_negative, narrow, low_byte, constant, signed_zeros, subnormals, nans, ascending, descending,
                                    one_thread, planted, tie_at_kth)}
# the families every route runs at one shape (the planted and edge cases come on top)
EVERY_ROUTE = (("gauss", {}), ("all_negative", {}), ("narrow", {}), ("low_byte", {}), ("signed_zeros", {}), ("subnormals", {}), ("nans", {}),
               ("ascending", {}), ("descending", {}), ("one_thread", {"where": "thread"}), ("one_thread", {"where": "wave"}),
               ("one_thread", {"where": "tail"}), ("tie_at_kth", {"extra": 5}), ("constant", {}))


# ---- the case table ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    entry: str                      # topk | topk_filtered | topk_candidates | topk_candidates_filtered | merge | merge_filtered
    n: int                          # columns (merge: k entries per rank)
    k: int                          # k, or k' of the filtered entries (merge: k_out resp. k')
    rows: tuple                     # ((family, params), ...), one per row, cycled up to nrows
    route: str                      # the route the case is there for
    nrows: int = 0
    want: tuple = ()                # per row: None, or a dict of row_select_trace / radix_trace items the row must show
    run_if: Optional[int] = None    # None: no launch predicate; 1 / 0: a predicate that lets the call run / keeps it from running
    k_out: int = 0                  # filtered entries: results per row
    width: int = 0                  # filtered entries: seen ids per row
    R: int = 0                      # merge: ranks
    unsorted: bool = False          # merge: rank 1's list is handed over unsorted

    @property
    def n_rows(self):
        return self.nrows or len(self.rows)

    @property
    def fused(self):
        return self.entry in ("topk_filtered", "topk_candidates_filtered")

    @property
    def indexed(self):
        return self.entry in ("topk_candidates", "topk_candidates_filtered")

    def seed(self, row: int) -> int:
        return zlib.crc32(self.name.encode()) * 31 + row


def _fam(name, **params):
    return (name, params)


def _cases():
    out = []

    def add(name, entry, n, k, rows, route_name, **kw):
        out.append(Case(name=name, entry=entry, n=n, k=k, rows=tuple(rows), route=route_name, **kw))

    tie, nan_, neg, zer = _fam("tie_at_kth", extra=3), _fam("nans"), _fam("all_negative"), _fam("signed_zeros")
    # -- sort_whole: block_sort_desc, block_rank_desc and block_sort_desc_multi<2 / 4 / 8 / 16> (gauss rows stay out of the k = n cases: see
    #    test_topk_keys_cpu, "the bars can fail")
    for n in (1, 2, 63, 64, 65, 512):
        for k in sorted({1, n}):
            add(f"sort_whole-{n}-{k}", "topk", n, k, [nan_, zer, neg], "sort_whole")
    for n, k in ((1000, 513), (2048, 1025), (3883, 3883), (4096, 2561), (8192, 4097), (16384, 16384)):
        add(f"sort_whole-{n}-{k}", "topk", n, k, [nan_, _fam("tie_at_kth", extra=min(3, n - k)), _fam("subnormals")], "sort_whole")
    # -- row_select, fast path: the survivor count on both sides of every sort of emit_sorted, and of the capacity
    for S in (2, 32, 33, 63, 64, 65, 512, 513, 1024, 1025, 4095, 4096, 4097):
        shapes = [(5000, 1)] + ([(5000, 120)] if S >= 120 else []) + ([(49152, 512)] if S >= 512 else [])
        for n, k in shapes:
            w = {"path": "fast" if S <= kRowCandCap else "overflow", "S": S, "L": 0xC0000000}
            if S <= kRowCandCap:
                w["branch"] = emit_branch(S)
            add(f"planted-{S}-{n}-{k}", "topk", n, k, [_fam("planted", S=S), _fam("planted", S=S)], "row_select", want=(w, w))
    for n in (513, 1024, 1025):     # fewer than k threads hold an element: L = 0, every element survives
        w = {"path": "fast", "L": 0, "S": n}
        add(f"fast-L0-{n}", "topk", n, 512, [neg, nan_, tie], "row_select", want=(w, w, w))
    for n in (4096, 4097, 8192, 8193, 16384, 16385, 28672, 28673, 40960, 40961, 49151, 49152):      # both sides of every VPT edge
        add(f"vpt-edge-{n}", "topk", n, 200, [_fam("gauss"), _fam("one_thread", where="tail"), tie], "row_select")
    # -- row_select, general path: through overflow ...
    for k in (1, 511, 512):
        add(f"overflow-5000-{k}", "topk", 5000, k, [_fam("narrow"), _fam("low_byte"), _fam("constant"), _fam("tie_at_kth", extra=4500 - k)],
            "row_select", want=({"path": "overflow"},) * 4)
    add("overflow-49152-512", "topk", 49152, 512, [_fam("narrow"), _fam("low_byte"), _fam("tie_at_kth", extra=6000)], "row_select",
        want=({"path": "overflow"},) * 3)
    add("overflow-early-exit", "topk", 5000, 120, [_fam("planted", S=4097)], "row_select", want=({"path": "overflow", "early": True},))
    add("overflow-position-bytes", "topk", 5000, 120, [_fam("constant"), _fam("low_byte")], "row_select",
        want=({"path": "overflow", "early": False}, {"path": "overflow", "early": False}))
    # ... and through k > 512
    for n in (5000, 49152):
        for k in (513, 1025, 4096):
            add(f"large-k-{n}-{k}", "topk", n, k, [_fam("narrow"), nan_, _fam("tie_at_kth", extra=7), _fam("low_byte")], "row_select",
                want=({"path": "large_k"},) * 4)
    # -- two_level
    for n in (49153, 98305):
        for k in (1, 200, 512):
            for nrows in (2, 9):
                add(f"two-level-{n}-{k}-r{nrows}", "topk", n, k, [_fam("ascending"), _fam("descending"), _fam("gauss"), tie, nan_], "two_level",
                    nrows=nrows)
    add("two-level-full-chunks", "topk", 98304, 200, [_fam("ascending"), _fam("descending"), _fam("gauss")], "two_level", nrows=9)
    add("two-level-8-keys-per-thread", "topk", 12 * 24576, 512, [_fam("gauss")], "two_level")
    add("two-level-16-keys-per-thread", "topk", 20 * 24576, 512, [_fam("tie_at_kth", extra=9)], "two_level")
    add("two-level-48x512", "topk", 48 * 24576, 512, [_fam("gauss")], "two_level")
    w = {"level1": {"overflow"}, "level2": "overflow", "S2": 12 * 512}      # the second level's fast path overflows too: 6 144 keys in one 16-bit bucket
    add("two-level-second-level-overflow", "topk", 12 * 24576, 512, [_fam("constant"), _fam("low_byte")], "two_level", want=(w, w))
    add("two-level-predicated-4096", "topk", 200000, 4096, [_fam("gauss"), _fam("tie_at_kth", extra=50)], "two_level", run_if=1)
    # -- radix
    add("radix-49153-513", "topk", 49153, 513, [_fam("gauss"), _fam("narrow"), neg, nan_], "radix")
    for k in (1500, 6000, 16384):      # the final sort at 2, 8 and 16 keys per thread
        add(f"radix-70001-{k}", "topk", 70001, k, [_fam("gauss"), _fam("tie_at_kth", extra=next_pow2(k) - k)], "radix")
    for k in (2561, 4096):
        npad = next_pow2(k)
        rows = [_fam("gauss"), _fam("narrow"), neg, nan_, _fam("low_byte"), _fam("tie_at_kth", extra=npad - k - 1),
                _fam("tie_at_kth", extra=npad - k)] if k == 2561 else \
               [_fam("gauss"), _fam("constant"), _fam("tie_at_kth", extra=1), _fam("tie_at_kth", extra=2)]
        want = (None,) * 4 + ({"settle": "pass2"}, {"settle": "pass0", "kept": npad}, {"settle": "tie", "kept": k}) if k == 2561 else \
               (None, {"settle": "tie", "second_walk": True}, {"settle": "tie"}, {"settle": "tie"})
        add(f"radix-200000-{k}", "topk", 200000, k, rows, "radix", want=want)
    add("radix-second-walk", "topk", 200000, 2561, [_fam("one_thread", where="run"), _fam("one_thread", where="run")], "radix",
        want=({"settle": "pass0", "second_walk": True}, {"settle": "pass0", "second_walk": True}))
    add("radix-small-k", "topk", 48 * 49152 + 1, 512, [_fam("gauss")], "radix")
    # -- a launch predicate of 0 leaves the outputs alone on every route (and one of 1 changes nothing)
    for tag, n, k in (("sort_whole", 300, 20), ("row_select", 5000, 120), ("two_level", 49153, 200), ("radix", 70001, 5000)):
        for flag in (0, 1):
            add(f"run-if-{flag}-{tag}", "topk", n, k, [_fam("gauss"), tie], tag, run_if=flag)
    # -- every family on every route
    for tag, n, k in (("sort_whole", 500, 100), ("row_select", 5003, 120), ("two_level", 60001, 200), ("radix", 70001, 600)):
        for fam, params in EVERY_ROUTE:
            label = fam + ("-" + params["where"] if "where" in params else "")
            add(f"family-{tag}-{label}", "topk", n, k, [(fam, params), (fam, params)], tag)
    # -- the fused seen-id filter and the candidate rows
    special = [tie, nan_, zer, _fam("low_byte")]
    add("filtered-row-select", "topk_filtered", 5003, 300, special, "row_select", k_out=260, width=64)
    add("filtered-row-select-backfill", "topk_filtered", 1025, 100, special, "row_select", k_out=90, width=40)
    add("filtered-two-level", "topk_filtered", 60001, 512, special, "two_level", k_out=500, width=256)
    add("filtered-run-if-0", "topk_filtered", 5003, 300, special[:2], "row_select", k_out=260, width=64, run_if=0)
    for n in (512, 513, 4096, 4097, 8192, 8193, 16384):
        route_name = "row_select" if 512 < n <= kIndexedMaxN else "sort_whole"
        add(f"candidates-{n}", "topk_candidates", n, 200, special, route_name)
    add("candidates-4097-1000", "topk_candidates", 4097, 1000, special, "row_select")
    for n in (1025, 8192):
        add(f"candidates-filtered-{n}", "topk_candidates_filtered", n, 300, special, "row_select", k_out=280, width=64)
    # -- merge of per-rank lists
    for R in (2, 8):
        for k in (1, 200):
            for unsorted in (False, True):
                if unsorted and k == 1:
                    continue          # a list of one entry is sorted
                add(f"merge-R{R}-k{k}" + ("-unsorted" if unsorted else ""), "merge", k, k, [_fam("gauss"), _fam("low_byte"), nan_, zer, _fam("constant")],
                    "merge", R=R, unsorted=unsorted)
    add("merge-filtered-R8", "merge_filtered", 200, 300, [_fam("low_byte"), nan_, zer], "merge", R=8, k_out=250, width=64)
    add("merge-filtered-R2-unsorted", "merge_filtered", 200, 200, [_fam("low_byte"), nan_], "merge", R=2, k_out=180, width=30, unsorted=True)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


CASES = _cases()
CASE = {c.name: c for c in CASES}
BIG_CASES = ("two-level-48x512", "radix-small-k")     # one long row each: rows and references are built once per process


def _build_rows(case: Case) -> np.ndarray:
    if case.route == "merge":
        raise ValueError("merge cases build messages (case_messages)")
    rows = []
    for r in range(case.n_rows):
        fam, params = case.rows[r % len(case.rows)]
        rows.append(_checked(FAMILIES[fam](case.n, case.k, np.random.default_rng(case.seed(r)), **params)))
    return np.stack(rows)


@functools.lru_cache(maxsize=4)
def _cached_rows(name):
    return _build_rows(CASE[name])


def case_rows(case: Case) -> np.ndarray:
    """(rows, n) uint32 score bit patterns of a selection case"""
    return _cached_rows(case.name) if case.name in BIG_CASES else _build_rows(case)


@functools.lru_cache(maxsize=4)
def _cached_expected(name):
    return _expected_selection(CASE[name], _cached_rows(name), select)


def _expected_selection(case, bits, select_fn):
    s = np.zeros((bits.shape[0], case.k), dtype=U32)
    p = np.zeros((bits.shape[0], case.k), dtype=np.int64)
    for r in range(bits.shape[0]):
        s[r], p[r] = select_fn(bits[r], case.k)
    return s, p


def case_selection(case: Case, bits: np.ndarray, select_fn=None):
    """(score bit patterns, positions) (rows, k) of the k largest keys of every row"""
    if select_fn is None and case.name in BIG_CASES:
        return _cached_expected(case.name)
    return _expected_selection(case, bits, select_fn or select)


def case_ids(case: Case, index: int):
    """How the case names its items: (mode, table).  The modes rotate over the table: positions themselves, one shared id row, ids per row.
    Candidate rows (the indexed entries) carry (rows, n) corpus positions and, every other case, a flat id table over the corpus."""
    rng = np.random.default_rng(case.seed(1000))
    n, rows = case.n, case.n_rows
    if case.indexed:
        corpus = 3 * n + 7
        positions = np.stack([rng.permutation(corpus)[:n] for _ in range(rows)]).astype(np.int64)
        table = (rng.permutation(corpus).astype(np.int64) * 5 + 11) if index % 2 == 0 else None
        return "indexed", (positions, table)
    mode = ("positions", "shared", "per_row")[index % 3] if n <= 200000 else "positions"
    if mode == "shared":
        return mode, rng.permutation(n).astype(np.int64) * 3 + 1
    if mode == "per_row":
        return mode, np.stack([rng.permutation(n).astype(np.int64) * 7 + r for r in range(rows)])
    return mode, None


def map_ids(mode, table, row: int, pos: np.ndarray) -> np.ndarray:
    if mode == "positions":
        return pos.astype(np.int64)
    if mode == "shared":
        return table[pos]
    if mode == "per_row":
        return table[row][pos]
    positions, ids = table
    at = positions[row][pos]
    return at if ids is None else ids[at]


def case_invalid(case: Case, sel_ids: np.ndarray) -> np.ndarray:
    """(rows, width) seen ids: every third winner of the row and ids no item has.  Row 1 sees enough of its winners that fewer than k_out
    remain and the filter fills up with dropped ones."""
    rng = np.random.default_rng(case.seed(2000))
    rows, kp = sel_ids.shape
    inv = -2 - rng.integers(0, 1 << 40, size=(rows, case.width)).astype(np.int64)
    for r in range(rows):
        take = sel_ids[r, ::3] if r != 1 else sel_ids[r, : kp - case.k_out + 5]
        take = take[: case.width]
        inv[r, rng.permutation(case.width)[: take.shape[0]]] = take
    return inv


def case_messages(case: Case):
    """merge cases: (R, rows, 2k) int64 messages built here, not by the pack kernel.  Every rank's list holds the family's values in
    descending key order; a quarter of the score words are repeated across ranks; the last rank's list of the last row ends in two real -inf
    entries followed by four (-inf, -1) pads; `unsorted` hands over rank 1's list of every row reversed."""
    R, k, rows = case.R, case.n, case.n_rows
    msg = np.zeros((R, rows, 2 * k), dtype=np.int64)
    for row in range(rows):
        fam, params = case.rows[row % len(case.rows)]
        rng = np.random.default_rng(case.seed(row))
        words = _checked(FAMILIES[fam](R * k, min(k, R * k), rng, **params)).reshape(R, k).copy()
        if k >= 4:
            shared = rng.permutation(k)[: k // 4]
            words[1:, shared] = words[0, shared]            # equal score words across ranks
        ids = rng.permutation(R * k * 4)[: R * k].astype(np.int64).reshape(R, k) + 1
        if row == rows - 1 and k >= 8:
            words[R - 1, k - 6:] = U32(0xFF800000)
            ids[R - 1, k - 4:] = -1
        for r in range(R):
            order = np.argsort(-orderable(words[r]).astype(np.int64), kind="stable")      # descending; equal words keep their order: pads last
            if case.unsorted and r == 1:
                order = order[::-1]
            msg[r, row, :k] = words[r][order].astype(np.int64)
            msg[r, row, k:] = ids[r][order]
    return msg


def lists_sorted(msg: np.ndarray, R: int, k: int) -> bool:
    """whether every rank's list of every row is descending by key (the rank merge), else the kernel sorts (the bitonic branch)"""
    for r in range(R):
        for row in range(msg.shape[1]):
            kv = (orderable((msg[r, row, :k] & 0xFFFFFFFF).astype(U32)).astype(U64) << U64(32)) | (~(np.arange(k) + r * k).astype(U32)).astype(U64)
            if np.any(kv[:-1] < kv[1:]):
                return False
    return True


def case_route(case: Case):
    if case.route == "merge":
        return "merge", {"npad": next_pow2(case.R * case.n, 2)}
    return route(case.n_rows, case.n, case.k, fused=case.fused, indexed=case.indexed, predicated=case.run_if is not None)


def case_tags(case: Case, bits: Optional[np.ndarray] = None):
    """the (route, parameter, branch) tuples a case reaches, one set per case, and its per-row traces"""
    name, p = case_route(case)
    tags, traces = set(), []
    if name == "merge":
        msg = case_messages(case)
        tags.add(("merge", "rank_merge" if lists_sorted(msg, case.R, case.n) else "bitonic"))
        return tags, traces
    bits = case_rows(case) if bits is None else bits
    if name == "sort_whole":
        tags.add(("sort_whole", p["sort"]))
    elif name == "row_select":
        for r in range(bits.shape[0]):
            t = row_select_trace(bits[r], case.k, p["vpt"])
            traces.append(t)
            tags.add(("row_select", "indexed" if p["indexed"] else "scores", p["vpt"]))
            tags.add(("row_select", t["path"], t["branch"]))
            if t["path"] != "fast":
                tags.add(("row_select", "radix_select", "early" if t["early"] else "to_the_end"))
                if t["position_passes"]:
                    tags.add(("row_select", "radix_select", "position_bytes"))
    elif name == "two_level":
        tags.add(("two_level", "vpt2", p["vpt2"]))
        tags.add(("two_level", "chunk", "halved" if p["halved"] else "full"))
        tags.add(("two_level", "vpt", p["vpt"]))
        for r in range(bits.shape[0]):
            t = two_level_trace(bits[r], case.k, p)
            traces.append(t)
            tags |= {("two_level", "level1", path) for path in t["level1"]}
            tags.add(("two_level", "level2", t["level2"]))
    else:
        tags.add(("radix", "sort", p["sort"]))
        for r in range(bits.shape[0]):
            t = radix_trace(bits[r], case.k, bits.shape[0])
            traces.append(t)
            tags.add(("radix", "settle", t["settle"]))
            tags.add(("radix", "second_walk", t["second_walk"]))
    return tags, traces


def check_wants(case: Case, traces) -> None:
    for r, want in enumerate(case.want):
        if want:
            got = {key: traces[r].get(key) for key in want}
            assert got == want, f"{case.name} row {r} left its branch: wanted {want}, the row gives {got}"


# every value route(), emit_branch() and the traces can return, as the tags of case_tags
def universe():
    u = set()
    u |= {("sort_whole", s) for s in SORT_KINDS}
    u |= {("row_select", "scores", v) for v in VPT_SCORES} | {("row_select", "indexed", v) for v in VPT_INDEXED}
    u |= {("row_select", "fast", b) for b in EMIT_BRANCHES}
    u |= {("row_select", path, b) for path in ("overflow", "large_k") for b in EMIT_BRANCHES}
    u -= {("row_select", "large_k", "block_sort_desc<64"), ("row_select", "large_k", "block_rank_desc"),     # k > 512 sorts >= 1 024 slots
          ("row_select", "overflow", "block_sort_desc"), ("row_select", "overflow", "lds_bitonic")}          # k <= 512 sorts <= 512 slots
    u |= {("row_select", "radix_select", x) for x in ("early", "to_the_end", "position_bytes")}
    u |= {("two_level", "vpt2", v) for v in VPT_KEYS} | {("two_level", "chunk", c) for c in ("halved", "full")}
    u |= {("two_level", "vpt", v) for v in (28, 40, 48)}      # a chunk is longer than half the largest one: > 12 288 would do for 16, but n > 49 152 rules it out
    u |= {("two_level", lvl, path) for lvl in ("level1", "level2") for path in ("fast", "overflow", "large_k")}
    u |= {("radix", "settle", s) for s in RADIX_SETTLES} | {("radix", "second_walk", b) for b in (False, True)}
    u |= {("radix", "sort", s) for s in SORT_KINDS if s != "block_sort_desc<64"}     # k <= 32 of a row no two-level plan takes: n > 10^9
    u |= {("merge", b) for b in ("rank_merge", "bitonic")}
    return u


# ---- bug classes applied to the restatement ("mutants") ----------------------------------------------------------------------------
def _top(kv, k, decode_fn=decode):
    return decode_fn(np.sort(kv)[::-1][:k])


def _pad(s, p, k):
    """a selection that came up short: the missing places decode the padding key 0"""
    if s.shape[0] < k:
        s = np.concatenate([s, np.full(k - s.shape[0], EXCLUDED, dtype=U32)])
        p = np.concatenate([p, np.full(k - p.shape[0], 0xFFFFFFFF, dtype=np.int64)])
    return s, p


def _by_hi(hi, bits, k):
    """order by a replaced score word hi, position ascending, and report the elements' own bit patterns"""
    kv = (hi.astype(U64) << U64(32)) | (~np.arange(bits.shape[0]).astype(U32)).astype(U64)
    _, pos = _top(kv, k)
    return bits[pos], pos


def mutant_ties_position_descending(bits, k, case=None):
    kv = (orderable(bits).astype(U64) << U64(32)) | np.arange(bits.shape[0]).astype(U64)
    top = np.sort(kv)[::-1][:k]
    pos = (top & U64(0xFFFFFFFF)).astype(np.int64)
    return bits[pos], pos


def mutant_zeros_tied(bits, k, case=None):
    return _by_hi(orderable(np.where(bits == U32(0x80000000), U32(0), bits)), bits, k)


def mutant_nan_greatest(bits, k, case=None):          # the argsort rule: every NaN ties at the top
    is_nan = (bits & U32(0x7FFFFFFF)) > U32(0x7F800000)
    return _by_hi(np.where(is_nan, U32(0xFFFFFFFF), orderable(bits)), bits, k)


def mutant_negatives_raw(bits, k, case=None):         # negative floats compared as raw unsigned words (no ~u)
    neg = (bits >> U32(31)).astype(bool)
    return _by_hi(np.where(neg, bits & U32(0x7FFFFFFF), bits | U32(0x80000000)), bits, k)


def mutant_tail_dropped(bits, k, case=None):          # the last n % 4 elements never read
    n = bits.shape[0] - bits.shape[0] % 4
    s, p = select(bits[:n], min(k, n)) if n else (np.zeros(0, U32), np.zeros(0, np.int64))
    return _pad(s, p, k)


def mutant_survivors_truncated(bits, k, case):        # the fast path keeps the first 4 096 survivors, in position order, and never starts over
    name, p = case_route(case)
    if name != "row_select" or k > kRowFastK:
        return select(bits, k)
    L, S = fast_path_survivors(bits, k, p["vpt"])
    if S <= kRowCandCap:
        return select(bits, k)
    idx = np.flatnonzero(orderable(bits) >= U32(L))[:kRowCandCap]
    return _pad(*_top(keys(bits)[idx], k), k)


def mutant_chunk_k_minus_1(bits, k, case):            # every first-level chunk hands on k - 1 winners (one at k = 1)
    name, p = case_route(case)
    if name != "two_level":
        return select(bits, k)
    kv = keys(bits)
    per = max(k - 1, 1)
    lvl1 = [np.sort(kv[c * p["chunk"]: (c + 1) * p["chunk"]])[::-1][:per] for c in range(p["chunks"])]
    return _pad(*_top(np.concatenate(lvl1), k), k)


def mutant_threshold_upper_edge(bits, k, case):       # the radix threshold taken at the upper edge of the k-th key's first-pass bin
    name, p = case_route(case)
    if name != "radix":
        return select(bits, k)
    kv = keys(bits)
    kth = np.sort(kv)[::-1][k - 1]
    keep = kv[(kv >> U64(kRadixPassShift[0])) > (kth >> U64(kRadixPassShift[0]))]
    return _pad(*_top(keep, k), k)


def mutant_merge_ties_by_list_index(words, R, k, k_out):
    """merge only: equal score words ordered by their index j inside their list, then by rank, instead of by position r * k + j"""
    pos = np.arange(R * k)
    alt = (pos % k) * R + pos // k
    kv = (orderable(words).astype(U64) << U64(32)) | (~alt.astype(U32)).astype(U64)
    order = np.argsort(kv)[::-1][:k_out]
    return words[order], pos[order]


MUTANTS = {f.__name__[7:]: f for f in (mutant_ties_position_descending, mutant_zeros_tied, mutant_nan_greatest, mutant_negatives_raw,
                                       mutant_tail_dropped, mutant_survivors_truncated, mutant_chunk_k_minus_1, mutant_threshold_upper_edge)}
MERGE_MUTANT = "merge_ties_by_list_index"
