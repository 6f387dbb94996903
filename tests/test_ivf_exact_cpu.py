"""The bar of tests/test_ivf_exact_gpu.py is sharp, shown on the very inputs the GPU file uses: the dyadic grid makes the fp32 fmaf chain
and the sample sums exact (so the restatement tests/_ivf_exact_ref.py alone decides every output: no band, nothing left out), and every
bug class below, applied to the restatement, changes a compared output.

Bug classes: ties to the higher list in assign and in the coarse pick; position descending among tied scores; an unstable scatter (two
equal-list items of one tile swapped); a dropped last entry of a segment; a segment bound taken from max_list instead of the list's size;
the rank-64 slot of the two-slot top-k not fed from rank 63; no continuation past nprobe; a continuation that counts list sizes where the
filter should count eligible entries; NaN left as NaN; the split taking the last of the tied largest lists; sizes not halved after a
split; the parity of the +-1/1024 swapped; the mean divided before summing.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

from tests import _ivf_exact_ref as R

F32 = np.float32


# ---- the arithmetic of the restatement -----------------------------------------------------------------------------------------------
def round_f32(v: Fraction) -> np.float32:
    """the fp32 number nearest to an exact rational, ties to even"""
    r = F32(float(v))
    cands = {float(r), float(np.nextafter(r, F32(np.inf))), float(np.nextafter(r, F32(-np.inf)))}
    best = min(abs(Fraction(c) - v) for c in cands)
    near = [c for c in cands if abs(Fraction(c) - v) == best]
    if len(near) == 2:
        near = [c for c in near if (np.array(c, F32).view(np.uint32) & 1) == 0]
    return F32(near[0])


def test_fma32_is_correctly_rounded():
    # exact sum 2^30 + 2^7 + 64 - 2^-40: float64 rounds it onto the fp32 midpoint, whose even neighbour is the WRONG one
    x, y, z = F32(64.0) * (F32(1) + F32(2.0 ** -23)), F32(1) - F32(2.0 ** -23), F32(2.0 ** 30 + 2.0 ** 7)
    assert F32(np.float64(x) * np.float64(y) + np.float64(z)) != z                 # product-plus-sum in float64 rounds twice
    assert R.fma32(x, y, z) == z == round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
    rng = np.random.default_rng(0)
    n = 3000
    xs = (rng.integers(-128, 129, n) / 64.0).astype(F32)                           # grid points times unit-range fp32 numbers
    ys = rng.standard_normal(n).astype(F32)
    zs = (rng.standard_normal(n) * 2.0 ** rng.integers(-3, 4, n)).astype(F32)
    zs[::3] = (-(xs[::3].astype(np.float64) * ys[::3]) * (1 + 2.0 ** -20)).astype(F32)      # cancellation
    got = R.fma32(xs, ys, zs)
    ref = np.array([round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))) for a, b, c in zip(xs, ys, zs)], F32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_chain_equals_exact_rational_chain_off_the_grid():
    rng = np.random.default_rng(1)
    x = R.dyadic(rng, (5, 32))
    c = R.normalise(rng.standard_normal((4, 32)).astype(F32))
    got = R.chain_scores(x, c)
    for p in range(5):
        for l in range(4):
            acc = F32(0)
            for j in range(32):
                acc = round_f32(Fraction(float(x[p, j])) * Fraction(float(c[l, j])) + Fraction(float(acc)))
            assert got[p, l] == acc


def exact_on_grid(x, c, chain=True):
    """x (points, d), c (lists, d): both on the grid and sum |terms| < 2^24 * 2^-12, so every partial sum, in any order, is an fp32 number;
    and on a corner of the case the sequential fmaf chain IS the float64 dot product"""
    fx, fc = np.isfinite(x).all(axis=-1), np.isfinite(c).all(axis=-1)
    x, c = np.asarray(x, F32)[fx], np.asarray(c, F32)[fc]
    assert R.on_grid(x) and R.on_grid(c) and x.shape[1] <= 128
    assert (np.abs(x.astype(np.float64)) @ np.abs(c.astype(np.float64)).T).max() * 4096 < 2 ** 24
    if chain:
        assert np.array_equal(R.chain_scores(x[:48], c[:48]).astype(np.float64), R.dot64(x[:48], c[:48]))


@pytest.mark.parametrize("case", R.BUILD_CASES, ids=lambda c: f"{c.shape}-n{c.n}-nlist{c.nlist}")
def test_build_cases_are_exact_and_decided_by_the_rules(case):
    x16, cent = R.build_inputs(case)
    d = x16.shape[2]
    chunk = 8192 // d                                   # centroids per LDS chunk of the assignment kernel
    changed_assign = changed_order = cross = False
    for m in range(x16.shape[0]):
        exact_on_grid(x16[m].astype(F32), cent[m], chain=m == 0)
        a, off, pos, vec = R.build_lists(x16[m], cent[m])
        assert (pos[1:] > pos[:-1])[np.repeat(np.arange(case.nlist), np.diff(off))[1:] == np.repeat(np.arange(case.nlist), np.diff(off))[:-1]].all()
        changed_assign |= not np.array_equal(a, R.assign(x16[m].astype(F32), cent[m], bug="assign_high"))
        changed_order |= not np.array_equal(pos, R.build_lists(x16[m], cent[m], bug="unstable")[2])
        for lo, hi in R.build_copies(case):
            if lo < hi:
                assert off[hi + 1] == off[hi]           # the copy never wins
                cross |= lo // chunk != hi // chunk and off[lo + 1] > off[lo]
    assert changed_assign == (case.nlist > 1)
    assert changed_order                                # some list holds two items of one tile
    if case.nlist > chunk:
        assert cross                                    # a tie between centroids of different chunks decided some point


def test_build_cases_cover_what_they_name():
    by = {(c.shape, c.n, c.nlist) for c in R.BUILD_CASES}
    assert {c.n for c in R.BUILD_CASES} >= {255, 256, 257, 4096, 4097, 8193}
    assert {("8x8x32", 257), ("8x8x32", 300), ("8x4x64", 129), ("8x4x128", 65), ("8x4x128", 70)} <= {(s, l) for s, _, l in by}
    assert any(l * -(-n // R.SORT_TILE) > 1024 for _, n, l in by) and any(l == 1 for _, _, l in by) and any(l == n for _, n, l in by)
    assert any(l == R.MAX_NLIST for _, _, l in by)


# ---- training -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LLOYD_CASES, ids=lambda c: f"{c.shape}-{c.kind}")
def test_lloyd_cases_are_exact_and_decided_by_the_rules(case):
    table, sample, start, sizes = R.lloyd_inputs(case)
    assert len(sample) <= 2048 and R.LLOYD_NLIST <= 64
    hit = {b: False for b in ("split_last_tied", "no_halve", "parity", "mean_div_first")}
    for m in range(table.shape[0]):
        xs = table[m][sample].astype(F32)
        exact_on_grid(xs, start[m])
        ref, first = R.lloyd_step(xs, start[m], want_sizes=True)
        assert np.array_equal(first, sizes)                                      # the sizes the case is about
        a = R.assign(xs, start[m])
        for l in range(R.LLOYD_NLIST):                                           # sums in sample order are exact: 19 bits
            members = xs[a == l].astype(np.float64)
            assert np.abs(members).sum(axis=0).max(initial=0) * 64 < 2 ** 24
            assert np.array_equal(np.cumsum(members.astype(F32), axis=0, dtype=F32).astype(np.float64), np.cumsum(members, axis=0))
        assert np.array_equal(ref, R.lloyd_step(xs, start[m], exact_chain=True))  # the fmaf chain agrees with float64 on the grid
        norms = np.linalg.norm(ref.astype(np.float64), axis=1)
        assert np.abs(norms - 1).max() < 1e-6
        for b in hit:
            hit[b] |= not np.array_equal(ref, R.lloyd_step(xs, start[m], bug=b))
    empties = int((sizes == 0).sum())
    assert hit["mean_div_first"]
    assert hit["parity"] == (empties > 0)
    assert hit["no_halve"] == (empties > 1)
    assert hit["split_last_tied"] or case.kind not in ("tied", "resplit")


def test_resplit_case_needs_the_float_halving():
    """41 -> 20.5 | 20.5: the new list 2 ties with 4 and, the lower id, is split next; with integer halves (20 | 21) list 4 would be"""
    sizes = R.lloyd_sizes("resplit", np.random.default_rng(0)).astype(F32)
    assert sizes.max() == 41 and sizes[4] == 41 and sorted(sizes)[-2] < 20
    sz = sizes.copy()
    sz[2] = sz[4] / F32(2)
    sz[4] -= sz[2]
    assert sz[2] == sz[4] == 20.5 and int(np.nonzero(sz == sz.max())[0][0]) == 2


def test_training_leaves_the_grid_and_stays_finite():
    table, sample = R.train_inputs()
    assert len(sample) == 512 and R.TRAIN_NLIST == 16
    for m in range(table.shape[0]):
        xs = table[m][sample].astype(F32)
        exact_on_grid(xs, xs[: R.TRAIN_NLIST])
        c1 = R.train(xs, R.TRAIN_NLIST, 1)
        assert np.array_equal(c1, R.lloyd_step(xs, xs[: R.TRAIN_NLIST]))         # the first step is on the grid
        assert not R.on_grid(c1) and np.isfinite(R.train(xs, R.TRAIN_NLIST, 3)).all()


# ---- the list edit -----------------------------------------------------------------------------------------------------------------
def test_edit_cases_hold_every_position_once():
    x16, cent = R.edit_base()
    assert x16.shape[1] == 4097 and cent.shape[1] == 37
    exact_on_grid(x16[0].astype(F32), cent[0])
    kinds = set()
    for case in R.EDIT_CASES:
        pos, n_keep, n_new, rows = R.edit_inputs(case)
        lim = min(R.EDIT_N, n_keep)
        assert len(set(pos.tolist())) == case.m and R.on_grid(rows)
        assert n_new == lim - int((pos < lim).sum()) + case.m                       # the header's formula
        assert set(range(lim)) | set(pos.tolist()) == set(range(n_new))
        kinds.add((case.kind, case.m, case.in_place))
        if case.m:
            assert int((pos < lim).sum()) == (0 if case.kind == "insert" else case.m - case.m // 3)
    assert {("both", 0, 1), ("both", 1, 0), ("both", 300, 1), ("insert", 40, 0), ("insert", 40, 1)} <= kinds


def test_pack_index_is_the_fragment_order():
    rng = np.random.default_rng(3)
    ex = rng.standard_normal((70, 4, 64)).astype(F32)
    buf = R.pack_index(ex, 8)
    tile = 32 * (4 * 64 + 8 * 4)
    assert buf.size == 3 * tile
    for item, m, dd in ((0, 0, 0), (33, 2, 31), (69, 3, 32), (31, 1, 63)):         # mol_layout.h ex_offset
        hi, s = dd // 32, dd % 32
        assert buf[(item >> 5) * tile + ((m * 8 + (s >> 2)) * 64 + hi * 32 + (item & 31)) * 4 + (s & 3)] == ex[item, m, dd]


# ---- the search ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_search(case, bug="", **kw):
    ix, eq = R.search_index(case.shape, case.kind), R.search_queries(case.shape, case.kind, case.B)
    mp, ml = R.plan(ix.off, case.nprobe, case.k)
    return R.search(ix, eq, case.nprobe, case.k, mp - case.below_plan, bug=bug, max_list=ml, **kw)


def test_search_inputs_are_exact():
    for shape, kind, B in sorted({(c.shape, c.kind, c.B) for c in R.SEARCH_CASES}):
        ix, eq = R.search_index(shape, kind), R.search_queries(shape, kind, B)
        q = eq.reshape(-1, eq.shape[2])
        for m in range(ix.cent.shape[0]):
            exact_on_grid(q, ix.cent[m], chain=m == 0)
            exact_on_grid(q, ix.vec[m].astype(F32), chain=m == 0)
            lid = ix.list_of_slot(m)
            assert (ix.pos[m][1:] > ix.pos[m][:-1])[lid[1:] == lid[:-1]].all() and sorted(ix.pos[m]) == list(range(ix.pos.shape[1]))
        if kind == "poison":
            assert np.isnan(eq).sum() == 1 and np.isnan(ix.vec.astype(F32)).sum() == ix.vec.shape[0] == np.isposinf(ix.vec.astype(F32)).sum()


def test_search_cases_cover_what_they_name():
    cases = R.SEARCH_CASES
    assert {c.k for c in cases} >= {1, 5, 63, 64, 65, 127, 128} and set(R.EDGE_SIZES) == {0, 1, 63, 64, 65, 127, 128, 129, 300}
    edges = [c for c in cases if c.kind == "edges"]
    assert {(c.k, c.nprobe) for c in edges} == {(k, p) for k in (1, 5, 63, 64, 65, 127, 128) for p in (1, 3, 12)}
    assert {c.shape for c in edges} == set(R.SHAPES) and len(R.INDEX_SIZES["edges"]) == 12
    for c in edges:                                   # 64-entry segments: a merge sees full, partial and missing segments
        PQ, G, _ = R.geometry(c.shape)
        assert R.scan_geometry(c.B, PQ, G, 12, c.nprobe, 300) == (64, 5)
    assert any(c.nprobe == 64 and len(R.INDEX_SIZES[c.kind]) == 64 for c in cases)
    assert any(c.B * R.geometry(c.shape)[0] > R.SLICE_ROWS and R.geometry(c.shape)[0] == pq for c in cases for pq in (8,))
    assert any(c.B * 16 > R.SLICE_ROWS and c.shape == "16x16x64" for c in cases)
    assert any(c.B == 1 for c in cases)


def test_search_cases_behave_as_they_are_meant_to():
    for case in R.SEARCH_CASES:
        ref, unfilled, probes, nprob = ref_search(case)
        assert unfilled == (1 if case.below_plan else 0)                          # one below the plan: the worst-case row runs short
        if case.below_plan:
            assert (ref.reshape(-1, case.k)[:, -1] == 0).any()
        else:
            rows = np.sort(ref.reshape(-1, case.k), axis=1)
            assert (rows[:, 1:] != rows[:, :-1]).all()                            # k distinct positions, NaN and inf rows included
        if case.kind == "short":
            assert nprob.max() == R.plan(R.search_index(case.shape, case.kind).off, case.nprobe, case.k)[0] - case.below_plan > case.nprobe
        # more than four rows probe one list: the scan's four waves loop over its match list
        assert max(np.bincount(probes[:, :, m][probes[:, :, m] >= 0]).max() for m in range(probes.shape[2])) > 4


EXPECT = {
    "coarse_high": lambda ch: {"edges", "small", "short"} <= {c.kind for c in ch},
    # ties decide rows at every k of every index
    "pos_desc": lambda ch: {(c.kind, c.k) for c in ch} == {(c.kind, c.k) for c in R.SEARCH_CASES},
    "seg_drop_last": lambda ch: {c.k for c in ch if c.kind == "edges"} == {1, 5, 63, 64, 65, 127, 128},
    "seg_from_max_list": lambda ch: len(ch) >= 10,
    "no_continue": lambda ch: {c for c in R.SEARCH_CASES if c.kind == "short" and not c.below_plan} <= set(ch) and "edges" in {c.kind for c in ch},
    "nan_kept": lambda ch: {c for c in R.SEARCH_CASES if c.kind == "poison"} == set(ch),
}


@pytest.mark.parametrize("bug", list(EXPECT))
def test_every_search_rule_decides_some_output(bug):
    cases = [c for c in R.SEARCH_CASES if not (bug == "nan_kept" and c.kind != "poison") and not (bug == "seg_from_max_list" and c.kind != "edges")]
    changed = [c for c in cases if not np.array_equal(ref_search(c)[0], ref_search(c, bug)[0])]
    assert EXPECT[bug](changed), (bug, changed)


def test_arrival_orders_and_the_rank_64_hand_over():
    """The kernel's own flow (a running top-k per 64-entry segment, then the merge, lane by lane) on the arrival-order rows of the `edges`
    index: it is the restatement's row; without the rank 63 -> 64 hand-over it is not."""
    shape = "8x8x32"
    ix, eq = R.search_index(shape, "edges"), R.search_queries(shape, "edges", 2)
    s = R.dot64(eq[0, 0][None], ix.vec[0])[0]
    for l, sign in ((9, 1), (10, -1), (11, 0)):       # ascending with the slot, descending, all equal
        seg = s[ix.off[0, l] : ix.off[0, l + 1]]
        assert (np.sign(np.diff(seg)) == sign).all()
    for k, hit in ((128, all), (127, all), (65, any), (64, lambda d: not any(d))):
        mp, _ = R.plan(ix.off, 12, k)
        ref, _, probes, nprob = R.search(ix, eq, 12, k, mp)
        ref = ref.reshape(2, 8, 8, k)
        differs = []
        for i in (0, 1, 2):                           # ascending arrival, descending arrival, a random row
            lists = probes[0, i, 0, : nprob[0, i, 0]].tolist()
            assert R.wave_search_row(ix, eq[0, i], 0, lists, k, 64) == ref[0, i, 0].tolist()
            differs.append(R.wave_search_row(ix, eq[0, i], 0, lists, k, 64, bug="rank64") != ref[0, i, 0].tolist())
        assert hit(differs), (k, differs)


# ---- the filtered search ---------------------------------------------------------------------------------------------------------
def test_filter_cases_are_decided_by_the_eligible_counts():
    differs_from_sizes, per_row, shared = [], 0, 0
    for case in R.FILTER_CASES:
        ix, eq = R.search_index(case.shape, "edges"), R.search_queries(case.shape, "edges", case.B)
        n = ix.pos.shape[1]
        eff, visible = R.filter_words(case.shape)
        assert n % 32 != 0 and len(visible) == (n + 31) // 32
        allowed = R.filter_allowed(case)
        words = R.list_words(ix.pos, n, eff=eff)
        counts = R.list_counts(ix, words, allowed)
        assert (counts[:, :, 3] == 0).all() and (R.list_counts(ix, words, np.array([0xFFFFFFFF], np.uint32))[:, :, 3] == 64).all()    # a list with no eligible entry
        for m in range(ix.pos.shape[0]):             # ... and a segment with none inside an eligible list
            lo = ix.off[m, 8]
            assert ((words[m, lo + 64 : lo + 128][None] & allowed[:, None]) == 0).all() and (counts[:, m, 8] > 0).all()
        mp = R.plan_filtered(counts if case.per_row else counts[:1], case.nprobe, case.k)
        ref, unfilled, probes, nprob = R.search(ix, eq, case.nprobe, case.k, mp, words=words, allowed=allowed)
        for b in range(case.B):                      # only eligible items come back
            mine = ref.reshape(case.B, -1)[b]
            assert unfilled or ((eff[mine] & allowed[b]) != 0).all()
        plain = R.search(ix, eq, case.nprobe, case.k, R.plan(ix.off, case.nprobe, case.k)[0])
        assert not np.array_equal(ref, plain[0]) and (case.nprobe == 12 or not np.array_equal(nprob, plain[3]))
        if not np.array_equal(ref, R.search(ix, eq, case.nprobe, case.k, mp, words=words, allowed=allowed, bug="filter_counts_sizes")[0]):
            differs_from_sizes.append(case)
        per_row += case.per_row
        shared += not case.per_row
    assert per_row and shared and len(differs_from_sizes) >= 4
    assert any(len(set(R.filter_allowed(c).tolist())) > 1 for c in R.FILTER_CASES)


def test_plans_are_the_worst_probe_order():
    off = np.array([[0, 5, 5, 6, 30, 31], [0, 10, 20, 30, 31, 31]], np.int32)
    assert R.plan(off, 1, 7) == (4, 24) and R.plan(off, 1, 1) == (2, 24) and R.plan(off, 5, 1) == (5, 24) and R.plan(off, 1, 40) == (5, 24)
    counts = np.diff(off.astype(np.int64), axis=1).astype(np.int32)[None]
    assert R.plan_filtered(counts, 1, 7) == 4 and R.plan_filtered(counts[:, :1], 1, 7) == 4 and R.plan_filtered(counts[:, 1:], 1, 7) == 3
