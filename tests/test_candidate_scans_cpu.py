"""The bars of tests/test_candidate_scans_gpu.py are sharp: on the very inputs the GPU file uses, every bug class listed below, applied to
the restatement (tests/_scan_ref.py), is rejected by the exact comparison (dyadic inputs) and by the admissible-interval rule (random
unit-norm inputs); the exactness precondition of the dyadic inputs holds; and the interval rule is not slack (at most a quarter of the
entries have two admissible values).

Bug classes: bf16 truncation instead of round-to-nearest-even; the qsum rounding dropped; the inner bf16 rounding of the coarse table
dropped; sum where mean is asked and vice versa; item groups m and m + 1 swapped in the component rows; rows b * P_Q + i transposed to
i * B + b; the last partial tile's columns scored as the previous tile's; ties broken by position descending; query row 32 reading row
0's fragment.  The table builds are compared on unit-norm Gaussian components here (the GPU file reads its Ex back from the index
build); the tie rule is held against the inputs of the fused top-k tests, whose reference is the key selection.
"""
import numpy as np
import pytest
import torch

from tests import _scan_ref as S
from tests._mol_ref64 import C_DOT, U


def test_bf16_rounding_is_torchs_and_keeps_nan():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 1.005859375, -1.005859375, 3.3895314e38, 3.4e38, np.inf, -np.inf], dtype=np.float32)])
    assert np.array_equal(S.bf16_rn(x).view(np.uint32), torch.from_numpy(x).bfloat16().float().numpy().view(np.uint32))
    assert np.array_equal(S.bf16_from_f64(x.astype(np.float64))[:-4].view(np.uint32), S.bf16_rn(x)[:-4].view(np.uint32))
    nan = np.array([0x7FC00001, 0xFFC12345, 0x7F800001], dtype=np.uint32)
    assert np.array_equal(S.bf16_rn(nan.view(np.float32)).view(np.uint32), nan)
    # one rounding, not two: 1 + 2^-8 + 2^-30 lies above the tie and rounds up; through fp32 (1 + 2^-8, a tie) it would round down to even
    assert float(S.bf16_from_f64(np.array([1 + 2.0 ** -8 + 2.0 ** -30]))[0]) == 1.0078125
    assert S.is_bf16(S.bf16_rn(x)).all() and not S.is_bf16(np.array([1.001], dtype=np.float32)).any()


def test_key_selection_is_score_descending_then_position_ascending():
    sc = np.array([[1.0, -0.0, 0.0, 1.0, -np.inf, np.inf, 0.5, 1.0]], dtype=np.float32)
    s, p = S.topk_keys(sc, 6)
    assert p.tolist() == [[5, 0, 3, 7, 6, 2]] and s.tolist() == [[np.inf, 1.0, 1.0, 1.0, 0.5, 0.0]]
    assert S.topk_keys(sc, 6, "ties_desc")[1].tolist() == [[5, 7, 3, 0, 6, 2]]
    rng = np.random.default_rng(1)
    sc = S.bf16_rn(rng.standard_normal((7, 300)).astype(np.float32))       # bf16 values: ties
    s, p = S.topk_keys(sc, 300)
    order = np.lexsort((np.arange(300)[None, :].repeat(7, 0), -sc.astype(np.float64)), axis=1)
    assert np.array_equal(p, order) and np.array_equal(s, np.take_along_axis(sc, order, 1))
    assert np.array_equal(S.unorderable(S.orderable(sc)).view(np.uint32), sc.view(np.uint32))


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_dyadic_cases_are_exact_and_reject_every_bug_class(shape):
    """For every dyadic case of the GPU file: the precondition (int64), and every applicable bug class changes a compared score."""
    cases = [c for c in S.SCORE_CASES if c.shape == shape]
    assert cases
    hit = set()
    for case in cases:
        eq, table = S.dyadic_inputs(case)
        S.check_exact(case, eq, table)
        for avg in S.modes(case):
            s, a = S.model(case, eq, table, avg, want_abs=True)
            ref = S.rounded(s)
            assert np.isfinite(ref).all() and float(a.max()) < 2.0 ** 11
            # exact sums: every S is a multiple of the product grid and needs at most 24 bits above it
            assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
            for mut in S.MUTATIONS:
                if S.applicable(case, mut):
                    assert not np.array_equal(S.rounded(S.model(case, eq, table, avg, mut)[0], mut), ref), (case, avg, mut)
                    hit.add(mut)
    want = set(S.MUTATIONS)
    assert hit == want, want - hit


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_table_bug_classes_change_the_tables(shape):
    _, pq, px, d = S.SHAPES[shape]
    for n in (1, 33, 4001):
        ex = S.unit_rows(np.random.default_rng([5, n, d, px]), n, px, d)
        ct, kt = S.coarse_table(ex), S.component_table(ex)
        assert S.is_bf16(ct).all() and S.is_bf16(kt).all() and kt.shape == (px, n, d)
        assert np.array_equal(kt[1], S.bf16_rn(ex[:, 1, :]))
        # The inner rounding: P_X is a power of two in all four shapes, the division is then exact and commutes with the rounding, so
        # bf16(bf16(acc) / P_X) == bf16(acc / P_X) -- dropping it is no bug there and no comparison can (or need) see it.  It applies to
        # no case of the GPU file; with three item groups it would show at once.
        assert np.array_equal(S.coarse_table(ex, "table_no_inner"), ct)
        ex3 = ex[:, :3, :]
        if n > 1:      # (the d values of a single item can all survive by chance)
            assert not np.array_equal(S.coarse_table(ex3, "table_no_inner"), S.coarse_table(ex3))
        assert not np.array_equal(S.coarse_table(ex, "trunc"), ct)
        assert not np.array_equal(S.component_table(ex, "trunc"), kt)


@pytest.mark.parametrize("case", S.RANDOM_CASES, ids=lambda c: f"{c.entry}-{c.shape}")
def test_interval_rule_rejects_every_bug_class_and_is_not_slack(case):
    """The random cases of the GPU file: bf16(S) itself passes; each applicable bug class puts an entry outside its interval; and the
    share of entries with two admissible values is at most a quarter (printed)."""
    eq, table = S.random_inputs(case)
    d = case.dims[2]
    muts = [m for m in S.MUTATIONS if S.applicable(case, m)]
    assert "ragged_prev" not in muts      # (4 000 items are whole tiles: the columns can be taken in blocks)
    caught = dict.fromkeys(muts, 0)
    ambiguous = total = 0
    for c0 in range(0, case.N, 1000):
        t = table[..., c0:c0 + 1000, :]
        for avg in S.modes(case):
            s, a = S.model(case, eq, t, avg, want_abs=True)
            lo, hi = S.admissible(s, a, d)
            assert S.passes(S.rounded(s), lo, hi).all()
            # equal or adjacent bf16 numbers wherever the bound is below half a bf16 step of S (all but the sums that cancel to ~0, whose
            # interval straddles zero; those count as ambiguous below)
            wide = C_DOT * U * (d + 2) * a > 2.0 ** -9 * np.abs(s)
            step = np.abs(hi.astype(np.float64) - lo) / np.maximum(np.abs(hi), np.abs(lo)).clip(1e-30)
            assert float(step[~wide].max()) <= 2.0 ** -7
            ambiguous += int((lo != hi).sum())
            total += lo.size
            for mut in muts:
                caught[mut] += int((~S.passes(S.rounded(S.model(case, eq, t, avg, mut)[0], mut), lo, hi)).sum())
    share = ambiguous / total
    print(f"{case.entry} {case.shape}: share of entries with two admissible values {share:.4f}; rejected entries per bug class {caught}")
    assert share <= 0.25, share
    assert all(v > 0 for v in caught.values()), caught


def test_select_cases_are_exact_and_the_tie_rule_decides():
    """The dyadic inputs of the fused top-k tests: exact (asserted by select_inputs), and on the kinds built for it ("dups", "few") the
    reversed tie rule returns other positions; "dups" ties straddle the k-th place of a planted row."""
    seen = set()
    for case in S.select_cases():
        if case.N > 4000 and (case.entry, case.kind) in seen:      # the large sizes once per entry and kind here
            continue
        seen.add((case.entry, case.kind))
        eq, table, n = S.select_inputs(case)
        few_rows = case._replace(B=min(case.B, 2))
        sc = S.select_scores(few_rows, eq[:few_rows.B], table)[:4]
        rs, rp = S.topk_keys(sc, case.k)
        assert (np.diff(rs.astype(np.float64), axis=1) <= 0).all()
        if case.kind in ("dups", "few"):
            assert not np.array_equal(S.topk_keys(sc, case.k, "ties_desc")[1], rp), case
        if case.kind == "dups":
            kth = rs[:, -1:]
            assert ((sc == kth).sum(1) > (rs == kth).sum(1)).any(), case      # more items at the k-th score than places for them
        if case.kind in ("front", "last_class"):
            win = np.arange(case.k) if case.kind == "front" else S.winners_last_class(n, case.k)
            assert all(set(r.tolist()) == set(win.tolist()) for r in rp), case
