"""CPU: the bar of tests/test_verdict_gpu.py can fail.  The clause tables that file runs through rails_rescore_verdict,
rails_candidates_finish and rails_merge_candidates_verdict are evaluated here with the host restatement of the contract
(tests/_verdict_ref.py) and with each of nine bug classes applied to that restatement, one at a time: every bug must move the state after
some call of some table row, or the table is missing a row.  The composition families of the whole-proof test are checked the same way:
the restatement proves every row of the benign families (so 'every proved row equals the dense top-k' leaves no row out on the device),
and on the planted family the merged top-k is NOT the dense one (so a verdict that proved it would be caught)."""
import numpy as np
import pytest

from tests import _verdict_ref as V


@pytest.fixture(scope="module")
def tables():
    cases = V.all_cases()
    return cases, [V.outcome(c) for c in cases]


def test_the_tables_state_their_clauses(tables):
    """the REDO word each row was written for is what the restatement gives: a row that stops failing (or passing) for its stated reason shows here"""
    cases, want = tables
    assert len({c.name for c in cases}) == len(cases)
    for case, states in zip(cases, want):
        assert [s[1] for s in states] == case.redo, case.name
        assert [np.array(s[5], dtype=np.uint32).view(np.float32) for s in states] == [float(i + 1) for i in range(len(states))], case.name


@pytest.mark.parametrize("bug", V.BUGS)
def test_every_bug_class_moves_a_table_row(tables, bug):
    cases, want = tables
    kinds = V.BUG_KINDS.get(bug, ("call", "finish", "merge"))
    got = [(c, w, V.outcome(c, bug)) for c, w in zip(cases, want) if c.kind in kinds]
    moved = [c.name for c, w, g in got if g != w]
    assert moved, f"no table row distinguishes {bug}"
    # ... and through the REDO word itself, not only the calibration state: the flag is what the caller acts on
    flagged = [c.name for c, w, g in got if [s[1] for s in g] != [s[1] for s in w]]
    assert flagged, f"{bug} changes no REDO word"


def test_row_verdict_edges():
    """strict inequality, NaN gap, the row's own error, a bad row's error left out"""
    assert V.row_verdict(2.0, 1.0, 0.0, False, 0.0, 1.0, 1.0) == (True, 1.0)
    assert V.row_verdict(2.0, 1.0, 0.0, False, 0.0, float(V.ONE_ULP_DOWN(1.0)), 1.0) == (False, 1.0)
    fail, gap = V.row_verdict(-np.inf, -np.inf, 0.0, False, 0.0, 0.0, 1.0)
    assert fail and np.isnan(gap)
    assert V.row_verdict(2.0, 1.0, 0.5, False, 0.25, 0.0, 1.0)[0] is False and V.row_verdict(2.0, 1.0, 0.5, False, 0.25, 0.0, 2.0)[0] is True
    assert V.row_verdict(2.0, 1.0, 0.25, False, 0.5, 0.0, 2.0)[0] is True
    assert V.row_verdict(2.0, -np.inf, 0.0, False, 0.0, 1e30, 1.0) == (False, np.inf)
    assert V.row_verdict(2.0, -np.inf, np.inf, True, 0.0, 0.0, 1.0)[0] is True


def test_fold_keeps_the_calibration_through_a_bad_call():
    st = V.new_state()
    st = V.fold([(False, 1.0, 0.25, False), (False, 2.0, 0.125, False)], st, 0.0, 2.0, 0.5)
    assert list(st[[0, 2, 3, 4, 5, 6, 7]]) == [0.25, 0.5, 0.25, 1.0, 1.0, 0.0, 0.5] and V.redo_of(st) == 0
    st = V.fold([(True, np.float32(np.nan), np.inf, True), (False, 2.0, 0.75, False)], st, 0.0, 2.0, np.inf)
    assert list(st[[0, 2, 3, 4, 5, 6, 7]]) == [0.25, 0.5, np.inf, -np.inf, 2.0, 1.0, np.inf] and V.redo_of(st) == 1
    st = V.fold([(False, 1.0, 0.125, False)], st, 0.0, 2.0, 0.0)
    assert list(st[[0, 2, 3, 4, 5, 6, 7]]) == [0.25, 0.5, 0.125, 1.0, 3.0, 1.0, np.inf] and V.redo_of(st) == 0


@pytest.fixture(scope="module", params=V.FAMILIES, ids=lambda f: f.name)
def family(request):
    f = request.param
    s32, approx = V.family_scores(f)
    return f, s32, approx


def _prove(f, s32, approx, default_eps=V.FAMILY_EPS):
    msgs = V.shard_messages(approx, s32, f.R, f.cap, f.k, V.FAMILY_LO, V.FAMILY_HI)
    return (msgs,) + V.merge_call(msgs, f.R, f.k, f.k, V.new_state(), default_eps, 1.0)


def test_the_benign_families_are_proved_on_every_row(family):
    f, s32, approx = family
    msgs, mg, fails, state = _prove(f, s32, approx)
    counts = [int(c) for c in V.is_candidate(f, approx).reshape(f.B, f.R, f.per_shard).sum(2).reshape(-1)]
    gap = float(state[4])
    print(f"{f.name}: smallest gap {gap:.3f}, candidate counts {min(counts)}-{max(counts)}, largest error {float(state[0]):.3e}")
    assert not any(fails) and V.redo_of(state) == 0
    assert f.k <= min(counts) and max(counts) <= f.cap
    assert float(state[0]) <= 1.001 * V.FAMILY_EPS and gap > 1.0          # three orders of magnitude over eps: no borderline row
    want_s, want_i = V.full_topk(s32, f.k)
    assert np.array_equal(mg.scores.view(np.uint32), want_s.view(np.uint32)) and np.array_equal(mg.ids, want_i)


def test_the_planted_winner_is_missed_by_the_merge_and_caught_by_the_verdict(family):
    f, s32, approx = family
    row = f.B - 1
    planted, x, eps = V.plant_hidden_winner(f, s32, approx, row)
    assert not V.is_candidate(f, approx)[row, x] and abs(float(planted[row, x]) - float(approx[row, x])) <= eps
    msgs, mg, fails, state = _prove(f, planted, approx, default_eps=eps)
    want_s, want_i = V.full_topk(planted, f.k)
    assert x in want_i[row] and x not in mg.ids[row]                        # the merged top-k of that row is wrong ...
    assert fails[row] and V.redo_of(state) == 1                             # ... and the verdict says so
    assert V.merge_call(msgs, f.R, f.k, f.k, V.new_state(), eps, 1.0, bug="ge_for_gt")[1][row] or float(state[4]) == np.float32(eps)
    # the bound the caller declared is what catches it: at the benign eps the same messages would be 'proved'
    assert not V.merge_call(msgs, f.R, f.k, f.k, V.new_state(), V.FAMILY_EPS, 1.0)[1][row]


def test_the_crowded_row_has_fewer_than_k_candidates_on_every_shard():
    f = V.FAMILIES[0]
    s32, approx = V.family_scores(f)
    row = 2
    s32, approx = V.crowd(f, s32, approx, row)
    counts = V.is_candidate(f, approx).reshape(f.B, f.R, f.per_shard).sum(2)
    assert (counts[row] < f.k).all() and (np.delete(counts, row, 0) >= f.k).all()
    msgs, mg, fails, state = _prove(f, s32, approx)
    assert fails == [b == row for b in range(f.B)] and V.redo_of(state) == 1 and float(state[4]) == -np.inf
