"""Host restatement of the verdict contract of the proved exact top-k (include/rails_amd.h: rails_rescore_verdict, rails_margin_stats,
rails_candidates_finish, rails_merge_candidates_verdict), the clause tables that tests/test_verdict_gpu.py runs through the kernels, and the
bug classes tests/test_verdict_cpu.py applies to this restatement to show that every one of them moves a table row.

Every float step is ONE IEEE fp32 operation on numpy float32 scalars (max / min are fmaxf / fminf: a NaN operand is dropped), so a state
computed here equals the device's bit for bit; states are 8 float32 whose word 1 is an int32."""
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from tests.test_candidates_gpu import _expected

F = np.float32
INF, NINF, NAN = F(np.inf), F(-np.inf), F(np.nan)


def ONE_ULP_UP(x) -> np.float32:
    return np.nextafter(F(x), INF, dtype=np.float32)


def ONE_ULP_DOWN(x) -> np.float32:
    return np.nextafter(F(x), NINF, dtype=np.float32)


# the bug classes of tests/test_verdict_cpu.py; bug=None everywhere is the contract
BUGS = ("ge_for_gt", "min_over_ranks", "err_inf_ignored", "seen_forgotten", "call_wide_error", "nan_gap_passes", "bad_call_raises_seen",
        "no_short_row_clause", "one_sided_as_two_sided")


# the entry points a bug class can show in (the others do not contain the clause)
BUG_KINDS = {"min_over_ranks": ("merge",), "err_inf_ignored": ("merge",), "call_wide_error": ("finish", "merge"), "no_short_row_clause": ("finish",),
             "one_sided_as_two_sided": ("finish",)}


def fmax(a, b) -> np.float32:
    return F(np.fmax(F(a), F(b)))


def fmin(a, b) -> np.float32:
    return F(np.fmin(F(a), F(b)))


def new_state() -> np.ndarray:
    return np.zeros(8, dtype=np.float32)


def state_words(state) -> List[int]:
    """the 8 words of a state (numpy or torch, any device) as integers: what 'bit for bit' compares"""
    if isinstance(state, torch.Tensor):
        state = state.detach().cpu().numpy()
    return [int(w) for w in np.ascontiguousarray(state, dtype=np.float32).view(np.uint32)]


def redo_of(state) -> int:
    return state_words(state)[1]


def _put_state(seen, redo, eps, err, gap, calls, redone, grd) -> np.ndarray:
    st = np.array([seen, 0.0, eps, err, gap, calls, redone, grd], dtype=np.float32)
    st.view(np.int32)[1] = int(redo)
    return st


# ---- one row, one call ---------------------------------------------------------------------------------------------------------------
def row_verdict(kth, m, err, bad, seen_before, default_eps, safety, bug: Optional[str] = None):
    """-> (fail, gap): the row is proved iff it is not bad and  kth - m > max(default_eps, safety * max(seen_before, this row's error))"""
    with np.errstate(all="ignore"):
        gap = F(F(kth) - F(m))
        if bug == "seen_forgotten":
            seen_before = F(0)
        eps = fmax(default_eps, F(F(safety) * fmax(seen_before, F(0) if bad else err)))
    if bug == "ge_for_gt":
        proved = bool(gap >= eps)
    elif bug == "nan_gap_passes":
        proved = not bool(gap <= eps)
    else:
        proved = bool(gap > eps)
    return bool(bad) or not proved, gap


def fold(rows, state, default_eps, safety, guard_max, bug: Optional[str] = None) -> np.ndarray:
    """rows: (fail, gap, err, bad) per row -> the call's new state, as the last workgroup of rails_candidates_finish /
    rails_merge_candidates_verdict leaves it"""
    with np.errstate(all="ignore"):
        e, g = F(0), INF
        any_bad = redo = False
        for fail, gap, err, bad in rows:
            e = fmax(e, F(0) if bad else err)
            g = fmin(g, NINF if np.isnan(gap) else gap)
            any_bad |= bool(bad)
            redo |= bool(fail)
        seen = F(0) if bug == "seen_forgotten" else F(state[0])
        if not any_bad or bug == "bad_call_raises_seen":
            seen = fmax(seen, e)
        return _put_state(seen, redo, fmax(default_eps, F(F(safety) * seen)), INF if any_bad else e, g, F(state[5]) + F(1),
                          F(state[6]) + F(1 if redo else 0), fmax(state[7], guard_max))


def _guard(values, limit):
    """-> (violated, largest magnitude with a NaN counted as inf)"""
    if values is None:
        return False, F(0)
    v = np.abs(np.asarray(values, dtype=np.float32).reshape(-1))
    if v.size == 0:
        return False, F(0)
    return bool((~(v <= F(limit))).any()), F(np.where(np.isnan(v), INF, v).max())


def call_verdict(row_stats, state, default_eps, safety, guard=None, guard_limit=0.0, bug: Optional[str] = None) -> np.ndarray:
    """rails_rescore_verdict: ONE eps for the call, from the largest error seen so far INCLUDING this call's; bad = a NaN stat, err = inf
    or the guard; the recorded margin is the smallest non-NaN one"""
    st = np.asarray(row_stats, dtype=np.float32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        err, gap = F(0), INF
        for e, g in st:
            err, gap = fmax(err, e), fmin(gap, g)
        violated, grd = _guard(guard, guard_limit)
        bad = bool(np.isnan(st).any()) or violated or not bool(err < INF)
        seen = F(0) if bug == "seen_forgotten" else F(state[0])
        if not bad or bug == "bad_call_raises_seen":
            seen = fmax(seen, err)
        eps = fmax(default_eps, F(F(safety) * seen))
        proved = bool(gap >= eps) if bug == "ge_for_gt" else bool(gap > eps)
        redo = bad or not proved
        return _put_state(seen, redo, eps, INF if bad else err, gap, F(state[5]) + F(1), F(state[6]) + F(1 if redo else 0), fmax(state[7], grd))


def margin_stats(kth_scores, col, m_max, err_max) -> np.ndarray:
    """rails_margin_stats: (rows, 2) [err_max[0], kth_scores[:, col] - m_max]"""
    kth = np.asarray(kth_scores, dtype=np.float32)[:, col]
    with np.errstate(all="ignore"):
        return np.stack([np.full_like(kth, F(np.asarray(err_max).reshape(-1)[0])), kth - np.asarray(m_max, dtype=np.float32)], 1)


# ---- the key order and the message words -----------------------------------------------------------------------------------------------
def _orderable(x: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 == 0, u | np.uint32(0x80000000), ~u)


def key_order(scores: np.ndarray, positions: np.ndarray) -> np.ndarray:
    """indices by (score descending in the kernels' bit-pattern order, position ascending)"""
    return np.lexsort((np.asarray(positions, dtype=np.int64), -_orderable(scores).astype(np.int64)))


def word(x) -> int:
    """a float as a message word: its fp32 bits in the low half of an int64"""
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def unword(w) -> np.ndarray:
    return (np.asarray(w, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


class FinishRow(NamedTuple):
    count: int
    positions: np.ndarray      # the candidates' local positions in key order
    scores: np.ndarray         # their exact scores, same order
    kth: np.float32
    m: np.float32
    err: np.float32
    bad: bool


_candidate_sets = {}


def _candidates(approx_t: torch.Tensor, lo, hi, cap) -> List[np.ndarray]:
    """the rows' candidate positions by the threshold bin rule (tests/test_candidates_gpu.py::_expected), kept per input: the tables reuse a
    few first-pass matrices over many cases"""
    key = (approx_t.numpy().tobytes(), tuple(approx_t.shape), float(lo), float(hi), int(cap))
    if key not in _candidate_sets:
        _candidate_sets[key] = [cand.numpy() for _, cand in _expected(approx_t, lo, hi, cap)]
    return _candidate_sets[key]


def finish_rows(approx, exact, cap, k, lo, hi, one_sided=False, bug: Optional[str] = None) -> List[FinishRow]:
    """Per row of approx / exact (B, n) -- first-pass and exact scores of every item --, what rails_candidates_select +
    rails_candidates_finish know about it: the candidates by the threshold bin rule, sorted by (exact desc, position asc), the k-th exact
    score (-inf below k candidates), m, the row's error and whether it is bad (a NaN)."""
    approx_t = torch.as_tensor(np.asarray(approx, dtype=np.float32))
    a_all, e_all = approx_t.numpy(), np.asarray(exact, dtype=np.float32)
    n = a_all.shape[1]
    out = []
    for r, pos in enumerate(_candidates(approx_t, lo, hi, cap)):
        c = int(pos.size)
        a, e = a_all[r, pos], e_all[r, pos]
        with np.errstate(all="ignore"):
            d = e - a
            dd = np.abs(d) if (not one_sided or bug == "one_sided_as_two_sided") else np.fmax(d, F(0))
            bad = bool(np.isnan(a_all[r]).any()) or bool((np.isnan(dd) | np.isnan(e) | np.isnan(a)).any())
            err = F(np.where(np.isnan(dd), INF, dd).max()) if c else F(0)
            m = NINF if c >= n else INF if c == 0 else F(np.fmin.reduce(a))
        order = key_order(e, pos)
        pos, e = pos[order], e[order]
        kth = e[k - 1] if c >= k else NINF
        if bug == "no_short_row_clause" and 0 < c < k:
            kth = e[c - 1]
        out.append(FinishRow(c, pos, e, F(kth), F(m), err, bad))
    return out


def finish_call(approx, exact, cap, k, lo, hi, state, default_eps, safety, one_sided=False, guard=None, guard_limit=0.0, bug: Optional[str] = None):
    """rails_candidates_finish with a state -> (rows, per-row fail, new state)"""
    rows = finish_rows(approx, exact, cap, k, lo, hi, one_sided, bug)
    return (rows,) + _call(
        [(r.kth, r.m, r.err, r.bad, r.count < k and bug != "no_short_row_clause") for r in rows], state, default_eps, safety, guard, guard_limit, bug)


def _call(rows, state, default_eps, safety, guard, guard_limit, bug):
    """rows: (kth, m, err, bad, short) -> (per-row fail, new state): row_verdict on every row with the state as the call found it, then fold"""
    folded, fails, grd_all = [], [], F(0)
    call_err = F(0)
    for _, _, err, bad, _ in rows:
        call_err = fmax(call_err, F(0) if bad else err)
    for i, (kth, m, err, bad, short) in enumerate(rows):
        violated, grd = _guard(None if guard is None else np.asarray(guard)[i], guard_limit)
        bad = bool(bad) or violated
        fail, gap = row_verdict(kth, m, call_err if bug == "call_wide_error" else err, bad, F(state[0]), default_eps, safety, bug)
        fail = fail or bool(short)
        folded.append((fail, gap, err, bad))
        fails.append(fail)
        grd_all = fmax(grd_all, grd)
    return fails, fold(folded, state, default_eps, safety, grd_all, bug)


def shard_message(approx_row, exact_row, first_position, ids, cap, k, lo, hi, one_sided=False) -> np.ndarray:
    """What one rank sends for one row (rails_candidates_finish's message form): [k score words | k ids | m | err] as int64.  ids: the
    shard's item ids by local position, or None for first_position + local position."""
    row = finish_rows(np.asarray(approx_row, dtype=np.float32)[None], np.asarray(exact_row, dtype=np.float32)[None], cap, k, lo, hi, one_sided)[0]
    return _message(row, first_position, ids, k)


def _message(row: FinishRow, first_position, ids, k) -> np.ndarray:
    msg = np.empty(2 * k + 2, dtype=np.int64)
    msg[:k], msg[k : 2 * k] = word(NINF), -1
    c = min(row.count, k)
    msg[:c] = row.scores[:c].view(np.uint32).astype(np.int64)
    msg[k : k + c] = (np.asarray(ids, dtype=np.int64)[row.positions[:c]] if ids is not None else first_position + row.positions[:c])
    msg[2 * k], msg[2 * k + 1] = word(row.m), word(INF if row.bad else row.err)
    return msg


def shard_messages(approx, exact, R, cap, k, lo, hi) -> np.ndarray:
    """(B, R * n) first-pass and exact scores, columns split into R contiguous shards, ids = global positions -> (R, B, 2k + 2) messages"""
    approx, exact = np.asarray(approx, dtype=np.float32), np.asarray(exact, dtype=np.float32)
    n = approx.shape[1] // R
    out = np.empty((R, approx.shape[0], 2 * k + 2), dtype=np.int64)
    for r in range(R):
        rows = finish_rows(approx[:, r * n : (r + 1) * n], exact[:, r * n : (r + 1) * n], cap, k, lo, hi)
        for b, row in enumerate(rows):
            out[r, b] = _message(row, r * n, None, k)
    return out


class Merged(NamedTuple):
    scores: np.ndarray         # (rows, k_out)
    ids: np.ndarray
    kth: np.ndarray            # (rows,)
    m: np.ndarray              # max over ranks, a NaN counted as +inf
    err: np.ndarray            # max over ranks, a NaN counted as +inf
    bad: np.ndarray            # some rank sent err = inf or a NaN


def merged(messages, R, k, k_out, bug: Optional[str] = None) -> Merged:
    """messages (R, rows, 2k + 2): candidate (r, j) has position r * k + j; the best k_out by (score desc, position asc), and what the
    verdict takes from the ranks"""
    messages = np.asarray(messages, dtype=np.int64).reshape(R, -1, 2 * k + 2)
    rows = messages.shape[1]
    sc = unword(messages[:, :, :k]).transpose(1, 0, 2).reshape(rows, R * k)
    ids = messages[:, :, k : 2 * k].transpose(1, 0, 2).reshape(rows, R * k)
    ms, errs = unword(messages[:, :, 2 * k]), unword(messages[:, :, 2 * k + 1])        # (R, rows)
    out_s, out_i = np.empty((rows, k_out), dtype=np.float32), np.empty((rows, k_out), dtype=np.int64)
    pos = np.arange(R * k)
    for b in range(rows):
        order = key_order(sc[b], pos)[:k_out]
        out_s[b], out_i[b] = sc[b, order], ids[b, order]
    with np.errstate(all="ignore"):
        m_in = np.where(np.isnan(ms), INF, ms)
        m = m_in.min(0) if bug == "min_over_ranks" else m_in.max(0)
        err = np.fmax(np.where(np.isnan(errs), INF, errs).max(0), F(0))
        bad = np.isnan(ms).any(0)
        if bug != "err_inf_ignored":
            bad = bad | (~(errs < INF)).any(0)
    return Merged(out_s, out_i, out_s[:, k_out - 1].copy(), m.astype(np.float32), err.astype(np.float32), bad)


def merge_call(messages, R, k, k_out, state, default_eps, safety, guard=None, guard_limit=0.0, bug: Optional[str] = None):
    """rails_merge_candidates_verdict -> (Merged, per-row fail, new state)"""
    mg = merged(messages, R, k, k_out, bug)
    return (mg,) + _call([(mg.kth[b], mg.m[b], mg.err[b], bool(mg.bad[b]), False) for b in range(mg.kth.size)], state, default_eps, safety, guard,
                         guard_limit, bug)


# ---- clause tables: sequences of calls on ONE state ------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    kind: str                  # "call" (rails_rescore_verdict), "finish" (rails_candidates_finish), "merge" (rails_merge_candidates_verdict)
    calls: list                # keyword dicts of call_verdict / finish_call / merge_call, without state and bug
    redo: Optional[list] = None   # what the clause is about, stated by hand: the REDO word after each call


def run_case(case: Case, bug: Optional[str] = None) -> List[np.ndarray]:
    """the state after each call of the case"""
    fn = {"call": call_verdict, "finish": finish_call, "merge": merge_call}[case.kind]
    state, out = new_state(), []
    for kw in case.calls:
        got = fn(state=state, bug=bug, **kw)
        state = got if case.kind == "call" else got[-1]
        out.append(state)
    return out


def outcome(case: Case, bug: Optional[str] = None):
    return [tuple(state_words(s)) for s in run_case(case, bug)]


# -- A: rails_rescore_verdict ---------------------------------------------------------------------------------------------------------
VERDICT_ROWS = (1, 7, 256, 257, 1000)


def _stats(rows, at, err, gap, err_rest=0.0, gap_rest=4.0) -> np.ndarray:
    st = np.empty((rows, 2), dtype=np.float32)
    st[:, 0], st[:, 1] = err_rest, gap_rest
    st[at] = (err, gap)
    return st


def deciding_rows(rows) -> List[int]:
    return sorted({rows - 1} | ({256} if rows > 256 else set()))


def call_cases() -> List[Case]:
    out = []
    for rows in VERDICT_ROWS:
        for at in deciding_rows(rows):
            for safety in (1.0, 8.0 / 3.0):
                kw = dict(default_eps=0.125, safety=safety, guard=None, guard_limit=0.0)
                tag = f"rows{rows}_at{at}_safety{safety:.2f}"
                # four calls: clean (error 0.25), a larger error (0.5), a NaN stat, clean again -- whose eps still reflects call 2; the
                # deciding row's margin 1.0 clears safety * 0.25 and not safety * 0.5 at safety 8/3, and clears both at safety 1
                out.append(Case("sequence_" + tag, "call", [
                    dict(row_stats=_stats(rows, at, 0.25, 1.0), **kw),
                    dict(row_stats=_stats(rows, at, 0.5, 1.0), **kw),
                    dict(row_stats=_stats(rows, at, NAN, 1.0, err_rest=0.75), **kw),
                    dict(row_stats=_stats(rows, at, 0.25, 1.0), **kw)],
                    redo=[0, 0, 1, 0] if safety == 1.0 else [0, 1, 1, 1]))
                eps = F(F(safety) * F(0.25))
                out.append(Case("margin_equals_eps_" + tag, "call", [dict(row_stats=_stats(rows, at, 0.25, eps), **kw)], redo=[1]))
                out.append(Case("margin_one_ulp_above_eps_" + tag, "call", [dict(row_stats=_stats(rows, at, 0.25, ONE_ULP_UP(eps)), **kw)], redo=[0]))
            kw = dict(default_eps=0.125, safety=1.0)
            clean = _stats(rows, at, 0.25, 1.0)
            g = np.full(rows * 3 + 1, 0.5, dtype=np.float32)
            g[0] = -0.75
            over, nan = g.copy(), g.copy()
            over[-1], nan[at] = ONE_ULP_DOWN(-1.0), NAN
            out.append(Case(f"guard_within_rows{rows}_at{at}", "call", [dict(row_stats=clean, guard=g, guard_limit=1.0, **kw)], redo=[0]))
            out.append(Case(f"guard_over_at_the_last_index_rows{rows}_at{at}", "call", [dict(row_stats=clean, guard=over, guard_limit=1.0, **kw)], redo=[1]))
            out.append(Case(f"guard_nan_rows{rows}_at{at}", "call", [dict(row_stats=clean, guard=nan, guard_limit=1.0, **kw)], redo=[1]))
            # err = +inf is a bad call: state[0] stays where the clean call left it
            out.append(Case(f"err_inf_rows{rows}_at{at}", "call", [dict(row_stats=clean, guard=None, guard_limit=0.0, **kw),
                                                                   dict(row_stats=_stats(rows, at, INF, 1.0), guard=None, guard_limit=0.0, **kw)], redo=[0, 1]))
            out.append(Case(f"nan_margin_rows{rows}_at{at}", "call", [dict(row_stats=_stats(rows, at, 0.25, NAN), guard=None, guard_limit=0.0, **kw)], redo=[1]))
    return out


# -- C: rails_candidates_finish on rows built for the purpose --------------------------------------------------------------------------
FINISH_ROWS, FINISH_AT = 130, (0, 63, 64, 129)
FINISH_N, FINISH_CAP, FINISH_K, FINISH_LO, FINISH_HI = 600, 64, 8, -16.0, 16.0        # bins of width 1 / 128


def crowd_row(top, n=FINISH_N, crowd=-1.0) -> np.ndarray:
    """first-pass scores of one row: `top` at scattered positions (descending values at descending positions), every other item at `crowd`
    -- more than cap items in one bin, so the candidates are exactly `top` (in distinct bins above it)"""
    row = np.full(n, crowd, dtype=np.float32)
    row[n - 5 - 7 * np.arange(len(top))] = np.asarray(top, dtype=np.float32)
    return row


# 20 candidates, m = 1.0, the 8th best at 1.75 (margin 0.75); MARGIN_02: the 8th best at float32(1.2)
PLAIN_TOP = [F(1.0 + j / 16.0) for j in range(19, -1, -1)]
MARGIN_02_TOP = [F(2.0 + j / 16.0) for j in range(6, -1, -1)] + [F(1.2)] + [F(1.0 + j / 128.0) for j in range(11, -1, -1)]
SHORT_TOP = PLAIN_TOP[:5]                                    # 5 candidates < k = 8


def plain_rows(rows=FINISH_ROWS) -> np.ndarray:
    return np.tile(crowd_row(PLAIN_TOP), (rows, 1))


def _finish_kw(approx, exact, **kw):
    base = dict(approx=approx, exact=exact, cap=FINISH_CAP, k=FINISH_K, lo=FINISH_LO, hi=FINISH_HI, default_eps=0.0, safety=1.0, one_sided=False,
                guard=None, guard_limit=0.0)
    base.update(kw)
    return base


def finish_cases() -> List[Case]:
    out = []
    # the per-row eps rule across two calls: row 0 has error 0.25, row 1 error 0 and margin 0.2
    approx = plain_rows()
    approx[1] = crowd_row(MARGIN_02_TOP)
    exact = approx.copy()
    exact[0] += F(0.25)
    out.append(Case("per_row_eps_two_calls", "finish", [_finish_kw(approx, exact), _finish_kw(approx, exact)], redo=[0, 1]))
    for at in FINISH_AT:
        approx = plain_rows()
        below = approx.copy()
        below[at] -= F(0.5)          # every exact score of the row half a unit UNDER its bound: no error, margin 1.25 - 1.0
        out.append(Case(f"one_sided_below_the_bound_at{at}", "finish", [_finish_kw(approx, below, one_sided=True)], redo=[0]))
        above = approx.copy()
        above[at, FINISH_N - 5] += F(0.5)      # the row's best score half a unit OVER its bound: the stat is 0.5, the margin 0.75
        out.append(Case(f"one_sided_above_safety1_at{at}", "finish", [_finish_kw(approx, above, one_sided=True)], redo=[0]))
        out.append(Case(f"one_sided_above_safety2_at{at}", "finish", [_finish_kw(approx, above, one_sided=True, safety=2.0)], redo=[1]))
        # 5 candidates for k = 8, every exact score of the row one unit over its first pass: the LAST candidate would clear m by 1.0 > eps = 0.5
        short = approx.copy()
        short[at] = crowd_row(SHORT_TOP)
        lifted = short.copy()
        lifted[at] += F(1.0)
        out.append(Case(f"fewer_than_k_candidates_at{at}", "finish", [_finish_kw(short, lifted, safety=0.5)], redo=[1]))
        none = approx.copy()
        none[at] = F(3.0)            # the whole row in one bin: more than cap scores in the top bin, no candidate
        out.append(Case(f"no_candidate_at{at}", "finish", [_finish_kw(none, none.copy())], redo=[1]))
        # a whole row (n <= cap) passes at any eps, but not with a NaN exact score or a guard violation
        g = torch.Generator().manual_seed(40 + at)
        whole = (torch.randn(FINISH_ROWS, 40, generator=g) * 2.0).numpy()
        out.append(Case(f"whole_row_at{at}", "finish", [_finish_kw(whole, whole.copy(), default_eps=1e9)], redo=[0]))
        nan = whole.copy()
        nan[at, 17] = NAN
        out.append(Case(f"whole_row_nan_exact_at{at}", "finish", [_finish_kw(whole, nan, default_eps=1e9)], redo=[1]))
        guard = np.full((FINISH_ROWS, 5), 0.5, dtype=np.float32)
        guard[at, 4] = ONE_ULP_UP(1.0)
        out.append(Case(f"whole_row_guard_at{at}", "finish", [_finish_kw(whole, whole.copy(), default_eps=1e9, guard=guard, guard_limit=1.0)], redo=[1]))
    return out


# -- D: rails_merge_candidates_verdict on hand-built messages --------------------------------------------------------------------------
def build_messages(R, rows, k, seed, shuffled_rank: Optional[int] = None, n_real=None):
    """(R, rows, 2k + 2) messages with strictly descending lists of scores in [1, 9) (two ranks may hold the same score), m = 0, err = 0; n_real[r] < k real entries in rank r's
    lists (the rest pads); shuffled_rank: that rank's lists are not sorted (legal for the C entry point)"""
    g = np.random.default_rng(seed)
    msgs = np.empty((R, rows, 2 * k + 2), dtype=np.int64)
    for r in range(R):
        sc = (1.0 + 8.0 * g.permutation(R * rows * k)[: rows * k].reshape(rows, k).astype(np.float64) / (R * rows * k)).astype(np.float32)
        sc = -np.sort(-sc, axis=1)
        ids = 1000 * r + g.permutation(k)[None, :] + 100_000 * np.arange(rows)[:, None]
        if n_real is not None:
            sc[:, n_real[r]:], ids[:, n_real[r]:] = NINF, -1
        if shuffled_rank == r:
            p = g.permutation(k)
            sc, ids = sc[:, p], ids[:, p]
        msgs[r, :, :k] = sc.view(np.uint32).astype(np.int64)
        msgs[r, :, k : 2 * k] = ids
        msgs[r, :, 2 * k], msgs[r, :, 2 * k + 1] = word(0.0), word(0.0)
    return msgs


def set_m(msgs, k, r, row, m):
    msgs[r, row, 2 * k] = word(m)


def set_err(msgs, k, r, row, err):
    msgs[r, row, 2 * k + 1] = word(err)


def _kth(msgs, R, k, k_out, row) -> np.float32:
    return merged(msgs, R, k, k_out).kth[row]


def _merge_kw(msgs, R, k, k_out, **kw):
    base = dict(messages=msgs, R=R, k=k, k_out=k_out, default_eps=0.0, safety=1.0, guard=None, guard_limit=0.0)
    base.update(kw)
    return base


def merge_cases() -> List[Case]:
    """every clause at R = 2, rows = 5, k = k_out = 8 and at R = 8, rows = 130, k = 200, k_out = 150, the deciding row last"""
    out = []
    for R, rows, k, k_out in ((2, 5, 8, 8), (8, 130, 200, 150), (1, 1, 1, 1)):
        row, tag, seed = rows - 1, f"R{R}_rows{rows}_k{k}_kout{k_out}", 7 * R + k

        def fresh(**kw):          # m = 0 in the deciding row, -8 in the others: their margins are 9 and more
            msgs = build_messages(R, rows, k, seed, **kw)
            msgs[:, :row, 2 * k] = word(-8.0)
            return msgs

        kth = _kth(fresh(), R, k, k_out, row)          # in [1, 9): the deciding row's margin against m = 0 is the smallest of the call, at least 1
        if R > 1:
            # the largest m sits in the LAST rank only: kth - 0.5 is less than the margin against the other ranks' m = 0
            msgs = fresh()
            set_m(msgs, k, R - 1, row, F(kth - F(0.5)))
            out.append(Case("largest_m_in_the_last_rank_" + tag, "merge", [_merge_kw(msgs, R, k, k_out, default_eps=0.75)], redo=[1]))
            # the largest error sits in a rank other than 0: eps = 2 * 0.75 against a margin below 1.5
            msgs = fresh()
            set_m(msgs, k, 0, row, F(kth - F(1.25)))
            set_err(msgs, k, R - 1, row, 0.75)
            out.append(Case("largest_err_in_another_rank_" + tag, "merge", [_merge_kw(msgs, R, k, k_out, safety=2.0)], redo=[1]))
        # one rank with err = inf, another row (or rank) with a finite error: state[0] does not move, state[3] = inf; the clean call that
        # follows is proved
        msgs = fresh()
        set_err(msgs, k, R - 1, row, INF)
        if rows > 1:
            set_err(msgs, k, 0, 0, 0.5)
        after = fresh()
        set_m(after, k, 0, row, F(kth - F(0.375)))      # a margin that 0.5, had the bad call recorded it, would not clear
        out.append(Case("a_rank_with_err_inf_" + tag, "merge", [_merge_kw(fresh(), R, k, k_out), _merge_kw(msgs, R, k, k_out), _merge_kw(after, R, k, k_out)],
                        redo=[0, 1, 0]))
        msgs = fresh()
        set_m(msgs, k, R - 1, row, NAN)
        out.append(Case("a_nan_m_" + tag, "merge", [_merge_kw(msgs, R, k, k_out)], redo=[1]))
        # every m = -inf (every shard sent all of its items) with a finite k-th score: proved at any eps
        msgs = fresh()
        msgs[:, :, 2 * k] = word(NINF)
        out.append(Case("every_m_minus_inf_" + tag, "merge", [_merge_kw(msgs, R, k, k_out, default_eps=1e30)], redo=[0]))
        # pads leave fewer than k_out real entries: kth = -inf; against a finite m the margin is -inf, against m = -inf it is a NaN
        n_real = [max(0, (k_out - 1) // R - (1 if r else 0)) for r in range(R)]
        msgs = fresh(n_real=n_real)
        out.append(Case("pads_below_k_out_" + tag, "merge", [_merge_kw(msgs, R, k, k_out)], redo=[1]))
        msgs = msgs.copy()
        msgs[:, :, 2 * k] = word(NINF)
        out.append(Case("pads_below_k_out_every_m_minus_inf_" + tag, "merge", [_merge_kw(msgs, R, k, k_out)], redo=[1]))
        # a gap equal to eps and one ulp either side (m = 0: the gap is the k-th score itself)
        for name, eps, redo in (("gap_equals_eps_", kth, 1), ("gap_one_ulp_above_eps_", ONE_ULP_DOWN(kth), 0), ("gap_one_ulp_below_eps_", ONE_ULP_UP(kth), 1)):
            out.append(Case(name + tag, "merge", [_merge_kw(fresh(), R, k, k_out, default_eps=float(eps))], redo=[redo]))
        # guard rows: within the limit, the violation in the last row only, a NaN
        guard = np.full((rows, 3), -0.5, dtype=np.float32)
        over, nan = guard.copy(), guard.copy()
        over[row, 2], nan[rows // 2, 1] = ONE_ULP_UP(1.0), NAN
        for name, gv, redo in (("guard_within_", guard, 0), ("guard_over_in_the_last_row_", over, 1), ("guard_nan_", nan, 1)):
            out.append(Case(name + tag, "merge", [_merge_kw(fresh(), R, k, k_out, guard=gv, guard_limit=1.0)], redo=[redo]))
        # three calls on one state: row 0 sees the errors 0.25, 0.5, 0.125 and the last row has a margin of 0.375 -- state[0] only rises; the
        # last row clears what the calls BEFORE it saw (its own error is 0), so it falls in the third call (rows = 1: in the second)
        calls = []
        for err in (0.25, 0.5, 0.125):
            msgs = fresh()
            set_err(msgs, k, R - 1, 0, err)
            set_m(msgs, k, 0, row, F(kth - F(0.375)))
            calls.append(_merge_kw(msgs, R, k, k_out))
        out.append(Case("three_calls_" + tag, "merge", calls, redo=[0, 0, 1] if rows > 1 else [0, 1, 1]))
    return out


def all_cases() -> List[Case]:
    return call_cases() + finish_cases() + merge_cases()


# ---- E: the whole proof on one device, ranks emulated -----------------------------------------------------------------------------------
class Family(NamedTuple):
    name: str
    B: int
    per_shard: int
    R: int
    cap: int
    k: int


# measured with the restatement (tests/test_verdict_cpu.py prints them): smallest gap 2.225 / 1.538 / 2.306 against eps = 1e-3, candidate
# counts 505-512 / 1016-1022 / 252-256 per shard and row, every row proved
FAMILIES = (Family("one_launch_select", 8, 10_000, 2, 512, 50), Family("two_launch_select", 4, 70_001, 2, 1024, 200), Family("eight_ranks", 4, 3_000, 8, 256, 100))
FAMILY_EPS, FAMILY_LO, FAMILY_HI = 1e-3, -20.4, 20.4


def family_scores(f: Family):
    """-> (s32, approx) (B, R * per_shard) float32: exact scores randn * 2 and a first pass within eps of them"""
    g = torch.Generator().manual_seed(1000 + f.per_shard)
    s32 = torch.randn(f.B, f.R * f.per_shard, generator=g) * 2.0
    approx = s32 + (torch.rand(f.B, f.R * f.per_shard, generator=g) * 2.0 - 1.0) * FAMILY_EPS
    return s32.numpy(), approx.numpy()


def is_candidate(f: Family, approx) -> np.ndarray:
    """(B, N) bool: the items some shard sends to the fp32 pass"""
    out = np.zeros(approx.shape, dtype=bool)
    for r in range(f.R):
        sl = slice(r * f.per_shard, (r + 1) * f.per_shard)
        for b, (_, cand) in enumerate(_expected(torch.as_tensor(approx[:, sl]), FAMILY_LO, FAMILY_HI, f.cap)):
            out[b, r * f.per_shard + cand.numpy()] = True
    return out


def plant_hidden_winner(f: Family, s32, approx, row):
    """The non-candidate of `row` with the best first-pass score gets an exact score one ulp above the row's k-th -> (s32', its column,
    the eps that makes |exact - approx| <= eps true for it).  It belongs to the dense top-k and is in nobody's message."""
    s32 = s32.copy()
    outside = np.where(is_candidate(f, approx)[row], NINF, approx[row])
    x = int(outside.argmax())
    kth = np.sort(s32[row])[::-1][f.k - 1]
    s32[row, x] = ONE_ULP_UP(kth)
    return s32, x, float(abs(F(s32[row, x] - approx[row, x])))


def crowd(f: Family, s32, approx, row, count=1500, value=6.0):
    """`count` items of `row`, spread evenly over the shards, tie at `value` in both passes: with more than cap of them per shard the
    threshold lies above them and fewer than k candidates are left"""
    s32, approx = s32.copy(), approx.copy()
    per = count // f.R
    for r in range(f.R):
        cols = r * f.per_shard + 3 + 2 * np.arange(per)
        s32[row, cols] = approx[row, cols] = F(value)
    return s32, approx


def full_topk(s32, k):
    """the dense top-k by (score desc, position asc) -> (scores, positions)"""
    out_s, out_i = np.empty((s32.shape[0], k), dtype=np.float32), np.empty((s32.shape[0], k), dtype=np.int64)
    pos = np.arange(s32.shape[1])
    for b in range(s32.shape[0]):
        order = key_order(s32[b], pos)[:k]
        out_s[b], out_i[b] = s32[b, order], order
    return out_s, out_i
