"""The verdict kernels of the proved exact top-k, clause by clause, against the host restatement of their contract (tests/_verdict_ref.py,
include/rails_amd.h): rails_rescore_verdict, rails_margin_stats, the clauses of rails_candidates_finish that tests/test_candidates_gpu.py
leaves open, rails_merge_candidates_verdict on hand-built messages, and the whole item-sharded proof on one device with the ranks emulated.
Everything here is integer or single-operation fp32 logic: every comparison is bit for bit.  tests/test_verdict_cpu.py shows that the
tables used here tell a correct verdict from nine kinds of wrong ones.  No counterpart in the reference, which scores every item in one
precision (rails/indexing/mol_top_k.py:99-130) on one device (eval_from_checkpoint.py:554-555)."""
import numpy as np
import pytest
import torch

from oracle import mol_oracle as O
from rails_amd import engine as E
from tests import _verdict_ref as V
from tests.test_candidates_gpu import _ws_clean

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(x, dev):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _words(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(_words(got), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))


def _pinned():
    return torch.zeros(8, dtype=torch.float32).pin_memory()


def _check_states(case, got, mirrors=None):
    want = V.run_case(case)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert V.state_words(g) == V.state_words(w), (case.name, i, g.tolist(), w.tolist())
        assert V.redo_of(g) == case.redo[i], (case.name, i)
        if mirrors is not None:
            assert V.state_words(mirrors[i]) == V.state_words(g), (case.name, i, "host mirror")
    seen = [float(g[0]) for g in got]
    assert seen == sorted(seen) and [float(g[5]) for g in got] == [float(i + 1) for i in range(len(got))], case.name
    assert [float(g[6]) for g in got] == [float(sum(case.redo[: i + 1])) for i in range(len(got))], case.name


# ---- A: rails_rescore_verdict ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", V.VERDICT_ROWS)
def test_rescore_verdict_follows_the_call_rule(dev, rows):
    cases = [c for c in V.call_cases() if f"rows{rows}_at" in c.name]
    assert len(cases) >= 11
    for case in cases:
        state = torch.zeros(8, dtype=torch.float32, device=dev)
        got = []
        for kw in case.calls:
            E.rescore_verdict(_t(kw["row_stats"], dev), state, kw["default_eps"], kw["safety"], _t(kw["guard"], dev), kw["guard_limit"])
            got.append(state.cpu().numpy().copy())
        _check_states(case, got)
        if case.name.startswith("sequence_"):
            # the NaN call leaves state[0] alone and records inf; the clean call after it still runs at call 2's eps
            assert float(got[2][0]) == 0.5 and float(got[2][3]) == np.inf and float(got[3][0]) == 0.5 and float(got[3][2]) == float(got[1][2])


# ---- B: rails_margin_stats ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 300])
def test_margin_stats_is_the_stated_difference(dev, rows):
    col, ld = 4, 9
    g = np.random.default_rng(rows)
    kth = (g.standard_normal((rows, ld)) * 3.0).astype(np.float32)
    m = g.standard_normal(rows).astype(np.float32)
    if rows > 1:
        m[[3, 64, 255, 256, 299]] = [np.inf, -np.inf, np.nan, np.inf, -np.inf]
        kth[[5, 64, 256], col] = [np.inf, -np.inf, np.inf]          # inf - (-inf) stays out; -inf - -inf and inf - inf are NaN
    err = np.array([0.375], dtype=np.float32)
    got = E.margin_stats(_t(kth, dev), col, _t(m, dev), _t(err, dev))
    want = V.margin_stats(kth, col, m, err)
    assert got.shape == (rows, 2)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got.cpu().numpy()), nan) and (rows == 1 or nan[:, 1].sum() == 3)
    assert np.array_equal(_words(got)[~nan], want.view(np.uint32)[~nan])
    # fed to rails_rescore_verdict: a NaN margin, or none
    for stats in (got, got[:3] if rows > 1 else got):
        state = torch.zeros(8, dtype=torch.float32, device=dev)
        E.rescore_verdict(stats.contiguous(), state, 0.0, 1.0)
        assert V.state_words(state) == V.state_words(V.call_verdict(stats.cpu().numpy(), V.new_state(), 0.0, 1.0))


# ---- C: rails_candidates_finish ----------------------------------------------------------------------------------------------------------
def _select(dev, approx, cap, lo, hi):
    B = approx.shape[0]
    ws = E.candidates_workspace(B, dev)
    pos = torch.zeros((B, cap), dtype=torch.int64, device=dev)
    a = torch.zeros((B, cap), dtype=torch.float32, device=dev)
    E.candidates_select(approx, cap, lo, hi, ws, pos, a)
    torch.cuda.synchronize()
    return ws, pos, a, ws[:B].cpu().numpy().copy()


def _finish(dev, kw, state, host):
    """select on kw's first-pass rows, the exact scores gathered at the candidates, finish -> (counts, out_scores, out_ids); the slots past a
    row's count hold item 0's values, which the kernel must not look at"""
    approx, exact_all = _t(kw["approx"], dev), _t(kw["exact"], dev)
    N, cap = approx.shape[1], kw["cap"]
    ws, pos, a, counts = _select(dev, approx, cap, kw["lo"], kw["hi"])
    exact = torch.gather(exact_all, 1, pos)
    ids = torch.arange(N, dtype=torch.int64, device=dev) * 3 + 1
    guard = _t(kw["guard"], dev)
    out_s, out_i, _, _ = E.candidates_finish(exact, a, pos, cap, ws, ids, N, kw["k"], kw["default_eps"], kw["safety"], kw["one_sided"], guard,
                                             0 if guard is None else guard.shape[1], kw["guard_limit"], state, host)
    torch.cuda.synchronize()
    assert _ws_clean(ws, approx.shape[0]), "the workspace is not left zeroed"
    return counts, out_s, out_i


@pytest.mark.parametrize("name", [c.name for c in V.finish_cases()])
def test_candidates_finish_clause(dev, name):
    case = next(c for c in V.finish_cases() if c.name == name)
    state, host = torch.zeros(8, dtype=torch.float32, device=dev), _pinned()
    got, mirrors = [], []
    for kw in case.calls:
        counts, out_s, out_i = _finish(dev, kw, state, host)
        got.append(state.cpu().numpy().copy())
        mirrors.append(host.numpy().copy())
        rows = V.finish_rows(kw["approx"], kw["exact"], kw["cap"], kw["k"], kw["lo"], kw["hi"], kw["one_sided"])
        assert [r.count for r in rows] == counts.tolist()
        k = kw["k"]
        for b, r in enumerate(rows):
            if r.count >= k and not r.bad:
                assert _same_bits(out_s[b], r.scores[:k]) and out_i[b].tolist() == (r.positions[:k] * 3 + 1).tolist(), (name, b)
    _check_states(case, got, mirrors)
    if name == "per_row_eps_two_calls":
        # row 1 (error 0, margin 0.2) is proved while nothing has been seen, and falls to row 0's 0.25 once the state carries it
        assert [float(g[0]) for g in got] == [0.25, 0.25] and float(got[0][4]) == float(np.float32(1.2) - np.float32(1.0))
    if name.startswith("one_sided_above"):
        assert float(got[0][3]) == 0.5 and float(got[0][4]) == 0.75
    if name.startswith("one_sided_below"):
        assert float(got[0][0]) == 0.0 and float(got[0][4]) == 0.25
    if name.startswith(("fewer_than_k", "no_candidate")):
        assert float(got[0][4]) == -np.inf and float(got[0][3]) != np.inf
    if name.startswith("whole_row"):
        assert float(got[0][2]) == float(np.float32(1e9))
        assert float(got[0][3]) == (np.inf if "nan" in name or "guard" in name else 0.0)


def test_candidates_finish_message_edges(dev):
    """m = -inf (whole row), +inf (no candidate) or the smallest first-pass score; err = inf for a NaN row; (-inf, -1) from the count on;
    k > cap only with a message"""
    cap, lo, hi, N = V.FINISH_CAP, V.FINISH_LO, V.FINISH_HI, V.FINISH_N
    approx = V.plain_rows()
    approx[1] = V.crowd_row(V.MARGIN_02_TOP)
    approx[0] = 3.0                                  # no candidate
    approx[63] = V.crowd_row(V.SHORT_TOP)            # 5 candidates
    approx[129, 2] = np.nan                          # a NaN in the first pass, outside the candidates
    exact = approx + np.float32(0.125)
    exact[64, N - 5 - 7 * 3] = np.nan                # a NaN exact score on a candidate
    exact[129, 2] = 0.0
    g = torch.Generator().manual_seed(3)
    whole = (torch.randn(V.FINISH_ROWS, 40, generator=g) * 2.0).numpy()
    for a_np, e_np, ks in ((approx, exact, (8, 20, 80)), (whole, whole + np.float32(0.25), (8, 40, 50))):
        B, n = a_np.shape
        ids = torch.arange(n, dtype=torch.int64, device=dev) * 2 + 5
        for k in ks:
            ws, pos, a, counts = _select(dev, _t(a_np, dev), cap, lo, hi)
            ex = torch.gather(_t(e_np, dev), 1, pos)
            msg = torch.full((B, 2 * k + 2), 77, dtype=torch.int64, device=dev)
            E.candidates_finish(ex, a, pos, cap, ws, ids, n, k, 0.0, 1.0, False, None, 0, 0.0, None, None, msg=msg)
            torch.cuda.synchronize()
            assert _ws_clean(ws, B)
            got = msg.cpu().numpy()
            for b in range(B):
                want = V.shard_message(a_np[b], e_np[b], 0, np.arange(n) * 2 + 5, cap, k, lo, hi)
                assert np.array_equal(got[b], want), (n, k, b, got[b], want)
            m, err = V.unword(got[:, 2 * k]), V.unword(got[:, 2 * k + 1])
            if n == N:
                assert m[0] == np.inf and m[63] == V.SHORT_TOP[-1] and m[1] == 1.0 and err[64] == np.inf and err[129] == np.inf and err[1] == 0.125
                assert (got[0, :k] == V.word(-np.inf)).all() and (got[0, k : 2 * k] == -1).all()
                assert (got[63, 5:k] == V.word(-np.inf)).all() and (got[63, k + 5 : 2 * k] == -1).all() and (got[63, k : k + 5] >= 0).all()
                assert (got[1, min(k, 20) : k] == V.word(-np.inf)).all() and (got[1, k + min(k, 20) : 2 * k] == -1).all()
            else:
                assert (m == -np.inf).all() and (np.abs(err - 0.25) < 1e-6).all() and (got[:, min(k, 40) : k] == V.word(-np.inf)).all()
    # without a message k > cap is refused before anything is launched
    ws, pos, a, counts = _select(dev, _t(approx, dev), cap, lo, hi)
    state = torch.zeros(8, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        E.candidates_finish(torch.gather(_t(exact, dev), 1, pos), a, pos, cap, ws, None, N, 80, 0.0, 1.0, False, None, 0, 0.0, state, None)
    torch.cuda.synchronize()
    assert V.state_words(state) == [0] * 8 and ws[: V.FINISH_ROWS].cpu().numpy().tolist() == counts.tolist()


# ---- D: rails_merge_candidates_verdict on hand-built messages ------------------------------------------------------------------------
def _call_ws(rows, dev):
    return torch.zeros(8 + 4 * rows, dtype=torch.int32, device=dev)


def _row_fails(call_ws, rows):
    """the rows' verdict words of the last call: 16 bytes per row behind the 8-word header, the fourth word's bit 0 = the row failed
    (verdict_commit, rails_amd/csrc/topk.hip)"""
    return [bool(int(w) & 1) for w in call_ws[8 : 8 + 4 * rows].cpu().numpy().reshape(rows, 4)[:, 3]]


def _merge(dev, kw, state, host, call_ws, seen=None):
    msgs = kw["messages"]
    R, rows = msgs.shape[0], msgs.shape[1]
    guard = _t(kw["guard"], dev)
    out = E.merge_candidates_verdict(_t(msgs.reshape(R * rows, -1), dev), R, kw["k"], kw["k_out"], kw["default_eps"], kw["safety"], guard,
                                     0 if guard is None else guard.shape[1], kw["guard_limit"], state, host, call_ws, seen)
    torch.cuda.synchronize()
    assert int(call_ws[0]) == 0, "the arrival counter is not left zero"
    return out


@pytest.mark.parametrize("R,rows,k,k_out,shuffled", [(1, 1, 1, 1, None), (1, 5, 8, 8, None), (2, 5, 8, 8, None), (2, 130, 8, 5, None), (2, 1, 200, 200, None),
                                                      (8, 130, 200, 200, None), (8, 130, 200, 150, None), (8, 1, 1, 1, None), (8, 5, 200, 200, 3),
                                                      (2, 130, 8, 8, 1), (8, 5, 8, 3, 0)])
def test_merge_verdict_outputs(dev, R, rows, k, k_out, shuffled):
    """the merged top-k_out under the key order (descending lists: rank counting; one shuffled list: the bitonic sort)"""
    msgs = V.build_messages(R, rows, k, 100 * R + k, shuffled_rank=shuffled)
    tie_row = rows - 1
    if R > 1 and shuffled is None:          # the best score of the last rank ties the best of rank 0, above everything else
        msgs[0, tie_row, 0] = msgs[R - 1, tie_row, 0] = V.word(9.5)
    state, host, call_ws = torch.zeros(8, dtype=torch.float32, device=dev), _pinned(), _call_ws(rows, dev)
    kw = dict(messages=msgs, k=k, k_out=k_out, default_eps=0.0, safety=1.0, guard=None, guard_limit=0.0)
    out_s, out_i = _merge(dev, kw, state, host, call_ws)
    mg, fails, want_state = V.merge_call(msgs, R, k, k_out, V.new_state(), 0.0, 1.0)
    assert _same_bits(out_s, mg.scores) and np.array_equal(out_i.cpu().numpy(), mg.ids)
    assert V.state_words(state) == V.state_words(want_state) == V.state_words(host) and _row_fails(call_ws, rows) == fails
    # the oracle's deterministic selection over the concatenated lists, ids gathered
    sc = V.unword(msgs[:, :, :k]).transpose(1, 0, 2).reshape(rows, R * k)
    ids = msgs[:, :, k : 2 * k].transpose(1, 0, 2).reshape(rows, R * k)
    o_s, o_pos = O.select_topk_deterministic(torch.from_numpy(sc.copy()), k_out)
    assert torch.equal(out_s.cpu(), o_s) and torch.equal(out_i.cpu(), torch.gather(torch.from_numpy(ids.copy()), 1, o_pos))
    # rails_merge_candidates on the same lists without the two verdict words
    plain = _t(np.ascontiguousarray(msgs[:, :, : 2 * k]).reshape(R * rows, 2 * k), dev)
    p_s, p_i = E.merge_candidates(plain, R, k, k_out)
    assert torch.equal(out_s, p_s) and torch.equal(out_i, p_i)
    if R > 1 and shuffled is None:
        assert int(out_i[tie_row, 0]) == int(msgs[0, tie_row, k])
        assert k_out == 1 or (int(out_i[tie_row, 1]) == int(msgs[R - 1, tie_row, k]) and float(out_s[tie_row, 1]) == 9.5)


@pytest.mark.parametrize("tag", ["R1_rows1_k1_kout1", "R2_rows5_k8_kout8", "R8_rows130_k200_kout150"])
def test_merge_verdict_clause_table(dev, tag):
    cases = [c for c in V.merge_cases() if c.name.endswith(tag)]
    assert len(cases) >= (12 if tag.startswith("R1_") else 14)
    for case in cases:
        rows = case.calls[0]["messages"].shape[1]
        state, host, call_ws = torch.zeros(8, dtype=torch.float32, device=dev), _pinned(), _call_ws(rows, dev)
        got, mirrors = [], []
        for kw in case.calls:
            kw = {key: val for key, val in kw.items() if key != "R"}
            out_s, out_i = _merge(dev, kw, state, host, call_ws)
            got.append(state.cpu().numpy().copy())
            mirrors.append(host.numpy().copy())
            mg, fails, _ = V.merge_call(state=V.new_state() if len(got) == 1 else got[-2], **case.calls[len(got) - 1])
            assert _same_bits(out_s, mg.scores) and np.array_equal(out_i.cpu().numpy(), mg.ids), case.name
            assert _row_fails(call_ws, rows) == fails, case.name
        _check_states(case, got, mirrors)
        if case.name.startswith("a_rank_with_err_inf"):
            assert float(got[1][0]) == float(got[0][0]) == 0.0 and float(got[1][3]) == np.inf and float(got[2][3]) == 0.0
        if case.name.startswith(("pads_below", "a_nan_m")):
            assert float(got[0][4]) == -np.inf
        if case.name.startswith("every_m_minus_inf"):
            assert float(got[0][4]) == np.inf
        if case.name.startswith("guard_over"):
            assert float(got[0][7]) == float(V.ONE_ULP_UP(1.0)) and _row_fails(call_ws, rows) == [b == rows - 1 for b in range(rows)]
        if case.name.startswith("guard_nan"):
            assert float(got[0][7]) == np.inf


@pytest.mark.parametrize("R,rows,k,k_out,width,k_f", [(2, 130, 8, 8, 5, 4), (8, 5, 200, 150, 40, 120)])
def test_merge_verdict_with_the_seen_filter(dev, R, rows, k, k_out, width, k_f):
    msgs = V.build_messages(R, rows, k, 31 * R + k)
    V.set_err(msgs, k, R - 1, 0, 0.25)
    kw = dict(messages=msgs, k=k, k_out=k_out, default_eps=0.0, safety=1.0, guard=None, guard_limit=0.0)
    s0, c0 = torch.zeros(8, dtype=torch.float32, device=dev), _call_ws(rows, dev)
    out_s, out_i = _merge(dev, kw, s0, None, c0)
    g = torch.Generator().manual_seed(width)
    pick = torch.stack([torch.randperm(k_out, generator=g)[:width] for _ in range(rows)]).to(dev)
    inv = torch.gather(out_i, 1, pick)
    inv[:, -1] = -5                          # an id nobody holds
    want_i, want_s = E.filter_seen_ids(out_i, out_s, inv, k_f)
    s1, h1, c1 = torch.zeros(8, dtype=torch.float32, device=dev), _pinned(), _call_ws(rows, dev)
    f_i, f_s = _merge(dev, kw, s1, h1, c1, seen=(inv, k_f))
    assert torch.equal(f_i, want_i) and torch.equal(f_s, want_s)
    assert V.state_words(s1) == V.state_words(s0) == V.state_words(h1) and float(s1[0]) == 0.25


# ---- E: the whole proof on one device, the ranks emulated -----------------------------------------------------------------------------
def _emulate(dev, f, s32, approx, default_eps):
    """per shard: select on the first pass, exact scores at the candidates, the message form of the finish with global ids; the messages
    rank-major through rails_merge_candidates_verdict -> (scores, ids, state, per-row fail, the gathered messages)"""
    s32_d, approx_d = _t(s32, dev), _t(approx, dev)
    n, msgs = f.per_shard, []
    for r in range(f.R):
        shard = approx_d[:, r * n : (r + 1) * n]
        ws, pos, a, counts = _select(dev, shard, f.cap, V.FAMILY_LO, V.FAMILY_HI)
        exact = torch.gather(s32_d[:, r * n : (r + 1) * n], 1, pos)
        ids = torch.arange(r * n, (r + 1) * n, dtype=torch.int64, device=dev)
        msg = torch.empty((f.B, 2 * f.k + 2), dtype=torch.int64, device=dev)
        E.candidates_finish(exact, a, pos, f.cap, ws, ids, n, f.k, 0.0, 1.0, False, None, 0, 0.0, None, None, msg=msg)
        torch.cuda.synchronize()
        assert _ws_clean(ws, f.B)
        msgs.append(msg)
    gathered = torch.cat(msgs, 0)
    state, host, call_ws = torch.zeros(8, dtype=torch.float32, device=dev), _pinned(), _call_ws(f.B, dev)
    out_s, out_i = E.merge_candidates_verdict(gathered, f.R, f.k, f.k, default_eps, 1.0, None, 0, 0.0, state, host, call_ws)
    torch.cuda.synchronize()
    assert int(call_ws[0]) == 0 and V.state_words(host) == V.state_words(state)
    return out_s, out_i, state.cpu().numpy(), _row_fails(call_ws, f.B), gathered.cpu().numpy().reshape(f.R, f.B, -1)


def _against_the_restatement(f, s32, approx, default_eps, state, fails, gathered):
    want = V.shard_messages(approx, s32, f.R, f.cap, f.k, V.FAMILY_LO, V.FAMILY_HI)
    assert np.array_equal(gathered, want)
    mg, want_fails, want_state = V.merge_call(want, f.R, f.k, f.k, V.new_state(), default_eps, 1.0)
    assert fails == want_fails and V.state_words(state) == V.state_words(want_state)


def _proved_rows_are_dense(f, s32, out_s, out_i, fails):
    d_s, d_i = O.select_topk_deterministic(torch.from_numpy(s32), f.k)
    for b in range(f.B):
        if not fails[b]:
            assert torch.equal(out_s[b].cpu(), d_s[b]) and torch.equal(out_i[b].cpu(), d_i[b]), b


@pytest.mark.parametrize("f", V.FAMILIES, ids=lambda f: f.name)
def test_whole_proof_benign_and_planted(dev, f):
    s32, approx = V.family_scores(f)
    out_s, out_i, state, fails, gathered = _emulate(dev, f, s32, approx, V.FAMILY_EPS)
    _against_the_restatement(f, s32, approx, V.FAMILY_EPS, state, fails, gathered)
    assert fails == [False] * f.B and V.redo_of(state) == 0           # every row is proved (tests/test_verdict_cpu.py), so none is left out below
    _proved_rows_are_dense(f, s32, out_s, out_i, fails)
    # a winner hidden outside the candidates, under a declared bound that is true for it: the call must not be proved
    row = f.B - 1
    planted, x, eps = V.plant_hidden_winner(f, s32, approx, row)
    out_s, out_i, state, fails, gathered = _emulate(dev, f, planted, approx, eps)
    _against_the_restatement(f, planted, approx, eps, state, fails, gathered)
    assert V.redo_of(state) == 1 and fails[row] and x not in out_i[row].tolist()
    _proved_rows_are_dense(f, planted, out_s, out_i, fails)


def test_whole_proof_crowded_row(dev):
    f = V.FAMILIES[0]
    row = 2
    s32, approx = V.crowd(f, *V.family_scores(f), row)
    out_s, out_i, state, fails, gathered = _emulate(dev, f, s32, approx, V.FAMILY_EPS)
    _against_the_restatement(f, s32, approx, V.FAMILY_EPS, state, fails, gathered)
    assert V.redo_of(state) == 1 and float(state[4]) == -np.inf and fails == [b == row for b in range(f.B)]
    assert (gathered[:, row, f.k - 1] == V.word(-np.inf)).all()          # fewer than k candidates on every shard
    _proved_rows_are_dense(f, s32, out_s, out_i, fails)
