"""CPU: the one speculate-and-verify flow of the candidate scans (topk_modules._speculative_scan) on its own, with no device -- stand-ins
replace the fused launcher, the scorer, the selection, the restriction and the word allocator (pinned memory needs a device) and record
their calls.  Scores are 1000 * (batch row) + column, so every output row names the batch row it was computed for."""
import pytest
import torch

from rails_amd import topk_modules as T

N, K, RPQ = 7, 3, 2      # items, selected per row, rows of the score matrix per batch row


class Module:
    """What the flow touches of a module: _no_fused, the free list of verdict words, the recycled buffers."""

    def __init__(self, log):
        self._no_fused, self._flag_free, self.log = False, [], log

    def _buf(self, tag, numel, dtype):
        self.log.append(("buf", tag, numel))
        return torch.empty(numel, dtype=dtype)


class Restr:
    """A restriction that records what is asked of it; its slices name their rows."""

    def __init__(self, log, rows=None):
        self.log, self.rows = log, rows

    @property
    def count(self):      # (what k is checked against: asked once per sub-call)
        self.log.append(("count", self.rows))
        return N

    def launch_kwargs(self):
        return {"visible": self}

    def mask(self, scores, run_if=None):
        self.log.append(("mask", self.rows, run_if))
        return scores

    def rows_slice(self, b0, b1):
        return Restr(self.log, (b0, b1))


def row_scores(eq):
    rows = eq[:, 0, 0].repeat_interleave(RPQ)
    return 1000.0 * rows[:, None] + torch.arange(N, dtype=torch.float32)[None, :]


def make_scan(log, route=(True, True), width=4, fused=True, on_device=False, device_word=None, n=N, k=K):
    def launch(eq, flag, **kw):
        log.append(("launch", eq.shape[0], flag, kw))
        s = row_scores(eq)[:, :k].clone()
        return (s, s.to(torch.int64), flag if flag is not None else torch.zeros(1, dtype=torch.int32)) if fused else None

    def scores(eq, out=None, run_if=None):
        log.append(("scores", eq.shape[0], None if out is None else tuple(out.shape), run_if))
        return row_scores(eq)

    return T.CandidateScan(n=n, k=k, rows_per_query=RPQ, route=lambda batch, restr: (log.append(("route", batch)), route)[1],
                           width=lambda allowed: (log.append(("width", allowed)), width)[1], launch=launch, scores=scores, redo_buffer="redo",
                           redo_on_device=lambda batch: on_device, device_flag=lambda: device_word, shaped=lambda pos, batch: pos.view(batch, -1))


@pytest.fixture
def flow(monkeypatch):
    log = []
    tk = Module(log)
    monkeypatch.setattr(T, "_pinned_word", lambda module: module._flag_free.pop() if module._flag_free else torch.zeros(1, dtype=torch.int32))

    def topk(scores, k, out=None, run_if=None):
        log.append(("topk", k, out is not None, run_if))
        return scores[:, :k].clone(), scores[:, :k].to(torch.int64)

    monkeypatch.setattr(T.E, "topk", topk)
    return tk, log


def queries(batch):
    return torch.arange(batch, dtype=torch.float32)[:, None, None].expand(batch, 2, 3).contiguous()


def kinds(log, *names):
    return [e[0] for e in log if e[0] in names]


def batch_rows(pos):
    return (pos.reshape(-1, K)[:, 0] // 1000).tolist()


@pytest.mark.parametrize("with_scores", [False, True])
@pytest.mark.parametrize("fused", [False, True])
def test_a_batch_wider_than_the_slice_goes_in_slices_concatenated_in_order(flow, with_scores, fused):
    tk, log = flow
    restr, pending = Restr(log), []
    out = T._speculative_scan(tk, make_scan(log, route=(fused, True), width=4), queries(10), restr, pending, with_scores)
    assert [e[1] for e in log if e[0] == "route"] == [10, 4, 4, 2]                          # the whole batch, then one sub-call per slice
    assert [e[1] for e in log if e[0] == ("launch" if fused else "scores")] == [4, 4, 2]
    assert [e[1] for e in log if e[0] == "count"] == [None, (0, 4), (4, 8), (8, 12)]      # rows_slice of the restriction, slice by slice
    want = [b for b in range(10) for _ in range(RPQ)]
    if with_scores:
        sc, pos = out
        assert sc.shape == pos.shape == (10 * RPQ, K) and batch_rows(pos) == want and torch.equal(sc, pos.float())
    else:
        assert out.shape == (10, RPQ * K) and batch_rows(out) == want
    if fused:      # the deferred verdict: one host word per slice, each slice's launch under its own word and its own restriction
        launches = [e for e in log if e[0] == "launch"]
        assert len(pending) == 3 and len({id(w) for w in pending}) == 3 and all(l[2] is w for l, w in zip(launches, pending))
        assert [l[3]["visible"].rows for l in launches] == [(0, 4), (4, 8), (8, 12)]
        assert not kinds(log, "scores", "mask", "topk")
    else:
        assert [e[1] for e in log if e[0] == "mask"] == [(0, 4), (4, 8), (8, 12)] and not pending


def test_a_fused_launch_that_answers_none_materialises_and_returns_its_word(flow):
    tk, log = flow
    word = torch.zeros(1, dtype=torch.int32)
    tk._flag_free.append(word)
    for _ in range(3):
        pending = []
        out = T._speculative_scan(tk, make_scan(log, fused=False), queries(2), Restr(log), pending)
        assert batch_rows(out) == [0, 0, 1, 1] and not pending
        assert len(tk._flag_free) == 1 and tk._flag_free[0] is word      # taken before the launch, back on the free list after it: no growth, no leak
    assert kinds(log, "launch", "scores", "mask", "topk") == ["launch", "scores", "mask", "topk"] * 3
    assert all(e[2] is word for e in log if e[0] == "launch")
    # nothing to return where no word was taken (a redo on the device, a verdict read at once)
    T._speculative_scan(tk, make_scan(log, fused=False, on_device=True, device_word=torch.zeros(1, dtype=torch.int32)), queries(2), None, [])
    T._speculative_scan(tk, make_scan(log, fused=False), queries(2), None, None)
    assert tk._flag_free == [word]


def test_the_redo_on_the_device_runs_scorer_mask_selection_under_the_flag(flow):
    tk, log = flow
    flag, pending = torch.zeros(1, dtype=torch.int32), []
    tk._flag_free.append(torch.zeros(1, dtype=torch.int32))
    out = T._speculative_scan(tk, make_scan(log, on_device=True, device_word=flag), queries(3), Restr(log), pending, with_scores=True)
    assert kinds(log, "launch", "scores", "mask", "topk") == ["launch", "scores", "mask", "topk"]
    launch, scores, mask, topk = (e for e in log if e[0] in ("launch", "scores", "mask", "topk"))
    assert launch[2] is flag and scores[3] is flag and mask[2] is flag and topk[3] is flag
    assert scores[2] == (3 * RPQ, N) and ("buf", "redo", 3 * RPQ * N) in log and topk[2]      # the recycled matrix; the selection overwrites the fused outputs
    assert not pending and len(tk._flag_free) == 1                                            # no host word is taken or deferred
    assert batch_rows(out[1]) == [0, 0, 1, 1, 2, 2]


def test_a_deferred_verdict_appends_one_host_word_and_returns_at_once(flow):
    tk, log = flow
    pending = []
    out = T._speculative_scan(tk, make_scan(log), queries(4), None, pending)
    launch, = (e for e in log if e[0] == "launch")
    assert len(pending) == 1 and launch[2] is pending[0] and not pending[0].is_cuda and launch[3] == {}
    assert batch_rows(out) == [0, 0, 1, 1, 2, 2, 3, 3] and not kinds(log, "scores", "mask", "topk")


@pytest.mark.parametrize("bad", [0, 1])
def test_a_verdict_nobody_defers_is_read_at_once(flow, bad):
    tk, log = flow
    word = torch.full((1,), bad, dtype=torch.int32)
    T._speculative_scan(tk, make_scan(log, device_word=word), queries(2), Restr(log), None)
    assert kinds(log, "launch", "scores", "mask", "topk") == (["launch", "scores", "mask", "topk"] if bad else ["launch"])
    assert next(e for e in log if e[0] == "launch")[2] is word and not tk._flag_free


@pytest.mark.parametrize("no_fused,route", [(True, (True, True)), (False, (False, True)), (False, (True, False))])
def test_a_scan_that_is_not_fused_masks_before_it_selects(flow, no_fused, route):
    tk, log = flow
    tk._no_fused = no_fused
    pending = []
    out = T._speculative_scan(tk, make_scan(log, route=route), queries(2), Restr(log), pending)
    assert kinds(log, "launch", "scores", "mask", "topk") == ["scores", "mask", "topk"] and not pending
    assert all(e[-1] is None for e in log if e[0] in ("scores", "mask", "topk"))      # no launch predicate
    assert batch_rows(out) == [0, 0, 1, 1]


def test_without_a_restriction_nothing_is_masked(flow):
    tk, log = flow
    flag = torch.zeros(1, dtype=torch.int32)
    T._speculative_scan(tk, make_scan(log, on_device=True, device_word=flag), queries(2), None, [])      # the redo on the device
    T._speculative_scan(tk, make_scan(log, route=(False, True)), queries(2), None, [])                   # the materialising route
    T._speculative_scan(tk, make_scan(log, fused=False), queries(2), None, None)                         # sizes without a plan
    T._speculative_scan(tk, make_scan(log, width=1), queries(2), None, [])                               # slices
    assert not kinds(log, "mask", "count") and all(e[3] == {} for e in log if e[0] == "launch")


def test_k_is_checked_before_the_route_is_asked(flow):
    tk, log = flow
    with pytest.raises(RuntimeError, match=r"selected index k out of range \(k=8, n=7\)"):
        T._speculative_scan(tk, make_scan(log, k=8), queries(2), Restr(log), [])
    assert not kinds(log, "route", "width", "launch", "scores")
    restr = T.Restriction.of(None, type("Filter", (), {"kept_min": 2})())      # the real value: the count each k is checked against
    with pytest.raises(RuntimeError, match=r"selected index k out of range \(k=3, n=2\)"):
        T._speculative_scan(tk, make_scan(log), queries(2), restr, [])
    assert not kinds(log, "route", "width", "launch", "scores")
