"""GPU: the streaming score calls (rank_of, rank_of_positions, log_partition, log_prob_of, log_prob_of_positions, sample_items, count_above,
range_search; DESIGN sections 3.17 - 3.19) as ONE flow: every error a call raises before its dense pass, character for character; a batch
sliced by the logit policy -- the last slice a single row -- against the unsliced call; a score matrix without rows.  MoLBruteForceTopK (the
fused route) and MIPSBruteForceTopK over N = 70 items (three 32-item tiles, a ragged tail) and B = 3 query rows.  Inputs: those of
tests/test_item_mask_gpu.py."""
import pytest
import torch

from rails_amd import engine as E
from tests import test_item_mask_gpu as M

pytestmark = pytest.mark.gpu
N, B = 70, 3
MODULES = [("brute", "default"), ("mips", "mips")]
CALLS = ("rank_of", "rank_of_positions", "log_partition", "log_prob_of", "log_prob_of_positions", "sample_items", "count_above", "range_search")
RANK_WHOLE = "a target's key must be read from the matrix that is counted, and corpus chunks are not built"
SOFTMAX_WHOLE = "the normaliser needs every item of a row, and corpus chunks are not built"
RANGE_WHOLE = "a row is counted and written whole, and corpus chunks are not built"
WITH_MIN_SCORE = "a score threshold is compared with the raw logit; temperature goes with min_log_prob="

# (call, what is wrong -- a key of wrong_arguments --, the exception, its str; {cls}: the module's class name)
ERRORS = [
    ("rank_of", "invalid_ids", ValueError, "rank_of_positions: invalid_ids must be (3, S) integer ids"),
    ("rank_of", "target_ids", ValueError, "rank_of: target_ids must be (3, T) integer ids"),
    ("rank_of", "policy", NotImplementedError, "{cls}.rank_of: one row of 70 logits exceeds MAX_LOGIT_BYTES; " + RANK_WHOLE),
    ("rank_of_positions", "invalid_ids", ValueError, "rank_of_positions: invalid_ids must be (3, S) integer ids"),
    ("rank_of_positions", "positions", ValueError, "rank_of_positions: positions must be (3, T) int64"),
    ("rank_of_positions", "policy", NotImplementedError, "{cls}.rank_of: one row of 70 logits exceeds MAX_LOGIT_BYTES; " + RANK_WHOLE),
    ("log_partition", "invalid_ids", ValueError, "log_partition: invalid_ids must be (3, S) integer ids"),
    ("log_partition", "temperature 0", ValueError, "{cls}.log_partition: temperature must be a finite number > 0, got 0"),
    ("log_partition", "temperature nan", ValueError, "{cls}.log_partition: temperature must be a finite number > 0, got nan"),
    ("log_partition", "temperature tiny", ValueError, "{cls}.log_partition: 1 / temperature is not a finite fp32 > 0 for temperature = 1e-60"),
    ("log_partition", "policy", NotImplementedError, "{cls}.log_partition: one row of 70 logits exceeds MAX_LOGIT_BYTES; " + SOFTMAX_WHOLE),
    ("log_prob_of", "invalid_ids", ValueError, "log_prob_of: invalid_ids must be (3, S) integer ids"),
    ("log_prob_of", "target_ids", ValueError, "log_prob_of: target_ids must be (3, T) integer ids"),
    ("log_prob_of", "temperature 0", ValueError, "{cls}.log_prob_of: temperature must be a finite number > 0, got 0"),
    ("log_prob_of", "policy", NotImplementedError, "{cls}.log_prob_of: one row of 70 logits exceeds MAX_LOGIT_BYTES; " + SOFTMAX_WHOLE),
    ("log_prob_of_positions", "invalid_ids", ValueError, "log_prob_of_positions: invalid_ids must be (3, S) integer ids"),
    ("log_prob_of_positions", "positions", ValueError, "log_prob_of_positions: positions must be (3, T) int64"),
    ("log_prob_of_positions", "temperature 0", ValueError, "{cls}.log_prob_of_positions: temperature must be a finite number > 0, got 0"),
    ("log_prob_of_positions", "policy", NotImplementedError,
     "{cls}.log_prob_of_positions: one row of 70 logits exceeds MAX_LOGIT_BYTES; " + SOFTMAX_WHOLE),
    ("sample_items", "invalid_ids", ValueError, "sample_items: invalid_ids must be (3, S) integer ids"),
    ("sample_items", "temperature 0", ValueError, "{cls}.sample_items: temperature must be a finite number > 0, got 0"),
    ("sample_items", "num_samples 0", ValueError,
     "sample_items: num_samples must be an int in [1, 70] (the corpus holds 70 items, the exact top-k takes k <= 16384), got 0"),
    ("sample_items", "num_samples 71", ValueError,
     "sample_items: num_samples must be an int in [1, 70] (the corpus holds 70 items, the exact top-k takes k <= 16384), got 71"),
    ("sample_items", "seed -1", ValueError, "sample_items: seed must be an int in [0, 2^64), got -1"),
    ("sample_items", "seed 2^64", ValueError, "sample_items: seed must be an int in [0, 2^64), got 18446744073709551616"),
    ("sample_items", "policy", NotImplementedError, "{cls}.sample_items: two rows of 70 logits exceed MAX_LOGIT_BYTES; " + SOFTMAX_WHOLE),
    ("count_above", "invalid_ids", ValueError, "count_above: invalid_ids must be (3, S) integer ids"),
    ("count_above", "temperature 0", ValueError, "{cls}.count_above: temperature must be a finite number > 0, got 0"),
    ("count_above", "both", ValueError, "{cls}.count_above: exactly one of min_score= and min_log_prob= is given, got both"),
    ("count_above", "neither", ValueError, "{cls}.count_above: exactly one of min_score= and min_log_prob= is given, got neither"),
    ("count_above", "temperature with min_score", ValueError, "{cls}.count_above: temperature = 2.0 with min_score=: " + WITH_MIN_SCORE),
    ("count_above", "policy", NotImplementedError, "{cls}.count_above: one row of 70 logits exceeds MAX_LOGIT_BYTES; " + RANGE_WHOLE),
    ("range_search", "invalid_ids", ValueError, "range_search: invalid_ids must be (3, S) integer ids"),
    ("range_search", "temperature 0", ValueError, "{cls}.range_search: temperature must be a finite number > 0, got 0"),
    ("range_search", "both", ValueError, "{cls}.range_search: exactly one of min_score= and min_log_prob= is given, got both"),
    ("range_search", "neither", ValueError, "{cls}.range_search: exactly one of min_score= and min_log_prob= is given, got neither"),
    ("range_search", "temperature with min_score", ValueError, "{cls}.range_search: temperature = 2.0 with min_score=: " + WITH_MIN_SCORE),
    ("range_search", "policy", NotImplementedError, "{cls}.range_search: one row of 70 logits exceeds MAX_LOGIT_BYTES; " + RANGE_WHOLE),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def wrong_arguments(dev):
    """What is wrong -> the forms of it: each a dict of arguments that replace those of a valid call ("policy": MAX_LOGIT_BYTES one byte short)."""
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)      # noqa: E731
    return {
        "invalid_ids": [{"invalid_ids": t} for t in (z((B,), torch.int64), z((B - 1, 2), torch.int64), z((B, 2), torch.float32), z((B, 2), torch.bool))],
        "target_ids": [{"target_ids": t} for t in (z((B,), torch.int64), z((B + 1, 2), torch.int64), z((B, 2), torch.float32), z((B, 2), torch.bool))],
        "positions": [{"positions": t} for t in (z((B,), torch.int64), z((B + 1, 2), torch.int64), z((B, 2), torch.int32))],
        "temperature 0": [{"temperature": 0}],
        "temperature nan": [{"temperature": float("nan")}],
        "temperature tiny": [{"temperature": 1e-60}],
        "both": [{"min_score": 0.5, "min_log_prob": -3.0}],
        "neither": [{"min_score": None, "min_log_prob": None}],
        "temperature with min_score": [{"min_score": 0.5, "min_log_prob": None, "temperature": 2.0}],
        "num_samples 0": [{"num_samples": 0}],
        "num_samples 71": [{"num_samples": N + 1}],
        "seed -1": [{"seed": -1}],
        "seed 2^64": [{"seed": 1 << 64}],
        "policy": [{}],
    }


def run(tk, call, a):
    """One of the calls with its own arguments out of `a`"""
    q, inv, t, kw = a["q"], a["invalid_ids"], a["temperature"], a["kw"]
    if call == "rank_of":
        return tk.rank_of(q, a["target_ids"], inv, **kw)
    if call == "rank_of_positions":
        return tk.rank_of_positions(q, a["positions"], inv, **kw)
    if call == "log_partition":
        return tk.log_partition(q, inv, t, **kw)
    if call == "log_prob_of":
        return tk.log_prob_of(q, a["target_ids"], inv, t, **kw)
    if call == "log_prob_of_positions":
        return tk.log_prob_of_positions(q, a["positions"], inv, t, **kw)
    if call == "sample_items":
        return tk.sample_items(q, a["num_samples"], a["seed"], t, inv, **kw)
    range_kw = dict(min_log_prob=a["min_log_prob"], temperature=t, invalid_ids=inv, **kw)
    if call == "count_above":
        return tk.count_above(q, a["min_score"], **range_kw)
    return tk.range_search(q, a["min_score"], sort=a["sort"], **range_kw)


def module_and_arguments(module, route, dev):
    make, X, ids, q, aux = M.setup(module, route, dev, n=N)
    tk = make(X.unsqueeze(0), ids.unsqueeze(0))
    g = torch.Generator().manual_seed(91)
    keep = torch.zeros(N, dtype=torch.bool)
    keep[0] = True
    keep[1 + torch.randperm(N - 2, generator=g)[:39]] = True      # 40 of the 70: position 0 among them, position 69 not
    pos = torch.tensor([[0, 69], [31, 32], [64, 5]])
    seen = torch.stack([ids[torch.randint(0, N, (B,), generator=g).to(dev)], torch.full((B,), 2, dtype=torch.int64, device=dev)], dim=1)      # (ids are 3 * position + 1: nobody has 2)
    a = {"q": q[:B].contiguous(), "target_ids": ids[pos.to(dev)], "positions": pos.to(dev), "invalid_ids": seen.contiguous(), "temperature": 2.0,
         "num_samples": 5, "seed": 0x1234_5678_9ABC_DEF0, "min_score": None, "min_log_prob": -3.7, "sort": True,
         "kw": {key: v[:B].contiguous() for key, v in aux.items()}}
    return tk, a, E.ItemMask(keep.to(dev))


@pytest.mark.parametrize("module,route", MODULES)
def test_every_error_before_the_dense_pass_word_for_word(module, route, dev):
    tk, a, _ = module_and_arguments(module, route, dev)
    wrong = wrong_arguments(dev)
    assert {e[0] for e in ERRORS} == set(CALLS)
    for call, what, exc, message in ERRORS:
        if what == "policy":
            tk.MAX_LOGIT_BYTES = (2 if call == "sample_items" else 1) * N * 4 - 1
        for form in wrong[what]:
            with pytest.raises(exc) as e:
                run(tk, call, {**a, **form})
            assert type(e.value) is exc and str(e.value) == message.format(cls=type(tk).__name__), (call, what, form)
        if what == "policy":
            del tk.MAX_LOGIT_BYTES
    run(tk, "range_search", a)      # (the arguments the forms replace are those of valid calls)


def same(got, want, what):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want), what
    for j, (x, y) in enumerate(zip(got, want)):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, j)


@pytest.mark.parametrize("module,route", MODULES)
def test_a_sliced_batch_is_the_unsliced_batch(module, route, dev):
    """MAX_LOGIT_BYTES = 2 rows of logits: two slices, the second a single row (a one-row view of the recycled logits buffer); sample_items,
    with its two live matrices, goes row by row."""
    tk, a, mask = module_and_arguments(module, route, dev)
    a["kw"]["item_mask"] = mask
    per_row = run(tk, "range_search", a)
    assert per_row[0].shape == (B + 1,) and int(per_row[0][-1]) >= B, "the log-probability threshold keeps something of every row"
    mid = torch.stack([per_row[1][per_row[0][b] : per_row[0][b + 1]].median() for b in range(B)])      # a (B,) score threshold inside every row's hits
    cases = [(call, {}) for call in CALLS[:6]]
    for form in ({}, {"min_score": mid, "min_log_prob": None, "temperature": 1.0}):
        cases += [("count_above", form), ("range_search", {**form, "sort": True}), ("range_search", {**form, "sort": False})]
    whole = [run(tk, call, {**a, **form}) for call, form in cases]
    tk.MAX_LOGIT_BYTES = 2 * N * 4
    for (call, form), want in zip(cases, whole):
        same(run(tk, call, {**a, **form}), want, (module, call, sorted(form)))
    counts = whole[[c for c, _ in cases].index("count_above")]
    assert torch.equal(counts, per_row[0][1:] - per_row[0][:-1]) and int(whole[0].min()) == 0 and int(whole[0].max()) >= 1
    assert whole[5][0].shape == (B, 5) and bool((whole[5][0] >= 0).all())


def test_a_score_matrix_without_rows(dev):
    scores = torch.empty((0, N), dtype=torch.float32, device=dev)
    pos = torch.empty((0, 2), dtype=torch.int64, device=dev)
    mask = E.ItemMask(torch.ones(N, dtype=torch.bool, device=dev))
    for m in (None, mask):
        lse = E.scores_lse(scores, m, 2.0)
        out = {"rank": E.scores_rank(scores, pos, m), "lse": lse, "log_prob": E.scores_log_prob(scores, pos, lse, m, 2.0),
               "gumbel": E.scores_gumbel(scores, 7, 0, m, 2.0), "count": E.scores_range_count(scores, 0.0, m)}
        want = {"rank": ((0, 2), torch.int64), "lse": ((0,), torch.float32), "log_prob": ((0, 2), torch.float32), "gumbel": ((0, N), torch.float32),
                "count": ((0,), torch.int64)}
        for name, (shape, dtype) in want.items():
            assert tuple(out[name].shape) == shape and out[name].dtype == dtype and out[name].device == scores.device, name
    assert E.scores_mask(scores, mask) is scores
    torch.cuda.synchronize(dev)
