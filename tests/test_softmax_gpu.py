"""GPU: the softmax over the corpus.  The kernels of rails_amd/csrc/softmax.hip against tests/_softmax_ref.py -- the
log-partition within its derived bound and exactly on the special rows, the log-probability gather and the run-to-run results bit for bit, the
Gumbel perturbation within 4 ulp, independent of batch slice and alignment, and under a chi-square bar --; the contract of log_partition /
log_prob_of / sample_items on MoLBruteForceTopK (every exact_mode, precision and route) and MIPSBruteForceTopK; the eval harness's nll switch.
Inputs and helpers: those of tests/test_rank_gpu.py."""
import numpy as np
import pytest
import torch

import rails_amd
from rails_amd import engine as E
from tests import _softmax_ref as S
from tests import test_index_update_gpu as U
from tests import test_item_mask_gpu as M
from tests import test_rank_gpu as RK
from tests.test_index_update_gpu import B
from tests.test_item_mask_gpu import N, SIZES
from tests.test_rank_gpu import FAMILY_NAMES, ROUTES, ROWS
from tests.test_softmax_cpu import CHI2_BAR, FREQ_LOGITS, FREQ_ROWS, FREQ_SEED

pytestmark = pytest.mark.gpu
TEMPERATURES = (1.0, 0.5, 7.3)
NEG_INF = float("-inf")
assert {4_095, 4_096, 4_097} <= set(SIZES)      # one chunk of the streaming kernels and its neighbours


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def beta_of(temperature):
    return np.float32(1.0 / temperature)


def check_lse(got, bits, eligible, temperature, what):
    """Special rows exactly; finite rows within 2^-24 (3A + |ref| + 20), A = the row's largest eligible |x beta|: 3A for the exponent's
    argument (y's rounding, half an ulp of A, and the subtraction's, at most one), 4 for two ulp of expf, 15 for the 16-term fp32 chain, 1 for
    the float64 part, |ref| for the final rounding."""
    beta = beta_of(temperature)
    eligible = np.broadcast_to(eligible, bits.shape)
    ref = S.lse(bits, eligible, beta)
    mags = np.abs(S.floats(bits) * float(beta))
    kinds = set()
    for r in range(bits.shape[0]):
        if np.isnan(ref[r]):
            assert np.isnan(got[r]), f"{what}, row {r}: {got[r]} for a row with an eligible NaN"
            kinds.add("nan")
        elif np.isinf(ref[r]):
            assert got[r] == ref[r], f"{what}, row {r}: {got[r]} instead of {ref[r]}"
            kinds.add("+inf" if ref[r] > 0 else "-inf")
        else:
            a = mags[r][eligible[r]].max()
            err, bound = abs(float(got[r]) - ref[r]), 2.0 ** -24 * (3 * a + abs(ref[r]) + 20)
            assert err <= bound, f"{what}, row {r}: |{got[r]} - {ref[r]}| = {err} > {bound}"
            if eligible[r].sum() == 1:
                assert float(got[r]) == float(np.float32(S.floats(bits)[r][eligible[r]][0]) * beta), f"{what}, row {r}: one eligible entry"
            kinds.add("finite")
    return kinds


@pytest.mark.parametrize("extra_ld", [0, 5])
def test_scores_lse_against_the_reference(extra_ld, dev):
    rng = np.random.default_rng(60 + extra_ld)
    case, seen, kinds = 0, set(), set()
    for n in SIZES:
        for what, eligible, make_mask in RK.kernel_cases(n, rng):
            fam, temperature = FAMILY_NAMES[case % len(FAMILY_NAMES)], TEMPERATURES[(case // 2) % len(TEMPERATURES)]
            bits = RK.family_rows(fam, n, rng)
            scores = RK.on_device(bits, n + extra_ld, 3 if extra_ld else 0, dev)
            mask = make_mask(dev)
            got = E.scores_lse(scores, mask, temperature)
            assert got.dtype == torch.float32 and got.shape == (ROWS,)
            again = E.scores_lse(scores, mask, temperature)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two runs differ"
            kinds |= check_lse(got.cpu().numpy(), bits, eligible, temperature, f"n = {n}, ld = n + {extra_ld}, T = {temperature}, {fam}, {what}")
            seen.add((fam, temperature))
            case += 1
    assert {f for f, _ in seen} == set(FAMILY_NAMES) and {t for _, t in seen} == set(TEMPERATURES)
    assert kinds == {"nan", "+inf", "-inf", "finite"}


def test_scores_lse_special_rows_and_many_chunks(dev):
    """The special rows stated on their own, in a row of 74 chunks whose deciding entries sit in the head, the tail and a late chunk."""
    rng = np.random.default_rng(62)
    n = 300_007
    x = rng.standard_normal((8, n)).astype(np.float32) * 3
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    eligible = rng.random((8, n)) < 0.5
    x[0, n - 1], eligible[0, n - 1] = nan, True            # an eligible NaN in the tail
    x[0, 5], eligible[0, 5] = inf, True
    x[1, 250_000], eligible[1, 250_000] = inf, True        # +inf in a late chunk, a NaN outside the mask
    x[1, 0], eligible[1, 0] = nan, False
    x[2, eligible[2]] = -inf                               # -inf alone among the eligible
    eligible[3] = False                                    # nothing eligible
    eligible[4] = False
    eligible[4, 123_456] = True                            # one eligible finite entry
    x[5, ::7] = -inf                                       # eligible -inf entries add 0
    x[6, 0], eligible[6, 0] = 80.0, True                   # the head decides: every other term underflows against it
    bits = x.view(np.uint32)
    scores = RK.on_device(bits, n + 2, 1, dev)
    for temperature in TEMPERATURES:
        for mask in (E.ItemMask(torch.from_numpy(eligible).to(dev)),):
            got = E.scores_lse(scores, mask, temperature)
            assert torch.equal(got.view(torch.int32), E.scores_lse(scores, mask.words, temperature).view(torch.int32))
            got = got.cpu().numpy()
            check_lse(got, bits, eligible, temperature, f"T = {temperature}")
            beta = beta_of(temperature)
            assert np.isnan(got[0]) and got[1] == np.inf and got[2] == -np.inf and got[3] == -np.inf
            assert got[4] == x[4, 123_456] * beta
    # the bits do not depend on where a row starts (what lets a batch slice reproduce the unsliced call): other strides and alignments
    mask = E.ItemMask(torch.from_numpy(eligible).to(dev))
    for m in (mask, None):
        want = E.scores_lse(scores, m, 0.5).view(torch.int32)
        for ld, lead in ((n, 0), (n + 1, 0), (n + 5, 3), (n + 3, 2)):
            assert torch.equal(E.scores_lse(RK.on_device(bits, ld, lead, dev), m, 0.5).view(torch.int32), want), (ld, lead)
        assert torch.equal(E.scores_lse(scores[5:], None if m is None else m.words[5:], 0.5).view(torch.int32), want[5:])
    full = E.scores_lse(scores, None, 1.0).cpu().numpy()
    assert np.isnan(full[0]) and np.isnan(full[1]) and np.isfinite(full[2:]).all()
    check_lse(full, bits, np.ones((1, n), dtype=bool), 1.0, "no mask")


def test_scores_lse_more_rows_than_the_grid_has(dev):
    """65 537 rows of 3 columns: the grid-y loop, rows at every alignment."""
    rng = np.random.default_rng(63)
    rows, n = 65_537, 3
    x = rng.standard_normal((rows, n)).astype(np.float32) * 4
    eligible = rng.random((rows, n)) < 0.7
    scores = torch.from_numpy(x).to(dev)
    got = E.scores_lse(scores, E.ItemMask(torch.from_numpy(eligible).to(dev)), 0.5)
    kinds = check_lse(got.cpu().numpy(), x.view(np.uint32), eligible, 0.5, "65 537 rows")
    assert kinds == {"finite", "-inf"}
    assert torch.equal(got.view(torch.int32), E.scores_lse(scores, E.ItemMask(torch.from_numpy(eligible).to(dev)), 0.5).view(torch.int32))


def test_scores_log_prob_is_the_ieee_difference(dev):
    rng = np.random.default_rng(64)
    case = 0
    for n in SIZES:
        for what, eligible, make_mask in RK.kernel_cases(n, rng):
            fam, temperature = FAMILY_NAMES[case % len(FAMILY_NAMES)], TEMPERATURES[(case // 2) % len(TEMPERATURES)]
            t = (1, 2, 10, 70)[(case // 3) % 4]
            bits = RK.family_rows(fam, n, rng)
            targets = RK.targets_for(bits, eligible, t, case % 10, rng)      # 0, n - 1, 31, 32, a cleared position, -1, a repeat, ...
            scores = RK.on_device(bits, n + 5, 3, dev)
            mask = make_mask(dev)
            lse = E.scores_lse(scores, mask, temperature)
            got = E.scores_log_prob(scores, torch.from_numpy(targets).to(dev), lse, mask, temperature)
            assert got.dtype == torch.float32 and got.shape == (ROWS, t)
            x, lse_h, beta = bits.view(np.float32), lse.cpu().numpy(), beta_of(temperature)
            want = np.full((ROWS, t), -np.inf, dtype=np.float32)
            with np.errstate(invalid="ignore", over="ignore"):
                for r in range(ROWS):
                    for j, p in enumerate(targets[r]):
                        if 0 <= p < n and eligible[r, p]:
                            want[r, j] = np.float32(np.float32(x[r, p] * beta) - lse_h[r])
            assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), f"n = {n}, T = {temperature}, t = {t}, {fam}, {what}"
            case += 1
    with pytest.raises(ValueError, match="positions"):
        E.scores_log_prob(scores, torch.zeros((ROWS + 1, 1), dtype=torch.int64, device=dev), lse)
    with pytest.raises(ValueError, match="lse"):
        E.scores_log_prob(scores, torch.zeros((ROWS, 1), dtype=torch.int64, device=dev), lse[:2])
    with pytest.raises(ValueError, match="rows"):
        E.scores_lse(scores, E.ItemMask(torch.ones((ROWS + 1, scores.shape[1]), dtype=torch.bool, device=dev)))
    with pytest.raises(ValueError, match="mask of"):
        E.scores_lse(scores[:, :-1], E.ItemMask(torch.ones((ROWS, scores.shape[1]), dtype=torch.bool, device=dev)))
    with pytest.raises(ValueError, match="temperature"):
        E.scores_lse(scores, None, 0.0)


def ulp32(m):
    return np.spacing(np.abs(m).astype(np.float32)).astype(np.float64)


def check_gumbel(got, bits, eligible, temperature, seed, first_row, what):
    """Ineligible entries exactly -inf; eligible finite ones within 4 ulp of max(1, |g|, |value|) of the float64 reference: the inner logf's
    ulp becomes 2^-23 absolute through the outer log, the outer logf's is one of |g|, y and the add round by half an ulp each."""
    eligible = np.broadcast_to(eligible, bits.shape)
    ref = S.perturbed(bits, eligible, beta_of(temperature), seed, first_row)
    g = S.gumbel(seed, first_row + np.arange(bits.shape[0]), bits.shape[1])
    assert (got[~eligible] == -np.inf).all(), f"{what}: an ineligible entry is not -inf"
    fin = eligible & np.isfinite(ref)
    tol = 4 * ulp32(np.maximum(1.0, np.maximum(np.abs(g), np.abs(ref)))[fin])
    err = np.abs(got[fin].astype(np.float64) - ref[fin])
    assert (err <= tol).all(), f"{what}: {err.max()} against {tol[err.argmax()]}"
    rest = eligible & ~fin
    assert np.array_equal(got[rest].astype(np.float64), ref[rest], equal_nan=True), f"{what}: non-finite entries"


@pytest.mark.parametrize("extra_ld", [0, 5])
def test_scores_gumbel_against_the_reference(extra_ld, dev):
    rng = np.random.default_rng(66 + extra_ld)
    case = 0
    for n in SIZES:
        for what, eligible, make_mask in RK.kernel_cases(n, rng):
            fam, temperature = FAMILY_NAMES[case % len(FAMILY_NAMES)], TEMPERATURES[(case // 2) % len(TEMPERATURES)]
            seed = int(rng.integers(0, 1 << 63)) * 2 + case % 2
            first_row = (0, 7, (1 << 32) + 3)[case % 3]
            bits = RK.family_rows(fam, n, rng)
            scores = RK.on_device(bits, n + extra_ld, 3 if extra_ld else 0, dev)
            got = E.scores_gumbel(scores, seed, first_row, make_mask(dev), temperature)
            assert got.dtype == torch.float32 and got.shape == (ROWS, n) and got.data_ptr() != scores.data_ptr()
            check_gumbel(got.cpu().numpy(), bits, eligible, temperature, seed, first_row, f"n = {n}, ld = n + {extra_ld}, T = {temperature}, {fam}, {what}")
            case += 1


def test_scores_gumbel_noise_belongs_to_seed_row_and_position(dev):
    rng = np.random.default_rng(68)
    n, seed = 3 * 4096 + 37, 0xFEDCBA9876543210
    row = rng.standard_normal(n).astype(np.float32)
    bits = np.broadcast_to(row.view(np.uint32), (10, n)).copy()      # ten identical rows: whatever differs is the noise
    eligible = rng.random((10, n)) < 0.8
    mask = E.ItemMask(torch.from_numpy(eligible).to(dev))
    scores = RK.on_device(bits, n, 0, dev)
    whole = E.scores_gumbel(scores, seed, 0, mask, 0.5)
    as_int = lambda t: t.contiguous().view(torch.int32)      # noqa: E731
    # rows 5..9 of the 10-row call are a 5-row call with first_row = 5
    part = E.scores_gumbel(scores[5:], seed, 5, mask.words[5:], 0.5)
    assert torch.equal(as_int(part), as_int(whole[5:]))
    # another row stride and alignment of the input, a misaligned and strided output
    moved = RK.on_device(bits, n + 5, 3, dev)
    assert torch.equal(as_int(E.scores_gumbel(moved, seed, 0, mask, 0.5)), as_int(whole))
    for lead, ld in ((1, n + 3), (2, n), (0, n + 4)):
        buf = torch.full((lead + 10 * ld,), 7.0, dtype=torch.float32, device=dev)
        out = buf[lead:].as_strided((10, n), (ld, 1))
        assert E.scores_gumbel(moved, seed, 0, mask, 0.5, out=out).data_ptr() == out.data_ptr()
        assert torch.equal(as_int(out), as_int(whole)), (lead, ld)
        if ld > n:
            assert bool((buf.as_strided((9, ld - n), (ld, 1), lead + n) == 7.0).all()) and bool((buf[:lead] == 7.0).all()), "written outside the rows"
    # another seed, another row: other bits
    both = torch.from_numpy(eligible[0] & eligible[1]).to(dev)
    assert not torch.equal(as_int(whole[0][both]), as_int(whole[1][both]))
    other = E.scores_gumbel(scores, seed + 1, 0, mask, 0.5)
    assert not torch.equal(as_int(other), as_int(whole))
    assert torch.equal(torch.isinf(other) & (other < 0), torch.isinf(whole) & (whole < 0))
    with pytest.raises(ValueError, match="seed"):
        E.scores_gumbel(scores, 1 << 64)
    with pytest.raises(ValueError, match="seed"):
        E.scores_gumbel(scores, -1)
    with pytest.raises(ValueError, match="out must"):
        E.scores_gumbel(scores, 1, out=torch.empty((10, n + 1), device=dev))


@pytest.mark.parametrize("temperature", [1.0, 2.0])
def test_gumbel_argmax_frequencies(temperature, dev):
    """4 096 identical rows of 8 logits: the row argmax of the perturbed matrix is a draw from softmax(logits / T).  Pearson's chi-square of the
    counts stays below the 1e-4 upper quantile at 7 degrees of freedom (the float64 reference with this seed: 5.70 at T = 1, 4.94 at T = 2 --
    tests/test_softmax_cpu.py), and the device's argmax is the reference's wherever the reference's two best lie further apart than the noise
    tolerance of check_gumbel allows two entries to move."""
    logits = torch.tensor(FREQ_LOGITS, dtype=torch.float32)
    scores = logits.to(dev).repeat(FREQ_ROWS, 1)
    got = E.scores_gumbel(scores, FREQ_SEED, 0, None, temperature).cpu().numpy()
    arg = got.argmax(axis=1)
    y = logits.numpy().astype(np.float64) * float(beta_of(temperature))
    p = np.exp(y - y.max())
    expected = FREQ_ROWS * p / p.sum()
    assert expected.min() >= 38
    counts = np.bincount(arg, minlength=len(FREQ_LOGITS))
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print(f"T = {temperature}: chi-square {chi2:.3f}, counts {counts.tolist()}")
    assert chi2 < CHI2_BAR, (chi2, counts.tolist())
    _, _, ref_arg, gap = S.chi_square(FREQ_LOGITS, temperature, FREQ_SEED, FREQ_ROWS)
    ref = S.perturbed(np.broadcast_to(logits.numpy().view(np.uint32), got.shape), True, beta_of(temperature), FREQ_SEED)
    g = S.gumbel(FREQ_SEED, np.arange(FREQ_ROWS), len(FREQ_LOGITS))
    tol = 2 * 4 * ulp32(np.maximum(1.0, np.maximum(np.abs(g), np.abs(ref))).max(axis=1))
    clear = gap > tol
    assert clear.sum() >= FREQ_ROWS - 8 and np.array_equal(arg[clear], ref_arg[clear])


# ---- the module contract -----------------------------------------------------------------------------------------------------------------
def own_logits(tk, q, aux):
    """The module's own all_logits (MIPSBruteForceTopK: the score matrix its forward selects from), copied out of the recycled buffer"""
    return (tk.all_logits(q, **aux) if hasattr(tk, "all_logits") else tk._index.score(q)).clone()


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def restrictions(tk, ids, g, dev):
    """Hides a set, sets tags, -> [(what, call kwargs, eligible (B, N) bool on the CPU)]: the hidden set alone, per-row allowed_tags=, a ragged
    per-row item_mask=, the last with seen ids, seen ids alone."""
    hidden = torch.unique(torch.cat([torch.randperm(N, generator=g)[:5000], torch.tensor([0, 31, 32, N - 1])]))
    vis = torch.ones(N, dtype=torch.bool)
    vis[hidden] = False
    r200 = torch.zeros(N, dtype=torch.bool)
    r200[torch.randperm(N, generator=g)[:200]] = True
    three = [torch.ones(N, dtype=torch.bool), torch.rand(N, generator=g) < 0.5, r200]
    per_row = torch.stack([three[b % 3] for b in range(B)])
    tags = torch.randint(0, 8, (N,), generator=g)
    allowed = [(1, 2, 5)[b % 3] for b in range(B)]
    seen_pos = torch.stack([torch.randperm(N, generator=g)[:61] for _ in range(B)])
    seen_pos[:, 0] = torch.nonzero(r200 & vis)[0, 0]                  # (an item every row's mask keeps is seen by every row)
    seen = torch.cat([ids.cpu()[seen_pos], torch.tensor([[2, 5]]).expand(B, -1)], dim=1).to(dev).contiguous()      # ... and two ids nobody has
    gone = torch.ones((B, N), dtype=torch.bool)
    gone.scatter_(1, seen_pos, False)
    out = []
    tk.hide_items(hidden)
    tk.set_item_tags(tags.to(dev))
    out.append(("hidden set", {}, vis[None].expand(B, N)))
    out.append(("per-row allowed_tags", {"allowed_tags": allowed}, ((tags[None, :] & torch.tensor(allowed)[:, None]) != 0) & vis[None]))
    out.append(("ragged item_mask", {"item_mask": E.ItemMask(per_row.to(dev))}, per_row & vis[None]))
    out.append(("ragged item_mask and seen ids", {"item_mask": E.ItemMask(per_row.to(dev)), "invalid_ids": seen}, per_row & vis[None] & gone))
    out.append(("seen ids", {"invalid_ids": seen}, vis[None] & gone))
    return out, hidden, seen_pos


@pytest.mark.parametrize("module,route", ROUTES)
def test_log_partition_and_log_prob_of(module, route, dev):
    make, X, ids, q, aux = M.setup(module, route, dev)
    g = torch.Generator().manual_seed(71)
    with torch.inference_mode():
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        logits = own_logits(tk, q, aux)
        # the ids get_top_k_outputs returns: fl32(fl32(score beta) - log_partition), without and with seen ids
        cand = rails_amd.CandidateIndex(ids=ids.reshape(1, -1), embeddings=X.unsqueeze(0))
        top_ids, top_scores, _ = cand.get_top_k_outputs(q, 200, aux, tk, None)
        seen = top_ids[:, 5:66].contiguous()
        for temperature in (1.0, 7.3):
            beta = float(beta_of(temperature))
            part = tk.log_partition(q, temperature=temperature, **aux)
            assert part.dtype == torch.float32 and part.shape == (B,) and part.device == q.device
            assert bits_equal(part, E.scores_lse(logits, None, temperature)), f"{module} {route}: log_partition, T = {temperature}"
            got = tk.log_prob_of(q, top_ids, temperature=temperature, **aux)
            assert got.shape == (B, 200) and bits_equal(got, top_scores.float() * beta - part[:, None]), f"{module} {route}: log_prob_of forward's ids"
            f_ids, f_scores, _ = cand.get_top_k_outputs(q, 50, aux, tk, seen)
            part_f = tk.log_partition(q, invalid_ids=seen, temperature=temperature, **aux)
            assert bool((part_f < part).all())
            got = tk.log_prob_of(q, f_ids, invalid_ids=seen, temperature=temperature, **aux)
            assert bits_equal(got, f_scores.float() * beta - part_f[:, None]), f"{module} {route}: log_prob_of the filtered top-50"
            assert bool((tk.log_prob_of(q, seen, invalid_ids=seen, temperature=temperature, **aux) == NEG_INF).all())
        # by position, and an id nobody has
        pos = torch.randint(0, N, (B, 5), generator=g).to(dev)
        by_id = ids[pos].clone()
        want = tk.log_prob_of_positions(q, pos, **aux)
        assert bits_equal(tk.log_prob_of(q, by_id, **aux), want) and bool(torch.isfinite(want).all())
        by_id[:, 2] = 2                                                  # (ids are 3 * position + 1)
        want[:, 2] = NEG_INF
        assert bits_equal(tk.log_prob_of(q, by_id, **aux), want)
        outside = torch.tensor([[-1, N, N + 5]], device=dev).expand(B, -1).contiguous()
        assert bool((tk.log_prob_of_positions(q, outside, **aux) == NEG_INF).all())
        # what a row may return: log_partition is scores_lse of the module's own logits under the row's eligible set; other targets get -inf
        cases, hidden, seen_pos = restrictions(tk, ids, g, dev)
        for what, kw, eligible in cases:
            mask = E.ItemMask(eligible.contiguous().to(dev))
            for temperature in (1.0, 0.5):
                want = E.scores_lse(logits, mask, temperature)
                assert bits_equal(tk.log_partition(q, temperature=temperature, **kw, **aux), want), f"{module} {route}: {what}, T = {temperature}"
                got = tk.log_prob_of_positions(q, pos, temperature=temperature, **kw, **aux)
                assert bits_equal(got, E.scores_log_prob(logits, pos, want, mask, temperature)), f"{module} {route}: {what}, log_prob_of"
                assert bool((got[~eligible.to(dev).gather(1, pos)] == NEG_INF).all())
        assert bool((tk.log_prob_of(q, ids[hidden[:B * 3].to(dev)].view(B, 3), **aux) == NEG_INF).all()), "hidden targets"
        kw = cases[3][1]
        assert cases[3][0] == "ragged item_mask and seen ids"
        assert bool((tk.log_prob_of(q, ids[seen_pos[:, :2].to(dev)], **kw, **aux) == NEG_INF).all()), "seen targets"
        # three batch slices under the logit policy give the unsliced result; one row beyond it is refused by name
        whole = tk.log_prob_of_positions(q, pos, temperature=0.5, **kw, **aux)
        whole_part = tk.log_partition(q, temperature=0.5, **kw, **aux)
        tk.MAX_LOGIT_BYTES = 11 * N * 4
        assert bits_equal(tk.log_prob_of_positions(q, pos, temperature=0.5, **kw, **aux), whole), f"{module} {route}: sliced"
        assert bits_equal(tk.log_partition(q, temperature=0.5, **kw, **aux), whole_part), f"{module} {route}: sliced"
        tk.MAX_LOGIT_BYTES = N * 4 - 1
        with pytest.raises(NotImplementedError, match=type(tk).__name__ + r"\.log_partition: one row"):
            tk.log_partition(q, **aux)
        tk.MAX_LOGIT_BYTES = 2 * N * 4 - 1
        with pytest.raises(NotImplementedError, match=type(tk).__name__ + r"\.sample_items: two rows"):
            tk.sample_items(q, 5, 1, **aux)


@pytest.mark.parametrize("module,route", ROUTES)
def test_probabilities_of_a_small_corpus_sum_to_one(module, route, dev):
    make, X, ids, q, aux = M.setup(module, route, dev, n=300)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        everyone = ids.view(1, -1).expand(B, -1).contiguous()
        for temperature in (1.0, 0.5):
            lp = tk.log_prob_of(q, everyone, temperature=temperature, **aux)
            total = torch.exp(lp.double()).sum(dim=1)
            assert bool(((total - 1).abs() <= 300 * 2.0 ** -23).all()), f"{module} {route}: T = {temperature}: {(total - 1).abs().max().item()}"
        seen = ids[:61].view(1, -1).expand(B, -1).contiguous()
        lp = tk.log_prob_of(q, everyone, invalid_ids=seen, **aux)
        assert bool((lp[:, :61] == NEG_INF).all()) and bool(((torch.exp(lp.double()).sum(dim=1) - 1).abs() <= 300 * 2.0 ** -23).all())


@pytest.mark.parametrize("module,route", ROUTES)
def test_sample_items(module, route, dev):
    make, X, ids, q, aux = M.setup(module, route, dev)
    g = torch.Generator().manual_seed(73)
    seed = 0x0123456789ABCDEF
    with torch.inference_mode():
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        logits = own_logits(tk, q, aux)
        # (a) what it is: the exact top-k of the perturbed matrix, with the clean matrix's log-probabilities
        got_ids, got_lp = tk.sample_items(q, 120, seed, temperature=0.5, **aux)
        assert got_ids.dtype == torch.int64 and got_ids.shape == (B, 120) and got_lp.dtype == torch.float32 and got_lp.shape == (B, 120)
        top, pos = E.topk(E.scores_gumbel(logits, seed, 0, None, 0.5), 120)
        assert torch.equal(got_ids, ids[pos]) and bool(torch.isfinite(top).all()), f"{module} {route}: ids"
        assert bits_equal(got_lp, tk.log_prob_of(q, got_ids, temperature=0.5, **aux)), f"{module} {route}: log_probs"
        assert all(len(set(row)) == 120 for row in got_ids.tolist()), "an item drawn twice"
        again = tk.sample_items(q, 120, seed, temperature=0.5, **aux)
        assert torch.equal(again[0], got_ids) and bits_equal(again[1], got_lp), f"{module} {route}: two calls"
        assert not torch.equal(tk.sample_items(q, 120, seed + 1, temperature=0.5, **aux)[0], got_ids)
        # (b) rows that may return 200 and 260 items, some of them hidden or seen: a permutation of exactly those, then (-1, -inf)
        keep = [torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)]
        keep[0][torch.randperm(N, generator=g)[:200]] = True
        keep[1][torch.randperm(N, generator=g)[:260]] = True
        per_row = torch.stack([keep[b % 2] for b in range(B)])
        hidden = torch.cat([torch.nonzero(keep[0])[:7, 0], torch.nonzero(keep[1])[:9, 0], torch.tensor([0, N - 1])])
        tk.hide_items(hidden)
        seen_pos = torch.stack([torch.nonzero(per_row[b])[20:25, 0] for b in range(B)])
        seen = torch.cat([ids.cpu()[seen_pos], torch.tensor([[2]]).expand(B, -1)], dim=1).to(dev).contiguous()
        eligible = per_row.clone()
        eligible[:, hidden] = False
        eligible.scatter_(1, seen_pos, False)
        kw = {"item_mask": E.ItemMask(per_row.to(dev)), "invalid_ids": seen}
        s_ids, s_lp = tk.sample_items(q, 260, seed, **kw, **aux)
        for b in range(B):
            want = ids.cpu()[eligible[b]]
            c = want.numel()
            assert c < 260 and torch.equal(torch.sort(s_ids[b, :c].cpu())[0], want), f"{module} {route}: row {b}"
            assert bool((s_ids[b, c:] == -1).all()) and bool((s_lp[b, c:] == NEG_INF).all()) and bool(torch.isfinite(s_lp[b, :c]).all())
        assert bits_equal(s_lp, tk.log_prob_of(q, s_ids, **kw, **aux))
        mask = E.ItemMask(eligible.to(dev))
        top, pos = E.topk(E.scores_gumbel(logits, seed, 0, mask, 1.0), 260)
        assert torch.equal(s_ids, torch.where(top != NEG_INF, ids[pos], -1))
        # (c) three batch slices under the logit policy (two matrices per slice) give the unsliced result
        tk.MAX_LOGIT_BYTES = 2 * 11 * N * 4
        sliced = tk.sample_items(q, 260, seed, **kw, **aux)
        assert torch.equal(sliced[0], s_ids) and bits_equal(sliced[1], s_lp), f"{module} {route}: sliced"


@pytest.mark.parametrize("module,route", ROUTES)
def test_softmax_calls_after_corpus_edits(module, route, dev):
    """update_items / append_items / remove_items, with the id map live: the answers of a module freshly built from the resulting corpus."""
    from tests import test_index_remove_gpu as RM

    make, X, ids, q, aux = M.setup(module, route, dev)
    cfg = U.O.CONFIGS["amzn-books"] if module == "mips" else U.setup_route(module, route, dev)[0]
    g = torch.Generator().manual_seed(74)
    with torch.inference_mode():
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        top = tk(q, k=10, **aux)[1]
        target_ids = torch.cat([top[:, :3], ids[torch.randint(0, N, (B, 3), generator=g).to(dev)], torch.tensor([[-7, -8]], device=dev).expand(B, -1)], dim=1).contiguous()
        first = tk.log_prob_of(q, target_ids, **aux)                      # (the id map exists from here on)
        assert bool(torch.isfinite(first[:, :6]).all()) and bool((first[:, 6:] == NEG_INF).all())
        X2, ids2 = X.clone(), ids.clone()
        upd = U.positions_for(N, g)
        rows = U.table(cfg, upd.numel(), 31, dev, first=20_000_000)
        tk.update_items(upd, rows)
        X2[upd.to(dev)] = rows
        extra = U.table(cfg, 70, 32, dev, first=30_000_000)
        extra[:2] = X[((top[:2, 0] - 1) // 3)]
        new_ids = torch.tensor(list(range(-7, -77, -1)), device=dev)
        tk.append_items(extra, new_ids)
        X2, ids2 = torch.cat([X2, extra]), torch.cat([ids2, new_ids])
        gone = RM.removal_set(N + 70, g, must=((top[:4, 1] - 1) // 3).cpu())
        tk.remove_items(gone)
        X2, ids2, _ = RM.after_removal(X2, ids2, gone)
        fresh = make(X2.clone().unsqueeze(0), ids2.clone().unsqueeze(0))
        seen = top[:, 3:9].contiguous()
        for kw in ({}, {"invalid_ids": seen}):
            assert bits_equal(tk.log_partition(q, temperature=0.5, **kw, **aux), fresh.log_partition(q, temperature=0.5, **kw, **aux)), f"{module} {route}: {sorted(kw)}"
            got, want = tk.log_prob_of(q, target_ids, **kw, **aux), fresh.log_prob_of(q, target_ids, **kw, **aux)
            assert bits_equal(got, want), f"{module} {route}: log_prob_of after the edits {sorted(kw)}"
            got, want = tk.sample_items(q, 50, 99, **kw, **aux), fresh.sample_items(q, 50, 99, **kw, **aux)
            assert torch.equal(got[0], want[0]) and bits_equal(got[1], want[1]), f"{module} {route}: sample_items after the edits {sorted(kw)}"
        got = tk.log_prob_of(q, target_ids, **aux)
        assert not bits_equal(got, first) and bool((got[:4, 1] == NEG_INF).all()) and bool(torch.isfinite(got[:, 6:]).all())      # (removed / appended)


def test_refusals(dev):
    """By name, before any launch: the approximate modules, collapse_groups=True, malformed arguments."""
    cfg, mol, make, aux = U.setup_route("brute", "default", dev)
    n = 20_000
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 16, dev), U.ids_of(n, dev)
        q = U.O.synthetic_queries(cfg, B, seed=11).to(dev)
        t = ids[:B].reshape(B, 1).contiguous()
        others = {"avg": U.MAKERS["avg"](mol, X.unsqueeze(0), ids.unsqueeze(0)), "naive": U.MAKERS["naive"](mol, X.unsqueeze(0), ids.unsqueeze(0)),
                  "comb": U.MAKERS["comb"](mol, X.unsqueeze(0), ids.unsqueeze(0)),
                  "ivf": rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), k_per_group=5, use_faiss=True)}
        for name, other in others.items():
            cls = type(other).__name__
            with pytest.raises(NotImplementedError, match=cls + r"\.log_partition.*MoLBruteForceTopK"):
                other.log_partition(q)
            with pytest.raises(NotImplementedError, match=cls + r"\.log_prob_of.*MoLBruteForceTopK"):
                other.log_prob_of(q, t)
            with pytest.raises(NotImplementedError, match=cls + r"\.log_prob_of_positions.*MoLBruteForceTopK"):
                other.log_prob_of_positions(q, t)
            with pytest.raises(NotImplementedError, match=cls + r"\.sample_items.*MoLBruteForceTopK"):
                other.sample_items(q, 5, 1)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        calls = {"log_partition": lambda **kw: tk.log_partition(q, **kw), "log_prob_of": lambda **kw: tk.log_prob_of(q, t, **kw),
                 "log_prob_of_positions": lambda **kw: tk.log_prob_of_positions(q, t, **kw), "sample_items": lambda **kw: tk.sample_items(q, 5, 1, **kw)}
        for name, call in calls.items():
            with pytest.raises(NotImplementedError, match=rf"MoLBruteForceTopK\.{name} takes no collapse_groups"):
                call(collapse_groups=True)
            for temperature in (0.0, -1.0, float("inf"), float("nan")):
                with pytest.raises(ValueError, match="temperature"):
                    call(temperature=temperature)
            with pytest.raises(ValueError, match="invalid_ids"):
                call(invalid_ids=t[:5])
            with pytest.raises(ValueError, match="invalid_ids"):
                call(invalid_ids=t.float())
        for num in (0, -1, n + 1, 2.0):
            with pytest.raises(ValueError, match="num_samples"):
                tk.sample_items(q, num, 1)
        for seed in (-1, 1 << 64, 1.0):
            with pytest.raises(ValueError, match="seed"):
                tk.sample_items(q, 5, seed)
        for wrong in (t[:5], t.reshape(-1), t.float()):
            with pytest.raises(ValueError, match="target_ids"):
                tk.log_prob_of(q, wrong)
        with pytest.raises(ValueError, match="positions"):
            tk.log_prob_of_positions(q, t.to(torch.int32))
        with pytest.raises(ValueError, match="rows"):
            tk.log_partition(q, item_mask=torch.ones((5, n), dtype=torch.bool, device=dev))
        ok_ids, ok_lp = tk.sample_items(q, 1000, (1 << 64) - 1)           # the largest seed
        assert all(len(set(row)) == 1000 for row in ok_ids.tolist()) and bool(torch.isfinite(ok_lp).all())


# ---- the eval harness ------------------------------------------------------------------------------------------------------------------
def test_eval_harness_nll(dev):
    from rails_amd import eval_harness as H
    from tests.test_gpu_parity import Fixture, build_module

    fx = Fixture("harness")
    mol = build_module(fx.cfg, fx.weights, dev)
    q = fx.t("q").to(dev)

    class StubEncoder:                       # the query encoder is upstream of the path: replay its output
        def encode(self, **kw):
            return q

        def get_item_embeddings(self, item_ids):
            return None

    model = StubEncoder()
    n_big = 3_000                             # beyond MAX_K + 61 items: the seen ids leave the rows' eligible sets
    Xb, idb = U.table(fx.cfg, n_big, 9, dev).unsqueeze(0), U.ids_of(n_big, dev).unsqueeze(0)
    tk = rails_amd.MoLBruteForceTopK(mol, Xb, idb)
    big = H.EvalState(all_item_ids=set(idb.view(-1).tolist()), candidate_index=rails_amd.CandidateIndex(ids=idb, embeddings=Xb), top_k_module=tk)
    with torch.inference_mode():
        _, top = tk(q, k=300)
    rows = torch.arange(q.shape[0], device=dev)
    past = top[:, 3:125:2].contiguous()
    at = torch.tensor([0, 1, 4, 9, 10, 49, 50, 99, 100, 119, 150, 250, 299, 7, 30, 75], device=dev)[: q.shape[0]]
    target = top[rows, at].unsqueeze(1).contiguous()
    feats = H.SequentialFeatures(past_lengths=torch.full((q.shape[0],), 61, device=dev), past_ids=past, past_embeddings=None, past_payloads={})
    for exact in (False, True):
        for filt in (True, False):
            plain = H.eval_metrics_v2_from_tensors(big, model, feats, target_ids=target, filter_invalid_ids=filt, exact_ranks=exact)
            for batch in (None, 7):
                with_nll = H.eval_metrics_v2_from_tensors(big, model, feats, target_ids=target, filter_invalid_ids=filt, exact_ranks=exact, nll=True,
                                                          user_max_batch_size=batch)
                assert set(with_nll) == set(plain) | {"nll"}
                for key in plain:
                    assert torch.equal(with_nll[key], plain[key]), key
                want = -tk.log_prob_of(q, target, invalid_ids=past if filt else None)[:, 0]
                assert bits_equal(with_nll["nll"], want), (exact, filt, batch)
                seen_target = (past == target).any(dim=1)
                assert bool(seen_target.any()) and bool((with_nll["nll"][seen_target] == float("inf")).all() if filt else torch.isfinite(with_nll["nll"]).all())
                assert bool(torch.isfinite(with_nll["nll"][~seen_target]).all()) and bool((with_nll["nll"][~seen_target] > 0).all())
    state = H.EvalState(all_item_ids=big.all_item_ids, candidate_index=big.candidate_index, top_k_module=rails_amd.MoLAvgTopK(mol, Xb, idb, avg_top_k=100))
    with pytest.raises(NotImplementedError, match=r"MoLAvgTopK\.log_prob_of"):
        H.eval_metrics_v2_from_tensors(state, model, feats, target_ids=target, nll=True)
