"""GPU: the range search.  The kernels of rails_amd/csrc/range.hip against tests/_range_ref.py and the contract of
count_above / range_search on MoLBruteForceTopK (every exact_mode, precision and route) and MIPSBruteForceTopK.  Every comparison is exact:
np.array_equal / torch.equal on bit patterns, positions and ids.  Inputs and helpers: those of tests/test_rank_gpu.py."""
import numpy as np
import pytest
import torch

import rails_amd
from rails_amd import engine as E
from tests import _range_ref as G
from tests import _topk_ref as R
from tests import test_index_update_gpu as U
from tests import test_item_mask_gpu as M
from tests.test_index_update_gpu import B
from tests.test_rank_gpu import PAD_BITS, ROUTES, family_rows, logit_bits
from tests.test_range_cpu import CAP_N, cap_fixture

pytestmark = pytest.mark.gpu
ROWS = 3
SHAPES = (1, 2, 3, 5, 31, 33, 255, 257, 4_095, 4_096, 4_097, 4_099, 8_193, 70_001, 300_007)
FAMILY_NAMES = ("gauss", "constant", "signed_zeros", "nans", "infs", "subnormals")
MASKS = ("none", "shared", "ragged", "empty row")
FORMS = ("scalar", "per row", "-inf", "+inf", "nan")
NM = 6_007          # items of the module tests
INF_BITS = 0x7F800000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def on_device(bits, ld, lead, dev, pad=PAD_BITS):
    """The rows as an (rows, n) fp32 view with row stride ld whose first element sits `lead` elements past an aligned address; `pad` lies
    between the rows"""
    rows, n = bits.shape
    buf = np.full(lead + rows * ld + 8, pad, dtype=np.uint32)
    for r in range(rows):
        buf[lead + r * ld : lead + r * ld + n] = bits[r]
    flat = torch.from_numpy(buf.view(np.int32)).to(dev).view(torch.float32)
    return flat[lead:].as_strided((rows, n), (ld, 1))


def make_mask(kind, rows, n, rng, dev):
    """-> (eligible (rows, n) bool, the engine's mask argument)"""
    if kind == "none":
        return np.ones((rows, n), dtype=bool), None
    if kind == "shared":
        m = rng.random((1, n)) < 0.5
        return np.broadcast_to(m, (rows, n)), E.ItemMask(torch.from_numpy(m[0]).to(dev))
    m = np.stack([np.ones(n, dtype=bool) if r % 3 == 0 else rng.random(n) < (0.5 if r % 3 == 1 else 0.01) for r in range(rows)])
    if kind == "empty row":
        m[1 % rows] = False
    return m, E.ItemMask(torch.from_numpy(m).to(dev))


def quantile_threshold(values_row, eligible_row, want):
    """the want-th largest non-NaN eligible value (the smallest if there are fewer; 0 without any)"""
    v = values_row[eligible_row & ~np.isnan(values_row)]
    return np.float32(0.0) if v.size == 0 else np.sort(v)[::-1][min(want, v.size) - 1]


def make_thresholds(form, values, eligible, want, dev):
    """-> (what the reference takes, what the engine takes)"""
    rows = values.shape[0]
    if form == "scalar":
        t = float(quantile_threshold(values[0], eligible[0], want))
        return t, t
    if form == "per row":
        t = np.array([quantile_threshold(values[r], eligible[r], want + 7 * r) for r in range(rows)], dtype=np.float32)
        return t, torch.from_numpy(t).to(dev)
    t = {"-inf": float("-inf"), "+inf": float("inf"), "nan": float("nan")}[form]
    return t, t


def check_against_reference(scores, bits, eligible, mask, t_ref, t_arg, what, ids=None, beta=None, temperature=1.0, lse=None):
    """scores_range_count and scores_range, sorted and unsorted, against the reference; -> the largest count"""
    rows = bits.shape[0]
    lse_np = None if lse is None else lse.cpu().numpy()
    want_counts = G.counts(bits, eligible, t_ref, beta, lse_np)
    got = E.scores_range_count(scores, t_arg, mask, temperature, lse)
    assert got.dtype == torch.int64 and got.shape == (rows,) and np.array_equal(got.cpu().numpy(), want_counts), f"{what}: counts"
    for sort in (True, False):
        if sort and want_counts.max(initial=0) > E.RANGE_SORT_MAX:
            with pytest.raises(ValueError, match=rf"row {int(want_counts.argmax())} has {int(want_counts.max())} hits.*sort=False"):
                E.scores_range(scores, t_arg, mask, temperature, lse, ids=ids, sort=True)
            continue
        lims, s, i = E.scores_range(scores, t_arg, mask, temperature, lse, ids=ids, sort=sort)
        w_lims, w_s, w_i = G.ragged(bits, eligible, t_ref, beta, lse_np, sort=sort, ids=None if ids is None else ids.cpu().numpy())
        assert lims.dtype == torch.int64 and s.dtype == torch.float32 and i.dtype == torch.int64 and lims.device == s.device == i.device == scores.device
        assert np.array_equal(lims.cpu().numpy(), w_lims), f"{what}, sort={sort}: lims"
        assert np.array_equal(i.cpu().numpy(), w_i), f"{what}, sort={sort}: ids"
        assert np.array_equal(s.view(torch.int32).cpu().numpy().view(np.uint32), w_s), f"{what}, sort={sort}: score bits"
    return int(want_counts.max(initial=0))


# ---- the engine ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_ld", [0, 5])
def test_scores_range_against_the_reference(extra_ld, dev):
    """Every shape with both strides (ld = n + 5 behind a lead of 3 elements: the three rows start at three alignments), the families, masks and
    threshold forms rotating over the cases so that each occurs with small and large rows."""
    rng = np.random.default_rng(70 + extra_ld)
    case, seen = 0, set()
    for n in SHAPES:
        for rep in range(4):
            fam, kind, form = FAMILY_NAMES[case % len(FAMILY_NAMES)], MASKS[(case // 2) % len(MASKS)], FORMS[(case // 3) % len(FORMS)]
            if n > 8_193 and rep < 2:      # the long rows: many chunks, a few thousand hits that are sorted
                fam, kind, form = (("gauss", "ragged", "per row"), ("nans", "shared", "scalar"))[rep]
            bits = family_rows(fam, n, rng)
            eligible, mask = make_mask(kind, ROWS, n, rng, dev)
            values = bits.view(np.float32)
            t_ref, t_arg = make_thresholds(form, values, eligible, max(1, min(n // 3, 3_000)), dev)
            if fam == "signed_zeros" and form == "scalar":
                t_ref = t_arg = (0.0, -0.0)[rep % 2]
            if fam == "constant" and form in ("scalar", "per row"):      # an all-tie row with t equal to the value: every eligible item is a hit
                t_ref = t_arg = float(values[0, 0])
                if form == "per row":
                    t_ref = np.full(ROWS, values[0, 0], dtype=np.float32)
                    t_arg = torch.from_numpy(t_ref).to(dev)
            scores = on_device(bits, n + extra_ld, 3 if extra_ld else 0, dev)
            check_against_reference(scores, bits, eligible, mask, t_ref, t_arg, f"n = {n}, ld = n + {extra_ld}, {fam}, mask {kind}, t {form}")
            seen.add((fam, kind, form))
            case += 1
    assert {f for f, _, _ in seen} == set(FAMILY_NAMES) and {k for _, k, _ in seen} == set(MASKS) and {f for _, _, f in seen} == set(FORMS)


@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_signed_zeros_pass_either_zero_and_rank_by_their_bits(zero, dev):
    """-0 >= +0 and +0 >= -0 hold, so both zeros are hits under either threshold; in the sorted row every +0 stands before every -0."""
    rng = np.random.default_rng(71)
    for n in (33, 4_099, 8_193):
        bits = np.stack([R.signed_zeros(n, max(2, n // 2), rng) for _ in range(ROWS)])
        eligible, mask = make_mask("ragged", ROWS, n, rng, dev)
        scores = on_device(bits, n + 5, 3, dev)
        check_against_reference(scores, bits, eligible, mask, zero, zero, f"n = {n}, t = {zero!r}")
        lims, s, _ = E.scores_range(scores, zero)
        row = s[: int(lims[1])].view(torch.int32).cpu().numpy().view(np.uint32)
        plus, minus = np.flatnonzero(row == 0), np.flatnonzero(row == 0x80000000)
        assert plus.size and minus.size and plus.max() < minus.min() and minus.max() == row.size - 1


def test_scores_range_many_rows(dev):
    """65 537 rows of 37 columns: the grid-y loop of the walks and an offset scan of 196 611 cells, many passes of one workgroup."""
    rng = np.random.default_rng(72)
    rows, n = 65_537, 37
    bits = rng.standard_normal((rows, n)).astype(np.float32).view(np.uint32)
    eligible = rng.random((rows, n)) < 0.8
    t = (rng.standard_normal(rows) * 0.5).astype(np.float32)
    t[::1000] = np.float32("-inf")
    t[7::1000] = np.float32("nan")
    hits = G.hit_mask(bits, eligible, t)
    r_idx, pos = np.nonzero(hits)                                    # (row-major: position order inside every row)
    w_lims = np.concatenate([[0], np.cumsum(hits.sum(axis=1))]).astype(np.int64)
    kv = (R.orderable(bits[r_idx, pos]).astype(np.uint64) << np.uint64(32)) | (~pos.astype(np.uint32)).astype(np.uint64)
    by_key = np.lexsort((~kv, r_idx))                                # rows ascending, keys descending inside a row
    scores = on_device(bits, n + 1, 1, dev)
    mask = E.ItemMask(torch.from_numpy(eligible).to(dev))
    t_dev = torch.from_numpy(t).to(dev)
    assert np.array_equal(E.scores_range_count(scores, t_dev, mask).cpu().numpy(), np.diff(w_lims))
    for sort, order in ((False, np.arange(pos.size)), (True, by_key)):
        lims, s, i = E.scores_range(scores, t_dev, mask, sort=sort)
        assert np.array_equal(lims.cpu().numpy(), w_lims) and np.array_equal(i.cpu().numpy(), pos[order]), sort
        assert np.array_equal(s.view(torch.int32).cpu().numpy().view(np.uint32), bits[r_idx, pos][order]), sort


@pytest.mark.parametrize("place", ["head", "tail", "chunk edge"])
def test_hits_in_the_peeled_columns_stand_in_position_order(place, dev):
    """Hits only in a row's first three columns (the unaligned head), only in its last three (the unaligned tail, which the walk visits on
    chunk 0 but which closes the row), or only at columns 4 095 / 4 096 of a misaligned row: position order and the slots' offsets."""
    rng = np.random.default_rng(73)
    n = 3 * 4_096 + 38
    cols = {"head": [0, 1, 2], "tail": [n - 3, n - 2, n - 1], "chunk edge": [4_095, 4_096]}[place]
    for lead in range(4):
        bits = np.stack([R.all_negative(n, 1, rng) for _ in range(ROWS)])
        for r in range(ROWS):
            bits[r, cols] = np.array([2.0 + r, 3.0, 2.5], dtype=np.float32).view(np.uint32)[: len(cols)]
        scores = on_device(bits, n + 5, lead, dev)
        check_against_reference(scores, bits, np.ones((ROWS, n), dtype=bool), None, 1.0, 1.0, f"{place}, lead {lead}")
        eligible, mask = make_mask("ragged", ROWS, n, rng, dev)
        check_against_reference(scores, bits, eligible, mask, 1.0, 1.0, f"{place}, lead {lead}, masked")
        lims = E.scores_range(scores, 1.0, None, sort=False)[0]
        assert lims.tolist() == [len(cols) * r for r in range(ROWS + 1)]


def test_count_tiers_of_the_sort(dev):
    """Rows of 0, 1, 2, 1 023, 1 024, 1 025, 2 048, 2 049 and exactly 16 384 hits, mixed inside one call (the launch's LDS is sized by the largest
    row; a row of up to 1 024 keys takes the exchange buffer); each sorted row also against the selection kernels: E.topk with k = its count."""
    rng = np.random.default_rng(74)
    for tiers in ((0, 1, 2), (1_023, 1_024, 1_025), (2_048, 2_049, 16_384), (1_024, 2_048, 5), (4_097, 8_192, 8_193)):
        bits = np.stack([R.gauss(CAP_N, c, rng) for c in tiers])
        keep = rng.random(CAP_N) < 0.9                                  # (about 18 000 eligible items: the largest tier fits)
        eligible, mask = np.broadcast_to(keep, (ROWS, CAP_N)), E.ItemMask(torch.from_numpy(keep).to(dev))
        t = np.array([G.threshold_for(bits[r], eligible[r], c) for r, c in enumerate(tiers)], dtype=np.float32)
        scores = on_device(bits, CAP_N + 5, 2, dev)
        t_dev = torch.from_numpy(t).to(dev)
        assert check_against_reference(scores, bits, eligible, mask, t, t_dev, f"tiers {tiers}") == max(tiers)
        lims, s, i = E.scores_range(scores, t_dev, mask)
        assert lims.tolist() == np.concatenate([[0], np.cumsum(tiers)]).tolist()
        masked = torch.where(torch.from_numpy(keep).to(dev), scores, torch.tensor(float("-inf"), device=dev)).contiguous()
        for r, c in enumerate(tiers):
            if c:
                top_s, top_p = E.topk(masked[r : r + 1], c)
                a, b = int(lims[r]), int(lims[r + 1])
                assert torch.equal(top_p[0], i[a:b]) and torch.equal(top_s[0].view(torch.int32), s[a:b].view(torch.int32)), (tiers, r)


def test_the_cap_of_a_sorted_row(dev):
    bits, t = cap_fixture(E.RANGE_SORT_MAX)
    scores = on_device(bits, CAP_N, 0, dev)
    assert check_against_reference(scores, bits, np.ones((1, CAP_N), dtype=bool), None, float(t), float(t), "exactly the cap") == E.RANGE_SORT_MAX
    bits, t = cap_fixture(E.RANGE_SORT_MAX + 1)
    two = np.concatenate([R.gauss(CAP_N, 5, np.random.default_rng(75))[None], bits])      # row 1 is the one beyond the cap
    scores = on_device(two, CAP_N + 1, 0, dev)
    t_dev = torch.tensor([float("inf"), float(t)], device=dev)
    with pytest.raises(ValueError, match=rf"row 1 has {E.RANGE_SORT_MAX + 1} hits.*sort=False"):
        E.scores_range(scores, t_dev)
    assert check_against_reference(scores, two, np.ones((2, CAP_N), dtype=bool), None, t_dev.cpu().numpy(), t_dev, "one beyond the cap") == E.RANGE_SORT_MAX + 1
    assert E.scores_range_count(scores, t_dev).tolist() == [0, E.RANGE_SORT_MAX + 1]


def test_output_does_not_depend_on_the_alignment(dev):
    """The same rows behind every lead offset, +inf between the rows (a padding element read by mistake would be a hit): equal output."""
    rng = np.random.default_rng(76)
    for n in (5, 4_097, 12_301):
        bits = family_rows("nans", n, rng)
        eligible, _ = make_mask("ragged", ROWS, n, rng, dev)
        t = np.array([quantile_threshold(bits[r].view(np.float32), eligible[r], n // 4 + 1) for r in range(ROWS)], dtype=np.float32)
        t_dev = torch.from_numpy(t).to(dev)
        outs = []
        for lead in range(4):
            scores = on_device(bits, n + 5 + lead, lead, dev, pad=INF_BITS)
            mask = E.ItemMask(torch.from_numpy(eligible).to(dev))
            outs.append([o.cpu() for sort in (True, False) for o in E.scores_range(scores, t_dev, mask, sort=sort)] + [E.scores_range_count(scores, t_dev, mask).cpu()])
        for other in outs[1:]:
            assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                       for a, b in zip(outs[0], other)), n
        w_lims, _, w_i = G.ragged(bits, eligible, t)
        assert np.array_equal(outs[0][0].numpy(), w_lims) and np.array_equal(outs[0][2].numpy(), w_i)


def test_log_probability_form_against_the_reference(dev):
    """v = fl32(fl32(s * beta) - lse) on the lse bits scores_lse gives, special rows included: a row with nothing eligible (lse = -inf), a row
    with an eligible NaN (lse = NaN: no hit), a row with an eligible +inf (lse = +inf)."""
    rng = np.random.default_rng(77)
    for n in (5, 4_097, 70_001):
        for temperature in (1.0, 2.0):
            bits = np.stack([R.gauss(n, 1, rng) for _ in range(5)])
            bits[3, n // 2] = 0x7FC00000
            bits[4, n - 1] = INF_BITS
            eligible = np.stack([np.ones(n, dtype=bool), rng.random(n) < 0.5, np.zeros(n, dtype=bool), np.ones(n, dtype=bool), np.ones(n, dtype=bool)])
            mask = E.ItemMask(torch.from_numpy(eligible).to(dev))
            scores = on_device(bits, n + 5, 1, dev)
            lse = E.scores_lse(scores, mask, temperature)
            beta = np.float32(E.inv_temperature(temperature))
            assert lse[2].item() == float("-inf") and np.isnan(lse[3].item()) and lse[4].item() == float("inf")
            v = G.values(bits, beta, lse.cpu().numpy())
            positions = torch.arange(n, device=dev).expand(5, n).contiguous()
            lp = E.scores_log_prob(scores, positions, lse, None, temperature).cpu().numpy()
            real = ~np.isnan(v)                                          # (the payload of a NaN that arithmetic makes is the machine's own)
            assert np.array_equal(np.isnan(lp), ~real) and np.array_equal(lp.view(np.uint32)[real], v.view(np.uint32)[real]), "the reference's v"
            t = np.array([quantile_threshold(v[r], eligible[r], n // 5 + 1) for r in range(5)], dtype=np.float32)
            t[4] = np.float32("-inf")
            t_dev = torch.from_numpy(t).to(dev)
            most = check_against_reference(scores, bits, eligible, mask, t, t_dev, f"n = {n}, T = {temperature}", beta=beta, temperature=temperature, lse=lse)
            assert most >= n // 5 + 1
            assert G.counts(bits, eligible, t, beta, lse.cpu().numpy())[2:].tolist() == [0, 0, n - 1]      # (+inf - +inf is NaN: the +inf item itself misses)
    with pytest.raises(ValueError, match="temperature = 2.0 without lse"):
        E.scores_range_count(scores, 0.0, None, 2.0)
    with pytest.raises(ValueError, match="lse must be"):
        E.scores_range_count(scores, 0.0, None, 1.0, lse[:2])
    with pytest.raises(ValueError, match="threshold tensor"):
        E.scores_range(scores, torch.zeros(4, device=dev))


def test_a_write_pass_that_disagrees_with_its_count_stays_in_bounds(dev):
    """The C ABI's two passes with different thresholds between them: every store is tested against its slot's count and the capacity, so a
    write pass that finds more hits (or fewer) than were counted writes nothing beyond what was counted and sets the workspace's error word."""
    from rails_amd import _lib

    rng = np.random.default_rng(78)
    n = 3 * 4_096 + 38
    bits = np.stack([R.gauss(n, 1, rng) for _ in range(ROWS)])
    scores = on_device(bits, n + 5, 1, dev)
    lib = _lib.load()
    need = int(lib.rails_scores_range_workspace_bytes(ROWS, n))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    error_word = ws[need - 256 : need - 252].view(torch.int32)
    counted, more, fewer = (torch.full((ROWS,), v, device=dev) for v in (1.0, 0.0, 2.0))
    counts = torch.empty(ROWS, dtype=torch.int64, device=dev)
    lims = torch.empty(ROWS + 1, dtype=torch.int64, device=dev)

    def inputs(thr):
        return (E._ptr(scores), n + 5, ROWS, n, E._ptr(thr), 1.0, None, None, 0, E._ptr(ws), need)

    def count():
        _lib.check(lib.rails_scores_range_count(*inputs(counted), E._ptr(counts), E._ptr(lims), E._stream()), "rails_scores_range_count")

    count()
    w_lims, w_s, w_p = G.ragged(bits, True, 1.0, sort=False)
    total = int(lims[-1])
    assert np.array_equal(lims.cpu().numpy(), w_lims) and total > 1_000
    keys = torch.full((total + 64,), -1, dtype=torch.int64, device=dev)      # (-1 is no key of a hit: its score word is a NaN's)
    _lib.check(lib.rails_scores_range_write(*inputs(counted), E._ptr(keys), total, E._stream()), "rails_scores_range_write")
    assert int(error_word) == 0 and bool((keys[total:] == -1).all())
    want = (R.keys(w_s) & ~np.uint64(0xFFFFFFFF)) | (~w_p.astype(np.uint32)).astype(np.uint64)
    assert np.array_equal(keys[:total].cpu().numpy().view(np.uint64), want)
    for thr, capacity in ((more, total), (fewer, total), (counted, total - 100)):
        keys.fill_(-1)
        count()                                                              # (zeroes the error word)
        assert int(error_word) == 0
        _lib.check(lib.rails_scores_range_write(*inputs(thr), E._ptr(keys), capacity, E._stream()), "rails_scores_range_write")
        assert int(error_word) == 1 and bool((keys[capacity:] == -1).all())
        got = keys[:capacity].cpu().numpy().view(np.uint64)
        written = got != np.uint64(0xFFFFFFFFFFFFFFFF)
        assert 0 < int(written.sum()) <= capacity
        if thr is counted:
            assert bool(written.all()) and np.array_equal(got, want[:capacity])      # the short buffer holds the first `capacity` keys


# ---- the module contract ----------------------------------------------------------------------------------------------------------------
def rank_thresholds(bits, rank):
    """(B,) fp32: every row's rank-th largest logit"""
    return np.sort(bits.view(np.float32), axis=1)[:, ::-1][:, rank - 1].copy()


def check_module(tk, q, aux, bits, eligible, ids, t, what, **kw):
    """range_search sorted and unsorted and count_above against the reference on the module's own logits -> the sorted result"""
    eligible = np.broadcast_to(eligible, bits.shape)
    t_arg = torch.from_numpy(t).to(q.device) if isinstance(t, np.ndarray) else t
    out = None
    for sort in (False, True):
        out = tk.range_search(q, t_arg, sort=sort, **kw, **aux)
        w_lims, w_s, w_i = G.ragged(bits, eligible, t, sort=sort, ids=ids.cpu().numpy())
        assert np.array_equal(out[0].cpu().numpy(), w_lims) and np.array_equal(out[2].cpu().numpy(), w_i), f"{what}, sort={sort}"
        assert np.array_equal(out[1].view(torch.int32).cpu().numpy().view(np.uint32), w_s), f"{what}, sort={sort}: score bits"
    counts = tk.count_above(q, t_arg, **kw, **aux)
    assert counts.dtype == torch.int64 and counts.device == q.device and torch.equal(counts, out[0].diff()), f"{what}: count_above"
    return out


@pytest.mark.parametrize("module,route", ROUTES)
def test_range_search_is_the_exhaustive_list_down_to_the_threshold(module, route, dev):
    make, X, ids, q, aux = M.setup(module, route, dev, n=NM)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        bits = logit_bits(tk, q, aux)
        everything = np.ones((1, NM), dtype=bool)
        t = rank_thresholds(bits, 50)
        lims, s, i = check_module(tk, q, aux, bits, everything, ids, t, f"{module} {route}: per-row thresholds")
        assert lims.shape == (B + 1,) and int(lims[0]) == 0 and int(lims.diff().min()) >= 50
        # the sorted rows are forward's list cut at the threshold
        top_i = tk(q, k=200, **aux)[1]
        for b in (0, 7, B - 1):
            a, c = int(lims[b]), int(lims[b + 1])
            assert torch.equal(i[a:c], top_i[b, : c - a]), f"{module} {route}: row {b}"
        check_module(tk, q, aux, bits, everything, ids, float(np.median(t)), f"{module} {route}: one threshold")
        for special, count in ((float("-inf"), NM), (float("inf"), 0), (float("nan"), 0)):
            assert tk.count_above(q, special, **aux).tolist() == [count] * B
        # seen ids leave the row's eligible set
        seen = torch.cat([top_i[:, 5:66], torch.tensor([[2, 5]], device=dev).expand(B, -1)], dim=1).contiguous()
        elig = np.ones((B, NM), dtype=bool)
        np.put_along_axis(elig, ((top_i[:, 5:66] - 1) // 3).cpu().numpy(), False, axis=1)
        whole = check_module(tk, q, aux, bits, elig, ids, t, f"{module} {route}: seen ids", invalid_ids=seen)
        assert not bool(torch.isin(whole[2][: int(whole[0][1])], seen[0]).any())
        # two and three batch slices under the logit policy give the unsliced result; the threshold tensor is sliced with the batch
        for rows in (16, 11):
            tk.MAX_LOGIT_BYTES = rows * NM * 4
            sliced = check_module(tk, q, aux, bits, elig, ids, t, f"{module} {route}: slices of {rows} rows", invalid_ids=seen)
            assert all(torch.equal(a, b) for a, b in zip(sliced, whole))
        tk.MAX_LOGIT_BYTES = NM * 4 - 1
        for call in (tk.count_above, tk.range_search):
            with pytest.raises(NotImplementedError, match=type(tk).__name__ + r"\.\w+: one row"):
                call(q, 0.0, **aux)


@pytest.mark.parametrize("module,route", ROUTES)
def test_range_search_honours_what_a_row_may_return(module, route, dev):
    """A hidden set, per-row allowed_tags= and a ragged per-row item_mask= with seen ids."""
    make, X, ids, q, aux = M.setup(module, route, dev, n=NM)
    g = torch.Generator().manual_seed(82)
    with torch.inference_mode():
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        bits = logit_bits(tk, q, aux)
        t = rank_thresholds(bits, 300)
        best = ((tk(q, k=10, **aux)[1][:8, :2] - 1) // 3).reshape(-1).cpu()
        hidden = torch.unique(torch.cat([best, torch.randperm(NM, generator=g)[:500], torch.tensor([0, 31, 32, NM - 1])]))
        vis = torch.ones(NM, dtype=torch.bool)
        vis[hidden] = False
        m60 = torch.rand(NM, generator=g) < 0.6
        r200 = torch.zeros(NM, dtype=torch.bool)
        r200[torch.randperm(NM, generator=g)[:200]] = True
        three = [torch.ones(NM, dtype=torch.bool), torch.rand(NM, generator=g) < 0.5, r200]
        per_row = torch.stack([three[b % 3] for b in range(B)])
        tags = torch.randint(0, 8, (NM,), generator=g)
        allowed = [(1, 2, 5)[b % 3] for b in range(B)]
        check_module(tk, q, aux, bits, m60.numpy()[None], ids, t, f"{module} {route}: shared mask", item_mask=E.ItemMask(m60.to(dev)))
        tk.hide_items(hidden)
        check_module(tk, q, aux, bits, vis.numpy()[None], ids, t, f"{module} {route}: hidden set")
        check_module(tk, q, aux, bits, (m60 & vis).numpy()[None], ids, t, f"{module} {route}: hidden set and shared mask", item_mask=m60.to(dev))
        check_module(tk, q, aux, bits, (per_row & vis[None]).numpy(), ids, t, f"{module} {route}: ragged per-row mask", item_mask=E.ItemMask(per_row.to(dev)))
        seen_pos = torch.from_numpy(np.argsort(bits.view(np.float32), axis=1)[:, ::-1][:, :4].copy())      # every row's four best items
        elig = (per_row & vis[None]).clone()
        elig[torch.arange(B)[:, None], seen_pos] = False
        check_module(tk, q, aux, bits, elig.numpy(), ids, t, f"{module} {route}: per-row mask and seen ids", item_mask=E.ItemMask(per_row.to(dev)),
                     invalid_ids=ids[seen_pos.to(dev)].contiguous())
        tk.set_item_tags(tags.to(dev))
        by_tag = (tags[None, :] & torch.tensor(allowed)[:, None]) != 0
        check_module(tk, q, aux, bits, (by_tag & vis[None]).numpy(), ids, t, f"{module} {route}: per-row allowed_tags", allowed_tags=allowed)
        with pytest.raises(ValueError, match="allowed_tags= and item_mask="):
            tk.range_search(q, 0.0, allowed_tags=5, item_mask=m60.to(dev), **aux)


@pytest.mark.parametrize("module,route", ROUTES)
def test_range_search_on_an_all_tie_corpus(module, route, dev):
    """Every item row identical: a threshold equal to the row's one value keeps every item, in position order under both orders."""
    make, X, ids, q, aux = M.setup(module, route, dev, n=NM)
    g = torch.Generator().manual_seed(83)
    with torch.inference_mode():
        tk = make(X[:1].expand(NM, -1).contiguous().unsqueeze(0), ids.unsqueeze(0))
        bits = logit_bits(tk, q, aux)
        assert (bits == bits[:, :1]).all(), "the scores of identical items differ"
        t = bits[:, 0].copy().view(np.float32)
        keep = torch.rand(NM, generator=g) < 0.5
        for sort in (True, False):
            lims, s, i = tk.range_search(q, torch.from_numpy(t).to(dev), sort=sort, item_mask=keep.to(dev), **aux)
            assert lims.tolist() == [int(keep.sum()) * b for b in range(B + 1)]
            assert torch.equal(i.view(B, -1).cpu(), ids.cpu()[keep].expand(B, -1)) and np.array_equal(s.view(B, -1).cpu().numpy().view(np.uint32)[:, 0], bits[:, 0])
        above = np.nextafter(t, np.float32(np.inf))
        assert tk.count_above(q, torch.from_numpy(above).to(dev), **aux).tolist() == [0] * B
        assert tk.count_above(q, torch.from_numpy(t).to(dev), **aux).tolist() == [NM] * B


@pytest.mark.parametrize("module,route", ROUTES)
def test_range_search_after_corpus_edits(module, route, dev):
    """Six edits -- update, append, remove, update, append, hide -- with the id map live: the answers of a module freshly built from the
    resulting corpus, and the reference on its logits."""
    from tests import test_index_remove_gpu as RM

    make, X, ids, q, aux = M.setup(module, route, dev, n=NM)
    cfg = U.O.CONFIGS["amzn-books"] if module == "mips" else U.setup_route(module, route, dev)[0]
    g = torch.Generator().manual_seed(84)
    with torch.inference_mode():
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        top = tk(q, k=10, **aux)[1]
        tk.positions_of(top[:, 0].contiguous())                           # (the id map exists from here on)
        X2, ids2 = X.clone(), ids.clone()
        n_now = NM
        for step, (first, m_new) in enumerate(((20_000_000, 70), (40_000_000, 33))):
            upd = U.positions_for(n_now, g)
            rows = U.table(cfg, upd.numel(), 31 + step, dev, first=first)
            tk.update_items(upd, rows)
            X2[upd.to(dev)] = rows
            extra = U.table(cfg, m_new, 41 + step, dev, first=first + 5_000_000)
            extra[:2] = X[((top[2 * step : 2 * step + 2, 0] - 1) // 3)]   # copies of two queries' best items: the appended rows enter the head
            new_ids = torch.arange(-7 - 100 * step, -7 - 100 * step - m_new, -1, device=dev)
            tk.append_items(extra, new_ids)
            X2, ids2 = torch.cat([X2, extra]), torch.cat([ids2, new_ids])
            n_now += m_new
            if step == 0:
                gone = RM.removal_set(n_now, g, must=((top[:4, 1] - 1) // 3).cpu())
                tk.remove_items(gone)
                X2, ids2, _ = RM.after_removal(X2, ids2, gone)
                n_now -= gone.numel()
        hidden = torch.unique(torch.cat([torch.randperm(n_now, generator=g)[:300], torch.tensor([0, 31, 32, n_now - 1])]))
        fresh = make(X2.clone().unsqueeze(0), ids2.clone().unsqueeze(0))
        bits = logit_bits(fresh, q, aux)
        tk.hide_items(hidden)
        fresh.hide_items(hidden)
        assert tk.num_items == fresh.num_items == n_now == bits.shape[1]
        vis = np.ones((1, n_now), dtype=bool)
        vis[0, hidden.numpy()] = False
        t = rank_thresholds(bits, 100)
        seen = top[:, 3:9].contiguous()
        for kw in ({}, {"invalid_ids": seen}):
            got = tk.range_search(q, torch.from_numpy(t).to(dev), **kw, **aux)
            want = fresh.range_search(q, torch.from_numpy(t).to(dev), **kw, **aux)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), f"{module} {route}: after the edits {sorted(kw)}"
        check_module(tk, q, aux, bits, vis, ids2, t, f"{module} {route}: after the edits, against the reference")


@pytest.mark.parametrize("module,route", ROUTES)
def test_min_log_prob_is_log_prob_of_down_to_the_threshold(module, route, dev):
    """The hit set is {x : log_prob_of_positions(q, every position)[b, x] >= t} at T = 1 and T = 2, a row that may return nothing (its
    log_partition is -inf) included; the order and the scores against the reference on log_partition's bits."""
    make, X, ids, q, aux = M.setup(module, route, dev, n=NM)
    g = torch.Generator().manual_seed(85)
    with torch.inference_mode():
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        bits = logit_bits(tk, q, aux)
        per_row = torch.rand((B, NM), generator=g) < 0.7
        per_row[3] = False
        mask = E.ItemMask(per_row.to(dev))
        every = torch.arange(NM, device=dev).expand(B, NM).contiguous()
        for temperature in (1.0, 2.0):
            lp = tk.log_prob_of_positions(q, every, temperature=temperature, item_mask=mask, **aux)
            lse = tk.log_partition(q, temperature=temperature, item_mask=mask, **aux)
            assert lse[3].item() == float("-inf") and bool((lp[3] == float("-inf")).all())
            t = torch.sort(lp, dim=1, descending=True)[0][:, 120].contiguous()
            t[3] = -50.0
            hit = (lp >= t[:, None]).cpu()
            assert not bool(hit[3].any()) and int(hit.sum(dim=1)[0]) >= 121
            for sort in (True, False):
                lims, s, i = tk.range_search(q, min_log_prob=t, temperature=temperature, sort=sort, item_mask=mask, **aux)
                w = G.ragged(bits, per_row.numpy(), t.cpu().numpy(), np.float32(E.inv_temperature(temperature)), lse.cpu().numpy(), sort=sort, ids=ids.cpu().numpy())
                assert np.array_equal(lims.cpu().numpy(), w[0]) and np.array_equal(i.cpu().numpy(), w[2]), f"{module} {route}: T = {temperature}, sort={sort}"
                assert np.array_equal(s.view(torch.int32).cpu().numpy().view(np.uint32), w[1])
                assert torch.equal(lims.diff().cpu(), hit.sum(dim=1))
            for b in (0, 3, B - 1):
                assert torch.equal(i[int(lims[b]) : int(lims[b + 1])].cpu(), ids.cpu()[hit[b]]), f"{module} {route}: row {b}"
            assert torch.equal(tk.count_above(q, min_log_prob=t, temperature=temperature, item_mask=mask, **aux), lims.diff())
            assert torch.equal(tk.count_above(q, min_log_prob=float(t[0]), temperature=temperature, item_mask=mask, **aux)[0], lims.diff()[0])


def test_refusals(dev):
    """By name and before any launch: the approximate modules, collapse_groups=True, malformed thresholds and invalid_ids, both forms or neither."""
    cfg, mol, make, aux = U.setup_route("brute", "default", dev)
    n = 20_000
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 16, dev), U.ids_of(n, dev)
        q = U.O.synthetic_queries(cfg, B, seed=11).to(dev)
        others = {"avg": U.MAKERS["avg"](mol, X.unsqueeze(0), ids.unsqueeze(0)), "naive": U.MAKERS["naive"](mol, X.unsqueeze(0), ids.unsqueeze(0)),
                  "comb": U.MAKERS["comb"](mol, X.unsqueeze(0), ids.unsqueeze(0)),
                  "ivf": rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), k_per_group=5, use_faiss=True)}
        for other in others.values():
            for call in (other.count_above, other.range_search):
                with pytest.raises(NotImplementedError, match=type(other).__name__ + r"\.(count_above|range_search).*MoLBruteForceTopK"):
                    call(q, 0.0)
        tk = make(X.unsqueeze(0), ids.unsqueeze(0))
        for name, call in (("count_above", tk.count_above), ("range_search", tk.range_search)):
            with pytest.raises(NotImplementedError, match=rf"MoLBruteForceTopK\.{name} takes no collapse_groups"):
                call(q, 0.0, collapse_groups=True)
            for kw in ({}, {"min_score": 0.0, "min_log_prob": -3.0}):
                with pytest.raises(ValueError, match="exactly one of"):
                    call(q, **kw)
            with pytest.raises(ValueError, match="with min_score="):
                call(q, 0.0, temperature=0.5)
            for wrong in (torch.zeros(5, device=dev), torch.zeros((B, 1), device=dev), "0", None, torch.zeros(B, dtype=torch.bool, device=dev)):
                with pytest.raises(ValueError, match="threshold|exactly one of"):
                    call(q, wrong)
            with pytest.raises(ValueError, match="invalid_ids"):
                call(q, 0.0, invalid_ids=ids[:5].reshape(5, 1))
            with pytest.raises(ValueError, match="rows"):
                call(q, 0.0, item_mask=torch.ones((5, n), dtype=torch.bool, device=dev))
        with pytest.raises(ValueError, match=r"row \d+ has 20000 hits.*sort=False"):
            tk.range_search(q, float("-inf"))
        lims, s, i = tk.range_search(q[:2], float("-inf"), sort=False)
        assert lims.tolist() == [0, n, 2 * n] and torch.equal(i, ids.repeat(2))
