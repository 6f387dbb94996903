"""The dot-product path -- rails_amd/csrc/mips.hip behind engine.MipsIndex, engine.dot_rowwise, DotProductSimilarity and MIPSBruteForceTopK
-- kernel by kernel against the float64 restatement of tests/_dot_ref64.py.

Arithmetic: every output of rails_mips_score and rails_dot_rowwise is held to the per-pair bound gamma_D <|q|, |x|> of an fp32 FMA chain of
length D (derived at the top of tests/_dot_ref64.py; no floor term, the inputs keep every product and partial sum normal).  Copies: the tile
layout of the index is pinned bit for bit by mips_layout, a statement of the layout in plain indexing that shares nothing with the pack,
scatter and gather kernels, so an error common to the three cannot pass; the in-place corpus calls are held to mips_layout of the resulting
table instead of to a fresh build.  Selection: MIPSBruteForceTopK.forward is bit-equal to the deterministic rule on the module's own scores,
and its returned set obeys the float64 rule of _dot_ref64.topk_rule.

Shapes are the smallest that reach each edge: D below 8, D % 8 != 0 (where Dp / 2 != D / 2), one item, a ragged last tile, a ragged last
query group, ld > N, and mips_score_kernel's persistent loop (more than 32 n_cu units), sized from the device's compute-unit count.

The CPU tests (unmarked) plant four bug classes in the float64 reference at the GPU cases' inputs -- the last k dropped, the second lane
half taken from D / 2, padding not zeroed, bq % B_I for bq / r -- and require at least 95 % of the affected outputs outside the bound;
they also check that the layout round-trips through the gather formula and that the float64 top-k rule leaves few places open.
"""
import pytest
import torch

from oracle import mol_oracle as O
from tests import _dot_ref64 as R

DS = [1, 4, 7, 8, 9, 50, 64, 100, 257]
NS = [1, 31, 32, 33, 517]
B0, N0, D0 = 33, 517, 50
# rails_mips_score: (B, N, D, kind)
SCORE_CASES = ([(B0, N0, D, "plain") for D in DS]
               + [(B, N, D0, "plain") for B, N in ((1, 1), (1, 31), (31, 32), (32, 33), (64, 1024), (65, 1025))]
               + [(B0, N0, D0, "x1e3"), (B0, N0, D0, "cancel"), (B0, N0, 257, "cancel")])
PERSISTENT_B, PERSISTENT_D = 225, 16          # 8 query groups, one row in the last
ROWWISE_CASES = [(BI, r, X, D) for BI in (2, 5) for r in (1, 3) for X in (1, 33, 200) for D in (1, 50, 64)]
TOPK_B, TOPK_D = 33, 50
TOPK_CASES = [(N, k) for N in (517, 5009) for k in (1, 10, N)]
MIN_CAUGHT = 0.95


def persistent_items(n_cu):
    """The smallest N whose tiles times 8 query groups exceed the 32 n_cu units one launch of mips_score_kernel holds, plus 1."""
    return 32 * (4 * n_cu) + 1 + 1


def case_id(c):
    return "-".join(str(v) for v in c)


# ============================================================================================================================
# CPU: the inputs, the layout restatement and the sensitivity of the bound
# ============================================================================================================================
def outside_share(mutated, ref, bound, affected=None):
    out = (mutated - ref).abs() > bound
    if affected is None:
        affected = torch.ones_like(out)
    assert bool(affected.any())
    return float(out[affected].double().mean())


def test_inputs_keep_every_product_normal():
    for B, N, D, kind in SCORE_CASES + [(PERSISTENT_B, persistent_items(256), PERSISTENT_D, "plain")]:
        assert R.products_stay_normal(*R.score_inputs(B, N, D, kind)), (B, N, D, kind)
    for BI, r, X, D in ROWWISE_CASES:
        q, items = R.rowwise_inputs(BI, r, X, D)
        assert R.products_stay_normal(q, items.reshape(-1, D)), (BI, r, X, D)
    for N, _ in TOPK_CASES:
        q, X, _, _ = R.topk_inputs(TOPK_B, N, TOPK_D)
        assert R.products_stay_normal(q, X)
    # the cancellation case keeps mag and loses digits of ref
    ref, bound = R.dot64(*R.score_inputs(B0, N0, D0, "cancel"))
    plain_ref, plain_bound = R.dot64(*R.score_inputs(B0, N0, D0, "plain"))
    assert float(ref.abs().median()) < 0.05 * float(plain_ref.abs().median()) and float(bound.median()) > 0.5 * float(plain_bound.median())


@pytest.mark.parametrize("case", SCORE_CASES, ids=case_id)
def test_bound_catches_a_dropped_k_a_wrong_half_and_live_padding(case):
    """(a) the last k dropped: every case.  (b) the item operand's second half from D / 2: where Dp / 2 != D / 2.  (c) padding not
    zeroed: where Dp > D (and the neighbouring row exists)."""
    B, N, D, kind = case
    q, X = R.score_inputs(B, N, D, kind)
    ref, bound = R.dot64(q, X)
    muts = ["drop_last_k"]
    if R.padded(D) // 2 != D // 2 and D in (50, 257):
        muts.append("half_at_D2")
    if R.padded(D) != D and B > 1 and N > 1:
        muts.append("pad_next_row")
    for mut in muts:
        m, _ = R.dot64(q, X, mut=mut)
        affected = m != ref
        assert float(affected.double().mean()) >= 0.99, (case, mut)
        share = outside_share(m, ref, bound, affected)
        print(f"[bug class] {mut} at B={B} N={N} D={D} {kind}: {100 * share:.2f} % of the affected outputs outside the bound")
        assert share >= MIN_CAUGHT, (case, mut, share)


def test_bound_catches_the_wrong_batch_of_items():
    """(d) bq % B_I in place of bq / r, on the rows where the two differ (r > 1)."""
    for BI, r, X, D in ROWWISE_CASES:
        if r == 1:
            continue
        q, items = R.rowwise_inputs(BI, r, X, D)
        ref, bound = R.rowwise64(q, items)
        m, _ = R.rowwise64(q, items, mut="mod_bi")
        rows = torch.arange(BI * r)
        affected = ((rows % BI) != (rows // r)).view(-1, 1).expand_as(ref)
        share = outside_share(m, ref, bound, affected)
        print(f"[bug class] mod_bi at B_I={BI} r={r} X={X} D={D}: {100 * share:.2f} % of the affected outputs outside the bound")
        assert share >= MIN_CAUGHT, (BI, r, X, D, share)


@pytest.mark.parametrize("D", DS)
def test_layout_round_trips_through_the_gather_formula(D):
    for N in NS:
        X = R.table(N, D, seed=N + D)
        buf = R.mips_layout(X)
        assert buf.numel() == R.index_floats(D, N) == -(-N // 32) * 32 * R.padded(D)
        assert int((buf != 0).sum()) == int((X != 0).sum()), "everything but the table's values is zero"
        pos = torch.cat([torch.arange(N), torch.tensor([-1, N])])
        rows = R.gather_rows(buf, N, D, pos)
        assert torch.equal(R.bits(rows[:N]), R.bits(X)) and bool((rows[N:] == 0).all()), (D, N)


@pytest.mark.parametrize("case", TOPK_CASES, ids=case_id)
def test_topk_rule_leaves_few_places_open(case):
    """Float64 alone: the share of the (row, rank) places inside the 2 eps band of the k-th score stays below 5 %, so the rule pins
    nearly every place.  (The exact ties of the copied rows are pinned by the bit-equal check against the deterministic selection.)"""
    N, k = case
    q, X, dup, src = R.topk_inputs(TOPK_B, N, TOPK_D)
    assert dup.numel() == N // 4 and torch.equal(X[dup], X[src]) and not bool(torch.isin(src, dup).any())
    ref, bound = R.dot64(q, X)
    share, open_rows = R.band_share(ref, bound, k)
    print(f"[band] N={N} k={k}: {100 * share:.3f} % of the (row, rank) places inside the 2 eps band; "
          f"{100 * open_rows:.1f} % of the rows have a tie across the k-th place")
    assert share < 0.05
    # the rule accepts the float64 ranking itself and rejects a set that swaps the best item for one 40 places past the k-th (the best
    # item is then missing -- at k = 1 it is the k-th itself, which only the second half of the rule holds -- and the other intrudes)
    order = torch.sort(ref, dim=1, descending=True, stable=True).indices
    assert R.topk_rule(ref, bound, order[:, :k], k) == (0, 0)
    if k < N:
        wrong = order[:, :k].clone()
        wrong[:, 0] = order[:, k + 40]
        missing, intruding = R.topk_rule(ref, bound, wrong, k)
        assert intruding >= 0.9 * TOPK_B and (k == 1 or missing >= 0.9 * TOPK_B)


def test_persistent_case_exceeds_one_launch_of_units():
    for n_cu in (64, 256, 304):
        N = persistent_items(n_cu)
        tiles, groups = -(-N // 32), -(-PERSISTENT_B // 32)
        assert groups == 8 and PERSISTENT_B % 32 == 1 and N % 32 == 2
        assert tiles * groups > 32 * n_cu and (tiles - 1) * groups <= 32 * n_cu


# ============================================================================================================================
# GPU
# ============================================================================================================================
RATIOS = {}   # kernel -> worst |got - ref| / bound seen by this module's GPU cases (printed when the module finishes)


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    for k in sorted(RATIOS):
        print(f"[ratio] {k}: {RATIOS[k]:.3f}")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def n_cu():
    from rails_amd import _lib

    n = int(_lib.load().rails_device_compute_units())
    assert n > 0
    return n


def assert_within(got, ref, bound, what, kernel, keep=None):
    """Every element (of `keep`, a bool mask, when given) inside its bound; the worst ratio goes to RATIOS and is printed."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(bound).all()), f"{what}: infinite bound"
    d = (got - ref).abs()
    bad = ~(d <= bound)
    ratio = d / bound.clamp(min=1e-300)
    if keep is not None:
        bad, ratio = bad & keep, ratio[keep]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), worst)
    print(f"[ratio] {what}: worst |err| / bound = {worst:.3f}")
    if bool(bad.any()):
        idx = tuple(int(t) for t in bad.nonzero()[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at {idx}: got {float(got[idx])!r}, "
                    f"ref {float(ref[idx])!r}, |d| {float(d[idx]):.3e} > bound {float(bound[idx]):.3e}")


SPECIALS = torch.tensor([-2 ** 31, 0x7F800000, 0x7FC01234, 0x00000123], dtype=torch.int32).view(torch.float32)   # -0.0, inf, a NaN, a subnormal


def with_specials(X):
    X = X.clone()
    flat = X.view(-1)
    n = flat.numel()
    for v, i in zip(SPECIALS, dict.fromkeys([0, n - 1, n // 2, n // 3])):
        flat[i] = v
    return X


# ---- 1. the layout, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_index_layout_bit_for_bit(dev, D):
    from rails_amd import _lib
    from rails_amd import engine as E

    for N in NS:
        X = with_specials(R.table(N, D, seed=3 * N + D))
        buf = E.MipsIndex(X.to(dev)).buf
        assert buf.numel() == _lib.load().rails_mips_index_floats(D, N) == R.index_floats(D, N)
        assert torch.equal(R.bits(buf), R.bits(R.mips_layout(X))), f"fp32 table, D={D} N={N}"
        X16 = X.bfloat16()
        assert torch.equal(R.bits(E.MipsIndex(X16.to(dev)).buf), R.bits(R.mips_layout(X16.float()))), f"bf16 table, D={D} N={N}"


# ---- 2. rails_mips_score against float64, per pair ----------------------------------------------------------------------
def score(dev, q, X):
    from rails_amd import engine as E

    return E.MipsIndex(X.to(dev)).score(q.to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCORE_CASES, ids=case_id)
def test_mips_score_matches_float64(dev, case):
    B, N, D, kind = case
    q, X = R.score_inputs(B, N, D, kind)
    ref, bound = R.dot64(q, X)
    assert_within(score(dev, q, X), ref, bound, f"mips_score B={B} N={N} D={D} {kind}", "mips_score_kernel")


@pytest.mark.gpu
def test_mips_score_persistent_loop_matches_float64(dev, n_cu):
    B, D, N = PERSISTENT_B, PERSISTENT_D, persistent_items(n_cu)
    tiles, groups = -(-N // 32), -(-B // 32)
    assert tiles * groups > 32 * n_cu, "the grid is capped at 8 n_cu workgroups of 4 waves: more units than that enter the loop"
    assert groups == 8 and B % 32 == 1 and N % 32 != 0
    q, X = R.score_inputs(B, N, D)
    ref, bound = R.dot64(q, X)
    assert_within(score(dev, q, X), ref, bound, f"mips_score persistent B={B} N={N} D={D} (n_cu={n_cu})", "mips_score_kernel")


# ---- 3. / 4. the write mask and containment, through the C entry point ----------------------------------------------------
SENTINEL = 0x5A5A5A5A


def score_raw(dev, q, X, ld, rows):
    """rails_mips_score into a (rows, ld) buffer pre-filled with SENTINEL -> the buffer (CPU)."""
    from rails_amd import _lib
    from rails_amd import engine as E

    lib = _lib.load()
    B, D = q.shape
    index = E.MipsIndex(X.to(dev))
    dq = q.to(dev).contiguous()
    ws = torch.empty(lib.rails_mips_query_ws_floats(D, B), dtype=torch.float32, device=dev)
    out = torch.empty((rows, ld), dtype=torch.float32, device=dev)
    out.view(torch.int32).fill_(SENTINEL)
    _lib.check(lib.rails_mips_score(E._ptr(dq), B, D, E._ptr(index.buf), X.shape[0], E._ptr(ws), E._ptr(out), ld, E._stream()), "rails_mips_score")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.gpu
def test_mips_score_writes_only_its_own_outputs(dev):
    q, X = R.score_inputs(B0, N0, D0)
    ref, bound = R.dot64(q, X)
    out = score_raw(dev, q, X, ld=N0 + 5, rows=B0 + 3)
    assert bool((R.bits(out[:B0, N0:]) == SENTINEL).all()), "columns at or past N were written"
    assert bool((R.bits(out[B0:]) == SENTINEL).all()), "rows at or past B were written"
    assert_within(out[:B0, :N0], ref, bound, "mips_score ld = N + 5", "mips_score_kernel")


@pytest.mark.gpu
def test_non_finite_rows_stay_in_their_row_and_column(dev):
    q, X = R.score_inputs(B0, N0, D0)
    ref, bound = R.dot64(q, X)
    x0, b0 = 100, 5                                    # an item inside a tile of 32, a query inside a group of 32
    Xn = X.clone()
    Xn[x0, 3] = float("nan")
    out = score_raw(dev, q, Xn, ld=N0 + 5, rows=B0 + 3)
    keep = torch.ones_like(ref, dtype=torch.bool)
    keep[:, x0] = False
    assert bool(torch.isnan(out[:B0, x0]).all()), "a NaN in an item row reaches every score of its column"
    assert_within(out[:B0, :N0], ref, bound, "mips_score, NaN in item 100", "mips_score_kernel", keep=keep)
    qi = q.clone()
    qi[b0, 7] = float("inf")
    out = score_raw(dev, qi, X, ld=N0 + 5, rows=B0 + 3)
    keep = torch.ones_like(ref, dtype=torch.bool)
    keep[b0] = False
    assert not bool(torch.isfinite(out[b0, :N0]).any()), "an inf in a query reaches every score of its row"
    assert_within(out[:B0, :N0], ref, bound, "mips_score, inf in query 5", "mips_score_kernel", keep=keep)
    assert bool((R.bits(out[:B0, N0:]) == SENTINEL).all()) and bool((R.bits(out[B0:]) == SENTINEL).all())


# ---- 5. rails_dot_rowwise through engine.dot_rowwise ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("BI,r", [(2, 1), (2, 3), (5, 1), (5, 3)])
def test_dot_rowwise_matches_float64(dev, BI, r):
    from rails_amd import engine as E

    for _, _, X, D in (c for c in ROWWISE_CASES if c[:2] == (BI, r)):
        q, items = R.rowwise_inputs(BI, r, X, D)
        ref, bound = R.rowwise64(q, items)
        got = E.dot_rowwise(q.to(dev), items.to(dev))
        assert_within(got, ref, bound, f"dot_rowwise B_I={BI} r={r} X={X} D={D}", "dot_rowwise_kernel")


# ---- 6. DotProductSimilarity ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dot_product_similarity_branches_match_float64(dev):
    import rails_amd

    dp = rails_amd.DotProductSimilarity()
    with torch.inference_mode():
        # B_I == 1: (B, D) x (1, X, D), also at B = 1
        for B in (B0, 1):
            q, X = R.score_inputs(B, N0, D0)
            out, aux = dp(q.to(dev), X.unsqueeze(0).to(dev))
            assert aux == {} and out.dtype == torch.float32
            assert_within(out, *R.dot64(q, X), f"DotProductSimilarity B_I=1 B={B}", "mips_score_kernel")
        # (B_I r, D) x (B_I, X, D), r = 3, and the per-row case B == B_I
        for BI, r in ((5, 3), (5, 1)):
            q, items = R.rowwise_inputs(BI, r, 33, D0)
            out, aux = dp(q.to(dev), items.to(dev))
            assert aux == {} and tuple(out.shape) == (BI * r, 33)
            assert_within(out, *R.rowwise64(q, items), f"DotProductSimilarity B_I={BI} r={r}", "dot_rowwise_kernel")
        q, items = R.rowwise_inputs(5, 1, 33, D0)
        with pytest.raises(RuntimeError):
            dp(torch.cat([q, q[:2]]).to(dev), items.to(dev))          # 7 queries, 5 batches of items


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_dot_product_similarity_half_inputs_round_once(dev, dtype):
    """fp32 arithmetic on the widened inputs, one rounding to the query's dtype at the end."""
    import rails_amd

    dp = rails_amd.DotProductSimilarity()
    with torch.inference_mode():
        q, X = R.score_inputs(B0, N0, D0)
        q16, X16 = q.to(dtype).to(dev), X.to(dtype).unsqueeze(0).to(dev)
        out, _ = dp(q16, X16)
        wide, _ = dp(q16.float(), X16.float())
        assert out.dtype == dtype and wide.dtype == torch.float32
        assert torch.equal(out, wide.to(dtype))
        assert_within(wide, *R.dot64(q16.float(), X16[0].float()), f"DotProductSimilarity {dtype} inputs, widened", "mips_score_kernel")
        q, items = R.rowwise_inputs(5, 3, 33, D0)
        q16, i16 = q.to(dtype).to(dev), items.to(dtype).to(dev)
        out, _ = dp(q16, i16)
        wide, _ = dp(q16.float(), i16.float())
        assert out.dtype == dtype and torch.equal(out, wide.to(dtype))
        assert_within(wide, *R.rowwise64(q16.float(), i16.float()), f"DotProductSimilarity {dtype} inputs, row-wise, widened", "dot_rowwise_kernel")


# ---- 7. MIPSBruteForceTopK.forward --------------------------------------------------------------------------------------
def item_ids(n, first=0):
    return torch.arange(first, first + n, dtype=torch.int64) * 3 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("N", [517, 5009])
def test_mips_topk_is_the_deterministic_selection_and_obeys_the_float64_rule(dev, N):
    import rails_amd

    q, X, dup, src = R.topk_inputs(TOPK_B, N, TOPK_D)
    ids = item_ids(N)
    ref, bound = R.dot64(q, X)
    with torch.inference_mode():
        tk = rails_amd.MIPSBruteForceTopK(X.unsqueeze(0).to(dev), ids.unsqueeze(0).to(dev))
        logits = tk._index.score(q.to(dev))
        assert_within(logits, ref, bound, f"MIPSBruteForceTopK scores N={N}", "mips_score_kernel")
        lc = logits.cpu()
        assert torch.equal(lc[:, dup], lc[:, src]), "a column's arithmetic does not depend on its slot: copies tie exactly"
        for k in (1, 10, N):
            scores, got = tk(q.to(dev), k=k)
            want_s, want_pos = O.select_topk_deterministic(lc, k)
            assert scores.dtype == torch.float32 and got.dtype == torch.int64
            assert torch.equal(R.bits(scores), R.bits(want_s)), f"scores, k={k}"
            assert torch.equal(got.cpu(), ids[want_pos]), f"ids, k={k}: ties must come out in ascending position"
            pos = (got.cpu() - 1) // 3
            assert R.topk_rule(ref, bound, pos, k) == (0, 0), f"float64 rule, k={k}"


# ---- 8. the in-place corpus calls -----------------------------------------------------------------------------------------
def check_module_against_table(tk, X, q, ref_ids, what, dev):
    """_index.buf is mips_layout of X; rows() returns X's rows bit for bit (first tile, last tile) and zeros outside; score is inside the
    float64 bound of X; the ids are ref_ids."""
    N, D = X.shape
    assert tk.num_items == N and torch.equal(tk._ids_flat.cpu(), ref_ids), what
    assert torch.equal(R.bits(tk._index.buf), R.bits(R.mips_layout(X))), f"{what}: index bytes"
    last = torch.arange(32 * ((N - 1) // 32), N)
    pos = torch.cat([torch.arange(min(32, N)), last, torch.tensor([-1, N])])
    rows = tk._index.rows(pos.to(dev)).cpu()
    assert torch.equal(R.bits(rows[:-2]), R.bits(X[pos[:-2]])), f"{what}: rows()"
    assert bool((rows[-2:] == 0).all()), f"{what}: rows() outside the index"
    ref, bound = R.dot64(q, X)
    assert_within(tk._index.score(q.to(dev)), ref, bound, f"{what}: score", "mips_score_kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("D", [50, 1])
def test_in_place_calls_leave_the_layout_of_the_resulting_table(dev, D):
    import rails_amd
    from rails_amd.topk_modules import removal_plan

    N = N0
    X, ids = R.table(N, D, seed=21 + D), item_ids(N)
    q = R.queries(B0, D, seed=5 + D)
    with torch.inference_mode():
        tk = rails_amd.MIPSBruteForceTopK(X.clone().unsqueeze(0).to(dev), ids.clone().unsqueeze(0).to(dev))
        check_module_against_table(tk, X, q, ids, f"D={D} as built", dev)
        # update
        p = torch.tensor([0, 31, 32, N - 1])
        rows = R.table(4, D, seed=22 + D, first=10_000)
        tk.update_items(p, rows.to(dev))
        X = X.clone()
        X[p] = rows
        check_module_against_table(tk, X, q, ids, f"D={D} update_items", dev)
        # append: the part-filled last tile is filled up and a new one is started
        extra, extra_ids = R.table(40, D, seed=23 + D, first=20_000), item_ids(40, first=50_000)
        tk.append_items(extra.to(dev), extra_ids.to(dev))
        X, ids = torch.cat([X, extra]), torch.cat([ids, extra_ids])
        check_module_against_table(tk, X, q, ids, f"D={D} append_items", dev)
        # remove: 557 -> 544 (a full last tile) -> 513 (one item past a full tile); holes below the cut are filled from the tail
        for gone in (torch.tensor([0, 31, 32, 100, 300, 516, 517, 540, 543, 544, 550, 555, 556]),
                     torch.cat([torch.tensor([1, 33, 64, 200, 511, 512]), torch.arange(513, 538)])):
            n = X.shape[0]
            n_new = n - gone.numel()
            holes, movers = removal_plan(gone, n)
            assert movers.numel() > 0 and n_new in (544, 513)
            moved = tk.remove_items(gone[torch.randperm(gone.numel(), generator=R.gen(n))])
            assert torch.equal(moved, torch.stack([movers, holes], dim=1))
            X2, ids2 = X[:n_new].clone(), ids[:n_new].clone()
            X2[holes], ids2[holes] = X[movers], ids[movers]
            X, ids = X2, ids2
            check_module_against_table(tk, X, q, ids, f"D={D} remove_items -> {n_new}", dev)


# ---- 9. end to end: a SASRec encoder, dot-product similarity, the eval harness -------------------------------------------------
@pytest.mark.gpu
def test_eval_harness_with_sasrec_and_dot_product_retrieval(dev):
    import rails_amd
    from rails_amd import eval_harness as H
    from tests import _sasrec_ref as S

    f = S.load("amzn-books")
    c = f["cfg"]
    m = rails_amd.SASRec(c["max_sequence_len"], c["max_output_len"], c["D"], c["blocks"], c["heads"], c["ffn"], c["act"], num_items=c["num_items"],
                         similarity_module=rails_amd.DotProductSimilarity(), output_postproc=c["postproc"])
    res = m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in f.items() if k.startswith("w/")}, strict=False)
    assert not res.unexpected_keys and not res.missing_keys
    m = m.to(dev).eval()
    lengths, past = torch.from_numpy(f["in/past_lengths"]), torch.from_numpy(f["in/past_ids"])
    n_items = c["num_items"]
    all_ids = torch.arange(1, n_items + 1, dtype=torch.int64)
    target = torch.randint(1, n_items + 1, (past.shape[0], 1), generator=R.gen(1))
    with torch.inference_mode():
        state = H.get_eval_state(m, all_ids.tolist(), None, lambda emb, eids: rails_amd.MIPSBruteForceTopK(emb, eids), dev)
        assert isinstance(state.top_k_module, rails_amd.MIPSBruteForceTopK)
        feats = H.SequentialFeatures(lengths.to(dev), past.to(dev), None, {})
        out = H.eval_metrics_v2_from_tensors(state, m, feats, target.to(dev), include_eval_top_k_ids=True)
        got = out["eval_top_k_ids"]
        k = got.shape[1]
        q = m.encode(lengths.to(dev), past.to(dev), m.get_item_embeddings(past.to(dev)), {})
        want, _, _ = state.candidate_index.get_top_k_outputs(query_embeddings=q, top_k_module=state.top_k_module, k=k, aux_payloads={},
                                                             invalid_ids=past.to(dev), return_embeddings=False)
        table = m.get_item_embeddings(all_ids.unsqueeze(0).to(dev))[0]
        sim, _ = m._ndp_module(q, table.unsqueeze(0))
    torch.cuda.synchronize()
    assert k == min(2500, n_items) and torch.equal(got.cpu(), want.cpu())
    ref, bound = R.dot64(q, table)
    assert_within(sim, ref, bound, "the model's own similarity on its embeddings", "mips_score_kernel")
    # the harness asks for k' = min(k + history, N) = N candidates here, so the ids are the whole ranking, best first: every prefix of it
    # is a top-k' set and is held to the float64 rule
    assert k == n_items and bool((torch.sort(got.cpu(), dim=1).values == all_ids).all())
    pos = got.cpu() - 1
    for kk in (1, 10, 100, k):
        assert R.topk_rule(ref, bound, pos[:, :kk], kk) == (0, 0), f"float64 rule on the first {kk} ids"
