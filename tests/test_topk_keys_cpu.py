"""CPU side of the exact top-k suite (tests/_topk_ref.py, tests/test_topk_keys_gpu.py): the case table reaches every route and branch the
restatement of the dispatch can name, the dispatch restatement is pinned at both sides of every line, and nine bug classes applied to the
restatement each change the expected output of some case -- the bars of the GPU test can fail."""
import numpy as np
import pytest

from tests import _topk_ref as T


def _bits(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32)


# ---- the contract itself -----------------------------------------------------------------------------------------------------------------
def test_key_order_on_the_documented_row():
    row = _bits([0.0, -0.0, np.nan, 1.0, 0.0, np.inf]).copy()
    row[2], row[4] = 0x7FC00000, 0xFFC00000          # the NaN a device makes, the NaN x86 host arithmetic makes for 0/0
    s, pos = T.select(row, 6)
    assert pos.tolist() == [2, 5, 3, 0, 1, 4]
    assert s.tolist() == [0x7FC00000, 0x7F800000, 0x3F800000, 0x00000000, 0x80000000, 0xFFC00000]
    assert T.orderable(np.array([T.EXCLUDED], dtype=np.uint32))[0] == 0          # the excluded pattern is the padding key
    every = np.arange(0, 1 << 32, 65521, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(T.unorderable(T.orderable(every)), every)
    # the key order is the float order wherever floats are ordered: finite values and infinities, no zeros of opposite sign
    x = np.random.default_rng(0).standard_normal(4000).astype(np.float32)
    x[:4] = [np.inf, -np.inf, 1e-40, -1e-40]
    assert np.array_equal(np.argsort(T.orderable(x.view(np.uint32)), kind="stable"), np.argsort(x, kind="stable"))


def test_filter_seen_and_merged_by_hand():
    ids, sc = np.array([10, 11, 12, 13, 14, 15]), np.arange(6, dtype=np.uint32)
    assert T.filter_seen(ids, sc, [11, 13], 3)[0].tolist() == [10, 12, 14]                 # first three unseen
    assert T.filter_seen(ids, sc, [], 2)[0].tolist() == [10, 11]
    assert T.filter_seen(ids, sc, [10, 11, 12, 13, 15], 3)[0].tolist() == [10, 11, 14]     # one unseen: the earliest dropped fill up, in candidate order
    assert T.filter_seen(ids, sc, [10, 11, 12, 13, 15], 3)[1].tolist() == [0, 1, 4]
    one, half, ninf = 0x3F800000, 0x3F000000, 0xFF800000
    msg = np.array([[[one, half, 7, 8]], [[one, ninf, 9, -1]]], dtype=np.int64)            # R = 2, one row, k = 2
    s, i = T.merged(msg, 2, 2, 3)
    assert s.tolist() == [[one, one, half]] and i.tolist() == [[7, 9, 8]]                  # equal words: rank 0's entry first


# ---- the dispatch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,kw,name,params", [
    ((2, 512, 1), {}, "sort_whole", {"npad": 512, "sort": "block_rank_desc"}),
    ((2, 513, 1), {}, "row_select", {"vpt": 4}),
    ((2, 513, 512), {}, "row_select", {"vpt": 4}),
    ((2, 513, 513), {}, "sort_whole", {"npad": 1024, "sort": "block_sort_desc"}),
    ((2, 1024, 513), {}, "sort_whole", {"npad": 1024}),
    ((2, 1025, 513), {}, "row_select", {"vpt": 4}),
    ((2, 1025, 1025), {}, "sort_whole", {"npad": 2048, "sort": "multi<2>"}),
    ((2, 4096, 2048), {}, "row_select", {"vpt": 4}),
    ((2, 4096, 2049), {}, "sort_whole", {"sort": "multi<4>"}),
    ((2, 4097, 4096), {}, "row_select", {"vpt": 8}),
    ((2, 4097, 4097), {}, "sort_whole", {"sort": "multi<8>"}),
    ((2, 16384, 4096), {}, "row_select", {"vpt": 16}),
    ((2, 16384, 4097), {}, "sort_whole", {"sort": "multi<16>"}),
    ((2, 16385, 4096), {}, "row_select", {"vpt": 28}),
    ((2, 16385, 4097), {}, "radix", {"npad": 8192, "sort": "multi<8>"}),
    ((2, 28672, 1), {}, "row_select", {"vpt": 28}),
    ((2, 28673, 1), {}, "row_select", {"vpt": 40}),
    ((2, 40960, 1), {}, "row_select", {"vpt": 40}),
    ((2, 40961, 1), {}, "row_select", {"vpt": 48}),
    ((2, 49152, 4096), {}, "row_select", {"vpt": 48}),
    ((2, 49153, 512), {}, "two_level", {"chunks": 3, "chunk": 16388, "vpt": 28, "vpt2": 4, "halved": True}),
    ((2, 49153, 513), {}, "radix", {"npad": 1024, "chunks": 7, "sort": "block_sort_desc"}),
    ((2, 49153, 513), {"predicated": True}, "two_level", {"chunks": 3}),
    ((2, 200000, 4096), {"predicated": True}, "two_level", {"chunks": 5, "chunk": 40000, "vpt": 40, "vpt2": 24, "halved": False}),
    ((2, 200000, 4097), {"predicated": True}, "radix", {"npad": 8192}),
    ((8, 98304, 200), {}, "two_level", {"chunks": 4, "chunk": 24576, "vpt": 28, "halved": True}),
    ((9, 98304, 200), {}, "two_level", {"chunks": 2, "chunk": 49152, "vpt": 48, "halved": False}),
    ((1, 48 * 24576, 512), {}, "two_level", {"chunks": 48, "chunk": 24576, "vpt2": 24}),            # c * k = 24 576: the second level is full
    ((1, 48 * 24576 + 1, 512), {}, "two_level", {"chunks": 25, "vpt": 48, "vpt2": 16, "halved": False}),   # 49 halved chunks do not fit: full chunks
    ((1, 48 * 49152, 512), {}, "two_level", {"chunks": 48, "chunk": 49152}),
    ((1, 48 * 49152 + 1, 512), {}, "radix", {"npad": 512, "sort": "block_rank_desc", "chunks": 289}),
    ((1, 48 * 49152 + 1, 501), {}, "two_level", {"chunks": 49, "chunk": 48152, "vpt2": 24}),        # 49 * 501 = 24 549 keys
    ((1, 48 * 49152 + 1, 502), {}, "radix", {"npad": 512}),
    ((2048, 49153, 513), {}, "radix", {"chunks": 1, "chunk": 49153}),
    ((2, 5000, 120), {"fused": True}, "row_select", {"vpt": 8}),
    ((2, 60001, 512), {"fused": True}, "two_level", {"chunks": 3}),
    ((2, 512, 200), {"indexed": True}, "sort_whole", {"npad": 512}),
    ((2, 513, 200), {"indexed": True}, "row_select", {"vpt": 4, "indexed": True}),
    ((2, 4096, 200), {"indexed": True}, "row_select", {"vpt": 4, "indexed": True}),
    ((2, 4097, 200), {"indexed": True}, "row_select", {"vpt": 8, "indexed": True}),
    ((2, 8192, 4096), {"indexed": True}, "row_select", {"vpt": 8, "indexed": True}),
    ((2, 8193, 200), {"indexed": True}, "sort_whole", {"npad": 16384, "sort": "multi<16>"}),
    ((2, 8192, 4097), {"indexed": True}, "sort_whole", {"npad": 8192}),
    ((2, 8192, 300), {"indexed": True, "fused": True}, "row_select", {"vpt": 8, "indexed": True}),
])
def test_route_at_both_sides_of_every_line(args, kw, name, params):
    got_name, got = T.route(*args, **kw)
    assert got_name == name and {key: got[key] for key in params} == params, (got_name, got)


def test_route_refuses_what_topk_refuses():
    for args, kw in (((2, 1024, 100), {"fused": True}), ((2, 5000, 513), {"fused": True}), ((2, 16385, 10), {"indexed": True}),
                     ((2, 8193, 100), {"indexed": True, "fused": True})):
        with pytest.raises(ValueError):
            T.route(*args, **kw)


def test_emit_branch_edges():
    got = {c: T.emit_branch(c) for c in (1, 2, 32, 33, 63, 64, 65, 512, 513, 1024, 1025, 4096)}
    assert got == {1: "block_sort_desc<64", 2: "block_sort_desc<64", 32: "block_sort_desc<64", 33: "block_rank_desc", 63: "block_rank_desc",
                   64: "block_rank_desc", 65: "block_rank_desc", 512: "block_rank_desc", 513: "block_sort_desc", 1024: "block_sort_desc",
                   1025: "lds_bitonic", 4096: "lds_bitonic"}


def test_fast_path_fixed_points():
    """The survivor counts of the selection tests that already exist (tests/test_gpu_parity.py, their seeds): random rows stay in the hundreds,
    the seven-value tie rows give 497 .. 774, one row 2 767, and everything else overflows the 4 096 slots; a narrow spread of distinct values --
    what MoL logits are -- gives more than 1 024."""
    torch = pytest.importorskip("torch")
    seen = {}
    for n in (5000, 30000):
        g = torch.Generator().manual_seed(n)
        scores = torch.randint(0, 7, (6, n), generator=g).float() - 3.0
        scores[0] = 0.0
        scores[1, ::3] = float("-inf")
        vpt = T.route(6, n, 50)[1]["vpt"]
        for k in (1, 50):
            seen[n, k] = [T.fast_path_survivors(scores[r].numpy().view(np.uint32), k, vpt)[1] for r in range(6)]
    assert seen[5000, 1] == seen[5000, 50] == [5000, 497, 774, 693, 664, 761]
    assert seen[30000, 1] == seen[30000, 50] == [30000, 2767, 4270, 4299, 4214, 4227]
    assert [T.emit_branch(s) for s in (497, 774, 2767)] == ["block_rank_desc", "block_sort_desc", "lds_bitonic"]     # one row on the bitonic branch
    g = torch.Generator().manual_seed(27278)
    assert 100 <= T.fast_path_survivors(torch.randn(27278, generator=g).numpy().view(np.uint32), 200, 28)[1] <= 400
    rng = np.random.default_rng(5)
    for n, vpt in ((5000, 8), (49152, 48)):
        logits = (0.1 + 2e-4 * rng.standard_normal(n)).astype(np.float32).view(np.uint32)
        assert T.fast_path_survivors(logits, 200, vpt)[1] > 1024
        assert T.fast_path_survivors(T.narrow(n, 200, rng), 200, vpt) == (T.orderable(np.uint32(0x3DCC0000)) & 0xFFFF0000, n)


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walked():
    """every case's route, tags and traces, computed once"""
    out = {}
    for case in T.CASES:
        out[case.name] = (T.case_route(case),) + T.case_tags(case)
    return out


def test_every_case_takes_the_route_it_is_there_for(walked):
    for case in T.CASES:
        (name, _), _, traces = walked[case.name]
        assert name == case.route, (case.name, name)
        T.check_wants(case, traces)


def test_planted_rows_yield_exactly_their_survivors():
    checked = 0
    for case in T.CASES:
        if case.rows[0][0] != "planted":
            continue
        S, vpt = case.rows[0][1]["S"], T.case_route(case)[1]["vpt"]
        for row in T.case_rows(case):
            assert T.fast_path_survivors(row, case.k, vpt) == (0xC0000000, S), case.name
            assert len(set(T.owner_thread(np.flatnonzero(T.orderable(row) >= 0xC0000000)).tolist())) >= case.k     # spread over at least k threads
            checked += 1
    assert checked >= 2 * 13


def test_the_table_reaches_every_route_and_branch(walked):
    reached = set().union(*(tags for _, tags, _ in walked.values()))
    assert not (T.universe() - reached), "unreached: %s" % sorted(map(str, T.universe() - reached))
    assert not (reached - T.universe()), "a tag the universe does not know: %s" % sorted(map(str, reached - T.universe()))
    entries = {case.entry for case in T.CASES}
    assert entries == {"topk", "topk_filtered", "topk_candidates", "topk_candidates_filtered", "merge", "merge_filtered"}
    for route_name in ("sort_whole", "row_select", "two_level", "radix"):       # every family on every route; a predicate of 0 and of 1
        fams = {(c.rows[0][0], c.rows[0][1].get("where")) for c in T.CASES if c.route == route_name and c.name.startswith("family-")}
        assert fams == {(f, p.get("where")) for f, p in T.EVERY_ROUTE}, route_name
        assert {c.run_if for c in T.CASES if c.route == route_name and c.name.startswith("run-if-")} == {0, 1}
    assert {c.route for c in T.CASES if c.entry == "topk_filtered"} == {"row_select", "two_level"}


def test_no_family_holds_the_excluded_pattern():
    for name, fam in T.FAMILIES.items():
        for n, k in ((1, 1), (2, 2), (65, 7), (5003, 120)):
            if name == "planted":
                continue          # built for the rows of the table (checked there)
            row = fam(n, k, np.random.default_rng(n))
            assert row.dtype == np.uint32 and row.shape == (n,) and not np.any(row == T.EXCLUDED), name
    with pytest.raises(AssertionError):
        T._checked(np.array([0, T.EXCLUDED], dtype=np.uint32))


# ---- the bars can fail ---------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


def test_every_bug_class_changes_an_expected_output():
    """Each mutant must change the expected output of a case; each family must be killed by a mutant that the gauss rows do not kill -- that
    is what the family adds over random rows.  (gauss rows of the table stay off k > n / 2, where random rows would show a wrong order of the
    negatives; `upper_edge` drops the k-th key's own bin, which any row shows.)"""
    mutants = list(T.MUTANTS) + [T.MERGE_MUTANT]
    families = sorted(T.FAMILIES)
    killed = {f: {m: 0 for m in mutants} for f in families}
    cases_hit = {m: set() for m in mutants}
    for case in T.CASES:
        if case.n > 200000:
            continue
        if case.route == "merge":
            msg, R, k = T.case_messages(case), case.R, case.n
            for row in range(msg.shape[1]):
                words = np.concatenate([(msg[r, row, :k] & 0xFFFFFFFF).astype(np.uint32) for r in range(R)])
                if _differs(T.mutant_merge_ties_by_list_index(words, R, k, case.k), T.select(words, case.k)):
                    killed[case.rows[row % len(case.rows)][0]][T.MERGE_MUTANT] += 1
                    cases_hit[T.MERGE_MUTANT].add(case.name)
            continue
        bits = T.case_rows(case)
        for row in range(bits.shape[0]):
            want = T.select(bits[row], case.k)
            for m, fn in T.MUTANTS.items():
                if _differs(fn(bits[row], case.k, case), want):
                    killed[case.rows[row % len(case.rows)][0]][m] += 1
                    cases_hit[m].add(case.name)
    width = max(len(f) for f in families)
    print("\nrows whose expected output a bug class changes (family x mutant):")
    print(" " * width, " ".join("%2d" % i for i in range(len(mutants))), "   " + ", ".join("%d=%s" % (i, m) for i, m in enumerate(mutants)))
    for f in families:
        print(f.ljust(width), " ".join("%2s" % (killed[f][m] if killed[f][m] < 100 else "99") if killed[f][m] else " ." for m in mutants))
    for m in mutants:
        assert cases_hit[m], "no case notices the bug class " + m
    beyond_gauss = [m for m in mutants if not killed["gauss"][m]]
    for f in families:
        if f != "gauss":
            assert any(killed[f][m] for m in beyond_gauss), "the family %s adds nothing over gauss rows" % f
