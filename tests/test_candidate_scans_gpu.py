"""The bf16 candidate scans (rails_amd/csrc/mol_coarse.hip) and the selection kernels only they reach (topk.hip: row_select on a bf16
source, bf16_rows_kth, sublist_select, sublist_rank), through MolEngine, against tests/_scan_ref.py -- integers and float64, no kernel of
this project:

  a. scores on dyadic inputs, where the fp32 accumulator is exact in any order: bit for bit
  b. scores on random unit-norm inputs: inside the admissible interval of the float64 sum
  c. the table builds: bit for bit
  d. the fused top-k at the smallest corpora its plans accept: the header's contract row by row, the reference being the key selection

tests/test_candidate_scans_cpu.py shows that both bars reject every bug class they are meant for, on these very inputs.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from tests import _scan_ref as S

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def E():
    from rails_amd import engine

    return engine


def cfg_of(shape):
    return O.CONFIGS[S.SHAPES[shape][0]]


@functools.lru_cache(maxsize=None)
def weights(shape):
    return O.synthetic_weights(cfg_of(shape), seed=2)


@functools.lru_cache(maxsize=None)
def engine(shape, precision="fp32"):
    cfg = cfg_of(shape)
    names = {f.name for f in dataclasses.fields(E().MolShapeSpec)}
    spec = E().MolShapeSpec(**{k: v for k, v in dataclasses.asdict(cfg).items() if k in names})
    return E().MolEngine(spec, {k: v.to(dev()) for k, v in weights(shape).items()}, precision=precision)


def module_of(shape):
    cfg = cfg_of(shape)
    mol, _ = rails_amd.create_mol_interaction_module(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
        cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
        cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
        query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None,
    )
    mol.load_state_dict(weights(shape), strict=True)
    return mol.to(dev()).eval()


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def table_dev(table):
    """fp32 holding bf16 values -> the bf16 tensor the entry points take (an exact conversion)"""
    assert S.is_bf16(table).all()
    return torch.from_numpy(np.ascontiguousarray(table)).bfloat16().to(dev())


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def scores_of(eng, entry, eq, table, avg=False, out=None, run_if=None):
    if entry == "coarse":
        return eng.coarse_scores(eq, table, avg, out=out, run_if=run_if)
    return eng.component_scores(eq, table, out=out, run_if=run_if)


def user_ids(shape, B):
    return torch.arange(B, dtype=torch.int64, device=dev()) * 7 + 1 if len(cfg_of(shape).uid_embedding_hash_sizes) > 0 else None


# ---- a. scores on dyadic inputs ------------------------------------------------------------------------------------------------
def check_dyadic_scores(case):
    """every column below N written with bf16(S), bit for bit; no column at or past N touched (ld = N + 5, NaN-filled buffer)"""
    eng = engine(case.shape)
    eq, table = S.dyadic_inputs(case)
    eq_d, table_d = to_dev(eq), table_dev(table)
    for avg in S.modes(case):
        ref = torch.from_numpy(S.rounded(S.model(case, eq, table, avg)[0]))
        assert bool(torch.isfinite(ref).all())
        buf = torch.full((ref.shape[0], case.N + 5), float("nan"), dtype=torch.float32, device=dev())
        scores_of(eng, case.entry, eq_d, table_d, avg, out=buf[:, :case.N])
        got = buf.cpu()
        assert bool(torch.isnan(got[:, case.N:]).all()), (case, avg)
        assert same_bits(got[:, :case.N], ref), (case, avg, int((bits(got[:, :case.N]) != bits(ref)).sum()))


SCORE_GROUPS = sorted({(c.entry, c.shape, c.B) for c in S.SCORE_CASES if c not in S.MULTI_TRIP})


@pytest.mark.parametrize("entry,shape,B", SCORE_GROUPS, ids=lambda v: str(v))
def test_scores_on_dyadic_inputs_bit_for_bit(entry, shape, B):
    """coarse B in {1, 5, 32, 33, 128} (1 to 4 query tiles, both average_queries values), component B * P_Q in {8 | 16, 40 | 48, 256 | 128};
    N in {1, 31, 32, 33, 1000}"""
    cases = [c for c in S.SCORE_CASES if (c.entry, c.shape, c.B) == (entry, shape, B) and c not in S.MULTI_TRIP]
    assert [c.N for c in cases] == list(S.SCORE_N)
    for case in cases:
        check_dyadic_scores(case)


@pytest.mark.parametrize("case", S.MULTI_TRIP, ids=lambda c: f"{c.entry}-{c.N}")
def test_scores_where_a_wave_takes_several_trips(case):
    check_dyadic_scores(case)


@pytest.mark.parametrize("entry", ["coarse", "component"])
def test_scores_run_if_predicate(entry):
    """a device word of 0 leaves the buffer untouched, 1 writes it"""
    case = S.ScoreCase(entry, "8x4x64", 5, 33)
    eng = engine(case.shape)
    eq, table = S.dyadic_inputs(case)
    ref = torch.from_numpy(S.rounded(S.model(case, eq, table, False)[0]))
    for word in (0, 1):
        buf = torch.full((ref.shape[0], case.N + 5), float("nan"), dtype=torch.float32, device=dev())
        scores_of(eng, entry, to_dev(eq), table_dev(table), False, out=buf[:, :case.N], run_if=torch.full((1,), word, dtype=torch.int32, device=dev()))
        got = buf.cpu()
        assert bool(torch.isnan(got[:, case.N:]).all())
        assert same_bits(got[:, :case.N], ref) if word else bool(torch.isnan(got).all())


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_one_size_past_each_documented_limit(shape):
    """The fused coarse top-K' takes B <= 128 and the fused component top-k B * P_Q <= 256 (128 at d = 128): one query more, resp. one query
    tile more, and the entry point returns None (a zero workspace size: "unsupported", nothing launched).  The materialising scans keep the
    queries' fragments in LDS (96 KiB): past that they raise NotImplementedError."""
    eng = engine(shape)
    _, pq, px, d = S.SHAPES[shape]
    rng = np.random.default_rng(7)
    n, k = 4000, 100
    coarse_t, comp_t = table_dev(S.dyadic_rows(rng, n, d)), table_dev(S.dyadic_rows(rng, px * n, d).reshape(px, n, d))
    assert eng.coarse_topk(to_dev(S.dyadic_eq(rng, 128, pq, d)), coarse_t, False, k) is not None
    assert eng.coarse_topk(to_dev(S.dyadic_eq(rng, 129, pq, d)), coarse_t, False, k) is None
    limit = 128 if d == 128 else 256
    assert eng.component_topk(to_dev(S.dyadic_eq(rng, limit // pq, pq, d)), comp_t, k) is not None
    assert eng.component_topk(to_dev(S.dyadic_eq(rng, (limit + 32) // pq, pq, d)), comp_t, k) is None
    rows_over = (96 * 1024) // (2 * d * 32) * 32 + 1       # query rows whose fragments alone pass 96 KiB
    with pytest.raises(NotImplementedError, match="do not fit LDS"):
        eng.coarse_scores(to_dev(S.dyadic_eq(rng, rows_over, pq, d)), coarse_t, False)
    with pytest.raises(NotImplementedError, match="do not fit LDS"):
        eng.component_scores(to_dev(S.dyadic_eq(rng, -(-rows_over // pq), pq, d)), comp_t)
    torch.cuda.synchronize()


# ---- b. scores on random unit-norm inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.RANDOM_CASES, ids=lambda c: f"{c.entry}-{c.shape}")
def test_scores_on_random_inputs_are_admissible(case):
    """B = 33, N = 4 000: every entry is a bf16 number inside [bf16(S - e), bf16(S + e)]; the share equal to bf16(S) is printed"""
    eng = engine(case.shape)
    eq, table = S.random_inputs(case)
    d = case.dims[2]
    eq_d, table_d = to_dev(eq), table_dev(table)
    for avg in S.modes(case):
        got = scores_of(eng, case.entry, eq_d, table_d, avg).cpu().numpy()
        assert S.is_bf16(got).all()
        equal = 0
        for c0 in range(0, case.N, 1000):
            s, a = S.model(case, eq, table[..., c0:c0 + 1000, :], avg, want_abs=True)
            lo, hi = S.admissible(s, a, d)
            g = got[:, c0:c0 + 1000]
            bad = ~S.passes(g, lo, hi)
            assert not bad.any(), (case, avg, int(bad.sum()), float(np.abs(g - s)[bad].max()))
            equal += int((g == S.rounded(s)).sum())
        print(f"{case.entry} {case.shape} average_queries={avg}: share of entries equal to bf16(S) {equal / got.size:.6f}")


# ---- c. table builds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_table_builds_bit_for_bit(shape):
    """Ex read back from the fp32 engine's index (the unpack call); build_coarse_table and build_component_table equal the restatement
    on it for N in {1, 33, 4 001}; the f16x3 engine's tables, cut from `items`, equal the fp32 engine's at N = 4 001."""
    eng = engine(shape)
    cfg = cfg_of(shape)
    for n in (1, 33, 4001):
        items = torch.from_numpy(O.hash_item_table(11, 0, n, cfg.item_embedding_dim)).to(dev())
        index = eng.build_index(items)
        ex = eng.unpack_index(index, want_gi=False)[0].cpu().numpy()
        coarse, comp = eng.build_coarse_table(index), eng.build_component_table(index)
        assert coarse.dtype == torch.bfloat16 and comp.dtype == torch.bfloat16
        assert same_bits(coarse.float().cpu(), torch.from_numpy(S.coarse_table(ex))), n
        assert same_bits(comp.float().cpu(), torch.from_numpy(S.component_table(ex))), n
        if n == 4001:
            e16 = engine(shape, "f16x3")
            i16 = e16.build_index(items)
            assert torch.equal(e16.build_coarse_table(i16, items).view(torch.int16), coarse.view(torch.int16))
            assert torch.equal(e16.build_component_table(i16, items).view(torch.int16), comp.view(torch.int16))


# ---- d. the fused top-k ------------------------------------------------------------------------------------------------------------
def fused(eng, entry, eq_d, table_d, k, avg=False, prefilter=None):
    """-> scores, positions, counts (CPU), flag, capacity"""
    B, n = eq_d.shape[0], table_d.shape[-2]
    if entry == "coarse":
        out = eng.coarse_topk(eq_d, table_d, avg, k, with_flag=True, prefilter=prefilter)
        cap = eng.coarse_topk_capacity(k, n, B)
        assert out is not None and cap > 0, (B, n, k)
        fs, fp, counts, flag = out
    else:
        flag = torch.ones(1, dtype=torch.int32, device=dev())      # zeroed by the call
        out = eng.component_topk(eq_d, table_d, k, flag)
        cap = eng.component_topk_capacity(B, n, k)
        assert out is not None and cap > 0, (B, n, k)
        fs, fp, counts = out
    return fs.cpu(), fp.cpu(), counts.cpu(), int(flag.item()), cap


def check_contract(got, ref_s, ref_p, k):
    """The header's contract: the flag is "some row's count left [k, capacity]", exactly; every row inside equals the reference's key
    top-k bit for bit.  -> the rows inside."""
    fs, fp, counts, flag, cap = got
    ok = (counts >= k) & (counts <= cap)
    assert flag == int(not bool(ok.all())), (flag, int(counts.min()), int(counts.max()), cap)
    assert same_bits(fs[ok], ref_s[ok]), int((bits(fs[ok]) != bits(ref_s[ok])).sum())
    assert torch.equal(fp[ok], ref_p[ok])
    return ok


def ref_topk(scores_of_rows, rows, k, step=512):
    """the key selection over (rows, n) fp32 scores delivered in blocks of rows"""
    parts = [S.topk_keys(scores_of_rows(r0, min(r0 + step, rows)), k) for r0 in range(0, rows, step)]
    return torch.from_numpy(np.concatenate([p[0] for p in parts])), torch.from_numpy(np.concatenate([p[1] for p in parts]))


def rows_per_query(case_or_entry, shape):
    _, pq, px, _ = S.SHAPES[shape]
    return 1 if case_or_entry == "coarse" else pq * px


def exact_ref_topk(case, eq, table, avg):
    per = rows_per_query(case.entry, case.shape)
    bstep = max(1, 512 // per)

    def block(r0, r1):
        b0, b1 = r0 // per, r1 // per
        return S.select_scores(case._replace(B=b1 - b0), eq[b0:b1], table, avg)
    return ref_topk(block, case.B * per, case.k, step=bstep * per)


RANDOM_TOPK = [("coarse", s, n, k, None) for s in S.SHAPES for n, k in S.COARSE_TOPK_SIZES] + \
    [("component", s, n, k, w) for s in S.SHAPES for n, k in S.COMPONENT_TOPK_SIZES for w in (0, 1)]


@pytest.mark.parametrize("entry,shape,n,k,which", RANDOM_TOPK, ids=lambda v: str(v))
def test_fused_topk_on_random_inputs(entry, shape, n, k, which):
    """(i) Unit-norm Eq from the query prologue, tables built from a hashed item table.  The float64 sum of such operands does not fix the
    bf16 score of every item (test b: a few per cent have two admissible values), so the reference's own count of items at or above the
    call's threshold cannot be known: the test asserts flag == 0 and every count inside [k, capacity] -- it cannot pass vacuously -- and
    then (1) the key selection (numpy) over the materialised scores returns the fused call's scores and positions bit for bit, (2) every
    returned score is admissible for the float64 sum at its position.  The int8 pre-filter returns the same scores, positions and counts."""
    eng = engine(shape)
    cfg = cfg_of(shape)
    _, pq, px, d = S.SHAPES[shape]
    items = torch.from_numpy(O.hash_item_table(13, 0, n, cfg.item_embedding_dim)).to(dev())
    index = eng.build_index(items)
    table_d = eng.build_coarse_table(index) if entry == "coarse" else eng.build_component_table(index)
    table = table_d.float().cpu().numpy()
    for B in (S.COARSE_TOPK_BATCHES if entry == "coarse" else (S.component_topk_batches(shape)[which],)):
        q = O.synthetic_queries(cfg, B, seed=4 + B).to(dev())
        _, eq_d, _ = eng.query_pack(q, user_ids(shape, B), want_plain=True)
        eq = eq_d.cpu().numpy()
        for avg in ((False, True) if entry == "coarse" else (False,)):
            got = fused(eng, entry, eq_d, table_d, k, avg)
            fs, fp, counts, flag, cap = got
            assert flag == 0 and int(counts.min()) >= k and int(counts.max()) <= cap, (flag, int(counts.min()), int(counts.max()), cap)
            ms = scores_of(eng, entry, eq_d, table_d, avg).cpu().numpy()
            ref_s, ref_p = ref_topk(lambda r0, r1: ms[r0:r1], ms.shape[0], k)
            assert bool(check_contract(got, ref_s, ref_p, k).all())
            # the returned scores against float64 at the returned positions
            qrows = (S.coarse_query(eq, avg) if entry == "coarse" else S.component_query(eq)).astype(np.float64)
            pos, per = fp.numpy(), rows_per_query(entry, shape)
            for r0 in range(0, pos.shape[0], 256):
                r = np.arange(r0, min(r0 + 256, pos.shape[0]))
                rows_t = (table[pos[r]] if entry == "coarse" else table[(r % px)[:, None], pos[r]]).astype(np.float64)      # (rows, k, d)
                qq = qrows[r // per if entry == "coarse" else r // px][:, None, :]
                s, a = (qq * rows_t).sum(-1), (np.abs(qq) * np.abs(rows_t)).sum(-1)
                lo, hi = S.admissible(s, a, d)
                assert S.passes(fs.numpy()[r], lo, hi).all()
            if entry == "coarse":
                pre = eng.build_coarse_prefilter(table_d)
                assert pre is not None
                ps, pp, pc, pflag, _ = fused(eng, entry, eq_d, table_d, k, avg, prefilter=pre)
                assert same_bits(ps, fs) and torch.equal(pp, fp) and torch.equal(pc, counts) and pflag == 0


@pytest.mark.parametrize("case", S.select_cases(), ids=lambda c: f"{c.entry}-{c.shape}-B{c.B}-N{c.N}-k{c.k}-{c.kind}")
def test_fused_topk_contract_on_exact_inputs(case):
    """(ii) dups: many distinct dyadic values and planted duplicates across the k-th place -- the tie rule decides membership and order.
    (iii) front / last_class: the winners at positions 0 .. k - 1, resp. in the ragged last tile and the tiles of its residue class mod 16.
    (iv) few: all items tied at one or two scores, so that the counts exceed the capacity (or, below 4 096 items, a sub-list's share of it)
    and the flag is raised.
    Whatever the counts say, the contract holds: the flag is exact, and every row inside [k, capacity] equals the key top-k of the exact
    scores bit for bit.  With the int8 pre-filter the same contract holds; its sub-lists are taken by tile, not by workgroup, so a row
    can overflow in one scan and not in the other -- where both are inside, the counts agree."""
    eng = engine(case.shape)
    eq, table, n = S.select_inputs(case)
    eq_d, table_d = to_dev(eq), table_dev(table)
    for avg in ((False, True) if case.entry == "coarse" else (False,)):
        ref_s, ref_p = exact_ref_topk(case, eq, table, avg)
        got = fused(eng, case.entry, eq_d, table_d, case.k, avg)
        ok = check_contract(got, ref_s, ref_p, case.k)
        if case.kind == "few":
            assert got[3] == 1 and not bool(ok.any()), (int(got[2].min()), got[4])
        if case.kind == "dups":
            assert bool(ok.all()), (int(got[2].min()), int(got[2].max()), got[4])      # ordinary data: nothing to fall back for
        if case.entry == "coarse":
            pre = eng.build_coarse_prefilter(table_d)
            assert pre is not None
            pgot = fused(eng, case.entry, eq_d, table_d, case.k, avg, prefilter=pre)
            pok = check_contract(pgot, ref_s, ref_p, case.k)
            both = ok & pok
            assert torch.equal(pgot[2][both], got[2][both])


def test_modules_fall_back_on_heavy_ties_at_small_sizes():
    """(iv) through MoLAvgTopK, MoLNaiveTopK and MoLCombTopK with the fused paths switched on for any corpus size: a corpus of 30 000 copies
    of two items overflows every candidate list (the flag is raised, asserted on the engine call), and the modules return what they
    return with the fused paths switched off, bit for bit."""
    shape = "8x8x32"
    cfg = cfg_of(shape)
    mol = module_of(shape)
    n, B = 30_000, 8
    base = torch.from_numpy(O.hash_item_table(6, 0, 2, cfg.item_embedding_dim))
    X = base[torch.arange(n) % 2].unsqueeze(0).to(dev())
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev()).unsqueeze(0)
    q = O.synthetic_queries(cfg, B, seed=4).to(dev())
    with torch.inference_mode():
        mods = [rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=1000), rails_amd.MoLNaiveTopK(mol, X, ids, k_per_group=100),
                rails_amd.MoLCombTopK(mol, X, ids, avg_top_k=1000, k_per_group=100)]
        eng = mods[0]._bind()
        _, eq_d, _ = eng.query_pack(q, None, want_plain=True)
        assert fused(eng, "coarse", eq_d, mods[0]._table(), 1000)[3] == 1
        assert fused(mods[1]._bind(), "component", eq_d, mods[1]._component_table(), 100)[3] == 1
        for mod in mods:
            mod.fused_coarse_min_items = 0
            mod.fused_component_min_items = 0
            s1, i1 = mod(q, k=50)
            mod.fused_coarse_min_items = 1 << 62
            mod.fused_component_min_items = 1 << 62
            s2, i2 = mod(q, k=50)
            assert same_bits(s1, s2) and torch.equal(i1, i2), type(mod).__name__


@pytest.mark.parametrize("entry", ["coarse", "component"])
def test_fused_topk_with_inf_and_nan_scores(entry):
    """(v) One table row and two queries scaled so that their scores overflow to +inf and -inf; two NaN table rows (sign bit clear, sign
    bit set); and one row whose products with the two scaled queries overflow with both signs, so that inf - inf makes a NaN inside the
    matrix unit.

    What the code says: the select scan keeps a score iff `sc >= thr` (coarse_scan_kernel) -- +inf passes, -inf passes only a threshold of
    -inf, NaN never passes; the sample's running maxima are taken with fmaxf, which drops NaN, so thresholds are never NaN.  make_key
    orders a NaN with the sign bit clear above +inf and one with the sign bit set below -inf, and that is where rails_topk over the
    materialised scores puts them.  So the two paths can differ only in a NaN score whose sign bit is clear.

    What the MI355X does: every NaN the bf16 matrix unit returns -- from a NaN operand of either sign, and from inf - inf among the
    products -- is the one pattern 0xFFC00000, sign bit set (bf16_rn keeps it as is).  Under the key codec that lies below -inf: the
    materialised top-k ranks such items last, the fused scan never collects them, and with k finite scores in the row neither path names
    them.  +inf scores are collected and ranked first by both, -inf scores last.  The counts stay inside [k, capacity], the flag stays 0,
    and the int8 pre-filter (whose statistics drop NaN and whose scale the 2^110 row sets, so that every tile is scored from the bf16 table)
    returns the same.  No kernel change was needed.

    Asserted: every row whose count is inside [k, capacity] equals coarse_scores / component_scores + rails_topk bit for bit (NaN
    patterns included), and the flag says exactly whether a row is outside -- the fused result is never silently different.  The int8
    pre-filter is held to the same.  The NaN patterns met are printed."""
    shape, n, k = "8x8x32", 4000, 100
    _, pq, px, d = S.SHAPES[shape]
    B = 33 if entry == "coarse" else 256 // pq
    eng = engine(shape)
    rng = np.random.default_rng(17)
    eq = S.dyadic_eq(rng, B, pq, d)
    g = 1 if entry == "coarse" else px
    t = S.dyadic_rows(rng, g * n, d).reshape(g, n, d)
    sign = np.where(rng.integers(0, 2, size=d) > 0, 1.0, -1.0).astype(np.float32)
    x_inf, x_nan, x_nneg, x_mix = 1234, 777, 2025, 3999
    t[:, x_inf] = sign * np.float32(2.0 ** 101)
    t[:, x_mix] = sign * np.where(np.arange(d) % 2 == 0, 1.0, -1.0).astype(np.float32) * np.float32(2.0 ** 110)      # products of both signs overflow
    big = np.float32(2.0 ** 20) if entry == "coarse" else np.float32(2.0 ** 26)      # coarse: summed over the 8 query groups
    eq[2] = sign * big
    eq[3] = -sign * big
    eq_d = to_dev(eq)
    table_d = torch.from_numpy(np.ascontiguousarray(t[0] if g == 1 else t)).bfloat16().to(dev())
    table_d.view(torch.int16)[..., x_nan, :] = 0x7FC0             # quiet NaN, sign bit clear
    table_d.view(torch.int16)[..., x_nneg, :] = 0xFFC0 - 0x10000  # quiet NaN, sign bit set
    per = rows_per_query(entry, shape)
    for avg in ((False, True) if entry == "coarse" else (False,)):
        ms = scores_of(eng, entry, eq_d, table_d, avg)
        rs, rp = E().topk(ms, k)
        ms, rs, rp = ms.cpu(), rs.cpu(), rp.cpu()
        assert bool(torch.isnan(ms[:, x_nan]).all()) and bool(torch.isnan(ms[:, x_nneg]).all())
        assert bool(torch.isnan(ms[2 * per:4 * per, x_mix]).all()) and bool(torch.isfinite(ms[4 * per:, x_mix]).all())
        if not avg:      # (the averaged query is eight times smaller: those two scores stay finite)
            assert float(ms[2 * per, x_inf]) == float("inf") and float(ms[3 * per, x_inf]) == float("-inf")
        nan = torch.isnan(ms)
        print(f"{entry} average_queries={avg}: NaN scores {int(nan.sum())}, of them with the sign bit set {int((bits(ms)[nan] < 0).sum())}; "
              f"patterns {sorted({hex(v & 0xFFFFFFFF) for v in bits(ms)[nan].tolist()})}; "
              f"rows whose materialised top-k holds a NaN item {int(torch.isnan(rs).any(1).sum())} of {rp.shape[0]}")
        got = fused(eng, entry, eq_d, table_d, k, avg)
        ok = check_contract(got, rs, rp, k)
        print(f"  fused: flag {got[3]}, rows inside [k, capacity] {int(ok.sum())} of {ok.numel()}, rows naming a NaN item {int(torch.isnan(got[0]).any(1).sum())}")
        if entry == "coarse":
            pre = eng.build_coarse_prefilter(table_d)
            pgot = fused(eng, entry, eq_d, table_d, k, avg, prefilter=pre)
            pok = check_contract(pgot, rs, rp, k)
            print(f"  int8 pre-filter: flag {pgot[3]}, rows inside {int(pok.sum())} of {pok.numel()}")
