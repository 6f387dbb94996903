"""SASRec multi-row cached decode step on the GPU (encode with cache= and new_rows=, rails_sasrec_decode_rows): one step from the
fixture chains' state 0 straight to state 3 agrees with the REFERENCE, with float64 and with the full encode at the bars of the
single-row tests; it is bit for bit M single-row steps, output and cache; a cache of NaN filled from nothing is a prefill; the cache
gains exactly rows [len - m, len); the shapes at which work-row slots can go wrong; the equivalent spellings of new_rows; an interior
edit; validation on the host and clamping on the device; the kernels' limits."""
import functools

import pytest
import torch

from tests import _sasrec_append_ref as A
from tests import _sasrec_decode_ref as R
from tests import _sasrec_ref as S
from tests.test_sasrec import build, tolerance
from tests.test_sasrec_decode_gpu import SHAPES, _module, _sequences, dev, full, prefill, step

pytestmark = pytest.mark.gpu


def rows(m, lengths, ids, cache, new_rows, **kw):
    d = dev()
    with torch.inference_mode():
        return m.encode(lengths, ids.to(d), m.get_item_embeddings(ids.to(d)), {}, cache=cache, new_rows=new_rows, **kw)


def clone(cache):
    return [(k.clone(), v.clone()) for k, v in cache]


def same(c1, c2):
    return all(torch.equal(a, b) for p, q in zip(c1, c2) for a, b in zip(p, q))


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(fixture, module, the cache of chain state 0, the step to state 3): made once; tests step on clones of the cache."""
    f = R.load(name)
    m = build(f, dev())
    _, cache = prefill(m, torch.from_numpy(f["chain/lengths"][0]), torch.from_numpy(f["chain/ids"][0]))
    return f, m, cache, A.fixture_step(f)


@functools.lru_cache(maxsize=None)
def chain64(name):
    return R.chain64(R.load(name))


def new_mask(lengths, counts, N):
    """(B, N) bool: rows [len - m, len)."""
    return (torch.arange(N) >= (lengths - counts).unsqueeze(1)) & (torch.arange(N) < lengths.unsqueeze(1))


def assert_is_single_steps(m, lengths, ids, counts, cache0):
    """The multi-row step equals, bit for bit in the output and in every cache tensor, one single-row step per new row."""
    c1, c2 = clone(cache0), clone(cache0)
    out = rows(m, lengths, ids, c1, counts)
    for L in A.single_steps(lengths, counts):
        one = step(m, L, ids, c2)
    assert torch.equal(out, one)
    assert same(c1, c2)
    return out, c1


# ---- 1. the reference chains -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.GEOMETRIES)
def test_one_step_over_the_chain_matches_the_reference_float64_and_a_full_encode(name):
    f, m, cache0, (L3, I3, counts) = fixture(name)
    tol = tolerance(f)
    cur = rows(m, L3, I3, clone(cache0), counts).cpu().double()
    d64, dref = R.distance(cur, chain64(name)[3]), R.distance(cur, torch.from_numpy(f["chain/out"][3]))
    denc = R.distance(cur, full(m, L3, I3).cpu())
    assert d64 <= tol, (d64, tol)
    assert dref <= 2 * tol, (dref, tol)
    assert denc <= tol, (denc, tol)


# ---- 2. bit-equality with single-row steps -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.GEOMETRIES)
def test_one_step_is_bitwise_the_single_row_steps(name):
    _, m, cache0, (L3, I3, counts) = fixture(name)
    assert_is_single_steps(m, L3, I3, counts, cache0)


# ---- 3. from nothing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.GEOMETRIES)
def test_every_row_new_on_a_cache_of_nan_is_a_prefill(name):
    f, m, cache0, _ = fixture(name)
    L, I = torch.from_numpy(f["chain/lengths"][0]), torch.from_numpy(f["chain/ids"][0])
    B, N = I.shape
    cache = [(torch.full_like(k, float("nan")), torch.full_like(v, float("nan"))) for k, v in cache0]
    cur = rows(m, L, I, cache, L)
    tol = tolerance(f)
    assert R.distance(cur.cpu(), full(m, L, I).cpu()) <= tol
    assert R.distance(cur.cpu(), full(m, L, I, fused=False).cpu()) <= tol      # the prefill's own result
    _, cache64 = R.prefill64(f, L, I)
    used = torch.arange(N) < L.unsqueeze(1)
    for (k, v), (k64, v64) in zip(cache, cache64):
        for t, t64 in ((k.cpu(), k64), (v.cpu(), v64)):
            assert R.distance(t[used], t64[used]) <= tol * (1.0 + float(t64.abs().max())), name
            assert bool(torch.isnan(t[~used]).all())


# ---- 4. the cache gains exactly those rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["amzn-books-gelu", "ml-20m"])
def test_cache_gains_the_new_rows_and_nothing_else(name):
    f, m, cache0, (L3, I3, counts) = fixture(name)
    B, N = I3.shape
    cache = clone(cache0)
    past = (torch.arange(N) >= L3.unsqueeze(1)).to(dev())
    g = torch.Generator(device=dev()).manual_seed(5)
    for t in (t for kv in cache for t in kv):      # rows >= len are never read: random numbers there show any write
        t[past] = torch.randn(t[past].shape, generator=g, device=dev())
    before = clone(cache)
    out, got = rows(m, L3, I3, cache, counts, return_cache_states=True)
    assert got is cache
    _, fresh = prefill(m, L3, I3)
    new = new_mask(L3, counts, N)
    tol = tolerance(f)
    for (k, v), (k0, v0), (kf, vf) in zip(cache, before, fresh):
        for t, t0, tf in ((k, k0, kf), (v, v0, vf)):
            t, t0, tf = t.cpu(), t0.cpu(), tf.cpu()
            assert torch.equal(t[~new], t0[~new])
            assert R.distance(t[new], tf[new]) <= tol * (1.0 + float(tf[new].abs().max()))


# ---- 5. the smallest shapes at which the slot scheme can go wrong ------------------------------------------------------------
def _edit(lengths, ids, counts, items, seed=2):
    """New ids at rows [len - m, len) of every sequence."""
    g = torch.Generator().manual_seed(seed)
    ids = ids.clone()
    mask = new_mask(lengths, counts, ids.shape[1])
    ids[mask] = torch.randint(1, items + 1, (int(mask.sum()),), generator=g)
    return ids


def _case(name):
    """(shape name, lengths before, lengths after, counts, new_rows argument, [(sequence, row)] given id 0)."""
    if name == "b5_m7_straddles_a_tile":     # 35 slots; sequence 4's slots 28 .. 34 cross the 32-row tile; counts hold 1 and M = 7;
        after = torch.tensor([40, 12, 9, 7, 20])          # m_b = len_b (sequence 3) beside m_b = 1 (sequence 1)
        counts = torch.tensor([7, 1, 3, 7, 5])
        return "hd8", after - counts + (counts == after), after, counts, counts, [(0, 36), (4, 16)]
    if name == "n512_rows_past_256":         # the attention loop strides: 256 threads, keys 0 .. p > 256
        after = torch.tensor([512, 300, 260])
        counts = torch.tensor([4, 2, 3])
        return "n512", after - counts, after, counts, counts, [(1, 298)]
    shape = name[:-3]                        # "<shape>_m2": two rows everywhere (an int: no count array)
    B, N = SHAPES[shape][:2]
    before, _ = _sequences(B, N, 500)
    after = torch.clamp(before + 2, max=N)   # a sequence at N has its last two rows replaced
    return shape, before, after, torch.full((B,), 2), 2, [(B // 2, int(after[B // 2]) - 2)]


CASES = ["b5_m7_straddles_a_tile", "n512_rows_past_256", "hd16_m2", "hd50_d_not_mult_4_m2", "hd64_m2", "odd_dims_m2", "b257_m2"]


@pytest.mark.parametrize("case", CASES)
def test_slot_shapes(case):
    """Against float64 and the module's full encode at test_shapes_beyond_the_fixtures' bar, 2 d(full encode, float64) + 2e-5, and
    bit for bit the single-row steps."""
    shape, before, after, counts, arg, zeros = _case(case)
    B, N, D, H, F, blocks, act, post = SHAPES[shape]
    m = _module(N, D, H, F, blocks, act, post)
    ids0 = torch.randint(1, 501, (B, N), generator=torch.Generator().manual_seed(1)) * (torch.arange(N).unsqueeze(0) < before.unsqueeze(1))
    _, cache0 = prefill(m, before, ids0)
    ids = _edit(after, ids0, counts, 500)
    for b, p in zeros:                       # a new row with id 0: masked to zero, still a key of the rows after it
        assert after[b] - counts[b] <= p < after[b] - 1
        ids[b, p] = 0
    out, cache = assert_is_single_steps(m, after, ids, counts, cache0)
    if not isinstance(arg, torch.Tensor):
        c2 = clone(cache0)
        assert torch.equal(rows(m, after, ids, c2, arg), out) and same(c2, cache)
    cur = out.cpu().double()
    enc = full(m, after, ids).cpu().double()
    fx = S.from_model(m, after, ids, dict(N=N, D=D, heads=H, blocks=blocks, act=act, postproc=post))
    cur64 = S.encoder64(fx, ids=ids, lengths=after)[1]
    bar = 2.0 * R.distance(enc, cur64) + 2e-5
    assert R.distance(cur, cur64) <= bar, (R.distance(cur, cur64), bar)
    assert R.distance(cur, enc) <= bar, (R.distance(cur, enc), bar)


# ---- 6. equivalent spellings -------------------------------------------------------------------------------------------------
def test_equivalent_spellings_change_no_bit():
    B, N, D, H, F, blocks, act, post = SHAPES["hd8"]
    m = _module(N, D, H, F, blocks, act, post)
    lengths = torch.tensor([40, 12, 9, 7, 20])
    ids0 = torch.randint(1, 501, (B, N), generator=torch.Generator().manual_seed(1)) * (torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1))
    _, cache0 = prefill(m, lengths, ids0)

    def run(ids, new_rows, **kw):
        c = clone(cache0)
        return rows(m, lengths, ids, c, new_rows, **kw), c

    def equal(a, b):
        return torch.equal(a[0], b[0]) and same(a[1], b[1])

    three = torch.full((B,), 3)
    ids = _edit(lengths, ids0, three, 500)
    by_int = run(ids, 3)
    assert equal(by_int, run(ids, three)) and equal(by_int, run(ids, [3] * B)) and equal(by_int, run(ids, three.int()))
    ids = _edit(lengths, ids0, torch.ones(B, dtype=torch.int64), 500)
    c = clone(cache0)
    assert equal(run(ids, 1), (step(m, lengths, ids, c), c))
    counts = torch.tensor([7, 1, 3, 7, 5])
    ids = _edit(lengths, ids0, counts, 500)
    host = run(ids, counts)
    assert equal(host, run(ids, counts.to(dev()), max_new_rows=7))
    assert equal(host, run(ids, counts, max_new_rows=10)) and equal(host, run(ids, counts.to(dev()), max_new_rows=10))
    assert equal(host, run(ids, counts.tolist(), max_new_rows=N))
    assert equal(by_int, run(_edit(lengths, ids0, three, 500), 3, max_new_rows=4))


# ---- 7. interior edit --------------------------------------------------------------------------------------------------------
def test_interior_edit():
    """The id at a row p < len - 1 changes; new_rows = len - p with the lengths unchanged re-encodes the rows from p on."""
    f = R.load("amzn-books")
    m = build(f, dev())
    L, I = torch.from_numpy(f["chain/lengths"][3]), torch.from_numpy(f["chain/ids"][3])
    _, cache = prefill(m, L, I)
    p = torch.clamp(L - 5, min=0)                     # len 4: row 0; len 51: row 46
    assert bool((p < L - 1).all())
    I2 = I.clone()
    I2[torch.arange(I.shape[0]), p] = (I[torch.arange(I.shape[0]), p] + 17) % f["cfg"]["num_items"] + 1
    cur = rows(m, L, I2, cache, L - p).cpu()
    tol = tolerance(f)
    assert R.distance(cur, S.encoder64(f, ids=I2, lengths=L)[1]) <= tol
    assert R.distance(cur, full(m, L, I2).cpu()) <= tol
    assert R.distance(cur, full(m, L, I).cpu()) > 10 * tol          # the edit is visible at this bar
    _, fresh = prefill(m, L, I2)
    used = torch.arange(I.shape[1]) < L.unsqueeze(1)     # rows >= len belong to no decode step (the fixture has ids there)
    for (k, v), (kf, vf) in zip(cache, fresh):
        for t, tf in ((k.cpu(), kf.cpu()), (v.cpu(), vf.cpu())):
            assert R.distance(t[used], tf[used]) <= tol * (1.0 + float(tf[used].abs().max()))


# ---- 8. validation -----------------------------------------------------------------------------------------------------------
def test_bad_new_rows_raise_with_the_cache_untouched():
    _, m, cache0, (L3, I3, counts) = fixture("amzn-books")
    B = I3.shape[0]
    cache = clone(cache0)
    zero, over = counts.clone(), counts.clone()
    zero[3] = 0
    over[1] = L3[1] + 1
    for bad, kw in [(zero, {}), (over, {}), (0, {}), (int(L3.min()) + 1, {}), (counts[:-1], {}), (counts.unsqueeze(0), {}), (counts.double(), {}),
                    (counts.to(dev()), {}), (counts.to(dev()).float(), dict(max_new_rows=3)), (counts.to(dev())[:-1], dict(max_new_rows=3)),
                    (counts, dict(max_new_rows=2)), (counts, dict(max_new_rows=0))]:
        with pytest.raises(ValueError, match="new_rows"):
            rows(m, L3, I3, cache, bad, **kw)
    d = dev()
    with pytest.raises(ValueError, match="need cache="):
        m.encode(L3, I3.to(d), m.get_item_embeddings(I3.to(d)), {}, new_rows=counts)
    torch.cuda.synchronize()
    assert same(cache, cache0)


def test_device_counts_are_clamped_counted_and_never_read_back():
    from rails_amd import SASRec

    _, m, cache0, (L3, I3, counts) = fixture("amzn-books")
    d = dev()
    bad = counts.clone()
    bad[2], bad[3], bad[1] = 0, 9, int(L3[1]) + 1      # clamped to 1, to M = 3 and to the sequence's length (4 > M: M)
    clamped = torch.minimum(bad.clamp(1, 3), L3)
    c1, c2 = clone(cache0), clone(cache0)
    Ld, ids, cd = L3.to(d), I3.to(d), bad.to(d)
    torch.cuda.synchronize()
    v0 = SASRec.length_violations()
    with torch.inference_mode():
        emb = m.get_item_embeddings(ids)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            cur = m.encode(Ld, ids, emb, {}, cache=c1, new_rows=cd, max_new_rows=3)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert SASRec.length_violations() == v0 + 3
    assert torch.equal(cur, rows(m, L3, I3, c2, clamped)) and same(c1, c2)
    # a count past its sequence's length, below M: the length is the limit
    short = torch.tensor([3, 2] * (I3.shape[0] // 2))
    c3, c4 = clone(cache0), clone(cache0)
    v0 = SASRec.length_violations()
    cur = rows(m, short.to(d), I3, c3, torch.full_like(short, 3).to(d), max_new_rows=3)
    assert SASRec.length_violations() == v0 + I3.shape[0] // 2
    assert torch.equal(cur, rows(m, short, I3, c4, torch.minimum(short, torch.tensor(3)))) and same(c3, c4)


def test_strict_device_lengths_covers_device_counts(monkeypatch):
    from rails_amd import SASRec

    _, m, cache0, (L3, I3, counts) = fixture("amzn-books")
    bad = counts.clone()
    bad[2] = 0
    cache = clone(cache0)
    monkeypatch.setattr(SASRec, "STRICT_DEVICE_LENGTHS", True)
    with pytest.raises(ValueError, match="new_rows"):
        rows(m, L3.to(dev()), I3, cache, bad.to(dev()), max_new_rows=3)
    over = counts.clone()
    over[1] = L3[1] + 1
    with pytest.raises(ValueError, match="new_rows"):
        rows(m, L3.to(dev()), I3, cache, over)            # host counts against device lengths, read back under the flag
    assert same(cache, cache0)


# ---- 9. at the limits --------------------------------------------------------------------------------------------------------
def test_at_the_limits_two_rows():
    """seq_len 2048, dim 1024, ffn 1024, head_dim 64, B = 2, M = 2: the last two rows at N and at a short length, against the
    per-layer encode at test_at_the_limits' bar."""
    N, D, H, F = 2048, 1024, 16, 1024
    m = _module(N, D, H, F, 1, seed=3)
    before = torch.tensor([N, 5])
    ids0 = torch.randint(1, 501, (2, N), generator=torch.Generator().manual_seed(4)) * (torch.arange(N).unsqueeze(0) < before.unsqueeze(1))
    _, cache = prefill(m, before, ids0)
    after = torch.tensor([N, 7])
    ids = _edit(after, ids0, torch.tensor([2, 2]), 500)
    cur = rows(m, after, ids, cache, 2)
    enc = full(m, after, ids, fused=False)
    assert torch.isfinite(cur).all()
    assert R.distance(cur.cpu(), enc.cpu()) <= 1e-4, R.distance(cur.cpu(), enc.cpu())


@pytest.mark.parametrize("new_rows", [None, 2])
def test_more_sequences_than_a_grid_y(new_rows):
    """B = 70 000 > 65 535 with 16 heads: the plain step (which then runs the slot kernels, their work rows on grid.x) and a two-row
    step (140 000 work rows, 4 375 row tiles), against the full encode at test_shapes_beyond_the_fixtures' bar, 2 d(enc, f64) + 2e-5,
    float64 on the first and last 64 sequences."""
    B, N, D, H, F = 70000, 4, 16, 16, 8
    m = _module(N, D, H, F, 1, "relu", "layer_norm", items=50)
    g = torch.Generator().manual_seed(6)
    before = torch.randint(1, N, (B,), generator=g)
    ids0 = torch.randint(1, 51, (B, N), generator=g) * (torch.arange(N).unsqueeze(0) < before.unsqueeze(1))
    _, cache = prefill(m, before, ids0)
    k = 1 if new_rows is None else new_rows
    after = torch.clamp(before + k, max=N)
    ids = _edit(after, ids0, torch.full((B,), k), 50)
    cur = (step(m, after, ids, cache) if new_rows is None else rows(m, after, ids, cache, new_rows)).cpu().double()
    enc = full(m, after, ids).cpu().double()
    ends = torch.cat([torch.arange(64), torch.arange(B - 64, B)])
    fx = S.from_model(m, after[ends], ids[ends], dict(N=N, D=D, heads=H, blocks=1, act="relu", postproc="layer_norm"))
    cur64 = S.encoder64(fx, ids=ids[ends], lengths=after[ends])[1]
    bar = 2.0 * R.distance(enc[ends], cur64) + 2e-5
    assert R.distance(cur[ends], cur64) <= bar, (R.distance(cur[ends], cur64), bar)
    assert R.distance(cur, enc) <= bar, (R.distance(cur, enc), bar)


def test_more_work_rows_than_a_launch_grid_are_refused_before_any_launch():
    from rails_amd import SASRec, _lib

    m = SASRec(1, 1, 2, 1, 1, 2, "relu", num_items=10).to(dev()).eval()
    B = _lib.RAILS_SASREC_DECODE_MAX_ROWS // 2 + 1
    ids = torch.ones((B, 2), dtype=torch.int64, device=dev())
    cache = [(torch.zeros((B, 2, 2), device=dev()), torch.zeros((B, 2, 2), device=dev()))]
    with torch.inference_mode(), pytest.raises(NotImplementedError, match=str(_lib.RAILS_SASREC_DECODE_MAX_ROWS)):
        m.encode(torch.full((B,), 2), ids, m.get_item_embeddings(ids), {}, cache=cache, new_rows=2)
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in cache[0])
