"""GPU: the HSTU encoder's cached incremental decoding (HSTU.encode / generate_user_embeddings with return_cache_states,
delta_x_offsets and cache; rails_hstu_decode).

- Invariant: a prefill, then a decode of a new item at lengths - 1 with the timestamps unchanged, equals the full re-encode of the edited
  sequences: within twice the fp32 oracle's own distance from float64, plus 1e-6 (the bar of tests/test_hstu_kernels_gpu.py's encoder
  cases), at the three shipped geometries with their real block counts; also after three chained decodes at the same position.
- Reference fixtures (tests/golden/hstu_cache_*.npz): the current embeddings and the cache rows a decode writes match the float64
  restatement within twice the reference's distance from it, plus 1e-6; an interior delta returns the prefill's embedding bit for bit.
- In place: the returned states are the cache's own storage and only the delta rows change.
- Host-side validation raises; a device-resident position past the length is clamped and counted.
- Calls without cache arguments keep their routes and results."""
import pytest
import torch

from tests import _hstu_cache_ref as R
from tests.test_hstu_kernels_gpu import encoder_bar, module, timestamps, gen

from rails_amd.hstu import HSTU

pytestmark = pytest.mark.gpu

# the rails-final geometries (tools/hstu_bench.py): N, D, blocks, heads, dqk = dv, postproc
SHIPPED = {
    "ml-1m": (211, 50, 8, 2, 25, "layer_norm"),
    "ml-20m": (211, 256, 16, 8, 32, "layer_norm"),
    "amzn-books": (61, 64, 16, 8, 8, "l2_norm"),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a GPU")
    return torch.device("cuda", 0)


_MODULES = {}


def shipped(name):
    if name not in _MODULES:
        N, D, blocks, H, dh, post = SHIPPED[name]
        _MODULES[name] = module(N, D, blocks, H, dh, dh, post, seed=3)
    return _MODULES[name]


def batch(B, N, kind, seed):
    g = gen(seed)
    if kind == "1":
        lengths = torch.ones(B, dtype=torch.int64)
    elif kind == "N":
        lengths = torch.full((B,), N, dtype=torch.int64)
    else:
        lengths = torch.randint(1, N + 1, (B,), generator=g)
        lengths[0] = N
        if B > 1:
            lengths[1] = 1
    ids = torch.randint(1, 501, (B, N), generator=g) * (torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1))
    return lengths, ids, timestamps(B, N, g)


def delta(lengths, pos):
    return (torch.cumsum(lengths, 0) - lengths + pos, pos)


def run_encode(m, dev, lengths, ids, ts, host_lengths=False, **kw):
    with torch.inference_mode():
        ids_d = ids.to(dev)
        return m.encode(lengths if host_lengths else lengths.to(dev), ids_d, m.get_item_embeddings(ids_d), {"timestamps": ts.to(dev)} if ts is not None else {}, **kw)


INVARIANT = [(name, B, kind) for name in SHIPPED for B, kind in ((1, "1"), (1, "N"), (5, "1"), (5, "N"), (5, "mixed"), (32, "N"), (32, "mixed"))]


@pytest.mark.parametrize("name,B,kind", INVARIANT, ids=lambda c: str(c))
def test_decode_at_the_last_position_equals_a_full_re_encode(dev, name, B, kind):
    m, cfg, w = shipped(name)
    m = m.to(dev)
    N = cfg.max_sequence_len
    lengths, ids, ts = batch(B, N, kind, seed=B * 7 + len(kind))
    pos = lengths - 1
    new = ids.clone()
    new[torch.arange(B), pos] = torch.randint(1, 501, (B,), generator=gen(B))
    _, cache = run_encode(m, dev, lengths, ids, ts, return_cache_states=True)
    cur = run_encode(m, dev, lengths, new, ts, delta_x_offsets=delta(lengths, pos), cache=cache)
    ref64, bar = encoder_bar(cfg, w, lengths, new, ts)
    err = float((cur.cpu().double() - ref64).abs().max())
    assert err <= bar, (name, B, kind, err, bar)


@pytest.mark.parametrize("name", list(SHIPPED))
def test_three_chained_decodes(dev, name):
    m, cfg, w = shipped(name)
    m = m.to(dev)
    N = cfg.max_sequence_len
    B = 5
    lengths, ids, ts = batch(B, N, "mixed", seed=11)
    pos = lengths - 1
    _, cache = run_encode(m, dev, lengths, ids, ts, return_cache_states=True)
    g = gen(12)
    for _ in range(3):
        ids = ids.clone()
        ids[torch.arange(B), pos] = torch.randint(1, 501, (B,), generator=g)
        cur, cache = run_encode(m, dev, lengths, ids, ts, delta_x_offsets=delta(lengths, pos), cache=cache, return_cache_states=True)
    ref64, bar = encoder_bar(cfg, w, lengths, ids, ts)
    err = float((cur.cpu().double() - ref64).abs().max())
    assert err <= bar, (name, err, bar)


# ---- the reference's own prefill / decode --------------------------------------------------------------------------------------
def fixture_module(name, dev):
    cfg, w, lengths, ids, ts, z = R.load(name)
    m = HSTU(cfg.max_sequence_len - 1, 1, cfg.embedding_dim, cfg.num_blocks, cfg.num_heads, cfg.linear_dim, cfg.attention_dim, cfg.num_items,
             output_postproc=cfg.postproc, num_buckets=cfg.num_buckets).eval()
    m.load_state_dict(w, strict=True)
    return m.to(dev), cfg, lengths, ids, ts, z


@pytest.mark.parametrize("name", R.NAMES)
def test_reference_fixtures(dev, name):
    m, cfg, lengths, ids, ts, z = fixture_module(name, dev)
    ref = R.expected(name)
    bars = R.bars(name, ref)
    cache = None
    for tag in R.TAGS:
        pos, new_ids, new_ts, pre_ts = R.scenario(z, tag, ts)
        if tag == "tail2":
            pre = cur
        else:
            pre, cache = run_encode(m, dev, lengths, ids, pre_ts, return_cache_states=True)
            if tag == "interior" and "sample/rows" in z.files:      # the prefill's states at the sampled rows
                rows = torch.from_numpy(z["sample/rows"])
                for l, (v, q, k, o) in enumerate(cache):
                    for key, got in (("v", v.cpu()[rows]), ("outputs", o.cpu()[rows]), ("q", q.cpu()[0]), ("k", k.cpu()[0])):
                        want = torch.from_numpy(z[f"sample/l{l}/{key}"])
                        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()) + 1e-6, (tag, l, key)
        cur, cache = run_encode(m, dev, lengths, new_ids, new_ts, delta_x_offsets=delta(lengths, pos), cache=cache, return_cache_states=True)
        got = {"prefill_current": pre.cpu(), "current": cur.cpu(), **R.touched([tuple(t.cpu() for t in s) for s in cache], lengths, pos)}
        for q in ("prefill_current", "current") + R.ROWS:
            err = float((got[q].double() - ref[tag][q]).abs().max())
            assert err <= bars[tag][q], (tag, q, err, bars[tag][q])
        if tag in ("interior", "ts"):
            stale = pos < lengths - 1
            assert bool(stale.any()) and torch.equal(cur.cpu()[stale], pre.cpu()[stale])
        if tag == "interior" and "full/l0/v" in z.files:
            for l, (s_ref, s_got) in enumerate(zip(ref[tag]["states"], cache)):
                for key, a, b in zip(R.ROWS, s_ref, s_got):
                    want = torch.from_numpy(z[f"full/l{l}/{key}"]).double()
                    bar = 2 * float((want - a).abs().max()) + 1e-6
                    assert float((b.cpu().double().reshape(a.shape) - a).abs().max()) <= bar, (l, key)


def test_cache_is_updated_in_place_and_only_at_the_delta_rows(dev):
    m, cfg, lengths, ids, ts, z = fixture_module("amzn-books", dev)
    pos, new_ids, _, _ = R.scenario(z, "interior", ts)
    _, cache = run_encode(m, dev, lengths, ids, ts, return_cache_states=True)
    before = [tuple(t.clone() for t in s) for s in cache]
    cur, states = run_encode(m, dev, lengths, new_ids, ts, delta_x_offsets=delta(lengths, pos), cache=cache, return_cache_states=True)
    rows = torch.cumsum(lengths, 0) - lengths + pos
    B, N = ids.shape
    for (v, q, k, o), (v2, q2, k2, o2), (v0, q0, k0, o0) in zip(cache, states, before):
        assert v2 is v and o2 is o
        assert q2.untyped_storage().data_ptr() == q.untyped_storage().data_ptr() and q2.shape == (B, N, q.shape[-1])
        assert k2.untyped_storage().data_ptr() == k.untyped_storage().data_ptr()
        keep = torch.ones(v.shape[0], dtype=torch.bool)
        keep[rows] = False
        assert torch.equal(v.cpu()[keep], v0.cpu()[keep]) and torch.equal(o.cpu()[keep], o0.cpu()[keep])
        assert not torch.equal(v.cpu()[rows], v0.cpu()[rows])
        pk = torch.ones((B, N), dtype=torch.bool)
        pk[torch.arange(B), pos] = False
        assert torch.equal(q.cpu()[pk], q0.cpu()[pk]) and torch.equal(k.cpu()[pk], k0.cpu()[pk])
    # return_cache_states=False still updates the cache and returns only (B, D)
    again = run_encode(m, dev, lengths, ids, ts, delta_x_offsets=delta(lengths, pos), cache=cache)
    assert isinstance(again, torch.Tensor) and again.shape == (B, cfg.embedding_dim)


def test_generate_user_embeddings(dev):
    m, cfg, lengths, ids, ts, z = fixture_module("ml-1m", dev)
    B, N = ids.shape
    with torch.inference_mode():
        ids_d = ids.to(dev)
        emb = m.get_item_embeddings(ids_d)
        pay = {"timestamps": ts.to(dev)}
        y, st = m.generate_user_embeddings(lengths.to(dev), ids_d, emb, pay)
        assert st == [] and torch.equal(y, m.forward(lengths.to(dev), ids_d, emb, pay))
        y2, cache = m.generate_user_embeddings(lengths.to(dev), ids_d, emb, pay, return_cache_states=True)
        assert torch.equal(y2, y) and len(cache) == cfg.num_blocks
        pos, new_ids, _, _ = R.scenario(z, "tail", ts)
        new_d = new_ids.to(dev)
        y3, st3 = m.generate_user_embeddings(lengths.to(dev), new_d, m.get_item_embeddings(new_d), pay, delta_x_offsets=delta(lengths, pos),
                                             cache=cache)
    assert st3 == [] and y3.shape == (B, N, cfg.embedding_dim)
    ref = R.expected("ml-1m")["tail"]["current"]
    got = y3.cpu()[torch.arange(B), lengths - 1].double()
    assert float((got - ref).abs().max()) < 1e-4
    assert bool((y3.cpu()[torch.arange(N).unsqueeze(0) >= lengths.unsqueeze(1)] == 0).all())     # padded positions: zero rows


def test_host_side_validation_raises(dev):
    m, cfg, lengths, ids, ts, z = fixture_module("amzn-books", dev)
    pos = lengths - 1
    _, cache = run_encode(m, dev, lengths, ids, ts, return_cache_states=True)
    good = delta(lengths, pos)

    def dec(d=good, c=cache):
        return run_encode(m, dev, lengths, ids, ts, host_lengths=True, delta_x_offsets=d, cache=c)

    dec()                                                            # the valid call works, with int64 ...
    dec((good[0].to(torch.int32), good[1].to(torch.int32)))         # ... and int32 offsets
    with pytest.raises(ValueError, match="jagged row"):
        dec((good[0] + 1, pos))
    with pytest.raises(ValueError, match="outside"):
        dec((good[0] + 1, pos + 1))
    with pytest.raises(ValueError, match="outside"):
        dec((good[0] - pos - 1, torch.full_like(pos, -1)))
    with pytest.raises(ValueError, match="one .* state per layer"):
        dec(c=cache[:-1])
    with pytest.raises(ValueError, match="cache"):
        dec(c=None)
    short = [(v[:-1].contiguous(), q, k, o[:-1].contiguous()) for v, q, k, o in cache]
    with pytest.raises(ValueError, match="lengths sum to"):
        dec(c=short)
    with pytest.raises(ValueError, match="float32"):
        dec(c=[(v.double(), q, k, o) for v, q, k, o in cache])
    with pytest.raises(ValueError, match="contiguous"):
        dec(c=[(v, q.transpose(0, 1), k, o) for v, q, k, o in cache])
    with pytest.raises(ValueError, match="float32 tensor on"):
        dec(c=[(v, q, k, o.cpu()) for v, q, k, o in cache])
    with pytest.raises(ValueError, match="must be"):
        dec(c=[(v, q[:, :-1].contiguous(), k, o) for v, q, k, o in cache])


def test_device_position_past_the_length_is_clamped_and_counted(dev):
    m, cfg, lengths, ids, ts, z = fixture_module("ml-20m", dev)
    assert int(lengths[2]) < cfg.max_sequence_len
    pos = lengths - 1
    _, cache = run_encode(m, dev, lengths, ids, ts, return_cache_states=True)
    base = [tuple(t.clone() for t in s) for s in cache]
    want = run_encode(m, dev, lengths, ids, ts, delta_x_offsets=delta(lengths, pos), cache=base)
    bad = pos.clone()
    bad[2] = lengths[2]                                              # p == length: inside the (B, N) allocation, outside the sequence
    before = HSTU.length_violations()
    got = run_encode(m, dev, lengths, ids, ts, delta_x_offsets=tuple(t.to(dev) for t in delta(lengths, bad)), cache=cache)
    assert HSTU.length_violations() == before + 1
    assert torch.equal(got, want)
    for s, b in zip(cache, base):
        assert all(torch.equal(x, y) for x, y in zip(s, b))


@pytest.mark.parametrize("fused", [True, False])
def test_calls_without_cache_arguments_are_unchanged(dev, fused):
    m, cfg, lengths, ids, ts, z = fixture_module("amzn-books", dev)
    m.use_fused_kernel = fused
    plain = run_encode(m, dev, lengths, ids, ts)
    cur, cache = run_encode(m, dev, lengths, ids, ts, return_cache_states=True)
    assert torch.equal(run_encode(m, dev, lengths, ids, ts, cache=cache), plain)           # a cache without delta_x_offsets is ignored
    m.use_fused_kernel = False
    assert torch.equal(cur, run_encode(m, dev, lengths, ids, ts))                         # prefill == the per-layer route, bit for bit
    ref = torch.from_numpy(R.load("amzn-books")[-1]["tail/prefill_current"])
    assert float((plain.cpu() - ref).abs().max()) < 2e-5


def test_geometry_outside_the_decode_limits_is_refused(dev):
    m, cfg, w = module(16, 32, 1, 1, 40, 8, "layer_norm")       # dqk 40: no per-layer attention either, so build the cache by hand
    m = m.to(dev)
    lengths, ids, ts = batch(2, 16, "N", seed=1)
    cache = [(torch.zeros((32, 8), device=dev), torch.zeros((2, 16, 40), device=dev), torch.zeros((2, 16, 40), device=dev),
              torch.zeros((32, 32), device=dev))]
    with pytest.raises(NotImplementedError, match="dqk <= 32"):
        run_encode(m, dev, lengths, ids, ts, delta_x_offsets=delta(lengths, lengths - 1), cache=cache)
