"""GPU: hstu_decode_kernel (csrc/hstu.hip, behind rails_hstu_decode and HSTU.encode(..., delta_x_offsets=, cache=)) on every route of
its uvqk matrix-vector product, with more heads than waves, dqk != dv, strided row loops, a jagged-row prefix sum across waves, at its
LDS bound, with 0 / 1 / 255 buckets and timestamps on the bucket thresholds -- the cases of tests/_hstu_decode_cases.py.

- Through the C ABI: the cache is the float64 restatement's prefill rounded to fp32; the current embeddings and the four rows per layer
  the decode writes match the float64 decode from exactly those states within 2 * max(d_blocked, d_chain) + 1e-6 (the module docstring
  of tests/_hstu_decode_cases.py); every other cache element and the sentinel rows around every tensor stay bit-identical; a delta
  before lengths - 1 returns rails_rows_normalize of the cached last-layer outputs row, bit for bit.
- The same with every layer's uvqk at a 4-byte offset (the one-column-per-thread product with W % 4 == 0).
- Through the module: prefill, then encode(delta_x_offsets=, cache=), under the same bar formula with every reference started from its
  own prefill.
- The kernel's own guard: a sequence whose length, position or rows are out of range, and every sequence after an out-of-range length,
  gets a NaN row and writes nothing; the others are unaffected, bit for bit.
- The first geometry past each limit is refused without touching `out` or the cache.

Every test prints its figures (bars, distances, route) as one JSON line before it asserts."""
import ctypes as C
import json

import pytest
import torch

from tests import _hstu_cache_ref as R
from tests import _hstu_decode_cases as K
from tests.test_hstu_kernels_gpu import _P, _S, gen, thresholds, timestamps

pytestmark = pytest.mark.gpu

FENCE = 4                  # sentinel rows before and after every tensor the kernel can write
SENTINEL = -12345.0
INT_SENTINEL = 7
# cases whose geometry HSTU.encode(..., return_cache_states=True) refuses (the module route then has no cache to decode against)
MODULE_PREFILL_REFUSES = ()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a GPU")
    return torch.device("cuda", 0)


# ---- fenced tensors ------------------------------------------------------------------------------------------------------------------
def fenced(t, dev, rows=FENCE):
    """-> (the whole allocation on `dev`, its view of `t`): `t` (n, ...) between `rows` sentinel rows on either side."""
    fill = SENTINEL if t.is_floating_point() else INT_SENTINEL
    big = torch.full((t.shape[0] + 2 * rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    big[rows: rows + t.shape[0]] = t
    big = big.to(dev)
    return big, big[rows: rows + t.shape[0]]


def fence_intact(big, rows=FENCE):
    c = big.cpu()
    fill = SENTINEL if c.is_floating_point() else INT_SENTINEL
    return bool((c[:rows] == fill).all()) and bool((c[-rows:] == fill).all())


# ---- one launch through the C ABI ------------------------------------------------------------------------------------------------------
def _call_kernel(a):
    """rails_hstu_decode on the views of `a` -> its return code."""
    from rails_amd import _lib

    table = [(l["uvqk"], l["o_w"], l["o_b"], l["ts_w"], l["pos_w"], l["v"], l["q"], l["k"], l["outputs"]) for l in a["layers"]]
    _, ptrs = _lib.layer_table(_lib.HstuDecodeLayer, table, a["out"].device)
    code = _lib.load().rails_hstu_decode(_P(a["emb"]), _P(a["ids"]), _P(a["positions"]), _P(a["lengths"]), _P(a["ts"]),
                                         _P(a["thresholds"]) if a["ts"] is not None else None, _P(a["pos_emb"]), _P(ptrs), len(table), a["B"],
                                         a["N"], a["cache_rows"], a["D"], a["H"], a["dqk"], a["dv"], a["buckets"], 1, a["mode"],
                                         C.c_float(a["eps"]), _P(a["out"]), _S())
    torch.cuda.synchronize()
    return code


def launch(dev, geom, blocks, postproc, w, lengths, positions, ids, ts, states, cache_rows=None, fence=FENCE, uvqk_shift=0, eps=1e-6):
    """One rails_hstu_decode call the way HSTU._decode makes it, with every tensor the kernel indexes by a length or a position between
    `fence` sentinel rows.  geom = (N, D, H, dqk, dv, buckets); w: the weights under the module's names; states: the cache per layer
    (v, q, k, outputs) on the CPU.  ts None: no timestamps (NULL).  uvqk_shift: floats by which every uvqk is moved off its alignment.
    -> (return code, out (B, D), the cache afterwards per layer, all on the CPU); asserts the fences."""
    N, D, H, dqk, dv, buckets = geom
    B = lengths.numel()
    pos_w_name = "_input_features_preproc._pos_emb.weight"
    bigs = {}

    def fence_in(key, t):
        bigs[key], view = fenced(t, dev, fence)
        return view

    layers = []
    keep = []
    for l in range(blocks):
        p = f"_hstu._attention_layers.{l}."
        store = torch.zeros(w[p + "_uvqk"].numel() + uvqk_shift)
        store[uvqk_shift:] = w[p + "_uvqk"].reshape(-1)
        store = store.to(dev)
        keep.append(store)
        uvqk = store[uvqk_shift:]
        assert (uvqk.data_ptr() % 16 == 0) == (uvqk_shift % 4 == 0)
        bias = p + "_rel_attn_bias._ts_w" in w and ts is not None
        v, q, k, o = states[l]
        layers.append({"uvqk": uvqk, "o_w": w[p + "_o.weight"].contiguous().to(dev), "o_b": w[p + "_o.bias"].to(dev),
                       "ts_w": w[p + "_rel_attn_bias._ts_w"].to(dev) if bias else None,
                       "pos_w": w[p + "_rel_attn_bias._pos_w"].to(dev) if bias else None,
                       "v": fence_in(f"v{l}", v), "q": fence_in(f"q{l}", q.reshape(B * max(N, 1), -1)),
                       "k": fence_in(f"k{l}", k.reshape(B * max(N, 1), -1)), "outputs": fence_in(f"outputs{l}", o)})
    emb = w["_embedding_module._item_emb.weight"][ids].reshape(B * ids.shape[1], D)
    a = {"layers": layers, "emb": fence_in("emb", emb), "ids": fence_in("ids", ids.reshape(-1, 1)), "positions": positions.to(dev),
         "lengths": lengths.to(dev), "ts": fence_in("ts", ts.reshape(-1, 1)) if ts is not None else None,
         "thresholds": thresholds(buckets).to(dev) if ts is not None else None, "pos_emb": fence_in("pos_emb", w[pos_w_name]),
         "out": fence_in("out", torch.full((B, D), SENTINEL)), "B": B, "N": N, "D": D, "H": H, "dqk": dqk, "dv": dv, "buckets": buckets,
         "cache_rows": states[0][0].shape[0] if cache_rows is None else cache_rows, "mode": 0 if postproc == "layer_norm" else 1, "eps": eps}
    code = _call_kernel(a)
    for key, big in bigs.items():
        assert fence_intact(big, fence), f"sentinel rows around {key} were written"
    after = [(l["v"].cpu().clone(), l["q"].cpu().reshape(states[i][1].shape).clone(), l["k"].cpu().reshape(states[i][2].shape).clone(),
              l["outputs"].cpu().clone()) for i, l in enumerate(layers)]
    return code, a["out"].cpu().clone(), after, a


def case_geom(name):
    c = K.CASES[name]
    return (c.N, c.D, c.H, c.dqk, c.dv, c.buckets)


def kernel_ts(name, b):
    """The kernel gets the timestamps whenever there is a threshold table to search (HSTU._decode passes them even to a stack without
    relative bias, whose layers then carry NULL ts_w / pos_w); with 0 buckets the C ABI takes none."""
    return b.ts if K.CASES[name].buckets > 0 else None


def assert_only_touched_rows_changed(before, after, lengths, positions, written):
    """Every cache element outside the delta rows of the sequences in `written` is bit-identical."""
    off = torch.cumsum(lengths, 0) - lengths
    for l, (s0, s1) in enumerate(zip(before, after)):
        keep_j = torch.ones(s0[0].shape[0], dtype=torch.bool)
        keep_p = torch.ones(s0[1].shape[:2], dtype=torch.bool)
        for b in written:
            keep_j[int(off[b] + positions[b])] = False
            keep_p[b, int(positions[b])] = False
        for key, x0, x1, keep in (("v", s0[0], s1[0], keep_j), ("q", s0[1], s1[1], keep_p), ("k", s0[2], s1[2], keep_p), ("outputs", s0[3], s1[3], keep_j)):
            assert torch.equal(x0[keep], x1[keep]), f"layer {l}: {key} changed outside the delta rows"


def check_against(figures, got, ref64, bars, dist):
    dists = {q: float((got[q].double() - ref64[q]).abs().max()) for q in K.QUANTITIES}
    figures.update({"bar": bars, "kernel": dists, "d_blocked": {q: dist[q][0] for q in dist}, "d_chain": {q: dist[q][1] for q in dist}})
    print(json.dumps(figures))
    for q in K.QUANTITIES:
        assert torch.isfinite(got[q]).all() and dists[q] <= bars[q], figures


def run_direct(dev, name, kind, scen, uvqk_shift=0):
    c = K.CASES[name]
    _, cfg, w = K.build(name)
    b = K.batch(name, kind, scen)
    d = K.direct(name, kind, scen)
    code, out, after, a = launch(dev, case_geom(name), c.blocks, c.postproc, w, b.lengths, b.positions, b.new_ids, kernel_ts(name, b), d.states32,
                                 uvqk_shift=uvqk_shift, eps=cfg.eps)
    assert code == 0, code
    got = {"current": out, **R.touched(after, b.lengths, b.positions)}
    figures = {"case": name, "ts": kind, "scenario": scen, "via": "c-abi", "route": list(K.route(c.W, aligned=uvqk_shift % 4 == 0))}
    check_against(figures, got, d.ref64, d.bars, d.dist)
    assert_only_touched_rows_changed(d.states32, after, b.lengths, b.positions, range(c.B))
    return b, out, a, cfg


@pytest.mark.parametrize("run", K.RUNS, ids=K.run_id)
def test_kernel_matches_float64_through_the_c_abi(dev, run):
    name, kind, scen = run
    b, out, a, cfg = run_direct(dev, name, kind, scen)
    stale = (b.positions < b.lengths - 1).nonzero().flatten()
    assert (stale.numel() > 0) == (scen == "interior")
    if stale.numel():
        # the result of a delta before lengths - 1 is the postprocessed CACHED row: rails_rows_normalize's arithmetic step for step
        from rails_amd import _lib

        c = K.CASES[name]
        rows = (torch.cumsum(b.lengths, 0) - 1)[stale].to(dev)
        want = torch.full((stale.numel(), c.D), SENTINEL, device=dev)
        last = a["layers"][-1]["outputs"]
        _lib.check(_lib.load().rails_rows_normalize(_P(last), c.D, _P(rows), stale.numel(), c.D, a["mode"], C.c_float(cfg.eps), _P(want), _S()),
                   "rails_rows_normalize")
        assert torch.equal(out[stale], want.cpu()), (run, float((out[stale] - want.cpu()).abs().max()))


@pytest.mark.parametrize("scen", K.SCENARIOS)
def test_unaligned_weights_take_the_per_column_route(dev, scen):
    assert K.CASES["nobias"].W == 256
    run_direct(dev, "nobias", "random", scen, uvqk_shift=1)


# ---- through the module ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [r for r in K.RUNS if r[1] == "random"], ids=K.run_id)
def test_module_route_matches_float64(dev, run):
    name, kind, scen = run
    c = K.CASES[name]
    m, cfg, w = K.build(name)
    m = m.to(dev)
    b = K.batch(name, kind, scen)
    pay = {"timestamps": b.ts.to(dev)} if c.buckets > 0 else {}
    delta = (torch.cumsum(b.lengths, 0) - b.lengths + b.positions, b.positions)
    with torch.inference_mode():
        ids_d, new_d = b.ids.to(dev), b.new_ids.to(dev)
        try:
            _, cache = m.encode(b.lengths.to(dev), ids_d, m.get_item_embeddings(ids_d), pay, return_cache_states=True)
        except NotImplementedError as e:
            print(json.dumps({"case": name, "via": "module", "prefill_refused": str(e)}))
            assert name in MODULE_PREFILL_REFUSES, e
            return
        assert name not in MODULE_PREFILL_REFUSES
        cur, states = m.encode(b.lengths.to(dev), new_d, m.get_item_embeddings(new_d), pay, delta_x_offsets=delta, cache=cache,
                               return_cache_states=True)
    r = K.routed(name, kind, scen)
    got = {"current": cur.cpu(), **R.touched([tuple(t.cpu() for t in s) for s in states], b.lengths, b.positions)}
    check_against({"case": name, "ts": kind, "scenario": scen, "via": "module", "route": list(K.route(c.W))}, got, r.ref64, r.bars, r.dist)


# ---- the kernel's own guard ----------------------------------------------------------------------------------------------------------------
def test_out_of_range_sequences_write_nothing_and_return_nan(dev):
    """Direct calls only: the Python host validates or clamps before it launches.  Every invalid value is within 1 of the valid range
    and every tensor is fenced by N + 2 rows, so a kernel WITHOUT the guard would still stay inside this test's own allocations."""
    name = "scalar_w30"
    c = K.CASES[name]
    _, cfg, w = K.build(name)
    N, B = c.N, 8
    g = gen(77)
    #                        valid  len 0  valid  p = -1  valid  p = len  len N+1  valid alone, after an out-of-range length
    lengths = torch.tensor([N,     0,     7,     5,      12,    6,       N + 1,   4])
    positions = torch.tensor([N - 1, 0,   3,     -1,     11,    6,       2,       3])
    ids = torch.randint(1, 501, (B, N), generator=g)
    ts = timestamps(B, N, g)
    HV, HQ = c.H * c.dv, c.H * c.dqk

    def cache_for(total):
        gg = gen(78)
        return [(0.5 * torch.randn((total, HV), generator=gg), 0.5 * torch.randn((B, N, HQ), generator=gg),
                 0.5 * torch.randn((B, N, HQ), generator=gg), 0.5 * torch.randn((total, c.D), generator=gg)) for _ in range(c.blocks)]

    def only(seqs, lengths, cache):
        """The batch holding only `seqs`, with their cache rows."""
        off = torch.cumsum(lengths, 0) - lengths
        jag = torch.cat([torch.arange(int(off[s]), int(off[s] + lengths[s])) for s in seqs])
        sel = torch.tensor(seqs)
        return lengths[sel], positions[sel], ids[sel], ts[sel], [(v[jag], q[sel], k[sel], o[jag]) for v, q, k, o in cache]

    def check(lengths, cache_rows, valid):
        total = int(lengths.sum())
        cache = cache_for(total)
        code, out, after, _ = launch(dev, case_geom(name), c.blocks, c.postproc, w, lengths, positions, ids, ts, cache, cache_rows=cache_rows,
                                     fence=N + 2, eps=cfg.eps)
        assert code == 0
        invalid = [s for s in range(B) if s not in valid]
        assert bool(torch.isnan(out[invalid]).all()), out[invalid]
        assert_only_touched_rows_changed(cache, after, lengths, positions, valid)
        sub = only(valid, lengths, cache)
        code, want, want_after, _ = launch(dev, case_geom(name), c.blocks, c.postproc, w, *sub, fence=N + 2, eps=cfg.eps)
        assert code == 0 and bool(torch.isfinite(want).all())
        assert torch.equal(out[valid], want)
        mine = R.touched(after, lengths, positions.clamp(min=0))
        theirs = R.touched(want_after, sub[0], sub[1])
        for q in R.ROWS:
            assert torch.equal(mine[q][:, valid], theirs[q]), q
            assert not torch.equal(theirs[q], R.touched(sub[4], sub[0], sub[1])[q]), q      # the valid sequences did write

    check(lengths, int(lengths.sum()), [0, 2, 4])
    second = lengths.clone()
    second[6] = 3                                                    # every length in range now: sequence 6 is valid at position 2 ...
    check(second, int(second.sum()) - 1, [0, 2, 4, 6])               # ... and the cache is one row short of the last sequence's rows


# ---- past the limits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", list(K.BOUNDARY_PAIRS))
def test_first_geometry_past_each_limit_is_refused_untouched(dev, limit):
    from rails_amd import _lib

    good, bad = K.BOUNDARY_PAIRS[limit]
    assert _lib.load().rails_hstu_decode_supported(*good) == 1 and _lib.load().rails_hstu_decode_supported(*bad) == 0
    N, D, H, dqk, dv, buckets = bad
    n = max(N, 1)                                                    # seq_len 0: the tensors of seq_len 1
    B = 2
    g = gen(5)
    p = "_hstu._attention_layers.0."
    w = {"_embedding_module._item_emb.weight": torch.randn((11, D), generator=g), "_input_features_preproc._pos_emb.weight": torch.randn((n, D), generator=g),
         p + "_uvqk": torch.randn((D, 2 * H * (dqk + dv)), generator=g), p + "_o.weight": torch.randn((D, H * dv), generator=g),
         p + "_o.bias": torch.randn(D, generator=g)}
    ts = None
    if buckets:
        w[p + "_rel_attn_bias._ts_w"] = torch.randn(buckets + 1, generator=g)
        w[p + "_rel_attn_bias._pos_w"] = torch.randn(2 * n - 1, generator=g)
        ts = timestamps(B, n, g)
    lengths = torch.full((B,), n)
    cache = [(torch.randn((B * n, H * dv), generator=g), torch.randn((B, n, H * dqk), generator=g), torch.randn((B, n, H * dqk), generator=g),
              torch.randn((B * n, D), generator=g))]
    code, out, after, _ = launch(dev, bad, 1, "layer_norm", w, lengths, lengths - 1, torch.randint(1, 11, (B, n), generator=g), ts, cache)
    # seq_len 0 is a bad size to rails_hstu_decode (RAILS_EINVAL, tests/test_hstu_cache.py), every other limit an unsupported geometry
    assert code == (_lib.RAILS_EINVAL if limit == "N" else _lib.RAILS_ENOTSUP), (limit, code, _lib.last_error())
    assert bool((out == SENTINEL).all())
    for s0, s1 in zip(cache, after):
        assert all(torch.equal(x, y) for x, y in zip(s0, s1))
