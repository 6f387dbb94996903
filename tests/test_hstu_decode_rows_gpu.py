"""GPU: the multi-row HSTU cached decode step (csrc/hstu_rows.hip behind rails_hstu_decode_rows and HSTU.encode(..., delta_rows=)).

- Through the C ABI on the geometries of tests/_hstu_decode_cases.py and the runs of tests/_hstu_rows_ref.py (uniform 1 and 2 rows, a
  ragged batch with a whole sequence, a run from 0, an interior run and a padding id, a 33-row run across two slot tiles): the current
  embeddings and every written row within 2 * max(d_blocked, d_chain) + 1e-6 of the float64 chain from the same fp32 states; every
  other cache element and the sentinel rows around every tensor bit-identical; an interior run returns rails_rows_normalize of the
  cached row bit for bit.
- One step over m rows is torch.equal, in out and in every cache tensor, to one-row calls of the same entry, at any slot count.
- The guards: out-of-range sequences write nothing and return NaN, the others are bit-identical to a call of their own; device counts
  out of range are clamped, and the module counts them.
- The launch grid: 66 000 sequences in one step; the first row count past RAILS_HSTU_DECODE_MAX_ROWS is refused untouched.
- Through the module on the shipped geometries: an edit of the last three rows against the module's own prefill of the edited ids, an
  append of two events through extend_cache_states from len_old - 1 against a prefill at the new lengths; delta_rows=None unchanged.
- The reference's own chained single-row steps and prefill (tests/golden/hstu_rows_*.npz).

Every test prints its figures as one JSON line before it asserts."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _hstu_cache_ref as R
from tests import _hstu_decode_cases as K
from tests import _hstu_rows_ref as M
from tests.test_hstu_cache_gpu import SHIPPED, fixture_module, shipped
from tests.test_hstu_decode_kernel_gpu import FENCE, SENTINEL, case_geom, fence_intact, fenced
from tests.test_hstu_kernels_gpu import _P, _S, gen, thresholds, timestamps

pytestmark = pytest.mark.gpu

CABI_CASES = ("scalar_w30", "scalar_w198", "one_slice", "heads9", "dqk_ne_dv", "d1024", "b600", "nobias")
CABI_RUNS = [(name, kind, "random") for name in CABI_CASES for kind in M.kinds(name)]
CABI_RUNS += [("scalar_w198", "ragged", ts_kind) for ts_kind in K.TS_KINDS["scalar_w198"] if ts_kind != "random"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a GPU")
    return torch.device("cuda", 0)


# ---- one step through the C ABI ----------------------------------------------------------------------------------------------------------
def launch(dev, geom, blocks, postproc, w, lengths, start, counts, max_rows, ids, ts, states, cache_rows=None, fence=FENCE, eps=1e-6):
    """One rails_hstu_decode_rows call with every tensor the kernels index by a length or a position between `fence` sentinel rows.
    counts None: NULL (max_rows everywhere).  -> (return code, out (B, D), the cache afterwards per layer on the CPU, the arguments)."""
    from rails_amd import _lib

    N, D, H, dqk, dv, buckets = geom
    B = lengths.numel()
    bigs = {}

    def fence_in(key, t):
        bigs[key], view = fenced(t, dev, fence)
        return view

    layers = []
    for l in range(blocks):
        p = f"_hstu._attention_layers.{l}."
        bias = p + "_rel_attn_bias._ts_w" in w and ts is not None
        v, q, k, o = states[l]
        layers.append({"uvqk": w[p + "_uvqk"].contiguous().to(dev), "o_w": w[p + "_o.weight"].contiguous().to(dev), "o_b": w[p + "_o.bias"].to(dev),
                       "ts_w": w[p + "_rel_attn_bias._ts_w"].to(dev) if bias else None,
                       "pos_w": w[p + "_rel_attn_bias._pos_w"].to(dev) if bias else None,
                       "v": fence_in(f"v{l}", v), "q": fence_in(f"q{l}", q.reshape(B * N, -1)), "k": fence_in(f"k{l}", k.reshape(B * N, -1)),
                       "outputs": fence_in(f"outputs{l}", o)})
    emb = w["_embedding_module._item_emb.weight"][ids].reshape(B * N, D)
    lib = _lib.load()
    floats = lib.rails_hstu_decode_rows_workspace_floats(B * max_rows, B, D, H, dqk, dv)
    a = {"layers": layers, "emb": fence_in("emb", emb), "ids": fence_in("ids", ids.reshape(-1, 1)), "start": start.to(dev),
         "counts": counts.to(dev) if counts is not None else None, "lengths": lengths.to(dev),
         "ts": fence_in("ts", ts.reshape(-1, 1)) if ts is not None else None, "thresholds": thresholds(buckets).to(dev) if ts is not None else None,
         "pos_emb": fence_in("pos_emb", w["_input_features_preproc._pos_emb.weight"]), "out": fence_in("out", torch.full((B, D), SENTINEL)),
         "work": fence_in("work", torch.zeros((floats, 1))), "mode": 0 if postproc == "layer_norm" else 1}
    table = [(l["uvqk"], l["o_w"], l["o_b"], l["ts_w"], l["pos_w"], l["v"], l["q"], l["k"], l["outputs"]) for l in layers]
    _, ptrs = _lib.layer_table(_lib.HstuDecodeLayer, table, dev)
    code = lib.rails_hstu_decode_rows(_P(a["emb"]), _P(a["ids"]), _P(a["start"]), _P(a["counts"]) if counts is not None else None, max_rows,
                                      _P(a["lengths"]), _P(a["ts"]), _P(a["thresholds"]) if ts is not None else None, _P(a["pos_emb"]), _P(ptrs),
                                      blocks, B, N, states[0][0].shape[0] if cache_rows is None else cache_rows, D, H, dqk, dv, buckets, 1, a["mode"],
                                      C.c_float(eps), _P(a["work"]), _P(a["out"]), _S())
    torch.cuda.synchronize()
    for key, big in bigs.items():
        assert fence_intact(big, fence), f"sentinel rows around {key} were written"
    after = [(l["v"].cpu().clone(), l["q"].cpu().reshape(states[i][1].shape).clone(), l["k"].cpu().reshape(states[i][2].shape).clone(),
              l["outputs"].cpu().clone()) for i, l in enumerate(layers)]
    return code, a["out"].cpu().clone(), after, a


def kernel_ts(name, ts):
    return ts if K.CASES[name].buckets > 0 else None


def assert_only_run_rows_changed(before, after, lengths, start, counts, written):
    """Every cache element outside the runs of the sequences in `written` is bit-identical."""
    off = torch.cumsum(lengths, 0) - lengths
    for l, (s0, s1) in enumerate(zip(before, after)):
        keep_j = torch.ones(s0[0].shape[0], dtype=torch.bool)
        keep_p = torch.ones(s0[1].shape[:2], dtype=torch.bool)
        for b in written:
            keep_j[int(off[b] + start[b]): int(off[b] + start[b] + counts[b])] = False
            keep_p[b, int(start[b]): int(start[b] + counts[b])] = False
        for key, x0, x1, keep in (("v", s0[0], s1[0], keep_j), ("q", s0[1], s1[1], keep_p), ("k", s0[2], s1[2], keep_p), ("outputs", s0[3], s1[3], keep_j)):
            assert torch.equal(x0[keep], x1[keep]), f"layer {l}: {key} changed outside the runs"


def check_against(figures, got, ref64, bars, dist):
    dists = {q: float((got[q].double() - ref64[q]).abs().max()) for q in M.QUANTITIES}
    figures.update({"bar": bars, "kernel": dists, "d_blocked": {q: dist[q][0] for q in dist}, "d_chain": {q: dist[q][1] for q in dist}})
    print(json.dumps(figures))
    for q in M.QUANTITIES:
        assert torch.isfinite(got[q]).all() and dists[q] <= bars[q], figures


def step(dev, name, r, states, counts="tensor", max_rows=None, **kw):
    c = K.CASES[name]
    _, cfg, w = K.build(name)
    mr = int(r.counts.max()) if max_rows is None else max_rows
    return launch(dev, case_geom(name), c.blocks, c.postproc, w, r.lengths, r.start, r.counts if counts == "tensor" else None, mr, r.new_ids,
                  kernel_ts(name, r.ts), states, eps=cfg.eps, **kw)


# ---- 1. the C ABI against float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", CABI_RUNS, ids=lambda r: "-".join(r))
def test_step_matches_the_float64_chain_through_the_c_abi(dev, run):
    name, kind, ts_kind = run
    c = K.CASES[name]
    r = M.run(name, kind, ts_kind)
    d = M.direct(name, kind, ts_kind)
    uniform = kind in ("uniform1", "uniform2")
    code, out, after, a = step(dev, name, r, d.states32, counts=None if uniform else "tensor")
    assert code == 0, code
    got = {"current": out, **M.touched(after, r.lengths, r.start, r.counts)}
    check_against({"case": name, "run": kind, "ts": ts_kind, "via": "c-abi", "max_rows": int(r.counts.max())}, got, d.ref64, d.bars, d.dist)
    assert_only_run_rows_changed(d.states32, after, r.lengths, r.start, r.counts, range(c.B))
    stale = (r.start + r.counts < r.lengths).nonzero().flatten()
    assert (stale.numel() > 0) == (kind == "ragged")
    if stale.numel():
        # an interior run's result is the postprocessed CACHED row: rails_rows_normalize's arithmetic step for step
        from rails_amd import _lib

        _, cfg, _ = K.build(name)
        rows = (torch.cumsum(r.lengths, 0) - 1)[stale].to(dev)
        want = torch.full((stale.numel(), c.D), SENTINEL, device=dev)
        _lib.check(_lib.load().rails_rows_normalize(_P(a["layers"][-1]["outputs"]), c.D, _P(rows), stale.numel(), c.D, a["mode"], C.c_float(cfg.eps),
                                                    _P(want), _S()), "rails_rows_normalize")
        torch.cuda.synchronize()
        assert torch.equal(out[stale], want.cpu()), (run, float((out[stale] - want.cpu()).abs().max()))


# ---- 2. slot independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ragged", "long"])
@pytest.mark.parametrize("name", ["scalar_w198", "heads9"])
def test_one_step_is_bitwise_the_one_row_calls_of_the_same_entry(dev, name, kind):
    if kind not in M.kinds(name):
        kind = "uniform2"                                       # heads9 (N = 33) has no 33-row run: its two-row batch instead
    r = M.run(name, kind)
    d = M.direct(name, kind)
    top = int(r.counts.max())
    states = d.states32
    for t in range(top):                                        # a sequence whose run is over repeats its last row: the same inputs
        one = r._replace(start=r.start + torch.minimum(torch.full_like(r.counts, t), r.counts - 1), counts=torch.ones_like(r.counts))
        code, want, states, _ = step(dev, name, one, states, counts=None, max_rows=1)
        assert code == 0
    for max_rows in (top, top + 5):
        code, out, after, _ = step(dev, name, r, d.states32, max_rows=max_rows)
        assert code == 0
        assert torch.equal(out, want), (name, kind, max_rows)
        assert all(torch.equal(x, y) for s, t in zip(after, states) for x, y in zip(s, t)), (name, kind, max_rows)
    if kind == "uniform2":                                      # NULL counts are max_rows everywhere
        code, out, after, _ = step(dev, name, r, d.states32, counts=None)
        assert code == 0 and torch.equal(out, want) and all(torch.equal(x, y) for s, t in zip(after, states) for x, y in zip(s, t))


# ---- 3. the guards -----------------------------------------------------------------------------------------------------------------------
def test_out_of_range_sequences_write_nothing_and_return_nan(dev):
    """Direct calls only: the Python host validates or clamps before it launches.  Every invalid value is within 2 rows of the valid
    range and every tensor is fenced by N + 2 rows, so kernels WITHOUT the guard would still stay inside this test's own allocations."""
    name = "scalar_w30"
    c = K.CASES[name]
    _, cfg, w = K.build(name)
    N, B = c.N, 8
    g = gen(91)
    #                        valid   len 0  valid  p = -1  valid  p = len  len N+1  valid alone, after an out-of-range length
    lengths = torch.tensor([N,      0,     7,     5,      12,    6,       N + 1,   4])
    start = torch.tensor([N - 2,    0,     3,     -1,     10,    6,       2,       2])
    counts = torch.tensor([2,       1,     2,     1,      2,     1,       1,       2])
    ids = torch.randint(1, 501, (B, N), generator=g)
    ts = timestamps(B, N, g)
    HV, HQ = c.H * c.dv, c.H * c.dqk

    def cache_for(total):
        gg = gen(92)
        return [(0.5 * torch.randn((total, HV), generator=gg), 0.5 * torch.randn((B, N, HQ), generator=gg),
                 0.5 * torch.randn((B, N, HQ), generator=gg), 0.5 * torch.randn((total, c.D), generator=gg)) for _ in range(c.blocks)]

    def only(seqs, lengths, cache):
        off = torch.cumsum(lengths, 0) - lengths
        jag = torch.cat([torch.arange(int(off[s]), int(off[s] + lengths[s])) for s in seqs])
        sel = torch.tensor(seqs)
        return lengths[sel], start[sel], counts[sel], ids[sel], ts[sel], [(v[jag], q[sel], k[sel], o[jag]) for v, q, k, o in cache]

    def call(lengths, start, counts, ids, ts, cache, cache_rows=None):
        return launch(dev, case_geom(name), c.blocks, c.postproc, w, lengths, start, counts, 2, ids, ts, cache, cache_rows=cache_rows, fence=N + 2,
                      eps=cfg.eps)

    def check(lengths, cache_rows, valid):
        cache = cache_for(int(lengths.sum()))
        code, out, after, _ = call(lengths, start, counts, ids, ts, cache, cache_rows)
        assert code == 0
        invalid = [s for s in range(B) if s not in valid]
        assert bool(torch.isnan(out[invalid]).all()), out[invalid]
        assert_only_run_rows_changed(cache, after, lengths, start, counts, valid)
        sub = only(valid, lengths, cache)
        code, want, want_after, _ = call(*sub)
        assert code == 0 and bool(torch.isfinite(want).all())
        assert torch.equal(out[valid], want)
        sel = torch.tensor(valid)
        mine = M.touched(after, lengths, start.clamp(min=0), torch.where(torch.isin(torch.arange(B), sel), counts, torch.zeros_like(counts)))
        theirs = M.touched(want_after, sub[0], sub[1], sub[2])
        for q in R.ROWS:
            assert torch.equal(mine[q], theirs[q]), q
            assert not torch.equal(theirs[q], M.touched(sub[5], sub[0], sub[1], sub[2])[q]), q      # the valid sequences did write

    check(lengths, int(lengths.sum()), [0, 2, 4])
    second = lengths.clone()
    second[6] = 3                                                    # every length in range now: sequence 6 is valid at row 2 ...
    check(second, int(second.sum()) - 1, [0, 2, 4, 6])               # ... and the cache is one row short of the last sequence's rows


def test_device_counts_out_of_range_are_clamped_and_the_module_counts_them(dev):
    from rails_amd.hstu import HSTU

    name = "scalar_w30"
    r = M.run(name, "ragged")
    d = M.direct(name, "ragged")
    assert int(r.counts[2]) == 3 and int(r.start[3] + r.counts[3]) == int(r.lengths[3])
    bad = r.counts.clone()
    bad[2] = 0                                                       # -> 1
    bad[3] = int(r.lengths[3] - r.start[3]) + 1                      # -> len - p
    clamped = r.counts.clone()
    clamped[2] = 1
    code, want, want_after, _ = step(dev, name, r._replace(counts=clamped), d.states32, max_rows=3)
    code2, out, after, _ = step(dev, name, r._replace(counts=bad), d.states32, max_rows=3)
    assert code == 0 and code2 == 0 and torch.equal(out, want)
    assert all(torch.equal(x, y) for s, t in zip(after, want_after) for x, y in zip(s, t))
    # the module: the same two counts on the device are counted, and the result is that of the clamped counts
    m, cfg, w = K.build(name)
    m = m.to(dev)
    off = torch.cumsum(r.lengths, 0) - r.lengths
    delta = tuple(t.to(dev) for t in (off + r.start, r.start))

    def enc(counts, cache):
        with torch.inference_mode():
            ids = r.new_ids.to(dev)
            return m.encode(r.lengths.to(dev), ids, m.get_item_embeddings(ids), {"timestamps": r.ts.to(dev)}, delta_x_offsets=delta, cache=cache,
                            delta_rows=counts.to(dev), max_delta_rows=3)

    def cache():
        B, N = r.ids.shape
        return [tuple(t.to(dev).contiguous() for t in s) for s in d.states32]

    c1, c2 = cache(), cache()
    before = HSTU.length_violations()
    good = enc(clamped, c1)
    assert HSTU.length_violations() == before
    got = enc(bad, c2)
    assert HSTU.length_violations() == before + 2
    assert torch.equal(got, good) and all(torch.equal(x, y) for s, t in zip(c1, c2) for x, y in zip(s, t))
    assert torch.equal(got.cpu(), want)                              # ... and the module makes the C-ABI call above
    with pytest.raises(ValueError, match="needs max_delta_rows=M"):
        with torch.inference_mode():
            ids = r.new_ids.to(dev)
            m.encode(r.lengths.to(dev), ids, m.get_item_embeddings(ids), {"timestamps": r.ts.to(dev)}, delta_x_offsets=delta, cache=c1,
                     delta_rows=bad.to(dev))


# ---- 5. the launch grid -------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_66000_sequences_is_one_step_and_the_first_row_count_past_the_limit_is_refused(dev):
    from rails_amd import _lib

    name = "b600"
    c = K.CASES[name]
    _, cfg, w = K.build(name)
    B, N = 66_000, c.N
    g = gen(66)
    lengths = torch.randint(1, N + 1, (B,), generator=g)
    ids = torch.randint(1, 501, (B, N), generator=g) * (torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1))
    new_ids = ids.clone()
    start = lengths - 1
    new_ids[torch.arange(B), start] = torch.randint(1, 501, (B,), generator=g)
    ts = timestamps(B, N, g)
    w64 = K._f64(w)
    _, st64 = R.prefill(cfg, w64, lengths, ids, ts)
    states32 = [tuple(t.float() for t in s) for s in st64]
    ones = torch.ones(B, dtype=torch.int64)
    code, out, after, _ = launch(dev, case_geom(name), c.blocks, c.postproc, w, lengths, start, None, 1, new_ids, ts, states32, eps=cfg.eps)
    assert code == 0, (code, _lib.last_error())
    assert bool(torch.isfinite(out).all())
    sample = torch.cat([torch.tensor([0, 1, B - 2, B - 1]), torch.randperm(B - 4, generator=g)[:60] + 2]).sort().values
    off = torch.cumsum(lengths, 0) - lengths
    jag = torch.cat([torch.arange(int(off[b]), int(off[b] + lengths[b])) for b in sample.tolist()])
    sub32 = [(v[jag], q[sample], k[sample], o[jag]) for v, q, k, o in states32]
    sl, si, sts, sp = lengths[sample], new_ids[sample], ts[sample], start[sample]

    def dec(weights, dtype, **kw):
        st = [tuple(t.to(dtype, copy=True) for t in s) for s in sub32]
        return {"current": R.decode(cfg, weights, sl, si, sts, sp, st, **kw), **R.touched(st, sl, sp)}

    ref64 = dec(w64, torch.float64)
    bars, dist = K._bars(ref64, dec(w, torch.float32), dec(w, torch.float32, gemv=R.chain_gemv))
    got = {"current": out[sample], **R.touched([(v[jag], q[sample], k[sample], o[jag]) for v, q, k, o in after], sl, sp)}
    check_against({"case": name, "batch": B, "via": "c-abi"}, got, ref64, bars, dist)
    assert_only_run_rows_changed(states32, after, lengths, start, ones, range(B))
    # batch x max_rows past the limit: refused before any launch, nothing touched (the tensors of the call above, tiny)
    max_rows = _lib.RAILS_HSTU_DECODE_MAX_ROWS // B + 1
    assert (max_rows - 1) * B <= _lib.RAILS_HSTU_DECODE_MAX_ROWS < max_rows * B
    code, out2, after2, _ = launch(dev, case_geom(name), c.blocks, c.postproc, w, lengths, start, None, max_rows, new_ids, ts, states32, eps=cfg.eps)
    assert code == _lib.RAILS_EINVAL and "work rows" in _lib.last_error(), (code, _lib.last_error())
    assert bool((out2 == SENTINEL).all()) and all(torch.equal(x, y) for s, t in zip(states32, after2) for x, y in zip(s, t))


# ---- 6. through the module ----------------------------------------------------------------------------------------------------------------
def _enc(m, dev, lengths, ids, ts, **kw):
    with torch.inference_mode():
        ids_d = ids.to(dev)
        return m.encode(lengths.to(dev), ids_d, m.get_item_embeddings(ids_d), {"timestamps": ts.to(dev)}, **kw)


def _cpu(states):
    return [tuple(t.cpu() for t in s) for s in states]


@pytest.mark.parametrize("name", list(SHIPPED))
def test_module_edit_and_append_match_float64_and_the_plain_step_is_unchanged(dev, name):
    m, cfg, w = shipped(name)
    m = m.to(dev)
    N, B = cfg.max_sequence_len, 6
    g = gen(600 + len(name))
    new_len = torch.randint(4, N + 1, (B,), generator=g)
    new_len[0] = N
    ids = torch.randint(1, 501, (B, N), generator=g) * (torch.arange(N).unsqueeze(0) < new_len.unsqueeze(1))
    ts = timestamps(B, N, g)
    off = torch.cumsum(new_len, 0) - new_len

    # ---- an edit of the last three rows, against the module's own prefill of the edited ids and the float64 chain
    start, counts = new_len - 3, torch.full((B,), 3)
    edited = ids.clone()
    eb, ep = M.run_rows(new_len, start, counts)
    edited[eb, ep] = torch.randint(1, 501, (eb.numel(),), generator=g)
    _, cache = _enc(m, dev, new_len, ids, ts, return_cache_states=True)
    plain_before = _enc(m, dev, new_len, ids, ts, delta_x_offsets=(off + new_len - 1, new_len - 1), cache=[tuple(t.clone() for t in s) for s in cache])
    cur, states = _enc(m, dev, new_len, edited, ts, delta_x_offsets=(off + start, start), cache=cache, delta_rows=3, return_cache_states=True)
    assert all(x is y for s, t in zip(states, cache) for x, y in ((s[0], t[0]), (s[3], t[3])))
    pre_cur, pre = _enc(m, dev, new_len, edited, ts, return_cache_states=True)

    def edit(weights, gemv=None):
        _, st = R.prefill(cfg, weights, new_len, ids, ts)
        return {"current": M.chain(cfg, weights, new_len, edited, ts, start, counts, st, gemv=gemv), **M.touched(st, new_len, start, counts)}

    ref64, bars, dist = M.routed(w, edit)
    got = {"current": cur.cpu(), **M.touched(_cpu(states), new_len, start, counts)}
    check_against({"case": name, "scenario": "edit", "via": "module"}, got, ref64, bars, dist)
    own = {"current": pre_cur.cpu(), **M.touched(_cpu(pre), new_len, start, counts)}
    print(json.dumps({"case": name, "edit_vs_own_prefill": {q: float((got[q] - own[q]).abs().max()) for q in M.QUANTITIES}}))
    for q in M.QUANTITIES:
        assert float((got[q] - own[q]).abs().max()) <= bars[q], q
    # generate_user_embeddings takes the same arguments
    with torch.inference_mode():
        ids_d = edited.to(dev)
        y, _ = m.generate_user_embeddings(new_len.to(dev), ids_d, m.get_item_embeddings(ids_d), {"timestamps": ts.to(dev)},
                                          delta_x_offsets=(off + start, start), cache=cache, delta_rows=[3] * B, max_delta_rows=4)
    assert torch.equal(y[torch.arange(B), new_len.to(dev) - 1], cur)

    # ---- an append of two events through extend_cache_states, from len_old - 1, against a prefill at the new lengths
    old_len = new_len - 2
    keep = torch.arange(N).unsqueeze(0) < old_len.unsqueeze(1)
    _, old_cache = _enc(m, dev, old_len, ids * keep, ts * keep, return_cache_states=True)
    ext = m.extend_cache_states(old_cache, old_len, new_len)
    assert all(e[1] is o[1] and e[2] is o[2] for e, o in zip(ext, old_cache))
    a_start, a_counts = old_len - 1, torch.full((B,), 3)
    cur, states = _enc(m, dev, new_len, ids, ts, delta_x_offsets=(off + a_start, a_start), cache=ext, delta_rows=a_counts, return_cache_states=True)
    full_cur, full = _enc(m, dev, new_len, ids, ts, return_cache_states=True)

    def append(weights, gemv=None):
        _, st = R.prefill(cfg, weights, old_len, ids * keep, ts * keep)
        st = M.extend_states(st, old_len, new_len)
        return {"current": M.chain(cfg, weights, new_len, ids, ts, a_start, a_counts, st, gemv=gemv), **M.touched(st, new_len, a_start, a_counts)}

    ref64, bars, dist = M.routed(w, append)
    _, st64 = R.prefill(cfg, K._f64(w), new_len, ids, ts)
    pre64 = {"current": R.prefill(cfg, K._f64(w), new_len, ids, ts)[0], **M.touched(st64, new_len, a_start, a_counts)}
    assert all(float((pre64[q] - ref64[q]).abs().max()) <= 1e-11 for q in M.QUANTITIES)     # the recipe: the chain IS the prefill
    got = {"current": cur.cpu(), **M.touched(_cpu(states), new_len, a_start, a_counts)}
    check_against({"case": name, "scenario": "append", "via": "module"}, got, ref64, bars, dist)
    own = {"current": full_cur.cpu(), **M.touched(_cpu(full), new_len, a_start, a_counts)}
    print(json.dumps({"case": name, "append_vs_own_prefill": {q: float((got[q] - own[q]).abs().max()) for q in M.QUANTITIES}}))
    for q in M.QUANTITIES:
        assert float((got[q] - own[q]).abs().max()) <= bars[q], q

    # ---- delta_rows=None is what it was: the same bits as before this module ever took a delta_rows call
    _, cache2 = _enc(m, dev, new_len, ids, ts, return_cache_states=True)
    plain_after = _enc(m, dev, new_len, ids, ts, delta_x_offsets=(off + new_len - 1, new_len - 1), cache=cache2)
    assert torch.equal(plain_after, plain_before)


# ---- 7. the reference's own chained steps -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_reference_fixture(dev, name):
    m, cfg, lengths, ids, ts, _ = fixture_module(name, dev)
    z = np.load(os.path.join(R.GOLDEN, f"hstu_rows_{name}.npz"))
    assert np.array_equal(z["in/past_lengths"], lengths.numpy()) and np.array_equal(z["in/past_ids"], ids.numpy())
    assert os.path.getsize(os.path.join(R.GOLDEN, f"hstu_rows_{name}.npz")) < os.path.getsize(os.path.join(R.GOLDEN, f"hstu_cache_{name}.npz"))
    w64 = K._f64(R.load(name)[1])
    T = lambda key: torch.from_numpy(z[key])   # noqa: E731

    def hold(tag, got, ref64, extra=()):
        figures = {"case": name, "scenario": tag}
        for q in M.QUANTITIES + tuple(extra):
            bar = 2 * float((T(f"{tag}/{q}").double() - ref64[q]).abs().max()) + 1e-6
            err = float((got[q].double() - ref64[q]).abs().max())
            figures[q] = {"bar": bar, "module": err}
        print(json.dumps(figures))
        assert all(v["module"] <= v["bar"] for k, v in figures.items() if isinstance(v, dict)), figures

    # edit
    start, counts, new_ids = T("edit/start"), T("edit/counts"), T("edit/ids")
    off = torch.cumsum(lengths, 0) - lengths
    pre64, st64 = R.prefill(cfg, w64, lengths, ids, ts)
    ref64 = {"prefill_current": pre64, "current": M.chain(cfg, w64, lengths, new_ids, ts, start, counts, st64), **M.touched(st64, lengths, start, counts)}
    pre, cache = _enc(m, dev, lengths, ids, ts, return_cache_states=True)
    cur, states = _enc(m, dev, lengths, new_ids, ts, delta_x_offsets=(off + start, start), cache=cache, delta_rows=counts, return_cache_states=True)
    hold("edit", {"prefill_current": pre.cpu(), "current": cur.cpu(), **M.touched(_cpu(states), lengths, start, counts)}, ref64, ("prefill_current",))
    # append
    old, new, ids_n = T("append/old_lengths"), T("append/new_lengths"), T("append/ids")
    keep = torch.arange(ids.shape[1]).unsqueeze(0) < old.unsqueeze(1)
    off = torch.cumsum(new, 0) - new
    start, counts = old - 1, new - old + 1
    _, st64 = R.prefill(cfg, w64, old, ids_n * keep, ts * keep)
    st64 = M.extend_states(st64, old, new)
    ref64 = {"current": M.chain(cfg, w64, new, ids_n, ts, start, counts, st64), **M.touched(st64, new, start, counts)}
    full64, fst64 = R.prefill(cfg, w64, new, ids_n, ts)
    ref64.update({"prefill_current": full64, **{f"prefill_{k}": v for k, v in M.touched(fst64, new, start, counts).items()}})
    _, cache = _enc(m, dev, old, ids_n * keep, ts * keep, return_cache_states=True)
    ext = m.extend_cache_states(cache, old, new)
    cur, states = _enc(m, dev, new, ids_n, ts, delta_x_offsets=(off + start, start), cache=ext, delta_rows=counts.tolist(), return_cache_states=True)
    full, fstates = _enc(m, dev, new, ids_n, ts, return_cache_states=True)
    got = {"current": cur.cpu(), **M.touched(_cpu(states), new, start, counts), "prefill_current": full.cpu(),
           **{f"prefill_{k}": v for k, v in M.touched(_cpu(fstates), new, start, counts).items()}}
    hold("append", got, ref64, ("prefill_current",) + tuple(f"prefill_{k}" for k in R.ROWS))
