"""HSTU multi-row cached decode step (encode with delta_rows=, rails_hstu_decode_rows), CPU side: the float64 chain of single-row steps
(tests/_hstu_rows_ref.py) is the float64 prefill of the updated sequence, for edits at fixed lengths and for appends decoded from
len_old - 1 (and NOT from len_old, wherever timestamps are used: the next-row timestamp of the relative bias); the bars of the GPU
tests reject the mistakes a multi-row implementation can make; extend_cache_states moves rows and nothing else; encode refuses bad
delta_rows before it touches the library; the C entry validates its arguments without a launch; the new kernels use no scratch.
Every test but the C-entry ones passes with or without the kernels."""
import json
import os
import re
import subprocess

import pytest
import torch

from tests import _hstu_cache_ref as R
from tests import _hstu_decode_cases as K
from tests import _hstu_rows_ref as M

CHAIN_CASES = ("scalar_w30", "scalar_w198", "heads9", "nobias")
MUTANT_CASES = ("scalar_w30", "scalar_w198", "heads9")


@pytest.fixture(scope="module")
def lib():
    from rails_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _dist(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


# ---- 1. the chain is the prefill of the updated sequence ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHAIN_CASES)
def test_float64_chain_of_an_edit_is_the_prefill_of_the_edited_sequence(name):
    """Rows up to a run's end equal the prefill of the edited ids to 1e-12; the rows above an interior run, which no decode step
    touches (the reference leaves them stale as well), keep the old prefill's bits; the result is the postprocessed row len - 1 of
    whichever of the two applies."""
    _, cfg, w = K.build(name)
    w64 = K._f64(w)
    for kind in M.kinds(name):
        r = M.run(name, kind)
        ts = M.ref_ts(name, r)
        _, old = R.prefill(cfg, w64, r.lengths, r.ids, ts)
        cur_new, new = R.prefill(cfg, w64, r.lengths, r.new_ids, ts)
        cur_old = R._postproc(cfg, old[-1][3][torch.cumsum(r.lengths, 0) - 1])
        st = R.clone_states(old)
        cur = M.chain(cfg, w64, r.lengths, r.new_ids, ts, r.start, r.counts, st)
        end = r.start + r.counts
        off = torch.cumsum(r.lengths, 0) - r.lengths
        reaches = end == r.lengths
        assert _dist(cur[reaches], cur_new[reaches]) <= 1e-12 and torch.equal(cur[~reaches], cur_old[~reaches]), (name, kind)
        assert bool((~reaches).any()) == (kind == "ragged")
        N = r.ids.shape[1]
        below_p = torch.arange(N).unsqueeze(0) < end.unsqueeze(1)                     # (B, N): rows of the updated prefill
        below_j = torch.cat([below_p[b, : int(r.lengths[b])] for b in range(len(off))])
        for s, so, sn in zip(st, old, new):
            for t, to, tn, below in ((s[0], so[0], sn[0], below_j), (s[1], so[1], sn[1], below_p), (s[2], so[2], sn[2], below_p),
                                     (s[3], so[3], sn[3], below_j)):
                assert _dist(t[below], tn[below]) <= 1e-12, (name, kind)
                assert torch.equal(t[~below], to[~below]), (name, kind)


def _append_scenario(name):
    """-> (old lengths, new lengths, old ids, new ids, old timestamps (zero past len_old), new timestamps)."""
    c = K.CASES[name]
    r = M.run(name, "uniform2")
    new_len = r.lengths
    grow = 1 + torch.arange(c.B) % 2
    old_len = (new_len - grow).clamp(min=1)
    keep = torch.arange(c.N).unsqueeze(0) < old_len.unsqueeze(1)
    return old_len, new_len, r.new_ids * keep, r.new_ids, r.ts * keep, r.ts


def _append_quantities(cfg, w, dtype, states_ext, old_len, new_len, ids, ts, first, **kw):
    st = [tuple(t.to(dtype, copy=True) for t in s) for s in states_ext]
    cur = M.chain(cfg, w, new_len, ids, ts, first, new_len - first, st, **kw)
    return {"current": cur, **M.touched(st, new_len, old_len - 1, new_len - old_len + 1)}, st


@pytest.mark.parametrize("name", CHAIN_CASES)
def test_append_recipe_is_a_prefill_from_the_old_last_row_and_not_from_the_first_new_row(name):
    c = K.CASES[name]
    _, cfg, w = K.build(name)
    w64 = K._f64(w)
    old_len, new_len, ids_o, ids_n, ts_o, ts_n = _append_scenario(name)
    assert bool((new_len > old_len).all())
    bias = c.rel_bias
    _, old = R.prefill(cfg, w64, old_len, ids_o, ts_o if bias else None)
    cur_new, new = R.prefill(cfg, w64, new_len, ids_n, ts_n if bias else None)
    ext = M.extend_states(old, old_len, new_len)
    # exact arithmetic: the recipe's chain is the prefill at the new lengths, in the whole cache
    got, st = _append_quantities(cfg, w64, torch.float64, ext, old_len, new_len, ids_n, ts_n if bias else None, old_len - 1)
    assert _dist(got["current"], cur_new) <= 1e-12
    valid = torch.arange(c.N).unsqueeze(0) < new_len.unsqueeze(1)
    for s, sn in zip(st, new):
        assert _dist(s[0], sn[0]) <= 1e-12 and _dist(s[3], sn[3]) <= 1e-12
        assert _dist(s[1][valid], sn[1][valid]) <= 1e-12 and _dist(s[2][valid], sn[2][valid]) <= 1e-12
    # the bars of that scenario, from references alone, reject the append decoded from len_old
    ext32 = [tuple(t.float() for t in s) for s in ext]
    ref64, _ = _append_quantities(cfg, w64, torch.float64, ext32, old_len, new_len, ids_n, ts_n if bias else None, old_len - 1)
    blocked, _ = _append_quantities(cfg, w, torch.float32, ext32, old_len, new_len, ids_n, ts_n if bias else None, old_len - 1)
    chained, _ = _append_quantities(cfg, w, torch.float32, ext32, old_len, new_len, ids_n, ts_n if bias else None, old_len - 1, gemv=R.chain_gemv)
    bars, _ = K._bars(ref64, blocked, chained)
    short, _ = _append_quantities(cfg, w64, torch.float64, ext32, old_len, new_len, ids_n, ts_n if bias else None, old_len)
    miss = {q: _dist(short[q], ref64[q]) for q in M.QUANTITIES}
    print(json.dumps({"case": name, "bars": bars, "append_from_len_old": miss}))
    if bias:
        assert miss["current"] > bars["current"] and miss["outputs"] > bars["outputs"], (name, miss, bars)
    else:   # no timestamps anywhere: row len_old - 1 does not change (from the unrounded states; rounding them moves it by 1e-7)
        exact, _ = _append_quantities(cfg, w64, torch.float64, ext, old_len, new_len, ids_n, None, old_len)
        assert all(_dist(exact[q], got[q]) <= 1e-12 for q in M.QUANTITIES), name
        assert all(miss[q] <= bars[q] for q in miss), (name, miss, bars)


def test_decode_limit_restatement_is_the_reference_step_at_its_own_limit():
    """The `limit_end` mutant's own step function, with the key limit at p, is R.decode."""
    name = "heads9"
    _, cfg, w = K.build(name)
    w64 = K._f64(w)
    r = M.run(name, "uniform1")
    _, st = R.prefill(cfg, w64, r.lengths, r.ids, r.ts)
    a, b = R.clone_states(st), R.clone_states(st)
    ca = R.decode(cfg, w64, r.lengths, r.new_ids, r.ts, r.start, a)
    cb = M._decode_limit(cfg, w64, r.lengths, r.new_ids, r.ts, r.start, r.start, b)
    assert _dist(ca, cb) <= 1e-13 and all(_dist(x, y) <= 1e-13 for s, t in zip(a, b) for x, y in zip(s, t))


# ---- 2. the bars reject the mistakes of a multi-row step -----------------------------------------------------------------------------
@pytest.mark.parametrize("bug", M.BUGS)
@pytest.mark.parametrize("name", MUTANT_CASES)
def test_bars_reject_multi_row_mistakes(name, bug):
    d = M.direct(name, "ragged")
    got = M.mutant(name, "ragged", bug)
    miss = {q: _dist(got[q], d.ref64[q]) for q in M.QUANTITIES}
    print(json.dumps({"case": name, "bug": bug, "bars": d.bars, "mutant": miss}))
    assert any(miss[q] > d.bars[q] for q in M.QUANTITIES), (name, bug, miss, d.bars)


def test_unmutated_chain_meets_its_own_bars():
    for name in MUTANT_CASES:
        d = M.direct(name, "ragged")
        assert all(max(d.dist[q]) <= d.bars[q] for q in M.QUANTITIES)


# ---- 3. extend_cache_states --------------------------------------------------------------------------------------------------------
def test_extend_cache_states_moves_rows_and_nothing_else():
    name = "scalar_w30"
    m, cfg, w = K.build(name)
    c = K.CASES[name]
    old = torch.tensor([3, 1, c.N - 2, 5, 2])
    new = torch.tensor([5, 1, c.N, 6, 4])
    g = torch.Generator().manual_seed(3)
    HV, HQ = c.H * c.dv, c.H * c.dqk
    cache = [(torch.randn((int(old.sum()), HV), generator=g), torch.randn((c.B, c.N, HQ), generator=g), torch.randn((c.B, c.N, HQ), generator=g),
              torch.randn((int(old.sum()), c.D), generator=g)) for _ in range(c.blocks)]
    got = m.extend_cache_states(cache, old, new)
    want = M.extend_states(cache, old, new)
    off_n = torch.cumsum(new, 0) - new
    for (v, q, k, o), (wv, _, _, wo), (cv, cq, ck, co) in zip(got, want, cache):
        assert torch.equal(v, wv) and torch.equal(o, wo)
        assert q is cq and k is ck
        assert v.shape == (int(new.sum()), HV) and o.shape == (int(new.sum()), c.D)
        for b in range(c.B):
            assert not bool(v[int(off_n[b] + old[b]): int(off_n[b] + new[b])].any()) and not bool(o[int(off_n[b] + old[b]): int(off_n[b] + new[b])].any())
    assert all(torch.equal(x, y) for s, t in zip(m.extend_cache_states(cache, old.tolist(), new.tolist()), got) for x, y in zip(s, t))
    for bad_old, bad_new in [(old, new[:-1]), (torch.tensor([0, 1, 3, 5, 2]), new), (new + 1, new), (old, torch.tensor([5, 1, c.N + 1, 6, 4])),
                             (old + torch.tensor([1, 0, 0, 0, 0]), new)]:
        with pytest.raises(ValueError):
            m.extend_cache_states(cache, bad_old, bad_new)
    with pytest.raises(ValueError):
        m.extend_cache_states([s[:3] for s in cache], old, new)


# ---- 4. encode's argument errors ----------------------------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """A host tensor that says it lives on the device: what encode sees of device-resident counts, without a device."""
    @property
    def is_cuda(self):
        return True


def test_delta_rows_argument_errors_are_raised_before_any_library_call(monkeypatch):
    from rails_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_library)
    name = "scalar_w30"
    m, cfg, w = K.build(name)
    r = M.run(name, "ragged")
    B = r.lengths.numel()
    emb = m.get_item_embeddings(r.new_ids)
    pay = {"timestamps": r.ts}
    off = torch.cumsum(r.lengths, 0) - r.lengths
    delta = (off + r.start, r.start)
    c = K.CASES[name]
    cache = [(torch.zeros(int(r.lengths.sum()), c.H * c.dv), torch.zeros(B, c.N, c.H * c.dqk), torch.zeros(B, c.N, c.H * c.dqk),
              torch.zeros(int(r.lengths.sum()), c.D)) for _ in range(c.blocks)]
    for call in (m.encode, m.generate_user_embeddings):
        for kw in (dict(delta_rows=2), dict(max_delta_rows=2), dict(delta_rows=2, cache=cache), dict(delta_rows=[1] * B, delta_x_offsets=delta)):
            with pytest.raises(ValueError, match="need delta_x_offsets= and cache="):
                call(r.lengths, r.new_ids, emb, pay, **kw)

        def bad(what, **kw):
            with pytest.raises(ValueError, match=what):
                call(r.lengths, r.new_ids, emb, pay, delta_x_offsets=delta, cache=cache, **kw)

        bad("needs delta_rows=", max_delta_rows=2)
        for v in ("three", [1.0] * B, torch.ones(B), torch.ones(B, dtype=torch.bool), [1] * (B + 1), [[1] * B]):
            bad("delta_rows must be", delta_rows=v)
        bad("delta_rows must lie", delta_rows=0)
        bad("delta_rows must lie", delta_rows=[0] + [1] * (B - 1))
        bad("delta_rows must lie", delta_rows=c.N + 1)
        over = r.counts.clone()
        over[2] = int(r.lengths[2] - r.start[2]) + 1
        bad("end past its length", delta_rows=over)
        bad("end past its length", delta_rows=over.tolist())
        bad("needs max_delta_rows=M", delta_rows=r.counts.as_subclass(_OnDevice))
        bad("less than the largest", delta_rows=r.counts, max_delta_rows=int(r.counts.max()) - 1)
        for v in (0, c.N + 1, 2.0, True):
            bad("max_delta_rows must be", delta_rows=1, max_delta_rows=v)
    assert all(not bool(t.any()) for s in cache for t in s)
    # good arguments get as far as the device check
    with pytest.raises(RuntimeError, match="GPU only"):
        m.encode(r.lengths, r.new_ids, emb, pay, delta_x_offsets=delta, cache=cache, delta_rows=r.counts)


# ---- 5. the C entry, without a device -------------------------------------------------------------------------------------------------
def rows_supported(N, D, H, dqk, dv, buckets):
    """rails_hstu_decode_rows_supported, restated: the single-row kernel's limits and the staged tile's LDS bound H dv <= 1024."""
    return N >= 1 and 1 <= D <= 1024 and H >= 1 and 1 <= dqk <= 32 and 1 <= dv <= 32 and 0 <= buckets <= 255 and H * dv <= 1024


ROWS_BOUNDARY_PAIRS = {
    "D": ((9, 1024, 2, 32, 32, 0), (9, 1025, 2, 32, 32, 0)),
    "dqk": ((9, 64, 2, 32, 32, 0), (9, 64, 2, 33, 32, 0)),
    "dv": ((9, 64, 2, 32, 32, 0), (9, 64, 2, 32, 33, 0)),
    "buckets": ((9, 64, 2, 32, 32, 255), (9, 64, 2, 32, 32, 256)),
    "N": ((1, 64, 2, 32, 32, 0), (0, 64, 2, 32, 32, 0)),
    "H dv": ((9, 64, 32, 32, 32, 0), (9, 64, 33, 32, 32, 0)),
    "H dv, dv 31": ((9, 64, 33, 32, 31, 0), (9, 64, 34, 32, 31, 0)),
    "H": ((9, 64, 1, 32, 32, 0), (9, 64, 0, 32, 32, 0)),
}


def test_rows_supported_agrees_with_its_restatement_on_both_sides_of_every_limit(lib):
    for limit, (good, bad) in ROWS_BOUNDARY_PAIRS.items():
        assert rows_supported(*good) and not rows_supported(*bad), limit
        assert lib.rails_hstu_decode_rows_supported(*good) == 1 and lib.rails_hstu_decode_rows_supported(*bad) == 0, limit
    for name, c in K.CASES.items():
        assert lib.rails_hstu_decode_rows_supported(c.N, c.D, c.H, c.dqk, c.dv, c.buckets) == int(rows_supported(c.N, c.D, c.H, c.dqk, c.dv, c.buckets)), name


def test_decode_rows_entry_rejects_bad_arguments_without_a_launch(lib):
    """Fails on a library without rails_hstu_decode_rows."""
    from rails_amd import _lib

    p = 16   # a non-NULL address that is never dereferenced: validation fails before any launch
    #     emb ids pos counts max_rows len ts thr pos_emb layers blocks B  N  cache_rows D  H dqk dv buckets act mode eps  work out
    ok = [p, p, p, p, 3, p, p, p, p, p, 2, 4, 19, 40, 24, 1, 8, 7, 128, 1, 0, 1e-6, p, p]
    dec = lib.rails_hstu_decode_rows
    for i, v, code, what in [(0, None, _lib.RAILS_EINVAL, "NULL"), (1, None, _lib.RAILS_EINVAL, "NULL"), (2, None, _lib.RAILS_EINVAL, "NULL"),
                             (5, None, _lib.RAILS_EINVAL, "NULL"), (8, None, _lib.RAILS_EINVAL, "NULL"), (9, None, _lib.RAILS_EINVAL, "NULL"),
                             (22, None, _lib.RAILS_EINVAL, "NULL"), (23, None, _lib.RAILS_EINVAL, "NULL"),
                             (4, 0, _lib.RAILS_EINVAL, "max_rows"), (4, -2, _lib.RAILS_EINVAL, "max_rows"), (4, 20, _lib.RAILS_EINVAL, "max_rows"),
                             (11, -1, _lib.RAILS_EINVAL, "bad size"), (10, 0, _lib.RAILS_EINVAL, "bad size"), (13, 3, _lib.RAILS_EINVAL, "bad size"),
                             (7, None, _lib.RAILS_EINVAL, "threshold"), (19, 2, _lib.RAILS_EINVAL, "linear_act"),
                             (14, 1025, _lib.RAILS_ENOTSUP, "not supported"), (16, 33, _lib.RAILS_ENOTSUP, "not supported"),
                             (17, 33, _lib.RAILS_ENOTSUP, "not supported"), (18, 256, _lib.RAILS_ENOTSUP, "not supported"),
                             (15, 147, _lib.RAILS_ENOTSUP, "not supported")]:
        args = list(ok)
        args[i] = v
        assert dec(*args, None) == code, (i, v, _lib.last_error())
        assert _lib.last_error().startswith("hstu_decode_rows") and what in _lib.last_error(), (i, _lib.last_error())
    # counts may be NULL (max_rows everywhere), timestamps too (no bias): both reach the geometry check below
    # the launch-grid limit, named, before any launch: batch x max_rows work rows
    assert _lib.RAILS_HSTU_DECODE_MAX_ROWS == 65535 * 32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rails_amd.h")).read()
    assert f"#define RAILS_HSTU_DECODE_MAX_ROWS {_lib.RAILS_HSTU_DECODE_MAX_ROWS} " in header
    args = list(ok)
    args[11], args[4], args[13] = _lib.RAILS_HSTU_DECODE_MAX_ROWS // 19 + 1, 19, 10 ** 9
    assert dec(*args, None) == _lib.RAILS_EINVAL
    assert "work rows" in _lib.last_error() and str(_lib.RAILS_HSTU_DECODE_MAX_ROWS) in _lib.last_error()
    args = list(ok)
    args[11] = 0          # an empty batch is a no-op, even with no pointers
    args[0] = args[3] = args[9] = args[22] = args[23] = None
    args[13] = 0
    assert dec(*args, None) == _lib.RAILS_OK
    # the workspace: the work rows' x, u and a, and the sequence table
    ws = lib.rails_hstu_decode_rows_workspace_floats
    assert ws(12, 4, 24, 1, 8, 7) >= 12 * (24 + 2 * 7) + 3 * 4 and ws(-1, 4, 24, 1, 8, 7) == 0


# ---- 6. resources -------------------------------------------------------------------------------------------------------------------
def test_rows_kernels_use_no_scratch():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-readelf")) and os.path.exists(os.path.join(llvm, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(root, "rails_amd", "csrc", "hstu_rows.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(root, "tools", "kernel_resources.sh"), "hsturows"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"vgpr\s+(\d+) agpr\s+\d+ sgpr\s+\d+ scratch\s+(\d+) lds\s+\d+\s+.*(hsturows_\w+_kernel(?:<[^>]*>)?)", line.strip()) for line in out.splitlines()]
    got = {m.group(3): int(m.group(2)) for m in rows if m}
    assert set(got) == {"hsturows_scan_kernel", "hsturows_gemm_kernel<0>", "hsturows_gemm_kernel<1>", "hsturows_attn_kernel", "hsturows_post_kernel"}, out
    assert all(s == 0 for s in got.values()), got
