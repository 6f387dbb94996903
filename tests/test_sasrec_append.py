"""SASRec multi-row cached decode step (encode with cache= and new_rows=), CPU side: the float64 multi-row step built from the
single-row step (tests/_sasrec_append_ref.py) is the float64 encode of the updated sequence and, block by block over work-row slots
as the kernels run it, the same numbers; on the fixture chains (state 0 straight to state 3, tests/golden/sasrec_decode_*.npz) the
bars of the GPU tests reject each mistake a multi-row implementation can make; the new C entry validates its arguments, the slot
limit included, without a launch; the module refuses bad new_rows before it touches a device.  These tests calibrate the bars: they
pass with or without the kernels' multi-row path."""
import functools
import os
import re
import subprocess

import pytest
import torch

from tests import _sasrec_append_ref as A
from tests import _sasrec_decode_ref as R
from tests import _sasrec_ref as S
from tests.test_sasrec import build, tolerance


@pytest.fixture(scope="module")
def lib():
    from rails_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def state0(name):
    """(fixture, the float64 cache of chain state 0, the step to state 3): computed once, never modified."""
    f = R.load(name)
    L, I = torch.from_numpy(f["chain/lengths"]), torch.from_numpy(f["chain/ids"])
    return f, R.prefill64(f, L[0], I[0])[1], A.fixture_step(f)


@pytest.mark.parametrize("name", S.GEOMETRIES)
def test_fixture_step_is_ragged_on_its_own(name):
    f, _, (L3, I3, m) = state0(name)
    N = f["cfg"]["N"]
    L0 = torch.from_numpy(f["chain/lengths"][0])
    assert int(m[0]) == 1 and int(L0[0]) == N                     # saturated: a replace-last row, one new row
    assert bool((m[L0 <= N - 3] == 3).all()) and int(m.max()) == 3 and int(m.min()) == 1
    assert bool((m <= L3).all())
    assert any(int(I3[b, p]) == 0 for b in range(len(m)) for p in range(int(L3[b] - m[b]), int(L3[b]) - 1))   # an id 0 among the new rows, not last


@pytest.mark.parametrize("name", S.GEOMETRIES)
def test_multi_row_step_is_the_float64_encode_of_the_updated_sequence(name):
    f, c0, (L3, I3, m) = state0(name)
    cur, cache = A.append64(f, c0, L3, I3, m)
    assert R.distance(cur, S.encoder64(f, ids=I3, lengths=L3)[1]) <= 1e-9
    assert R.distance(cur, R.chain64(f)[3]) <= 1e-9                # ... and the chain's three single steps
    assert R.distance(cur, torch.from_numpy(f["chain/out"][3])) <= tolerance(f)
    _, fresh = R.prefill64(f, L3, I3)
    B, N = I3.shape
    new = (torch.arange(N) >= (L3 - m).unsqueeze(1)) & (torch.arange(N) < L3.unsqueeze(1))
    for (k, v), (k0, v0), (kf, vf) in zip(cache, c0, fresh):
        for t, t0, tf in ((k, k0, kf), (v, v0, vf)):
            assert torch.equal(t[~new], t0[~new])
            assert R.distance(t[new], tf[new]) <= 1e-9
    # the slot form, as the kernels run it, with more slots than any sequence uses as well
    for M in (None, 5):
        cur2, cache2 = A.rows64(f, c0, L3, I3, m, M=M)
        assert R.distance(cur2, cur) <= 1e-12
        assert all(R.distance(x, y) <= 1e-12 for p, q in zip(cache2, cache) for x, y in zip(p, q))


def test_single_steps_lengths():
    L, m = torch.tensor([10, 4, 7]), torch.tensor([1, 3, 2])
    assert [s.tolist() for s in A.single_steps(L, m)] == [[10, 2, 6], [10, 3, 7], [10, 4, 7]]


# bug -> the fixture geometries whose OUTPUT separates it (measured on the CPU; every other geometry is listed in the docstring below)
SEPARATES = {bug: list(S.GEOMETRIES) for bug in A.BUGS}
SEPARATES["sees_later_new_rows"] = ["amzn-books", "amzn-books-gelu", "ml-1m"]


@pytest.mark.parametrize("bug", A.BUGS)
def test_tolerance_rejects_multi_row_bugs(bug):
    """Each mistake lands more than 10 x tolerance(f) from the reference's chain/out[3] (the GPU test allows 2 x tolerance) on the
    geometries of SEPARATES, asserted on each of them: all four, except that ml-20m does not separate `sees_later_new_rows` in the
    output (0.08 x tolerance: the last new row, whose embedding is the output, sees no later row, and the earlier new rows' changed
    k / v of the deeper blocks barely move it there) -- amzn-books (6 000 x), amzn-books-gelu (900 x) and ml-1m (150 x) do.
    `inactive_slot_writes` shows in the output only through a sequence saturated at N, whose idle slots clamp onto its own new row
    (row 0 of every fixture).  Elsewhere an idle slot lands on a row >= len, which in a prefilled cache already holds what a zero
    row writes (the in-projection bias): no number changes there, and the GPU tests catch it on a cache filled with NaN instead
    (rows >= len stay NaN) and bitwise on a prefilled one whose rows >= len were overwritten with random numbers.  Not a mistake, so
    not here: a first new row one too LOW with the last one in place (one row more than needed is re-encoded, to the bits it had)."""
    for name in S.GEOMETRIES:
        f, c0, (L3, I3, m) = state0(name)
        out, _ = A.rows64(f, c0, L3, I3, m, bug=bug)
        miss = R.distance(out, torch.from_numpy(f["chain/out"][3]))
        if name in SEPARATES[bug]:
            assert miss > 10 * tolerance(f), (bug, name, miss, tolerance(f))


def test_decode_rows_entry_rejects_bad_arguments_without_a_launch(lib):
    import ctypes as C

    from rails_amd import _lib

    p = 16   # a non-NULL address that is never dereferenced: validation fails before any launch
    layers = (C.c_void_p * 20)(*([p] * 20))
    #     emb ids len counts max_new pos layers blocks B  N   D  H  F   act                postproc eps work out
    ok = [p, p, p, p, 3, p, layers, 2, 4, 51, 64, 4, 64, _lib.RAILS_ACT_RELU, 0, 1e-6, p, p]
    dec = lib.rails_sasrec_decode_rows
    for i, v, code, what in [(0, None, _lib.RAILS_EINVAL, "NULL"), (2, None, _lib.RAILS_EINVAL, "NULL"), (16, None, _lib.RAILS_EINVAL, "NULL"),
                             (8, -1, _lib.RAILS_EINVAL, "bad size"), (9, 2049, _lib.RAILS_ENOTSUP, "not supported"),
                             (4, 0, _lib.RAILS_ENOTSUP, "max_new"), (4, -3, _lib.RAILS_ENOTSUP, "max_new"),
                             (4, 52, _lib.RAILS_ENOTSUP, "max_new")]:
        args = list(ok)
        args[i] = v
        assert dec(*args, None) == code, (i, v)
        assert _lib.last_error().startswith("sasrec_decode_rows") and what in _lib.last_error(), (i, _lib.last_error())
    # the launch-grid limit, named, before any launch: batch x max_new work rows
    assert _lib.RAILS_SASREC_DECODE_MAX_ROWS == 65535 * 32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rails_amd.h")).read()
    assert f"#define RAILS_SASREC_DECODE_MAX_ROWS {_lib.RAILS_SASREC_DECODE_MAX_ROWS} " in header
    args = list(ok)
    args[8], args[4] = _lib.RAILS_SASREC_DECODE_MAX_ROWS // 51 + 1, 51
    assert dec(*args, None) == _lib.RAILS_ENOTSUP
    assert "work rows" in _lib.last_error() and str(_lib.RAILS_SASREC_DECODE_MAX_ROWS) in _lib.last_error()
    args[11] = 16         # the limit does not depend on the heads: the slot attention grid has them on its y
    assert dec(*args, None) == _lib.RAILS_ENOTSUP and str(_lib.RAILS_SASREC_DECODE_MAX_ROWS) in _lib.last_error()
    args = list(ok)
    args[8] = 0           # an empty batch is a no-op, even with no pointers
    args[0] = args[3] = args[6] = args[16] = args[17] = None
    assert dec(*args, None) == _lib.RAILS_OK


def test_new_rows_api_errors(monkeypatch):
    """What encode refuses before it reaches a device: new_rows without a cache, and (with the device check out of the way) host
    counts of 0, of len + 1, of the wrong shape or dtype, a max_new_rows below the largest count or out of range."""
    f = S.load("amzn-books")
    c = f["cfg"]
    m = build(f)
    ids = torch.from_numpy(f["in/past_ids"])
    lengths = torch.from_numpy(f["in/past_lengths"])
    B, N, D = ids.shape + (c["D"],)
    emb = m.get_item_embeddings(ids)
    for kw in (dict(new_rows=2), dict(new_rows=[1] * B), dict(max_new_rows=2), dict(new_rows=2, return_cache_states=True)):
        with pytest.raises(ValueError, match="need cache="):
            m.encode(lengths, ids, emb, {}, **kw)
    cache = [(torch.zeros(B, N, D), torch.zeros(B, N, D)) for _ in range(c["blocks"])]
    with pytest.raises(RuntimeError, match="GPU only"):
        m.encode(lengths, ids, emb, {}, cache=cache, new_rows=1)
    with pytest.raises(ValueError, match="needs new_rows="):
        m.encode(lengths, ids, emb, {}, cache=cache, max_new_rows=2)
    monkeypatch.setattr(type(m), "_check_device", lambda self, t: None)   # reach the host-side checks without a GPU
    short = int(lengths.argmin())
    over = [1] * B
    over[short] = int(lengths[short]) + 1
    for bad, what in [(0, "new_rows must lie"), ([0] + [1] * (B - 1), "new_rows must lie"), (over, "new rows and length"), (N + 1, "new_rows must lie"),
                      ([1] * (B + 1), "shape"), ([[1] * B], "shape"), (torch.ones(B), "integer"), ([1.0] * B, "integer"),
                      (torch.ones(B, dtype=torch.bool), "integer"), ("three", "new_rows must be")]:
        with pytest.raises(ValueError, match=what):
            m.encode(lengths, ids, emb, {}, cache=cache, new_rows=bad)
    for kw, what in [(dict(new_rows=[1] * (B - 1) + [1], max_new_rows=0), "max_new_rows must be"), (dict(new_rows=1, max_new_rows=N + 1), "max_new_rows must be"),
                     (dict(new_rows=1, max_new_rows=2.0), "max_new_rows must be"), (dict(new_rows=1, max_new_rows=True), "max_new_rows must be")]:
        with pytest.raises(ValueError, match=what):
            m.encode(lengths, ids, emb, {}, cache=cache, **kw)
    full = torch.full((B,), N)
    with pytest.raises(ValueError, match="less than the largest"):
        m.encode(full, ids, emb, {}, cache=cache, new_rows=[3] + [1] * (B - 1), max_new_rows=2)
    assert all(not bool(t.any()) for kv in cache for t in kv)


def test_slot_kernels_use_no_scratch_and_no_more_registers():
    """The slot-scheme instances of the decode kernels (kv_rows_kernel / kv_attn_kernel over KvSlotArgs, kvslot_post_kernel) beside
    the single-row ones (over KvDecArgs, kvdec_post_kernel): twelve, no scratch, and the VGPRs of their single-row twins."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-readelf")) and os.path.exists(os.path.join(llvm, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(root, "rails_amd", "csrc", "kvdec.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(root, "tools", "kernel_resources.sh"), "kv_rows_kernel|kv_attn_kernel|kvslot_post|kvdec_post"],
                         capture_output=True, text=True, timeout=600).stdout
    # an instance's twin key: its name and template arguments without the SLOTS flag and the argument block (kv_rows_kernel<0, true>),
    # the post kernels' without their prefix; it is a slot instance iff it takes a KvSlotArgs
    rows = [re.match(r"vgpr\s+(\d+) agpr\s+\d+ sgpr\s+\d+ scratch\s+(\d+) lds\s+\d+\s+(?:void )?mol::(?:kvdec_|kvslot_)?(\w+_kernel)"
                     r"(?:<(.*?), (?:true|false), mol::Kv\w+Args>)?\((mol::Kv(?:Slot|Dec)Args|float const\*)", line.strip()) for line in out.splitlines()]
    got = {(m.group(5) == "mol::KvSlotArgs", m.group(3), m.group(4)): (int(m.group(1)), int(m.group(2))) for m in rows if m}
    slot = {k[1:]: v for k, v in got.items() if k[0]}
    single = {k[1:]: v for k, v in got.items() if not k[0]}
    assert len(slot) == 12 and set(slot) == set(single), out
    assert all(scratch == 0 for _, scratch in list(slot.values()) + list(single.values())), (slot, single)
    assert all(slot[k][0] <= single[k][0] for k in slot), (slot, single)
