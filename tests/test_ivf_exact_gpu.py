"""The IVF-Flat index kernels (rails_amd/csrc/ivf.hip) through their C entries, on crafted buffers, against tests/_ivf_exact_ref.py --
integers, float64 where the dyadic inputs make it exact, single float32 operations, no kernel of this project.  Every comparison is an
equality: assignments, offsets, list contents, centroids, probe plans and the returned positions.  No row, item or group is left out.

  a. assignment and list build: the 256-point blocks, the LDS centroid chunks, one to three sort tiles, the prefix carry, the limits
  b. one Lloyd step from crafted centroids (no / several / tied / re-split empty lists); init + 1 and 3 iterations against the exact fmaf chain
  c. the list edit against the build of the resulting table
  d. the search on crafted lists: segment edges, the two top-k slots, short lists, arrival orders, ties, slices, NaN and inf
  e. the filtered search, its list words, counts and plan
  f. the same search through engine.IvfIndex (its arrays replaced by the crafted ones)

tests/test_ivf_exact_cpu.py shows on these very inputs that the grid is exact and that every tie and order rule decides some output.
"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import mol_oracle as O
from tests import _ivf_exact_ref as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def E():
    from rails_amd import engine

    return engine


def L():
    from rails_amd import _lib

    return _lib


def lib():
    return L().load()


@functools.lru_cache(maxsize=None)
def spec_of(shape):
    cfg = O.CONFIGS[R.SHAPES[shape][0]]
    names = {f.name for f in dataclasses.fields(E().MolShapeSpec)}
    return E().MolShapeSpec(**{k: v for k, v in dataclasses.asdict(cfg).items() if k in names})


@functools.lru_cache(maxsize=None)
def shape_c(shape):
    return spec_of(shape).to_c("fp32")


def dv(x):
    """numpy -> device; unsigned and half arrays travel as the signed integers of their bits"""
    x = np.ascontiguousarray(x)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.float16): np.int16}.get(x.dtype)
    return torch.from_numpy(x.view(view) if view else x).to(dev())


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return E()._stream()


def ws_of(nbytes):
    assert nbytes > 0, L().last_error()
    return torch.empty(nbytes, dtype=torch.uint8, device=dev())


def same(got, ref):
    ref = torch.from_numpy(np.ascontiguousarray(ref))
    got = got.cpu()
    return got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(got, ref)


# ---- a. assignment and list build ---------------------------------------------------------------------------------------------------
def gpu_build(shape, x16, cent):
    """x16 (G, n, d) float16, cent (G, nlist, d) -> assign, offsets, positions, vectors (int16 bits) on the device"""
    G, n, d = x16.shape
    nlist = cent.shape[1]
    s, xd, cd = shape_c(shape), dv(x16), dv(cent)
    assign = torch.full((G, n), -7, dtype=torch.int32, device=dev())
    L().check(lib().rails_ivf_assign(C.byref(s), None, ptr(xd), n, nlist, ptr(cd), ptr(assign), stream()), "rails_ivf_assign")
    ws = ws_of(lib().rails_ivf_build_workspace_bytes(C.byref(s), n, nlist, 0))
    vec = torch.full((G, n, d), -7, dtype=torch.int16, device=dev())
    pos = torch.full((G, n), -7, dtype=torch.int32, device=dev())
    off = torch.full((G, nlist + 1), -7, dtype=torch.int32, device=dev())
    L().check(lib().rails_ivf_build_lists(C.byref(s), None, ptr(xd), n, nlist, ptr(cd), ptr(vec), ptr(pos), ptr(off), ptr(ws), ws.numel(), stream()),
              "rails_ivf_build_lists")
    return assign, off, pos, vec


def ref_build(x16, cent):
    parts = [R.build_lists(x16[m], cent[m]) for m in range(x16.shape[0])]
    return [np.stack([p[i] for p in parts]) for i in range(4)]


@pytest.mark.parametrize("case", R.BUILD_CASES, ids=lambda c: f"{c.shape}-n{c.n}-nlist{c.nlist}")
def test_assignment_and_list_build(case):
    x16, cent = R.build_inputs(case)
    got = gpu_build(case.shape, x16, cent)
    a, off, pos, vec = ref_build(x16, cent)
    assert same(got[0], a), ("assign", int((got[0].cpu().numpy() != a).sum()))
    assert same(got[1], off), "offsets"
    assert same(got[2], pos), ("positions", int((got[2].cpu().numpy() != pos).sum()))
    assert same(got[3], vec.view(np.int16)), "vectors"
    for lo, hi in R.build_copies(case):              # the higher copy of a centroid never wins: its list is empty
        if lo < hi:
            assert (off[:, hi + 1] == off[:, hi]).all()


def test_build_refusals():
    case = R.BUILD_CASES[0]
    x16, cent = R.build_inputs(case)
    s, xd, cd = shape_c(case.shape), dv(x16), dv(cent)
    G, n, _ = x16.shape
    assign = torch.empty((G, n), dtype=torch.int32, device=dev())
    with pytest.raises(NotImplementedError, match="nlist"):
        L().check(lib().rails_ivf_assign(C.byref(s), None, ptr(xd), n, 4097, ptr(cd), ptr(assign), stream()), "rails_ivf_assign")
    with pytest.raises(ValueError, match="nlist"):
        L().check(lib().rails_ivf_assign(C.byref(s), None, ptr(xd), case.nlist - 1, case.nlist, ptr(cd), ptr(assign), stream()), "rails_ivf_assign")
    with pytest.raises(ValueError, match="exactly one"):
        L().check(lib().rails_ivf_assign(C.byref(s), None, None, n, case.nlist, ptr(cd), ptr(assign), stream()), "rails_ivf_assign")


# ---- b. training ------------------------------------------------------------------------------------------------------------------
def gpu_train(shape, table16, sample, nlist, iters, init, start):
    G, n, d = table16.shape
    s, td, sd = shape_c(shape), dv(table16), dv(sample)
    cent = dv(start) if start is not None else torch.full((G, nlist, d), float("nan"), dtype=torch.float32, device=dev())
    ws = ws_of(lib().rails_ivf_build_workspace_bytes(C.byref(s), n, nlist, len(sample)))
    L().check(lib().rails_ivf_train(C.byref(s), None, ptr(td), n, ptr(sd), len(sample), nlist, iters, init, ptr(cent), ptr(ws), ws.numel(), stream()),
              "rails_ivf_train")
    return cent


@pytest.mark.parametrize("case", R.LLOYD_CASES, ids=lambda c: f"{c.shape}-{c.kind}")
def test_one_lloyd_step(case):
    table, sample, start, _ = R.lloyd_inputs(case)
    got = gpu_train(case.shape, table, sample, R.LLOYD_NLIST, 1, 0, start)
    ref = np.stack([R.lloyd_step(table[m][sample].astype(np.float32), start[m]) for m in range(table.shape[0])])
    assert np.isfinite(ref).all()
    assert same(got, ref), (case, int((got.cpu().numpy() != ref).sum()))


@pytest.mark.parametrize("iters", [1, 3])
def test_training_from_the_first_sample_rows(iters):
    table, sample = R.train_inputs()
    got = gpu_train(R.TRAIN_SHAPE, table, sample, R.TRAIN_NLIST, iters, 1, None)
    ref = np.stack([R.train(table[m][sample].astype(np.float32), R.TRAIN_NLIST, iters) for m in range(table.shape[0])])
    assert np.isfinite(ref).all()
    assert same(got, ref), (iters, int((got.cpu().numpy() != ref).sum()))


# ---- c. the list edit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.EDIT_CASES, ids=lambda c: f"{c.kind}-m{c.m}-inplace{c.in_place}")
def test_list_edit_equals_the_build_of_the_resulting_table(case):
    PQ, G, d = R.geometry(R.EDIT_SHAPE)
    x16, cent = R.edit_base()
    _, old_off, old_pos, old_vec = ref_build(x16, cent)
    pos, n_keep, n_new, rows = R.edit_inputs(case)
    table = R.edited_table(case)
    s = shape_c(R.EDIT_SHAPE)
    src = None
    if case.m:
        src = dv(R.pack_index(table.astype(np.float32).transpose(1, 0, 2) if case.in_place else rows, PQ))
    posd = dv(pos) if case.m else None
    ws = ws_of(lib().rails_ivf_lists_edit_workspace_bytes(C.byref(s), R.EDIT_N, R.EDIT_NLIST, case.m))
    ov, op, oo, cd = dv(old_vec), dv(old_pos), dv(old_off), dv(cent)
    nv = torch.full((G, n_new, d), -7, dtype=torch.int16, device=dev())
    np_ = torch.full((G, n_new), -7, dtype=torch.int32, device=dev())
    no = torch.full((G, R.EDIT_NLIST + 1), -7, dtype=torch.int32, device=dev())
    L().check(lib().rails_ivf_lists_edit(C.byref(s), ptr(src), case.in_place, ptr(posd), case.m, n_keep, R.EDIT_NLIST, ptr(cd), ptr(ov), ptr(op), ptr(oo),
                                         R.EDIT_N, ptr(nv), ptr(np_), ptr(no), n_new, ptr(ws), ws.numel(), stream()), "rails_ivf_lists_edit")
    _, off, order, vec = ref_build(table, cent)
    assert same(no, off), "offsets"
    assert same(np_, order), ("positions", int((np_.cpu().numpy() != order).sum()))
    assert same(nv, vec.view(np.int16)), "vectors"


# ---- d. the search ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def index_dev(shape, kind):
    ix = R.search_index(shape, kind)
    return dv(ix.cent), dv(ix.vec), dv(ix.pos), dv(ix.off)


def gpu_plan(shape, ix, nprobe, k):
    mp, ml = C.c_int32(0), C.c_int32(0)
    off = np.ascontiguousarray(ix.off)
    L().check(lib().rails_ivf_plan(C.byref(shape_c(shape)), C.c_void_p(off.ctypes.data), ix.off.shape[1] - 1, nprobe, k, C.byref(mp), C.byref(ml)), "rails_ivf_plan")
    return mp.value, ml.value


def gpu_search(shape, kind, eq, nprobe, k, max_probes, max_list, words=None, allowed=None, counts=None):
    """-> (positions (B, P_Q * G * k) int64 on the host, the unfilled word).  words / allowed / counts: device tensors of the filtered form."""
    ix = R.search_index(shape, kind)
    cent, vec, pos, off = index_dev(shape, kind)
    B, PQ, _ = eq.shape
    G, nlist, n = ix.cent.shape[0], ix.cent.shape[1], ix.pos.shape[1]
    s, eqd = shape_c(shape), dv(eq)
    ws = ws_of(lib().rails_ivf_search_workspace_bytes(C.byref(s), B, nlist, nprobe, max_probes, max_list, k))
    out = torch.full((B, PQ * G * k), -7, dtype=torch.int64, device=dev())
    unfilled = torch.full((1,), -7, dtype=torch.int32, device=dev())
    if words is None:
        L().check(lib().rails_ivf_search(C.byref(s), ptr(eqd), B, ptr(cent), ptr(vec), ptr(pos), ptr(off), n, nlist, nprobe, max_probes, max_list, k, ptr(ws),
                                         ws.numel(), ptr(out), ptr(unfilled), stream()), "rails_ivf_search")
    else:
        L().check(lib().rails_ivf_search_filtered(C.byref(s), ptr(eqd), B, ptr(cent), ptr(vec), ptr(pos), ptr(off), n, nlist, nprobe, max_probes, max_list, k,
                                                  ptr(ws), ws.numel(), ptr(out), ptr(unfilled), ptr(words), ptr(allowed), ptr(counts), counts.shape[0], stream()),
                  "rails_ivf_search_filtered")
    return out.cpu(), int(unfilled.item())


@pytest.mark.parametrize("case", R.SEARCH_CASES, ids=lambda c: f"{c.shape}-{c.kind}-B{c.B}-k{c.k}-nprobe{c.nprobe}-below{c.below_plan}")
def test_search(case):
    ix, eq = R.search_index(case.shape, case.kind), R.search_queries(case.shape, case.kind, case.B)
    mp, ml = gpu_plan(case.shape, ix, case.nprobe, case.k)
    assert (mp, ml) == R.plan(ix.off, case.nprobe, case.k)
    got, unfilled = gpu_search(case.shape, case.kind, eq, case.nprobe, case.k, mp - case.below_plan, ml)
    ref, ref_unfilled, _, _ = R.search(ix, eq, case.nprobe, case.k, mp - case.below_plan)
    assert unfilled == ref_unfilled == (1 if case.below_plan else 0)
    assert same(got, ref), (case, int((got.numpy() != ref).sum()))
    if not case.below_plan:                          # NaN and inf rows included: k distinct positions everywhere
        rows = np.sort(got.numpy().reshape(-1, case.k), axis=1)
        assert (rows[:, 1:] != rows[:, :-1]).all()


def test_search_refusals():
    shape, kind = "8x8x32", "sixtyfour"
    ix, eq = R.search_index(shape, kind), R.search_queries(shape, kind, 1)
    for nlist_kind, nprobe, k, what in ((kind, 1, 129, "k_per_group"), (kind, 65, 5, "nprobe"), ("small", 7, 5, "nprobe")):
        ix = R.search_index(shape, nlist_kind)
        with pytest.raises(NotImplementedError, match=what):
            cent, vec, pos, off = index_dev(shape, nlist_kind)
            out = torch.empty((1, 64 * k), dtype=torch.int64, device=dev())
            ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev())
            nlist = ix.cent.shape[1]
            L().check(lib().rails_ivf_search(C.byref(shape_c(shape)), ptr(dv(eq)), 1, ptr(cent), ptr(vec), ptr(pos), ptr(off), ix.pos.shape[1], nlist, nprobe,
                                             min(nprobe, nlist), 1, k, ptr(ws), ws.numel(), ptr(out), None, stream()), "rails_ivf_search")


# ---- e. the filtered search ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_list_words_counts_and_filtered_plan(shape):
    ix = R.search_index(shape, "edges")
    G, n = ix.pos.shape
    nlist = ix.cent.shape[1]
    assert n % 32 != 0
    eff, visible = R.filter_words(shape)
    _, _, pos, off = index_dev(shape, "edges")
    words = {}
    for mode, (e, v) in (("eff", (eff, None)), ("visible", (None, visible))):
        out = torch.full((G, n), -7, dtype=torch.int32, device=dev())
        L().check(lib().rails_ivf_list_words(ptr(pos), G, n, ptr(dv(e)) if e is not None else None, ptr(dv(v)) if v is not None else None, ptr(out), stream()),
                  "rails_ivf_list_words")
        ref = R.list_words(ix.pos, n, eff=e, visible=v)
        assert same(out, ref.view(np.int32)), mode
        words[mode] = (out, ref)
    rng = np.random.default_rng(R.seed_of("count rows", shape))
    for rows in (1, 64, 65, 130):                    # the allow words pass through LDS 64 at a time
        allowed = rng.integers(0, 1 << 32, rows, dtype=np.uint64).astype(np.uint32) & rng.choice(np.array([0xF, 0x3, 0xFFFFFFFF, 0x40000000], np.uint32), rows)
        counts = torch.full((rows, G, nlist), -7, dtype=torch.int32, device=dev())
        L().check(lib().rails_ivf_list_counts(ptr(words["eff"][0]), ptr(off), G, n, nlist, ptr(dv(allowed)), rows, ptr(counts), stream()), "rails_ivf_list_counts")
        ref = R.list_counts(ix, words["eff"][1], allowed)
        assert same(counts, ref), rows
        for nprobe, k in ((1, 5), (3, 100), (12, 128)):
            mp = C.c_int32(0)
            L().check(lib().rails_ivf_plan_filtered(C.c_void_p(ref.ctypes.data), rows, G, nlist, nprobe, k, C.byref(mp)), "rails_ivf_plan_filtered")
            assert mp.value == R.plan_filtered(ref, nprobe, k), (rows, nprobe, k)


@pytest.mark.parametrize("case", R.FILTER_CASES, ids=lambda c: f"{c.shape}-B{c.B}-k{c.k}-nprobe{c.nprobe}-{'rows' if c.per_row else 'shared'}")
def test_filtered_search(case):
    ix, eq = R.search_index(case.shape, "edges"), R.search_queries(case.shape, "edges", case.B)
    n = ix.pos.shape[1]
    eff, _ = R.filter_words(case.shape)
    allowed = R.filter_allowed(case)
    words = R.list_words(ix.pos, n, eff=eff)
    counts = R.list_counts(ix, words, allowed if case.per_row else allowed[:1])
    mp = R.plan_filtered(counts, case.nprobe, case.k)
    ml = R.plan(ix.off, case.nprobe, case.k)[1]
    got, unfilled = gpu_search(case.shape, "edges", eq, case.nprobe, case.k, mp, ml, dv(words), dv(allowed), dv(counts))
    ref, ref_unfilled, _, _ = R.search(ix, eq, case.nprobe, case.k, mp, words=words, allowed=allowed)
    assert unfilled == ref_unfilled
    assert same(got, ref), (case, int((got.numpy() != ref).sum()))


# ---- f. through engine.IvfIndex -----------------------------------------------------------------------------------------------------------
def test_search_through_the_python_class():
    """IvfIndex keeps centroids, vectors, positions and offsets as plain attributes: with the crafted arrays in their place its own plan,
    workspace, filter caches and slicing run under the same check."""
    shape, kind, B, k, nprobe = "8x8x32", "edges", 3, 65, 3
    ix, eq = R.search_index(shape, kind), R.search_queries(shape, kind, B)
    G, n = ix.pos.shape
    cfg = O.CONFIGS[R.SHAPES[shape][0]]
    weights = {name: v.to(dev()) for name, v in O.synthetic_weights(cfg, seed=2).items()}
    eng = E().MolEngine(spec_of(shape), weights, precision="fp32")
    items = torch.from_numpy(O.hash_item_table(5, 0, n, cfg.item_embedding_dim)).to(dev())
    cent, vec, pos, off = index_dev(shape, kind)
    ivf = E().IvfIndex(eng, eng.build_index(items), nlist=ix.cent.shape[1], centroids=cent)
    ivf._centroids, ivf._vectors, ivf._positions, ivf._offsets = cent, vec.view(torch.float16), pos, off
    ivf._offsets_host = off.cpu().contiguous()
    ivf._plans.clear()
    mp, _ = R.plan(ix.off, nprobe, k)
    ref, unfilled, _, _ = R.search(ix, eq, nprobe, k, mp)
    assert unfilled == 0
    assert same(ivf.search(dv(eq), k, nprobe=nprobe, check=True), ref)
    _, visible = R.filter_words(shape)
    words = R.list_words(ix.pos, n, visible=visible)
    ones = np.full(B, 0xFFFFFFFF, np.uint32)
    mpf = R.plan_filtered(R.list_counts(ix, words, ones[:1]), nprobe, k)
    ref, unfilled, _, _ = R.search(ix, eq, nprobe, k, mpf, words=words, allowed=ones)
    assert unfilled == 0
    assert same(ivf.search(dv(eq), k, nprobe=nprobe, check=True, filter=dv(visible).view(1, -1)), ref)
