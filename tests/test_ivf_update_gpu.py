"""GPU: MoLNaiveTopK(use_faiss=True, frozen_centroids=True) follows update_items / append_items / remove_items and the by-id calls
(DESIGN sections 3.10 and 3.12).  The contract is NOT "equals a freshly constructed module" (that one would train new centroids): after
every call the centroids are bit for bit what they were, and vectors / positions / offsets are torch.equal to what rails_ivf_build_lists
writes from the resulting table with those centroids -- the TWIN, engine.IvfIndex(engine, index of the resulting table, centroids=...),
and in module form MoLNaiveTopK(..., ivf_centroids=...).  Search at nprobe = 1 and nprobe = nlist, forward and get_top_k_outputs equal the
twin's.  The resulting table is kept by a mirror in this file (removal_plan's tail-fill rule), not read back from the module.  Shapes are
the smallest that cross the kernels' boundaries: N = 4096 + 37 (one 4096-slot scan tile boundary in the middle of a list at nlist = 5),
the 32-item index tile, the 16 384-entry limit of one edit call."""
import numpy as np
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from rails_amd.topk_modules import removal_plan
from tests import _ivf_ref as R
from tests.test_generic_route_gpu import build_module
from tests.test_index_update_gpu import ids_of, same, table

pytestmark = pytest.mark.gpu
B, KG, NLIST, N0 = 8, 5, 5, 4096 + 37
NEAR = 1e-6        # centroid scores closer than this are near-ties (tests/test_ivf_gpu.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_MOLS = {}


def setup(route, dev):
    """-> (cfg, mol, q): amzn-books (d = 32) in fp32 or split-f16 precision, or the 16x16x64 shape (d = 64)."""
    if route not in _MOLS:
        cfg = O.CONFIGS["synthetic-16x16x64" if route == "c4" else "amzn-books"]
        mol = build_module(cfg, O.synthetic_weights(cfg, seed=1), dev, precision="f16x3" if route == "f16x3" else None)
        _MOLS[route] = (cfg, mol, O.synthetic_queries(cfg, B, seed=3).to(dev))
    return _MOLS[route]


def make(mol, X, ids, nlist=NLIST, **kw):
    return rails_amd.MoLNaiveTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0), k_per_group=KG, use_faiss=True, nlist=nlist, **kw)


class Mirror:
    """The table and ids the calls must leave: update writes rows, append concatenates, remove fills the holes from the tail."""

    def __init__(self, X, ids):
        self.X, self.ids = X.clone(), ids.clone()

    def update(self, pos, rows, ids=None):
        self.X[pos.to(self.X.device)] = rows
        if ids is not None:
            self.ids[pos.to(self.X.device)] = ids

    def append(self, rows, ids):
        self.X, self.ids = torch.cat([self.X, rows]), torch.cat([self.ids, ids])

    def remove(self, pos):
        n = self.X.shape[0]
        holes, movers = removal_plan(pos.cpu(), n)
        n_new = n - pos.numel()
        X, ids = self.X[:n_new].clone(), self.ids[:n_new].clone()
        X[holes.to(X.device)] = self.X[movers.to(X.device)]
        ids[holes.to(X.device)] = self.ids[movers.to(X.device)]
        self.X, self.ids = X, ids


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def lists_equal(a, b, what):
    assert a.n_items == b.n_items, (what, a.n_items, b.n_items)
    for name in ("vectors", "positions", "offsets", "centroids"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name, x.shape, y.shape)
        assert torch.equal(bits(x), bits(y)), (what, name)


def check(tk, mol, mir, q, cent0, what, module_calls=True):
    """The edited module against its twins built from the mirror's table with the centroids from before the edits."""
    ivf = tk._ivf
    assert ivf is not None and tk.num_items == mir.X.shape[0] == ivf.n_items, what
    assert torch.equal(bits(ivf.centroids), bits(cent0)), f"{what}: the centroids were written"
    same(tk._item_embeddings[0], mir.X, f"{what}: table")
    same(tk._ids_flat, mir.ids, f"{what}: ids")
    eng = tk._bind()
    twin = E.IvfIndex(eng, eng.build_index(mir.X), nlist=ivf.nlist, centroids=cent0, items=mir.X)
    lists_equal(ivf, twin, what)
    assert torch.equal(ivf.list_sizes(), twin.list_sizes()), what
    _, eq, _ = eng.query_pack(q, None, want_plain=True)
    for nprobe in (1, ivf.nlist):
        assert torch.equal(ivf.search(eq, KG, nprobe=nprobe, check=True), twin.search(eq, KG, nprobe=nprobe, check=True)), (what, nprobe)
    if module_calls:
        other = make(mol, mir.X, mir.ids, nlist=ivf.nlist, ivf_centroids=cent0, frozen_centroids=True)
        n = mir.X.shape[0]
        got, want = tk(q, k=10), other(q, k=10)
        same(got, want, f"{what}: forward")
        lists_equal(tk._ivf, other._ivf, f"{what}: module twin")
        cand = rails_amd.CandidateIndex(ids=mir.ids.reshape(1, -1), embeddings=mir.X.unsqueeze(0))
        k_out = min(50, max(1, n // 2))
        seen = want[1][:, :61].contiguous() if n >= 1000 else None
        same(cand.get_top_k_outputs(q, k_out, {}, tk, seen)[:2], cand.get_top_k_outputs(q, k_out, {}, other, seen)[:2], f"{what}: get_top_k_outputs")
    return twin


def list_of_position(ivf, g=0):
    """(N,) the list that holds each position in group g (host)."""
    off, pos = ivf.offsets[g].cpu().long(), ivf.positions[g].cpu().long()
    lists = torch.repeat_interleave(torch.arange(ivf.nlist), off[1:] - off[:-1])
    out = torch.empty(ivf.n_items, dtype=torch.int64)
    out[pos] = lists
    return out


def members(ivf, l, g=0):
    off = ivf.offsets[g].cpu().long()
    return ivf.positions[g, off[l] : off[l + 1]].cpu().long()


def start(route, dev, n=N0, nlist=NLIST, seed=21):
    cfg, mol, q = setup(route, dev)
    X, ids = table(cfg, n, seed, dev), ids_of(n, dev)
    tk = make(mol, X, ids, nlist=nlist, frozen_centroids=True)
    ivf = tk.ivf_index()
    return cfg, mol, q, tk, Mirror(X, ids), ivf.centroids.clone()


def numpy_oracle(ivf, eng, X):
    """tests/_ivf_ref.build_lists on the fp16-rounded components of the table X, tie-aware as tests/test_ivf_gpu.py's build invariants."""
    ex16 = eng.unpack_index(eng.build_index(X), want_gi=False)[0].half().cpu()
    off, pos, vec, c = ivf.offsets.cpu().long(), ivf.positions.cpu().long(), ivf.vectors.cpu(), ivf.centroids.cpu().double().numpy()
    n = X.shape[0]
    for g in range(ivf.groups):
        assert off[g, 0] == 0 and off[g, -1] == n and bool((off[g, 1:] >= off[g, :-1]).all())
        assert torch.equal(torch.sort(pos[g]).values, torch.arange(n))
        assert torch.equal(vec[g].view(torch.int16), ex16[pos[g], g].view(torch.int16))
        x = ex16[:, g].double().numpy()
        a, gap = R.assign(x, c[g])
        if (gap >= NEAR).all():      # no near-tie between two centroids: the reference's lists are THE lists
            order, offsets = R.build_lists(x, c[g])
            assert np.array_equal(order, pos[g].numpy()) and np.array_equal(offsets, off[g].numpy()), g
        else:
            lists = torch.repeat_interleave(torch.arange(ivf.nlist), off[g, 1:] - off[g, :-1]).numpy()
            wrong = (a[pos[g].numpy()] != lists) & (gap[pos[g].numpy()] >= NEAR)
            assert not wrong.any(), g
            inside = lists[1:] == lists[:-1]
            assert bool((pos[g, 1:][inside] > pos[g, :-1][inside]).all())


# ---- update ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 300])
def test_update(dev, m):
    cfg, mol, q, tk, mir, cent0 = start("fp32", dev)
    ivf, n = tk._ivf, N0
    home = list_of_position(ivf)
    g = torch.Generator().manual_seed(5)
    if m == 1:
        pos = torch.tensor([4095])
    else:
        fixed = torch.tensor([0, n - 1, 4095, 4096, 31, 32])
        rest = torch.randperm(n, generator=g)
        pos = torch.cat([fixed, rest[~torch.isin(rest, fixed)][: m - fixed.numel()]])
    rows = table(cfg, m, 77, dev, first=5_000_000)
    moved = min(m, 40)
    for j in range(moved):             # planted on another centroid: the row of a member of the next list of group 0
        rows[j] = mir.X[members(ivf, (int(home[pos[j]]) + 1) % NLIST)[j % 7]]
    for j in range(moved, min(m, 80)):  # planted on their own: the row of another member of the list they are in
        rows[j] = mir.X[members(ivf, int(home[pos[j]]))[j % 7]]
    tk.update_items(pos.to(dev) if m > 1 else pos, rows)
    mir.update(pos, rows)
    check(tk, mol, mir, q, cent0, f"update M = {m}")
    now = list_of_position(tk._ivf)
    assert bool((now[pos[:moved]] != home[pos[:moved]]).all()), "the planted rows did not change lists"
    if m > 1:
        assert bool((now[pos[moved:80]] == home[pos[moved:80]]).all())
        numpy_oracle(tk._ivf, tk._bind(), mir.X)


# ---- append ---------------------------------------------------------------------------------------------------------------------
def test_append_across_the_tiles(dev):
    cfg, mol, q, tk, mir, cent0 = start("fp32", dev, n=4000)
    target = members(tk._ivf, 2)[3]
    first = 4000
    for step, m in enumerate((96, 1, 4203)):       # 4000 -> 4096 -> 4097 -> 8300
        rows = mir.X[target].unsqueeze(0).repeat(m, 1)      # every row planted on one centroid: the tail of one list per group
        ids = ids_of(m, dev, first=first)
        sizes = tk._ivf.list_sizes()
        tk.append_items(rows, ids)
        mir.append(rows, ids)
        first += m
        check(tk, mol, mir, q, cent0, f"append {m}", module_calls=step != 1)
        grown = tk._ivf.list_sizes() - sizes
        assert bool(((grown == 0) | (grown == m)).all()) and int(grown.sum()) == m * tk._ivf.groups and int(grown[0, 2]) == m
    assert tk.num_items == 8300


# ---- remove ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tail", "holes", "mixed", "empty_list", "down_to_nlist"])
def test_remove(dev, kind):
    cfg, mol, q, tk, mir, cent0 = start("fp32", dev)
    n, ivf = N0, tk._ivf
    g = torch.Generator().manual_seed(9)
    if kind == "tail":               # no holes: a pure truncation (across the 4096 boundary)
        pos = torch.arange(n - 50, n)
    elif kind == "holes":            # every removed position below N': as many movers from the tail
        pos = torch.cat([torch.tensor([0, 31, 32, 4000]), torch.randperm(n - 200, generator=g)[:90] + 40])
        pos = torch.unique(pos)
    elif kind == "mixed":
        pos = torch.unique(torch.cat([torch.tensor([0, 4095, 4096, n - 1, n - 2]), torch.randperm(n, generator=g)[:300]]))
    elif kind == "empty_list":       # every member of list 1 of group 0
        pos = members(ivf, 1)
    else:
        pos = torch.randperm(n, generator=g)[: n - NLIST]
    pos = pos[torch.randperm(pos.numel(), generator=g)]
    moved = tk.remove_items(pos.to(dev))
    mir.remove(pos)
    assert moved.shape[1] == 2
    check(tk, mol, mir, q, cent0, f"remove {kind}")
    if kind == "empty_list":
        assert int(tk._ivf.list_sizes()[0, 1]) == 0
    if kind == "down_to_nlist":
        assert tk.num_items == NLIST


def test_remove_below_nlist_is_refused_untouched(dev):
    cfg, mol, q, tk, mir, cent0 = start("fp32", dev)
    ivf = tk._ivf
    before = {t: getattr(ivf, t).clone() for t in ("vectors", "positions", "offsets", "centroids")}
    table0, ids0, buf0 = tk._item_embeddings, tk._item_ids, tk._index.buf.clone()
    with pytest.raises(ValueError, match="nlist"):
        tk.remove_items(torch.randperm(N0)[: N0 - NLIST + 1].to(dev))
    assert tk._ivf is ivf and tk._item_embeddings is table0 and tk._item_ids is ids0 and tk.num_items == N0 == ivf.n_items
    for t, v in before.items():
        assert torch.equal(bits(getattr(ivf, t)), bits(v)), t
    same(tk._item_embeddings[0], mir.X, "table")
    same(tk._ids_flat, mir.ids, "ids")
    assert torch.equal(bits(tk._index.buf), bits(buf0))
    check(tk, mol, mir, q, cent0, "after the refusal", module_calls=False)


# ---- chains and the by-id calls --------------------------------------------------------------------------------------------------
def test_chain_of_ten_steps_with_by_id_calls(dev):
    cfg, mol, q, tk, mir, cent0 = start("fp32", dev, n=4090)
    g = torch.Generator().manual_seed(13)
    next_id = 4090
    for step in range(10):
        n = tk.num_items
        op = ("update", "append", "remove", "upsert", "append", "remove_by_id", "update", "remove", "append", "update")[step]
        if op == "update":
            pos = torch.randperm(n, generator=g)[:57]
            rows = table(cfg, 57, 100 + step, dev, first=6_000_000)
            rows[:20] = mir.X[torch.randperm(n, generator=g)[:20].to(dev)]      # (rows of other items: most change lists)
            tk.update_items(pos, rows)
            mir.update(pos, rows)
        elif op == "append":
            m = (9, 40, 1)[step % 3]
            rows, ids = table(cfg, m, 200 + step, dev, first=7_000_000), ids_of(m, dev, first=next_id)
            next_id += m
            tk.append_items(rows, ids)
            mir.append(rows, ids)
        elif op == "remove":
            pos = torch.randperm(n, generator=g)[:33]
            tk.remove_items(pos)
            mir.remove(pos)
        elif op == "upsert":          # 12 items the corpus holds and 5 it does not
            held = torch.randperm(n, generator=g)[:12]
            new_ids = ids_of(5, dev, first=next_id)
            next_id += 5
            rows = table(cfg, 17, 300 + step, dev, first=8_000_000)
            order = torch.randperm(17, generator=g)
            all_ids = torch.cat([mir.ids[held.to(dev)], new_ids])
            tk.upsert_items(all_ids[order.to(dev)], rows[order.to(dev)])
            absent = order[order >= 12].to(dev)       # appended in the order given
            mir.update(held, rows[:12])
            mir.append(rows[absent], all_ids[absent])
        else:
            pos = torch.randperm(n, generator=g)[:21]
            tk.remove_items_by_id(mir.ids[pos.to(dev)])
            mir.remove(pos)
        check(tk, mol, mir, q, cent0, f"chain step {step} ({op})", module_calls=step in (3, 5, 9))


# ---- other geometries and precisions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["c4", "f16x3"])
def test_other_vector_width_and_split_f16_engine(dev, route):
    """c4: d = 64 (8 copies of 16 bytes per vector, 16 item groups); f16x3: update_source is a temporary index of the M rows alone."""
    cfg, mol, q, tk, mir, cent0 = start(route, dev, nlist=7)
    assert tk._bind().precision == ("f16x3" if route == "f16x3" else "fp32")
    g = torch.Generator().manual_seed(17)
    pos = torch.unique(torch.cat([torch.tensor([0, N0 - 1, 4095, 4096]), torch.randperm(N0, generator=g)[:120]]))
    rows = table(cfg, pos.numel(), 31, dev, first=9_000_000)
    rows[:30] = mir.X[torch.randperm(N0, generator=g)[:30].to(dev)]
    tk.update_items(pos.to(dev), rows)
    mir.update(pos, rows)
    check(tk, mol, mir, q, cent0, f"{route}: update", module_calls=False)
    rows, ids = table(cfg, 70, 32, dev, first=9_500_000), ids_of(70, dev, first=N0)
    tk.append_items(rows, ids)
    mir.append(rows, ids)
    check(tk, mol, mir, q, cent0, f"{route}: append", module_calls=False)
    pos = torch.randperm(N0 + 70, generator=g)[:150]
    tk.remove_items(pos)
    mir.remove(pos)
    check(tk, mol, mir, q, cent0, f"{route}: remove")


# ---- the fallback beyond one edit call, determinism ------------------------------------------------------------------------------------
def test_more_positions_than_one_edit_call_takes(dev):
    cfg, mol, q, tk, mir, cent0 = start("fp32", dev, n=20_000)
    m = E.IvfIndex.EDIT_MAX + 1
    pos = torch.randperm(20_000, generator=torch.Generator().manual_seed(3))[:m]
    rows = table(cfg, m, 41, dev, first=10_000_000)
    tk.update_items(pos.to(dev), rows)
    mir.update(pos, rows)
    check(tk, mol, mir, q, cent0, "update M = 16 385")


def test_append_beyond_one_edit_call_on_a_split_f16_engine(dev):
    """The rebuild reads the engine's index and the raw table AFTER the module grew them: 4 000 + 16 385 items, the fp16 table cut again."""
    cfg, mol, q, tk, mir, cent0 = start("f16x3", dev, n=4000)
    m = E.IvfIndex.EDIT_MAX + 1
    rows, ids = table(cfg, m, 43, dev, first=17_000_000), ids_of(m, dev, first=4000)
    tk.append_items(rows, ids)
    mir.append(rows, ids)
    check(tk, mol, mir, q, cent0, "append M = 16 385, split-f16", module_calls=False)
    pos = torch.randperm(4000 + m, generator=torch.Generator().manual_seed(4))[:m]      # and back: M holes and tail positions in one removal
    tk.remove_items(pos.to(dev))
    mir.remove(pos)
    check(tk, mol, mir, q, cent0, "remove M = 16 385, split-f16")


def test_two_identical_sequences_give_equal_buffers(dev):
    out = []
    for _ in range(2):
        cfg, mol, q, tk, mir, cent0 = start("fp32", dev)
        g = torch.Generator().manual_seed(23)
        pos = torch.randperm(N0, generator=g)[:200]
        tk.update_items(pos, table(cfg, 200, 51, dev, first=11_000_000))
        tk.append_items(table(cfg, 45, 52, dev, first=12_000_000), ids_of(45, dev, first=N0))
        tk.remove_items(torch.randperm(N0 + 45, generator=g)[:99])
        out.append(tk)
    lists_equal(out[0]._ivf, out[1]._ivf, "two runs")
    same(out[0]._item_embeddings, out[1]._item_embeddings, "table")


# ---- the surrounding contract ---------------------------------------------------------------------------------------------------------
def test_edit_is_issued_behind_enqueued_work(dev):
    cfg, mol, q, tk, mir, cent0 = start("fp32", dev)
    big = torch.randn(2048, 2048, device=dev)
    acc = big
    pos = torch.randperm(N0, generator=torch.Generator().manual_seed(29))[:150]
    rows = table(cfg, 150, 61, dev, first=13_000_000)
    torch.cuda.synchronize()
    for _ in range(8):                 # work in flight on the current stream when the calls are made
        acc = (acc @ big) * 1e-2
    before = tk(q, k=10)
    tk.update_items(pos.to(dev), rows)
    tk.remove_items(pos[:40].to(dev))
    mir.update(pos, rows)
    mir.remove(pos[:40])
    assert before[0].shape[0] == B and torch.isfinite(acc).any()
    check(tk, mol, mir, q, cent0, "behind enqueued work")


def test_an_unbuilt_index_stays_unbuilt(dev):
    cfg, mol, q = setup("fp32", dev)
    X, ids = table(cfg, N0, 21, dev), ids_of(N0, dev)
    tk = make(mol, X, ids, frozen_centroids=True)
    mir = Mirror(X, ids)
    pos = torch.randperm(N0, generator=torch.Generator().manual_seed(31))[:64]
    rows = table(cfg, 64, 71, dev, first=14_000_000)
    tk.update_items(pos, rows)
    mir.update(pos, rows)
    tk.append_items(rows[:9], ids_of(9, dev, first=N0))
    mir.append(rows[:9], ids_of(9, dev, first=N0))
    tk.remove_items(pos[:10])
    mir.remove(pos[:10])
    assert tk._ivf is None
    fresh = make(mol, mir.X, mir.ids, frozen_centroids=True)       # both train at first use, on the same table with the same seed
    same(tk(q, k=10), fresh(q, k=10), "forward")
    lists_equal(tk._ivf, fresh._ivf, "built at first use")


def test_arguments_are_validated_and_the_default_still_refuses(dev):
    cfg, mol, q = setup("fp32", dev)
    X, ids = table(cfg, 600, 21, dev), ids_of(600, dev)
    G, d = cfg.item_dot_product_groups, cfg.dot_product_dimension
    good = torch.nn.functional.normalize(torch.randn(G, NLIST, d, device=dev), dim=2)
    for bad in (good[:, :4], good[:, :, :16], good[:1], good.double(), good.cpu(), good.reshape(G * NLIST, d)):
        with pytest.raises(ValueError, match="ivf_centroids"):
            make(mol, X, ids, ivf_centroids=bad)
    eng = mol.engine()
    for bad in (good[:, :4], good.double(), good.cpu()):
        with pytest.raises(ValueError, match="centroids"):
            E.IvfIndex(eng, eng.build_index(X), nlist=NLIST, centroids=bad)
    with pytest.raises(ValueError, match="frozen_centroids"):
        rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), k_per_group=KG, frozen_centroids=True)
    # given centroids are used as they are, copied: nothing is trained, the caller's tensor is never aliased or written
    keep = good.clone()
    tk = make(mol, X, ids, ivf_centroids=good, frozen_centroids=True)
    ivf = tk.ivf_index()
    assert torch.equal(ivf.centroids, keep) and ivf.centroids.data_ptr() != good.data_ptr()
    good.zero_()
    tk.update_items(torch.tensor([0, 599]), table(cfg, 2, 81, dev, first=15_000_000))
    assert torch.equal(tk._ivf.centroids, keep)
    # the default module refuses exactly as before
    plain = make(mol, X, ids)
    rows = table(cfg, 2, 82, dev, first=16_000_000)
    for call in (lambda: plain.update_items(torch.tensor([0, 1]), rows), lambda: plain.append_items(rows, ids_of(2, dev, first=600)),
                 lambda: plain.remove_items(torch.tensor([0, 1])), lambda: plain.upsert_items(ids[:2], rows),
                 lambda: plain.remove_items_by_id(ids[:2])):
        with pytest.raises(NotImplementedError, match="IVF"):
            call()
