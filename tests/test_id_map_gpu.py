"""GPU: the device-resident item id -> position map (rails_id_map_*, engine.ItemIdMap) against a Python dict, and the by-id corpus API of the
top-k modules (positions_of / update_items_by_id / upsert_items / remove_items_by_id).  The oracle of the module tests is,
as in tests/test_index_update_gpu.py (whose helpers are used through the module, U), a module FRESHLY CONSTRUCTED from the resulting table and ids
-- every held buffer and every result torch.equal -- plus a twin module driven by the equivalent by-position calls, which must hold the same bytes.

mix / unmix below restate the formula of include/rails_amd.h in Python integers; tests/test_id_map_cpu.py pins that they invert each other."""
import pytest
import torch

import rails_amd
from oracle import mol_oracle as O
from rails_amd import engine as E
from tests import test_index_remove_gpu as R
from tests import test_index_update_gpu as U

pytestmark = pytest.mark.gpu
B = U.B
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
C1, C2, GAMMA = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0x9E3779B97F4A7C15


def mix(x):
    z = (x + GAMMA) & M64
    z = ((z ^ (z >> 30)) * C1) & M64
    z = ((z ^ (z >> 27)) * C2) & M64
    return z ^ (z >> 31)


def unmix(h):
    z = h ^ (h >> 31) ^ (h >> 62)
    z = (z * pow(C2, -1, 1 << 64)) & M64
    z = z ^ (z >> 27) ^ (z >> 54)
    z = (z * pow(C1, -1, 1 << 64)) & M64
    z = z ^ (z >> 30) ^ (z >> 60)
    return (z - GAMMA) & M64


def signed(x):
    return x - (1 << 64) if x >> 63 else x


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def sparse_ids(n, g, avoid=()):
    """n distinct int64 ids spread over the whole range, none reserved, none in `avoid`; the first ones are INT64_MIN + 2, 0, INT64_MAX, -1."""
    special = [I64_MIN + 2, 0, I64_MAX, -1]
    taken, out = set(avoid) | set(E.ID_MAP_RESERVED), []
    hi, lo = torch.randint(-(1 << 31), 1 << 31, (2 * n + 16,), generator=g).tolist(), torch.randint(0, 1 << 32, (2 * n + 16,), generator=g).tolist()
    for v in special + [(h << 32) | l for h, l in zip(hi, lo)]:
        if v not in taken:
            taken.add(v)
            out.append(v)
        if len(out) == n:
            break
    assert len(out) == n
    return out


def new_table(slots, dev):
    return E.id_map_new(slots, dev), torch.zeros(4, dtype=torch.int32, device=dev)


def lookups(table, slots, ids, dev):
    return E.id_map_lookup(table, slots, torch.tensor(ids, dtype=torch.int64, device=dev)).tolist()


@pytest.mark.parametrize("n", [1, 33, 1_000, 70_001])
def test_lookups_against_a_dict(n, dev):
    g = torch.Generator().manual_seed(100 + n)
    ids = sparse_ids(n, g)
    order = torch.randperm(n, generator=g).tolist()
    ids = [ids[j] for j in order]                       # shuffled: position p holds ids[p]
    want = {v: p for p, v in enumerate(ids)}
    absent = sparse_ids(n, g, avoid=ids)
    slots = E.id_map_slots(n)
    assert slots >= 4 * n and slots & (slots - 1) == 0
    table, flags = new_table(slots, dev)
    E.id_map_insert(table, slots, torch.tensor(ids, dtype=torch.int64, device=dev), None, 0, flags)
    assert flags.tolist() == [0, 0, 0, 0]
    ask = ids + absent + list(E.ID_MAP_RESERVED)        # (a reserved value is never found, and must not match an empty slot)
    ask = [ask[j] for j in torch.randperm(len(ask), generator=g).tolist()]
    assert lookups(table, slots, ask, dev) == [want.get(v, -1) for v in ask]
    if n == 70_001:
        assert min(ids) < 0 < max(ids) and {I64_MIN + 2, 0, I64_MAX} <= set(ids)
    # explicit positions instead of first + u
    table2, flags2 = new_table(slots, dev)
    pos = torch.randperm(n, generator=g)
    E.id_map_insert(table2, slots, torch.tensor(ids, dtype=torch.int64), pos.to(dev), 0, flags2)
    assert flags2.tolist() == [0, 0, 0, 0] and lookups(table2, slots, ids[:50], dev) == pos[:50].tolist()


def chain_ids(slots, count, home):
    ids = [signed(unmix((j << 40) | home)) for j in range(1, count + 1)]
    assert all(mix(v & M64) & (slots - 1) == home for v in ids) and len(set(ids)) == count and not set(ids) & set(E.ID_MAP_RESERVED)
    return ids


def test_one_long_probe_chain_that_wraps_and_erasing_inside_it(dev):
    slots = 4096
    g = torch.Generator().manual_seed(7)
    chain = chain_ids(slots, 300, slots - 5)            # 300 ids whose home slot is slots - 5: the chain runs over the end of the table
    others = sparse_ids(200, g, avoid=chain)
    ids = others + chain
    ids = [ids[j] for j in torch.randperm(500, generator=g).tolist()]
    want = {v: p for p, v in enumerate(ids)}
    table, flags = new_table(slots, dev)
    E.id_map_insert(table, slots, torch.tensor(ids, dtype=torch.int64, device=dev), None, 0, flags)
    assert flags.tolist() == [0, 0, 0, 0]
    assert lookups(table, slots, chain, dev) == [want[v] for v in chain]
    assert lookups(table, slots, others, dev) == [want[v] for v in others]
    # erase every third id of the chain: those are gone, the others are found behind the tombstones
    erased = chain[::3]
    E.id_map_erase(table, slots, torch.tensor(erased, dtype=torch.int64, device=dev), flags[3:])
    assert flags.tolist() == [0, 0, 0, 0]
    for v in erased:
        del want[v]
    assert lookups(table, slots, ids, dev) == [want.get(v, -1) for v in ids]
    # an erased id comes back at a new position
    again = erased[::2]
    new_pos = torch.arange(1000, 1000 + len(again), dtype=torch.int64, device=dev)
    E.id_map_insert(table, slots, torch.tensor(again, dtype=torch.int64, device=dev), new_pos, 0, flags)
    assert flags.tolist() == [0, 0, 0, 0]
    want.update({v: 1000 + j for j, v in enumerate(again)})
    assert lookups(table, slots, ids, dev) == [want.get(v, -1) for v in ids]


def test_flags_count_exactly(dev):
    g = torch.Generator().manual_seed(8)
    ids = sparse_ids(100, g)
    slots = E.id_map_slots(100)
    table, flags = new_table(slots, dev)
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)      # noqa: E731
    E.id_map_insert(table, slots, t(ids), None, 0, flags)
    assert flags.tolist() == [0, 0, 0, 0]
    E.id_map_insert(table, slots, t(ids[10:17]), None, 500, flags)              # 7 ids already present
    assert flags.tolist() == [7, 0, 0, 0]
    a, b, c = sparse_ids(3, g, avoid=ids)
    E.id_map_insert(table, slots, t([a, a, b, b, b, c]), None, 600, flags)      # one id twice, one three times: 1 + 2 repeats
    assert flags.tolist() == [10, 0, 0, 0]
    got = lookups(table, slots, [a, b, c], dev)
    assert got[0] in (600, 601) and got[1] in (602, 603, 604) and got[2] == 605
    E.id_map_insert(table, slots, t([I64_MIN, I64_MIN + 1, I64_MIN]), None, 700, flags)     # reserved
    assert flags.tolist() == [10, 3, 0, 0]
    E.id_map_erase(table, slots, t(sparse_ids(4, g, avoid=ids + [a, b, c]) + [ids[0], I64_MIN]), flags[3:])      # 4 absent, 1 present, 1 reserved
    assert flags.tolist() == [10, 3, 0, 5]
    E.id_map_erase(table, slots, t([ids[1], ids[1]]), flags[3:])                # twice in one call: the second finds it gone
    assert flags.tolist() == [10, 3, 0, 6]
    assert lookups(table, slots, ids[:3], dev) == [-1, -1, 2]
    assert lookups(table, slots, ids[10:17], dev) == list(range(10, 17)), "a refused insert leaves the entry it met"


def test_item_id_map_rebuilds_before_load_one_half(dev):
    n = 40
    g = torch.Generator().manual_seed(9)
    ids = torch.tensor(sparse_ids(n, g), dtype=torch.int64, device=dev)
    fresh = sparse_ids(200, g, avoid=ids.tolist())
    m = E.ItemIdMap(dev)
    m.build(ids)
    assert m.info() == {"slots": 256, "live": n, "tombstones": 0, "rebuilds": 0}
    arange = torch.arange(n, device=dev)
    for step in range(200):
        p = int(torch.randint(0, n, (1,), generator=g))
        old, new = ids[p : p + 1].clone(), torch.tensor([fresh[step]], dtype=torch.int64, device=dev)
        ids[p] = new[0]
        m.erase(old)
        m.insert(new, torch.tensor([p], dtype=torch.int64, device=dev), ids)
        info = m.info()
        assert info["live"] == n and info["live"] + info["tombstones"] <= info["slots"] // 2 and info["slots"] == 256, (step, info)
        assert torch.equal(m.lookup(ids), arange) and m.lookup(old).tolist() == [-1], step
        assert m.take_flags() == (0, 0, 0, 0), step
    assert m.info()["rebuilds"] >= 1
    with pytest.raises(ValueError, match="1 of its 40 item ids repeat"):
        m.build(torch.cat([ids[:-1], ids[:1]]))


# ---- the modules -------------------------------------------------------------------------------------------------------------------------

def mol_case(module, dev):
    """-> (make(x, i), rows(m, seed), snapshot(tk), check(tk, X, ids, what), n)"""
    cfg, mol, _, aux = U.setup_route("brute", "default", dev)
    q = O.synthetic_queries(cfg, B, seed=5).to(dev)
    make = {
        "brute": lambda x, i: rails_amd.MoLBruteForceTopK(mol, x, i),
        "dense": lambda x, i: rails_amd.MoLBruteForceTopK(mol, x, i, exact_mode="dense"),
        "avg": lambda x, i: rails_amd.MoLAvgTopK(mol, x, i, avg_top_k=200),
        "naive": lambda x, i: rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=2),
        "comb": lambda x, i: rails_amd.MoLCombTopK(mol, x, i, avg_top_k=200, k_per_group=5),
    }[module]
    rows = lambda m, seed: U.table(cfg, m, seed, dev, first=1_000_000 * seed)      # noqa: E731
    check = lambda tk, X, ids, what: U.equals_fresh(tk, make, X, ids, q, aux, what, ks=(10, 100))      # noqa: E731
    return make, rows, U.held, check, (2_080 if module == "comb" else 300)


def mips_case(dev):
    D = 64
    q = torch.from_numpy(O.hash_item_table(99, 0, B, D)).to(dev)
    make = lambda x, i: rails_amd.MIPSBruteForceTopK(x, i)      # noqa: E731
    rows = lambda m, seed: torch.from_numpy(O.hash_item_table(seed, 1_000_000 * seed, m, D)).to(dev)      # noqa: E731
    snapshot = lambda tk: {"index": tk._index.buf, "ids": tk._ids_flat, "item_ids": tk._item_ids.reshape(-1)}      # noqa: E731
    check = lambda tk, X, ids, what: R.mips_equals_fresh(tk, X, ids, q, what)      # noqa: E731
    return make, rows, snapshot, check, 300


def in_step(tk, twin, snapshot, check, X, ids, what, dev):
    n = X.shape[0]
    assert torch.equal(tk.positions_of(tk._ids_flat), torch.arange(n, device=dev)), f"{what}: positions_of(ids) is not arange"
    assert torch.equal(tk.positions_of(ids.cpu().unsqueeze(0)), torch.arange(n, device=dev)), what
    absent = torch.tensor([-123_456_789, 2, I64_MAX - 1, I64_MIN], device=dev)
    assert tk.positions_of(absent).tolist() == [-1] * 4, what
    check(tk, X, ids, what)
    a, b = snapshot(tk), snapshot(twin)
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for name in a:
        U.same(a[name], b[name], f"{what}: twin buffer {name}")
    assert tk._id_map is not None and twin._id_map is None


@pytest.mark.parametrize("module", ["brute", "dense", "avg", "naive", "comb", "mips"])
def test_by_id_chain_equals_fresh_and_by_position_twin(module, dev):
    make, rows, snapshot, check, n = mips_case(dev) if module == "mips" else mol_case(module, dev)
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)      # noqa: E731
    with torch.inference_mode():
        X, ids = rows(n, 3), U.ids_of(n, dev)
        tk, twin = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        check(tk, X, ids, "as built")          # every lazily built buffer exists now
        check(twin, X, ids, "twin as built")
        # 1. update by id: 0, both sides of a tile boundary, the last item
        p = t([0, 31, 32, n - 1, 7, 100])
        r = rows(6, 11)
        tk.update_items_by_id(ids[p], r)                                    # device ids
        twin.update_items(p, r)
        X[p] = r
        in_step(tk, twin, snapshot, check, X, ids, "update by id", dev)
        # 2. update by id with new ids: two items swap theirs, a third gets a new one
        p = t([5, n - 2, 40])
        r = rows(3, 12)
        new = torch.stack([ids[n - 2], ids[5], t(-77)])
        tk.update_items_by_id(ids[p].cpu(), r.unsqueeze(0), new.unsqueeze(0))      # CPU ids, (1, M, D) rows, (1, M) new ids
        twin.update_items(p, r, new)
        X[p], ids[p] = r, new
        in_step(tk, twin, snapshot, check, X, ids, "update by id with a swap", dev)
        # 3. upsert: half present, half new, interleaved
        p = t([3, 64, n - 1])
        fresh_ids = t([9_000_000_001, -9_000_000_002, 9_000_000_003])
        given = torch.stack([fresh_ids[0], ids[3], fresh_ids[1], ids[64], ids[n - 1], fresh_ids[2]])
        r = rows(6, 13)
        tk.upsert_items(given, r)
        twin.update_items(p, r[t([1, 3, 4])])
        twin.append_items(r[t([0, 2, 5])], fresh_ids)
        X[p] = r[t([1, 3, 4])]
        X, ids = torch.cat([X, r[t([0, 2, 5])]]), torch.cat([ids, fresh_ids])
        n += 3
        in_step(tk, twin, snapshot, check, X, ids, "upsert", dev)
        # 4. remove by id: the tail, a tile boundary, below N'
        p = t([n - 1, n - 3, 31, 32, 10])
        gone = ids[p]
        want_X, want_ids, want_moved = R.after_removal(X, ids, p)
        moved = tk.remove_items_by_id(gone)
        assert torch.equal(moved, want_moved) and torch.equal(twin.remove_items(p), want_moved)
        X, ids, n = want_X, want_ids, n - 5
        in_step(tk, twin, snapshot, check, X, ids, "remove by id", dev)
        assert tk.positions_of(gone).tolist() == [-1] * 5
        # 5. - 7. the by-position calls with the map live: it follows
        p = t([1, n - 1, 33])
        r, new = rows(3, 14), torch.stack([ids[33], t(123_456_789_012), ids[1]])      # ids swap between positions 1 and 33
        tk.update_items(p, r, new)
        twin.update_items(p, r, new)
        X[p], ids[p] = r, new
        in_step(tk, twin, snapshot, check, X, ids, "update_items with a live map", dev)
        r, new = rows(40, 15), U.ids_of(40, dev, first=70_000_000)
        tk.append_items(r, new)
        twin.append_items(r, new)
        X, ids, n = torch.cat([X, r]), torch.cat([ids, new]), n + 40
        in_step(tk, twin, snapshot, check, X, ids, "append_items with a live map", dev)
        p = t([n - 2, 0, 63, 64, n - 40])
        want_X, want_ids, want_moved = R.after_removal(X, ids, p)
        assert torch.equal(tk.remove_items(p), want_moved) and torch.equal(twin.remove_items(p), want_moved)
        X, ids, n = want_X, want_ids, n - 5
        in_step(tk, twin, snapshot, check, X, ids, "remove_items with a live map", dev)
        # 8. by id again, on items the by-position calls renamed, appended and moved
        given = torch.stack([t(123_456_789_012), ids[n - 1], ids[0], t(555)])
        r = rows(4, 16)
        found = tk.positions_of(given)
        assert found[3].item() == -1 and (found[:3] >= 0).all()
        tk.upsert_items(given, r)
        twin.update_items(found[:3], r[:3])
        twin.append_items(r[3:], t([555]))
        X[found[:3]] = r[:3]
        X, ids = torch.cat([X, r[3:]]), torch.cat([ids, t([555])])
        in_step(tk, twin, snapshot, check, X, ids, "upsert after the by-position calls", dev)
        assert tk._id_map.info()["live"] == X.shape[0]


@pytest.mark.parametrize("module", ["brute", "mips"])
def test_by_id_errors_leave_the_module_as_it_was(module, dev):
    make, rows, snapshot, check, n = mips_case(dev) if module == "mips" else mol_case(module, dev)
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)      # noqa: E731
    with torch.inference_mode():
        X, ids = rows(n, 4), U.ids_of(n, dev)
        tk = make(X.clone().unsqueeze(0), ids.clone().unsqueeze(0))
        check(tk, X, ids, "as built")
        snap = {k: v.clone() for k, v in snapshot(tk).items()}
        r = rows(3, 21)
        unknown, twice = torch.stack([ids[1], t(2), t(5)]), torch.stack([ids[1], ids[2], ids[1]])
        with pytest.raises(ValueError, match="2 of the 3 item ids are not in the corpus"):
            tk.update_items_by_id(unknown, r)
        with pytest.raises(ValueError, match="2 of the 3 item ids are not in the corpus"):
            tk.remove_items_by_id(unknown)
        for call in (lambda: tk.update_items_by_id(twice, r), lambda: tk.remove_items_by_id(twice), lambda: tk.upsert_items(twice, r)):
            with pytest.raises(ValueError, match="1 of the 3 item ids repeat"):
                call()
        with pytest.raises(ValueError):
            tk.upsert_items(ids[:2], r)                                     # two ids, three rows
        with pytest.raises(ValueError):
            tk.upsert_items(torch.stack([ids[1], t(2), t(5)]), r[:, :-1].contiguous())     # wrong D: refused before the present id is updated
        with pytest.raises(ValueError):
            tk.positions_of(ids.float())
        now = snapshot(tk)
        for k in snap:
            U.same(now[k], snap[k], f"nothing is modified by a refused call: {k}")
        check(tk, X, ids, "after the refused calls")
        # a by-position update that plants a duplicate id drops the live map; the next by-id call says what a fresh module would
        assert tk._id_map is not None
        tk.update_items(t([7]), r[:1], ids[8:9].clone())
        ids[7] = ids[8]
        X[7] = r[0]
        assert tk._id_map is None
        with pytest.raises(ValueError, match=f"1 of its {n} item ids repeat"):
            tk.positions_of(ids[:3])
        check(tk, X, ids, "with a duplicate id the module still answers")
        # a corpus with two equal ids from the start: refused at the first by-id call, and the by-position calls keep working
        ids2 = U.ids_of(n, dev)
        ids2[n - 1] = ids2[4]
        X2 = rows(n, 5)
        tk2 = make(X2.clone().unsqueeze(0), ids2.clone().unsqueeze(0))
        snap2 = {k: v.clone() for k, v in snapshot(tk2).items()}
        with pytest.raises(ValueError, match=f"1 of its {n} item ids repeat"):
            tk2.update_items_by_id(ids2[:3], r)
        now = snapshot(tk2)
        for k in snap2:
            U.same(now[k], snap2[k], f"a refused map build modifies nothing: {k}")
        tk2.update_items(t([4, n - 1, 9]), r)
        X2[t([4, n - 1, 9])] = r
        check(tk2, X2, ids2, "update_items by position on a corpus with equal ids")
        reserved = U.ids_of(n, dev)
        reserved[2] = I64_MIN + 1
        tk3 = make(X2.clone().unsqueeze(0), reserved.unsqueeze(0))
        with pytest.raises(ValueError, match="1 are reserved"):
            tk3.positions_of(reserved[:1])


def test_the_ivf_module_answers_positions_of_and_refuses_the_rest(dev):
    cfg, mol, _, aux = U.setup_route("naive", "default", dev)
    n = 300
    with torch.inference_mode():
        X, ids = U.table(cfg, n, 6, dev), U.ids_of(n, dev)
        ivf = rails_amd.MoLNaiveTopK(mol, X.unsqueeze(0), ids.unsqueeze(0), k_per_group=2, use_faiss=True, nlist=4)
        assert torch.equal(ivf.positions_of(ids.flip(0)), torch.arange(n, device=dev).flip(0))
        assert ivf.positions_of(torch.tensor([2, -5])).tolist() == [-1, -1]
        r = U.table(cfg, 2, 7, dev)
        for call in (lambda: ivf.update_items_by_id(ids[:2], r), lambda: ivf.remove_items_by_id(ids[:2]), lambda: ivf.upsert_items(ids[:2], r)):
            with pytest.raises(NotImplementedError, match="IVF"):
                call()
        assert ivf.num_items == n and torch.equal(ivf._ids_flat, U.ids_of(n, dev)) and torch.equal(ivf._item_embeddings[0], U.table(cfg, n, 6, dev))
