"""CPU: removal_plan, the one rule of remove_items -- holes below N' filled from the surviving tail, both ascending -- and
the entry points the removal and the MIPS corpus API add under the unchanged ABI version."""
import os
import re

import pytest
import torch

from rails_amd import _lib
from rails_amd.topk_modules import removal_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rails_mol_index_clear_tail", "rails_mol_generic_index_clear_tail", "rails_mips_index_update", "rails_mips_index_gather_rows",
       "rails_mips_index_clear_tail")


def plan(positions, n):
    holes, movers = removal_plan(torch.tensor(positions, dtype=torch.int64), n)
    assert holes.dtype == movers.dtype == torch.int64 and holes.shape == movers.shape and not holes.is_cuda
    return holes.tolist(), movers.tolist()


def apply_plan(n, positions):
    """The resulting table of arange(n) under the plan: rows 0 .. N' - 1 after the moves."""
    holes, movers = removal_plan(positions, n)
    rows = torch.arange(n)
    rows[holes] = rows[movers]
    return rows[: n - positions.numel()], holes, movers


def test_only_tail_positions_need_no_move():
    assert plan([9, 8, 7], 10) == ([], [])
    assert plan([99], 100) == ([], [])
    assert plan([], 10) == ([], [])


def test_only_head_positions():
    assert plan([0, 1, 2], 10) == ([0, 1, 2], [7, 8, 9])
    assert plan([0], 10) == ([0], [9])


def test_removed_tail_positions_are_no_movers():
    # N = 10, M = 4, N' = 6: 8 and 6 are removed themselves, so the movers are 7 and 9
    assert plan([1, 8, 4, 6], 10) == ([1, 4], [7, 9])
    # 0, 31, 32, N - 1, N - 2 of N = 70: N' = 65; the tail 65 .. 69 keeps 65, 66, 67
    assert plan([0, 31, 32, 69, 68], 70) == ([0, 31, 32], [65, 66, 67])


def test_all_but_one():
    assert plan(list(range(1, 10)), 10) == ([], [])              # position 0 survives where it is
    assert plan(list(range(0, 9)), 10) == ([0], [9])             # the last item survives and moves to 0
    assert plan([0, 1, 2, 3, 5, 6, 7, 8, 9], 10) == ([0], [4])


def test_shuffled_input_gives_the_same_plan():
    g = torch.Generator().manual_seed(3)
    p = torch.randperm(1000, generator=g)[:137]
    want = removal_plan(torch.sort(p).values, 1000)
    for _ in range(3):
        got = removal_plan(p[torch.randperm(p.numel(), generator=g)], 1000)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_random_plans_keep_the_survivors_and_their_positions():
    g = torch.Generator().manual_seed(4)
    for _ in range(200):
        n = int(torch.randint(1, 201, (1,), generator=g))
        m = int(torch.randint(0, n, (1,), generator=g))
        p = torch.randperm(n, generator=g)[:m]
        rows, holes, movers = apply_plan(n, p)
        n_new = n - m
        survivors = sorted(set(range(n)) - set(p.tolist()))
        assert rows.numel() == n_new and sorted(rows.tolist()) == survivors             # every survivor once, nothing else
        stay = [v for v in survivors if v < n_new]
        assert all(int(rows[v]) == v for v in stay)                                   # a survivor below N' keeps its position
        assert holes.tolist() == sorted(holes.tolist()) and movers.tolist() == sorted(movers.tolist())
        assert all(v < n_new for v in holes.tolist()) and all(v >= n_new for v in movers.tolist())
        assert set(holes.tolist()) == {v for v in p.tolist() if v < n_new}
        assert holes.numel() <= m                                                     # O(M) rows move


def test_refused_plans():
    for bad in ([1, 2, 1], [1, 10], [-1, 2], list(range(10))):                        # a duplicate, out of range twice, M = N
        with pytest.raises(ValueError):
            removal_plan(torch.tensor(bad, dtype=torch.int64), 10)
    with pytest.raises(ValueError):
        removal_plan(torch.tensor([1, 2], dtype=torch.int32), 10)
    with pytest.raises(ValueError):
        removal_plan(torch.tensor([[1, 2]], dtype=torch.int64), 10)
    with pytest.raises(ValueError):
        removal_plan([1, 2], 10)


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    declared = set(re.findall(r"\b(rails_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES, name
        assert _lib.PROTOTYPES[name][1][-1] is _lib.C.c_void_p, f"{name}: the last argument is the stream"
    assert re.search(r"#define RAILS_ABI_VERSION 15\b", header) and _lib.RAILS_ABI_VERSION == 15
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.rails_abi_version() == 15
    # argument validation before any launch (no device needed)
    from rails_amd import engine as E
    C = _lib.C
    s = E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, 128).to_c()
    assert lib.rails_mol_index_clear_tail(C.byref(s), None, 64, None) == _lib.RAILS_OK                     # a full last tile: nothing to do
    assert lib.rails_mol_index_clear_tail(C.byref(s), None, 65, None) == _lib.RAILS_EINVAL and "NULL" in _lib.last_error()
    assert lib.rails_mol_index_clear_tail(C.byref(s), None, -1, None) == _lib.RAILS_EINVAL
    assert lib.rails_mol_generic_index_clear_tail(C.byref(s), None, 65, None) == _lib.RAILS_EINVAL
    assert lib.rails_mips_index_update(None, 0, 64, None, None, 10, None) == _lib.RAILS_OK
    assert lib.rails_mips_index_update(None, 3, 64, None, None, 10, None) == _lib.RAILS_EINVAL and "NULL" in _lib.last_error()
    assert lib.rails_mips_index_update(None, 3, 0, None, None, 10, None) == _lib.RAILS_EINVAL
    assert lib.rails_mips_index_gather_rows(None, 10, 64, None, 0, None, None) == _lib.RAILS_OK
    assert lib.rails_mips_index_gather_rows(None, 10, 64, None, 3, None, None) == _lib.RAILS_EINVAL
    assert lib.rails_mips_index_clear_tail(None, 64, 64, None) == _lib.RAILS_OK
    assert lib.rails_mips_index_clear_tail(None, 65, 64, None) == _lib.RAILS_EINVAL
