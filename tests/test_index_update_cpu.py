"""CPU: the in-place update entry points are declared, bound and exported under the unchanged ABI version, and the global -> local routing of
a sharded update is what rails_amd/sharded.py says it is."""
import os
import re

import pytest
import torch

from rails_amd import _lib
from rails_amd.sharded import route_update_positions, shard_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rails_mol_index_update", "rails_mol_generic_index_update", "rails_mol_index_rows_update", "rails_mol_coarse_update", "rails_mol_component_update")


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    declared = set(re.findall(r"\b(rails_[a-z0-9_]+)\s*\(", header))
    binding = open(os.path.join(ROOT, "rails_amd", "_lib.py")).read()
    for name in NEW:
        assert name in declared, name
        assert f'"{name}"' in binding and name in _lib.PROTOTYPES, name
        assert _lib.PROTOTYPES[name][1][-1] is _lib.C.c_void_p, f"{name}: the last argument is the stream"
    assert re.search(r"#define RAILS_ABI_VERSION 15\b", header) and _lib.RAILS_ABI_VERSION == 15
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.rails_abi_version() == 15
    for name in NEW:
        assert getattr(lib, name) is not None
    # argument validation before any launch (no device needed)
    from rails_amd import engine as E
    s = E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, 128).to_c()
    C = _lib.C
    assert lib.rails_mol_index_update(C.byref(s), None, None, 0, None, None, 10, None) == _lib.RAILS_OK             # nothing to do
    assert lib.rails_mol_index_update(C.byref(s), None, None, 3, None, None, 10, None) == _lib.RAILS_EINVAL and "NULL" in _lib.last_error()
    assert lib.rails_mol_index_update(C.byref(s), None, None, -1, None, None, 10, None) == _lib.RAILS_EINVAL
    assert lib.rails_mol_index_rows_update(C.byref(s), None, 10, None, 3, None, None) == _lib.RAILS_EINVAL
    assert lib.rails_mol_coarse_update(C.byref(s), None, 1, None, 3, None, 10, None) == _lib.RAILS_EINVAL
    assert lib.rails_mol_component_update(C.byref(s), None, 0, None, 3, None, 10, None) == _lib.RAILS_EINVAL
    s16 = E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, 128).to_c("f16x3")
    assert lib.rails_mol_index_rows_update(C.byref(s16), None, 10, None, 3, None, None) == _lib.RAILS_ENOTSUP
    assert lib.rails_mol_coarse_update(C.byref(s16), None, 1, None, 0, None, 10, None) == _lib.RAILS_ENOTSUP and "fp32-format" in _lib.last_error()


ROUTING = [
    # (n_total, world, global positions, per rank: (local positions, rows of the update))
    (10, 2, [0, 4, 5, 9], {0: ([0, 4], [0, 1]), 1: ([0, 4], [2, 3])}),
    (10, 2, [9, 5, 4, 0], {0: ([4, 0], [2, 3]), 1: ([4, 0], [0, 1])}),                        # the order given is kept
    (10, 3, [9, 8, 3, 4, 7], {0: ([3], [2]), 1: ([0, 3], [3, 4]), 2: ([1, 0], [0, 1])}),      # ragged: 4 + 4 + 2 items
    (5, 4, [4, 0, 3], {0: ([0], [1]), 1: ([1], [2]), 2: ([0], [0]), 3: ([], [])}),            # an empty last shard (2 + 2 + 1 + 0)
    (10, 2, [], {0: ([], []), 1: ([], [])}),
    (10, 2, [6, 7], {0: ([], []), 1: ([1, 2], [0, 1])}),                                      # nothing for rank 0
]


@pytest.mark.parametrize("n_total,world,positions,want", ROUTING)
def test_routing_table(n_total, world, positions, want):
    p = torch.tensor(positions, dtype=torch.int64)
    emb = torch.arange(len(positions), dtype=torch.float32)[:, None] * 10.0          # row j of the update is recognisable
    seen = []
    for rank in range(world):
        lo, hi = shard_bounds(n_total, world, rank)
        local, rows = route_update_positions(p, lo, hi)
        assert local.dtype == torch.int64 and rows.dtype == torch.int64
        assert local.tolist() == want[rank][0] and rows.tolist() == want[rank][1], rank
        assert emb[rows, 0].tolist() == [10.0 * r for r in want[rank][1]]            # the embedding rows follow in the same order
        assert all(0 <= v < hi - lo for v in local.tolist())
        seen += rows.tolist()
    assert sorted(seen) == list(range(len(positions)))                               # every update lands on exactly one rank


def test_positions_outside_every_shard_are_ignored():
    local, rows = route_update_positions(torch.tensor([-3, 2, 10, 11, 7]), 0, 5)
    assert local.tolist() == [2] and rows.tolist() == [1]
    local, rows = route_update_positions(torch.tensor([-3, 2, 10, 11, 7]), 5, 10)
    assert local.tolist() == [2] and rows.tolist() == [4]
    local, rows = route_update_positions(torch.tensor([1, 2]), 4, 4)                 # an empty shard
    assert local.numel() == 0 and rows.numel() == 0


HELD_READS = {      # what tests/test_index_update_gpu.py::held reads of each module class, beside the table and the ids
    "MoLBruteForceTopK": {"_index", "_rows_cache", "_index32", "_rows32"},
    "MoLAvgTopK": {"_index", "_rows_cache", "_coarse_table", "_coarse_prefilter"},
    "MoLNaiveTopK": {"_index", "_rows_cache", "_comp_table"},
    "MoLCombTopK": {"_index", "_rows_cache", "_coarse_table", "_coarse_prefilter", "_comp_table"},
    "MIPSBruteForceTopK": {"_index"},
}
CORPUS = {"_item_embeddings", "_item_ids", "_ids_flat"}      # written by the edit flow itself


def test_the_held_buffer_lists_name_what_the_gpu_tests_compare():
    """The edit flow resizes, refreshes and drops what a class lists in _HELD and nothing else: every attribute the GPU tests' held() compares
    with a fresh module's is named by the list of every class that has it, so a buffer added later cannot be forgotten by the flow."""
    from unittest import mock

    import rails_amd
    from tests.test_index_update_gpu import held

    class Probe:
        def __init__(self):
            self.read = set()

        def __getattr__(self, name):
            self.read.add(name)
            return mock.MagicMock()

    probe = Probe()
    held(probe)
    assert probe.read == CORPUS.union(*HELD_READS.values()), "held() reads an attribute this test does not assign to a class"
    for name, reads in HELD_READS.items():
        cls = getattr(rails_amd, name)
        listed = {a for h in cls._held_buffers() for a in h.attrs}
        assert reads <= listed, (name, sorted(reads - listed))
    assert [h.attrs[0] for h in rails_amd.MoLCombTopK._held_buffers() if h.refresh is not None] == ["_index", "_rows_cache", "_coarse_table", "_comp_table"]
    assert [h.attrs[0] for h in rails_amd.MoLBruteForceTopK._held_buffers() if h.refresh is not None] == ["_index", "_rows_cache", "_index32", "_rows32", "_policy"]
    assert [h.attrs[0] for h in rails_amd.MoLNaiveTopK._held_buffers() if h.refresh is not None] == ["_index", "_rows_cache", "_comp_table", "_ivf"]
