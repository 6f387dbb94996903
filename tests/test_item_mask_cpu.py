"""CPU: the host side of the item masks (rails_item_mask_*, rails_scores_mask) -- the entries are additions under ABI 15,
their argument validation before any launch, the kernels' scratch use, the pure routing rule of a masked call (topk_modules.mask_strategy)
at its boundaries, and the pure checks of a masked call (engine.check_item_mask) and the refusals, none of which needs a device."""
import os
import re
import subprocess

import pytest
import torch

import rails_amd
from rails_amd import _lib
from rails_amd import engine as E
from rails_amd import sharded
from rails_amd.topk_modules import mask_strategy, refuse_item_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NAMES = ("rails_item_mask_words", "rails_item_mask_tile_items", "rails_item_mask_pack", "rails_item_mask_set", "rails_item_mask_count",
         "rails_item_mask_positions_workspace_bytes", "rails_item_mask_positions", "rails_scores_mask")
KERNELS = ["item_mask_count_kernel", "item_mask_pack_kernel", "item_mask_pad_kernel", "item_mask_set_kernel", "item_mask_tile_counts_kernel",
           "item_mask_tile_scan_kernel", "item_mask_tile_write_kernel", "scores_mask_kernel"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_entry_points_are_additions_under_abi_15(lib):
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert re.search(r"#define RAILS_ABI_VERSION 15\b", header) and _lib.RAILS_ABI_VERSION == 15 and lib.rails_abi_version() == 15
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    assert "item_mask.hip" in open(os.path.join(ROOT, "rails_amd", "csrc", "Makefile")).read()
    assert rails_amd.ItemMask is E.ItemMask and "ItemMask" in rails_amd.__all__


def test_size_helpers(lib):
    for n, words in {0: 0, 1: 1, 31: 1, 32: 1, 33: 2, 64: 2, 65: 3, 695_762: 21_743, (1 << 31) - 1: 1 << 26}.items():
        assert lib.rails_item_mask_words(n) == words == E.item_mask_words(n), n
    assert lib.rails_item_mask_words(-5) == 0
    tile = lib.rails_item_mask_tile_items()
    assert tile == 8192
    # one 64-bit tile offset per tile and row, one total per row
    for rows, n in ((1, 1), (3, tile), (3, tile + 1), (32, 125_000_000)):
        assert lib.rails_item_mask_positions_workspace_bytes(rows, n) == 8 * rows * (-(-n // tile) + 1), (rows, n)
    assert lib.rails_item_mask_positions_workspace_bytes(0, 5) == 0 and lib.rails_item_mask_positions_workspace_bytes(1, 0) == 0
    assert lib.rails_item_mask_positions_workspace_bytes(1, 1 << 31) == 0


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    bad = _lib.RAILS_EINVAL
    for args in ((None, 10, 1, 10, 1, 1, None), (1, 10, 1, 10, None, 1, None), (1, 10, 1, 10, 1, None, None)):
        assert lib.rails_item_mask_pack(*args) == bad and "NULL" in _lib.last_error(), args
    assert lib.rails_item_mask_pack(1, 9, 2, 10, 1, 1, None) == bad and "ld" in _lib.last_error()
    for rows, n in ((0, 10), (-1, 10), (1, 0), (1, -3), (1, 1 << 31), ((1 << 24) + 1, 10)):
        assert lib.rails_item_mask_pack(1, max(n, 0), rows, n, 1, 1, None) == bad, (rows, n)
        assert lib.rails_item_mask_count(1, rows, n, 1, None) == bad, (rows, n)
        assert lib.rails_item_mask_positions(1, rows, n, 1, 4, 1, 1 << 40, None) == bad, (rows, n)
    assert lib.rails_item_mask_set(None, 3, 10, 1, None) == bad and lib.rails_item_mask_set(1, 3, 10, None, None) == bad
    assert lib.rails_item_mask_set(1, -1, 10, 1, None) == bad and lib.rails_item_mask_set(1, 3, 0, 1, None) == bad
    assert lib.rails_item_mask_set(None, 0, 10, 1, None) == _lib.RAILS_OK           # m = 0: nothing to do
    assert lib.rails_item_mask_count(None, 1, 10, 1, None) == bad and lib.rails_item_mask_count(1, 1, 10, None, None) == bad
    assert lib.rails_item_mask_positions(1, 2, 8193, 1, -1, 1, 1 << 20, None) == bad
    assert lib.rails_item_mask_positions(1, 2, 8193, None, 4, 1, 1 << 20, None) == bad
    assert lib.rails_item_mask_positions(1, 2, 8193, 1, 4, 1, 8 * 2 * 3 - 1, None) == _lib.RAILS_ENOMEM and "workspace" in _lib.last_error()
    # rails_scores_mask: ld < n, negative sizes, a mask row shorter than first_item + n bits, NULL pointers; rows = 0 / n = 0 are no-ops
    assert lib.rails_scores_mask(1, 9, 1, 10, 0, 1, 0, 0.0, None, None) == bad
    assert lib.rails_scores_mask(1, 10, 1, 10, -1, 1, 0, 0.0, None, None) == bad
    assert lib.rails_scores_mask(1, 10, -1, 10, 0, 1, 0, 0.0, None, None) == bad
    assert lib.rails_scores_mask(1, 10, 3, 10, 101, 1, 3, 0.0, None, None) == bad and "shorter" in _lib.last_error()      # 111 bits need 4 words
    assert lib.rails_scores_mask(None, 10, 3, 10, 0, 1, 0, 0.0, None, None) == bad and lib.rails_scores_mask(1, 10, 3, 10, 0, None, 0, 0.0, None, None) == bad
    assert lib.rails_scores_mask(None, 10, 0, 10, 0, None, 0, 0.0, None, None) == _lib.RAILS_OK
    assert lib.rails_scores_mask(None, 10, 3, 0, 0, None, 0, 0.0, None, None) == _lib.RAILS_OK


def test_item_mask_kernels_use_no_scratch():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "item_mask.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "item_mask|scores_mask"], capture_output=True, text=True, timeout=600).stdout
    rows = re.findall(r"scratch\s+(\d+) lds\s+(\d+)\s+mol::(\w+_kernel)", out)
    assert sorted(r[2] for r in rows) == KERNELS, out
    assert all(r[0] == "0" for r in rows), out


def test_routing_at_its_boundaries():
    T = rails_amd.MoLBruteForceTopK
    assert T.MASK_SPARSE_MAX == 16384 and T.MASK_SPARSE_FACTOR == 4
    route = lambda kept, n, ok=True, cap=T.MASK_SPARSE_MAX: mask_strategy(kept, n, cap, T.MASK_SPARSE_FACTOR, ok)      # noqa: E731
    big = 695_762
    assert route(16_384, big) == "sparse" and route(16_385, big) == "dense"         # the limit of one ranking launch
    assert route(3_004, 70_001) == "sparse" and route(1, 4) == "sparse"
    for n in (40_000, 60_001):                                                        # 4 * kept_max == N / N + 1
        kept = n // 4
        assert route(kept, 4 * kept) == "sparse" and route(kept, 4 * kept + 1) == "sparse" and route(kept, 4 * kept - 1) == "dense"
        assert route(kept + 1, 4 * kept + 3) == "dense" and route(kept + 1, 4 * kept + 4) == "sparse"
    assert route(10_000, 40_000) == "sparse" and route(10_001, 40_000) == "dense"     # 4 * kept_max == N, N + 1
    # an engine that cannot score positions in place (the generic route, the split-f16 precisions) is always dense
    for kept, n in ((1, 4), (3_004, 70_001), (16_384, big)):
        assert route(kept, n, ok=False) == "dense"
    # the instance override of the cap: 0 = never sparse; a cap beyond the ranking launch's limit does not lift it; an empty mask is dense
    assert route(3_004, 70_001, cap=0) == "dense" and route(16_385, big, cap=1 << 20) == "dense" and route(0, big) == "dense"


def test_the_pure_checks_of_a_masked_call():
    check = E.check_item_mask          # (mask items, mask rows, shared, kept_min, module items, batch, k)
    check(70_001, 1, True, 3_004, 70_001, 32, 200)
    check(70_001, 32, False, 200, 70_001, 32, 200)
    check(70_001, 32, False, 200, 70_001, 32, None)
    with pytest.raises(ValueError, match="by position"):       # a stale mask: the corpus grew or shrank
        check(70_001, 1, True, 3_004, 70_002, 32, 10)
    with pytest.raises(ValueError, match="rows"):              # a per-row mask of another batch
        check(70_001, 31, False, 200, 70_001, 32, 10)
    with pytest.raises(ValueError, match="rows"):
        check(70_001, 1, False, 200, 70_001, 32, 10)
    with pytest.raises(RuntimeError, match=r"selected index k out of range \(k=201, n=200\)"):     # the text of k > N
        check(70_001, 32, False, 200, 70_001, 32, 201)
    # a CPU mask: the error of CPU tensors everywhere else
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.ItemMask(torch.ones(10, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.ItemMask.from_positions(10, torch.tensor([1, 2]), "cpu")
    for wrong in (torch.ones(10), torch.ones((2, 3, 4), dtype=torch.bool), torch.ones((0,), dtype=torch.bool), [True, False]):
        with pytest.raises(ValueError):
            E.ItemMask(wrong)


def test_refusals_name_the_module():
    class MoLAvgTopK:          # (refuse_item_mask reads the type's name and _use_faiss alone)
        pass

    class MoLNaiveTopK:
        _use_faiss = True

    refuse_item_mask(MoLAvgTopK(), {"user_ids": None})
    refuse_item_mask(MoLAvgTopK(), {"item_mask": None})
    with pytest.raises(NotImplementedError, match="MoLAvgTopK takes no item_mask"):
        refuse_item_mask(MoLAvgTopK(), {"item_mask": object()})
    with pytest.raises(NotImplementedError, match="IVF"):
        refuse_item_mask(MoLNaiveTopK(), {"item_mask": object()})
    src = {name: open(os.path.join(ROOT, "rails_amd", name)).read() for name in ("topk_modules.py", "sharded.py")}
    assert src["topk_modules.py"].count("refuse_item_mask(self, kwargs)") >= 4      # Avg submit / forward_filtered, the component modules, the base all_logits
    # every entry point of the sharded wrappers refuses
    entries = re.findall(r"    def (?:forward|forward_filtered|submit)\(self, query_embeddings", src["sharded.py"])
    assert len(entries) >= 9 and src["sharded.py"].count("refuse_item_mask(self, kwargs, _MASK_WHY)") == len(entries)
    assert issubclass(sharded.ShardedMoLBruteForceTopK, sharded.ShardedTopK)
