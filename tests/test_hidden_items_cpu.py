"""CPU: the host side of hidden items -- how a visibility row follows remove_items and append_items
(topk_modules.visibility_after_removal / visibility_after_append, against a numpy model on random plans), the routing rule of a scan over a
hidden set (topk_modules.hidden_scan_route), the new entries as additions under ABI 15 with their argument validation, the zero scratch of the
scans' visible kernels, and the refusals that need no device."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rails_amd
from rails_amd import _lib
from rails_amd import engine as E
from rails_amd import sharded
from rails_amd.topk_modules import hidden_scan_route, removal_plan, visibility_after_append, visibility_after_removal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NAMES = ("rails_item_mask_clear", "rails_mol_coarse_topk_visible", "rails_mol_component_topk_visible")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def packed(bits):
    """(n,) bool numpy -> (1, ceil(n / 32)) int32 tensor: little-endian bits, zero high bits in the last word (numpy alone)"""
    by = np.packbits(bits, bitorder="little")
    by = np.concatenate([by, np.zeros((-by.size) % 4, dtype=np.uint8)])
    return torch.from_numpy(np.ascontiguousarray(by).view("<u4").astype(np.uint32).view(np.int32).copy()).reshape(1, -1)


def test_removal_moves_a_movers_bit_to_its_hole():
    """The numpy model: visibility is one more column of the table -- remove_items moves the i-th mover's entry to the i-th hole and cuts to N'."""
    rng = np.random.default_rng(5)
    cases = [(33, 1), (64, 32), (65, 33), (4_037, 200), (4_037, 4_036), (8_192, 4_000), (70_001, 3)]
    for n, m in cases:
        for density in (0.0, 0.5, 0.97, 1.0):
            for tail_heavy in (False, True):
                vis = rng.random(n) < density
                if tail_heavy:      # removed positions crowd the tail: few movers, many plain cuts
                    pos = np.sort(rng.choice(np.arange(n - min(n, 2 * m), n), size=m, replace=False))
                else:
                    pos = rng.choice(n, size=m, replace=False)
                holes, movers = removal_plan(torch.from_numpy(pos.astype(np.int64)), n)
                want = vis.copy()
                want[holes.numpy()] = vis[movers.numpy()]
                want = want[: n - m]
                got = visibility_after_removal(packed(vis), n - m, holes, movers)
                assert got.dtype == torch.int32 and got.shape == (1, (n - m + 31) // 32), (n, m)
                assert torch.equal(got, packed(want)), (n, m, density, tail_heavy)
    # the flat form of the row, and a removal without holes (only tail items go): a plain cut
    vis = rng.random(100) < 0.5
    holes, movers = removal_plan(torch.arange(90, 100), 100)
    assert holes.numel() == 0 and torch.equal(visibility_after_removal(packed(vis).reshape(-1), 90, holes, movers), packed(vis[:90]))


def test_append_adds_visible_items():
    rng = np.random.default_rng(6)
    for n, n_new in ((1, 2), (31, 32), (32, 33), (33, 64), (35, 70), (64, 65), (4_037, 4_107), (4_064, 4_065), (100, 8_300)):
        for density in (0.0, 0.5, 1.0):
            vis = rng.random(n) < density
            got = visibility_after_append(packed(vis), n, n_new)
            assert torch.equal(got, packed(np.concatenate([vis, np.ones(n_new - n, dtype=bool)]))), (n, n_new, density)
    assert E.last_word_mask(32) == -1 and E.last_word_mask(33) == 1 and E.last_word_mask(63) == (1 << 31) - 1 and E.last_word_mask(5) == 31


def test_routing_rule():
    """fused while at least half the corpus is visible (the plan's 4 r sample groups keep 2 r finite maxima in expectation), materialised below;
    k beyond the visible items is what a fresh module of that size raises."""
    assert rails_amd.MoLAvgTopK.HIDDEN_FUSED_MIN_VISIBLE == 0.5 == rails_amd.MoLNaiveTopK.HIDDEN_FUSED_MIN_VISIBLE
    n = 695_762
    assert hidden_scan_route(n, n, 4000) == "fused" and hidden_scan_route(n, n - 1, 4000) == "fused"
    assert hidden_scan_route(n, n // 2, 100) == "fused" and hidden_scan_route(n, n // 2 - 1, 100) == "materialised"
    assert hidden_scan_route(4_037, 2_019, 100) == "fused" and hidden_scan_route(4_037, 2_018, 100) == "materialised"
    assert hidden_scan_route(4_037, 200, 100) == "materialised" and hidden_scan_route(4_037, 100, 100) == "materialised"
    assert hidden_scan_route(4_037, 200, 100, 0.0) == "fused"                      # (the fraction is the caller's: tests switch the rule off)
    with pytest.raises(RuntimeError, match=r"selected index k out of range \(k=101, n=100\)"):
        hidden_scan_route(4_037, 100, 101)


def test_entry_points_are_additions_under_abi_15(lib):
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert re.search(r"#define RAILS_ABI_VERSION 15\b", header) and _lib.RAILS_ABI_VERSION == 15 and lib.rails_abi_version() == 15
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    # the plain entries keep their signatures: the visible forms take one pointer more
    for plain in ("rails_mol_coarse_topk", "rails_mol_component_topk"):
        assert len(_lib.PROTOTYPES[plain + "_visible"][1]) == len(_lib.PROTOTYPES[plain][1]) + 1
    assert _lib.PROTOTYPES["rails_item_mask_clear"] == _lib.PROTOTYPES["rails_item_mask_set"]
    for cls in (rails_amd.MoLBruteForceTopK, rails_amd.MoLAvgTopK, rails_amd.MoLNaiveTopK, rails_amd.MoLCombTopK, rails_amd.MIPSBruteForceTopK):
        for name in ("hide_items", "unhide_items", "hide_items_by_id", "unhide_items_by_id", "hidden_positions", "compact", "num_hidden", "num_visible"):
            assert hasattr(cls, name), (cls.__name__, name)


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    bad = _lib.RAILS_EINVAL
    assert lib.rails_item_mask_clear(None, 3, 10, 1, None) == bad and lib.rails_item_mask_clear(1, 3, 10, None, None) == bad
    assert lib.rails_item_mask_clear(1, -1, 10, 1, None) == bad and lib.rails_item_mask_clear(1, 3, 0, 1, None) == bad
    assert lib.rails_item_mask_clear(1, 3, 1 << 31, 1, None) == bad
    assert lib.rails_item_mask_clear(None, 0, 10, 1, None) == _lib.RAILS_OK           # m = 0: nothing to do
    for visible in (None, torch.zeros(3, dtype=torch.int32)):
        E._check_visible_words(visible, 96, torch.device("cpu"))
    for wrong in (torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), torch.zeros(6, dtype=torch.int32)[::2], [0, 0, 0]):
        with pytest.raises(ValueError, match="visible"):
            E._check_visible_words(wrong, 96, torch.device("cpu"))


def test_visible_kernels_use_no_scratch():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "mol_coarse.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "visible_kernel|mask_bits_clear"], capture_output=True, text=True,
                         timeout=600).stdout
    rows = re.findall(r"scratch\s+(\d+) lds\s+\d+\s+(?:void )?mol::(\w+_kernel)", out)
    names = [r[1] for r in rows]
    # sample scans: coarse 3, component 3 + 2 wide; select scans: 3 x 2 load policies; int8: d = 32 and 64, 2 load policies; the bit clear
    assert names.count("coarse_scan_visible_kernel") == 14 and names.count("coarse_scan_i8_visible_kernel") == 4 and names.count("mask_bits_clear_kernel") == 1, out
    assert all(r[0] == "0" for r in rows), out


def test_refusals_without_a_device():
    for cls in (sharded.ShardedMoLBruteForceTopK, sharded.ShardedMoLAvgTopK, sharded.ShardedMoLNaiveTopK, sharded.ShardedMoLCombTopK):
        w = cls.__new__(cls)
        for call in (lambda: w.hide_items(torch.tensor([1])), lambda: w.unhide_items(torch.tensor([1])), lambda: w.hide_items_by_id(torch.tensor([1])),
                     lambda: w.unhide_items_by_id(torch.tensor([1])), w.hidden_positions, w.compact):
            with pytest.raises(NotImplementedError, match=cls.__name__):
                call()
