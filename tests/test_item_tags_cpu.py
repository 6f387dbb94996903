"""CPU: the host side of item tags -- how the tag row follows append_items and remove_items (topk_modules.tags_after_append /
tags_after_removal, against a numpy model), the validation of allowed_tags= without a device, the new entries as additions under ABI 15 with
their argument checks, the zero scratch of the tag kernels with the listing of the kernels around them unchanged, and the refusals that need
no device."""
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
from rails_amd.topk_modules import parse_allowed_tags, refuse_allowed_tags, removal_plan, tagged_scan_route, tags_after_append, tags_after_removal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NAMES = ("rails_item_tags_effective", "rails_item_tags_count", "rails_item_mask_from_tags", "rails_scores_mask_tags", "rails_mol_coarse_topk_tagged",
         "rails_mol_component_topk_tagged", "rails_mol_scan_plan")
KERNELS = ["item_tags_count_kernel", "item_tags_effective_kernel", "item_tags_to_mask_kernel", "scores_tags_fill_kernel"]
TAGGED_SCANS = 12      # sample scans: coarse 3 + component 3 (d = 32, 64, 128; four row tiles); select scans: 3 x 2 load policies
TAGGED_I8_SCANS = 4    # the int8 select scan: d = 32 and 64, 2 load policies


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def as_i32(words):
    """uint32 numpy bit patterns -> the int32 tensor that holds them"""
    return torch.from_numpy(words.astype(np.uint32).view(np.int32).copy())


def test_removal_moves_a_movers_word_to_its_hole():
    """The numpy model: the tag word is one more column of the table -- remove_items moves the i-th mover's entry to the i-th hole and cuts to N'."""
    rng = np.random.default_rng(7)
    for n, m in [(33, 1), (64, 32), (65, 33), (4_037, 200), (4_037, 4_036), (8_192, 4_000), (70_001, 3)]:
        for tail_heavy in (False, True):
            tags = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
            if tail_heavy:      # removed positions crowd the tail: few movers, many plain cuts
                pos = np.sort(rng.choice(np.arange(n - min(n, 2 * m), n), size=m, replace=False))
            else:
                pos = rng.choice(n, size=m, replace=False)
            holes, movers = removal_plan(torch.from_numpy(pos.astype(np.int64)), n)
            want = tags.copy()
            want[holes.numpy()] = tags[movers.numpy()]
            want = want[: n - m]
            row = as_i32(tags)
            before = row.clone()
            got = tags_after_removal(row, n - m, holes, movers)
            assert got.dtype == torch.int32 and got.shape == (n - m,) and torch.equal(got, as_i32(want)), (n, m, tail_heavy)
            assert torch.equal(row, before) and got.data_ptr() != row.data_ptr()      # a copy: the row in use is not written
    tags = rng.integers(0, 1 << 32, size=100, dtype=np.uint64).astype(np.uint32)      # a removal without holes (only tail items go): a plain cut
    holes, movers = removal_plan(torch.arange(90, 100), 100)
    assert holes.numel() == 0 and torch.equal(tags_after_removal(as_i32(tags), 90, holes, movers), as_i32(tags[:90]))


def test_append_adds_untagged_items():
    rng = np.random.default_rng(8)
    for n, n_new in ((1, 2), (31, 32), (32, 33), (33, 64), (4_037, 4_107), (100, 8_300)):
        tags = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        got = tags_after_append(as_i32(tags), n, n_new)
        assert got.dtype == torch.int32 and torch.equal(got, as_i32(np.concatenate([tags, np.zeros(n_new - n, dtype=np.uint32)]))), (n, n_new)


def test_allowed_tags_validation_without_a_device():
    assert parse_allowed_tags(5, 32) == (5,) and parse_allowed_tags((1 << 32) - 1, 1) == ((1 << 32) - 1,)
    assert parse_allowed_tags([1, 2, 1 << 31], 3) == (1, 2, 1 << 31) and parse_allowed_tags((4, 4), 2) == (4, 4)
    assert parse_allowed_tags(torch.tensor([3, 1 << 31]), 2) == (3, 1 << 31)
    assert parse_allowed_tags(torch.tensor([3, 9], dtype=torch.int32), 2) == (3, 9)
    for bad, batch in ((0, 4), (-1, 4), (1 << 32, 4), (True, 4), (1.0, 4), ("3", 1), (None, 4), ([1, 2], 3), ([1, 0, 2], 3), ([1, -5, 2], 3), ([1, 1 << 32, 2], 3),
                       ([1.0, 2.0], 2), ([True, True], 2), (torch.tensor([1, 2]), 3), (torch.tensor([1.0, 2.0]), 2), (torch.tensor([[1, 2]]), 2),
                       (torch.tensor([1, 0]), 2), (torch.tensor([True, True]), 2)):
        with pytest.raises(ValueError):
            parse_allowed_tags(bad, batch)
    assert E.tag_word_i32(1) == 1 and E.tag_word_i32((1 << 31) - 1) == (1 << 31) - 1 and E.tag_word_i32(1 << 31) == -(1 << 31) and E.tag_word_i32((1 << 32) - 1) == -1
    # set_item_tags refuses before it looks at a device: shapes, dtypes, and a module without tags refuses the call
    tk = rails_amd.MoLAvgTopK.__new__(rails_amd.MoLAvgTopK)
    assert tk.item_tags is None
    with pytest.raises(ValueError, match="without tags"):
        tk._take_allowed_tags({"allowed_tags": 1}, 4, ())
    assert tk._take_allowed_tags({"user_ids": None}, 4, ()) is None and tk._take_allowed_tags({"allowed_tags": None}, 4, ()) is None


def test_routing_rule_on_hand_computed_plans(lib):
    """fused iff the least-kept row still expects 2 r finite group maxima: G (1 - (1 - v)^s) >= 2 r."""
    assert rails_amd.MoLAvgTopK.TAGGED_FUSED_MIN_GROUPS == 2.0 == rails_amd.MoLNaiveTopK.TAGGED_FUSED_MIN_GROUPS
    # groups of ONE item: the rule is hidden_scan_route's v >= 1/2 on a plan of 4 r groups
    one = (4, 10, 40, 1)
    assert tagged_scan_route(one, 50, 100, 5) == "fused" and tagged_scan_route(one, 49, 100, 5) == "materialised"
    assert tagged_scan_route(one, 100, 100, 5) == "fused" and tagged_scan_route(one, 5, 100, 5) == "materialised"
    assert tagged_scan_route(one, 5, 100, 5, 0.0) == "fused"                            # (the factor is the caller's: tests switch the rule off)
    assert tagged_scan_route(None, 50, 100, 5) == "materialised"                        # sizes without a fused plan
    with pytest.raises(RuntimeError, match=r"selected index k out of range \(k=6, n=5\)"):
        tagged_scan_route(one, 5, 100, 6)
    # amzn-books, B = 32, K' = 200: 21 743 tiles, a small corpus -> stride = max(200 / 64, ceil(N / 65 536)) = 11, 1 977 sampled tiles, 124 workgroups
    # of four waves of which ceil(1 977 / 4) = 495 see a trip: G = 495 * 32 = 15 840 maxima of ceil(1 977 / 495) = 4 sampled items each
    n = 695_762
    plan = E.scan_plan(32, n, 200)
    assert plan[0] == 11 and plan[2:] == (15_840, 4) and 30 <= plan[1] <= 70, plan
    r = plan[1]
    assert 15_840 * (1 - 0.95 ** 4) > 2_900 > 2 * r and tagged_scan_route(plan, n // 20, n, 200) == "fused"            # 5 % kept: ~2 938 finite maxima
    assert tagged_scan_route(plan, n // 100, n, 200) == "fused"                                                          # 1 %: ~624
    assert tagged_scan_route(plan, 400, n, 200) == "materialised"                                                        # 0.06 %: ~36 < 2 r
    # the component plan of the same call (k_g = 5; 2 048 rows, 256 query rows): stride 4, 32 workgroups per item group -> 4 096 maxima of 43 items
    comp = E.scan_plan(32 * 64, n, 5, 32 * 8)
    assert comp[0] == 4 and comp[2:] == (4_096, 43) and tagged_scan_route(comp, n // 100, n, 5) == "fused", comp
    # the tests' corpus: N = 4 037, K' = 100 -> 256 maxima of 4 items, r = 61: fused at 60 % kept, materialised at one category of eight
    small = E.scan_plan(2, 4_037, 100)
    assert small[2:] == (256, 4) and tagged_scan_route(small, 2_400, 4_037, 100) == "fused" and tagged_scan_route(small, 500, 4_037, 100) == "materialised"
    assert E.scan_plan(2, 3_000, 100) is None and E.scan_plan(2, 50, 100) is None       # too small for a sparse sample; k beyond n


def test_entry_points_are_additions_under_abi_15(lib):
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert re.search(r"#define RAILS_ABI_VERSION 15\b", header) and _lib.RAILS_ABI_VERSION == 15 and lib.rails_abi_version() == 15
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    # each is its plain counterpart plus its extra arguments: the tag mask takes (eff_tags, allowed, rows_per_allowed) where rails_scores_mask
    # takes (words, words_row_stride); the mask rows come from (eff_tags, n, allowed) where rails_item_mask_pack takes (mask_u8, ld)
    assert len(_lib.PROTOTYPES["rails_scores_mask_tags"][1]) == len(_lib.PROTOTYPES["rails_scores_mask"][1]) + 1
    assert len(_lib.PROTOTYPES["rails_item_mask_from_tags"][1]) == len(_lib.PROTOTYPES["rails_item_mask_pack"][1])
    # the tagged scans are the _visible entries with (eff_tags, allowed) in place of visible_words, the plain ones plus two pointers
    for plain in ("rails_mol_coarse_topk", "rails_mol_component_topk"):
        assert len(_lib.PROTOTYPES[plain + "_tagged"][1]) == len(_lib.PROTOTYPES[plain + "_visible"][1]) + 1 == len(_lib.PROTOTYPES[plain][1]) + 2
        assert _lib.PROTOTYPES[plain + "_tagged"][1][:len(_lib.PROTOTYPES[plain][1]) - 1] == _lib.PROTOTYPES[plain][1][:-1]
    for cls in (rails_amd.MoLBruteForceTopK, rails_amd.MoLAvgTopK, rails_amd.MoLNaiveTopK, rails_amd.MoLCombTopK, rails_amd.MIPSBruteForceTopK):
        assert hasattr(cls, "set_item_tags") and isinstance(cls.item_tags, property), cls.__name__


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    bad, ok = _lib.RAILS_EINVAL, _lib.RAILS_OK
    assert lib.rails_item_tags_effective(None, 1, 10, 1, None) == bad and lib.rails_item_tags_effective(1, None, 10, 1, None) == bad
    assert lib.rails_item_tags_effective(1, 1, 10, None, None) == bad and lib.rails_item_tags_effective(1, 1, 0, 1, None) == bad
    assert lib.rails_item_tags_effective(1, 1, 1 << 31, 1, None) == bad
    assert lib.rails_item_tags_count(None, 10, 1, 2, 1, None) == bad and lib.rails_item_tags_count(1, 10, None, 2, 1, None) == bad
    assert lib.rails_item_tags_count(1, 10, 1, 2, None, None) == bad and lib.rails_item_tags_count(1, 0, 1, 2, 1, None) == bad
    assert lib.rails_item_tags_count(1, 10, 1, -1, 1, None) == bad and lib.rails_item_tags_count(1, 10, 1, (1 << 16) + 1, 1, None) == bad
    assert lib.rails_item_tags_count(None, 10, None, 0, None, None) == ok                    # no words: nothing to do
    assert lib.rails_item_mask_from_tags(None, 10, 1, 2, 1, 1, None) == bad and lib.rails_item_mask_from_tags(1, 10, None, 2, 1, 1, None) == bad
    assert lib.rails_item_mask_from_tags(1, 10, 1, 2, None, 1, None) == bad and lib.rails_item_mask_from_tags(1, 10, 1, 2, 1, None, None) == bad
    assert lib.rails_item_mask_from_tags(1, 10, 1, 0, 1, 1, None) == bad and lib.rails_item_mask_from_tags(1, 0, 1, 2, 1, 1, None) == bad
    # rails_scores_mask_tags: ld < n, negative sizes, rows_per_allowed < 1, NULL pointers; rows = 0 / n = 0 are no-ops
    assert lib.rails_scores_mask_tags(1, 9, 1, 10, 0, 1, 1, 1, 0.0, None, None) == bad
    assert lib.rails_scores_mask_tags(1, 10, 1, 10, -1, 1, 1, 1, 0.0, None, None) == bad
    assert lib.rails_scores_mask_tags(1, 10, -1, 10, 0, 1, 1, 1, 0.0, None, None) == bad
    assert lib.rails_scores_mask_tags(1, 10, 3, 10, 0, 1, 1, 0, 0.0, None, None) == bad and "rows_per_allowed" in _lib.last_error()
    assert lib.rails_scores_mask_tags(None, 10, 3, 10, 0, 1, 1, 1, 0.0, None, None) == bad and lib.rails_scores_mask_tags(1, 10, 3, 10, 0, None, 1, 1, 0.0, None, None) == bad
    assert lib.rails_scores_mask_tags(1, 10, 3, 10, 0, 1, None, 1, 0.0, None, None) == bad
    assert lib.rails_scores_mask_tags(None, 10, 0, 10, 0, None, None, 1, 0.0, None, None) == ok
    assert lib.rails_scores_mask_tags(None, 10, 3, 0, 0, None, None, 1, 0.0, None, None) == ok


def test_tag_kernels_use_no_scratch_and_their_neighbours_did_not_move():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "item_mask.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "item_tags|scores_tags|coarse|item_mask|scores_mask|mask_bits"],
                         capture_output=True, text=True, timeout=600).stdout
    lines = [line for line in out.splitlines() if line.startswith("vgpr")]
    new = [line for line in lines if re.search(r"item_tags|scores_tags|tagged_kernel", line)]
    rows = re.findall(r"scratch\s+(\d+) lds\s+\d+\s+(?:void )?mol::(\w+_kernel)", "\n".join(new))
    assert sorted(r[1] for r in rows) == sorted(KERNELS + ["coarse_scan_tagged_kernel"] * TAGGED_SCANS + ["coarse_scan_i8_tagged_kernel"] * TAGGED_I8_SCANS) and all(r[0] == "0" for r in rows), out
    # the kernels that existed before the feature in the files it touched (item_mask.hip, mol_coarse.hip): registers, LDS and scratch as recorded
    # then.  Only those symbols are compared: a kernel the recorded listing does not know is none of this test's business.
    before = open(os.path.join(ROOT, "tests", "golden", "item_tags_kernels_before.txt")).read().splitlines()
    missing = sorted(set(before) - set(lines))
    assert not missing, missing


def test_refusals_without_a_device():
    class MoLAvgTopK:          # (refuse_allowed_tags reads the type's name alone)
        pass

    refuse_allowed_tags(MoLAvgTopK(), {"user_ids": None}, "why")
    refuse_allowed_tags(MoLAvgTopK(), {"allowed_tags": None}, "why")
    with pytest.raises(NotImplementedError, match="MoLAvgTopK takes no allowed_tags: why"):
        refuse_allowed_tags(MoLAvgTopK(), {"allowed_tags": 1}, "why")
    # the IVF module refuses at the resolution of the argument, before it looks at its tags
    for frozen in (False, True):
        ivf = rails_amd.MoLNaiveTopK.__new__(rails_amd.MoLNaiveTopK)
        ivf._use_faiss, ivf._frozen_centroids = True, frozen
        with pytest.raises(NotImplementedError, match="MoLNaiveTopK.*IVF"):
            ivf._take_allowed_tags({"allowed_tags": 1}, 4, (5,))
    # every entry point of the sharded wrappers refuses, beside its item_mask refusal
    src = open(os.path.join(ROOT, "rails_amd", "sharded.py")).read()
    entries = re.findall(r"    def (?:forward|forward_filtered|submit)\(self, query_embeddings", src)
    assert len(entries) >= 9 and src.count("refuse_allowed_tags(self, kwargs, _TAGS_WHY)") == len(entries) == src.count("refuse_item_mask(self, kwargs, _MASK_WHY)")
    for cls in (sharded.ShardedMoLBruteForceTopK, sharded.ShardedMoLAvgTopK, sharded.ShardedMoLNaiveTopK, sharded.ShardedMoLCombTopK):
        w = cls.__new__(cls)
        with pytest.raises(NotImplementedError, match=cls.__name__):
            w.set_item_tags(torch.tensor([1]))
        with pytest.raises(NotImplementedError, match=cls.__name__):
            w.item_tags
        with pytest.raises(NotImplementedError, match=f"{cls.__name__} takes no allowed_tags"):
            refuse_allowed_tags(w, {"allowed_tags": 3}, sharded._TAGS_WHY)
