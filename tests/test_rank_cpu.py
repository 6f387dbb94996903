"""CPU: rank_of without a device -- the three entry points are additions under ABI 15 and validate before any launch, the new
kernels use no scratch, tests/_rank_ref.py agrees with an explicit sort, the refusals name their module, the harness refuses what the exact path
cannot give."""
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rails_amd
from rails_amd import _lib
from rails_amd import engine as E
from rails_amd import eval_harness as H
from rails_amd import sharded
from tests import _rank_ref
from tests import _topk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NAMES = ("rails_scores_rank_keys", "rails_scores_rank", "rails_item_mask_clear_rows")
KERNELS = {"scores_rank_keys_kernel", "scores_rank_kernel", "scores_rank_finish_kernel", "mask_rows_clear_kernel"}


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
    assert "rank.hip" in open(os.path.join(ROOT, "rails_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "rails_amd", "csrc", "rank.hip")).read()
    assert '#include "topk_keys.h"' in src and "orderable(float" not in src and "make_key(float" not in src      # one codec: the header's
    assert E.RANK_MAX_TARGETS == 64


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    bad, ok = _lib.RAILS_EINVAL, _lib.RAILS_OK
    # rails_scores_rank_keys(scores, ld, rows, n, positions, t, keys_out, stream)
    for args in ((None, 10, 2, 10, 1, 3, 1), (1, 10, 2, 10, None, 3, 1), (1, 10, 2, 10, 1, 3, None)):
        assert lib.rails_scores_rank_keys(*args, None) == bad and "NULL" in _lib.last_error(), args
    assert lib.rails_scores_rank_keys(1, 9, 2, 10, 1, 3, 1, None) == bad and "ld" in _lib.last_error()
    for t in (0, -1, 65):
        assert lib.rails_scores_rank_keys(1, 10, 2, 10, 1, t, 1, None) == bad and "[1, 64]" in _lib.last_error(), t
    # rails_scores_rank(scores, ld, rows, n, keys, t, mask_words, words_row_stride, ranks_out, stream)
    for args in ((None, 10, 2, 10, 1, 3, None, 0, 1), (1, 10, 2, 10, None, 3, None, 0, 1), (1, 10, 2, 10, 1, 3, None, 0, None)):
        assert lib.rails_scores_rank(*args, None) == bad and "NULL" in _lib.last_error(), args
    assert lib.rails_scores_rank(1, 9, 2, 10, 1, 3, None, 0, 1, None) == bad and "ld" in _lib.last_error()
    for t in (0, -1, 65):
        assert lib.rails_scores_rank(1, 10, 2, 10, 1, t, None, 0, 1, None) == bad and "[1, 64]" in _lib.last_error(), t
    for stride in (1, 3, -1):      # 100 bits need 4 words; 0 is the shared row
        assert lib.rails_scores_rank(1, 100, 2, 100, 1, 3, 1, stride, 1, None) == bad and "shorter" in _lib.last_error(), stride
    for rows, n in ((-1, 10), (1, 0), (1, -3), (1, 1 << 31), ((1 << 24) + 1, 10)):
        assert lib.rails_scores_rank_keys(1, max(n, 0), rows, n, 1, 1, 1, None) == bad, (rows, n)
        assert lib.rails_scores_rank(1, max(n, 0), rows, n, 1, 1, None, 0, 1, None) == bad, (rows, n)
        assert lib.rails_item_mask_clear_rows(1, rows, 5, n, 1, 1 << 26, None) == bad, (rows, n)
    # rows = 0: nothing to do
    assert lib.rails_scores_rank_keys(None, 10, 0, 10, None, 3, None, None) == ok
    assert lib.rails_scores_rank(None, 10, 0, 10, None, 3, None, 0, None, None) == ok
    # rails_item_mask_clear_rows(positions, rows, m, n, words, words_row_stride, stream)
    assert lib.rails_item_mask_clear_rows(None, 2, 5, 100, 1, 4, None) == bad and "NULL" in _lib.last_error()
    assert lib.rails_item_mask_clear_rows(1, 2, 5, 100, None, 4, None) == bad and "NULL" in _lib.last_error()
    assert lib.rails_item_mask_clear_rows(1, 2, -1, 100, 1, 4, None) == bad
    for stride in (0, 3, -4):
        assert lib.rails_item_mask_clear_rows(1, 2, 5, 100, 1, stride, None) == bad and "shorter" in _lib.last_error(), stride
    assert lib.rails_item_mask_clear_rows(None, 0, 5, 100, None, 4, None) == ok
    assert lib.rails_item_mask_clear_rows(None, 2, 0, 100, None, 4, None) == ok


def test_engine_argument_checks():
    """The checks of scores_mask on the new calls: CPU tensors are refused as everywhere else, before anything else is looked at."""
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.scores_rank(torch.zeros((2, 10)), torch.zeros((2, 1), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.item_mask_clear_rows(torch.zeros((2, 1), dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64))
    assert list(inspect.signature(E.scores_rank).parameters) == ["scores", "positions", "mask"]


def test_rank_kernels_use_no_scratch():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "rank.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "scores_rank|mask_rows_clear"], capture_output=True, text=True,
                         timeout=600).stdout
    rows = re.findall(r"scratch\s+(\d+) lds\s+(\d+)\s+(?:void )?mol::(\w+_kernel)", out)
    assert {r[2] for r in rows} == KERNELS, out
    assert sum(r[2] == "scores_rank_kernel" for r in rows) == 8, out      # four tiers of t, with and without a mask
    assert all(r[0] == "0" for r in rows), out


# ---- the reference against an explicit sort --------------------------------------------------------------------------------------
def _orderable(u: int) -> int:      # the codec of rails_amd/csrc/topk_keys.h on Python integers
    return (~u) & 0xFFFFFFFF if u & 0x80000000 else u | 0x80000000


def _by_sort(bits, eligible, targets):
    out = np.zeros(targets.shape, dtype=np.int64)
    for b in range(bits.shape[0]):
        # score descending (by the codec's order), then position ascending
        order = sorted((y for y in range(bits.shape[1]) if eligible[b, y]), key=lambda y: (-_orderable(int(bits[b, y])), y))
        for j, x in enumerate(targets[b]):
            if x in order:
                out[b, j] = 1 + order.index(x)
    return out


def test_reference_against_an_explicit_sort():
    rng = np.random.default_rng(5)
    seen_sizes = set()
    for n in list(range(1, 34)) + [63, 64, 65, 100, 127, 128, 129, 199, 200]:
        for name in ("gauss", "constant", "signed_zeros", "nans", "all_negative", "low_byte") + (("subnormals",) if n in (1, 33, 200) else ()):
            bits = np.stack([R.FAMILIES[name](n, max(1, n // 2), rng) for _ in range(2)])
            for p in (1.0, 0.5, 0.0):
                eligible = rng.random((2, n)) < p
                targets = np.stack([np.concatenate([rng.integers(0, n, size=4), [-1, n, 0, n - 1]]) for _ in range(2)])
                want = _by_sort(bits, eligible, targets)
                got = _rank_ref.ranks(bits, eligible, targets)
                assert got.dtype == np.int64 and np.array_equal(got, want), (n, name, p)
                if p == 1.0:
                    assert got[:, 4].tolist() == [0, 0] and got[:, 5].tolist() == [0, 0] and (got[:, 6:] >= 1).all()
                if p == 0.0:
                    assert not got.any()
        seen_sizes.add(n)
    assert {1, 200} <= seen_sizes
    # ties break by position ascending; +0 above -0; a NaN by its bits (positive ones above +inf, negative ones below -inf)
    bits = np.array([[0x3F000000] * 5], dtype=np.uint32)
    assert _rank_ref.ranks(bits, np.ones((1, 5), bool), np.arange(5)[None]).tolist() == [[1, 2, 3, 4, 5]]
    assert _rank_ref.ranks(bits, np.array([[0, 1, 0, 1, 1]], bool), np.arange(5)[None]).tolist() == [[0, 1, 0, 2, 3]]
    bits = np.array([[0x80000000, 0x00000000, 0x7F800000, 0x7FC00000, 0xFF800000, 0xFFC00000]], dtype=np.uint32)
    assert _rank_ref.ranks(bits, np.ones((1, 6), bool), np.arange(6)[None]).tolist() == [[4, 3, 2, 1, 5, 6]]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _bare(cls):
    return cls.__new__(cls)      # (a refusal reads the type alone: nothing is constructed, nothing is launched)


def test_refusals_name_the_module():
    for cls in (rails_amd.MoLAvgTopK, rails_amd.MoLNaiveTopK, rails_amd.MoLCombTopK):
        for call in ("rank_of", "rank_of_positions"):
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call}: .*MoLBruteForceTopK"):
                getattr(_bare(cls), call)(None, None)
    for cls in (rails_amd.MoLBruteForceTopK, rails_amd.MIPSBruteForceTopK):
        for call in ("rank_of", "rank_of_positions"):
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call} takes no collapse_groups"):
                getattr(_bare(cls), call)(None, None, collapse_groups=True)
    # the sharded wrappers: every class of sharded.py that is a top-k module refuses, through the one base that says why
    src = open(os.path.join(ROOT, "rails_amd", "sharded.py")).read()
    classes = [getattr(sharded, name) for name in re.findall(r"^class (\w+)\(", src, flags=re.M)]
    wrappers = [c for c in classes if issubclass(c, rails_amd.topk_modules.TopKModule)]
    assert len(wrappers) >= 6 and all(issubclass(c, sharded.ShardedTopK) for c in wrappers)
    assert src.count("def rank_of(") == 1 and src.count("def rank_of_positions(") == 1
    for cls in wrappers:
        for call in ("rank_of", "rank_of_positions"):
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call}: .*single-device MoLBruteForceTopK"):
                getattr(_bare(cls), call)(None, None)


def test_harness_refuses_what_the_exact_path_cannot_give():
    call = functools.partial(H.eval_metrics_v2_from_tensors, None, None, None, torch.zeros((2, 1), dtype=torch.int64), exact_ranks=True)
    with pytest.raises(ValueError, match="include_eval_time"):
        call(include_eval_time=True)
    with pytest.raises(ValueError, match="include_eval_top_k_ids"):
        call(include_eval_top_k_ids=True)

    class NoRanks:
        pass

    state = H.EvalState(all_item_ids=set(), candidate_index=None, top_k_module=NoRanks())
    with pytest.raises(NotImplementedError, match="NoRanks has no rank_of"):
        H.eval_metrics_v2_from_tensors(state, None, None, torch.zeros((2, 1), dtype=torch.int64), exact_ranks=True)
    assert inspect.signature(H.eval_metrics_v2_from_tensors).parameters["exact_ranks"].default is False
