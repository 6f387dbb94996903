"""CPU: the range search without a device -- the entry points additions under ABI 15 that validate before any launch, the
kernels' resources and sources, the engine's argument checks, the refusals by name, and the reference of tests/_range_ref.py against the
selection reference it is built on."""
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
from rails_amd import sharded
from tests import _range_ref as G
from tests import _topk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rails_scores_range_workspace_bytes", "rails_scores_range_count", "rails_scores_range_write", "rails_scores_range_sort",
         "rails_scores_range_decode")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = {"scores_range_count_kernel", "scores_range_offsets_kernel", "scores_range_write_kernel", "scores_range_sort_kernel",
           "scores_range_decode_kernel"}
CALLS = ("count_above", "range_search")
CAP_N = 20_000      # the cap fixture: a row of CAP_N distinct values whose threshold 16 384 (16 385) of them meet


def cap_fixture(count: int):
    """(bits (1, CAP_N) uint32, threshold) with exactly `count` hits"""
    bits = R.gauss(CAP_N, count, np.random.default_rng(61))[None]
    return bits, G.threshold_for(bits[0], np.ones(CAP_N, dtype=bool), count)


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
    assert "range.hip" in open(os.path.join(ROOT, "rails_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "rails_amd", "csrc", "range.hip")).read()
    for header_name in ("score_rows.h", "wave_ops.h", "topk_keys.h"):
        assert f'#include "{header_name}"' in src
    assert "for_row_chunk<MASKED>" in src and "block_scan_excl" in src and "lds_sort_desc" in src and "__fmul_rn" in src
    assert list(inspect.signature(E.scores_range_count).parameters) == ["scores", "thresholds", "mask", "temperature", "lse"]
    assert list(inspect.signature(E.scores_range).parameters) == ["scores", "thresholds", "mask", "temperature", "lse", "ids", "sort"]
    assert inspect.signature(E.scores_range).parameters["sort"].default is True
    assert E.RANGE_SORT_MAX == E.TOPK_MAX_K == R.kSortCap


def test_no_atomics_on_the_path():
    """Bit-reproducible by construction: the range kernels and the two headers they stand on hold no atomic of any kind, floating-point or not
    (rank.hip's integer atomics are its own)."""
    for name in ("range.hip", "score_rows.h", "wave_ops.h"):
        src = open(os.path.join(ROOT, "rails_amd", "csrc", name)).read()
        code = "\n".join(line.split("//")[0] for line in src.splitlines())
        assert not re.search(r"\batomic\w*\s*\(|__atomic_|__hip_atomic", code), name
        assert "__expf" not in src and "__logf" not in src and "fmaf" not in code, name


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    bad, ok, nomem, notsup = _lib.RAILS_EINVAL, _lib.RAILS_OK, _lib.RAILS_ENOMEM, _lib.RAILS_ENOTSUP
    big = 1 << 30
    # rails_scores_range_count(scores, ld, rows, n, thresholds, inv_temperature, lse, mask_words, words_row_stride, workspace, workspace_bytes,
    #                          counts_out, lims_out, stream)
    good = [1, 10, 2, 10, 1, 1.0, None, None, 0, 1, big, 1, 1]
    for at in (0, 4, 9, 11, 12):      # scores, thresholds, workspace, counts_out, lims_out
        args = list(good)
        args[at] = None
        assert lib.rails_scores_range_count(*args, None) == bad and "NULL" in _lib.last_error(), at
    # rails_scores_range_write(the same inputs ..., workspace, workspace_bytes, keys_out, capacity, stream)
    good_w = [1, 10, 2, 10, 1, 1.0, None, None, 0, 1, big, 1, 5]
    for at in (0, 4, 9, 11):          # scores, thresholds, workspace, keys_out
        args = list(good_w)
        args[at] = None
        assert lib.rails_scores_range_write(*args, None) == bad and "NULL" in _lib.last_error(), at
    for call, args in ((lib.rails_scores_range_count, good), (lib.rails_scores_range_write, good_w)):
        a = list(args)
        a[1] = 9
        assert call(*a, None) == bad and "ld" in _lib.last_error()
        for rows, n in ((-1, 10), (1, 0), (1, -3), ((1 << 24) + 1, 10), (1, 1 << 31)):
            a = list(args)
            a[1], a[2], a[3] = max(n, 0), rows, n
            assert call(*a, None) == bad, (rows, n)
        for beta in (0.0, -1.0, float("inf"), float("nan")):
            a = list(args)
            a[5] = beta
            assert call(*a, None) == bad and "inv_temperature" in _lib.last_error(), beta
        for stride in (1, 3, -1):      # 100 bits need 4 words; 0 is the shared row
            a = list(args)
            a[1], a[3], a[7], a[8] = 100, 100, 1, stride
            assert call(*a, None) == bad and "shorter" in _lib.last_error(), stride
    for rows, n in ((-1, 10), (0, 10), (1, 0), (1, 1 << 31)):
        assert lib.rails_scores_range_workspace_bytes(rows, n) == 0
    need = lib.rails_scores_range_workspace_bytes(3, 5000)
    assert need >= 3 * 4 * (8 + 4) + 4 and need % 256 == 0      # two chunks per row and the head's and the tail's slots: an int64 and an int32 each
    assert lib.rails_scores_range_workspace_bytes(3, 4096) == lib.rails_scores_range_workspace_bytes(3, 1)      # one chunk: three slots per row
    for call, args in ((lib.rails_scores_range_count, good), (lib.rails_scores_range_write, good_w)):
        a = list(args)
        a[1], a[2], a[3], a[10] = 5000, 3, 5000, need - 1
        assert call(*a, None) == nomem and "workspace" in _lib.last_error()
    assert lib.rails_scores_range_count(None, 10, 0, 10, None, 1.0, None, None, 0, None, 0, None, None, None) == ok      # rows = 0: nothing to do
    assert lib.rails_scores_range_write(None, 10, 0, 10, None, 1.0, None, None, 0, None, 0, None, 7, None) == ok
    assert lib.rails_scores_range_write(None, 10, 2, 10, None, 1.0, None, None, 0, None, 0, None, 0, None) == ok         # capacity = 0: no hits
    assert lib.rails_scores_range_write(*good_w[:12], -1, None) == bad and "capacity" in _lib.last_error()
    # rails_scores_range_sort(keys, lims, rows, max_count, stream)
    assert lib.rails_scores_range_sort(1, 1, 4, 16385, None) == notsup and "16384" in _lib.last_error()
    assert lib.rails_scores_range_sort(None, 1, 4, 16384, None) == bad and "NULL" in _lib.last_error()
    assert lib.rails_scores_range_sort(1, None, 4, 2, None) == bad and "NULL" in _lib.last_error()
    assert lib.rails_scores_range_sort(1, 1, -1, 2, None) == bad and lib.rails_scores_range_sort(1, 1, 4, -1, None) == bad
    for rows, most in ((0, 100), (4, 0), (4, 1)):      # nothing to sort
        assert lib.rails_scores_range_sort(None, None, rows, most, None) == ok
    # rails_scores_range_decode(keys, total, ids, n, scores_out, ids_out, stream)
    for args in ((None, 5, None, 10, 1, 1), (1, 5, None, 10, None, 1), (1, 5, None, 10, 1, None)):
        assert lib.rails_scores_range_decode(*args, None) == bad and "NULL" in _lib.last_error(), args
    assert lib.rails_scores_range_decode(1, -1, None, 10, 1, 1, None) == bad and lib.rails_scores_range_decode(1, 5, None, 0, 1, 1, None) == bad
    assert lib.rails_scores_range_decode(None, 0, None, 10, None, None, None) == ok      # total = 0: nothing to do


def test_range_kernels_use_no_scratch():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "range.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "scores_range"], capture_output=True, text=True, timeout=600).stdout
    rows = re.findall(r"scratch\s+(\d+) lds\s+(\d+)\s+(?:void )?mol::(\w+_kernel)", out)
    assert {r[2] for r in rows} == KERNELS and len(rows) == 7, out      # the masked and unmasked forms of count and write, offsets, sort, decode
    assert all(r[0] == "0" for r in rows), out


def test_engine_argument_checks():
    s = torch.zeros((2, 10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.scores_range_count(s, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.scores_range(s, 0.5)
    with pytest.raises(ValueError, match="ids must be"):
        E.scores_range(s, 0.5, ids=torch.zeros(9, dtype=torch.int64))
    with pytest.raises(ValueError, match="ids must be"):
        E.scores_range(s, 0.5, ids=torch.zeros(10, dtype=torch.int32))
    for wrong in (None, "1", True, [0.5, 0.5], 1j):
        with pytest.raises(ValueError, match="threshold"):
            E.range_thresholds("here", wrong, 2, "cpu")
    for wrong in (torch.zeros(3), torch.zeros((2, 1)), torch.zeros(2, dtype=torch.bool), torch.zeros(2, dtype=torch.complex64)):
        with pytest.raises(ValueError, match="threshold tensor"):
            E.range_thresholds("here", wrong, 2, "cpu")
    for t in (0.1, -0.0, float("inf"), float("-inf"), 3, 1e60):
        got = E.range_thresholds("here", t, 3, "cpu")
        assert got.dtype == torch.float32 and got.shape == (3,) and np.array_equal(got.numpy().view(np.uint32), G.thresholds(t, 3).view(np.uint32)), t
    assert bool(torch.isnan(E.range_thresholds("here", float("nan"), 2, "cpu")).all())
    got = E.range_thresholds("here", torch.tensor([0.1, 2.0], dtype=torch.float64), 2, "cpu")      # converted to fp32 once
    assert got.dtype == torch.float32 and float(got[0]) == float(np.float32(0.1))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _bare(cls):
    return cls.__new__(cls)      # (a refusal reads the type alone: nothing is constructed, nothing is launched)


def test_refusals_name_the_module():
    for cls in (rails_amd.MoLAvgTopK, rails_amd.MoLNaiveTopK, rails_amd.MoLCombTopK):
        for call in CALLS:
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call}: .*MoLBruteForceTopK"):
                getattr(_bare(cls), call)(None, 0.5)
    for cls in (rails_amd.MoLBruteForceTopK, rails_amd.MIPSBruteForceTopK):
        for call in CALLS:
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call} takes no collapse_groups"):
                getattr(_bare(cls), call)(None, 0.5, collapse_groups=True)
            for kw in ({}, {"min_score": 0.5, "min_log_prob": -3.0}):      # neither form, both forms: before anything of the module is read
                with pytest.raises(ValueError, match=rf"^{cls.__name__}\.{call}: exactly one of min_score= and min_log_prob="):
                    getattr(_bare(cls), call)(None, **kw)
            with pytest.raises(ValueError, match=rf"^{cls.__name__}\.{call}: temperature = 2.0 with min_score="):
                getattr(_bare(cls), call)(None, 0.5, temperature=2.0)
            for t in (0, float("nan"), "1"):
                with pytest.raises(ValueError, match="temperature"):
                    getattr(_bare(cls), call)(None, min_log_prob=-3.0, temperature=t)
    src = open(os.path.join(ROOT, "rails_amd", "sharded.py")).read()
    classes = [getattr(sharded, name) for name in re.findall(r"^class (\w+)\(", src, flags=re.M)]
    wrappers = [c for c in classes if issubclass(c, rails_amd.topk_modules.TopKModule)]
    assert len(wrappers) >= 6
    for cls in wrappers:
        for call in CALLS:
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call}: .*single-device MoLBruteForceTopK"):
                getattr(_bare(cls), call)(None, 0.5)


# ---- the reference against the selection reference ---------------------------------------------------------------------------------
def test_sorted_reference_is_a_prefix_of_the_exhaustive_ranking():
    rng = np.random.default_rng(62)
    for fam in ("gauss", "constant", "signed_zeros", "subnormals", "all_negative", "tie_at_kth"):
        n = 777
        bits = np.stack([R.FAMILIES[fam](n, 200, rng) for _ in range(3)])
        eligible = rng.random((3, n)) < 0.7
        t = np.array([bits[r].view(np.float32)[rng.integers(0, n)] for r in range(3)], dtype=np.float32)
        lims, s, p = G.ragged(bits, eligible, t)
        _, s_u, p_u = G.ragged(bits, eligible, t, sort=False)
        assert np.array_equal(np.diff(lims), G.counts(bits, eligible, t)) and lims[0] == 0
        for r in range(3):
            masked = np.where(eligible[r], bits[r], np.uint32(0xFF800000))      # what the masked strategies select from; no eligible -inf in these families
            want_s, want_p = R.select(masked, int(lims[r + 1] - lims[r]))
            assert np.array_equal(s[lims[r]:lims[r + 1]], want_s) and np.array_equal(p[lims[r]:lims[r + 1]], want_p), fam
            seg = p_u[lims[r]:lims[r + 1]]
            assert np.array_equal(seg, np.sort(p[lims[r]:lims[r + 1]])) and np.array_equal(s_u[lims[r]:lims[r + 1]], bits[r][seg])
    # with NaNs the hits are the ranking with the non-hits taken out: the sign-clear NaNs stand above +inf in the ranking and are no hits
    bits = R.nans(500, 100, rng)[None]
    lims, s, p = G.ragged(bits, True, -np.inf)
    full_s, full_p = R.select(bits[0], 500)
    keep = ~np.isnan(full_s.view(np.float32))
    assert lims[1] == keep.sum() < 500 and np.array_equal(p, full_p[keep]) and np.array_equal(s, full_s[keep])


def test_reference_special_thresholds():
    f = lambda *v: np.array([v], dtype=np.float32).view(np.uint32)      # noqa: E731
    inf, nan = np.inf, np.nan
    row = f(1.0, -inf, nan, inf, -0.0, 0.0, -1.0)
    assert G.counts(row, True, -inf)[0] == 6 and G.counts(row, True, inf)[0] == 1 and G.counts(row, True, nan)[0] == 0
    for zero in (0.0, -0.0):      # -0 >= +0 holds, and +0 >= -0
        assert G.hit_mask(row, True, zero)[0].tolist() == [True, False, False, True, True, True, False]
    lims, s, p = G.ragged(row, True, 0.0)
    assert p.tolist() == [3, 0, 5, 4] and lims.tolist() == [0, 4]      # +0 ranks above -0 on the bits
    assert G.ragged(row, True, 0.0, sort=False)[2].tolist() == [0, 3, 4, 5]
    assert G.hit_mask(row, np.array([[True, True, True, False, True, False, True]]), -0.0)[0].tolist() == [True, False, False, False, True, False, False]
    # the log-probability form: fl32(fl32(s * beta) - lse), special lse included
    one, half = np.float32(1.0), np.float32(0.5)
    assert G.values(f(3.0, 1.0), half, np.array([0.25], dtype=np.float32))[0].tolist() == [1.25, 0.25]
    assert G.counts(f(3.0, 1.0), True, 1.0, half, np.array([0.25], dtype=np.float32))[0] == 1
    assert G.counts(row, True, -inf, one, np.array([-inf], dtype=np.float32))[0] == 5      # -inf - (-inf) is NaN; the rest is +inf
    assert G.counts(row, True, -inf, one, np.array([nan], dtype=np.float32))[0] == 0
    assert G.counts(row, True, -inf, one, np.array([inf], dtype=np.float32))[0] == 5       # inf - inf is NaN; the rest is -inf >= -inf
    # one rounded multiply, then the subtraction: an fma would keep the product's low bits
    s, beta, lse = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12), np.float32(1.0)
    assert G.values(np.array([[s]]).view(np.uint32), beta, np.array([lse]))[0, 0] == np.float32(2.0 ** -11)
    assert np.float32(np.float64(s) * np.float64(beta) - 1.0) == np.float32(2.0 ** -11 + 2.0 ** -24)      # (what the fused form would give)


def test_cap_fixture_counts():
    for count in (E.RANGE_SORT_MAX, E.RANGE_SORT_MAX + 1):
        bits, t = cap_fixture(count)
        assert bits.shape == (1, CAP_N) and G.counts(bits, True, t)[0] == count
