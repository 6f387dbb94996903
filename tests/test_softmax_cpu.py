"""CPU: the softmax over the corpus without a device -- the reference Philox of tests/_softmax_ref.py against the published
known answers, the uniform variate exact in fp32, the entry points additions under ABI 15 that validate before any launch, the reference alone
under the statistical bar of the GPU test, the refusals by name."""
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
from tests import _softmax_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rails_scores_lse_workspace_bytes", "rails_scores_lse", "rails_scores_log_prob", "rails_scores_gumbel")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = {"scores_lse_max_kernel", "scores_lse_rowmax_kernel", "scores_lse_sum_kernel", "scores_lse_finish_kernel", "scores_log_prob_kernel",
           "scores_gumbel_kernel"}
CALLS = ("log_partition", "log_prob_of", "log_prob_of_positions", "sample_items")
FREQ_LOGITS = [0, .5, 1, 1.5, 2, -1, .25, 3]
FREQ_SEED = 0x1234567887654321
FREQ_ROWS = 4096
CHI2_BAR = 29.88      # the 1e-4 upper quantile of chi-square with 7 degrees of freedom


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_reference_philox_known_answers():
    """The known-answer vectors of the Random123 distribution (kat_vectors: philox4x32 10)."""
    assert _hex(S.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(S.philox4x32_10((ones,) * 4, (ones,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(S.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised: an array of counters gives what the counters give one by one
    x = np.array([0, 1, 0xFFFFFFFF], dtype=np.uint64)
    many = S.philox4x32_10((x, 7, 9, 0), (3, 4))[0]
    assert [int(v) for v in many] == [int(S.philox4x32_10((int(c), 7, 9, 0), (3, 4))[0]) for c in x]


def test_the_uniform_variate_is_exact_in_fp32():
    rng = np.random.default_rng(3)
    w23 = np.unique(np.concatenate([np.arange(0, 4096), np.arange((1 << 23) - 4096, 1 << 23), rng.integers(0, 1 << 23, size=100_000)])).astype(np.uint32)
    in32 = (w23.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)      # the kernel's expression, each step rounded to fp32
    assert in32.dtype == np.float32
    want = S.uniform(w23.astype(np.uint64) << np.uint64(9))
    assert np.array_equal(in32.astype(np.float64), want)
    assert want.min() == 2.0 ** -24 and want.max() == 1.0 - 2.0 ** -24
    assert np.isfinite(-np.log(-np.log(want))).all()


def test_entry_points_are_additions_under_abi_15(lib):
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert re.search(r"#define RAILS_ABI_VERSION 15\b", header) and _lib.RAILS_ABI_VERSION == 15 and lib.rails_abi_version() == 15
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    assert "softmax.hip" in open(os.path.join(ROOT, "rails_amd", "csrc", "Makefile")).read()
    for name in ("softmax.hip", "score_rows.h", "wave_ops.h"):      # the kernels, their row walk and their wave sum
        src = open(os.path.join(ROOT, "rails_amd", "csrc", name)).read()
        assert "atomicAdd" not in src and "__expf" not in src and "__logf" not in src, name      # no floating-point atomics, the accurate expf / log
    assert '#include "score_rows.h"' in open(os.path.join(ROOT, "rails_amd", "csrc", "softmax.hip")).read()
    assert list(inspect.signature(E.scores_lse).parameters) == ["scores", "mask", "temperature"]
    assert list(inspect.signature(E.scores_log_prob).parameters) == ["scores", "positions", "lse", "mask", "temperature"]
    assert list(inspect.signature(E.scores_gumbel).parameters) == ["scores", "seed", "first_row", "mask", "temperature", "out"]


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    bad, ok, nomem = _lib.RAILS_EINVAL, _lib.RAILS_OK, _lib.RAILS_ENOMEM
    big = 1 << 30
    # rails_scores_lse(scores, ld, rows, n, inv_temperature, mask_words, words_row_stride, workspace, workspace_bytes, lse_out, stream)
    for args in ((None, 10, 2, 10, 1.0, None, 0, 1, big, 1), (1, 10, 2, 10, 1.0, None, 0, None, big, 1), (1, 10, 2, 10, 1.0, None, 0, 1, big, None)):
        assert lib.rails_scores_lse(*args, None) == bad and "NULL" in _lib.last_error(), args
    assert lib.rails_scores_lse(1, 9, 2, 10, 1.0, None, 0, 1, big, 1, None) == bad and "ld" in _lib.last_error()
    for rows, n in ((-1, 10), (1, 0), (1, -3)):
        assert lib.rails_scores_lse(1, max(n, 0), rows, n, 1.0, None, 0, 1, big, 1, None) == bad, (rows, n)
        assert lib.rails_scores_log_prob(1, max(n, 0), rows, n, 1, 1, 1.0, 1, None, 0, 1, None) == bad, (rows, n)
        assert lib.rails_scores_gumbel(1, max(n, 0), rows, n, 1.0, 5, 0, None, 0, 1, max(n, 0), None) == bad, (rows, n)
        assert lib.rails_scores_lse_workspace_bytes(rows, n) == 0
    for beta in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.rails_scores_lse(1, 10, 2, 10, beta, None, 0, 1, big, 1, None) == bad and "inv_temperature" in _lib.last_error(), beta
        assert lib.rails_scores_log_prob(1, 10, 2, 10, 1, 1, beta, 1, None, 0, 1, None) == bad and "inv_temperature" in _lib.last_error(), beta
        assert lib.rails_scores_gumbel(1, 10, 2, 10, beta, 5, 0, None, 0, 1, 10, None) == bad and "inv_temperature" in _lib.last_error(), beta
    for stride in (1, 3, -1):      # 100 bits need 4 words; 0 is the shared row
        assert lib.rails_scores_lse(1, 100, 2, 100, 1.0, 1, stride, 1, big, 1, None) == bad and "shorter" in _lib.last_error(), stride
    need = lib.rails_scores_lse_workspace_bytes(3, 5000)
    assert need >= 3 * 2 * 8 + 3 * 2 * 4 + 3 * 4 and need % 256 == 0      # two chunks per row: a float64 and an fp32 partial each, an fp32 per row
    assert lib.rails_scores_lse(1, 5000, 3, 5000, 1.0, None, 0, 1, need - 1, 1, None) == nomem and "workspace" in _lib.last_error()
    assert lib.rails_scores_lse(None, 10, 0, 10, 1.0, None, 0, None, 0, None, None) == ok      # rows = 0: nothing to do
    # rails_scores_log_prob(scores, ld, rows, n, positions, t, inv_temperature, lse, mask_words, words_row_stride, out, stream)
    for args in ((None, 10, 2, 10, 1, 3, 1.0, 1, None, 0, 1), (1, 10, 2, 10, None, 3, 1.0, 1, None, 0, 1), (1, 10, 2, 10, 1, 3, 1.0, None, None, 0, 1),
                 (1, 10, 2, 10, 1, 3, 1.0, 1, None, 0, None)):
        assert lib.rails_scores_log_prob(*args, None) == bad and "NULL" in _lib.last_error(), args
    assert lib.rails_scores_log_prob(1, 9, 2, 10, 1, 3, 1.0, 1, None, 0, 1, None) == bad and "ld" in _lib.last_error()
    for t in (0, -1):
        assert lib.rails_scores_log_prob(1, 10, 2, 10, 1, t, 1.0, 1, None, 0, 1, None) == bad and "t =" in _lib.last_error(), t
    assert lib.rails_scores_log_prob(None, 10, 0, 10, None, 3, 1.0, None, None, 0, None, None) == ok
    # rails_scores_gumbel(scores, ld, rows, n, inv_temperature, seed, first_row, mask_words, words_row_stride, out, out_ld, stream)
    for args in ((None, 10, 2, 10, 1.0, 5, 0, None, 0, 1, 10), (1, 10, 2, 10, 1.0, 5, 0, None, 0, None, 10)):
        assert lib.rails_scores_gumbel(*args, None) == bad and "NULL" in _lib.last_error(), args
    assert lib.rails_scores_gumbel(1, 9, 2, 10, 1.0, 5, 0, None, 0, 1, 10, None) == bad and "ld" in _lib.last_error()
    assert lib.rails_scores_gumbel(1, 10, 2, 10, 1.0, 5, 0, None, 0, 1, 9, None) == bad and "out_ld" in _lib.last_error()
    assert lib.rails_scores_gumbel(1, 10, 2, 10, 1.0, 5, -1, None, 0, 1, 10, None) == bad and "first_row" in _lib.last_error()
    assert lib.rails_scores_gumbel(None, 10, 0, 10, 1.0, (1 << 64) - 1, 0, None, 0, None, 10, None) == ok


def test_softmax_kernels_use_no_scratch():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "softmax.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "scores_lse|scores_log_prob|scores_gumbel"], capture_output=True, text=True,
                         timeout=600).stdout
    rows = re.findall(r"scratch\s+(\d+) lds\s+(\d+)\s+(?:void )?mol::(\w+_kernel)", out)
    assert {r[2] for r in rows} == KERNELS and len(rows) == 10, out      # the masked and unmasked forms of four kernels, rowmax, finish
    assert all(r[0] == "0" for r in rows), out


def test_engine_argument_checks():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.scores_lse(torch.zeros((2, 10)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.scores_log_prob(torch.zeros((2, 10)), torch.zeros((2, 1), dtype=torch.int64), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.scores_gumbel(torch.zeros((2, 10)), 5)
    for t in (0, 0.0, -1.0, float("inf"), float("nan"), None, "1", True, 1e-60, 1e60):
        with pytest.raises(ValueError, match="temperature"):
            E.inv_temperature(t)
    for t in (1.0, 0.5, 7.3, 2):
        assert E.inv_temperature(t) == float(np.float32(1.0 / t))


def test_the_reference_alone_meets_the_statistical_bar():
    """The bar of the GPU frequency test on the float64 reference with the test's seed: what the kernel is held to is not an accident of the
    seed.  4 096 draws over 8 items; Pearson's statistic against softmax(logits / T)."""
    for temperature, figure in ((1.0, 5.70), (2.0, 4.94)):
        chi2, smallest, arg, gap = S.chi_square(FREQ_LOGITS, temperature, FREQ_SEED, FREQ_ROWS)
        assert abs(chi2 - figure) <= 0.01, (temperature, chi2)
        assert chi2 < CHI2_BAR and smallest >= 38, (temperature, chi2, smallest)
        assert arg.shape == (FREQ_ROWS,) and (gap >= 0).all()


def test_reference_lse_special_rows():
    f = lambda *v: np.array([v], dtype=np.float32).view(np.uint32)      # noqa: E731
    inf, nan = np.inf, np.nan
    one = np.float32(1.0)
    assert S.lse(f(1.0, 2.0), np.array([[False, False]]), one)[0] == -inf
    assert S.lse(f(-inf, -inf, 5.0), np.array([[True, True, False]]), one)[0] == -inf
    assert np.isnan(S.lse(f(1.0, nan, inf), True, one)[0]) and S.lse(f(1.0, nan, inf), np.array([[True, False, True]]), one)[0] == inf
    assert S.lse(f(-inf, 3.5, nan), np.array([[True, True, False]]), np.float32(0.5))[0] == 1.75
    assert abs(S.lse(f(0.0, 0.0), True, one)[0] - np.log(2.0)) < 1e-15


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _bare(cls):
    return cls.__new__(cls)      # (a refusal reads the type alone: nothing is constructed, nothing is launched)


def test_refusals_name_the_module():
    for cls in (rails_amd.MoLAvgTopK, rails_amd.MoLNaiveTopK, rails_amd.MoLCombTopK):
        for call in CALLS:
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call}: .*MoLBruteForceTopK"):
                getattr(_bare(cls), call)(None, None, None) if call == "sample_items" else getattr(_bare(cls), call)(None, None)
    for cls in (rails_amd.MoLBruteForceTopK, rails_amd.MIPSBruteForceTopK):
        for call in CALLS:
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call} takes no collapse_groups"):
                getattr(_bare(cls), call)(None, None, 5, collapse_groups=True) if call == "sample_items" else getattr(_bare(cls), call)(None, None, collapse_groups=True)
    src = open(os.path.join(ROOT, "rails_amd", "sharded.py")).read()
    classes = [getattr(sharded, name) for name in re.findall(r"^class (\w+)\(", src, flags=re.M)]
    wrappers = [c for c in classes if issubclass(c, rails_amd.topk_modules.TopKModule)]
    assert len(wrappers) >= 6
    for cls in wrappers:
        for call in CALLS:
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call}: .*single-device MoLBruteForceTopK"):
                getattr(_bare(cls), call)(None, None, None) if call == "sample_items" else getattr(_bare(cls), call)(None, None)


def test_harness_refuses_a_module_without_log_prob_of():
    class NoSoftmax:
        def rank_of(self, *a, **k):
            raise AssertionError("not reached")

    state = H.EvalState(all_item_ids=set(), candidate_index=None, top_k_module=NoSoftmax())
    for exact in (False, True):
        with pytest.raises(NotImplementedError, match="NoSoftmax has no log_prob_of"):
            H.eval_metrics_v2_from_tensors(state, None, None, torch.zeros((2, 1), dtype=torch.int64), exact_ranks=exact, nll=True)
    assert inspect.signature(H.eval_metrics_v2_from_tensors).parameters["nll"].default is False
    assert "dense pass" in H.eval_metrics_v2_from_tensors.__doc__
