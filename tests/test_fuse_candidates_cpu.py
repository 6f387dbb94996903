"""CPU: query fusion over the candidate union without a device -- rails_lists_union is an addition under ABI 15 and
validates before any launch, its kernel uses no scratch, the switch fuse_candidates defaults to off and leaves every refusal where it was,
tests/_fuse_candidates_ref.py agrees with tests/_fuse_ref.py."""
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
from tests import _fuse_candidates_ref as R
from tests import _fuse_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
CLASSES = (rails_amd.MoLAvgTopK, rails_amd.MoLNaiveTopK, rails_amd.MoLCombTopK)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_entry_point_is_an_addition_under_abi_15(lib):
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert re.search(r"#define RAILS_ABI_VERSION 15\b", header) and _lib.RAILS_ABI_VERSION == 15 and lib.rails_abi_version() == 15
    assert re.search(r"\brails_lists_union\s*\(", header) and "rails_lists_union" in _lib.PROTOTYPES and lib.rails_lists_union is not None
    src = open(os.path.join(ROOT, "rails_amd", "csrc", "fuse.hip")).read()
    assert "lists_union_kernel" in src and src.count("lds_sort_desc(") == 3      # the list merge's two sorts and this one: no second implementation
    assert "atomic" not in src.lower().replace("no atomics", "")
    assert list(inspect.signature(E.lists_union).parameters) == ["positions", "lims", "n_items", "out"]


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (A small integer stands for a non-NULL pointer; nothing
    dereferences it.)"""
    bad, ok, unsup = _lib.RAILS_EINVAL, _lib.RAILS_OK, _lib.RAILS_ENOTSUP
    # rails_lists_union(positions, ld, rows_in, width, lims, n_out, max_segment, n_items, out, w_out, counts, stream)
    fine = [1, 8, 6, 8, 1, 2, 3, 100, 1, 24, None]
    for at in (0, 4, 8):
        args = list(fine)
        args[at] = None
        assert lib.rails_lists_union(*args, None) == bad and "NULL" in _lib.last_error(), at
    for at, value in ((1, 7), (2, -1), (3, 0), (5, -1), (6, 0), (7, -1), (9, 0), (9, 23)):
        args = list(fine)
        args[at] = value
        assert lib.rails_lists_union(*args, None) == bad and "bad size" in _lib.last_error(), (at, value)
    args = list(fine)
    args[7] = 1 << 32
    assert lib.rails_lists_union(*args, None) == unsup and "positions" in _lib.last_error() and str(1 << 32) in _lib.last_error()
    args = list(fine)
    args[1], args[3], args[6], args[9] = 16385, 16385, 1, 16385      # one row of 16 385 entries
    assert lib.rails_lists_union(*args, None) == unsup and "16385" in _lib.last_error() and "16384" in _lib.last_error()
    args = list(fine)
    args[1], args[3], args[6], args[9] = 4097, 4097, 4, 16388      # 4 x 4 097 = 16 388
    assert lib.rails_lists_union(*args, None) == unsup and "16388" in _lib.last_error()
    args = list(fine)
    args[5] = 0      # nothing to do: returns before 16 384 entries would be launched
    args[1], args[3], args[6], args[9] = 16384, 16384, 1, 16384
    assert lib.rails_lists_union(*args, None) == ok
    assert E.FUSE_LIST_MAX_ENTRIES == 16384


def test_union_kernel_uses_no_scratch():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "fuse.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "lists_union"], capture_output=True, text=True, timeout=600).stdout
    rows = re.findall(r"scratch\s+(\d+) lds\s+(\d+)\s+(?:void )?mol::(\w+_kernel)", out)
    assert [r[2] for r in rows] == ["lists_union_kernel"], out
    assert rows[0][0] == "0", out


# ---- the switch ----------------------------------------------------------------------------------------------------------------------------------
def _bare(cls, **state):
    tk = cls.__new__(cls)      # (checks that read the type and the arguments alone: nothing is constructed, nothing is launched)
    tk.__dict__.update(state)
    return tk


def test_the_switch_defaults_to_off_and_the_refusals_stay():
    lims = torch.tensor([0, 2])
    for cls in CLASSES:
        assert cls.fuse_candidates is False and _bare(cls).fuse_candidates is False
        for call, args in (("forward", (None, 5)), ("forward_filtered", (None, 7, None, 5)), ("all_logits", (None,))):
            for kw in ({"query_lims": lims}, {"fuse": "sum"}, {"query_weights": torch.ones(2)}):
                with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}(\.\w+)? takes no {next(iter(kw))}: .*MoLBruteForceTopK.*fuse_candidates = True"):
                    getattr(_bare(cls), call)(*args, **kw)


def test_calls_that_refuse_with_the_switch_on():
    lims = torch.tensor([0, 2])
    for cls in CLASSES:
        tk = _bare(cls)
        tk.fuse_candidates = True
        assert tk.fuse_candidates is True and cls.fuse_candidates is False
        with pytest.raises(NotImplementedError, match=rf"^{cls.__name__} takes no query_lims"):
            tk.all_logits(None, query_lims=lims)
        for call in ("rank_of", "log_partition", "count_above", "range_search", "sample_items"):
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call}: .*MoLBruteForceTopK"):
                getattr(tk, call)(None, None, **({"seed": 1} if call == "sample_items" else {}), query_lims=lims)
    for cls in (rails_amd.MoLAvgTopK, rails_amd.MoLCombTopK):
        tk = _bare(cls, fuse_candidates=True)
        with pytest.raises(NotImplementedError, match=rf"^{cls.__name__} takes no query_lims"):
            tk.submit(None, 5, query_lims=lims)
        for call in ("topk_ids", "coarse_candidates"):
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call} takes no query_lims"):
                getattr(tk, call)(None, query_lims=lims)
    for cls in (rails_amd.MoLNaiveTopK, rails_amd.MoLCombTopK):
        with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.local_candidates takes no fuse"):
            _bare(cls, fuse_candidates=True).local_candidates(None, fuse="sum")
    # the IVF module: the switch cannot be set, and a call that was opted in some other way names the IVF module
    ivf = _bare(rails_amd.MoLNaiveTopK, _use_faiss=True)
    with pytest.raises(NotImplementedError, match=r"^MoLNaiveTopK \(IVF, use_faiss=True\) takes no fuse_candidates"):
        ivf.fuse_candidates = True
    assert ivf.fuse_candidates is False
    ivf.__dict__["fuse_candidates"] = True
    for call, args in (("forward", (None, 5)), ("forward_filtered", (None, 7, None, 5))):
        with pytest.raises(NotImplementedError, match=r"^MoLNaiveTopK \(IVF, use_faiss=True\)\.\w+ takes no query_lims"):
            getattr(ivf, call)(*args, query_lims=lims)


def test_fused_calls_check_their_arguments_before_any_launch():
    """On bare instances with the switch on: what _resolve_fusion says, the combinations that are not built, the entry limit with both numbers."""

    class Rows:
        def size(self, dim):
            return 11

    lims = torch.tensor([0, 1, 3, 6, 11])
    for cls in CLASSES:
        state = dict(fuse_candidates=True, _ids_flat=torch.zeros(4, dtype=torch.int64), _avg_top_k=4000, _k_per_group=70)
        with pytest.raises(ValueError, match=rf"^{cls.__name__}\.forward: fuse= without query_lims="):
            _bare(cls, **state).forward(Rows(), 5, fuse="sum")
        with pytest.raises(ValueError, match=r"fuse must be one of \['max', 'sum'\], got 'mean'"):
            _bare(cls, **state).forward(Rows(), 5, query_lims=lims, fuse="mean")
        with pytest.raises(ValueError, match=r'query_weights= goes with fuse="sum"'):
            _bare(cls, **state).forward(Rows(), 5, query_lims=lims, query_weights=torch.ones(11))
        with pytest.raises(ValueError, match=r"query_lims\[U\] = 10 but there are 11 sub-query rows"):
            _bare(cls, **state).forward_filtered(Rows(), 7, None, 5, query_lims=torch.tensor([0, 10]))
        for extra in ({"collapse_groups": True}, {"max_per_group": 2}, {"diversify": 0.5}, {"item_mask": torch.ones(4, dtype=torch.bool)}):
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}(\.forward)?: .*together with query_lims="):
                _bare(cls, **state).forward(Rows(), 5, query_lims=lims, **extra)
    with pytest.raises(ValueError, match=r"avg_top_k \(100\) must be larger than k \(101\)"):
        _bare(rails_amd.MoLAvgTopK, fuse_candidates=True, _ids_flat=torch.zeros(4, dtype=torch.int64), _avg_top_k=100).forward(Rows(), 101, query_lims=lims)
    # 5 rows x 4 000 coarse candidates = 20 000 entries
    with pytest.raises(NotImplementedError, match=r"^MoLAvgTopK\.forward: a fused row of 5 sub-query rows x 4000 candidates holds 20000 candidate entries, beyond the 16384"):
        tk = _bare(rails_amd.MoLAvgTopK, fuse_candidates=True, _ids_flat=torch.zeros(4, dtype=torch.int64), _avg_top_k=4000)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(rails_amd.MoLAvgTopK, "num_items", property(lambda self: 100_000))
            tk.forward(Rows(), 5, query_lims=lims)


# ---- the reference against tests/_fuse_ref.py --------------------------------------------------------------------------------------------------
def _case(rng, lims, n, width):
    S = int(lims[-1])
    scores = rng.standard_normal((S, n)).astype(np.float32).round(1)      # (rounded: ties occur)
    cand = np.stack([rng.integers(-1, n + 2, size=width) for _ in range(S)])      # duplicates, -1 and positions >= n among them
    return scores, cand


def _gathered(scores, union_pos, lims):
    rows = np.repeat(np.arange(lims.size - 1), np.diff(lims))
    return np.take_along_axis(scores, np.clip(union_pos[rows], 0, scores.shape[1] - 1), axis=1)


def test_reference_union():
    out, counts = R.union(np.array([[5, 3, 5, -1], [9, 3, 10, 0], [7, 7, 7, 7]]), [0, 2, 3], 10)
    assert out.tolist() == [[0, 3, 5, 9, -1, -1, -1, -1], [7, -1, -1, -1, -1, -1, -1, -1]] and counts.tolist() == [4, 1] and counts.dtype == np.int32
    out, counts = R.union(np.array([[2, 1]]), [0, 1], 10, w_out=5)
    assert out.tolist() == [[1, 2, -1, -1, -1]] and counts.tolist() == [2]


def test_reference_segments_of_one_row_reproduce_the_plain_walk():
    rng = np.random.default_rng(11)
    n, S = 60, 6
    lims = np.arange(S + 1)
    ids = np.arange(n, dtype=np.int64) * 3 + 1
    scores, cand = _case(rng, lims, n, 17)
    union_pos, counts = R.union(cand, lims, n)
    seen = ids[rng.integers(0, n, size=(S, 9))]
    member = np.zeros((S, n), dtype=bool)
    for r in range(S):
        member[r, union_pos[r, : counts[r]]] = True
    for mode in ("max", "sum"):
        for inv in (None, seen):
            got = R.walk(union_pos, counts, _gathered(scores, union_pos, lims), lims, mode, None, ids, 8, inv)
            want = F.topk_walk(scores, member, ids, 8, inv)      # the plain walk of every row over its own candidates
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (mode, inv is None)


def test_reference_walk_equals_the_matrix_walk_outside_the_union():
    """The union walk is F.topk_walk on the fused (U, n) matrix restricted to C_u: fusing the union's columns is fusing every column."""
    rng = np.random.default_rng(12)
    n = 80
    lims = np.array([0, 1, 3, 6, 11])
    ids = np.arange(n, dtype=np.int64) * 3 + 1
    scores, cand = _case(rng, lims, n, 9)
    weights = rng.standard_normal(11).astype(np.float32)
    union_pos, counts = R.union(cand, lims, n)
    member = np.zeros((4, n), dtype=bool)
    for u in range(4):
        member[u, union_pos[u, : counts[u]]] = True
    seen = ids[rng.integers(0, n, size=(4, 12))]
    for mode, w in (("max", None), ("sum", None), ("sum", weights)):
        fused = F.fuse(scores, lims, mode, w)
        for k in (5, 40):      # 40: more than some unions hold -- the (-1, -inf) padding
            for inv in (None, seen):
                got = R.walk(union_pos, counts, _gathered(scores, union_pos, lims), lims, mode, w, ids, k, inv)
                want = F.topk_walk(np.where(member, fused, -np.inf).astype(np.float32), member, ids, k, inv)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (mode, k, inv is None)
    assert (R.walk(union_pos, counts, _gathered(scores, union_pos, lims), lims, "max", None, ids, 40)[0][:, -1] == -1).all()
