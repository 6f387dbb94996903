"""CPU: query fusion without a device -- the two entry points are additions under ABI 15 and validate before any launch,
query_lims is checked on the host with messages that say what is wrong, tests/_fuse_ref.py agrees with itself, the new kernels use no scratch,
the refusals name their module."""
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
from rails_amd import topk_modules as T
from tests import _fuse_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NAMES = ("rails_scores_fuse_rows", "rails_topk_fuse_lists")
SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC0FFEE, 0xFFFFFFFF, 0x00000001, 0x80000001, 0x007FFFFF,
                     0x3F800000, 0xBF800000], dtype=np.uint32)      # +-0, +-inf, NaNs of both signs, subnormals, +-1


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
    assert re.search(r"#define RAILS_FUSE_MAX 0\b", header) and re.search(r"#define RAILS_FUSE_SUM 1\b", header)
    assert (_lib.RAILS_FUSE_MAX, _lib.RAILS_FUSE_SUM) == (0, 1) and E.FUSE_MODES == {"max": 0, "sum": 1}
    assert "fuse.hip" in open(os.path.join(ROOT, "rails_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "rails_amd", "csrc", "fuse.hip")).read()
    assert '#include "topk_keys.h"' in src and "orderable(float" not in src and "make_key(float" not in src      # one codec: the header's
    assert "atomic" not in src.lower().replace("no atomics", "")
    assert E.FUSE_LIST_MAX_ENTRIES == 16384 and rails_amd.MoLBruteForceTopK.FUSE_LIST_MAX_ENTRIES == rails_amd.MIPSBruteForceTopK.FUSE_LIST_MAX_ENTRIES == 16384
    assert list(inspect.signature(E.scores_fuse_rows).parameters) == ["scores", "lims", "mode", "weights", "out", "run_if"]
    assert list(inspect.signature(E.topk_fuse_lists).parameters)[:6] == ["scores", "positions", "lims", "k", "ids", "invalid_ids"]


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (A small integer stands for a non-NULL pointer; nothing
    dereferences it.)"""
    bad, ok, unsup = _lib.RAILS_EINVAL, _lib.RAILS_OK, _lib.RAILS_ENOTSUP
    # rails_scores_fuse_rows(scores, ld, rows_in, n, lims, n_out, mode, weights, out, ld_out, run_if, stream)
    fine = [1 << 20, 10, 4, 10, 64, 2, 0, None, 1 << 30, 10, None]
    for at in (0, 4, 8):
        args = list(fine)
        args[at] = None
        assert lib.rails_scores_fuse_rows(*args, None) == bad and "NULL" in _lib.last_error(), at
    for at, value in ((1, 9), (9, 9), (3, 0), (3, 1 << 31), (2, -1), (5, -1), (2, (1 << 24) + 1)):
        args = list(fine)
        args[at] = value
        assert lib.rails_scores_fuse_rows(*args, None) == bad and "bad size" in _lib.last_error(), (at, value)
    args = list(fine)
    args[6] = 2
    assert lib.rails_scores_fuse_rows(*args, None) == bad and "mode" in _lib.last_error()
    args = list(fine)
    args[7] = 1 << 10      # weights with max
    assert lib.rails_scores_fuse_rows(*args, None) == bad and "weights" in _lib.last_error()
    for out in (1 << 20, (1 << 20) + 4 * 39, (1 << 20) - 4 * 19):      # out inside, at the last element of, and reaching into scores
        args = list(fine)
        args[8] = out
        assert lib.rails_scores_fuse_rows(*args, None) == bad and "overlaps" in _lib.last_error(), out
    args = list(fine)
    args[5] = 0
    assert lib.rails_scores_fuse_rows(*args, None) == ok
    # rails_topk_fuse_lists(scores, ld, positions, rows_in, depth, lims, n_out, max_segment, n_items, ids, invalid, width, k, out_ids, out_scores, stream)
    fine = [1, 8, 1, 6, 8, 1, 2, 3, 100, None, None, 0, 4, 1, 1]
    for at in (0, 2, 5, 13, 14):
        args = list(fine)
        args[at] = None
        assert lib.rails_topk_fuse_lists(*args, None) == bad and "NULL" in _lib.last_error(), at
    args = list(fine)
    args[11] = 3      # a width without seen ids
    assert lib.rails_topk_fuse_lists(*args, None) == bad and "NULL" in _lib.last_error()
    for at, value in ((1, 7), (4, 0), (7, 0), (3, -1), (6, -1), (8, -1), (11, -1), (12, -1)):
        args = list(fine)
        args[at] = value
        assert lib.rails_topk_fuse_lists(*args, None) == bad and "bad size" in _lib.last_error(), (at, value)
    for at, value, word in ((7, 2049, "entries"), (12, 513, "k ="), (8, 1 << 32, "positions")):
        args = list(fine)
        args[at] = value
        assert lib.rails_topk_fuse_lists(*args, None) == unsup and word in _lib.last_error(), (at, value)
    args = list(fine)
    args[10], args[11] = 1, 4097
    assert lib.rails_topk_fuse_lists(*args, None) == unsup and "seen ids" in _lib.last_error()
    args = list(fine)
    args[4], args[7], args[1] = 16385, 1, 16385      # m * k' = 16 385
    assert lib.rails_topk_fuse_lists(*args, None) == unsup and "16385 entries" in _lib.last_error()
    args = list(fine)
    args[6] = 0
    assert lib.rails_topk_fuse_lists(*args, None) == ok


def test_query_lims_messages():
    ok = E.parse_query_lims(torch.tensor([0, 1, 3, 6, 11]), 11)
    assert ok.dtype == torch.int64 and ok.device.type == "cpu" and ok.tolist() == [0, 1, 3, 6, 11]
    for lims, rows, message in (
        (torch.tensor([1, 3, 11]), 11, r"query_lims\[0\] must be 0, got 1"),
        (torch.tensor([0, 3, 10]), 11, r"query_lims\[U\] = 10 but there are 11 sub-query rows"),
        (torch.tensor([0, 3, 3, 11]), 11, r"increase strictly: segment 1 = \[3, 3\) is empty"),
        (torch.tensor([0, 5, 3, 11]), 11, r"increase strictly: segment 1 = \[5, 3\) is empty"),
        (torch.tensor([0]), 0, r"\(U \+ 1,\) int64 tensor with U >= 1"),
        (torch.tensor([0, 11], dtype=torch.int32), 11, r"\(U \+ 1,\) int64"),
        (torch.tensor([[0, 11]]), 11, r"\(U \+ 1,\) int64"),
        ([0, 11], 11, r"\(U \+ 1,\) int64"),
    ):
        with pytest.raises(ValueError, match=message):
            E.parse_query_lims(lims, rows, "here")
    ql = E.QueryLims(torch.tensor([0, 1, 3, 6, 11]), 11, "cpu")
    assert (ql.fused, ql.rows, ql.max_segment) == (4, 11, 5) and ql.fused_row_of().tolist() == [0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3]
    part = ql.rows_slice(1, 3)
    assert part.host.tolist() == [0, 2, 5] and (part.fused, part.rows, part.max_segment) == (2, 5, 3) and ql.rows_slice(0, 4) is ql


def _bare(cls):
    return cls.__new__(cls)      # (a check that reads the type and the arguments alone: nothing is constructed, nothing is launched)


class _Rows:
    def __init__(self, rows):
        self.rows = rows

    def size(self, dim):
        return self.rows


def test_call_argument_messages():
    for cls in (rails_amd.MoLBruteForceTopK, rails_amd.MIPSBruteForceTopK):
        tk, name = _bare(cls), cls.__name__
        tk.__dict__["_ids_flat"] = torch.zeros(4, dtype=torch.int64)
        q = _Rows(11)
        assert tk._resolve_fusion({"user_ids": 1}, q, "forward") is None
        with pytest.raises(ValueError, match=rf"^{name}\.forward: fuse= without query_lims="):
            tk._resolve_fusion({"fuse": "sum"}, q, "forward")
        with pytest.raises(ValueError, match=rf"^{name}\.rank_of: query_weights= without query_lims="):
            tk._resolve_fusion({"query_weights": torch.ones(11)}, q, "rank_of")
        lims = torch.tensor([0, 1, 3, 6, 11])
        with pytest.raises(ValueError, match=r"fuse must be one of \['max', 'sum'\], got 'mean'"):
            tk._resolve_fusion({"query_lims": lims, "fuse": "mean"}, q, "forward")
        for fuse in ({}, {"fuse": "max"}):
            with pytest.raises(ValueError, match=r'query_weights= goes with fuse="sum"'):
                tk._resolve_fusion({"query_lims": lims, "query_weights": torch.ones(11), **fuse}, q, "forward")
        for w in (torch.ones(4), torch.ones(11, dtype=torch.float64), [1.0] * 11):
            with pytest.raises(ValueError, match=r"query_weights must be \(11,\) fp32"):
                tk._resolve_fusion({"query_lims": lims, "fuse": "sum", "query_weights": w}, q, "forward")
        with pytest.raises(ValueError, match=rf"^{name}\.forward: query_lims\[U\] = 11 but there are 12 sub-query rows"):
            tk._resolve_fusion({"query_lims": lims}, _Rows(12), "forward")
        for extra in ({"collapse_groups": True}, {"max_per_group": 2}):
            with pytest.raises(NotImplementedError, match=rf"^{name}\.forward: collapse_groups= / max_per_group= together with query_lims="):
                tk._resolve_fusion({"query_lims": lims, **extra}, q, "forward")
            with pytest.raises(NotImplementedError, match=rf"^{name}: \w+= together with query_lims="):
                tk._take_collapse({"query_lims": lims, **extra})
        kwargs = {"query_lims": lims, "fuse": "sum", "query_weights": torch.ones(11), "user_ids": 5}
        fusion = tk._resolve_fusion(kwargs, q, "forward")
        assert sorted(kwargs) == ["_fusion", "user_ids"] and kwargs["_fusion"] is fusion and tk._resolve_fusion(kwargs, q, "again") is fusion
        assert (fusion.mode, fusion.lims.fused, fusion.lims.max_segment) == ("sum", 4, 5) and tk._result_rows(q, kwargs) == 4 and tk._result_rows(q, {}) == 11
        assert tk._resolve_fusion({"query_lims": lims}, q, "forward").mode == "max"      # the default
        s0, s1, part = fusion.rows_slice(2, 4)
        assert (s0, s1) == (3, 11) and part.lims.host.tolist() == [0, 3, 8] and part.weights.shape == (8,)


def test_slices_hold_whole_segments():
    plan = T._StreamingScores._slice_plan
    assert plan(10, 4, None) == [(0, 4), (4, 8), (8, 10)] and plan(3, 100, None) == [(0, 3)]
    fusion = T.Fusion(E.QueryLims(torch.tensor([0, 1, 3, 6, 11]), 11, "cpu"), "max", None)
    assert plan(4, 15, fusion) == [(0, 4)]                       # 11 sub-query rows + 4 fused rows
    assert plan(4, 14, fusion) == [(0, 3), (3, 4)]
    assert plan(4, 6, fusion) == [(0, 2), (2, 3), (3, 4)]       # (1 + 1) + (2 + 1), then 3 + 1, then 5 + 1
    assert plan(4, 17, fusion, 2) == [(0, 3), (3, 4)] and plan(4, 19, fusion, 2) == [(0, 4)]      # sample_items: two rows per fused row
    for cls in (rails_amd.MoLBruteForceTopK, rails_amd.MIPSBruteForceTopK):
        tk = _bare(cls)
        tk.__dict__["MAX_LOGIT_BYTES"] = 6 * 100 * 4
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(cls, "num_items", property(lambda self: 100))
            assert tk._fused_budget("X.rank_of", fusion, 1, "why") == 6
            with pytest.raises(NotImplementedError, match=r"^X\.sample_items: a segment of 5 sub-query rows and its fused rows of 100 logits exceed MAX_LOGIT_BYTES"):
                tk._fused_budget("X.sample_items", fusion, 2, "why")


def test_fuse_kernels_use_no_scratch():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "fuse.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "scores_fuse_rows|topk_fuse_lists"], capture_output=True, text=True,
                         timeout=600).stdout
    rows = re.findall(r"scratch\s+(\d+) lds\s+(\d+)\s+(?:void )?mol::(\w+_kernel)", out)
    assert {r[2] for r in rows} == {"scores_fuse_rows_kernel", "topk_fuse_lists_kernel"}, out
    assert sum(r[2] == "scores_fuse_rows_kernel" for r in rows) == 6, out      # three modes, with 16-byte accesses and without
    assert all(r[0] == "0" for r in rows), out
    assert all(r[1] == "0" for r in rows if r[2] == "scores_fuse_rows_kernel"), out      # no LDS in the matrix kernel


# ---- the reference against itself -------------------------------------------------------------------------------------------------------
def _matrix(rng, rows, n):
    bits = rng.standard_normal((rows, n)).astype(np.float32).view(np.uint32).copy()
    where = rng.random((rows, n)) < 0.3
    bits[where] = rng.choice(SPECIALS, size=int(where.sum()))
    return bits.view(np.float32)


def test_reference_size_one_identity_and_order():
    rng = np.random.default_rng(3)
    for n in (1, 3, 64, 257):
        s = _matrix(rng, 7, n)
        ones = np.arange(8)
        for mode in ("max", "sum"):
            assert np.array_equal(F.fuse(s, ones, mode).view(np.uint32), s.view(np.uint32)), (n, mode)      # bits, NaN payloads included
        lims = np.array([0, 1, 3, 7])
        got = F.fuse(s, lims, "max").view(np.uint32)
        for u in range(3):
            seg = s[lims[u] : lims[u + 1]].view(np.uint32)
            for x in range(n):      # the explicit rule on Python integers
                want = max(seg[:, x].tolist(), key=lambda b: (~b) & 0xFFFFFFFF if b & 0x80000000 else b | 0x80000000)
                assert int(got[u, x]) == want, (n, u, x)
    # -0 < +0; a positive NaN above +inf; a negative NaN below -inf
    col = np.array([[0x80000000], [0x00000000]], dtype=np.uint32).view(np.float32)
    assert F.fuse(col, [0, 2], "max").view(np.uint32).tolist() == [[0x00000000]]
    col = np.array([[0x7F800000], [0x7FC00000], [0xFFC00000]], dtype=np.uint32).view(np.float32)
    assert F.fuse(col, [0, 3], "max").view(np.uint32).tolist() == [[0x7FC00000]]
    col = np.array([[0xFF800000], [0xFFC00000]], dtype=np.uint32).view(np.float32)
    assert F.fuse(col, [0, 2], "max").view(np.uint32).tolist() == [[0xFF800000]]
    # the sum is a float32 chain in row order: (1e8 + 1) - 1e8 = 0 in float32, 1e8 - 1e8 + 1 = 1
    col = np.array([[1e8], [1.0], [-1e8]], dtype=np.float32)
    assert F.fuse(col, [0, 3], "sum").tolist() == [[0.0]] and F.fuse(col[[0, 2, 1]], [0, 3], "sum").tolist() == [[1.0]]
    w = np.array([3.0, 1.0, 3.0], dtype=np.float32)
    third = np.float32(1.0) / np.float32(3.0)
    col = np.array([[third], [-1.0], [third]], dtype=np.float32)
    want = np.float32(np.float32(np.float32(w[0] * third) + np.float32(-1.0)) + np.float32(w[2] * third))
    assert F.fuse(col, [0, 3], "sum", w).view(np.uint32).tolist() == [[int(want.view(np.uint32))]]


def test_reference_list_merge():
    ids = np.arange(100, dtype=np.int64) * 3 + 1
    scores = np.array([[5.0, 4.0, 1.0], [6.0, 4.0, 2.0], [9.0, -np.inf, 0.0]], dtype=np.float32)
    pos = np.array([[7, 3, 9], [3, 8, 7], [50, 51, -1]], dtype=np.int64)
    got_i, got_s = F.merge_lists(scores, pos, [0, 2, 3], 4, ids=ids)
    assert got_i.tolist() == [[10, 22, 25, 28], [151, -1, -1, -1]]      # 3: 6 beats 4; 7: 5 beats 2; the tie at 4.0 cannot occur twice for one position
    assert got_s.tolist() == [[6.0, 5.0, 4.0, 1.0], [9.0, -np.inf, -np.inf, -np.inf]]
    got_i, got_s = F.merge_lists(scores, pos, [0, 2, 3], 2, ids=ids, invalid_ids=np.array([[10, 777], [151, 151]]))
    assert got_i.tolist() == [[22, 25], [-1, -1]] and got_s.tolist() == [[5.0, 4.0], [-np.inf, -np.inf]]
    tie = np.full((2, 3), 2.5, dtype=np.float32)
    got_i, _ = F.merge_lists(tie, np.array([[9, 4, 6], [5, 4, 1]]), [0, 2], 5, ids=None, n_items=10)
    assert got_i.tolist() == [[1, 4, 5, 6, 9]]      # all ties: position ascending
    # the size-1 identity: a sorted list is its own merge
    rng = np.random.default_rng(4)
    s = -np.sort(-rng.standard_normal((3, 8)).astype(np.float32), axis=1)
    p = np.stack([rng.permutation(100)[:8] for _ in range(3)])
    got_i, got_s = F.merge_lists(s, p, [0, 1, 2, 3], 8, ids=ids)
    assert np.array_equal(got_i, ids[p]) and np.array_equal(got_s, s)
    # the walk over a fused matrix is the merge of exhaustive lists
    m = _matrix(rng, 5, 40)
    m[np.isneginf(m)] = 0.0
    fused = F.fuse(m, [0, 2, 5], "max")
    order = np.argsort(~F.keys_of(m, np.broadcast_to(np.arange(40), m.shape)), axis=1, kind="stable")
    lists_s, lists_p = np.take_along_axis(m, order, 1), order
    seen = np.array([[int(ids[order[0, 0]]), 1], [int(ids[order[4, 1]]), int(ids[order[2, 0]])]])
    a = F.merge_lists(lists_s, lists_p, [0, 2, 5], 6, ids=ids[:40], invalid_ids=seen)
    b = F.topk_walk(fused, np.ones((2, 40), bool), ids[:40], 6, invalid_ids=seen)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_module():
    lims = torch.tensor([0, 2])
    for cls in (rails_amd.MoLAvgTopK, rails_amd.MoLNaiveTopK, rails_amd.MoLCombTopK):
        for call, args in (("forward", (None, 5)), ("forward_filtered", (None, 7, None, 5)), ("all_logits", (None,))):
            for kw in ({"query_lims": lims}, {"fuse": "sum"}, {"query_weights": torch.ones(2)}):
                with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}(\.\w+)? takes no {next(iter(kw))}: .*MoLBruteForceTopK"):
                    getattr(_bare(cls), call)(*args, **kw)
        for call in ("rank_of", "log_partition", "count_above", "range_search"):
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call}: .*MoLBruteForceTopK"):
                getattr(_bare(cls), call)(None, None, query_lims=lims)
    for cls in (rails_amd.MoLAvgTopK, rails_amd.MoLCombTopK):
        with pytest.raises(NotImplementedError, match=rf"^{cls.__name__} takes no query_lims"):
            _bare(cls).submit(None, 5, query_lims=lims)
        with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.topk_ids takes no query_lims"):
            _bare(cls).topk_ids(None, query_lims=lims)
    src = open(os.path.join(ROOT, "rails_amd", "sharded.py")).read()
    classes = [getattr(sharded, name) for name in re.findall(r"^class (\w+)\(", src, flags=re.M)]
    wrappers = [c for c in classes if issubclass(c, T.TopKModule)]
    assert len(wrappers) >= 6
    for cls in wrappers:
        for call, args in (("forward", (None, 5)), ("submit", (None, 5)), ("forward_filtered", (None, 7, None, 5))):
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__} takes no query_lims: .*single-device"):
                getattr(_bare(cls), call)(*args, query_lims=lims)
        with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.rank_of: .*single-device MoLBruteForceTopK"):
            _bare(cls).rank_of(None, None, query_lims=lims)
