"""CPU: the filtered lists of the IVF index (include/rails_amd.h rails_ivf_list_words / rails_ivf_list_counts /
rails_ivf_plan_filtered / rails_ivf_search_filtered).  The host planner against a numpy restatement on hand-made counts, the validation
of the entry points before any launch, the constructor keyword of MoLNaiveTopK, the refusals a module without the keyword keeps, and
the ABI: four additions under the unchanged version."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import rails_amd
from rails_amd import _lib
from rails_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rails_ivf_list_words", "rails_ivf_list_counts", "rails_ivf_plan_filtered", "rails_ivf_search_filtered")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def plan(lib, counts, nprobe, k):
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    rows, groups, nlist = counts.shape
    out = C.c_int32(-1)
    assert lib.rails_ivf_plan_filtered(counts.ctypes.data_as(C.c_void_p), rows, groups, nlist, nprobe, k, C.byref(out)) == _lib.RAILS_OK
    return out.value


def plan_ref(counts, nprobe, k):
    """The short-list rule's worst case per (row, group): the lists in the order that reaches k last -- smallest counts first."""
    counts = np.asarray(counts, dtype=np.int64)
    nlist = counts.shape[-1]
    need = min(nprobe, nlist)
    for c in counts.reshape(-1, nlist):
        held = np.cumsum(np.sort(c))
        reach = np.nonzero(held >= k)[0]
        need = max(need, int(reach[0]) + 1 if reach.size else nlist)
    return min(need, nlist)


def test_plan_filtered_on_hand_made_counts(lib):
    # one row, one group: 3 + 3 + 4 reach k = 10 with the three smallest of five lists
    assert plan(lib, [[[3, 50, 4, 3, 60]]], 1, 10) == 3 == plan_ref([[[3, 50, 4, 3, 60]]], 1, 10)
    # a row that needs every list (its counts never reach k), beside a row that needs exactly nprobe
    counts = [[[1, 0, 2, 0, 1, 0]], [[9, 9, 9, 9, 9, 9]]]
    assert plan(lib, counts, 2, 5) == 6 == plan_ref(counts, 2, 5)
    assert plan(lib, counts[1:], 2, 5) == 2 == plan_ref(counts[1:], 2, 5)        # 9 >= 5 after one list: nprobe decides
    assert plan(lib, counts[1:], 2, 19) == 3                                    # 9 + 9 < 19 <= 27
    assert plan(lib, counts[:1], 1, 4) == 6                                     # 0 + 0 + 0 + 1 + 1 + 2 = 4 only with all six
    assert plan(lib, counts[:1], 1, 3) == 6 and plan(lib, counts[:1], 1, 2) == 5
    # the worst (row, group) decides; nprobe is clamped to nlist
    counts = np.full((3, 2, 4), 100, dtype=np.int32)
    assert plan(lib, counts, 1, 5) == 1 and plan(lib, counts, 9, 5) == 4
    counts[2, 1] = [0, 0, 7, 100]
    assert plan(lib, counts, 1, 5) == 3 and plan(lib, counts, 1, 8) == 4
    rng = np.random.default_rng(3)
    for case in range(200):
        rows, groups, nlist = (int(v) for v in rng.integers(1, 6, 3))
        c = rng.integers(0, 8, (rows, groups, nlist)) * rng.integers(0, 2, (rows, groups, nlist))
        nprobe, k = int(rng.integers(1, nlist + 1)), int(rng.integers(1, 20))
        assert plan(lib, c, nprobe, k) == plan_ref(c, nprobe, k), (case, c.tolist(), nprobe, k)


def test_entry_points_are_additions_under_the_unchanged_abi(lib):
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert int(re.search(r"#define RAILS_ABI_VERSION (\d+)", header).group(1)) == _lib.RAILS_ABI_VERSION == lib.rails_abi_version() == 15
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    # the filtered search is the plain one plus (list_words, allowed, counts, count_rows), in front of the stream
    plain, filt = _lib.PROTOTYPES["rails_ivf_search"][1], _lib.PROTOTYPES["rails_ivf_search_filtered"][1]
    assert len(filt) == len(plain) + 4 and filt[: len(plain) - 1] == plain[:-1] and filt[-1] == plain[-1]
    assert _lib.PROTOTYPES["rails_ivf_search"][1] == [_lib._SHAPE_P, C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_int32] * 5 + [
        C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]      # (the entry every earlier caller binds did not move)


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    bad = _lib.RAILS_EINVAL
    assert lib.rails_ivf_list_words(None, 8, 100, 1, None, 1, None) == bad and lib.rails_ivf_list_words(1, 8, 100, 1, None, None, None) == bad
    assert lib.rails_ivf_list_words(1, 8, 100, None, None, 1, None) == bad and "exactly one" in _lib.last_error()
    assert lib.rails_ivf_list_words(1, 8, 100, 1, 1, 1, None) == bad and "exactly one" in _lib.last_error()
    assert lib.rails_ivf_list_words(1, 0, 100, 1, None, 1, None) == bad and lib.rails_ivf_list_words(1, 8, 0, 1, None, 1, None) == bad
    assert lib.rails_ivf_list_words(1, 8, 1 << 31, 1, None, 1, None) == bad
    for args in ((None, 1, 8, 100, 16, 1, 1, 1), (1, None, 8, 100, 16, 1, 1, 1), (1, 1, 8, 100, 16, None, 1, 1), (1, 1, 8, 100, 16, 1, 1, None),
                 (1, 1, 0, 100, 16, 1, 1, 1), (1, 1, 8, 0, 16, 1, 1, 1), (1, 1, 8, 100, 0, 1, 1, 1), (1, 1, 8, 100, 4097, 1, 1, 1), (1, 1, 8, 100, 16, 1, 0, 1)):
        assert lib.rails_ivf_list_counts(*args, None) == bad, args
    out = C.c_int32(0)
    for args in ((None, 1, 1, 4, 1, 5), (1, 0, 1, 4, 1, 5), (1, 1, 0, 4, 1, 5), (1, 1, 1, 0, 1, 5), (1, 1, 1, 4, 0, 5), (1, 1, 1, 4, 1, 0)):
        assert lib.rails_ivf_plan_filtered(*args, C.byref(out)) == bad, args
    assert lib.rails_ivf_plan_filtered(1, 1, 1, 4, 1, 5, None) == bad
    # the filtered search: the plain search's checks first, then its own pointers and count_rows in {1, batch}
    s = E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, 128).to_c()
    call = lambda batch=4, nprobe=1, k=5, allowed=1, counts=1, count_rows=1, words=1: lib.rails_ivf_search_filtered(      # noqa: E731
        C.byref(s), 1, batch, 1, 1, 1, 1, 1000, 16, nprobe, 4, 100, k, 1, 1 << 30, 1, None, words, allowed, counts, count_rows, None)
    assert call(nprobe=17) == _lib.RAILS_ENOTSUP and call(k=129) == _lib.RAILS_ENOTSUP and call(batch=-1) == bad
    assert call(allowed=None) == bad and call(counts=None) == bad and "NULL" in _lib.last_error()
    assert call(count_rows=3) == bad and "count_rows" in _lib.last_error() and call(count_rows=0) == bad
    assert call(batch=0) == _lib.RAILS_OK
    assert call(words=None, nprobe=17) == _lib.RAILS_ENOTSUP and "ivf_search:" in _lib.last_error()       # list_words == NULL: rails_ivf_search itself


def test_constructor_keyword():
    """The keyword, keyword-only and off by default.  (The constructor itself builds the item index on the device: its ValueError for
    filtered_lists=True without use_faiss=True is tests/test_ivf_filtered_gpu.py's.)"""
    p = inspect.signature(rails_amd.MoLNaiveTopK.__init__).parameters["filtered_lists"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(E.IvfIndex.search).parameters["filter"].default is None


def test_default_refusals_through_the_new_form():
    """A module built with __new__ that sets only _use_faiss and _frozen_centroids (tests/test_item_tags_cpu.py) refuses as before; the flag
    alone lifts the refusals."""
    for frozen in (False, True):
        ivf = rails_amd.MoLNaiveTopK.__new__(rails_amd.MoLNaiveTopK)
        ivf._use_faiss, ivf._frozen_centroids = True, frozen
        how = "use_faiss=True, frozen_centroids=True" if frozen else "use_faiss=True"
        with pytest.raises(NotImplementedError, match=rf"MoLNaiveTopK takes no allowed_tags: the IVF index \({re.escape(how)}\) searches its lists without a tag test"):
            ivf._take_allowed_tags({"allowed_tags": 1}, 4, (5,))
        with pytest.raises(NotImplementedError, match=rf"MoLNaiveTopK\.hide_items: the IVF index \({re.escape(how)}\) searches its lists without a visibility test"):
            ivf._check_hideable("hide_items")
        for what in ("unhide_items", "hide_items_by_id", "unhide_items_by_id", "hidden_positions", "compact"):
            with pytest.raises(NotImplementedError, match=rf"MoLNaiveTopK\.{what}: the IVF index"):
                ivf._check_hideable(what)
        ivf._filtered_lists = True
        ivf._check_hideable("hide_items")
        ivf._check_taggable("allowed_tags")
    plain = rails_amd.MoLNaiveTopK.__new__(rails_amd.MoLNaiveTopK)
    plain._use_faiss, plain._frozen_centroids = False, False
    plain._check_hideable("hide_items")
    plain._check_taggable("allowed_tags")
