"""CPU: the IVF entry points (include/rails_amd.h rails_ivf_*) refuse arguments outside their limits before any launch, and the
host-side plan of the short-list rule (rails_ivf_plan) takes the fewest lists whose sizes reach k_per_group."""
import ctypes as C

import numpy as np
import pytest

from rails_amd import _lib
from rails_amd import engine as E


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def shape(d=32, px=8):
    return E.MolShapeSpec(64, 64, d, 8, px, 512, 128, 128, 128).to_c()


def test_limits_are_refused_before_any_launch(lib):
    dummy = C.c_void_p(16)      # never dereferenced: every check below fails first
    s = shape()
    assert lib.rails_ivf_train(C.byref(shape(d=48)), dummy, None, 1000, dummy, 100, 10, 1, 1, dummy, dummy, 1 << 20, None) == _lib.RAILS_ENOTSUP
    assert "d = 48" in _lib.last_error()
    assert lib.rails_ivf_train(C.byref(s), dummy, None, 1000, dummy, 1000, 5000, 1, 1, dummy, dummy, 1 << 20, None) == _lib.RAILS_ENOTSUP
    assert "nlist" in _lib.last_error()
    assert lib.rails_ivf_build_lists(C.byref(s), dummy, None, 50, 100, dummy, dummy, dummy, dummy, dummy, 1 << 20, None) == _lib.RAILS_EINVAL
    assert "nlist" in _lib.last_error()
    assert lib.rails_ivf_train(C.byref(s), dummy, None, 1000, dummy, 99, 100, 1, 1, dummy, dummy, 1, None) == _lib.RAILS_EINVAL
    s16 = E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, 128).to_c("f16x3")
    assert lib.rails_ivf_assign(C.byref(s16), dummy, None, 1000, 10, dummy, dummy, None) == _lib.RAILS_ENOTSUP
    for both in ((dummy, dummy), (None, None)):       # exactly one source: the fp32-format index or the fp16 component table
        assert lib.rails_ivf_assign(C.byref(s), *both, 1000, 10, dummy, dummy, None) == _lib.RAILS_EINVAL
        assert "exactly one" in _lib.last_error()
    search = lambda **kw: lib.rails_ivf_search(C.byref(s), dummy, 4, dummy, dummy, dummy, dummy, kw.get("n", 1000), kw.get("nlist", 100),   # noqa: E731
                                               kw.get("nprobe", 1), kw.get("mp", kw.get("nprobe", 1)), 50, kw.get("k", 5), dummy, 1 << 30, dummy, None, None)
    for kw, code, what in ((dict(nprobe=65, mp=65), _lib.RAILS_ENOTSUP, "nprobe"), (dict(nlist=10, nprobe=11, mp=11), _lib.RAILS_ENOTSUP, "nprobe"),
                           (dict(k=129), _lib.RAILS_ENOTSUP, "k_per_group"), (dict(nlist=4097), _lib.RAILS_ENOTSUP, "nlist"),
                           (dict(n=4, k=5), _lib.RAILS_EINVAL, "out of range"), (dict(nprobe=2, mp=1), _lib.RAILS_EINVAL, "max_probes")):
        assert search(**kw) == code, kw
        assert what in _lib.last_error(), (kw, _lib.last_error())
    assert lib.rails_ivf_search_workspace_bytes(C.byref(s), 4, 100, 65, 65, 50, 5) == 0
    assert lib.rails_ivf_search_workspace_bytes(C.byref(s), 4, 100, 1, 1, 50, 5) > 0


def test_plan_takes_the_fewest_lists_that_reach_k(lib):
    s = shape(px=2)
    sizes = np.array([[0, 3, 1, 50, 2, 7], [10, 10, 10, 10, 10, 10]], np.int32)     # two groups, six lists
    offsets = np.concatenate([np.zeros((2, 1), np.int32), np.cumsum(sizes, axis=1, dtype=np.int32)], axis=1).copy()
    mp, ml = C.c_int32(0), C.c_int32(0)
    for nprobe, k, want in ((1, 5, 4), (1, 1, 2), (3, 1, 3), (1, 13, 5), (1, 60, 6), (5, 10, 5)):
        assert lib.rails_ivf_plan(C.byref(s), offsets.ctypes.data_as(C.c_void_p), 6, nprobe, k, C.byref(mp), C.byref(ml)) == 0
        assert (mp.value, ml.value) == (want, 50), (nprobe, k, mp.value)
