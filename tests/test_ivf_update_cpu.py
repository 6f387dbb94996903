"""CPU: the list edit of the IVF index under frozen centroids (include/rails_amd.h rails_ivf_lists_edit[_workspace_bytes]) is exported
under the unchanged ABI version, its workspace function is a pure host function that refuses arguments outside the limits with an error
string and grows with n_old and m inside them, and the host formula for the edited size agrees with brute force."""
import ctypes as C
import random
import re
import os

import pytest

from rails_amd import _lib
from rails_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def shape(d=32, px=8):
    return E.MolShapeSpec(64, 64, d, 8, px, 512, 128, 128, 128).to_c()


def test_entry_points_are_exported_under_the_same_abi(lib):
    assert hasattr(lib, "rails_ivf_lists_edit") and hasattr(lib, "rails_ivf_lists_edit_workspace_bytes")
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert int(re.search(r"#define RAILS_ABI_VERSION (\d+)", header).group(1)) == 15 == lib.rails_abi_version()
    assert "rails_ivf_lists_edit(" in header and "rails_ivf_lists_edit_workspace_bytes(" in header


def test_workspace_refuses_outside_the_limits_and_grows_inside(lib):
    s = shape()
    ws = lambda n_old, nlist, m: lib.rails_ivf_lists_edit_workspace_bytes(C.byref(s), n_old, nlist, m)     # noqa: E731
    for args, what in (((1000, 0, 5), "nlist"), ((1000, 4097, 5), "nlist"), ((1000, 10, -1), "inserted"), ((1000, 10, 16385), "inserted"),
                       ((0, 10, 5), "old entries")):
        assert ws(*args) == 0, args
        assert what in _lib.last_error(), (args, _lib.last_error())
    assert lib.rails_ivf_lists_edit_workspace_bytes(C.byref(shape(d=48)), 1000, 10, 5) == 0 and "d = 48" in _lib.last_error()
    assert ws(1000, 1, 0) > 0 and ws(1000, 4096, 16384) > 0
    sizes_n = [ws(n, 10, 100) for n in (1, 2, 4095, 4096, 4097, 100_000, 695_762, 5_000_000)]
    sizes_m = [ws(100_000, 10, m) for m in (0, 1, 2, 300, 1024, 16383, 16384)]
    assert all(b >= a > 0 for a, b in zip(sizes_n, sizes_n[1:])), sizes_n
    assert all(b >= a > 0 for a, b in zip(sizes_m, sizes_m[1:])), sizes_m
    # room for what the launches keep: a drop byte per old position, K (P_X, n_old + 1) int32, two key arrays (P_X, m) int64
    assert ws(100_000, 10, 300) >= 100_000 + 8 * 100_001 * 4 + 2 * 8 * 300 * 8


def test_edit_refuses_before_any_launch(lib):
    dummy = C.c_void_p(16)      # never dereferenced: every check below fails first
    s = shape()
    edit = lambda **kw: lib.rails_ivf_lists_edit(C.byref(kw.get("s", s)), dummy, 1, dummy, kw.get("m", 5), kw.get("n_keep", 1000), kw.get("nlist", 10),      # noqa: E731
                                                 dummy, dummy, dummy, dummy, kw.get("n_old", 1000), dummy, dummy, dummy, kw.get("n_new", 1000), dummy, 1 << 30, None)
    s16 = E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, 128).to_c("f16x3")
    for kw, code, what in ((dict(m=16385), _lib.RAILS_ENOTSUP, "inserted"), (dict(nlist=4097), _lib.RAILS_ENOTSUP, "nlist"),
                           (dict(n_new=1006), _lib.RAILS_EINVAL, "n_new"), (dict(n_keep=500, n_new=506), _lib.RAILS_EINVAL, "n_new"),
                           (dict(n_new=0), _lib.RAILS_EINVAL, "n_new"), (dict(s=s16), _lib.RAILS_ENOTSUP, "fp32-format")):
        assert edit(**kw) == code, kw
        assert what in _lib.last_error(), (kw, _lib.last_error())


def test_edited_size_equals_brute_force():
    rng = random.Random(7)
    for case in range(400):
        n_old = rng.randint(1, 60)
        n_keep = rng.randint(0, 80)
        m = rng.randint(0, 25)
        positions = rng.sample(range(0, 100), m)
        # brute force over the lists' contents: the old lists hold 0 .. n_old - 1 once
        kept = [p for p in range(n_old) if p < n_keep and p not in positions]
        want = len(kept) + len(positions)
        assert E.ivf_edited_size(n_old, n_keep, positions) == want, (case, n_old, n_keep, positions)
        below = sum(1 for p in positions if p < min(n_old, n_keep))      # (the form IvfIndex.edit calls: the count comes from the device)
        assert E.ivf_edited_size(n_old, n_keep, m=m, below=below) == want
    import torch

    assert E.ivf_edited_size(10, 8, torch.tensor([0, 9, 20], dtype=torch.int64)) == 8 - 1 + 3
    assert E.ivf_edited_size(10, 10, []) == 10 and E.ivf_edited_size(10, 4, []) == 4
    for bad in (dict(), dict(m=3), dict(m=3, below=4), dict(m=3, below=-1), dict(m=9, below=6)):
        with pytest.raises(ValueError):
            E.ivf_edited_size(10, 5, **bad)
