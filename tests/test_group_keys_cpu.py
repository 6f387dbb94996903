"""Device-free checks of the candidate-key entry points (include/rails_amd.h rails_group_keys_*): the scratch (register spill) budget of
the two kernels, read from the built objects as tests/test_kernel_resources_cpu.py reads the scoring kernels', and the argument checks
that answer before any launch."""
import os
import re
import subprocess

import pytest

from rails_amd import _lib
from rails_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_the_group_key_kernels_use_no_scratch():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "group_keys.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "group_keys"], capture_output=True, text=True, timeout=600).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"vgpr\s+(\d+) agpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+)\s+(.*)$", line.strip())
        if m:
            rows[m.group(6).split("(")[0]] = {"vgpr": int(m.group(1)), "scratch": int(m.group(4))}
    assert set(rows) == {"mol::group_keys_pack_kernel", "mol::group_keys_merge_own_kernel"}, out
    # one key per thread and a binary search: nothing here may spill, and both kernels stay far below the 128 VGPRs of four waves per SIMD
    assert all(r["scratch"] == 0 and r["vgpr"] <= 64 for r in rows.values()), rows


def test_sizes_and_refusals_without_a_device():
    lib = _lib.load()
    assert E.group_keys_supported(8, 2048) and E.group_keys_supported(1, 16384) and E.group_keys_supported(2, 100)
    assert not E.group_keys_supported(8, 2049) and not E.group_keys_supported(0, 5) and not E.group_keys_supported(2, 0)
    # global positions of 2^48 or more: refused before any launch (no pointer is looked at)
    assert lib.rails_group_keys_pack(None, None, 4, 3, (1 << 48) - 9, 10, 3, None, None) == _lib.RAILS_EINVAL and "48 bits" in _lib.last_error()
    assert lib.rails_group_keys_pack(None, None, 4, 3, -1, 10, 3, None, None) == _lib.RAILS_EINVAL
    assert lib.rails_group_keys_pack(None, None, 4, 3, 0, 10, 2, None, None) == _lib.RAILS_EINVAL          # k_slots < k_local
    assert lib.rails_group_keys_pack(None, None, 0, 3, (1 << 48) - 10, 10, 3, None, None) == _lib.RAILS_OK  # the last range that fits; no rows
    # merge: sizes first, then the capacity, all before a launch
    assert lib.rails_group_keys_merge_own(None, 2, 10, 4, 5, 0, 9, None, None, 5, 0, 1, None) == _lib.RAILS_EINVAL     # rank_stride < rows * k
    assert lib.rails_group_keys_merge_own(None, 2, 20, 4, 5, 0, 9, None, None, 9, 0, 2, None) == _lib.RAILS_EINVAL     # two rows do not fit out_ld
    assert lib.rails_group_keys_merge_own(None, 9, 8192, 4, 2048, 0, 9, None, None, 2048, 0, 1, None) == _lib.RAILS_ENOTSUP
    assert lib.rails_group_keys_merge_own(None, 2, 20, 0, 5, 0, 9, None, None, 5, 0, 1, None) == _lib.RAILS_OK         # no rows
