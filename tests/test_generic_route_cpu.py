"""The shape-generic scoring route, device-free: the C ABI's envelope and size helpers, the fixture against the oracle, and the
scratch budget of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from oracle import mol_oracle as O
from rails_amd import _lib
from rails_amd import engine as E
from tests._generic_fixtures import generic_cases, spec_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
CASES = ["g_4x4x64", "g_2x2x128_h32", "g_1x1x64", "g_4x8x24_h96", "g_8x8x40", "g_12x3x20_h50_swiglu", "g_16x8x32_h256", "g_32x8x16",
         "g_8x8x32_h192", "g_uid_4x4x32", "g_none_4x4x24"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_abi_version_of_header_and_binding():
    text = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert int(re.search(r"#define RAILS_ABI_VERSION (\d+)", text).group(1)) == _lib.RAILS_ABI_VERSION == 15
    assert " 15: " in text   # the version history names it


def test_every_fixture_case_is_generic_only(lib):
    names = []
    for name, cfg, w, a in generic_cases():
        s = spec_of(cfg, E).to_c()
        assert lib.rails_mol_shape_supported(C.byref(s)) == 0 and "no fused scoring kernel" in _lib.last_error(), name
        assert lib.rails_mol_generic_supported(C.byref(s)) == 1, (name, _lib.last_error())
        names.append(name)
    assert names == sorted(CASES)


def test_size_helpers_answer_without_a_device(lib):
    s = E.MolShapeSpec(64, 64, 24, 4, 8, 512, 128, 128, 96).to_c()      # d = 24 -> 24, L = 32, H = 96
    assert lib.rails_mol_generic_gate_pack_floats(C.byref(s)) == 2 * 96 * 32 + 96 + 32
    assert lib.rails_mol_generic_index_floats(C.byref(s), 33) == 2 * 32 * (8 * 24 + 32)           # two tiles of 32 rows
    assert lib.rails_mol_generic_query_pack_floats(C.byref(s), 5) == 5 * (4 * 24 + 32)
    s = E.MolShapeSpec(64, 64, 20, 12, 3, 512, 128, 128, 50).to_c()     # d = 20 -> 24, L = 36 -> Lp 64, H = 50 -> 64
    assert lib.rails_mol_generic_gate_pack_floats(C.byref(s)) == 2 * 64 * 64 + 64 + 64
    assert lib.rails_mol_generic_index_floats(C.byref(s), 1) == 32 * (3 * 24 + 36)
    assert lib.rails_mol_generic_query_pack_floats(C.byref(s), 7) == 7 * (12 * 24 + 36)
    assert lib.rails_mol_generic_index_floats(C.byref(s), 0) == 0
    fused = E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, 128).to_c()  # a fused shape is inside the envelope too (the forced route)
    assert lib.rails_mol_shape_supported(C.byref(fused)) == 1 and lib.rails_mol_generic_supported(C.byref(fused)) == 1


@pytest.mark.parametrize("spec, precision, needle", [
    (E.MolShapeSpec(64, 64, 16, 257, 1, 64, 128, 128, 128), "fp32", "P_Q * P_X <= 256"),
    (E.MolShapeSpec(64, 64, 257, 4, 4, 64, 128, 128, 128), "fp32", "dot_product_dimension <= 256"),
    (E.MolShapeSpec(64, 64, 64, 4, 4, 64, 128, 128, 513), "fp32", "gating_qi_hidden_dim <= 512"),
    (E.MolShapeSpec(64, 64, 64, 4, 4, 64, 128, 128, -1), "fp32", "hidden layer"),
    (E.MolShapeSpec(64, 64, 64, 4, 4, 64, 128, 128, 128), "f16x3", "fp32 only"),
    (E.MolShapeSpec(64, 64, 256, 128, 2, 64, 128, 128, 128), "fp32", "query prologue needs"),     # the prologue's LDS bound, inherited
])
def test_shapes_outside_the_envelope_name_the_limit(lib, spec, precision, needle):
    s = spec.to_c(precision)
    assert lib.rails_mol_generic_supported(C.byref(s)) == 0
    assert needle in _lib.last_error(), _lib.last_error()
    assert lib.rails_mol_generic_gate_pack_floats(C.byref(s)) == 0


def test_oracle_reproduces_the_reference_on_the_generic_shapes():
    """The bar of tests/test_oracle_golden.py for variants.npz: logits, Eq and Ex bit for bit, per-row logits within 2e-6."""
    n = 0
    for name, cfg, w, a in generic_cases():
        uid = a.get("user_ids")
        st = O.mol_stages(cfg, w, a["q"], a["X"], uid)
        assert torch.equal(st["logits"], a["logits"]) and torch.equal(st["Eq"], a["Eq"]) and torch.equal(st["Ex"].reshape(a["Ex"].shape), a["Ex"]), name
        rows = O.mol_stages(cfg, w, a["q"], a["cand"], uid)["logits"]
        assert float((rows - a["row_logits"]).abs().max()) <= 2e-6, name
        n += 1
    assert n == len(CASES)


def test_generic_kernels_use_no_scratch():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "mol_generic.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "mol_generic"], capture_output=True, text=True, timeout=600).stdout
    rows = re.findall(r"scratch\s+(\d+) lds\s+\d+\s+(.*mol_generic.*)$", out, flags=re.M)
    assert len(rows) >= 18, out[-2000:]      # 8 logit-tile counts x (resident, streamed) + the two pack kernels
    assert all(int(sc) == 0 for sc, _ in rows), [(n, sc) for sc, n in rows if int(sc)]
