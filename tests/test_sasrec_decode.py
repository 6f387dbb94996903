"""SASRec cached incremental decoding, CPU side: the float64 incremental restatement (tests/_sasrec_decode_ref.py) reproduces the
REFERENCE's encode along each append chain (tests/golden/sasrec_decode_*.npz, written by tools/gen_golden_sasrec_decode.py) within
tests/test_sasrec.py's bar, and that bar rejects each plausible decode bug; the new C entries state their limits and validate their
arguments without a launch; the module refuses what it does not run; the new kernels use no scratch."""
import os
import re
import subprocess

import pytest
import torch

from tests import _sasrec_decode_ref as R
from tests import _sasrec_ref as S
from tests.test_sasrec import build, tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from rails_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.mark.parametrize("name", S.GEOMETRIES)
def test_chain_fixture_holds_the_edge_cases(name):
    f = R.load(name)
    L, I = f["chain/lengths"], f["chain/ids"]
    N = f["cfg"]["N"]
    assert L.shape[0] == 4 and I.shape == (4,) + f["in/past_ids"].shape
    assert (L[0] == f["in/past_lengths"]).all() and (I[0] == f["in/past_ids"]).all()   # the prefill is the SASRec fixture's input
    assert L[0, 0] == N and (L[:, 0] == N).all()                                       # a replace-last row
    assert L[0, 1] == 1                                                                # a row that starts at length 1
    assert any(I[s, b, L[s, b] - 1] == 0 for s in range(1, 4) for b in range(L.shape[1]))   # an appended id 0
    assert any(I[s, 0, N - 1] != I[s - 1, 0, N - 1] for s in range(1, 4))              # the replaced item changed


@pytest.mark.parametrize("name", S.GEOMETRIES)
def test_incremental_restatement_reproduces_the_reference(name):
    f = R.load(name)
    inc = R.chain64(f)
    L, I = torch.from_numpy(f["chain/lengths"]), torch.from_numpy(f["chain/ids"])
    for s in range(L.shape[0]):   # the incremental form is the full encode of the updated sequence, in float64
        assert R.distance(inc[s], S.encoder64(f, ids=I[s], lengths=L[s])[1]) <= 1e-9
    assert R.distance(inc, torch.from_numpy(f["chain/out"])) <= tolerance(f)


@pytest.mark.parametrize("name", S.GEOMETRIES)
@pytest.mark.parametrize("bug", R.BUGS)
def test_tolerance_rejects_decode_bugs(name, bug):
    f = R.load(name)
    tol = tolerance(f)
    miss = R.distance(R.chain64(f, bug=bug)[1:], torch.from_numpy(f["chain/out"][1:]))
    assert miss > 10 * tol, (bug, miss, tol)


def test_decode_supported_answers_at_and_past_its_limits(lib):
    q = lib.rails_sasrec_decode_supported
    assert q(51, 64, 4, 64) == 1 and q(201, 50, 1, 50) == 1 and q(201, 256, 4, 256) == 1    # the shipped geometries
    assert q(2048, 1024, 16, 1024) == 1       # every limit at once (head_dim 64)
    assert q(2049, 64, 4, 64) == 0
    assert q(64, 1025, 25, 64) == 0
    assert q(64, 64, 4, 1025) == 0
    assert q(64, 130, 2, 64) == 0             # head_dim 65
    assert q(64, 128, 1, 64) == 0             # head_dim 128
    assert q(1, 1, 1, 1) == 1
    assert q(0, 64, 4, 64) == 0 and q(64, 64, 3, 64) == 0 and q(64, 64, 0, 64) == 0 and q(64, 0, 1, 64) == 0 and q(64, 64, 4, 0) == 0
    assert lib.rails_sasrec_decode_workspace_floats(32, 256, 512) == 32 * (6 * 256 + 512)
    assert lib.rails_sasrec_decode_workspace_floats(-1, 256, 512) == 0


def test_decode_entry_rejects_bad_arguments_without_a_launch(lib):
    import ctypes as C

    from rails_amd import _lib

    p = 16   # a non-NULL address that is never dereferenced: validation fails before any launch
    layers = (C.c_void_p * 20)(*([p] * 20))
    ok = [p, p, p, p, layers, 2, 4, 51, 64, 4, 64, _lib.RAILS_ACT_RELU, 0, 1e-6, p, p]
    dec = lib.rails_sasrec_decode
    for i, v, code, what in [(0, None, _lib.RAILS_EINVAL, "NULL"), (1, None, _lib.RAILS_EINVAL, "NULL"), (2, None, _lib.RAILS_EINVAL, "NULL"),
                             (3, None, _lib.RAILS_EINVAL, "NULL"), (4, None, _lib.RAILS_EINVAL, "NULL"), (14, None, _lib.RAILS_EINVAL, "NULL"),
                             (15, None, _lib.RAILS_EINVAL, "NULL"), (5, 0, _lib.RAILS_EINVAL, "bad size"), (6, -1, _lib.RAILS_EINVAL, "bad size"),
                             (9, 3, _lib.RAILS_EINVAL, "multiple"), (11, _lib.RAILS_ACT_SILU, _lib.RAILS_EINVAL, "ffn_act"),
                             (12, 2, _lib.RAILS_EINVAL, "postproc"), (7, 2049, _lib.RAILS_ENOTSUP, "not supported"),
                             (8, 1028, _lib.RAILS_ENOTSUP, "not supported"), (10, 1025, _lib.RAILS_ENOTSUP, "not supported")]:
        args = list(ok)
        args[i] = v
        assert dec(*args, None) == code, (i, v)
        assert _lib.last_error().startswith("sasrec_decode") and what in _lib.last_error(), (i, _lib.last_error())
    args = list(ok)
    args[8], args[9] = 128, 1   # head_dim 128
    assert dec(*args, None) == _lib.RAILS_ENOTSUP and "head_dim <= 64" in _lib.last_error()
    bad = (C.c_void_p * 20)(*([p] * 20))
    bad[13] = None        # layers[1].conv1_bias
    args = list(ok)
    args[4] = bad
    assert dec(*args, None) == _lib.RAILS_EINVAL and "layers[1]" in _lib.last_error()
    args = list(ok)
    args[6] = 0           # an empty batch is a no-op, even with no pointers
    args[0] = args[4] = args[14] = args[15] = None
    assert dec(*args, None) == _lib.RAILS_OK


def _inputs(f):
    ids = torch.from_numpy(f["in/past_ids"])
    return torch.from_numpy(f["in/past_lengths"]), ids


def test_decode_api_errors():
    f = S.load("amzn-books")
    c = f["cfg"]
    m = build(f)
    B, N, D = f["in/past_ids"].shape + (c["D"],)
    lengths, ids = _inputs(f)
    emb = m.get_item_embeddings(ids)
    cache = [(torch.zeros(B, N, D), torch.zeros(B, N, D)) for _ in range(c["blocks"])]
    with pytest.raises(RuntimeError, match="GPU only"):
        m.encode(lengths, ids, emb, {}, cache=cache)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.encode(lengths, ids, emb, {}, return_cache_states=True)
    with pytest.raises(ValueError, match="expected past_ids"):
        m.encode(lengths, ids[:, :-1], emb[:, :-1], {}, cache=cache)
    m.train()
    with pytest.raises(NotImplementedError, match="eval-only"):
        m.encode(lengths, ids, emb, {}, cache=cache)
    with pytest.raises(NotImplementedError, match="eval-only"):
        m.encode(lengths, ids, emb, {}, return_cache_states=True)


def test_cache_checks_need_no_device():
    """_check_cache runs on the host before anything is launched: wrong length, pair shape, dtype, contiguity, device."""
    f = S.load("amzn-books")
    c = f["cfg"]
    m = build(f)
    B, N, D = 8, c["N"], c["D"]
    dev = torch.device("cpu")
    good = [(torch.zeros(B, N, D), torch.zeros(B, N, D)) for _ in range(c["blocks"])]
    m._check_cache(good, B, N, dev)
    for cache, what in [(good[:-1], "one \\(k, v\\) pair per block"), (good + good[:1], "one \\(k, v\\) pair per block"),
                        ("nope", "one \\(k, v\\) pair per block"), (good[:-1] + [(good[0][0],)], "must be a pair"),
                        (good[:-1] + [(good[0][0], torch.zeros(B, N, D, dtype=torch.float64))], "float32"),
                        (good[:-1] + [(good[0][0], torch.zeros(B, D, N).transpose(1, 2))], "contiguous"),
                        (good[:-1] + [(good[0][0], torch.zeros(B, N - 1, D))], "must be"),
                        (good[:-1] + [(torch.zeros(B + 1, N, D), good[0][1])], "must be")]:
        with pytest.raises(ValueError, match=what):
            m._check_cache(cache, B, N, dev)
    with pytest.raises(ValueError, match="on cuda"):
        m._check_cache(good, B, N, torch.device("cuda", 0))


def test_unsupported_geometry_names_the_limits(monkeypatch):
    """A geometry past the decode kernels' limits raises NotImplementedError naming them (head_dim 128), before any device work."""
    from rails_amd import SASRec

    m = SASRec(50, 1, 128, 1, 1, 64, "relu", num_items=10).eval()
    ids = torch.ones((2, 51), dtype=torch.int64)
    emb = m.get_item_embeddings(ids)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))   # reach the geometry check without a GPU
    with pytest.raises(NotImplementedError, match="head_dim <= 64"):
        m.encode(torch.full((2,), 51), ids, emb, {}, cache=[])


def test_new_kernels_use_no_scratch():
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-readelf")) and os.path.exists(os.path.join(llvm, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "kvdec.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    # the single-row step's kernels: the instances over its argument block KvDecArgs, and its post kernel
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "KvDecArgs|kvdec_post_kernel"], capture_output=True, text=True,
                         timeout=600).stdout
    rows = [re.match(r"vgpr\s+\d+ agpr\s+\d+ sgpr\s+\d+ scratch\s+(\d+) lds\s+\d+\s+(.*)$", line.strip()) for line in out.splitlines()]
    rows = [(m.group(2), int(m.group(1))) for m in rows if m]
    names = " ".join(n for n, _ in rows)
    assert "kv_rows_kernel" in names and "kv_attn_kernel" in names and "kvdec_post_kernel" in names, out
    assert len(rows) == 12 and all(s == 0 for _, s in rows), rows
    assert not any("sasrec" in n for n, _ in rows)   # tests/test_sasrec.py counts the kernels whose names hold that word
