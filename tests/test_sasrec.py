"""SASRec query encoder, CPU side: the module mirrors the reference's state_dict and constructor, refuses what it does not run,
the new C entries validate their arguments without a launch, the fused route states its limits, and the float64 restatement
(tests/_sasrec_ref.py) reproduces the REFERENCE's outputs (tests/golden/sasrec_*.npz, written by tools/gen_golden_sasrec.py from
modeling/sequential/sasrec.py) -- with bars tight enough that each plausible implementation bug lands outside them."""
import os
import re
import subprocess

import pytest
import torch

from tests import _sasrec_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def distance(f, seq, cur):
    """max |fixture - (seq, cur)| over forward (at the stored positions) and encode."""
    pos = torch.from_numpy(f["out/sequence_positions"])
    return max(float((seq[:, pos] - torch.from_numpy(f["out/sequence_embeddings"]).double()).abs().max()),
               float((cur - torch.from_numpy(f["out/current_embeddings"]).double()).abs().max()))


def fp32_distance(f):
    """The fp32 reference's own distance from the float64 restatement."""
    return distance(f, *S.encoder64(f))


def tolerance(f):
    """The bar an fp32 evaluation of the encoder is held to against float64: twice the reference's own fp32 distance, plus 1e-5
    (about 2^-17: a few ulps of the unit-scale postprocessed outputs, for a different but equally valid fp32 summation order)."""
    return 2.0 * fp32_distance(f) + 1e-5


@pytest.fixture(scope="module")
def lib():
    from rails_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def build(f, dev="cpu", **kw):
    from rails_amd import SASRec
    c = f["cfg"]
    m = SASRec(c["max_sequence_len"], c["max_output_len"], c["D"], c["blocks"], c["heads"], c["ffn"], c["act"], num_items=c["num_items"],
               output_postproc=c["postproc"], **kw)
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in f.items() if k.startswith("w/")}, strict=True)
    return m.to(dev).eval()


@pytest.mark.parametrize("name", S.GEOMETRIES)
def test_restatement_reproduces_the_reference(name):
    f = S.load(name)
    assert fp32_distance(f) <= 5e-6


@pytest.mark.parametrize("name", S.GEOMETRIES)
@pytest.mark.parametrize("bug", S.BUGS)
def test_tolerance_rejects_likely_bugs(name, bug):
    f = S.load(name)
    tol = tolerance(f)
    miss = distance(f, *S.encoder64(f, bug=bug))
    assert miss > 10 * tol, (bug, miss, tol)


def test_fixtures_hold_the_quirk_inputs():
    for name in S.GEOMETRIES:
        f = S.load(name)
        N = f["cfg"]["N"]
        lengths, ids = torch.from_numpy(f["in/past_lengths"]), torch.from_numpy(f["in/past_ids"])
        pos = torch.arange(N).unsqueeze(0)
        assert int(lengths.min()) == 1 and int(lengths.max()) == N and bool(((lengths > 1) & (lengths < N)).any())
        assert bool(((ids == 0) & (pos < lengths.unsqueeze(1) - 1)).any())            # an id 0 inside a length
        assert bool(((ids != 0) & (pos >= lengths.unsqueeze(1))).any())               # nonzero ids past a length
        # the forward output is stored at every position those quirks touch
        stored = set(f["out/sequence_positions"].tolist())
        quirks = ((ids == 0) & (pos < lengths.unsqueeze(1))) | ((ids != 0) & (pos >= lengths.unsqueeze(1)))
        assert {int(j) for j in quirks.nonzero()[:, 1]} | {int(n) - 1 for n in lengths} <= stored
        assert f["out/sequence_embeddings"].shape == (ids.shape[0], len(stored), f["cfg"]["D"])
        for k in f:
            if k.startswith("w/") and k.endswith("bias"):
                assert float(torch.from_numpy(f[k]).abs().min()) >= 0.1, k             # every bias randomised at O(0.1 - 1)


def test_state_dict_matches_the_reference_and_both_constructors():
    from rails_amd import SASRec
    from rails_amd.hstu import L2NormEmbeddingPostprocessor, LayerNormEmbeddingPostprocessor
    from rails_amd.modeling.sequential.embedding_modules import LocalEmbeddingModule
    from rails_amd.modeling.sequential.input_features_preprocessors import LearnablePositionalEmbeddingInputFeaturesPreprocessor
    from rails_amd.modeling.sequential.sasrec import SASRec as Mirror

    assert Mirror is SASRec
    for name in S.GEOMETRIES:
        f = S.load(name)
        c = f["cfg"]
        w = {k[2:]: torch.from_numpy(v) for k, v in f.items() if k.startswith("w/")}
        m = build(f)
        sd = m.state_dict()
        assert sorted(sd) == sorted(w) and all(tuple(sd[k].shape) == tuple(w[k].shape) for k in w)
        assert torch.equal(sd["_attn_mask"], w["_attn_mask"])
        # the reference's constructor call, keyword and positional
        D = c["D"]
        post = (LayerNormEmbeddingPostprocessor(D, 1e-6) if c["postproc"] == "layer_norm" else L2NormEmbeddingPostprocessor(D, 1e-6))
        kw = dict(max_sequence_len=c["max_sequence_len"], max_output_len=c["max_output_len"], embedding_dim=D, num_blocks=c["blocks"],
                  num_heads=c["heads"], ffn_hidden_dim=c["ffn"], ffn_activation_fn=c["act"], ffn_dropout_rate=0.2,
                  embedding_module=LocalEmbeddingModule(c["num_items"], D), similarity_module=None,
                  input_features_preproc_module=LearnablePositionalEmbeddingInputFeaturesPreprocessor(c["N"], D, 0.2),
                  output_postproc_module=post, activation_checkpoint=False, verbose=False)
        r = SASRec(**kw)
        r.load_state_dict(w, strict=True)
        assert r._postproc == c["postproc"]
        r2 = SASRec(*kw.values())
        r2.load_state_dict(w, strict=True)


def test_unsupported_inputs_raise():
    f = S.load("amzn-books")
    m = build(f)
    N, D = f["cfg"]["N"], f["cfg"]["D"]
    ids = torch.from_numpy(f["in/past_ids"])
    lengths = torch.from_numpy(f["in/past_lengths"])
    emb = m.get_item_embeddings(ids)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.encode(lengths, ids, emb, {})
    with pytest.raises(RuntimeError, match="GPU only"):
        m.forward(lengths, ids, emb, {})
    with pytest.raises(ValueError, match="expected past_ids"):
        m.encode(lengths, ids[:, :-1], emb[:, :-1], {})
    with pytest.raises(ValueError, match="expected past_ids"):
        m.forward(lengths, ids[:, :-1], emb[:, :-1], {})
    for bad in (0, N + 1, -3):
        bl = lengths.clone()
        bl[2] = bad
        with pytest.raises(ValueError, match="past_lengths"):
            m.encode(bl, ids, emb, {})
    m.train()
    with pytest.raises(NotImplementedError, match="eval-only"):
        m.encode(lengths, ids, emb, {})
    with pytest.raises(NotImplementedError, match="eval-only"):
        m.forward(lengths, ids, emb, {})
    from rails_amd import SASRec
    with pytest.raises(ValueError, match="activation"):
        SASRec(50, 1, D, 1, 4, D, "swish", num_items=10)
    with pytest.raises(ValueError, match="divisible"):
        SASRec(50, 1, 50, 1, 4, 50, "relu", num_items=10)


def test_fused_supported_answers_at_and_past_its_limits(lib):
    q = lib.rails_sasrec_fused_supported
    assert q(51, 64, 4, 64) == 1            # amzn-books
    assert q(201, 50, 1, 50) == 0           # ml-1m
    assert q(201, 256, 4, 256) == 0         # ml-20m
    assert q(64, 128, 2, 128) == 1          # every limit at once (hd 64)
    assert q(65, 128, 2, 128) == 0
    assert q(64, 129, 3, 128) == 0
    assert q(64, 128, 2, 129) == 0
    assert q(64, 128, 1, 128) == 0          # hd 128
    assert q(64, 65, 1, 64) == 0            # hd 65
    assert q(1, 1, 1, 1) == 1
    assert q(0, 64, 4, 64) == 0 and q(64, 64, 3, 64) == 0 and q(64, 64, 0, 64) == 0


def test_new_entries_reject_bad_arguments_without_a_launch(lib):
    from rails_amd import _lib

    p = 16   # a non-NULL address that is never dereferenced: validation fails before any launch
    att = lib.rails_sasrec_attention
    for args, code, what in [
        ((p, 3 * 130, 2, 51, 130, 2, p), _lib.RAILS_ENOTSUP, "head_dim"),     # hd 65
        ((p, 3 * 128, 2, 51, 128, 1, p), _lib.RAILS_ENOTSUP, "head_dim"),     # hd 128
        ((p, 3 * 64, 2, 51, 64, 3, p), _lib.RAILS_EINVAL, "multiple"),        # H * hd != D
        ((None, 3 * 64, 2, 51, 64, 4, p), _lib.RAILS_EINVAL, "NULL"),
        ((p, 3 * 64, 2, 51, 64, 4, None), _lib.RAILS_EINVAL, "NULL"),
        ((p, 3 * 64 - 1, 2, 51, 64, 4, p), _lib.RAILS_EINVAL, "stride"),
        ((p, 3 * 64, -1, 51, 64, 4, p), _lib.RAILS_EINVAL, "bad size"),
        ((p, 3 * 64, 2, 51, 64, 0, p), _lib.RAILS_EINVAL, "bad size"),
    ]:
        assert att(*args, None) == code, args
        assert what in _lib.last_error(), (_lib.last_error(), what)
    enc = lib.rails_sasrec_encode_fused
    ok = (p, p, p, p, p, 4, 2, 51, 64, 4, 64, _lib.RAILS_ACT_RELU, 0, 1e-6, p)
    for i, v, code in [(0, None, _lib.RAILS_EINVAL), (1, None, _lib.RAILS_EINVAL), (2, None, _lib.RAILS_EINVAL), (3, None, _lib.RAILS_EINVAL),
                       (4, None, _lib.RAILS_EINVAL), (14, None, _lib.RAILS_EINVAL),
                       (9, 3, _lib.RAILS_EINVAL), (11, _lib.RAILS_ACT_SILU, _lib.RAILS_EINVAL), (12, 2, _lib.RAILS_EINVAL),
                       (7, 65, _lib.RAILS_ENOTSUP), (7, 201, _lib.RAILS_ENOTSUP), (10, 129, _lib.RAILS_ENOTSUP), (6, -1, _lib.RAILS_EINVAL)]:
        args = list(ok)
        args[i] = v
        assert enc(*args, None) == code, (i, v)
        assert _lib.last_error().startswith("sasrec_encode_fused"), _lib.last_error()
    g = lib.rails_gemm_f32_id_masked
    assert g(p, 64, p, 1, None, None, 0, 10, 64, 64, 0, None, p, 64, None) == _lib.RAILS_EINVAL        # NULL row_ids
    assert g(p, 63, p, 1, None, None, 0, 10, 64, 64, 0, p, p, 64, None) == _lib.RAILS_EINVAL           # short lda
    assert g(p, 64, p, 1, None, None, 0, 10, 64, 64, 4, p, p, 64, None) == _lib.RAILS_EINVAL           # unknown activation
    assert "activation" in _lib.last_error()
    assert lib.rails_gemm_f32(p, 64, p, 1, None, None, 0, 10, 64, 64, 4, None, 0, p, 64, None) == _lib.RAILS_EINVAL
    assert lib.rails_gemm_f32(p, 64, p, 1, None, None, 0, 10, 64, 64, -1, None, 0, p, 64, None) == _lib.RAILS_EINVAL


def test_new_kernels_use_no_scratch():
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-readelf")) and os.path.exists(os.path.join(llvm, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "sasrec.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "sasrec"], capture_output=True, text=True,
                         timeout=600).stdout
    rows = [re.match(r"vgpr\s+\d+ agpr\s+\d+ sgpr\s+\d+ scratch\s+(\d+) lds\s+\d+\s+(.*)$", line.strip()) for line in out.splitlines()]
    rows = [(m.group(2), int(m.group(1))) for m in rows if m]
    names = " ".join(n for n, _ in rows)
    assert "sasrec_attention_kernel" in names and "sasrec_fused_kernel" in names, out
    assert len(rows) == 6 and all(s == 0 for _, s in rows), rows
