"""SASRec encoder kernels on the GPU: the module against the REFERENCE's fixtures (tests/golden/sasrec_*.npz) on both routes, the
attention entry against float64 at the sequence lengths and head widths the routes meet, the fused route at its limits against the
per-layer route and float64, and the eval harness end to end with a SASRec encoder.

Tolerances are derived, not guessed.  Module outputs: twice the fp32 reference's own distance from float64 (torch fp32 on the CPU, the
same computation in another summation order), plus 1e-5 (tests/test_sasrec.py::tolerance; that file checks the bar rejects each
likely implementation bug).  Attention: a per-element bound from float64 absolute sums with u = 2^-24, constants named below."""

import pytest
import torch

from tests import _sasrec_ref as S
from tests.test_sasrec import build, tolerance

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_DOT = 2.0    # fp32 dot products of n terms: |err| <= C_DOT * u * (n + 2) * sum |terms| (gamma_n <= 1.01 n u, doubled for safety)
C_EXP = 4.0    # v_exp_f32 (~1 ulp) plus the roundings of the log2e product and the max subtraction: relative error of a softmax weight
               # <= C_EXP * u * (1 + |s| + |s_max|) on top of the score error
C_SUM = 1.01   # round-to-nearest sums of n terms: gamma_n <= 1.01 n u (Higham, Lemma 3.1)


def dev():
    return torch.device("cuda", 0)


def lib():
    from rails_amd import _lib
    return _lib.load()


def tensors(f):
    return (torch.from_numpy(f["in/past_lengths"]), torch.from_numpy(f["in/past_ids"]))


def run_model(m, f, on_device_lengths=False):
    lengths, ids = tensors(f)
    d = dev()
    with torch.inference_mode():
        emb = m.get_item_embeddings(ids.to(d))
        cur = m.encode(lengths.to(d) if on_device_lengths else lengths, ids.to(d), emb, {})
        seq = m.forward(lengths, ids.to(d), emb, {})
    torch.cuda.synchronize()
    return seq.cpu().double(), cur.cpu().double()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", S.GEOMETRIES)
def test_encode_and_forward_match_the_reference(name, fused):
    f = S.load(name)
    c = f["cfg"]
    m = build(f, dev())
    m.use_fused_kernel = fused
    took_fused = fused and bool(lib().rails_sasrec_fused_supported(c["N"], c["D"], c["heads"], c["ffn"]))
    assert took_fused == (fused and name.startswith("amzn-books"))
    seq64, cur64 = S.encoder64(f)
    tol = tolerance(f)
    for on_dev in (False, True):
        seq, cur = run_model(m, f, on_device_lengths=on_dev)
        assert float((cur - cur64).abs().max()) <= tol, (float((cur - cur64).abs().max()), tol)
        assert float((seq - seq64).abs().max()) <= tol, (float((seq - seq64).abs().max()), tol)
        # and the reference's own fp32 outputs, within the same bar plus their own distance
        assert float((cur - torch.from_numpy(f["out/current_embeddings"]).double()).abs().max()) <= 2 * tol


# ----------------------------------------------------------------------------------------------------------------------------
# the attention entry against float64
# ----------------------------------------------------------------------------------------------------------------------------
def attention_bound(qkv64, B, N, H):
    """Per-element bound on |fp32 kernel - float64| for softmax(q k^T / sqrt(hd)) v, from float64 absolute sums:
    score error e_j = C_DOT u (hd + 3) sum_d |q_d k_jd| / sqrt(hd) (the dot product and the pre-scaling of q); weight error
    eps_j = e_j + C_EXP u (1 + |s_j| + |s_max|) relative; a convex combination moves by <= 2 max eps_j max_j |v_j - out| <= 4 max eps_j
    max |v|; the n-term sums (numerator, denominator, rescales) add C_SUM u (n + 2) max |v| each, twice."""
    D = qkv64.shape[1] // 3
    hd = D // H
    q, k, v = (qkv64[:, i * D:(i + 1) * D].reshape(B, N, H, hd).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / hd ** 0.5
    e = C_DOT * U * (hd + 3) * (q.abs() @ k.abs().transpose(-1, -2)) / hd ** 0.5
    causal = torch.tril(torch.ones((N, N), dtype=torch.bool))
    s_max = s.masked_fill(~causal, float("-inf")).amax(-1, keepdim=True)
    eps = (e + C_EXP * U * (1 + s.abs() + s_max.abs())).masked_fill(~causal, 0).amax(-1)          # (B, H, N)
    vmax = torch.cummax(v.abs().amax(-1), dim=-1).values                                          # max |v_j| over j <= i
    n = torch.arange(1, N + 1, dtype=torch.float64)
    bound = vmax * (4 * eps + 2 * C_SUM * U * (n + 2)) + 1e-30
    return bound.transpose(1, 2).reshape(B * N, H).repeat_interleave(hd, dim=1)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 201, 512])
@pytest.mark.parametrize("hd", [16, 50, 64])
@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_attention_matches_float64(N, hd, scale):
    """scale 30: scores in the thousands, where exp without the maximum subtracted overflows."""
    from rails_amd import _lib
    from rails_amd.engine import _ptr, _stream

    H, B = 2, 3
    D = H * hd
    ld = 3 * D + 5                                   # a row stride wider than the rows
    g = torch.Generator().manual_seed(N * 131 + hd * 7 + int(scale))
    qkv = torch.randn((B * N, ld), generator=g) * scale
    d = dev()
    out = torch.full((B * N, D), float("nan"), device=d)
    with torch.inference_mode():
        qd = qkv.to(d)
        _lib.check(lib().rails_sasrec_attention(_ptr(qd), ld, B, N, D, H, _ptr(out), _stream()), "rails_sasrec_attention")
    torch.cuda.synchronize()
    qkv64 = qkv[:, :3 * D].double()
    ref = S.attention64(qkv64, B, N, H)
    err = (out.cpu().double() - ref).abs()
    bound = attention_bound(qkv64, B, N, H)
    assert bool(torch.isfinite(out).all())
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound).max()))


# ----------------------------------------------------------------------------------------------------------------------------
# the fused route at its limits
# ----------------------------------------------------------------------------------------------------------------------------
def random_model(N, D, H, F, act, postproc, seed):
    from rails_amd import SASRec
    torch.manual_seed(seed)
    num_items = 150
    m = SASRec(N - 1, 1, D, 2, H, F, act, num_items=num_items, output_postproc=postproc)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 2)
    B = 5
    lengths = torch.randint(1, N + 1, (B,), generator=g)
    lengths[0], lengths[1] = N, 1
    ids = torch.randint(1, num_items + 1, (B, N), generator=g) * (torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1))
    ids[2, (int(lengths[2]) - 1) // 2] = 0
    ids[3, int(lengths[3]):] = torch.randint(1, num_items + 1, (N - int(lengths[3]),), generator=g)
    cfg = dict(max_sequence_len=N - 1, max_output_len=1, N=N, D=D, blocks=2, heads=H, ffn=F, num_items=num_items, act=act, postproc=postproc)
    f = S.from_model(m, lengths, ids, cfg)
    return m.to(dev()).eval(), f


def random_tolerance(f):
    seq64, cur64 = S.encoder64(f)
    seq32, cur32 = S.encoder64(f, dtype=torch.float32)
    return 2.0 * max(float((seq32.double() - seq64).abs().max()), float((cur32.double() - cur64).abs().max())) + 1e-5


@pytest.mark.parametrize("N,D,H,F,act,postproc,fits", [
    (64, 128, 2, 128, "relu", "layer_norm", True),     # every limit at once (hd 64)
    (64, 128, 8, 128, "gelu", "l2_norm", True),        # hd 16
    (64, 96, 3, 128, "relu", "l2_norm", True),         # hd 32, D not a power of two
    (1, 64, 4, 64, "relu", "layer_norm", True),        # one position
    (65, 128, 2, 128, "relu", "layer_norm", False),    # one position too many
    (64, 128, 2, 129, "gelu", "layer_norm", False),    # FFN one too wide
    (64, 132, 4, 128, "relu", "l2_norm", False),       # D past 128
])
def test_fused_route_at_its_limits(N, D, H, F, act, postproc, fits):
    m, f = random_model(N, D, H, F, act, postproc, seed=N + D + F)
    assert bool(lib().rails_sasrec_fused_supported(N, D, H, F)) == fits
    tol = random_tolerance(f)
    seq64, cur64 = S.encoder64(f)
    m.use_fused_kernel = True
    seq_f, cur_f = run_model(m, f)
    m.use_fused_kernel = False
    seq_l, cur_l = run_model(m, f)
    assert float((cur_f - cur64).abs().max()) <= tol, (float((cur_f - cur64).abs().max()), tol)
    assert float((cur_l - cur64).abs().max()) <= tol, (float((cur_l - cur64).abs().max()), tol)
    assert float((seq_l - seq64).abs().max()) <= tol
    assert float((cur_f - cur_l).abs().max()) <= 2 * tol
    if not fits:   # refused: the per-layer route ran both times
        assert torch.equal(cur_f, cur_l)


def test_gemm_new_activations_and_id_mask():
    from rails_amd import _lib
    from rails_amd.engine import _ptr, _stream

    d = dev()
    M, N, K = 300, 96, 64
    g = torch.Generator().manual_seed(3)
    a = torch.randn((M, K), generator=g)
    w = torch.randn((N, K), generator=g) / K ** 0.5
    b = torch.randn((N,), generator=g)
    r = torch.randn((M, N), generator=g)
    ids = torch.randint(0, 3, (M,), generator=g)
    pre = a.double() @ w.double().T + b.double()
    bound = C_DOT * U * (K + 2) * (a.double().abs() @ w.double().abs().T + b.double().abs()) * 1.2 + 4 * U * r.double().abs() + 1e-30
    for act, fn in [(_lib.RAILS_ACT_RELU, torch.relu), (_lib.RAILS_ACT_GELU, torch.nn.functional.gelu)]:
        for masked in (False, True):
            out = torch.full((M, N), float("nan"), device=d)
            with torch.inference_mode():
                ad, wd, bd, rd, idd = (t.to(d) for t in (a, w, b, r, ids))
                if masked:
                    rc = lib().rails_gemm_f32_id_masked(_ptr(ad), K, _ptr(wd), 1, _ptr(bd), _ptr(rd), N, M, N, K, act, _ptr(idd), _ptr(out), N, _stream())
                else:
                    rc = lib().rails_gemm_f32(_ptr(ad), K, _ptr(wd), 1, _ptr(bd), _ptr(rd), N, M, N, K, act, None, 0, _ptr(out), N, _stream())
                _lib.check(rc, "gemm")
            torch.cuda.synchronize()
            ref = fn(pre) + r.double()
            if masked:
                ref = ref * (ids != 0).double().unsqueeze(1)
            err = (out.cpu().double() - ref).abs()
            assert bool((err <= bound + 2 * U * ref.abs() + 4 * U * pre.abs()).all()), (act, masked, float(err.max()))
            if masked:
                assert bool((out.cpu()[ids == 0] == 0).all())


# ----------------------------------------------------------------------------------------------------------------------------
# the eval harness end to end
# ----------------------------------------------------------------------------------------------------------------------------
def test_eval_harness_with_a_sasrec_encoder():
    """eval_metrics_v2_from_tensors unchanged, with rails_amd.SASRec as `model` (amzn-books fixture, MoL similarity): its top-k ids
    match those of the fixture's reference `encode` output fed to the same top-k module."""
    import random

    import rails_amd
    from oracle import mol_oracle as O
    from rails_amd import eval_harness as H
    from tests._fixtures import assert_topk_matches

    f = S.load("amzn-books")
    c = f["cfg"]
    mcfg = O.CONFIGS["amzn-books"]
    mol, _ = rails_amd.create_mol_interaction_module(
        mcfg.query_embedding_dim, mcfg.item_embedding_dim, mcfg.dot_product_dimension, mcfg.query_dot_product_groups,
        mcfg.item_dot_product_groups, mcfg.temperature, 0.0, mcfg.query_hidden_dim, 0.1, mcfg.item_hidden_dim,
        mcfg.gating_query_hidden_dim, mcfg.gating_qi_hidden_dim, mcfg.gating_item_hidden_dim, mcfg.softmax_dropout_rate, False,
        query_nonlinearity=mcfg.query_nonlinearity)
    mol.load_state_dict(O.synthetic_weights(mcfg, seed=4), strict=True)
    from rails_amd import SASRec
    m = SASRec(c["max_sequence_len"], c["max_output_len"], c["D"], c["blocks"], c["heads"], c["ffn"], c["act"], num_items=c["num_items"],
               similarity_module=mol, output_postproc=c["postproc"])
    res = m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in f.items() if k.startswith("w/")}, strict=False)
    assert not res.unexpected_keys and all(k.startswith("_ndp_module.") for k in res.missing_keys)
    d = dev()
    m = m.to(d).eval()
    lengths, ids = tensors(f)
    all_ids = torch.arange(1, c["num_items"] + 1, dtype=torch.int64)
    target = torch.randint(1, c["num_items"] + 1, (ids.shape[0], 1), generator=torch.Generator().manual_seed(1))
    with torch.inference_mode():
        state = H.get_eval_state(m, all_ids.tolist(), None, lambda emb, eids: rails_amd.MoLBruteForceTopK(m._ndp_module, emb, eids), d)
        feats = H.SequentialFeatures(lengths.to(d), ids.to(d), None, {})
        rs = random.getstate()
        out = H.eval_metrics_v2_from_tensors(state, m, feats, target.to(d), include_eval_top_k_ids=True)
        random.setstate(rs)
        k = out["eval_top_k_ids"].shape[1]

        def topk(q):
            return state.candidate_index.get_top_k_outputs(query_embeddings=q, top_k_module=state.top_k_module, k=k, aux_payloads={},
                                                           invalid_ids=ids.to(d), return_embeddings=False)

        q_gpu = m.encode(lengths.to(d), ids.to(d), m.get_item_embeddings(ids.to(d)), {})
        gi, gs, _ = topk(q_gpu)
        ri, rs_, _ = topk(torch.from_numpy(f["out/current_embeddings"]).to(d))
    torch.cuda.synchronize()
    assert torch.equal(out["eval_top_k_ids"].cpu(), gi.cpu())
    assert_topk_matches(gs, gi, rs_, ri, atol=1e-4)
