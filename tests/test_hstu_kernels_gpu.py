"""HSTU encoder kernels (rails_amd/csrc/hstu.hip) one by one against float64 restatements, on every launch route and at the
geometry limits the host code draws between the routes.

Every float result is held to a per-element bound built from float64 absolute sums with u = 2^-24; every constant of a bound is
named below.  Time buckets, padded output rows and the columns past N of a wider output stride are exact.  The CPU tests
(unmarked) apply the bug classes a kernel could plausibly have -- an off-by-one key, a shifted bias slot, ts[i] for ts[i + 1], an
unmasked padded row, a dropped K tail, a LayerNorm without mean subtraction -- to the float64 reference and check that each lands
outside the bound at the geometry the GPU test uses, so the bars are known to catch them.

Routes are decided by geometry (hstu.hip: gemm_f32, hstu_attention, hstu_fused_supported); each GPU case states the route its
geometry takes, from the same formulas, and asserts it.  The RAILS_ATTN / RAILS_GEMM overrides are not used.
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import hstu_oracle as HO

U = 2.0 ** -24
# Bound constants (each <= 8):
C_DOT = 2.0    # chained fp32 MFMA / VALU sums: |err| <= C_DOT * u * (n + 2) * sum |terms|; gamma_n <= 1.01 n u, doubled because the
               # MFMA's internal rounding of its two products is not documented as round-to-nearest (truncation doubles u)
C_SUM = 1.01   # VALU (round-to-nearest) sums of n terms: gamma_n <= 1.01 n u while n u <= 0.01 (Higham, Lemma 3.1)
C_SILU = 2.0   # silu_fast(z) = z * rcp(1 + exp2(-log2e z)): exp2 and rcp ~1 ulp (2 u) each, three ordinary roundings, and the rounded
               # exponent argument (log2e and the product: 2 u |z|) -> relative error <= C_SILU * u * (4 + |z|)
C_NORM = 4.0   # sqrtf, the reciprocal / division, the / D and the + eps of a row normalisation: relative error <= C_NORM * u each side
SILU_LIP = 1.1  # max |d silu / dz| = 1.0998
TINY = 1e-30   # absolute floor (silu of very negative arguments underflows to 0 on the hardware exp2)

LDS_MAX = 150 * 1024      # the dynamic-LDS budget both LDS-staged kernels are given (hstu.hip)
ATTN_LD = 36              # kAttnLd
FUSED_ROWS = 64           # kFusedRows


# ----------------------------------------------------------------------------------------------------------------------------
# routes, from the host code's formulas
# ----------------------------------------------------------------------------------------------------------------------------
def attention_route(N, num_buckets):
    """hstu_attention: the workgroup kernel for N > 64 while its LDS fits, else the one-wave kernel."""
    NP = (N + 31) // 32 * 32
    lds_wg = 4 * (((NP + N + 3) & ~3) + ((num_buckets + 2 + 3) & ~3) + 3 * NP * ATTN_LD)
    return "wg" if lds_wg <= LDS_MAX and N > 64 else "wave"


def gemm_route(M, N, K, lda, w_is_nk, a_addr, w_addr):
    """gemm_f32: the LDS-tiled kernel for M >= 256 rows, N >= 64 columns and aligned operands, else the per-wave kernel."""
    aligned = K % 32 == 0 and K >= 32 and lda % 4 == 0 and a_addr % 16 == 0 and w_addr % 16 == 0 and (w_is_nk or (N % 4 == 0 and N >= 4))
    return "tiled" if aligned and M >= 256 and N >= 64 else "wave"


def fused_lds_bytes(D, H, dqk, dv):
    HV, W = H * dv, 2 * H * (dv + dqk)
    XS, AS, YS = D + 1, max(HV, D) + 1, W + 1
    return 4 * (FUSED_ROWS * (XS + AS + YS) + 2 * FUSED_ROWS + 132) + FUSED_ROWS * FUSED_ROWS


def fused_supported(N, D, H, dqk, dv, num_buckets):
    HV, W = H * dv, 2 * H * (dv + dqk)
    if N < 1 or N > FUSED_ROWS or D % 32 or D > 128 or HV % 32 or HV > 128 or W % 32 or W > 512:
        return False
    if dqk > 32 or dv > 32 or num_buckets > 128:
        return False
    return fused_lds_bytes(D, H, dqk, dv) <= LDS_MAX


# ----------------------------------------------------------------------------------------------------------------------------
# float64 references, each returning (value, per-element error bound)
# ----------------------------------------------------------------------------------------------------------------------------
def silu_bound(z, ez):
    """|silu_fast(z + e) - silu(z)| for |e| <= ez."""
    s = z * torch.sigmoid(z)
    return s, SILU_LIP * ez + C_SILU * U * (4 + z.abs()) * s.abs() + TINY


def gemm_ref(A, W, w_is_nk, bias, res, act, lengths, seq, k_drop=0, unmask=False):
    """act(A W + bias) + residual, rows r = b * seq + n with n >= lengths[b] exactly 0.  k_drop / unmask: the mutations."""
    A, W = A.double(), W.double()
    Wkn = W.T if w_is_nk else W
    K = A.shape[1]
    Ak, Wk = A[:, : K - k_drop], Wkn[: K - k_drop]
    t = Ak @ Wk
    tabs = A.abs() @ Wkn.abs()
    if bias is not None:
        t, tabs = t + bias.double(), tabs + bias.double().abs()
    e = C_DOT * U * (K + 2) * tabs
    if act:
        t, e = silu_bound(t, e)
    if res is not None:
        t = t + res.double()
        e = e * (1 + U) + U * t.abs()
    if lengths is not None and not unmask:
        pad = (torch.arange(A.shape[0]) % seq) >= lengths.cpu().repeat_interleave(seq)
        t[pad], e[pad] = 0.0, 0.0
    return t, e


def row_sum_depth(D):
    """Additions a term of a one-wave row sum passes through: ceil(D / 64) serial terms per lane, then a 6-level butterfly; never
    more than D - 1 of them change the sum (the others add zeros)."""
    return min(-(-D // 64) + 6, D)


def ln_ref(x, mul=None, eps=1e-6, depth=None, center=True):
    """LayerNorm without affine (biased variance), optionally * mul.  depth: the longest addition chain of the kernel's sums."""
    x = x.double()
    D = x.shape[1]
    n = depth if depth is not None else row_sum_depth(D)
    mean = x.mean(1, keepdim=True) if center else torch.zeros_like(x[:, :1])
    c = x - mean
    var = (c * c).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = c * rstd
    dm = C_SUM * U * (n + 1) * x.abs().mean(1, keepdim=True)           # error of the computed mean
    ec = dm + U * (c.abs() + dm)                                          # ... of each computed centred value
    ev = (C_SUM * U * n * ((c.abs() + ec) ** 2).sum(1, keepdim=True) + (2 * c.abs() * ec + ec * ec).sum(1, keepdim=True)) / D
    rel = ev / (var + eps) + C_NORM * U                                   # relative error of v / D + eps
    # of rstd: (1 - rel)^(-1/2) - 1 <= rel / (2 (1 - rel)), then sqrtf and the reciprocal
    er = torch.where(rel < 0.5, rel / (2 * (1 - rel)), torch.full_like(rel, float("inf"))) + C_NORM * U
    e = ec * rstd * (1 + er) + c.abs() * rstd * er + U * y.abs()
    if mul is not None:
        m = mul.double()
        y, e = y * m, e * m.abs() + U * (y * m).abs()
    return y, e


def l2_ref(x, eps=1e-6, depth=None):
    x = x.double()
    D = x.shape[1]
    n = depth if depth is not None else row_sum_depth(D)
    nrm = torch.sqrt((x * x).sum(1, keepdim=True))
    clamped = nrm < eps
    y = x / torch.clamp(nrm, min=eps)
    rel = 0.5 * C_SUM * U * (n + 1) + 2 * C_NORM * U
    e = torch.where(clamped, U * y.abs(), y.abs() * rel)
    return y, e


def buckets_ref(ts, num_buckets, query_shift=1):
    """(B, N keys, N queries): bucketize(ts[min(i + query_shift, N - 1)] - ts[j]).  query_shift = 0 is the ts[i] mutation."""
    N = ts.shape[1]
    qi = torch.clamp(torch.arange(N) + query_shift, max=N - 1)
    return HO.bucketize(ts[:, qi].unsqueeze(1) - ts.unsqueeze(2), num_buckets).to(torch.uint8)


def attention_ref(uvqk, B, N, H, dqk, dv, lengths, buckets, ts_w, pos_w, num_buckets, key_shift=0, slot_shift=0, unmask=False):
    """a[b, i, h, :] = sum_{j <= i} silu(q_i . k_j + pos_w[N - 1 + j - i] + ts_w[bucket[b, j, i]]) / N * v_j, rows i >= length 0."""
    x = uvqk.double().reshape(B, N, -1)
    HV, HQ = H * dv, H * dqk
    v = x[..., HV: 2 * HV].reshape(B, N, H, dv).transpose(1, 2)
    q = x[..., 2 * HV: 2 * HV + HQ].reshape(B, N, H, dqk).transpose(1, 2)
    k = x[..., 2 * HV + HQ: 2 * HV + 2 * HQ].reshape(B, N, H, dqk).transpose(1, 2)
    z = q @ k.transpose(-1, -2)                                           # (B, H, query i, key j)
    zabs = q.abs() @ k.abs().transpose(-1, -2)
    i = torch.arange(N).view(N, 1)
    j = torch.arange(N).view(1, N)
    if buckets is not None:
        bk = torch.clamp(buckets.cpu().long().transpose(1, 2) + slot_shift, max=num_buckets)   # (B, i, j)
        pos = pos_w.double()[N - 1 + j - i]
        tsb = ts_w.double()[bk]
        z = z + (pos + tsb).unsqueeze(1)
        zabs = zabs + (pos.abs() + tsb.abs()).unsqueeze(1)
    s, es = silu_bound(z, C_DOT * U * (dqk + 3) * zabs)
    P = s / N
    eP = es / N + 2 * U * P.abs()                                          # rounded 1 / N and the product
    causal = (j <= i + key_shift).double()
    P, eP = P * causal, eP * causal
    out = P @ v
    e = C_DOT * U * (N + 2) * (P.abs() @ v.abs()) + eP @ v.abs()
    if not unmask:
        pad = (torch.arange(N).view(1, N) >= lengths.cpu().view(B, 1)).view(B, 1, N, 1)
        out, e = out.masked_fill(pad, 0.0), e.masked_fill(pad, 0.0)
    return out.transpose(1, 2).reshape(B * N, HV), e.transpose(1, 2).reshape(B * N, HV)


def preprocess_ref(emb, ids, lengths, pos, scale):
    B, N, D = emb.shape
    p = emb.double() * scale
    y = p + pos.double()[:N].unsqueeze(0)
    valid = (ids.cpu() != 0) & (torch.arange(N).view(1, N) < lengths.cpu().view(B, 1))
    y = y * valid.unsqueeze(-1)
    e = 1.001 * U * (p.abs() + y.abs()) * valid.unsqueeze(-1)             # two roundings, or one with an FMA contraction
    return y, e


def outside(got, ref, bound):
    """Elements whose distance from ref exceeds the bound (a NaN counts as outside)."""
    d = (got.double().cpu() - ref).abs()
    return ~(d <= bound)


def assert_within(got, ref, bound, what):
    bad = outside(got, ref, bound)
    if bool(bad.any()):
        d = (got.double().cpu() - ref).abs()
        idx = tuple(int(t) for t in bad.nonzero()[0])
        pytest.fail(f"{what}: {int(bad.sum())} elements outside the bound; first at {idx}: got {float(got.cpu()[idx])!r}, "
                    f"ref {float(ref[idx])!r}, |d| {float(d[idx]):.3e} > bound {float(bound[idx]):.3e}")


def catches(mutated, ref, bound):
    return bool(((mutated - ref).abs() > bound).any())


# ----------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def thresholds(num_buckets):
    from rails_amd.hstu import _bucket_thresholds

    return _bucket_thresholds(num_buckets)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def timestamps(B, N, g, kind="random"):
    if kind == "random":
        return 1_000_000_000 + torch.cumsum((10.0 ** (torch.rand((B, N), generator=g) * 6)).long(), 1)
    if kind == "equal":
        return torch.full((B, N), 1_700_000_000, dtype=torch.int64)
    if kind == "decreasing":
        return 10 ** 12 - torch.cumsum((10.0 ** (torch.rand((B, N), generator=g) * 8)).long(), 1)
    if kind == "huge":          # deltas up to 1e15, both signs
        return (torch.rand((B, N), generator=g).double() * 1e15).long()
    if kind == "thresholds":    # ts[0] = 0, the others at thr - 1 / thr / thr + 1 of thresholds spread over the table
        thr = thresholds(128)
        picks = thr[torch.tensor([1, 2, 3, 8, 20, 40, 60, 80, 100, 110])]
        vals = torch.stack([picks - 1, picks, picks + 1], 1).flatten()
        row = torch.cat([torch.zeros(1, dtype=torch.int64), vals])
        reps = -(-N // row.numel())
        out = row.repeat(reps)[:N]
        return torch.stack([torch.roll(out, s) for s in range(B)])
    raise ValueError(kind)


def attention_seed(N, H, dqk):
    return N * 13 + H + dqk


def attention_inputs(B, N, H, dqk, dv, biased, nb, lengths_kind, seed, ld_extra=0, offset=0):
    g = gen(seed)
    W = 2 * H * (dqk + dv)
    ld = W + ld_extra
    store = torch.randn(B * N * ld + offset, generator=g)
    uvqk = store[offset:].view(B * N, ld)
    if lengths_kind == "one":
        lengths = torch.ones(B, dtype=torch.int64)
    elif lengths_kind == "full":
        lengths = torch.full((B,), N, dtype=torch.int64)
    else:
        lengths = torch.randint(1, N + 1, (B,), generator=g)
        lengths[0] = N
    ts = timestamps(B, N, g) if biased else None
    ts_w = torch.randn(nb + 1, generator=g) if biased else None     # O(1), distinct per slot: bias mistakes are not small
    pos_w = torch.randn(2 * N - 1, generator=g) if biased else None
    return store, uvqk, ld, lengths, ts, ts_w, pos_w


# ----------------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------------
HEADS = [(1, 1, 1), (2, 25, 25), (8, 8, 8), (4, 32, 32), (3, 31, 7), (2, 32, 17)]
# (N, (H, dqk, dv), biased, lengths, expected route).  One-wave: N <= 64; workgroup: 65 <= N <= 320; one-wave again from N = 321
# (NP = 352: the workgroup kernel's LDS no longer fits).
ATTN_CASES = [
    (1, HEADS[0], True, "full", "wave"),
    (1, HEADS[3], False, "full", "wave"),
    (31, HEADS[4], True, "random", "wave"),
    (32, HEADS[1], True, "one", "wave"),
    (33, HEADS[5], True, "random", "wave"),
    (33, HEADS[2], False, "random", "wave"),
    (64, HEADS[3], True, "full", "wave"),
    (64, HEADS[0], True, "random", "wave"),
    (65, HEADS[3], True, "random", "wg"),
    (65, HEADS[4], False, "one", "wg"),
    (211, HEADS[1], True, "random", "wg"),
    (211, HEADS[5], True, "full", "wg"),
    (320, HEADS[3], True, "random", "wg"),
    (320, HEADS[2], False, "random", "wg"),
    (321, HEADS[3], True, "random", "wave"),
    (321, HEADS[0], True, "one", "wave"),
    (400, HEADS[4], True, "random", "wave"),
    (512, HEADS[2], True, "random", "wave"),
    (512, HEADS[5], False, "full", "wave"),
]

# (M, N, K, w_is_nk, act, bias, residual, lengths (seq_len or 0), lda - K, A offset (floats), ldc - N, expected route)
GEMM_CASES = [
    (1, 1, 1, 1, 1, True, True, 1, 0, 0, 0, "wave"),
    (31, 3, 7, 0, 1, True, False, 31, 0, 0, 2, "wave"),
    (33, 4, 16, 1, 0, False, True, 11, 0, 0, 0, "wave"),
    (33, 50, 17, 0, 1, True, True, 0, 3, 1, 0, "wave"),
    (255, 64, 31, 1, 1, True, True, 51, 1, 0, 5, "wave"),
    (255, 100, 33, 0, 0, False, False, 0, 0, 0, 0, "wave"),
    (256, 260, 50, 1, 1, True, True, 64, 0, 0, 0, "wave"),
    (300, 1, 256, 0, 1, True, False, 50, 0, 0, 3, "wave"),
    (300, 3, 256, 1, 1, False, True, 0, 0, 0, 0, "wave"),
    (256, 64, 256, 1, 1, True, True, 64, 0, 0, 0, "tiled"),
    (300, 100, 256, 0, 1, True, True, 50, 0, 0, 7, "tiled"),
    (300, 260, 256, 1, 0, False, True, 0, 4, 0, 0, "tiled"),
    (256, 260, 256, 0, 1, False, False, 32, 0, 0, 0, "tiled"),
    (300, 64, 256, 1, 1, True, True, 60, 0, 1, 0, "wave"),        # misaligned A: the per-wave kernel's scalar loads
    (300, 64, 256, 1, 1, True, True, 60, 2, 0, 0, "wave"),        # lda % 4 != 0
    (256, 50, 256, 0, 1, True, True, 0, 0, 0, 0, "wave"),         # (K, N) weights with N % 4 != 0
    (256, 100, 50, 0, 1, True, True, 64, 0, 0, 0, "wave"),        # K % 32 != 0
    (1, 260, 256, 1, 1, True, True, 1, 0, 0, 1, "wave"),
    (31, 64, 1, 0, 1, True, True, 31, 0, 0, 0, "wave"),
    (255, 4, 7, 1, 0, True, False, 0, 5, 3, 0, "wave"),
]


def gemm_inputs(M, N, K, w_is_nk, bias, res, seq, lda_extra, a_off, ldc_extra, seed):
    g = gen(seed)
    lda = K + lda_extra
    a_store = torch.randn(M * lda + a_off + 4, generator=g)
    A = a_store[a_off: a_off + M * lda].view(M, lda)
    W = torch.randn((N, K) if w_is_nk else (K, N), generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    r = torch.randn((M, N), generator=g) if res else None
    lengths = torch.randint(0, seq + 1, (M // seq,), generator=g) if seq else None
    if lengths is not None:
        lengths[0] = seq
    return a_store, A, lda, W, b, r, lengths


def module(N, D, blocks, H, dqk, dv, postproc, num_buckets=128, rel_bias=True, seed=0):
    from rails_amd.hstu import HSTU

    torch.manual_seed(seed)
    m = HSTU(N - 1, 1, D, blocks, H, dv, dqk, 500, output_postproc=postproc, num_buckets=num_buckets,
             enable_relative_attention_bias=rel_bias).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("_o.bias"):
                p.normal_(0, 0.05)
            elif name.endswith("_uvqk"):
                p.normal_(0, D ** -0.5)
            elif name.endswith("_ts_w") or name.endswith("_pos_w"):
                p.normal_(0, 1.0)                       # O(1), distinct per slot
    cfg = HO.HSTUConfig(max_sequence_len=N, embedding_dim=D, num_blocks=blocks, num_heads=H, attention_dim=dqk, linear_dim=dv, num_items=500,
                        num_buckets=num_buckets, postproc=postproc)
    return m, cfg, {k: v.detach().clone() for k, v in m.state_dict().items()}


def sequences(B, N, seed, lengths=None):
    g = gen(seed)
    if lengths is None:
        lengths = torch.randint(1, N + 1, (B,), generator=g)
        lengths[0] = N
    ids = torch.randint(1, 501, (B, N), generator=g) * (torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1))
    if N > 2:
        ids[0, N // 2] = 0                              # a padding id inside the valid prefix
    return lengths, ids, timestamps(B, N, g)


def encoder_bar(cfg, w, lengths, ids, ts):
    """(float64 oracle, allowed |hip - f64|_inf): twice the fp32 oracle's own distance from float64, plus 1e-6."""
    ref64 = HO.encode(cfg, {k: v.double() for k, v in w.items()}, lengths, ids, ts)
    ref32 = HO.encode(cfg, w, lengths, ids, ts)
    return ref64, 2 * float((ref32.double() - ref64).abs().max()) + 1e-6


# ============================================================================================================================
# CPU: routes and the sensitivity of every bar
# ============================================================================================================================
def test_route_formulas_match_the_host_code():
    """The routes the GPU cases assert, from the host code's formulas: the attention split at N = 64 / 320, the fused kernel's
    limits (the library's own answer), its 153 360-byte corner."""
    import os

    from rails_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert [attention_route(n, 128) for n in (1, 64, 65, 320, 321, 512)] == ["wave", "wave", "wg", "wg", "wave", "wave"]
    assert fused_lds_bytes(128, 4, 8, 32) == 153_360 and fused_supported(64, 128, 4, 8, 32, 128)
    lib = _lib.load()
    for N in (1, 2, 33, 64, 65):
        for D in (32, 50, 64, 96, 128, 160):
            for H, dqk, dv in ((1, 32, 32), (4, 8, 32), (4, 16, 8), (8, 4, 4), (8, 8, 8), (16, 3, 2), (2, 32, 17), (4, 33, 8)):
                for nb in (8, 128, 129):
                    assert bool(lib.rails_hstu_fused_supported(N, D, H, dqk, dv, nb)) == fused_supported(N, D, H, dqk, dv, nb), (N, D, H, dqk, dv, nb)


def test_bucket_reference_is_the_oracle_bias():
    """buckets_ref is HO.rel_bias's bucket matrix (transposed to the kernels' key-major layout) and the shifted-query mutation moves it."""
    g = gen(1)
    B, N = 2, 33
    ts = timestamps(B, N, g)
    bk = buckets_ref(ts, 128)
    cfg = HO.HSTUConfig(max_sequence_len=N, embedding_dim=32, num_blocks=1, num_heads=1, attention_dim=8, linear_dim=8, num_items=1)
    ts_w = torch.arange(129, dtype=torch.float64)
    pos_w = torch.zeros(2 * N - 1, dtype=torch.float64)
    assert torch.equal(HO.rel_bias(cfg, ts_w, pos_w, ts).long(), bk.long().transpose(1, 2))
    assert not torch.equal(buckets_ref(ts, 128, query_shift=0), bk)


@pytest.mark.parametrize("case", [c for c in ATTN_CASES if c[2]], ids=lambda c: f"N{c[0]}-h{c[1][0]}x{c[1][1]}x{c[1][2]}-{c[3]}")
def test_attention_bound_catches_bias_and_key_bugs(case):
    N, (H, dqk, dv), _, lk, _ = case
    B = 2 if N <= 321 else 1
    store, uvqk, ld, lengths, ts, ts_w, pos_w = attention_inputs(B, N, H, dqk, dv, True, 128, lk, seed=attention_seed(N, H, dqk))
    bk = buckets_ref(ts, 128)
    ref, bound = attention_ref(uvqk[:, : 2 * H * (dqk + dv)], B, N, H, dqk, dv, lengths, bk, ts_w, pos_w, 128)
    args = (uvqk, B, N, H, dqk, dv, lengths)
    if N > 1:
        assert catches(attention_ref(*args, bk, ts_w, pos_w, 128, key_shift=1)[0], ref, bound), "off-by-one key"
        assert catches(attention_ref(*args, buckets_ref(ts, 128, query_shift=0), ts_w, pos_w, 128)[0], ref, bound), "ts[i] for ts[i+1]"
    assert catches(attention_ref(*args, bk, ts_w, pos_w, 128, slot_shift=1)[0], ref, bound), "shifted bias slot"
    if int(lengths.min()) < N:
        assert catches(attention_ref(*args, bk, ts_w, pos_w, 128, unmask=True)[0], ref, bound), "unmasked padded row"


@pytest.mark.parametrize("case", GEMM_CASES, ids=lambda c: "M{}-N{}-K{}-nk{}".format(*c[:4]))
def test_gemm_bound_catches_a_dropped_k_tail_and_an_unmasked_row(case):
    M, N, K, w_is_nk, act, bias, res, seq, lda_x, a_off, ldc_x, _ = case
    _, A, _, W, b, r, lengths = gemm_inputs(M, N, K, w_is_nk, bias, res, seq, lda_x, a_off, ldc_x, seed=M * 31 + N * 7 + K)
    A = A[:, :K]
    ref, bound = gemm_ref(A, W, w_is_nk, b, r, act, lengths, seq)
    if K % 16:
        assert catches(gemm_ref(A, W, w_is_nk, b, r, act, lengths, seq, k_drop=K % 16)[0], ref, bound), "dropped K tail"
    if lengths is not None and int(lengths.min()) < seq:
        assert catches(gemm_ref(A, W, w_is_nk, b, r, act, lengths, seq, unmask=True)[0], ref, bound), "unmasked padded row"


def row_shapes(rows, D, g):
    """random rows, rows of mean 1e3 and spread 1e-2, constant rows, zero rows."""
    x = torch.randn((rows, D), generator=g)
    q = rows // 4
    x[q: 2 * q] = 1e3 + 1e-2 * torch.randn((q, D), generator=g)
    x[2 * q: 3 * q] = torch.randn((q, 1), generator=g) * 10
    x[3 * q:] = 0.0
    return x


ROW_DIMS = [1, 2, 50, 63, 64, 65, 128, 256, 1000]


@pytest.mark.parametrize("D", [d for d in ROW_DIMS if d > 1])
def test_layer_norm_bound_catches_a_missing_mean_subtraction(D):
    x = row_shapes(16, D, gen(D + 1))                # the rows test_rows_layer_norm_matches_float64 runs
    ref, bound = ln_ref(x)
    assert catches(ln_ref(x, center=False)[0], ref, bound)
    assert float(bound[4:8].max()) < 1.0           # the large-mean rows keep a useful bar


# ============================================================================================================================
# GPU
# ============================================================================================================================
@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    from rails_amd import _lib

    return _lib.load()


def _call(name, *args):
    from rails_amd import _lib

    _lib.check(getattr(_lib.load(), name)(*args), name)


def _P(t):
    from rails_amd.engine import _ptr

    return _ptr(t)


def _S():
    from rails_amd.engine import _stream

    return _stream()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 2, 33, 211, 400])
@pytest.mark.parametrize("nb", [8, 128, 255])
def test_time_buckets_equal_the_oracle_bucketing(dev, B, N, nb):
    thr = thresholds(nb).to(dev)
    for kind in ("random", "equal", "decreasing", "huge", "thresholds"):
        ts = timestamps(B, N, gen(N + B + nb), kind)
        out = torch.full((B, N, N), 77, dtype=torch.uint8, device=dev)
        _call("rails_hstu_time_buckets", _P(ts.to(dev)), B, N, _P(thr), nb, _P(out), _S())
        ref = buckets_ref(ts, nb)
        assert torch.equal(out.cpu(), ref), (kind, int((out.cpu() != ref).sum()))


@pytest.mark.gpu
def test_time_buckets_refuse_256_buckets_without_launching(dev):
    thr = thresholds(256).to(dev)
    ts = timestamps(2, 40, gen(0)).to(dev)
    out = torch.full((2, 40, 40), 77, dtype=torch.uint8, device=dev)
    with pytest.raises(NotImplementedError, match="byte"):
        _call("rails_hstu_time_buckets", _P(ts), 2, 40, _P(thr), 256, _P(out), _S())
    torch.cuda.synchronize()
    assert bool((out == 77).all())


def _run_attention(dev, case, ld_extra=0, offset=0):
    N, (H, dqk, dv), biased, lk, route = case
    nb = 128
    assert attention_route(N, nb if biased else 0) == route
    B = 2 if N <= 321 else 1
    store, uvqk, ld, lengths, ts, ts_w, pos_w = attention_inputs(B, N, H, dqk, dv, biased, nb, lk, seed=attention_seed(N, H, dqk),
                                                                 ld_extra=ld_extra, offset=offset)
    d_store = store.to(dev)
    d_uvqk = d_store[offset:].view(B * N, ld)
    assert d_uvqk.data_ptr() % 16 == (4 * offset) % 16
    bk = buckets_ref(ts, nb) if biased else None
    out = torch.full((B * N, H * dv), float("nan"), device=dev)
    d = lambda t: t.to(dev) if t is not None else None   # noqa: E731
    keep = [d(lengths), d(bk), d(ts_w), d(pos_w)]
    _call("rails_hstu_attention", _P(d_uvqk), ld, B, N, H, dqk, dv, _P(keep[0]), _P(keep[1]), _P(keep[2]), _P(keep[3]), nb if biased else 0,
          _P(out), _S())
    ref, bound = attention_ref(uvqk, B, N, H, dqk, dv, lengths, bk, ts_w, pos_w, nb)
    got = out.cpu()
    pad = (torch.arange(N).view(1, N) >= lengths.view(B, 1)).flatten()
    assert bool((got[pad] == 0).all()), "rows at positions >= length must be exactly 0"
    assert_within(got, ref, bound, f"attention N={N} H={H} dqk={dqk} dv={dv} biased={biased} lengths={lk} route={route}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: f"N{c[0]}-h{c[1][0]}x{c[1][1]}x{c[1][2]}-{'bias' if c[2] else 'nobias'}-{c[3]}-{c[4]}")
def test_attention_matches_float64(dev, case):
    _run_attention(dev, case)


@pytest.mark.gpu
@pytest.mark.parametrize("N,route", [(40, "wave"), (211, "wg"), (400, "wave")])
def test_attention_wide_unaligned_rows(dev, N, route):
    """dqk = 32 with a row stride wider than the module's and the base one float off 16-byte alignment: the one-wave kernel's
    scalar Q / K loads instead of its 16-byte ones."""
    _run_attention(dev, (N, (4, 32, 32), True, "random", route), ld_extra=5, offset=1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GEMM_CASES, ids=lambda c: "M{}-N{}-K{}-nk{}-act{}-b{:d}-r{:d}-s{}-lda+{}-off{}-ldc+{}-{}".format(*c))
def test_gemm_matches_float64(dev, case):
    M, N, K, w_is_nk, act, bias, res, seq, lda_x, a_off, ldc_x, route = case
    a_store, A, lda, W, b, r, lengths = gemm_inputs(M, N, K, w_is_nk, bias, res, seq, lda_x, a_off, ldc_x, seed=M * 31 + N * 7 + K)
    d_store = a_store.to(dev)
    dA = d_store[a_off: a_off + M * lda]
    dW = W.to(dev)
    assert gemm_route(M, N, K, lda, w_is_nk, dA.data_ptr(), dW.data_ptr()) == route
    ldc = N + ldc_x
    out = torch.full((M, ldc), float("nan"), device=dev)
    keep = [t.to(dev) if t is not None else None for t in (b, r, lengths)]
    _call("rails_gemm_f32", _P(dA), lda, _P(dW), w_is_nk, _P(keep[0]), _P(keep[1]), N, M, N, K, act, _P(keep[2]), seq if seq else 0,
          _P(out), ldc, _S())
    got = out.cpu()
    assert bool(got[:, N:].isnan().all()), "columns past N of a wider ldc must keep their fill"
    ref, bound = gemm_ref(A[:, :K], W, w_is_nk, b, r, act, lengths, seq)
    if lengths is not None:
        pad = (torch.arange(M) % seq) >= lengths.repeat_interleave(seq)
        assert bool((got[pad, :N] == 0).all()), "rows at positions >= length must be exactly 0"
    assert_within(got[:, :N], ref, bound, f"gemm {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("w_is_nk", [1, 0])
@pytest.mark.parametrize("act,bias,res", [(0, False, False), (1, True, False), (0, False, True)])
def test_tiled_and_per_wave_gemm_are_bit_identical(dev, w_is_nk, act, bias, res):
    """The rows of a tiled call (M = 300) equal the same rows computed by the per-wave kernel (M = 200), with the optional
    operands absent in every combination."""
    M, small, N, K = 300, 200, 128, 64
    _, A, lda, W, b, r, _ = gemm_inputs(M, N, K, w_is_nk, bias, res, 0, 0, 0, 0, seed=5 + w_is_nk)
    dA, dW = A.to(dev), W.to(dev)
    db, dr = (b.to(dev) if b is not None else None), (r.to(dev) if r is not None else None)
    assert gemm_route(M, N, K, lda, w_is_nk, dA.data_ptr(), dW.data_ptr()) == "tiled"
    assert gemm_route(small, N, K, lda, w_is_nk, dA.data_ptr(), dW.data_ptr()) == "wave"

    def run(rows):
        out = torch.empty((rows, N), device=dev)
        _call("rails_gemm_f32", _P(dA), lda, _P(dW), w_is_nk, _P(db), _P(dr), N, rows, N, K, act, None, 0, _P(out), N, _S())
        return out

    assert torch.equal(run(M)[:small], run(small))


@pytest.mark.gpu
@pytest.mark.parametrize("D", ROW_DIMS)
def test_rows_layer_norm_matches_float64(dev, D):
    rows, ldx, ldm, ldo = 16, D + 3, D + 5, D + 2
    g = gen(D + 1)
    x = torch.full((rows, ldx), float("nan"))
    x[:, :D] = row_shapes(rows, D, g)
    mul = torch.randn((rows, ldm), generator=g)
    for with_mul in (False, True):
        out = torch.full((rows, ldo), float("nan"), device=dev)
        dm = mul.to(dev) if with_mul else None
        dx = x.to(dev)
        _call("rails_rows_layer_norm", _P(dx), ldx, rows, D, C.c_float(1e-6), _P(dm), ldm if with_mul else 0, _P(out), ldo, _S())
        got = out.cpu()
        assert bool(got[:, D:].isnan().all())
        ref, bound = ln_ref(x[:, :D], mul[:, :D] if with_mul else None)
        assert_within(got[:, :D], ref, bound, f"rows_layer_norm D={D} mul={with_mul}")


@pytest.mark.gpu
@pytest.mark.parametrize("D", ROW_DIMS)
def test_rows_normalize_matches_float64(dev, D):
    rows, ldx = 16, D + 7
    g = gen(D + 2)
    x = torch.full((rows, ldx), float("nan"))
    x[:, :D] = row_shapes(rows, D, g)
    dx = x.to(dev)
    index = torch.tensor([15, 0, 5, 5, 9, 12, 3, 14, 1], dtype=torch.int64)
    for mode in (0, 1):
        for row_index in (None, index):
            n = rows if row_index is None else row_index.numel()
            out = torch.full((n, D), float("nan"), device=dev)
            di = row_index.to(dev) if row_index is not None else None
            _call("rails_rows_normalize", _P(dx), ldx, _P(di), n, D, mode, C.c_float(1e-6), _P(out), _S())
            src = x[:, :D] if row_index is None else x[row_index, :D]
            ref, bound = ln_ref(src) if mode == 0 else l2_ref(src)
            got = out.cpu()
            assert_within(got, ref, bound, f"rows_normalize D={D} mode={mode} gather={row_index is not None}")
            if mode == 1:
                zero = (src == 0).all(1)
                assert bool((got[zero] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,D", [(1, 1, 1), (3, 33, 50), (2, 211, 64), (2, 400, 256)])
def test_preprocess_matches_float64(dev, B, N, D):
    g = gen(B * N + D)
    emb = torch.randn((B, N, D), generator=g) * 0.05
    pos = torch.randn((N, D), generator=g) * D ** -0.5
    ids = torch.randint(1, 100, (B, N), generator=g)
    ids[0, 0] = 0
    if N > 3:
        ids[min(1, B - 1), N // 2] = 0                 # inside the valid prefix of a full-length row
    lengths = torch.tensor([1, N, max(1, N // 3)][:B], dtype=torch.int64)
    scale = float(torch.tensor(D ** 0.5, dtype=torch.float32))
    out = torch.full((B, N, D), float("nan"), device=dev)
    keep = [t.to(dev) for t in (emb, ids, lengths, pos)]
    _call("rails_hstu_preprocess", _P(keep[0]), _P(keep[1]), _P(keep[2]), _P(keep[3]), B, N, D, C.c_float(scale), _P(out), _S())
    ref, bound = preprocess_ref(emb, ids, lengths, pos, scale)
    got = out.cpu()
    assert bool((got[ref == 0] == 0).all())
    assert_within(got, ref, bound, f"preprocess B={B} N={N} D={D}")


# (N, D, H, dqk, dv, num_buckets, lengths, postproc, fused?)
FUSED_CASES = [
    (64, 64, 4, 16, 8, 128, "full", "layer_norm", True),      # the row limit, all lengths 64, dqk != dv
    (1, 32, 1, 32, 32, 128, "full", "l2_norm", True),         # N = 1
    (40, 32, 8, 4, 4, 128, "random", "layer_norm", True),     # D = 32
    (64, 128, 4, 8, 32, 128, "random", "l2_norm", True),      # 153 360 of 153 600 LDS bytes
    (60, 64, 16, 3, 2, 8, "random", "layer_norm", True),      # odd dqk, 16 heads, 8 buckets
    (65, 64, 4, 16, 8, 128, "random", "layer_norm", False),   # one row past the limit
    (60, 64, 4, 16, 8, 129, "random", "l2_norm", False),      # one bucket past the limit
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "N{}-D{}-h{}x{}x{}-nb{}-{}-{}".format(*c[:8]))
def test_fused_encoder_at_and_past_its_limits(dev, lib, case):
    N, D, H, dqk, dv, nb, lk, post, fused = case
    assert bool(lib.rails_hstu_fused_supported(N, D, H, dqk, dv, nb)) == fused == fused_supported(N, D, H, dqk, dv, nb)
    m, cfg, w = module(N, D, 2, H, dqk, dv, post, num_buckets=nb, seed=N + D)
    B = 3
    lengths, ids, ts = sequences(B, N, seed=N * 3 + D, lengths=torch.full((B,), N, dtype=torch.int64) if lk == "full" else None)
    m = m.to(dev)
    for stamps in (ts, None):
        ref64, bar = encoder_bar(cfg, w, lengths, ids, stamps)
        payload = {"timestamps": stamps.to(dev)} if stamps is not None else {}
        with torch.inference_mode():
            emb = m.get_item_embeddings(ids.to(dev))
            m.use_fused_kernel, m._fused_ptrs = True, None
            cur = m.encode(lengths.to(dev), ids.to(dev), emb, payload)
            took_fused = m._fused_ptrs is not None
            m.use_fused_kernel = False
            per_layer = m.encode(lengths.to(dev), ids.to(dev), emb, payload)
        assert took_fused == fused
        err = float((cur.cpu().double() - ref64).abs().max())
        assert err <= bar, (case, stamps is not None, err, bar)
        err_pl = float((per_layer.cpu().double() - ref64).abs().max())
        assert err_pl <= bar, (case, stamps is not None, err_pl, bar)
        if not fused:
            assert torch.equal(cur, per_layer)


# (N, D, H, dqk, dv, postproc)
MODULE_CASES = [
    (65, 64, 2, 32, 32, "layer_norm"),
    (211, 50, 2, 25, 25, "l2_norm"),
    (321, 64, 3, 31, 7, "layer_norm"),
    (400, 32, 2, 32, 17, "l2_norm"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", MODULE_CASES, ids=lambda c: "N{}-D{}-h{}x{}x{}-{}".format(*c))
def test_module_per_layer_path_matches_float64(dev, case):
    N, D, H, dqk, dv, post = case
    assert not fused_supported(N, D, H, dqk, dv, 128)
    m, cfg, w = module(N, D, 2, H, dqk, dv, post, seed=N)
    B = 3
    lengths, ids, ts = sequences(B, N, seed=N + 1)
    m = m.to(dev)
    for stamps in (ts, None):
        ref64, bar = encoder_bar(cfg, w, lengths, ids, stamps)
        with torch.inference_mode():
            cur = m.encode(lengths.to(dev), ids.to(dev), m.get_item_embeddings(ids.to(dev)),
                           {"timestamps": stamps.to(dev)} if stamps is not None else {})
        err = float((cur.cpu().double() - ref64).abs().max())
        assert err <= bar, (case, stamps is not None, err, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("N,fused", [(40, True), (211, False)])
def test_disabled_relative_bias_ignores_timestamps(dev, N, fused):
    """enable_relative_attention_bias=False with timestamps passed: the oracle run without timestamps (as the reference does)."""
    D, H, dqk, dv = 64, 2, 16, 16
    assert fused_supported(N, D, H, dqk, dv, 128) == fused
    m, cfg, w = module(N, D, 2, H, dqk, dv, "layer_norm", rel_bias=False, seed=7)
    lengths, ids, ts = sequences(3, N, seed=N + 5)
    ref64, bar = encoder_bar(cfg, w, lengths, ids, None)
    m = m.to(dev)
    with torch.inference_mode():
        emb = m.get_item_embeddings(ids.to(dev))
        for use_fused in (True, False):
            m.use_fused_kernel = use_fused
            with_ts = m.encode(lengths.to(dev), ids.to(dev), emb, {"timestamps": ts.to(dev)})
            without = m.encode(lengths.to(dev), ids.to(dev), emb, {})
            assert torch.equal(with_ts, without)
            err = float((with_ts.cpu().double() - ref64).abs().max())
            assert err <= bar, (use_fused, err, bar)
