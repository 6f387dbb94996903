"""The differentiable MoLSimilarity.forward on the GPU.

Kernel level: MolEngine.pair_backward (rails_mol_generic_pair_backward) against the analytic float64 backward of tests/_mol_grad_ref.py
on the kernel's own unpacked inputs, every element within 2^-24 ((n + C) A + F); the per-tensor relative L2 error is printed next to that
of the same chain evaluated in float32 (a figure, not a bar).  Module level: the gradients of q, items and every
parameter against float64 autograd of the restatement, held to 8 x the error of fp32 eager autograd of the same restatement (floor
2^-22), and against the reference's own gradients (tests/golden/mol_grad.npz)."""
import numpy as np
import pytest
import torch

import rails_amd
from rails_amd import engine as E
from tests import _mol_grad_ref as G
from tests._generic_fixtures import spec_of

pytestmark = pytest.mark.gpu

SHAPES = G.kernel_shapes()
GOLDEN = {c[0]: c for c in G.golden_cases()}
CHUNK = 2048        # pairs per weight-gradient chunk in the kernel-level cases: 33 x 130 pairs (33 rows of 160 slots) span three chunks


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class _Shape:
    """One kernel-level shape: the engine, the packs of the 33 queries, the inputs on the device and (lazily) the unpacked float64 inputs."""

    def __init__(self, name, dev):
        self.cfg = cfg = SHAPES[name]
        w, q, items, dy = G.kernel_inputs(cfg)
        self.w = w
        self.eng = E.MolEngine(spec_of(cfg, E), {k: v.to(dev) for k, v in w.items()}, precision="fp32", route="generic")
        self.q, self.items, self.dy = q.to(dev), items.to(dev), dy.to(dev)
        self.PQ, self.PX, self.d, self.L = cfg.query_dot_product_groups, cfg.item_dot_product_groups, cfg.dot_product_dimension, cfg.num_logits
        self.dp = (self.d + 7) // 8 * 8
        self.C = G.factor_roundings(self.PQ, self.PX, self.d, cfg.gating_qi_hidden_dim)
        g = "_gating_fn._qi_partial_module."
        self.gate = [w[g + k].numpy() for k in ("1.weight", "1.bias", "3.weight", "3.bias")]
        self.inv_tau = float(np.float32(1.0) / np.float32(cfg.temperature))
        self.none = cfg.gating_combination_type == "none"

    def packs(self, B, X):
        qpack, _, _ = self.eng.query_pack(self.q[:B])
        cand = self.eng.build_index(self.items[:B, :X].reshape(B * X, -1))
        return qpack, cand

    def unpack_q(self, t, B):
        t = t.reshape(B, -1).cpu().double().numpy()
        return t[:, : self.PQ * self.dp].reshape(B, self.PQ, self.dp), t[:, self.PQ * self.dp :]

    def unpack_i(self, t, B, X):
        t = t.reshape(-1, self.PX * self.dp + (self.L + 3) // 4 * 4)[: B * X].cpu().double().numpy()
        return t[:, : self.PX * self.dp].reshape(B, X, self.PX, self.dp), t[:, self.PX * self.dp :].reshape(B, X, -1)

    def reference(self, qpack, cand, dy, B, X, mut=None):
        eqs, gq = self.unpack_q(qpack, B)
        ex, gi = self.unpack_i(cand.buf, B, X)
        args = (eqs[..., : self.d], gq[:, : self.L], ex[..., : self.d], gi[..., : self.L], *self.gate, dy.cpu().numpy(), self.inv_tau, self.none)
        ref = G.pair_backward64(*args)
        self.f32 = {k: v[0] for k, v in G.pair_backward64(*args, dtype=np.float32).items()}      # the same chain at the kernel's precision
        return ref

    def compare(self, got, ref, B, X, tag):
        """got = pair_backward's (d_qpack, d_ipack, weights) -> {tensor: largest err / bound}; asserts the bound and the zero pads."""
        dq, di, dw = got
        out = {}
        if dq is not None:
            deq, dgq = self.unpack_q(dq, B)
            out.update({"dEq": deq[..., : self.d], "dgq": dgq[:, : self.L]})
            assert not deq[..., self.d :].any() and not dgq[:, self.L :].any(), "pads of d_qpack"
        if di is not None:
            dex, dgi = self.unpack_i(di, B, X)
            out.update({"dEx": dex[..., : self.d], "dgi": dgi[..., : self.L]})
            assert not dex[..., self.d :].any() and not dgi[..., self.L :].any(), "pads of d_ipack"
        if dw is not None:
            out.update({k: t.cpu().double().numpy() for k, t in zip(("dW1", "db1", "dW2", "db2"), dw)})
        worst = {}
        for k, v in out.items():
            val, A, n, F = ref[k]
            assert np.isfinite(v).all(), (tag, k)
            bound = G.grad_bound(A, n, self.C, F)
            ratio = np.abs(v - val) / np.maximum(bound, 1e-300)
            ratio[(bound == 0) & (v == val)] = 0.0
            worst[k] = float(ratio.max())
        print("MOLGRAD", tag, B, X, " ".join(f"{k}={r:.4f}" for k, r in sorted(worst.items())))
        l2 = {k: (G.rel_l2(v, ref[k][0]), G.rel_l2(self.f32[k], ref[k][0])) for k, v in out.items()}
        print("MOLGRADL2", tag, B, X, " ".join(f"{k}={o:.2e}/{f:.2e}" for k, (o, f) in sorted(l2.items())))
        assert all(r <= 1.0 for r in worst.values()), (tag, B, X, worst)
        return worst


_CACHE = {}


def shape_of(name, dev) -> _Shape:
    if name not in _CACHE:
        _CACHE[name] = _Shape(name, dev)
    return _CACHE[name]


@pytest.mark.parametrize("X", G.KERNEL_X)
@pytest.mark.parametrize("B", G.KERNEL_B)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_pair_backward_against_float64(name, B, X, dev):
    s = shape_of(name, dev)
    qpack, cand = s.packs(B, X)
    dy = s.dy[:B, :X]                                     # a view: leading dimension 130 whatever X is
    got = s.eng.pair_backward(qpack, B, cand, X, dy, chunk_pairs=CHUNK)
    s.compare(got, s.reference(qpack, cand, dy, B, X), B, X, name)


def test_zero_dy_gives_zeros(dev):
    s = shape_of("12x3x20_h50", dev)
    B, X = 3, 33
    qpack, cand = s.packs(B, X)
    dq, di, dw = s.eng.pair_backward(qpack, B, cand, X, torch.zeros((B, X), device=dev))
    for t in (dq, di) + tuple(dw):
        assert not t.any()


def test_leading_dimension_and_two_runs(dev):
    s = shape_of("8x8x32_h128", dev)
    B, X = 33, 130
    qpack, cand = s.packs(B, X)
    wide = torch.full((B, X + 61), float("nan"), device=dev)     # what lies between the rows is never read
    wide[:, :X] = s.dy
    a = s.eng.pair_backward(qpack, B, cand, X, wide[:, :X], chunk_pairs=CHUNK)
    b = s.eng.pair_backward(qpack, B, cand, X, s.dy.contiguous(), chunk_pairs=CHUNK)
    c = s.eng.pair_backward(qpack, B, cand, X, s.dy.contiguous(), chunk_pairs=CHUNK)
    for x, y, z in zip((a[0], a[1]) + a[2], (b[0], b[1]) + b[2], (c[0], c[1]) + c[2]):
        assert torch.equal(x, y) and torch.equal(y, z)
    # the default chunk holds the whole call: another partition of the weight sums, the same values to the bound
    s.compare(s.eng.pair_backward(qpack, B, cand, X, s.dy), s.reference(qpack, cand, s.dy, B, X), B, X, "8x8x32_h128/default-chunk")


def test_skipped_outputs_leave_the_others_bit_for_bit(dev):
    s = shape_of("4x4x64_h128", dev)
    B, X = 3, 33
    qpack, cand = s.packs(B, X)
    dy = s.dy[:B, :X]
    full = s.eng.pair_backward(qpack, B, cand, X, dy)
    only_q = s.eng.pair_backward(qpack, B, cand, X, dy, need=(True, False, False))
    only_i = s.eng.pair_backward(qpack, B, cand, X, dy, need=(False, True, False))
    only_w = s.eng.pair_backward(qpack, B, cand, X, dy, need=(False, False, True))
    assert only_q[1] is None and only_q[2] is None and torch.equal(only_q[0], full[0])
    assert only_i[0] is None and only_i[2] is None and torch.equal(only_i[1], full[1])
    assert only_w[0] is None and only_w[1] is None and all(torch.equal(x, y) for x, y in zip(only_w[2], full[2]))


def test_no_candidates_gives_zeros(dev):
    s = shape_of("12x3x20_h50", dev)
    qpack, cand = s.packs(3, 1)
    dq, di, dw = s.eng.pair_backward(qpack, 3, cand, 0, torch.zeros((3, 0), device=dev))
    assert dq.shape[0] == 3 and not dq.any() and di.shape[0] == 0 and all(not t.any() for t in dw)


def test_a_row_longer_than_the_chunk_is_refused_for_weight_gradients(dev):
    s = shape_of("1x1x64_h128", dev)
    X = 3 * 130                                           # one row of 390 candidates; the smallest chunk holds 256 pairs
    qpack, _ = s.packs(1, 1)
    cand = s.eng.build_index(s.items[:3].reshape(X, -1))
    dy = s.dy[:3].reshape(1, X)
    with pytest.raises(NotImplementedError, match="chunk_pairs"):
        s.eng.pair_backward(qpack, 1, cand, X, dy, chunk_pairs=256)
    dq, di, dw = s.eng.pair_backward(qpack, 1, cand, X, dy, need=(True, True, False), chunk_pairs=256)
    assert dw is None and dq is not None and di is not None
    s.compare(s.eng.pair_backward(qpack, 1, cand, X, dy, chunk_pairs=512), s.reference(qpack, cand, dy, 1, X), 1, X, "1x1x64_h128/long-row")


# ---- module level ---------------------------------------------------------------------------------------------------------------
def build_module(cfg, weights, dev, differentiable=True, precision=None, route=None):
    mol, _ = rails_amd.create_mol_interaction_module(
        query_embedding_dim=cfg.query_embedding_dim, item_embedding_dim=cfg.item_embedding_dim,
        dot_product_dimension=cfg.dot_product_dimension, query_dot_product_groups=cfg.query_dot_product_groups,
        item_dot_product_groups=cfg.item_dot_product_groups, temperature=cfg.temperature, query_dropout_rate=0.0,
        query_hidden_dim=cfg.query_hidden_dim, item_dropout_rate=0.1, item_hidden_dim=cfg.item_hidden_dim,
        gating_query_hidden_dim=cfg.gating_query_hidden_dim, gating_qi_hidden_dim=cfg.gating_qi_hidden_dim,
        gating_item_hidden_dim=cfg.gating_item_hidden_dim, softmax_dropout_rate=cfg.softmax_dropout_rate, bf16_training=False,
        gating_query_fn=cfg.gating_query_fn, gating_item_fn=cfg.gating_item_fn, query_nonlinearity=cfg.query_nonlinearity,
        item_nonlinearity=cfg.item_nonlinearity, gating_combination_type=cfg.gating_combination_type, eps=cfg.eps,
        uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None)
    mol.load_state_dict(weights, strict=True)
    mol = mol.to(dev).eval()
    mol.differentiable, mol.precision, mol.route = differentiable, precision, route
    return mol


def restatement_grads(cfg, w, q, cand, dy, user_ids, dtype):
    ws = {k: v.detach().cpu().to(dtype).requires_grad_(True) if v.is_floating_point() else v.cpu() for k, v in w.items()}
    q, cand = q.detach().cpu().to(dtype).requires_grad_(True), cand.detach().cpu().to(dtype).requires_grad_(True)
    y = G.stages(cfg, ws, q, cand, None if user_ids is None else user_ids.cpu())
    keys = [k for k, v in ws.items() if v.requires_grad]
    got = torch.autograd.grad((y * dy.cpu().to(dtype)).sum(), [q, cand] + [ws[k] for k in keys], allow_unused=True)
    out = {"q": got[0], "cand": got[1]}
    out.update({"w/" + k: g for k, g in zip(keys, got[2:]) if g is not None})
    return y.detach(), out


def module_grads(mol, q, cand, dy, kw):
    for p in mol.parameters():
        p.grad = None
    q, cand = q.detach().clone().requires_grad_(True), cand.detach().clone().requires_grad_(True)
    y, aux = mol(q, cand, **kw)
    assert aux == {} and y.requires_grad
    y.backward(dy)
    out = {"q": q.grad, "cand": cand.grad}
    out.update({"w/" + k: p.grad for k, p in mol.named_parameters() if p.grad is not None})
    return y.detach(), out


def rel_l2(a, ref):
    return float((a.double().cpu() - ref.double()).norm() / max(float(ref.double().norm()), 1e-300))


def check_module(tag, cfg, w, q, cand, dy, user_ids, dev, golden=None, **modkw):
    mol = build_module(cfg, w, dev, **modkw)
    kw = {} if user_ids is None else {"user_ids": user_ids.to(dev)}
    y, got = module_grads(mol, q.to(dev), cand.to(dev), dy.to(dev), kw)
    _, g64 = restatement_grads(cfg, w, q, cand, dy, user_ids, torch.float64)
    _, g32 = restatement_grads(cfg, w, q, cand, dy, user_ids, torch.float32)
    assert set(got) == set(g64), sorted(set(got) ^ set(g64))
    for k in sorted(g64):
        eager = rel_l2(g32[k], g64[k])
        ours = rel_l2(got[k], g64[k])
        bar = max(8.0 * eager, 2.0 ** -22)
        print("MOLGRADMOD", tag, k, f"ours={ours:.3e} eager={eager:.3e} ratio={ours / max(eager, 2.0 ** -25):.2f}")
        assert ours <= bar, (tag, k, ours, eager)
        if golden is not None:       # the same verdict against the reference's own gradients
            assert rel_l2(got[k], golden[k]) <= bar, (tag, k, rel_l2(got[k], golden[k]), bar)
    return mol, y


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_module_gradients_on_the_golden_cases(name, dev):
    _, cfg, w, a, grads = GOLDEN[name]
    mol, y = check_module(name, cfg, w, a["q"], a["cand"], a["dY"], a.get("user_ids"), dev, golden=grads)
    assert float((y.cpu() - a["y"]).abs().max()) <= 2e-5


def _synthetic(name, B, X):
    cfg = SHAPES[name]
    w, q, items, dy = G.kernel_inputs(cfg)
    return cfg, w, q[:B], items[:B, :X], dy[:B, :X].contiguous()


def test_module_gradients_on_the_headline_shape_with_f16x3_precision(dev):
    """A module whose own precision is f16x3: the differentiable path still runs in fp32 on the generic route, and its forward value is
    the no-grad generic-route call of an fp32 module, bit for bit."""
    cfg, w, q, cand, dy = _synthetic("8x8x32_h128", 33, 40)
    mol, y = check_module("8x8x32_h128/f16x3", cfg, w, q, cand, dy, None, dev, precision="f16x3")
    plain = build_module(cfg, w, dev, differentiable=False, route="generic")
    with torch.no_grad():
        ref, _ = plain(q.to(dev), cand.to(dev))
    assert torch.equal(y, ref)


def test_forward_bits_and_the_switch(dev):
    cfg, w, q, cand, dy = _synthetic("12x3x20_h50", 5, 33)
    q, cand = q.to(dev), cand.to(dev)
    off = build_module(cfg, w, dev, differentiable=False)
    with torch.no_grad():
        today, _ = off(q, cand)
    qg = q.clone().requires_grad_(True)
    y_off, _ = off(qg, cand)                              # switch off: no graph, today's bits, with grad enabled too
    assert not y_off.requires_grad and torch.equal(y_off, today)
    on = build_module(cfg, w, dev, route="generic")
    y_on, _ = on(qg, cand)
    assert y_on.requires_grad
    with torch.no_grad():
        y_ng, _ = on(qg, cand)
    assert not y_ng.requires_grad and torch.equal(y_ng, y_on.detach()) and torch.equal(y_ng, today)   # (a generic-only shape: one route)
    with torch.inference_mode():
        y_inf, _ = on(q, cand)
    assert torch.equal(y_inf, today)
    for p in on.parameters():
        p.requires_grad_(False)
    y_frozen, _ = on(q, cand)                             # nothing requires grad: the switch has no effect
    assert not y_frozen.requires_grad and torch.equal(y_frozen, today)


def test_subsets_of_requires_grad(dev):
    cfg, w, q, cand, dy = _synthetic("4x4x64_h128", 5, 33)
    mol = build_module(cfg, w, dev)
    q, cand, dy = q.to(dev), cand.to(dev), dy.to(dev)
    _, full = module_grads(mol, q, cand, dy, {})

    def run(q_grad, cand_grad, params_grad):
        for p in mol.parameters():
            p.requires_grad_(params_grad)
            p.grad = None
        qq, cc = q.clone().requires_grad_(q_grad), cand.clone().requires_grad_(cand_grad)
        y, _ = mol(qq, cc)
        y.backward(dy)
        return qq.grad, cc.grad, {"w/" + k: p.grad for k, p in mol.named_parameters()}

    gq, gc, gp = run(True, False, False)
    assert torch.equal(gq, full["q"]) and gc is None and all(v is None for v in gp.values())
    gq, gc, gp = run(False, True, False)
    assert gq is None and torch.equal(gc, full["cand"]) and all(v is None for v in gp.values())
    gq, gc, gp = run(False, False, True)
    assert gq is None and gc is None and all(torch.equal(v, full[k]) for k, v in gp.items())
    for p in mol.parameters():
        p.requires_grad_(True)


def test_shared_corpus_branch_sums_the_item_gradient_over_the_batch(dev):
    cfg, w, q, cand, dy = _synthetic("12x3x20_h50", 5, 33)
    mol = build_module(cfg, w, dev)
    shared = cand[:1].to(dev)
    y, one = module_grads(mol, q.to(dev), shared, dy.to(dev), {})
    plain = build_module(cfg, w, dev, differentiable=False, route="generic")
    with torch.no_grad():
        dense, _ = plain(q.to(dev), shared)                      # the shared-corpus launch of the no-grad call
    assert torch.equal(y, dense)
    _, rows = module_grads(mol, q.to(dev), shared.expand(5, -1, -1).contiguous(), dy.to(dev), {})
    assert one["cand"].shape == (1, 33, cfg.item_embedding_dim)
    ref = rows["cand"].double().sum(0, keepdim=True)
    assert float((one["cand"].double() - ref).abs().max()) <= 2.0 ** -20 * float(rows["cand"].abs().sum(0).max())
    for k in rows:
        if k != "cand":
            assert torch.equal(one[k], rows[k]), k


def test_positives_and_negatives_in_one_call(dev):
    """SampledSoftmaxLoss's layout: X = 1 positives and X = R negatives concatenated along the candidate axis."""
    cfg, w, q, cand, dy = _synthetic("8x8x32_h128", 9, 1 + 16)
    mol = build_module(cfg, w, dev)
    q, dy = q.to(dev), dy.to(dev)
    pos, neg = cand[:, :1].to(dev).requires_grad_(True), cand[:, 1:].to(dev).requires_grad_(True)
    y, _ = mol(q, torch.cat([pos, neg], dim=1))
    y.backward(dy)
    _, whole = module_grads(mol, q, cand.to(dev), dy, {})
    assert torch.equal(torch.cat([pos.grad, neg.grad], dim=1), whole["cand"])


def test_training_mode_raises_as_before(dev):
    cfg, w, q, cand, dy = _synthetic("12x3x20_h50", 3, 5)
    mol = build_module(cfg, w, dev).train()
    with pytest.raises(NotImplementedError, match="eval-mode path only"):
        mol(q.to(dev).requires_grad_(True), cand.to(dev))


def test_three_sgd_steps_on_a_sampled_softmax_loss(dev):
    cfg, w, q, items, _ = _synthetic("8x8x32_h128", 33, 17)
    g = torch.Generator().manual_seed(3)
    q = torch.cat([q, q.flip(0)[:31] * 0.5 + 0.01 * torch.randn((31, q.shape[1]), generator=g)])          # 64 rows
    items = torch.cat([items, items.flip(1)[:31]])
    q, items = q.to(dev), items.to(dev)
    mol = build_module(cfg, w, dev)
    opt = torch.optim.SGD(mol.parameters(), lr=0.05)
    losses = []
    for step in range(3):
        opt.zero_grad()
        y, _ = mol(q, items)                                                  # candidate 0 is the positive
        loss = torch.nn.functional.cross_entropy(y, torch.zeros(64, dtype=torch.int64, device=dev))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        fresh = build_module(cfg, {k: v.detach().cpu() for k, v in mol.state_dict().items()}, dev, differentiable=False, route="generic")
        with torch.no_grad():
            want, _ = fresh(q, items)
        got, _ = mol(q, items)                                                # the engine follows the in-place step
        assert got.requires_grad and torch.equal(got.detach(), want), step
    with torch.no_grad():
        y, _ = mol(q, items)
        losses.append(float(torch.nn.functional.cross_entropy(y, torch.zeros(64, dtype=torch.int64, device=dev))))
    print("MOLGRADSGD", losses)
    assert losses[-1] < losses[0] and all(b < a for a, b in zip(losses, losses[1:])), losses
