"""GPU: the generic scoring route (rails_amd/csrc/mol_generic.hip and the plain writers of mol_query.hip / mol_index.hip) on the sweep of
tests/_generic_sweep.py -- every (TL, RES) instantiation a shape inside the envelope can select, in its dense, per-row, indexed and
explaining forms, at the limits of d, H, P_Q, P_X and L and at every padded axis -- with both weight sets.

Per shape and weight set (B = 3 queries, N = 131 items, 45 candidates per row):
  writers      Eq, gq (query_pack) and Ex, gi (unpack_index) against prologue64 / index64 inside their bounds
  pads         the index, the query pack and the gate pack written into NaN-filled buffers with a fence behind them: every pad an exact 0,
               every real entry written, the fence untouched; the gate pack equals its layout restated here, entry by entry
  dense        against score64 on the engine's own operands inside its bound, and against the oracle's fp32 forward within LOGIT_TOL
  explaining   explain_candidates / explain_indexed on cl, pi and the logit, element by element, inside explain64's bounds
  same bits    dense == per-row candidates == score_indexed == score_indexed_rows (live slots; dead slots keep their sentinel) == the
               logit of both explaining launches; sum_l pi inside its bound of explain64's, every pi[l < L] finite
Several units per workgroup (n_cu read from the device): score_dense and explain_indexed on more than 2 x grid units equal, bit for bit,
the same items scored in slices that each fit one grid.

The only tolerances are the a-priori bounds of tests/_mol_ref64.py and tests/_explain_ref.py and LOGIT_TOL; every stage prints
max |err| / bound.  The largest figures of one run on an MI355X (all 38 cases; also in docs/HISTORY.md):
  Eq 0.015, gq 0.0091, Ex 0.067, gi 0.023; dense logits 0.077 of score64's bound, 8.2e-5 from the oracle (7x9x3 / H 300: |cl| near 20)
  explaining launches (both forms alike): cl 0.46, pi 0.038, sum pi 0.029, logit 0.053
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import mol_oracle as O
from rails_amd import _lib
from rails_amd import engine as E
from tests import _explain_ref as X64
from tests import _generic_sweep as G
from tests import _mol_ref64 as R
from tests.test_generic_candidates_gpu import _positions
from tests.test_generic_route_gpu import build_module
from tests.test_gpu_parity import LOGIT_TOL

pytestmark = pytest.mark.gpu

CASES = [(shape, kind) for shape in G.SWEEP for kind in G.KINDS]
NAN = float("nan")
FENCE, FENCE_VALUE = 256, -7.0


def case_id(case):
    return f"{G.name_of(case[0])}-{case[1]}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def n_cu():
    n = int(_lib.load().rails_device_compute_units())
    assert n > 0
    return n


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def within(got, ref, bound, what):
    err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"{what}: max |err| / bound = {worst:.3g}, max |err| = {float(err.max()):.3g}")
    assert bool((err <= bound).all()), (what, worst)


def explain_into(eng, qpack, batch, index, n_cand, positions=None):
    """The explaining launches into NaN-filled outputs of the caller's (the engine's own wrappers allocate unwritten memory): positions
    None -- per-row candidates held in `index`; else positions (batch, n_cand) of the shared `index`.  -> (logits, cl, pi)"""
    dev, L = index.buf.device, eng.spec.num_logits
    out = torch.full((batch, n_cand), NAN, device=dev)
    cl, pi = torch.full((batch, n_cand, L), NAN, device=dev), torch.full((batch, n_cand, L), NAN, device=dev)
    with E._on_device(dev):
        if positions is None:
            _lib.check(eng.lib.rails_mol_generic_explain(C.byref(eng.shape), E._ptr(eng.gate_pack), E._ptr(qpack), batch, E._ptr(index.buf), n_cand,
                                                         E._ptr(out), out.stride(0), E._ptr(cl), E._ptr(pi), E._stream()), "rails_mol_generic_explain")
        else:
            positions = positions.to(device=dev, dtype=torch.int64).contiguous()
            assert positions.shape == (batch, n_cand)
            _lib.check(eng.lib.rails_mol_generic_explain_indexed(C.byref(eng.shape), E._ptr(eng.gate_pack), E._ptr(qpack), batch, E._ptr(index.buf),
                                                                 index.n_items, E._ptr(positions), n_cand, E._ptr(out), out.stride(0), E._ptr(cl), E._ptr(pi),
                                                                 E._stream()), "rails_mol_generic_explain_indexed")
    return out, cl, pi


class State:
    """One shape and weight set on the device: the engine, its packs, its plain operands and the dense logits (computed once per case)."""

    def __init__(self, shape, kind, dev):
        self.shape, self.kind, self.name = shape, kind, case_id((shape, kind))
        self.cfg, self.w, self.k = G.config(shape), G.weights(shape, kind), G.launch(shape)
        self.q, self.X = G.raw_inputs(shape)
        self.mol = build_module(self.cfg, self.w, dev)
        self.mol.generic_candidates = True
        with torch.inference_mode():
            eng = self.eng = self.mol.engine()
            assert eng.route == "generic" and eng.candidates and eng.table_width == G.table_width(shape[2])
            self.qpack, self.eq, self.gq = eng.query_pack(self.q.to(dev), None, want_plain=True)
            self.index = eng.build_index(self.X.to(dev))
            self.ex, self.gi = eng.unpack_index(self.index)
            self.dense = torch.full((G.B, G.N), NAN, device=dev)
            eng.score_dense(self.qpack, G.B, self.index, out=self.dense)
        self.pos = _positions(G.B, G.N_CAND, G.N, 7 + G.SWEEP.index(shape))      # repeats, both ends, the last partial tile, out-of-range slots
        self.at = self.pos.clamp(0, G.N - 1)

    @functools.cached_property
    def explained(self):
        """explain64 on the engine's own operands -> ((cl, e_cl), (pi, e_pi), (out, e_out)) over all (B, N) pairs"""
        return X64.explain64(self.cfg, self.w, self.eq, self.ex, self.gq, self.gi)


@functools.lru_cache(maxsize=None)      # (38 small states: the largest index holds 160 rows)
def state(shape, kind, dev):
    return State(shape, kind, dev)


# ---- the writers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_prologue_and_index_writers_against_float64(case, dev):
    s = state(*case, dev)
    (eq64, eeq), (gq64, egq) = R.prologue64(s.cfg, s.w, s.q)
    (ex64, eex), (gi64, egi) = R.index64(s.cfg, s.w, s.X)
    within(s.eq, eq64, eeq, s.name + " Eq")
    within(s.gq, gq64, egq, s.name + " gq")
    within(s.ex, ex64, eex, s.name + " Ex")
    within(s.gi, gi64, egi, s.name + " gi")


def fenced(floats, dev):
    buf = torch.full((floats + FENCE,), NAN, device=dev)
    buf[floats:] = FENCE_VALUE
    return buf


def gate_pack_layout(w, k):
    """The gate pack of mol_generic.hip restated: W1f[t][c][lane][j] = W1[32 t + (lane & 31)][8 c + 4 (lane >> 5) + j],
    W2f[t][v][g][lane][j] = W2[32 v + (lane & 31)][32 t + j + 8 g + 4 (lane >> 5)], b1 [Hp], b2 [Lp], zero-padded; and which entries are real."""
    p = "_gating_fn._qi_partial_module."
    W1, b1, W2, b2 = (w[p + key].float() for key in ("1.weight", "1.bias", "3.weight", "3.bias"))
    H, L = W1.shape
    Lp, Hp = k["Lp"], k["Hp"]
    packs = []
    for real in (False, True):
        W1p, W2p, b1p, b2p = torch.zeros(Hp, Lp), torch.zeros(Lp, Hp), torch.zeros(Hp), torch.zeros(Lp)
        W1p[:H, :L], W2p[:L, :H], b1p[:H], b2p[:L] = (1, 1, 1, 1) if real else (W1, W2, b1, b2)
        lane, j = torch.arange(64).view(1, 1, 64, 1), torch.arange(4).view(1, 1, 1, 4)
        t, c = torch.arange(Hp // 32).view(-1, 1, 1, 1), torch.arange(Lp // 8).view(1, -1, 1, 1)
        W1f = W1p[32 * t + (lane & 31), 8 * c + 4 * (lane >> 5) + j]
        lane, j = lane.unsqueeze(0), j.unsqueeze(0)
        t, v, g = torch.arange(Hp // 32).view(-1, 1, 1, 1, 1), torch.arange(Lp // 32).view(1, -1, 1, 1, 1), torch.arange(4).view(1, 1, -1, 1, 1)
        W2f = W2p[32 * v + (lane & 31), 32 * t + j + 8 * g + 4 * (lane >> 5)]
        packs.append(torch.cat([W1f.reshape(-1), W2f.reshape(-1), b1p, b2p]))
    return packs[0], packs[1] != 0


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_pads_are_written_not_assumed(case, dev):
    s = state(*case, dev)
    eng, k, lib = s.eng, s.k, s.eng.lib
    pq, px, d, _ = s.shape
    L, dp, Lq = k["L"], k["dp"], k["Lq"]
    shape = C.byref(eng.shape)
    with torch.inference_mode(), E._on_device(dev):
        # the index: whole 32-item tiles of [P_X][dp] Ex then [Lq] gi
        floats = lib.rails_mol_generic_index_floats(shape, G.N)
        rows_n, row = (G.N + 31) // 32 * 32, px * dp + Lq
        assert floats == rows_n * row
        buf = fenced(floats, dev)
        X = s.X.to(dev).contiguous()
        _lib.check(lib.rails_mol_generic_index_build(shape, C.byref(eng.weights), E._ptr(X), G.N, E._ptr(buf), E._stream()), "rails_mol_generic_index_build")
        torch.cuda.synchronize()
        assert bool((buf[floats:] == FENCE_VALUE).all()), s.name + ": index fence"
        rows = buf[:floats].view(rows_n, row)
        ex = rows[: G.N, : px * dp].reshape(G.N, px, dp)
        assert bits_equal(ex[:, :, :d], s.ex) and bits_equal(rows[: G.N, px * dp : px * dp + L], s.gi), s.name + ": index values"
        assert bool((ex[:, :, d:] == 0).all()), s.name + ": index columns d .. dp"
        assert bool((rows[: G.N, px * dp + L :] == 0).all()), s.name + ": index columns L .. Lq"
        assert bool((rows[G.N :] == 0).all()), s.name + ": index rows n .. 32 tiles"
        assert bits_equal(buf[:floats], s.index.buf), s.name + ": the engine's index"
        # the query pack: per query [P_Q][dp] Eq / tau then [Lq] gq
        floats = lib.rails_mol_generic_query_pack_floats(shape, G.B)
        row = pq * dp + Lq
        assert floats == G.B * row
        buf = fenced(floats, dev)
        q = s.q.to(dev).contiguous()
        _lib.check(lib.rails_mol_generic_query_prologue(shape, C.byref(eng.weights), E._ptr(q), None, G.B, E._ptr(buf), None, None, E._stream()),
                   "rails_mol_generic_query_prologue")
        torch.cuda.synchronize()
        assert bool((buf[floats:] == FENCE_VALUE).all()), s.name + ": query pack fence"
        rows = buf[:floats].view(G.B, row)
        eq = rows[:, : pq * dp].reshape(G.B, pq, dp)
        assert bool(torch.isfinite(eq[:, :, :d]).all()) and bits_equal(rows[:, pq * dp : pq * dp + L], s.gq), s.name + ": query pack values"
        assert bits_equal(eq[:, :, :d], s.eq / torch.tensor(s.cfg.temperature, dtype=torch.float32, device=dev)), s.name + ": Eq / tau"
        assert bool((eq[:, :, d:] == 0).all()), s.name + ": query pack columns d .. dp"
        assert bool((rows[:, pq * dp + L :] == 0).all()), s.name + ": query pack columns L .. Lq"
        assert bits_equal(buf[:floats], s.qpack), s.name + ": the engine's query pack"
        # the gate pack: a permuted copy of the weights, zero in the Hp / Lp pads
        floats = lib.rails_mol_generic_gate_pack_floats(shape)
        want, real = gate_pack_layout(s.w, k)
        assert floats == want.numel() == 2 * k["Hp"] * k["Lp"] + k["Hp"] + k["Lp"]
        buf = fenced(floats, dev)
        _lib.check(lib.rails_mol_generic_pack_gate_weights(shape, C.byref(eng.weights), E._ptr(buf), E._stream()), "rails_mol_generic_pack_gate_weights")
        torch.cuda.synchronize()
        assert bool((buf[floats:] == FENCE_VALUE).all()), s.name + ": gate pack fence"
        got = buf[:floats].cpu()
        assert bool((got[~real] == 0).all()), s.name + ": gate pack pads"
        assert bits_equal(got[real], want[real]) and bits_equal(buf[:floats], eng.gate_pack), s.name + ": gate pack values"


# ---- the scoring kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dense_logits_against_float64_and_the_oracle(case, dev):
    s = state(*case, dev)
    out64, e64 = R.score64(s.cfg, s.w, s.eq, s.ex, s.gq, s.gi)
    within(s.dense, out64, e64, s.name + " logits")
    ref = O.mol_logits(s.cfg, s.w, s.q, s.X.unsqueeze(0))
    worst = float((s.dense.cpu() - ref).abs().max())
    print(f"{s.name} logits against the oracle: max |err| = {worst:.3g} (LOGIT_TOL {LOGIT_TOL:.3g})")
    assert worst <= LOGIT_TOL, (s.name, worst)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_explaining_launches_against_float64(case, dev):
    s = state(*case, dev)
    (cl64, ecl), (pi64, epi), (out64, eout) = s.explained
    L, K = s.k["L"], G.N_CAND
    rows = torch.arange(G.B).unsqueeze(1)
    with torch.inference_mode():
        eng = s.eng
        cidx = eng.build_index(s.X.to(dev)[s.at.to(dev)].reshape(G.B * K, -1))
        for what, (out, cl, pi) in (("explain_candidates", explain_into(eng, s.qpack, G.B, cidx, K)),
                                    ("explain_indexed", explain_into(eng, s.qpack, G.B, s.index, K, s.pos))):
            tag = f"{s.name} {what}"
            within(cl, cl64[rows, s.at], ecl[rows, s.at], tag + " cl")
            within(pi, pi64[rows, s.at], epi[rows, s.at], tag + " pi")
            within(out, out64[rows, s.at], eout[rows, s.at], tag + " out")
            assert bool(torch.isfinite(pi).all()) and pi.shape == (G.B, K, L), tag
            got, want, bound = pi.cpu().double().sum(-1), pi64[rows, s.at].sum(-1), epi[rows, s.at].sum(-1)
            print(f"{tag} sum pi: max |err| / bound = {float(((got - want).abs() / bound).max()):.3g}")
            assert bool(((got - want).abs() <= bound).all()), tag + " sum pi"
            # the explaining engine wrappers (unwritten outputs of their own): the same launch, the same bits
            own = eng.explain_candidates(s.qpack, G.B, cidx, K) if what == "explain_candidates" else eng.explain_indexed(s.qpack, G.B, s.index, s.pos.to(dev))
            assert bits_equal(own[0], out) and bits_equal(own[1], cl) and bits_equal(own[2], pi), tag


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_launch_form_has_the_dense_bits(case, dev):
    s = state(*case, dev)
    K, ld = G.N_CAND, G.N_CAND + 9
    with torch.inference_mode():
        eng = s.eng
        assert bool(torch.isfinite(s.dense).all()), s.name
        assert bits_equal(eng.score_dense(s.qpack, G.B, s.index), s.dense), s.name
        want = torch.gather(s.dense, 1, s.at.to(dev))
        cidx = eng.build_index(s.X.to(dev)[s.at.to(dev)].reshape(G.B * K, -1))
        assert bits_equal(eng.score_candidates(s.qpack, G.B, cidx, K), want), s.name + ": per-row candidates"
        assert bits_equal(eng.score_indexed(s.qpack, G.B, s.index, s.pos.to(dev)), want), s.name + ": score_indexed"
        counts = torch.tensor([0, 33, K - 1], dtype=torch.int32, device=dev)
        wide = torch.full((G.B, ld), FENCE_VALUE, device=dev)
        eng.score_indexed_rows(s.qpack, G.B, s.index.buf, G.N, s.pos.to(dev), counts=counts, out=wide[:, :K])
        live = torch.arange(K, device=dev)[None, :] < counts[:, None]
        assert bits_equal(wide[:, :K][live], want[live]), s.name + ": score_indexed_rows, live slots"
        assert bool((wide[:, :K][~live] == FENCE_VALUE).all()) and bool((wide[:, K:] == FENCE_VALUE).all()), s.name + ": score_indexed_rows, dead slots"
        assert bits_equal(explain_into(eng, s.qpack, G.B, cidx, K)[0], want), s.name + ": explain_candidates' logit"
        assert bits_equal(explain_into(eng, s.qpack, G.B, s.index, K, s.pos)[0], want), s.name + ": explain_indexed's logit"


# ---- several units per workgroup ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.PERSISTENT, ids=G.name_of)
def test_a_workgroups_later_units_have_the_first_units_bits(shape, dev, n_cu):
    """B = 32 rows over N items with more than 2 x grid units, the last block ragged: every workgroup of the persistent loop takes at least
    two units.  The same items scored in slices that each fit one grid (no workgroup takes a second unit) give the same bits; those launches
    are what the float64 tests above hold to account."""
    cfg, w, k = G.config(shape), G.weights(shape, "plain"), G.launch(shape)
    batch, grid = 32, G.max_grid(shape, n_cu)
    n = 128 * ((2 * grid + 1 + 31) // 32) + 5
    assert G.units(batch, n) > 2 * grid and G.grid(shape, batch, n, n_cu) == grid
    per = 128 * (grid // batch)
    assert per > 0 and G.units(batch, per) <= grid
    q, X = G.raw_inputs(shape, batch, n)
    mol = build_module(cfg, w, dev)
    L = k["L"]
    with torch.inference_mode():
        eng = mol.engine()
        assert eng.route == "generic"
        qpack, _, _ = eng.query_pack(q.to(dev), None)
        index = eng.build_index(X.to(dev))
        dense = torch.full((batch, n), NAN, device=dev)
        eng.score_dense(qpack, batch, index, out=dense)
        pos = torch.arange(n, dtype=torch.int64, device=dev).unsqueeze(0).expand(batch, -1).contiguous()
        out, cl, pi = explain_into(eng, qpack, batch, index, n, pos)
        assert bool(torch.isfinite(dense).all()) and bool(torch.isfinite(cl).all()) and bool(torch.isfinite(pi).all()), G.name_of(shape)
        assert bits_equal(out, dense), G.name_of(shape)
        slices = 0
        for lo in range(0, n, per):
            hi = min(lo + per, n)
            assert G.units(batch, hi - lo) == G.grid(shape, batch, hi - lo, n_cu)      # one unit per workgroup
            part = torch.full((batch, hi - lo), NAN, device=dev)
            eng.score_dense(qpack, batch, index.items(lo, hi), out=part)
            assert bits_equal(part, dense[:, lo:hi]), (G.name_of(shape), "score_dense", lo, hi)
            o, c, p = explain_into(eng, qpack, batch, index, hi - lo, pos[:, lo:hi].contiguous())
            assert bits_equal(o, out[:, lo:hi]), (G.name_of(shape), "explain_indexed logit", lo, hi)
            assert bits_equal(c, cl[:, lo:hi]), (G.name_of(shape), "explain_indexed cl", lo, hi)
            assert bits_equal(p, pi[:, lo:hi]), (G.name_of(shape), "explain_indexed pi", lo, hi)
            slices += 1
        assert slices >= 3 and (n - lo) % 128 == 5
    print(f"{G.name_of(shape)}: n_cu {n_cu}, grid {grid}, units {G.units(batch, n)}, N {n}, {slices} slices of {per} items, L {L}")
