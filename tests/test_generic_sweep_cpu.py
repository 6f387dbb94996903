"""CPU: the shape sweep of the generic scoring route (tests/_generic_sweep.py) and the bars it is held to, proved without a device.

  * coverage: the launch formulas restated in tests/_generic_sweep.py put the sweep on all 13 (TL, RES) pairs a shape inside the envelope
    can select; an enumeration of Hp shows that the other three cannot occur; every limit of the envelope and every padded axis is met
  * every sweep shape is inside the generic envelope and has no fused kernel (the library answers without a device)
  * the meta-test: on every sweep shape an fp32 emulation of the pair arithmetic stays inside explain64's bars, and a mutant that drops
    the last query block, the tail of d, the tail of H, or that runs the softmax over a padded width (Lp or Lq) exceeds them by a factor
    of 10 on cl, pi or out -- the bars tests/test_generic_sweep_gpu.py applies would see each of these bugs

Figures of one run (max |err| / bound over cl, pi, out; B = 3, N = 131):
  emulation                 at most 0.49 (cl of 7x9x3 / H 300) on every shape and weight set
  q_block                   at least 2.2e4 (6x11x256), plain weights, all 19 shapes
  d_tail                    at least 4.1e5 (40x2x20), plain weights, the 15 shapes with d % 8 != 0
  hid_tail                  at least 42 (2x1x1 / H 1; 91 on 6x11x256 / H 40, above 6 000 elsewhere), plain weights, the 10 shapes with H % 32 != 0
  padded_softmax (Lp)       plain weights: below 10 on 11 of the 16 shapes with L % 32 != 0 (0.007 on 7x9x3 / H 300, 0.04 on 51x5x9):
                            the bars do not see it there; flat gate: at least 15.7 (51x5x9) on all 16
  padded_softmax_lq (Lq)    flat gate: at least 15.7 (51x5x9, where Lq = Lp) on the 12 shapes with L % 4 != 0
"""
import ctypes as C
import os

import pytest

from rails_amd import _lib
from rails_amd import engine as E
from tests import _explain_ref as X
from tests import _generic_sweep as G
from tests._generic_fixtures import spec_of
from tests.test_score_of_cpu import worst

FACTOR = 10.0      # the factor of tests/test_score_of_cpu.py


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- coverage -------------------------------------------------------------------------------------------------------------------------------
def reachable_pairs():
    """Every (TL, res) some (L, H) inside the envelope selects: L <= 256, H <= 512, by the restated formula."""
    pairs = set()
    for tl in range(1, 9):
        for hp in range(32, 512 + 1, 32):
            pairs.add((tl, 512 * 32 * tl + 8 * hp * 32 * tl <= G.MAX_LDS))
    return pairs


def test_the_sweep_reaches_every_reachable_instantiation():
    reach = reachable_pairs()
    assert reach == {(tl, True) for tl in range(1, 7)} | {(tl, False) for tl in range(2, 9)} and len(reach) == 13
    for never in ((1, False), (7, True), (8, True)):
        assert never not in reach
    got = {}
    for shape in G.SWEEP:
        k = G.launch(shape)
        got.setdefault((k["TL"], k["res"]), []).append(G.name_of(shape))
    for (tl, res), names in sorted(got.items()):
        print(f"TL {tl} {'resident' if res else 'streamed'}: {', '.join(names)}")
    assert set(got) == reach


def test_the_sweep_meets_every_limit_and_padded_axis():
    ks = {shape: G.launch(shape) for shape in G.SWEEP}
    assert len(set(G.SWEEP)) == len(G.SWEEP) == 19
    assert {k["L"] % 4 for k in ks.values()} == {0, 1, 2, 3}
    assert any(pq > 32 and pq % 32 for pq, _, _, _ in G.SWEEP) and any(pq == 256 for pq, _, _, _ in G.SWEEP) and any(px > 32 for _, px, _, _ in G.SWEEP)
    assert sum(1 for _, _, d, _ in G.SWEEP if d % 8) >= 8 and sum(1 for _, _, _, h in G.SWEEP if h % 32) >= 8
    assert max(d for _, _, d, _ in G.SWEEP) == 256 and max(h for _, _, _, h in G.SWEEP) == 512 and max(k["L"] for k in ks.values()) == 256
    assert min(d for _, _, d, _ in G.SWEEP) == 1 and min(h for _, _, _, h in G.SWEEP) == 1
    assert (16, 16, 256, 512) in ks      # every limit at once
    # the LDS boundary, met with equality from both sides of TL, and one hidden unit past it
    at = [s for s, k in ks.items() if k["res"] and k["lds"] == G.MAX_LDS]
    assert {ks[s]["TL"] for s in at} == {4, 5}, at
    assert ks[(9, 13, 7, 96)]["res"] and not ks[(9, 13, 7, 97)]["res"]
    # N = 131: a second 128-item block of 3 items; 45 candidates: a second wave tile of 13
    assert G.units(G.B, G.N) == 2 * G.B and G.N % 128 == 3 and G.N_CAND % 32 == 13
    # the persistent shapes: two at two workgroups per CU, one at the LDS boundary, one streamed
    mult = [G.max_grid(s, 1) for s in G.PERSISTENT]
    assert mult == [2, 2, 1, 1] and ks[G.PERSISTENT[2]]["lds"] == G.MAX_LDS and not ks[G.PERSISTENT[3]]["res"]
    assert all(s in ks for s in G.PERSISTENT)
    assert [G.table_width(d) for d in (1, 7, 32, 33, 64, 65, 72, 128, 129, 256)] == [32, 32, 32, 64, 64, 128, 128, 128, 0, 0]


def test_every_sweep_shape_is_generic_only(lib):
    for shape in G.SWEEP:
        cfg = G.config(shape)
        s = spec_of(cfg, E).to_c()
        assert lib.rails_mol_generic_supported(C.byref(s)) == 1, (shape, _lib.last_error())
        assert lib.rails_mol_shape_supported(C.byref(s)) == 0, shape
        k = G.launch(shape)
        pq, px, d, h = shape
        assert lib.rails_mol_generic_gate_pack_floats(C.byref(s)) == 2 * k["Hp"] * k["Lp"] + k["Hp"] + k["Lp"], shape
        assert lib.rails_mol_generic_index_floats(C.byref(s), G.N) == 160 * (px * k["dp"] + k["Lq"]), shape
        assert lib.rails_mol_generic_query_pack_floats(C.byref(s), G.B) == G.B * (pq * k["dp"] + k["Lq"]), shape
        assert int(lib.rails_mol_generic_table_width(C.byref(s))) == G.table_width(d), shape


def test_the_table_shapes_are_generic_only_and_meet_every_width(lib):
    """The synthetic shapes tests/test_generic_candidates_gpu.py cuts the two-pass tables from: widths 32, 64, 128 (d below the width and d
    equal to it) and a shape with no table."""
    widths = []
    for shape in tuple(G.TABLE_SHAPES.values()) + (G.NO_TABLE,):
        s = spec_of(G.config(shape), E).to_c()
        assert lib.rails_mol_generic_supported(C.byref(s)) == 1 and lib.rails_mol_shape_supported(C.byref(s)) == 0, shape
        widths.append(int(lib.rails_mol_generic_table_width(C.byref(s))))
        assert widths[-1] == G.table_width(shape[2]), shape
    assert widths == [32, 64, 128, 128, 0] and G.TABLE_SHAPES["s_2x3x128"][2] == 128


# ---- the meta-test --------------------------------------------------------------------------------------------------------------------------
def applies(mut, shape):
    """Does the mutant change anything on this shape?"""
    pq, px, d, h = shape
    L = pq * px
    return {"q_block": True, "d_tail": d % 8 != 0, "hid_tail": h % 32 != 0, "padded_softmax": L % 32 != 0, "padded_softmax_lq": L % 4 != 0}[mut]


# mutant -> the weight set it is judged on
MUTANTS = {"q_block": "plain", "d_tail": "plain", "hid_tail": "plain", "padded_softmax": "flat", "padded_softmax_lq": "flat"}


def ratios(shape, kind, mut=None):
    cfg, w = G.config(shape), G.weights(shape, kind)
    ins = G.operands(shape, kind)
    (cl, ecl), (pi, epi), (out, eout) = X.explain64(cfg, w, *ins)
    g_cl, g_pi, g_out = X.emulate32(cfg, w, *ins, mut=mut)
    return {"cl": worst(g_cl, (cl, ecl))[0], "pi": worst(g_pi, (pi, epi))[0], "out": worst(g_out, (out, eout))[0]}


def fmt(r):
    return " ".join(f"{k} {v:.3g}" for k, v in r.items())


@pytest.mark.parametrize("shape", G.SWEEP, ids=G.name_of)
def test_the_bars_pass_the_emulation_and_reject_every_mutant(shape):
    name = G.name_of(shape)
    for kind in G.KINDS:
        good = ratios(shape, kind)
        print(f"{name} {kind}: emulation, max |err| / bound: {fmt(good)}")
        assert max(good.values()) <= 1.0, (name, kind, good)
    seen = 0
    for mut, kind in MUTANTS.items():
        if not applies(mut, shape):
            continue
        r = ratios(shape, kind, mut)
        print(f"{name} {kind}: mutant {mut}, max |err| / bound: {fmt(r)}")
        assert max(r.values()) >= FACTOR, (name, mut, kind, r)
        seen += 1
        if mut == "padded_softmax":      # what the plain set would have seen of it: printed, not asserted (the reason for the flat set)
            print(f"{name} plain: mutant {mut}, max |err| / bound: {fmt(ratios(shape, 'plain', mut))}")
    assert seen >= 1


def test_every_mutant_is_judged_somewhere():
    for mut in MUTANTS:
        assert sum(applies(mut, s) for s in G.SWEEP) >= 8, mut
