"""CPU: score_of / explain_of without a device.

  * tests/_explain_ref.py against the reference's own fp32 stages: explain64 on F1/Eq, F1/Ex, F1/gq, F1/gi with the fixture weights
    reproduces F1/cl, F1/pi and F1/logits inside its bounds on all four configs (the figures are printed: how far the bounds lie above).
  * the meta-test: an fp32 emulation of the explaining kernel's pair arithmetic passes the bars, and every mutant of it fails them by a factor
    of at least 10 in some entry of the same inputs.
  * header, binding and library agree on the new entry points under ABI 15; their argument checks return before any launch.
  * every refusal names the class and the argument.
"""
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch

import rails_amd
from rails_amd import _lib, sharded
from rails_amd import engine as E
from rails_amd import topk_modules as T
from tests import _explain_ref as X
from tests import _mol_ref64 as R
from tests._fixtures import PER_CONFIG, Fixture
from tests._generic_fixtures import generic_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rails_mol_generic_explain", "rails_mol_generic_explain_indexed", "rails_scores_at_eligible", "rails_mips_score_indexed")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def f1_inputs(fx):
    return fx.t("F1/Eq"), fx.t("F1/Ex")[0], fx.t("F1/gq"), fx.t("F1/gi")[0]


def worst(got, ref_and_bound):
    ref, bound = ref_and_bound
    err = (got.double().reshape(ref.shape) - ref).abs()
    return float((err / bound).max()), float(err.max())


# ---- the reference against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PER_CONFIG)
def test_explain64_reproduces_the_reference_stages(name):
    fx = Fixture(name)
    cl, pi, out = X.explain64(fx.cfg, fx.weights, *f1_inputs(fx))
    pi, out = (pi[0], pi[1]), (out[0], out[1])
    for what, got, ref in (("cl", fx.t("F1/cl"), cl), ("pi", fx.t("F1/pi"), pi), ("logits", fx.t("F1/logits"), out)):
        ratio, err = worst(got, ref)
        rel = float(((got.double() - ref[0]).abs() / ref[0].abs().clamp(min=1e-300)).max())
        print(f"{name} {what}: max |F1 - ref64| = {err:.3g} (relative {rel:.3g}), max |err| / bound = {ratio:.3g}: the bound lies {1 / ratio:.3g} x above")
        assert ratio <= 1.0, (name, what, ratio)
    s = pi[0].sum(-1)
    assert float((s - 1).abs().max()) < 1e-12 and float(pi[0].min()) > 0


# ---- the meta-test -----------------------------------------------------------------------------------------------------------------------
def meta_inputs():
    """(name, cfg, weights, Eq, Ex, gq, gi): the F1 inputs of c1 (L = 32) and the 12x3x20 / H = 50 shape off the fused grid (L = 36: not a
    multiple of 32, so a softmax over the padded logits shows), its gate rows from the float64 prologue / index build."""
    fx = Fixture("c1_ml1m")
    yield ("c1_ml1m", fx.cfg, fx.weights) + f1_inputs(fx)
    name, cfg, w, a = next(c for c in generic_cases() if c[0].startswith("g_12x3x20"))
    (_, _), (gq, _) = R.prologue64(cfg, w, a["q"], a.get("user_ids"))
    (_, _), (gi, _) = R.index64(cfg, w, a["X"][0])
    yield name, cfg, w, a["Eq"], a["Ex"].reshape(-1, *a["Ex"].shape[-2:]), gq.float(), gi.float()


MUTANTS = ("transposed", "no_tau", "padded_softmax", "no_renorm", "silu_gqgi", "pi_before_den")


def ratios(cfg, w, ins, mut=None, eps=None):
    """max |emulation - float64| / bound over the three outputs; with eps the reference is renormalised by it, as the combiner does."""
    (cl, ecl), (pi, epi), (out, eout) = X.explain64(cfg, w, *ins)
    if eps is not None:
        scale = 1.0 / max(1.0, R.f32(eps))
        pi, epi, out, eout = pi * scale, epi * scale, out * scale, eout * scale
    g_cl, g_pi, g_out = X.emulate32(cfg, w, *ins, mut=mut, eps=eps)
    return {"cl": worst(g_cl, (cl, ecl))[0], "pi": worst(g_pi, (pi, epi))[0], "out": worst(g_out, (out, eout))[0]}


def test_the_bars_pass_the_emulation_and_reject_every_mutant():
    for name, cfg, w, *ins in meta_inputs():
        L = cfg.num_logits
        good = ratios(cfg, w, ins)
        print(f"{name}: emulation, max |err| / bound = {good}")
        assert max(good.values()) <= 1.0, (name, good)
        good2 = ratios(cfg, w, ins, eps=2.0)
        assert max(good2.values()) <= 1.0, (name, "eps = 2", good2)
        for mut in MUTANTS:
            if mut == "padded_softmax" and L % 32 == 0:
                continue      # (nothing is padded)
            if mut == "transposed" and cfg.query_dot_product_groups == cfg.item_dot_product_groups == 1:
                continue
            r = ratios(cfg, w, ins, mut=mut, eps=2.0 if mut == "no_renorm" else None)
            print(f"{name}: mutant {mut}, max |err| / bound = {r}")
            assert max(r.values()) >= 10.0, (name, mut, r)
    # the float64 side's own mutants move the VALUE by more than ten bounds as well (they are what the GPU tests' bars would see)
    name, cfg, w, *ins = next(meta_inputs())
    ref = X.explain64(cfg, w, *ins)
    for mut in ("transposed", "no_tau", "silu_gqgi"):
        got = X.explain64(cfg, w, *ins, mut=mut)
        assert max(worst(got[i][0], ref[i])[0] for i in range(3)) >= 10.0, mut


# ---- the entry points ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_additions_under_abi_15(lib):
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert re.search(r"#define RAILS_ABI_VERSION 15\b", header) and _lib.RAILS_ABI_VERSION == 15 and lib.rails_abi_version() == 15
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
        decl = re.search(r"\bint " + name + r"\s*\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name][1]), name      # as many arguments bound as declared
    src = open(os.path.join(ROOT, "rails_amd", "csrc", "mol_generic.hip")).read()
    assert "bool EXP" in src and "atomic" not in src.split("emit_tile")[1].split("template")[0]
    assert "atomic" not in open(os.path.join(ROOT, "rails_amd", "csrc", "item_mask.hip")).read().split("pairs_eligible_kernel")[1].split("int scores_at_eligible")[0]


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    bad, ok = _lib.RAILS_EINVAL, _lib.RAILS_OK
    # rails_scores_at_eligible(scores, ld, rows, t, positions, n, words, stride, eff, allowed, invalid, width, item_ids, extra_a, extra_b, len, stream)
    e = lib.rails_scores_at_eligible
    assert e(None, 4, 2, 4, 1, 10, None, 0, None, None, None, 0, None, None, None, 0, None) == bad and "NULL" in _lib.last_error()
    assert e(1, 4, 2, 4, None, 10, None, 0, None, None, None, 0, None, None, None, 0, None) == bad and "NULL" in _lib.last_error()
    assert e(1, 3, 2, 4, 1, 10, None, 0, None, None, None, 0, None, None, None, 0, None) == bad and "ld" in _lib.last_error()
    assert e(1, 4, 2, 4, 1, 0, None, 0, None, None, None, 0, None, None, None, 0, None) == bad
    assert e(1, 4, 2, 4, 1, 10, None, 0, 1, None, None, 0, None, None, None, 0, None) == bad and "go together" in _lib.last_error()
    assert e(1, 4, 2, 4, 1, 100, 1, 2, None, None, None, 0, None, None, None, 0, None) == bad and "shorter" in _lib.last_error()
    assert e(1, 4, 2, 4, 1, 10, None, 0, None, None, 1, 3, None, None, None, 0, None) == bad and "item_ids" in _lib.last_error()
    assert e(1, 4, 2, 4, 1, 10, None, 0, None, None, None, 0, None, 1, None, 5, None) == bad and "extra" in _lib.last_error()
    assert e(1, 4, 0, 4, 1, 10, None, 0, None, None, None, 0, None, None, None, 0, None) == ok
    assert e(1, 4, 2, 0, 1, 10, None, 0, None, None, None, 0, None, None, None, 0, None) == ok
    # rails_mips_score_indexed(queries, batch, dim, index, n_items, positions, n_cand, query_ws, logits, ld, stream)
    m = lib.rails_mips_score_indexed
    assert m(1, 2, 8, 1, 10, None, 4, 1, 1, 4, None) == bad and "NULL" in _lib.last_error()
    assert m(1, 2, 8, 1, 10, 1, 4, 1, 1, 3, None) == bad and "ld" in _lib.last_error()
    assert m(1, 2, 8, 1, 0, 1, 4, 1, 1, 4, None) == bad
    assert m(1, 0, 8, 1, 10, 1, 4, 1, 1, 4, None) == ok and m(1, 2, 8, 1, 10, 1, 0, 1, 1, 4, None) == ok
    # the explaining launches: the generic route's envelope first, then sizes and pointers
    s = E.MolShapeSpec(64, 64, 40, 8, 8, 512, 128, 128, 128).to_c()
    x, xi = lib.rails_mol_generic_explain, lib.rails_mol_generic_explain_indexed
    assert x(C.byref(s), 1, 1, 2, 1, 4, 1, 3, 1, 1, None) == bad and "ld" in _lib.last_error()
    assert x(C.byref(s), 1, 1, 2, 1, 4, 1, 4, None, 1, None) == bad and "NULL" in _lib.last_error()
    assert x(C.byref(s), 1, 1, 2, 1, 4, 1, 4, 1, None, None) == bad and "NULL" in _lib.last_error()
    assert x(C.byref(s), 1, 1, 0, 1, 4, 1, 4, 1, 1, None) == ok
    assert xi(C.byref(s), 1, 1, 2, 1, 10, None, 4, 1, 4, 1, 1, None) == bad and "NULL" in _lib.last_error()
    assert xi(C.byref(s), 1, 1, 2, 1, 0, 1, 4, 1, 4, 1, 1, None) == bad and "empty index" in _lib.last_error()
    assert xi(C.byref(s), 1, 1, 2, 1, 10, 1, 0, 1, 4, 1, 1, None) == ok
    one_linear = E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, -1).to_c()
    assert x(C.byref(one_linear), 1, 1, 2, 1, 4, 1, 4, 1, 1, None) == _lib.RAILS_ENOTSUP and "hidden layer" in _lib.last_error()


def test_engine_argument_checks():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.scores_at_eligible(torch.zeros((2, 3)), torch.zeros((2, 3), dtype=torch.int64), 10)
    src = inspect.getsource(E.scores_at_eligible)
    assert src.index("invalid_ids.dim() != 2") < src.index("invalid_ids.shape[1] > 0")      # a 1-D invalid_ids is a ValueError, not an IndexError
    assert list(inspect.signature(E.scores_at_eligible).parameters) == ["scores", "positions", "n_items", "mask", "tags", "invalid_ids", "item_ids", "extras"]
    assert T.Explained._fields == ("logits", "weights", "component_logits")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _bare(cls, **attrs):
    obj = cls.__new__(cls)      # (a refusal reads the type and the kwargs alone: nothing is constructed, nothing is launched)
    obj.__dict__.update(attrs)
    return obj


CALLS = ("score_of", "score_of_positions", "explain_of", "explain_of_positions")
SINGLE = (rails_amd.MoLBruteForceTopK, rails_amd.MoLAvgTopK, rails_amd.MoLNaiveTopK, rails_amd.MoLCombTopK, rails_amd.MIPSBruteForceTopK)


def test_refusals_name_the_class_and_the_argument():
    for cls in SINGLE:
        for call in CALLS:
            if cls is rails_amd.MIPSBruteForceTopK and call.startswith("explain"):
                continue
            for kw, word in (({"query_lims": torch.tensor([0, 1])}, "query_lims"), ({"fuse": "max"}, "fuse"), ({"query_weights": torch.ones(2)}, "query_weights"),
                             ({"collapse_groups": True}, "collapse_groups"), ({"max_per_group": 2}, "max_per_group"), ({"diversify": 0.5}, "diversify"),
                             ({"diversity_pool": 10}, "diversity_pool")):
                with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call} takes no {word}\b"):
                    getattr(_bare(cls), call)(None, None, **kw)
    for cls in (rails_amd.MoLAvgTopK, rails_amd.MoLNaiveTopK, rails_amd.MoLCombTopK):      # item_mask= stays refused where all_logits refuses it
        for call in CALLS:
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call} takes no item_mask\b"):
                getattr(_bare(cls), call)(None, None, item_mask=torch.ones(4, dtype=torch.bool))
    for call in CALLS:      # the IVF module
        with pytest.raises(NotImplementedError, match=rf"^MoLNaiveTopK \(IVF, use_faiss=True\)\.{call}: "):
            getattr(_bare(rails_amd.MoLNaiveTopK, _use_faiss=True), call)(None, None)
    for call in ("explain_of", "explain_of_positions"):      # no mixture on MIPS
        with pytest.raises(NotImplementedError, match=rf"^MIPSBruteForceTopK\.{call}: there is no mixture"):
            getattr(_bare(rails_amd.MIPSBruteForceTopK), call)(None, None)


def test_sharded_wrappers_refuse_by_name():
    src = open(os.path.join(ROOT, "rails_amd", "sharded.py")).read()
    classes = [getattr(sharded, name) for name in re.findall(r"^class (\w+)\(", src, flags=re.M)]
    wrappers = [c for c in classes if issubclass(c, T.TopKModule)]
    assert len(wrappers) >= 6
    for cls in wrappers:
        for call in CALLS:
            with pytest.raises(NotImplementedError, match=rf"^{cls.__name__}\.{call}: .*single-device"):
                getattr(_bare(cls), call)(None, None)


def test_precision_and_envelope_refusals():
    """The helpers the modules call once they hold an engine (a module cannot be constructed without a device)."""
    tk = _bare(rails_amd.MoLBruteForceTopK)
    fp32 = types.SimpleNamespace(precision="fp32", dense_precision="fp32")
    f16x3 = types.SimpleNamespace(precision="f16x3", dense_precision="f16x3")      # (the pack format of every split precision is "f16x3")
    f16x1 = types.SimpleNamespace(precision="f16x3", dense_precision="f16x1")
    for what in CALLS:
        T.refuse_pair_precision(tk, fp32, what)
        with pytest.raises(NotImplementedError, match=rf"^MoLBruteForceTopK\.{what}: precision='f16x1'"):
            T.refuse_pair_precision(tk, f16x1, what)
        if what.startswith("explain_of"):
            with pytest.raises(NotImplementedError, match=rf"^MoLBruteForceTopK\.{what}: precision='f16x3' -- the mixture"):
                T.refuse_pair_precision(tk, f16x3, what)
        else:
            T.refuse_pair_precision(tk, f16x3, what)      # the gather route returns the dense pass's bits there
    err = T.explain_outside_envelope(_bare(rails_amd.MoLAvgTopK), NotImplementedError("the generic scoring route needs a pair gate with a hidden layer"))
    assert isinstance(err, NotImplementedError) and str(err).startswith("MoLAvgTopK.explain_of: ") and "hidden layer" in str(err)
    # the envelope itself is answered without a device: the three one-Linear-gate shapes and the limits of mol_generic.h
    lib = _lib.load()
    for spec, word in ((E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, -1), "hidden layer"), (E.MolShapeSpec(64, 64, 16, 32, 16, 512, 128, 128, 128), "P_Q"),
                       (E.MolShapeSpec(64, 64, 264, 2, 2, 512, 128, 128, 128), "dot_product_dimension"), (E.MolShapeSpec(64, 64, 32, 8, 8, 512, 128, 128, 520), "gating_qi_hidden_dim")):
        assert lib.rails_mol_generic_supported(C.byref(spec.to_c())) == 0 and word in _lib.last_error(), word


def test_argument_checks_come_before_any_launch():
    tk = _bare(rails_amd.MIPSBruteForceTopK)
    q = torch.zeros((2, 4))
    with pytest.raises(ValueError, match=r"score_of: item_ids must be \(2, T\)"):
        tk.score_of(q, torch.zeros((3, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"score_of_positions: positions must be \(2, T\) int64"):
        tk.score_of_positions(q, torch.zeros((2, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="T >= 1"):
        tk.score_of_positions(q, torch.zeros((2, 0), dtype=torch.int64))
    assert tk.pair_stats() == {}
