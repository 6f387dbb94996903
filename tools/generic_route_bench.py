#!/usr/bin/env python3
"""Times the shape-generic fp32 scoring route (rails_mol_generic_*) at the amzn-books corpus size, N = 695 762, B = 1 and 32:
the dense scoring kernel and a whole CandidateIndex.get_top_k_outputs step (k = 200, no history) for three shapes that only the
generic route runs, and 8x8x32 / H = 128 forced through the generic route next to its fused fp32 kernel in the same process.

Warm-up launches first, then the median of per-launch device times (CUDA events around each launch, the stream drained before each).
  python tools/generic_route_bench.py [--out profiles/generic_route.json] [--items 695762] [--reps 15]
--candidates: instead, MoLAvgTopK1000 / MoLNaiveTopK5 / MoLCombTopK5_200 on a candidate-capable generic engine (generic_candidates = True)
against the same shape's brute-force step, 4x4x64 and 16x8x32 / H = 256, medians of 20 calls -> profiles/generic_candidates.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import rails_amd  # noqa: E402
from oracle import mol_oracle as O  # noqa: E402

SHAPES = {
    "4x4x64_h128": O.MoLConfig(64, 64, 64, 4, 4),
    "16x8x32_h256": O.MoLConfig(64, 64, 32, 16, 8, gating_qi_hidden_dim=256),
    "32x8x16_h128": O.MoLConfig(64, 64, 16, 32, 8),
}
FUSED = ("8x8x32_h128", O.CONFIGS["amzn-books"])


def module(cfg, dev, route=None):
    w = O.synthetic_weights(cfg, seed=0)
    mol, _ = rails_amd.create_mol_interaction_module(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups, cfg.item_dot_product_groups,
        cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim, cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim,
        cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False, query_nonlinearity=cfg.query_nonlinearity)
    mol.load_state_dict(w, strict=True)
    mol = mol.to(dev).eval()
    mol.route = route
    return mol


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def measure(cfg, dev, route, n_items, reps):
    mol = module(cfg, dev, route)
    X = torch.from_numpy(O.hash_item_table(1, 0, n_items, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(n_items, dtype=torch.int64, device=dev).unsqueeze(0)
    out = {}
    with torch.inference_mode():
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids, exact_mode="dense")
        ci = rails_amd.CandidateIndex(ids=ids, embeddings=X)
        eng = tk._bind()
        out["route"] = eng.route
        for B in (1, 32):
            q = O.synthetic_queries(cfg, B, seed=2).to(dev)
            qpack, _, _ = eng.query_pack(q)
            logits = torch.empty((B, n_items), dtype=torch.float32, device=dev)
            med, lo, hi = median_ms(lambda: eng.score_dense(qpack, B, tk._index, out=logits), reps)
            smed, slo, shi = median_ms(lambda: ci.get_top_k_outputs(q, 200, {}, tk, None), reps)
            out[f"B{B}"] = {"score_dense_ms": round(med, 4), "score_dense_min_max_ms": [round(lo, 4), round(hi, 4)],
                            "top_k_step_ms": round(smed, 4), "top_k_step_min_max_ms": [round(slo, 4), round(shi, 4)]}
    del tk, ci, X
    torch.cuda.empty_cache()
    return out


CANDIDATE_SHAPES = ("4x4x64_h128", "16x8x32_h256")
CANDIDATE_ALGORITHMS = ("MoLAvgTopK1000", "MoLNaiveTopK5", "MoLCombTopK5_200")


def measure_candidates(cfg, dev, n_items, reps):
    """The two-pass algorithms on a candidate-capable generic engine (generic_candidates = True) against the same shape's brute-force step:
    whole CandidateIndex.get_top_k_outputs calls (k = 200, no history), medians of `reps` calls."""
    mol = module(cfg, dev)
    mol.generic_candidates = True

    class Model:      # what get_top_k_module reads
        _ndp_module = mol

    X = torch.from_numpy(O.hash_item_table(1, 0, n_items, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(n_items, dtype=torch.int64, device=dev).unsqueeze(0)
    ci = rails_amd.CandidateIndex(ids=ids, embeddings=X)
    out = {}
    with torch.inference_mode():
        eng = mol.engine()
        out["route"], out["table_width"] = eng.route, eng.table_width
        for name in ("MoLBruteForceTopK",) + CANDIDATE_ALGORITHMS:
            tk = rails_amd.MoLBruteForceTopK(mol, X, ids, exact_mode="dense") if name == "MoLBruteForceTopK" else rails_amd.get_top_k_module(name, Model, X, ids)
            row = {}
            for B in (1, 32):
                q = O.synthetic_queries(cfg, B, seed=2).to(dev)
                med, lo, hi = median_ms(lambda: ci.get_top_k_outputs(q, 200, {}, tk, None), reps)
                row[f"B{B}"] = {"top_k_step_ms": round(med, 4), "top_k_step_min_max_ms": [round(lo, 4), round(hi, 4)]}
            out[name] = row
            print(" ", name, json.dumps(row), flush=True)
            del tk
            torch.cuda.empty_cache()
        for name in CANDIDATE_ALGORITHMS:
            out[name]["brute_force_over_it"] = {b: round(out["MoLBruteForceTopK"][b]["top_k_step_ms"] / out[name][b]["top_k_step_ms"], 1) for b in ("B1", "B32")}
    del ci, X
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--items", type=int, default=695762)
    ap.add_argument("--reps", type=int, default=None, help="timed calls per figure (default 15; 20 with --candidates)")
    ap.add_argument("--candidates", action="store_true", help="time MoLAvgTopK1000 / MoLNaiveTopK5 / MoLCombTopK5_200 on the generic route "
                    "(generic_candidates = True) against the brute-force step; default output profiles/generic_candidates.json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.candidates:
        reps = args.reps or 20
        res = {"device": torch.cuda.get_device_name(0), "n_items": args.items, "k": 200, "reps": reps, "what": "median ms of whole "
               "CandidateIndex.get_top_k_outputs calls, no history; brute force = MoLBruteForceTopK(exact_mode='dense') on the same engine", "shapes": {}}
        for name in CANDIDATE_SHAPES:
            print(name, flush=True)
            res["shapes"][name] = measure_candidates(SHAPES[name], dev, args.items, reps)
        print(json.dumps(res, indent=1))
        with open(args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "generic_candidates.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    args.reps = args.reps or 15
    res = {"device": torch.cuda.get_device_name(0), "n_items": args.items, "k": 200, "reps": args.reps, "exact_mode": "dense", "shapes": {}}
    for name, cfg in SHAPES.items():
        res["shapes"][name] = measure(cfg, dev, None, args.items, args.reps)
        print(name, json.dumps(res["shapes"][name]), flush=True)
    name, cfg = FUSED
    fused = measure(cfg, dev, None, args.items, args.reps)
    forced = measure(cfg, dev, "generic", args.items, args.reps)
    assert fused["route"] == "fused" and forced["route"] == "generic"
    res["shapes"][name + "_fused"], res["shapes"][name + "_forced_generic"] = fused, forced
    res["generic_over_fused_8x8x32"] = {b: round(forced[b]["score_dense_ms"] / fused[b]["score_dense_ms"], 2) for b in ("B1", "B32")}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
