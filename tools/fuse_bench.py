#!/usr/bin/env python3
"""What query fusion costs on MoLBruteForceTopK (default mode), amzn-books geometry (N = 695 762, synthetic weights,
hashed item table), U = 32 users x m = 1 / 2 / 4 / 8 sub-queries, k = 120, bench.py's 61-wide seen list per user.  Per m:
  get_top_k_outputs max, list route     the S = 32 m sub-query rows through the module's own forward (k' = 181), the id lookup, one merge launch
  get_top_k_outputs max, matrix route   forced (FUSE_LIST_MAX_ENTRIES = 0): the dense fp32 pass on S rows, the fuse launch, the fused selection
  get_top_k_outputs sum                 the matrix route
  plain get_top_k_outputs, S rows       the yardstick, from the same run: the unfused call on the S sub-query rows (seen lists repeated per row)
  scores_fuse_rows max / sum            engine.scores_fuse_rows alone on an (S, N) matrix already there: (S + U) N 4 bytes moved
  topk_fuse_lists                       engine.topk_fuse_lists alone on (S, k') lists already there
One timing = one call between two device events behind a device synchronise; per cell --calls timings after --warmup calls, the cells
interleaved call by call so that they share the clocks; medians in microseconds.
Writes profiles/query_fusion.json (or --out) and prints it as one JSON line.  Reads nothing outside the repository.
  python tools/fuse_bench.py [--calls 20] [--warmup 3] [--items 695762] [--out PATH]
--candidates: the same protocol for fusion over the candidate union on the approximate modules (fuse_candidates = True): MoLAvgTopK1000,
MoLNaiveTopK5 and MoLCombTopK5_200; per m the fused get_top_k_outputs with max and sum, the plain get_top_k_outputs of the same module on the S
sub-query rows (what a caller runs today before merging by hand), engine.lists_union alone on MoLNaiveTopK5's candidates, and the exact
module's fused call (what fusion costs today); and, per module, the device kernels one fused call and one plain S-row call launch, counted
under torch.profiler.  Writes profiles/query_fusion_candidates.json.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rails_amd  # noqa: E402
from oracle import mol_oracle as O  # noqa: E402
from rails_amd import engine as E  # noqa: E402
from tools.item_mask_bench import build_mol, timed  # noqa: E402


def kernels_launched(call):
    """Device kernels one call launches (torch.profiler's device events whose name is no memcpy / memset); None where the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        call()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        return sum(1 for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()) or None
    except Exception:      # (a box without a working tracer: the timings do not depend on it)
        return None


def candidates_main(args):
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(9)
    n, users, width, k = args.items, 32, 61, 120
    makers = {"MoLAvgTopK1000": lambda x, i: rails_amd.MoLAvgTopK(mol, x, i, avg_top_k=1000),
              "MoLNaiveTopK5": lambda x, i: rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=5),
              "MoLCombTopK5_200": lambda x, i: rails_amd.MoLCombTopK(mol, x, i, avg_top_k=200, k_per_group=5)}
    result = {"box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"calls_per_cell": args.calls, "warmup_calls_per_cell": args.warmup, "n_items": n, "users": users, "seen_width": width, "k": k,
                           "unit": "us per call, device events, median; the cells of one m interleaved call by call"},
              "cells": {}, "kernels_launched": {}, "fused_candidate_calls": {}}
    with torch.inference_mode():
        X = E.hash_item_table(1, 0, n, cfg.item_embedding_dim, dev).unsqueeze(0)
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
        cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
        exact = rails_amd.MoLBruteForceTopK(mol, X, ids)
        modules = {name: make(X, ids) for name, make in makers.items()}
        for tk in modules.values():
            tk.fuse_candidates = True
        for m in (1, 2, 4, 8):
            rows = users * m
            q = O.synthetic_queries(cfg, rows, seed=3 + m).to(dev)
            lims = torch.arange(0, rows + 1, m, dtype=torch.int64, device=dev)
            _, top_ids = exact(q, k=200, query_lims=lims)
            inv = torch.zeros((users, width), dtype=torch.int64, device=dev)      # bench.py's seen ids, per user
            for u in range(users):
                sel = torch.randperm(top_ids.shape[1], generator=g)[: width // 2].to(dev)
                inv[u, : width // 2] = top_ids[u, sel]
            inv_rows = inv.repeat_interleave(m, dim=0).contiguous()
            naive_pos = modules["MoLNaiveTopK5"].positions_of(modules["MoLNaiveTopK5"](q, k=1)[1].reshape(-1)).view(rows, -1).contiguous()
            cells = {"exact module, get_top_k_outputs max": lambda: cand.get_top_k_outputs(q, k, {"query_lims": lims}, exact, inv),
                     "lists_union alone (MoLNaiveTopK5's candidates)": lambda: E.lists_union(naive_pos, lims, n)}
            for name, tk in modules.items():
                cells[f"{name}: fused get_top_k_outputs max"] = lambda tk=tk: cand.get_top_k_outputs(q, k, {"query_lims": lims}, tk, inv)
                cells[f"{name}: fused get_top_k_outputs sum"] = lambda tk=tk: cand.get_top_k_outputs(q, k, {"query_lims": lims, "fuse": "sum"}, tk, inv)
                cells[f"{name}: plain get_top_k_outputs, S rows"] = lambda tk=tk: cand.get_top_k_outputs(q, k, {}, tk, inv_rows)
            for _ in range(args.warmup):
                for call in cells.values():
                    call()
            torch.cuda.synchronize()
            us = {label: [] for label in cells}
            for _ in range(args.calls):
                for label, call in cells.items():
                    us[label].append(timed(call, 1))
            out = {label: {"us": v, "us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)} for label, v in us.items()}
            for name in modules:
                out[f"{name}: fused max / plain S rows"] = (out[f"{name}: fused get_top_k_outputs max"]["us_median"]
                                                            / out[f"{name}: plain get_top_k_outputs, S rows"]["us_median"])
            result["cells"][f"m = {m}"] = out
            result["kernels_launched"][f"m = {m}"] = {
                name: {"fused max": kernels_launched(cells[f"{name}: fused get_top_k_outputs max"]),
                       "plain S rows": kernels_launched(cells[f"{name}: plain get_top_k_outputs, S rows"])} for name in modules}
        result["fused_candidate_calls"] = {name: tk.stats() for name, tk in modules.items()}
    result["not_measured"] = ["kernel-level times (only whole calls between events)", "other geometries, user counts, k or seen widths", "ragged segments",
                              "query_weights=", "allowed_tags= and a hidden set under a fused call", "a 125 M-item shard"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, default=695_762)
    ap.add_argument("--candidates", action="store_true", help="fusion over the candidate union on the approximate modules")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "query_fusion_candidates.json" if args.candidates else "query_fusion.json")
    assert torch.cuda.is_available(), "fuse_bench needs a GPU"
    if args.candidates:
        return candidates_main(args)
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(9)
    n, users, width, k = args.items, 32, 61, 120
    result = {"box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"calls_per_cell": args.calls, "warmup_calls_per_cell": args.warmup, "n_items": n, "users": users, "seen_width": width, "k": k,
                           "unit": "us per call, device events, median; the cells of one m interleaved call by call"},
              "cells": {}, "agreement": {}, "routes": {}}
    with torch.inference_mode():
        X = E.hash_item_table(1, 0, n, cfg.item_embedding_dim, dev).unsqueeze(0)
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
        cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
        for m in (1, 2, 4, 8):
            tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
            forced = rails_amd.MoLBruteForceTopK(mol, X, ids)
            forced.FUSE_LIST_MAX_ENTRIES = 0
            rows = users * m
            q = O.synthetic_queries(cfg, rows, seed=3 + m).to(dev)
            lims = torch.arange(0, rows + 1, m, dtype=torch.int64, device=dev)
            fused_kw = {"query_lims": lims}
            _, top_ids = tk(q, k=200, **fused_kw)
            inv = torch.zeros((users, width), dtype=torch.int64, device=dev)      # bench.py's seen ids, per user
            for u in range(users):
                sel = torch.randperm(top_ids.shape[1], generator=g)[: width // 2].to(dev)
                inv[u, : width // 2] = top_ids[u, sel]
            inv_rows = inv.repeat_interleave(m, dim=0).contiguous()
            k_prime = min(k + width, n)
            scores = tk.all_logits(q).clone()
            list_s, list_i = tk(q, k=k_prime)
            list_s, list_p = list_s.clone(), tk.positions_of(list_i.reshape(-1)).view(rows, k_prime)
            cells = {
                "get_top_k_outputs max, list route": lambda: cand.get_top_k_outputs(q, k, dict(fused_kw), tk, inv),
                "get_top_k_outputs max, matrix route": lambda: cand.get_top_k_outputs(q, k, dict(fused_kw), forced, inv),
                "get_top_k_outputs sum": lambda: cand.get_top_k_outputs(q, k, dict(fused_kw, fuse="sum"), tk, inv),
                "plain get_top_k_outputs, S rows": lambda: cand.get_top_k_outputs(q, k, {}, tk, inv_rows),
                "scores_fuse_rows max": lambda: E.scores_fuse_rows(scores, lims, "max"),
                "scores_fuse_rows sum": lambda: E.scores_fuse_rows(scores, lims, "sum"),
                "topk_fuse_lists": lambda: E.topk_fuse_lists(list_s, list_p, lims, k, ids[0], inv),
            }
            a, b = cells["get_top_k_outputs max, list route"](), cells["get_top_k_outputs max, matrix route"]()
            result["agreement"][f"m = {m}: list route == matrix route"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
            for _ in range(args.warmup):
                for call in cells.values():
                    call()
            torch.cuda.synchronize()
            us = {label: [] for label in cells}
            for _ in range(args.calls):
                for label, call in cells.items():
                    us[label].append(timed(call, 1))
            out = {label: {"us": v, "us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)} for label, v in us.items()}
            for label in ("scores_fuse_rows max", "scores_fuse_rows sum"):
                out[label]["bytes_moved"] = (rows + users) * n * 4
                out[label]["bytes_per_s"] = out[label]["bytes_moved"] / (out[label]["us_median"] * 1e-6)
            out["topk_fuse_lists"]["bytes_moved"] = rows * k_prime * 12 + users * (width * 8 + k * 12)
            out["list route / plain S rows"] = out["get_top_k_outputs max, list route"]["us_median"] / out["plain get_top_k_outputs, S rows"]["us_median"]
            out["matrix route / plain S rows"] = out["get_top_k_outputs max, matrix route"]["us_median"] / out["plain get_top_k_outputs, S rows"]["us_median"]
            result["cells"][f"m = {m}"] = out
            result["routes"][f"m = {m}"] = {"list module": {key: v for key, v in tk.stats().items() if isinstance(v, (int, float))}, "matrix module": {key: v for key, v in forced.stats().items() if key.startswith("fused_")}}
    result["not_measured"] = ["kernel-level times (only whole calls between events)", "other geometries, user counts, k or seen widths", "ragged segments",
                              "query_weights=", "the streaming calls under query_lims= (they cost their unfused form on S rows plus the fuse launch)",
                              "MIPSBruteForceTopK and the other routes"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
