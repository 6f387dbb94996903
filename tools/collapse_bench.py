#!/usr/bin/env python3
"""What collapse_groups=True costs: CandidateIndex.get_top_k_outputs(k = 120) with bench.py's seen-id list (width 61: half
of each row's own top-200, zero padding) on MoLBruteForceTopK (default mode) and MoLAvgTopK1000, amzn-books geometry (N = 695 762, synthetic
weights, hashed item table), B = 32.  Cells: no groups (the plain call -- unchanged code, the yardstick of the same run), all items ungrouped,
random groups of mean size 4 and 32, and a Zipf layout whose largest group holds 10 % of the corpus.  One timing = one call between two device
events behind a device synchronise; per cell --calls timings after --warmup calls, the cells of a module interleaved call by call so that they
share the clocks; the median is reported in microseconds with the cell's walk_redos and fallbacks (collapse_stats) over the timed calls.
Writes profiles/collapse.json (or --out) and prints it as one JSON line.  Reads nothing outside the repository.
  python tools/collapse_bench.py [--calls 20] [--warmup 30] [--items 695762] [--out PATH]
--max-per-group: the quota leg instead.  Per module and layout with groups, the cells collapse_groups=True (the yardstick of the same run) and
max_per_group = 1, 2, 4, 8 on ONE module holding the layout's key row; same geometry, seen ids and protocol, all cells of a module interleaved
call by call; per cell the median, its ratio to the collapse_groups=True cell of its layout, and the walk_redos / fallbacks of its timed
calls.  Writes profiles/group_quota.json (or --out).
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

MODULES = {
    "MoLBruteForceTopK": lambda mol, x, i: rails_amd.MoLBruteForceTopK(mol, x, i),
    "MoLAvgTopK1000": lambda mol, x, i: rails_amd.MoLAvgTopK(mol, x, i, avg_top_k=1000),
}


def layouts(n, g):
    """name -> (n,) int64 keys on the CPU (None: no groups, the plain call)"""
    zipf = torch.empty(n, dtype=torch.int64)
    zipf[: n // 10] = 0                                        # the largest group: 10 % of the corpus ...
    lo, key, size = n // 10, 1, n // 10
    while lo < n:                                              # ... then groups of size ~ 1 / rank of it
        size = max(1, (n // 10) // (key + 1))
        zipf[lo : lo + size] = key
        lo, key = lo + size, key + 1
    zipf = zipf[torch.randperm(n, generator=g)]
    return {
        "no groups": None,
        "all ungrouped": torch.full((n,), -1, dtype=torch.int64),
        "random, mean size 4": torch.randint(0, n // 4, (n,), generator=g),
        "random, mean size 32": torch.randint(0, n // 32, (n,), generator=g),
        "zipf, largest 10 %": zipf,
    }


QUOTAS = (1, 2, 4, 8)


def quota_cells(make, mol, X, ids, keys, dev):
    """label -> (module, call kwargs): per layout with groups one module, five cells on it"""
    cells = {}
    for label, row in keys.items():
        if row is None:
            continue
        tk = make(mol, X, ids)
        tk.set_item_groups(row.to(dev))
        cells[f"{label} | collapse_groups=True"] = (tk, {"collapse_groups": True})
        for m in QUOTAS:
            cells[f"{label} | max_per_group={m}"] = (tk, {"max_per_group": m})
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--items", type=int, default=695_762)
    ap.add_argument("--max-per-group", action="store_true", help="the quota leg: max_per_group = 1, 2, 4, 8 against collapse_groups=True")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "group_quota.json" if args.max_per_group else "collapse.json")
    assert torch.cuda.is_available(), "collapse_bench needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(6)
    n, B, k, kp, width = args.items, 32, 120, 200, 61
    result = {"box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"calls_per_cell": args.calls, "warmup_calls_per_cell": args.warmup, "n_items": n, "batch": B, "k": k, "seen_width": width,
                           "unit": "us per get_top_k_outputs call, device events, median; the cells of a module interleaved call by call"},
              "modules": {}}
    with torch.inference_mode():
        X = E.hash_item_table(1, 0, n, cfg.item_embedding_dim, dev).unsqueeze(0)
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
        q = O.synthetic_queries(cfg, B).to(dev)
        cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
        keys = layouts(n, g)
        for name, make in MODULES.items():
            cells = {}
            for label, row in keys.items():      # one module per cell: each holds its own key row
                if args.max_per_group and row is not None:
                    continue
                tk = make(mol, X, ids)
                if row is not None:
                    tk.set_item_groups(row.to(dev))
                cells[label] = (tk, {} if row is None else {"collapse_groups": True})
            _, top_ids = cells["no groups"][0](q, k=kp)
            if args.max_per_group:
                cells.update(quota_cells(make, mol, X, ids, keys, dev))
            inv = torch.zeros((B, width), dtype=torch.int64, device=dev)      # bench.py's seen ids
            for b in range(B):
                sel = torch.randperm(top_ids.shape[1], generator=g)[: width // 2].to(dev)
                inv[b, : width // 2] = top_ids[b, sel]
            call = lambda tk, kw: cand.get_top_k_outputs(q, k, kw, tk, inv, truncate_k_prime_to=kp)      # noqa: E731
            for _ in range(args.warmup):
                for tk, kw in cells.values():
                    call(tk, kw)
            torch.cuda.synchronize()
            us = {label: [] for label in cells}
            took = {label: {"calls": 0, "walk_redos": 0, "fallbacks": 0} for label in cells}      # (the quota leg's cells share modules: counted call by call)
            for _ in range(args.calls):
                for label, (tk, kw) in cells.items():
                    before = tk.collapse_stats()
                    us[label].append(timed(lambda: call(tk, kw), 1))
                    after = tk.collapse_stats()
                    for key in took[label]:
                        took[label][key] += after[key] - before[key]
            rows = {}
            plain = statistics.median(us["no groups"])
            for label in cells:
                med = statistics.median(us[label])
                rows[label] = {"us": us[label], "us_median": med, "over_plain": med / plain, **took[label]}
                if args.max_per_group and " | " in label:
                    rows[label]["over_collapse_groups"] = med / statistics.median(us[label.split(" | ")[0] + " | collapse_groups=True"])
            result["modules"][name] = rows
            del cells
            torch.cuda.empty_cache()
    result["not_measured"] = ["kernel-level times of the walk and of the group-maxima pass (only whole calls)", "other geometries, batch sizes, k or seen widths",
                              "the cost of set_item_groups (one torch.unique over the key row)", "COLLAPSE_DEPTH_FACTOR / COLLAPSE_MAX_DEPTH other than the defaults"]
    if args.max_per_group:
        result["not_measured"] = ["the m-round exact fallback (rails_scores_group_next: one pass over the scores per round) and the depth doubling under a quota, "
                                  "unless a cell's fallbacks / walk_redos say it took them", "max_per_group beyond 8",
                                  "kernel-level times of the walk with a quota (only whole calls)", "other geometries, batch sizes, k or seen widths",
                                  "COLLAPSE_DEPTH_FACTOR / COLLAPSE_MAX_DEPTH other than the defaults"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
