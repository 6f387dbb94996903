#!/usr/bin/env python3
"""Calls of the approximate modules with a hidden set beside the same module with nothing hidden: amzn-books geometry
(N = 695 762, synthetic weights, hashed item table), B = 32, forward(k = 10) of MoLAvgTopK (K' = 200 / 4 000), MoLNaiveTopK (k_g = 5 / 100) and
MoLCombTopK (k_g = 100, K' = 1 000), with 0 %, one item, 1 %, 10 %, 50 % and 90 % of the corpus hidden at random.
  0 %        nothing hidden: the module holds no visibility row and runs the unmasked launches (the same kernel symbols as before the feature);
  one item   the visible kernels over all but one item: against the 0 % row, what the hidden-aware sample and select scans cost by themselves;
  90 %       below hidden_scan_route's fraction: the materialising route (scores of every item, hidden columns set to -inf, rails_topk).
One timing = --steps calls between two device events; the hidden module and its twin with nothing hidden are interleaved round by round
(--rounds), the median over the rounds is reported in microseconds per call.  Then hide_items of 1 000 random positions (and the unhide_items
that undoes it) beside remove_items of the same positions on a module with every buffer built: wall time around a device synchronisation,
--edit-rounds fresh removals.  Writes profiles/hidden_items.json (or --out) and prints it as one JSON line.
  python tools/hidden_items_bench.py [--steps 10] [--rounds 5] [--warmup 2] [--edit-rounds 3] [--out PATH]
"""
import argparse
import json
import os
import platform
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rails_amd  # noqa: E402
from oracle import mol_oracle as O  # noqa: E402
from rails_amd import engine as E  # noqa: E402
from tools.item_mask_bench import build_mol, timed  # noqa: E402

ALGORITHMS = {
    "MoLAvgTopK200": lambda mol, x, i: rails_amd.MoLAvgTopK(mol, x, i, avg_top_k=200),
    "MoLAvgTopK4000": lambda mol, x, i: rails_amd.MoLAvgTopK(mol, x, i, avg_top_k=4000),
    "MoLNaiveTopK5": lambda mol, x, i: rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=5),
    "MoLNaiveTopK100": lambda mol, x, i: rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=100),
    "MoLCombTopK100_1000": lambda mol, x, i: rails_amd.MoLCombTopK(mol, x, i, avg_top_k=1000, k_per_group=100),
}
SHARES = (("0 %", 0.0), ("one item", None), ("1 %", 0.01), ("10 %", 0.10), ("50 %", 0.50), ("90 %", 0.90))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--edit-rounds", type=int, default=3)
    ap.add_argument("--items", type=int, default=695_762)
    ap.add_argument("--algorithms", default=",".join(ALGORITHMS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hidden_items.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hidden_items_bench needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(5)
    n, B, k = args.items, 32, 10
    result = {"box": {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"steps_per_timing": args.steps, "rounds": args.rounds, "warmup_calls": args.warmup, "n_items": n, "batch": B, "k": k,
                           "unit": "us per forward call, device events; hidden module and its twin with nothing hidden interleaved"},
              "algorithms": {}}
    with torch.inference_mode():
        X = E.hash_item_table(1, 0, n, cfg.item_embedding_dim, dev).unsqueeze(0)
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
        q = O.synthetic_queries(cfg, B).to(dev)
        order = torch.randperm(n, generator=g)
        for name in args.algorithms.split(","):
            plain, tk = ALGORITHMS[name](mol, X, ids), ALGORITHMS[name](mol, X, ids)
            rows = {}
            for label, share in SHARES:
                if tk.num_hidden:
                    tk.unhide_items(tk.hidden_positions())
                m = 1 if share is None else int(n * share)
                if m:
                    tk.hide_items(order[:m])
                for _ in range(args.warmup):
                    plain(q, k=k)
                    tk(q, k=k)
                us = {"hidden": [], "nothing_hidden": []}
                for _ in range(args.rounds):
                    us["nothing_hidden"].append(timed(lambda: plain(q, k=k), args.steps))
                    us["hidden"].append(timed(lambda: tk(q, k=k), args.steps))
                med = {key: statistics.median(v) for key, v in us.items()}
                rows[label] = {"num_hidden": tk.num_hidden, "us": us, "us_median": med, "hidden_minus_nothing_hidden_us": med["hidden"] - med["nothing_hidden"],
                               "ratio": med["hidden"] / med["nothing_hidden"]}
            result["algorithms"][name] = rows
            del plain, tk
            torch.cuda.empty_cache()
        # hide_items against remove_items, 1 000 positions, every buffer of MoLAvgTopK200 built
        pos = order[:1000].contiguous()
        edits = {"hide_items": [], "unhide_items": [], "remove_items": []}
        tk = ALGORITHMS["MoLAvgTopK200"](mol, X, ids)
        tk(q, k=k)
        for _ in range(args.edit_rounds + 1):      # (the first round warms the kernels and the allocator up and is dropped)
            edits["hide_items"].append(wall(lambda: tk.hide_items(pos))[0])
            edits["unhide_items"].append(wall(lambda: tk.unhide_items(pos))[0])
        del tk
        for _ in range(args.edit_rounds + 1):
            victim = ALGORITHMS["MoLAvgTopK200"](mol, X, ids)
            victim(q, k=k)
            edits["remove_items"].append(wall(lambda: victim.remove_items(pos))[0])
            del victim
            torch.cuda.empty_cache()
        result["edits_1000_positions"] = {key: {"us": v[1:], "us_median": statistics.median(v[1:])} for key, v in edits.items()}
        result["edits_1000_positions"]["unit"] = "us wall time per call, device synchronised before and after; MoLAvgTopK200 with its index, row copy and coarse table built"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
