#!/usr/bin/env python3
"""What score_of / explain_of cost on MoLBruteForceTopK (default mode), amzn-books geometry (N = 695 762, synthetic
weights, hashed item table), B = 32, 61 seen ids per row (half of each row's own top-200, zero padding: bench.py's list), T = 100 / 1 000 /
4 000 random item ids per row -- and, from the same run, what the two dense routes to the same numbers cost:
  score_of               the whole call: the id lookup, the in-place scoring of the B T positions, the eligibility launch
  explain_of             the whole call: that, the gather of the B T raw rows, their per-row generic index, the explaining launch
  all_logits + gather    the dense fp32 pass over the corpus and a torch gather of the B T entries (no seen ids: all_logits takes none)
  log_prob_of            the dense pass, the normaliser's two reads and the target read
One timing = one call between two device events, the second waited for (one synchronise behind the warm-ups, none between timings);
per cell --calls timings after --warmup calls, the cells interleaved call by call so that they share the clocks; medians in microseconds.
Writes profiles/score_of.json (or --out) and prints it as one JSON line.  Reads nothing outside the repository.
  python tools/score_of_bench.py [--calls 20] [--warmup 3] [--items 695762] [--out PATH]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, default=695_762)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_of.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "score_of_bench needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(9)
    n, B, width = args.items, 32, 61
    result = {"box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"calls_per_cell": args.calls, "warmup_calls_per_cell": args.warmup, "n_items": n, "batch": B, "seen_width": width,
                           "unit": "us per call, device events, median; the cells interleaved call by call", "runs": 1}}
    with torch.inference_mode():
        X = E.hash_item_table(1, 0, n, cfg.item_embedding_dim, dev).unsqueeze(0)
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
        q = O.synthetic_queries(cfg, B).to(dev)
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
        _, top_ids = tk(q, k=200)
        inv = torch.zeros((B, width), dtype=torch.int64, device=dev)      # bench.py's seen ids
        for b in range(B):
            sel = torch.randperm(top_ids.shape[1], generator=g)[: width // 2].to(dev)
            inv[b, : width // 2] = top_ids[b, sel]
        cells, agree = {}, {}
        for t in (100, 1000, 4000):
            pos = torch.randint(0, n, (B, t), generator=g).to(dev)
            target = ids[0, pos].contiguous()
            label = f"T = {t}"
            cells[f"score_of, {label}"] = (lambda target=target: tk.score_of(q, target, invalid_ids=inv))
            cells[f"explain_of, {label}"] = (lambda target=target: tk.explain_of(q, target, invalid_ids=inv))
            cells[f"all_logits + gather, {label}"] = (lambda pos=pos: tk.all_logits(q).gather(1, pos))
            cells[f"log_prob_of, {label}"] = (lambda target=target: tk.log_prob_of(q, target, invalid_ids=inv))
            got = tk.score_of(q, target)
            agree[f"score_of == all_logits gathered, {label}"] = bool(torch.equal(got, tk.all_logits(q).gather(1, pos)))
            agree[f"explain_of.logits == score_of, {label}"] = bool(torch.equal(tk.explain_of(q, target).logits, got))
        result["agreement"] = agree
        for _ in range(args.warmup):
            for call in cells.values():
                call()
        torch.cuda.synchronize()
        us = {label: [] for label in cells}
        for _ in range(args.calls):
            for label, call in cells.items():
                us[label].append(timed(call, 1))
        result["cells"] = {label: {"us": v, "us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)} for label, v in us.items()}
        result["stats"] = tk.pair_stats()
    result["not_measured"] = ["kernel-level times (only whole calls between events)", "more than one run: these are first figures, no bar was set in advance",
                              "other geometries, batch sizes or seen widths", "the approximate modules, MIPSBruteForceTopK and the generic route",
                              "restricted calls (hidden set, item_mask=, allowed_tags=)"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
