#!/usr/bin/env python3
"""What the softmax over the corpus costs on MoLBruteForceTopK (default mode), amzn-books geometry (N = 695 762, synthetic
weights, hashed item table), B = 32, 61 seen ids per row (half of each row's own top-200, zero padding: bench.py's list):
  log_partition      the whole call: id lookups, the per-row mask copy, the dense fp32 pass, the max / sum / finish launches
  log_prob_of        T = 1 target per row: the same, plus the gather
  sample_items       S = 120 draws per row: the dense pass, the Gumbel pass, the exact top-k of the perturbed matrix, the lse and the gather
  rank_of            T = 1, beside them from the same run, for scale (section 3.17)
  scores_lse         the four launches alone, on a score matrix already there with the per-row mask
  scores_gumbel      the perturbation alone, into a buffer already there
One timing = one call between two device events behind a device synchronise; per cell --calls timings after --warmup calls, the cells
interleaved call by call so that they share the clocks; medians in microseconds.  Also reports the effective rates of the two kernels-only
cells (the score matrix's bytes over the call's time: two reads for scores_lse, a read and a write for scores_gumbel -- upper bounds of the
kernels' own times, not a kernel trace).
Writes profiles/softmax.json (or --out) and prints it as one JSON line.  Reads nothing outside the repository.
  python tools/softmax_bench.py [--calls 20] [--warmup 3] [--items 695762] [--out PATH]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "softmax_bench needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(8)
    n, B, width, draws, seed = args.items, 32, 61, min(120, args.items), 0x1234567887654321
    result = {"box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"calls_per_cell": args.calls, "warmup_calls_per_cell": args.warmup, "n_items": n, "batch": B, "seen_width": width,
                           "num_samples": draws, "temperature": 1.0, "unit": "us per call, device events, median; the cells interleaved call by call"}}
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
        target = ids[0, torch.randint(0, n, (B, 1), generator=g).to(dev)].contiguous()
        scores = tk.all_logits(q).clone()
        noisy = torch.empty_like(scores)
        words = E.visibility_row(n, dev).repeat(B, 1)
        E.item_mask_clear_rows(words, tk.positions_of(inv.reshape(-1)).view(B, -1), n)
        cells = {"log_partition": lambda: tk.log_partition(q, invalid_ids=inv),
                 "log_prob_of, T = 1": lambda: tk.log_prob_of(q, target, invalid_ids=inv),
                 f"sample_items, S = {draws}": lambda: tk.sample_items(q, draws, seed, invalid_ids=inv),
                 "rank_of, T = 1": lambda: tk.rank_of(q, target, invalid_ids=inv),
                 "scores_lse": lambda: E.scores_lse(scores, words),
                 "scores_gumbel": lambda: E.scores_gumbel(scores, seed, 0, words, out=noisy)}
        # the calls agree with each other: the draws' log-probabilities are log_prob_of's, and the module's normaliser is the kernels'
        s_ids, s_lp = tk.sample_items(q, draws, seed, invalid_ids=inv)
        result["agreement"] = {"sample_items' log_probs == log_prob_of(its ids)": bool(torch.equal(s_lp, tk.log_prob_of(q, s_ids, invalid_ids=inv))),
                               "log_partition == scores_lse(all_logits)": bool(torch.equal(tk.log_partition(q, invalid_ids=inv), E.scores_lse(scores, words)))}
        for _ in range(args.warmup):
            for call in cells.values():
                call()
        torch.cuda.synchronize()
        us = {label: [] for label in cells}
        for _ in range(args.calls):
            for label, call in cells.items():
                us[label].append(timed(call, 1))
        result["cells"] = {label: {"us": v, "us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)} for label, v in us.items()}
        for label in ("scores_lse", "scores_gumbel"):      # both move the matrix's bytes twice
            result["cells"][label]["matrix_bytes_per_s"] = 2 * B * n * 4 / (result["cells"][label]["us_median"] * 1e-6)
        result["stats"] = {key: v for key, v in tk.stats().items() if key in ("calls", "proved_calls", "fallbacks")}
    result["not_measured"] = ["kernel-level times (only whole calls between events)", "other geometries, batch sizes, temperatures, sample counts or seen widths",
                              "MIPSBruteForceTopK and the other routes"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
