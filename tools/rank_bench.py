#!/usr/bin/env python3
"""What rank_of costs on MoLBruteForceTopK (default mode), amzn-books geometry (N = 695 762, synthetic weights, hashed item
table), B = 32, 61 seen ids per row (half of each row's own top-200, zero padding: bench.py's list), T = 1 and 16 targets per row:
  rank_of            the whole call: id lookups, the per-row mask copy, the dense fp32 pass, the key / count / finish launches
  scores_rank        the key / zero / count / finish launches alone (engine.scores_rank on a score matrix already there, with the per-row mask)
  get_top_k_outputs  beside them, from the same run: the accuracy protocol's top-k call (k = 2 500, k' = 2 561) of the same module
One timing = one call between two device events behind a device synchronise; per cell --calls timings after --warmup calls, the cells
interleaved call by call so that they share the clocks; medians in microseconds.  Also reports the count's effective read rate (the score
matrix's bytes over the scores_rank time -- an upper bound of the count kernel's own time, not a kernel trace).
Writes profiles/rank_of.json (or --out) and prints it as one JSON line.  Reads nothing outside the repository.
  python tools/rank_bench.py [--calls 20] [--warmup 3] [--items 695762] [--out PATH]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_of.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rank_bench needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(8)
    n, B, k, width = args.items, 32, min(2500, args.items), 61
    result = {"box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"calls_per_cell": args.calls, "warmup_calls_per_cell": args.warmup, "n_items": n, "batch": B, "seen_width": width, "top_k": k,
                           "unit": "us per call, device events, median; the cells interleaved call by call"}}
    with torch.inference_mode():
        X = E.hash_item_table(1, 0, n, cfg.item_embedding_dim, dev).unsqueeze(0)
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
        q = O.synthetic_queries(cfg, B).to(dev)
        cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
        _, top_ids = tk(q, k=200)
        inv = torch.zeros((B, width), dtype=torch.int64, device=dev)      # bench.py's seen ids
        for b in range(B):
            sel = torch.randperm(top_ids.shape[1], generator=g)[: width // 2].to(dev)
            inv[b, : width // 2] = top_ids[b, sel]
        targets = ids[0, torch.randint(0, n, (B, 16), generator=g).to(dev)].contiguous()
        scores = tk.all_logits(q).clone()
        words = E.visibility_row(n, dev).repeat(B, 1)
        E.item_mask_clear_rows(words, tk.positions_of(inv.reshape(-1)).view(B, -1), n)
        cells = {"get_top_k_outputs": lambda: cand.get_top_k_outputs(q, k, {}, tk, inv)}
        for t in (1, 16):
            tgt = targets[:, :t].contiguous()
            pos = tk.positions_of(tgt.reshape(-1)).view(B, t)
            cells[f"rank_of, T = {t}"] = (lambda tgt=tgt: tk.rank_of(q, tgt, invalid_ids=inv))
            cells[f"scores_rank, T = {t}"] = (lambda pos=pos: E.scores_rank(scores, pos, words))
        # the two paths agree where both can answer: the filtered top-k's ids rank 1 .. k
        top = cand.get_top_k_outputs(q, k, {}, tk, inv)[0]
        ranks = tk.rank_of(q, top[:, :64].contiguous(), invalid_ids=inv)
        result["agreement"] = {"rank_of(top-64 ids of get_top_k_outputs) == 1 .. 64": bool(torch.equal(ranks.cpu(), torch.arange(1, 65).expand(B, -1)))}
        for _ in range(args.warmup):
            for call in cells.values():
                call()
        torch.cuda.synchronize()
        us = {label: [] for label in cells}
        for _ in range(args.calls):
            for label, call in cells.items():
                us[label].append(timed(call, 1))
        result["cells"] = {label: {"us": v, "us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)} for label, v in us.items()}
        for t in (1, 16):
            med = result["cells"][f"scores_rank, T = {t}"]["us_median"]
            result["cells"][f"scores_rank, T = {t}"]["score_bytes_per_s"] = B * n * 4 / (med * 1e-6)
        result["stats"] = {key: v for key, v in tk.stats().items() if key in ("calls", "proved_calls", "fallbacks")}
    result["not_measured"] = ["kernel-level times (only whole calls between events)", "other geometries, batch sizes, target counts or seen widths",
                              "MIPSBruteForceTopK and the other routes"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
