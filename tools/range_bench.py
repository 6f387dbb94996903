#!/usr/bin/env python3
"""What count_above / range_search cost on MoLBruteForceTopK (default mode), amzn-books geometry (N = 695 762, synthetic
weights, hashed item table), B = 32, 61 seen ids per row (half of each row's own top-200, zero padding: bench.py's list), per-row thresholds
taken from the row's own scores so that about 100 / about 10 000 items pass:
  count_above            the whole call: id lookups, the per-row mask copy, the dense fp32 pass, the count and offsets launches
  range_search           the whole call, sorted and unsorted: that, the lims read-back, the write pass, the per-row sort, the decode
  scores_range           count / offsets / read-back / write / sort / decode alone (engine.scores_range on a score matrix already there)
  rank_of, scores_rank   beside them, from the same run, T = 1: the other streaming consumer of the same matrix, as the yardstick
One timing = one call between two device events behind a device synchronise; per cell --calls timings after --warmup calls, the cells
interleaved call by call so that they share the clocks; medians in microseconds.
Writes profiles/range_search.json (or --out) and prints it as one JSON line.  Reads nothing outside the repository.
  python tools/range_bench.py [--calls 20] [--warmup 3] [--items 695762] [--out PATH]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_search.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "range_bench needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(9)
    n, B, width = args.items, 32, 61
    result = {"box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"calls_per_cell": args.calls, "warmup_calls_per_cell": args.warmup, "n_items": n, "batch": B, "seen_width": width,
                           "unit": "us per call, device events, median; the cells interleaved call by call"}}
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
        words = E.visibility_row(n, dev).repeat(B, 1)
        E.item_mask_clear_rows(words, tk.positions_of(inv.reshape(-1)).view(B, -1), n)
        pos = tk.positions_of(target.reshape(-1)).view(B, 1)
        cells = {"rank_of, T = 1": lambda: tk.rank_of(q, target, invalid_ids=inv), "scores_rank, T = 1": lambda: E.scores_rank(scores, pos, words)}
        hits = {}
        for want in (100, 10_000):
            want = min(want, n)
            thr = E.topk(scores, want)[0][:, -1].contiguous()             # every row's want-th largest score
            label = f"~{want} hits"
            hits[label] = tk.count_above(q, thr, invalid_ids=inv).tolist()
            cells[f"count_above, {label}"] = (lambda thr=thr: tk.count_above(q, thr, invalid_ids=inv))
            cells[f"range_search sorted, {label}"] = (lambda thr=thr: tk.range_search(q, thr, invalid_ids=inv))
            cells[f"range_search unsorted, {label}"] = (lambda thr=thr: tk.range_search(q, thr, invalid_ids=inv, sort=False))
            cells[f"scores_range sorted, {label}"] = (lambda thr=thr: E.scores_range(scores, thr, words, ids=ids[0]))
            cells[f"scores_range_count, {label}"] = (lambda thr=thr: E.scores_range_count(scores, thr, words))
            # the sorted rows are the filtered top-k's head
            lims, _, got = tk.range_search(q, thr, invalid_ids=inv)
            c0 = int(lims[1])
            cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
            head = cand.get_top_k_outputs(q, min(c0, 2500), {}, tk, inv)[0][0]
            result.setdefault("agreement", {})[f"range_search row 0 == get_top_k_outputs' first ids, {label}"] = bool(torch.equal(got[: head.numel()], head))
        result["hits_per_row"] = hits
        for _ in range(args.warmup):
            for call in cells.values():
                call()
        torch.cuda.synchronize()
        us = {label: [] for label in cells}
        for _ in range(args.calls):
            for label, call in cells.items():
                us[label].append(timed(call, 1))
        result["cells"] = {label: {"us": v, "us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)} for label, v in us.items()}
        for label in cells:
            if label.startswith("scores_range_count"):
                result["cells"][label]["score_bytes_per_s"] = B * n * 4 / (result["cells"][label]["us_median"] * 1e-6)
    result["not_measured"] = ["kernel-level times (only whole calls between events)",
                              "whether the write pass's second read of the 89 MB matrix is served from the 256 MB last-level cache",
                              "the log-probability form (it adds log_partition's two reads)", "other geometries, batch sizes, hit counts or seen widths",
                              "MIPSBruteForceTopK and the other routes"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
