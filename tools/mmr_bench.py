#!/usr/bin/env python3
"""What diversify=lam costs and what it buys: CandidateIndex.get_top_k_outputs(k = 120) with bench.py's seen-id list (width
61: half of each row's own top-200, zero padding) on MoLBruteForceTopK (default mode) and MoLAvgTopK1000, amzn-books geometry (N = 695 762,
synthetic weights, hashed item table), B = 32, lam = 0.7.  Cells per module: the plain call (unchanged code, the yardstick of the same run) and
the diversified call for every pool size D in {240, 480, 1024} and vector width E in {32, 64, 256} (clustered unit vectors); beside each
diversified cell the walk alone, engine.topk_mmr on a ranked list of D + 61 entries taken once.  One timing = one call between two device
events behind a device synchronise; per cell --calls timings after --warmup calls, the cells of one E interleaved call by call so that they
share the clocks; medians in microseconds.  Per cell also engine.list_similarity of the result lists (mean pairwise dot product of the returned
items' vectors, averaged over the batch), plain against diversified.  Writes profiles/mmr.json (or --out) and prints it as one JSON line.
Reads nothing outside the repository.
  python tools/mmr_bench.py [--calls 20] [--warmup 3] [--items 695762] [--out PATH]
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
POOLS = (240, 480, 1024)
DIMS = (32, 64, 256)
LAM = 0.7


def clustered_unit_vectors(n, dim, g, dev, clusters=64):
    """items near one of `clusters` centres, normalised: a result list of 120 items holds several near-duplicates of most of its members, the
    slate diversify= is for (the vectors are independent of the scores: what a plain top-k returns is a random draw of the clusters)"""
    centres = torch.randn(clusters, dim, generator=g).to(dev)
    which = torch.randint(0, clusters, (n,), generator=g).to(dev)
    v = centres[which] + 0.3 * torch.randn(n, dim, generator=g).to(dev)
    return v / torch.linalg.vector_norm(v, dim=1, keepdim=True).clamp_min(1e-12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, default=695_762)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mmr_bench needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(6)
    n, B, k, kp, width = args.items, 32, 120, 200, 61
    result = {"box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"calls_per_cell": args.calls, "warmup_calls_per_cell": args.warmup, "n_items": n, "batch": B, "k": k, "seen_width": width, "lam": LAM,
                           "unit": "us per call, device events, median; the cells of one vector width interleaved call by call",
                           "vectors": "unit vectors: one of 64 Gaussian centres per item plus 0.3 x Gaussian noise, independent of the scores",
                           "similarity": "engine.list_similarity: mean pairwise dot product of the returned items' unit vectors, mean over the batch"},
              "modules": {}}
    with torch.inference_mode():
        X = E.hash_item_table(1, 0, n, cfg.item_embedding_dim, dev).unsqueeze(0)
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)      # (id = position + 1)
        q = O.synthetic_queries(cfg, B).to(dev)
        cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
        vectors = {dim: clustered_unit_vectors(n, dim, g, dev) for dim in DIMS}
        for name, make in MODULES.items():
            tk = make(mol, X, ids)
            _, top_ids = tk(q, k=kp)
            inv = torch.zeros((B, width), dtype=torch.int64, device=dev)      # bench.py's seen ids
            for b in range(B):
                sel = torch.randperm(top_ids.shape[1], generator=g)[: width // 2].to(dev)
                inv[b, : width // 2] = top_ids[b, sel]
            call = lambda kw: cand.get_top_k_outputs(q, k, kw, tk, inv, truncate_k_prime_to=kp)      # noqa: E731
            rows = {}
            for dim in DIMS:
                tk.set_item_vectors(vectors[dim])
                cells = {"plain": lambda: call({})}
                for D in POOLS:
                    cells[f"diversify, D = {D}"] = (lambda D: lambda: call({"diversify": LAM, "diversity_pool": D}))(D)
                    with tk._positions_as_ids():      # the walk alone: a ranked list of D + width entries, taken once
                        ls, lp = tk(q, k=1000 if "Avg" in name else D + width)      # (MoLAvgTopK1000 walks its 1 000 reranked candidates)
                    word = torch.zeros(1, dtype=torch.int32, device=dev)
                    cells[f"walk alone, D = {D}"] = (lambda D, ls, lp: lambda: E.topk_mmr(ls, lp, tk.item_vectors, LAM, k, D, tk._ids_flat, inv, word))(D, ls, lp)
                for _ in range(args.warmup):
                    for fn in cells.values():
                        fn()
                torch.cuda.synchronize()
                us = {label: [] for label in cells}
                for _ in range(args.calls):
                    for label, fn in cells.items():
                        us[label].append(timed(fn, 1))
                plain = statistics.median(us["plain"])
                plain_sim = float(E.list_similarity(cells["plain"]()[0] - 1, vectors[dim]).mean())
                out = {}
                for label, fn in cells.items():
                    med = statistics.median(us[label])
                    out[label] = {"us": us[label], "us_median": med, "over_plain": med / plain}
                    if label.startswith("diversify"):
                        out[label]["list_similarity"] = float(E.list_similarity(fn()[0] - 1, vectors[dim]).mean())
                    if label.startswith("walk alone"):
                        out[label]["us_per_step"] = med / k
                out["plain"]["list_similarity"] = plain_sim
                rows[f"E = {dim}"] = out
            result["modules"][name] = rows
            del tk
            torch.cuda.empty_cache()
    result["not_measured"] = ["kernel-level times from a profiler (the walk alone is a whole engine call between device events, allocation of its outputs included)",
                              "other geometries, batch sizes, k, lam or seen widths", "the cost of set_item_vectors", "real item vectors (these are synthetic clusters)"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
