#!/usr/bin/env python3
"""In-place corpus changes of MoLNaiveTopK(use_faiss=True, frozen_centroids=True) on synthetic amzn-books 8x8x32 (N = 695 762,
nlist = 100): medians of device-event timings of update_items / append_items / remove_items at M in {1, 1 024, 16 384}, next to the two
ways to get the same lists without the edit path, on the same box:
  rebuild       constructing engine.IvfIndex again (train + build): the only route without frozen centroids
  build_lists   rails_ivf_build_lists alone with the kept centroids (IvfIndex(..., centroids=))
The question: does an edit cost about one read plus one write of the lists, independent of nlist * d?  A measuring
tool, not a gate.  Writes profiles/ivf_update.json and prints it.
  python tools/ivf_update_bench.py [--reps 7] [--nlist 100] [--sizes 1,1024,16384] [--out profiles/ivf_update.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import rails_amd  # noqa: E402
from oracle import mol_oracle as O  # noqa: E402   (input generators only)
from rails_amd import engine as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--nlist", type=int, default=100)
ap.add_argument("--sizes", default="1,1024,16384")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_update.json"))
a = ap.parse_args()
dev = torch.device("cuda:0")
cfg_key, N, _ = bench.WORKLOADS["amzn-books"]
cfg = O.CONFIGS[cfg_key]
mol, _ = rails_amd.create_mol_interaction_module(
    cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
    cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
    cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
    query_nonlinearity=cfg.query_nonlinearity)
mol.load_state_dict(O.synthetic_weights(cfg, seed=0), strict=True)
mol = mol.to(dev).eval()
X = torch.from_numpy(O.hash_item_table(1, 0, N, cfg.item_embedding_dim)).to(dev)
ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev)
sizes = [int(s) for s in a.sizes.split(",")]
fresh_rows = torch.from_numpy(O.hash_item_table(2, 0, max(sizes), cfg.item_embedding_dim)).to(dev)


def median_ms(fn, reps, before=None):
    """Median of `reps` device-event timings of fn() (one warm-up first); before(): untimed preparation of every repetition."""
    ts = []
    for r in range(reps + 1):
        if before is not None:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    ts.sort()
    return {"ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1], "reps": reps}


out = {"workload": f"amzn-books {cfg.query_dot_product_groups}x{cfg.item_dot_product_groups}x{cfg.dot_product_dimension}, N={N}, nlist={a.nlist}, "
                   "random-init weights, hashed items",
       "protocol": f"median of {a.reps} device-event timings after one warm-up; each timing covers the whole call (table and id writes, index, "
                   "lists, the read-back of the offsets)",
       "rows": []}
with torch.inference_mode():
    tk = rails_amd.MoLNaiveTopK(mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0), k_per_group=5, use_faiss=True, nlist=a.nlist, frozen_centroids=True)
    ivf = tk.ivf_index()
    eng = tk._bind()
    lists_bytes = ivf.vectors.numel() * 2 + ivf.positions.numel() * 4
    out["lists_bytes"] = lists_bytes
    out["baselines"] = {
        "rebuild": median_ms(lambda: E.IvfIndex(eng, tk._index, nlist=a.nlist), max(3, a.reps // 2)),
        "build_lists": median_ms(lambda: E.IvfIndex(eng, tk._index, nlist=a.nlist, centroids=ivf.centroids), max(3, a.reps // 2)),
    }
    gen = torch.Generator().manual_seed(7)
    next_id = [N + 1]
    for m in sizes:
        rows = fresh_rows[:m]
        pos = [None]

        def draw():
            pos[0] = torch.randperm(tk.num_items, generator=gen)[:m].to(dev)

        def append():
            tk.append_items(rows, torch.arange(next_id[0], next_id[0] + m, dtype=torch.int64, device=dev))
            next_id[0] += m

        row = {"m": m, "update_items": median_ms(lambda: tk.update_items(pos[0], rows), a.reps, before=draw),
               "append_items": median_ms(append, a.reps)}
        row["remove_items"] = median_ms(lambda: tk.remove_items(pos[0]), a.reps, before=draw)       # (takes the appended items' count back)
        row["n_items_after"] = tk.num_items
        for name in ("update_items", "append_items", "remove_items"):
            row[name]["lists_bytes_moved_per_s"] = 2 * lists_bytes / (row[name]["ms_median"] * 1e-3)
        out["rows"].append(row)
    out["list_sizes_min_max"] = [int(tk.ivf_index().list_sizes().min()), int(tk.ivf_index().list_sizes().max())]
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
