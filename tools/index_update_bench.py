#!/usr/bin/env python3
"""update_items / append_items against what they replace -- constructing the module again from the full table plus its first call -- at
amzn-books size (N = 695 762): MoLBruteForceTopK in the default (proved) mode and MoLCombTopK100_1000.  Every derived buffer is built
before timing (calls through forward and get_top_k_outputs), so an update refreshes all of them.
  update_items   M in {1, 1 024, 65 536}: device events around the call (fresh random positions and rows per repetition, drawn outside the
                 timed window; positions on the HOST, so the validation's copy is not a device sync), median of --iters after --warmup
  append_items   M = 1 024: a module per repetition would dominate the run, so the appends are chained (N grows by 1 024 per repetition)
  rebuild        constructor + first forward from the same table, host clock around a device synchronise, median of --rebuilds
Beside each: the bytes the update kernels are expected to touch, from the shapes (per buffer: what is written; the raw rows are read once
per index format).  Writes profiles/index_update.json and prints it as one JSON line.
  python tools/index_update_bench.py [--items 695762] [--warmup 3] [--iters 15] [--rebuilds 3]
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


def build_mol(cfg, dev):
    mol, _ = rails_amd.create_mol_interaction_module(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
        cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
        cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
        query_nonlinearity=cfg.query_nonlinearity)
    mol.load_state_dict(O.synthetic_weights(cfg, seed=0), strict=True)
    return mol.to(dev).eval()


def held_buffers(tk):
    """name -> (tensor, bytes written per updated item) of every derived buffer the module holds"""
    out = {"index": (tk._index.buf, tk._index.buf.numel() * 4 / max(1, (tk._index.n_items + 31) // 32 * 32))}
    c = tk._rows_cache
    if c is not None and c[2] is not None:
        out["rows"] = (c[2], c[2].numel() * 4 / tk._index.n_items)
    if getattr(tk, "_index32", None) is not None:
        out["index32"] = (tk._index32.buf, out["index"][1])
    for name in ("_rows32", "_coarse_table", "_comp_table"):
        t = getattr(tk, name, None)
        if t is not None:
            out[name.strip("_")] = (t, t.numel() * t.element_size() / tk.num_items)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=695_762)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--rebuilds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_update.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "index_update_bench needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    N, D, B = args.items, cfg.item_embedding_dim, 32
    mol = build_mol(cfg, dev)
    q = O.synthetic_queries(cfg, B).to(dev)
    g = torch.Generator().manual_seed(3)
    makers = {
        "MoLBruteForceTopK": lambda x, i: rails_amd.MoLBruteForceTopK(mol, x, i),
        "MoLCombTopK100_1000": lambda x, i: rails_amd.MoLCombTopK(mol, x, i, avg_top_k=1000, k_per_group=100),
    }
    result = {"box": {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__, "hip": torch.version.hip},
              "workload": {"config": "amzn-books", "n_items": N, "batch": B}, "protocol": {"warmup": args.warmup, "iters": args.iters, "rebuilds": args.rebuilds},
              "modules": {}}
    with torch.inference_mode():
        for name, make in makers.items():
            X = E.hash_item_table(1, 0, N, D, dev).unsqueeze(0)
            ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
            cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)

            def first_call(tk):
                tk(q, k=200)

            rebuild = []
            for _ in range(args.rebuilds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tk = make(X, ids)
                first_call(tk)
                torch.cuda.synchronize()
                rebuild.append((time.perf_counter() - t0) * 1e3)
                del tk
            tk = make(X, ids)
            first_call(tk)
            cand.get_top_k_outputs(q, 100, {}, tk, ids[:, :61].expand(B, 61).contiguous())
            bufs = held_buffers(tk)
            per_item = {k: v[1] for k, v in bufs.items()}
            rec = {"rebuild_plus_first_call_ms": {"median": statistics.median(rebuild), "all": rebuild},
                   "held_buffers_bytes": {k: v[0].numel() * v[0].element_size() for k, v in bufs.items()},
                   "bytes_written_per_updated_item": per_item, "update_items": {}, "append_items": {}}
            for M in (1, 1024, 65536):
                times = []
                for it in range(args.warmup + args.iters):
                    pos = torch.randperm(tk.num_items, generator=g)[:M]
                    rows = E.hash_item_table(100 + it, 0, M, D, dev)
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    tk.update_items(pos, rows)
                    b.record()
                    b.synchronize()
                    if it >= args.warmup:
                        times.append((a.elapsed_time(b), (time.perf_counter() - t0) * 1e3))
                rec["update_items"][str(M)] = {"device_ms_median": statistics.median(t[0] for t in times), "host_wall_ms_median": statistics.median(t[1] for t in times),
                                               "device_ms_all": [t[0] for t in times],
                                               "expected_bytes": {"raw_rows_written": M * D * 4, **{k: int(M * v) for k, v in per_item.items()}}}
            first_call(tk)
            times = []
            M = 1024
            for it in range(args.warmup + args.iters):
                rows = E.hash_item_table(500 + it, 0, M, D, dev)
                new_ids = torch.arange(M, dtype=torch.int64, device=dev) + 10_000_000 + it * M
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                tk.append_items(rows, new_ids)
                b.record()
                b.synchronize()
                if it >= args.warmup:
                    times.append(a.elapsed_time(b))
            rec["append_items"][str(M)] = {"device_ms_median": statistics.median(times), "device_ms_all": times, "n_items_after": tk.num_items,
                                           "growth_copy_bytes": sum(rec["held_buffers_bytes"].values()) + N * D * 4 + N * 16}
            first_call(tk)       # the module still answers
            torch.cuda.synchronize()
            result["modules"][name] = rec
            del tk, X, ids, cand
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
