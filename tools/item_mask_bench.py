#!/usr/bin/env python3
"""A masked get_top_k_outputs step against the unmasked one, MoLBruteForceTopK in the default (proved) mode, B = 32,
k = 200, a 61-wide seen list, synthetic weights and hashed item table:
  amzn-books geometry (N = 695 762)   a shared mask keeping 1 %, 2 %, 10 %, 50 % and 90 % of the corpus, forced through each strategy that
                                      admits it (sparse: at most 16 384 kept items) -- beside the unmasked call of the same module;
  the crossover geometries            N = 65 536 with kept = N / 16, N / 8, N / 4 through both strategies and N / 2 (dense only), and
                                      N = 32 768 with kept = N / 4, N / 3, N / 2 through both: where the sparse rule's factor
                                      (MASK_SPARSE_FACTOR: sparse iff factor * kept_max <= N) can be read off below the 16 384 cap.
One timing = --steps calls between two device events; the variants of a geometry are interleaved round by round (--rounds), the median over
the rounds is reported in microseconds per call.  Masks are built once, outside the timed windows (a reused ItemMask costs a call no sync).
The strategy is forced through the instance attributes MASK_SPARSE_MAX / MASK_SPARSE_FACTOR; "flow" says what the dense strategy ran (the
proved flow where the mask keeps more than MASK_PROVED_MIN_KEPT items, the dense fp32 kernels otherwise).  Writes profiles/item_mask.json
(or --out) and prints it as one JSON line.
  python tools/item_mask_bench.py [--steps 20] [--rounds 9] [--warmup 2] [--out PATH]
"""
import argparse
import json
import os
import platform
import statistics
import sys

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


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps      # us per call


def geometry(mol, cfg, dev, n, kept_counts, args, g):
    B, k = 32, 200
    X = E.hash_item_table(1, 0, n, cfg.item_embedding_dim, dev).unsqueeze(0)
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, B).to(dev)
    seen = ids[0, torch.randint(0, n, (B, 61), generator=g).to(dev)].contiguous()
    tk = rails_amd.MoLBruteForceTopK(mol, X, ids)
    cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
    variants = {"unmasked": (None, None)}
    for label, kept in kept_counts:
        mask = E.ItemMask.from_positions(n, torch.randperm(n, generator=g)[:kept], dev)
        mask.positions()
        variants[f"{label} dense"] = (mask, "dense")
        if kept <= 16384:
            variants[f"{label} sparse"] = (mask, "sparse")

    def call(mask, how):
        if mask is None:
            return cand.get_top_k_outputs(q, k, {}, tk, seen)
        tk.MASK_SPARSE_MAX, tk.MASK_SPARSE_FACTOR = (0, 4) if how == "dense" else (16384, 1)
        return cand.get_top_k_outputs(q, k, {"item_mask": mask}, tk, seen)

    rec = {name: {"kept": None if m is None else m.kept_max, "strategy": how, "us": []} for name, (m, how) in variants.items()}
    for name, (m, how) in variants.items():      # warm-up, and what each variant ran
        before = dict(tk.stats())
        for _ in range(args.warmup):
            call(m, how)
        after = tk.stats()
        rec[name]["flow"] = "proved" if after["calls"] > before["calls"] else ("sparse" if how == "sparse" else "dense fp32")
        if m is not None:
            assert after.get(f"masked_{how}_calls", 0) > before.get(f"masked_{how}_calls", 0), (name, before, after)
    for _ in range(args.rounds):
        for name, (m, how) in variants.items():
            rec[name]["us"].append(timed(lambda: call(m, how), args.steps))
    st = tk.stats()
    for v in rec.values():
        v["us_median"] = statistics.median(v["us"])
    return {"n_items": n, "batch": B, "k": k, "seen_width": 61, "first_pass_matrix_bytes": B * n * 4, "variants": rec,
            "module_stats": {key: st[key] for key in ("calls", "proved_calls", "fallbacks") if key in st}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--items", type=int, default=695_762)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "item_mask.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "item_mask_bench needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(5)
    result = {"box": {"device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"steps_per_timing": args.steps, "rounds": args.rounds, "warmup_calls": args.warmup, "unit": "us per get_top_k_outputs call, device events"}}
    with torch.inference_mode():
        n = args.items
        result["amzn_books"] = geometry(mol, cfg, dev, n, [(f"{p} %", n * p // 100) for p in (1, 2, 10, 50, 90)], args, g)
        torch.cuda.empty_cache()
        for key, n, factors in (("crossover", 65_536, (16, 8, 4, 2)), ("crossover_32k", 32_768, (4, 3, 2))):
            torch.cuda.empty_cache()
            result[key] = geometry(mol, cfg, dev, n, [(f"N / {f}", n // f) for f in factors], args, g)
            v = result[key]["variants"]
            result[key]["sparse_over_dense"] = {f"N / {f}": v[f"N / {f} sparse"]["us_median"] / v[f"N / {f} dense"]["us_median"]
                                                for f in factors if f"N / {f} sparse" in v}
    a = result["amzn_books"]["variants"]
    result["amzn_books"]["masked_dense_minus_unmasked_us"] = {name: a[name]["us_median"] - a["unmasked"]["us_median"] for name in a if name.endswith("dense")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
