#!/usr/bin/env python3
"""Calls with allowed_tags= on the approximate modules beside the same module's unfiltered call and beside MoLBruteForceTopK
with the equivalent per-row item_mask=: amzn-books geometry (N = 695 762, synthetic weights, hashed item table), B = 32, forward(k = 10) of
MoLAvgTopK200, MoLNaiveTopK5 and MoLCombTopK100_1000, with 100 %, 50 %, 10 % and 1 % of the corpus kept -- once with one allow word shared by
the batch, once with a word per row (ten distinct words of the same kept fraction, cycled over the 32 rows).
Tag layout: bit 0 on every item (the 100 % word); bits 1-10 each on a random 50 %, bits 11-20 each on a random 10 %, bits 21-30 each on a
random 1 % of the items, independently.
One timing = --steps calls between two device events; the filtered call, the unfiltered call and the exact module's masked call are
interleaved round by round (--rounds), the median over the rounds is reported in microseconds per call.  Every cell records the route its
candidate scans took and, from one call of the fused tagged entries on the same filter, their verdict flags and candidate counts (would the
fused scan have answered without its redo, whatever the routing rule chose).  Writes profiles/item_tags.json (or --out) and prints it as one JSON line.
  python tools/item_tags_bench.py [--steps 5] [--rounds 5] [--warmup 2] [--out PATH]
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

ALGORITHMS = {
    "MoLAvgTopK200": lambda mol, x, i: rails_amd.MoLAvgTopK(mol, x, i, avg_top_k=200),
    "MoLNaiveTopK5": lambda mol, x, i: rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=5),
    "MoLCombTopK100_1000": lambda mol, x, i: rails_amd.MoLCombTopK(mol, x, i, avg_top_k=1000, k_per_group=100),
}
FRACTIONS = (("100 %", 1.0, 0), ("50 %", 0.5, 1), ("10 %", 0.1, 11), ("1 %", 0.01, 21))      # (label, kept fraction, first of its ten bits)


def tag_layout(n, g):
    tags = torch.ones(n, dtype=torch.int64)
    for _, fraction, first in FRACTIONS[1:]:
        for j in range(10):
            tags |= (torch.rand(n, generator=g) < fraction).to(torch.int64) << (first + j)
    return tags


def fused_verdicts(tk, q, allowed, B):
    """The fused tagged entries on this filter, whatever route the module's rule picks for it: per scan the verdict flag (1 = a row's candidate
    count left [k, capacity]: the call would pay its redo) and the range of the counts."""
    filt = tk._take_allowed_tags({"allowed_tags": allowed}, B, ())
    eng = tk._bind()
    eq = eng.query_pack(q, None, want_plain=True)[1]
    out = {}
    if getattr(tk, "_k_per_group", None) is not None:
        kg, step = tk._k_per_group, max(1, E.TAGGED_COMPONENT_ROWS // eng.spec.query_dot_product_groups)
        flags, lo, hi = [], [], []
        for b0 in range(0, B, step):
            flag = torch.ones(1, dtype=torch.int32, device=q.device)
            r = eng.component_topk(eq[b0:b0 + step].contiguous(), tk._component_table(), kg, flag, tags=filt.rows_slice(b0, b0 + step))
            if r is None:
                return {"component": None}
            flags.append(int(flag.item())), lo.append(int(r[2].min())), hi.append(int(r[2].max()))
        out["component"] = {"slices": len(flags), "flag": max(flags), "counts_min": min(lo), "counts_max": max(hi), "k": kg,
                            "capacity": eng.component_topk_capacity(min(B, step), tk.num_items, kg)}
    if getattr(tk, "_avg_top_k", None) is not None:
        kp = tk._avg_top_k
        r = eng.coarse_topk(eq, tk._table(), isinstance(tk, rails_amd.MoLCombTopK), kp, with_flag=True, tags=filt)
        out["coarse"] = None if r is None else {"flag": int(r[3].item()), "counts_min": int(r[2].min()), "counts_max": int(r[2].max()), "k": kp,
                                                "capacity": E.MolEngine.coarse_topk_capacity(kp, tk.num_items, B)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--items", type=int, default=695_762)
    ap.add_argument("--algorithms", default=",".join(ALGORITHMS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "item_tags.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "item_tags_bench needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS["amzn-books"]
    mol = build_mol(cfg, dev)
    g = torch.Generator().manual_seed(5)
    n, B, k = args.items, 32, 10
    result = {"box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip},
              "protocol": {"steps_per_timing": args.steps, "rounds": args.rounds, "warmup_calls": args.warmup, "n_items": n, "batch": B, "k": k,
                           "unit": "us per forward call, device events; filtered, unfiltered and exact-with-item_mask calls interleaved"},
              "algorithms": {}}
    with torch.inference_mode():
        X = E.hash_item_table(1, 0, n, cfg.item_embedding_dim, dev).unsqueeze(0)
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
        q = O.synthetic_queries(cfg, B).to(dev)
        tags = tag_layout(n, g).to(dev)
        exact = rails_amd.MoLBruteForceTopK(mol, X, ids)
        for name in args.algorithms.split(","):
            tk = ALGORITHMS[name](mol, X, ids)
            tk.set_item_tags(tags)
            rows = {}
            for label, _, first in FRACTIONS:
                for sharing in ("shared word", "word per row"):
                    words = [1 << first] * B if (sharing == "shared word" or first == 0) else [1 << (first + b % 10) for b in range(B)]
                    allowed = words[0] if sharing == "shared word" else words
                    w = torch.tensor(words, device=dev)
                    mask = E.ItemMask(((tags.unsqueeze(0) & w.unsqueeze(1)) != 0).contiguous() if sharing == "word per row" else (tags & words[0]) != 0)
                    for _ in range(args.warmup):
                        tk(q, k=k, allowed_tags=allowed)
                        tk(q, k=k)
                        exact(q, k=k, item_mask=mask)
                    us = {"filtered": [], "unfiltered": [], "exact_item_mask": []}
                    for _ in range(args.rounds):
                        us["unfiltered"].append(timed(lambda: tk(q, k=k), args.steps))
                        us["filtered"].append(timed(lambda: tk(q, k=k, allowed_tags=allowed), args.steps))
                        us["exact_item_mask"].append(timed(lambda: exact(q, k=k, item_mask=mask), args.steps))
                    med = {key: statistics.median(v) for key, v in us.items()}
                    rows[f"{label}, {sharing}"] = {"kept_min": mask.kept_min, "kept_max": mask.kept_max, "distinct_words": len(set(words)),
                                                   "route": tk.allowed_tags_route(allowed, B), "fused_verdicts": fused_verdicts(tk, q, allowed, B),
                                                   "us": us, "us_median": med,
                                                   "filtered_over_unfiltered": med["filtered"] / med["unfiltered"],
                                                   "filtered_over_exact": med["filtered"] / med["exact_item_mask"]}
                    del mask
            result["algorithms"][name] = rows
            del tk
            torch.cuda.empty_cache()
    result["not_measured"] = ["kernel-level times of the tagged scans (only whole calls)", "the tagged int8 pre-filter scan (these modules hold no int8 copy at this N)",
                              "item tags on other geometries, batch sizes or corpus sizes", "the cost of set_item_tags and of the first call "
                              "with a new allow word (one launch and one read-back per word)"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
