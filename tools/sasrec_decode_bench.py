#!/usr/bin/env python3
"""Latency of SASRec's cached incremental decoding (rails_amd.SASRec.encode with cache=) against a full re-encode, at the
geometries of tools/sasrec_bench.py, B = 1 and 32, full histories (every length N: the decode step runs at p = N - 1 and reads
the most cache).  Per geometry and batch: the prefill that returns the cache states, one decode step (device-resident lengths: the
sync-free path; a replace-last step, so the cache holds the same sequence every call), and the default full encode (the fused
kernel where it fits, else the per-layer kernels).  Each call is timed with device events around it; the record is the median of
the timed calls after warm-up.  Prints one JSON line.
  python tools/sasrec_decode_bench.py [--warmup 10] [--iters 50]

--new-rows: the multi-row step (encode with cache= and new_rows=m) instead.  Per geometry, B and m = 1, 2, 4, 8: the one multi-row
step over the last m rows, m single-row steps at lengths N - m + 1 .. N, the full encode and the prefill with states; then the
multi-row step alone at m = 16, 32, ... N, for the m at which the prefill becomes the cheaper call.  The variants of a point are
timed in turn inside one loop (one call each per round), so that drift of the machine lands on all of them alike.
  python tools/sasrec_decode_bench.py --new-rows [--tree PATH] [--label NAME] [--out FILE]
--tree PATH measures the rails_amd package of another checkout (built there), the parent commit's for instance; a package without
new_rows= gives the single-row columns only.  --geometry / --batch / --rows / --only COLUMN narrow the run to one point and one
variant, for a `rocprofv3 --kernel-trace` run whose kernel records then all belong to warmup + iters calls of that variant.
  python tools/sasrec_decode_bench.py --merge RUN.json [RUN.json ...] [--out profiles/sasrec_append_bench.json]
merges alternating runs labelled "parent" and "new": per point the median over each label's runs, the parent's run-to-run spread
(largest minus smallest of its runs), the runs' own checks of the multi-row result (its largest distance from the full encode,
whether it was torch.equal to the single-row steps in every run), and the two comparisons of DESIGN.md 3.9's table;
--kernel-times FILE carries a JSON file of kernel times per step, summed from the trace runs, into the merged record.
"""
import argparse
import inspect
import json
import os
import statistics
import sys

GEOM = {   # as tools/sasrec_bench.py
    "amzn-books": dict(N=51, D=64, blocks=4, heads=4, ffn=64, items=10000),
    "ml-1m": dict(N=201, D=50, blocks=2, heads=1, ffn=50, items=3883),
    "ml-20m": dict(N=201, D=256, blocks=4, heads=4, ffn=256, items=27278),
}
NEW_ROWS = (1, 2, 4, 8)
FAR_ROWS = (16, 32, 64, 128)     # and N: the multi-row step alone, for the crossover with the prefill


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def timed_in_turn(fns, warmup, iters):
    """{name: median ms}: one event-timed call of every fn per round."""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in out.items()}


def setup(SASRec, gm, B, dev):
    import torch
    N = gm["N"]
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, gm["items"] + 1, (B, N), generator=g)
    return torch.full((B,), N, dtype=torch.int64).to(dev), ids.to(dev)


def bench_single(args, SASRec, dev):
    import torch
    rows = []
    for name, gm in GEOM.items():
        torch.manual_seed(0)
        N = gm["N"]
        m = SASRec(N - 1, 1, gm["D"], gm["blocks"], gm["heads"], gm["ffn"], "relu", num_items=gm["items"],
                   output_postproc="layer_norm").to(dev).eval()
        for B in (1, 32):
            l_d, i_d = setup(SASRec, gm, B, dev)
            with torch.inference_mode():
                emb = m.get_item_embeddings(i_d)
                _, cache = m.encode(l_d, i_d, emb, {}, return_cache_states=True)
                full = m.encode(l_d, i_d, emb, {})
                dec = m.encode(l_d, i_d, emb, {}, cache=cache)   # the same last row again: the same sequence
                prefill_ms = timed(lambda: m.encode(l_d, i_d, emb, {}, return_cache_states=True), args.warmup, args.iters)
                decode_ms = timed(lambda: m.encode(l_d, i_d, emb, {}, cache=cache), args.warmup, args.iters)
                full_ms = timed(lambda: m.encode(l_d, i_d, emb, {}), args.warmup, args.iters)
            rows.append({"geometry": name, "D": gm["D"], "blocks": gm["blocks"], "heads": gm["heads"], "ffn": gm["ffn"], "N": N, "B": B,
                         "prefill_with_states_ms": prefill_ms, "decode_step_ms": decode_ms, "full_encode_ms": full_ms,
                         "full_over_decode": full_ms / decode_ms, "max_abs_decode_vs_full": float((dec - full).abs().max()),
                         "launches_per_step": 5 * gm["blocks"] + 1})
    return {"sasrec_decode_bench": rows, "warmup": args.warmup, "iters": args.iters}


def bench_new_rows(args, SASRec, dev):
    import torch
    multi = "new_rows" in inspect.signature(SASRec.encode).parameters
    rows = []
    for name, gm in GEOM.items():
        if args.geometry not in (None, name):
            continue
        torch.manual_seed(0)
        N = gm["N"]
        m = SASRec(N - 1, 1, gm["D"], gm["blocks"], gm["heads"], gm["ffn"], "relu", num_items=gm["items"],
                   output_postproc="layer_norm").to(dev).eval()
        for B in (1, 32) if args.batch is None else (args.batch,):
            l_d, i_d = setup(SASRec, gm, B, dev)
            with torch.inference_mode():
                emb = m.get_item_embeddings(i_d)
                _, cache = m.encode(l_d, i_d, emb, {}, return_cache_states=True)
                full = m.encode(l_d, i_d, emb, {})
                for r in NEW_ROWS if args.rows is None else (args.rows,):
                    steps = [l_d - (r - 1 - s) for s in range(r)]     # lengths N - r + 1 .. N, on the device

                    def singles():
                        for L in steps:
                            out = m.encode(L, i_d, emb, {}, cache=cache)
                        return out

                    fns = {"single_steps_ms": singles, "full_encode_ms": lambda: m.encode(l_d, i_d, emb, {}),
                           "prefill_with_states_ms": lambda: m.encode(l_d, i_d, emb, {}, return_cache_states=True)}
                    if multi:
                        fns = {"multi_row_step_ms": lambda: m.encode(l_d, i_d, emb, {}, cache=cache, new_rows=r), **fns}
                    if args.only:
                        fns = {args.only: fns[args.only]}
                    row = {"geometry": name, "N": N, "B": B, "m": r, **timed_in_turn(fns, args.warmup, args.iters)}
                    if multi and not args.only:
                        row["max_abs_multi_vs_full"] = float((m.encode(l_d, i_d, emb, {}, cache=cache, new_rows=r) - full).abs().max())
                        row["multi_equals_single_steps"] = bool(torch.equal(m.encode(l_d, i_d, emb, {}, cache=cache, new_rows=r), singles()))
                    rows.append(row)
                if multi and args.rows is None:
                    for r in [x for x in FAR_ROWS if x < N] + [N]:
                        t = timed_in_turn({"multi_row_step_ms": lambda: m.encode(l_d, i_d, emb, {}, cache=cache, new_rows=r),
                                           "prefill_with_states_ms": lambda: m.encode(l_d, i_d, emb, {}, return_cache_states=True)},
                                          args.warmup, args.iters)
                        rows.append({"geometry": name, "N": N, "B": B, "m": r, **t})
    return {"sasrec_append_bench": rows, "label": args.label, "warmup": args.warmup, "iters": args.iters,
            "launches_per_step": {k: 5 * v["blocks"] + 1 for k, v in GEOM.items()}}


def merge(paths, kernel_times=None):
    runs = [json.load(open(p)) for p in paths]
    by, checks = {}, {}
    for run in runs:
        for row in run["sasrec_append_bench"]:
            key = (row["geometry"], row["B"], row["m"])
            for k, v in row.items():
                if k.endswith("_ms"):
                    by.setdefault(key, {}).setdefault((run["label"], k), []).append(v)
            if "multi_equals_single_steps" in row:   # the runs' own checks of the multi-row result: the worst over the runs
                c = checks.setdefault(key, {"max_abs_multi_vs_full": 0.0, "multi_equals_single_steps": True})
                c["max_abs_multi_vs_full"] = max(c["max_abs_multi_vs_full"], row["max_abs_multi_vs_full"])
                c["multi_equals_single_steps"] = c["multi_equals_single_steps"] and row["multi_equals_single_steps"]
    points = []
    for (geom, B, r), cols in sorted(by.items(), key=lambda kv: (list(GEOM).index(kv[0][0]), kv[0][1], kv[0][2])):
        p = {"geometry": geom, "B": B, "m": r, **checks.get((geom, B, r), {})}
        for (label, k), v in sorted(cols.items()):
            p[f"{label}/{k}"] = statistics.median(v)
            p[f"{label}/{k[:-3]}_spread_ms"] = max(v) - min(v)
        points.append(p)
    at = {(p["geometry"], p["B"], p["m"]): p for p in points}
    single, burst, cross = [], [], []
    for geom in GEOM:
        for B in (1, 32):
            p = at[(geom, B, 1)]
            if "parent/single_steps_ms" in p and "new/single_steps_ms" in p:
                single.append({"geometry": geom, "B": B, "parent_ms": p["parent/single_steps_ms"], "new_ms": p["new/single_steps_ms"],
                               "parent_spread_ms": p["parent/single_steps_spread_ms"],
                               "not_slower": p["new/single_steps_ms"] <= p["parent/single_steps_ms"] + p["parent/single_steps_spread_ms"]})
            far = [(r, at[(geom, B, r)]) for (g2, b2, r) in sorted(at) if g2 == geom and b2 == B and "new/multi_row_step_ms" in at[(g2, b2, r)]]
            over = [r for r, q in far if q["new/multi_row_step_ms"] > q["new/prefill_with_states_ms"]]
            cross.append({"geometry": geom, "B": B, "measured_m": [r for r, _ in far], "prefill_cheaper_from_m": over[0] if over else None})
        p = at[(geom, 32, 4)]
        if "parent/single_steps_ms" in p and "new/multi_row_step_ms" in p:
            burst.append({"geometry": geom, "B": 32, "m": 4, "parent_four_single_steps_ms": p["parent/single_steps_ms"],
                          "new_multi_row_step_ms": p["new/multi_row_step_ms"], "parent_spread_ms": p["parent/single_steps_spread_ms"],
                          "faster": p["new/multi_row_step_ms"] < p["parent/single_steps_ms"] - p["parent/single_steps_spread_ms"]})
    extra = {"kernel_us_per_step": json.load(open(kernel_times))} if kernel_times else {}
    return {**extra, "sasrec_append_bench": points, "single_row_step_vs_parent": single, "multi_row_step_vs_four_parent_steps": burst,
            "prefill_crossover": cross, "runs": {lab: sum(1 for r in runs if r["label"] == lab) for lab in sorted({r["label"] for r in runs})},
            "warmup": runs[0]["warmup"], "iters": runs[0]["iters"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--new-rows", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="new")
    ap.add_argument("--geometry", choices=list(GEOM))
    ap.add_argument("--batch", type=int)
    ap.add_argument("--rows", type=int)
    ap.add_argument("--only", choices=["multi_row_step_ms", "single_steps_ms", "full_encode_ms", "prefill_with_states_ms"])
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--kernel-times", help="with --merge: a JSON file of kernel times per step (from the trace runs) to carry along")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.merge:
        res = merge(args.merge, args.kernel_times)
    else:
        import torch
        sys.path.insert(0, args.tree)
        from rails_amd import SASRec  # noqa: E402
        dev = torch.device("cuda", 0)
        res = bench_new_rows(args, SASRec, dev) if args.new_rows else bench_single(args, SASRec, dev)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
