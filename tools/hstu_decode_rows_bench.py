#!/usr/bin/env python3
"""Latency of the HSTU encoder's multi-row cached decode step (HSTU.encode(..., delta_rows=), rails_hstu_decode_rows) at the three
rails-final geometries, B = 1 and 32, m = 1, 2, 4, 8 rows per sequence, full histories, device-resident offsets and counts.  Per
point: one multi-row step over the last m rows, the same rows as m single-row steps (delta_rows=None, rails_hstu_decode), the default
full encode, and the prefill that returns the cache states.  The variants of a point are timed in turn inside one loop (one call each
per round, device events around each), so that drift of the machine lands on all of them alike; the figure is the median of the timed
rounds after the warm-up rounds.  The record also says whether the multi-row step was torch.equal, in the result and in every cache
tensor, to m one-row calls of the same entry (delta_rows=1), and how far its result lies from the full encode.
  python tools/hstu_decode_rows_bench.py [--label new] [--out FILE]
  python tools/hstu_decode_rows_bench.py --plain-only [--tree PATH] [--label parent] [--out FILE]
--plain-only times the single-row step alone (six points); --tree PATH measures the rails_amd package of another checkout (built
there), the parent commit's for instance.  --geometry / --batch / --rows / --only VARIANT narrow a run to one point and one variant,
for a `rocprofv3 --kernel-trace --stats` run whose kernel records then all belong to warmup + iters calls of that variant.
  python tools/hstu_decode_rows_bench.py --merge RUN.json [RUN.json ...] [--kernel-stats GEOMETRY=kernel_stats.csv ...] [--out profiles/hstu_decode_rows_bench.json]
merges runs: per point the median over the runs labelled "new"; for the plain step the medians of "parent" and "new" (run
alternately) and the parent's run-to-run spread (largest minus smallest); per --kernel-stats file the launches and kernel
microseconds per step of the traced variant.
"""
import argparse
import csv
import json
import os
import statistics
import sys

GEOM = {   # as tools/hstu_bench.py
    "ml-1m": dict(D=50, blocks=8, heads=2, dh=25, N=211, items=3883),
    "ml-20m": dict(D=256, blocks=16, heads=8, dh=32, N=211, items=27278),
    "amzn-books": dict(D=64, blocks=16, heads=8, dh=8, N=61, items=695762),
}
ROWS = (1, 2, 4, 8)
BATCHES = (1, 32)
VARIANTS = ("multi_row_step_ms", "single_row_steps_ms", "full_encode_ms", "prefill_with_states_ms")


def timed_in_turn(fns, warmup, iters):
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


def measure(args):
    import torch

    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from rails_amd.hstu import HSTU

    dev = torch.device("cuda", 0)
    points = []
    for name, gm in GEOM.items():
        if args.geometry and name != args.geometry:
            continue
        torch.manual_seed(0)
        m = HSTU(gm["N"] - 1, 1, gm["D"], gm["blocks"], gm["heads"], gm["dh"], gm["dh"], gm["items"]).eval().to(dev)
        N = gm["N"]
        for B in BATCHES:
            if args.batch and B != args.batch:
                continue
            g = torch.Generator().manual_seed(1)
            lengths = torch.full((B,), N, dtype=torch.int64)
            ids = torch.randint(1, gm["items"] + 1, (B, N), generator=g)
            ts = 1_000_000_000 + torch.cumsum((10.0 ** (torch.rand((B, N), generator=g) * 6)).long(), 1)
            l_d, i_d, pay = lengths.to(dev), ids.to(dev), {"timestamps": ts.to(dev)}
            off = torch.cumsum(l_d, 0) - l_d
            with torch.inference_mode():
                emb = m.get_item_embeddings(i_d)
                full, cache = m.encode(l_d, i_d, emb, pay, return_cache_states=True)

                def clone():
                    return [tuple(t.clone() for t in s) for s in cache]

                def plain(p, c):
                    pos = torch.full((B,), p, dtype=torch.int64, device=dev)
                    return lambda: m.encode(l_d, i_d, emb, pay, delta_x_offsets=(off + pos, pos), cache=c)

                if args.plain_only:
                    c = clone()
                    points.append({"geometry": name, "B": B, "N": N, **timed_in_turn({"plain_step_ms": plain(N - 1, c)}, args.warmup, args.iters)})
                    continue
                for rows in ROWS:
                    if args.rows and rows != args.rows:
                        continue
                    start = torch.full((B,), N - rows, dtype=torch.int64, device=dev)
                    counts = torch.full((B,), rows, dtype=torch.int64, device=dev)
                    delta = (off + start, start)
                    c1, c2, c3 = clone(), clone(), clone()
                    singles = [plain(N - rows + t, c3) for t in range(rows)]
                    fns = {"multi_row_step_ms": lambda: m.encode(l_d, i_d, emb, pay, delta_x_offsets=delta, cache=c1, delta_rows=counts, max_delta_rows=rows),
                           "single_row_steps_ms": lambda: [f() for f in singles],
                           "full_encode_ms": lambda: m.encode(l_d, i_d, emb, pay),
                           "prefill_with_states_ms": lambda: m.encode(l_d, i_d, emb, pay, return_cache_states=True)}
                    if args.only:
                        fns = {args.only: fns[args.only]}
                    out = fns["multi_row_step_ms"]() if not args.only else None      # a traced run holds the timed calls only
                    point = {"geometry": name, "B": B, "N": N, "rows": rows}
                    if out is not None:
                        for t in range(rows):
                            pos = start + t
                            one = m.encode(l_d, i_d, emb, pay, delta_x_offsets=(off + pos, pos), cache=c2, delta_rows=1)
                        point["multi_equals_chained_single_row_entry"] = bool(torch.equal(out, one)) and all(
                            torch.equal(x, y) for s, t2 in zip(c1, c2) for x, y in zip(s, t2))
                        point["max_abs_multi_vs_full_encode"] = float((out - m.encode(l_d, i_d, emb, pay)).abs().max())
                    point.update(timed_in_turn(fns, args.warmup, args.iters))
                    points.append(point)
    return {"label": args.label, "plain_only": bool(args.plain_only), "warmup": args.warmup, "iters": args.iters, "points": points}


def kernel_stats(path, steps):
    """-> launches and kernel microseconds per step of a rocprofv3 --stats kernel_stats.csv over `steps` calls."""
    rows = list(csv.DictReader(open(path)))
    mine = [r for r in rows if "hsturows" in r["Name"]]
    return {"launches_per_step": sum(int(r["Calls"]) for r in mine) / steps,
            "kernel_us_per_step": sum(float(r["TotalDurationNs"]) for r in mine) / steps / 1e3,
            "by_kernel_us_per_step": {r["Name"].split("hsturows_")[1].split("(")[0]: float(r["TotalDurationNs"]) / steps / 1e3 for r in mine}}


def merge(files, stats):
    runs = [json.load(open(f)) for f in files]
    new = [r for r in runs if r["label"] == "new" and not r["plain_only"]]
    at = {}
    for r in new:
        for p in r["points"]:
            at.setdefault((p["geometry"], p["B"], p["rows"]), []).append(p)
    points = []
    for (geom, B, rows), ps in sorted(at.items(), key=lambda kv: (list(GEOM).index(kv[0][0]), kv[0][1], kv[0][2])):
        q = {"geometry": geom, "B": B, "N": ps[0]["N"], "rows": rows, "runs": len(ps)}
        for v in VARIANTS:
            q[v] = statistics.median(p[v] for p in ps)
        q["multi_equals_chained_single_row_entry"] = all(p["multi_equals_chained_single_row_entry"] for p in ps)
        q["max_abs_multi_vs_full_encode"] = max(p["max_abs_multi_vs_full_encode"] for p in ps)
        q["single_steps_over_multi"] = q["single_row_steps_ms"] / q["multi_row_step_ms"]
        q["full_encode_over_multi"] = q["full_encode_ms"] / q["multi_row_step_ms"]
        points.append(q)
    plain = {}
    for r in runs:
        if r["plain_only"]:
            for p in r["points"]:
                plain.setdefault((p["geometry"], p["B"]), {}).setdefault(r["label"], []).append(p["plain_step_ms"])
    vs = []
    for (geom, B), by in sorted(plain.items(), key=lambda kv: (list(GEOM).index(kv[0][0]), kv[0][1])):
        if "parent" in by and "new" in by:
            spread = max(by["parent"]) - min(by["parent"])
            vs.append({"geometry": geom, "B": B, "parent_ms": statistics.median(by["parent"]), "new_ms": statistics.median(by["new"]),
                       "parent_spread_ms": spread, "runs": [len(by["parent"]), len(by["new"])],
                       "within_parent_spread": abs(statistics.median(by["new"]) - statistics.median(by["parent"])) <= spread})
    first = (new or runs)[0]
    steps = first["warmup"] + first["iters"]
    traced = {}
    for item in stats:
        geom, path = item.split("=", 1)
        traced[geom] = {"B": 32, "rows": 4, **kernel_stats(path, steps)}
    return {"hstu_decode_rows_bench": points, "plain_single_row_step_vs_parent": vs, "kernel_trace_multi_row_step": traced,
            "warmup": first["warmup"], "iters": first["iters"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--label", default="new")
    ap.add_argument("--tree")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--geometry", choices=list(GEOM))
    ap.add_argument("--batch", type=int)
    ap.add_argument("--rows", type=int)
    ap.add_argument("--only", choices=VARIANTS)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    ap.add_argument("--out")
    args = ap.parse_args()
    rec = merge(args.merge, args.kernel_stats) if args.merge else measure(args)
    text = json.dumps(rec, indent=1 if args.merge else None)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text if not args.merge else json.dumps({k: rec[k] for k in ("plain_single_row_step_vs_parent", "kernel_trace_multi_row_step")}))


if __name__ == "__main__":
    main()
