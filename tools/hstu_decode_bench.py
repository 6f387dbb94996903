#!/usr/bin/env python3
"""Latency of the HSTU encoder's cached incremental decoding (rails_amd.HSTU.encode with delta_x_offsets / cache) against a full
re-encode, at the three rails-final geometries, B = 1 and 32.  Per geometry and batch: the prefill that returns the cache states, one
decode step at lengths - 1 (device-resident offsets: the sync-free path), and the default full encode (the fused kernel where it fits,
else the per-layer kernels).  Each call is timed with device events around it; the record is the median of the timed calls after
warm-up.  Prints one JSON line.
  python tools/hstu_decode_bench.py [--warmup 10] [--iters 50]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rails_amd.hstu import HSTU  # noqa: E402

GEOM = {   # as tools/hstu_bench.py
    "ml-1m": dict(D=50, blocks=8, heads=2, dh=25, N=211, items=3883),
    "ml-20m": dict(D=256, blocks=16, heads=8, dh=32, N=211, items=27278),
    "amzn-books": dict(D=64, blocks=16, heads=8, dh=8, N=61, items=695762),
}


def timed(fn, warmup, iters):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for name, gm in GEOM.items():
        torch.manual_seed(0)
        m = HSTU(gm["N"] - 1, 1, gm["D"], gm["blocks"], gm["heads"], gm["dh"], gm["dh"], gm["items"]).eval().to(dev)
        N = gm["N"]
        for B in (1, 32):
            g = torch.Generator().manual_seed(1)
            lengths = torch.randint(N // 2, N + 1, (B,), generator=g)
            ids = torch.randint(1, gm["items"] + 1, (B, N), generator=g) * (torch.arange(N).unsqueeze(0) < lengths.unsqueeze(1))
            ts = 1_000_000_000 + torch.cumsum((10.0 ** (torch.rand((B, N), generator=g) * 6)).long(), 1)
            l_d, i_d, pay = lengths.to(dev), ids.to(dev), {"timestamps": ts.to(dev)}
            pos = (lengths - 1).to(dev)
            delta = (torch.cumsum(l_d, 0) - l_d + pos, pos)
            with torch.inference_mode():
                emb = m.get_item_embeddings(i_d)
                _, cache = m.encode(l_d, i_d, emb, pay, return_cache_states=True)
                full = m.encode(l_d, i_d, emb, pay)
                dec = m.encode(l_d, i_d, emb, pay, delta_x_offsets=delta, cache=cache)   # the same row again: the same sequence
                prefill_ms = timed(lambda: m.encode(l_d, i_d, emb, pay, return_cache_states=True), args.warmup, args.iters)
                decode_ms = timed(lambda: m.encode(l_d, i_d, emb, pay, delta_x_offsets=delta, cache=cache), args.warmup, args.iters)
                full_ms = timed(lambda: m.encode(l_d, i_d, emb, pay), args.warmup, args.iters)
            rows.append({"geometry": name, "D": gm["D"], "blocks": gm["blocks"], "heads": gm["heads"], "dh": gm["dh"], "N": N, "B": B,
                         "prefill_with_states_ms": prefill_ms, "decode_step_ms": decode_ms, "full_encode_ms": full_ms,
                         "full_over_decode": full_ms / decode_ms, "max_abs_decode_vs_full": float((dec - full).abs().max())})
    print(json.dumps({"hstu_decode_bench": rows, "warmup": args.warmup, "iters": args.iters}))


if __name__ == "__main__":
    main()
