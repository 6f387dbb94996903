#!/usr/bin/env python3
"""Latency of SASRec's cached incremental decoding (rails_amd.SASRec.encode with cache=) against a full re-encode, at the
geometries of tools/sasrec_bench.py, B = 1 and 32, full histories (every length N: the decode step runs at p = N - 1 and reads
the most cache).  Per geometry and batch: the prefill that returns the cache states, one decode step (device-resident lengths: the
sync-free path; a replace-last step, so the cache holds the same sequence every call), and the default full encode (the fused
kernel where it fits, else the per-layer kernels).  Each call is timed with device events around it; the record is the median of
the timed calls after warm-up.  Prints one JSON line.
  python tools/sasrec_decode_bench.py [--warmup 10] [--iters 50]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rails_amd import SASRec  # noqa: E402

GEOM = {   # as tools/sasrec_bench.py
    "amzn-books": dict(N=51, D=64, blocks=4, heads=4, ffn=64, items=10000),
    "ml-1m": dict(N=201, D=50, blocks=2, heads=1, ffn=50, items=3883),
    "ml-20m": dict(N=201, D=256, blocks=4, heads=4, ffn=256, items=27278),
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
        N = gm["N"]
        m = SASRec(N - 1, 1, gm["D"], gm["blocks"], gm["heads"], gm["ffn"], "relu", num_items=gm["items"],
                   output_postproc="layer_norm").to(dev).eval()
        for B in (1, 32):
            g = torch.Generator().manual_seed(1)
            lengths = torch.full((B,), N, dtype=torch.int64)
            ids = torch.randint(1, gm["items"] + 1, (B, N), generator=g)
            l_d, i_d = lengths.to(dev), ids.to(dev)
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
    print(json.dumps({"sasrec_decode_bench": rows, "warmup": args.warmup, "iters": args.iters}))


if __name__ == "__main__":
    main()
