#!/usr/bin/env python3
"""First figures of the differentiable MoLSimilarity.forward -> profiles/mol_grad.json.

amzn-books geometry (8x8x32, H = 128) on the per-row branch, B rows x X = 1 + R candidates: forward + backward of (y * dY).sum() with
gradients of q, the items and every parameter, set against eager torch autograd of the same restatement (tests/_mol_grad_ref.py) on
the same GPU in the same run, with the peak memory of both; MolEngine.pair_backward alone between device events.
  python tools/mol_grad_bench.py [--out profiles/mol_grad.json] [--points 4096x513,512x129]
  python tools/mol_grad_bench.py --kernel-trace DIR [--out ...]     the backward kernels alone: a fresh child under
                                                                    `rocprofv3 --kernel-trace --stats` (no counters in that run) makes
                                                                    pair_backward calls only; its per-kernel statistics are merged
                                                                    into the JSON under "kernel_trace"
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import rails_amd  # noqa: E402
from oracle.mol_oracle import CONFIGS, synthetic_weights  # noqa: E402
from tests import _mol_grad_ref as G  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


TRACE_CALLS = 5


def kernel_trace(args):
    """Parent side: never touches the GPU itself."""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.kernel_trace, "-o", "mol_grad", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child", "--points", args.points]
    subprocess.run(cmd, check=True, timeout=600)
    rows = []
    for path in glob.glob(os.path.join(args.kernel_trace, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                r = {k.strip().lower(): v for k, v in r.items()}
                name = r.get("name", "")
                if "mol_generic" in name:
                    rows.append({"kernel": name[:120], "calls": int(float(r.get("calls", 0))), "total_ns": int(float(r.get("totaldurationns", 0))),
                                 "average_ns": float(r.get("averagens", 0))})
    if not rows:
        raise SystemExit(f"no kernel statistics under {args.kernel_trace}")
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result["kernel_trace"] = {"what": f"rocprofv3 --kernel-trace --stats over a child that makes {TRACE_CALLS} pair_backward calls per point after one warm-up "
                                      "(weight gradients included), the generic route's kernels only", "points": args.points, "kernels": rows}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for r in rows:
        print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mol_grad.json"))
    ap.add_argument("--points", default="4096x513,512x129")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-trace", default=None, metavar="DIR")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernel_trace:
        return kernel_trace(args)
    dev = torch.device("cuda:0")
    cfg = CONFIGS["amzn-books"]
    w = synthetic_weights(cfg, seed=0)
    mol, _ = rails_amd.create_mol_interaction_module(
        query_embedding_dim=cfg.query_embedding_dim, item_embedding_dim=cfg.item_embedding_dim, dot_product_dimension=cfg.dot_product_dimension,
        query_dot_product_groups=cfg.query_dot_product_groups, item_dot_product_groups=cfg.item_dot_product_groups, temperature=cfg.temperature,
        query_dropout_rate=0.0, query_hidden_dim=cfg.query_hidden_dim, item_dropout_rate=0.0, item_hidden_dim=cfg.item_hidden_dim,
        gating_query_hidden_dim=cfg.gating_query_hidden_dim, gating_qi_hidden_dim=cfg.gating_qi_hidden_dim,
        gating_item_hidden_dim=cfg.gating_item_hidden_dim, softmax_dropout_rate=cfg.softmax_dropout_rate, bf16_training=False,
        query_nonlinearity=cfg.query_nonlinearity, item_nonlinearity=cfg.item_nonlinearity, gating_combination_type=cfg.gating_combination_type,
        eps=cfg.eps)
    mol.load_state_dict(w, strict=True)
    mol = mol.to(dev).eval()
    mol.differentiable = True
    ws = {k: v.to(dev).requires_grad_(True) for k, v in w.items()}
    result = {"geometry": "amzn-books 8x8x32 H=128", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "points": []}
    for point in args.points.split(","):
        B, X = (int(v) for v in point.split("x"))
        g = torch.Generator().manual_seed(1)
        q = torch.randn((B, cfg.query_embedding_dim), generator=g).to(dev).requires_grad_(True)
        items = (0.02 * torch.randn((B, X, cfg.item_embedding_dim), generator=g)).to(dev).requires_grad_(True)
        dy = torch.randn((B, X), generator=g).to(dev)

        def ours():
            y, _ = mol(q, items)
            return torch.autograd.grad((y * dy).sum(), [q, items] + list(mol.parameters()))

        def eager():
            y = G.stages(cfg, ws, q, items)
            return torch.autograd.grad((y * dy).sum(), [q, items] + list(ws.values()))

        eng = mol.grad_engine()
        with torch.no_grad():
            qpack, _, _ = eng.query_pack(q.detach())
            cand = eng.build_index(items.detach().reshape(B * X, -1))
        if args.trace_child:
            for _ in range(1 + TRACE_CALLS):
                eng.pair_backward(qpack, B, cand, X, dy)
            torch.cuda.synchronize()
            continue
        a, b = ours(), eager()
        agree = max(float((x - y).norm() / y.norm()) for x, y in zip(a[:2], b[:2]))
        del a, b
        row = {"B": B, "X": X, "pairs": B * X,
               "ours_fwd_bwd_ms": timed(ours, args.warmup, args.reps), "eager_fwd_bwd_ms": timed(eager, args.warmup, args.reps),
               "pair_backward_all_ms": timed(lambda: eng.pair_backward(qpack, B, cand, X, dy), args.warmup, args.reps),
               "pair_backward_no_weights_ms": timed(lambda: eng.pair_backward(qpack, B, cand, X, dy, need=(True, True, False)), args.warmup, args.reps),
               "pair_forward_ms": timed(lambda: eng.score_candidates(qpack, B, cand, X), args.warmup, args.reps),
               "ours_peak_bytes": peak(ours), "eager_peak_bytes": peak(eager), "rel_l2_q_items_ours_vs_eager": agree}
        print(json.dumps(row))
        result["points"].append(row)
    if args.trace_child:
        return
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
