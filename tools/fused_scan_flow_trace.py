#!/usr/bin/env python3
"""One fixed, seeded pass over the calls of the candidate modules, for an A/B of two trees (profiles/fused_scan_flow_kernels_*.txt):
MoLAvgTopK / MoLNaiveTopK / MoLCombTopK at 8x8x32, N = 4 037, B = 5 and 33, both scans on the fused route; unrestricted, half hidden and under a
per-row allowed_tags=; DEVICE_REDO_BYTES at its default and at 0; forward, get_top_k_outputs with a 61-wide seen list and without,
submit / result.  Inputs and calls are those of tests/test_hidden_items_gpu.py and tests/test_item_tags_gpu.py.
  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/fused_scan_flow_trace.py [--tree OTHER_TREE] --out outputs.pt
  python tools/fused_scan_flow_trace.py --kernels DIR           # that trace's kernels in dispatch order: a code per kernel, then the sequence
--tree: the directory rails_amd is imported from (another checkout, with RAILS_AMD_LIBRARY naming this tree's library)."""
import argparse
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=ROOT)
ap.add_argument("--out", default="")
ap.add_argument("--kernels", default="")
a = ap.parse_args()
if a.kernels:      # the trace's directory, or a file of names, one per line
    if os.path.isdir(a.kernels):
        path, = glob.glob(os.path.join(a.kernels, "**", "*kernel_trace.csv"), recursive=True)
        with open(path, newline="") as f:      # (Dispatch_Id: the order of the host's launches)
            names = [r["Kernel_Name"] for r in sorted(csv.DictReader(f), key=lambda r: int(r.get("Dispatch_Id") or r["Correlation_Id"]))]
    else:
        names = open(a.kernels).read().splitlines()
    # a short code per distinct kernel in order of first appearance, then the sequence of codes
    labels = {}
    for n in names:
        labels.setdefault(n, f"k{len(labels) + 1:02d}")
    print(f"{len(names)} launches of {len(labels)} kernels, in the order of the host's launches; code*N: N launches in a row")
    for n, lab in labels.items():
        print(f"{lab} = {n}")
    runs = []
    for n in names:
        if runs and runs[-1][0] == labels[n]:
            runs[-1][1] += 1
        else:
            runs.append([labels[n], 1])
    words = [lab if c == 1 else f"{lab}*{c}" for lab, c in runs]
    line = ""
    for w in words + [None]:
        if w is None or len(line) + len(w) > 150:
            print(line.rstrip())
            line = ""
        line += (w or "") + " "
    sys.exit(0)
sys.path[:0] = [os.path.abspath(a.tree), ROOT]
import torch  # noqa: E402

import rails_amd  # noqa: E402
from tests import test_hidden_items_gpu as H  # noqa: E402
from tests import test_index_update_gpu as U  # noqa: E402
from tests import test_item_tags_gpu as TG  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(rails_amd.__file__))) == os.path.abspath(a.tree), rails_amd.__file__
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(61)
outs = {}
default_redo = rails_amd.MoLAvgTopK.DEVICE_REDO_BYTES
with torch.inference_mode():
    for batch in (5, 33):
        cfg, mol, aux, q = H.shape_setup("8x8x32", dev, batch)
        X, ids = U.table(cfg, H.N, 7, dev), U.ids_of(H.N, dev)
        tags = TG.tag_layout(H.N, g).to(dev)
        hide = torch.randperm(H.N, generator=g)[: H.N // 2]      # 2 019 of 4 037 stay visible: still the fused route
        mix = [TG.MIX[b % 4] for b in range(batch)]
        for kind in ("avg", "naive", "comb"):
            for redo_bytes in (default_redo, 0):
                rails_amd.MoLAvgTopK.DEVICE_REDO_BYTES = redo_bytes
                tk = H.routed(H.MAKERS[kind](mol, X.clone().unsqueeze(0), ids.clone().unsqueeze(0)), H.FUSED)
                tk.set_item_tags(tags)
                for state in ("unrestricted", "half hidden", "allowed_tags"):
                    if state == "half hidden":
                        tk.hide_items(hide)
                    elif state == "allowed_tags":
                        tk.unhide_items(hide)
                    got, _ = H.approx_calls(tk, q, ids, X, dict(aux, allowed_tags=mix) if state == "allowed_tags" else aux)
                    for name, value in got.items():
                        outs[f"{kind}, B = {batch}, redo bytes {redo_bytes}, {state}: {name}"] = tuple(t.cpu() for t in value)
                rails_amd.MoLAvgTopK.DEVICE_REDO_BYTES = default_redo
    torch.cuda.synchronize()
if a.out:
    torch.save(outs, a.out)
print(f"{len(outs)} outputs from {os.path.abspath(a.tree)}")
