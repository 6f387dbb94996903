#!/usr/bin/env python3
"""profiles/mol_grad_errors.json from a log of tests/test_mol_grad_gpu.py run with -s: the test prints, per
kernel-level case, the largest |kernel - float64| / bound of every output tensor (MOLGRAD) and its relative L2 error next to that of the
same chain in float32 (MOLGRADL2); per module-level tensor its relative L2 error next to eager fp32 autograd's (MOLGRADMOD); and the
losses of the SGD steps (MOLGRADSGD).
  python -m pytest tests/test_mol_grad_gpu.py -s -q > log.txt; python tools/mol_grad_errors.py log.txt [profiles/mol_grad_errors.json]
"""
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    txt = open(sys.argv[1]).read()
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mol_grad_errors.json")
    worst, l2, cases = collections.defaultdict(dict), collections.defaultdict(dict), collections.Counter()
    for m in re.finditer(r"MOLGRAD (\S+) (\d+) (\d+) ((?:\w+=[0-9.e+-]+ ?)+)", txt):
        tag = m.group(1)
        cases[tag] += 1
        for kv in m.group(4).split():
            k, v = kv.split("=")
            if k not in worst[tag] or float(v) > worst[tag][k]["ratio"]:
                worst[tag][k] = {"ratio": float(v), "B": int(m.group(2)), "X": int(m.group(3))}
    for m in re.finditer(r"MOLGRADL2 (\S+) (\d+) (\d+) ((?:\w+=[0-9.e+-]+/[0-9.e+-]+ ?)+)", txt):
        for kv in m.group(4).split():
            k, v = kv.split("=")
            ours, f32 = (float(t) for t in v.split("/"))
            ratio = ours / max(f32, 2.0 ** -25)
            if k not in l2[m.group(1)] or ratio > l2[m.group(1)][k]["ours_over_float32_chain"]:
                l2[m.group(1)][k] = {"ours_over_float32_chain": ratio, "ours_rel_l2": ours, "float32_chain_rel_l2": f32, "B": int(m.group(2)), "X": int(m.group(3))}
    mod = {}
    for m in re.finditer(r"MOLGRADMOD (\S+) (\S+) ours=(\S+) eager=(\S+) ratio=(\S+)", txt):
        t = mod.setdefault(m.group(1), {"largest_ratio": 0.0, "tensor": None, "tensors": 0})
        t["tensors"] += 1
        if float(m.group(5)) > t["largest_ratio"]:
            t.update(largest_ratio=float(m.group(5)), tensor=m.group(2), ours_rel_l2=float(m.group(3)), eager_rel_l2=float(m.group(4)))
    sgd = re.search(r"MOLGRADSGD (\[.*?\])", txt)
    out = {"what": "rails_mol_generic_pair_backward against the float64 analytic backward (tests/_mol_grad_ref.py), over B in {1, 3, 33} x X in "
                   "{1, 31, 32, 33, 130}: per shape and output tensor the largest |error| / bound (bound 2^-24 ((n + C) A + F)) and the largest "
                   "ratio of its relative L2 error to that of the same chain in float32; per module-level case the largest ratio of the relative "
                   "L2 error to fp32 eager autograd's; the SGD losses.  ONE run of tests/test_mol_grad_gpu.py on an MI355X.",
           "kernel_level": {k: {"cases": cases[k], "worst_over_bound": v, "worst_rel_l2": l2.get(k, {})} for k, v in sorted(worst.items())},
           "module_level": mod, "sgd_losses": json.loads(sgd.group(1)) if sgd else None}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for k, v in sorted(worst.items()):
        print(k, cases[k], {a: round(b["ratio"], 4) for a, b in v.items()}, {a: round(b["ours_over_float32_chain"], 2) for a, b in l2.get(k, {}).items()})
    for k, v in mod.items():
        print(k, v["largest_ratio"], v["tensor"])


if __name__ == "__main__":
    main()
