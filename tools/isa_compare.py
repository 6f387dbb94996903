#!/usr/bin/env python3
"""Compare the gfx950 code of the same kernels in two checkouts, kernel by kernel (CPU only: hipcc cross-compiles, no GPU).

    tools/isa_compare.py BEFORE_TREE AFTER_TREE kvdec.hip hstu.hip ... [--map 'REGEX=REPLACEMENT' ...] [--only REGEX]

Each FILE of rails_amd/csrc is compiled in both trees with that tree's Makefile flags (CXXFLAGS and FLAGS_<file>) plus
`--cuda-device-only -S`.  A kernel's instruction lines are what is left of its body after dropping labels, directives and
comments (basic-block labels in branch targets lose their function number, which changes when kernels move).  Kernels are paired by
their demangled name without return type, namespace and parameter list; every --map is a re.sub applied to the names of both trees
first, for kernels whose names changed, e.g.
    --map 'kv_rows_kernel<(\\d), (\\w+), false, KvDecArgs>=kvdec_rows_kernel<\\1, \\2>'
One line per paired kernel, in the format of profiles/derived_tables_one_body_isa.txt:
    file kernel | instructions before -> after | sequence | VGPRs | SGPRs | scratch bytes
sequence: `identical` (the same lines in the same order), `same instructions, scheduled in another order` (the same multiset of
whole lines, operands and registers included), `same opcodes, other operands` (only the multiset of opcodes is the same) or
`different`.  Kernels found in one tree only are listed at the end.  Sequences are compared and nothing else."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def make_flags(csrc, stem):
    """CXXFLAGS (+ FLAGS_<stem>) and the compiler of a tree's Makefile."""
    var = {}
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"(\w+)\s*[:?]?=\s*(.*)$", line.rstrip("\n"))
        if m:
            var[m.group(1)] = m.group(2)
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
    return expand(var.get("HIPCC", "hipcc")), (expand(var["CXXFLAGS"]) + " " + expand(var.get("FLAGS_" + stem, ""))).split()


def assemble(tree, name, tmp, tag):
    csrc = os.path.join(tree, "rails_amd", "csrc")
    stem = os.path.splitext(name)[0]
    hipcc, flags = make_flags(csrc, stem)
    out = os.path.join(tmp, f"{tag}_{stem}.s")
    subprocess.run([hipcc, *flags, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", name, "-o", out], cwd=csrc, check=True)
    return open(out).read()


def demangle(names):
    tool = os.path.join(LLVM, "llvm-cxxfilt")
    out = subprocess.run([tool if os.path.exists(tool) else "c++filt", *names], capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def short(name):
    """`void mol::(anonymous namespace)::k<1, mol::A>(mol::A)` -> `k<1, A>`"""
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, c in enumerate(name):   # cut the parameter list: the first `(` outside the template arguments, the namespace aside
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0 and not name.startswith("(anonymous namespace)", i):
            name = name[:i]
            break
    return name.replace("(anonymous namespace)::", "").replace("mol::", "")


def kernels(asm):
    """{mangled name: (instruction lines, vgprs, sgprs, scratch bytes)} of the kernels of one assembly file."""
    lines = asm.splitlines()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
        if not (m and m.group(1) in names):
            i += 1
            continue
        name, body = m.group(1), []
        i += 1
        while i < len(lines) and not re.match(r"^\.Lfunc_end\d+:", lines[i]):
            text = lines[i].split(";")[0].strip()
            if text and not text.endswith(":") and not text.startswith("."):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", text)))
            i += 1
        note = {}
        while i < len(lines) and len(note) < 3 and not re.match(r"^[A-Za-z_][\w$.]*:", lines[i]):   # the resource notes behind the body
            m = re.match(r"^; (NumVgprs|TotalNumSgprs|ScratchSize): (\d+)", lines[i])
            if m:
                note[m.group(1)] = int(m.group(2))
            i += 1
        res[name] = (body, note.get("NumVgprs"), note.get("TotalNumSgprs"), note.get("ScratchSize"))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("files", nargs="+", help="sources of rails_amd/csrc, e.g. kvdec.hip")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPLACEMENT", help="rename kernels before pairing them")
    ap.add_argument("--only", default=None, help="print only kernels whose paired name matches")
    args = ap.parse_args()
    maps = [m.split("=", 1) for m in args.map]

    def keyed(asm):
        ks = kernels(asm)
        plain = demangle(list(ks)) if ks else {}
        out = {}
        for mangled, v in ks.items():
            key = short(plain[mangled])
            for pat, rep in maps:
                key = re.sub(pat, rep, key)
            out[key] = v
        return out

    print("kernel | instructions before -> after | sequence | VGPRs | SGPRs | scratch bytes")
    alone = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.files:
            a, b = keyed(assemble(args.before, name, tmp, "before")), keyed(assemble(args.after, name, tmp, "after"))
            for key in sorted(set(a) | set(b)):
                if args.only and not re.search(args.only, key):
                    continue
                if key not in a or key not in b:
                    alone.append(f"{name} {key}: only {'before' if key in a else 'after'}")
                    continue
                (ia, va, sa, xa), (ib, vb, sb, xb) = a[key], b[key]
                op = lambda seq: collections.Counter(l.split(" ")[0] for l in seq)
                verdict = ("identical" if ia == ib else
                           "same instructions, scheduled in another order" if collections.Counter(ia) == collections.Counter(ib) else
                           "same opcodes, other operands" if op(ia) == op(ib) else "different")
                print(f"{name} {key} | {len(ia)} -> {len(ib)} | {verdict} | {va} -> {vb} | {sa} -> {sb} | {xa} -> {xb}")
    for line in alone:
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
