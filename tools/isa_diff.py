#!/usr/bin/env python3
r"""Compare the device code of two builds of the library, kernel by kernel.

    tools/isa_diff.py TREE_A TREE_B [--out DIR] [--jobs N] [--only a.hip,b.hip] [--lines N] [--rename 'OLD=NEW' ...]

Each TREE is a checkout (or any directory that holds aloception-oss_amd/csrc and include/).  Every .hip file of both trees is
compiled to gfx950 assembly with the command its own Makefile would use for the object file (`make -n`, so per-file flags such
as msda.hip's -fno-slp-vectorize are kept), `-c` replaced by `--offload-device-only -S`.  Per kernel the script compares

  * the resource figures of the code object's metadata (.vgpr_count, .agpr_count, .sgpr_count, .private_segment_fixed_size,
    .group_segment_fixed_size),
  * the instruction count and the count per opcode,
  * the instruction sequence in order, register numbers and a branch target's function ordinal (the N of `.LBBN_k`, which counts
    the functions of the file) ignored: class (a) identical, class (b) not.

A kernel that tree B renamed is paired by --rename OLD=NEW (repeatable): OLD is a regular expression, rewritten to NEW (re.sub)
in the short names of tree A's kernels, the ones the table prints (c++filt's spelling: `> >`), so groups carry template arguments
over, e.g. 'conv3x3_d2_kernel<([a-z]+)>=conv3x3_kernel<PlanS1<2>, \1>'.  The pair is then classed like any other and listed
as "old -> new".

Exit status 0: the same kernels on both sides, equal figures and equal counts everywhere (class (b) is reported, not an error).
Exit status 1: anything else.  The assembly is kept under --out (default: a temporary directory) as A/<file>.s and B/<file>.s.
"""
import argparse
import collections
import difflib
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("aloception-oss_amd", "csrc")
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")
REG = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")
LABEL = re.compile(r"\.LBB\d+_(\d+)")   # .LBB<function's ordinal in its file>_<block>: the ordinal moves when a kernel is added before it


def compile_command(tree, src, out):
    """The Makefile's own compile line for src's object file, turned into a device-only assembly build."""
    obj = src[:-4] + ".o"
    dry = subprocess.run(["make", "-C", os.path.join(tree, CSRC), "-n", "-B", obj], check=True, capture_output=True, text=True).stdout
    line = next(l for l in dry.splitlines() if src in l and " -c " in l)
    words = shlex.split(line)
    words[words.index("-c")] = "--offload-device-only"
    words[words.index("-o") + 1] = out
    return words + ["-S"]


def build(tree, src, out):
    if not os.path.exists(out):
        subprocess.run(compile_command(tree, src, out), check=True, cwd=os.path.join(tree, CSRC))
    return out


def parse(path):
    """{kernel: {"figures": {...}, "ops": [opcode, ...], "seq": [instruction with register numbers blanked, ...]}}"""
    bodies, meta, name, in_meta, cur = {}, [], None, False, None
    with open(path) as f:
        for raw in f:
            line = raw.rstrip("\n")
            if in_meta:  # the code object's YAML note: one "  - .key: value" block per kernel, its own keys at four spaces
                m = re.match(r"^  - \.(\w+):\s*(.*)$", line)
                if m:
                    cur = {}
                    meta.append(cur)
                m = m or re.match(r"^    \.(\w+):\s*(.*)$", line)
                if m and cur is not None:
                    cur[m.group(1)] = m.group(2).strip("'\"")
                if line.startswith("amdhsa.") and not line.startswith("amdhsa.kernels"):
                    cur = None
                in_meta = ".end_amdgpu_metadata" not in line
                continue
            if ".amdgpu_metadata" in line:
                in_meta, cur = True, None
                continue
            m = re.match(r"^([A-Za-z_][\w$.]*):", line)
            if m and not m.group(1).startswith(".L"):
                name = m.group(1)
                bodies[name] = []
                continue
            if line.startswith(".Lfunc_end"):
                name = None
                continue
            text = line.split(";")[0].strip()
            if name is None or not text or text.startswith(".") or text.endswith(":"):
                continue
            bodies[name].append(text)
    kernels = {}
    for k in meta:
        body = bodies.get(k.get("name"), [])
        kernels[k["name"]] = {
            "figures": {f: k.get(f, "?") for f in FIGURES},
            "ops": [t.split()[0] for t in body],
            "seq": [LABEL.sub(r".LBB#_\1", REG.sub(r"\1#", t)) for t in body],
        }
    return kernels


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        # kernel<template arguments> is what tells kernels apart: drop the namespaces and the parameter list
        short = [re.sub(r"\(.*$", "", o.replace("(anonymous namespace)::", "").replace("alo::", "").replace("void ", "", 1)) for o in out]
        return dict(zip(names, short if len(set(short)) == len(short) else out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--out", default=None, help="where the assembly goes (kept; existing files are reused)")
    ap.add_argument("--jobs", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--only", default=None, help="comma-separated .hip files instead of all")
    ap.add_argument("--lines", type=int, default=12, help="differing lines shown per class (b) kernel")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="pair tree A's kernel OLD (a regular expression over the short name) with tree B's kernel NEW; repeatable")
    args = ap.parse_args()
    renames = [r.split("=", 1) for r in args.rename]
    if any(len(r) != 2 for r in renames):
        ap.error("--rename takes OLD=NEW")
    out = args.out or tempfile.mkdtemp(prefix="isa_diff_")
    trees = {"A": os.path.abspath(args.tree_a), "B": os.path.abspath(args.tree_b)}
    srcs = {s: sorted(f for f in os.listdir(os.path.join(t, CSRC)) if f.endswith(".hip")) for s, t in trees.items()}
    if args.only:
        srcs = {s: [f for f in fs if f in args.only.split(",")] for s, fs in srcs.items()}
    jobs = []
    with ThreadPoolExecutor(args.jobs) as pool:
        for side, tree in trees.items():
            os.makedirs(os.path.join(out, side), exist_ok=True)
            for src in srcs[side]:
                jobs.append((side, src, pool.submit(build, tree, src, os.path.join(out, side, src[:-4] + ".s"))))
    kernels = {"A": {}, "B": {}}
    for side, src, job in jobs:
        for name, k in parse(job.result()).items():
            k["file"] = src
            kernels[side][name] = k

    # from here on a kernel goes by its short name; tree A's are rewritten by --rename first, so a renamed kernel meets its successor
    short = demangle(sorted(set(kernels["A"]) | set(kernels["B"])))
    pretty, keyed = {}, {"A": {}, "B": {}}
    for side in ("A", "B"):
        for mangled, k in kernels[side].items():
            name = short[mangled]
            if side == "A":
                for old, new in renames:
                    name = re.sub(old, new, name)
            if name in keyed[side]:
                sys.exit(f"isa_diff: two kernels of tree {side} are called {name} (after --rename)")
            keyed[side][name] = k
            if name != short[mangled]:
                pretty[name] = f"{short[mangled]} -> {name}"
    kernels = keyed
    names = sorted(set(kernels["A"]) | set(kernels["B"]))
    pretty = {n: pretty.get(n, n) for n in names}
    bad, same, reordered = [], 0, []
    print(f"{'file':18} {'instr':>7} {'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch':>7} {'lds':>7}  class  kernel")
    for n in names:
        a, b = kernels["A"].get(n), kernels["B"].get(n)
        if a is None or b is None:
            bad.append(f"{pretty[n]}: only in {'B' if a is None else 'A'}")
            continue
        why = [f"{f} {a['figures'][f]} -> {b['figures'][f]}" for f in FIGURES if a["figures"][f] != b["figures"][f]]
        if len(a["ops"]) != len(b["ops"]):
            why.append(f"instructions {len(a['ops'])} -> {len(b['ops'])}")
        ca, cb = collections.Counter(a["ops"]), collections.Counter(b["ops"])
        why += [f"{op} {ca[op]} -> {cb[op]}" for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]]
        cls = "DIFF" if why else ("a" if a["seq"] == b["seq"] else "b")
        fg = b["figures"]
        print(f"{b['file']:18} {len(b['ops']):7} {fg['vgpr_count']:>5} {fg['agpr_count']:>5} {fg['sgpr_count']:>5} "
              f"{fg['private_segment_fixed_size']:>7} {fg['group_segment_fixed_size']:>7}  {cls:5}  {pretty[n]}")
        if why:
            bad.append(f"{pretty[n]}: " + "; ".join(why))
        elif cls == "a":
            same += 1
        else:
            delta = [l for l in difflib.unified_diff(a["seq"], b["seq"], "A", "B", n=0, lineterm="") if not l.startswith(("---", "+++"))]
            reordered.append((pretty[n], delta))
    print(f"\n{len(names)} kernels: {same} in class (a), {len(reordered)} in class (b), {len(bad)} with unequal figures or counts")
    for name, delta in reordered:
        print(f"\n(b) {name}: {sum(l.startswith('-') for l in delta)} lines differ")
        for l in delta[:args.lines]:
            print("    " + l)
        if len(delta) > args.lines:
            print(f"    ... {len(delta) - args.lines} more")
    for line in bad:
        print("UNEQUAL " + line)
    print(f"assembly kept in {out}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
