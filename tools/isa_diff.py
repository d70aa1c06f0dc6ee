#!/usr/bin/env python3
"""Device assembly of kernel sources, a parent checkout against this tree, kernel by kernel.  Needs no GPU.

Every named .hip file of ideas_amd/csrc is compiled with the flags of tools/isa.sh (hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -S
--cuda-device-only), once from the parent checkout and once from this tree.  Per kernel the instruction stream (labels kept, comments
and directives dropped) is compared as text; for a kernel that differs the assembler's own resource lines are listed: instructions,
VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes per lane, waves per SIMD (Occupancy).  The exit status is 1 if a kernel that differs
uses scratch, changes its LDS bytes or loses waves per SIMD.

    git worktree add /tmp/parent HEAD~1
    python tools/isa_diff.py --parent /tmp/parent --title "..." --out profiles/x_isa.txt stego.hip attack.hip ...
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-S", "--cuda-device-only"]
RES = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("sgpr", "TotalNumSgprs"), ("lds", "LDSByteSize"), ("scratch", "ScratchSize"), ("waves", "Occupancy"))


def kernels(root, name, tmp):
    """{demangled kernel: (instruction lines, {resource: int})} of one source of a checkout"""
    out = os.path.join(tmp, name + ".s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(root, "ideas_amd", "csrc", name), "-o", out], check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    plain = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    found = {}
    for sym, dem in zip(names, plain):
        body = text[text.index("\n%s:" % sym):]
        body = body[:body.index(".Lfunc_end")]
        ins = []
        for ln in body.split("\n")[2:]:
            code = ln.split(";")[0].rstrip()
            if not code.strip() or code.strip().startswith(".") and not code.strip().endswith(":"):
                continue
            ins.append(re.sub(r"\.LBB\d+_", ".LBB_", code.strip()))
        tail = text[text.index(".Lfunc_end", text.index("\n%s:" % sym)):]
        res = {k: int(re.search(r";\s*%s:\s*(\d+)" % key, tail).group(1)) for k, key in RES}
        res["instructions"] = sum(1 for i in ins if not i.endswith(":"))
        short = re.sub(r"\(anonymous namespace\)::", "", dem)
        short = re.sub(r"^void ", "", short)
        depth, cut = 0, len(short)
        for i, ch in enumerate(short):                  # drop the parameter list: the first '(' outside the template arguments
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                cut = i
                break
        found[short[:cut]] = (ins, res)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="root of a checkout of the parent commit")
    ap.add_argument("--title", default="Device assembly, parent commit against this tree, kernel by kernel")
    ap.add_argument("--out", required=True)
    ap.add_argument("files", nargs="+")
    args = ap.parse_args()
    lines = [args.title, "=" * len(args.title), "",
             "How: every .hip file with the flags of tools/isa.sh (hipcc %s), once from the parent commit's csrc and once from this tree's "
             "(tools/isa_diff.py); per kernel the instruction stream (labels kept, comments and directives dropped) is compared as text, and "
             "for a kernel that differs the assembler's own resource lines are listed: VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes per "
             "lane, waves per SIMD (Occupancy)." % " ".join(FLAGS), "", "%-24s %8s %11s %8s" % ("file", "kernels", "identical", "differ")]
    detail, bad = [], []
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for name in args.files:
            a, b = kernels(args.parent, name, ta), kernels(ROOT, name, tb)
            assert sorted(a) == sorted(b), (name, "the two trees have different kernels", sorted(set(a) ^ set(b)))
            diff = [k for k in sorted(a) if a[k][0] != b[k][0]]
            lines.append("%-24s %8d %11d %8d" % (name, len(a), len(a) - len(diff), len(diff)))
            for k in sorted(a):                         # the three conditions hold for every kernel, identical stream or not
                ra, rb = a[k][1], b[k][1]
                if rb["scratch"] or rb["lds"] != ra["lds"] or rb["waves"] < ra["waves"]:
                    bad.append("%s: %s" % (name, k))
            if diff:
                detail += ["", name, "%-50s %16s %11s %9s %9s %15s %9s %7s" % ("kernel", "instructions", "vgpr", "agpr", "sgpr", "lds", "scratch", "waves")]
                for k in diff:
                    ra, rb = a[k][1], b[k][1]
                    detail.append("%-50s %6d -> %6d %4d -> %4d %3d -> %3d %3d -> %3d %6d -> %6d %3d -> %3d %2d -> %2d" % (
                        k, ra["instructions"], rb["instructions"], ra["vgpr"], rb["vgpr"], ra["agpr"], rb["agpr"], ra["sgpr"], rb["sgpr"],
                        ra["lds"], rb["lds"], ra["scratch"], rb["scratch"], ra["waves"], rb["waves"]))
    lines += ["", "Kernels that differ (parent -> this tree)", "-----------------------------------------"] + (detail or ["", "none"])
    lines += ["", "Scratch 0, LDS bytes unchanged and waves per SIMD not lower than the parent's, in every kernel: %s"
              % ("yes" if not bad else "NO -- " + "; ".join(bad))]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
