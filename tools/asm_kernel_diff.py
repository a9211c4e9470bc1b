#!/usr/bin/env python3
"""Compare kernels of two `make asm` outputs (curvis_amd/csrc/Makefile: build/asm/*.s and resource_usage.txt), one function at
a time: which kernels have the same instructions, which differ, which exist on one side only, and the registers and occupancy
of each.  Needs no GPU.

    make -C curvis_amd/csrc asm && cp -r build/asm /tmp/asm_before      # on the commit to compare against
    make -C curvis_amd/csrc asm                                          # on this one
    python tools/asm_kernel_diff.py /tmp/asm_before build/asm [--only REGEX] [--show]

A kernel's text is everything between its label and its .Lfunc_end label, with the assembler's function-local label numbers
(.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>) renumbered: they count the functions of the file and shift when one is added.  A kernel
template that gained a trailing template parameter is compared, in its instantiation with that parameter at its default (1 for a
factor, 0 for a switch), with its old self; so is a kernel that became a template with one such parameter, and one whose argument
type is spelled differently (such a kernel has a NEW mangled symbol with the old instructions: a profile or a rocprof filter keyed on
the full signature no longer matches it, one keyed on the name and template arguments does).
Exit status 1 when a kernel present on both sides differs."""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels_of(asm_dir):
    (path,) = glob.glob(os.path.join(asm_dir, "*amdgcn*.s"))
    bodies, name, lines = {}, None, []
    for line in open(path):
        if name is None:
            m = re.match(r"^(_Z\w+):\s", line)
            if m:
                name, lines = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            bodies[name] = [l.replace(name, "<this kernel>") for l in lines]
            name = None
            continue
        s = line.split(";")[0].rstrip() if not line.lstrip().startswith(";") else ""
        if s.strip():
            lines.append(re.sub(r"\.L(BB|tmp|func_end)\d+", r".L\1N", s))
    usage, cur = {}, None
    ru = os.path.join(asm_dir, "resource_usage.txt")
    if os.path.exists(ru):
        for line in open(ru):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = usage.setdefault(m.group(1), {})
            m = re.search(r"remark: [^:]*:\d+:\d+:\s+(VGPRs|AGPRs|TotalSGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|ScratchSize \[bytes/lane\]): (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return bodies, usage


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--only", default=".", help="regular expression on the demangled kernel name")
    ap.add_argument("--show", action="store_true", help="print the unified diff of kernels that differ")
    a = ap.parse_args()
    (b0, u0), (b1, u1) = kernels_of(a.before), kernels_of(a.after)
    names = demangle(sorted(set(b0) | set(b1)))
    # a kernel template that gained a trailing template parameter whose default (1: a factor, 0: a switch) is what it was before, or
    # a kernel that became a template with such a parameter (then "void name<0>(...)"): paired with its old name
    # (names are paired without their parameter lists: the type of a kernel's argument may be spelled through the new parameter)
    head = lambda d: d.replace("(anonymous namespace)::", "").split("(")[0] + "("  # noqa: E731
    old_of = {head(names[n]): n for n in b0}
    # a kernel whose argument type alone is spelled differently (through a template parameter it already had): the same name in front
    # of the parameter list
    for n in [n for n in b1 if n not in b0]:
        was = old_of.get(head(names[n]))
        if was is not None and was not in b1:
            b1[was], u1[was] = b1.pop(n), u1.pop(n, {})
            names[was] = names.pop(n)
    for pattern, to in ((r", 0>\(", ">("), (r"^void (.*)<0>\(", r"\1("), (r", 1>\(", ">(")):
        for n in [n for n in b1 if n not in b0 and re.search(pattern, head(names[n]))]:
            was = old_of.get(re.sub(pattern, to, head(names[n]), count=1))
            if was is not None and was not in b1:
                b1[was], u1[was] = b1.pop(n), u1.pop(n, {})
                names[was] = names.pop(n)
    fmt = lambda u: "VGPR %s AGPR %s SGPR %s occupancy %s LDS %s scratch %s" % tuple(  # noqa: E731
        u.get(k, "?") for k in ("VGPRs", "AGPRs", "TotalSGPRs", "Occupancy", "LDS", "ScratchSize"))
    differ = 0
    for n in sorted(names, key=names.get):
        d = names[n].replace("(anonymous namespace)::", "").split("(")[0]
        if not re.search(a.only, d):
            continue
        if n not in b0 or n not in b1:
            print("%-8s %s: %s" % ("new" if n in b1 else "gone", d, fmt((u1 if n in b1 else u0).get(n, {}))))
            continue
        same = b0[n] == b1[n] and u0.get(n) == u1.get(n)
        differ += not same
        print("%-8s %s: %s" % ("same" if same else "DIFFERS", d, fmt(u1.get(n, {}))))
        if not same:
            if u0.get(n) != u1.get(n):
                print("         before: %s" % fmt(u0.get(n, {})))
            if a.show:
                sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(b0[n], b1[n], "before", "after", lineterm="", n=2))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
