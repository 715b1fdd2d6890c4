#!/usr/bin/env python3
"""Are the kernels of two sets of gfx950 assembly listings the same device code?

    hipcc <build.FLAGS> -S --cuda-device-only csrc/x.hip -o x.s        (once per translation unit and side)
    tools/isa_diff.py old/x.s -- new/x.s new/y.s new/z.s

For a change that only moves kernels between translation units.  Per kernel symbol (`.amdhsa_kernel`) it compares
  * the instruction lines and local labels of the function, trailing comments stripped and the function number in
    `.LBB<n>_` labels normalised, and
  * the kernel's `.amdhsa_*` descriptor block.
Kernels are matched by demangled base name with its template arguments (no namespace, no parameter list), so a kernel
keeps its identity when it moves into or out of a namespace.  Prints the kernels that only one side has and the ones
that differ, then a count line; exits 1 if anything differs or is unmatched.  It compares and does nothing else: it
reads listings on the CPU and never touches a GPU."""
import difflib
import os
import re
import shutil
import subprocess
import sys


def _cxxfilt():
    for name in ("llvm-cxxfilt", "c++filt", "/opt/rocm/llvm/bin/llvm-cxxfilt"):
        path = shutil.which(name)
        if path:
            return path
    sys.exit("isa_diff: no llvm-cxxfilt / c++filt found")


def base_names(symbols):
    """{mangled symbol: `name<template arguments>`}"""
    if not symbols:
        return {}
    out = subprocess.run([_cxxfilt()], input="\n".join(symbols) + "\n", capture_output=True, text=True, check=True).stdout
    names = {}
    for sym, dem in zip(symbols, out.splitlines()):
        dem = dem.replace("(anonymous namespace)::", "")
        depth, end = 0, len(dem)
        for i, ch in enumerate(dem):  # the parameter list opens at the first '(' outside template arguments
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                end = i
                break
        head = dem[:end].strip()
        depth = 0
        for i in range(len(head) - 1, -1, -1):  # drop a return type: cut at the last space outside template arguments
            if head[i] == ">":
                depth += 1
            elif head[i] == "<":
                depth -= 1
            elif head[i] == " " and depth == 0:
                head = head[i + 1:]
                break
        names[sym] = head
    return names


_LBB = re.compile(r"\.LBB\d+_")


def parse(path):
    """{mangled kernel symbol: (instruction lines, descriptor lines)} of one listing"""
    with open(path) as f:
        lines = f.read().splitlines()
    kernels = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]
    found = {}
    for sym in kernels:
        start = lines.index(next(ln for ln in lines if ln.startswith(sym + ":")))
        code, desc, in_desc = [], [], False
        for ln in lines[start + 1:]:
            text = ln.split(";", 1)[0].strip()
            if text.startswith(".Lfunc_end"):
                break
            if not text:
                continue
            if text.startswith(".amdhsa_kernel"):
                in_desc = True
            elif text.startswith(".end_amdhsa_kernel"):
                in_desc = False
            elif in_desc:
                desc.append(text)
            elif text.startswith(".LBB") or not text.startswith("."):  # a local label or an instruction, no directive
                code.append(_LBB.sub(".LBB_", text))
        found[sym] = (code, desc)
    return found


def load(paths):
    """{base name: (instruction lines, descriptor lines, listing)} of one side"""
    side = {}
    for path in paths:
        found = parse(path)
        names = base_names(list(found))
        for sym, (code, desc) in found.items():
            name = names[sym]
            if name in side:
                sys.exit(f"isa_diff: {name} is in both {side[name][2]} and {path}")
            side[name] = (code, desc, os.path.basename(path))
    return side


def main(argv):
    if "--" not in argv or argv[0] == "--" or argv[-1] == "--":
        sys.exit(__doc__)
    cut = argv.index("--")
    old, new = load(argv[:cut]), load(argv[cut + 1:])
    missing, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    for name in missing:
        print(f"only in the first set:  {name} ({old[name][2]})")
    for name in added:
        print(f"only in the second set: {name} ({new[name][2]})")
    ncode = ndesc = 0
    for name in sorted(set(old) & set(new)):
        for what, a, b in (("instructions", old[name][0], new[name][0]), ("descriptor", old[name][1], new[name][1])):
            if a == b:
                continue
            ncode, ndesc = ncode + (what == "instructions"), ndesc + (what == "descriptor")
            print(f"{name}: {what} differ ({old[name][2]}: {len(a)} lines, {new[name][2]}: {len(b)} lines)")
            for ln in list(difflib.unified_diff(a, b, old[name][2], new[name][2], lineterm="", n=1))[:40]:
                print("    " + ln)
    print(f"{len(old)} kernels against {len(new)}: {len(missing)} missing, {len(added)} new, "
          f"{ncode} differing instruction sequences, {ndesc} differing descriptors")
    return 1 if missing or added or ncode or ndesc else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
