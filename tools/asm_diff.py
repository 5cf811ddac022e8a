#!/usr/bin/env python
"""Kernel-by-kernel comparison of two gfx950 assembly files of the same source at two commits
(build.py's flags plus `--cuda-device-only -S`): proves that a refactor left the instruction streams alone.

    python tools/asm_diff.py OLD.s NEW.s [--rename REGEX=REPL ...]

A kernel is the text from its label to .Lfunc_end, comments dropped, its own symbol and the function ordinal inside
block labels (.LBB<ordinal>_<n>) normalised, section directives dropped (a kernel that became a template instantiation
moves from .text into a comdat group), plus its .amdhsa_ descriptor (registers, LDS, scratch).  --rename rewrites
OLD's mangled kernel names before matching (a dropped template parameter).  Prints the kernels that differ, that
disappeared and that are new; exit status 1 if any differ or are new.
"""
import argparse
import re
import sys


def kernels(path):
    lines = [l.strip() for l in open(path).read().splitlines()]
    names = [l.split()[1] for l in lines if l.startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        beg = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(beg, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d0 = lines.index(".amdhsa_kernel " + name)
        d1 = next(i for i in range(d0, len(lines)) if lines[i] == ".end_amdhsa_kernel")
        body = []
        for l in lines[beg + 1:end] + lines[d0 + 1:d1]:
            l = l.split(";")[0].strip().replace(name, "@self")
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)
            if l == ".text" or l.startswith(".section"):
                continue        # where the linker puts the function (a template instantiation sits in a comdat group)
            if l:
                body.append(l)
        out[name] = body
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    a = ap.parse_args()
    args = [a.old, a.new]
    old, new = kernels(a.old), kernels(a.new)
    for r in a.rename:
        pat, repl = r.split("=", 1)
        old = {re.sub(pat, repl, k): v for k, v in old.items()}
    differ = [k for k in old if k in new and old[k] != new[k]]
    gone = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    same = len(old) - len(differ) - len(gone)
    print("%s: %d kernels -> %d; identical %d, differ %d, gone %d, new %d"
          % (args[1], len(old), len(new), same, len(differ), len(gone), len(added)))
    for tag, ks in (("DIFFERS", differ), ("gone", gone), ("NEW", added)):
        for k in ks:
            print("  %s %s" % (tag, k))
    for k in differ:
        n = next((i for i, (a, b) in enumerate(zip(old[k], new[k])) if a != b), min(len(old[k]), len(new[k])))
        print("  first difference of %s at line %d of %d / %d" % (k, n, len(old[k]), len(new[k])))
    return 1 if differ or added else 0


if __name__ == "__main__":
    sys.exit(main())
