#!/usr/bin/env python3
"""Compare the kernels of two device assembly files (a refactor must not change an instruction).

    hipcc $(HIPFLAGS) --cuda-device-only -S -o old.s csrc/unit.hip     (the Makefile's HIPFLAGS)
    python scripts/kernel_isa_diff.py old.s new.s

A file may be the concatenation of several units' assembly. Kernels are matched by mangled name;
a kernel's text is its instructions and labels from its symbol to its .Lfunc_end, comments
dropped and the function index in .LBB<n>_ labels normalised. Exit status 1 on any difference.

Moving a kernel to another unit can by itself change it: the compiler carries the callers'
argument ranges into a unit-local helper before inlining it, so what else calls the helper in the
unit matters (contigs_probe_quad_kernel compiles `part & 2` of quad_reduce_scatter differently
without the protein probe beside it). To tell that from an edit, compare against the old code
compiled as the same unit.
"""
import re
import sys


def kernels(path):
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out = {}
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        if m.group(1) in names:
            lines = (re.sub(r";.*", "", ln).strip() for ln in m.group(2).split("\n"))
            out[m.group(1)] = [re.sub(r"\.LBB\d+_", ".LBB_", ln) for ln in lines if ln]
    assert set(out) == names, "kernel descriptors without a body: %s" % sorted(names - set(out))
    return out


if __name__ == "__main__":
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    missing, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    for tag, ks in (("missing", missing), ("new", added), ("different", differ)):
        for k in ks:
            print(tag, k)
    print("kernels: %d old, %d new; %d identical, %d different, %d missing, %d new" % (
        len(old), len(new), len(set(old) & set(new)) - len(differ), len(differ), len(missing),
        len(added)))
    sys.exit(1 if missing or added or differ else 0)
