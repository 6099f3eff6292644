#!/usr/bin/env python3
"""
Instruction census of a source-line range of one kernel, from the compiler's assembly listing (a sibling of tools/stepper_census.py,
which knows the time loops of k_ode_sym only).

    hipcc <the flags of vgpa_amd/build.py> -S --cuda-device-only -gline-tables-only vgpa_amd/csrc/energy.hip -o energy.s
    python tools/kernel_census.py energy.s k_energy_l96_rILi10ELb0E 1107-1200 [161-240 ...]

The kernel: the one function of the listing whose mangled name contains the given string.  Its registers and scratch come first.  Then
every instruction whose line-table entry (.loc, of the innermost inlined function) falls into one of the given line ranges is counted by
class -- v_mfma by shape, ds_read*, ds_write*, other ds, global loads and stores, fp64 vector arithmetic, other vector, scalar, waits --
once for the ranges as a whole and once per basic block of the listing that holds a matrix-core product or at least eight LDS reads of
the ranges.  Counts are static: the blocks tell apart the branches of which a launch executes one (the three output layouts of the
Lorenz-96 energy kernel's phase 5 are three such blocks; the packed one is the block whose stores are masked by col <= row).
It only counts mnemonics.
"""
import collections
import re
import sys

from stepper_census import kernels, summary

CLASSES = [
    ("v_mfma_f64_16x16x4", re.compile(r"^v_mfma_f64_16x16x4")),
    ("v_mfma_f64_4x4x4", re.compile(r"^v_mfma_f64_4x4x4")),
    ("ds_read2 / ds_read_b128", re.compile(r"^ds_read(2|_b128)")),
    ("ds_read_b64 / b32", re.compile(r"^ds_read")),
    ("ds_write", re.compile(r"^ds_write")),
    ("ds other (bpermute, swizzle)", re.compile(r"^ds_")),
    ("global_load", re.compile(r"^global_load")),
    ("global_store", re.compile(r"^global_store")),
    ("fp64 valu", re.compile(r"^v_(fma|fmac|add|mul|max|min)_f64")),
    ("other valu", re.compile(r"^v_")),
    ("s_waitcnt", re.compile(r"^s_waitcnt")),
    ("s_nop", re.compile(r"^s_nop")),
    ("other salu", re.compile(r"^s_")),
]


def classify(op):
    for name, rx in CLASSES:
        if rx.match(op):
            return name
    return "other"


def show(title, cnt):
    print("-" * 100)
    print("  %s: %d instructions" % (title, sum(cnt.values())))
    for name, _ in CLASSES + [("other", None)]:
        if cnt[name]:
            print("    %-40s %5d" % (name, cnt[name]))


def main():
    path, want, ranges = sys.argv[1], sys.argv[2], [tuple(int(v) for v in r.split("-")) for r in sys.argv[3:]]
    lines = open(path).read().split("\n")
    hits = [(n, lo, hi) for n, lo, hi in kernels(lines) if want in n]
    if len(hits) != 1:
        raise SystemExit("%d kernels of the listing contain %r" % (len(hits), want))
    name, lo, hi = hits[0]
    print(name)
    print("  " + "  ".join("%s=%s" % (k.lstrip("."), v) for k, v in summary(lines, name).items()))
    print("  lines counted: " + ", ".join("%d-%d" % r for r in ranges))
    whole, blocks, label, loc = collections.Counter(), collections.OrderedDict(), "entry", None
    for i in range(lo + 1, hi):
        ln = lines[i].strip()
        if not ln or ln.startswith(";"):
            continue
        m = re.match(r"^\.loc\s+\d+\s+(\d+)", ln)
        if m:
            loc = int(m.group(1))
            continue
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            label = m.group(1)
            continue
        if ln.startswith("."):
            continue
        if loc is not None and any(a <= loc <= b for a, b in ranges):
            c = classify(ln.split()[0])
            whole[c] += 1
            blocks.setdefault(label, collections.Counter())[c] += 1
    show("all blocks", whole)
    for label, cnt in blocks.items():
        reads = cnt["ds_read2 / ds_read_b128"] + cnt["ds_read_b64 / b32"]
        if cnt["v_mfma_f64_16x16x4"] or cnt["v_mfma_f64_4x4x4"] or reads >= 8:
            show("block %s" % label, cnt)


if __name__ == "__main__":
    main()
