#!/usr/bin/env python3
"""
Instruction census of the time loops of k_ode_sym kernels, from the compiler's assembly listing.

    hipcc <the flags of vgpa_amd/build.py> -S --cuda-device-only -gline-tables-only vgpa_amd/csrc/ode_mfma_m3.hip -o m3.s
    python tools/stepper_census.py m3.s 'ILi3ELb1ELi10ELb0ELi0ELi2ELb0ELb0ELb0ELb0ELb0E' 'ILi3ELb0ELi10ELb0ELi0ELi3ELb1ELb1ELb1ELb0ELb0E'
    python tools/stepper_census.py m3.s --resources      # registers and scratch of every k_ode_sym instantiation of the listing

For every kernel whose mangled name contains one of the given template-argument strings: the kernel's resource summary (registers,
scratch, LDS) and, for every loop of the kernel that holds matrix-core products or at least 100 instructions (a loop = a strongly
connected component of the kernel's control-flow graph, i.e. an outermost loop with everything nested in it), the count of each
instruction class in the loop body and the source lines (.loc) that the selects, the EXEC-masked regions and the integer address
arithmetic belong to.  Counts are static: an instruction inside a branch of the loop body counts once whether or not the branch is
taken.  The time loops of a kernel are told apart by their products: 280 per step = the product role (four-wave kernels: products and
chores in one loop), none = a helper role, the rest = the gradient role, whose loop body is TWO steps (one per operand set).
"""
import collections
import re
import sys

CLASSES = [
    ("mfma_f64", re.compile(r"^v_mfma_f64")),
    ("ds_read_b128", re.compile(r"^ds_read_b128")),
    ("ds_read other", re.compile(r"^ds_read")),
    ("ds_write", re.compile(r"^ds_write")),
    ("ds other (bpermute, swizzle)", re.compile(r"^ds_")),
    ("global_load", re.compile(r"^global_load")),
    ("global_store", re.compile(r"^global_store")),
    ("v_cndmask", re.compile(r"^v_cndmask")),
    ("v_cmp", re.compile(r"^v_cmpx?_")),
    ("fp64 valu", re.compile(r"^v_(fma|fmac|add|mul|max|min)_f64")),
    ("v_lshl_add_u64 / v_mad_u64_u32 / v_mul_lo_u32", re.compile(r"^v_(lshl_add_u64|mad_u64_u32|mad_i64_i32|mul_lo_u32|mul_hi_u32)")),
    ("v_lshl_add_u32 / v_add_lshl / v_add3", re.compile(r"^v_(lshl_add_u32|add_lshl_u32|add3_u32|lshl_or_b32|mad_u32_u24|mad_i32_i24)")),
    ("v_add / v_sub (32-bit int)", re.compile(r"^v_(add|sub|subrev)(_co)?_(u32|i32)|^v_addc_co_u32|^v_subb")),
    ("v_bitop3 / v_or / v_and / v_xor / shifts", re.compile(r"^v_(bitop3|or|and|xor|or3|and_or|lshlrev|lshrrev|ashrrev|bfe|not)_")),
    ("v_mov / v_accvgpr", re.compile(r"^v_(mov|accvgpr)")),
    ("v_readfirstlane / v_readlane", re.compile(r"^v_read(first)?lane")),
    ("other valu", re.compile(r"^v_")),
    ("s_mul_i32 / s_mul_hi", re.compile(r"^s_mul")),
    ("exec-masked regions (s_and_saveexec / s_or_saveexec)", re.compile(r"^s_(and|or|andn2)_saveexec")),
    ("s_cbranch", re.compile(r"^s_cbranch")),
    ("s_nop", re.compile(r"^s_nop")),
    ("s_waitcnt", re.compile(r"^s_waitcnt")),
    ("s_barrier", re.compile(r"^s_barrier")),
    ("other salu", re.compile(r"^s_")),
]
NON_FP64_VALU = ("v_cndmask", "v_cmp", "v_lshl_add_u64 / v_mad_u64_u32 / v_mul_lo_u32", "v_lshl_add_u32 / v_add_lshl / v_add3",
                 "v_add / v_sub (32-bit int)", "v_bitop3 / v_or / v_and / v_xor / shifts", "v_mov / v_accvgpr", "v_readfirstlane / v_readlane",
                 "other valu")
ATTRIBUTED = ("v_cndmask", "exec-masked regions (s_and_saveexec / s_or_saveexec)", "v_lshl_add_u64 / v_mad_u64_u32 / v_mul_lo_u32",
              "v_lshl_add_u32 / v_add_lshl / v_add3", "v_add / v_sub (32-bit int)", "s_mul_i32 / s_mul_hi")


def classify(op):
    for name, rx in CLASSES:
        if rx.match(op):
            return name
    return "other"


def kernels(lines):
    """(name, first line, last line) of every function in the listing"""
    start = None
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and start is None:
            start = (m.group(1), i)
        elif start and ln.startswith(".Lfunc_end"):
            yield start[0], start[1], i
            start = None


def census(lines, lo, hi):
    files, labels, body = {}, {}, []
    loc = None
    for i in range(lo, hi):
        ln = lines[i].strip()
        if not ln or ln.startswith(";"):
            continue
        m = re.match(r"^\.loc\s+(\d+)\s+(\d+)", ln)
        if m:
            loc = (int(m.group(1)), int(m.group(2)))
            continue
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            labels[m.group(1)] = len(body)
            continue
        if ln.startswith("."):
            continue
        op = ln.split()[0]
        body.append((op, ln, loc))
    # basic blocks and their successors; a loop = a strongly connected component of the control-flow graph (the block layout is not
    # in program order, so the span between a label and a backward branch to it says nothing)
    starts = sorted(set([0] + list(labels.values()) + [i + 1 for i, (op, _, _) in enumerate(body) if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc"))]))
    starts = [s for s in starts if s < len(body)]
    block_of = {s: n for n, s in enumerate(starts)}
    succ = [[] for _ in starts]
    for n, s in enumerate(starts):
        e = starts[n + 1] if n + 1 < len(starts) else len(body)
        op, ln, _ = body[e - 1]
        if op.startswith(("s_cbranch", "s_branch")):
            tgt = ln.split()[-1]
            if tgt in labels and labels[tgt] in block_of:
                succ[n].append(block_of[labels[tgt]])
        if not op.startswith(("s_branch", "s_endpgm", "s_setpc")) and n + 1 < len(starts):
            succ[n].append(n + 1)
    index, low, on, stack, comps, counter = {}, {}, set(), [], [], [0]
    for root in range(len(starts)):              # Tarjan, iterative
        if root in index:
            continue
        work = [(root, 0)]
        while work:
            v, i = work.pop()
            if i == 0:
                index[v] = low[v] = counter[0]; counter[0] += 1
                stack.append(v); on.add(v)
            if i < len(succ[v]):
                work.append((v, i + 1))
                w = succ[v][i]
                if w not in index:
                    work.append((w, 0))
                elif w in on:
                    low[v] = min(low[v], index[w])
            else:
                if low[v] == index[v]:
                    comp = []
                    while True:
                        w = stack.pop(); on.discard(w); comp.append(w)
                        if w == v:
                            break
                    if len(comp) > 1 or v in succ[v]:
                        comps.append(sorted(comp))
                if work:
                    u = work[-1][0]
                    low[u] = min(low[u], low[v])
    out = []
    for comp in sorted(comps):
        cnt = collections.Counter()
        src = collections.defaultdict(collections.Counter)
        for n in comp:
            e = starts[n + 1] if n + 1 < len(starts) else len(body)
            for op, ln, loc in body[starts[n]:e]:
                c = classify(op)
                cnt[c] += 1
                if c in ATTRIBUTED:
                    src[c][loc] += 1
        if cnt["mfma_f64"] or sum(cnt.values()) >= 100:
            out.append((starts[comp[0]], len(comp), cnt, src))
    return out


def file_table(lines):
    t = {}
    for ln in lines:
        m = re.match(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', ln)
        if m:
            t[int(m.group(1))] = (m.group(3) or m.group(2)).split("/")[-1]
    return t


def summary(lines, name):
    keys = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
            ".group_segment_fixed_size")
    for i, ln in enumerate(lines):
        if ln.strip() == ".name:           " + name or ln.strip() == ".name: " + name:
            got = {}
            j = i
            while j > 0 and not lines[j].lstrip().startswith("- .agpr_count") and not lines[j].lstrip().startswith("- .args"):
                j -= 1
            while j < len(lines) and len(got) < len(keys) and j < i + 40:
                s = lines[j].strip().lstrip("- ")
                for k in keys:
                    if s.startswith(k + ":"):
                        got[k] = s.split(":")[1].strip()
                j += 1
            return got
    return {}


def main():
    path, wanted = sys.argv[1], sys.argv[2:]
    lines = open(path).read().split("\n")
    files = file_table(lines)
    if "--resources" in wanted:
        print("%-86s %5s %5s %8s" % ("k_ode_sym<METHOD, FWD, NB, DENSEJ, GR, WPE, QOUT, HLP, GF, H2, PJ>", "VGPRs", "SGPRs", "scratch"))
        worst = 0
        for name, lo, hi in kernels(lines):
            if "k_ode_sym" in name:
                r = summary(lines, name)
                args = re.sub(r"L[ib](\d+)E", r"\1,", name.split("k_ode_symI")[1].split("EEv")[0] + "E").rstrip(",")
                print("%-86s %5s %5s %8s" % ("<" + args + ">", r.get(".vgpr_count"), r.get(".sgpr_count"), r.get(".private_segment_fixed_size")))
                worst = max(worst, int(r.get(".private_segment_fixed_size", 0)))
        print("largest scratch of any k_ode_sym instantiation: %d bytes" % worst)
        return
    for name, lo, hi in kernels(lines):
        if "k_ode_sym" not in name or not any(w in name for w in wanted):
            continue
        print("=" * 120)
        print(name)
        print("  " + "  ".join("%s=%s" % (k.lstrip("."), v) for k, v in summary(lines, name).items()))
        print("  (dynamic LDS: the launch passes SGeo::LDS_DOUBLES (+ GradLds::DOUBLES) * 8 bytes; group_segment_fixed_size is the static part)")
        for n, (a, b, cnt, src) in enumerate(census(lines, lo, hi)):
            total = sum(cnt.values())
            nonfp = sum(cnt[c] for c in NON_FP64_VALU)
            print("-" * 120)
            role = ("product role, one step" if cnt["mfma_f64"] == 280 else "helper role, one step" if not cnt["mfma_f64"]
                    else "gradient role, TWO steps")
            print("  loop %d (%s): %d instructions; non-fp64 vector-ALU %d, scalar multiplies %d -> %d" %
                  (n, role, total, nonfp, cnt["s_mul_i32 / s_mul_hi"], nonfp + cnt["s_mul_i32 / s_mul_hi"]))
            for cname, _ in CLASSES + [("other", None)]:
                if cnt[cname]:
                    print("    %-58s %5d" % (cname, cnt[cname]))
            for cname in ATTRIBUTED:
                if src[cname]:
                    known = sorted((loc, k) for loc, k in src[cname].items() if loc is not None)
                    if known:
                        print("    source of %s: %s" % (cname, ", ".join("%s:%d x%d" % (files.get(f, "?"), l, k) for (f, l), k in known)))


if __name__ == "__main__":
    main()
