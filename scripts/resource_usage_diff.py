#!/usr/bin/env python3
"""Compile-only comparison of two builds of the kernels (no GPU needed).

Each build directory holds, per source file NAME.hip compiled with the Makefile's flags plus
`-Rpass-analysis=kernel-resource-usage --save-temps`, the remarks in NAME.remarks (the compiler's
stderr) and the device assembly NAME-hip-amdgcn-amd-amdhsa-gfx950.s.

    python scripts/resource_usage_diff.py PARENT_DIR TREE_DIR > profiles/acc_resource_usage.txt

Reports, per kernel symbol present in both builds, VGPRs, AGPRs, scratch, LDS and occupancy and
whether they are equal; the symbols only the tree has, with theirs; and for every kernel of
blind_rotate_v6 present in both builds whether its 500-step loop has the same instructions: the loop
is the longest run of the function's instructions between a label and the last backward branch to
it, compared as text with label names replaced by their order of appearance and the offsets of
scalar loads from the kernel-argument segment left out (they are counted and reported)."""
import glob
import os
import re
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def remarks(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.remarks"))):
        name = None
        for line in open(path):
            m = re.search(r"remark: .*?(Function Name|[A-Za-z]+(?: [A-Za-z\[\]/]+)*): (.+)$", line.strip())
            if not m:
                continue
            k, v = m.group(1).strip(), m.group(2).replace("[-Rpass-analysis=kernel-resource-usage]", "").strip()
            if k == "Function Name":
                name = v
                out[name] = {"file": os.path.basename(path)[:-8]}
            elif name:
                out[name][k] = v
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split("\n")))
    except Exception:
        return {n: n for n in names}


def functions(asm_path):
    """symbol -> list of instruction lines (comments stripped), labels kept as 'L:<name>'"""
    out, cur = {}, None
    for line in open(asm_path):
        s = line.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+):", s)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if re.match(r"^\s*\.(end_amdhsa_kernel|Lfunc_end)", s) or s.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            cur.append("L:" + m.group(1))
        elif s.startswith("\t") and not s.strip().startswith("."):
            cur.append(" ".join(s.split()))
    return out


def main_loop(ins):
    """the longest label .. backward-branch span, labels renamed by order of appearance"""
    pos = {x[2:]: i for i, x in enumerate(ins) if x.startswith("L:")}
    best = (0, 0)
    for i, x in enumerate(ins):
        m = re.match(r"s_cbranch_\w+ (\.LBB\w+)|s_branch (\.LBB\w+)", x)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in pos and pos[tgt] < i and i - pos[tgt] > best[1] - best[0]:
                best = (pos[tgt], i + 1)
    body = ins[best[0]:best[1]]
    order = {}
    norm = []
    for x in body:
        for lab in re.findall(r"\.LBB\w+", x):
            order.setdefault(lab, f"L{len(order)}")
        norm.append(re.sub(r"\.LBB\w+", lambda m: order[m.group(0)], x))
    return [x for x in norm if not x.startswith("L:")]


def main():
    parent, tree = sys.argv[1], sys.argv[2]
    rp, rt = remarks(parent), remarks(tree)
    names = demangle(sorted(set(rp) | set(rt)))
    short = lambda n: re.sub(r"\(anonymous namespace\)::|tfhe_amd::|^void ", "", names[n])

    # The gate kernels gained a trailing template flag (the tlwe form, false for every instantiation
    # the parent has); later the rows kernels gained the same flag and a trailing kernel argument (the
    # accumulator samples, null in those instantiations): a tree kernel is matched with the parent's by
    # its name, or by its name without the flag (and that argument) where the parent has no kernel of
    # the full name.  The automaton kernel gained a trailing flag the same way (the transition weights).
    parent_names = {short(n) for n in rp}

    def key(n):
        k = short(n)
        if k in parent_names:
            return k
        k = re.sub(r"^(k_blind_rotate_v(?:6p?|4)(?:_rows)?<[^>]*|k_tgsw_dfa_v4<[^>]*), false>", r"\1>", k)
        return k if k in parent_names else re.sub(r"^(k_blind_rotate_v(?:6|4)_rows<.*), int const\*\)$", r"\1)", k)
    by_key = {short(n): n for n in rp}
    rt_all = rt
    rp = {n: rp[by_key[key(n)]] for n in rt if key(n) in by_key}       # parent figures under the tree's symbol
    parent_only = sorted(set(by_key) - {key(n) for n in rt})
    rt = rt_all
    row = lambda r: "  ".join(f"{r.get(k, '?'):>6}" for k in FIELDS)
    print("kernel resource usage, parent against tree (hipcc -O3 --offload-arch=gfx950 -munsafe-fp-atomics "
          "-Rpass-analysis=kernel-resource-usage)")
    print("columns: VGPRs  AGPRs  scratch bytes/lane  LDS bytes/block  occupancy waves/SIMD\n")
    changed = 0
    print("== kernels in both builds")
    for n in sorted(set(rp) & set(rt), key=short):
        same = all(rp[n].get(k) == rt[n].get(k) for k in FIELDS)
        changed += not same
        print(f"{'same   ' if same else 'CHANGED'} {row(rt[n])}  {short(n)}")
        if not same:
            print(f"  parent  {row(rp[n])}")
    print(f"\n{len(set(rp) & set(rt))} kernels in both builds, {changed} with a changed figure; "
          f"{len(parent_only)} only in the parent {parent_only}\n")
    print("== kernels only in the tree")
    for n in sorted(set(rt) - set(rp), key=short):
        print(f"new     {row(rt[n])}  {short(n)}")
    asm = "blind_rotate_v6-hip-amdgcn-amd-amdhsa-gfx950.s"
    fp, ft = functions(os.path.join(parent, asm)), functions(os.path.join(tree, asm))
    fp = {n: fp[by_key[key(n)]] for n in ft if n in rt and key(n) in by_key and by_key[key(n)] in fp}
    print("\n== blind_rotate_v6: the 500-step loop of every kernel in both builds")
    differ = 0
    for n in sorted(set(fp) & set(ft), key=short):
        lp, lt = main_loop(fp[n]), main_loop(ft[n])
        # BrInput grew, so the kernel arguments behind it moved: a scalar load from the kernel-argument
        # segment inside the loop keeps its instruction and registers and changes its offset only
        karg = lambda ins: [re.sub(r"^(s_load_dword\w* \S+ s\[\d+:\d+\],) 0x[0-9a-f]+$", r"\1 KARG", x) for x in ins]
        moved = sum(x != y for x, y in zip(lp, lt)) if len(lp) == len(lt) else -1
        same = karg(lp) == karg(lt)
        differ += not same
        note = f"  ({moved} kernel-argument load offset{'s' if moved != 1 else ''} moved)" if same and moved else ""
        print(f"{'same   ' if same else 'DIFFERS'} {len(lt):>6} instructions  {short(n)}{note}")
    print(f"\n{differ} loops differ")
    return 1 if changed or differ else 0


if __name__ == "__main__":
    sys.exit(main())
