#!/usr/bin/env python3
"""Device code of two builds of kernels.hip, function by function.  Needs no GPU: it reads the assembly hipcc writes with the
library's flags plus --cuda-device-only -S.

usage: tools/isa_identity.py PARENT.s THIS.s

Labels, comments and directives are stripped, so two functions compare equal when they hold the same instructions with the same
operands in the same order.  Prints how many functions are identical, different, or in one build only, the identical ones by kernel
family, and for every differing function both instruction counts and the resources the assembler reports for it (NumVgprs, NumSgprs,
ScratchSize, Occupancy, the spill counts and the static LDS of the kernel's metadata), a changed resource marked `->`.
Exit status 1 if any function of THIS.s needs more of a resource than the parent's (fewer waves per SIMD for Occupancy), 0 otherwise."""
import collections
import re
import subprocess
import sys

# resource -> the pattern of its line; the first four come from the "; Kernel info:" block behind a function, the others from the
# kernel's entry of the amdhsa metadata at the end of the file
INFO = {"NumVgprs": r"^; NumVgprs: (\d+)", "NumSgprs": r"^; (?:Total)?NumSgprs: (\d+)", "ScratchSize": r"^; ScratchSize: (\d+)",
        "Occupancy": r"^; Occupancy: (\d+)"}
META = {"sgpr_spill": r"^\s*\.sgpr_spill_count:\s*(\d+)", "vgpr_spill": r"^\s*\.vgpr_spill_count:\s*(\d+)",
        "LDS": r"^\s*\.group_segment_fixed_size:\s*(\d+)"}
COLUMNS = ["NumVgprs", "NumSgprs", "ScratchSize", "Occupancy", "sgpr_spill", "vgpr_spill", "LDS"]
MORE_IS_BETTER = {"Occupancy"}


def read(path):
    """{symbol: [instruction, ...]}, {symbol: {resource: value}}"""
    code, res = {}, collections.defaultdict(dict)
    cur = last = None
    meta = {}
    functions = set()
    for line in open(path, errors="replace"):
        if cur is None:
            m = re.match(r"^\s*\.type\s+([\w$.]+),@function", line)
            if m:
                functions.add(m.group(1))
                continue
            m = re.match(r"^([A-Za-z_][\w$.]*):", line)
            if m and m.group(1) in functions and m.group(1) not in code:  # a function's entry label
                cur = m.group(1)
                code[cur] = []
                continue
            if last is not None:
                for key, pat in INFO.items():
                    m = re.match(pat, line)
                    if m:
                        res[last][key] = int(m.group(1))
            if line.startswith("  - ."):  # the next kernel's entry of amdhsa.kernels (its own keys: four spaces, its arguments' deeper)
                meta = {}
            for key, pat in META.items():
                m = re.match(pat, line)
                if m:
                    meta[key] = int(m.group(1))
            m = re.match(r"^    \.name:\s*(\S+)", line)
            if m:
                res[m.group(1)] = meta = dict(res[m.group(1)], **meta)  # (keys are sorted: the spill counts follow the name)
            continue
        if line.startswith(".Lfunc_end"):
            last, cur = cur, None
            continue
        t = re.sub(r";.*$", "", line).strip()
        if not t or t.startswith(".") or re.match(r"^[\w$.]+:$", t):
            continue
        code[cur].append(re.sub(r"\.L[\w$.]+", "L", t))
    code = {k: v for k, v in code.items() if v}
    return code, res


def demangle(symbols):
    if not symbols:
        return {}
    out = subprocess.run(["c++filt"] + symbols, capture_output=True, text=True).stdout.splitlines()
    return {s: re.sub(r"\(.*$", "", re.sub(r"^void ", "", n)) for s, n in zip(symbols, out)}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, ra = read(sys.argv[1])
    b, rb = read(sys.argv[2])
    names = demangle(sorted(set(a) | set(b)))
    same = [k for k in a if k in b and a[k] == b[k]]
    diff = [k for k in a if k in b and a[k] != b[k]]
    only_a = [k for k in a if k not in b]
    only_b = [k for k in b if k not in a]
    print("functions in the parent: %d; in this tree: %d" % (len(a), len(b)))
    print("identical instruction for instruction (labels and comments stripped): %d" % len(same))
    print("present in both, different: %d" % len(diff))
    print("only in the parent: %d" % len(only_a))
    for k in only_a:
        print("  - %s (%d instructions)" % (names[k], len(a[k])))
    print("only in this tree: %d" % len(only_b))
    for k in only_b:
        print("  + %s (%d instructions)" % (names[k], len(b[k])))
    for title, keys in (("identical", same), ("different", diff)):
        print("%s kernels by family:" % title)
        fam = collections.Counter(re.match(r"[\w:]+", names[k]).group(0) for k in keys)
        for f in sorted(fam):
            print("%6d  %s" % (fam[f], f))
    worse = []
    # identical code can still differ in what it is given (a resource is an attribute of the kernel, not an instruction)
    for k in same:
        for c in COLUMNS:
            va, vb = ra[k].get(c), rb[k].get(c)
            if va is not None and vb is not None and (vb < va if c in MORE_IS_BETTER else vb > va):
                worse.append((k, c, va, vb))
    if diff:
        print()
        print("The differing functions (parent -> this tree; a resource that did not change is printed once):")
        print("  %15s  %s  function" % ("instructions", "  ".join("%11s" % c for c in COLUMNS)))
    for k in diff:
        cells = []
        for c in COLUMNS:
            va, vb = ra[k].get(c), rb[k].get(c)
            if va == vb:
                cells.append("%11s" % ("-" if va is None else va))
            else:
                cells.append("%11s" % ("%s->%s" % (va, vb)))
                if va is not None and vb is not None and (vb < va if c in MORE_IS_BETTER else vb > va):
                    worse.append((k, c, va, vb))
        print("  %6d ->%6d  %s  %s" % (len(a[k]), len(b[k]), "  ".join(cells), names[k]))
    print()
    print("resources worse than the parent's: %d" % len(worse))
    for k, c, va, vb in worse:
        print("  ! %s: %s %s -> %s" % (names[k], c, va, vb))
    sys.exit(1 if worse else 0)


if __name__ == "__main__":
    main()
