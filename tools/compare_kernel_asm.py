#!/usr/bin/env python3
"""Compare the device code of two builds of one .hip file, kernel symbol by kernel symbol.

    hipcc <the Makefile's CXXFLAGS> -S --cuda-device-only FILE.hip -o before.s        (at the commit to compare against)
    hipcc <the Makefile's CXXFLAGS> -S --cuda-device-only FILE.hip -o after.s
    python tools/compare_kernel_asm.py before.s after.s [--filter REGEX] [--short]

Per kernel symbol of either listing: instruction count, VGPRs, AGPRs, SGPRs and scratch bytes of both sides, and whether the two instruction streams are
identical.  A stream is every line of the function's body that is an instruction: comments and directives are dropped, local labels (`.LBB12_3`, which
carry the function's ordinal in the unit) are renumbered in the order in which the stream first names them, so a kernel that merely moved inside the
unit compares equal.  Whole streams are compared; nothing is searched for.  Exit status 1 if a symbol differs or exists on one side only."""
import argparse
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")
RESOURCES = (("vgpr", "num_vgpr", "NumVgprs"), ("agpr", "num_agpr", "NumAgprs"), ("sgpr", "numbered_sgpr", "NumSgprs"), ("scratch", "private_seg_size", "ScratchSize"))


def kernels(path):
    """{symbol: (instruction stream, {resource: value})} of the kernels (`.amdhsa_kernel`) of a listing."""
    funcs, res, is_kernel, cur, last = {}, {}, set(), None, None
    with open(path) as f:
        for raw in f:
            code, _, comment = raw.partition(";")
            line = code.strip()
            m = re.match(r"\.set\s+(\S+)\.(\w+),\s*(\S+)", line)
            if m:
                res.setdefault(m.group(1), {})[m.group(2)] = m.group(3)
                continue
            m = re.match(r"\s*(\w+):\s*(\d+)\s*$", comment)              # the "; Kernel info:" block behind a function (listings without the .set lines)
            if m and last:
                res.setdefault(last, {}).setdefault(m.group(1), m.group(2))
            m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
            if m:
                is_kernel.add(m.group(1))
            m = re.match(r"\.type\s+(\S+),@function", line)
            if m:
                cur, last = m.group(1), m.group(1)
                funcs[cur] = []
                continue
            if cur is None or not line:
                continue
            if re.match(r"\.Lfunc_end\d+:", line):
                cur = None
            elif line.endswith(":"):
                if line[:-1] != cur:
                    funcs[cur].append(line)                                   # a local label: part of the stream, renumbered below
            elif not line.startswith("."):
                funcs[cur].append(" ".join(line.split()))
    out = {}
    for name in funcs:
        if name not in is_kernel:
            continue
        seen = {}
        stream = [LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), ln) for ln in funcs[name]]
        r = res.get(name, {})
        out[name] = (stream, {short: r.get(a, r.get(b, "?")) for short, a, b in RESOURCES})
    return out


def demangle(names):
    if not names or not shutil.which("c++filt"):
        return {n: n for n in names}
    got = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: g.replace("(anonymous namespace)::", "").split("(")[0] for n, g in zip(names, got)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--filter", default=".", help="only symbols whose demangled name matches")
    ap.add_argument("--short", action="store_true", help="only the symbols that differ, and the summary")
    args = ap.parse_args()
    a, b = kernels(args.before), kernels(args.after)
    names = sorted(set(a) | set(b))
    pretty = demangle(names)
    count = {"identical": 0, "differs": 0, "only before": 0, "only after": 0}
    print("%-72s %9s %5s %5s %5s %7s  %s" % ("kernel", "instr", "vgpr", "agpr", "sgpr", "scratch", "streams"))
    for n in names:
        if not re.search(args.filter, pretty[n]):
            continue
        sa, ra = a.get(n, (None, {}))
        sb, rb = b.get(n, (None, {}))
        if sa is None or sb is None:
            status = "only after" if sa is None else "only before"
        else:
            status = "identical" if sa == sb and ra == rb else "differs"
        count[status] += 1
        if args.short and status == "identical":
            continue
        both = lambda x, y: str(x) if x == y else "%s>%s" % (x, y)
        cell = lambda k: both(ra.get(k, "-"), rb.get(k, "-"))
        print("%-72s %9s %5s %5s %5s %7s  %s" % (pretty[n][:72], both("-" if sa is None else len(sa), "-" if sb is None else len(sb)), cell("vgpr"), cell("agpr"),
                                                cell("sgpr"), cell("scratch"), status))
        if status == "differs" and sa != sb:
            at = next((i for i, (x, y) in enumerate(zip(sa, sb)) if x != y), min(len(sa), len(sb)))
            print("    first difference at instruction %d:  %s  |  %s" % (at, sa[at] if at < len(sa) else "<end>", sb[at] if at < len(sb) else "<end>"))
    print("kernel symbols: %d identical, %d differ, %d only before, %d only after" % tuple(count[k] for k in ("identical", "differs", "only before", "only after")))
    return 0 if count["identical"] == sum(count.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
