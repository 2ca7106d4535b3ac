#!/usr/bin/env python3
"""Compare the kernels of two assembly listings (hipcc ... --cuda-device-only -S).

    isa_compare.py OLD.s NEW.s [--rename REGEX=REPL ...] [--only SUBSTRING]

Per kernel: the resource line (vgpr, sgpr, spill, scratch, lds) of both files and the difference of
their opcode histograms (instructions per mnemonic, NEW minus OLD).  Kernels are matched by mangled
name; --rename rewrites OLD's names first (re.sub), for a kernel that was renamed or whose template
parameters changed, e.g. a dropped trailing bool:
    --rename '(trace_kernelILi\\d+E(?:Lb[01]E){3})Lb0E=\\1'
The comparison is generic: every mnemonic counts alike.  Exit status 1 if anything differs or a
kernel has no partner.
"""
import argparse
import collections
import re
import sys

RES = (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("spill", "vgpr_spill_count"),
       ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"))


def kernels(path):
    """name -> (resources, opcode histogram)"""
    text = open(path).read()
    res = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        res[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1)) for _, key in RES)
    hist = {}
    name = None
    for line in text.splitlines():
        m = re.match(r"(\w+):\s*(;.*)?$", line)
        if m and m.group(1) in res:
            name = m.group(1)
            hist[name] = collections.Counter()
            continue
        if name is None:
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end") or s.startswith(".section"):
            name = None
        elif line.startswith("\t") and s and s[0] not in ".;":
            hist[name][s.split()[0]] += 1
    return {k: (res[k], hist.get(k, collections.Counter())) for k in res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--only", default="", help="kernels whose (new) name contains this")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    for rule in args.rename:
        pat, repl = rule.split("=", 1)
        old = {re.sub(pat, repl, k): v for k, v in old.items()}
    fmt = lambda r: " ".join("%s %d" % (label, v) for (label, _), v in zip(RES, r))
    differ = 0
    for name in sorted(set(old) | set(new)):
        if args.only not in name:
            continue
        if name not in old or name not in new:
            print("%s\n    only in %s" % (name, args.new if name in new else args.old))
            differ += 1
            continue
        (r0, h0), (r1, h1) = old[name], new[name]
        delta = {op: h1[op] - h0[op] for op in set(h0) | set(h1) if h1[op] != h0[op]}
        same = r0 == r1 and not delta
        differ += 0 if same else 1
        print("%s\n    %s | %d instructions%s" % (name, fmt(r1), sum(h1.values()), "  (identical)" if same else ""))
        if r0 != r1:
            print("    was: %s" % fmt(r0))
        if delta:
            print("    was: %d instructions; new - old: %s"
                  % (sum(h0.values()), ", ".join("%s %+d" % (op, d) for op, d in sorted(delta.items()))))
    print("%d kernel(s) differ" % differ)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
