#!/usr/bin/env python3
"""Are the kernels of two builds the same code?

Compares the device assembly of two builds (`make isa` in csrc/: the --save-temps files
build/*-hip-amdgcn-amd-amdhsa-gfx950.s) kernel by kernel.  A kernel is every symbol an
`.amdhsa_kernel` directive names; its text is what stands between its label and the next
`.Lfunc_end`, comments dropped and the block labels `.LBB<n>_` rewritten to `.LBB_` (n is the
function's position in its unit, which moving it changes), as are the labels `.Lpost_getpc<n>`
of long branches (n counts them through the unit).  With
--resources also the -Rpass-analysis=kernel-resource-usage figures (build/resource_*.txt).

  python3 profiles/isa_compare.py --a A.s [A2.s ...] --b B.s [B2.s ...]
      [--resources-a R.txt [...] --resources-b R.txt [...]] [--only SUBSTRING ...]

A side may be several files (a build whose kernels are spread over several units); a kernel
name may appear only once per side.  Prints one line per kernel and a summary; exit status 1
if a kernel both sides have differs (code or figures).  --only restricts the comparison to
kernels whose (mangled) name contains one of the substrings.
"""
import argparse
import re
import sys

KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
BLOCK = re.compile(r"\.(LBB|Lpost_getpc)\d+_?")
# (the remark's two spellings: from a --save-temps compile, and from a plain one)
REMARK = re.compile(r"^(?:remark: \S+?:\d+:\d+:|\S+?:\d+:\d+: remark:)\s+(.*?)\s*"
                    r"\[-Rpass-analysis=kernel-resource-usage\]\s*$")


def kernels(paths):
    out = {}
    for path in paths:
        lines = open(path).read().split("\n")
        names = [m.group(1) for m in map(KERNEL.match, lines) if m]
        starts = {m.group(1): i for i, m in enumerate(map(LABEL.match, lines)) if m}
        for name in names:
            if name in out:
                sys.exit(f"{name}: in more than one file of a side")
            text = []
            for ln in lines[starts[name] + 1:]:
                if ln.startswith(".Lfunc_end"):
                    break
                ln = BLOCK.sub(r".\1_", ln.split(";", 1)[0]).strip()
                if ln:
                    text.append(ln)
            else:
                sys.exit(f"{name}: no .Lfunc_end in {path}")
            out[name] = text
    return out


def resources(paths):
    out, name = {}, None
    for path in paths:
        for ln in open(path):
            m = REMARK.match(ln)
            if not m:
                continue
            key, _, value = m.group(1).partition(": ")
            if key == "Function Name":
                name = value
                out[name] = {}
            elif name is not None:
                out[name][key] = value
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    ap.add_argument("--resources-a", nargs="+", default=[])
    ap.add_argument("--resources-b", nargs="+", default=[])
    ap.add_argument("--only", nargs="+", default=[])
    args = ap.parse_args()
    a, b = kernels(args.a), kernels(args.b)
    ra, rb = resources(args.resources_a), resources(args.resources_b)
    keep = lambda n: not args.only or any(s in n for s in args.only)
    both = sorted(n for n in a if n in b and keep(n))
    differ = 0
    for n in both:
        same = a[n] == b[n]
        note = f"{len(a[n])} lines"
        if not same:
            at = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
            note = f"{len(a[n])} / {len(b[n])} lines, first difference at line {at + 1}"
        if ra or rb:
            fa, fb = ra.get(n), rb.get(n)
            if fa is None or fb is None or fa != fb:
                same = False
                note += f"; figures {fa} / {fb}"
            else:
                note += "; " + ", ".join(f"{k} {v}" for k, v in fa.items())
        differ += not same
        print(f"{'identical' if same else 'DIFFERS  '}  {n}  ({note})")
    for side, mine, other in (("a", a, b), ("b", b, a)):
        for n in sorted(n for n in mine if n not in other and keep(n)):
            print(f"only in {side}  {n}")
    only_a = sum(1 for n in a if n not in b and keep(n))
    only_b = sum(1 for n in b if n not in a and keep(n))
    print(f"a: {len([n for n in a if keep(n)])} kernels, b: {len([n for n in b if keep(n)])}; in both: {len(both)}, "
          f"identical: {len(both) - differ}, differing: {differ}; only in a: {only_a}, only in b: {only_b}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
