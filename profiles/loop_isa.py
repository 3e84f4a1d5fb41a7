#!/usr/bin/env python3
"""Print the innermost loops that hold a global load in one kernel of an ISA listing
(hipcc -S / --save-temps, e.g. `make isa1`), with instruction counts by class.
  python profiles/loop_isa.py build/isa1.s march_kernelILi0ELi1ELb0E [--print] [--pads] [--json] [--load OPCODE] [--outer]
--outer: also loops that hold a child loop (the VCS longest-axis walk, whose crawl fast-forward is
one): their own blocks, the child's left out.
--load: the load that marks a walk loop, by opcode prefix (default global_load_dwordx2, the VCS mask
word; the cuckoo walk's filter word is `--load "global_load_dword "`).

Per loop, two spans:
  first : from the loop's first back-edge target to that back edge -- the straight-line path of
          an iteration that takes no side block (in the VCS walks: no lane skips a cluster).  This
          is the span earlier notes quote (`N VALU, M SALU/branch`, waits and pads left out).
  body  : every block the compiler attributes to the loop (its `in Loop: Header=` comments), side
          blocks included -- skip block, IEEE-division fallback, crawl bookkeeping.
Classes: VALU (v_*, lane spill ops included), SALU (s_* but branches, waits, pads), branch
(s_branch, s_cbranch_*, s_setpc), wait (s_waitcnt*), pad (s_nop), load (global/flat/scratch/ds
loads), lane (v_readlane / v_writelane: SGPR spill traffic), scratch (scratch_*).
--pads names, for every s_nop of a loop, the instruction before it (an `asm:` prefix marks one that
an inline-asm statement wrote) and the instruction after it."""
import json
import re
import sys

path, kname = sys.argv[1], sys.argv[2]
show, pads, as_json = "--print" in sys.argv, "--pads" in sys.argv, "--json" in sys.argv
outer = "--outer" in sys.argv
mark = sys.argv[sys.argv.index("--load") + 1] if "--load" in sys.argv else "global_load_dwordx2"
lines = open(path).read().splitlines()
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + kname + r"\w*:", l))
end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
body = lines[start:end]
labels = {l.split(":")[0]: i for i, l in enumerate(body) if re.match(r"^\.LBB\w+:", l)}


def is_ins(x):
    x = x.strip()
    return bool(x) and not x.startswith((";", ".", "//"))


def classes(ins):
    c = dict(valu=0, salu=0, branch=0, wait=0, pad=0, load=0, lane=0, scratch=0)
    for x in ins:
        op = x.split()[0]
        if op.startswith("s_nop"):
            c["pad"] += 1
        elif op.startswith("s_waitcnt"):
            c["wait"] += 1
        elif op.startswith(("s_cbranch", "s_branch", "s_setpc")):
            c["branch"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if op.startswith(("v_readlane", "v_writelane")):
                c["lane"] += 1
        elif op.startswith("scratch_"):
            c["scratch"] += 1
            if "load" in op:
                c["load"] += 1
        elif op.startswith(("global_load", "flat_load", "ds_read", "ds_load", "buffer_load")):
            c["load"] += 1
    return c


# blocks: (first line, header label or None, is an innermost loop's header)
blocks = []
for i, l in enumerate(body):
    m = re.match(r"^(\.LBB\w+):|^; %bb\.\d+:", l)
    if not m:
        continue
    head = re.search(r"in Loop: Header=(BB\w+)", l)
    inner = False
    for j in range(i, min(i + 8, len(body))):      # the comment lines under a header label
        if j > i and not body[j].lstrip().startswith(";"):
            break
        if "This Inner Loop Header" in body[j] or (outer and "This Loop Header" in body[j]):
            inner = True
    blocks.append([i, "." + "L" + head.group(1) if head else None, inner, m.group(1)])
for k, b in enumerate(blocks):
    b.append(blocks[k + 1][0] if k + 1 < len(blocks) else len(body))

out = []
for i0, _, inner, label, i1 in blocks:
    if not inner:
        continue
    member = [(a, b) for a, h, _, lab, b in blocks if lab == label or h == label]
    span = [body[k].strip() for a, b in member for k in range(a, b) if is_ins(body[k])]
    if not any(x.startswith(mark) for x in span):
        continue
    # the first span: from the load on, the closest back edge to a label at or before the load
    ld = next(k for a, b in member for k in range(a, b) if body[k].strip().startswith(mark))
    first = None
    for j in range(ld, len(body)):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\w+)|s_branch\s+(\.LBB\w+)", body[j])
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in labels and labels[tgt] <= ld:
                first = (labels[tgt], j)
                break
    fins = [body[k].strip() for k in range(first[0], first[1] + 1) if is_ins(body[k])] if first else []
    cf, cb = classes(fins), classes(span)
    rec = dict(loop=label, header_line=start + i0 + 1, first=cf, body=cb)
    out.append(rec)
    if as_json:
        continue
    # (the opening line keeps the form earlier notes quote: SALU and branches together)
    print(f"loop {body[first[0]].split(':')[0] if first else label} (header {label}, line {start + i0 + 1}): "
          f"{len(fins)} instructions, {cf['valu']} VALU, {cf['salu'] + cf['branch']} SALU/branch, {cf['load']} loads")
    for name, c in (("first", cf), ("body", cb)):
        print(f"   {name:5s} " + " ".join(f"{k} {v}" for k, v in c.items()))
    if pads:
        in_asm, prev, last = False, None, None
        for a, b in member:
            if a != last:            # (a block that does not follow the one before in the listing)
                prev = None
            last = b
            for k in range(a, b):
                x = body[k].strip()
                if x.startswith(";;#ASMSTART"):
                    in_asm = True
                elif x.startswith(";;#ASMEND"):
                    in_asm = False
                    prev = prev if prev and prev[0] == "asm" else ("asm", "(empty statement)")
                elif is_ins(x):
                    if x.startswith("s_nop"):
                        nxt = next((body[q].strip() for q in range(k + 1, len(body)) if is_ins(body[q])), "")
                        print(f"   pad at line {start + k + 1}: after {prev[0] + ': ' if prev and prev[0] else ''}"
                              f"`{prev[1] if prev else ''}` before `{nxt}`")
                    prev = ("asm" if in_asm else "", x)
    if show:
        print("\n".join("      " + x for x in span))
if as_json:
    print(json.dumps(out))
