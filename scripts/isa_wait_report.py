#!/usr/bin/env python3
"""s_waitcnt report of the k_lpull instantiations, from gs_relax.hip's assembly.

    make -C dst-libp2p-test-node_amd isa
    scripts/isa_wait_report.py dst-libp2p-test-node_amd/build/gs_relax.s

gfx950 counts vector loads and stores in one in-order counter (vmcnt). The
compiler cannot count the stores of a loop with a variable trip count, so a
wait for a load issued before such stores becomes vmcnt(0): a drain of every
store acknowledgement. This report shows where the
waits are. For every k_lpull<...> in the `-S` output and every loop (the
assembler's block comments: header label and depth; "-" is the code outside
every loop) it prints the loop's instruction count, its vector memory loads,
its vector memory stores and atomics, and its s_waitcnt instructions that
have a vmcnt field, grouped by the field's value. A block is counted in the
innermost loop it stands in.

k_lpull's loops: depth 1 = the 64-row scan, 2 = the row loop, 3 = the entry /
append / emit loops of a row, 4 = the loops inside those.

--kernel SUBSTR keeps the instantiations whose name holds SUBSTR (e.g.
"<1, 16, false, false, false, false, true>"); --lines adds the line (counted
from the kernel's label) of every wait; --json prints one JSON document.
"""
import argparse
import json
import re
import sys

from isa_spill_report import RE_BLOCK, RE_INSN, parse

RE_HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")  # (an innermost loop's header says "Inner")
RE_INLOOP = re.compile(r"in Loop: Header=(\w+) Depth=(\d+)")
RE_LABEL = re.compile(r"^\.L(BB\d+_\d+):")
RE_VMCNT = re.compile(r"vmcnt\((\d+)\)")
RE_VSTORE = re.compile(r"^(?:global|flat|buffer)_(?:store|atomic)")
RE_VLOAD = re.compile(r"^(?:global|flat|buffer)_load")


def analyse(k, lines=False):
    body = k["body"]
    loops = {}  # header label -> row
    order = []

    def row(label, depth):
        if label not in loops:
            loops[label] = {"header": label, "depth": depth, "insns": 0, "vmem_loads": 0, "vmem_stores": 0, "waits": {}}
            if lines:
                loops[label]["wait_lines"] = []
            order.append(label)
        return loops[label]

    cur = row("-", 0)
    i, n = 0, len(body)
    while i < n:
        ln = body[i]
        if RE_BLOCK.match(ln):
            # the block's loop comment: on the label's line or the comment lines below it
            label, depth = "-", 0
            own = RE_LABEL.match(ln)
            j = i
            while j < n and (j == i or body[j].lstrip().startswith(";")):
                if j > i and RE_BLOCK.match(body[j]):
                    break
                m = RE_HEADER.search(body[j])
                if m and own:
                    label, depth = own.group(1), int(m.group(1))
                    break
                m = RE_INLOOP.search(body[j])
                if m:
                    label, depth = m.group(1), int(m.group(2))
                    break
                j += 1
            cur = row(label, depth)
            i += 1
            continue
        m = RE_INSN.match(ln)
        if m:
            op, args = m.group(1), m.group(2).split(";")[0]
            cur["insns"] += 1
            if RE_VSTORE.match(op):
                cur["vmem_stores"] += 1
            elif RE_VLOAD.match(op):
                cur["vmem_loads"] += 1
            elif op == "s_waitcnt":
                v = RE_VMCNT.search(args)
                if v:
                    cur["waits"][v.group(1)] = cur["waits"].get(v.group(1), 0) + 1
                    if lines:
                        cur["wait_lines"].append([i + 1, int(v.group(1))])
        i += 1
    rows = [loops[h] for h in order if loops[h]["insns"]]
    return {"kernel": k["name"], "loops": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm", help="-S output of gs_relax.hip (make isa)")
    ap.add_argument("--kernel", default="", help="only instantiations whose name contains this")
    ap.add_argument("--lines", action="store_true", help="list every wait's line within its kernel")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    with open(a.asm) as f:
        reps = [analyse(k, a.lines) for k in parse(f.read().splitlines())]
    reps = [r for r in reps if a.kernel in r["kernel"]]
    reps.sort(key=lambda r: r["kernel"])
    if not reps:
        sys.exit("no k_lpull instantiation found in %s" % a.asm)
    if a.json:
        print(json.dumps(reps, indent=1))
        return
    for r in reps:
        print(r["kernel"])
        print("  %-12s %5s %6s %6s %7s  %s" % ("loop", "depth", "insns", "loads", "stores", "s_waitcnt vmcnt(n): count"))
        drains = 0
        for lp in r["loops"]:
            w = "  ".join("(%s): %d" % (v, c) for v, c in sorted(lp["waits"].items(), key=lambda t: int(t[0])))
            print("  %-12s %5d %6d %6d %7d  %s" % (lp["header"], lp["depth"], lp["insns"], lp["vmem_loads"],
                                                 lp["vmem_stores"], w or "none"))
            if a.lines and lp["wait_lines"]:
                print("  %-12s lines: %s" % ("", " ".join("%d:(%d)" % (l, v) for l, v in lp["wait_lines"])))
            drains += lp["waits"].get("0", 0)
        print("  vmcnt(0) in all: %d" % drains)
        print()


if __name__ == "__main__":
    main()
