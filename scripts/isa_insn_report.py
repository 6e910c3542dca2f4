#!/usr/bin/env python3
"""Instruction-class report of the k_lpull instantiations, from gs_relax.hip's assembly.

    make -C dst-libp2p-test-node_amd isa
    scripts/isa_insn_report.py dst-libp2p-test-node_amd/build/gs_relax.s

k_lpull issues about as many scalar as vector instructions, and its vector
pipes are busy most of the time: what a row costs is
largely the number of instructions of its straight-line code. For every
k_lpull<...> in the `-S` output and every loop (the assembler's block
comments: header label and depth; "-" is the code outside every loop) this
report prints the loop's instructions by class:

  VALU    v_* but the lane reads / writes
  lane    v_readlane / v_writelane / v_readfirstlane
  SALU    s_* but branches, waits, s_nop and scalar memory
  branch  s_branch / s_cbranch_* / s_setpc / s_endpgm
  SMEM    s_load_* / s_buffer_load_*
  LDS     ds_*
  VMEM    global_* / flat_* / buffer_* / scratch_*
  wait    s_waitcnt / s_nop / s_sleep / s_barrier

A block is counted in the innermost loop it stands in; the counts are static
(one per instruction of the text, not per execution).

k_lpull's loops: depth 1 = the 64-row scan, 2 = the row loop (the per-row
straight-line code: header, classification, steps 5 / 6), 3 = the entry /
stream / append / emit loops of a row, 4 = the loops inside those.

--kernel SUBSTR keeps the instantiations whose name holds SUBSTR (e.g.
"<1, 16, false, false, false, false, true>"); --json prints one JSON document.
"""
import argparse
import json
import re
import sys

from isa_spill_report import RE_BLOCK, RE_INSN, parse

RE_HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")  # (an innermost loop's header says "Inner")
RE_INLOOP = re.compile(r"in Loop: Header=(\w+) Depth=(\d+)")
RE_LABEL = re.compile(r"^\.L(BB\d+_\d+):")

CLASSES = ("valu", "lane", "salu", "branch", "smem", "lds", "vmem", "wait")
LANE_OPS = ("v_readlane", "v_writelane", "v_readfirstlane")
BRANCH_OPS = ("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_endpgm", "s_call")
WAIT_OPS = ("s_waitcnt", "s_nop", "s_sleep", "s_barrier")
VMEM_OPS = ("global_", "flat_", "buffer_", "scratch_")


def classify(op):
    if op.startswith(LANE_OPS):
        return "lane"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(VMEM_OPS):
        return "vmem"
    if op.startswith(BRANCH_OPS):
        return "branch"
    if op.startswith(WAIT_OPS):
        return "wait"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    return None  # a directive


def analyse(k):
    body = k["body"]
    loops = {}  # header label -> row
    order = []

    def row(label, depth):
        if label not in loops:
            loops[label] = dict({"header": label, "depth": depth, "insns": 0}, **{c: 0 for c in CLASSES})
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
            c = classify(m.group(1))
            if c:
                cur["insns"] += 1
                cur[c] += 1
        i += 1
    rows = [loops[h] for h in order if loops[h]["insns"]]
    total = dict({"header": "all", "depth": 0, "insns": sum(r["insns"] for r in rows)},
                 **{c: sum(r[c] for r in rows) for c in CLASSES})
    return {"kernel": k["name"], "loops": rows, "all": total}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm", help="-S output of gs_relax.hip (make isa)")
    ap.add_argument("--kernel", default="", help="only instantiations whose name contains this")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    with open(a.asm) as f:
        reps = [analyse(k) for k in parse(f.read().splitlines())]
    reps = [r for r in reps if a.kernel in r["kernel"]]
    reps.sort(key=lambda r: r["kernel"])
    if not reps:
        sys.exit("no k_lpull instantiation found in %s" % a.asm)
    if a.json:
        print(json.dumps(reps, indent=1))
        return
    fmt = "  %-12s %5s %6s" + " %6s" * len(CLASSES)
    for r in reps:
        print(r["kernel"])
        print(fmt % (("loop", "depth", "insns") + tuple(c.upper() if c != "lane" else "lane" for c in CLASSES)))
        for lp in r["loops"] + [r["all"]]:
            depth = "" if lp["header"] == "all" else lp["depth"]
            print(fmt % ((lp["header"], depth, lp["insns"]) + tuple(lp[c] for c in CLASSES)))
        print()


if __name__ == "__main__":
    main()
