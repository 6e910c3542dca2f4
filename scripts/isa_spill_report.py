#!/usr/bin/env python3
"""SGPR-spill report of the k_lpull instantiations, from gs_relax.hip's assembly.

    make -C dst-libp2p-test-node_amd isa
    scripts/isa_spill_report.py dst-libp2p-test-node_amd/build/gs_relax.s

For each k_lpull<...> in the `-S` output it prints the resource comments
(NumVgprs, TotalNumSgprs, ScratchSize, Occupancy), the VGPRs the register
allocator spills SGPRs into (its "SGPR spill to VGPR lane" comments) and, per
loop depth (the assembler's `Depth=` block comments; blocks outside every loop
are depth 0): the lane writes into the spill VGPRs, the lane reads out of them
(the reloads) and all VALU instructions (mnemonics starting with v_).

k_lpull's loops: 1 = the 64-row scan and row set-up, 2 = the row loop's body,
3 = the neighbour-group / entry / append / emit loops, 4 = the record loop.

It reads only lane read / write instructions and the resource comments; the
depth of a block is approximate where the block placement moved code (a block
is counted where it stands, not where it came from).

--kernel SUBSTR keeps the instantiations whose name holds SUBSTR (e.g.
"<1, 16, false, false, false, false>"); --json prints one JSON document.
"""
import argparse
import json
import re
import sys

RE_BEGIN = re.compile(r"^(_Z\w*k_lpullI\w+):")
RE_BLOCK = re.compile(r"^(?:\.LBB\d+_\d+:|; %bb\.\d+:)")
RE_DEPTH = re.compile(r"(?:Loop Header: |in Loop: Header=\w+ )Depth=(\d+)")  # not the "Parent Loop" lines
RE_SPILLV = re.compile(r"implicit-def: \$vgpr(\d+) : SGPR spill to VGPR lane")
RE_INSN = re.compile(r"^\s+([a-z_][a-z0-9_]*)\s*(.*)$")
RE_RES = re.compile(r"^; (NumVgprs|TotalNumSgprs|ScratchSize|Occupancy): (\d+)")
RE_TARG = re.compile(r"L([ijb])(\d+)E")


def pretty(mangled):
    """k_lpullILi1ELj16ELb0E...E -> k_lpull<1, 16, false, ...>"""
    m = re.search(r"k_lpullI((?:L[ijb]\d+E)+)E", mangled)
    if not m:
        return mangled
    out = []
    for t, v in RE_TARG.findall(m.group(1)):
        out.append(("true" if int(v) else "false") if t == "b" else v)
    return "k_lpull<" + ", ".join(out) + ">"


def parse(lines):
    kernels = []
    cur = None
    i, n = 0, len(lines)
    while i < n:
        ln = lines[i]
        if cur is None:
            m = RE_BEGIN.match(ln)
            if m:
                cur = {"name": pretty(m.group(1)), "mangled": m.group(1), "body": [], "res": {}}
            i += 1
            continue
        if ln.startswith(".Lfunc_end"):
            cur["end"] = True
        elif cur.get("end"):
            m = RE_RES.match(ln)
            if m:
                cur["res"][m.group(1)] = int(m.group(2))
                if len(cur["res"]) == 4:
                    kernels.append(cur)
                    cur = None
        else:
            cur["body"].append(ln)
        i += 1
    return kernels


def analyse(k):
    body = k["body"]
    spillv = sorted({int(m.group(1)) for ln in body for m in [RE_SPILLV.search(ln)] if m})
    names = {"v%d" % v for v in spillv}
    depth = 0
    rows = {}
    lanes_all = 0
    i, n = 0, len(body)
    while i < n:
        ln = body[i]
        if RE_BLOCK.match(ln):
            # the block's loop comment: on the label's line or the comment lines below it
            depth = 0
            j = i
            while j < n and (j == i or body[j].lstrip().startswith(";")):
                if j > i and RE_BLOCK.match(body[j]):
                    break
                m = RE_DEPTH.search(body[j])
                if m:
                    depth = int(m.group(1))
                j += 1
            i += 1
            continue
        m = RE_INSN.match(ln)
        if m and m.group(1).startswith("v_"):
            op, args = m.group(1), m.group(2).split(";")[0]
            r = rows.setdefault(depth, {"valu": 0, "reloads": 0, "spill_writes": 0})
            r["valu"] += 1
            ops = [a.strip() for a in args.split(",")]
            if op.startswith("v_readlane") or op.startswith("v_writelane"):
                lanes_all += 1
            if op.startswith("v_writelane") and ops and ops[0] in names:
                r["spill_writes"] += 1
            elif op.startswith("v_readlane") and len(ops) > 1 and ops[1] in names:
                r["reloads"] += 1
        i += 1
    return {
        "kernel": k["name"],
        "NumVgprs": k["res"].get("NumVgprs"),
        "TotalNumSgprs": k["res"].get("TotalNumSgprs"),
        "ScratchSize": k["res"].get("ScratchSize"),
        "Occupancy": k["res"].get("Occupancy"),
        "spill_vgprs": ["v%d" % v for v in spillv],
        "lane_ops": lanes_all,
        "depth": {str(d): rows[d] for d in sorted(rows)},
    }


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
    for r in reps:
        print(r["kernel"])
        print("  NumVgprs %d  TotalNumSgprs %d  ScratchSize %d  Occupancy %d" %
              (r["NumVgprs"], r["TotalNumSgprs"], r["ScratchSize"], r["Occupancy"]))
        print("  spill VGPRs: %s   lane reads + writes of any kind: %d" %
              (" ".join(r["spill_vgprs"]) or "none", r["lane_ops"]))
        print("  %-6s %8s %14s %13s" % ("depth", "VALU", "spill reloads", "spill writes"))
        tot = {"valu": 0, "reloads": 0, "spill_writes": 0}
        for d, row in r["depth"].items():
            print("  %-6s %8d %14d %13d" % (d, row["valu"], row["reloads"], row["spill_writes"]))
            for k in tot:
                tot[k] += row[k]
        print("  %-6s %8d %14d %13d" % ("all", tot["valu"], tot["reloads"], tot["spill_writes"]))
        print()


if __name__ == "__main__":
    main()
