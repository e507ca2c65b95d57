#!/usr/bin/env python3
"""Static census of a v2 transient kernel's barrier phases from its gfx950 assembly (profiles/NOTES_r04.md).

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only spicey_amd/csrc/kernels.hip -o kernels.s
  tools/phase_census.py kernels.s [substring of the mangled kernel name, default the headline instantiation]

The kernel text is cut at every s_barrier (layout order, which for the time loop is execution order: the phases of a
step follow each other in the source).  Per segment: scalar loads, how many of them are issued before the segment's
first LDS read / vector memory load, whether the first `s_waitcnt lgkmcnt` that precedes a use of an LDS value is
reached with a scalar load still outstanding (scalar loads return out of order, so that wait is lgkmcnt(0)), and the
v_readlane / v_writelane traffic of the SGPR spill slots."""
import re
import sys

HEADLINE = "spicey_tran_kernel_v2ILi1ELi4ELi6ELi2ELi512ELi4ELb0E"


def kernel_body(text, key):
    m = re.search(r"^(_ZN\S*" + re.escape(key) + r"\S*):.*?\n(.*?)\n\s*s_endpgm", text, re.S | re.M)
    if not m:
        sys.exit(f"no kernel matching {key}")
    return m.group(1), m.group(2).splitlines()


def census(lines):
    segs, cur, start = [], [], 0
    for i, l in enumerate(lines):
        ins = l.strip().split(" ")[0].split("\t")[0]
        if not ins or ins.startswith(";") or ins.startswith(".") or ins.endswith(":"):
            continue
        cur.append((i, l.strip()))
        if ins == "s_barrier":
            segs.append((start, cur))
            cur, start = [], i + 1
    segs.append((start, cur))
    rows = []
    for start, seg in segs:
        r = dict(line=start, n=len(seg), sload=0, sload_head=0, dep=0, readlane=0, writelane=0, ds=0, vmem=0, prio="", wait_covers_smem="-")
        work_seen = False
        smem_out = False      # a scalar load issued and not yet waited for
        waited_smem = 0       # scalar-load waits in front of the first LDS / vector memory instruction
        for _, l in seg:
            ins = re.split(r"[ \t]", l)[0]
            if ins.startswith("s_load") or ins.startswith("s_buffer_load"):
                r["sload"] += 1
                smem_out = True
                if not work_seen:
                    r["sload_head"] += 1
            elif ins == "v_readlane_b32":
                r["readlane"] += 1
            elif ins == "v_writelane_b32":
                r["writelane"] += 1
            elif ins.startswith("ds_read") or ins.startswith("ds_load"):
                r["ds"] += 1
                work_seen = True
            elif ins.startswith("global_load") or ins.startswith("flat_load") or ins.startswith("buffer_load"):
                r["vmem"] += 1
                work_seen = True
            elif ins == "s_setprio":
                r["prio"] += l.split()[-1]
            elif ins == "s_waitcnt" and "lgkmcnt" in l:
                if not work_seen and smem_out:
                    waited_smem += 1  # a dependent round trip before any work was issued
                    smem_out = False
                elif work_seen and r["wait_covers_smem"] == "-":
                    r["wait_covers_smem"] = "yes" if smem_out else "no"
                    smem_out = False
        r["dep"] = waited_smem
        rows.append(r)
    return rows


def main():
    text = open(sys.argv[1]).read()
    key = sys.argv[2] if len(sys.argv) > 2 else HEADLINE
    name, lines = kernel_body(text, key)
    rows = census(lines)
    print(f"# {name}")
    print("| seg | asm line | instr | s_load | s_load before first ds/vmem | dependent s_load waits before first ds/vmem | first LDS wait covers s_load | ds_read | vmem loads | v_readlane | v_writelane | s_setprio |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for i, r in enumerate(rows):
        print(f"| {i} | {r['line']} | {r['n']} | {r['sload']} | {r['sload_head']} | {r['dep']} | {r['wait_covers_smem']} | {r['ds']} | {r['vmem']} | {r['readlane']} | {r['writelane']} | {r['prio']} |")
    tot = {k: sum(r[k] for r in rows) for k in ("n", "sload", "readlane", "writelane")}
    print(f"\ntotal: {tot['n']} instructions, {tot['sload']} scalar loads, {tot['readlane']} v_readlane, {tot['writelane']} v_writelane")


if __name__ == "__main__":
    main()
