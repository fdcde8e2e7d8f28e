"""Static instruction counts of the loops of a trial_kernel assembly dump (tools/one_inst.hip -S), per
basic block: the table of a profiles/<round>/*/static_counts.txt.

usage: python tools/static_counts.py <dump.s> [<dump.s> ...]
For every depth-1 loop: its blocks, VALU and instruction totals; for the largest loop with Philox
products (the array pass) one line per block with its VALU, s_nop, global loads, LDS operations,
Philox products, barriers and float64 FMAs, and the vector scratch loads / stores if any.
"""
import collections
import os
import re
import sys


def blocks_of(path):
    blocks, cur = [], None
    for line in open(path).read().split("\n"):
        m = re.match(r"^\.L(BB\d+_\d+):(.*)", line) or re.match(r"^; (%bb\.\d+):(.*)", line)
        if m:
            cur = [m.group(1), m.group(2), collections.Counter()]
            blocks.append(cur)
            continue
        s = line.strip()
        if cur and s and s[0] not in ";.":
            cur[2][s.split()[0]] += 1
    return blocks


def summary(c):
    n = lambda pred: sum(v for k, v in c.items() if pred(k))
    out = (f"instrs {sum(c.values()):4d} VALU {n(lambda k: k.startswith('v_')):4d} s_nop {c['s_nop']:2d} "
           f"gload {n(lambda k: k.startswith('global_load')):2d} ds {n(lambda k: k.startswith('ds_')):3d} "
           f"philox_mad {c['v_mad_u64_u32']:3d} barrier {c['s_barrier']} fma64 {n(lambda k: k.startswith(('v_fma_f64', 'v_fmac_f64'))):d}")
    scr = n(lambda k: k.startswith("scratch_"))
    return out + (f" scratch {scr}" if scr else "")


def main():
    for path in sys.argv[1:]:
        print("==", os.path.basename(path))
        blocks = blocks_of(path)
        loops = collections.OrderedDict()
        for name, comment, c in blocks:
            m = re.search(r"Header=(BB\d+_\d+) Depth=1", comment)
            hdr = m.group(1) if m else (name if "Loop Header: Depth=1" in comment else None)
            if hdr:
                loops.setdefault(hdr, []).append((name, c))
        for hdr, bl in loops.items():
            tot = sum((c for _, c in bl), collections.Counter())
            valu = sum(v for k, v in tot.items() if k.startswith("v_"))
            print(f" loop {hdr} blocks {len(bl)} VALU {valu} instrs {sum(tot.values())}")
        if not loops:
            continue
        main_hdr = max(loops, key=lambda h: (sum(c["v_mad_u64_u32"] for _, c in loops[h]), sum(sum(c.values()) for _, c in loops[h])))
        for name, c in loops[main_hdr]:
            print(f"   {name:9s} {summary(c)}")


if __name__ == "__main__":
    main()
