"""Are the trial kernels of two builds the same code?  Compares two assembly dumps of the trial objects.

A dump is a directory with one file per trial object (the Makefile's object names), written by
that object's own compile line with ``--cuda-device-only -S`` in place of ``-c``, for instance

    make -C m-mimo-ofdm-with-nonlinear-pa-sim_amd/csrc -j8 BUILD=<dir> \\
         HIPCC="/opt/rocm/bin/hipcc --cuda-device-only -S" <dir>/trial_F2048_f64_soft.o ...

    python tools/isa_identity.py <dump of the old tree> <dump of the new tree>

The kernels of an object are paired by their template arguments behind the mode (type, F, T, slots,
aligned, channel, CSI, waves, buffers, symbols in LDS): the mode is the object's.  Left out of the
comparison are the kernels' symbol names (each becomes its template arguments), the size of the
kernel arguments (``.amdhsa_kernarg_size``, ``.kernarg_segment_size`` and the ``.args`` lists of the
metadata), the ``__hip_cuid_*`` symbol, and the register allocator's ``; implicit-def:`` / ``; kill:``
comment lines, which assemble to nothing and whose order among themselves is not stable from one
compile to the next.  Everything else -- every instruction, label and
directive, the resource block of every kernel (VGPRs, SGPRs, scratch, LDS) -- must be equal line
for line.  Prints one line per object and the first differing lines of one that differs; the exit
status is the number of objects that differ.
"""
import os
import re
import sys

# a trial kernel's symbol, old (trial_kernel_<mode><args...>) or new (trial_kernel<mode, args..., the mode's argument types>), and its arguments behind the mode
KERNEL = re.compile(r"\.type\s+_Z(N4mimo\d+trial_kernel(?:_[a-z]+)?I(?:Li\d+E)?"
                    r"([df])Li(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELi(\d)ELb(\d)ELi(\d)ELi(\d)ELb(\d)E(?:J[A-Za-z]*E)?EEv\w+),@function")
SKIP = re.compile(r"\.amdhsa_kernarg_size|\.kernarg_segment_size|__hip_cuid_|^\s*; (implicit-def|kill):")
RESOURCES = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def normalised(path):
    """The dump's lines with the kernels' names replaced and the kernel-argument sizes dropped."""
    text = open(path).read()
    names = {m.group(1): "KERNEL<" + ",".join(m.groups()[1:]) + ">" for m in KERNEL.finditer(text)}
    for sym in sorted(names, key=len, reverse=True):  # (also inside the names of the kernel's LDS arrays)
        text = text.replace(sym, names[sym])
    out, in_args = [], False
    for line in text.split("\n"):
        if in_args:  # the metadata's argument list: its entries are indented deeper than the kernel's own fields
            if re.match(r"\s{6}", line):
                continue
            in_args = False
        if re.match(r"\s+\.args:\s*$", line):
            in_args = True
            continue
        if SKIP.search(line):
            continue
        out.append(line)
    return out


def kernels(lines):
    """-> {template arguments: (instructions, {resource: value})} from the normalised lines."""
    insts, res, cur = {}, {}, None
    for line in lines:
        m = re.match(r"(_Z|_ZZ)?(KERNEL<[^>]*>):\s", line + " ")
        if m and not line.startswith("\t"):
            cur = m.group(2)
            insts[cur] = 0
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and re.match(r"\t[a-z]+_\w+", line):
            insts[cur] += 1
        m = re.match(r"\s+\.name:\s+_Z(KERNEL<[^>]*>)", line)
        if m:
            res[m.group(1)] = block
        m = re.match(r"\s+- \.agpr_count:", line)
        if m:
            block = {}
        m = re.match(r"\s+\.(\w+):\s+(\d+)\s*$", line)
        if m and m.group(1) in RESOURCES:
            block[m.group(1)] = int(m.group(2))
    return {k: (insts.get(k, 0), res.get(k, {})) for k in set(insts) | set(res)}


def main():
    old, new = sys.argv[1], sys.argv[2]
    names = sorted(f for f in os.listdir(old) if f.startswith("trial_F"))
    missing = sorted(set(names) ^ set(f for f in os.listdir(new) if f.startswith("trial_F")))
    if missing:
        sys.exit("objects in one dump only: " + " ".join(missing))
    differ = n_kernels = 0
    for name in names:
        a, b = normalised(os.path.join(old, name)), normalised(os.path.join(new, name))
        ka = kernels(a)
        same = a == b
        differ += not same
        n_kernels += len(ka)
        n_inst = sum(v[0] for v in ka.values())
        vg = [v[1].get("vgpr_count", 0) for v in ka.values()]
        sc = [v[1].get("private_segment_fixed_size", 0) for v in ka.values()]
        lds = [v[1].get("group_segment_fixed_size", 0) for v in ka.values()]
        print("%-28s %2d kernels %8d instructions  vgpr %3d-%3d  scratch %4d-%4d B  lds %6d-%6d B  %s" % (
            name, len(ka), n_inst, min(vg), max(vg), min(sc), max(sc), min(lds), max(lds),
            "identical" if same else "DIFFERENT"))
        if not same:
            shown = 0
            for i, (x, y) in enumerate(zip(a, b)):
                if x != y:
                    print("  line %d\n    old: %s\n    new: %s" % (i + 1, x, y))
                    shown += 1
                    if shown == 5:
                        break
            if len(a) != len(b):
                print("  %d lines against %d" % (len(a), len(b)))
    print("%d objects, %d kernels: %s" % (len(names), n_kernels,
                                          "all identical" if not differ else "%d objects differ" % differ))
    sys.exit(differ)


if __name__ == "__main__":
    main()
