#!/usr/bin/env python3
"""tools/isa_blocks.py c3.s [MIN]: static instruction counts per basic block of every wide_filter_kernel in a device
assembly file (tools/regs_c3.sh with REGS_ASM=1 writes one): VALU / v_mov / MFMA / LDS / VMEM / SALU, and the
kernel's totals and resource lines.  Blocks with fewer than MIN (default 24) instructions are summed into one line."""
import re
import subprocess
import sys


def kind(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith(("v_mov_b", "v_accvgpr")):
        return "vmov"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    path = sys.argv[1]
    small = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    cols = ("valu", "vmov", "mfma", "lds", "vmem", "salu")
    name, blocks, cur = None, [], None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w*wide_filter_kernel\w*):", s)
        if m:
            name, blocks, cur = m.group(1), [], ["entry", dict.fromkeys(cols + ("other",), 0)]
            blocks.append(cur)
            continue
        if name is None:
            continue
        if s.startswith(".Lfunc_end"):
            _done.append((name, blocks))
            name = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            cur = [m.group(1), dict.fromkeys(cols + ("other",), 0)]
            blocks.append(cur)
            continue
        if not s or s.startswith((";", ".", "//")):
            continue
        op = s.split()[0]
        if op.endswith(":"):
            continue
        cur[1][kind(op)] += 1


_done = []          # (mangled kernel name, [[block label, counts], ...])


def report(path, small):
    cols = ("valu", "vmov", "mfma", "lds", "vmem", "salu")
    text = open(path).read()
    for name, blocks in _done:
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        print("==", dem[dem.find("wide_filter_kernel"):][:70])
        m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\b(.*?)\.end_amdhsa_kernel", text, re.S)
        if m:
            vg = re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(1))
            sc = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(1))
            ld = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(1))
            print("   next_free_vgpr", vg and vg.group(1), " scratch bytes", sc and sc.group(1), " static LDS", ld and ld.group(1))
        m = re.search(re.escape(name) + r":.*?; Occupancy: (\d+)", text, re.S)
        if m:
            print("   occupancy", m.group(1))
        print("   %-12s" % "block" + "".join("%7s" % c for c in cols))
        tot = dict.fromkeys(cols, 0)
        rest = dict.fromkeys(cols, 0)
        nrest = 0
        for label, c in blocks:
            for k in cols:
                tot[k] += c[k]
            if sum(c[k] for k in cols) < small:
                nrest += 1
                for k in cols:
                    rest[k] += c[k]
                continue
            print("   %-12s" % label + "".join("%7d" % c[k] for k in cols))
        print("   %-12s" % ("<%d: %d blk" % (small, nrest)) + "".join("%7d" % rest[k] for k in cols))
        print("   %-12s" % "total" + "".join("%7d" % tot[k] for k in cols))


if __name__ == "__main__":
    main()
    report(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 24)
