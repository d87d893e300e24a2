#!/usr/bin/env python3
"""Static instruction counts of a kernel by source-line range, from device assembly with line tables
(hipcc ... -gline-tables-only -S --cuda-device-only).  Every instruction is attributed to the `.loc` in force -- for inlined code the
line of the inlined function -- so a range names a stage of the streaming workgroups whatever kernel it was inlined into.  The counts
are static: a stage whose loop is unrolled behind wave-uniform branches (rs_gram_terms' chunks) shows the sum over all its copies.
usage: asm_count.py file.s KERNEL_SUBSTRING HEADER:FIRST-LAST[=label] ...
  e.g. asm_count.py hgibbs.s k_sweep_limbILi2ELi0ELi0E hg_resident.hip.h:512-543=gram hg_streamer2.hip.h:453-523=pass
Per range: all instructions, then by class (valu, salu, lds, vmem, mfma, nop, wait).  --lines adds the count of every line of a range."""
import re
import sys

args = [a for a in sys.argv[1:] if a != "--lines"]
per_line = "--lines" in sys.argv
if len(args) < 3:
    sys.exit(__doc__)
path, kern = args[0], args[1]
ranges = []
for a in args[2:]:
    spec, _, label = a.partition("=")
    f, _, lr = spec.partition(":")
    lo, _, hi = lr.partition("-")
    ranges.append((f, int(lo), int(hi or lo), label or spec))


def klass(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op in ("s_nop",):
        return "nop"
    if op.startswith("s_waitcnt") or op.startswith("s_barrier") or op.startswith("s_sleep"):
        return "wait"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    return "vmem"


files = {}
counts = [dict() for _ in ranges]
lines_of = [dict() for _ in ranges]
inside = False
found = 0
cur = (None, 0)
for l in open(path, errors="replace"):
    m = re.match(r'\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]*)"', l) or re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"', l)
    if m:
        files[int(m.group(1))] = m.group(2).rsplit("/", 1)[-1]
        continue
    m = re.match(r"^([A-Za-z_][\w.$]*):", l)
    if m and not l.startswith(".L"):
        inside = kern in m.group(1)
        found += inside
        continue
    if not inside:
        continue
    m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
    if m:
        cur = (files.get(int(m.group(1))), int(m.group(2)))
        continue
    t = l.split(";")[0].strip()
    if not t or t.startswith((".", "#")) or t.endswith(":"):
        continue
    op = t.split()[0]
    if not re.match(r"^(v_|s_|ds_|global_|buffer_|flat_|scratch_)", op):
        continue
    for i, (f, lo, hi, _) in enumerate(ranges):
        if cur[0] == f and lo <= cur[1] <= hi:
            k = klass(op)
            counts[i][k] = counts[i].get(k, 0) + 1
            lines_of[i][cur[1]] = lines_of[i].get(cur[1], 0) + 1
if not found:
    sys.exit("no kernel matches %r" % kern)
for i, (f, lo, hi, label) in enumerate(ranges):
    c = counts[i]
    print("%-28s %s:%d-%d  total %5d  %s" % (label, f, lo, hi, sum(c.values()), "  ".join("%s %d" % (k, c[k]) for k in ("valu", "salu", "lds", "vmem", "mfma", "nop", "wait") if k in c)))
    if per_line:
        for ln in sorted(lines_of[i]):
            print("    line %5d: %d" % (ln, lines_of[i][ln]))
