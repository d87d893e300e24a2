"""From a rocprofv3 csv trace of bench.py (--kernel-trace --memory-copy-trace --output-format csv): how long the device waits
between k_res_finish and the next sweep kernel, how much of that is device work, and every kernel and copy of the last such
gap with its start and duration.  usage: trace_gaps.py TRACE_DIR"""
import csv
import glob
import os
import sys

d = sys.argv[1]


def rows(pat):
    fs = glob.glob(os.path.join(d, "**", pat), recursive=True)
    if not fs:
        return []
    with open(fs[0]) as f:
        return list(csv.DictReader(f))


k = rows("*kernel_trace.csv")
m = rows("*memory_copy_trace.csv")
if k:
    print("kernel trace columns:", list(k[0].keys()))
if m:
    print("memory copy columns:", list(m[0].keys()))
ev = []
for r in k:
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "K", r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:60], 0))
for r in m:
    b = r.get("Bytes") or r.get("Size") or "0"
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "C", r.get("Direction", "?"), int(b) if b.isdigit() else 0))
ev.sort()
sweeps = [i for i, e in enumerate(ev) if e[2] == "K" and ("k_sweep_limb" in e[3] or "k_sweep_resident" in e[3])]
fin = [i for i, e in enumerate(ev) if e[2] == "K" and "k_res_finish" in e[3]]
print("sweep kernels: %d, k_res_finish: %d" % (len(sweeps), len(fin)))
for a, b in zip(fin[:-1], sweeps[1:]):
    gap = (ev[b][0] - ev[a][1]) / 1e6
    busy = sum(e[1] - e[0] for e in ev[a + 1:b]) / 1e6
    print("idle between k_res_finish and the next sweep kernel: %.3f ms wall, %.3f ms of it device work (kernels + copies)" % (gap, busy))
if len(fin) >= 2:
    a, b = fin[-2], sweeps[-1]
    t0 = ev[a][1]
    print("last gap, every device activity (start offset ms, duration ms, kind, name, bytes):")
    for e in ev[a + 1:b]:
        print("  %9.3f %8.3f %s %-50s %d" % ((e[0] - t0) / 1e6, (e[1] - e[0]) / 1e6, e[2], e[3], e[4]))
