#!/usr/bin/env python3
"""The refill's group pass in instructions a wave issues: the streaming workgroups' second form
(hg_streamer2.hip.h, res_streamer_limb) in a parent's device assembly and in this tree's, every build (T = 1, 2, 4; plain and MISS;
without and with stage clocks).  Both assemblies are built with line tables:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -gline-tables-only -S --cuda-device-only \\
        -o hgibbs.s hydra_amd/csrc/hgibbs.hip
A pass begins at the statement that names the set's group (`const uint32_t G = gb...`) and ends where the next one begins or the
group loop is left; everything a wave issues in between is counted, whatever file it was inlined from -- the set's reads, the
expansion, the products, the x form, the sums and the loads of the set's next group.  Wave 0's block (the slots' (mave, mstd) and their
load) is part of the count where every wave issues it under an exec mask (the per-lane form) and listed apart where it stands behind a
scalar branch (rounds of whole groups: waves 1 - 7 issue the branch alone).  Per build: the passes of each form, then
tools/asm_count.py's static totals of the refill's lines and of the functions inlined into it, registers and scratch.
usage: refill_pass_counts.py PARENT_TREE PARENT.s THIS_TREE THIS.s > profiles/refill_pass_instructions.txt"""
import os
import re
import subprocess
import sys

H = "hg_streamer2.hip.h"
if len(sys.argv) != 5:
    sys.exit(__doc__)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source_lines(tree):
    src = open(os.path.join(tree, "hydra_amd", "csrc", H)).read().split("\n")

    def line_of(text, after=0, need=True):
        for i in range(after, len(src)):
            if text in src[i]:
                return i + 1
        if need:
            sys.exit("statement not found in %s of %s: %r" % (H, tree, text))
        return 0

    d = {"nnew": line_of("if (nnew) {")}
    d["G"] = line_of("const uint32_t G = gb", d["nnew"])
    d["end"] = line_of("(one(std::integral_constant", d["G"])  # (where the passes are called from: the group loop's own lines begin again)
    d["whole"] = line_of("const uint32_t s16 =", d["G"], need=False)  # (this tree: the first statement of the form for rounds of whole groups)
    d["wave0"] = line_of("if (wave == 0) {", d["whole"], need=False) if d["whole"] else 0
    d["load_set"] = line_of("auto load_set = [&]")
    d["load_end"] = line_of("};", line_of("auto load_set_whole", need=False) or d["load_set"])
    d["tab1"] = line_of("if (upd && tid < 4)")
    return d


def instructions(path, kern):
    """(file, line, opcode) of every instruction of the kernels whose symbol holds `kern`"""
    files, out, inside, cur = {}, [], False, (None, 0)
    for l in open(path, errors="replace"):
        m = re.match(r'\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]*)"', l) or re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"', l)
        if m:
            files[int(m.group(1))] = m.group(2).rsplit("/", 1)[-1]
            continue
        m = re.match(r"^([A-Za-z_][\w.$]*):", l)
        if m and not l.startswith(".L"):
            inside = kern in m.group(1)
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
        if re.match(r"^(v_|s_|ds_|global_|buffer_|flat_|scratch_)", op):
            out.append((cur[0], cur[1], op))
    return out


def passes(ins, d):
    """the passes of a kernel: (form, instructions a wave other than wave 0 issues, wave 0's block, MFMAs)"""
    out, cur = [], None
    prev_line = 0
    for f, ln, op in ins:
        own = f == H
        if own and ln in (d["G"], d["G"] + 1) and prev_line not in (d["G"], d["G"] + 1):  # (the group's number and the test `G <= G1` behind it)
            if cur:
                out.append(cur)
            cur = {"n": 0, "w0": 0, "mfma": 0, "whole": False}
        elif cur and own and (d["nnew"] <= ln < d["G"] or ln >= d["end"]):
            out.append(cur)
            cur = None
        if own:
            prev_line = ln
        if not cur:
            continue
        if own and d["whole"] and ln == d["whole"]:
            cur["whole"] = True
        if cur.get("in_w0"):  # (behind wave 0's scalar branch, to the end of the pass)
            cur["w0"] += 1
        else:
            cur["n"] += 1
        if own and d["wave0"] and ln == d["wave0"] and op.startswith("s_cbranch"):
            cur["in_w0"] = True
        cur["mfma"] += op.startswith("v_mfma")
    if cur:
        out.append(cur)
    return out


def registers(path, kern):
    f, got = False, []
    for l in open(path, errors="replace"):
        if re.match(r"^[A-Za-z_][\w.$]*:", l) and not l.startswith(".L"):
            f = kern in l
        if f and re.match(r"; (NumVgprs|TotalNumSgprs|ScratchSize)", l):
            got.append(l.strip().lstrip("; "))
            if "ScratchSize" in l:
                break
    return "  ".join(got)


BUILDS = [("k_sweep_limbILi%dELi%dELi%dE" % (T, dbg, miss), "T = %d, %s%s" % (T, "MISS" if miss else "plain", ", stage clocks" if dbg else "")) for T in (1, 2) for dbg in (0, 1) for miss in (0, 1)]
BUILDS += [("k_sweep_limb4ILi%dELi%dE" % (dbg, miss), "T = 4, %s%s" % ("MISS" if miss else "plain", ", stage clocks" if dbg else "")) for dbg in (0, 1) for miss in (0, 1)]
print("The refill's group pass in instructions a wave issues (DESIGN.md section 4R, section 8); tools/refill_pass_counts.py PARENT_TREE PARENT.s THIS_TREE THIS.s")
print("per pass: what a wave other than wave 0 issues (+ wave 0's block behind its scalar branch, where there is one); the register sets in order")
print("(sixteen passes in a row of eight sets: the compiler peeled the group loop's first turn -- the first eight are the turn every round takes, the")
print(" rest the further turns of a first fill or a long advance; a pass that ends a sequence also counts the stage clock's read where there is one)")
for kern, name in BUILDS:
    print("\n%s  (%s)" % (name, kern))
    for tag, tree, path in (("parent", sys.argv[1], sys.argv[2]), ("this tree", sys.argv[3], sys.argv[4])):
        d = source_lines(tree)
        ps = passes(instructions(path, kern), d)
        for form, label in ((True, "rounds of whole groups"), (False, "by lane")):
            sel = [q for q in ps if q["whole"] == form]
            if sel:
                print("  %-9s %-22s %s   (MFMAs per pass: %s)" % (tag, label, " ".join("%d+%d" % (q["n"], q["w0"]) if q["w0"] else "%d" % q["n"] for q in sel), sorted({q["mfma"] for q in sel})))
        ranges = ["%s:%d-%d=refill" % (H, d["nnew"], d["end"] + 1), "%s:%d-%d=load_set" % (H, d["load_set"], d["load_end"]), "%s:62-170=set_registers" % H, "%s:172-181=rl_expand16" % H,
                  "%s:%d-%d=tab1" % (H, d["tab1"], d["tab1"] + 4)]
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "asm_count.py"), path, kern] + ranges).decode()
        for l in out.splitlines():
            print("  %-9s static %s" % (tag, l))
        print("  %-9s %s" % (tag, registers(path, kern)))
