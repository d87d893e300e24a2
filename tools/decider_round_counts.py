#!/usr/bin/env python3
"""The decider's instructions per round as tools/asm_count.py counts them: the stages of a decider round in the
parent's device assembly and in this tree's, for the decider that c1 - c4 run (one rank, 256-column window, no predicted pivots, K = 4),
without and with missing calls, without and with stage clocks.  Both assemblies are built with line tables:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -gline-tables-only -S --cuda-device-only \\
        -o hgibbs.s hydra_amd/csrc/hgibbs.hip
The parent's stages are the line ranges of hg_walker2.hip.h at the commit before this work (the function there is
w2_chain<DBG, MISS, 256, 0, 1, 0>); this tree's are found from the source by the statements that begin them (w2_chain_k4<DBG, MISS>).
usage: decider_round_counts.py PARENT.s THIS.s > profiles/decider_round_instructions.txt"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = "hg_walker2.hip.h"
if len(sys.argv) != 3:
    sys.exit(__doc__)
parent_s, this_s = sys.argv[1], sys.argv[2]

PARENT = [("preheader", 409, 409), ("record", 410, 650), ("answers", 654, 712), ("search", 713, 731), ("values", 732, 771), ("a5", 772, 812),
          ("draw", 813, 858), ("message", 859, 909), ("behind", 910, 966), ("serial", 654, 909)]

src = open(os.path.join(ROOT, "hydra_amd", "csrc", H)).read().split("\n")


def line_of(text, after=0):
    for i in range(after, len(src)):
        if text in src[i]:
            return i + 1
    sys.exit("statement not found in %s: %r" % (H, text))


body = line_of("void w2_chain_body(")
loop = next(i + 1 for i in range(body, len(src)) if src[i] == "    for (;;) {")  # (the round loop: the function's own, not a lambda's)
lap5 = line_of("lap(5);", loop)
site = line_of("const uint32_t s0 = C & bmask;", lap5) - 1
cand = line_of("const uint32_t qc = pos_of_slot(qs, C);", site)
a5 = line_of("// a5 (src/BayesRRm.cpp", cand)
draw = line_of("double bnew = 0.0;", a5)
msg = line_of("lap(3);", draw)
behind = line_of("// ---- behind the message", msg)
rec = line_of("publish(rtype,", behind)
fn = line_of("uint32_t w2_first_candidate(")
fn_end = line_of("return mm ?", fn)
wo = line_of("unsigned long long w2_without_candidate(")
cm = line_of("auto cm_of = [&]", body)
THIS = [("preheader", loop, loop), ("record", loop + 1, lap5), ("answers", lap5 + 1, site - 1), ("search_site", site, cand - 1), ("search_fn", fn, fn_end + 1),
        ("cm_of", cm, cm + 2), ("values", cand, a5 - 1), ("a5", a5, draw - 1), ("draw", draw, msg - 1), ("without", wo, wo + 3),
        ("message", msg, behind - 1), ("behind", behind, rec + 1)]


def counts(path, kern, stages):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "asm_count.py"), path, kern] +
                                  ["%s:%d-%d=%s" % (H, lo, hi, name) for name, lo, hi in stages]).decode()
    tot = {l.split()[0]: int(re.search(r"total\s+(\d+)", l).group(1)) for l in out.splitlines()}
    return out, tot


def registers(path, symbol):
    f = False
    got = []
    for l in open(path, errors="replace"):
        if l.startswith(symbol + ":"):
            f = True
        if f and re.match(r"; (TotalNumSgprs|ScratchSize)", l):
            got.append(l.strip())
            if "ScratchSize" in l:
                break
    return "  ".join(got)


print("The decider's instructions per round (DESIGN.md section 4R, section 8); tools/decider_round_counts.py PARENT.s THIS.s")
print("Static instructions by source line of %s (tools/asm_count.py).  preheader: the line of the round loop's `for`, loop-invariant" % H)
print("set-up that runs once per sweep.  The search is its call site, w2_first_candidate and the lambda cm_of; the draw includes w2_without_candidate.")
for dbg in (0, 1):
    for miss in (0, 1):
        k = "w2_chainILi%dELi%dELi256ELi0ELi1ELi0E" % (dbg, miss)
        out, tp = counts(parent_s, k, PARENT)
        print("\nparent, w2_chain<%d, %d, 256, 0, 1, 0>%s" % (dbg, miss, "  (stage clocks: what the anatomy times)" if dbg else ""))
        print(out.rstrip())
        print(registers(parent_s, "_ZN2hg8%sEEvRKNS_9ResParamsE" % k))
        k = "w2_chain_k4ILi%dELi%dE" % (dbg, miss)
        out, tt = counts(this_s, k, THIS)
        print("this tree, w2_chain_k4<%d, %d>" % (dbg, miss))
        print(out.rstrip())
        print(registers(this_s, "_ZN2hg11%sEEvRKNS_9ResParamsE" % k))
        serial = tt["answers"] + tt["search_site"] + tt["search_fn"] + tt["cm_of"] + tt["values"] + tt["a5"] + tt["draw"] + tt["without"] + tt["message"]
        print("serial part (answers .. message): parent %d, this tree %d" % (tp["serial"], serial))
