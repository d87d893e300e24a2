#!/usr/bin/env python3
"""The chain's Gram words ("The chain's Gram words") as tools/asm_count.py counts them: the record stage of a chain
wave -- from the round loop's head to lap(5): taking the record, the event's Gram words, the window move, the bound test -- and inside it
the poll of the event's Gram accumulator words, in the parent's device assembly and in this tree's, for six instances of w2_chain_body:
the decider c1 - c4 run (w2_chain_k4<0, MISS>), waves 1 - 3 beside it, the decider of a run-time window and the decider of several ranks.
Both assemblies are built with line tables, each in its own tree:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -gline-tables-only -S --cuda-device-only \\
        -o hgibbs.s hydra_amd/csrc/hgibbs.hip
The stages are found in each tree's hg_walker2.hip.h by the statements that begin them, not by line numbers: the poll block runs from
the statement that forms the parity's address to the line before the several-ranks exchange, plus whatever helpers it calls outside
those lines (this tree: w2_gram_rows32 / 64 and the lambda gram_wait_fail; the parent had none).
The parent's source is read from PARENT_TREE, the tree PARENT.s was built in.
usage: gram_words_counts.py PARENT.s THIS.s PARENT_TREE > profiles/gram_words_instructions.txt"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = "hg_walker2.hip.h"
if len(sys.argv) != 4:
    sys.exit(__doc__)
parent_s, this_s = sys.argv[1:3]
REL = "hydra_amd/csrc/" + H
parent_src = open(os.path.join(sys.argv[3], REL)).read()

INSTANCES = [("decider w2_chain_k4<0,0> (c1 - c4)", "w2_chain_k4ILi0ELi0E", 0),
             ("decider w2_chain_k4<0,1> (MISS)", "w2_chain_k4ILi0ELi1E", 1),
             ("waves 1-3 w2_chain<0,0,256,0,0,0>", "w2_chainILi0ELi0ELi256ELi0ELi0ELi0E", 0),
             ("waves 1-3 w2_chain<0,1,256,0,0,0> (MISS)", "w2_chainILi0ELi1ELi256ELi0ELi0ELi0E", 1),
             ("run-time-window decider <0,0,0,0,1,0>", "w2_chainILi0ELi0ELi0ELi0ELi1ELi0E", 0),
             ("several ranks decider <0,0,0,1,1,0>", "w2_chainILi0ELi0ELi0ELi1ELi1ELi0E", 0)]


def stages(text, tree):
    """[(name, first, last)] per build (plain, MISS): the record stage, the poll block, the poll's helpers outside it"""
    src = text.split("\n")

    def line_of(text, after=0, need=True):
        for i in range(after, len(src)):
            if text in src[i]:
                return i + 1
        if need:
            sys.exit("statement not found in %s of %s: %r" % (H, tree, text))
        return 0

    body = line_of("void w2_chain_body(")
    loop = next(i + 1 for i in range(body, len(src)) if src[i] == "    for (;;) {")
    lap5 = line_of("lap(5);", loop)
    out = []
    at = loop
    for miss in (1, 0):  # (the source has the build MISS first)
        first = line_of(" wp = gacc", at)
        last = line_of("if (RANKS && hit && !bad) {", first) - 1
        at = last
        helpers = []
        fn = line_of("w2_gram_rows%d(unsigned long long base" % (64 if miss else 32), 0, need=False)
        if fn:
            helpers.append(("rows", fn, line_of("return ", fn)))
        lam = line_of("auto gram_wait_fail = [&]", body, need=False)
        if lam:
            helpers.append(("retry", lam, line_of("};", lam)))
        out.append([("record", loop + 1, lap5), ("poll", first, last)] + helpers)
    return {1: out[0], 0: out[1]}


def counts(path, kern, st):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "asm_count.py"), path, kern] +
                                  ["%s:%d-%d=%s" % (H, lo, hi, name) for name, lo, hi in st]).decode()
    tot = {l.split()[0]: int(re.search(r"total\s+(\d+)", l).group(1)) for l in out.splitlines()}
    helpers = sum(v for k, v in tot.items() if k not in ("record", "poll"))
    return tot["record"] + helpers, tot["poll"] + helpers, out


def registers(path, kern):
    f = False
    got = []
    for l in open(path, errors="replace"):
        if not f and re.match(r"^_ZN2hg\d+%s\w*:" % re.escape(kern), l):
            f = True
        if f and re.match(r"; (TotalNumSgprs|NumVgprs|ScratchSize)", l):
            got.append(l.strip("; \n"))
            if "ScratchSize" in l:
                break
    return "  ".join(got)


def spill_reads(path, kern, st):
    """v_readlane_b32 instructions of the poll block: what the loop reads back from lanes of a spill register"""
    lo, hi = next((a, b) for n, a, b in st if n == "poll")
    inside, cur, n, files = False, (None, 0), 0, {}
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
        elif cur[0] == H and lo <= cur[1] <= hi and l.split(";")[0].strip().startswith("v_readlane_b32"):
            n += 1
    return n


ps, ts = stages(parent_src, "the parent"), stages(open(os.path.join(ROOT, REL)).read(), "this tree")
print("The chain's Gram words (DESIGN.md section 4R, section 8); tools/gram_words_counts.py PARENT.s THIS.s PARENT_TREE")
print("Static instructions by source line of %s (tools/asm_count.py).  record: the stage between lap(4) and lap(5), from the round" % H)
print("loop's head to lap(5); poll: the event's Gram accumulator words, from the parity's address to the several-ranks exchange, with the")
print("helpers it calls (this tree: w2_gram_rows32 / 64, gram_wait_fail).  readlane: v_readlane_b32 inside the poll block (spilled masks).")
print()
print("%-44s %15s %15s %17s" % ("instance", "record  p -> t", "poll  p -> t", "readlane  p -> t"))
detail = []
for name, kern, miss in INSTANCES:
    pr, pp, po = counts(parent_s, kern, ps[miss])
    tr, tp, to = counts(this_s, kern, ts[miss])
    print("%-44s %6d -> %5d %6d -> %5d %8d -> %5d" % (name, pr, tr, pp, tp, spill_reads(parent_s, kern, ps[miss]), spill_reads(this_s, kern, ts[miss])))
    detail.append((name, kern, po, to))
print()
for name, kern, po, to in detail:
    print(name)
    print("  parent     %s" % registers(parent_s, kern))
    print("  this tree  %s" % registers(this_s, kern))
    for tag, o in (("parent", po), ("this tree", to)):
        for l in o.rstrip().splitlines():
            print("  %-10s %s" % (tag, l))
