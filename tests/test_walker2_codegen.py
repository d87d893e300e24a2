"""The second walker's chain function as the compiler emits it (hg_walker2.hip.h, w2_chain): the decider's round loop -- wave 0, the
default instance of c4 (window 256, one rank, no missing calls, no predicted pivots) -- carries its uniform state in scalar registers
and runs without scratch memory; waves 1-3 and the sweeps without predicted pivots run instances without the code they never use.
The counts of the parent's loop were 48 v_writelane_b32 (SGPR spills), 178 s_and_saveexec_b64 and 3 806 instructions."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chain_symbol(dbg, miss, bc, ranks, decide, piv):
    return "_ZN2hg8w2_chainILi%dELi%dELi%dELi%dELi%dELi%dEEEvRKNS_9ResParamsE" % (dbg, miss, bc, ranks, decide, piv)


def function_body(asm, sym):
    start = asm.index("\n%s:" % sym)
    end = asm.index("\n\t.size\t%s," % sym, start)
    return asm[start:end].split("\n")


def round_loop(lines):
    """the outermost loop: the backward branch that spans the most lines"""
    labels = {}
    for i, line in enumerate(lines):
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            labels[m.group(1)] = i
    best = None
    for i, line in enumerate(lines):
        m = re.match(r"^\s+s_(?:branch|cbranch_\w+)\s+(\.LBB\w+)", line)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            if best is None or i - labels[m.group(1)] > best[1] - best[0]:
                best = (labels[m.group(1)], i)
    assert best is not None, "no loop"
    return lines[best[0]:best[1] + 1]


def mnemonics(lines):
    return [l.split()[0] for l in lines if l.startswith("\t") and l.strip() and not l.lstrip().startswith((";", "."))]


def loop_counts(asm, sym):
    loop = mnemonics(round_loop(function_body(asm, sym)))
    n = lambda m: sum(1 for x in loop if x == m)
    return {
        "instructions": len(loop),
        "v_writelane_b32": n("v_writelane_b32"),
        "v_readlane_b32": n("v_readlane_b32"),
        "s_and_saveexec_b64": n("s_and_saveexec_b64"),
        "s_cbranch_execz": n("s_cbranch_execz"),
        "s_cbranch_scc": n("s_cbranch_scc0") + n("s_cbranch_scc1"),
        "scratch": sum(1 for x in loop if x.startswith(("scratch_", "buffer_"))),
    }


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("w2") / "hgibbs.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only",
                           "-o", str(out), os.path.join(ROOT, "hydra_amd", "csrc", "hgibbs.hip")], stderr=subprocess.DEVNULL)
    return out.read_text()


def test_every_role_and_feature_instance_is_emitted(device_asm):
    for dbg in (0, 1):
        for miss in (0, 1):
            for decide in (0, 1):
                shapes = [(256, 0, 0), (0, 0, 0), (0, 1, 0)] + ([(256, 0, 1), (0, 0, 1)] if not miss else [])
                for bc, ranks, piv in shapes:
                    sym = chain_symbol(dbg, miss, bc, ranks, decide, piv)
                    assert "\n%s:" % sym in device_asm, sym


def test_decider_round_loop(device_asm):
    c = loop_counts(device_asm, chain_symbol(0, 0, 256, 0, 1, 0))
    print("decider <DBG=0, MISS=0, BC=256, RANKS=0, PIV=0> round loop:", c)
    assert c["scratch"] == 0
    assert c["v_writelane_b32"] < 48
    assert c["s_and_saveexec_b64"] < 178
    assert c["instructions"] < 3806


def test_chain_waves_carry_no_decider(device_asm):
    d = loop_counts(device_asm, chain_symbol(0, 0, 256, 0, 1, 0))
    c = loop_counts(device_asm, chain_symbol(0, 0, 256, 0, 0, 0))
    print("chain wave <DECIDE=0> round loop:", c)
    assert c["scratch"] == 0 and c["v_writelane_b32"] == 0
    assert c["instructions"] < d["instructions"] // 3


def test_pivots_compiled_out(device_asm):
    """the predicted-pivot path (the fired list, the staged pred list, the batches' pivots) is in the PIV = 1 instance only"""
    for decide in (0, 1):
        p0 = loop_counts(device_asm, chain_symbol(0, 0, 256, 0, decide, 0))
        p1 = loop_counts(device_asm, chain_symbol(0, 0, 256, 0, decide, 1))
        print("DECIDE=%d: PIV=0 %d instructions, PIV=1 %d" % (decide, p0["instructions"], p1["instructions"]))
        assert p0["instructions"] < p1["instructions"]
