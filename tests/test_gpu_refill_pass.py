"""The refill's group pass of the streaming workgroups' second form (hydra_amd/csrc/hg_streamer2.hip.h, DESIGN.md section 4R "The
refill's group pass") against the CPU oracle: a round of whole groups of an aligned window takes the pass without a test per lane;
the sweep's last groups (the one that holds M among them), a window that ends anywhere and the first walker take it by lane as
before.  Every case runs two or three iterations on the
resident engine with refill = 2 through test_gpu_resident.run_vs_oracle -- its bar is the yardstick: marker order, components, cass,
generator state and the number of updates exact, beta, acum, the hyper-parameters and the residual within 1e-9.

The shapes are the smallest at which the two forms of the pass, the choice between them and the loads of a set's next groups can go
wrong: M below, on and above a group boundary and a multiple of the register sets' 128 positions; both window forms; shards with tail
dwords and workgroups with tiles past the shard's end at one, two and four tiles per workgroup; a dense model in a small window.
"""
import numpy as np
import pytest

from hydra_amd import capi
from test_gpu_parity import close
from test_gpu_resident import make_case, run_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("window", [0, 32])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 127, 128, 129, 255, 257, 400])
def test_the_group_that_holds_M_and_set_rotation(oracle, M, window):
    """N = 4099: one tile per workgroup, eight workgroups (three of them past the shard's end).  A partial last group (M = 1, 15, 17, 127, 129, 255, 257, 400 = 25 groups), M on a
    group boundary (16, 128), the ids and (mave, mstd) asked for behind M (every M: the first fill asks for eight groups and their
    successors), a first fill with more groups than register sets (M > 128 at the default window of 256), and with window = 32 every
    set reloaded many times a sweep."""
    opts = {"refill": 2}
    if window:
        opts["window"] = window
    run_vs_oracle(oracle, M, 4099, iters=2, opts=opts, expect_T=1, expect_refill=2)


@pytest.mark.parametrize("window", [32, 256])
@pytest.mark.parametrize("wend", [0, 1])
def test_both_window_forms(oracle, wend, window):
    """window_end16 = 1: the window ends on a multiple of sixteen and whole groups take the pass without lane masks; 0: it ends anywhere
    and every group is tested by lane.  M = 300: eighteen whole groups and one of twelve positions."""
    run_vs_oracle(oracle, 300, 4099, iters=2, opts={"refill": 2, "window_end16": wend, "window": window}, expect_walker=2, expect_refill=2)


@pytest.mark.parametrize("N,cus,T,miss", [(4099, 0, 1, 0.0), (4099, 5, 2, 0.0), (4099, 5, 2, 0.02), (4099, 3, 4, 0.0)])
@pytest.mark.parametrize("window", [32, 0])
def test_rounds_of_whole_groups(oracle, window, N, cus, T, miss):
    """The form of the pass is chosen once per round: a round whose groups, their sets' next groups and the ids behind those all lie below
    M takes the form without lane tests, the sweep's last 256 positions (128 at four tiles) the per-lane form.  M = 1000: most of the
    sweep runs in whole rounds, its end by lane, at every number of tiles per workgroup; the first fill of the default window is a
    whole round of sixteen groups (two turns of the register sets)."""
    opts = {"refill": 2}
    if window:
        opts["window"] = window
    if cus:
        opts["res_cus"] = cus
    run_vs_oracle(oracle, 1000, N, iters=2, opts=opts, expect_T=T, expect_refill=2, expect_walker=2, missing_rate=miss)


@pytest.mark.parametrize("window", [32, 256])
def test_first_walker_takes_the_pass_by_lane(oracle, window):
    # the first walker's window is C + B whatever window_end16 says: the per-lane form by default
    run_vs_oracle(oracle, 300, 4099, iters=2, opts={"refill": 2, "walker": 1, "window": window}, expect_walker=1, expect_refill=2)


# (N, res_cus, T): a shard is padded to whole blocks of four wave tiles -- N = 37 and N = 1024 are four tiles (one with individuals, three
# past the shard's end), N = 4099 eight (the fifth holds three individuals), N = 9001 twelve (nine in use); res_cus - 1 streaming
# workgroups share them, two or four to a workgroup
TAILS = [(37, 3, 2), (37, 2, 4), (1024, 3, 2), (1024, 2, 4), (4099, 5, 2), (4099, 3, 4), (9001, 7, 2), (9001, 4, 4)]


@pytest.mark.parametrize("miss", [0.0, 0.02])
@pytest.mark.parametrize("N,cus,T", TAILS)
def test_tail_dwords_and_invalid_lanes(oracle, N, cus, T, miss):
    """The lanes' `keep` masks: a last dword with fewer than sixteen individuals (N = 37, 4099, 9001), whole dwords and whole lanes past
    the shard's end, tiles of a workgroup past it (T = 2, T = 4); plain and with missing calls (the second product and its accumulator)."""
    run_vs_oracle(oracle, 200, N, iters=2, opts={"refill": 2, "res_cus": cus}, expect_T=T, expect_refill=2, missing_rate=miss)


def test_accumulator_indexing_across_rounds(oracle):
    """A dense model in a window of 64: events every few positions, the ring wraps six times a sweep, rounds admit no group, one group and
    several -- the accumulator of a position is found from the round's start in every one of them."""
    run_vs_oracle(oracle, 400, 2048, iters=3, causal_frac=0.3, opts={"refill": 2, "window": 64}, expect_refill=2)


def test_the_chain_does_not_depend_on_the_form_of_the_pass(oracle):
    """Same data, early_advance = 0 (no message that depends on timing): window_end16 = 0 (every group by lane) against 1 (whole groups
    without masks).  The window's end moves which round a column's dot is taken in, not the chain: order and components identical, beta
    and acum within the tolerance of test_gpu_resident."""
    M, N = 400, 4099
    bed, y = make_case(M, N, seed=11)
    outs = []
    for wend in (0, 1):
        dev = capi.Device(0)
        dev.load_bed(bed, N)
        dev.set_option("engine", 2)
        dev.set_option("refill", 2)
        dev.set_option("early_advance", 0)
        dev.set_option("window_end16", wend)
        ch = capi.Chain(dev, y, seed=31, shuffle=1)
        for _ in range(3):
            ch.iterate()
        ss = dev.sweep_stats()
        assert ss["engine"] == 2 and ss["refill"] == 2 and ss["walker"] == 2
        beta, comp, acum = dev.get_beta()
        outs.append((beta, comp, acum, np.array(ch.order())))
    assert np.array_equal(outs[0][1], outs[1][1]), "components differ between the two forms of the pass"
    assert np.array_equal(outs[0][3], outs[1][3]), "marker order differs between the two forms of the pass"
    assert close(outs[0][0], outs[1][0]) and close(outs[0][2], outs[1][2])
