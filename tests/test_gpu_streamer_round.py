"""The streaming workgroups' round of the resident sweep engine -- the Gram terms of the window columns behind an event
(hg_resident.hip.h: rs_gram_terms) and the refill's group pass (hg_streamer2.hip.h) -- as chains against the CPU oracle, at the bar
of tests/test_gpu_resident.py (run_vs_oracle: order, components, cass, generator state and number of updates exact; beta, acum, the
hyper-parameters and the residual within 1e-9).

rs_gram_terms takes the V columns behind the event in groups of eight per wave: one address per group where the group does not
straddle the ring's wrap and a slot per column where it does, half a group where the wave's columns end there, a reduce-scatter
over four, eight or sixteen accumulators by the wave's number of columns.  M = 700 markers and three iterations, sparse and dense
in events, are chosen so that events fall at every distance from the window's end (every V from 1 to B - 1), with the wrap inside a
wave's group and at every width of the reduction; windows of 32, 64 and 256 columns; one and two tiles per workgroup, a ragged
last tile, both forms of the streaming workgroups (the first calls the same function).  The group pass shares these shapes; four tiles per workgroup (a
128-column window) and a column set with missing calls (the other build of the same pass) are added for it.  Every case asserts the
tiles per workgroup, the form and the walker that sweep_stats() reports: none can run another path unnoticed.
"""
import pytest

from test_gpu_resident import run_vs_oracle

pytestmark = pytest.mark.gpu

M = 700
# N, option res_cus (None: every compute unit), tiles per workgroup
SHAPES = [(3000, None, 1),  # three workgroups of one tile
          (8000, 5, 2),     # four workgroups of two tiles
          (4099, None, 1)]  # a ragged fifth tile


def _opts(window, cus, refill):
    o = {"window": window, "refill": refill}
    if cus:
        o["res_cus"] = cus
    return o


@pytest.mark.parametrize("refill", [1, 2])
@pytest.mark.parametrize("causal_frac", [0.05, 0.3])
@pytest.mark.parametrize("window", [32, 64, 256])
@pytest.mark.parametrize("N,cus,T", SHAPES)
def test_gram_terms_and_refill_at_every_distance_from_the_windows_end(oracle, N, cus, T, window, causal_frac, refill):
    run_vs_oracle(oracle, M, N, iters=3, opts=_opts(window, cus, refill), causal_frac=causal_frac, expect_T=T, expect_refill=refill, expect_walker=2)


@pytest.mark.parametrize("causal_frac", [0.05, 0.3])
def test_four_tiles_per_workgroup_and_a_window_of_128(oracle, causal_frac):
    run_vs_oracle(oracle, M, 8000, iters=3, opts={"res_cus": 3}, causal_frac=causal_frac, expect_T=4, expect_refill=2, expect_walker=2)


@pytest.mark.parametrize("window", [32, 64, 256])
def test_missing_calls_share_the_group_pass(oracle, window):
    run_vs_oracle(oracle, M, 4099, iters=3, opts={"window": window}, causal_frac=0.05, missing_rate=0.01, expect_T=1, expect_refill=2, expect_walker=2)
