"""The decider's round of the resident engine's second walker (hg_walker2.hip.h, w2_chain<..., DECIDE = 1, ...>): the other waves'
answers, the first candidate in window order, a5 over the lanes (with the number of components as a constant, K = 4 at a 256-column
window, and as a run-time value), the draw, and the "too close to call, no event: next candidate" loop -- against the CPU oracle.

The bar is tests/test_gpu_resident.py's run_vs_oracle: marker order, components, cass, the generator state and the number of updates
exact, everything else within 1e-9.  Every case runs the second walker (asserted)."""
import numpy as np
import pytest

from test_gpu_resident import run_vs_oracle

pytestmark = pytest.mark.gpu

MS4 = [0.0, 1e-4, 1e-3, 1e-2]
MS_BY_K = {2: [0.0, 0.01], 3: [0.0, 0.001, 0.01], 4: MS4, 5: [0.0, 1e-4, 1e-3, 1e-2, 1e-1], 8: [0.0, 1e-5, 1e-4, 5e-4, 1e-3, 5e-3, 1e-2, 1e-1]}

# Option bound_slack is taken off every threshold of the tabulated bound.  A threshold is log(1 / u - 1) - 1e-9 with u a 32-bit
# uniform: within [-22.2, 22.2] (or + infinity for u = 0).  The bound it is compared with is a chord of f = log sum_l>0 exp(c_l + n2 r_l)
# with n2 r_l >= 0, so it is never below the smallest c_l, and the table is in use only where every c_l >= -699.  With 1000 taken off,
# every finite threshold is below -977 < -699: every position with a dot is a candidate and goes through the exact decision, and
# every round that passes markers without an event runs the retry loop once per marker.
ALL_CANDIDATES = 1000


def few_turned_down(markers_without_event):
    """Without slack a marker without an event is a candidate only where the chord lies above its threshold although the function does
    not: the chord over 256 intervals is within about 1e-3 of the function, and the threshold log(1 / u - 1) has a density of at most
    1 / 4 (that of the logistic distribution, at 0), so that happens to fewer than 2.5e-4 of them -- 0.2 markers of 700.  A tenth of them
    is four hundred times that, and a tenth of what the sweep turns down with every position a candidate (test_retry_path)."""
    return markers_without_event // 10


@pytest.mark.parametrize("causal_frac", [0.05, 0.3])
@pytest.mark.parametrize("window", [8, 32, 64, 128, 256])
def test_windows(oracle, window, causal_frac):
    # one to four chain waves and a partly used one; three sweeps of 700 markers put the cursor, and events, at every slot of the window
    # with the wrap in each wave.  K = 4: the 256-column window runs a5 with K as a constant, the others with the run-time K
    _, _, dev = run_vs_oracle(oracle, 700, 3000, iters=3, mS=np.array([MS4]), opts={"window": window}, causal_frac=causal_frac, expect_walker=2)
    # without slack the retry loop hardly runs (see few_turned_down)
    ss = dev.sweep_stats()
    print("window %d: turned down %d of %d markers without an event" % (window, ss["turned_down"], 700 - ss["events"]))
    assert ss["turned_down"] <= few_turned_down(700 - ss["events"])


@pytest.mark.parametrize("K", [2, 3, 4, 5, 8])
def test_component_counts(oracle, K):
    run_vs_oracle(oracle, 300, 2500, mS=np.array([MS_BY_K[K]]), expect_walker=2)


def test_three_groups_of_four_components(oracle):
    M = 300
    groups = (np.arange(M) % 3).astype(np.int32)
    mS = np.array([[0.0, 0.001, 0.01, 0.1], [0.0, 0.0001, 0.001, 0.01], [0.0, 0.01, 0.1, 1.0]])
    run_vs_oracle(oracle, M, 2500, groups=groups, mS=mS, expect_walker=2)


@pytest.mark.parametrize("missing_rate", [0.0, 0.01])
@pytest.mark.parametrize("K", [4, 3])
@pytest.mark.parametrize("window", [8, 256])
def test_retry_path(oracle, window, K, missing_rate):
    # every position is a candidate (see ALL_CANDIDATES): the bound only ever skips exact evaluations, so the chain is the oracle's still
    M = 700
    _, _, dev = run_vs_oracle(oracle, M, 3000, iters=3, mS=np.array([MS_BY_K[K]]), opts={"window": window, "bound_slack": ALL_CANDIDATES},
                              causal_frac=0.05, missing_rate=missing_rate, expect_walker=2)
    # The slack did reach the thresholds and the retry loop did run: the last sweep's count of candidates that the exact decision turned
    # down.  Every marker is a candidate and is decided exactly once (the search stops at an event, and a candidate turned down is cleared);
    # it is turned down unless an event is found at it -- component k > 0, whose drawn effect differs from the old one (a continuous draw), or
    # k = 0 at a non-zero effect, which changes it too -- so the markers turned down are exactly those without an event.
    ss = dev.sweep_stats()
    print("window %d K %d: turned down %d, markers %d, events %d" % (window, K, ss["turned_down"], M, ss["events"]))
    assert ss["turned_down"] == M - ss["events"]


# (30 000 individuals: with 90 causal markers of 300 the largest effects give num^2 / (2 sigmaE denom) > 700; the oracle's sweeps of
# this case meet the cut-off at two to four markers each, at 8 000 individuals at none)
CUT_M, CUT_N = 300, 30000


def test_cutoffs(oracle):
    """Variances five orders of magnitude apart and large effects: |logL_l - logL_k| > 700 occurs, a5's `bigp` branch (the step's
    threshold is 0).  The oracle's acum is the first step's threshold: exactly 0.0 where the cut-off applied (checked here, on the
    oracle's own chain, so that the inputs cannot silently stop exercising the branch)."""
    _, ref, _ = run_vs_oracle(oracle, CUT_M, CUT_N, iters=3, mS=np.array([[0.0, 1e-5, 1e-2, 1.0]]), causal_frac=0.3, expect_walker=2)
    assert np.any(ref.arr("acum") == 0.0)
