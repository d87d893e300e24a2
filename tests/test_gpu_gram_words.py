"""The chain's Gram words (hydra_amd/csrc/hg_walker2.hip.h, DESIGN.md 4R "The chain's Gram words"): a chain wave takes an event's Gram
terms as the growth of ONE sum over the slot's eight accumulator rows -- complete when the sum's count field has grown by W, the number
of streaming workgroups -- and keeps one last-seen sum per parity.  What can go wrong with that is a matter of the geometry: how W
spreads over the rows (W % 8, W < 8: rows nobody adds to), how often the sums wrap mod 2^32 (2^64 with missing calls), the polls that
start before any word is there, and the size of the total term.

The bar is test_gpu_resident.run_vs_oracle's: order, components, generator state and update count exact, the rest within 1e-9.

The geometries.  A shard is padded to whole blocks of 4096 individuals, so the number of wave tiles (1024 individuals) is a multiple of
four, a workgroup holds T = 1, 2 or 4 of them (plan_sweep: ceil(tiles / (res_cus - 1)), anything above 2 becomes 4) and W = ceil(tiles / T).
At T = 1 and T = 2, W is therefore even: the uneven split over the eight rows at T = 1 is W = 12 (rows 0 - 3 take two arrivals, rows
4 - 7 one), and the odd counts 13, 5 and 3 exist at T = 4 only.  Both are run."""
import numpy as np
import pytest

import orc
from hydra_amd import capi, synth
from test_gpu_parity import close, _same_stream
from test_gpu_resident import run_vs_oracle

pytestmark = pytest.mark.gpu

# name: N, res_cus, T, W
GEOM = {
    "W12_T1": (12001, 13, 1, 12),  # uneven rows: 2 2 2 2 1 1 1 1
    "W13_T4": (50001, 14, 4, 13),  # uneven rows, odd: 2 2 2 2 2 1 1 1
    "W3_T4": (12001, 4, 4, 3),     # rows 3 - 7 are never written
    "W4_T1": (4000, 5, 1, 4),      # rows 4 - 7 are never written
    "W8_T1": (8000, 9, 1, 8),      # the exact multiple: one arrival per row
    "W6_T2": (12001, 7, 2, 6),     # two tiles per workgroup
    "W5_T4": (20011, 6, 4, 5),
}
M = 400


def plan_of(N, cus):
    """plan_sweep's geometry (hgibbs.hip): tiles per workgroup and streaming workgroups"""
    tiles = (N + 4095) // 4096 * 4
    T = -(-tiles // (cus - 1))
    T = T if T <= 2 else 4
    return T, -(-tiles // T)


def run_geom(oracle, name, opts=None, min_events=0, **kw):
    N, cus, T, W = GEOM[name]
    assert plan_of(N, cus) == (T, W)
    o = {"res_cus": cus}
    o.update(opts or {})
    # causal_frac 0.3, four sweeps: from the second sweep on most markers are consecutive, announced events -- both parities are used
    # again and again, and a slot's row sum gains W 2^24 per event: it wraps after 256 / W events
    ch, ref, dev = run_vs_oracle(oracle, M, N, iters=4, causal_frac=0.3, opts=o, expect_T=T, expect_walker=2, **kw)
    ss = dev.sweep_stats()
    assert ss["events"] >= min_events, "events in the last sweep: %d" % ss["events"]
    return ss


@pytest.mark.parametrize("name", list(GEOM))
def test_row_sums(oracle, name):
    # (the last sweep alone wraps a slot's sum at least twice where W >= 12: 2 x 256 / 12 = 43 events)
    run_geom(oracle, name, min_events=43 if GEOM[name][3] >= 12 else 0)


@pytest.mark.parametrize("opts", [{"announce": 0}, {"early_advance": 0}], ids=["announce_off", "early_advance_off"])
def test_polls_that_start_from_nothing(oracle, opts):
    """Without announcements the streaming workgroups learn of an event from its message only: the chain's poll starts before any word
    of the event is there and goes through its retry path.  Without early advances every round waits for its event."""
    run_geom(oracle, "W12_T1", opts=opts, min_events=43)


@pytest.mark.parametrize("window", [64, 128])
def test_run_time_window_and_mixture(oracle, window):
    """The instances with the window and the number of components as run-time values (the constant-window K = 4 decider does not apply)."""
    run_geom(oracle, "W12_T1", opts={"window": window}, mS=np.array([[0.0, 0.001, 0.01]]))


@pytest.mark.parametrize("name,cols", [("W12_T1", 1.0), ("W13_T4", 1.0), ("W3_T4", 1.0), ("W8_T1", 1.0), ("W6_T2", 1.0), ("W12_T1", 0.25)],
                         ids=["W12_T1", "W13_T4", "W3_T4", "W8_T1", "W6_T2", "W12_T1_quarter_of_the_columns"])
def test_row_sums_missing_calls(oracle, name, cols):
    """Missing calls: the build with 8-byte words, count in the top byte, fixed-point terms below."""
    run_geom(oracle, name, missing_rate=0.02, missing_cols=cols)


def test_the_largest_total_term(oracle):
    """The sum's low 24 bits hold the TOTAL term of a slot, at most 4 n_local.  Columns that are genotype 2 nearly everywhere (thirty 0s
    each, so that the variance is not zero) at N = 130 001, 128 streaming workgroups: every raw Gram term A_jq is within 240 of
    4 N = 520 004.  The columns' standardised values are +- 1 / sqrt(N) but for the thirty: the chain is an ordinary one."""
    N, Mc, zeros = 130001, 96, 30
    rng = np.random.default_rng(5)
    geno = np.full((Mc, N), 2, dtype=np.uint8)
    for j in range(Mc):
        geno[j, rng.choice(N, size=zeros, replace=False)] = 0
    y, _ = synth.make_phenotype(geno, seed=6, h2=0.5, causal_frac=0.3)
    bed = synth.pack_bed_columns(geno)
    assert plan_of(N, 256)[1] == 128
    ref = orc.Chain(oracle, bed, N, y, seed=1222, shuffle=1)
    dev = capi.Device(0)
    dev.load_bed(bed, N)
    dev.set_option("engine", 2)
    ch = capi.Chain(dev, y, seed=1222, shuffle=1)
    events = 0
    for it in range(3):
        ref.iterate()
        ch.iterate()
        beta, comp, acum = dev.get_beta()
        st = ch.state()
        ss = dev.sweep_stats()
        events += ss["events"]
        assert ss["engine"] == 2 and ss["launches"] == 1 and ss["accepted_markers"] == Mc and ss["walker"] == 2
        assert ss["tiles_per_workgroup_max"] == 1
        assert np.array_equal(ch.order(), ref.arr("order")), "marker order diverged at it %d" % it
        assert np.array_equal(comp, ref.arr("components")), "component indices differ at it %d" % it
        assert np.array_equal(st["cass"].ravel(), ref.arr("cass"))
        assert close(beta, ref.arr("beta")), "beta beyond tolerance at it %d" % it
        assert close(acum, ref.arr("acum"))
        assert close(st["sigmaG"], ref.arr("sigmaG")) and close(st["estPi"].ravel(), ref.arr("estPi"))
        assert close(st["sigmaE"], ref.sigmaE) and close(st["mu"], ref.mu)
        rx, ridx = ref.rng_state()
        assert st["rng_idx"] % 624 == ridx % 624 and np.array_equal(st["rng_x"], rx) or _same_stream(st["rng_x"], st["rng_idx"], rx, ridx)
        assert close(dev.get_residual(), ref.arr("eps"), 1e-9)
        assert ch.last_nnz() == oracle.orc_chain_last_nnz(ref.h)
    assert events > 0, "no event took the Gram trip"
