"""The device's three entry points of the summary-statistics sweep (hgibbs_ss_sweep, hgibbs_ss_sweep_streams,
hgibbs_ss_sweep_replicas; DESIGN.md sections 31 to 33) held to the dense restatement of tests/ss_restate.py on the device's own band,
fetched with hgibbs_ss_band_get.  Every other GPU test of the sweep holds the device to the host engine, which is built from the same
header, or to the oracle's chain at a band that covers every pair; this one holds the windowed sampler to a program that shares
nothing with it but the oracle's draws.

Plans, rule, invariant and the conditions on the inputs are tests/test_ss_restatement_cpu.py's: components, cass, nnz and every
generator's 624 words and index equal; beta, acum and c within ss_common.close; the zero patterns equal; after every sweep the
device's c is `close` to b - A beta of the device's effects in longdouble.  The mask the restatement is given is adaV and "the
marker's standard deviation is finite" from hgibbs_marker_stats.  The seeds were chosen on the CPU, with NumPy's band of the same
panel (test_ss_restatement_cpu.panel_band) in the device's place.

Shapes: M = 257, N = 131 with ragged windows of W = 5, 64 and 300 (below, inside and above the workgroup's 256 threads), two groups,
one switched off in one sweep, a non-zero start and xty scaled by up to 600; one marker; two with W = 1; K = 2 and K = 8 at W = 16;
n_eff = 3777.5 through step_py; a monomorphic marker; M = 1500, where a sweep crosses a 624-word generator block; intervals of 1, 2
and 254 markers; two replicas of two intervals each."""
import numpy as np
import pytest

import test_ss_restatement_cpu as rc
from hydra_amd import capi, synth
from test_ss_streams_cpu import copy_rng, words

pytestmark = pytest.mark.gpu

N = 131
SMALL = dict(patterns=False, back_to_zero=False)
MONO = 77
# (name, M, W, make_plan's arguments, check_inputs' arguments); the seeds are ones that meet check_inputs
SWEEP_CASES = [
    ("W5", 257, 5, dict(seed=21, two_groups=True), {}),
    ("W64", 257, 64, dict(seed=22, two_groups=True), {}),
    ("W300", 257, 300, dict(seed=23, two_groups=True), {}),
    ("M1", 1, 1, dict(seed=24, ragged=False), SMALL),
    ("M2-W1", 2, 1, dict(seed=25, ragged=False), SMALL),
    ("K2", 257, 16, dict(seed=26, mS=rc.MS2K), {}),
    ("K8", 257, 16, dict(seed=27, mS=rc.MS8), {}),
    ("n_eff-3777.5", 257, 64, dict(seed=28, two_groups=True, n_eff=3777.5), {}),
    ("monomorphic", 257, 16, dict(seed=29, mono=MONO), {}),
    ("M1500", 1500, 5, dict(seed=30), {}),
]
STREAMS_CASE = ("streams-1-2-254", 257, 5, dict(seed=31, two_groups=True, sizes=[1, 2, 254]), {})
REPLICAS_CASE = ("replicas-2x2", 257, 16, dict(seed=32, two_groups=True, sizes=[128, 129], R=2, starts=("xty", "zero")), {})


def make(case):
    name, M, W, kw, conditions = case
    plan = rc.make_plan(M, N, W, **kw)
    if kw.get("mono") is not None:
        for sweep in plan["reps"][0]["sweeps"]:
            sweep[4][kw["mono"]] = 1  # adaV = 1, and still never adaptive
        plan["reps"][0]["beta0"][kw["mono"]] = 0.02
    return name, plan, conditions


def open_device(plan):
    """(dev, ok): the panel loaded, the model set; ok = the marker's standard deviation is finite"""
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(plan["geno"]), plan["N"])
    dev.set_model(plan["groups"], plan["cVa"], plan["cVaI"])
    return dev, np.isfinite(dev.marker_stats()[1]).astype(np.uint8)


def run_device(dev, plan):
    """hgibbs_ss_sweep, or hgibbs_ss_sweep_streams where the plan has intervals, over the three sweeps"""
    rep = plan["reps"][0]
    dev.ss_begin(plan["n_eff"], plan["W"], plan["xty"], plan["ahead"])
    dev.set_beta(rep["beta0"])
    rngs = [copy_rng(g) for g in rep["rngs"]]
    out = []
    for order, sigmaE, sigmaG, estPi, adaV in rep["sweeps"]:
        if len(rngs) == 1:
            cass, nnz = dev.ss_sweep(order, sigmaE, sigmaG, estPi, adaV, rngs[0])
        else:
            cass, nnz = dev.ss_sweep_streams(order, sigmaE, sigmaG, estPi, adaV, plan["bounds"], rngs)
        beta, comp, acum = dev.get_beta()
        out.append(rc.snapshot(cass, nnz, beta, comp, acum, dev.ss_state()[0], rngs))
    return out


def run_replicas(dev, plan):
    """hgibbs_ss_sweep_replicas over the three sweeps: out[r][sweep]"""
    reps = plan["reps"]
    R = len(reps)
    dev.ss_begin(plan["n_eff"], plan["W"], plan["xty"], plan["ahead"])
    dev.ss_replicas(R)
    for r, rep in enumerate(reps):
        dev.ss_replica_set_beta(r, rep["beta0"])
    rngs = [[copy_rng(g) for g in rep["rngs"]] for rep in reps]
    out = [[] for _ in reps]
    for s in range(3):
        sw = [rep["sweeps"][s] for rep in reps]
        cass, nnz = dev.ss_sweep_replicas(np.stack([x[0] for x in sw]), [x[1] for x in sw], np.stack([x[2] for x in sw]), np.stack([x[3] for x in sw]),
                                          np.stack([x[4] for x in sw]), rngs, bounds=plan["bounds"])
        for r in range(R):
            beta, comp, acum, c = dev.ss_replica_get(r)
            out[r].append(rc.snapshot(cass[r], nnz[r], beta, comp, acum, c, rngs[r]))
    return out


@pytest.mark.parametrize("case", SWEEP_CASES, ids=[c[0] for c in SWEEP_CASES])
def test_sweep_against_the_restatement(oracle, case):
    name, plan, conditions = make(case)
    dev, ok = open_device(plan)
    got = run_device(dev, plan)
    band = dev.ss_band()
    mono = case[3].get("mono")
    if mono is None:
        assert ok.all()
    else:
        W = plan["W"]
        assert not ok[mono] and np.delete(ok, mono).all()
        assert not band[mono].any() and not any(band[mono - d, d - 1] for d in range(1, W + 1))
        for g in got:  # adaV = 1 there, and the marker takes no step: its effect goes to 0 with acum 1
            assert g["beta"][mono] == 0.0 and g["acum"][mono] == 1.0 and g["comp"][mono] == 0
    if name == "M1500":
        x0 = words(plan["reps"][0]["rngs"][0])[0]
        assert not np.array_equal(got[0]["x"][0], x0) and got[0]["idx"][0] <= 624  # 1500 markers a sweep: the block was refilled
    rc.hold_case(oracle, name, plan, band, ok, got, **conditions)


def test_streams_against_the_restatement(oracle):
    name, plan, conditions = make(STREAMS_CASE)
    dev, ok = open_device(plan)
    got = run_device(dev, plan)
    rc.hold_case(oracle, name, plan, dev.ss_band(), ok, got, **conditions)


def test_replicas_against_the_restatement(oracle):
    name, plan, conditions = make(REPLICAS_CASE)
    assert plan["reps"][0]["beta0"].any() and not plan["reps"][1]["beta0"].any()
    dev, ok = open_device(plan)
    got = run_replicas(dev, plan)
    band = dev.ss_band()
    for r in range(2):
        rc.hold_case(oracle, "%s replica %d" % (name, r), plan, band, ok, got[r], r=r, **conditions)
