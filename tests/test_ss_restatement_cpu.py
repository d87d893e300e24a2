"""The summary-statistics sweep held to an independent restatement on a dense matrix (tests/ss_restate.py), the
part that needs no device.  Every other test of the sweep compares two programs built from hg_ss_step.h, or uses a band that covers
every pair; here the windowed sampler -- ragged `ahead`, zeros, runs of zeros, markers whose neighbours behind hold nobody while a
window from further back covers them -- meets a program that shares nothing with it but the oracle's two draws.

  step_py against orc_marker_draw on a grid of num up to 600 sqrt(n) 8 in both signs: the restatement's own step is the oracle's.
  hgibbs_ss_sweep_host against sweep(use_orc=True) over three sweeps from a non-zero start, and against step_py at n_eff = 3777.5.
  hgibbs_ss_sweep_streams_host against one sweep per interval on the order grouped by a list comprehension.
  After every sweep c is `close` to b - A beta in longdouble, for the engine and for the restatement.

The rule is the project's (tests/test_gpu_ss_sweep.py): components, cass, nnz, the generators' 624 words and index equal; beta, acum
and c within ss_common.close; the zero patterns equal.  `close`, not bits: the two sides are different programs.

The inputs are what makes the comparison worth anything, so they are checked too, on the restatement's log alone (`check_inputs`):
xty ~ N(0, n_eff) with a fifth of the entries times 8 .. 600 and a pi entry of 1e-300 in one sweep, so that the 700 rule of share()
fires in each of its patterns; a pi entry of 1e-306 in another sweep, so that the rule also zeroes a share that would have counted
(see TINY: with the inputs above alone, `l > k + 1` in place of `l > k` in share() changed no result); every component chosen; an effect that steps back to 0; c bounded (the band comes from real columns: a random band is not positive
semi-definite and the chain leaves every bound); and no decision closer than 1e-9 to its threshold, the reason
tests/test_ss_host_vs_oracle_cpu.py gives for its seeds.  Where a case is too small for a condition (one or two markers; K = 2 has no
component strictly between 0 and K - 1 and no later share that the rule can zero) the condition is not asked of it, and the
test says so in its arguments.  tests/test_gpu_ss_restate.py holds the device's three entry points to the same restatement with this
module's plans and rule."""
import ctypes as C

import numpy as np
import pytest

import orc
import ss_common as sc
import ss_restate as sr
from hydra_amd import capi, synth
from test_ss_streams_cpu import blocks_ahead, copy_rng, seeded, words

MS4 = sc.MS1
MS2K = np.array([[0.0, 0.01]])
MS8 = np.array([[0.0, 1e-5, 1e-4, 1e-3, 3e-3, 1e-2, 3e-2, 1e-1]])
SCALES = (8.0, 20.0, 40.0, 80.0, 200.0, 600.0)
MARGIN = 1e-9
# A share of 1e-300 puts a component 690.8 below the others: short of the 700 rule unless the data add to it, and then the component
# that is 700 above swamps the sum, so the rule replaces a share of next to nothing by 0.  With this entry (log = -704.6) a later
# component lies 700 BELOW an earlier one at every null marker, and the rule zeroes a share of order 1: there it changes the draw.
TINY = 1e-306


def ragged_ahead(M, W, rs):
    """Windows of mixed lengths with zeros, a run of zeros, and (where there is room) a marker whose window covers the four behind it
    while none of those holds anybody: the engines have to skip them by ahead[k] >= d"""
    ahead = np.minimum(rs.integers(0, W + 1, M), M - 1 - np.arange(M))
    ahead[rs.random(M) < 0.2] = 0
    if M >= 30:
        a, b = M // 3, M // 6
        ahead[a:a + 10] = 0
        ahead[b] = min(W, 4)
        ahead[b + 1:b + 5] = 0
    return ahead.astype(np.uint32)


def marker_stats(geno):
    """mave, mstd of the chain's columns (src/BayesRRm.cpp:1502-1507); mstd is inf at a monomorphic marker"""
    called = geno != 3
    g = np.where(called, geno, 0).astype(np.float64)
    mave = g.sum(axis=1) / called.sum(axis=1)
    ss = (np.where(called, g - mave[:, None], 0.0) ** 2).sum(axis=1)
    with np.errstate(divide="ignore"):
        return mave, np.sqrt((geno.shape[1] - 1) / ss)


def make_plan(M, N, W, mS=MS4, seed=1, n_eff=4000.0, two_groups=False, ragged=True, sizes=None, mono=None, R=1, starts=("random",)):
    """A case: the panel, the window, xty and, per replica, a start, three sweeps and one generator per interval.
    sizes: the intervals of independent blocks (None: one); mono: a marker made monomorphic; starts[r]: "random", "xty" (the marginal
    estimate xty / (n_eff - 1) at the scaled entries) or "zero"."""
    if two_groups:
        mS = np.vstack([mS[0], mS[0] * 10.0])  # (K = 4: ss_common.MS2)
    G, K = mS.shape
    rs = np.random.default_rng(seed)
    geno = synth.make_genotypes(M, N, seed=seed, missing_rate=0.02)
    if mono is not None:
        geno[mono, :] = np.where(geno[mono, :] == 3, 3, 2)
    ahead = ragged_ahead(M, W, rs) if ragged else np.minimum(W, M - 1 - np.arange(M)).astype(np.uint32)
    if sizes is not None:
        ahead = np.minimum(ahead, blocks_ahead(sizes, W)).astype(np.uint32)
    xty = rs.normal(0.0, np.sqrt(n_eff), M)
    big = rs.random(M) < 0.2
    xty[big] *= rs.choice(SCALES, int(big.sum()))
    groups = (np.arange(M) % 3 == 0).astype(np.int32) if two_groups else None
    cVa = mS.copy()
    cVaI = np.zeros_like(mS)
    cVaI[:, 1:] = 1.0 / mS[:, 1:]
    S = 1 if sizes is None else len(sizes)
    reps = []
    for r in range(R):
        if starts[r] == "random":
            beta0 = np.where(rs.random(M) < 0.3, rs.normal(0.0, 0.05, M), 0.0)
        elif starts[r] == "xty":
            beta0 = np.where(big, xty / (n_eff - 1.0), 0.0)
        else:
            beta0 = np.zeros(M)
        sweeps = []
        for s in range(3):
            sigmaG = rs.uniform(0.2, 0.6, G)
            if two_groups and s == 1:
                sigmaG[G - 1] = 0.0  # one group switched off in one sweep
            estPi = rs.dirichlet(np.ones(K) * 2.0, G)
            if s == 2:
                estPi[0, 1 if K > 2 else 0] = 1e-300
            if s == 0:
                estPi[G - 1, 1] = TINY
            adaV = (rs.random(M) < 0.85).astype(np.uint8) if M > 2 else np.ones(M, dtype=np.uint8)
            sweeps.append((rs.permutation(M).astype(np.int32), 0.4 + 0.1 * s + 0.03 * r, sigmaG, estPi, adaV))
        reps.append(dict(beta0=beta0, sweeps=sweeps, rngs=[seeded(seed + 100 + 1000 * r + i) for i in range(S)]))
    bounds = np.concatenate([[0], np.cumsum([M] if sizes is None else sizes)]).astype(np.uint32)
    return dict(M=M, N=N, W=W, K=K, G=G, n_eff=float(n_eff), geno=geno, ahead=ahead, xty=xty, groups=groups, cVa=cVa, cVaI=cVaI, bounds=bounds,
                reps=reps, use_orc=float(n_eff) == int(n_eff))


def panel_band(plan):
    """(band, ok): the band of the plan's panel from NumPy's standardised columns -- (n_eff - 1) r with r = x_j'x_k / (N - 1), 0 beyond
    ahead[j] and at a marker without a finite standard deviation -- and the flag "the marker's standard deviation is finite\""""
    M, N, W = plan["M"], plan["N"], plan["W"]
    mave, mstd = marker_stats(plan["geno"])
    ok = np.isfinite(mstd)
    X = sc.standardised(synth.pack_bed_columns(plan["geno"]), N, mave, np.where(ok, mstd, 0.0))
    band = sc.full_band(X, W) * ((plan["n_eff"] - 1.0) / (N - 1.0))
    band[np.arange(1, W + 1)[None, :] > plan["ahead"][:, None]] = 0.0
    return band, ok.astype(np.uint8)


def snapshot(cass, nnz, beta, comp, acum, c, rngs):
    return dict(cass=np.array(cass), nnz=int(nnz), beta=beta.copy(), comp=comp.copy(), acum=acum.copy(), c=c.copy(),
                x=np.stack([words(g)[0] for g in rngs]), idx=[int(g.idx) for g in rngs])


def run_host(plan, band, r=0):
    """The host engine over the three sweeps of replica r: hgibbs_ss_sweep_host, or hgibbs_ss_sweep_streams_host where there are intervals"""
    rep = plan["reps"][r]
    M = plan["M"]
    c, beta, comp, acum = plan["xty"].copy(), rep["beta0"].copy(), np.zeros(M, dtype=np.int32), np.zeros(M)
    rngs = [copy_rng(g) for g in rep["rngs"]]
    out = []
    for order, sigmaE, sigmaG, estPi, adaV in rep["sweeps"]:
        args = (plan["n_eff"], plan["W"], plan["ahead"], band, c, beta, comp, acum, plan["groups"], plan["cVa"], plan["cVaI"], order, sigmaE, sigmaG, estPi, adaV)
        if len(rngs) == 1:
            cass, nnz = capi.ss_sweep_host(*args, rngs[0])
        else:
            cass, nnz = capi.ss_sweep_streams_host(*args, plan["bounds"], rngs)
        out.append(snapshot(cass, nnz, beta, comp, acum, c, rngs))
    return out


def drift(c, want):
    """max |c - want| / max(1, |c|), in longdouble"""
    c = np.asarray(c, dtype=np.longdouble)
    return float(np.max(np.abs(c - want) / np.maximum(1.0, np.abs(c))))


def check_inputs(name, log, cs, xty, K, M, patterns=True, back_to_zero=True):
    """The conditions on a case's inputs, on the restatement's log and its c after every sweep.  patterns: the case is large enough to
    be asked for every component and every pattern of the 700 rule that its K allows."""
    assert max(np.max(np.abs(c)) for c in cs) < 1e3 * np.max(np.abs(xty)), name
    margin = min(v[3] for v in log)
    print("%s: visits %d, smallest |prob - acum| %.3g" % (name, len(log), margin))
    assert margin > MARGIN, (name, margin)
    if back_to_zero:
        assert any(v[4] != 0.0 and v[5] == 0.0 for v in log), name
    if not patterns:
        return
    if K <= 4:
        assert {v[2] for v in log} == set(range(K)), name
    assert any(v[1][0] for v in log), name  # share 0 zeroed
    assert any(v[6] > 1e-3 for v in log), name  # the rule zeroed a share that would have counted
    if K > 2:
        # share 0 kept while a later share that entered the walk (k <= the chosen component) is zeroed
        assert any(not v[1][0] and any(v[1][1:v[2] + 1]) for v in log), name
        assert any(not any(v[1]) and 0 < v[2] < K - 1 for v in log), name


def hold_case(L, name, plan, band, ok, got, r=0, **conditions):
    """The rule: `got` (the snapshots of an engine after each of replica r's three sweeps) against the restatement on the dense matrix
    of `band`; then the invariant on both sides and the conditions on the inputs.  Returns the figures (restatement's drift, engine's
    drift, largest |c|)."""
    M, K, n_eff, bounds = plan["M"], plan["K"], plan["n_eff"], [int(b) for b in plan["bounds"]]
    rep = plan["reps"][r]
    A = sr.dense(band, plan["ahead"], n_eff)
    assert np.array_equal(A, A.T) and np.all(np.diag(A) == n_eff - 1.0)
    AL = A.astype(np.longdouble)
    b = np.asarray(plan["xty"], dtype=np.longdouble) + AL @ rep["beta0"].astype(np.longdouble)  # c starts at xty beside beta0
    c, beta, comp, acum = plan["xty"].copy(), rep["beta0"].copy(), np.zeros(M, dtype=np.int32), np.zeros(M)
    rngs = [sr.rng_from(*words(g)) for g in rep["rngs"]]
    log, cs, fig = [], [], [0.0, 0.0, 0.0]
    for s, (order, sigmaE, sigmaG, estPi, adaV) in enumerate(rep["sweeps"]):
        mask = adaV.astype(bool) & ok.astype(bool)
        cass, nnz = np.zeros((plan["G"], K), dtype=np.int32), 0
        for i, g in enumerate(rngs):  # an interval's markers in the order the shuffle gave them, with that interval's generator
            part = [j for j in order if bounds[i] <= j < bounds[i + 1]]
            ca, nz, lg = sr.sweep(L, A, c, beta, comp, acum, plan["groups"], plan["cVa"], plan["cVaI"], part, sigmaE, sigmaG, estPi, mask, g, n_eff, plan["use_orc"])
            cass += ca
            nnz += nz
            log += lg
        cs.append(c.copy())
        e = got[s]
        want = sr.invariant(b, AL, beta)
        fig = [max(fig[0], drift(c, want)), max(fig[1], drift(e["c"], sr.invariant(b, AL, e["beta"]))), max(fig[2], float(np.max(np.abs(c))))]
        print("%s sweep %d: drift of c from b - A beta: restatement %.3g, engine %.3g; max |c| %.6g; nnz %d" % (name, s, fig[0], fig[1], fig[2], nnz))
        assert np.array_equal(e["comp"], comp) and np.array_equal(e["cass"], cass) and e["nnz"] == nnz, (name, s)
        assert e["idx"] == [int(g.idx) for g in rngs] and np.array_equal(e["x"], np.stack([sr.rng_words(g)[0] for g in rngs])), (name, s)
        assert sc.close(e["beta"], beta) and sc.close(e["acum"], acum) and sc.close(e["c"], c), (name, s)
        assert np.array_equal(e["beta"] == 0.0, beta == 0.0), (name, s)
        # the invariant: the restatement's own c first (where it fails the input is unfit), then the engine's on the engine's effects
        assert sc.close(c, want.astype(np.float64)), (name, s)
        assert sc.close(e["c"], sr.invariant(b, AL, e["beta"]).astype(np.float64)), (name, s)
    check_inputs(name, log, cs, plan["xty"], K, M, **conditions)
    return fig


# ---- the restatement's own step is the oracle's ----
@pytest.mark.parametrize("K", [2, 4, 8])
def test_step_py_is_orc_marker_draw(oracle, K):
    L = oracle
    n = 4000
    rs = np.random.default_rng(K)
    mS = {2: MS2K, 4: MS4, 8: MS8}[K]
    cVa = mS[0].copy()
    cVaI = np.zeros(K)
    cVaI[1:] = 1.0 / cVa[1:]
    top = 600.0 * np.sqrt(n) * 8.0
    grid = np.concatenate([[0.0], np.geomspace(1.0, top, 60)])
    grid = np.concatenate([grid, -grid[1:]])
    ga, gb = sr.rng_from(*words(seeded(5 + K))), sr.rng_from(*words(seeded(5 + K)))
    bn, kk, ac = C.c_double(), C.c_int(), C.c_double()
    chosen, zeroed0, zeroed_later, counted = set(), 0, 0, 0
    for sigmaG in (0.4, 0.0):
        for tiny in (0.0, 1e-300, TINY):
            estPi = rs.dirichlet(np.ones(K) * 2.0)
            if tiny:
                estPi[1 if K > 2 or tiny == TINY else 0] = tiny
            for num in grid:
                for beta_old in (0.0, 0.03):
                    c_j = float(num) - beta_old * (n - 1)  # so that num is the grid's value
                    sigmaE = 0.5
                    assert L.orc_marker_draw(c_j, beta_old, n, K, orc.dptr(cVa), orc.dptr(cVaI), orc.dptr(estPi), sigmaE, sigmaG, C.byref(ga),
                                             C.byref(bn), C.byref(kk), C.byref(ac)) == 0
                    new, k, a0, z, _, cut = sr.step_py(L, c_j, beta_old, float(n - 1), K, list(cVa), list(cVaI), list(estPi), sigmaE, sigmaG, gb)
                    assert k == kk.value, (num, sigmaG, tiny)
                    assert ga.idx == gb.idx and np.array_equal(sr.rng_words(ga)[0], sr.rng_words(gb)[0])
                    assert sc.close(new, bn.value) and sc.close(a0, ac.value), (num, sigmaG, tiny)
                    assert (new == 0.0) == (bn.value == 0.0) and (a0 == 0.0) == z[0]
                    chosen.add(k)
                    zeroed0 += z[0]
                    zeroed_later += (not z[0]) and any(z[1:])
                    counted += cut > 1e-3
    assert chosen == set(range(K)) if K <= 4 else {0, K - 1} <= chosen
    assert zeroed0 > 0 and (K == 2 or zeroed_later > 0) and counted > 0


# ---- the host engine against the restatement ----
# (name, M, N, W, make_plan's and check_inputs' arguments); the seeds are ones that meet check_inputs
HOST_CASES = [
    ("W1", 257, 517, 1, dict(seed=1, two_groups=True), {}),
    ("W5", 257, 517, 5, dict(seed=2, two_groups=True), {}),
    ("W64", 257, 517, 64, dict(seed=3, two_groups=True), {}),
    ("W256", 257, 517, 256, dict(seed=4, two_groups=True), {}),
    ("W300", 257, 517, 300, dict(seed=5, two_groups=True), {}),
    ("K2", 64, 131, 8, dict(seed=6, mS=MS2K), {}),
    ("K8", 64, 131, 8, dict(seed=7, mS=MS8), {}),
    ("M1", 1, 131, 1, dict(seed=8, ragged=False), dict(patterns=False, back_to_zero=False)),
    ("M2-W1", 2, 131, 1, dict(seed=9, ragged=False), dict(patterns=False, back_to_zero=False)),
    ("n_eff-3777.5", 257, 517, 64, dict(seed=10, two_groups=True, n_eff=3777.5), {}),
    ("streams-1-2-254", 257, 517, 5, dict(seed=11, two_groups=True, sizes=[1, 2, 254]), {}),
]


@pytest.mark.parametrize("case", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_host_engine_against_the_restatement(oracle, case):
    name, M, N, W, kw, conditions = case
    plan = make_plan(M, N, W, **kw)
    band, ok = panel_band(plan)
    assert ok.all()
    if M >= 30:
        ah = plan["ahead"]
        assert (ah == 0).any() and (ah[M // 3:M // 3 + 10] == 0).all() and ah[M // 6] == min(W, 4) and not ah[M // 6 + 1:M // 6 + 5].any()
    hold_case(oracle, name, plan, band, ok, run_host(plan, band), **conditions)
