"""hgibbs_reml_eval and hgibbs_reml against the dense restatement (tests/reml_restate.py, X from the device's own marker
statistics), the host rule and finish against the device's own trace, the --reml command line against the binding, and one
planted-signal run against the dense REML root.

Bound of the sums and of f: 4 kappa (tol + drift), kappa = (lambda_max(P_c A P_c) + delta) / delta, drift = 100 iters kappa 2^-52
as in tests/test_gpu_reml_solve.py: a relative residual of tol leaves a relative error of at most kappa tol in v, each of the sums
is a second moment of v (twice that), and the worst case is reached only by a residual that lies along the smallest eigenvector.
The same bound holds f, a difference of logarithms of ratios of the sums."""
import math
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import capi, synth

import reml_restate as rr
from pca_restate import device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N0, M0, Q0 = 300, 500, 3


def phenotype(X, h2, seed):
    rng = np.random.default_rng(seed)
    M = X.shape[1]
    g = X @ (rng.standard_normal(M) * math.sqrt(h2 / M))
    return g + rng.standard_normal(X.shape[0]) * math.sqrt(1.0 - h2)


@pytest.fixture(scope="module")
def base():
    geno = rr.cohort(N0, M0, miss=0.02, seed=21)
    geno[3] = 3
    dev = device(geno)
    mave, mstd = dev.marker_stats()[:2]
    X, good = rr.xmat(geno, mave, mstd)
    Z = rr.covariates(N0, Q0, seed=4)
    y = phenotype(X, 0.5, 22) + Z @ np.array([2.0, 0.5, -1.0])
    return {"dev": dev, "d": rr.Dense(X, good, Z), "Z": Z, "y": y, "geno": geno}


def bound(d, delta, tol, iters):
    kappa = d.kappa(delta)
    return 4.0 * kappa * (tol + 100.0 * iters * kappa * 2.0 ** -52)


@pytest.mark.parametrize("delta", [0.1, 1.0, 10.0])
def test_eval_against_dense_sums(base, delta):
    dev, d, Z, y = base["dev"], base["d"], base["Z"], base["y"]
    T, seed, tol = 15, 77, 1e-10
    sums, iters = dev.reml_eval(y, Z, delta, trials=T, seed=seed, tol=tol, max_iters=500)
    G, E = rr.probes(d, seed, T, np.arange(N0))
    want = rr.eval_sums(d, G, E, y, delta)[0]
    err = float(np.max(np.abs(sums - want) / np.abs(want)))
    b = bound(d, delta, tol, iters)
    print("MEASURED delta = %g: sums vs dense %.3g (bound %.3g), %d iterations, kappa %.3g, f %.9g vs %.9g"
          % (delta, err, b, iters, d.kappa(delta), rr.f_of(sums), rr.f_of(want)))
    assert sums.shape == (T + 1, 3) and err <= b
    assert abs(rr.f_of(sums) - rr.f_of(want)) <= b
    # other probes with another seed, the same y
    other = dev.reml_eval(y, Z, delta, trials=T, seed=seed + 1, tol=tol, max_iters=500)[0]
    assert not np.array_equal(other[:T], sums[:T]) and np.max(np.abs(other[T] - sums[T]) / np.abs(sums[T])) <= b


@pytest.mark.parametrize("T", [1, 15, 31])
def test_driver(base, T):
    dev, d, Z, y = base["dev"], base["d"], base["Z"], base["y"]
    seed, tol, x_tol = 5, 1e-5, 0.01
    G, E = rr.probes(d, seed, T, np.arange(N0))
    dense_f = lambda x: rr.f_of(rr.eval_sums(d, G, E, y, math.exp(x))[0])
    # the condition of the comparison, on the restatement's own run: no step lands within 1e-6 of x_tol
    rx, rf, rst = rr.run_rule(dense_f, x_tol=x_tol)
    assert rst == rr.CONVERGED and np.all(np.abs(np.abs(np.diff(rx)) - x_tol) > 1e-6), rx
    r = dev.reml(y, Z, trials=T, seed=seed, cg_tol=tol, x_tol=x_tol, blup=True)
    k = r["steps"]
    print("T = %d: device x %s, restatement x %s, cg iterations %s, h2 %.4f (SE %.3g, SE_MC %.3g), products %.2f ms, algebra %.2f ms"
          % (T, r["x"], rx, r["cg_iters"], r["h2"], r["se_h2"], r["se_mc"], r["products_ms"], r["algebra_ms"]))
    assert r["status"] == capi.REML_CONVERGED and (r["n"], r["m_used"], r["q"], r["trials"]) == (N0, d.m_used, Q0, T)
    for i in range(k):
        b = bound(d, math.exp(r["x"][i]), tol, int(r["cg_iters"][i]))
        assert abs(r["f"][i] - dense_f(r["x"][i])) <= b, (i, r["f"][i], dense_f(r["x"][i]), b)
        xn, st = capi.reml_next(r["x"][:i], r["f"][:i], x_tol=x_tol)
        assert st == capi.REML_CONTINUE and xn == r["x"][i]
    assert capi.reml_next(r["x"], r["f"], x_tol=x_tol) == (r["x"][-1], capi.REML_CONVERGED)
    # finish on the device's sums is the result
    est = capi.reml_finish(N0, Q0, r["x"][-2:], r["sums_prev"], r["sums_last"], r["ai3"])
    for key, v in est.items():
        assert (math.isnan(v) and math.isnan(r[key])) or v == r[key], key
    assert r["f"][-1] == rr.f_of(r["sums_last"]) and r["f"][-2] == rr.f_of(r["sums_prev"])
    assert math.isnan(r["se_mc"]) == (T == 1) and r["se_h2"] > 0
    # the average-information numbers and the effects against the dense restatement at the device's estimate
    delta = r["delta"]
    b = bound(d, delta, tol, max(int(r["ai_cg_iters"]), int(r["cg_iters"][-1])))
    want = rr.ai_numbers(d, y, delta)
    assert np.max(np.abs(r["ai3"] - want) / np.abs(want)) <= 2.0 * b  # (z comes from a solve whose right-hand side came from a solve)
    v = d.solve(y[None, :], delta)[0]
    beta = d.X.T @ v / d.m_used
    good = np.isfinite(dev.marker_stats()[1])
    assert np.isnan(r["blup"][~good]).all() and not good[3]
    # |X'(v - v^)| / M_used <= |X|_2 |v - v^| / M_used, and |v - v^| <= kappa (tol + drift) |v|
    assert np.linalg.norm(r["blup"][good] - beta[good]) <= np.linalg.norm(d.X, 2) / d.m_used * (b / 4.0) * np.linalg.norm(v)
    want_est = rr.finish(N0, Q0, r["x"][-2:], r["sums_prev"], r["sums_last"], r["ai3"])
    for key, v in want_est.items():
        assert (math.isnan(v) and math.isnan(r[key])) or abs(r[key] - v) <= 1e-12 * abs(v), key


def test_driver_refusals(base):
    dev, Z, y = base["dev"], base["Z"], base["y"]
    for kw, msg in [({"trials": 0}, r"hgibbs_reml: trials = 0, must be in \[1, 31\]"), ({"trials": 32}, r"hgibbs_reml: trials = 32, must be in \[1, 31\]"),
                    ({"h2_start": 1.0}, "hgibbs_reml: h2_start = 1, must lie inside"), ({"cg_tol": 0.0}, "hgibbs_reml: tol = 0, must be positive and finite"),
                    ({"cg_iters": 0}, "hgibbs_reml: max_iters = 0"), ({"x_tol": float("nan")}, "hgibbs_reml: x_tol = nan"),
                    ({"max_steps": 1}, "hgibbs_reml: max_steps = 1"), ({"max_steps": 33}, "hgibbs_reml: max_steps = 33"),
                    ({"cg_iters": 1}, "hgibbs_reml: column [0-9]+ has not converged after max_iters = 1 iterations"),
                    ({"max_steps": 2, "x_tol": 1e-9}, "hgibbs_reml_next: no root after max_steps = 2 evaluations")]:
        trials = kw.pop("trials", 3)
        with pytest.raises(capi.HgError, match=msg):
            dev.reml(y, Z, trials=trials, **kw)
    bad = y.copy()
    bad[9] = np.nan
    with pytest.raises(capi.HgError, match=r"hgibbs_reml: y\[9\] = nan is not finite"):
        dev.reml(bad, Z, trials=3)
    with pytest.raises(capi.HgError, match=r"hgibbs_reml_eval: trials = 32, must be in \[1, 31\]"):
        dev.reml_eval(y, Z, 1.0, trials=32)
    assert dev.reml(y, Z, trials=3)["status"] == capi.REML_CONVERGED


def scale(y):
    """scale_phenotype of the command line: centre, then y'y = N - 1, with sequential sums"""
    n = len(y)
    mean = 0.0
    for v in y:
        mean += float(v)
    mean /= n
    y = np.array([float(v) - mean for v in y])
    s = 0.0
    for v in y:
        s += v * v
    return y * math.sqrt((n - 1) / s)


@pytest.mark.parametrize("ncov", [0, 2])
def test_cli_equals_the_binding(base, tmp_path, ncov):
    geno, y = base["geno"], base["y"]
    na = [7, 150]
    keep = np.ones(N0, dtype=np.uint8)
    keep[na] = 0
    kb = keep.astype(bool)
    prefix = str(tmp_path / "t")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N0, y=y, na_rows=na)
    args = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"), "--mcmc-out-name", "r",
            "--number-individuals", str(N0), "--number-markers", str(M0), "--seed", "9", "--reml", "--reml-blup", "--reml-trials", "7"]
    cov = base["Z"][:, 1:1 + ncov]
    if ncov:
        with open(prefix + ".cov", "w") as f:
            for i in range(N0):
                f.write("fam%d ind%d %s\n" % (i, i, " ".join("%.17g" % v for v in cov[i])))
        args += ["--covariates", prefix + ".cov"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "REML   :" in r.stdout and "products" in r.stdout
    n = int(kb.sum())
    Z = np.column_stack([np.ones(n), cov[kb]])
    yy = scale(y[kb])
    if ncov:
        yy = scale(yy - Z @ np.linalg.solve(Z.T @ Z, Z.T @ yy))
    dev = device(geno, keep=keep)
    res = dev.reml(yy, Z, trials=7, seed=9, blup=True)
    g = lambda v: "%.9g" % v
    want = ["Source\tVariance\tSE", "V(G)\t%s\t%s" % (g(res["vg"]), g(res["se_vg"])), "V(e)\t%s\t%s" % (g(res["ve"]), g(res["se_ve"])),
            "Vp\t%s\t%s" % (g(res["vp"]), g(res["se_vp"])), "V(G)/Vp\t%s\t%s" % (g(res["h2"]), g(res["se_h2"])), "logdelta\t" + g(res["logdelta"]),
            "SE_MC\t" + g(res["se_mc"]), "n\t%d" % n, "M_used\t%d" % res["m_used"], "q\t%d" % (1 + ncov), "trials\t7", "steps\t%d" % res["steps"],
            "cg_iters\t%d" % res["cg_iters"].sum(), "status\tCONVERGED"]
    got = open(str(tmp_path / "o" / "r.reml")).read().split("\n")
    assert got[-1] == "" and got[:-1] == want, (got, want)
    mstd = dev.marker_stats()[1]
    lines = open(str(tmp_path / "o" / "r.reml.blup")).read().split("\n")
    assert lines[0] == "CHR\tSNP\tBP\tA1\tA2\tBETA" and len(lines) == M0 + 2 and lines[-1] == ""
    for j in range(M0):
        beta = "NA" if not np.isfinite(mstd[j]) else g(res["blup"][j] * mstd[j])
        assert lines[1 + j] == "1\tsnp%d\t%d\tA\tC\t%s" % (j, j + 1, beta), j
    assert lines[1 + 3].endswith("\tNA")


def test_planted_signal():
    """N = 2000, M = 4000, h2 = 0.5: the estimate lands within 5 SE_MC of the dense REML root (the root of f with exact traces)"""
    N, M, q = 2000, 4000, 3
    geno = rr.cohort(N, M, miss=0.02, seed=31)
    dev = device(geno)
    mave, mstd = dev.marker_stats()[:2]
    X, good = rr.xmat(geno, mave, mstd)
    Z = rr.covariates(N, q, seed=6)
    y = phenotype(X, 0.5, 32) + Z @ np.array([1.0, -0.5, 0.25])
    d = rr.Dense(X, good, Z)
    xs, fs, st = rr.run_rule(lambda x: rr.f_exact(d, y, math.exp(x)), x_tol=1e-6, max_steps=30)
    assert st == rr.CONVERGED
    h2_root = 1.0 / (1.0 + math.exp(xs[-1]))
    r = dev.reml(y, Z, trials=15, seed=33)
    print("MEASURED planted h2 = 0.5: device h2 %.4f (SE %.3g, SE_MC %.3g, log delta %.4f, %d evaluations, cg %s), dense REML root h2 %.4f (log delta %.4f); "
          "products %.1f ms, algebra %.1f ms" % (r["h2"], r["se_h2"], r["se_mc"], r["logdelta"], r["steps"], r["cg_iters"], h2_root, xs[-1],
                                                 r["products_ms"], r["algebra_ms"]))
    assert r["status"] == capi.REML_CONVERGED and r["se_mc"] > 0
    assert abs(r["h2"] - h2_root) <= 5.0 * r["se_mc"]
    assert abs(r["h2"] - 0.5) <= 5.0 * math.hypot(r["se_h2"], r["se_mc"])
