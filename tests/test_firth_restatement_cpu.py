"""Firth's penalised fit of the logistic score test's one-parameter model as tests/firth_restate.py restates it:
the rule converges on every entry of the GPU tests' grid, the point it finds is a stationary point and a local maximum of the penalised
likelihood in longdouble, the near-separated marker gets a finite effect, hgibbs_firth_stats' validity rules, and the float64 /
longdouble differences the GPU tests take their tolerances from.  No GPU needed."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from hydra_amd import capi

import firth_restate as F
import spa_restate as R

GRID = [(n, q) for n in F.GRID_N for q in F.GRID_Q]


@functools.lru_cache(maxsize=None)
def grid_case(n, q):
    case = F.fit_case(n, q)
    return case, F.case_fits(case)


@pytest.mark.parametrize("n,q", GRID)
def test_the_rule_converges_on_every_entry_of_the_grid(n, q):
    case, fits = grid_case(n, q)
    assert len(fits) == F.GRID_M + 1
    for e, r in enumerate(fits):
        if e == F.FLAT:
            assert r["flags"] == F.DEGENERATE and all(r[k] == 0 for k in ("beta", "K", "K2", "g", "k2_0", "iters")), r
            continue
        assert r["flags"] == F.CONVERGED and 1 <= r["iters"] <= F.PASSES, (e, r)
        assert F.stats(case["s"][e], r)[3], (e, r)
    print("n %d q %d: at most %d passes" % (n, q, max(r["iters"] for r in fits)))


@pytest.mark.parametrize("n,q", GRID)
def test_the_point_is_stationary_and_a_local_maximum_in_longdouble(n, q):
    case, fits = grid_case(n, q)
    for e, r in enumerate(fits[:F.GRID_M]):
        a, s = F.entry_a(case, e, np.longdouble), case["s"][e]
        scale = 1.0 / math.sqrt(r["k2_0"])
        top, g = F.penalised(a, case["mu"], s, r["beta"])
        assert abs(g) <= 1e-6 * math.sqrt(r["k2_0"]), (e, float(g))
        for step in (-1e-3 * scale, 1e-3 * scale):
            assert top >= F.penalised(a, case["mu"], s, r["beta"] + step)[0], (e, step)


@pytest.mark.parametrize("n,q", GRID)
def test_the_near_separated_marker_gets_a_finite_effect(n, q):
    case, fits = grid_case(n, q)
    e = F.NEAR_SEPARATED
    carriers = case["geno"][e] == 1
    assert carriers.sum() == min(6, int(case["d"].sum())) and np.all(case["d"][carriers] == 1.0) and np.all(case["geno"][e][~carriers] == 0)
    r = fits[e]
    lrt, se, p, ok = F.stats(case["s"][e], r)
    chisq = case["s"][e] ** 2 / r["k2_0"]
    print("n %d q %d: beta %.4g se %.4g, penalised likelihood ratio %.4g against the score statistic %.4g" % (n, q, r["beta"], se, lrt, chisq))
    assert ok and np.isfinite(r["beta"]) and r["beta"] > 0.0 and case["s"][e] > 0.0
    assert lrt < chisq


def test_a_zero_score_leaves_the_penalty_s_own_effect():
    """g(0) = s + K'''(0) / (2 K''(0)): with s = 0 the fit does not stay at 0, it moves where the penalty's slope points"""
    for n, q in GRID:
        case, fits = grid_case(n, q)
        e = F.ZERO_SCORE
        a = F.entry_a(case, e)
        k3 = F.sums(a, case["mu"], 0.0)[3]
        r = fits[e]
        assert case["s"][e] == 0.0 and r["flags"] == F.CONVERGED
        assert r["beta"] != 0.0 and (r["beta"] > 0) == (k3 > 0)


def rec(beta=0.5, K=1.0, K2=4.0, k2_0=5.0, flags=1, iters=3):
    return dict(beta=np.float64(beta), K=np.float64(K), K2=np.float64(K2), g=np.float64(0), k2_0=np.float64(k2_0), iters=iters, flags=flags)


def both(s, r):
    """the restatement's and the library's statistics of the same record, compared; returns the library's"""
    want = F.stats(s, r)
    got = capi.firth_stats(s, capi.FirthRec(float(r["beta"]), float(r["K"]), float(r["K2"]), float(r["g"]), float(r["k2_0"]), r["iters"], r["flags"]))
    assert got[3] == want[3]
    for a, b in zip(got[:3], want[:3]):
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-14 * abs(b), (got, want)
    return got


def test_stats_validity_rules():
    s = 6.0
    lrt, se, p, ok = both(s, rec())
    assert ok and abs(lrt - 2 * (0.5 * s - 1.0 + 0.5 * math.log(0.8))) < 1e-14 and se == 0.5 and abs(p - math.erfc(math.sqrt(lrt / 2))) < 1e-16
    invalid = [rec(flags=0), rec(flags=2), rec(flags=3), rec(K2=0.0), rec(K2=-1.0), rec(K2=math.nan), rec(K=4.0), rec(k2_0=0.0), rec(beta=math.inf),
               rec(K=math.nan)]
    for r in invalid:
        got = both(s, r)
        assert not got[3] and all(math.isnan(v) for v in got[:3]), (r, got)
    # the clamp: a ratio that rounding left just below 0 is 0; one further below is not
    r = rec(beta=0.0, K=2e-10, K2=5.0)
    assert both(s, r) == (0.0, 1.0 / math.sqrt(5.0), 1.0, True)
    assert not both(s, rec(beta=0.0, K=1e-8, K2=5.0))[3]


def test_stats_null_arguments():
    L = capi.lib()
    r = capi.FirthRec(0.5, 1.0, 4.0, 0.0, 5.0, 3, 1)
    p, ok = C.c_double(), C.c_int()
    assert L.hgibbs_firth_stats(6.0, C.byref(r), None, None, C.byref(p), None) == 0 and 0.0 < p.value < 1.0
    assert L.hgibbs_firth_stats(6.0, None, None, None, C.byref(p), C.byref(ok)) != 0
    assert "hgibbs_firth_stats: null argument" in L.hgibbs_last_error().decode()
    assert L.hgibbs_firth_stats(6.0, C.byref(r), None, None, None, C.byref(ok)) != 0
    assert "hgibbs_firth_stats: null argument" in L.hgibbs_last_error().decode()


def gaps(cases):
    """the largest float64 / longdouble relative differences over the entries of `cases`; the flags agree"""
    worst = dict(beta=0.0, K=0.0, K2=0.0, p=0.0, k2_0=0.0)
    for case in cases:
        for e in range(R.case_size(case)):
            a, b = (F.fit(R.case_a(case, e, dt), np.asarray(case["mu"], dt), case["s"][e], dt) for dt in (np.float64, np.longdouble))
            assert a["flags"] == b["flags"] == F.CONVERGED, (case["n"], e)
            for k in ("beta", "K", "K2", "k2_0"):
                worst[k] = max(worst[k], F.rel(a[k], b[k]))
            sa, sb = F.stats(case["s"][e], a), F.stats(case["s"][e], b)
            assert sa[3] and sb[3], (case["n"], e)
            worst["p"] = max(worst["p"], F.rel(sa[2], sb[2]))
    return worst


def report(what, worst):
    print("%s, largest relative difference float64 / longdouble: %s" % (what, ", ".join("%s %.3g" % kv for kv in worst.items())))


def case_traces(cases, dtype=np.float64):
    return [R.traced(F.fit, R.case_a(case, e, dtype), case["mu"], case["s"][e], dtype) + (case, e) for case in cases for e in range(R.case_size(case))]


def test_rule_cases_admitted_entries_are_well_conditioned():
    """Every admitted entry of rule_cases() passes spa_restate.admission(): the GPU test may hold the device to the float64 rule's flags
    and passes there.  Prints the coverage table and what the tolerances of test_admitted_entries_against_the_restatement are ten times
    of.  Every branch of the rule is taken by an admitted entry; only the open entry needs ill-conditioned input."""
    admitted, ill = F.rule_cases()
    for case in admitted:
        for e in range(R.case_size(case)):
            assert R.admission(F.fit, R.case_a(case, e), case["mu"], case["s"][e]) is None, (case["n"], e)
    here, there = case_traces(admitted), case_traces(ill)
    print("branch: admitted entries, ill-conditioned entries (float64)")
    count = {}
    for letter in "NSCMDFXO":
        count[letter] = [sum(letter in tr[0] for _, tr, _, _ in which) for which in (here, there)]
        print("  %s: %d, %d" % (letter, *count[letter]))
    assert all(count[letter][0] > 0 for letter in "NSCMDFX"), count
    assert count["O"][0] == 0 and count["O"][1] > 0  # an open entry in float64: no flag, iters == PASSES
    assert all(r["iters"] == F.PASSES and r["flags"] == 0 and r["K"] == r["K2"] == 0 for r, tr, _, _ in there if R.OPEN in tr[0])
    for which in (admitted, ill):  # the shapes and the inputs the two lists are meant to span
        assert {case["n"] for case in which} == set(R.RULE_N)
        assert any((case["geno"] == 3).any() for case in which) and any((case["geno"] != 3).all() for case in which)
        assert any(case["mu"].min() == 1e-12 and case["mu"].max() == 1 - 1e-12 for case in which)
        assert any(np.ptp(case["mu"]) == 0 for case in which)
    for r, _, case, e in here:  # what the rule calls converged is a stationary point and a local maximum
        assert F.stationary(R.case_a(case, e, np.longdouble), case["mu"], case["s"][e], r), (case["n"], e)
    report("admitted entries", gaps(admitted))


def test_rule_cases_the_rule_does_not_stop_next_to_a_minimum():
    """NEAR_MINIMUM: g'(0) > 0 and a proposal within 1e-9 scale of 0, on the wrong side of the bracket end that g's sign has just set
    there.  The rule takes +-scale with g's sign and ends at the local maximum on that side, a fit of the order of scale."""
    for spec in F.NEAR_MINIMUM:
        e = F.near_minimum_entry(*spec)
        a = e["xv"][e["geno"]]
        for dtype in (np.float64, np.longdouble):
            _, k1, k2, k3, k4 = F.sums(np.asarray(a, dtype), np.asarray(e["mu"], dtype), dtype(0), dtype)
            g, gp = F.score(e["s"], k1, k2, k3, k4, dtype)
            assert gp > 0 and g != 0 and abs(g / gp) < 0.5 * F.STOP / np.sqrt(k2), spec
        r, tr = R.traced(F.fit, a, e["mu"], e["s"])
        assert tr[0][0] == R.FIRST_STEP and r["flags"] == F.CONVERGED and (r["beta"] > 0) == (g > 0), (spec, tr)
        assert abs(r["beta"]) > 0.1 / math.sqrt(r["k2_0"]), (spec, r["beta"])
        assert F.stationary(np.asarray(a, np.longdouble), e["mu"], e["s"], r) and F.stats(e["s"], r)[3], spec


def test_rule_cases_saturating_entries_saturate():
    """the five entries before the open ones of ILL: at the point of the first Newton step every row with a != 0 has p (1 - p) < 1e-7"""
    k = 0
    for spec in F.ILL:
        if spec[4] != 300.0:
            continue
        k += 1
        e = R.rule_entry(*spec)
        a, mu = e["xv"][e["geno"]], e["mu"]
        _, k1, k2, k3, k4 = F.sums(a, mu, 0.0)
        g, gp = F.score(e["s"], k1, k2, k3, k4)
        u = a[a != 0] * (-g / gp)
        with np.errstate(over="ignore"):
            p = mu[a != 0] / (mu[a != 0] + (1 - mu[a != 0]) * np.exp(-u))
        assert np.all(p * (1 - p) < 1e-7), spec
    assert k == 5


def test_float64_against_longdouble_on_the_edges_of_q_and_n():
    """The existing tolerances of tests/test_gpu_firth.py (beta 8.3e-12, K 9.9e-12, K'' 1.9e-11, p 8.6e-13; 1e-12 on K''(0)) hold for
    test_edges_of_q_and_n there if the gap measured here stays under a tenth of them."""
    worst = gaps([R.edge_case(n, q) for n, q in R.EDGE_SHAPES])
    report("edges of q and n", worst)
    for k, tol in dict(beta=8.3e-12, K=9.9e-12, K2=1.9e-11, p=8.6e-13, k2_0=1e-12).items():
        assert worst[k] < tol / 10, (k, worst[k])


def test_float64_against_longdouble_on_the_gpu_tests_entries():
    """prints what the tolerances of tests/test_gpu_firth.py are ten times of"""
    worst = dict(beta=0.0, K=0.0, K2=0.0, p=0.0)
    for n, q in GRID:
        case, r64 = grid_case(n, q)
        r80 = F.case_fits(case, np.longdouble)
        for e, (a, b) in enumerate(zip(r64, r80)):
            assert a["flags"] == b["flags"], (n, q, e)
            if not a["flags"] & F.CONVERGED:
                continue
            for k in ("beta", "K", "K2"):
                worst[k] = max(worst[k], F.rel(a[k], b[k]))
            sa, sb = F.stats(case["s"][e], a), F.stats(case["s"][e], b)
            assert sa[3] and sb[3]
            worst["p"] = max(worst["p"], F.rel(sa[2], sb[2]))
    print("largest relative difference float64 / longdouble: beta %.3g, K %.3g, K2 %.3g, p %.3g" % (worst["beta"], worst["K"], worst["K2"], worst["p"]))
    assert worst["beta"] < 1e-9 and worst["p"] < 1e-9
