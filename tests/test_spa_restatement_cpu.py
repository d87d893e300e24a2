"""The saddlepoint approximation of the logistic score test as tests/spa_restate.py restates it, against an
exact enumeration and its own identities; and the float64 / longdouble differences the GPU tests take their tolerances from.  No GPU
needed."""
import math

import numpy as np

import spa_restate as R


def intercept_case(counts, cases, mu):
    a, codes, U, V = R.intercept_only(counts, cases, mu)
    return a, a[codes], np.full(codes.size, mu), U, V


def test_rare_unbalanced_marker_against_the_enumeration():
    counts, mu = (1960, 39, 1), 0.05
    a, ai, m, U, V = intercept_case(counts, (98, 8, 1), mu)
    exact = R.exact_two_sided(counts, a, mu, U)
    r = R.roots(ai, m, U)
    _, _, p, ok = R.pvalue(U, r)
    print("exact %.4g, normal %.4g, saddlepoint %.4g" % (exact, R.normal_p(U, V), p))
    assert ok and r["flags"] == 3
    assert abs(exact - 2.674e-05) < 1e-8
    assert abs(math.log10(p / exact)) < 0.1
    assert math.log10(exact / R.normal_p(U, V)) > 2.5
    # the zero-step trap: the stop rule is tested before the bracket safeguard
    assert max(r["iters"]) <= 10
    # the second case of the same marker: 6 heterozygous cases, no homozygous one
    a, ai, m, U, V = intercept_case(counts, (98, 6, 0), mu)
    exact = R.exact_two_sided(counts, a, mu, U)
    p = R.pvalue(U, R.roots(ai, m, U))[2]
    assert abs(exact - 0.01208) < 1e-5 and abs(p - 0.01071) < 1e-5 and abs(R.normal_p(U, V) - 0.00627) < 1e-5


def test_common_balanced_marker_stays_at_the_normal_p():
    counts, mu = (1000, 800, 200), 0.3
    a, ai, m, U, V = intercept_case(counts, (300, 280, 75), mu)
    assert abs(U / math.sqrt(V) - 2.72) < 0.005
    r = R.roots(ai, m, U)
    _, _, p, ok = R.pvalue(U, r)
    assert ok and abs(p / R.normal_p(U, V) - 1.0) < 0.05
    assert abs(R.exact_two_sided(counts, a, mu, U) - 0.006624) < 1e-6 and abs(p - 0.006478) < 1e-6


def test_cumulant_derivatives_at_zero():
    case = R.roots_case(4099, 3)
    Z, mu = case["Z"], case["mu"]
    w = mu * (1 - mu)
    for j in (0, 20, 40, 63):
        x = case["xv"][j][case["geno"][j]]
        a = R.adjusted(case["geno"][j], case["xv"][j], Z, case["B"][j])
        K, k1, k2 = R.terms(a, mu, 0.0)
        assert K == 0.0 and k1 == 0.0
        t = Z.T @ (w * x)
        V = (w * x) @ x - t @ np.linalg.solve(Z.T @ (Z * w[:, None]), t)  # the projection formula of the score test
        assert abs(k2 - V) <= 1e-10 * V
        assert abs(R.pass0(a, mu)[0] - V) <= 1e-10 * V
        # K' is strictly increasing
        ts = np.linspace(-3.0, 3.0, 13) / math.sqrt(V)
        k1s = [R.terms(a, mu, t)[1] for t in ts]
        assert all(p < q for p, q in zip(k1s, k1s[1:]))


def test_a_score_beyond_the_range_of_the_derivative_is_unreachable():
    case = R.roots_case(261, 1)
    r = R.case_roots(case)[5]
    assert abs(case["s"][5]) > r["s_hi"] > 0.0 > r["s_lo"] > -abs(case["s"][5])
    assert r["flags"] == 12 and r["iters"] == [0, 0] and r["t"] == [0.0, 0.0]
    assert math.isnan(R.pvalue(case["s"][5], r)[2]) and not R.pvalue(case["s"][5], r)[3]
    # one tail only: a score between the two ends
    a = R.adjusted(case["geno"][5], case["xv"][5], case["Z"], case["B"][5])
    ends = sorted([r["s_hi"], -r["s_lo"]])
    if ends[0] < ends[1]:
        one = R.roots(a, case["mu"], 0.5 * (ends[0] + ends[1]))
        assert one["flags"] & 12 == (4 if r["s_hi"] < -r["s_lo"] else 8)


def test_float64_against_longdouble_on_the_gpu_tests_markers():
    """prints what the tolerances of tests/test_gpu_spa_roots.py are ten times of"""
    worst = dict(t=0.0, K=0.0, K2=0.0, p=0.0)
    for n in R.GRID_N:
        for q in R.GRID_Q:
            case = R.roots_case(n, q)
            r64, r80 = R.case_roots(case), R.case_roots(case, np.longdouble)
            for j, (a, b) in enumerate(zip(r64, r80)):
                assert a["flags"] == b["flags"], (n, q, j)
                for z in range(2):
                    if a["flags"] >> z & 1:
                        for k in ("t", "K", "K2"):
                            worst[k] = max(worst[k], R.rel(a[k][z], b[k][z]))
                pa, pb = R.pvalue(case["s"][j], a), R.pvalue(case["s"][j], b)
                assert pa[3] == pb[3]
                if pa[3]:
                    worst["p"] = max(worst["p"], R.rel(pa[2], pb[2]))
            assert max(max(r["iters"]) for r in r64) <= R.PASSES
    print("largest relative difference float64 / longdouble: t %.3g, K %.3g, K2 %.3g, p %.3g" % (worst["t"], worst["K"], worst["K2"], worst["p"]))
    assert worst["t"] < 1e-9 and worst["p"] < 1e-9
