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


def gaps(cases, worst):
    """the largest float64 / longdouble relative differences over the entries of `cases`, into worst; the flags agree"""
    for case in cases:
        for e in range(R.case_size(case)):
            a, b = (R.roots(R.case_a(case, e, dt), np.asarray(case["mu"], dt), case["s"][e], dt) for dt in (np.float64, np.longdouble))
            assert a["flags"] == b["flags"], (case["n"], e)
            for k in ("k2_0", "s_lo", "s_hi"):
                worst[k] = max(worst[k], R.rel(a[k], b[k]))
            for z in range(2):
                if a["flags"] >> z & 1:
                    for k in ("t", "K", "K2"):
                        worst[k] = max(worst[k], R.rel(a[k][z], b[k][z]))
            pa, pb = R.pvalue(case["s"][e], a), R.pvalue(case["s"][e], b)
            assert pa[3] == pb[3], (case["n"], e)
            if pa[3]:
                worst["p"] = max(worst["p"], R.rel(pa[2], pb[2]))
    return worst


def report(what, worst):
    print("%s, largest relative difference float64 / longdouble: %s" % (what, ", ".join("%s %.3g" % kv for kv in worst.items())))


def case_traces(cases, dtype=np.float64):
    return [R.traced(R.roots, R.case_a(case, e, dtype), case["mu"], case["s"][e], dtype) + (case, e) for case in cases for e in range(R.case_size(case))]


def test_rule_cases_admitted_entries_are_well_conditioned():
    """Every admitted entry of rule_cases() passes admission(): the GPU test may hold the device to the float64 rule's flags and passes
    there.  Prints the coverage table and what the tolerances of test_admitted_entries_against_the_restatement are ten times of."""
    admitted, ill = R.rule_cases()
    for case in admitted:
        for e in range(R.case_size(case)):
            assert R.admission(R.roots, R.case_a(case, e), case["mu"], case["s"][e]) is None, (case["n"], e)
    here, there = case_traces(admitted), case_traces(ill)
    print("branch: tails of admitted entries, tails of ill-conditioned entries (float64)")
    count = {}
    for letter in "NSCMDO":
        count[letter] = [sum(letter in t for _, tr, _, _ in which for t in tr) for which in (here, there)]
        print("  %s: %d, %d" % (letter, *count[letter]))
    # 2 t needs a proposal outside a bracket with an infinite end.  From inside (0, inf) the sign of K' - tau moves the finite end to t and a
    # Newton step with K'' > 0 goes towards the other, so it stays inside unless it is not a number or not finite: K'' = 0 to the last
    # place, every row saturated, and K' - tau <= 0 there -- a score within rounding of the reachable edge.  Ill-conditioned input only.
    assert all(count[letter][0] > 0 for letter in "NSCM") and count["D"] == [0, count["D"][1]] and count["D"][1] > 0, count
    assert count["O"][0] == 0 and count["O"][1] > 0  # an open tail in float64: neither bit set, iters == PASSES
    opened = [(r, z) for r, tr, _, _ in there for z in range(2) if R.OPEN in tr[z]]
    assert all(r["iters"][z] == R.PASSES and not r["flags"] >> z & 5 and r["K"][z] == r["K2"][z] == 0 for r, z in opened)
    for which in (admitted, ill):  # the shapes and the inputs the two lists are meant to span
        assert {case["n"] for case in which} == set(R.RULE_N)
        assert any((case["geno"] == 3).any() for case in which) and any((case["geno"] != 3).all() for case in which)
        assert any(case["mu"].min() == 1e-12 and case["mu"].max() == 1 - 1e-12 for case in which)
        assert any(np.ptp(case["mu"]) == 0 for case in which)
    assert {r["flags"] for r, _, _, _ in here} >= {3, 1 | 8, 2 | 4}  # both tails, and one reachable tail of either side
    report("admitted entries", gaps(admitted, dict(t=0.0, K=0.0, K2=0.0, p=0.0, k2_0=0.0, s_lo=0.0, s_hi=0.0)))


def test_rule_cases_saturating_entries_saturate():
    """the five entries before the open ones of ILL: at the first point t = tau / K''(0) every row with a != 0 has p (1 - p) < 1e-7"""
    k = 0
    for spec in R.ILL:
        if spec[4] != 300.0:
            continue
        k += 1
        e = R.rule_entry(*spec)
        a = e["xv"][e["geno"]]
        k2_0, _, _ = R.pass0(a, e["mu"])
        u = a[a != 0] * (abs(e["s"]) / k2_0)
        p = e["mu"][a != 0] / (e["mu"][a != 0] + (1 - e["mu"][a != 0]) * np.exp(-u))
        assert np.all(p * (1 - p) < 1e-7), spec
    assert k == 5


def test_float64_against_longdouble_on_the_edges_of_q_and_n():
    """The existing tolerances of tests/test_gpu_spa_roots.py (t 2.7e-12, K 4.0e-11, K'' 2.5e-12, p 1.2e-10; 1e-12 on the sums of pass 0) hold
    for test_edges_of_q_and_n there if the gap measured here stays under a tenth of them."""
    worst = gaps([R.edge_case(n, q) for n, q in R.EDGE_SHAPES], dict(t=0.0, K=0.0, K2=0.0, p=0.0, k2_0=0.0, s_lo=0.0, s_hi=0.0))
    report("edges of q and n", worst)
    for k, tol in dict(t=2.7e-12, K=4.0e-11, K2=2.5e-12, p=1.2e-10, k2_0=1e-12, s_lo=1e-12, s_hi=1e-12).items():
        assert worst[k] < tol / 10, (k, worst[k])


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
