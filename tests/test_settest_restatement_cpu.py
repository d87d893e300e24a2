"""The restatement of tests/settest_restate.py against a case typed out by hand and against itself in longdouble: the raw sums of
hgibbs_set_gram as integers, out, the statistics of hgibbs_set_tests; and the tolerance of out that tests/test_gpu_set_gram.py asserts,
measured on that test's own grid.  No library, no GPU."""
import math

import numpy as np
import pytest

import settest_restate as S

# 3 markers, 8 rows, one missing call (marker 1, row 5); integer weights, so every sum below is exact
GENO = np.array([[0, 1, 2, 0, 1, 0, 0, 2],
                 [1, 0, 0, 2, 1, 3, 0, 1],
                 [0, 0, 1, 1, 0, 2, 0, 0]], dtype=np.uint8)
W = np.array([1, 2, 3, 4, 5, 6, 7, 8], dtype=np.float64)
# by hand: GG_ab = sum w g_a g_b (g = 0 at the missing call), GC_ab = sum w g_a c_b, CC_ab = sum w c_a c_b
GG_HAND = [[2 + 12 + 5 + 32, 5 + 16, 6], [5 + 16, 1 + 16 + 5 + 8, 8], [6, 8, 3 + 4 + 24]]
GC_HAND = [[2 + 6 + 5 + 16, 2 + 6 + 5 + 16, 2 + 6 + 5 + 16], [1 + 8 + 5 + 8, 1 + 8 + 5 + 8, 1 + 8 + 5 + 8], [3 + 4 + 12, 3 + 4, 3 + 4 + 12]]
CC_HAND = [[36, 30, 36], [30, 30, 30], [36, 30, 36]]


def test_hand_case_raw_sums():
    E, GG, GC, CC = S.raw_integers(GENO, [0, 1, 2], W)
    assert E == 52 - 4  # max w = 8 < 2^4
    for got, want in ((GG, GG_HAND), (GC, GC_HAND), (CC, CC_HAND)):
        assert [[int(x) for x in row] for row in got] == [[v << E for v in row] for row in want]
    raw = S.raw_floats(GENO, [2, 0], W)  # any order, any subset
    assert raw[:, :, 0].tolist() == [[31.0, 6.0], [6.0, 51.0]]
    assert raw[:, :, 1].tolist() == [[19.0, 19.0], [29.0, 29.0]]


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_hand_case_out_is_the_weighted_gram_of_the_standardised_columns(dtype):
    av, sd = S.marker_stats(GENO, dtype)
    assert float(av[1]) == pytest.approx(5.0 / 7.0) and float(av[0]) == 0.75
    # marker 0: n0 = 4, n1 = 2, n2 = 2 -> sum of squares 4 (.75)^2 + 2 (.25)^2 + 2 (1.25)^2 = 5.5
    assert float(sd[0]) == pytest.approx(math.sqrt(7.0 / 5.5))
    out, scale = S.gram_out(S.raw_floats(GENO, [0, 1, 2], W), av, sd, dtype)
    direct = S.gram_direct(GENO, [0, 1, 2], W, dtype)
    assert np.max(np.abs(out - direct) / scale) < 8 * np.finfo(dtype).eps
    assert np.array_equal(out, out.T)


def test_monomorphic_and_all_missing_columns_give_nan_out_and_exact_raw():
    case = S.grid_case(64, True)
    av, sd = S.marker_stats(case["geno"])
    assert not np.isfinite(sd[S.MONO]) and not np.isfinite(sd[S.ALLMISS])
    idx = case["sets"][4]
    out, _ = S.gram_out(S.raw_floats(case["geno"], idx, case["w"]), av[idx], sd[idx])
    assert np.all(np.isnan(out[:2])) and np.all(np.isnan(out[:, :2])) and np.all(np.isfinite(out[2:, 2:]))


def test_rounding_bound_of_w():
    case = S.grid_case(1000, True)
    w = 10.0 ** np.random.default_rng(3).uniform(-12, 0, 1000)
    idx = case["sets"][3]
    E, GG, GC, CC = S.raw_integers(case["geno"], idx, w)
    codes = case["geno"][idx]
    c = (codes != 3).astype(np.longdouble)
    g = np.where(codes == 3, 0, codes).astype(np.longdouble)
    wl = w.astype(np.longdouble)
    bound = S.rounding_bound(1000, E)
    for k, (ints, want) in enumerate(((GG, (g * wl) @ g.T), (GC, (g * wl) @ c.T), (CC, (c * wl) @ c.T))):
        got = np.array([[np.longdouble(int(x)) for x in row] for row in ints]) * np.longdouble(2.0) ** -E
        assert np.max(np.abs(got - want)) <= bound[k] + 1000 * 4 * float(np.finfo(np.longdouble).eps)


def test_out_tolerance_measured_on_the_gpu_grid(capsys):
    """what tests/test_gpu_set_gram.py asserts ten times of: printed, and pinned here so that it cannot drift unnoticed"""
    cases = [S.grid_case(n, miss) for n in S.GRID_N for miss in (False, True)] + [S.big_case(True)]
    worst = S.measure_out_tolerance(cases)
    with capsys.disabled():
        print("\nout: largest |float64 - longdouble| / sum |terms| over the grid: %.3g" % worst)
    assert 0.0 < worst <= S.OUT_F64_LD


@pytest.mark.parametrize("name", sorted(S.spectra()))
def test_statistics_float64_against_longdouble(name):
    lam = S.spectra()[name]
    for sig in S.SIGMAS:
        Q = S.q_at(lam, sig)
        if Q <= 0:
            continue
        p64, ok64 = S.skat_tail(lam, Q, np.float64)
        pl, okl = S.skat_tail(lam, Q, np.longdouble)
        assert ok64 and okl, (name, sig)
        assert abs(p64 - float(pl)) <= 1e-8 * float(pl), (name, sig, p64, pl)
        assert 0.0 < p64 < 1.0


def test_limit_meets_the_formula_at_the_switch():
    for name, lam in S.spectra().items():
        sd = math.sqrt(2.0 * float(np.sum(lam * lam)))
        mean = float(np.sum(lam))
        for side in (-1.0, 1.0):
            inside, _ = S.skat_tail(lam, mean + side * 0.5e-6 * sd)
            outside, ok = S.skat_tail(lam, mean + side * 2e-6 * sd)
            assert ok and abs(inside - outside) < S.switch_bound(lam), (name, side, inside, outside)


def test_equal_eigenvalues_against_the_chi_square_tail(capsys):
    lo, hi = 0.0, 0.0
    for df in S.EQUAL_DF:
        for sig in S.SIGMAS:
            Q = S.q_at(np.ones(df), sig)
            if Q <= 0:
                continue
            p, ok = S.skat_tail(np.full(df, 0.7), 0.7 * Q)
            assert ok
            rel = p / S.chi2_tail(Q, df) - 1.0
            lo, hi = min(lo, rel), max(hi, rel)
    with capsys.disabled():
        print("\nsaddlepoint against the exact chi-square tail, equal eigenvalues: %+.2f %% .. %+.2f %%" % (100 * lo, 100 * hi))
    assert -0.12 < lo and hi < 0.12  # section 28 claims -4.9 % .. +10.6 %


def test_burden_and_weights():
    a = S.beta_weights([0.01, 0.2, 0.5], 1.0, 1.0)
    assert np.allclose(a, 1.0)
    a = S.beta_weights([0.01], 1.0, 25.0)
    assert a[0] == pytest.approx(25.0 * 0.99 ** 24)
    Phi = np.array([[2.0, 0.5], [0.5, 1.0]])
    r = S.set_tests([1.0, -2.0], Phi, [1.0, 1.0])
    assert float(r["t_burden"]) == pytest.approx(1.0 / 4.0) and float(r["q"]) == pytest.approx(5.0) and r["neig"] == 2
    r = S.set_tests([1.0, -1.0], np.array([[1.0, -1.0], [-1.0, 1.0]]), [1.0, 1.0])  # a'Phi a = 0
    assert math.isnan(float(r["t_burden"])) and r["neig"] == 1
    r = S.set_tests([1.0, 2.0], np.zeros((2, 2)), [1.0, 1.0])
    assert r["neig"] == 0 and all(math.isnan(float(r[k])) for k in ("q", "p_skat", "t_burden", "p_burden", "lam_sum", "lam_max"))
