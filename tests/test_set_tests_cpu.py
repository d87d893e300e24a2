"""hgibbs_set_tests (host only) through the built library against the restatement of tests/settest_restate.py: burden and SKAT on a
grid of spectra from 1 to 200 eigenvalues and Q from below the mean to 20 sigma above it, the switch to the limit on both sides, a
rank-deficient, a zero and a burden-degenerate covariance; equal eigenvalues against the closed-form chi-square tail.  No GPU."""
import math

import numpy as np
import pytest

from hydra_amd import capi

import settest_restate as S

# Two converged roots of the same equation lie within the stop rule's 1e-9 of each other (relative to max(|z|, 1 / sqrt K''(0))), the
# exponent z Q - K is stationary there and the prefactor z sqrt(K'') is linear in z; the eigenvalues of Jacobi and of LAPACK agree
# to a few m 2^-52 lam_max, which the tail at 20 sigma (d log p / d log lam up to Q / (2 lam_max) < 1e3) turns into < 1e-10.
TOL_P = 1e-8
TOL_SUM = 1e-12  # q, t_burden, lam_sum, lam_max: sums of at most 200 terms and eigenvalues of a matrix of norm lam_max


def close(got, want, tol):
    return abs(got - float(want)) <= tol * abs(float(want))


def compare(U, Phi, a, p_abs=0.0):
    """p_abs: an absolute allowance for p_skat, for the points next to the switch, where the formula's rounding is amplified"""
    got = capi.set_tests(U, Phi, a)
    want = S.set_tests(U, Phi, a)
    assert got.neig == want["neig"]
    for name, tol in (("q", TOL_SUM), ("lam_sum", TOL_SUM), ("lam_max", TOL_SUM), ("t_burden", TOL_SUM), ("p_burden", TOL_P), ("p_skat", TOL_P)):
        g, w = getattr(got, name), float(want[name])
        if math.isnan(w):
            assert math.isnan(g), (name, g)
        else:
            assert close(g, w, tol) or (name == "p_skat" and abs(g - w) <= p_abs), (name, g, w)
    assert got.skat_ok == want["skat_ok"]
    return got


GRID = [(name, sig) for name in sorted(S.spectra()) for sig in S.SIGMAS]


@pytest.mark.parametrize("name,sig", GRID)
def test_grid_against_the_restatement(name, sig):
    lam = S.spectra()[name]
    Q = S.q_at(lam, sig)
    assert Q > 0  # (mean / sigma >= 1 / sqrt 2 for any spectrum: half a sigma below the mean is still positive)
    m = lam.size
    a = 0.5 + np.arange(m) % 3  # weights that are not flat
    Phi = S.matrix_with_spectrum(lam, seed=m) / (a[:, None] * a[None, :])  # diag(a) Phi diag(a) has the spectrum
    U = S.scores_for(m, Q) / a
    got = compare(U, Phi, a)
    assert got.neig == m and got.skat_ok == 1
    assert close(got.q, Q, 1e-12)


@pytest.mark.parametrize("name", sorted(S.spectra()))
@pytest.mark.parametrize("side", [-1.0, 1.0])
def test_switch_to_the_limit(name, side):
    lam = S.spectra()[name]
    m = lam.size
    Phi = S.matrix_with_spectrum(lam, seed=m)
    sd = math.sqrt(2.0 * float(np.sum(lam * lam)))
    inside = compare(S.scores_for(m, float(np.sum(lam)) + side * 0.5e-6 * sd), Phi, np.ones(m))
    # outside, the library's and the restatement's evaluation of the formula each carry its rounding error there (switch_bound's second
    # term, which is all but the whole of it): they may lie twice that apart
    outside = compare(S.scores_for(m, float(np.sum(lam)) + side * 2e-6 * sd), Phi, np.ones(m), p_abs=2.0 * S.switch_bound(lam))
    assert inside.skat_ok == 1 and outside.skat_ok == 1
    assert abs(inside.p_skat - outside.p_skat) < S.switch_bound(lam)


def equal_bound():
    """1.5 times the restatement's own worst relative difference from the closed form on this grid"""
    worst = 0.0
    for df in S.EQUAL_DF:
        for sig in S.SIGMAS:
            Q = S.q_at(np.ones(df), sig)
            if Q > 0:
                p, _ = S.skat_tail(np.full(df, 0.7), 0.7 * Q)
                worst = max(worst, abs(p / S.chi2_tail(Q, df) - 1.0))
    return 1.5 * worst


@pytest.mark.parametrize("df", S.EQUAL_DF)
def test_equal_eigenvalues_against_the_chi_square_tail(df):
    bound = equal_bound()
    assert 0.05 < bound < 0.2  # section 28: near 11 % times 1.5
    for sig in S.SIGMAS:
        Q = S.q_at(np.ones(df), sig)
        if Q <= 0:
            continue
        r = capi.set_tests(S.scores_for(df, 0.7 * Q), 0.7 * np.eye(df), np.ones(df))
        assert r.neig == df and r.skat_ok == 1
        exact = S.chi2_tail(Q, df)
        assert abs(r.p_skat / exact - 1.0) <= bound, (df, sig, r.p_skat, exact)


def test_rank_deficient_duplicated_column():
    rng = np.random.default_rng(4)
    X = rng.standard_normal((50, 6))
    X[:, 5] = X[:, 2]  # a duplicated marker
    Phi = X.T @ X
    U = X.T @ rng.standard_normal(50)
    got = compare(U, Phi, np.ones(6))
    assert got.neig == 5 and got.skat_ok == 1 and math.isfinite(got.t_burden)


def test_zero_covariance_everything_nan():
    r = capi.set_tests([1.0, 2.0, 3.0], np.zeros((3, 3)), np.ones(3))
    assert r.neig == 0 and r.skat_ok == 0
    assert all(math.isnan(getattr(r, k)) for k in ("q", "p_skat", "t_burden", "p_burden", "lam_sum", "lam_max"))


def test_zero_burden_denominator():
    got = compare([1.0, -1.0], np.array([[1.0, -1.0], [-1.0, 1.0]]), [1.0, 1.0])
    assert math.isnan(got.t_burden) and math.isnan(got.p_burden) and got.neig == 1 and got.skat_ok == 1


def test_single_marker_burden_is_the_score_test():
    r = capi.set_tests([3.0], [[4.0]], [0.37])
    assert close(r.t_burden, 9.0 / 4.0, 1e-15) and close(r.p_burden, math.erfc(math.sqrt(9.0 / 8.0)), 1e-15)
    assert r.neig == 1 and close(r.lam_max, 0.37 * 0.37 * 4.0, 1e-15)


def test_bit_reproducible():
    lam = S.spectra()["forty_decay"]
    Phi = S.matrix_with_spectrum(lam, seed=1)
    U = S.scores_for(40, S.q_at(lam, 4.0))
    assert bytes(capi.set_tests(U, Phi, np.ones(40))) == bytes(capi.set_tests(U, Phi, np.ones(40)))


def test_refusals():
    with pytest.raises(capi.HgError, match="hgibbs_set_tests: m = 0"):
        capi.set_tests(np.zeros(0), np.zeros((0, 0)), np.zeros(0))
    with pytest.raises(capi.HgError, match=r"hgibbs_set_tests: Phi\[0\]\[1\] = nan is not finite"):
        capi.set_tests([1.0, 1.0], [[1.0, np.nan], [0.0, 1.0]], [1.0, 1.0])
    with pytest.raises(capi.HgError, match="hgibbs_set_tests: U"):
        capi.set_tests([np.inf], [[1.0]], [1.0])
