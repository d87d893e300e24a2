"""The references of tests/test_gpu_operators.py, checked without a GPU: the Python BetaLogDensity through the product's host ARS on
the seven draw cases (with the stability condition of the draw's tolerance), the fsum references at one small N against exact
rational arithmetic and a dense restatement, and the finiteness condition of the BayesW sums."""
import math
from fractions import Fraction

import numpy as np
import pytest

import test_gpu_operators as T
from hydra_amd import synth


@pytest.mark.parametrize("name,seed", T.ARS_CASES)
def test_host_draws_are_steady_under_a_few_ulps(name, seed):
    d, b, sl = T.ARS_SETS[name]
    err, evals, last = T.host_ars(d, b, sl, seed, T.ARS_NDRAWS)
    assert err == 0 and evals >= 9 * T.ARS_NDRAWS // 2 and b - sl < last < b + sl
    assert T.host_ars(d, b, sl, seed, T.ARS_NDRAWS) == (err, evals, last)  # (the generator is the caller's: a repeat is a repeat)
    counts, worst = T.ars_sensitivity(name, seed)
    assert counts == [evals] * 4  # a case whose evaluation count the reference alone cannot hold steady would check nothing
    assert 0.0 < worst <= T.ARS_SENSITIVITY  # the recorded figure covers what is measured here


def test_the_seventh_case_is_rejected_by_the_host():
    d, b, sl = T.ARS_NOT_CONCAVE
    assert T.host_ars(d, b, sl, 7, 4)[0] == 2000


def test_beta_logdens_is_the_oracle_test_case():
    """the weibull set is tests/test_bayesw_oracle.py's case, written as nine numbers: the same values, bit for bit"""
    weibull = lambda x: (-1.3 * x * 4.0 - math.exp(1.3 * x * 0.8) * (50 + 30 * math.exp(-1.3 * x / 0.6) + 8 * math.exp(-2 * 1.3 * x / 0.6))
                         - x * x / (2 * 0.01 * 0.5))
    d, b, sl = T.ARS_SETS["weibull"]
    f = T.beta_logdens(d)
    assert (b, sl) == (0.0, 0.5)
    for x in np.linspace(-0.49, 0.49, 99):
        assert f(float(x)) == weibull(float(x))


def test_sum_references_at_one_small_size():
    N, M = 1025, 8
    geno = T.special_geno(N, M)
    assert (geno[0] == 3).all() and (geno[1] == 0).all() and (geno[2] == 2).all() and geno[3].sum() == 1 and geno[3, N - 1] == 1
    for eps in (T.cancelling_residual(N), T.wide_residual(N), np.random.default_rng(1).normal(size=N)):
        exact = sum(Fraction(float(v)) for v in eps)
        s, bound = T.fsum_and_bound(eps)
        assert abs(Fraction(s) - exact) <= Fraction(T.U) * abs(exact) and bound == N * T.U * math.fsum(np.abs(eps).tolist())
        assert T.within(s, eps) and T.within(float(np.sum(eps)), eps)  # numpy's pairwise order is one of "any order"
        assert not T.within(s + 4 * bound + abs(s) * 2.0 ** -40, eps)
    assert abs(T.fsum_and_bound(T.cancelling_residual(N))[0]) < 1e8 < T.fsum_and_bound(np.abs(T.cancelling_residual(N)))[0] / N * 1.01
    # mave, mstd, dot and update against the dense restatement x = (g - mave) mstd, 0 at a missing call
    eps = np.random.default_rng(2).normal(size=N)
    Xs = synth.standardize(geno[3:])
    for k, j in enumerate(range(3, M)):
        cnt = [int((geno[j] == c).sum()) for c in (1, 2, 3)]
        mave, mstd = T.stats_ref(*cnt, N)
        x = Xs[:, k]
        called = geno[j] != 3
        assert np.allclose(x[called], (geno[j][called] - mave) * mstd, rtol=1e-12, atol=0) and abs(x @ x - (N - 1)) < 1e-9 * N
        ref, bound = T.dot_ref(geno[j], eps, mave, mstd)
        assert abs(float(ref) - float(x.astype(np.longdouble) @ eps.astype(np.longdouble))) <= 1e-12 * np.abs(x * eps).sum()
        assert 0 < bound < 1e-10 * np.abs(x * eps).sum() + 1e-9 and T.dot_within(float(ref), geno[j], eps, mave, mstd)
        assert not T.dot_within(float(ref) + 3 * bound, geno[j], eps, mave, mstd)
        new = T.update_ref(geno[j], eps, mave, mstd, 0.03)
        assert np.allclose(new, eps + 0.03 * x, rtol=0, atol=1e-14) and np.array_equal(new[~called], eps[~called])
    # the columns without a finite mstd
    assert math.isnan(T.stats_ref(0, 0, N, N)[0]) and T.stats_ref(0, 0, 0, N) == (0.0, math.inf) and T.stats_ref(0, N, 0, N) == (2.0, math.inf)
    assert np.isnan(T.update_ref(geno[1], eps, 0.0, math.inf, 0.25)).all() and np.isnan(T.update_ref(geno[2], eps, 2.0, math.inf, 0.25)).all()
    assert np.array_equal(T.update_ref(geno[0], eps, math.nan, math.nan, 0.25), eps)
    assert T.same_bits([math.nan, 1.0, -0.0], [math.nan, 1.0, -0.0]) and not T.same_bits([0.0], [-0.0]) and not T.same_bits([math.nan], [1.0])


@pytest.mark.parametrize("N", T.W_NS)
def test_bayesw_references_stay_finite(N):
    """at alpha = 20 the exponent passes 400 and exp stays finite in float64; the plain float64 references of
    test_density_sums_vi_and_marker_sums agree with the np.longdouble ones to the 1e-12 the device is held to"""
    M = 8
    geno = T.special_geno(N, M)
    rng = np.random.default_rng(N + 2)
    X = rng.normal(size=(N, 3))
    eps = T.w_residual(N)
    assert np.abs(eps).max() <= 25.0 and np.abs(20.0 * eps - T.EULER).max() > 400
    for a in T.ALPHAS:
        for kind, col, p in ((0, 0, (0.25, 0.31, a)), (1, 0, (a, 0.0, 0.0)), (2, 0, (0.2, -0.1, a)), (2, 2, (0.2, -0.1, a))):
            x64 = T.w_exponent(kind, eps, X[:, col], *p, np.float64)
            assert np.abs(x64).max() < 600 and np.isfinite(np.exp(x64)).all()
            plain, ref = T.w_sum_ref(kind, eps, X[:, col], *p)
            assert math.isfinite(plain) and math.isfinite(ref) and T.close(plain, ref, 1e-12)
        for j in (0, 3, M - 1):
            cnt = [int((geno[j] == c).sum()) for c in (1, 2, 3)]
            mave = (cnt[0] + 2.0 * cnt[1]) / (N - cnt[2]) if cnt[2] < N else math.nan
            for b in (0.0, 0.03):
                plain, ref = T.w_marker_sums_ref(geno[j], eps, a, b, mave, 0.7)
                assert np.isfinite(ref).all() and T.close(plain, ref, 1e-12)
        # a monomorphic column with an effect to take out: every called row is NaN, by the reference as on the device
        _, ref = T.w_marker_sums_ref(geno[1], eps, a, 0.03, 0.0, 0.0)
        assert math.isnan(ref[0]) and ref[1:] == [0.0, 0.0]
    assert T.close([math.nan, 1.0], [math.nan, 1.0 + 1e-13], 1e-12) and not T.close([1.0], [math.nan], 1e-12) and not T.close([2.0], [2.0 + 1e-11], 1e-12)
