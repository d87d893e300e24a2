"""hgibbs_mcmc_diag (host only) held to tests/mcmcdiag_restate.py within ss_common.close: split-R^ and the
effective sample size over R = 1, 2, 5 chains of T = 4, 5 (odd: the middle draw dropped), 101 and 2000 draws of AR(1) chains;
chains shifted apart; a constant chain among moving ones; all constant (NaN); a case worked out by hand; iid draws; the refusals."""
import numpy as np
import pytest

import mcmcdiag_restate as md
import ss_common as sc
from hydra_amd import capi


def ar1(R, T, phi, seed, shift=0.0):
    rs = np.random.default_rng(seed)
    e = rs.normal(size=(R, T))
    x = np.zeros((R, T))
    x[:, 0] = e[:, 0]
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x + shift * np.arange(R)[:, None]


def same(got, want):
    for g, w, name in zip(got, want, ("mean", "sd", "rhat", "ess")):
        if np.isnan(w):
            assert np.isnan(g), name
        else:
            assert sc.close(g, w), (name, g, w)


@pytest.mark.parametrize("phi", [0.0, 0.9, -0.5])
@pytest.mark.parametrize("T", [4, 5, 101, 2000])
@pytest.mark.parametrize("R", [1, 2, 5])
def test_ar1_chains_match_the_restatement(R, T, phi):
    x = ar1(R, T, phi, seed=1000 * R + T + int(10 * phi))
    same(capi.mcmc_diag(x), md.diag(x))


def test_odd_length_drops_the_middle_draw():
    x = ar1(2, 5, 0.0, seed=3)
    y = x.copy()
    y[:, 2] = 1e6  # (mean and sd see it; the half-chains do not)
    a, b = capi.mcmc_diag(x), capi.mcmc_diag(y)
    assert a[2:] == b[2:] and a[:2] != b[:2]
    assert a[2:] == capi.mcmc_diag(np.delete(x, 2, axis=1))[2:]


def test_chains_shifted_apart():
    x = ar1(4, 200, 0.3, seed=5, shift=3.0)
    got = capi.mcmc_diag(x)
    same(got, md.diag(x))
    assert got[2] > 1.5


def test_one_constant_chain_among_moving_ones():
    x = ar1(3, 100, 0.5, seed=6)
    x[1] = 0.25
    got = capi.mcmc_diag(x)
    same(got, md.diag(x))
    assert np.isfinite(got[2]) and np.isfinite(got[3])


def test_all_constant_is_nan():
    x = np.full((3, 10), 2.5)
    mean, sd, rhat, ess = capi.mcmc_diag(x)
    assert (mean, sd) == (2.5, 0.0) and np.isnan(rhat) and np.isnan(ess)
    same((mean, sd, rhat, ess), md.diag(x))


def test_two_chains_of_four_draws_by_hand():
    # half-chains (0, 2), (1, 3), (2, 4), (5, 7): means 1, 2, 3, 6, every variance 2, so W = 2 and B / n = 14 / 3;
    # var+ = W / 2 + 14 / 3 = 17 / 3; every lag-1 autocovariance is (-1)(1) / 2, so rho_1 = 1 - 2.5 / (17 / 3) = 9.5 / 17,
    # P_0 = 26.5 / 17, tau = 36 / 17, ESS = 8 / tau = 34 / 9 (below the cap 8 log10 8)
    x = np.array([[0.0, 2.0, 1.0, 3.0], [2.0, 4.0, 5.0, 7.0]])
    mean, sd, rhat, ess = capi.mcmc_diag(x)
    assert mean == 3.0
    assert sc.close(sd, np.sqrt(36.0 / 7.0)) and sc.close(rhat, np.sqrt(17.0 / 6.0)) and sc.close(ess, 34.0 / 9.0)
    same((mean, sd, rhat, ess), md.diag(x))


def test_iid_draws():
    x = ar1(4, 2000, 0.0, seed=8)
    got, want = capi.mcmc_diag(x), md.diag(x)
    same(got, want)
    assert 0.99 <= got[2] <= 1.01


def test_one_chain_is_allowed():
    x = ar1(1, 50, 0.2, seed=9)
    got = capi.mcmc_diag(x)
    same(got, md.diag(x))
    assert np.isfinite(got[2])


def test_two_runs_give_the_same_bits():
    x = ar1(3, 101, 0.9, seed=10)
    assert capi.mcmc_diag(x) == capi.mcmc_diag(x)


def test_refusals():
    L = capi.lib()
    x = np.zeros((2, 8))
    out = [capi.C.c_double() for _ in range(4)]
    refs = [capi.C.byref(o) for o in out]
    for R, T, ptr, msg in ((2, 3, capi._dp(x), "hgibbs_mcmc_diag: T = 3 draws per chain, split-R^ needs at least 4"),
                           (0, 8, capi._dp(x), "hgibbs_mcmc_diag: R = 0, there must be at least one chain"),
                           (2, 8, None, "hgibbs_mcmc_diag: null argument")):
        with pytest.raises(capi.HgError) as e:
            capi.check(L.hgibbs_mcmc_diag(R, T, ptr, *refs))
        assert msg in str(e.value), str(e.value)
    with pytest.raises(capi.HgError):
        capi.mcmc_diag(np.zeros((2, 3)))
