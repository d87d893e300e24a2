"""tests/sspost_restate.py (the restatement the device's per-marker posterior table is held to) against
hgibbs_mcmc_diag on the same series: mean, sd and split-R^ per marker at ss_common.close -- Welford's steps against two-pass sums, so
no bit equality -- with NaN in the same places; and a case of four records of one chain worked out by hand.  No GPU needed."""
import math

import numpy as np
import pytest

import ss_common as sc
import sspost_restate as pr
from hydra_amd import capi

K = 4


def series(R, T, seed):
    """beta, comp (T, R, M = 4): marker 0 always 0; marker 1 non-zero in one record of one chain only; marker 2 the chains (and the
    second half of each) shifted apart; marker 3 a spike-and-slab series"""
    rs = np.random.default_rng(seed)
    beta = np.zeros((T, R, 4))
    beta[1, R - 1, 1] = 0.37
    n = T // 2
    for r in range(R):
        beta[:, r, 2] = rs.normal(0.0, 0.1, T) + 10.0 * r + 10.0 * (np.arange(T) >= T - n)
    beta[:, :, 3] = np.where(rs.random((T, R)) < 0.6, rs.normal(0.0, 0.05, (T, R)), 0.0)
    comp = np.where(beta != 0.0, 1 + (np.abs(beta) > 0.05) + (np.abs(beta) > 1.0), 0).astype(np.int32)
    return beta, comp


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("T", [4, 5, 12])
def test_against_mcmc_diag(R, T):
    beta, comp = series(R, T, 100 * R + T)
    p = pr.run(zip(beta, comp), R, 4, K, T)
    mean, sd, pip, rhat = p.final()
    for j in range(4):
        wm, ws, wr, _ = capi.mcmc_diag(np.ascontiguousarray(beta[:, :, j].T))
        assert sc.close(mean[j], wm) and sc.close(sd[j], ws), (j, mean[j], wm, sd[j], ws)
        assert math.isnan(rhat[j]) == math.isnan(wr), (j, rhat[j], wr)
        if not math.isnan(wr):
            assert sc.close(rhat[j], wr), (j, rhat[j], wr)
        assert pip[j] == np.count_nonzero(beta[:, :, j]) / (R * T)
        assert [int(p.cnt[k, j]) for k in range(K)] == [int(np.count_nonzero(comp[:, :, j] == k)) for k in range(K)]
    assert math.isnan(rhat[0]) and pip[0] == 0.0 and sd[0] == 0.0 and mean[0] == 0.0
    assert pip[1] == 1.0 / (R * T) and mean[1] != 0.0
    assert rhat[2] > 1.5
    # the middle record of an odd T is in no half, and in the pooled pair
    assert p.raw(R, 0)[0][2] == mean[2]
    if T == 5:
        lone = pr.run(zip(np.delete(beta, 2, axis=0), np.delete(comp, 2, axis=0)), R, 4, K, 4)
        for r in range(R):
            for half in range(2):
                assert np.array_equal(lone.raw(r, half)[0], p.raw(r, half)[0]) and np.array_equal(lone.raw(r, half)[1], p.raw(r, half)[1])


def test_four_records_of_one_chain_by_hand():
    # x = 1, 3, 0, 4 with the components 1, 2, 0, 1.  Pooled: mean 2, m2 = 1 + 1 + 4 + 4 = 10, sd = sqrt(10 / 3), PIP = 3 / 4.
    # Halves (1, 3) and (0, 4): means 2 and 2, m2 2 and 8, variances 2 and 8: W = 5, B / n = 0, var+ = 1/2 W, R^ = sqrt(1/2).
    x, k = [1.0, 3.0, 0.0, 4.0], [1, 2, 0, 1]
    p = pr.run([(np.array([[v]]), np.array([[c]])) for v, c in zip(x, k)], 1, 1, 3, 4)
    mean, sd, pip, rhat = p.final()
    assert [p.raw(0, 0)[i][0] for i in (0, 1)] == [2.0, 2.0] and [p.raw(0, 1)[i][0] for i in (0, 1)] == [2.0, 8.0]
    assert p.cnt[:, 0].tolist() == [1, 2, 1] and pip[0] == 0.75
    assert rhat[0] == math.sqrt(0.5)
    # the thirds of the pooled steps round: the last bits, not more
    assert abs(mean[0] - 2.0) <= 4 * 2.0 ** -52 and abs(p.raw(1, 0)[1][0] - 10.0) <= 16 * 2.0 ** -52
    assert abs(sd[0] - math.sqrt(10.0 / 3.0)) <= 8 * 2.0 ** -52
