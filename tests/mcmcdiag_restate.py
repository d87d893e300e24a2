"""A plain NumPy restatement of hgibbs_mcmc_diag (no test of its own): split-R^ of Gelman et al. (BDA3 section 11.4; no rank
normalisation) and the effective sample size of the Stan reference manual from the same half-chains, with Geyer's initial monotone
positive sequence.  Written from the formulas, with NumPy's sums, every lag's autocovariance computed up front."""
import numpy as np


def halves(x):
    """(R, T) -> (2 R, n), n = T // 2: the first n and the last n draws of every chain (an odd T drops the middle draw)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1] // 2
    return np.stack([h for row in x for h in (row[:n], row[x.shape[1] - n:])])


def diag(x):
    """(mean, sd, rhat, ess) of the (R, T) draws x."""
    x = np.asarray(x, dtype=np.float64)
    mean, sd = x.mean(), x.std(ddof=1)
    h = halves(x)
    m, n = h.shape
    W = h.var(axis=1, ddof=1).mean()
    Bn = h.mean(axis=1).var(ddof=1)  # B / n
    varp = (n - 1) / n * W + Bn
    if not W > 0.0:
        return mean, sd, np.nan, np.nan
    rhat = np.sqrt(varp / W)
    d = h - h.mean(axis=1, keepdims=True)
    acov = np.array([(d[:, :n - t] * d[:, t:]).sum(axis=1).mean() / n for t in range(n)])
    rho = 1.0 - (W - acov) / varp
    rho[0] = 1.0
    pairs = []
    for k in range(n // 2):  # 2 k + 1 <= n - 1
        P = rho[2 * k] + rho[2 * k + 1]
        if not P > 0.0:
            break
        pairs.append(min(P, pairs[-1]) if pairs else P)
    tau = -1.0 + 2.0 * sum(pairs)
    cap = m * n * np.log10(m * n)
    ess = min(m * n / tau, cap) if tau > 0.0 else cap
    return mean, sd, rhat, ess
