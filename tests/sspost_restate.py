"""A plain restatement of hgibbs_ss_post_* (no test of its own): the Welford steps of k_ss_post_add and the
formulas of k_ss_post_final in the kernels' order, in scalar f64 operations (Python floats) in loops.  Every step is a correctly
rounded + - x / of two doubles, so the accumulators are the device's bit for bit; sqrt is math.sqrt."""
import math

import numpy as np


class Post:
    """Accumulators over T planned records of C chains of M markers with K components."""

    def __init__(self, C, M, K, T):
        assert C >= 1 and T >= 4
        self.C, self.M, self.K, self.T, self.t = C, M, K, T, 0
        self.pmean, self.pm2 = [0.0] * M, [0.0] * M
        self.hmean = [[[0.0] * M for _ in range(2)] for _ in range(C)]
        self.hm2 = [[[0.0] * M for _ in range(2)] for _ in range(C)]
        self.cnt = np.zeros((K, M), dtype=np.uint32)

    def add(self, beta, comp):
        """One record: beta (C, M) float64 and comp (C, M) integers, the chains' state as it stands."""
        beta = np.asarray(beta, dtype=np.float64).reshape(self.C, self.M)
        comp = np.asarray(comp).reshape(self.C, self.M)
        C, T, t, n = self.C, self.T, self.t, self.T // 2
        assert t < T
        half, nh = (0, t + 1) if t < n else (1, t - (T - n) + 1) if t >= T - n else (None, 0)
        for j in range(self.M):
            mean, m2 = self.pmean[j], self.pm2[j]
            for r in range(C):
                x = float(beta[r, j])
                d = x - mean
                mean = mean + d / float(t * C + r + 1)
                m2 = m2 + d * (x - mean)
                if half is not None:
                    hm, h2 = self.hmean[r][half][j], self.hm2[r][half][j]
                    d = x - hm
                    hm = hm + d / float(nh)
                    h2 = h2 + d * (x - hm)
                    self.hmean[r][half][j], self.hm2[r][half][j] = hm, h2
                k = int(comp[r, j])
                assert 0 <= k < self.K
                self.cnt[k, j] += 1
            self.pmean[j], self.pm2[j] = mean, m2
        self.t = t + 1

    def final(self):
        """(mean, sd, pip, rhat), M each, after exactly T records."""
        assert self.t == self.T
        C, T, M = self.C, self.T, self.M
        n, m, total = T // 2, 2 * C, C * T
        mean, sd, pip, rhat = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)
        for j in range(M):
            mean[j] = self.pmean[j]
            sd[j] = math.sqrt(self.pm2[j] / float(total - 1))
            pip[j] = float(total - int(self.cnt[0, j])) / float(total)
            W = gm = 0.0
            for r in range(C):
                for half in range(2):
                    W += self.hm2[r][half][j] / float(n - 1)
                    gm += self.hmean[r][half][j]
            W /= float(m)
            gm /= float(m)
            Bn = 0.0
            for r in range(C):
                for half in range(2):
                    cm = self.hmean[r][half][j]
                    Bn += (cm - gm) * (cm - gm)
            Bn /= float(m - 1)
            varp = float(n - 1) / float(n) * W + Bn
            rhat[j] = math.sqrt(varp / W) if W > 0.0 else math.nan
        return mean, sd, pip, rhat

    def raw(self, r, half):
        """(mean, m2) of half `half` of chain r; r = C, half = 0: the pooled pair."""
        if r == self.C:
            return np.array(self.pmean), np.array(self.pm2)
        return np.array(self.hmean[r][half]), np.array(self.hm2[r][half])


def run(records, C, M, K, T):
    """Post over the sequence of (beta, comp) records."""
    p = Post(C, M, K, T)
    for beta, comp in records:
        p.add(beta, comp)
    return p
