"""--reml restated in dense f64 NumPy (hydra_amd/csrc/hg_reml.hip.h, hg_remlfit.cpp), and the helpers the REML
tests share: the sign probes from mix64, X from marker statistics, Q by modified Gram-Schmidt, dense solves through one
eigendecomposition, f, the root rule, the average-information numbers, the jackknife, and the dense REML likelihood.

The restatement is dense: it forms A = X X'/M_used and solves with it, which is what the library avoids.  The comparisons with the
device are therefore to a tolerance computed from the conditioning (the tests state it); only next_rule is held to the library's
hgibbs_reml_next exactly, and it takes its logarithms from math.log, the C library's, as the library does."""
import math

import numpy as np

from hydra_amd import synth

from pca_restate import mix64

_M64 = (1 << 64) - 1
STEP = 0xD1B54A32D192ED03
XMAX = math.log(9999.0)
CONTINUE, CONVERGED, AT_BOUND = 0, 1, 2


# ---- probes ----
def signs(seed, c, idx):
    """s(c, i) = +1 when the top bit of mix64((seed ^ mix64(c)) + i STEP) is 0, else -1, for the indices idx"""
    base = np.uint64((seed & _M64) ^ synth._mix64(c))
    with np.errstate(over="ignore"):
        h = mix64(base + np.asarray(idx, dtype=np.uint64) * np.uint64(STEP))
    return np.where((h >> np.uint64(63)) == 0, 1.0, -1.0)


def sign_one(seed, c, i):
    """the same for one index, in Python integers"""
    return -1.0 if synth._mix64((((seed & _M64) ^ synth._mix64(c)) + i * STEP) & _M64) >> 63 else 1.0


# ---- data ----
def cohort(N, M, miss=0.02, seed=1):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.5, size=M)
    geno = rng.binomial(2, p[:, None], size=(M, N)).astype(np.int8)
    if miss > 0:
        geno[rng.random((M, N)) < miss] = 3
    return geno


def stats_of(geno):
    """mave, mstd as the chain defines them (synth.standardize), NaN mstd where a marker has no spread or no call"""
    M, N = geno.shape
    nm = geno != 3
    g = np.where(nm, geno, 0).astype(np.float64)
    cnt = nm.sum(axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        mave = g.sum(axis=1) / cnt
        ss = np.sum(np.where(nm, (g - mave[:, None]) ** 2, 0.0), axis=1)
        mstd = np.sqrt((N - 1) / ss)
    mstd[~np.isfinite(mstd)] = np.nan
    return mave, mstd


def xmat(geno, mave, mstd):
    """X (n x M): (g - mave) mstd at a call, 0 at a missing call, zero columns outside M_used; and the mask of M_used"""
    good = np.isfinite(mstd)
    nm = geno != 3
    with np.errstate(all="ignore"):
        X = np.where(nm & good[:, None], (geno.astype(np.float64) - mave[:, None]) * mstd[:, None], 0.0)
    return np.ascontiguousarray(X.T), good


def covariates(n, q, seed=5):
    """Z (n x q): the column of ones, then q - 1 standard normal columns"""
    rng = np.random.default_rng(seed)
    return np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(q - 1)])


def basis(Z):
    """Q (n x q): modified Gram-Schmidt applied twice, column after column"""
    Q = np.array(Z, dtype=np.float64)
    for c in range(Q.shape[1]):
        before = float(Q[:, c] @ Q[:, c])
        for _ in range(2):
            for b in range(c):
                Q[:, c] -= (Q[:, b] @ Q[:, c]) * Q[:, b]
        after = float(Q[:, c] @ Q[:, c])
        if not after > 1e-20 * before:
            raise ValueError("column %d is dependent" % c)
        Q[:, c] /= math.sqrt(after)
    return Q


class Dense:
    """A' = P_c A P_c on the n - q dimensions off the covariates: U (n x (n - q)) orthonormal with U'Q = 0, A'' = U'AU = W diag(w) W'.
    H(delta)^-1 b = S diag(1 / (w + delta)) S' b on the range of P_c, S = U W."""

    def __init__(self, X, good, Z):
        self.n = X.shape[0]
        self.m_used = int(good.sum())
        self.Q = basis(Z)
        self.q = self.Q.shape[1]
        U = np.linalg.qr(self.Q, mode="complete")[0][:, self.q:]  # (the first q columns of the full factor span Q)
        XU = X.T @ U
        self.w, W = np.linalg.eigh(XU.T @ XU / self.m_used)
        self.w = np.maximum(self.w, 0.0)
        self.S = U @ W
        self.X = X

    def project(self, b):
        return b - self.Q @ (self.Q.T @ b)

    def A(self):
        return self.X @ self.X.T / self.m_used

    def H(self, delta):
        P = np.eye(self.n) - self.Q @ self.Q.T
        return P @ self.A() @ P + delta * np.eye(self.n)

    def kappa(self, delta):
        return (float(self.w.max()) + delta) / delta  # (H has the eigenvalue delta on the span of Q)

    def solve(self, B, delta):
        """H^-1 P_c b for the rows of B"""
        return ((self.S.T @ self.project(B.T)) / (self.w + delta)[:, None]).T @ self.S.T

    def apply(self, v):
        """P_c A P_c v"""
        pv = self.project(v)
        return self.project(self.X @ (self.X.T @ pv) / self.m_used)


def probes(d, seed, T, rows):
    """G (T x n) and E (T x n): G_t = P_c X s(2t, marker)/sqrt(M_used), E_t = P_c s(2t + 1, row), rows the handle's row indices"""
    M = d.X.shape[1]
    G = np.zeros((T, d.n))
    E = np.zeros((T, d.n))
    for t in range(T):
        G[t] = d.project(d.X @ signs(seed, 2 * t, np.arange(M)) / math.sqrt(d.m_used))
        E[t] = d.project(signs(seed, 2 * t + 1, rows))
    return G, E


def eval_sums(d, G, E, y, delta):
    """(T + 1) x 3: vAv, vv, vb of b_t = G_t + sqrt(delta) E_t and b_T = P_c y"""
    B = np.vstack([G + math.sqrt(delta) * E, d.project(y)[None, :]])
    V = d.solve(B, delta)
    U = V @ d.X
    return np.column_stack([np.sum(U * U, axis=1) / d.m_used, np.sum(V * V, axis=1), np.sum(V * B, axis=1)]), V, B


def f_of(sums, skip=-1):
    T = sums.shape[0] - 1
    a = b = 0.0
    for t in range(T):
        if t == skip:
            continue
        a += float(sums[t, 0])
        b += float(sums[t, 1])
    return math.log(a / b) - math.log(float(sums[T, 0]) / float(sums[T, 1]))


def f_exact(d, y, delta):
    """f with the probes' expectations in place of the probes: E b b' = H on the range of P_c, so the sums become traces"""
    yt = d.S.T @ y
    tA = float(np.sum(d.w / (d.w + delta)))
    t1 = float(np.sum(1.0 / (d.w + delta)))
    vAv = float(np.sum(d.w * yt ** 2 / (d.w + delta) ** 2))
    vv = float(np.sum(yt ** 2 / (d.w + delta) ** 2))
    return math.log(tA / t1) - math.log(vAv / vv)


def reml_loglik(d, y, x):
    """the REML log-likelihood at log delta = x with sigma_G^2 profiled out, up to a constant"""
    delta = math.exp(x)
    yt = d.S.T @ y
    m = d.n - d.q
    return -0.5 * (m * math.log(float(np.sum(yt ** 2 / (d.w + delta))) / m) + float(np.sum(np.log(d.w + delta))))


def reml_maximiser(d, y, spacing=0.05, width=2e-4):
    """argmax of reml_loglik over |x| <= log 9999: a grid of the given spacing, then golden section on the bracket around its best
    point until the bracket is narrower than `width`"""
    grid = np.arange(-XMAX, XMAX + spacing, spacing)
    ll = np.array([reml_loglik(d, y, x) for x in grid])
    at = int(np.argmax(ll))
    lo, hi = grid[max(at - 1, 0)], grid[min(at + 1, grid.size - 1)]
    g = (math.sqrt(5.0) - 1.0) / 2.0
    c, e = hi - g * (hi - lo), lo + g * (hi - lo)
    fc, fe = reml_loglik(d, y, c), reml_loglik(d, y, e)
    while hi - lo > width:
        if fc > fe:
            hi, e, fe = e, c, fc
            c = hi - g * (hi - lo)
            fc = reml_loglik(d, y, c)
        else:
            lo, c, fc = c, e, fe
            e = lo + g * (hi - lo)
            fe = reml_loglik(d, y, e)
    return 0.5 * (lo + hi)


# ---- the root rule: hgibbs_reml_next, operation for operation ----
def next_rule(x, f, h0=0.25, x_tol=0.01, max_steps=12):
    """(x_next, status); raises ValueError where the library refuses"""
    k = len(x)
    if k == 0:
        return math.log((1.0 - h0) / h0), CONTINUE
    if k == 1:
        h1 = min(2.0 * h0, (1.0 + h0) / 2.0) if f[0] < 0.0 else h0 / 2.0
        return math.log((1.0 - h1) / h1), CONTINUE
    x1, x0, f1, f0 = float(x[-1]), float(x[-2]), float(f[-1]), float(f[-2])
    if x1 == x0 and abs(x1) == XMAX:
        return x1, AT_BOUND
    if abs(x1 - x0) < x_tol:
        return x1, CONVERGED
    if f1 == f0:
        raise ValueError("flat")
    if k >= max_steps:
        raise ValueError("max_steps")
    xn = x1 - f1 * (x1 - x0) / (f1 - f0)
    return (XMAX if xn > XMAX else -XMAX if xn < -XMAX else xn), CONTINUE


def run_rule(fun, h0=0.25, x_tol=0.01, max_steps=12):
    """the driver's loop around a function of x: the trace (x, f) and the status"""
    xs, fs = [], []
    while True:
        xn, st = next_rule(xs, fs, h0, x_tol, max_steps)
        if st != CONTINUE:
            return np.array(xs), np.array(fs), st
        xs.append(xn)
        fs.append(fun(xn))


# ---- the estimate: hgibbs_reml_finish ----
def ai_numbers(d, y, delta):
    """a'z1, a'z2, v'z2 with v = H^-1 P_c y, a = P_c A P_c v, H z1 = a, H z2 = v"""
    v = d.solve(y[None, :], delta)[0]
    a = d.apply(v)
    z = d.solve(np.vstack([a, v]), delta)
    return np.array([a @ z[0], a @ z[1], v @ z[1]])


def finish(n, q, x2, sums_prev, sums_last, ai3=None):
    T = sums_last.shape[0] - 1
    delta = math.exp(x2[1])
    vg = float(sums_last[T, 2]) / (n - q)
    ve = delta * vg
    vp = vg + ve
    h2 = 1.0 / (1.0 + delta)
    out = {"logdelta": x2[1], "delta": delta, "vg": vg, "ve": ve, "vp": vp, "h2": h2}
    for k in ("se_vg", "se_ve", "se_vp", "se_h2", "se_mc", "se_logdelta_mc"):
        out[k] = float("nan")
    if ai3 is not None:
        AI = np.array([[ai3[0], ai3[1]], [ai3[1], ai3[2]]]) / (2.0 * vg ** 3)
        C = np.linalg.inv(AI)
        g = np.array([ve / vp ** 2, -vg / vp ** 2])
        out.update(se_vg=math.sqrt(C[0, 0]), se_ve=math.sqrt(C[1, 1]), se_vp=math.sqrt(C[0, 0] + C[1, 1] + 2.0 * C[0, 1]),
                   se_h2=math.sqrt(float(g @ C @ g)))
    if T >= 2:
        r = np.zeros(T)
        for t in range(T):
            f0, f1 = f_of(sums_prev, t), f_of(sums_last, t)
            r[t] = x2[1] - f1 * (x2[1] - x2[0]) / (f1 - f0)
        se = math.sqrt((T - 1) / T * float(np.sum((r - r.mean()) ** 2)))
        out.update(se_logdelta_mc=se, se_mc=se * h2 * (1.0 - h2))
    return out
