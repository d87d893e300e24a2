"""A NumPy restatement of hgibbs_spa_roots and hgibbs_spa_pvalue, not a test: pass 0, the root rule and the
p-value, in float64 or longdouble; an exact two-sided tail for intercept-only models by convolving the binomials of the genotype
classes; and the inputs that the CPU and GPU tests of the operator share, so that the tolerance measured on the CPU is measured on
the markers the GPU tests use."""
import math

import numpy as np

STOP = 1e-9
PASSES = 64


def adjusted(codes, xv, Z, b, dtype=np.float64):
    """a_i = xv[code_i] - sum_k Z_ik b_k"""
    return np.asarray(xv, dtype)[codes] - np.asarray(Z, dtype) @ np.asarray(b, dtype)


def terms(a, mu, t, dtype=np.float64):
    """K(t), K'(t), K''(t) in the branch-free stable form"""
    one = dtype(1)
    u = a * dtype(t)
    neg = u <= 0
    E = np.expm1(-np.abs(u))
    c = np.where(neg, mu, one - mu)
    D = one + c * E
    p = np.where(neg, mu * (one + E), mu) / D
    K = np.sum(np.where(neg, dtype(0), u) + np.log1p(c * E) - u * mu)
    return K, np.sum(a * (p - mu)), np.sum(a * a * (p * (one - p)))


def pass0(a, mu):
    c = np.sum(a * mu)
    return np.sum(a * a * (mu * (1 - mu))), np.sum(np.minimum(a, 0)) - c, np.sum(np.maximum(a, 0)) - c  # k2_0, s_lo, s_hi


def roots(a, mu, s, dtype=np.float64):
    """the record of hgibbs_spa_roots for one marker, as a dict with the struct's fields"""
    a, mu = np.asarray(a, dtype), np.asarray(mu, dtype)
    k2_0, s_lo, s_hi = pass0(a, mu)
    r = dict(t=[dtype(0)] * 2, K=[dtype(0)] * 2, K2=[dtype(0)] * 2, k2_0=k2_0, s_lo=s_lo, s_hi=s_hi, iters=[0, 0], flags=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = dtype(1) / np.sqrt(k2_0)
        for z in range(2):
            tau = dtype(abs(s)) if z == 0 else -dtype(abs(s))
            if not (s_lo < tau < s_hi):
                r["flags"] |= 4 << z
                continue
            lo, hi = (dtype(0), dtype(np.inf)) if z == 0 else (dtype(-np.inf), dtype(0))
            t = tau / k2_0
            closing = False
            for _ in range(PASSES):
                K, k1, k2 = terms(a, mu, t, dtype)
                r["iters"][z] += 1
                if closing:
                    r["K"][z], r["K2"][z] = K, k2
                    r["flags"] |= 1 << z
                    break
                g = k1 - tau
                if g > 0:
                    hi = t
                elif g < 0:
                    lo = t
                tn = t - g / k2
                if abs(tn - t) <= dtype(STOP) * max(abs(t), scale):  # the stop rule FIRST
                    closing = True
                elif not (lo < tn < hi):
                    tn = (lo + hi) / 2 if np.isfinite(lo) and np.isfinite(hi) else 2 * t
                t = tn
            r["t"][z] = t
    return r


def tail(tau, converged, t, K, K2):
    """one tail of the Barndorff-Nielsen form, or None where a validity rule fails"""
    t, K, K2, tau = float(t), float(K), float(K2), float(tau)
    h = t * tau - K
    if not converged or not h > 0 or not K2 > 0:
        return None
    w = math.copysign(math.sqrt(2 * h), t)
    v = t * math.sqrt(K2)
    if not v / w > 0:
        return None
    z = w + math.log(v / w) / w
    if not math.isfinite(z) or not (z > 0 if tau > 0 else z < 0):
        return None
    return 0.5 * math.erfc(abs(z) / math.sqrt(2))


def pvalue(s, r):
    """(p_upper, p_lower, p, valid) of hgibbs_spa_pvalue; None / NaN where not valid"""
    up = tail(abs(s), r["flags"] & 1, r["t"][0], r["K"][0], r["K2"][0])
    dn = tail(-abs(s), r["flags"] & 2, r["t"][1], r["K"][1], r["K2"][1])
    ok = up is not None and dn is not None
    return up, dn, (up + dn if ok else math.nan), ok


def normal_p(s, v):
    return math.erfc(abs(s) / math.sqrt(2 * v))


# ---- intercept-only models: the score and its exact distribution ----
def intercept_only(counts, cases, mu):
    """counts, cases: rows and cases by genotype 0, 1, 2; returns the per-class a (x standardised with the sample SD, minus its
    mean), the per-row codes, the score U and V"""
    counts = np.asarray(counts)
    n = counts.sum()
    g = np.arange(3.0)
    m = (counts * g).sum() / n
    sd = math.sqrt((counts * (g - m) ** 2).sum() / (n - 1))
    a = (g - m) / sd  # (the weights are constant, so b is the mean of x, which is 0)
    U = float((a * (np.asarray(cases) - mu * counts)).sum())
    V = float(mu * (1 - mu) * (counts * a * a).sum())
    return a, np.repeat(np.arange(3), counts), U, V


def binom_pmf(n, p):
    k = np.arange(n + 1)
    lg = np.array([math.lgamma(n + 1) - math.lgamma(x + 1) - math.lgamma(n - x + 1) for x in k])
    return np.exp(lg + k * math.log(p) + (n - k) * math.log1p(-p))


def exact_two_sided(counts, a, mu, U):
    """P(U* >= |U|) + P(U* <= -|U|) for U* = sum_c a_c (D_c - n_c mu), D_c ~ Binomial(n_c, mu) independent; values within 1e-9 |U| of
    the observed one count as equal to it"""
    big = int(np.argmax(counts))  # the largest class goes last, through its cumulative sums: no array of all triples
    val = np.zeros(1)
    pr = np.ones(1)
    for c in range(3):
        if c == big:
            continue
        k = np.arange(counts[c] + 1)
        val = (val[:, None] + a[c] * (k - counts[c] * mu)[None, :]).ravel()
        pr = (pr[:, None] * binom_pmf(counts[c], mu)[None, :]).ravel()
    k = np.arange(counts[big] + 1)
    v = a[big] * (k - counts[big] * mu)
    order = np.argsort(v)
    v, cum = v[order], np.concatenate([[0.0], np.cumsum(binom_pmf(counts[big], mu)[order])])
    edge = abs(U) * (1 - 1e-9)
    upper = cum[-1] - cum[np.searchsorted(v, edge - val, side="left")]   # v >= edge - val
    lower = cum[np.searchsorted(v, -edge - val, side="right")]           # v <= -edge - val
    return float((pr * (upper + lower)).sum())


# ---- the inputs of the operator's tests ----
GRID_N = (37, 261, 4099, 8197)  # padding inside the last dword; the workgroup's stride of 256 rows plus 5; 4096 + 3; 8192 + 5
GRID_Q = (1, 5)
GRID_M = 64


def roots_case(n, q, seed=0):
    """genotypes (GRID_M, n) with MAF from 0.005 to 0.4 and 2 % missing calls in every fourth column, q - 1 covariates, about 8 %
    cases, mu from a real hgibbs_logit_null fit; B, xv and s as --assoc-spa forms them.  Three scores are moved: entry 3 to three times
    its value, entry 5 past s_hi and -s_lo (both tails unreachable), entry 7 to 0."""
    from hydra_amd import capi

    rng = np.random.default_rng(1000 * n + q + seed)
    maf = np.geomspace(0.005, 0.4, GRID_M)
    geno = rng.binomial(2, maf[:, None], size=(GRID_M, n)).astype(np.uint8)
    for j in range(GRID_M):  # keep every column polymorphic
        if geno[j].min() == geno[j].max():
            geno[j, (7 * j) % n] = 1 if geno[j, 0] != 1 else 0
    for j in range(0, GRID_M, 4):
        geno[j, rng.random(n) < 0.02] = 3
        if (geno[j] != 3).sum() < 2 or geno[j][geno[j] != 3].min() == geno[j][geno[j] != 3].max():
            geno[j, :2] = (0, 1)
    Z = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(q - 1)])
    liab = rng.standard_normal(n) + (0.3 * Z[:, 1] if q > 1 else 0.0)
    ncase = max(int(round(0.08 * n)), 4)
    d = np.zeros(n)
    d[np.argsort(-liab)[:ncase]] = 1.0
    fit = capi.logit_null(Z, d)
    mu, w = fit["mu"], fit["w"]
    info = Z.T @ (Z * w[:, None])
    B, xv, s = np.zeros((GRID_M, q)), np.zeros((GRID_M, 4)), np.zeros(GRID_M)
    for j in range(GRID_M):
        called = geno[j] != 3
        g = geno[j][called].astype(np.float64)
        m, sd = g.mean(), 1.0 / g.std(ddof=1)
        xv[j] = ((0 - m) * sd, (1 - m) * sd, (2 - m) * sd, 0.0)
        B[j] = np.linalg.solve(info, Z.T @ (w * xv[j][geno[j]]))
        s[j] = np.sum(adjusted(geno[j], xv[j], Z, B[j]) * (d - mu))
    s[3] *= 3.0
    _, lo5, hi5 = pass0(adjusted(geno[5], xv[5], Z, B[5]), mu)
    s[5] = 1.5 * max(hi5, -lo5)
    s[7] = 0.0
    return dict(geno=geno, Z=Z, d=d, mu=mu, B=B, xv=xv, s=s)


def case_roots(case, dtype=np.float64):
    return [roots(adjusted(case["geno"][j], case["xv"][j], case["Z"], case["B"][j], dtype), np.asarray(case["mu"], dtype), case["s"][j], dtype)
            for j in range(GRID_M)]


def rel(a, b):
    a, b = float(a), float(b)
    return 0.0 if a == b else abs(a - b) / max(abs(a), abs(b))
