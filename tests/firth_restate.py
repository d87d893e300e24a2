"""A NumPy restatement of hgibbs_firth_fit and hgibbs_firth_stats, not a test: the sums of a pass, the root
rule and the statistics, in float64 or longdouble; and the inputs that the CPU and GPU tests of the operator share, so that the
tolerance measured on the CPU is measured on the entries the GPU tests use."""
import math

import numpy as np

import spa_restate as R

STOP = 1e-9
PASSES = 64
CONVERGED, DEGENERATE = 1, 2


def sums(a, mu, t, dtype=np.float64):
    """K(t), K'(t), K''(t), K'''(t), K''''(t) in the branch-free stable form of section 26"""
    one = dtype(1)
    u = a * dtype(t)
    neg = u <= 0
    E = np.expm1(-np.abs(u))
    c = np.where(neg, mu, one - mu)
    cE = c * E
    p = np.where(neg, mu * (one + E), mu) / (one + cE)
    v = p * (one - p)
    a2 = a * a
    K = np.sum((np.where(neg, dtype(0), u) + np.log1p(cE)) - u * mu)
    return (K, np.sum(a * (p - mu)), np.sum(a2 * v), np.sum((a2 * a) * (v * (one - dtype(2) * p))),
            np.sum((a2 * a2) * (v * (one - dtype(6) * v))))


def score(s, k1, k2, k3, k4, dtype=np.float64):
    """the modified score g and its derivative from the sums at one point"""
    half = dtype(0.5)
    r = k3 / k2
    return dtype(s) - k1 + half * r, -k2 + half * (k4 / k2 - r * r)


def fit(a, mu, s, dtype=np.float64):
    """the record of hgibbs_firth_fit for one entry, as a dict with the struct's fields"""
    a, mu = np.asarray(a, dtype), np.asarray(mu, dtype)
    zero = dtype(0)
    r = dict(beta=zero, K=zero, K2=zero, g=zero, k2_0=zero, iters=0, flags=0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t, tg, lo, hi = zero, zero, dtype(-np.inf), dtype(np.inf)
        closing = False
        scale = zero
        for it in range(PASSES + 1):
            K, k1, k2, k3, k4 = sums(a, mu, t, dtype)
            if it == 0:
                if not (np.isfinite(k2) and k2 > 0):
                    r["flags"] = DEGENERATE
                    return r
                r["k2_0"] = k2
                scale = dtype(1) / np.sqrt(k2)
            else:
                r["iters"] += 1
            if closing:
                r["K"], r["K2"] = K, k2
                r["flags"] |= CONVERGED
                break
            g, gp = score(s, k1, k2, k3, k4, dtype)
            if np.isfinite(g) and np.isfinite(gp):
                r["g"] = g
                tg = t
                if g > 0:
                    lo = t
                elif g < 0:
                    hi = t
                tn = t - g / gp
                if abs(tn - t) <= dtype(STOP) * max(abs(t), scale):  # the stop rule FIRST
                    closing = True
                elif not (lo < tn < hi):
                    if np.isfinite(lo) and np.isfinite(hi):
                        tn = (lo + hi) / 2
                    elif t == 0:
                        tn = scale if g > 0 else -scale
                    else:
                        tn = 2 * t
            else:  # the probabilities have saturated: back towards the last good point, no sign taken
                if t > tg:
                    hi = t
                elif t < tg:
                    lo = t
                tn = (t + tg) / 2
            t = tn
        r["beta"] = t
    return r


def stats(s, r):
    """(lrt, se, p, valid) of hgibbs_firth_stats; NaN where not valid"""
    nan = (math.nan, math.nan, math.nan, False)
    if not r["flags"] & CONVERGED or r["flags"] & DEGENERATE or not r["K2"] > 0:
        return nan
    dtype = type(r["K2"]) if isinstance(r["K2"], np.floating) else np.float64
    with np.errstate(divide="ignore", invalid="ignore"):
        lrt = dtype(2) * (r["beta"] * dtype(s) - r["K"] + dtype(0.5) * np.log(r["K2"] / r["k2_0"]))
    if -1e-9 <= lrt < 0:
        lrt = dtype(0)
    if not (np.isfinite(lrt) and lrt >= 0):
        return nan
    return float(lrt), float(dtype(1) / np.sqrt(r["K2"])), math.erfc(math.sqrt(float(lrt) / 2)), True


def penalised(a, mu, s, t, dtype=np.longdouble):
    """l*(t) - l(0) up to the constant -log(K''(0)) / 2, and the modified score there"""
    a, mu = np.asarray(a, dtype), np.asarray(mu, dtype)
    K, k1, k2, k3, k4 = sums(a, mu, dtype(t), dtype)
    return dtype(t) * dtype(s) - K + np.log(k2) / 2, score(s, k1, k2, k3, k4, dtype)[0]


# ---- the inputs of the operator's tests ----
GRID_N, GRID_Q, GRID_M = R.GRID_N, R.GRID_Q, R.GRID_M
NEAR_SEPARATED, ZERO_SCORE, FLAT = 5, 7, GRID_M  # entries of the list
FLAT_C = 0.75


def fit_case(n, q):
    """spa_restate.roots_case(n, q) as it comes -- entry 3's score is three times its computed value there, which can put it outside
    (s_lo, s_hi): a score no phenotype gives, which the operator takes all the same (any finite s) and for which the rule must still end
    -- with column 5 rewritten: its carriers (genotype 1) are exactly min(6, ncase) of the cases and nobody else, B, xv and s of the
    entry formed anew; entry 7 keeps the score 0; and one more entry at the end of the list, marker 0 again with xv = (c, c, c, c) and B
    = (c, 0, ...): against the column of ones a is 0 in every row. `markers` is the list (GRID_M + 1 entries)."""
    case = R.roots_case(n, q)
    geno, Z, d, mu = case["geno"], case["Z"], case["d"], case["mu"]
    j = NEAR_SEPARATED
    geno[j] = 0
    geno[j, np.flatnonzero(d == 1.0)[:6]] = 1
    g = geno[j].astype(np.float64)
    m, sd = g.mean(), 1.0 / g.std(ddof=1)
    w = mu * (1 - mu)
    case["xv"][j] = ((0 - m) * sd, (1 - m) * sd, (2 - m) * sd, 0.0)
    case["B"][j] = np.linalg.solve(Z.T @ (Z * w[:, None]), Z.T @ (w * case["xv"][j][geno[j]]))
    case["s"][j] = np.sum(R.adjusted(geno[j], case["xv"][j], Z, case["B"][j]) * (d - mu))
    assert case["s"][ZERO_SCORE] == 0.0
    flat_b = np.zeros((1, q))
    flat_b[0, 0] = FLAT_C
    case["B"] = np.vstack([case["B"], flat_b])
    case["xv"] = np.vstack([case["xv"], np.full((1, 4), FLAT_C)])
    case["s"] = np.append(case["s"], 0.25)
    case["markers"] = np.append(np.arange(GRID_M), 0).astype(np.uint32)
    return case


def entry_a(case, e, dtype=np.float64):
    return R.adjusted(case["geno"][case["markers"][e]], case["xv"][e], case["Z"], case["B"][e], dtype)


def case_fits(case, dtype=np.float64):
    return [fit(entry_a(case, e, dtype), np.asarray(case["mu"], dtype), case["s"][e], dtype) for e in range(len(case["markers"]))]


rel = R.rel
