"""A NumPy restatement of hgibbs_firth_fit and hgibbs_firth_stats, not a test: the sums of a pass, the root
rule and the statistics, in float64 or longdouble; and the inputs that the CPU and GPU tests of the operator share, so that the
tolerance measured on the CPU is measured on the entries the GPU tests use."""
import math

import numpy as np

import spa_restate as R

STOP = 1e-9
PASSES = 64
CONVERGED, DEGENERATE = 1, 2


def sums(a, mu, t, dtype=np.float64, jitter=None):
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
    return R.shaken((K, np.sum(a * (p - mu)), np.sum(a2 * v), np.sum((a2 * a) * (v * (one - dtype(2) * p))),
                     np.sum((a2 * a2) * (v * (one - dtype(6) * v)))), jitter, dtype)


def score(s, k1, k2, k3, k4, dtype=np.float64):
    """the modified score g and its derivative from the sums at one point"""
    half = dtype(0.5)
    r = k3 / k2
    return dtype(s) - k1 + half * r, -k2 + half * (k4 / k2 - r * r)


def fit(a, mu, s, dtype=np.float64, trace=None, jitter=None):
    """the record of hgibbs_firth_fit for one entry, as a dict with the struct's fields.  trace: a list that receives one string, a
    letter of spa_restate per pass after pass 0 ("" for a degenerate entry); jitter: see spa_restate.shaken()"""
    a, mu = np.asarray(a, dtype), np.asarray(mu, dtype)
    zero = dtype(0)
    r = dict(beta=zero, K=zero, K2=zero, g=zero, k2_0=zero, iters=0, flags=0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t, tg, lo, hi = zero, zero, dtype(-np.inf), dtype(np.inf)
        closing = False
        scale = zero
        took = ""
        for it in range(PASSES + 1):
            K, k1, k2, k3, k4 = sums(a, mu, t, dtype, jitter)
            if it == 0:
                if not (np.isfinite(k2) and k2 > 0):
                    r["flags"] = DEGENERATE
                    if trace is not None:
                        trace.append(took)
                    return r
                r["k2_0"] = k2
                scale = dtype(1) / np.sqrt(k2)
            else:
                r["iters"] += 1
            if closing:
                r["K"], r["K2"] = K, k2
                r["flags"] |= CONVERGED
                took += R.CLOSING
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
                if gp < 0 and abs(tn - t) <= dtype(STOP) * max(abs(t), scale):  # the stop rule FIRST, and only where g falls
                    closing = True
                    took += R.STOP_RULE
                elif not (lo < tn < hi):
                    if np.isfinite(lo) and np.isfinite(hi):
                        tn = (lo + hi) / 2
                        took += R.MIDPOINT
                    elif t == 0:
                        tn = scale if g > 0 else -scale
                        took += R.FIRST_STEP
                    else:
                        tn = 2 * t
                        took += R.DOUBLED
                else:
                    took += R.NEWTON
            else:  # the probabilities have saturated: back towards the last good point, no sign taken
                if t > tg:
                    hi = t
                elif t < tg:
                    lo = t
                tn = (t + tg) / 2
                took += R.SATURATED
            t = tn
        r["beta"] = t
        if trace is not None:
            trace.append(took if r["flags"] & CONVERGED else took + R.OPEN)
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


# ---- the branches of the rule on tiny synthetic entries (spa_restate.rule_entry) ----
# Behind each the float64 trace.  F: with few rows and a small mu the penalty outweighs the likelihood at 0, g' (0) > 0 and Newton's
# step points away from the root.  X: mu = 2^-k (1 - mu is exact, so a saturated row's p is exactly 1 in both precisions), no negative
# a, and a first Newton step past 45 / min a: K'' = 0 and g is 0 / 0.  D: a step past the open end's side that the signs of g allow.
# Chosen as spa_restate.ADMITTED was (the X entries from a draw over mu in {2^-6, 2^-7, 2^-8} with `positive`), and replaced the same way.
ADMITTED = (
    (2, 85, 0.92, 0.6, 1.0, False, False),  # FNNSC
    (2, 612, 0.01, 0.3, 1.0, True, False),  # FMNNNNSC
    (2, 805, 0.00390625, 0.05, 10.0, False, True),  # NXMMMNNNSC
    (3, 582, 0.01, 0.05, 1.0, False, False),  # FMNNNNSC
    (3, 746, 0.01, -0.99, 1.0, False, True),  # NMMNNNNNNSC
    (3, 186, 0.00390625, 0.05, 1.0, True, True),  # NXMMMNNNSC
    (5, 703, 0.01, -0.6, 1.0, True, False),  # FNNNNNSC
    (5, 45, 0.01, 0.9999, 1.0, False, False),  # FMNNNNSC
    (5, 761, 0.92, 0.3, 1.0, True, False),  # NDDDNNNNSC
    (5, 870, 0.015625, 0.99, 1.0, True, True),  # NXMMNNNNNSC
    (16, 447, 0.01, 0.99, 3.0, False, False),  # FNNNNNNSC
    (16, 680, 0.01, -0.9, 3.0, True, False),  # FNMNNNNSC
    (16, 886, 0.01, 0.9, 3.0, False, False),  # FNNNNDNMNNNSC
    (16, 980, 0.015625, 0.9999, 10.0, False, True),  # NXMMNNNNNSC
    (17, 999, 0.01, 0.05, 1.0, True, False),  # FNNNNSC
    (17, 602, 0.01, -0.9999, 1.0, False, False),  # FNMMNNNNNSC
    (17, 430, "random", -0.9, 3.0, False, False),  # NNNNDNNNSC
    (17, 505, 0.015625, 0.99, 3.0, True, True),  # NXMMNNNNSC
    (37, 738, 0.01, 0.6, 1.0, False, False),  # FNMNNNSC
    (37, 64, 0.01, -0.6, 1.0, False, True),  # NMMNNNNNSC
    (37, 841, 0.01, 0.999, 1.0, True, False),  # FNDNNNNNNNSC
    (37, 335, 0.0078125, 0.999, 10.0, False, True),  # NXXMMNNNNSC
    (37, 16, "random", 0.05, 1.0, True, False),  # NNNNNSC
    (64, 543, 0.01, 0.9, 3.0, True, False),  # FNNNNNSC
    (64, 630, 0.01, 0.05, 10.0, False, True),  # NMNNNNSC
    (64, 324, 0.0078125, 0.9, 10.0, False, True),  # NXXMMNNNNNSC
    (64, 17, "edge", 0.0, 1.0, True, False),  # NNSC
    (261, 623, 0.01, -0.9999, 3.0, True, False),  # NMMMNNNNSC
    (261, 692, 0.015625, 0.999, 1.0, False, True),  # NXMMNNNNNNNSC
    (261, 18, "random", -0.6, 1.0, True, False),  # NNNNNNSC
    (261, 19, "edge", 0.3, 1.0, True, False),  # NNNSC
)
# Entries next to a local MINIMUM of the penalised likelihood: g'(0) > 0 as for F, and a score that leaves g(0) at 1e-10 of the penalty's
# slope K'''(0) / (2 K''(0)).  Newton's proposal lies 1e-10 scale or so from 0, on the wrong side of the bracket end there.  A stop rule
# without "g' < 0" closed such an entry in its first pass, converged and valid at the minimum; the rule goes to +-scale and on to the
# maximum on that side.
NEAR_MINIMUM = ((3, 582, 0.01, False), (5, 45, 0.01, False), (5, 703, 0.01, True))  # FMNNNNNSC, FMNNNNNNSC, FMNNNNNSC
NEAR_MINIMUM_EPS = 1e-10

# Only properties can be asked of these: the scores a hair inside the reachable edge and beyond it (any finite s is taken), xv times 300
# (the first Newton step saturates every row), and entries that the float64 rule leaves open.
ILL = tuple((n, 100 + k, kind, f, 1.0, k % 2 == 1, False)
            for k, (n, kind) in enumerate(((2, 0.5), (5, 0.08), (16, "random"), (17, "edge"), (37, 0.92), (64, "random"), (261, "edge"), (3, 0.01)))
            for f in ((1 - 1e-9, -(1 - 1e-13), 1.2, -1.5, 10.0) if k % 2 == 0 else (-(1 - 1e-9), 1 - 1e-13, -1.2, 1.5, -10.0))) + (
    (64, 125, 0.01, 0.99, 300.0, True, False), (261, 126, 0.01, 0.999, 300.0, False, True), (64, 127, 0.01, 0.99, 300.0, False, True),
    (261, 123, 0.01, 0.99, 300.0, True, False), (64, 124, 0.01, 0.999, 300.0, False, True),  # SATURATING: the last five before the open ones
    (37, 643, "edge", 0.999, 1.0, False, False), (16, 183, "edge", 0.999, 1.0, False, False), (64, 82, "edge", -0.9999, 30.0, False, False),  # open in float64
)


def near_minimum_entry(n, seed, kind, missing):
    e = R.rule_entry(n, seed, kind, 0.0, 1.0, missing)
    _, _, k2, k3, _ = sums(e["xv"][e["geno"]], e["mu"], 0.0)
    e["s"] = float(-0.5 * (k3 / k2) * (1 - NEAR_MINIMUM_EPS))
    return e


def rule_cases():
    """(admitted, ill-conditioned): two lists of cases in the form of fit_case, each entry of which tests/test_firth_restatement_cpu.py
    holds to spa_restate.admission() resp. to its place in the second list"""
    admitted = [R.rule_entry(*spec) for spec in ADMITTED] + [near_minimum_entry(*spec) for spec in NEAR_MINIMUM]
    return R.rule_groups(admitted), R.rule_groups([R.rule_entry(*spec) for spec in ILL])


def stationary(a, mu, s, rec):
    """whether rec's point is a stationary point and a local maximum of the penalised likelihood in longdouble, to the bounds of
    test_the_point_is_stationary_and_a_local_maximum_in_longdouble"""
    scale = 1.0 / math.sqrt(rec["k2_0"])
    top, g = penalised(a, mu, s, rec["beta"])
    return bool(abs(g) <= 1e-6 * math.sqrt(rec["k2_0"]) and all(top >= penalised(a, mu, s, rec["beta"] + step)[0] for step in (-1e-3 * scale, 1e-3 * scale)))


rel = R.rel
