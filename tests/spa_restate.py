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


def shaken(sums, jitter, dtype=np.float64):
    """the reduced sums of a pass as they come, or, with jitter = (generator, eps), each times 1 + eps u, u uniform in [-1, 1]: another
    summation order's last places"""
    if jitter is None:
        return sums
    rng, eps = jitter
    return tuple(x * (dtype(1) + dtype(eps) * dtype(rng.uniform(-1.0, 1.0))) for x in sums)


def terms(a, mu, t, dtype=np.float64, jitter=None):
    """K(t), K'(t), K''(t) in the branch-free stable form"""
    one = dtype(1)
    u = a * dtype(t)
    neg = u <= 0
    E = np.expm1(-np.abs(u))
    c = np.where(neg, mu, one - mu)
    D = one + c * E
    p = np.where(neg, mu * (one + E), mu) / D
    K = np.sum(np.where(neg, dtype(0), u) + np.log1p(c * E) - u * mu)
    return shaken((K, np.sum(a * (p - mu)), np.sum(a * a * (p * (one - p)))), jitter, dtype)


def pass0(a, mu, jitter=None):
    dtype = a.dtype.type if jitter is not None else None
    k2_0, c, neg, pos = shaken((np.sum(a * a * (mu * (1 - mu))), np.sum(a * mu), np.sum(np.minimum(a, 0)), np.sum(np.maximum(a, 0))), jitter, dtype)
    return k2_0, neg - c, pos - c  # k2_0, s_lo, s_hi


# One letter per pass of a tail (roots) or an entry (firth_restate.fit), for the optional trace: the branch of the rule that the pass took.
NEWTON, STOP_RULE, MIDPOINT, DOUBLED, FIRST_STEP, SATURATED, CLOSING, OPEN = "NSMDFXCO"  # OPEN follows the last pass of a tail left open


def roots(a, mu, s, dtype=np.float64, trace=None, jitter=None):
    """the record of hgibbs_spa_roots for one marker, as a dict with the struct's fields.  trace: a list that receives one string per
    tail, a letter per pass ("" for an unreachable tail); jitter: see shaken()"""
    a, mu = np.asarray(a, dtype), np.asarray(mu, dtype)
    k2_0, s_lo, s_hi = pass0(a, mu, jitter)
    r = dict(t=[dtype(0)] * 2, K=[dtype(0)] * 2, K2=[dtype(0)] * 2, k2_0=k2_0, s_lo=s_lo, s_hi=s_hi, iters=[0, 0], flags=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = dtype(1) / np.sqrt(k2_0)
        for z in range(2):
            tau = dtype(abs(s)) if z == 0 else -dtype(abs(s))
            took = ""
            if trace is not None:
                trace.append(took)
            if not (s_lo < tau < s_hi):
                r["flags"] |= 4 << z
                continue
            lo, hi = (dtype(0), dtype(np.inf)) if z == 0 else (dtype(-np.inf), dtype(0))
            t = tau / k2_0
            closing = False
            for _ in range(PASSES):
                K, k1, k2 = terms(a, mu, t, dtype, jitter)
                r["iters"][z] += 1
                if closing:
                    r["K"][z], r["K2"][z] = K, k2
                    r["flags"] |= 1 << z
                    took += CLOSING
                    break
                g = k1 - tau
                if g > 0:
                    hi = t
                elif g < 0:
                    lo = t
                tn = t - g / k2
                if abs(tn - t) <= dtype(STOP) * max(abs(t), scale):  # the stop rule FIRST
                    closing = True
                    took += STOP_RULE
                elif not (lo < tn < hi):
                    bracketed = np.isfinite(lo) and np.isfinite(hi)
                    tn = (lo + hi) / 2 if bracketed else 2 * t
                    took += MIDPOINT if bracketed else DOUBLED
                else:
                    took += NEWTON
                t = tn
            r["t"][z] = t
            if trace is not None:
                trace[-1] = took if r["flags"] >> z & 1 else took + OPEN
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


# ---- the branches of the root rules on tiny synthetic entries: no phenotype, no null fit (also firth_restate.rule_cases) ----
RULE_N = (2, 3, 5, 16, 17, 37, 64, 261)  # the two-row handle; one full BED dword and one row into the next; the grids' two smallest
JITTERS, JITTER_EPS = 20, 1e-12  # (1e-12: the bound the GPU tests put on the sums of pass 0)


def rule_mu(n, kind):
    """the fitted probabilities of n rows: a constant, "random" in (0.02, 0.98), or "edge": those with the first row at 1e-12 and the
    last at 1 - 1e-12.  They depend on (n, kind) only, so that the entries of one cohort size share a null model"""
    if not isinstance(kind, str):
        return np.full(n, float(kind))
    mu = np.random.default_rng(77 * n + 5).uniform(0.02, 0.98, n)
    if kind == "edge":
        mu[0], mu[n - 1] = 1e-12, 1 - 1e-12
    return mu


def rule_entry(n, seed, kind, frac, xscale=1.0, missing=False, positive=False):
    """One entry against the null model Z = (1), B = 0 (so a_i = xv[code_i]) and mu = rule_mu(n, kind): a polymorphic genotype column of
    n rows from `seed`, with one missing call if asked (n >= 5); xv standardised over the called rows as --assoc-spa forms it, or
    (0, 1, 2, 0) with `positive` (no row has a negative a then), times xscale; the score at frac of s_hi, or at -frac of s_lo for frac < 0."""
    rng = np.random.default_rng(100000 * n + seed)
    g = rng.binomial(2, rng.uniform(0.05, 0.5), n).astype(np.uint8)
    if g.min() == g.max():
        g[seed % n] = 1 if g[0] != 1 else 0
    if missing and n >= 5:
        g[rng.integers(0, n)] = 3
        called = np.flatnonzero(g != 3)
        if g[called].min() == g[called].max():
            g[called[0]] = 1 if g[called[0]] != 1 else 0
    c = g[g != 3].astype(np.float64)
    m, sd = c.mean(), 1.0 / c.std(ddof=1)
    xv = np.array((0.0, 1.0, 2.0, 0.0) if positive else ((0 - m) * sd, (1 - m) * sd, (2 - m) * sd, 0.0)) * xscale
    mu = rule_mu(n, kind)
    _, s_lo, s_hi = pass0(xv[g], mu)
    return dict(n=n, kind=kind, geno=g, mu=mu, xv=xv, s=float(frac * s_hi if frac >= 0 else -frac * s_lo))


def rule_groups(entries):
    """the entries of one list as cases in the form of roots_case / fit_case, one per (n, kind): what one handle and one call take"""
    cases = {}
    for e in entries:
        cases.setdefault((e["n"], str(e["kind"])), []).append(e)
    return [dict(n=n, geno=np.array([e["geno"] for e in es]), Z=np.ones((n, 1)), mu=es[0]["mu"], B=np.zeros((len(es), 1)),
                 xv=np.array([e["xv"] for e in es]), s=np.array([e["s"] for e in es]), markers=np.arange(len(es), dtype=np.uint32))
            for (n, _), es in cases.items()]


def case_size(case):
    return len(case["s"])


def traced(run, a, mu, s, dtype=np.float64, jitter=None):
    """(record, trace) of run = roots or firth_restate.fit; the trace of roots is the pair of its tails'"""
    trace = []
    r = run(np.asarray(a, dtype), np.asarray(mu, dtype), s, dtype, trace=trace, jitter=jitter)
    return r, tuple(trace)


def admission(run, a, mu, s):
    """None where the entry is well conditioned for `run`, else the reason it is not: the float64 and the longdouble rule take the same
    branch in every pass and set the same flags, no tail or entry is left open, and all that also under JITTERS seeded relative
    perturbations of size JITTER_EPS of every reduced sum, in both precisions"""
    r64, t64 = traced(run, a, mu, s)
    r80, t80 = traced(run, a, mu, s, np.longdouble)
    if any(OPEN in t for t in t64):
        return "open in float64 (%s)" % (t64,)
    if t64 != t80 or r64["flags"] != r80["flags"]:
        return "float64 %s flags %d, longdouble %s flags %d" % (t64, r64["flags"], t80, r80["flags"])
    for k in range(JITTERS):
        for dtype in (np.float64, np.longdouble):
            r, t = traced(run, a, mu, s, dtype, (np.random.default_rng(k), JITTER_EPS))
            if t != t64 or r["flags"] != r64["flags"]:
                return "jitter %d in %s: %s flags %d, not %s flags %d" % (k, dtype.__name__, t, r["flags"], t64, r64["flags"])
    return None


# (n, seed, kind, frac, xscale, missing, positive) of rule_entry; behind each the float64 traces of the two tails.  A tail whose first
# Newton step overshoots the root finds K' - tau > 0 there, the bracket closes and the midpoints follow: small mu and a score well up
# the range.  An entry with both ends of the range on one side of |s| has one unreachable tail.
# How they were chosen: seeds below 100 are hand-picked plain entries; the others are the first hits of a random draw over
# (n in RULE_N, seed < 1000, kind, frac in +-{0.05 .. 0.9999}, xscale in {1, 3, 10}, missing, positive) whose float64 trace held a letter
# other than N, S, C and for which admission() returned None.  Should an entry stop being admitted (another NumPy, another libm), draw
# again in the same way and replace it: the CPU test names the entry and admission() gives the reason.
ADMITTED = (
    (2, 496, 0.01, -0.3, 1.0, False, False),  # MMNNNSC MMNNNSC
    (2, 676, 0.08, 0.6, 1.0, True, True),  # MNNNNSC -
    (2, 11, "random", 0.3, 1.0, False, False),  # NNNSC NNSC
    (3, 80, 0.01, 0.999, 3.0, False, False),  # MMNNNNNNNSC MMMNNNNNNNSC
    (3, 849, 0.08, 0.99, 1.0, True, True),  # MNNNNNSC -
    (3, 12, "random", 0.0, 1.0, False, False),  # SC SC: the score 0, t = 0 is an end of the bracket
    (5, 525, 0.01, -0.9, 3.0, True, False),  # MMMNNNNNSC MMMNNNNNSC
    (5, 13, "edge", 0.3, 1.0, True, False),  # NNNSC NNNSC
    (16, 379, 0.08, 0.999, 10.0, False, True),  # MNNNNNNNSC -
    (16, 706, 0.92, -0.99, 10.0, False, True),  # - MNNNNNSC
    (16, 14, "edge", -0.3, 1.0, False, False),  # NNNNNSC NNNSC
    (17, 430, 0.01, 0.3, 10.0, True, False),  # MMNNNNSC MMNNNNSC
    (17, 813, 0.01, 0.6, 1.0, False, True),  # MMMNNNNSC -
    (17, 15, "random", 0.6, 1.0, True, False),  # NNNSC NNSC
    (37, 369, 0.01, -0.99, 10.0, True, False),  # MMMNNNNNSC MNNNNSC
    (37, 198, 0.92, -0.9, 3.0, False, True),  # - MNNNNNSC
    (37, 16, "edge", 0.05, 1.0, True, False),  # NNNSC NNNSC
    (64, 71, 0.01, -0.6, 1.0, True, False),  # MMMNNNSC NNNNNNSC
    (64, 249, 0.01, 0.6, 1.0, True, True),  # MMMNNNNSC -
    (64, 17, "random", 0.0, 3.0, True, False),  # SC SC
    (261, 963, 0.01, -0.99, 1.0, False, False),  # MMMNNNNNSC MNNNNSC
    (261, 18, "random", -0.6, 1.0, True, False),  # NNNNSC NNNNNSC
    (261, 19, "edge", 0.3, 1.0, True, False),  # NNSC NNNSC
)

# What only properties can be asked of: scores a hair inside the reachable edge (the root lies where every row has saturated and K'' is a
# rounding error: this is where 2 t is taken, after a K'' of exactly 0 -- with a K'' > 0 and the bracket (0, inf) resp. (-inf, 0) a
# Newton step from inside it towards tau stays inside it, so well-conditioned input cannot reach that branch); xv times 300, whose first
# Newton step saturates every row; and entries that the float64 rule leaves open.
EDGE_FRACS = (1 - 1e-9, 1 - 1e-13, -(1 - 1e-9), -(1 - 1e-13))
ILL = tuple((n, 100 + k, kind, f, 1.0, k % 2 == 1, False)
            for k, (n, kind) in enumerate(((2, 0.5), (5, 0.08), (16, "random"), (17, "edge"), (37, 0.92), (64, "random"), (261, "edge"), (3, 0.01)))
            for f in EDGE_FRACS[k % 2::2]) + (
    (5, 120, 0.01, 0.99, 300.0, False, False), (17, 121, 0.01, 0.99, 300.0, True, True), (37, 122, 0.01, 0.99, 300.0, False, True),
    (261, 123, 0.01, 0.99, 300.0, True, False), (64, 124, 0.01, 0.999, 300.0, False, True),  # SATURATING: the last five before the open ones
    (37, 643, "edge", 0.999, 1.0, False, False),  # open in float64
    # further tails that take 2 t in float64 (one of the entries above does): DNNNNM..O, NNDDDM..O, NNNDM..SC, NNNNNNDM..SC
    (5, 218, "edge", 1 - 1e-9, 1.0, True, False), (17, 713, "edge", 1 - 1e-13, 1.0, True, False),
    (17, 483, "edge", -(1 - 1e-13), 1.0, True, False), (64, 667, "edge", 1 - 1e-9, 1.0, True, False),
)


def rule_cases():
    """(admitted, ill-conditioned): two lists of cases in the form of roots_case, each entry of which tests/test_spa_restatement_cpu.py
    holds to admission() resp. to its place in the second list"""
    return rule_groups([rule_entry(*spec) for spec in ADMITTED]), rule_groups([rule_entry(*spec) for spec in ILL])


# ---- the edges of q and n that the ABI takes ----
# q = 64 = SPA_QMAX fills the kernels' b from exactly one wave and is 16 full trips of the four-fold unrolled product; 63 and 4 lie on
# either side of a trip's end; n = 2 is the smallest handle, 16 and 17 one full BED dword and one row into the next.
EDGE_SHAPES = tuple((n, q) for n in (37, 261) for q in (4, 63, 64)) + tuple((n, 1) for n in (2, 16, 17))
EDGE_M = 16


def edge_case(n, q):
    """EDGE_M entries in the form of roots_case with random finite Z, B and xv (nothing of a null fit: a_i is whatever they give), mu
    random in (0.02, 0.98), polymorphic columns with a missing call in every fourth where n >= 5, and scores between 0.05 and 0.6 of
    either end of the reachable range, entry 3 at 0"""
    rng = np.random.default_rng(9000 + 100 * n + q)
    geno = rng.binomial(2, rng.uniform(0.1, 0.5, (EDGE_M, 1)), size=(EDGE_M, n)).astype(np.uint8)
    for j in range(EDGE_M):
        if geno[j].min() == geno[j].max():
            geno[j, j % n] = 1 if geno[j, 0] != 1 else 0
        if j % 4 == 0 and n >= 5:
            geno[j, (3 * j + 2) % n] = 3
    Z = rng.standard_normal((n, q))
    mu = rng.uniform(0.02, 0.98, n)
    B = 0.3 * rng.standard_normal((EDGE_M, q))
    xv = rng.standard_normal((EDGE_M, 4))
    s = np.zeros(EDGE_M)
    for j in range(EDGE_M):
        _, s_lo, s_hi = pass0(adjusted(geno[j], xv[j], Z, B[j]), mu)
        f = rng.uniform(0.05, 0.6)
        s[j] = f * s_hi if j % 2 == 0 else f * s_lo
    s[3] = 0.0
    return dict(n=n, geno=geno, Z=Z, mu=mu, B=B, xv=xv, s=s, markers=np.arange(EDGE_M, dtype=np.uint32))


def case_a(case, e, dtype=np.float64):
    return adjusted(case["geno"][case["markers"][e]], case["xv"][e], case["Z"], case["B"][e], dtype)


def rel(a, b):
    a, b = float(a), float(b)
    return 0.0 if a == b else abs(a - b) / max(abs(a), abs(b))
