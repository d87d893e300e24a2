"""A NumPy restatement of hgibbs_set_gram, hgibbs_set_tests and the set statistics of --assoc-sets, not a test:
the raw sums as Python integers, out, Phi, the weights and both statistics, in float64 or longdouble; and the inputs that the CPU and
GPU tests share, so that a tolerance measured on the CPU is measured on the entries the GPU tests use.  Independent of the library."""
import math

import numpy as np

STOP = 1e-9
PASSES = 64
EIG_KEEP = 1e-10
LIMIT = 1e-6
BURDEN_GUARD = 1e-9


# ---- section 1: the operator ---------------------------------------------------------------------------------------------------

def quantise(w):
    """E = 52 - e with max w < 2^e (0 for an all-zero w), q = rint(w 2^E) as int64"""
    m = float(np.max(w)) if w.size else 0.0
    E = 52 - int(np.frexp(m)[1]) if m > 0 else 0
    return E, np.rint(np.ldexp(np.asarray(w, np.float64), E)).astype(np.int64)


def weighted_products(A, q, B):
    """A (ma, n), B (mb, n) small non-negative integers as f64, q (n,) int64 -> (ma, mb) Python ints sum_i q_i A_ai B_bi, exact: q in
    26-bit halves so that every f64 product sum stays below 2^53"""
    lo = ((A * (q & ((1 << 26) - 1)).astype(np.float64)) @ B.T).astype(np.int64).astype(object)
    hi = ((A * (q >> 26).astype(np.float64)) @ B.T).astype(np.int64).astype(object)
    return hi * (1 << 26) + lo


def raw_integers(geno, idx, w):
    """E and the (m, m) arrays of Python ints GG, GC, CC for the listed markers of geno (M, n; codes 0..3, 3 a missing call)"""
    E, q = quantise(w)
    codes = geno[np.asarray(idx, dtype=np.int64)]
    c = (codes != 3).astype(np.float64)
    g = np.where(codes == 3, 0, codes).astype(np.float64)
    return E, weighted_products(g, q, g), weighted_products(g, q, c), weighted_products(c, q, c)


_to_f = np.vectorize(float, otypes=[np.float64])  # Python's int -> float rounds to nearest even once


def raw_floats(geno, idx, w):
    """(m, m, 3) f64: each exact sum rounded ONCE, times 2^-E"""
    E, GG, GC, CC = raw_integers(geno, idx, w)
    return np.stack([np.ldexp(_to_f(x), -E) for x in (GG, GC, CC)], axis=2)


def marker_stats(geno, dtype=np.float64):
    """mave, mstd of the chain's standardisation from the counts, per marker; mstd is not finite for a marker without variance"""
    N = geno.shape[1]
    n1, n2, nm = [np.count_nonzero(geno == c, axis=1).astype(dtype) for c in (1, 2, 3)]
    n0 = dtype(N) - n1 - n2 - nm
    with np.errstate(divide="ignore", invalid="ignore"):
        av = (n1 + dtype(2) * n2) / (dtype(N) - nm)
        ss = n0 * (dtype(0) - av) ** 2 + n1 * (dtype(1) - av) ** 2 + n2 * (dtype(2) - av) ** 2
        sd = np.sqrt(dtype(N - 1) / ss)
    return av, sd


def gram_out(raw, mave, mstd, dtype=np.float64):
    """out from the rounded sums in the operator's order; raw (m, m, 3), mave and mstd of the listed markers (m,).  Also returns the
    sum of the absolute values of the four terms times |sd_a sd_b|: the scale an error of the combination is measured against."""
    raw = np.asarray(raw, dtype)
    ma, sd = np.asarray(mave, dtype), np.asarray(mstd, dtype)
    GG, GC, CC = raw[:, :, 0], raw[:, :, 1], raw[:, :, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        t1, t2, t3 = ma[None, :] * GC, ma[:, None] * GC.T, (ma[:, None] * ma[None, :]) * CC
        ss = sd[:, None] * sd[None, :]
        out = ss * (((GG - t1) - t2) + t3)
        scale = np.abs(ss) * (np.abs(GG) + np.abs(t1) + np.abs(t2) + np.abs(t3))
    ok = np.isfinite(sd)[:, None] & np.isfinite(sd)[None, :]
    return np.where(ok, out, dtype(np.nan)), np.where(ok, scale, dtype(np.nan))


def gram_direct(geno, idx, w, dtype=np.longdouble):
    """sum_i w_i x_ia x_ib with the standardised x formed directly (0 at a missing call): what out stands for"""
    av, sd = marker_stats(geno, dtype)
    codes = geno[np.asarray(idx, dtype=np.int64)]
    with np.errstate(invalid="ignore"):
        x = np.where(codes == 3, dtype(0), (codes.astype(dtype) - av[idx][:, None]) * sd[idx][:, None])
        return (x * np.asarray(w, dtype)) @ x.T


def rounding_bound(n, E):
    """the error of GG, GC, CC from the rounding of w, before the one rounding of each sum"""
    return np.array([2.0 * n, 1.0 * n, 0.5 * n]) * 2.0 ** -E


# ---- section 2: the statistics -------------------------------------------------------------------------------------------------

def cgf(lam, z, dtype):
    d = dtype(1) - dtype(2) * z * lam
    r = lam / d
    return np.sum(-np.log1p(-dtype(2) * z * lam)) / dtype(2), np.sum(r), np.sum(dtype(2) * r * r)


def skat_tail(lam, Q, dtype=np.float64):
    """(p, ok): the saddlepoint tail of sum lam chi^2_1 at Q, lam sorted descending; or the limit near the mean"""
    lam = np.asarray(lam, dtype)
    Q = dtype(Q)
    s1, s2, s3 = np.sum(lam), np.sum(lam * lam), np.sum(lam * lam * lam)
    k2_0 = dtype(2) * s2
    sd = np.sqrt(k2_0)
    if abs(Q - s1) < dtype(LIMIT) * sd:
        return dtype(0.5) * erfc(dtype(8) * s3 / (k2_0 * sd) / (dtype(6) * np.sqrt(dtype(2))), dtype), True  # the form's own limit
    fallback = dtype(0.5) * dtype(math.erfc(float((Q - s1) / sd) / math.sqrt(2.0)))
    scale, pole = dtype(1) / sd, dtype(1) / (dtype(2) * lam[0])
    lo, hi = (dtype(0), pole) if Q > s1 else (dtype(-np.inf), dtype(0))
    z = (Q - s1) / k2_0
    if not (lo < z < hi):
        z = (lo + hi) / 2 if np.isfinite(lo) and np.isfinite(hi) else 2 * z
    done = False
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for _ in range(PASSES):
            K, K1, K2 = cgf(lam, z, dtype)
            f = K1 - Q
            if f > 0:
                hi = z
            elif f < 0:
                lo = z
            zn = z - f / K2
            if abs(zn - z) <= dtype(STOP) * max(abs(z), scale):  # the stop rule FIRST
                if not zn < pole:
                    return fallback, False
                z = zn
                K, K1, K2 = cgf(lam, z, dtype)
                done = True
                break
            if not (lo < zn < hi):
                zn = (lo + hi) / 2 if np.isfinite(lo) and np.isfinite(hi) else 2 * z
            z = zn
        if not done:
            return fallback, False
        h = z * Q - K
        if not (h > 0 and K2 > 0):
            return fallback, False
        w = (-1 if z < 0 else 1) * np.sqrt(dtype(2) * h)
        v = z * np.sqrt(K2)
        if not v / w > 0:
            return fallback, False
        x = w + np.log(v / w) / w
        if not np.isfinite(x):  # (no sign rule: between the median and the mean x > 0 while z < 0)
            return fallback, False
    return dtype(0.5) * erfc(x / np.sqrt(dtype(2)), dtype), True


def switch_bound(lam, sig=2e-6):
    """how far the limit and the formula `sig` standard deviations from the mean may lie apart.  The tail moves by at most 0.4 per
    standard deviation (the normal density's peak): 0.4 (sig + 1e-6).  z Q - K is the difference of two numbers of size
    delta mean / K''(0) that leaves delta^2 / (2 K''(0)), delta = sig sd.  Four roundings of 2^-53 of that size enter it (Q's own, the
    product z Q, the terms of K, their sum), so its relative error is 2^-52 4 mean / delta; half of it goes to w, stays in
    log(v / w) as an absolute error and is divided by w = sig: 2^-52 2 (mean / sd) / sig^2 in the argument, times 0.4."""
    lam = np.asarray(lam, np.float64)
    mean, sd = float(np.sum(lam)), math.sqrt(2.0 * float(np.sum(lam * lam)))
    return 0.4 * (sig + 1e-6) + 0.4 * 2.0 ** -52 * 2.0 * (mean / sd) / sig ** 2


def erfc(x, dtype):
    """math.erfc in both precisions: NumPy has none in longdouble, and the tests compare p at 1e-8, far above float64's last places"""
    return dtype(math.erfc(float(x)))


def set_tests(U, Phi, a, dtype=np.float64):
    """the fields of hgibbs_set_result as a dict; the eigenvalues by LAPACK in float64 (there is none in longdouble)"""
    U, Phi, a = np.asarray(U, dtype), np.asarray(Phi, dtype), np.asarray(a, dtype)
    nan = dtype(np.nan)
    r = dict(q=nan, p_skat=nan, t_burden=nan, p_burden=nan, lam_sum=nan, lam_max=nan, neig=0, skat_ok=0)
    den = a @ (Phi @ a)
    if den > dtype(BURDEN_GUARD) * np.sum(a * a * np.diag(Phi)):
        r["t_burden"] = np.sum(a * U) ** 2 / den
        r["p_burden"] = dtype(math.erfc(math.sqrt(float(r["t_burden"]) / 2.0)))
    A = (a[:, None] * Phi * a[None, :]).astype(np.float64)
    ev = np.sort(np.linalg.eigvalsh((A + A.T) / 2.0))[::-1]
    lam = ev[ev > EIG_KEEP * ev[0]] if ev[0] > 0 else ev[:0]
    r["neig"] = int(lam.size)
    if lam.size == 0:
        return r
    lam = lam.astype(dtype)
    r["q"] = np.sum((a * U) ** 2)
    r["lam_sum"], r["lam_max"] = np.sum(lam), lam[0]
    p, ok = skat_tail(lam, r["q"], dtype)
    r["p_skat"], r["skat_ok"] = p, int(ok)
    return r


def chi2_tail(x, df):
    """P(chi^2_df >= x) in closed form: erfc for 1 df, the finite sum e^(-x/2) sum_{i<k} (x/2)^i / i! for df = 2 k"""
    if df == 1:
        return math.erfc(math.sqrt(x / 2.0))
    assert df % 2 == 0
    term, total = 1.0, 0.0
    for i in range(df // 2):
        total += term
        term *= (x / 2.0) / (i + 1)
    return math.exp(-x / 2.0) * total


# ---- section 3: the weights and Phi of --assoc-sets ------------------------------------------------------------------------------

def beta_weights(maf, A=1.0, B=25.0):
    """a_j = dbeta(MAF_j; A, B) by lgamma"""
    c = math.lgamma(A + B) - math.lgamma(A) - math.lgamma(B)
    return np.array([math.exp(c + (A - 1.0) * math.log(p) + (B - 1.0) * math.log1p(-p)) if 0.0 < p < 1.0 else
                     (math.exp(c) if (p == 0.0 and A == 1.0) else 0.0) for p in np.asarray(maf, np.float64)])


def phi_per_copy(out, Lt, sd, dtype=np.float64):
    """Phi^g_jk = (out_jk - (L^-1 t_j).(L^-1 t_k)) / (sd_j sd_k); Lt (m, q) the rows L^-1 t_j of the per-marker pass"""
    out, Lt, sd = np.asarray(out, dtype), np.asarray(Lt, dtype), np.asarray(sd, dtype)
    return (out - Lt @ Lt.T) / (sd[:, None] * sd[None, :])


# ---- shared inputs ------------------------------------------------------------------------------------------------------------

SET_SIZES = (1, 15, 16, 17, 33)
GRID_N = (37, 63, 64, 65, 257, 1000)
GRID_M = 90
MONO, ALLMISS = 44, 61  # a monomorphic marker and a column missing in every row; both lie in the set of 33


def genotypes(n, M, seed, missing):
    """codes (M, n): binomial(2, p_j) with mixed allele frequencies, rare ones among them; with `missing`, 1 % missing calls in
    every third column and at least one in each of them"""
    rng = np.random.default_rng(seed)
    p = np.where(np.arange(M) % 2 == 0, rng.uniform(0.02, 0.1, M), rng.uniform(0.1, 0.5, M))
    geno = rng.binomial(2, p[:, None], size=(M, n)).astype(np.uint8)
    for j in range(M):  # no accidental monomorphic column
        if np.all(geno[j] == geno[j, 0]):
            geno[j, j % n] = (geno[j, 0] + 1) % 3
    if missing:
        for j in range(0, M, 3):
            geno[j, rng.random(n) < 0.01] = 3
            geno[j, (7 * j) % n] = 3
    return geno


def grid_case(n, missing):
    """the cohort of n rows of the operator's grid: genotypes, the sets (non-contiguous, descending and ascending lists) and w"""
    geno = genotypes(n, GRID_M, 100 + n + (1 if missing else 0), missing)
    geno[MONO] = 1
    if missing:
        geno[ALLMISS] = 3
    rng = np.random.default_rng(n)
    sets = [np.array([GRID_M - 1]),                                     # 1
            np.arange(GRID_M - 2, GRID_M - 2 - 30, -2),                 # 15, descending, every other marker
            rng.permutation(GRID_M)[:16],                               # 16, any order
            np.arange(3, 3 + 17 * 5, 5),                                # 17, ascending, stride 5
            np.concatenate([[MONO, ALLMISS], np.setdiff1d(np.arange(GRID_M - 1, GRID_M - 40, -1), [MONO, ALLMISS])[:31][::-1]])]  # 33
    assert tuple(len(s) for s in sets) == SET_SIZES
    mu = rng.uniform(0.02, 0.98, n)
    return dict(geno=geno, sets=[np.asarray(s, dtype=np.uint32) for s in sets], w=mu * (1.0 - mu))


def big_case(missing):
    """one set of 1024 markers on 257 rows, in descending order with gaps"""
    n, M = 257, 1100
    geno = genotypes(n, M, 7 + (1 if missing else 0), missing)
    rng = np.random.default_rng(5)
    idx = np.sort(rng.permutation(M)[:1024])[::-1]
    mu = rng.uniform(0.02, 0.98, n)
    return dict(geno=geno, sets=[np.asarray(idx, dtype=np.uint32)], w=mu * (1.0 - mu))


# The largest |float64 - longdouble| of out over the grid below (every grid_case and big_case(True)), relative to the sum of the
# absolute terms of the combination, as tests/test_settest_restatement_cpu.py measures and prints it: 3.85e-16.  The GPU test asserts
# ten times this.
OUT_F64_LD = 3.9e-16


def measure_out_tolerance(cases):
    """the largest |float64 - longdouble| of out over the cases, relative to the sum of the absolute terms of the combination"""
    worst = 0.0
    for case in cases:
        av64, sd64 = marker_stats(case["geno"], np.float64)
        avl, sdl = marker_stats(case["geno"], np.longdouble)
        for idx in case["sets"]:
            raw = raw_floats(case["geno"], idx, case["w"])
            o64, _ = gram_out(raw, av64[idx], sd64[idx], np.float64)
            ol, scale = gram_out(raw, avl[idx], sdl[idx], np.longdouble)
            ok = np.isfinite(ol) & (scale > 0)
            if ok.any():
                worst = max(worst, float(np.max(np.abs(o64[ok] - ol[ok]) / scale[ok])))
    return worst


# the spectra of the statistics' grid: name -> eigenvalues (descending)
def spectra():
    rng = np.random.default_rng(11)
    return {
        "one": np.array([1.7]),
        "two_mixed": np.array([3.0, 0.4]),
        "five": np.sort(rng.uniform(0.1, 2.0, 5))[::-1],
        "forty_decay": 2.0 * 0.85 ** np.arange(40),
        "two_hundred": np.sort(rng.gamma(0.5, 1.0, 199) + 1e-3)[::-1],
    }


SIGMAS = (-0.5, -0.1, 0.0, 0.3, 1.0, 2.0, 4.0, 8.0, 12.0, 20.0)
EQUAL_DF = (1, 2, 40, 200)


def q_at(lam, sig):
    """Q at `sig` standard deviations from the mean of sum lam chi^2_1"""
    lam = np.asarray(lam, np.float64)
    return float(np.sum(lam) + sig * math.sqrt(2.0 * np.sum(lam * lam)))


def matrix_with_spectrum(lam, seed):
    """a symmetric matrix with the eigenvalues lam in a random orthogonal basis"""
    lam = np.asarray(lam, np.float64)
    Qm, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((lam.size, lam.size)))
    A = (Qm * lam) @ Qm.T
    return (A + A.T) / 2.0


def scores_for(m, Q):
    """m scores with sum U^2 = Q, not all equal"""
    u = 1.0 + 0.3 * np.cos(np.arange(m))
    return u * math.sqrt(Q / float(np.sum(u * u)))
