"""A restatement of the epistasis path in numpy, for the tests: a helper, not a test.

  tables      the 2 x 3 x 3 tables of pairs of markers as exact integer sums over the rows
  ksa         BOOST's Kirkwood superposition bound, hg_epi_math.h's operations in their order, in float64 or np.longdouble
  ipf_lr      the likelihood-ratio statistic of the homogeneous-association model by iterative proportional fitting, hg_epi.cpp's
              operations in their order with its pinned stopping rule (EPI_TOL, EPI_CYCLES)
  df, tail    the degrees of freedom and the closed-form chi-square tails
  delta       the screen's slack as a function of the rows
  the grid of tables, the planted cohort and the second cohort of the GPU tests, and the .epi.cc table of a cohort
"""
import math

import numpy as np

EPI_TOL = 1e-10     # a cycle in which no cell moves by more than EPI_TOL n ends the fit
EPI_CYCLES = 2000   # the cap: converged = 0 when it is hit

# Ten times the largest |float64 - longdouble| of KSA over grid_tables(), relative to the sum of the absolute terms
# sum n_ijk (|log(n_ijk / n)| + |log p^K_ijk|).  tests/test_epi_restatement_cpu.py measures 3.92e-16 (x 10 = 3.92e-15) and asserts that
# this constant covers it.  The library's value and the device's must lie within ten times this constant of the float64 restatement, and
# the screen's slack delta (2^-44 = 5.7e-14 of the bound of that sum) covers ten times it on every table.
KSA_F64_LD = 4e-15

# The same for LR relative to sum n_ijk (|log(n_ijk / n)| + |log(m_ijk / n)|), the fit m taken from the float64 run: measured 1.48e-16
LR_F64_LD = 1.6e-15


def delta(n):
    """the slack of the screen for n rows: 2^-44 times the bound 2 n (4 ln n + ln 18) of the sum of the absolute terms"""
    n = max(float(n), 2.0)
    return 2.0 ** -44 * (2.0 * n * (4.0 * math.log(n) + math.log(18.0)))


def tables(geno, idxA, idxB, cls=None):
    """int64 (na, nb, 2, 3, 3): [a, b, k, i, j] = rows of class k with code i at marker idxA[a] and code j at idxB[b]; code 3 (a
    missing call) in no cell; cls None = every row class 0"""
    geno = np.asarray(geno)
    n = geno.shape[1]
    cls = np.zeros(n, dtype=np.int64) if cls is None else np.asarray(cls, dtype=np.int64)
    K = np.stack([cls == 0, cls == 1]).astype(np.int64)
    A = np.stack([geno[np.asarray(idxA, dtype=np.int64)] == i for i in range(3)], axis=1).astype(np.int64)  # (na, 3, n)
    B = np.stack([geno[np.asarray(idxB, dtype=np.int64)] == j for j in range(3)], axis=1).astype(np.int64)
    out = np.zeros((A.shape[0], B.shape[0], 2, 3, 3), dtype=np.int64)
    for k in range(2):
        Ak = (A * K[k]).reshape(A.shape[0] * 3, n)
        out[:, :, k] = (Ak @ B.reshape(B.shape[0] * 3, n).T).reshape(A.shape[0], 3, B.shape[0], 3).transpose(0, 2, 1, 3)
    return out


def margins(t):
    """t (..., 2, 3, 3) integers -> nij (..., 3, 3), nik (..., 2, 3), njk (..., 2, 3), ni, nj (..., 3), nk (..., 2), n (...)"""
    t = np.asarray(t, dtype=np.int64)
    nij = t[..., 0, :, :] + t[..., 1, :, :]
    nik = t.sum(axis=-1)
    njk = t.sum(axis=-2)
    return nij, nik, njk, nik.sum(axis=-2), njk.sum(axis=-2), nik.sum(axis=-1), t.sum(axis=(-1, -2, -3))


def ksa(t, dtype=np.float64):
    """(KSA, sum of the absolute terms) of tables t (..., 2, 3, 3), every operation in hg_epi_ksa's order, in dtype"""
    t = np.asarray(t, dtype=np.int64)
    nij, nik, njk, ni, nj, nk, n = margins(t)
    f = lambda x: np.asarray(x).astype(dtype)
    shape = t.shape[:-3]
    q = {}
    eta = np.zeros(shape, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(2):
            for i in range(3):
                for j in range(3):
                    live = (ni[..., i] > 0) & (nj[..., j] > 0) & (nk[..., k] > 0)
                    num = (f(nij[..., i, j]) * f(nik[..., k, i])) * f(njk[..., k, j])
                    den = (f(ni[..., i]) * f(nj[..., j])) * f(nk[..., k])
                    q[k, i, j] = np.where(live, num / np.where(live, den, 1), 0).astype(dtype)
                    eta = eta + q[k, i, j]
        s = np.zeros(shape, dtype=dtype)
        a = np.zeros(shape, dtype=dtype)
        for k in range(2):
            for i in range(3):
                for j in range(3):
                    x = f(t[..., k, i, j])
                    pos = t[..., k, i, j] > 0
                    ls = np.log(np.where(pos, x / np.where(pos, f(n), 1), 1))
                    lk = np.log(np.where(pos, q[k, i, j] / np.where(pos, eta, 1), 1))
                    s = s + np.where(pos, x * (ls - lk), 0)
                    a = a + np.where(pos, x * (np.abs(ls) + np.abs(lk)), 0)
    return 2 * s, a


def df(t):
    nij, nik, njk, ni, nj, nk, n = margins(t)
    I, J = (ni > 0).sum(axis=-1), (nj > 0).sum(axis=-1)
    return np.where((I > 0) & (J > 0), (I - 1) * (J - 1), 0)


def tail(x, d):
    """the chi-square upper tail for d in {1, 2, 4} in closed form; NaN at d = 0"""
    if d == 1:
        return math.erfc(math.sqrt(x / 2.0))
    if d == 2:
        return math.exp(-x / 2.0)
    if d == 4:
        return math.exp(-x / 2.0) * (1.0 + x / 2.0)
    return float("nan")


def tail_tol(x, d, dx):
    """how far the tail may move when its argument moves by dx (the tail is steep in sqrt(x) at 0 for d = 1)"""
    return abs(tail(max(x - dx, 0.0), d) - tail(x + dx, d)) + 1e-12 * tail(x, d)


def ipf(t):
    """The fit of the homogeneous-association model to tables t (T, 2, 3, 3) in float64, hg_epi.cpp's operations in their order: returns
    m (T, 2, 3, 3), iters (T,), converged (T,).  Tables with df = 0 are not fitted (iters 0, converged 1, m = ones)."""
    t = np.asarray(t, dtype=np.int64).reshape(-1, 2, 3, 3)
    nij, nik, njk, ni, nj, nk, n = margins(t)
    T = t.shape[0]
    m = np.ones((T, 2, 3, 3))
    iters = np.zeros(T, dtype=np.int64)
    conv = np.ones(T, dtype=np.int64)
    act = np.flatnonzero(df(t) > 0)
    conv[act] = 0
    fij, fik, fjk, lim = nij.astype(np.float64), nik.astype(np.float64), njk.astype(np.float64), EPI_TOL * n.astype(np.float64)

    def ratio(want, s):
        ok = s > 0.0
        return np.where(ok, want / np.where(ok, s, 1.0), 0.0)

    for _ in range(EPI_CYCLES):
        if act.size == 0:
            break
        x = m[act]
        old = x.copy()
        x = x * ratio(fij[act], x[:, 0] + x[:, 1])[:, None, :, :]
        x = x * ratio(fik[act], (x[..., 0] + x[..., 1]) + x[..., 2])[..., None]
        x = x * ratio(fjk[act], (x[:, :, 0, :] + x[:, :, 1, :]) + x[:, :, 2, :])[:, :, None, :]
        m[act] = x
        iters[act] += 1
        d = np.abs(x - old).reshape(act.size, 18).max(axis=1)
        done = d <= lim[act]
        conv[act[done]] = 1
        act = act[~done]
    return m, iters, conv


def lr_of(t, m, dtype=np.float64):
    """(LR, sum of the absolute terms) of tables t with fits m, hg_epi.cpp's order; LR is 0 where df = 0 and is not below 0"""
    t = np.asarray(t, dtype=np.int64).reshape(-1, 2, 3, 3)
    n = t.sum(axis=(1, 2, 3)).astype(dtype)
    s = np.zeros(t.shape[0], dtype=dtype)
    a = np.zeros(t.shape[0], dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(2):
            for i in range(3):
                for j in range(3):
                    pos = t[:, k, i, j] > 0
                    x = t[:, k, i, j].astype(dtype)
                    ls = np.log(np.where(pos, x / np.where(pos, n, 1), 1))
                    lm = np.log(np.where(pos, m[:, k, i, j].astype(dtype) / np.where(pos, n, 1), 1))
                    s = s + np.where(pos, x * (ls - lm), 0)
                    a = a + np.where(pos, x * (np.abs(ls) + np.abs(lm)), 0)
    lr = np.maximum(2 * s, 0)
    return np.where(df(t) > 0, lr, 0), a


def epi_test(t):
    """what hgibbs_epi_test returns for tables t (T, 2, 3, 3), as arrays: ksa, lr, df, iters, converged, p, and the two scales"""
    t = np.asarray(t, dtype=np.int64).reshape(-1, 2, 3, 3)
    k, ka = ksa(t)
    m, iters, conv = ipf(t)
    lr, la = lr_of(t, m)
    d = df(t)
    p = np.array([tail(float(x), int(v)) for x, v in zip(lr, d)])
    return {"ksa": k, "lr": lr, "df": d, "iters": iters, "converged": conv, "p": p, "ksa_scale": ka, "lr_scale": la}





def grid_tables(seed=11, count=3000):
    """random 2 x 3 x 3 tables: totals from tens to a few thousand, uneven cell weights, and in a share of them empty rows, columns
    or single cells; followed by hand-made corners"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.choice([20, 60, 200, 600, 2000, 5000]))
        w = rng.gamma(rng.choice([0.3, 1.0, 3.0]), size=(2, 3, 3))
        u = rng.random()
        if u < 0.15:
            w[:, rng.integers(3), :] = 0
        elif u < 0.30:
            w[:, :, rng.integers(3)] = 0
        elif u < 0.40:
            w[:, rng.integers(3), :] = 0
            w[:, :, rng.integers(3)] = 0
        elif u < 0.55:
            w[rng.integers(2), rng.integers(3), rng.integers(3)] = 0
        if w.sum() == 0:
            w[0, 0, 0] = 1
        out.append(rng.multinomial(n, (w / w.sum()).reshape(-1)).reshape(2, 3, 3))
    one = np.zeros((2, 3, 3), dtype=np.int64)
    one[0, 1, 1] = 7
    out += [np.zeros((2, 3, 3), dtype=np.int64), one, np.full((2, 3, 3), 5), np.arange(18).reshape(2, 3, 3)]
    return np.array(out, dtype=np.int64)


def with_missing(geno, rate, seed):
    geno = np.array(geno, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    geno[rng.random(geno.shape) < rate] = 3
    return geno


PLANTED = (5, 33)  # the two markers that carry the interaction


def planted_case(seed=7):
    """N = 600, M = 40, 2 % missing calls; markers 5 and 33 carry the interaction: penetrance 0.8 where both or neither carry an A1
    allele, 0.2 elsewhere.  Returns geno (M, N) of codes and cls (N,) of 0 / 1."""
    N, M = 600, 40
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.5, size=M)
    p[list(PLANTED)] = 0.3
    geno = rng.binomial(2, p[:, None], size=(M, N)).astype(np.uint8)
    same = (geno[PLANTED[0]] > 0) == (geno[PLANTED[1]] > 0)
    cls = (rng.random(N) < np.where(same, 0.8, 0.2)).astype(np.uint8)
    return with_missing(geno, 0.02, seed + 1), cls


def second_case(seed=19):
    """N = 1000, M = 64, clean, classes at random"""
    rng = np.random.default_rng(seed)
    geno = rng.binomial(2, rng.uniform(0.05, 0.5, size=64)[:, None], size=(64, 1000)).astype(np.uint8)
    return geno, (rng.random(1000) < 0.4).astype(np.uint8)


# The thresholds of the cases: chosen so that the restatement alone puts no pair's KSA within 2 delta of one (asserted by
# tests/test_epi_restatement_cpu.py for these seeds)
T_PLANTED = (30.0, 12.0)
T_SECOND = 9.0


def triangle(geno, cls, markers=None):
    """every pair a < b of `markers` (default all): ab (P, 2) positions, tables (P, 2, 3, 3)"""
    idx = np.arange(geno.shape[0]) if markers is None else np.asarray(markers)
    t = tables(geno, idx, idx, cls)
    a, b = np.triu_indices(idx.size, 1)
    return np.stack([a, b], axis=1), t[a, b]


def fmt(x):
    return "%.9g" % x


def epi_cc(geno, cls, pairs, T, chrom=None, bp=None, ids=None):
    """The rows of .epi.cc for the marker pairs `pairs` (j1 < j2, in order) of a cohort: a list of lists of text fields, header first.
    A pair is screened by KSA >= T - delta and written when CHISQ >= T and DF > 0."""
    M, N = geno.shape
    chrom = ["1"] * M if chrom is None else chrom
    bp = list(range(1, M + 1)) if bp is None else bp
    ids = ["snp%d" % j for j in range(M)] if ids is None else ids
    rows = [["CHR1", "SNP1", "BP1", "CHR2", "SNP2", "BP2", "N", "N_CASE", "N_CTRL", "KSA", "CHISQ", "DF", "P", "OK"]]
    nums = []
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.shape[0] == 0:
        return rows, nums
    t = np.array([tables(geno, [a], [b], cls)[0, 0] for a, b in pairs])
    r = epi_test(t)
    for p, (a, b) in enumerate(pairs):
        if not (r["ksa"][p] >= T - delta(N) and r["lr"][p] >= T and r["df"][p] > 0):
            continue
        rows.append([chrom[a], ids[a], str(bp[a]), chrom[b], ids[b], str(bp[b]), str(int(t[p].sum())), str(int(t[p, 1].sum())), str(int(t[p, 0].sum())),
                     fmt(r["ksa"][p]), fmt(r["lr"][p]), str(int(r["df"][p])), fmt(r["p"][p]), str(int(r["converged"][p]))])
        nums.append((r["ksa"][p], r["lr"][p], r["p"][p], r["ksa_scale"][p], r["lr_scale"][p]))
    return rows, nums
