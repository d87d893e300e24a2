"""hgibbs_he_fit (host only) against dense OLS over all pairs in longdouble, and its delete-one-individual jackknife against literal
refits.  The row sums the fit takes are computed here in NumPy from a dense random A = X X' / M and y.  No GPU needed."""
import functools

import numpy as np
import pytest

from hydra_amd import capi

LD = np.longdouble


@functools.lru_cache(maxsize=None)
def data(n, seed=0):
    rng = np.random.default_rng(1000 + n + seed)
    M = 3 * n + 7
    X = rng.standard_normal((n, M))
    A = X @ X.T / M
    y = rng.standard_normal(n) + 0.3 * X[:, :5].sum(axis=1) + 0.7
    A.setflags(write=False)
    y.setflags(write=False)
    return A, y


def rowsums(A, y, used=None):
    """ay, ayy, a1, a2, partners over each row's partners: every other used row"""
    n = len(y)
    used = np.ones(n, dtype=bool) if used is None else used
    O = np.where(used[:, None] & used[None, :] & ~np.eye(n, dtype=bool), A, 0.0)
    partners = np.where(used, used.sum() - 1, 0).astype(np.uint32)
    return O @ y, O @ (y * y), O.sum(axis=1), (O * O).sum(axis=1), partners


def dense_ols(A, y, rows, dtype=LD):
    """OLS of z on A with an intercept over all pairs a < b of `rows`, for both forms: {form: (icpt, slope, se_icpt, se_slope)}, and m"""
    A = np.asarray(A, dtype=dtype)[np.ix_(rows, rows)]
    y = np.asarray(y, dtype=dtype)[rows]
    a, b = np.triu_indices(len(rows), 1)
    x = A[a, b]
    m = dtype(x.size)
    out = {}
    for form, z in (("cp", y[a] * y[b]), ("sd", (y[a] - y[b]) ** 2)):
        sx, sz, sxx, sxz = x.sum(), z.sum(), (x * x).sum(), (x * z).sum()
        den = m * sxx - sx * sx
        slope = (m * sxz - sx * sz) / den
        icpt = (sz - slope * sx) / m
        res = z - icpt - slope * x
        s2 = (res * res).sum() / (m - 2)
        out[form] = (icpt, slope, np.sqrt(s2 * sxx / den), np.sqrt(s2 * m / den))
    return out, int(x.size)


def rel(got, want):
    return float(abs(LD(got) - want) / abs(want))


def vp_of(y, rows):
    v = np.asarray(y, dtype=LD)[rows]
    return ((v - v.mean()) ** 2).sum() / (len(rows) - 1)


H2 = {"cp": lambda s, vp: s / vp, "sd": lambda s, vp: -s / (2 * vp)}


@pytest.mark.parametrize("n", [4, 5, 60, 200, 513])
def test_against_dense_longdouble_ols(n):
    A, y = data(n)
    fit = capi.he_fit(y, *rowsums(A, y))
    rows = np.arange(n)
    ref, m = dense_ols(A, y, rows)
    vp = vp_of(y, rows)
    assert fit["n_used"] == n and fit["n_left_out"] == 0 and fit["pairs"] == m == n * (n - 1) // 2
    worst = rel(fit["vp"], vp)
    for form in ("cp", "sd"):
        icpt, slope, se_i, se_s = ref[form]
        g = fit[form]
        k = abs(H2[form](LD(1), vp))
        for name, got, want in (("intercept", g["intercept"], icpt), ("slope", g["slope"], slope), ("intercept_se", g["intercept_se"], se_i),
                                ("slope_se", g["slope_se"], se_s), ("h2", g["h2"], H2[form](slope, vp)), ("h2_se", g["h2_se"], k * se_s)):
            d = rel(got, want)
            worst = max(worst, d)
            assert d <= 1e-12, (form, name, got, want, d)
    print("MEASURED n=%d: he_fit against dense longdouble OLS, largest relative difference %.3g (bound 1e-12)" % (n, worst))


@pytest.mark.parametrize("n", [4, 5, 60, 200])
def test_jackknife_against_literal_refits(n):
    A, y = data(n)
    fit = capi.he_fit(y, *rowsums(A, y))
    vp = vp_of(y, np.arange(n))
    est = {"cp": [], "sd": []}
    for a in range(n):
        r, _ = dense_ols(A, y, np.delete(np.arange(n), a))
        for form in est:
            est[form].append(r[form][:2])
    worst = 0.0
    for form in est:
        th = np.array(est[form], dtype=LD)  # (n, 2): intercept, slope
        se = np.sqrt(LD(n - 1) / n * ((th - th.mean(axis=0)) ** 2).sum(axis=0))
        g = fit[form]
        k = abs(H2[form](LD(1), vp))
        for name, got, want in (("intercept_se_jk", g["intercept_se_jk"], se[0]), ("slope_se_jk", g["slope_se_jk"], se[1]),
                                ("h2_se_jk", g["h2_se_jk"], k * se[1])):
            d = rel(got, want)
            worst = max(worst, d)
            print("MEASURED n=%d %s %s: %.17g against the refits' %.17g, relative difference %.3g" % (n, form, name, got, float(want), d))
            assert d <= 1e-9, (form, name, got, want, d)
    print("MEASURED n=%d: jackknife SEs against literal refits, largest relative difference %.3g (bound 1e-9)" % (n, worst))


def test_p_values_are_two_sided_normal():
    import math
    A, y = data(60)
    fit = capi.he_fit(y, *rowsums(A, y))
    for form in ("cp", "sd"):
        g = fit[form]
        for est, se, p in (("intercept", "intercept_se", "intercept_p"), ("slope", "slope_se", "slope_p"),
                           ("intercept", "intercept_se_jk", "intercept_p_jk"), ("slope", "slope_se_jk", "slope_p_jk")):
            want = math.erfc(abs(g[est] / g[se]) / math.sqrt(2.0))
            assert abs(g[p] - want) <= 1e-13 * max(want, 1e-300), (form, p, g[p], want)


def test_rows_without_partners_are_left_out_and_counted():
    n = 63
    A, y = data(n)
    used = np.ones(n, dtype=bool)
    used[[0, 17, 62]] = False
    sums = [np.array(v) for v in rowsums(A, y, used)]
    yy = np.array(y)
    yy[17] = 1e6  # what a left-out row holds does not matter, not even a NaN
    sums[0][0] = np.nan
    fit = capi.he_fit(yy, *sums)
    rows = np.flatnonzero(used)
    ref, m = dense_ols(A, y, rows)
    assert fit["n_used"] == n - 3 and fit["n_left_out"] == 3 and fit["pairs"] == m
    assert rel(fit["vp"], vp_of(y, rows)) <= 1e-12
    for form in ("cp", "sd"):
        for name, want in zip(("intercept", "slope", "intercept_se", "slope_se"), ref[form]):
            assert rel(fit[form][name], want) <= 1e-12, (form, name)


def test_row_with_too_few_partners_is_refused_by_name():
    A, y = data(60)
    sums = list(rowsums(A, y))
    pt = sums[4].copy()
    pt[23] = 58
    pt[40] = 57
    with pytest.raises(capi.HgError, match=r"row 23 has 58 partners .* should each have 59"):
        capi.he_fit(y, *sums[:4], pt)


def test_other_refusals():
    A, y = data(60)
    sums = rowsums(A, y)
    # n' < 4
    used = np.zeros(60, dtype=bool)
    used[:3] = True
    with pytest.raises(capi.HgError, match="3 rows with a partner"):
        capi.he_fit(y, *rowsums(A, y, used))
    A3, y3 = data(4)
    with pytest.raises(capi.HgError, match="at least 4"):
        capi.he_fit(y3[:3], *rowsums(A3[:3, :3], y3[:3]))
    # a non-finite input, in every array
    for k in range(5):
        arrs = [np.array(y)] + [np.array(v) for v in sums[:4]]
        arrs[k][7] = np.inf if k % 2 else np.nan
        with pytest.raises(capi.HgError, match="non-finite input at row 7"):
            capi.he_fit(*arrs, sums[4])
    # a constant A: no slope
    const = np.full((60, 60), 0.25)
    with pytest.raises(capi.HgError, match="A is constant"):
        capi.he_fit(y, *rowsums(const, y))
    # a constant y: Vp = 0
    with pytest.raises(capi.HgError, match=r"y is constant over the 60 used rows \(Vp = 0\)"):
        capi.he_fit(np.full(60, 1.5), *rowsums(A, np.full(60, 1.5)))
    # after the refusals the fit still works
    assert capi.he_fit(y, *sums)["n_used"] == 60
