"""tests/pca_restate.py, the restatement that tests/test_gpu_pca_exact.py compares hgibbs_pca with bit for bit, checked on its own with
plain f64 NumPy products in place of the device's operators: (a) it is the algorithm (against numpy.linalg.eigh and numpy_pca), (b) its
two host transliterations do what their names say, (c) a comparison of bits sees a reordering that the tolerances of
tests/test_gpu_pca.py cannot, (d) every case of the GPU grid runs to its end without a refusal.

Measured here (NumPy 2 on x86-64; each bound of (b) is ten times the measured value, never above 1e-12):

  (a) restatement against eigh of Z Z'/M_used (N = 400, M = 1500, four populations 3 : 4 : 5 : 6 at F = 0.1, K = 3, 20 iterations):
      vectors 1.5e-15 at L = 5, 8 and 13, eigenvalues 3.4e-16; against numpy_pca vectors 9.1e-16 .. 1.2e-15, eigenvalues 6.9e-16 ..
      8.2e-16, loadings 8.8e-16 .. 1.1e-15; reported residuals 3.4e-16 .. 4.2e-16.  On the n777_m2999 recipe of test_gpu_pca.py
      (F = 0.02, whose 20 iterations are short of rounding at these widths: residuals 6e-14 .. 3e-10, so eigh is no reference there)
      against numpy_pca: vectors 1.0e-15 .. 1.2e-15, eigenvalues 4.1e-16 .. 1.0e-15, loadings 1.1e-15 .. 1.3e-15, and the reported
      residuals equal NumPy's to 1e-3 relative, the bound asserted.  All under VEC_BOUND = 8.8e-14 and VAL_BOUND = 2.2e-14, the bounds of test_gpu_pca.py.
  (b) in units of eps = 2^-52, largest over L = 1, 2, 5, 13, 32 (Gram matrices of 500-row panels, columns of unequal size, one pair
      correlated):
      max |R^-1' G R^-1 - I|                      3.0 eps     (bound 30 eps = 6.7e-15)
      max |W diag(theta) W' - S| / max |S|        33.7 eps    (bound 337 eps = 7.5e-14; 9.4 eps at L = 13, 6.8 at L = 5)
      max |theta - eigvalsh(S)| / max theta       17.2 eps    (bound 172 eps = 3.8e-14; 6.4 eps at L = 13, 5.1 at L = 5)
  (c) n = 1025, L = 13, 169 entries: the rows of each workgroup summed in reverse order change the bits of 94.7 % of the entries,
      np.sum over the rows of a workgroup 89.3 %, dropping row 1024 (the second workgroup's only row) 100 %.  The largest change of
      the two reorderings is 2.6e-15 of |p_a| |p_b|, a thirtieth of VEC_BOUND.  End to end (n = 1025, M = 200, L = 5, K = 3, two
      iterations) the reversed order changes the bits of every eigenvalue and residual, of 99.4 % of the PC entries and of every
      loading of a used marker, by at most 2.5e-15 in a PC entry.
  (d) all 60 cases of the grid and the three single cases run to their end; the stop-rule case stops after 16 of 40 iterations.  A
      rank loss INSIDE the iteration from clean input was looked for with duplicated individuals (fewer distinct rows than L): the
      start panel passes and the first Y = X T loses rank, always in iteration 1, at the pivot that equals the rank of X or, when the
      rounding of the products lets that one pass, at a later one (n = 130 as 26 copies of 5, L = 8: pivot 5, not 4).  No input was
      found that passes iteration 1 and loses rank later (Y keeps the rank of X from then on), so the GPU file has no such case."""
import numpy as np
import pytest

import pca_restate
from pca_restate import (GRID, OPTIONS, SEEDED, SIZES, STOP, VAL_BOUND, VEC_BOUND, chol_inv, cpu_products, dense, gram, gram_partials, gram_sum,
                         jacobi, numpy_pca, planted, restate, same_bits, start_for, structured, val_err, vec_err, zmat)

EPS = 2.0 ** -52
CHOL_BOUND = 30 * EPS
JACOBI_PAIR_BOUND = 337 * EPS
JACOBI_VAL_BOUND = 172 * EPS
assert max(CHOL_BOUND, JACOBI_PAIR_BOUND, JACOBI_VAL_BOUND) <= 1e-12


def changed(a, b):
    return float((a.view(np.uint64) != b.view(np.uint64)).mean())


# ---- (a) the restatement is the algorithm ----
@pytest.fixture(scope="module")
def converged():
    N, M = 400, 1500
    geno, _ = structured(N, M, P=4, F=0.1, miss=0.02, seed=11, sizes=SIZES)
    geno[M - 1] = 3
    geno[M // 3] = np.where(geno[M // 3] == 3, 3, 1)
    geno[:, N // 2] = 3
    Z, good = zmat(geno)
    m = int(good.sum())
    assert m == M - 2
    lam, U = dense(Z, m, 3)
    return geno, Z, good, m, lam, U


@pytest.mark.parametrize("L", [5, 8, 13])
def test_against_eigh_and_numpy_pca(converged, L):
    geno, Z, good, m, lam, U = converged
    M, N = geno.shape
    products, mave, mstd = cpu_products(geno)
    assert np.array_equal(np.isfinite(mstd), good)
    Q0 = np.random.default_rng(7).standard_normal((L, N))
    r = restate(products, mave, mstd, N, M, 3, L, 20, 0.0, Q0)
    rval, rV, rld, rit = numpy_pca(Z, m, 3, L, 20, 0.0, Q0)
    figs = (vec_err(r["pcs"], U), val_err(r["eigval"], lam[:3]), vec_err(r["pcs"], rV), val_err(r["eigval"], rval),
            vec_err(r["loadings"][:, good], rld[:, good]))
    print("MEASURED L = %d: restatement vs eigh: vectors %.3g, eigenvalues %.3g; vs numpy_pca: vectors %.3g, eigenvalues %.3g, loadings %.3g" % ((L,) + figs))
    assert r["iters_run"] == rit == 20 and r["m_used"] == m and r["ritz_change"] <= 1e-12
    assert figs[0] <= VEC_BOUND and figs[2] <= VEC_BOUND and figs[4] <= VEC_BOUND
    assert figs[1] <= VAL_BOUND and figs[3] <= VAL_BOUND
    assert np.isnan(r["loadings"][:, ~good]).all() and np.isfinite(r["loadings"][:, good]).all()
    assert np.all(r["pcs"][:, N // 2] == 0.0)
    for k in range(3):
        assert r["pcs"][k, int(np.argmax(np.abs(r["pcs"][k])))] > 0
    res = np.array([np.linalg.norm(Z @ (Z.T @ r["pcs"][k]) / m - r["eigval"][k] * r["pcs"][k]) / r["eigval"][k] for k in range(3)])
    print("  residuals: restatement %s, NumPy on the returned pair %s" % (r["resid"], res))
    assert np.all(r["resid"] <= 1e-13) and np.all(res <= 1e-13)


@pytest.mark.parametrize("L", [5, 8, 13])
def test_against_numpy_pca_on_a_shape_of_the_gpu_suite(L):
    """test_gpu_pca.py's n777_m2999 recipe.  Its 20 iterations are short of rounding at these widths (residuals 1e-13 .. 3e-10), so the
    reference is numpy_pca, which makes the same 20 steps, and the residual the restatement reports is checked against NumPy's."""
    N, M, K = 777, 2999, 3
    geno, _ = structured(N, M, P=4, F=0.02, miss=0.02, seed=11, sizes=SIZES)
    Z, good = zmat(geno)
    m = int(good.sum())
    products, mave, mstd = cpu_products(geno)
    Q0 = np.random.default_rng(7).standard_normal((L, N))
    r = restate(products, mave, mstd, N, M, K, L, 20, 0.0, Q0)
    rval, rV, rld, _ = numpy_pca(Z, m, K, L, 20, 0.0, Q0)
    figs = (vec_err(r["pcs"], rV), val_err(r["eigval"], rval), vec_err(r["loadings"][:, good], rld[:, good]))
    print("MEASURED n777_m2999, L = %d: restatement vs numpy_pca: vectors %.3g, eigenvalues %.3g, loadings %.3g" % ((L,) + figs))
    assert r["m_used"] == m
    assert figs[0] <= VEC_BOUND and figs[1] <= VAL_BOUND and figs[2] <= VEC_BOUND
    res = np.array([np.linalg.norm(Z @ (Z.T @ r["pcs"][k]) / m - r["eigval"][k] * r["pcs"][k]) / r["eigval"][k] for k in range(K)])
    print("  residuals: restatement %s, NumPy %s" % (r["resid"], res))
    assert np.all(np.abs(r["resid"] - res) <= 1e-3 * res + 1e-14)


# ---- (b) the two host transliterations ----
def panels():
    """Gram matrices of panels with columns of unequal size and some correlation: what CholeskyQR and the Ritz step see"""
    for L in (1, 2, 5, 13, 32):
        rng = np.random.default_rng(40 + L)
        P = rng.standard_normal((500, L)) * np.exp2(rng.uniform(-1, 1, size=L))[None, :]
        P[:, L // 2] += 0.5 * P[:, 0]
        yield L, gram(P, 0)


def test_chol_inv():
    worst = 0.0
    for L, G in panels():
        bad, piv, Rinv = chol_inv(G)
        assert bad == -1 and Rinv.shape == (L, L)
        assert np.all(np.tril(Rinv, -1) == 0.0) and np.all(np.diag(Rinv) > 0.0)
        err = float(np.max(np.abs(Rinv.T @ G @ Rinv - np.eye(L))))
        print("MEASURED L = %d: max |R^-1' G R^-1 - I| = %.3g = %.2f eps" % (L, err, err / EPS))
        worst = max(worst, err)
        assert err <= CHOL_BOUND
    # the pivot test: a dependent column ends it at that column; a pivot is refused up to 1e-13 of its diagonal entry and not above
    P = np.random.default_rng(3).standard_normal((100, 4))
    P[:, 2] = P[:, 0] - 2.0 * P[:, 1]
    bad, piv, Rinv = chol_inv(gram(P, 0))
    assert bad == 2 and Rinv is None and abs(piv) <= 1e-13 * gram(P, 0)[2, 2]
    for delta, want in ((0.5e-13, 1), (2e-13, -1)):  # G = [[1, c], [c, 1]]: pivot 1 is 1 - c^2 = delta up to rounding
        c = np.sqrt(1.0 - delta)
        assert chol_inv(np.array([[1.0, c], [c, 1.0]]))[0] == want
    assert chol_inv(np.array([[np.nan]]))[0] == 0 and chol_inv(np.array([[np.inf]]))[0] == 0 and chol_inv(np.array([[0.0]]))[0] == 0
    print("MEASURED chol_inv worst: %.2f eps" % (worst / EPS))


def test_jacobi():
    worst_pair = worst_val = 0.0
    for L, S in panels():
        ok, theta, W = jacobi(S)
        assert ok and theta.shape == (L,) and W.shape == (L, L)
        assert np.all(theta[:-1] >= theta[1:])
        pair = float(np.max(np.abs((W * theta[None, :]) @ W.T - S)) / np.max(np.abs(S)))
        val = float(np.max(np.abs(theta - np.linalg.eigvalsh(S)[::-1])) / np.max(np.abs(theta)))
        orth = float(np.max(np.abs(W.T @ W - np.eye(L))))
        print("MEASURED L = %d: |W theta W' - S| / max|S| = %.2f eps, |theta - eigvalsh| / max theta = %.2f eps, |W'W - I| = %.2f eps"
              % (L, pair / EPS, val / EPS, orth / EPS))
        worst_pair, worst_val = max(worst_pair, pair), max(worst_val, val)
        assert pair <= JACOBI_PAIR_BOUND and val <= JACOBI_VAL_BOUND
    print("MEASURED jacobi worst: pairs %.2f eps, eigenvalues %.2f eps" % (worst_pair / EPS, worst_val / EPS))
    # the symmetrisation comes first; equal eigenvalues keep index order (a stable sort)
    S = np.array([[2.0, 1.0 + 2.0 ** -40, 0.5], [1.0 - 2.0 ** -40, 3.0, 0.25], [0.5 + 2.0 ** -30, 0.25, 1.0]])
    one, two = jacobi(S), jacobi(0.5 * (S + S.T))
    assert one[0] and same_bits(one[1], two[1]) and same_bits(one[2], two[2])
    assert not same_bits(one[1], jacobi(np.triu(S) + np.triu(S, 1).T)[1])
    ok, theta, W = jacobi(np.diag([1.0, 5.0, 1.0, 5.0]))
    assert ok and list(theta) == [5.0, 5.0, 1.0, 1.0] and np.array_equal(W, np.eye(4)[:, [1, 3, 0, 2]])
    # as in the code, NaN > x is false: a NaN sum of squares reads as converged (hgibbs_pca then refuses the NaN Ritz value of a NaN row)
    ok, theta, W = jacobi(np.array([[np.nan, np.nan], [np.nan, 1.0]]))
    assert ok and np.isnan(theta).any()


# ---- (c) what a comparison of bits sees ----
def test_bits_see_a_reordering():
    n, L = 1025, 13
    P = np.random.default_rng(5).standard_normal((n, L))
    G = gram(P, 0)
    assert np.array_equal(G, G.T) and np.array_equal(G.view(np.uint64), gram(np.ascontiguousarray(P.T), 1).view(np.uint64))
    rev = np.concatenate([P[1023::-1], P[1024:]])  # the rows of each workgroup in reverse order
    G_rev = gram(rev, 0)
    # np.sum over the rows of a workgroup, the rows along the contiguous axis (where NumPy adds pairwise)
    G_sum = gram_sum(np.stack([np.sum(np.ascontiguousarray((P[w:w + 1024, :, None] * P[w:w + 1024, None, :]).transpose(1, 2, 0)), axis=-1)
                               for w in range(0, n, 1024)]))
    G_drop = gram(P[:-1], 0)
    s_rev, s_sum, s_drop = changed(G, G_rev), changed(G, G_sum), changed(G, G_drop)
    scale = np.sqrt(np.diag(G)[:, None] * np.diag(G)[None, :])  # (an off-diagonal entry is a sum that cancels: measured on |p_a| |p_b|)
    rel = max(float(np.max(np.abs(G_rev - G) / scale)), float(np.max(np.abs(G_sum - G) / scale)))
    print("MEASURED n = %d, L = %d: share of the %d entries whose bits change: rows reversed %.3f, np.sum %.3f, last row dropped %.3f; "
          "largest change of the reorderings over |p_a| |p_b| %.3g" % (n, L, L * L, s_rev, s_sum, s_drop, rel))
    assert s_rev > 0.5 and s_sum > 0.5
    assert s_drop == 1.0
    assert rel < 0.1 * VEC_BOUND  # far below what a tolerance of that size can notice
    # the partition is part of the order: the same rows split at another row change bits as well
    other = gram_sum(np.stack([gram_partials(P[:1000], 0)[0], gram_partials(P[1000:], 0)[0]]))
    assert changed(G, other) > 0.5


def test_outputs_see_a_reordered_gram(monkeypatch):
    """end to end: with the rows of every workgroup of k_pca_gram summed in reverse order, the restatement returns other bits"""
    c = GRID["n1025"]
    geno, keep, kept = planted(c["n"], c["M"], c["drop"], c["seed"])
    products, mave, mstd = cpu_products(kept)
    args = (products, mave, mstd, c["n"], c["M"], c["K"], c["L"], c["iters"], c["tol"], start_for(c))
    one = restate(*args)
    assert all(same_bits(one[k], restate(*args)[k]) for k in ("eigval", "pcs", "loadings", "resid"))
    forward = pca_restate.gram_partials

    def backward(P, vecmajor):
        X = pca_restate.rows_of(P, vecmajor)
        return forward(np.concatenate([X[w:w + 1024][::-1] for w in range(0, X.shape[0], 1024)]), 0)

    monkeypatch.setattr(pca_restate, "gram_partials", backward)
    two = restate(*args)
    shares = {k: changed(one[k], two[k]) for k in ("eigval", "pcs", "loadings", "resid")}
    print("MEASURED n = 1025, M = 200, L = 5, K = 3: share of entries whose bits change under a reversed Gram order: %s; largest change of a PC entry %.3g"
          % (shares, float(np.max(np.abs(one["pcs"] - two["pcs"])))))
    assert shares["pcs"] > 0.5 and shares["loadings"] > 0.25
    assert float(np.max(np.abs(one["pcs"] - two["pcs"]))) < 0.1 * VEC_BOUND


# ---- (d) the premise of the GPU grid: no case ends in a refusal ----
def run_cpu(c):
    geno, keep, kept = planted(c["n"], c["M"], c["drop"], c["seed"])
    assert kept.shape == (c["M"], c["n"]) and geno.shape[1] == c["n"] + c["drop"]
    products, mave, mstd = cpu_products(kept)
    return restate(products, mave, mstd, c["n"], c["M"], c["K"], c["L"], c["iters"], c["tol"], start_for(c)), mstd


def test_grid_has_every_case_of_the_issue():
    names = set(GRID)
    assert len(GRID) == 32 + 12 + 9 + 5 + 2
    assert {"width_L%d" % L for L in range(1, 33)} <= names
    assert {"n%d" % n for n in (6, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)} <= names
    assert {"m%d" % m for m in (7, 63, 64, 65, 129, 1023, 1024, 1025, 2049)} <= names
    for c in GRID.values():
        assert c["n"] + c["M"] <= 20000 and c["K"] <= c["L"] < c["n"]
    assert GRID["n6"]["n"] == GRID["n6"]["L"] + 1 and any(c["drop"] for c in GRID.values())


@pytest.mark.parametrize("name", list(GRID) + ["stop", "options", "seeded"])
def test_grid_case_runs_without_refusal(name):
    c = {"stop": STOP, "options": OPTIONS, "seeded": SEEDED}.get(name) or GRID[name]
    r, mstd = run_cpu(c)
    assert "refused" not in r, r
    assert r["m_used"] == int(np.isfinite(mstd).sum()) <= c["M"] - 2  # the two planted markers, and whatever else is monomorphic
    assert np.isfinite(r["eigval"]).all() and np.isfinite(r["pcs"]).all() and np.isfinite(r["resid"]).all()
    assert np.isnan(r["loadings"][:, ~np.isfinite(mstd)]).all() and np.isfinite(r["loadings"][:, np.isfinite(mstd)]).all()
    if name == "m7":
        assert r["m_used"] == c["L"] == 5
    if name == "stop":
        print("MEASURED stop rule on the CPU products: %d of %d iterations, last change %.3g" % (r["iters_run"], c["iters"], r["ritz_change"]))
        assert 1 < r["iters_run"] < c["iters"] and r["ritz_change"] <= c["tol"]
    else:
        assert r["iters_run"] == c["iters"]
        assert r["ritz_change"] == np.inf if c["iters"] == 1 else np.isfinite(r["ritz_change"])


def duplicated(n, copies, M=200):
    """n individuals that are `copies` copies of n / copies distinct ones: X has fewer distinct rows than a panel of L > n / copies"""
    base, _ = structured(n // copies, M, P=2, F=0.05, miss=0.0, seed=5, sizes=[1, 1])
    return np.ascontiguousarray(np.tile(base, (1, copies)))


REFUSALS = [dict(n=12, copies=3, L=5, K=1), dict(n=40, copies=10, L=6, K=2)]


@pytest.mark.parametrize("c", REFUSALS, ids=lambda c: "n%d" % c["n"])
def test_rank_loss_comes_in_iteration_one(c):
    """duplicated individuals: rank X = (distinct rows) - 1 < L.  One iteration (no Y) passes; any more end at the first Y = X T, in
    iteration 1, at a pivot from the rank on: never in iteration 2 or later, so tests/test_gpu_pca_exact.py has no such case"""
    geno = duplicated(c["n"], c["copies"])
    rank = c["n"] // c["copies"] - 1
    products, mave, mstd = cpu_products(geno)
    Q0 = np.random.default_rng(3).standard_normal((c["L"], c["n"]))
    assert "refused" not in restate(products, mave, mstd, c["n"], 200, c["K"], c["L"], 1, 0.0, Q0)
    for iters in (2, 3, 5):
        r = restate(products, mave, mstd, c["n"], 200, c["K"], c["L"], iters, 0.0, Q0)
        assert r["refused"] == "lost rank" and r["iteration"] == 1 and rank <= r["pivot"] < c["L"], r
    bad = np.ones((c["L"], c["n"]))  # dependent start vectors: iteration 0
    r = restate(products, mave, mstd, c["n"], 200, c["K"], c["L"], 3, 0.0, bad)
    assert r["refused"] == "lost rank" and r["iteration"] == 0 and r["pivot"] == 1
