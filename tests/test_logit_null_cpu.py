"""hgibbs_logit_null (capi.logit_null, host only) against a NumPy Newton iteration run well past convergence: coefficients, fitted
probabilities, the score at the fit, the Cholesky factor, bit-reproducibility, and every refusal by name.  No GPU needed."""
import numpy as np
import pytest

from hydra_amd import capi


def make(n, q, frac, seed):
    """Z = [1 | q - 1 standard normal columns, one shifted and scaled], y ~ Bernoulli(logistic(Z b)) with about `frac` cases"""
    rng = np.random.default_rng(seed)
    Z = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(q - 1)])
    if q > 2:
        Z[:, 2] = 3.0 * Z[:, 2] + 10.0
    b = np.concatenate([[0.0], 0.4 * rng.standard_normal(q - 1)])
    eta = Z @ b
    eta += np.log(frac / (1.0 - frac)) - np.mean(eta)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    assert 0 < y.sum() < n
    return Z, y


def newton(Z, y, iters=40):
    """plain Newton from 0, far past convergence (the quadratic phase ends within ten steps on these shapes)"""
    b = np.zeros(Z.shape[1])
    for _ in range(iters):
        mu = 1.0 / (1.0 + np.exp(-(Z @ b)))
        w = mu * (1.0 - mu)
        b = b + np.linalg.solve(Z.T @ (Z * w[:, None]), Z.T @ (y - mu))
    mu = 1.0 / (1.0 + np.exp(-(Z @ b)))
    return b, mu


CASES = [(n, q, frac) for n in (500, 5000) for q in (1, 3, 6) for frac in (0.5, 0.05)]


@pytest.mark.parametrize("n,q,frac", CASES)
def test_matches_numpy_newton(n, q, frac):
    Z, y = make(n, q, frac, seed=1000 + n + 10 * q + int(100 * frac))
    f = capi.logit_null(Z, y)
    b, mu = newton(Z, y)
    assert 1 <= f["iters"] <= 50
    assert np.all(np.abs(f["coef"] - b) <= 1e-9 * np.abs(b)), (f["coef"], b)
    assert np.max(np.abs(f["mu"] - mu)) <= 1e-12
    assert np.array_equal(f["w"], f["mu"] * (1.0 - f["mu"]))
    # Z'(y - mu) is 0 to rounding: n terms of magnitude <= |z| each carry a rounding error of 2^-53
    score = Z.T @ (y - f["mu"])
    assert np.all(np.abs(score) <= 64 * n * 2.0 ** -53 * np.max(np.abs(Z), axis=0)), score
    # the Cholesky factor of Z'WZ at the fit
    L = f["chol"]
    assert np.array_equal(L, np.tril(L)) and np.all(np.diag(L) > 0)
    info = Z.T @ (Z * f["w"][:, None])
    assert np.allclose(L @ L.T, info, rtol=1e-12, atol=0.0)


def test_repeated_calls_are_bit_identical():
    Z, y = make(5000, 6, 0.05, seed=7)
    a, b = capi.logit_null(Z, y), capi.logit_null(Z.copy(), y.copy())
    for k in ("coef", "mu", "w", "chol"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["iters"] == b["iters"]


def refused(Z, y, *words):
    with pytest.raises(capi.HgError) as e:
        capi.logit_null(Z, y)
    msg = str(e.value)
    assert msg.startswith("hgibbs_logit_null: "), msg
    for w in words:
        assert w in msg, msg


def test_dependent_columns_refused():
    Z, y = make(500, 3, 0.5, seed=3)
    refused(np.column_stack([Z, 2.0 * Z[:, 1] - Z[:, 2]]), y, "dependent columns", "Cholesky")
    refused(np.column_stack([Z, 1.5 * Z[:, 0]]), y, "dependent columns")


def test_perfect_separation_refused():
    rng = np.random.default_rng(4)
    x = rng.standard_normal(500)
    Z = np.column_stack([np.ones(500), x])
    refused(Z, (x > 0.1).astype(np.float64), "separation")


def test_y_outside_01_refused():
    Z, y = make(500, 3, 0.5, seed=5)
    y[17] = 2.0
    refused(Z, y, "y[17] = 2", "outside {0, 1}")


def test_too_few_rows_refused():
    Z, y = make(500, 6, 0.5, seed=6)
    refused(Z[:7], y[:7], "7 rows", "at least 8")
    Z1, y1 = make(500, 1, 0.5, seed=6)
    refused(Z1[:2], np.array([0.0, 1.0]), "2 rows", "at least 3")
    assert capi.logit_null(Z1[:3], np.array([0.0, 1.0, 1.0]))["coef"][0] == pytest.approx(np.log(2.0), rel=1e-12)  # q + 2 rows pass


def test_first_column_must_be_ones():
    Z, y = make(500, 3, 0.5, seed=8)
    Z[3, 0] = 2.0
    refused(Z, y, "first column")
