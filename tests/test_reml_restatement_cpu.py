"""The host half of --reml (hgibbs_reml_next, hgibbs_reml_finish; no device) against tests/reml_restate.py, and the restatement
against the dense REML likelihood: with the probes' expectations in place of the probes, the root of f is the maximiser of the
likelihood; the average-information numbers equal the same matrix from an explicit inverse; the probe signs at a few typed-out places."""
import math

import numpy as np
import pytest

from hydra_amd import capi

import reml_restate as rr


def trace_of(fun, **kw):
    """the library's rule driven like the driver drives it"""
    xs, fs = [], []
    while True:
        xn, st = capi.reml_next(xs, fs, **kw)
        if st != capi.REML_CONTINUE:
            return np.array(xs), np.array(fs), st
        xs.append(xn)
        fs.append(fun(xn))


# ---- the rule ----
@pytest.mark.parametrize("root", [-1.3, 0.2, 2.5])  # f_0 > 0 (delta too small), f_0 < 0 twice
def test_next_both_signs(root):
    fun = lambda x: math.tanh(0.4 * (root - x)) + 0.05 * (root - x) ** 3
    x0 = math.log(3.0)
    assert (fun(x0) < 0) == (root < x0)
    xs, fs, st = trace_of(fun)
    rx, rf, rst = rr.run_rule(fun)
    assert st == rst == capi.REML_CONVERGED
    assert np.array_equal(xs, rx) and np.array_equal(fs, rf)
    assert xs[0] == math.log(0.75 / 0.25)
    assert xs[1] == (math.log(0.5 / 0.5) if fs[0] < 0 else math.log(0.875 / 0.125))
    assert abs(xs[-1] - xs[-2]) < 0.01 and abs(xs[-1] - root) < 0.01
    for k in range(len(xs)):  # every prefix gives the next point
        xn, s = capi.reml_next(xs[:k], fs[:k])
        assert s == capi.REML_CONTINUE and xn == xs[k] == rr.next_rule(list(xs[:k]), list(fs[:k]))[0]


@pytest.mark.parametrize("h0", [0.1, 0.25, 0.6, 0.9])
def test_next_first_step(h0):
    x0, st = capi.reml_next([], [], h2_start=h0)
    assert st == capi.REML_CONTINUE and x0 == math.log((1.0 - h0) / h0)
    up, _ = capi.reml_next([x0], [-0.3], h2_start=h0)
    dn, _ = capi.reml_next([x0], [0.3], h2_start=h0)
    h1 = min(2.0 * h0, (1.0 + h0) / 2.0)
    assert up == math.log((1.0 - h1) / h1) == rr.next_rule([x0], [-0.3], h0)[0] and up < x0
    assert dn == math.log((1.0 - h0 / 2.0) / (h0 / 2.0)) == rr.next_rule([x0], [0.3], h0)[0] and dn > x0


def test_next_clamp_and_at_bound():
    # f > 0 everywhere: the secant step leaves the range, is clamped, and the bound comes twice
    fun = lambda x: 1.0 + 0.01 * x
    xs, fs, st = trace_of(fun)
    rx, rf, rst = rr.run_rule(fun)
    assert st == rst == capi.REML_AT_BOUND
    assert np.array_equal(xs, rx)
    assert xs[-1] == xs[-2] == -rr.XMAX or xs[-1] == xs[-2] == rr.XMAX
    # one clamped step that is not the end
    xn, st = capi.reml_next([0.0, 1.0], [1.0, 0.999])
    assert st == capi.REML_CONTINUE and xn == rr.XMAX == rr.next_rule([0.0, 1.0], [1.0, 0.999])[0]
    xn, st = capi.reml_next([0.0, 1.0], [1.0, 1.001])
    assert st == capi.REML_CONTINUE and xn == -rr.XMAX == rr.next_rule([0.0, 1.0], [1.0, 1.001])[0]


def test_next_refusals():
    with pytest.raises(capi.HgError, match="hgibbs_reml_next: f is flat"):
        capi.reml_next([0.0, 1.0], [0.5, 0.5])
    with pytest.raises(ValueError, match="flat"):
        rr.next_rule([0.0, 1.0], [0.5, 0.5])
    # a function the secant rule does not settle on in 12 evaluations
    fun = lambda x: math.sin(40.0 * x) + 0.3
    with pytest.raises(capi.HgError, match="hgibbs_reml_next: no root after max_steps = 12 evaluations"):
        trace_of(fun)
    with pytest.raises(ValueError, match="max_steps"):
        rr.run_rule(fun)
    xs = list(np.linspace(0.0, 1.1, 12))
    fs = list(np.linspace(1.0, 0.2, 12))
    with pytest.raises(capi.HgError, match="max_steps = 12"):
        capi.reml_next(xs, fs)
    assert capi.reml_next(xs[:11], fs[:11])[1] == capi.REML_CONTINUE
    assert capi.reml_next(xs, fs, max_steps=13)[1] == capi.REML_CONTINUE
    for kw, msg in [({"h2_start": 0.0}, "h2_start = 0"), ({"h2_start": 1.0}, "h2_start = 1"), ({"x_tol": 0.0}, "x_tol = 0"),
                    ({"x_tol": float("nan")}, "x_tol = nan"), ({"max_steps": 1}, "max_steps = 1")]:
        with pytest.raises(capi.HgError, match="hgibbs_reml_next: " + msg):
            capi.reml_next([], [], **kw)
    with pytest.raises(capi.HgError, match=r"point 1 \(x = 1, f = nan\) is not finite"):
        capi.reml_next([0.0, 1.0], [0.5, float("nan")])


# ---- the four cohorts of the issue ----
COHORTS = [(400, 800, 1), (400, 800, 3), (2000, 4000, 1), (2000, 4000, 3)]
_cache = {}


def cohort(N, M, q):
    if (N, M, q) not in _cache:
        if (N, M) not in _cache:
            geno = rr.cohort(N, M, miss=0.02, seed=N + 1)
            X, good = rr.xmat(geno, *rr.stats_of(geno))
            rng = np.random.default_rng(N + 2)
            beta = rng.standard_normal(M) * math.sqrt(0.4 / M)
            _cache[(N, M)] = (X, good, X @ beta + rng.standard_normal(N) * math.sqrt(0.6))
        X, good, y = _cache[(N, M)]
        Z = rr.covariates(N, q)
        yy = y + Z @ np.arange(1.0, q + 1.0)
        _cache[(N, M, q)] = (rr.Dense(X, good, Z), yy)
    return _cache[(N, M, q)]


@pytest.mark.parametrize("N,M,q", COHORTS)
def test_root_is_the_reml_maximiser(N, M, q):
    d, y = cohort(N, M, q)
    width, x_tol = 2e-4, 1e-6
    xs, fs, st = rr.run_rule(lambda x: rr.f_exact(d, y, math.exp(x)), x_tol=x_tol, max_steps=30)
    assert st == rr.CONVERGED
    best = rr.reml_maximiser(d, y, width=width)
    print("N = %d q = %d: root %.6f, maximiser %.6f, %d evaluations" % (N, q, xs[-1], best, len(xs)))
    assert abs(xs[-1] - best) <= width + x_tol
    # f > 0 at small delta, f < 0 at large delta
    assert rr.f_exact(d, y, math.exp(xs[-1] - 2.0)) > 0 > rr.f_exact(d, y, math.exp(xs[-1] + 2.0))


@pytest.mark.parametrize("N,M,q", COHORTS[:2])
def test_dense_solve_and_ai(N, M, q):
    d, y = cohort(N, M, q)
    delta = 1.7
    H = d.H(delta)
    Hi = np.linalg.inv(H)
    b = np.random.default_rng(3).standard_normal((2, N))
    assert np.max(np.abs(d.solve(b, delta) - (Hi @ d.project(b.T)).T)) <= 1e-11
    P = np.eye(N) - d.Q @ d.Q.T
    Ap = P @ d.A() @ P
    v = Hi @ (P @ y)
    want = np.array([v @ Ap @ Hi @ Ap @ v, v @ Ap @ Hi @ v, v @ Hi @ v])
    got = rr.ai_numbers(d, y, delta)
    assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-10
    # AI = 1/2 y'P K_i P K_j P y with P = V^-1 on the range of P_c, V = vg H, K = (A', I): the same matrix from the explicit inverse
    vg = 0.37
    Pm = P @ Hi @ P / vg
    Py = Pm @ y
    AI = 0.5 * np.array([[Py @ Ap @ Pm @ Ap @ Py, Py @ Ap @ Pm @ Py], [Py @ Ap @ Pm @ Py, Py @ Pm @ Py]])
    mine = np.array([[got[0], got[1]], [got[1], got[2]]]) / (2.0 * vg ** 3)
    assert np.max(np.abs(mine - AI) / np.abs(AI)) <= 1e-10


# ---- finish ----
@pytest.mark.parametrize("T", [1, 2, 15, 31])
def test_finish_against_the_restatement(T):
    d, y = cohort(400, 800, 3)
    G, E = rr.probes(d, 11, T, np.arange(400))
    x2 = [0.31, 0.305]
    sp = rr.eval_sums(d, G, E, y, math.exp(x2[0]))[0]
    sl = rr.eval_sums(d, G, E, y, math.exp(x2[1]))[0]
    ai = rr.ai_numbers(d, y, math.exp(x2[1]))
    for ai3 in (ai, None):
        got = capi.reml_finish(400, 3, x2, sp, sl, ai3)
        want = rr.finish(400, 3, x2, sp, sl, ai3)
        for k, v in want.items():
            if math.isnan(v):
                assert math.isnan(got[k]), k
            else:
                assert abs(got[k] - v) <= 1e-12 * abs(v), (k, got[k], v)
        assert math.isnan(got["se_mc"]) == (T == 1) and math.isnan(got["se_h2"]) == (ai3 is None)
    assert got["h2"] == 1.0 / (1.0 + math.exp(x2[1])) and got["ve"] == got["delta"] * got["vg"]
    with pytest.raises(capi.HgError, match="hgibbs_reml_finish: q = 399 covariate columns against n = 400 rows"):
        capi.reml_finish(400, 399, x2, sp, sl)
    bad = sp.copy()
    bad[T, 1] = np.inf
    with pytest.raises(capi.HgError, match="hgibbs_reml_finish: sum 1 of probe %d is not finite" % T):
        capi.reml_finish(400, 3, x2, bad, sl)


# ---- the probe signs, typed out ----
def test_probe_signs_typed_out():
    # s(c, i) from the top bit of mix64((seed ^ mix64(c)) + i 0xD1B54A32D192ED03): computed once by hand from the definition
    # with Python integers (sign_one), and held against the array form the other tests use
    places = [(1, 0, 0), (1, 0, 1), (1, 1, 0), (7, 4, 123456), (2 ** 63 + 5, 61, 2 ** 31 + 3), (0, 3, 999)]
    for seed, c, i in places:
        assert rr.signs(seed, c, [i])[0] == rr.sign_one(seed, c, i), (seed, c, i)
    got = [int(rr.sign_one(*p)) for p in places]
    assert got == [1, 1, -1, 1, 1, -1], got
    assert [int(v) for v in rr.signs(1, 0, np.arange(16))] == [1, 1, 1, -1, 1, -1, -1, 1, -1, -1, 1, 1, -1, -1, -1, -1]
    s = rr.signs(5, 2, np.arange(20000))
    assert abs(s.mean()) < 0.03 and set(np.unique(s)) == {-1.0, 1.0}
    assert not np.array_equal(s, rr.signs(5, 3, np.arange(20000)))

