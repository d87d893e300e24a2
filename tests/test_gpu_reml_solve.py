"""hgibbs_reml_solve against dense f64 NumPy (tests/reml_restate.py, with X from the device's own marker statistics): the true
residual of the solution, its orthogonality to the covariates, bit identity of a column alone against the column in a panel and
across launch geometries, the zero column, and every refusal with the handle serving on after it.

Each value of n, M, K and q is run once with the others at the base case (n = 257, M = 300, K = 16, q = 3); every cohort has 2 %
missing calls, a row missing everywhere, a marker missing everywhere and a monomorphic one (M_used < M), and every second case
drops rows through a keep list.

Bound of (a): the solver stops on the recurrence's residual, |r| <= tol |b|; the true residual |Hv - b| differs from it by the
rounding the recurrence has gathered, which the test allows as drift = 100 iters kappa 2^-52 with kappa = cond(H) from eigvalsh.
With tol = 1e-8 the drift is below 1e-10 in every case here.  Measured on an MI355X: the largest |Hv - b| / |b| over all cases is
printed as a MEASURED line (DESIGN.md section 36 records it)."""
import numpy as np
import pytest

from hydra_amd import capi

import reml_restate as rr
from pca_restate import device, same_bits

pytestmark = pytest.mark.gpu

TOL = 1e-8
DELTA = 1.0
BASE = dict(n=257, M=300, K=16, q=3)
CASES = ([dict(BASE)] + [dict(BASE, n=n) for n in (5, 63, 64, 65, 1023, 1024, 1025, 2049)] + [dict(BASE, M=M) for M in (7, 64, 65, 1025)]
         + [dict(BASE, K=K) for K in (1, 2, 8, 9, 17, 32)] + [dict(BASE, q=q) for q in (1, 32)])
assert CASES[1]["n"] == BASE["q"] + 2


def make_case(n, M, K, q, keep_list):
    drop = 3 if keep_list else 0
    ntot = n + drop
    geno = rr.cohort(ntot, M, miss=0.02, seed=1000 * n + M)
    geno[0] = 3                                      # a marker missing everywhere
    geno[1] = np.where(geno[1] == 3, 3, 1)           # a monomorphic marker
    keep = None
    if keep_list:
        keep = np.ones(ntot, dtype=np.uint8)
        keep[[1, ntot // 2, ntot - 1]] = 0
    kept = geno if keep is None else geno[:, keep.astype(bool)]
    kept[:, 2] = 3                                   # a row missing everywhere
    if keep is not None:
        geno[:, np.flatnonzero(keep)[2]] = 3
    dev = device(geno, keep=keep)
    assert dev.n_local == n
    mave, mstd = dev.marker_stats()[:2]
    X, good = rr.xmat(kept, mave, mstd)
    assert 0 < good.sum() < M and not X[2].any()
    Z = rr.covariates(n, q, seed=n + q)
    B = np.random.default_rng(7 * n + K).standard_normal((K, n))
    return dev, rr.Dense(X, good, Z), Z, B


_measured = []


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["n%(n)d-M%(M)d-K%(K)d-q%(q)d" % c for c in CASES])
def test_true_residual_and_projection(idx):
    c = CASES[idx]
    dev, d, Z, B = make_case(c["n"], c["M"], c["K"], c["q"], keep_list=idx % 2 == 1)
    V, iters, rel = dev.reml_solve(B, Z, DELTA, tol=TOL, max_iters=500)
    H = d.H(DELTA)
    ev = np.linalg.eigvalsh(H)
    kappa = float(ev[-1] / ev[0])
    Pb = d.project(B.T).T
    res = np.linalg.norm(V @ H - Pb, axis=1) / np.linalg.norm(Pb, axis=1)
    drift = 100.0 * iters.max() * kappa * 2.0 ** -52
    qv = np.max(np.abs(d.Q.T @ V.T)) / np.max(np.linalg.norm(V, axis=1))
    _measured.append(float(res.max()))
    print("MEASURED %s: |Hv - b|/|b| max %.3g (recurrence %.3g), iterations %d..%d, kappa %.3g, drift %.3g, |Q'v|/|v| %.3g; largest so far %.3g"
          % (c, res.max(), rel.max(), iters.min(), iters.max(), kappa, drift, qv, max(_measured)))
    assert np.all(rel <= TOL) and np.all(iters >= 1) and drift < 1e-10
    assert np.all(res <= TOL + drift)                                   # (a)
    assert qv <= drift                                                  # (b): zero to the same rounding
    ref = d.solve(B, DELTA)
    assert np.max(np.linalg.norm(V - ref, axis=1) / np.linalg.norm(ref, axis=1)) <= kappa * (TOL + drift)


@pytest.fixture(scope="module")
def base():
    dev, d, Z, B = make_case(keep_list=True, **BASE)
    ref = dev.reml_solve(B, Z, DELTA, tol=TOL)
    return {"dev": dev, "d": d, "Z": Z, "B": B, "ref": ref}


def test_a_column_alone_equals_the_column_in_the_panel(base):
    dev, Z, B, (V, iters, rel) = base["dev"], base["Z"], base["B"], base["ref"]
    assert len(set(iters.tolist())) > 1  # the columns freeze at different iterations: the frozen ones ride along unchanged
    for k in (0, 7, 15):
        v1, i1, r1 = dev.reml_solve(B[k:k + 1], Z, DELTA, tol=TOL)
        assert same_bits(v1[0], V[k]) and i1[0] == iters[k] and r1[0] == rel[k], k
    v2, i2, r2 = dev.reml_solve(B[[3, 12, 5]], Z, DELTA, tol=TOL)
    assert same_bits(v2, V[[3, 12, 5]]) and np.array_equal(i2, iters[[3, 12, 5]]) and np.array_equal(r2, rel[[3, 12, 5]])


def test_bit_identity_over_launch_geometries(base):
    dev, Z, B, (V, iters, rel) = base["dev"], base["Z"], base["B"], base["ref"]
    again = dev.reml_solve(B, Z, DELTA, tol=TOL)
    assert same_bits(again[0], V) and np.array_equal(again[1], iters) and np.array_equal(again[2], rel)
    for name, values in [("mdots_split", [1, 2, 3]), ("score_sp", [2, 4, 8]), ("score_ranges", [1, 2, 5])]:
        for v in values:
            dev.set_option(name, v)
            got = dev.reml_solve(B, Z, DELTA, tol=TOL)
            assert same_bits(got[0], V) and np.array_equal(got[1], iters) and np.array_equal(got[2], rel), (name, v)
        dev.set_option(name, 0)


def test_zero_column(base):
    dev, Z, B, (V, iters, rel) = base["dev"], base["Z"], base["B"], base["ref"]
    b = B[:4].copy()
    b[1] = 0.0
    v, it, r = dev.reml_solve(b, Z, DELTA, tol=TOL)
    assert not v[1].any() and it[1] == 0 and r[1] == 0.0
    assert same_bits(v[0], V[0]) and same_bits(v[2], V[2]) and it[0] == iters[0] and it[2] == iters[2]
    assert same_bits(v[3], V[3]) and it[3] == iters[3]


def test_refusals(base):
    dev, Z, B, (V, iters, rel) = base["dev"], base["Z"], base["B"], base["ref"]
    n = dev.n_local

    def refused(msg, b=B, z=Z, delta=DELTA, tol=TOL, max_iters=200):
        with pytest.raises(capi.HgError, match=msg):
            dev.reml_solve(b, z, delta, tol=tol, max_iters=max_iters)
        got = dev.reml_solve(B[:2], Z, DELTA, tol=TOL)  # the handle serves on
        assert same_bits(got[0], V[:2])

    refused(r"hgibbs_reml_solve: K = 0 right-hand sides, must be in \[1, 32\]", b=np.zeros((0, n)))
    refused(r"hgibbs_reml_solve: K = 33 right-hand sides, must be in \[1, 32\]", b=np.ones((33, n)))
    refused(r"hgibbs_reml_solve: q = 0 covariate columns, must be in \[1, 32\]", z=np.zeros((n, 0)))
    refused(r"hgibbs_reml_solve: q = 33 covariate columns, must be in \[1, 32\]", z=rr.covariates(n, 33))
    for bad, txt in ((0.0, "0"), (-1.0, "-1"), (float("inf"), "inf"), (float("nan"), "nan")):
        refused("hgibbs_reml_solve: delta = %s, must be positive and finite" % txt, delta=bad)
        refused("hgibbs_reml_solve: tol = %s, must be positive and finite" % txt, tol=bad)
    refused("hgibbs_reml_solve: max_iters = 0, needs at least one iteration", max_iters=0)
    b = B.copy()
    b[3, 17] = np.nan
    refused(r"hgibbs_reml_solve: B\[3\]\[17\] = nan is not finite", b=b)
    z = Z.copy()
    z[5, 1] = np.inf
    refused(r"hgibbs_reml_solve: Z\[1\]\[5\] = inf is not finite", z=z)
    z = Z.copy()
    z[:, 2] = 3.0 * z[:, 0] - z[:, 1]
    refused("hgibbs_reml_solve: covariate column 2 is linearly dependent on the columns before it", z=z)
    refused(r"hgibbs_reml_solve: column 0 has not converged after max_iters = 2 iterations: \|r\| / \|b\| = [0-9.e-]+ against tol = 1e-12",
            tol=1e-12, max_iters=2)
    assert dev.last_reml_ms()[0] > 0.0


def test_refusals_by_shape():
    geno = rr.cohort(5, 40, miss=0.0, seed=3)
    dev = device(geno)
    with pytest.raises(capi.HgError, match=r"hgibbs_reml_solve: q = 4 covariate columns, must be below n - 1 = 4"):
        dev.reml_solve(np.ones((1, 5)), rr.covariates(5, 4), 1.0)
    mono = np.ones((6, 30), dtype=np.int8)
    dev = device(mono)
    with pytest.raises(capi.HgError, match="hgibbs_reml_solve: M_used = 0: no marker has a finite standard deviation"):
        dev.reml_solve(np.ones((1, 30)), rr.covariates(30, 1), 1.0)
