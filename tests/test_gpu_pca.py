"""hgibbs_pca against NumPy in f64: the dense eigendecomposition of Z Z'/M_used and a plain restatement of the algorithm (block subspace
iteration with Householder QR in place of CholeskyQR), the properties of the result, bit identity across launch geometries and
against the NumPy twin of the start panel, population structure, odd shapes, a size where the products take several slices and
ranges, every refusal, and the --pca command line.

Bounds of the comparison with NumPy (VEC_BOUND on max_k |v_k - s_k v_k^ref|_2, VAL_BOUND relative on the eigenvalues): ten times the
larger value measured on an MI355X for the base case against numpy.linalg.eigh (vectors 7.2e-15 at L = 8 and
8.8e-15 at L = 16, eigenvalues 1.5e-15 and 2.2e-15), never above 1e-9 and 1e-12.  The rounding of the operators' inputs is amplified
by 1 / gap of the wanted eigenvalues (about 30 in the base case), so the other cases draw populations of unequal sizes, whose
eigenvalues are further apart than the base case's: the bound measures the code, not the conditioning of a test's data."""
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import capi, synth

from pca_restate import VAL_BOUND, VEC_BOUND, dense, device, numpy_pca, same_bits, start_panel, structured, val_err, vec_err, zmat

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")

assert VEC_BOUND == 8.8e-14 and VAL_BOUND == 2.2e-14  # (the bounds of the docstring above; they live beside the shared helpers)


def between_share(v, pop):
    tot = np.sum((v - v.mean()) ** 2)
    return sum(np.sum(pop == p) * (v[pop == p].mean() - v.mean()) ** 2 for p in np.unique(pop)) / tot


N0, M0 = 1500, 6000


@pytest.fixture(scope="module")
def base():
    geno, pop = structured(N0, M0, P=4, F=0.02, miss=0.02, seed=1)
    geno[:, 700] = 3     # an individual with every call missing
    geno[100] = 3        # a marker missing everywhere
    geno[200] = np.where(geno[200] == 3, 3, 1)  # a monomorphic marker
    Z, good = zmat(geno)
    m_used = int(good.sum())
    assert m_used == M0 - 2
    lam, U = dense(Z, m_used, 3)
    Q0 = {L: np.random.default_rng(100 + L).standard_normal((L, N0)) for L in (8, 16)}
    return {"geno": geno, "pop": pop, "Z": Z, "good": good, "m": m_used, "lam": lam, "U": U, "Q0": Q0, "dev": device(geno)}


# ---- 1. against the dense eigendecomposition ----
@pytest.mark.parametrize("L", [8, 16])
def test_matches_dense_eigendecomposition(base, L):
    Z, m, lam, U = base["Z"], base["m"], base["lam"], base["U"]
    rval, rV, rld, _ = numpy_pca(Z, m, 3, L, 20, 0.0, base["Q0"][L])
    print("restatement vs eigh, L = %d: vectors %.3g, eigenvalues %.3g" % (L, vec_err(rV, U), val_err(rval, lam[:3])))
    assert vec_err(rV, U) <= 1e-13 and val_err(rval, lam[:3]) <= 1e-14
    val, V, ld, rep = base["dev"].pca(3, L=L, iters=20, tol=0.0, Q0=base["Q0"][L], loadings=True)
    ev, el = vec_err(V, U), val_err(val, lam[:3])
    print("MEASURED L = %d: device vs eigh: vectors %.3g, eigenvalues %.3g; vs restatement: vectors %.3g, eigenvalues %.3g; loadings %.3g"
          % (L, ev, el, vec_err(V, rV), val_err(val, rval), vec_err(ld[:, base["good"]], rld[:, base["good"]])))
    assert rep["iters_run"] == 20 and rep["m_used"] == m
    assert ev <= VEC_BOUND
    assert el <= VAL_BOUND


# ---- 2. properties ----
def test_properties(base):
    Z, m, good = base["Z"], base["m"], base["good"]
    dev = base["dev"]
    val, V, ld, rep = dev.pca(3, L=8, iters=20, tol=0.0, Q0=base["Q0"][8], loadings=True)
    assert np.max(np.abs(V @ V.T - np.eye(3))) <= 1e-13
    assert np.max(np.abs(V.sum(axis=1))) <= 1e-10
    for k in range(3):
        at = int(np.argmax(np.abs(V[k])))
        assert V[k, at] > 0
    assert np.all(V[:, 700] == 0.0)  # every call missing: an empty sum
    assert not good[100] and not good[200] and rep["m_used"] == M0 - 2
    assert np.isnan(ld[:, ~good]).all() and np.isfinite(ld[:, good]).all()
    assert np.max(np.abs(np.sum(ld[:, good] ** 2, axis=1) - 1.0)) <= 1e-12
    want = (Z.T @ V.T / np.sqrt(m * val)).T
    print("MEASURED loadings vs Z'v / sqrt(M lambda): %.3g" % vec_err(ld[:, good], want[:, good]))
    assert vec_err(ld[:, good], want[:, good]) <= VEC_BOUND
    res = np.array([np.linalg.norm(Z @ (Z.T @ V[k]) / m - val[k] * V[k]) / val[k] for k in range(3)])
    print("MEASURED residuals at 20 iterations: report %s, NumPy %s" % (rep["resid"], res))
    assert np.all(rep["resid"] <= 1e-8) and np.all(res <= 1e-8)
    # cut short: the residual is far above rounding, and the report agrees with NumPy on the returned pair
    val, V, _, rep = dev.pca(3, L=8, iters=4, tol=0.0, Q0=base["Q0"][8])
    res = np.array([np.linalg.norm(Z @ (Z.T @ V[k]) / m - val[k] * V[k]) / val[k] for k in range(3)])
    print("residuals at 4 iterations: report %s, NumPy %s" % (rep["resid"], res))
    assert rep["iters_run"] == 4 and np.all(res > 1e-8)
    assert np.all(np.abs(rep["resid"] - res) <= 1e-3 * res)


def test_without_report(base):
    """rep = NULL (no residuals, no extra products), which the Python binding never passes: the same bytes as the reporting call,
    also after a single iteration, where no X T product runs at all"""
    dev, Q0 = base["dev"], base["Q0"][8]
    n, M = dev.n_local, dev.M
    for iters in (1, 5):
        ref = dev.pca(3, L=8, iters=iters, tol=0.0, Q0=Q0, loadings=True)
        val, pcs, ld = np.zeros(3), np.zeros((3, n)), np.zeros((3, M))
        q = np.ascontiguousarray(Q0)
        capi.check(dev.L.hgibbs_pca(dev.h, 3, 8, iters, 0.0, capi._dp(q), 0, capi._dp(val), capi._dp(pcs), capi._dp(ld), None))
        assert same_bits(val, ref[0]) and same_bits(pcs, ref[1]) and same_bits(ld, ref[2]), iters
        assert ref[3]["iters_run"] == iters


# ---- 3. bit identity ----
def test_bit_identity(base):
    dev = device(base["geno"])
    Q0 = base["Q0"][8]

    def run(**kw):
        val, V, ld, _ = dev.pca(3, L=8, iters=6, tol=0.0, loadings=True, **kw)
        return val, V, ld

    ref = run(Q0=Q0)
    again = run(Q0=Q0)
    assert all(same_bits(a, b) for a, b in zip(ref, again))
    for name, values in [("mdots_split", [1, 2, 3]), ("score_sp", [2, 4, 8]), ("score_ranges", [1, 2, 5])]:
        for v in values:
            dev.set_option(name, v)
            got = run(Q0=Q0)
            assert all(same_bits(a, b) for a, b in zip(ref, got)), (name, v)
        dev.set_option(name, 0)
    seeded = run(seed=77)
    twin = run(Q0=start_panel(77, 8, N0))
    assert all(same_bits(a, b) for a, b in zip(seeded, twin))
    other = run(seed=78)
    assert not same_bits(seeded[1], other[1])
    val, V, _, _ = dev.pca(3, L=8, iters=20, tol=0.0, seed=78)
    assert vec_err(V, base["U"]) <= VEC_BOUND and val_err(val, base["lam"][:3]) <= VAL_BOUND


# ---- 4. structure, early stop ----
def test_structure_and_early_stop(base):
    dev, lam = base["dev"], base["lam"]
    val, V, _, rep = dev.pca(4, L=16, iters=20, tol=0.0, seed=5)
    shares = [between_share(V[k], base["pop"]) for k in range(3)]
    print("between-population shares %s, lambda %s" % (shares, val))
    assert min(shares) >= 0.95
    assert val[2] / val[3] >= 3.0
    val, V, _, rep = dev.pca(3, iters=40, tol=1e-10, seed=5)
    print("early stop after %d iterations, last change %.3g" % (rep["iters_run"], rep["ritz_change"]))
    assert rep["iters_run"] < 20 and rep["ritz_change"] <= 1e-10
    assert val_err(val, lam[:3]) <= 1e-8


# ---- 5. shapes ----
SHAPES = {
    "n1501_m3003": dict(N=1501, M=3003, K=3, L=8, miss=0.02),
    "n777_m2999_k1": dict(N=777, M=2999, K=1, L=8, miss=0.02),
    "k_equals_l": dict(N=777, M=4001, K=8, L=8, miss=0.02, P=9, sizes=[5, 6, 7, 8, 9, 10, 11, 12, 13], F=0.1),
    "l32": dict(N=1501, M=3003, K=3, L=32, miss=0.02),
    "keep": dict(N=1501, M=3003, K=3, L=16, miss=0.02, drop=97),
    "clean": dict(N=1030, M=3003, K=3, L=8, miss=0.0),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(name):
    c = dict(SHAPES[name])
    N, M, K, L = c["N"], c["M"], c["K"], c["L"]
    geno, pop = structured(N, M, P=c.get("P", 4), F=c.get("F", 0.02), miss=c["miss"], seed=11, sizes=c.get("sizes", [3, 4, 5, 6]))
    keep = None
    if "drop" in c:
        keep = np.ones(N, dtype=np.uint8)
        keep[np.random.default_rng(3).choice(N, size=c["drop"], replace=False)] = 0
    dev = device(geno, keep=keep)
    if keep is not None:
        geno = geno[:, keep != 0]
    n = geno.shape[1]
    assert dev.n_local == n and (n % 16 or c["miss"] == 0.0)
    Z, good = zmat(geno)
    Q0 = np.random.default_rng(7).standard_normal((L, n))
    rval, rV, rld, _ = numpy_pca(Z, int(good.sum()), K, L, 20, 0.0, Q0)
    val, V, ld, rep = dev.pca(K, L=L, iters=20, tol=0.0, Q0=Q0, loadings=True)
    print("%s: vectors %.3g, eigenvalues %.3g, loadings %.3g" % (name, vec_err(V, rV), val_err(val, rval), vec_err(ld[:, good], rld[:, good])))
    assert rep["m_used"] == int(good.sum())
    assert vec_err(V, rV) <= VEC_BOUND
    assert val_err(val, rval) <= VAL_BOUND
    assert vec_err(ld[:, good], rld[:, good]) <= VEC_BOUND
    assert np.max(np.abs(V @ V.T - np.eye(K))) <= 1e-13


def test_refusals(base):
    dev = base["dev"]
    n = dev.n_local
    with pytest.raises(capi.HgError, match="no genotypes"):
        capi.Device(0).pca(3)
    with pytest.raises(capi.HgError, match="K = 0, needs at least one component"):
        dev.pca(0, L=8)
    with pytest.raises(capi.HgError, match="K = 9 above the panel width L = 8"):
        dev.pca(9, L=8)
    with pytest.raises(capi.HgError, match="L = 33, at most 32"):
        dev.pca(3, L=33)
    with pytest.raises(capi.HgError, match="iters = 0"):
        dev.pca(3, iters=0)
    for t in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(capi.HgError, match="must be finite and not negative"):
            dev.pca(3, tol=t)
    Q0 = np.ones((8, n))
    Q0[3, 5] = np.nan
    with pytest.raises(capi.HgError, match=r"Q0\[3\]\[5\] = nan is not finite"):
        dev.pca(3, L=8, Q0=Q0)
    with pytest.raises(capi.HgError, match="lost rank"):
        dev.pca(3, L=8, Q0=np.ones((8, n)))  # linearly dependent start vectors: not papered over
    geno, _ = structured(20, 40, miss=0.0, seed=2)
    small = device(geno)
    with pytest.raises(capi.HgError, match="L = 24, must be below the 20 individuals"):
        small.pca(10, L=24)
    geno, _ = structured(200, 12, miss=0.0, seed=2)
    few = device(geno)
    with pytest.raises(capi.HgError, match="L = 16 above the 12 markers"):
        few.pca(3, L=16)
    # marker-dots' own limit, checked before the marker stats and any allocation: 2^29 rows of one marker (a 128 MiB BED made in HBM)
    big = capi.Device(0)
    big.synth_bed(1 << 29, 1, seed=3)
    with pytest.raises(capi.HgError, match="536870912 individuals, at most 536870911"):
        big.pca(1, L=8)
    big.close()
    # free device memory: 5e8 rows on a panel of 32 need 3 x 8 n L = 384 GB for Q, Q1 and Y alone and 256 GB for the score sums,
    # more than any device this library runs on holds (an MI355X has 288 GB), whatever else is resident; the BED itself is 4 GB
    big = capi.Device(0)
    big.synth_bed(500_000_000, 32, seed=3)
    with pytest.raises(capi.HgError, match=r"the panels and work buffers need [0-9.]+ MiB, [0-9.]+ MiB of device memory are free"):
        big.pca(1, L=32)
    big.close()
    ranks = capi.Device(0)
    ranks.comm_init_external(2, 0, lambda arr: None)
    ranks.load_bed(synth.pack_bed_columns(base["geno"]), N0, row_begin=0, row_end=N0 // 2, n_global=N0)
    with pytest.raises(capi.HgError, match="one rank only"):
        ranks.pca(3)


# ---- 6. size ----
def test_size():
    N, M, K = 100_000, 50_000, 10
    dev = capi.Device(0)
    dev.synth_bed(N, M, seed=9, missing_rate=0.01)
    mave, mstd, *_ = dev.marker_stats()
    val, V, _, rep = dev.pca(K, iters=3, tol=0.0, seed=4)
    ms = dev.last_pca_ms()
    print("N = %d, M = %d, K = %d, 3 iterations: device ms %s" % (N, M, K, ms))
    assert np.isfinite(val).all() and np.isfinite(V).all()
    assert np.max(np.abs(V @ V.T - np.eye(K))) <= 1e-12
    m = int(np.isfinite(mstd).sum())
    assert rep["m_used"] == m and rep["iters_run"] == 3
    assert ms[0] > 0 and ms[0] >= ms[1] + ms[2] + ms[3] - 1e-6
    # the residual of the first two PCs through the public host-pointer operators
    T = dev.marker_dots(V[:2])
    T[~np.isfinite(mstd)] = 0.0
    sd = np.where(np.isfinite(mstd), mstd, 0.0)
    a = (T * sd[:, None]).T
    o = -(a * mave[None, :])
    Y = dev.score(a, o)
    for k in range(2):
        r = np.linalg.norm(Y[:, k] / m - val[k] * V[k]) / val[k]
        print("PC%d: residual %.6g from the host, %.6g reported" % (k + 1, r, rep["resid"][k]))
        assert r > 1e-6
        assert abs(rep["resid"][k] - r) <= 1e-6 * r


# ---- 7. the command line ----
def test_cli(tmp_path):
    N, M = 400, 1500
    geno, _ = structured(N, M, P=3, F=0.05, miss=0.02, seed=21)
    y = np.random.default_rng(4).standard_normal(N)
    na = [3, 21, 50, 51, 399]
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=na)
    kept = np.setdiff1d(np.arange(N), na)
    out = str(tmp_path / "o")
    base = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", out,
            "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(M), "--seed", "12"]
    r = subprocess.run(base + ["--pca", "3", "--pca-loadings"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    keep = np.ones(N, dtype=np.uint8)
    keep[na] = 0
    dev = device(geno, keep=keep)
    val, V, ld, rep = dev.pca(3, iters=20, tol=1e-10, seed=12, loadings=True)
    want = ["#FID\tIID\tPC1\tPC2\tPC3"] + ["fam%d\tind%d\t%s" % (i, i, "\t".join("%.12g" % V[k, a] for k in range(3))) for a, i in enumerate(kept)]
    with open(out + "/n.eigenvec") as f:
        assert f.read().splitlines() == want
    with open(out + "/n.eigenval") as f:
        assert f.read().splitlines() == ["%.12g" % v for v in val]
    with open(out + "/n.cov") as f:
        cov = f.read().splitlines()
    at = {int(i): a for a, i in enumerate(kept)}
    assert cov == ["fam%d ind%d %s" % (i, i, " ".join("%.12g" % V[k, at[i]] for k in range(3)) if i in at else "NA NA NA") for i in range(N)]
    with open(out + "/n.var") as f:
        var = f.read().splitlines()
    assert var[0] == "#CHR\tSNP\tA1\tA2\tPC1\tPC2\tPC3" and len(var) == M + 1
    assert var[1:] == ["1\tsnp%d\tA\tC\t%s" % (j, "\t".join("%.12g" % ld[k, j] for k in range(3))) for j in range(M)]
    assert "PCA    : %d rows, %d markers used, panel of 16, %d iterations run" % (len(kept), rep["m_used"], rep["iters_run"]) in r.stdout
    # the .cov file feeds --covariates as it stands, and a dropped row stays dropped (no chain has run: no LOCO offsets to take)
    r = subprocess.run(base + ["--covariates", out + "/n.cov", "--assoc", "--assoc-no-loco"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "3 covariates, %d individuals" % len(kept) in r.stdout
    r = subprocess.run(base + ["--covariates", out + "/n.cov", "--chain-length", "5", "--thin", "1", "--save", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # --pca-out F: <out> is F without its .eigenvec; a monomorphic marker is outside M_used and has NA loadings
    geno[7] = np.where(geno[7] == 3, 3, 2)
    synth.write_plink(prefix + "_m", synth.pack_bed_columns(geno), N, y=y, na_rows=na)
    alt = str(tmp_path / "alt.eigenvec")
    args = [(prefix + "_m" + a[len(prefix):] if a.startswith(prefix) else a) for a in base]
    r = subprocess.run(args + ["--pca", "2", "--pca-iters", "3", "--pca-tol", "0", "--pca-loadings", "--pca-out", alt],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "%d markers used, panel of 16, 3 iterations run" % (M - 1) in r.stdout
    for ext in (".eigenvec", ".eigenval", ".cov", ".var"):
        assert os.path.exists(str(tmp_path / "alt") + ext)
    with open(str(tmp_path / "alt.var")) as f:
        var = f.read().splitlines()
    assert len(var) == M + 1 and var[8] == "1\tsnp7\tA\tC\tNA\tNA"
    assert all("NA" not in line for line in var[1:8] + var[9:])
