"""hydra_mi355x --he against the binding (Device.grm_rowsums and capi.he_fit on the same kept rows and the same projected phenotype),
and a planted-signal run as a sanity check on the statistics."""
import math
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")

pytestmark = pytest.mark.gpu


def make(N, M, seed):
    """tests/test_gpu_grm.py's recipe"""
    geno = synth.make_genotypes(M, N, seed=seed)
    rng = np.random.default_rng(seed + 7)
    for j in rng.choice(M, size=max(1, M // 5), replace=False):  # 1-5 % missing calls in a fifth of the columns
        geno[j, rng.random(N) < rng.uniform(0.01, 0.05)] = 3
    if M >= 3:
        geno[M // 3] = 3  # a marker missing everywhere
        geno[M // 2] = 1 if M % 2 else 0  # a monomorphic marker
    if M >= 5:
        geno[M - 2] = 2
    if N >= 3:
        geno[:, N // 2] = 3  # an individual missing everywhere
    if N >= 6:
        geno[:, 1] = geno[:, N - 1]  # a duplicate
    return geno


# ---- the CLI's phenotype, operation by operation (hydra_main.cpp: scale_phenotype, CovProjector), so that it is the same f64 vector ----
def scale(y):
    n = len(y)
    mean = 0.0
    for v in y:
        mean += v
    mean /= n
    y = [v - mean for v in y]
    sq = 0.0
    for v in y:
        sq += v * v
    sq = math.sqrt(float(n - 1) / sq)
    return [v * sq for v in y]


def project(y, cov):
    n, C = cov.shape
    q = 1 + C
    Z = [[1.0] * n] + [[float(cov[i, c]) for i in range(n)] for c in range(C)]

    def dot(u, v):
        s = 0.0
        for a, b in zip(u, v):
            s += a * b
        return s

    L = [[dot(Z[a], Z[b]) for b in range(q)] for a in range(q)]
    for k in range(q):  # Cholesky, in place, lower triangle
        d = L[k][k]
        for p in range(k):
            d -= L[k][p] * L[k][p]
        d = math.sqrt(d)
        L[k][k] = d
        for i in range(k + 1, q):
            v = L[i][k]
            for p in range(k):
                v -= L[i][p] * L[k][p]
            L[i][k] = v / d
    w = [dot(Z[a], y) for a in range(q)]
    for i in range(q):
        for p in range(i):
            w[i] -= L[i][p] * w[p]
        w[i] /= L[i][i]
    for i in range(q - 1, -1, -1):
        for p in range(i + 1, q):
            w[i] -= L[p][i] * w[p]
        w[i] /= L[i][i]
    y = list(y)
    for a in range(q):
        for i in range(n):
            y[i] -= Z[a][i] * w[a]
    return y


def close(tok, want, digits):
    """a %.<digits>g token against the value it was printed from: half a unit of the last digit is at most 5 10^-digits |value|"""
    v = float(tok)
    if math.isnan(want):
        return math.isnan(v)
    return abs(v - want) <= 5.0 * 10.0 ** -digits * abs(want)


def parse_hereg(path):
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[0] == "HE-CP" and lines[4] == "" and lines[5] == "HE-SD" and lines[9:] == [""], lines
    out = {}
    for form, at in (("cp", 0), ("sd", 5)):
        assert lines[at + 1] == "Coefficient\tEstimate\tSE_OLS\tSE_Jackknife\tP_OLS\tP_Jackknife"
        for name, ln in (("Intercept", lines[at + 2]), ("V(G)/Vp", lines[at + 3])):
            tok = ln.split("\t")
            assert tok[0] == name and len(tok) == 6, ln
            out[form, name] = tok[1:]
    return out


@pytest.mark.parametrize("with_cov", [False, True])
def test_cli_against_the_binding(tmp_path, with_cov):
    N, M = 200, 300
    geno = make(N, M, seed=23)
    y = np.random.default_rng(4).standard_normal(N)
    na = [3, 150]
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=na)
    cov = np.random.default_rng(6).standard_normal((N, 2))
    cov[:, 1] = cov[:, 1] * 3.0 + 10.0
    with open(prefix + ".cov", "w") as f:
        for i in range(N):
            f.write("fam%d ind%d %.17g %.17g\n" % (i, i, cov[i, 0], cov[i, 1]))
    kept = np.setdiff1d(np.arange(N), na)
    n = len(kept)
    assert n == 198
    odir = str(tmp_path / "o")
    cmd = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", odir, "--mcmc-out-name", "n",
           "--number-individuals", str(N), "--number-markers", str(M)] + (["--covariates", prefix + ".cov"] if with_cov else []) + ["--he"]
    out = str(tmp_path / "h.txt")
    r = subprocess.run(cmd + ["--he-rows", "--he-out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr

    # the same kept rows and the same phenotype through the binding
    yk = scale([float(v) for v in y[kept]])
    if with_cov:
        yk = scale(project(yk, cov[kept]))
    yk = np.array(yk)
    keep = np.zeros(N, dtype=np.uint8)
    keep[kept] = 1
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N, keep=keep)
    ay, a1, a2, diag, partners = dev.grm_rowsums(np.stack([yk, yk * yk]))
    m_used, _ = dev.grm_info()
    fit = capi.he_fit(yk, ay[:, 0], ay[:, 1], a1, a2, partners)
    lost = int(np.flatnonzero(kept == N // 2)[0])  # the individual missing everywhere
    assert partners[lost] == 0 and fit["n_left_out"] == 1 and fit["n_used"] == n - 1

    got = parse_hereg(out)
    for form in ("cp", "sd"):
        g = fit[form]
        want = {"Intercept": [g["intercept"], g["intercept_se"], g["intercept_se_jk"], g["intercept_p"], g["intercept_p_jk"]],
                "V(G)/Vp": [g["h2"], g["h2_se"], g["h2_se_jk"], g["slope_p"], g["slope_p_jk"]]}
        for name, vals in want.items():
            for tok, v in zip(got[form, name], vals):
                assert close(tok, v, 9), (form, name, tok, v)
    with open(out + ".rows") as f:
        rows = [ln.split("\t") for ln in f.read().splitlines()]
    assert rows[0] == ["FID", "IID", "NPARTNERS", "A_DIAG", "A_SUM", "A_SQSUM", "AY"] and len(rows) == n + 1
    for x, i in enumerate(kept):
        t = rows[1 + x]
        assert t[:3] == ["fam%d" % i, "ind%d" % i, str(int(partners[x]))], t
        for tok, v in zip(t[3:], (diag[x], a1[x], a2[x], ay[x, 0])):
            assert close(tok, v, 12), (i, tok, v)

    # standard output
    assert "HE     : %d rows, %d of %d markers used, %d pairs, 1 rows left out, %d covariates -> %s" % (
        n, m_used, M, (n - 1) * (n - 2) // 2, 2 if with_cov else 0, out) in r.stdout, r.stdout
    assert "HE     : HE-CP V(G)/Vp %.6g " % fit["cp"]["h2"] in r.stdout and "HE-SD V(G)/Vp %.6g " % fit["sd"]["h2"] in r.stdout, r.stdout
    assert "HE     : products " in r.stdout and " ms, reduce " in r.stdout and "the per-row sums in %s.rows" % out in r.stdout
    assert "WARNING: --he leaves out fam%d ind%d" % (N // 2, N // 2) in r.stdout

    # the default output path is <dir>/<name>.HEreg, without --he-rows no .rows
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(odir, "n.HEreg")) as f, open(out) as g:
        assert f.read() == g.read()
    assert not os.path.exists(os.path.join(odir, "n.HEreg.rows"))


def test_planted_signal():
    """A sanity check on the statistics, not a tolerance on the kernel: y simulated from the standardised genotypes with h2 = 0.5."""
    N, M, h2 = 2000, 4000, 0.5
    geno = synth.make_genotypes(M, N, seed=77, maf_lo=0.05)
    rng = np.random.default_rng(78)
    g = geno.T.astype(np.float64)
    X = (g - g.mean(axis=0)) / g.std(axis=0)
    y = X @ rng.standard_normal(M) * math.sqrt(h2 / M) + rng.standard_normal(N) * math.sqrt(1.0 - h2)
    y = (y - y.mean()) / y.std(ddof=1)
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    ay, a1, a2, _, partners = dev.grm_rowsums(np.stack([y, y * y]))
    fit = capi.he_fit(y, ay[:, 0], ay[:, 1], a1, a2, partners)
    assert fit["n_used"] == N and fit["n_left_out"] == 0

    # dense NumPy HE on the same matrix
    S, nsnp = dev.grm()
    a, b = np.tril_indices(N)
    offd = a != b
    x = (S / nsnp)[offd]
    a, b = a[offd], b[offd]
    vp = y.var(ddof=1)
    dense = {}
    for form, z, k in (("cp", y[a] * y[b], 1.0 / vp), ("sd", (y[a] - y[b]) ** 2, -0.5 / vp)):
        xc = x - x.mean()
        dense[form] = k * float(xc @ (z - z.mean()) / (xc @ xc))
    cp, sd = fit["cp"], fit["sd"]
    print("MEASURED planted h2 %.2f: HE-CP %.4f (jackknife SE %.4f, dense %.4f), HE-SD %.4f (jackknife SE %.4f, dense %.4f)"
          % (h2, cp["h2"], cp["h2_se_jk"], dense["cp"], sd["h2"], sd["h2_se_jk"], dense["sd"]))
    assert abs(cp["h2"] - sd["h2"]) <= 4.0 * max(cp["h2_se_jk"], sd["h2_se_jk"])
    assert abs(cp["h2"] - dense["cp"]) <= 4.0 * cp["h2_se_jk"]
    assert abs(sd["h2"] - dense["sd"]) <= 4.0 * sd["h2_se_jk"]
