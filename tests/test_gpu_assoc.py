"""hydra_mi355x --assoc after a short real chain: every row of the table against a NumPy restatement (LOCO residuals from the .bet,
covariates projected out), --assoc-no-loco against an independent full OLS fit, and --assoc-out."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402

pytestmark = pytest.mark.gpu

N, M, MN = 2000, 200, 193  # individuals, .bim / .bed rows, --number-markers
NA_PHEN = [3, 17, 400, 1999]
NA_COV = 250
MONO = 77  # made monomorphic after the chain (a chain cannot take one: its scale divides by zero)


def chrom_of(j):  # three chromosomes; "1" in two non-adjacent runs
    return "1" if j < 60 else "2" if j < 120 else "1" if j < 150 else "3"


def oracle_stats(geno):
    L = orc.load()
    Mx, Nx = geno.shape
    mave, mstd = np.zeros(Mx), np.zeros(Mx)
    for j in range(Mx):
        n1, n2, nm = (int(np.count_nonzero(geno[j] == v)) for v in (1, 2, 3))
        a, s = C.c_double(), C.c_double()
        L.orc_marker_stats(n1, n2, nm, Nx, C.byref(a), C.byref(s))
        mave[j], mstd[j] = a.value, s.value
    return mave, mstd


def read_bet(path):
    raw = open(path, "rb").read()
    m = int(np.frombuffer(raw[:4], np.uint32)[0])
    rec = 4 + 8 * m
    n = (len(raw) - 4) // rec
    its = np.array([int(np.frombuffer(raw[4 + k * rec:8 + k * rec], np.uint32)[0]) for k in range(n)])
    betas = np.stack([np.frombuffer(raw[8 + k * rec:4 + (k + 1) * rec], np.float64) for k in range(n)])
    return its, betas


def read_table(path):
    with open(path) as f:
        assert f.readline().split() == ["CHR", "SNP", "BP", "A1", "A2", "FREQ", "N", "BETA", "SE", "CHISQ", "P"]
        return [line.split() for line in f]


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("assoc")
    geno = synth.make_genotypes(M, N, seed=31, missing_rate=0.01)
    y, _ = synth.make_phenotype(geno, seed=32, causal_frac=0.1)
    prefix = str(tmp / "train")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=NA_PHEN)
    bp = np.cumsum(np.random.default_rng(5).integers(1, 500, size=M)) + 1000
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%s snp%d 0 %d G T\n" % (chrom_of(j), j, bp[j]))
    cov = np.random.default_rng(6).standard_normal((N, 2))
    cov[:, 1] = cov[:, 1] * 3.0 + 10.0
    with open(prefix + ".cov", "w") as f:
        for i in range(N):
            f.write("fam%d ind%d %s\n" % (i, i, "NA 1.0" if i == NA_COV else "%.17g %.17g" % (cov[i, 0], cov[i, 1])))
    out = str(tmp / "out")
    base = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--covariates", prefix + ".cov",
            "--mcmc-out-dir", out, "--mcmc-out-name", "r", "--number-individuals", str(N), "--number-markers", str(MN),
            "--chain-length", "8", "--thin", "1", "--save", "7", "--seed", "9"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    geno[MONO] = np.where(geno[MONO] == 3, 3, 1)
    synth.write_plink(prefix + "_m", synth.pack_bed_columns(geno), N)
    os.replace(prefix + "_m.bed", prefix + ".bed")
    base = [a for a in base if a not in ("--chain-length", "8", "--save", "7")] + ["--burn-in", "3"]
    kept = np.ones(N, dtype=bool)
    kept[NA_PHEN] = False
    kept[NA_COV] = False
    return dict(geno=geno, y=y, cov=cov, kept=kept, bp=bp, out=out, base=base)


def restate(ch, loco):
    kept = ch["kept"]
    g = ch["geno"][:MN][:, kept]
    n = g.shape[1]
    yk = ch["y"][kept] - np.mean(ch["y"][kept])
    yk *= math.sqrt((n - 1) / np.dot(yk, yk))
    Z = np.column_stack([np.ones(n), ch["cov"][kept]])
    mave, mstd = oracle_stats(g)
    ok = np.isfinite(mstd)
    with np.errstate(invalid="ignore"):
        x = np.where(g == 3, 0.0, (g - mave[:, None]) * mstd[:, None])
    x[~ok] = 0.0
    chroms = np.array([chrom_of(j) for j in range(MN)])
    if loco:
        its, betas = read_bet(ch["out"] + "/r.bet")
        bbar = betas[its >= 3].mean(axis=0)
        assert bbar.shape == (MN,) and np.count_nonzero(bbar) > 0
        Gc = {c: (bbar[chroms == c] * ok[chroms == c]) @ x[chroms == c] for c in set(chroms)}
        G = sum(Gc.values())
    proj = lambda v: v - Z @ np.linalg.lstsq(Z, v, rcond=None)[0]  # noqa: E731
    ZtZinv = np.linalg.inv(Z.T @ Z)
    rows = []
    for j in range(MN):
        r = proj(yk - (G - Gc[chroms[j]]) if loco else yk)
        s, t, xx = x[j] @ r, Z.T @ x[j], x[j] @ x[j]
        v = xx - t @ ZtZinv @ t
        if not ok[j] or v <= 1e-9 * xx:
            rows.append(None)
            continue
        b = s / v
        s2 = (r @ r - s * s / v) / (n - Z.shape[1] - 1)
        se = math.sqrt(s2 / v)
        rows.append((b * mstd[j], se * mstd[j], b * b / (se * se), mave[j] / 2, int(np.count_nonzero(g[j] != 3))))
    return rows, x, yk, Z


def check_rows(table, ref, ch):
    assert len(table) == MN
    for j, (row, want) in enumerate(zip(table, ref)):
        assert row[:5] == [chrom_of(j), "snp%d" % j, str(ch["bp"][j]), "G", "T"], j
        if want is None:
            assert row[7:] == ["NA"] * 4, (j, row)
            continue
        beta, se, chisq, freq, ncalled = want
        assert int(row[6]) == ncalled and abs(float(row[5]) - freq) <= 1e-11, (j, row)
        # 1e-9 relative; an effect near 0 is held to 1e-12 of its SE instead
        for got, w, floor in zip(map(float, row[7:10]), (beta, se, chisq), (1e-12 * se, 0.0, 1e-13)):
            assert abs(got - w) <= 1e-9 * abs(w) + floor, (j, row, want)
        p = math.erfc(math.sqrt(float(row[9]) / 2))
        assert abs(float(row[10]) - p) <= 1e-9 * p, (j, row)
    na = [j for j, row in enumerate(table) if row[7] == "NA"]
    assert na == [MONO]


def test_assoc_loco_matches_numpy(chain):
    r = subprocess.run(chain["base"] + ["--assoc"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ASSOC  : %d markers, 3 chromosomes in 4 runs, 2 covariates, %d individuals" % (MN, int(chain["kept"].sum())) in r.stdout
    assert "wrote %d rows" % MN in r.stdout
    table = read_table(chain["out"] + "/r.assoc")
    ref, *_ = restate(chain, loco=True)
    check_rows(table, ref, chain)
    # the same table through --assoc-out
    alt = chain["out"] + "/alt.assoc"
    r = subprocess.run(chain["base"] + ["--assoc", "--assoc-out", alt], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(alt).read() == open(chain["out"] + "/r.assoc").read()


def test_assoc_no_loco_matches_full_ols(chain):
    out = chain["out"] + "/nl.assoc"
    r = subprocess.run(chain["base"] + ["--assoc", "--assoc-no-loco", "--assoc-out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    table = read_table(out)
    ref, x, yk, Z = restate(chain, loco=False)
    check_rows(table, ref, chain)
    # independent of the projection algebra: a full OLS fit of [Z, x_j] on the scaled phenotype
    n, q = Z.shape
    mave, mstd = oracle_stats(chain["geno"][:MN][:, chain["kept"]])
    for j in (0, 5, 61, 130, 190):
        A = np.column_stack([Z, x[j]])
        coef, *_ = np.linalg.lstsq(A, yk, rcond=None)
        res = yk - A @ coef
        s2 = res @ res / (n - q - 1)
        se = math.sqrt(s2 * np.linalg.inv(A.T @ A)[q, q])
        assert abs(float(table[j][7]) - coef[q] * mstd[j]) <= 1e-8 * abs(coef[q] * mstd[j]) + 1e-11 * se * mstd[j], j
        assert abs(float(table[j][8]) - se * mstd[j]) <= 1e-8 * se * mstd[j], j
