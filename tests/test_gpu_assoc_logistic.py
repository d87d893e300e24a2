"""hydra_mi355x --assoc --assoc-logistic after a short real chain on a case/control phenotype: every row of the table against a NumPy
restatement (dense genotypes, its own Newton fit per chromosome on [1 | covariates | G - G_c], the score test's formulas), with and
without the LOCO predictor; V against the full information matrix; --assoc-out; and --assoc alone unchanged by it."""
import ctypes as C
import math
import os
import re
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
HEADER = ["CHR", "SNP", "BP", "A1", "A2", "FREQ", "N", "BETA", "SE", "CHISQ", "P", "N_CASE", "N_CTRL", "FREQ_CASE", "FREQ_CTRL"]

# An effect near zero is held to this many SE instead of a relative bound: ten times the largest move of the restatement's U / sqrt(V)
# between its stop rule and five further Newton steps.  Measured on the CPU over every marker of this cohort: 3.55e-15 without a LOCO
# predictor, 1.33e-15 with a stand-in predictor (marginal effects shrunk by five); with the chain's own .bet the LOCO test prints it
# (3.55e-15).  The smallest |U / sqrt(V)| of the cohort is 0.0047, so the relative bound is the one that binds.
FLOOR_SE = 3.6e-14


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
        assert f.readline().split() == HEADER
        return [line.split() for line in f]


def make_cohort():
    """genotypes with 1 % missing calls in a quarter of the columns, two covariates, and a liability-threshold phenotype with about
    30 % cases, coded 1/2"""
    geno = synth.make_genotypes(M, N, seed=31)
    rng = np.random.default_rng(33)
    for j in rng.choice(M, size=M // 4, replace=False):
        geno[j, rng.random(N) < 0.01] = 3
    liab, _ = synth.make_phenotype(geno, seed=32, causal_frac=0.1)
    cov = np.random.default_rng(6).standard_normal((N, 2))
    liab = (liab - liab.mean()) / liab.std() + 0.5 * cov[:, 0]
    cov[:, 1] = cov[:, 1] * 3.0 + 10.0
    y = 1.0 + (liab > np.quantile(liab, 0.7))
    bp = np.cumsum(np.random.default_rng(5).integers(1, 500, size=M)) + 1000
    kept = np.ones(N, dtype=bool)
    kept[NA_PHEN] = False
    kept[NA_COV] = False
    return dict(geno=geno, y=y, cov=cov, kept=kept, bp=bp)


def make_monomorphic(geno):
    geno[MONO] = np.where(geno[MONO] == 3, 3, 1)


def newton(Z, d, extra=0):
    """the fit's stop rule restated: Newton from 0 until max_a |score_a| / sqrt(info_aa) <= 1e-10, then one more full step; `extra`
    further steps after that.  Returns mu, w, the steps to the stop"""
    b = np.zeros(Z.shape[1])
    steps = None
    for it in range(50):
        mu = 1.0 / (1.0 + np.exp(-(Z @ b)))
        w = mu * (1.0 - mu)
        s, info = Z.T @ (d - mu), Z.T @ (Z * w[:, None])
        b = b + np.linalg.solve(info, s)
        if np.max(np.abs(s) / np.sqrt(np.diag(info))) <= 1e-10:
            steps = it + 1
            break
    assert steps is not None, "the restatement's fit did not converge within 50 steps"
    for _ in range(extra):
        mu = 1.0 / (1.0 + np.exp(-(Z @ b)))
        w = mu * (1.0 - mu)
        b = b + np.linalg.solve(Z.T @ (Z * w[:, None]), Z.T @ (d - mu))
    mu = 1.0 / (1.0 + np.exp(-(Z @ b)))
    return mu, mu * (1.0 - mu), steps


def restate(ch, bbar, extra=0):
    """rows[j] = None (NA) or (BETA, SE, CHISQ); counts[j] = (FREQ, N, N_CASE, N_CTRL, FREQ_CASE, FREQ_CTRL); and x, d, the Z, mu, w of
    each chromosome.  bbar: the mean effects of the .bet records (MN,), or None for no LOCO predictor"""
    kept = ch["kept"]
    g = ch["geno"][:MN][:, kept]
    n = g.shape[1]
    yk = ch["y"][kept]
    d = (yk == yk.max()).astype(np.float64)
    Z0 = np.column_stack([np.ones(n), ch["cov"][kept]])
    mave, mstd = oracle_stats(g)
    ok = np.isfinite(mstd)
    with np.errstate(invalid="ignore"):
        x = np.where(g == 3, 0.0, (g - mave[:, None]) * mstd[:, None])
    x[~ok] = 0.0
    chroms = np.array([chrom_of(j) for j in range(MN)])
    fits = {}
    if bbar is not None:
        Gc = {c: (bbar[chroms == c] * ok[chroms == c]) @ x[chroms == c] for c in set(chroms)}
        G = sum(Gc.values())
        for c in sorted(set(chroms)):
            Z = np.column_stack([Z0, G - Gc[c]])
            fits[c] = (Z,) + newton(Z, d, extra)
    else:
        fit = (Z0,) + newton(Z0, d, extra)
        fits = {c: fit for c in set(chroms)}
    rows, counts = [], []
    for j in range(MN):
        Z, mu, w, _ = fits[chroms[j]]
        U, xwx, t = x[j] @ (d - mu), (w * x[j]) @ x[j], Z.T @ (w * x[j])
        V = xwx - t @ np.linalg.solve(Z.T @ (Z * w[:, None]), t)
        rows.append(None if not ok[j] or V <= 1e-9 * xwx else (mstd[j] * U / V, mstd[j] / math.sqrt(V), U * U / V))
        ca, co = g[j][(d == 1) & (g[j] != 3)], g[j][(d == 0) & (g[j] != 3)]
        counts.append((mave[j] / 2, int(np.count_nonzero(g[j] != 3)), ca.size, co.size, ca.sum() / (2 * ca.size), co.sum() / (2 * co.size)))
    return rows, counts, x, d, fits, mstd


def newton_drift(ch, bbar):
    """the largest move of U / sqrt(V) over the markers between the stop rule and five further steps (FLOOR_SE is ten times this)"""
    a, b = restate(ch, bbar)[0], restate(ch, bbar, extra=5)[0]
    z = lambda r: r[0] / r[1]  # noqa: E731  BETA / SE = U / sqrt(V)
    return max(abs(z(p) - z(q)) for p, q in zip(a, b) if p is not None)


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("assoc_logistic")
    ch = make_cohort()
    geno, cov = ch["geno"], ch["cov"]
    prefix = str(tmp / "train")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=ch["y"], na_rows=NA_PHEN)
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%s snp%d 0 %d G T\n" % (chrom_of(j), j, ch["bp"][j]))
    with open(prefix + ".cov", "w") as f:
        for i in range(N):
            f.write("fam%d ind%d %s\n" % (i, i, "NA 1.0" if i == NA_COV else "%.17g %.17g" % (cov[i, 0], cov[i, 1])))
    out = str(tmp / "out")
    base = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--covariates", prefix + ".cov",
            "--mcmc-out-dir", out, "--mcmc-out-name", "r", "--number-individuals", str(N), "--number-markers", str(MN),
            "--chain-length", "8", "--thin", "1", "--save", "7", "--seed", "9"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    make_monomorphic(geno)
    synth.write_plink(prefix + "_m", synth.pack_bed_columns(geno), N)
    os.replace(prefix + "_m.bed", prefix + ".bed")
    base = [a for a in base if a not in ("--chain-length", "8", "--save", "7")] + ["--burn-in", "3"]
    its, betas = read_bet(out + "/r.bet")
    bbar = betas[its >= 3].mean(axis=0)
    assert bbar.shape == (MN,) and np.count_nonzero(bbar) > 0
    # the linear table before any logistic run, to compare with one after
    r = subprocess.run(base + ["--assoc"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ch.update(out=out, base=base, bbar=bbar, linear=open(out + "/r.assoc", "rb").read())
    return ch


def check_rows(table, ref, counts, ch):
    assert len(table) == MN
    for j, (row, want, cnt) in enumerate(zip(table, ref, counts)):
        assert len(row) == len(HEADER) and row[:5] == [chrom_of(j), "snp%d" % j, str(ch["bp"][j]), "G", "T"], j
        freq, ncalled, ncase, nctrl, fcase, fctrl = cnt
        assert (int(row[6]), int(row[11]), int(row[12])) == (ncalled, ncase, nctrl), (j, row)
        for got, w in zip((row[5], row[13], row[14]), (freq, fcase, fctrl)):
            assert abs(float(got) - w) <= 1e-11, (j, row)
        if want is None:
            assert row[7:11] == ["NA"] * 4, (j, row)
            continue
        beta, se, chisq = want
        # 1e-9 relative; an effect near 0 is held to FLOOR_SE of its SE instead (for CHISQ = z^2 a move of z by F is 2 |z| F + F^2)
        zabs = abs(beta) / se
        for got, w, floor in zip(map(float, row[7:10]), want, (FLOOR_SE * se, 0.0, 2.0 * zabs * FLOOR_SE + FLOOR_SE ** 2)):
            assert abs(got - w) <= 1e-9 * abs(w) + floor, (j, row, want)
        p = math.erfc(math.sqrt(float(row[9]) / 2))
        assert abs(float(row[10]) - p) <= 1e-9 * p, (j, row)
    assert [j for j, row in enumerate(table) if row[7] == "NA"] == [MONO]


def closing_line(stdout):
    m = re.search(r"ASSOC  : wrote (\d+) rows to \S+ \((\d+) cases, (\d+) controls, (\d+) iterations of (\d+) null models?, ([0-9.]+) ms on the device\)", stdout)
    assert m, stdout
    return [int(v) for v in m.groups()[:5]] + [float(m.group(6))]


def test_logistic_loco_matches_numpy(chain):
    r = subprocess.run(chain["base"] + ["--assoc", "--assoc-logistic"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    n = int(chain["kept"].sum())
    assert "ASSOC  : %d markers, 3 chromosomes in 4 runs, 2 covariates, %d individuals" % (MN, n) in r.stdout
    ref, counts, x, d, fits, mstd = restate(chain, chain["bbar"])
    print("largest move of U / sqrt(V) over five further Newton steps (LOCO): %.3g" % newton_drift(chain, chain["bbar"]))
    rows, ncase, nctrl, iters, nfits, ms = closing_line(r.stdout)
    assert (rows, ncase, nctrl, nfits) == (MN, int(d.sum()), n - int(d.sum()), 3) and ms > 0.0
    assert iters == sum(f[3] for f in fits.values())
    table = read_table(chain["out"] + "/r.assoc.logistic")
    check_rows(table, ref, counts, chain)
    # independent of the projection algebra: V = 1 / [I^-1]_xx of the full information matrix of [Z_c, x_j] at the null fit
    for j in (0, 5, 61, 130, 190):
        Z, mu, w, _ = fits[chrom_of(j)]
        A = np.column_stack([Z, x[j]])
        V = 1.0 / np.linalg.inv(A.T @ (A * w[:, None]))[-1, -1]
        got = (mstd[j] / float(table[j][8])) ** 2
        assert abs(got - V) <= 1e-8 * V, j
    # the same table through --assoc-out
    alt = chain["out"] + "/alt.logistic"
    r = subprocess.run(chain["base"] + ["--assoc", "--assoc-logistic", "--assoc-out", alt], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(alt).read() == open(chain["out"] + "/r.assoc.logistic").read()


def test_logistic_no_loco_matches_numpy(chain):
    out = chain["out"] + "/nl.logistic"
    r = subprocess.run(chain["base"] + ["--assoc", "--assoc-logistic", "--assoc-no-loco", "--assoc-out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ref, counts, _, d, fits, _ = restate(chain, None)
    rows, ncase, nctrl, iters, nfits, ms = closing_line(r.stdout)
    assert (rows, ncase, nfits, iters) == (MN, int(d.sum()), 1, fits["1"][3])
    check_rows(read_table(out), ref, counts, chain)


def test_linear_assoc_unchanged_after_a_logistic_run(chain):
    r = subprocess.run(chain["base"] + ["--assoc", "--assoc-logistic"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(chain["base"] + ["--assoc"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(chain["out"] + "/r.assoc", "rb").read() == chain["linear"]
    assert open(chain["out"] + "/r.assoc", "rb").readline().split() == [h.encode() for h in HEADER[:11]]
