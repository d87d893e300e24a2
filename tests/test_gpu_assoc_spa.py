"""hydra_mi355x --assoc --assoc-logistic --assoc-spa after a short real chain on an unbalanced case/control phenotype with rare
markers: the two new columns and the corrected P against the NumPy restatement of tests/spa_restate.py, with and without the LOCO
predictor; --assoc-spa-sd; and the table without the flag unchanged by all of it."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from hydra_amd import synth

import spa_restate as R
import test_gpu_assoc_logistic as tl  # the cohort's layout, the chain's recipe and the restatement of the score test

pytestmark = pytest.mark.gpu

N, M, MN = tl.N, tl.M, tl.MN
HEADER = tl.HEADER + ["P_NORM", "SPA"]

# P on the rows with SPA = 1 against the restatement: ten times the largest relative difference of p between the float64 and the
# longdouble restatement over this cohort's flagged markers.  Measured on the CPU without a LOCO predictor: 9.78e-15; with the
# chain's own .bet the LOCO test prints it (6.15e-15).  The table holds twelve digits, so the text adds half a unit of the
# twelfth: 5e-12.
TOL_P = 9.8e-14
TEXT = 5e-12


def make_cohort():
    """tl.make_cohort's recipe with a quarter of the markers redrawn at MAF 0.005 .. 0.02, a dozen of them raising the liability of
    their carriers, and about 6 % cases"""
    geno = synth.make_genotypes(M, N, seed=41)
    rng = np.random.default_rng(43)
    rare = np.sort(rng.choice(M, size=M // 4, replace=False))
    geno[rare] = rng.binomial(2, rng.uniform(0.005, 0.02, size=rare.size)[:, None], size=(rare.size, N))
    assert all(geno[j].min() < geno[j].max() for j in rare)
    for j in rng.choice(M, size=M // 4, replace=False):
        geno[j, rng.random(N) < 0.01] = 3
    liab, _ = synth.make_phenotype(geno, seed=42, causal_frac=0.1)
    cov = np.random.default_rng(6).standard_normal((N, 2))
    liab = (liab - liab.mean()) / liab.std() + 0.5 * cov[:, 0]
    for k, j in enumerate(rare[rare != tl.MONO][:12]):
        liab += (0.8 + 0.1 * k) * np.where(geno[j] == 3, 0, geno[j])
    cov[:, 1] = cov[:, 1] * 3.0 + 10.0
    y = 1.0 + (liab > np.quantile(liab, 0.94))
    bp = np.cumsum(np.random.default_rng(5).integers(1, 500, size=M)) + 1000
    kept = np.ones(N, dtype=bool)
    kept[tl.NA_PHEN] = False
    kept[tl.NA_COV] = False
    return dict(geno=geno, y=y, cov=cov, kept=kept, bp=bp)


def restate_spa(ch, bbar, sd=2.0, dtype=np.float64):
    """per marker None (NA row) or (P_NORM, SPA, P): SPA None where the saddlepoint was not applied, else 0 / 1"""
    rows, _, x, d, fits, _ = tl.restate(ch, bbar)
    out = []
    for j, row in enumerate(rows):
        if row is None:
            out.append(None)
            continue
        Z, mu, w, _ = fits[tl.chrom_of(j)]
        U = x[j] @ (d - mu)
        t = Z.T @ (w * x[j])
        b = np.linalg.solve(Z.T @ (Z * w[:, None]), t)
        V = (w * x[j]) @ x[j] - t @ b
        pn = R.normal_p(U, V)
        if not abs(U) / math.sqrt(V) > sd:
            out.append((pn, None, pn))
            continue
        r = R.roots(np.asarray(x[j], dtype) - np.asarray(Z, dtype) @ np.asarray(b, dtype), np.asarray(mu, dtype), U, dtype)
        p, ok = R.pvalue(U, r)[2:]
        out.append((pn, int(ok), p if ok else pn))
    return out


def precision_gap(ch, bbar):
    a, b = restate_spa(ch, bbar), restate_spa(ch, bbar, dtype=np.longdouble)
    return max(R.rel(p[2], q[2]) for p, q in zip(a, b) if p is not None and p[1] == 1)


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("assoc_spa")
    ch = make_cohort()
    # on the CPU first: the cohort must show what the correction is for
    tl.make_monomorphic(ch["geno"])
    ref = restate_spa(ch, None)
    moved = [j for j, r in enumerate(ref) if r is not None and r[1] == 1 and r[2] > 10.0 * r[0]]
    assert len(moved) >= 5, moved
    ch = make_cohort()
    geno, cov = ch["geno"], ch["cov"]
    prefix = str(tmp / "train")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=ch["y"], na_rows=tl.NA_PHEN)
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%s snp%d 0 %d G T\n" % (tl.chrom_of(j), j, ch["bp"][j]))
    with open(prefix + ".cov", "w") as f:
        for i in range(N):
            f.write("fam%d ind%d %s\n" % (i, i, "NA 1.0" if i == tl.NA_COV else "%.17g %.17g" % (cov[i, 0], cov[i, 1])))
    out = str(tmp / "out")
    base = [tl.EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--covariates", prefix + ".cov",
            "--mcmc-out-dir", out, "--mcmc-out-name", "r", "--number-individuals", str(N), "--number-markers", str(MN),
            "--chain-length", "8", "--thin", "1", "--save", "7", "--seed", "9"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    tl.make_monomorphic(geno)
    synth.write_plink(prefix + "_m", synth.pack_bed_columns(geno), N)
    os.replace(prefix + "_m.bed", prefix + ".bed")
    base = [a for a in base if a not in ("--chain-length", "8", "--save", "7")] + ["--burn-in", "3", "--assoc", "--assoc-logistic"]
    its, betas = tl.read_bet(out + "/r.bet")
    bbar = betas[its >= 3].mean(axis=0)
    # the tables before the flag is given, to compare with the ones after
    plain = {}
    for name, flags in (("loco", []), ("noloco", ["--assoc-no-loco"])):
        path = "%s/%s.plain" % (out, name)
        r = subprocess.run(base + flags + ["--assoc-out", path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        plain[name] = open(path, "rb").read()
    ch.update(out=out, base=base, bbar=bbar, plain=plain)
    return ch


def spa_line(stdout):
    m = re.search(r"ASSOC  : wrote \d+ rows to [^\n]*\nASSOC  : SPA on (\d+) markers \(\|z\| > (\S+)\): (\d+) valid, (\d+) fell back, ([0-9.]+) ms on the device\n", stdout)
    assert m, stdout
    return int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4)), float(m.group(5))


def run_and_check(ch, name, flags, bbar, sd=None):
    path = "%s/%s.spa" % (ch["out"], name)
    extra = ["--assoc-spa"] + (["--assoc-spa-sd", sd] if sd else [])
    r = subprocess.run(ch["base"] + flags + extra + ["--assoc-out", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ref = restate_spa(ch, bbar, float(sd or 2))
    with open(path) as f:
        assert f.readline().split() == HEADER
        table = [line.split() for line in f]
    old = [line.split() for line in ch["plain"][name].decode().splitlines()[1:]]
    assert len(table) == len(old) == MN
    applied = valid = 0
    for j, (row, was, want) in enumerate(zip(table, old, ref)):
        assert len(row) == len(HEADER), (j, row)
        if want is None:
            assert row[:15] == was and row[15:] == ["NA", "NA"] and row[7:11] == ["NA"] * 4, (j, row)
            continue
        pn, spa, p = want
        assert row[15] == was[10], (j, row)  # P_NORM is the old P's text
        assert row[16] == ("NA" if spa is None else str(spa)), (j, row, want)
        if spa == 1:
            assert row[:10] == was[:10] and row[11:15] == was[11:], (j, row)
            assert abs(float(row[10]) - p) <= (TOL_P + TEXT) * p, (j, row, want)
        else:
            assert row[:15] == was, (j, row)
        applied += spa is not None
        valid += spa == 1
    n, t, ok, fell, ms = spa_line(r.stdout)
    assert (n, ok, fell) == (applied, valid, applied - valid) and float(t) == float(sd or 2) and (ms > 0.0) == (applied > 0)
    return applied, valid, table


def test_spa_loco_matches_the_restatement(chain):
    print("largest relative difference of p, float64 / longdouble restatement (LOCO): %.3g" % precision_gap(chain, chain["bbar"]))
    applied, valid, table = run_and_check(chain, "loco", [], chain["bbar"])
    assert valid >= 5
    assert sum(1 for row in table if row[16] == "1" and float(row[10]) > 10.0 * float(row[15])) >= 5


def test_spa_no_loco_matches_the_restatement(chain):
    print("largest relative difference of p, float64 / longdouble restatement (no LOCO): %.3g" % precision_gap(chain, None))
    applied, valid, _ = run_and_check(chain, "noloco", ["--assoc-no-loco"], None)
    assert valid >= 5
    fewer, _, _ = run_and_check(chain, "noloco", ["--assoc-no-loco"], None, sd="4")
    assert 0 < fewer < applied


def test_the_table_without_the_flag_is_unchanged_after_spa_runs(chain):
    run_and_check(chain, "noloco", ["--assoc-no-loco"], None)
    for name, flags in (("loco", []), ("noloco", ["--assoc-no-loco"])):
        path = "%s/%s.again" % (chain["out"], name)
        r = subprocess.run(chain["base"] + flags + ["--assoc-out", path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "SPA" not in r.stdout
        assert open(path, "rb").read() == chain["plain"][name]
        assert open(path).readline().split() == tl.HEADER
