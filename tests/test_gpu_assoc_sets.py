"""hydra_mi355x --assoc --assoc-logistic --assoc-sets after a short real chain on a small case/control cohort: the .assoc.sets table
against the restatement of tests/settest_restate.py (dense genotypes, its own Newton fit per chromosome on [1 | covariate | G - G_c],
Phi from the definition), with the default and with flat weights; the singleton's burden test against the per-marker CHISQ; the
per-marker table byte for byte what it is without the flag."""
import os
import re
import subprocess

import numpy as np
import pytest

from hydra_amd import synth

import settest_restate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")

pytestmark = pytest.mark.gpu

N, M = 600, 400
NA_PHEN, NA_COV = [7, 311], 100
MONO = 260
MAF_X = 0.25
HEADER = ["SET", "CHR", "BP_FIRST", "BP_LAST", "NSNP", "NUSED", "NEIG", "Q", "P_SKAT", "SKAT_OK", "T_BURDEN", "P_BURDEN"]

# Both null fits stop at max |score| / sqrt(info) <= 1e-10 and take one more Newton step, which leaves the coefficients correct to
# rounding; what separates the table from the restatement is the order of the f64 sums over the 597 rows (597 x 2^-53 = 7e-14) and the
# subtraction of the projected part in Phi and in U, which loses at most three digits here (the covariate and the LOCO predictor
# explain little of a rare marker): 1e-10 for Q and T_BURDEN.  A p-value moves by d log p / d log Q <= Q / (2 lam_max) + 1 times that,
# below 100 on this cohort: 1e-8.  Twelve written digits add 5e-12.
TOL_STAT = 1e-10 + 5e-12
TOL_P = 1e-8 + 5e-12


def chrom_of(j):
    return "1" if j < 200 else "2"


def make_cohort():
    geno = S.genotypes(N, M, 41, True)
    rng = np.random.default_rng(42)
    cov = rng.standard_normal(N)
    mave, mstd = S.marker_stats(geno)
    x = np.where(geno == 3, 0.0, (geno - mave[:, None]) * mstd[:, None])
    causal = rng.choice(M, size=30, replace=False)
    liab = x[causal].T @ rng.standard_normal(30) * 0.25 + 0.5 * cov + rng.standard_normal(N)
    y = 1.0 + (liab > np.quantile(liab, 0.65))
    kept = np.ones(N, dtype=bool)
    kept[NA_PHEN] = False
    kept[NA_COV] = False
    bp = np.cumsum(rng.integers(1, 500, size=M)) + 1000
    return dict(geno=geno, y=y, cov=cov, kept=kept, bp=bp)


def newton(Z, d):
    b = np.zeros(Z.shape[1])
    for _ in range(50):
        mu = 1.0 / (1.0 + np.exp(-(Z @ b)))
        w = mu * (1.0 - mu)
        s, info = Z.T @ (d - mu), Z.T @ (Z * w[:, None])
        b = b + np.linalg.solve(info, s)
        if np.max(np.abs(s) / np.sqrt(np.diag(info))) <= 1e-10:
            mu = 1.0 / (1.0 + np.exp(-(Z @ b)))
            return mu, mu * (1.0 - mu)
    raise AssertionError("the restatement's fit did not converge within 50 steps")


def restate(ch, sets, A, B, maf_x):
    """per set: dict(nsnp, nused, and S.set_tests' fields), and the per-marker CHISQ"""
    kept = ch["kept"]
    g = ch["geno"][:, kept]
    n = g.shape[1]
    d = (ch["y"][kept] == ch["y"][kept].max()).astype(np.float64)
    mave, mstd = S.marker_stats(g)
    ok = np.isfinite(mstd)
    with np.errstate(invalid="ignore"):
        x = np.where(g == 3, 0.0, (g - mave[:, None]) * mstd[:, None])
    x[~ok] = 0.0
    chroms = np.array([chrom_of(j) for j in range(M)])
    Z0 = np.column_stack([np.ones(n), ch["cov"][kept]])
    Gc = {c: (ch["bbar"][chroms == c] * ok[chroms == c]) @ x[chroms == c] for c in ("1", "2")}
    fits = {}
    for c in ("1", "2"):
        Z = np.column_stack([Z0, Gc["1"] + Gc["2"] - Gc[c]])
        fits[c] = (Z,) + newton(Z, d)
    maf = np.minimum(mave / 2.0, 1.0 - mave / 2.0)
    chisq = {}
    out = []
    for name, ids in sets:
        found = [int(i[3:]) for i in ids if i.startswith("snp")]
        r = dict(name=name, nsnp=len(found), nused=0)
        if found:
            Z, mu, w = fits[chrom_of(found[0])]
            info = Z.T @ (Z * w[:, None])
            used = []
            for j in sorted(found):
                xwx, t = (w * x[j]) @ x[j], Z.T @ (w * x[j])
                V = xwx - t @ np.linalg.solve(info, t)
                if ok[j] and V > 1e-9 * xwx:
                    chisq[j] = (x[j] @ (d - mu)) ** 2 / V
                    if maf[j] <= maf_x:
                        used.append(j)
            r["nused"] = len(used)
            if used:
                X = x[used]
                T = (X * w) @ Z
                Phi = (X * w) @ X.T - T @ np.linalg.solve(info, T.T)
                sd = mstd[used]
                r.update(S.set_tests((X @ (d - mu)) / sd, Phi / (sd[:, None] * sd[None, :]), S.beta_weights(maf[used], A, B)))
        out.append(r)
    return out, chisq


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("assoc_sets")
    ch = make_cohort()
    geno = ch["geno"]
    prefix = str(tmp / "train")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=ch["y"], na_rows=NA_PHEN)
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%s snp%d 0 %d G T\n" % (chrom_of(j), j, ch["bp"][j]))
    with open(prefix + ".cov", "w") as f:
        for i in range(N):
            f.write("fam%d ind%d %s\n" % (i, i, "NA" if i == NA_COV else "%.17g" % ch["cov"][i]))
    out = str(tmp / "out")
    base = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--covariates", prefix + ".cov",
            "--mcmc-out-dir", out, "--mcmc-out-name", "r", "--number-individuals", str(N), "--number-markers", str(M),
            "--chain-length", "8", "--thin", "1", "--save", "7", "--seed", "9"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    geno[MONO] = np.where(geno[MONO] == 3, 3, 1)  # made monomorphic after the chain, which cannot take such a marker
    synth.write_plink(prefix + "_m", synth.pack_bed_columns(geno), N)
    os.replace(prefix + "_m.bed", prefix + ".bed")
    base = [a for a in base if a not in ("--chain-length", "8", "--save", "7")] + ["--burn-in", "3", "--assoc", "--assoc-logistic"]
    raw = open(out + "/r.bet", "rb").read()
    rec = 4 + 8 * M
    its = np.array([int(np.frombuffer(raw[4 + k * rec:8 + k * rec], np.uint32)[0]) for k in range((len(raw) - 4) // rec)])
    betas = np.stack([np.frombuffer(raw[8 + k * rec:4 + (k + 1) * rec], np.float64) for k in range(its.size)])
    ch["bbar"] = betas[its >= 3].mean(axis=0)
    # the sets: a singleton, a set of 17, one with the monomorphic member, one with an id the .bim lacks, one of common markers only
    g = geno[:, ch["kept"]]
    mave, _ = S.marker_stats(g)
    maf = np.minimum(mave / 2.0, 1.0 - mave / 2.0)
    common = [j for j in range(201, 400, 2) if maf[j] > MAF_X + 0.02 and j != MONO][:6]
    rare = [j for j in range(0, 400) if maf[j] < MAF_X - 0.02 and j != MONO]
    assert len(common) == 6
    sets = [("one", ["snp%d" % rare[5]]),
            ("seventeen", ["snp%d" % j for j in [r for r in rare if r < 200][10:27]]),
            ("withmono", ["snp%d" % j for j in [r for r in rare if r > 200][:4] + [MONO]]),
            ("unknown", ["snp%d" % j for j in [r for r in rare if r > 200][6:9]] + ["rs999"]),
            ("common", ["snp%d" % j for j in common])]
    path = str(tmp / "sets.txt")
    with open(path, "w") as f:
        for name, ids in sets:
            for i in ids[::-1]:  # (any order within a set)
                f.write("%s\t%s\n" % (name, i))
    plain = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr[-2000:]
    ch.update(out=out, base=base, sets=sets, path=path, plain=open(out + "/r.assoc.logistic", "rb").read())
    return ch


def close(got, want, tol):
    return abs(got - float(want)) <= tol * abs(float(want))


def check_table(path, ref, ch):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == HEADER and len(lines) == 1 + len(ref)
    for line, want in zip(lines[1:], ref):
        row = line.split("\t")
        assert len(row) == len(HEADER) and row[0] == want["name"]
        found = [int(i[3:]) for i in dict(ch["sets"])[want["name"]] if i.startswith("snp")]
        assert row[1:4] == [chrom_of(found[0]), str(min(ch["bp"][found])), str(max(ch["bp"][found]))], row
        assert (int(row[4]), int(row[5])) == (want["nsnp"], want["nused"]), row
        if want["nused"] == 0:
            assert row[6:] == ["0", "NA", "NA", "NA", "NA", "NA"], row
            continue
        assert int(row[6]) == want["neig"] and want["neig"] >= 1 and row[9] == "1", row  # SKAT_OK = 1 wherever NEIG >= 1
        for k, name, tol in ((7, "q", TOL_STAT), (8, "p_skat", TOL_P), (10, "t_burden", TOL_STAT), (11, "p_burden", TOL_P)):
            print("%s %s: %s against %.12g" % (want["name"], name, row[k], float(want[name])))
            assert close(float(row[k]), want[name], tol), (row, name, float(want[name]))
    return [line.split("\t") for line in lines[1:]]


def test_sets_table_matches_the_restatement(chain):
    r = subprocess.run(chain["base"] + ["--assoc-sets", chain["path"], "--assoc-set-maf", str(MAF_X)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ASSOC  : 5 sets of 32 markers from %s (1 ids are not in the .bim)" % chain["path"] in r.stdout, r.stdout
    m = re.search(r"ms on the device\), 5 sets to \S+ \(([0-9.]+) ms of hgibbs_set_gram on the device\)", r.stdout)
    assert m and float(m.group(1)) > 0.0, r.stdout
    print("hgibbs_set_gram: %s ms on the device" % m.group(1))
    ref, chisq = restate(chain, chain["sets"], 1.0, 25.0, MAF_X)
    assert [x["nused"] for x in ref] == [1, 17, 4, 3, 0]
    rows = check_table(chain["out"] + "/r.assoc.sets", ref, chain)
    # the per-marker table is byte for byte what it is without the flag
    assert open(chain["out"] + "/r.assoc.logistic", "rb").read() == chain["plain"]
    # the singleton: T_BURDEN is the marker's CHISQ
    j = int(chain["sets"][0][1][0][3:])
    marker = [line.split() for line in chain["plain"].decode().splitlines()][1 + j]
    assert marker[1] == "snp%d" % j and close(float(rows[0][10]), float(marker[9]), 1e-11), (rows[0], marker)
    assert close(float(rows[0][10]), chisq[j], TOL_STAT)


def test_flat_weights_given_explicitly_and_the_corrections_leave_the_table_alone(chain):
    out = chain["out"] + "/flat.sets"
    flags = ["--assoc-sets", chain["path"], "--assoc-set-maf", str(MAF_X), "--assoc-set-beta", "1", "1", "--assoc-set-out", out]
    r = subprocess.run(chain["base"] + flags, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ref, _ = restate(chain, chain["sets"], 1.0, 1.0, MAF_X)
    check_table(out, ref, chain)
    assert open(chain["out"] + "/r.assoc.logistic", "rb").read() == chain["plain"]
    flat = open(out, "rb").read()
    for corr in ("--assoc-spa", "--assoc-firth"):  # the set table always comes from the plain scores
        r = subprocess.run(chain["base"] + flags + [corr, "--assoc-out", chain["out"] + "/corr.logistic"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(out, "rb").read() == flat, corr


def test_no_maf_bound_keeps_the_common_set(chain):
    out = chain["out"] + "/all.sets"
    r = subprocess.run(chain["base"] + ["--assoc-sets", chain["path"], "--assoc-set-out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ref, _ = restate(chain, chain["sets"], 1.0, 25.0, 0.5)
    assert ref[4]["nused"] == 6
    check_table(out, ref, chain)
