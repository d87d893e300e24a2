"""hydra_mi355x --assoc --assoc-logistic --assoc-firth after a short real chain on an unbalanced case/control phenotype with rare
markers: the four new columns and the refitted BETA, SE, CHISQ and P against the NumPy restatement of tests/firth_restate.py, with and
without the LOCO predictor; --assoc-firth-p; --clump on the new table; and the table without the flag unchanged by all of it."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hydra_amd import synth

import firth_restate as F
import test_gpu_assoc_logistic as tl  # the cohort's layout and the restatement of the score test
import test_gpu_assoc_spa as ts       # the cohort's recipe

pytestmark = pytest.mark.gpu

N, M, MN = tl.N, tl.M, tl.MN
HEADER = tl.HEADER + ["P_NORM", "BETA_SCORE", "SE_SCORE", "FIRTH"]

# BETA, SE, CHISQ and P on the rows with FIRTH = 1 against the restatement: ten times the largest relative difference between the
# float64 and the longdouble restatement over this cohort's fitted markers, measured on the CPU without a LOCO predictor (the tests print
# it, the LOCO test with the chain's own .bet).  At the default threshold 0.05 (26 markers): BETA 6.24e-16, SE 5.06e-16, CHISQ 6.14e-16,
# P 1.04e-14.  At --assoc-firth-p 1 every tested marker is fitted (192), the ones with a likelihood ratio near 0 included (the smallest is
# 2.1e-4), whose ratio is what the terms beta s, K and the penalty leave of each other: BETA 2.8e-15, SE 5.06e-16, CHISQ 8.51e-13,
# P 1.04e-14.  The table holds twelve digits, so the text adds half a unit of the twelfth: 5e-12.
TOL = {0.05: dict(beta=6.3e-15, se=5.1e-15, chisq=6.2e-15, p=1.1e-13), 1.0: dict(beta=2.8e-14, se=5.1e-15, chisq=8.6e-12, p=1.1e-13)}
TEXT = 5e-12


def restate_firth(ch, bbar, t=0.05, dtype=np.float64):
    """per marker None (NA row) or a dict: firth None where the fit was not applied, else 0 / 1, and beta, se, chisq, p where it is 1"""
    rows, _, x, d, fits, mstd = tl.restate(ch, bbar)
    out = []
    for j, row in enumerate(rows):
        if row is None:
            out.append(None)
            continue
        Z, mu, w, _ = fits[tl.chrom_of(j)]
        U = x[j] @ (d - mu)
        tz = Z.T @ (w * x[j])
        b = np.linalg.solve(Z.T @ (Z * w[:, None]), tz)
        V = (w * x[j]) @ x[j] - tz @ b
        pn = math.erfc(math.sqrt(U * U / V / 2.0))
        if not pn <= t:
            out.append(dict(firth=None))
            continue
        r = F.fit(np.asarray(x[j], dtype) - np.asarray(Z, dtype) @ np.asarray(b, dtype), np.asarray(mu, dtype), U, dtype)
        lrt, se, p, ok = F.stats(U, r)
        out.append(dict(firth=int(ok), beta=mstd[j] * float(r["beta"]), se=mstd[j] * se, chisq=lrt, p=p))
    return out


def precision_gap(ch, bbar, t=0.05):
    a, b = restate_firth(ch, bbar, t), restate_firth(ch, bbar, t, dtype=np.longdouble)
    fitted = [(p, q) for p, q in zip(a, b) if p is not None and p["firth"] == 1]
    assert all(q["firth"] == 1 for _, q in fitted)
    return {k: max(F.rel(p[k], q[k]) for p, q in fitted) for k in ("beta", "se", "chisq", "p")}


def show_gap(what, gap):
    print("largest relative difference, float64 / longdouble restatement (%s): BETA %.3g, SE %.3g, CHISQ %.3g, P %.3g"
          % (what, gap["beta"], gap["se"], gap["chisq"], gap["p"]))


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("assoc_firth")
    ch = ts.make_cohort()
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
    common = [tl.EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--covariates", prefix + ".cov",
              "--mcmc-out-dir", out, "--mcmc-out-name", "r", "--number-individuals", str(N), "--number-markers", str(MN), "--thin", "1", "--seed", "9"]
    r = subprocess.run(common + ["--chain-length", "8", "--save", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    tl.make_monomorphic(geno)
    synth.write_plink(prefix + "_m", synth.pack_bed_columns(geno), N)
    os.replace(prefix + "_m.bed", prefix + ".bed")
    base = common + ["--burn-in", "3", "--assoc", "--assoc-logistic"]
    its, betas = tl.read_bet(out + "/r.bet")
    bbar = betas[its >= 3].mean(axis=0)
    # the tables before the flag is given, to compare with the ones after
    plain = {}
    for name, flags in (("loco", []), ("noloco", ["--assoc-no-loco"])):
        path = "%s/%s.plain" % (out, name)
        r = subprocess.run(base + flags + ["--assoc-out", path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        plain[name] = open(path, "rb").read()
    ch.update(out=out, common=common, base=base, bbar=bbar, plain=plain)
    return ch


def firth_line(stdout):
    m = re.search(r"ASSOC  : wrote \d+ rows to [^\n]*\nASSOC  : Firth on (\d+) markers \(P <= (\S+)\): (\d+) valid, (\d+) fell back, ([0-9.]+) ms on the device\n", stdout)
    assert m, stdout
    return int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4)), float(m.group(5))


def run_and_check(ch, name, flags, bbar, t=None):
    path = "%s/%s.firth" % (ch["out"], name)
    extra = ["--assoc-firth"] + (["--assoc-firth-p", t] if t else [])
    r = subprocess.run(ch["base"] + flags + extra + ["--assoc-out", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SPA" not in r.stdout
    ref = restate_firth(ch, bbar, float(t or 0.05))
    tol = TOL[float(t or 0.05)]
    with open(path) as f:
        assert f.readline().split() == HEADER
        table = [line.split() for line in f]
    old = [line.split() for line in ch["plain"][name].decode().splitlines()[1:]]
    assert len(table) == len(old) == MN
    applied = valid = 0
    worst = dict(beta=0.0, se=0.0, chisq=0.0, p=0.0)
    for j, (row, was, want) in enumerate(zip(table, old, ref)):
        assert len(row) == len(HEADER) == 19, (j, row)
        if want is None:
            assert row[:15] == was and row[15:] == ["NA"] * 4 and row[7:11] == ["NA"] * 4, (j, row)
            continue
        assert row[15:18] == [was[10], was[7], was[8]], (j, row)  # P_NORM, BETA_SCORE and SE_SCORE are the old P's, BETA's and SE's text
        assert row[18] == ("NA" if want["firth"] is None else str(want["firth"])), (j, row, want)
        if want["firth"] == 1:
            assert row[:7] == was[:7] and row[11:15] == was[11:], (j, row)
            for k, name_ in enumerate(("beta", "se", "chisq", "p")):
                worst[name_] = max(worst[name_], F.rel(float(row[7 + k]), want[name_]))
                assert abs(float(row[7 + k]) - want[name_]) <= (tol[name_] + TEXT) * abs(want[name_]), (j, name_, row, want)
        else:
            assert row[:15] == was, (j, row)
        applied += want["firth"] is not None
        valid += want["firth"] == 1
    print("largest relative difference table / restatement: BETA %.3g, SE %.3g, CHISQ %.3g, P %.3g" % (worst["beta"], worst["se"], worst["chisq"], worst["p"]))
    n, thr, ok, fell, ms = firth_line(r.stdout)
    print("Firth on %d markers: %.3f ms on the device" % (n, ms))
    assert (n, ok, fell) == (applied, valid, applied - valid) and float(thr) == float(t or 0.05) and (ms > 0.0) == (applied > 0)
    return applied, valid, table, path


def test_firth_loco_matches_the_restatement(chain):
    show_gap("LOCO", precision_gap(chain, chain["bbar"]))
    applied, valid, table, _ = run_and_check(chain, "loco", [], chain["bbar"])
    assert valid >= 5
    # what the fit is for: on the rare markers that the score test puts furthest out, the penalised ratio is the smaller statistic
    assert sum(1 for row in table if row[18] == "1" and float(row[9]) < float(row[16]) ** 2 / float(row[17]) ** 2) >= 5


def test_firth_no_loco_matches_the_restatement(chain):
    show_gap("no LOCO", precision_gap(chain, None))
    show_gap("no LOCO, every tested marker", precision_gap(chain, None, 1.0))
    applied, valid, _, _ = run_and_check(chain, "noloco", ["--assoc-no-loco"], None)
    assert valid >= 5
    every, _, table, _ = run_and_check(chain, "noloco", ["--assoc-no-loco"], None, t="1")
    assert applied < every == sum(1 for row in table if row[7] != "NA") == MN - 1
    assert all(row[18] in ("0", "1") for row in table if row[7] != "NA")


def test_clump_reads_the_table(chain):
    _, _, table, path = run_and_check(chain, "noloco", ["--assoc-no-loco"], None)
    out = chain["out"] + "/f.clumped"
    # --clump takes every chromosome as one contiguous run, and this cohort's chromosome 1 comes in two: the same markers on one chromosome
    prefix = chain["common"][chain["common"].index("--bfile") + 1]
    for ext in (".bed", ".fam"):
        shutil.copyfile(prefix + ext, prefix + "_one" + ext)
    with open(prefix + "_one.bim", "w") as f:
        for j in range(M):
            f.write("1 snp%d 0 %d G T\n" % (j, chain["bp"][j]))
    common = [prefix + "_one" if a == prefix else a for a in chain["common"]]
    r = subprocess.run(common + ["--clump", path, "--clump-p1", "0.05", "--clump-p2", "0.5", "--clump-snps", "30", "--clump-out", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "%d rows read from" % MN in r.stdout and "(0 ids not in it, 1 without a P in [0, 1])" in r.stdout, r.stdout
    lines = open(out).read().splitlines()
    assert lines[0] == "CHR F SNP BP P TOTAL NSIG S05 S01 S001 S0001 SP2" and len(lines) > 1
    p_of = {row[1]: float(row[10]) for row in table if row[10] != "NA"}
    for line in lines[1:]:  # the index markers carry the table's P, the refitted one where FIRTH = 1
        w = line.split()
        assert abs(float(w[4]) - p_of[w[2]]) <= 1e-3 * p_of[w[2]], line


def test_the_table_without_the_flag_is_unchanged_after_firth_runs(chain):
    run_and_check(chain, "noloco", ["--assoc-no-loco"], None)
    for name, flags in (("loco", []), ("noloco", ["--assoc-no-loco"])):
        path = "%s/%s.again" % (chain["out"], name)
        r = subprocess.run(chain["base"] + flags + ["--assoc-out", path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "Firth" not in r.stdout
        assert open(path, "rb").read() == chain["plain"][name]
        assert open(path).readline().split() == tl.HEADER
