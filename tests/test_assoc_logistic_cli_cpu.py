"""hydra_mi355x --assoc --assoc-logistic, the part that runs before any device is touched: every new refusal, the existing ones with
the new flag on the line, and that a valid command line prints its report and reaches the device.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 60, 12


def run(*args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=60, env=e)


def has_gpu():
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        return hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        return False


def write_cohort(tmp_path, y):
    geno = synth.make_genotypes(M, N, seed=1)
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=np.asarray(y, dtype=np.float64), na_rows=[4])
    with open(prefix + ".bim", "w") as f:  # chromosomes 1 1 1 1 2 2 2 2 1 1 3 3: four runs, three chromosomes
        for j, c in enumerate("111122221133"):
            f.write("%s snp%d 0 %d A C\n" % (c, j, 100 * j + 1))
    return ["--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"),
            "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(M)]


def case_control(seed=3):
    return 1.0 + (np.random.default_rng(seed).random(N) < 0.4)  # coded 1/2


def write_cov(tmp_path, cols):
    cov = str(tmp_path / "cov.txt")
    with open(cov, "w") as f:
        for i in range(N):
            f.write("f%d i%d %s\n" % (i, i, " ".join("%.17g" % c[i] for c in cols)))
    return cov


def refused(r, msg):
    assert r.returncode != 0, r.stdout
    assert msg in r.stderr, r.stderr
    assert "invalid option" not in r.stderr and "hgibbs_create" not in r.stderr


LOGISTIC = ["--assoc", "--assoc-logistic", "--assoc-no-loco"]


def test_logistic_needs_assoc(tmp_path):
    refused(run(*write_cohort(tmp_path, case_control()), "--assoc-logistic"), "--assoc-logistic needs --assoc")


def test_existing_refusals_keep_their_messages(tmp_path):
    base = write_cohort(tmp_path, case_control())
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--assoc", "--assoc-logistic"),
            "--assoc takes a bayesMPI command line, not --mpibayes bayesWMPI")
    refused(run(*base, "--assoc", "--assoc-logistic", "--ld-window", "5"), "--assoc cannot be combined with --ld-window")
    refused(run(*base, "--assoc", "--assoc-logistic", env={"WORLD_SIZE": "2", "RANK": "0"}), "--assoc runs on one process (WORLD_SIZE = 2)")
    refused(run(*base, "--assoc", "--assoc-logistic"), "--assoc takes its LOCO offsets from the chain's effects: run the chain first")
    refused(run(*base, "--assoc-out", "t", "--assoc-logistic"), "--assoc-out needs --assoc")
    cov = write_cov(tmp_path, [np.full(N, 1.5), np.arange(N) % 3])  # a constant column next to the intercept
    refused(run(*base, "--covariates", cov, *LOGISTIC), "the covariates are rank-deficient")


@pytest.mark.parametrize("y,count", [(np.arange(N) % 3, 3), (np.ones(N), 1), (np.random.default_rng(2).standard_normal(N), N - 1)])
def test_phenotype_must_take_two_values(tmp_path, y, count):
    refused(run(*write_cohort(tmp_path, y), *LOGISTIC),
            "--assoc-logistic: the phenotype takes %d distinct values on the kept rows, a case/control phenotype takes exactly two" % count)


def test_too_many_covariates_names_their_count(tmp_path):
    rng = np.random.default_rng(5)
    cov = write_cov(tmp_path, [rng.standard_normal(N) for _ in range(30)])
    refused(run(*write_cohort(tmp_path, case_control()), "--covariates", cov, *LOGISTIC), "--assoc-logistic: 30 covariates make 33 vectors")


def test_null_model_refusals_come_before_the_device(tmp_path):
    y = case_control()
    # a covariate that separates the cases from the controls
    sep = np.where(y == 2.0, 1.0, -1.0) * (1.0 + np.random.default_rng(6).random(N))
    refused(run(*write_cohort(tmp_path, y), "--covariates", write_cov(tmp_path, [sep]), *LOGISTIC), "--assoc-logistic: hgibbs_logit_null: separation")


def test_valid_command_line_reports_and_reaches_the_device(tmp_path):
    base = write_cohort(tmp_path, case_control())
    out = str(tmp_path / "t.logistic")
    r = run(*base, *LOGISTIC, "--assoc-out", out)
    assert "ASSOC  : 12 markers, 3 chromosomes in 4 runs, 0 covariates, %d individuals -> %s" % (N - 1, out) in r.stdout, r.stdout
    assert "no LOCO predictor (--assoc-no-loco)" in r.stdout
    if has_gpu():
        assert r.returncode == 0 and "wrote 12 rows" in r.stdout, r.stderr
        assert open(out).readline().split()[-4:] == ["N_CASE", "N_CTRL", "FREQ_CASE", "FREQ_CTRL"]
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    r = run(*base, *LOGISTIC)  # the default name
    assert "-> %s" % str(tmp_path / "o" / "n.assoc.logistic") in r.stdout, r.stdout
