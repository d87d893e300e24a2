"""hydra_mi355x --reml, the part that runs before any device is touched: every refusal, its message and the order of the checks, and
that a valid command line reaches the device with its files created.  No GPU needed."""
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


@pytest.fixture()
def base(tmp_path):
    geno = synth.make_genotypes(M, N, seed=1)
    y, _ = synth.make_phenotype(geno, seed=2)
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=[4])
    return ["--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"),
            "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(M)]


def write_cov(base, C, dependent=False):
    prefix = base[3]
    cov = np.random.default_rng(3).standard_normal((N, C))
    if dependent:
        cov[:, -1] = 2.0 * cov[:, 0] - 1.0
    with open(prefix + ".cov", "w") as f:
        for i in range(N):
            f.write("fam%d ind%d %s\n" % (i, i, " ".join("%.17g" % v for v in cov[i])))
    return ["--covariates", prefix + ".cov"]


def refused(r, msg):
    assert r.returncode != 0, r.stdout
    assert msg in r.stderr, r.stderr
    assert "invalid option" not in r.stderr and "hgibbs_create" not in r.stderr


@pytest.mark.parametrize("extra", [["--reml-trials", "4"], ["--reml-h2-start", "0.3"], ["--reml-cg-tol", "1e-4"], ["--reml-cg-iters", "9"],
                                   ["--reml-tol", "0.1"], ["--reml-out", "x"], ["--reml-blup"]])
def test_reml_options_need_reml(base, extra):
    refused(run(*base, *extra), "%s needs --reml" % extra[0])


def test_refused_with_bayesw(base):
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--reml"),
            "--reml takes a bayesMPI command line, not --mpibayes bayesWMPI")


@pytest.mark.parametrize("other", [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"], ["--pve"], ["--grm"],
                                   ["--ld-score"], ["--clump", "t"], ["--ld-prune", "0.5"], ["--he"], ["--qc"], ["--homozyg"], ["--epistasis"],
                                   ["--cs"]])
def test_refused_with_an_earlier_mode(base, other):
    refused(run(*base, "--reml", *other), "--reml cannot be combined with %s" % other[0])


def test_refused_with_sumstats(base):
    refused(run(*base, "--reml", "--sumstats", "s"), "--sumstats cannot be combined with --reml")


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--reml"), "--reml does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--reml", env={"WORLD_SIZE": "2", "RANK": "0"}), "--reml runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("extra,msg", [
    (["--reml-trials", "0"], "--reml-trials 0: the number of probes must be an integer from 1 to 31"),
    (["--reml-trials", "32"], "--reml-trials 32: the number of probes must be an integer from 1 to 31"),
    (["--reml-trials", "x"], "--reml-trials x: the number of probes must be an integer from 1 to 31"),
    (["--reml-h2-start", "0"], "--reml-h2-start 0: the start value must be a number inside (0, 1)"),
    (["--reml-h2-start", "1"], "--reml-h2-start 1: the start value must be a number inside (0, 1)"),
    (["--reml-h2-start", "nan"], "--reml-h2-start nan: the start value must be a number inside (0, 1)"),
    (["--reml-cg-tol", "0"], "--reml-cg-tol 0: the tolerance must be a finite number > 0"),
    (["--reml-cg-tol", "inf"], "--reml-cg-tol inf: the tolerance must be a finite number > 0"),
    (["--reml-cg-iters", "0"], "--reml-cg-iters 0: needs at least one iteration"),
    (["--reml-tol", "-1"], "--reml-tol -1: the tolerance on log delta must be a finite number > 0"),
])
def test_values_out_of_range(base, extra, msg):
    refused(run(*base, "--reml", *extra), msg)


def test_order_of_the_checks(base):
    """an orphan option of an earlier mode, the earlier modes' own checks, then --reml's: bayesW, the combination, --restart, the
    processes, the values, and only then the files (the covariates)"""
    w = [("bayesWMPI" if a == "bayesMPI" else a) for a in base]
    refused(run(*base, "--reml", "--he-out", "x"), "--he-out needs --he")
    refused(run(*base, "--reml", "--ld-window", "0"), "the window must be 1 to 4096 markers")
    refused(run(*w, "--reml", "--he", "--restart", "--reml-trials", "0"), "--he takes a bayesMPI command line")
    refused(run(*w, "--reml", "--restart", "--reml-trials", "0"), "--reml takes a bayesMPI command line")
    refused(run(*base, "--reml", "--he", "--restart", "--reml-trials", "0", env={"WORLD_SIZE": "2", "RANK": "0"}), "--he does not sample")
    refused(run(*base, "--reml", "--restart", "--reml-trials", "0", env={"WORLD_SIZE": "2", "RANK": "0"}), "--reml does not sample")
    refused(run(*base, "--reml", "--reml-trials", "0", env={"WORLD_SIZE": "2", "RANK": "0"}), "--reml runs on one process")
    refused(run(*base, "--reml", "--reml-trials", "0", "--reml-tol", "0"), "--reml-trials 0")
    refused(run(*base, "--reml", "--reml-tol", "0", *write_cov(base, 32)), "--reml-tol 0")
    refused(run(*base, "--reml", "--reml-trials", "0", "--sumstats", "s"), "--reml-trials 0")


def test_refused_with_too_many_covariates(base):
    refused(run(*base, "--reml", *write_cov(base, 32)), "--reml takes at most 31 covariates (32 given)")


def test_refused_with_dependent_covariates(base):
    refused(run(*base, "--reml", *write_cov(base, 3, dependent=True)), "--reml: the covariates are rank-deficient")


def test_valid_command_line_reaches_the_device(base, tmp_path):
    """Every option check passes and the outputs are opened before the device: on a machine without a GPU the first device call
    refuses, with .reml and .reml.blup there; with one the run succeeds and leaves the same files."""
    has_gpu = os.path.exists("/dev/kfd")
    out = str(tmp_path / "h.reml")
    r = run(*base, "--reml", "--reml-blup", "--reml-out", out, "--reml-trials", "3", "--seed", "5", *write_cov(base, 2))
    if has_gpu:
        assert r.returncode == 0 and "REML   :" in r.stdout, r.stderr
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    assert os.path.exists(out) and os.path.exists(out + ".blup")
    r = run(*base, "--reml", "--seed", "5")  # the default path is <dir>/<name>.reml
    assert (r.returncode == 0) == has_gpu, r.stderr
    assert os.path.exists(str(tmp_path / "o" / "n.reml")) and not os.path.exists(str(tmp_path / "o" / "n.reml.blup"))
