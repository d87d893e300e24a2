"""hydra_mi355x --pca, the part that runs before any device is touched: every refusal, the order of the checks, and that a valid
command line reaches the device with the .eigenvec header already written.  No GPU needed."""
import ctypes
import os
import subprocess

import pytest

from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 30, 12


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


def refused(r, msg):
    assert r.returncode != 0, r.stdout
    assert msg in r.stderr, r.stderr
    assert "invalid option" not in r.stderr and "hgibbs_create" not in r.stderr


def test_refused_with_bayesw(base):
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--pca", "3"),
            "--pca takes a bayesMPI command line, not --mpibayes bayesWMPI")


def test_refused_with_predict_bfile(base):
    refused(run(*base, "--pca", "3", "--predict-bfile", "t"), "--pca cannot be combined with --predict-bfile")


def test_refused_with_ld_window(base):
    refused(run(*base, "--pca", "3", "--ld-window", "5"), "--pca cannot be combined with --ld-window")


def test_refused_with_assoc(base):
    refused(run(*base, "--pca", "3", "--assoc"), "--pca cannot be combined with --assoc")


def test_refused_with_king(base):
    refused(run(*base, "--pca", "3", "--king"), "--pca cannot be combined with --king")


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--pca", "3"), "--pca does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--pca", "3", env={"WORLD_SIZE": "2", "RANK": "0"}), "--pca runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("k", ["0", "-1", "25", "100", "2.5", "abc", "3x", "", "nan"])
def test_k_not_an_integer_from_1_to_24(base, k):
    refused(run(*base, "--pca", k), "the number of components must be an integer from 1 to 24")


@pytest.mark.parametrize("p", ["0", "-3", "1.5", "abc", ""])
def test_iterations_below_one(base, p):
    refused(run(*base, "--pca", "3", "--pca-iters", p), "needs at least one iteration")


def test_iterations_beyond_an_int(base):
    refused(run(*base, "--pca", "3", "--pca-iters", "3000000000"), "at most 2147483647 iterations")


@pytest.mark.parametrize("t", ["nan", "inf", "-inf", "-1e-3", "abc", "1e-3x", ""])
def test_tolerance_not_a_finite_number_ge_0(base, t):
    refused(run(*base, "--pca", "3", "--pca-tol", t), "the tolerance must be a finite number >= 0")


@pytest.mark.parametrize("extra", [["--pca-iters", "5"], ["--pca-tol", "1e-6"], ["--pca-out", "x.eigenvec"], ["--pca-loadings"]])
def test_pca_options_need_pca(base, extra):
    refused(run(*base, *extra), "%s needs --pca" % extra[0])


def test_existing_checks_run_first(base):
    """the --ld-window, --predict-bfile, --assoc and --king checks come before --pca's and keep their messages"""
    refused(run(*base, "--pca", "3", "--ld-window", "0"), "the window must be 1 to 4096 markers")
    refused(run(*base, "--pca", "3", "--ld-window", "5", "--predict-bfile", "t"), "--ld-window cannot be combined with --predict-bfile")
    refused(run(*base, "--pca", "3", "--assoc", "--ld-window", "5"), "--assoc cannot be combined with --ld-window")
    refused(run(*base, "--pca", "3", "--king", "--assoc"), "--king cannot be combined with --assoc")
    refused(run(*base, "--pca", "3", "--king", "--king-cutoff", "x"), "the cutoff must be a finite number")
    refused(run(*base, "--pca", "3", "--predict-out", "p"), "--predict-out needs --predict-bfile")
    refused(run(*base, "--pca", "3", "--king-out", "k"), "--king-out needs --king")


def test_valid_command_line_reaches_the_device(base, tmp_path):
    """Every option check passes; on a machine without a GPU the first device call refuses (on a GPU box this test is moot)."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        has_gpu = hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        has_gpu = False
    if has_gpu:
        pytest.skip("a GPU is present")
    out = str(tmp_path / "p.eigenvec")
    r = run(*base, "--pca", "3", "--pca-iters", "7", "--pca-tol", "0", "--pca-loadings", "--pca-out", out, "--seed", "5")
    assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    # the table is opened, and its header written, before the device
    with open(out) as f:
        assert f.read() == "#FID\tIID\tPC1\tPC2\tPC3\n"
    assert "seed 5" in r.stdout
