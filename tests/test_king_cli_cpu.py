"""hydra_mi355x --king, the part that runs before any device is touched: every refusal, the order of the checks, and that a valid
command line reaches the device.  No GPU needed."""
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
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--king"),
            "--king takes a bayesMPI command line, not --mpibayes bayesWMPI")


def test_refused_with_predict_bfile(base):
    refused(run(*base, "--king", "--predict-bfile", "t"), "--king cannot be combined with --predict-bfile")


def test_refused_with_ld_window(base):
    refused(run(*base, "--king", "--ld-window", "5"), "--king cannot be combined with --ld-window")


def test_refused_with_assoc(base):
    refused(run(*base, "--king", "--assoc"), "--king cannot be combined with --assoc")


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--king"), "--king does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--king", env={"WORLD_SIZE": "2", "RANK": "0"}), "--king runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("t", ["nan", "inf", "-inf", "abc", "0.1x", ""])
def test_cutoff_not_a_finite_number(base, t):
    refused(run(*base, "--king", "--king-cutoff", t), "the cutoff must be a finite number")


@pytest.mark.parametrize("extra", [["--king-out", "x.kin0"], ["--king-cutoff", "0.1"]])
def test_king_options_need_king(base, extra):
    refused(run(*base, *extra), "%s needs --king" % extra[0])


def test_existing_checks_run_first(base):
    """the --ld-window, --predict-bfile and --assoc checks come before --king's and keep their messages"""
    refused(run(*base, "--king", "--ld-window", "0"), "the window must be 1 to 4096 markers")
    refused(run(*base, "--king", "--ld-window", "5", "--predict-bfile", "t"), "--ld-window cannot be combined with --predict-bfile")
    refused(run(*base, "--king", "--assoc", "--ld-window", "5"), "--assoc cannot be combined with --ld-window")
    refused(run(*base, "--king", "--predict-out", "p"), "--predict-out needs --predict-bfile")


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
    out = str(tmp_path / "k.kin0")
    r = run(*base, "--king", "--king-cutoff", "-0.5", "--king-out", out)
    assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    # the table is opened, and its header written, before the device
    with open(out) as f:
        assert f.read() == "#FID1\tIID1\tFID2\tIID2\tNSNP\tHETHET\tIBS0\tKINSHIP\n"
