"""hydra_mi355x --grm, the part that runs before any device is touched: every refusal, the order of the checks, and that a valid
command line reaches the device with its .grm.id written.  No GPU needed."""
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
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--grm"),
            "--grm takes a bayesMPI command line, not --mpibayes bayesWMPI")


@pytest.mark.parametrize("other", [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"], ["--pve"]])
def test_refused_with_an_earlier_mode(base, other):
    refused(run(*base, "--grm", *other), "--grm cannot be combined with %s" % other[0])


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--grm"), "--grm does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--grm", env={"WORLD_SIZE": "2", "RANK": "0"}), "--grm runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("t", ["nan", "inf", "-inf", "abc", "0.1x", ""])
def test_sparse_cutoff_not_a_finite_number(base, t):
    refused(run(*base, "--grm", "--grm-sparse", t), "--grm-sparse %s: the cutoff must be a finite number" % t)


@pytest.mark.parametrize("extra", [["--grm-out", "x"], ["--grm-sparse", "0.05"]])
def test_grm_options_need_grm(base, extra):
    refused(run(*base, *extra), "%s needs --grm" % extra[0])


def test_existing_checks_run_first(base):
    """the --ld-window, --predict-bfile and --assoc checks come before --grm's and keep their messages"""
    refused(run(*base, "--grm", "--ld-window", "0"), "the window must be 1 to 4096 markers")
    refused(run(*base, "--grm", "--ld-window", "5", "--predict-bfile", "t"), "--ld-window cannot be combined with --predict-bfile")
    refused(run(*base, "--grm", "--assoc", "--ld-window", "5"), "--assoc cannot be combined with --ld-window")
    refused(run(*base, "--grm", "--predict-out", "p"), "--predict-out needs --predict-bfile")


def test_valid_command_line_reaches_the_device(base, tmp_path):
    """Every option check passes and the outputs are opened before the device: on a machine without a GPU the first device call
    refuses, with .grm.id complete and .grm.bin there; with one the run succeeds and leaves the same files."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        has_gpu = hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        has_gpu = False
    prefix = str(tmp_path / "g")
    r = run(*base, "--grm", "--grm-sparse", "-0.5", "--grm-out", prefix)
    if has_gpu:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    kept = [i for i in range(N) if i != 4]
    with open(prefix + ".grm.id") as f:
        assert f.read() == "".join("fam%d\tind%d\n" % (i, i) for i in kept)
    assert len(kept) == 29
    assert os.path.exists(prefix + ".grm.bin") and os.path.exists(prefix + ".grm.N.bin") and os.path.exists(prefix + ".grm.sp")
