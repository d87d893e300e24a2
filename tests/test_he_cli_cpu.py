"""hydra_mi355x --he, the part that runs before any device is touched: every refusal, the order of the checks, and that a valid
command line reaches the device with its .HEreg created.  No GPU needed."""
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
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--he"),
            "--he takes a bayesMPI command line, not --mpibayes bayesWMPI")


@pytest.mark.parametrize("other", [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"], ["--pve"], ["--grm"],
                                   ["--ld-score"], ["--clump", "t"], ["--ld-prune", "0.5"]])
def test_refused_with_an_earlier_mode(base, other):
    refused(run(*base, "--he", *other), "--he cannot be combined with %s" % other[0])


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--he"), "--he does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--he", env={"WORLD_SIZE": "2", "RANK": "0"}), "--he runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("extra", [["--he-out", "x"], ["--he-rows"]])
def test_he_options_need_he(base, extra):
    refused(run(*base, *extra), "%s needs --he" % extra[0])


def test_existing_checks_run_first(base):
    """the checks of the earlier modes come before --he's and keep their messages"""
    refused(run(*base, "--he", "--ld-window", "0"), "the window must be 1 to 4096 markers")
    refused(run(*base, "--he", "--ld-window", "5", "--predict-bfile", "t"), "--ld-window cannot be combined with --predict-bfile")
    refused(run(*base, "--he", "--assoc", "--ld-window", "5"), "--assoc cannot be combined with --ld-window")
    refused(run(*base, "--he", "--predict-out", "p"), "--predict-out needs --predict-bfile")
    refused(run(*base, "--he", "--grm", "--grm-sparse", "abc"), "--grm-sparse abc: the cutoff must be a finite number")
    refused(run(*base, "--he", "--grm-out", "g"), "--grm-out needs --grm")


def test_valid_command_line_reaches_the_device(base, tmp_path):
    """Every option check passes and the outputs are opened before the device: on a machine without a GPU the first device call
    refuses, with .HEreg and .HEreg.rows there; with one the run succeeds and leaves the same files."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        has_gpu = hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        has_gpu = False
    out = str(tmp_path / "h.HEreg")
    r = run(*base, "--he", "--he-rows", "--he-out", out)
    if has_gpu:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    assert os.path.exists(out) and os.path.exists(out + ".rows")
    # the default path is <dir>/<name>.HEreg
    r = run(*base, "--he")
    assert (r.returncode == 0) == has_gpu, r.stderr
    assert os.path.exists(str(tmp_path / "o" / "n.HEreg")) and not os.path.exists(str(tmp_path / "o" / "n.HEreg.rows"))
