"""hydra_mi355x --ld-window, the part that runs before any device is touched: every refusal, and that a valid command line reaches
the device.  No GPU needed."""
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
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--ld-window", "5"),
            "--ld-window takes a bayesMPI command line, not --mpibayes bayesWMPI")


def test_refused_with_predict_bfile(base):
    refused(run(*base, "--ld-window", "5", "--predict-bfile", "t"), "--ld-window cannot be combined with --predict-bfile")


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--ld-window", "5"), "--ld-window does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--ld-window", "5", env={"WORLD_SIZE": "2", "RANK": "0"}), "--ld-window runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("w", ["0", "-3", "4097", "100000"])
def test_window_out_of_range(base, w):
    refused(run(*base, "--ld-window", w), "the window must be 1 to 4096 markers")


@pytest.mark.parametrize("t", ["-0.1", "1.5"])
def test_r2_threshold_out_of_range(base, t):
    refused(run(*base, "--ld-window", "5", "--ld-window-r2", t), "--ld-window-r2 must be in [0, 1]")


def test_negative_kb(base):
    refused(run(*base, "--ld-window", "5", "--ld-window-kb", "-1"), "--ld-window-kb must not be negative")


@pytest.mark.parametrize("extra", [["--ld-out", "x.ld"], ["--ld-window-kb", "100"], ["--ld-window-r2", "0.5"], ["--ld-bin"]])
def test_ld_options_need_ld_window(base, extra):
    refused(run(*base, *extra), "%s needs --ld-window" % extra[0])


def test_valid_command_line_reaches_the_device(base):
    """Every option check passes; on a machine without a GPU the first device call refuses (on a GPU box this test is moot)."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        has_gpu = hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        has_gpu = False
    if has_gpu:
        pytest.skip("a GPU is present")
    r = run(*base, "--ld-window", "4", "--ld-window-kb", "1000", "--ld-window-r2", "0", "--ld-bin")
    assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    # the report comes before the device: 12 markers on one chromosome, pairs (j, j + d) for d <= 4: 11 + 10 + 9 + 8
    assert "LD     : 12 markers, window 4 markers and 1000000 bp, 1 chromosomes, 38 pairs in the window" in r.stdout
