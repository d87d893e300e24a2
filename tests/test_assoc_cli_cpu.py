"""hydra_mi355x --assoc, the part that runs before any device is touched: every refusal, and that a valid command line prints its
report and reaches the device.  No GPU needed."""
import ctypes
import os
import struct
import subprocess

import numpy as np
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


def has_gpu():
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        return hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        return False


@pytest.fixture()
def base(tmp_path):
    geno = synth.make_genotypes(M, N, seed=1)
    y, _ = synth.make_phenotype(geno, seed=2)
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=[4])
    with open(prefix + ".bim", "w") as f:  # chromosomes 1 1 1 1 2 2 2 2 1 1 3 3: four runs, three chromosomes
        for j, c in enumerate("111122221133"):
            f.write("%s snp%d 0 %d A C\n" % (c, j, 100 * j + 1))
    return ["--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"),
            "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(M)]


def write_bet(path, its, m=M):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", m))
        for it in its:
            f.write(struct.pack("<I", it))
            f.write(np.full(m, 0.01).tobytes())


def refused(r, msg):
    assert r.returncode != 0, r.stdout
    assert msg in r.stderr, r.stderr
    assert "invalid option" not in r.stderr and "hgibbs_create" not in r.stderr


def test_refused_with_bayesw(base):
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--assoc"),
            "--assoc takes a bayesMPI command line, not --mpibayes bayesWMPI")


def test_refused_with_predict_bfile(base):
    refused(run(*base, "--assoc", "--predict-bfile", "t"), "--assoc cannot be combined with --predict-bfile")


def test_refused_with_ld_window(base):
    refused(run(*base, "--assoc", "--ld-window", "5"), "--assoc cannot be combined with --ld-window")


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--assoc"), "--assoc does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--assoc", env={"WORLD_SIZE": "2", "RANK": "0"}), "--assoc runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("extra", [["--assoc-out", "x.assoc"], ["--assoc-no-loco"]])
def test_assoc_options_need_assoc(base, extra):
    refused(run(*base, *extra), "%s needs --assoc" % extra[0])


def test_existing_refusals_keep_their_messages(base):
    """the --ld-window and --predict-bfile checks come first: their messages are unchanged with --assoc on the line"""
    refused(run(*base, "--assoc", "--ld-window", "5", "--predict-bfile", "t"), "--ld-window cannot be combined with --predict-bfile")
    refused(run(*base, "--assoc", "--predict-bfile", "t", "--restart"), "--predict-bfile does not sample: it cannot be combined with --restart")


def test_bet_problems_refused(base, tmp_path):
    bet = str(tmp_path / "o" / "n.bet")
    refused(run(*base, "--assoc"), "--assoc takes its LOCO offsets from the chain's effects: run the chain first")
    write_bet(bet, [10, 20], m=M + 1)
    refused(run(*base, "--assoc"), "holds %d markers, --number-markers says %d" % (M + 1, M))
    write_bet(bet, [10, 20])
    refused(run(*base, "--assoc", "--burn-in", "50"), "no record at or after --burn-in 50 (2 records)")


def test_rank_deficient_covariates_refused(base, tmp_path):
    cov = str(tmp_path / "cov.txt")
    with open(cov, "w") as f:
        for i in range(N):
            f.write("f%d i%d 1.5 %d\n" % (i, i, i % 3))  # a constant column next to the intercept
    refused(run(*base, "--covariates", cov, "--assoc", "--assoc-no-loco"), "the covariates are rank-deficient")


def test_valid_command_line_reports_and_reaches_the_device(base, tmp_path):
    """Every check passes and the report comes first; without a GPU the first device call refuses, with one the table is written."""
    write_bet(str(tmp_path / "o" / "n.bet"), [5, 10, 15, 20])
    out = str(tmp_path / "t.assoc")
    r = run(*base, "--assoc", "--burn-in", "10", "--assoc-out", out)
    assert "ASSOC  : 12 markers, 3 chromosomes in 4 runs, 0 covariates, 29 individuals -> %s" % out in r.stdout, r.stdout
    assert "ASSOC  : LOCO offsets from 3 records of %s (iterations 10 .. 20)" % str(tmp_path / "o" / "n.bet") in r.stdout
    if has_gpu():
        assert r.returncode == 0 and "wrote 12 rows" in r.stdout, r.stderr
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    r = run(*base, "--assoc", "--assoc-no-loco")
    assert "no LOCO offsets (--assoc-no-loco)" in r.stdout, r.stdout
    assert (r.returncode == 0) if has_gpu() else ("hgibbs_create" in r.stderr), r.stderr


def test_one_chromosome_warns(base, tmp_path):
    prefix = base[base.index("--bfile") + 1]
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("7 snp%d 0 %d A C\n" % (j, j + 1))
    write_bet(str(tmp_path / "o" / "n.bet"), [5])
    r = run(*base, "--assoc", "--burn-in", "0")
    assert "WARNING: --assoc with one chromosome: G - G_c is 0" in r.stdout, r.stdout
