"""hydra_mi355x --epistasis, the part that runs before any device is touched: every refusal, the order of the checks, and that a valid
command line reaches the device with .epi.cc created and its header written.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 30, 12
HEADER = "CHR1\tSNP1\tBP1\tCHR2\tSNP2\tBP2\tN\tN_CASE\tN_CTRL\tKSA\tCHISQ\tDF\tP\tOK\n"
TWO = "a case/control phenotype takes exactly two (the larger one is the case)"


def run(*args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=60, env=e)


def make(tmp_path, y):
    geno = synth.make_genotypes(M, N, seed=1)
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=[4])
    return ["--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"),
            "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(M)]


@pytest.fixture()
def base(tmp_path):
    return make(tmp_path, (np.arange(N) % 3 == 0).astype(float))


def refused(r, msg):
    assert r.returncode != 0, r.stdout
    assert msg in r.stderr, r.stderr
    assert "invalid option" not in r.stderr and "hgibbs_create" not in r.stderr


def sets_file(tmp_path, rows):
    p = str(tmp_path / "sets.txt")
    with open(p, "w") as f:
        for s, snp in rows:
            f.write("%s %s\n" % (s, snp))
    return p


def test_refused_with_bayesw(base):
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--epistasis"),
            "--epistasis takes a bayesMPI command line, not --mpibayes bayesWMPI")


@pytest.mark.parametrize("other", [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"], ["--pve"], ["--grm"],
                                   ["--ld-score"], ["--clump", "t"], ["--ld-prune", "0.5"], ["--he"], ["--qc"], ["--homozyg"]])
def test_refused_with_an_earlier_mode(base, other):
    refused(run(*base, "--epistasis", *other), "--epistasis cannot be combined with %s" % other[0])


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--epistasis"), "--epistasis does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--epistasis", env={"WORLD_SIZE": "2", "RANK": "0"}), "--epistasis runs on one process (WORLD_SIZE = 2)")


def test_refused_without_bfile(base):
    args = [a for a in base if a != "--bfile" and not a.endswith("/x")]
    refused(run(*args, "--sparse-dir", "d", "--sparse-basename", "b", "--epistasis"), "--epistasis needs --bfile")


@pytest.mark.parametrize("extra", [["--epistasis-chisq", "20"], ["--epistasis-sets", "s"], ["--epistasis-gap", "100"], ["--epistasis-out", "x"]])
def test_epistasis_options_need_epistasis(base, extra):
    refused(run(*base, *extra), "%s needs --epistasis" % extra[0])


CHISQ = "the threshold on the statistic must be a finite number > 0"
GAP = "the gap must be a finite number of kilobases from 0 to 1e12"


@pytest.mark.parametrize("extra,msg", [
    (["--epistasis-chisq", "0"], "--epistasis-chisq 0: " + CHISQ),
    (["--epistasis-chisq", "-3"], "--epistasis-chisq -3: " + CHISQ),
    (["--epistasis-chisq", "inf"], "--epistasis-chisq inf: " + CHISQ),
    (["--epistasis-chisq", "nan"], "--epistasis-chisq nan: " + CHISQ),
    (["--epistasis-chisq", "30x"], "--epistasis-chisq 30x: " + CHISQ),
    (["--epistasis-gap", "-1"], "--epistasis-gap -1: " + GAP),
    (["--epistasis-gap", "nan"], "--epistasis-gap nan: " + GAP),
    (["--epistasis-gap", "10kb"], "--epistasis-gap 10kb: " + GAP),
])
def test_bad_arguments(base, extra, msg):
    refused(run(*base, "--epistasis", *extra), msg)


@pytest.mark.parametrize("y,count", [(np.zeros(N), 1), (np.arange(N) % 3, 3), (np.linspace(0.0, 1.0, N), N - 1)])
def test_phenotype_that_is_not_two_valued(tmp_path, y, count):
    base = make(tmp_path, np.asarray(y, dtype=float))
    refused(run(*base, "--epistasis"), "--epistasis: the phenotype takes %d distinct values on the kept rows, %s" % (count, TWO))
    # --assoc-logistic keeps its own text
    refused(run(*base, "--assoc", "--assoc-no-loco", "--assoc-logistic"), "--assoc-logistic: the phenotype takes %d distinct values on the kept rows, %s" % (count, TWO))


def test_the_na_row_does_not_count_as_a_value(tmp_path):
    y = (np.arange(N) % 2).astype(float)
    y[4] = 7.0  # the NA row: written as NA
    base = make(tmp_path, y)
    r = run(*base, "--epistasis")
    assert "the phenotype takes" not in r.stderr and "invalid option" not in r.stderr, r.stderr
    assert "EPISTASIS: 29 rows (15 cases, 14 controls); 12 markers listed, 66 pairs; CHISQ >= 30\n" in r.stdout, r.stdout
    assert r.returncode == 0 or "hgibbs_create" in r.stderr, r.stderr


def test_sets_refusals(base, tmp_path):
    three = sets_file(tmp_path, [("g1", "snp0"), ("g1", "snp1"), ("g2", "snp2"), ("g3", "snp3")])
    refused(run(*base, "--epistasis", "--epistasis-sets", three),
            "--epistasis-sets %s names 3 sets (g1, g2, g3): one set is scanned within itself, two against each other, more are not taken" % three)
    four = sets_file(tmp_path, [("g1", "snp0"), ("g2", "snp2"), ("g3", "snp3"), ("g4", "snp3")])
    refused(run(*base, "--epistasis", "--epistasis-sets", four), "names 4 sets (g1, g2, g3, ...)")
    empty = sets_file(tmp_path, [("g1", "snp0"), ("g1", "snp1"), ("g2", "nosuch")])
    refused(run(*base, "--epistasis", "--epistasis-sets", empty), "--epistasis-sets %s: set g2 is empty (none of its ids is in " % empty)
    refused(run(*base, "--epistasis", "--epistasis-sets", str(tmp_path / "absent")), "can not open the file")
    bad = sets_file(tmp_path, [("g1", "snp0"), ("g1", "snp0")])
    refused(run(*base, "--epistasis", "--epistasis-sets", bad), "SNP snp0 is given twice for set g1")


def test_order_of_the_refusals(base, tmp_path):
    """the checks of the earlier modes come before --epistasis's and keep their messages; then the frame's, the arguments, the
    phenotype, the sets"""
    refused(run(*base, "--epistasis", "--ld-window", "0"), "the window must be 1 to 4096 markers")
    refused(run(*base, "--epistasis", "--homozyg", "--homozyg-window-snp", "99"), "--homozyg-window-snp 99")
    refused(run(*base, "--epistasis", "--homozyg-gap", "5"), "--homozyg-gap needs --homozyg")
    refused(run(*base, "--epistasis", "--epistasis-chisq", "0", "--qc"), "--epistasis cannot be combined with --qc")
    refused(run(*base, "--epistasis", "--epistasis-chisq", "0", "--restart"), "--epistasis does not sample")
    three = sets_file(tmp_path, [("g1", "snp0"), ("g2", "snp2"), ("g3", "snp3")])
    refused(run(*base, "--epistasis", "--epistasis-chisq", "0", "--epistasis-sets", three), "--epistasis-chisq 0: " + CHISQ)
    base3 = make(tmp_path, (np.arange(N) % 3).astype(float))
    refused(run(*base3, "--epistasis", "--epistasis-gap", "-1", "--epistasis-sets", three), "--epistasis-gap -1: " + GAP)
    refused(run(*base3, "--epistasis", "--epistasis-sets", three), "--epistasis: the phenotype takes 3 distinct values")


def has_gpu():
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        return hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        return False


def test_valid_command_line_reaches_the_device(base, tmp_path):
    """Every check passes, the markers and pairs are printed and the output is opened before the device: on a machine without a GPU
    the first device call refuses, with .epi.cc there and its header written; with one the run succeeds and leaves the same file."""
    gpu = has_gpu()
    out = str(tmp_path / "e.txt")
    two = sets_file(tmp_path, [("g1", "snp0"), ("g1", "snp1"), ("g1", "snp5"), ("g2", "snp1"), ("g2", "snp5"), ("g2", "snp7"), ("g2", "nosuch")])
    r = run(*base, "--epistasis", "--epistasis-out", out, "--epistasis-chisq", "3.5", "--epistasis-gap", "0.001", "--epistasis-sets", two)
    if gpu:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    # 3 x 3 pairs, less (snp1, snp1) and (snp5, snp5), and (snp1, snp5) with (snp5, snp1) once
    assert "EPISTASIS: 29 rows (10 cases, 19 controls); 6 markers in two sets listed, 6 pairs; CHISQ >= 3.5, gap 0.001 kb, 1 ids of the sets are not in the .bim" in r.stdout
    assert open(out).readline() == HEADER
    # the default file is <dir>/<name>.epi.cc, the default scan every marker against every later one
    r = run(*base, "--epistasis")
    assert (r.returncode == 0) == gpu, r.stderr
    assert "EPISTASIS: 29 rows (10 cases, 19 controls); 12 markers listed, 66 pairs; CHISQ >= 30\n" in r.stdout
    assert open(str(tmp_path / "o" / "n.epi.cc")).readline() == HEADER
