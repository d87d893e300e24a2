"""hydra_mi355x --homozyg, the part that runs before any device is touched: every refusal, the order of the checks, and that a valid
command line reaches the device with its three tables created and their headers written.  No GPU needed."""
import ctypes
import os
import subprocess

import pytest

from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 30, 12

HEADERS = {
    ".hom": "FID\tIID\tCHR\tSNP1\tSNP2\tPOS1\tPOS2\tKB\tNSNP\tDENSITY\tPHOM\tPHET\n",
    ".hom.indiv": "FID\tIID\tNSEG\tKB\tKBAVG\tFROH\n",
    ".hom.summary": "CHR\tSNP\tBP\tN_ROH\n",
}


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
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--homozyg"),
            "--homozyg takes a bayesMPI command line, not --mpibayes bayesWMPI")


@pytest.mark.parametrize("other", [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"], ["--pve"], ["--grm"],
                                   ["--ld-score"], ["--clump", "t"], ["--ld-prune", "0.5"], ["--he"], ["--qc"]])
def test_refused_with_an_earlier_mode(base, other):
    refused(run(*base, "--homozyg", *other), "--homozyg cannot be combined with %s" % other[0])


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--homozyg"), "--homozyg does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--homozyg", env={"WORLD_SIZE": "2", "RANK": "0"}), "--homozyg runs on one process (WORLD_SIZE = 2)")


def test_refused_without_bfile(base):
    args = [a for a in base if a != "--bfile" and not a.endswith("/x")]
    refused(run(*args, "--sparse-dir", "d", "--sparse-basename", "b", "--homozyg"), "--homozyg needs --bfile")


@pytest.mark.parametrize("extra", [["--homozyg-window-snp", "20"], ["--homozyg-window-het", "0"], ["--homozyg-window-missing", "2"],
                                   ["--homozyg-window-threshold", "0.1"], ["--homozyg-snp", "10"], ["--homozyg-kb", "500"], ["--homozyg-density", "20"],
                                   ["--homozyg-gap", "100"], ["--homozyg-het", "3"], ["--homozyg-out", "x"]])
def test_homozyg_options_need_homozyg(base, extra):
    refused(run(*base, *extra), "%s needs --homozyg" % extra[0])


WINDOW = "the window must be an integer from 1 to 64 markers (the widest hgibbs_roh takes: a window is one 64-bit word)"
THRESHOLD = "the share of homozygous windows must be a number in (0, 1]"


@pytest.mark.parametrize("extra,msg", [
    (["--homozyg-window-snp", "0"], "--homozyg-window-snp 0: " + WINDOW),
    (["--homozyg-window-snp", "65"], "--homozyg-window-snp 65: " + WINDOW),
    (["--homozyg-window-snp", "50x"], "--homozyg-window-snp 50x: " + WINDOW),
    (["--homozyg-window-snp", "5.5"], "--homozyg-window-snp 5.5: " + WINDOW),
    (["--homozyg-window-het", "-1"], "--homozyg-window-het -1: the hets a window may hold must be an integer from 0 to 64"),
    (["--homozyg-window-het", "one"], "--homozyg-window-het one: the hets a window may hold must be an integer from 0 to 64"),
    (["--homozyg-window-missing", "65"], "--homozyg-window-missing 65: the missing calls a window may hold must be an integer from 0 to 64"),
    (["--homozyg-window-missing", "1 "], "--homozyg-window-missing 1 : the missing calls a window may hold must be an integer from 0 to 64"),
    (["--homozyg-window-threshold", "0"], "--homozyg-window-threshold 0: " + THRESHOLD),
    (["--homozyg-window-threshold", "1.01"], "--homozyg-window-threshold 1.01: " + THRESHOLD),
    (["--homozyg-window-threshold", "nan"], "--homozyg-window-threshold nan: " + THRESHOLD),
    (["--homozyg-window-threshold", "0.05x"], "--homozyg-window-threshold 0.05x: " + THRESHOLD),
    (["--homozyg-snp", "0"], "--homozyg-snp 0: the markers a segment needs must be an integer >= 1"),
    (["--homozyg-snp", "1e2"], "--homozyg-snp 1e2: the markers a segment needs must be an integer >= 1"),
    (["--homozyg-snp", "2147483648"], "--homozyg-snp 2147483648: the markers a segment needs must be an integer >= 1"),
    (["--homozyg-het", "-2"], "--homozyg-het -2: the hets a segment may hold must be an integer >= 0"),
    (["--homozyg-het", "x"], "--homozyg-het x: the hets a segment may hold must be an integer >= 0"),
    (["--homozyg-kb", "-1"], "--homozyg-kb -1: the length a segment needs must be a finite number of kilobases from 0 to 1e12"),
    (["--homozyg-kb", "inf"], "--homozyg-kb inf: the length a segment needs must be a finite number of kilobases from 0 to 1e12"),
    (["--homozyg-kb", "1000kb"], "--homozyg-kb 1000kb: the length a segment needs must be a finite number of kilobases from 0 to 1e12"),
    (["--homozyg-density", "-0.5"], "--homozyg-density -0.5: the kilobases per marker a segment may have must be a finite number from 0 to 1e12"),
    (["--homozyg-density", "nan"], "--homozyg-density nan: the kilobases per marker a segment may have must be a finite number from 0 to 1e12"),
    (["--homozyg-gap", "-1"], "--homozyg-gap -1: the gap that cuts a segment must be a finite number of kilobases from 0 to 1e12"),
    (["--homozyg-gap", "1e13"], "--homozyg-gap 1e13: the gap that cuts a segment must be a finite number of kilobases from 0 to 1e12"),
])
def test_bad_arguments(base, extra, msg):
    refused(run(*base, "--homozyg", *extra), msg)


def test_existing_checks_run_first(base):
    """the checks of the earlier modes come before --homozyg's and keep their messages"""
    refused(run(*base, "--homozyg", "--ld-window", "0"), "the window must be 1 to 4096 markers")
    refused(run(*base, "--homozyg", "--assoc", "--ld-window", "5"), "--assoc cannot be combined with --ld-window")
    refused(run(*base, "--homozyg", "--predict-out", "p"), "--predict-out needs --predict-bfile")
    refused(run(*base, "--homozyg", "--qc", "--qc-maf", "7"), "--qc-maf 7: the minor allele frequency must be a number in [0, 0.5]")
    refused(run(*base, "--homozyg", "--qc-maf", "0.1"), "--qc-maf needs --qc")
    refused(run(*base, "--homozyg", "--homozyg-window-snp", "99", "--he"), "--homozyg cannot be combined with --he")


def rewrite_bim(base, rows):
    prefix = base[base.index("--bfile") + 1]
    with open(prefix + ".bim", "w") as f:
        for j, (c, bp) in enumerate(rows):
            f.write("%s snp%d 0 %d A C\n" % (c, j, bp))
    return prefix + ".bim"


def test_bim_refusals(base):
    """an autosome must be one run of the .bim, in bp order; other chromosomes may come in any shape"""
    bim = rewrite_bim(base, [(1, 10), (1, 20), (2, 5), (2, 6), (1, 30)] + [(3, 10 * j) for j in range(7)])
    refused(run(*base, "--homozyg"), bim + ": chromosome 1 comes back at marker snp4 (row 5) after another chromosome: --homozyg needs every "
            "chromosome as one contiguous run")
    bim = rewrite_bim(base, [(1, 10), (1, 20), (2, 5), (2, 4)] + [(3, 10 * j) for j in range(8)])
    refused(run(*base, "--homozyg"), bim + ": bp decreases at marker snp3 (row 4) inside chromosome 2: --homozyg needs the markers of a "
            "chromosome in bp order")
    rewrite_bim(base, [(23, 10), (1, 20), (23, 5), (23, 4)] + [(3, 10 * j) for j in range(8)])
    r = run(*base, "--homozyg")
    assert r.returncode == 0 or "hgibbs_create" in r.stderr, r.stderr


def has_gpu():
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        return hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        return False


def test_valid_command_line_reaches_the_device(base, tmp_path):
    """Every option check passes and the outputs are opened before the device: on a machine without a GPU the first device call
    refuses, with the three tables there and their headers written; with one the run succeeds and leaves the same files."""
    gpu = has_gpu()
    out = str(tmp_path / "h")
    r = run(*base, "--homozyg", "--homozyg-out", out, "--homozyg-window-snp", "4", "--homozyg-window-het", "0", "--homozyg-window-missing", "1",
            "--homozyg-window-threshold", "0.5", "--homozyg-snp", "3", "--homozyg-kb", "0.001", "--homozyg-density", "1", "--homozyg-gap", "0.5",
            "--homozyg-het", "0")
    if gpu:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    for ext, head in HEADERS.items():
        assert open(out + ext).readline() == head, ext
    # the default prefix is <dir>/<name>
    r = run(*base, "--homozyg")
    assert (r.returncode == 0) == gpu, r.stderr
    d = str(tmp_path / "o" / "n")
    assert all(os.path.exists(d + ext) for ext in HEADERS)
