"""hydra_mi355x --qc, the part that runs before any device is touched: every refusal, the order of the checks, and that a valid
command line reaches the device with its six tables and two lists created and their headers written.  No GPU needed."""
import ctypes
import os
import subprocess

import pytest

from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 30, 12

HEADERS = {
    ".frq": "CHR\tSNP\tA1\tA2\tMAF\tNCHROBS\n",
    ".lmiss": "CHR\tSNP\tN_MISS\tN_GENO\tF_MISS\n",
    ".hwe": "CHR\tSNP\tTEST\tA1\tA2\tGENO\tO(HET)\tE(HET)\tP\n",
    ".imiss": "FID\tIID\tN_MISS\tN_GENO\tF_MISS\n",
    ".het": "FID\tIID\tO(HOM)\tE(HOM)\tN(NM)\tF\n",
    ".ibc": "FID\tIID\tNOMISS\tFhat1\tFhat2\tFhat3\n",
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
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--qc"),
            "--qc takes a bayesMPI command line, not --mpibayes bayesWMPI")


@pytest.mark.parametrize("other", [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"], ["--pve"], ["--grm"],
                                   ["--ld-score"], ["--clump", "t"], ["--ld-prune", "0.5"], ["--he"]])
def test_refused_with_an_earlier_mode(base, other):
    refused(run(*base, "--qc", *other), "--qc cannot be combined with %s" % other[0])


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--qc"), "--qc does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--qc", env={"WORLD_SIZE": "2", "RANK": "0"}), "--qc runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("extra", [["--qc-out", "x"], ["--qc-maf", "0.01"], ["--qc-geno", "0.1"], ["--qc-mind", "0.1"], ["--qc-hwe", "1e-6"],
                                   ["--qc-het-sd", "3"]])
def test_qc_options_need_qc(base, extra):
    refused(run(*base, *extra), "%s needs --qc" % extra[0])


@pytest.mark.parametrize("extra,msg", [
    (["--qc-maf", "0.6"], "--qc-maf 0.6: the minor allele frequency must be a number in [0, 0.5]"),
    (["--qc-maf", "-0.1"], "--qc-maf -0.1: the minor allele frequency must be a number in [0, 0.5]"),
    (["--qc-maf", "0.1x"], "--qc-maf 0.1x: the minor allele frequency must be a number in [0, 0.5]"),
    (["--qc-geno", "1.5"], "--qc-geno 1.5: the missing rate of a marker must be a number in [0, 1]"),
    (["--qc-geno", "abc"], "--qc-geno abc: the missing rate of a marker must be a number in [0, 1]"),
    (["--qc-mind", "-1"], "--qc-mind -1: the missing rate of an individual must be a number in [0, 1]"),
    (["--qc-mind", "nan"], "--qc-mind nan: the missing rate of an individual must be a number in [0, 1]"),
    (["--qc-hwe", "2"], "--qc-hwe 2: the P value must be a number in [0, 1]"),
    (["--qc-hwe", "1e-6 "], "--qc-hwe 1e-6 : the P value must be a number in [0, 1]"),
    (["--qc-het-sd", "0"], "--qc-het-sd 0: the number of standard deviations must be a finite number > 0"),
    (["--qc-het-sd", "-3"], "--qc-het-sd -3: the number of standard deviations must be a finite number > 0"),
    (["--qc-het-sd", "inf"], "--qc-het-sd inf: the number of standard deviations must be a finite number > 0"),
    (["--qc-het-sd", "three"], "--qc-het-sd three: the number of standard deviations must be a finite number > 0"),
])
def test_bad_thresholds(base, extra, msg):
    refused(run(*base, "--qc", *extra), msg)


def test_existing_checks_run_first(base):
    """the checks of the earlier modes come before --qc's and keep their messages"""
    refused(run(*base, "--qc", "--ld-window", "0"), "the window must be 1 to 4096 markers")
    refused(run(*base, "--qc", "--ld-window", "5", "--predict-bfile", "t"), "--ld-window cannot be combined with --predict-bfile")
    refused(run(*base, "--qc", "--assoc", "--ld-window", "5"), "--assoc cannot be combined with --ld-window")
    refused(run(*base, "--qc", "--predict-out", "p"), "--predict-out needs --predict-bfile")
    refused(run(*base, "--qc", "--grm", "--grm-sparse", "abc"), "--grm-sparse abc: the cutoff must be a finite number")
    refused(run(*base, "--qc", "--he-rows"), "--he-rows needs --he")
    refused(run(*base, "--qc", "--qc-maf", "7", "--he"), "--qc cannot be combined with --he")


def has_gpu():
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        return hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        return False


def test_valid_command_line_reaches_the_device(base, tmp_path):
    """Every option check passes and the outputs are opened before the device: on a machine without a GPU the first device call
    refuses, with the six tables and the two lists there and their headers written; with one the run succeeds and leaves the same
    files."""
    gpu = has_gpu()
    out = str(tmp_path / "q")
    r = run(*base, "--qc", "--qc-out", out, "--qc-maf", "0.05", "--qc-geno", "0.1", "--qc-mind", "0.1", "--qc-hwe", "1e-6", "--qc-het-sd", "3")
    if gpu:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    for ext, head in HEADERS.items():
        assert open(out + ext).readline() == head, ext
    assert open(out + ".qc.exclude").readline() == "SNP\tREASON\n"
    assert open(out + ".qc.remove").readline() == "FID\tIID\tREASON\n"
    # the default prefix is <dir>/<name>; without thresholds no list; one kind of threshold, one list
    r = run(*base, "--qc")
    assert (r.returncode == 0) == gpu, r.stderr
    d = str(tmp_path / "o" / "n")
    assert all(os.path.exists(d + ext) for ext in HEADERS)
    assert not os.path.exists(d + ".qc.exclude") and not os.path.exists(d + ".qc.remove")
    r = run(*base, "--qc", "--qc-mind", "0.2")
    assert (r.returncode == 0) == gpu, r.stderr
    assert not os.path.exists(d + ".qc.exclude") and os.path.exists(d + ".qc.remove")
