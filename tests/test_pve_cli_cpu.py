"""hydra_mi355x --pve, the part that runs before any device is touched: every refusal, and that a valid command line prints its
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
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--pve"),
            "--pve takes a bayesMPI command line, not --mpibayes bayesWMPI")


@pytest.mark.parametrize("mode", [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"]])
def test_refused_with_an_earlier_mode(base, mode):
    refused(run(*base, "--pve", *mode), "--pve cannot be combined with %s" % mode[0])


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--pve"), "--pve does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--pve", env={"WORLD_SIZE": "2", "RANK": "0"}), "--pve runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("extra", [["--pve-window-kb", "100"], ["--pve-window-snps", "5"], ["--pve-sets", "s.txt"], ["--pve-groups"],
                                   ["--pve-threshold", "0.1"], ["--pve-out", "x.pve"], ["--pve-bin"]])
def test_pve_options_need_pve(base, extra):
    refused(run(*base, *extra), "%s needs --pve" % extra[0])


@pytest.mark.parametrize("x,y", [(["--pve-window-kb", "1"], ["--pve-window-snps", "5"]), (["--pve-window-kb", "1"], ["--pve-sets", "s.txt"]),
                                 (["--pve-window-snps", "5"], ["--pve-groups"]), (["--pve-sets", "s.txt"], ["--pve-groups"])])
def test_two_set_definers_refused(base, x, y):
    refused(run(*base, "--pve", *y, *x), "%s cannot be combined with %s" % (x[0], y[0]))


@pytest.mark.parametrize("extra,msg", [
    (["--pve-window-kb", "0"], "--pve-window-kb 0: the window must be a finite number of kilobases > 0"),
    (["--pve-window-kb", "-3"], "--pve-window-kb -3: the window must be"),
    (["--pve-window-kb", "1x"], "--pve-window-kb 1x: the window must be"),
    (["--pve-window-kb", "inf"], "--pve-window-kb inf: the window must be"),
    (["--pve-window-snps", "0"], "--pve-window-snps 0: the window must be an integer >= 1"),
    (["--pve-window-snps", "2.5"], "--pve-window-snps 2.5: the window must be an integer >= 1"),
    (["--pve-threshold", "1"], "--pve-threshold 1: the threshold must be a finite number in [0, 1)"),
    (["--pve-threshold", "-0.1"], "--pve-threshold -0.1: the threshold must be"),
    (["--pve-threshold", "nan"], "--pve-threshold nan: the threshold must be"),
    (["--pve-threshold", "half"], "--pve-threshold half: the threshold must be"),
])
def test_bad_arguments_refused(base, extra, msg):
    refused(run(*base, "--pve", *extra), msg)


def test_groups_need_the_group_file(base):
    refused(run(*base, "--pve", "--pve-groups"), "--pve-groups needs --groupIndexFile")


def test_sets_file_problems_refused(base, tmp_path):
    write_bet(str(tmp_path / "o" / "n.bet"), [5, 10])
    sets = str(tmp_path / "sets.txt")
    refused(run(*base, "--pve", "--pve-sets", sets), "can not open the file [%s]" % sets)
    open(sets, "w").write("g1 snp0\ng1 snp3\n\ng2 snp4\ng2 nosuch\n")
    refused(run(*base, "--pve", "--pve-sets", sets), "%s line 5: SNP nosuch is not among the first 12 markers" % sets)
    open(sets, "w").write("g1 snp0\ng2 snp0\ng1 snp3\ng1 snp0\n")
    refused(run(*base, "--pve", "--pve-sets", sets), "%s line 4: SNP snp0 is given twice for set g1" % sets)
    open(sets, "w").write("g1 snp0\ng1\n")
    refused(run(*base, "--pve", "--pve-sets", sets), "%s line 2: expected SETNAME SNPID" % sets)
    open(sets, "w").write("\n")
    refused(run(*base, "--pve", "--pve-sets", sets), "%s names no set" % sets)


def test_bet_problems_refused(base, tmp_path):
    bet = str(tmp_path / "o" / "n.bet")
    refused(run(*base, "--pve"), "--pve takes the variance explained from the chain's effects: run the chain first")
    write_bet(bet, [10, 20], m=M + 1)
    refused(run(*base, "--pve"), "holds %d markers, --number-markers says %d" % (M + 1, M))
    write_bet(bet, [10, 20])
    refused(run(*base, "--pve", "--burn-in", "50"), "no record at or after --burn-in 50 (2 records)")


def test_existing_refusals_keep_their_messages(base):
    """the earlier modes' checks come first: their messages are unchanged with --pve on the line"""
    refused(run(*base, "--pve", "--ld-window", "5", "--predict-bfile", "t"), "--ld-window cannot be combined with --predict-bfile")
    refused(run(*base, "--pve", "--predict-bfile", "t", "--restart"), "--predict-bfile does not sample: it cannot be combined with --restart")
    refused(run(*base, "--pve", "--assoc", "--ld-window", "5"), "--assoc cannot be combined with --ld-window")
    refused(run(*base, "--pve", "--king", "--king-cutoff", "x"), "--king-cutoff x: the cutoff must be a finite number")
    refused(run(*base, "--pve", "--pca", "0"), "--pca 0: the number of components must be an integer from 1 to 24")
    refused(run(*base, "--pve", "--pca-iters", "3"), "--pca-iters needs --pca")


def reaches_the_device(r, rows):
    if has_gpu():
        assert r.returncode == 0 and "PVE    : wrote %d rows" % rows in r.stdout.splitlines()[-1], r.stderr
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr


def test_valid_command_lines_report_and_reach_the_device(base, tmp_path):
    """Every check passes and the report comes first; without a GPU the first device call refuses, with one the table is written."""
    bet = str(tmp_path / "o" / "n.bet")
    write_bet(bet, [5, 10, 15, 20])
    out = str(tmp_path / "t.pve")
    r = run(*base, "--pve", "--burn-in", "10", "--pve-out", out)
    assert ("PVE    : 3 sets (one per chromosome), 12 markers, 29 individuals, 3 records of %s (iterations 10 .. 20), threshold 0.333333 -> %s"
            % (bet, out)) in r.stdout, r.stdout
    reaches_the_device(r, 4)
    r = run(*base, "--pve", "--burn-in", "10", "--pve-window-snps", "3", "--pve-threshold", "0.25")
    # runs of 4, 4, 2, 2 markers in windows of 3: 2 + 2 + 1 + 1
    assert "PVE    : 6 sets (windows of 3 markers), 12 markers, 29 individuals, 3 records of" in r.stdout, r.stdout
    assert "threshold 0.25 -> %s" % str(tmp_path / "o" / "n.pve") in r.stdout, r.stdout
    reaches_the_device(r, 7)
    r = run(*base, "--pve", "--burn-in", "0", "--pve-window-kb", "0.5")
    # bp = 100 j + 1 in windows of 500: chromosome 1 has j = 0..3 | 8, 9, chromosome 2 j = 4 | 5..7, chromosome 3 j = 10, 11
    assert "PVE    : 5 sets (windows of 0.5 kb), 12 markers, 29 individuals, 4 records of" in r.stdout, r.stdout
    reaches_the_device(r, 6)
    sets = str(tmp_path / "sets.txt")
    open(sets, "w").write("far snp11\nnear snp0\nfar snp2\n")
    r = run(*base, "--pve", "--burn-in", "0", "--pve-sets", sets)
    assert "PVE    : 2 sets (from %s), 12 markers" % sets in r.stdout, r.stdout
    reaches_the_device(r, 3)
    grp = str(tmp_path / "groups.txt")
    open(grp, "w").write("\n".join(str(j % 2) for j in range(M)) + "\n")
    mix = str(tmp_path / "mix.txt")
    open(mix, "w").write("0.001,0.01;0.001,0.01\n")
    r = run(*base, "--pve", "--burn-in", "0", "--pve-groups", "--groupIndexFile", grp, "--groupMixtureFile", mix)
    assert "PVE    : 2 sets (the groups of %s), 12 markers" % grp in r.stdout, r.stdout
    reaches_the_device(r, 3)
