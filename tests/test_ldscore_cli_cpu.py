"""hydra_mi355x --ld-score, the part that runs before any device is touched: every refusal, and that a valid command line prints its
report and reaches the device.  No GPU needed."""
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


def has_gpu():
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        return hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        return False


def command(tmp_path, chroms="111111122222", bps=None, m=M):
    """a bayesMPI command line over m markers on the given chromosomes, bp 100 apart unless given"""
    geno = synth.make_genotypes(m, N, seed=1)
    y, _ = synth.make_phenotype(geno, seed=2)
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=[4])
    with open(prefix + ".bim", "w") as f:
        for j in range(m):
            f.write("%s snp%d 0 %d A C\n" % (chroms[j], j, bps[j] if bps else 100 * j + 1))
    return ["--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"),
            "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(m)]


@pytest.fixture()
def base(tmp_path):
    return command(tmp_path)


def refused(r, msg):
    assert r.returncode != 0, r.stdout
    assert msg in r.stderr, r.stderr
    assert "invalid option" not in r.stderr and "hgibbs_create" not in r.stderr


def test_refused_with_bayesw(base):
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--ld-score"),
            "--ld-score takes a bayesMPI command line, not --mpibayes bayesWMPI")


@pytest.mark.parametrize("mode", [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"], ["--pve"], ["--grm"]])
def test_refused_with_an_earlier_mode(base, mode):
    refused(run(*base, "--ld-score", *mode), "--ld-score cannot be combined with %s" % mode[0])


def test_refused_with_restart(base):
    refused(run(*base, "--restart", "--ld-score"), "--ld-score does not sample: it cannot be combined with --restart")


def test_refused_with_several_ranks(base):
    refused(run(*base, "--ld-score", env={"WORLD_SIZE": "2", "RANK": "0"}), "--ld-score runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("extra", [["--ld-score-kb", "100"], ["--ld-score-snps", "5"], ["--ld-score-sets", "s.txt"], ["--ld-score-groups"],
                                   ["--ld-score-raw"], ["--ld-score-out", "p"]])
def test_dependent_options_need_ld_score(base, extra):
    refused(run(*base, *extra), "%s needs --ld-score" % extra[0])


def test_both_windows(base):
    refused(run(*base, "--ld-score", "--ld-score-kb", "100", "--ld-score-snps", "5"),
            "--ld-score-kb cannot be combined with --ld-score-snps: one way to define the window")


def test_both_annotation_options(base, tmp_path):
    refused(run(*base, "--ld-score", "--ld-score-sets", str(tmp_path / "s.txt"), "--ld-score-groups"),
            "--ld-score-sets cannot be combined with --ld-score-groups: one way to define the annotations")


@pytest.mark.parametrize("kb", ["-1", "abc", "nan", "12x"])
def test_kb_negative_or_not_a_number(base, kb):
    refused(run(*base, "--ld-score", "--ld-score-kb", kb), "--ld-score-kb %s: the window must be a finite number of kilobases >= 0" % kb)


@pytest.mark.parametrize("w", ["0", "-3", "4097", "2.5", "many"])
def test_snps_window_out_of_range(base, w):
    refused(run(*base, "--ld-score", "--ld-score-snps", w), "--ld-score-snps %s: the window must be an integer from 1 to 4096 markers" % w)


def test_groups_need_a_group_file(base):
    refused(run(*base, "--ld-score", "--ld-score-groups"), "--ld-score-groups needs --groupIndexFile")


def test_chromosomes_not_contiguous(tmp_path):
    cmd = command(tmp_path, chroms="111122221133")
    refused(run(*cmd, "--ld-score"), "chromosome 1 comes back at marker snp8 (row 9) after another chromosome: --ld-score needs every chromosome "
                                      "as one contiguous run")
    refused(run(*cmd, "--ld-score", "--ld-score-snps", "3"), "chromosome 1 comes back at marker snp8 (row 9)")


def test_bp_decreases_inside_a_run(tmp_path):
    bps = [100 * j + 1 for j in range(M)]
    bps[9] = bps[8] - 5  # inside chromosome 2's run
    cmd = command(tmp_path, bps=bps)
    refused(run(*cmd, "--ld-score", "--ld-score-kb", "1"), "bp decreases at marker snp9 (row 10) inside chromosome 2")
    # a marker window is an index interval whatever the bp: this one gets past the checks (to the device, or through on a GPU)
    r = run(*cmd, "--ld-score", "--ld-score-snps", "3")
    assert "bp decreases" not in r.stderr and "LDSCORE: 12 markers" in r.stdout
    # bp may step back where the chromosome changes
    bps = [100 * j + 1 for j in range(7)] + [100 * j + 1 for j in range(5)]
    r = run(*command(tmp_path, bps=bps), "--ld-score")
    assert "bp decreases" not in r.stderr and "LDSCORE: 12 markers" in r.stdout


def test_window_wider_than_4096_markers(tmp_path):
    m = 4100
    cmd = command(tmp_path, chroms="1" * m, bps=[j + 1 for j in range(m)], m=m)
    # the default window of 1000 kb holds every marker: snp0 has 4099 ahead; snp2 is the last that is too wide
    refused(run(*cmd, "--ld-score"), "marker snp0 (row 1) has 4099 markers ahead of it in its window, at most 4096")
    refused(run(*cmd, "--ld-score", "--ld-score-kb", "4.097"), "marker snp0 (row 1) has 4097 markers ahead of it in its window, at most 4096")
    r = run(*cmd, "--ld-score", "--ld-score-kb", "4.096")
    assert "markers ahead of it in its window" not in r.stderr and "widest window 4096 markers ahead" in r.stdout


def test_too_many_annotations(base, tmp_path):
    sets = str(tmp_path / "s.txt")
    with open(sets, "w") as f:
        for s in range(64):
            f.write("set%d snp%d\n" % (s, s % M))
    refused(run(*base, "--ld-score", "--ld-score-sets", sets), "64 annotations, at most 63 beside the base column")


def test_sets_file_is_read_as_pve_reads_it(base, tmp_path):
    sets = str(tmp_path / "s.txt")
    with open(sets, "w") as f:
        f.write("a snp1\na snp99\n")
    refused(run(*base, "--ld-score", "--ld-score-sets", sets), "line 2: SNP snp99 is not among the first 12 markers of")
    refused(run(*base, "--ld-score", "--ld-score-sets", str(tmp_path / "none.txt")), "can not open the file")


def test_valid_command_line_reaches_the_device(base, tmp_path):
    """Every option check passes and the report comes before the device; on a machine without a GPU the first device call refuses"""
    if has_gpu():
        pytest.skip("a GPU is present")
    # chromosomes of 7 and 5 markers, bp 100 apart, window 0.25 kb: two markers ahead except at the runs' ends: 5 x 2 + 1 and 3 x 2 + 1
    r = run(*base, "--ld-score", "--ld-score-kb", "0.25", "--ld-score-raw")
    assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    assert ("LDSCORE: 12 markers, 2 chromosomes, window 250 bp, 18 pairs in the window, widest window 2 markers ahead, 1 columns (raw r^2)"
            in r.stdout), r.stdout
    sets = str(tmp_path / "s.txt")
    with open(sets, "w") as f:
        f.write("a snp1\nb snp2\na snp3\n")
    # a window of 3 markers: 4 x 3 + 3 + 2 + 1 and 2 x 3 + 3 + 2 + 1... = (3+3+3+3+2+1+0) + (3+3+2+1+0)
    r = run(*base, "--ld-score", "--ld-score-snps", "3", "--ld-score-sets", sets, "--ld-score-out", str(tmp_path / "p"))
    assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    assert ("LDSCORE: 12 markers, 2 chromosomes, window 3 markers, 24 pairs in the window, widest window 3 markers ahead, 3 columns (adjusted r^2) -> %s"
            % str(tmp_path / "p.l2.ldscore")) in r.stdout, r.stdout
