"""hydra_mi355x --clump and --ld-prune, the part that runs before any device is touched: every refusal of both modes, through the table
of the modes and through their own arguments, the refusals of the table FILE, and that a valid command line prints its first report
line with the right counts and reaches the device.  No GPU needed."""
import ctypes
import os
import subprocess

import pytest

from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 30, 12
MODES = {"--clump": ["--clump", "FILE"], "--ld-prune": ["--ld-prune", "0.5"]}
EARLIER = [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"], ["--pve"], ["--grm"], ["--ld-score"]]


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


def table(tmp_path, rows, header="SNP P", name="t.assoc"):
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(header + "\n")
        for r in rows:
            f.write(r + "\n")
    return path


@pytest.fixture()
def base(tmp_path):
    return command(tmp_path)


def mode_args(mode, tmp_path):
    if mode == "--clump":
        return ["--clump", table(tmp_path, ["snp1 1e-6", "snp2 0.001"])]
    return MODES[mode]


def refused(r, msg):
    assert r.returncode != 0, r.stdout
    assert msg in r.stderr, r.stderr
    assert "invalid option" not in r.stderr and "hgibbs_create" not in r.stderr


# ---- through the table of the modes ----
@pytest.mark.parametrize("mode", sorted(MODES))
def test_refused_with_bayesw(base, tmp_path, mode):
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], *mode_args(mode, tmp_path)),
            "%s takes a bayesMPI command line, not --mpibayes bayesWMPI" % mode)


@pytest.mark.parametrize("earlier", EARLIER)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_refused_with_an_earlier_mode(base, tmp_path, mode, earlier):
    refused(run(*base, *mode_args(mode, tmp_path), *earlier), "%s cannot be combined with %s" % (mode, earlier[0]))


def test_prune_refused_with_clump(base, tmp_path):
    refused(run(*base, "--ld-prune", "0.5", *mode_args("--clump", tmp_path)), "--ld-prune cannot be combined with --clump")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_refused_with_restart(base, tmp_path, mode):
    refused(run(*base, "--restart", *mode_args(mode, tmp_path)), "%s does not sample: it cannot be combined with --restart" % mode)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_refused_with_several_ranks(base, tmp_path, mode):
    refused(run(*base, *mode_args(mode, tmp_path), env={"WORLD_SIZE": "2", "RANK": "0"}), "%s runs on one process (WORLD_SIZE = 2)" % mode)


@pytest.mark.parametrize("extra", [["--clump-p1", "0.1"], ["--clump-p2", "0.1"], ["--clump-r2", "0.1"], ["--clump-kb", "100"], ["--clump-snps", "5"],
                                   ["--clump-snp-field", "ID"], ["--clump-field", "PVAL"], ["--clump-out", "p"]])
def test_dependent_options_need_clump(base, extra):
    refused(run(*base, *extra), "%s needs --clump" % extra[0])


@pytest.mark.parametrize("extra", [["--ld-prune-kb", "100"], ["--ld-prune-snps", "5"], ["--ld-prune-out", "p"]])
def test_dependent_options_need_ld_prune(base, extra):
    refused(run(*base, *extra), "%s needs --ld-prune" % extra[0])


# ---- their own arguments ----
@pytest.mark.parametrize("bad", ["-0.1", "1.5", "abc", "nan", "0.5x", "inf"])
@pytest.mark.parametrize("flag", ["--clump-p1", "--clump-p2", "--clump-r2"])
def test_clump_thresholds(base, tmp_path, flag, bad):
    refused(run(*base, *mode_args("--clump", tmp_path), flag, bad), "%s %s: " % (flag, bad))
    refused(run(*base, *mode_args("--clump", tmp_path), flag, bad), "must be a number in [0, 1]")


@pytest.mark.parametrize("bad", ["-0.1", "1.5", "abc", "nan", "0.5x", "inf"])
def test_prune_threshold(base, bad):
    refused(run(*base, "--ld-prune", bad), "--ld-prune %s: the threshold on r^2 must be a number in [0, 1]" % bad)


def test_p2_below_p1(base, tmp_path):
    refused(run(*base, *mode_args("--clump", tmp_path), "--clump-p1", "0.01", "--clump-p2", "0.001"), "is below --clump-p1")
    refused(run(*base, *mode_args("--clump", tmp_path), "--clump-p1", "0.05"), "is below --clump-p1")  # the default P2 = 0.01
    refused(run(*base, *mode_args("--clump", tmp_path), "--clump-p2", "0.00001"), "is below --clump-p1")  # the default P1 = 0.0001


@pytest.mark.parametrize("mode", sorted(MODES))
def test_both_windows(base, tmp_path, mode):
    refused(run(*base, *mode_args(mode, tmp_path), mode + "-kb", "100", mode + "-snps", "5"),
            "%s-kb cannot be combined with %s-snps: one way to define the window" % (mode, mode))


@pytest.mark.parametrize("kb", ["-1", "abc", "nan", "12x"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_kb_negative_or_not_a_number(base, tmp_path, mode, kb):
    refused(run(*base, *mode_args(mode, tmp_path), mode + "-kb", kb), "%s-kb %s: the window must be a finite number of kilobases >= 0" % (mode, kb))


@pytest.mark.parametrize("w", ["0", "-3", "4097", "2.5", "many"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_snps_window_out_of_range(base, tmp_path, mode, w):
    refused(run(*base, *mode_args(mode, tmp_path), mode + "-snps", w), "%s-snps %s: the window must be an integer from 1 to 4096 markers" % (mode, w))


# ---- the window, shared with --ld-score ----
@pytest.mark.parametrize("mode", sorted(MODES))
def test_chromosomes_not_contiguous(tmp_path, mode):
    cmd = command(tmp_path, chroms="111122221133")
    refused(run(*cmd, *mode_args(mode, tmp_path)), "chromosome 1 comes back at marker snp8 (row 9) after another chromosome: %s needs every chromosome "
                                                   "as one contiguous run" % mode)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_bp_decreases_inside_a_run(tmp_path, mode):
    bps = [100 * j + 1 for j in range(M)]
    bps[9] = bps[8] - 5
    cmd = command(tmp_path, bps=bps)
    refused(run(*cmd, *mode_args(mode, tmp_path), mode + "-kb", "1"), "bp decreases at marker snp9 (row 10) inside chromosome 2")
    refused(run(*cmd, *mode_args(mode, tmp_path), mode + "-kb", "1"), "%s-snps takes any order" % mode)
    r = run(*cmd, *mode_args(mode, tmp_path), mode + "-snps", "3")
    assert "bp decreases" not in r.stderr and "window 3 markers" in r.stdout


def test_window_wider_than_4096_markers(tmp_path):
    m = 4100
    cmd = command(tmp_path, chroms="1" * m, bps=[j + 1 for j in range(m)], m=m)
    refused(run(*cmd, "--ld-prune", "0.5", "--ld-prune-kb", "4.097"),
            "marker snp0 (row 1) has 4097 markers ahead of it in its window, at most 4096 (the widest hgibbs_ld_mask takes)")
    r = run(*cmd, "--ld-prune", "0.5", "--ld-prune-kb", "4.096")
    assert "markers ahead of it in its window" not in r.stderr and "widest window 4096 markers ahead" in r.stdout


# ---- FILE ----
def test_file_unreadable(base, tmp_path):
    refused(run(*base, "--clump", str(tmp_path / "none.assoc")), "--clump: can not open the file [%s] to read." % str(tmp_path / "none.assoc"))


def test_file_missing_field(base, tmp_path):
    refused(run(*base, "--clump", table(tmp_path, ["snp1 0.1"], header="ID P")), "has no column SNP in its header line")
    refused(run(*base, "--clump", table(tmp_path, ["snp1 0.1"], header="SNP PVAL")), "has no column P in its header line")
    refused(run(*base, "--clump", table(tmp_path, ["snp1 0.1"], header="SNP P"), "--clump-field", "PVAL"), "has no column PVAL in its header line")
    refused(run(*base, "--clump", table(tmp_path, ["snp1 0.1"], header="SNP P"), "--clump-snp-field", "ID"), "has no column ID in its header line")
    refused(run(*base, "--clump", table(tmp_path, [], header="")), "has no")


def test_file_duplicate_id(base, tmp_path):
    refused(run(*base, "--clump", table(tmp_path, ["snp1 0.1", "snp2 0.2", "snp1 0.3"])), "line 4: SNP id snp1 was already on line 2")
    refused(run(*base, "--clump", table(tmp_path, ["other 0.1", "other 0.3"])), "line 3: SNP id other was already on line 2")


def test_file_short_row(base, tmp_path):
    refused(run(*base, "--clump", table(tmp_path, ["snp1 0.1", "snp2"])), "line 3 has 1 columns")


# ---- a valid command line ----
def reaches_the_device(r):
    """on a machine without a GPU the first device call refuses; with one the run goes through"""
    if has_gpu():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr


def test_valid_clump_reaches_the_device(base, tmp_path):
    rows = ["1 snp0 1e-7", "1 snp1 NA", "1 snp2 0.005", "1 snp3 0.2", "1 snp4 0.01", "1 ghost 0.001", "1 snp5 0.0001", "2 snp7 1.5", "2 snp8 -1", "2 snp9 0",
            "2 snp10 abc", "", "2 snp11 0.00011"]
    path = table(tmp_path, rows, header="CHR SNP P")
    # 12 rows, 11 ids of the .bim, one unknown; NA, 1.5, -1 and abc are no P; P <= 0.01: snp0, 2, 4, 5, 9, 11; P <= 1e-4: snp0, 5, 9
    # chromosomes of 7 and 5 markers, bp 100 apart, window 0.25 kb: two markers ahead except at the runs' ends: 5 x 2 + 1 and 3 x 2 + 1
    r = run(*base, "--clump", path, "--clump-kb", "0.25")
    reaches_the_device(r)
    assert ("CLUMP  : 12 rows read from %s, 11 matched to the .bim (1 ids not in it, 4 without a P in [0, 1]), 6 participating (P <= 0.01), 3 able to lead "
            "(P <= 0.0001), window 250 bp, 18 pairs in the window, widest window 2 markers ahead, r^2 >= 0.5 -> %s"
            % (path, str(tmp_path / "o" / "n.clumped"))) in r.stdout, r.stdout
    # named fields, a marker window (24 pairs as in tests/test_ldscore_cli_cpu.py), other thresholds, an output of its own
    path = table(tmp_path, rows, header="CHR ID PVAL", name="u.txt")
    r = run(*base, "--clump", path, "--clump-snps", "3", "--clump-snp-field", "ID", "--clump-field", "PVAL", "--clump-p1", "0.001", "--clump-p2", "0.2",
            "--clump-r2", "0.25", "--clump-out", str(tmp_path / "c.txt"))
    reaches_the_device(r)
    assert ("CLUMP  : 12 rows read from %s, 11 matched to the .bim (1 ids not in it, 4 without a P in [0, 1]), 7 participating (P <= 0.2), 4 able to lead "
            "(P <= 0.001), window 3 markers, 24 pairs in the window, widest window 3 markers ahead, r^2 >= 0.25 -> %s"
            % (path, str(tmp_path / "c.txt"))) in r.stdout, r.stdout


def test_valid_prune_reaches_the_device(base, tmp_path):
    # the default window of 50 markers holds each chromosome whole: 7 x 6 / 2 + 5 x 4 / 2 pairs
    r = run(*base, "--ld-prune", "0.2")
    reaches_the_device(r)
    assert ("PRUNE  : 12 markers, 2 chromosomes, window 50 markers, 31 pairs in the window, widest window 6 markers ahead, r^2 > 0.2 -> %s"
            % str(tmp_path / "o" / "n.prune.in")) in r.stdout, r.stdout
    r = run(*base, "--ld-prune", "0.2", "--ld-prune-kb", "0.25", "--ld-prune-out", str(tmp_path / "p"))
    reaches_the_device(r)
    assert ("PRUNE  : 12 markers, 2 chromosomes, window 250 bp, 18 pairs in the window, widest window 2 markers ahead, r^2 > 0.2 -> %s"
            % str(tmp_path / "p.prune.in")) in r.stdout, r.stdout
