"""hydra_mi355x --sumstats, the part that runs before any device is touched: every refusal of the mode (other modes, --covariates,
bayesWMPI, several processes, checkpoint options, its own options without it or out of range, the window) and the parsing of FILE
(sign flip of swapped alleles, NA, other allele pairs, unknown ids, a duplicate id, a missing column), and that a valid command line
prints its report line with the right counts and reaches the device.  No GPU needed."""
import ctypes
import os
import subprocess

import pytest

from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 30, 12
MODES = [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"], ["--pve"], ["--grm"], ["--ld-score"], ["--clump", "f"],
         ["--ld-prune", "0.5"], ["--he"], ["--qc"], ["--homozyg"], ["--epistasis"]]
HEADER = "CHR SNP BP A1 A2 FREQ N BETA SE CHISQ P"


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


def command(tmp_path, chroms="111111122222", bps=None, m=M, pheno=True):
    geno = synth.make_genotypes(m, N, seed=1)
    y, _ = synth.make_phenotype(geno, seed=2)
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=[4])
    with open(prefix + ".bim", "w") as f:
        for j in range(m):
            f.write("%s snp%d 0 %d A C\n" % (chroms[j], j, bps[j] if bps else 100 * j + 1))
    cmd = ["--mpibayes", "bayesMPI", "--bfile", prefix, "--mcmc-out-dir", str(tmp_path / "o"), "--mcmc-out-name", "n", "--number-individuals", str(N),
           "--number-markers", str(m), "--chain-length", "2", "--seed", "5"]
    return cmd + (["--pheno", prefix + ".phen"] if pheno else [])


def row(j, a1="A", a2="C", n="100", beta="0.1", se="0.05", snp=None):
    return "1 %s %d %s %s 0.3 %s %s %s 4 0.04" % (snp or "snp%d" % j, 100 * j + 1, a1, a2, n, beta, se)


def table(tmp_path, rows, header=HEADER, name="t.assoc"):
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(header + "\n")
        for r in rows:
            f.write(r + "\n")
    return path


@pytest.fixture()
def base(tmp_path):
    return command(tmp_path)


@pytest.fixture()
def good(tmp_path):
    return table(tmp_path, [row(j) for j in range(M)])


def refused(r, msg):
    assert r.returncode != 0, r.stdout
    assert msg in r.stderr, r.stderr
    assert "invalid option" not in r.stderr and "hgibbs_create" not in r.stderr


# ---- the mode against the rest of the command line ----
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_refused_with_an_analysis_mode(base, good, mode):
    refused(run(*base, "--sumstats", good, *mode), "--sumstats cannot be combined with %s" % mode[0])


def test_refused_with_covariates(base, good):
    refused(run(*base, "--sumstats", good, "--covariates", "c.cov"), "--sumstats cannot be combined with --covariates")


def test_refused_with_bayesw(base, good):
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--sumstats", good), "--sumstats takes a bayesMPI command line, not --mpibayes bayesWMPI")


def test_refused_with_several_processes(base, good):
    refused(run(*base, "--sumstats", good, env={"WORLD_SIZE": "2", "RANK": "0"}), "--sumstats runs on one process (WORLD_SIZE = 2)")


@pytest.mark.parametrize("extra", [["--restart"], ["--save", "4"], ["--ignore-xfiles"]], ids=lambda e: e[0])
def test_refused_with_checkpoint_options(base, good, extra):
    refused(run(*base, "--sumstats", good, *extra), "--sumstats cannot be combined with %s: checkpoint and restart are not built for it" % extra[0])


@pytest.mark.parametrize("extra", [["--sumstats-window", "5"], ["--sumstats-window-kb", "100"], ["--sumstats-n", "1000"]], ids=lambda e: e[0])
def test_its_options_need_the_mode(base, extra):
    refused(run(*base, *extra), "%s needs --sumstats" % extra[0])


def test_needs_bfile(tmp_path, good):
    refused(run("--mpibayes", "bayesMPI", "--sparse-dir", str(tmp_path), "--sparse-basename", "s", "--mcmc-out-dir", str(tmp_path), "--mcmc-out-name", "n",
                "--number-individuals", "5", "--number-markers", "5", "--sumstats", good), "--sumstats needs --bfile")


# ---- its own arguments ----
def test_both_windows(base, good):
    refused(run(*base, "--sumstats", good, "--sumstats-window", "5", "--sumstats-window-kb", "100"),
            "--sumstats-window-kb cannot be combined with --sumstats-window: one way to define the window")


@pytest.mark.parametrize("kb", ["-1", "abc", "nan", "12x"])
def test_kb_negative_or_not_a_number(base, good, kb):
    refused(run(*base, "--sumstats", good, "--sumstats-window-kb", kb), "--sumstats-window-kb %s: the window must be a finite number of kilobases >= 0" % kb)


@pytest.mark.parametrize("w", ["0", "-3", "4097", "2.5", "many"])
def test_marker_window_out_of_range(base, good, w):
    refused(run(*base, "--sumstats", good, "--sumstats-window", w), "--sumstats-window %s: the window must be an integer from 1 to 4096 markers" % w)


@pytest.mark.parametrize("n", ["1", "0", "-5", "abc", "nan", "inf", "100x"])
def test_sample_size_out_of_range(base, good, n):
    refused(run(*base, "--sumstats", good, "--sumstats-n", n), "--sumstats-n %s: the sample size must be a finite number >= 2" % n)


# ---- the window, shared with --ld-score ----
def test_chromosomes_not_contiguous(tmp_path, good):
    refused(run(*command(tmp_path, chroms="111122221133"), "--sumstats", good),
            "chromosome 1 comes back at marker snp8 (row 9) after another chromosome: --sumstats needs every chromosome as one contiguous run")


def test_bp_decreases_inside_a_run(tmp_path, good):
    bps = [100 * j + 1 for j in range(M)]
    bps[9] = bps[8] - 5
    cmd = command(tmp_path, bps=bps)
    refused(run(*cmd, "--sumstats", good), "bp decreases at marker snp9 (row 10) inside chromosome 2")
    refused(run(*cmd, "--sumstats", good), "--sumstats-window takes any order")
    r = run(*cmd, "--sumstats", good, "--sumstats-window", "3")
    assert "bp decreases" not in r.stderr and "window 3 markers" in r.stdout


def test_window_wider_than_4096_markers(tmp_path):
    m = 4100
    cmd = command(tmp_path, chroms="1" * m, bps=[j + 1 for j in range(m)], m=m)
    t = table(tmp_path, [row(0)])
    refused(run(*cmd, "--sumstats", t, "--sumstats-window-kb", "4.097"),
            "marker snp0 (row 1) has 4097 markers ahead of it in its window, at most 4096 (the widest hgibbs_ss_begin takes)")
    r = run(*cmd, "--sumstats", t, "--sumstats-window-kb", "4.096")
    assert "markers ahead of it in its window" not in r.stderr and "widest window 4096 markers ahead" in r.stdout


# ---- FILE ----
def test_file_unreadable(base, tmp_path):
    refused(run(*base, "--sumstats", str(tmp_path / "none")), "--sumstats: can not open the file [%s] to read." % str(tmp_path / "none"))


@pytest.mark.parametrize("col", ["SNP", "A1", "A2", "BETA", "SE", "N"])
def test_file_missing_column(base, tmp_path, col):
    header = " ".join(("X" + h) if h == col else h for h in HEADER.split())
    refused(run(*base, "--sumstats", table(tmp_path, [row(1)], header=header)), "has no column %s in its header line" % col)


def test_file_empty(base, tmp_path):
    path = str(tmp_path / "empty")
    open(path, "w").close()
    refused(run(*base, "--sumstats", path), "has no header line")


def test_file_duplicate_id(base, tmp_path):
    refused(run(*base, "--sumstats", table(tmp_path, [row(1), row(2), row(1)])), "line 4: SNP id snp1 was already on line 2")
    refused(run(*base, "--sumstats", table(tmp_path, [row(0, snp="other"), row(0, snp="other")])), "line 3: SNP id other was already on line 2")


def test_file_short_row(base, tmp_path):
    refused(run(*base, "--sumstats", table(tmp_path, [row(1), "1 snp2 201 A"])), "line 3 has 4 columns")


def test_file_without_a_usable_row(base, tmp_path):
    refused(run(*base, "--sumstats", table(tmp_path, [row(1, beta="NA"), row(0, snp="ghost"), row(2, a1="G")])), "no row of")


# ---- a valid command line ----
def reaches_the_device(r):
    """on a machine without a GPU the first device call refuses; with one the run goes through"""
    if has_gpu():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr


ROWS = [row(0, n="90"), row(1, a1="C", a2="A", n="110"), row(2, beta="NA"), row(3, se="0"), row(4, n="-3"), row(5, a1="G", a2="T"), row(0, snp="ghost"),
        row(6, se="NA"), "", row(7, n="100"), row(8, a1="A", a2="G"), row(9, n="NA"), row(10, n="120"), row(11, se="-0.1")]


def test_valid_reaches_the_device_with_the_counts(base, tmp_path):
    # 13 rows: 12 ids of the .bim, one unknown; 5, 8: another allele pair; 2, 3, 4, 6, 9, 11: NA or a non-positive SE or N;
    # matched 0, 1 (swapped), 7, 10 with N 90, 110, 100, 120: median 105
    # chromosomes of 7 and 5 markers, bp 100 apart, the default 1000 kb holds each whole: 7 x 6 / 2 + 5 x 4 / 2 pairs
    path = table(tmp_path, ROWS)
    r = run(*base, "--sumstats", path)
    reaches_the_device(r)
    assert ("SUMSTAT: 13 rows read from %s, 4 matched to the .bim (1 with swapped alleles, sign flipped), 1 ids not in it, 2 with another allele pair, "
            "6 without usable BETA, SE and N; n_eff 105 (the median N of the matched rows); window 1000000 bp, 31 pairs in the window, "
            "widest window 6 markers ahead" % path) in r.stdout, r.stdout
    # --sumstats-n, a marker window, and no --pheno: every row of the panel is kept
    r = run(*command(tmp_path, pheno=False), "--sumstats", path, "--sumstats-n", "250.5", "--sumstats-window", "3")
    reaches_the_device(r)
    assert "n_eff 250.5 (--sumstats-n); window 3 markers, 24 pairs in the window, widest window 3 markers ahead" in r.stdout, r.stdout
    assert "due to NAs in phenotype file" not in r.stdout
    r = run(*base, "--sumstats", path, "--sumstats-window-kb", "0.25")
    reaches_the_device(r)
    assert "window 250 bp, 18 pairs in the window, widest window 2 markers ahead" in r.stdout and "adjusted to 30 - 1 = 29 due to NAs" in r.stdout, r.stdout
