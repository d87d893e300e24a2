"""hydra_mi355x --sumstats-cs and --cs, the part that runs before any device is touched: every refusal of both routes by its sentence,
through the table of the modes, through the option checks of --sumstats, and through the routes' own arguments.  No GPU needed."""
import os
import subprocess

import pytest

from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 30, 12
EARLIER = [["--predict-bfile", "t"], ["--ld-window", "5"], ["--assoc"], ["--king"], ["--pca", "2"], ["--pve"], ["--grm"], ["--ld-score"], ["--clump", "F"],
           ["--ld-prune", "0.5"], ["--he"], ["--qc"], ["--homozyg"], ["--epistasis"]]
# the sub-options the two routes share: (suffix, what the refusal calls it)
UNIT = [("-r2", "the threshold on r^2"), ("-alpha", "the sum of PIPs a set must reach"), ("-pep", "the posterior existence probability a set must have"),
        ("-lead", "the PIP a marker needs to lead a set")]
ROUTES = {"--cs": ["--cs"], "--sumstats-cs": ["--sumstats", "FILE", "--sumstats-cs"]}


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
    return ["--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"), "--mcmc-out-name", "n",
            "--number-individuals", str(N), "--number-markers", str(M), "--chain-length", "10", "--burn-in", "2", "--thin", "1"]


def refused(r, msg):
    assert r.returncode != 0, r.stdout
    assert msg in r.stderr, r.stderr
    assert "invalid option" not in r.stderr and "hgibbs_create" not in r.stderr


# ---- --cs through the table of the modes ----
def test_cs_refused_with_bayesw(base):
    refused(run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--cs"), "--cs takes a bayesMPI command line, not --mpibayes bayesWMPI")


@pytest.mark.parametrize("earlier", EARLIER)
def test_cs_refused_with_an_earlier_mode(base, earlier):
    refused(run(*base, "--cs", *earlier), "--cs cannot be combined with %s" % earlier[0])


def test_cs_refused_with_restart(base):
    refused(run(*base, "--restart", "--cs"), "--cs does not sample: it cannot be combined with --restart")


def test_cs_refused_with_several_ranks(base):
    refused(run(*base, "--cs", env={"WORLD_SIZE": "2", "RANK": "0"}), "--cs runs on one process (WORLD_SIZE = 2)")


def test_cs_refused_with_sumstats(base):
    refused(run(*base, "--cs", "--sumstats", "FILE"), "--sumstats cannot be combined with --cs: it samples a chain, the analysis modes sample nothing")


@pytest.mark.parametrize("extra", [["--cs-chains", "2"], ["--cs-window-kb", "100"], ["--cs-window-snps", "5"], ["--cs-r2", "0.1"], ["--cs-alpha", "0.5"],
                                   ["--cs-pep", "0.5"], ["--cs-lead", "0.1"], ["--cs-max-size", "5"], ["--cs-out", "p"]])
def test_dependent_options_need_cs(base, extra):
    refused(run(*base, *extra), "%s needs --cs" % extra[0])


# ---- --sumstats-cs through the option checks of --sumstats ----
def test_sumstats_cs_needs_sumstats(base):
    refused(run(*base, "--sumstats-cs"), "--sumstats-cs needs --sumstats")


@pytest.mark.parametrize("extra", [["--sumstats-cs-r2", "0.1"], ["--sumstats-cs-alpha", "0.5"], ["--sumstats-cs-pep", "0.5"], ["--sumstats-cs-lead", "0.1"],
                                   ["--sumstats-cs-max-size", "5"], ["--sumstats-cs-out", "p"]])
@pytest.mark.parametrize("sumstats", [[], ["--sumstats", "FILE"]], ids=["alone", "with --sumstats"])
def test_dependent_options_need_sumstats_cs(base, sumstats, extra):
    refused(run(*base, *sumstats, *extra), "%s needs --sumstats-cs" % extra[0])


# ---- the values, the same under both names ----
@pytest.mark.parametrize("bad", ["0", "-0.1", "1.5", "x", "0.5x", "nan"])
@pytest.mark.parametrize("suffix,what", UNIT)
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_unit_values(base, route, suffix, what, bad):
    refused(run(*base, *ROUTES[route], route + suffix, bad), "%s%s %s: %s must be a number in (0, 1]" % (route, suffix, bad, what))


@pytest.mark.parametrize("bad", ["0", "257", "-1", "3.5", "k"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_max_size(base, route, bad):
    refused(run(*base, *ROUTES[route], route + "-max-size", bad),
            "%s-max-size %s: the largest set must be an integer from 1 to 256 markers (the most hgibbs_cs_sets takes)" % (route, bad))


@pytest.mark.parametrize("plan", [["--burn-in", "10"], ["--burn-in", "50"], ["--chain-length", "9", "--burn-in", "7", "--thin", "5"]])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_a_plan_of_zero_records(base, route, plan):
    r = run(*base, *ROUTES[route], *plan)
    refused(r, "%s: 0 records per chain (--chain-length " % route)
    assert "the history needs a thinned iteration at or after the burn-in" in r.stderr


def test_the_plan_counts_thinned_iterations_whatever_post_all_says(base):
    # iterations 7 to 11 are at or after the burn-in, none is a multiple of --thin 6: --sumstats-post-all counts the five, the history none
    refused(run(*base, "--sumstats", "FILE", "--sumstats-post", "--sumstats-post-all", "--sumstats-cs", "--chain-length", "12", "--burn-in", "7", "--thin", "6"),
            "--sumstats-cs: 0 records per chain (--chain-length 12, --burn-in 7, --thin 6)")


# ---- --cs' own arguments ----
@pytest.mark.parametrize("bad", ["0", "65", "-2", "1.5", "r"])
def test_cs_chains(base, bad):
    refused(run(*base, "--cs", "--cs-chains", bad), "--cs-chains %s: the number of chains must be an integer from 1 to 64" % bad)


def test_cs_both_windows(base):
    refused(run(*base, "--cs", "--cs-window-kb", "100", "--cs-window-snps", "5"), "--cs-window-kb cannot be combined with --cs-window-snps: one way to define the window")


@pytest.mark.parametrize("kb", ["-1", "abc", "inf"])
def test_cs_window_kb(base, kb):
    refused(run(*base, "--cs", "--cs-window-kb", kb), "--cs-window-kb %s: the window must be a finite number of kilobases >= 0" % kb)


@pytest.mark.parametrize("w", ["0", "4097", "2.5"])
def test_cs_window_snps(base, w):
    refused(run(*base, "--cs", "--cs-window-snps", w), "--cs-window-snps %s: the window must be an integer from 1 to 4096 markers" % w)


def test_cs_needs_the_chains_effects(base):
    r = run(*base, "--cs")
    refused(r, "n.bet (--cs takes the inclusion history from the chain's effects: run the chain first)")
