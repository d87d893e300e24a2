"""hydra_mi355x --assoc --assoc-logistic --assoc-sets, the part that runs before any device is touched: every refusal with its message
and its place in the order, an id the .bim lacks counted and reported, and that a valid command line reaches the device.  No GPU
needed."""
import numpy as np
import pytest

from hydra_amd import synth

from test_assoc_logistic_cli_cpu import LOGISTIC, N, case_control, has_gpu, refused, run, write_cohort

# write_cohort's .bim: chromosomes 1 1 1 1 2 2 2 2 1 1 3 3, so snp0 .. snp3 and snp8, snp9 are two runs of chromosome 1


def sets_file(tmp_path, lines, name="sets.txt"):
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write("".join(line + "\n" for line in lines))
    return path


GOOD = ["A snp0", "A snp2", "B snp5", "C snp10", "C snp11"]


@pytest.mark.parametrize("flags", [["--assoc-set-beta", "1", "1"], ["--assoc-set-maf", "0.1"], ["--assoc-set-out", "t"]])
def test_set_options_need_the_sets(tmp_path, flags):
    base = write_cohort(tmp_path, case_control())
    refused(run(*base, *LOGISTIC, *flags), flags[0] + " needs --assoc-sets")
    refused(run(*base, *flags), flags[0] + " needs --assoc")


def test_sets_need_assoc_and_the_logistic_test(tmp_path):
    base = write_cohort(tmp_path, case_control())
    sets = sets_file(tmp_path, GOOD)
    refused(run(*base, "--assoc-sets", sets), "--assoc-sets needs --assoc")
    refused(run(*base, "--assoc", "--assoc-no-loco", "--assoc-sets", sets), "--assoc-sets needs --assoc-logistic")
    # the options' own dependency is looked at first
    refused(run(*base, "--assoc", "--assoc-no-loco", "--assoc-set-maf", "0.1"), "--assoc-set-maf needs --assoc-sets")


def test_the_readers_own_messages(tmp_path):
    base = write_cohort(tmp_path, case_control())
    missing = str(tmp_path / "nowhere.txt")
    refused(run(*base, *LOGISTIC, "--assoc-sets", missing), "can not open the file [%s] to read." % missing)
    three = sets_file(tmp_path, ["A snp0", "A snp1 extra"])
    refused(run(*base, *LOGISTIC, "--assoc-sets", three), three + " line 2: expected SETNAME SNPID")
    twice = sets_file(tmp_path, ["A snp0", "B snp1", "A snp0"], "twice.txt")
    refused(run(*base, *LOGISTIC, "--assoc-sets", twice), twice + " line 3: SNP snp0 is given twice for set A")
    empty = sets_file(tmp_path, [], "empty.txt")
    refused(run(*base, *LOGISTIC, "--assoc-sets", empty), empty + " names no set")


@pytest.mark.parametrize("a,b", [("0", "1"), ("1", "-2"), ("nan", "1"), ("1", "inf"), ("1", "25x")])
def test_beta_parameters_must_be_positive(tmp_path, a, b):
    base = write_cohort(tmp_path, case_control())
    refused(run(*base, *LOGISTIC, "--assoc-sets", sets_file(tmp_path, GOOD), "--assoc-set-beta", a, b),
            "--assoc-set-beta %s %s: both parameters of the weights' beta density must be finite numbers > 0" % (a, b))


@pytest.mark.parametrize("x", ["0", "0.6", "-0.1", "nan", "0.1x"])
def test_maf_bound_must_lie_in_the_half_open_interval(tmp_path, x):
    base = write_cohort(tmp_path, case_control())
    refused(run(*base, *LOGISTIC, "--assoc-sets", sets_file(tmp_path, GOOD), "--assoc-set-maf", x),
            "--assoc-set-maf %s: the bound on the minor allele frequency must be a finite number in (0, 0.5]" % x)


def test_a_set_on_two_runs_is_named(tmp_path):
    base = write_cohort(tmp_path, case_control())
    sets = sets_file(tmp_path, ["A snp0", "A snp1", "G snp2", "G snp8"])  # two runs of the same chromosome: two null models all the same
    refused(run(*base, *LOGISTIC, "--assoc-sets", sets), "--assoc-sets: set G has markers on more than one chromosome run (snp2 on 1, snp8 on 1)")
    sets = sets_file(tmp_path, ["A snp0", "H snp5", "H snp11"], "h.txt")
    refused(run(*base, *LOGISTIC, "--assoc-sets", sets), "--assoc-sets: set H has markers on more than one chromosome run (snp5 on 2, snp11 on 3)")


def big_cohort(tmp_path, M=1100):
    """one chromosome of M markers"""
    geno = synth.make_genotypes(M, N, seed=2)
    prefix = str(tmp_path / "big")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=case_control())
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("1 snp%d 0 %d A C\n" % (j, 10 * j + 1))
    return ["--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"),
            "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(M)]


def test_a_set_of_more_than_1024_markers_is_named(tmp_path):
    base = big_cohort(tmp_path)
    sets = sets_file(tmp_path, ["small snp3"] + ["huge snp%d" % j for j in range(1025)])
    refused(run(*base, *LOGISTIC, "--assoc-sets", sets), "--assoc-sets: set huge has 1025 markers, hgibbs_set_gram takes at most 1024 a set")
    # 1024 ids found and five that the .bim lacks: taken (a bound that leaves no marker in keeps the run short where there is a device)
    sets = sets_file(tmp_path, ["full snp%d" % j for j in range(1024)] + ["full rs%d" % j for j in range(5)], "full.txt")
    r = run(*base, *LOGISTIC, "--assoc-sets", sets, "--assoc-set-maf", "1e-9")
    assert "ASSOC  : 1 sets of 1024 markers from %s (5 ids are not in the .bim)" % sets in r.stdout, r.stdout + r.stderr


def test_no_id_of_the_file_in_the_bim(tmp_path):
    base = write_cohort(tmp_path, case_control())
    sets = sets_file(tmp_path, ["A rs1", "A rs2", "B rs3"])
    refused(run(*base, *LOGISTIC, "--assoc-sets", sets), "--assoc-sets: none of the 3 ids of %s is among the first 12 markers" % sets)


def test_order_of_the_refusals(tmp_path):
    base = write_cohort(tmp_path, case_control())
    good = sets_file(tmp_path, GOOD)
    nowhere = str(tmp_path / "nowhere.txt")
    tworuns = sets_file(tmp_path, ["G snp2", "G snp8"], "g.txt")
    none = sets_file(tmp_path, ["A rs1"], "none.txt")
    # section 25's come first: the phenotype, before the file is opened
    (tmp_path / "three").mkdir()
    three = write_cohort(tmp_path / "three", np.arange(N) % 3)
    refused(run(*three, *LOGISTIC, "--assoc-sets", nowhere), "the phenotype takes 3 distinct values")
    refused(run(*base, *LOGISTIC, "--assoc-sets", nowhere, "--assoc-firth", "--assoc-spa"), "choose one correction")
    # then the file, the weights' parameters, the bound, the runs, the ids
    refused(run(*base, *LOGISTIC, "--assoc-sets", nowhere, "--assoc-set-beta", "0", "1"), "can not open the file")
    refused(run(*base, *LOGISTIC, "--assoc-sets", good, "--assoc-set-beta", "0", "1", "--assoc-set-maf", "0.7"), "--assoc-set-beta 0 1")
    refused(run(*base, *LOGISTIC, "--assoc-sets", tworuns, "--assoc-set-maf", "0.7"), "--assoc-set-maf 0.7")
    refused(run(*base, *LOGISTIC, "--assoc-sets", none, "--assoc-set-maf", "0.7"), "--assoc-set-maf 0.7")
    big = big_cohort(tmp_path)
    both = sets_file(tmp_path, ["huge snp%d" % j for j in range(1025)] + ["G snp1", "G rs1"], "both.txt")
    refused(run(*big, *LOGISTIC, "--assoc-sets", both), "set huge has 1025 markers")


@pytest.mark.parametrize("extra", [[], ["--assoc-spa"], ["--assoc-firth"], ["--assoc-set-beta", "1", "1", "--assoc-set-maf", "0.5"]])
def test_valid_command_line_reports_and_reaches_the_device(tmp_path, extra):
    base = write_cohort(tmp_path, case_control())
    sets = sets_file(tmp_path, GOOD + ["B rs77", "D rs78"])  # ids the .bim lacks: counted and reported, not refused
    out = str(tmp_path / "t.sets")
    r = run(*base, *LOGISTIC, "--assoc-sets", sets, "--assoc-set-out", out, *extra)
    a, b = ("1", "1") if "--assoc-set-beta" in extra else ("1", "25")
    assert "ASSOC  : 4 sets of 5 markers from %s (2 ids are not in the .bim), weights dbeta(MAF; %s, %s), MAF <= 0.5 -> %s" % (sets, a, b, out) in r.stdout, r.stdout
    if has_gpu():
        assert r.returncode == 0 and "wrote 12 rows" in r.stdout and ", 4 sets to %s (" % out in r.stdout, r.stderr
        lines = open(out).read().splitlines()
        assert lines[0].split("\t") == ["SET", "CHR", "BP_FIRST", "BP_LAST", "NSNP", "NUSED", "NEIG", "Q", "P_SKAT", "SKAT_OK", "T_BURDEN", "P_BURDEN"]
        assert [x.split("\t")[0] for x in lines[1:]] == ["A", "B", "C", "D"] and lines[4].split("\t")[1:6] == ["NA", "NA", "NA", "0", "0"]
    else:
        assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
    r = run(*base, *LOGISTIC, "--assoc-sets", sets)  # the default name
    assert "-> %s" % str(tmp_path / "o" / "n.assoc.sets") in r.stdout, r.stdout
