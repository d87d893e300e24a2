"""hydra_mi355x --assoc --assoc-logistic --assoc-firth, the part that runs before any device is touched: the new refusals, and that a
valid command line reaches the device.  No GPU needed."""
import pytest

from test_assoc_logistic_cli_cpu import LOGISTIC, N, case_control, has_gpu, refused, run, write_cohort


@pytest.mark.parametrize("flags", [["--assoc-firth"], ["--assoc-firth-p", "0.1"], ["--assoc-firth", "--assoc-firth-p", "0.1"]])
def test_firth_needs_the_logistic_test(tmp_path, flags):
    base = write_cohort(tmp_path, case_control())
    refused(run(*base, "--assoc", "--assoc-no-loco", *flags), flags[0] + " needs --assoc-logistic")
    refused(run(*base, *flags), flags[0] + " needs --assoc")


def test_the_threshold_needs_the_flag(tmp_path):
    refused(run(*write_cohort(tmp_path, case_control()), *LOGISTIC, "--assoc-firth-p", "0.1"), "--assoc-firth-p needs --assoc-firth")


@pytest.mark.parametrize("t", ["0", "-0.05", "1.5", "nan", "inf", "0.05x", ""])
def test_threshold_must_be_a_finite_number_in_the_unit_interval(tmp_path, t):
    refused(run(*write_cohort(tmp_path, case_control()), *LOGISTIC, "--assoc-firth", "--assoc-firth-p", t),
            "--assoc-firth-p %s: the threshold must be a finite number in (0, 1]" % t)


@pytest.mark.parametrize("extra", [[], ["--assoc-spa-sd", "3"], ["--assoc-firth-p", "0.1"]])
def test_refused_together_with_the_saddlepoint(tmp_path, extra):
    refused(run(*write_cohort(tmp_path, case_control()), *LOGISTIC, "--assoc-firth", "--assoc-spa", *extra), "choose one correction")


def test_valid_command_line_reaches_the_device(tmp_path):
    base = write_cohort(tmp_path, case_control())
    out = str(tmp_path / "t.logistic")
    for flags in (["--assoc-firth"], ["--assoc-firth", "--assoc-firth-p", "1"]):
        r = run(*base, *LOGISTIC, *flags, "--assoc-out", out)
        assert "ASSOC  : 12 markers, 3 chromosomes in 4 runs, 0 covariates, %d individuals -> %s" % (N - 1, out) in r.stdout, r.stdout
        if has_gpu():
            assert r.returncode == 0 and "wrote 12 rows" in r.stdout, r.stderr
            assert "ASSOC  : Firth on " in r.stdout and "(P <= %s): " % ("0.05" if len(flags) == 1 else "1") in r.stdout
            assert open(out).readline().split()[-8:] == ["N_CASE", "N_CTRL", "FREQ_CASE", "FREQ_CTRL", "P_NORM", "BETA_SCORE", "SE_SCORE", "FIRTH"]
        else:
            assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
