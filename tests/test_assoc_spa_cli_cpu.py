"""hydra_mi355x --assoc --assoc-logistic --assoc-spa, the part that runs before any device is touched: the new refusals, and that a
valid command line reaches the device.  No GPU needed."""
import pytest

from test_assoc_logistic_cli_cpu import LOGISTIC, N, case_control, has_gpu, refused, run, write_cohort


@pytest.mark.parametrize("flags", [["--assoc-spa"], ["--assoc-spa-sd", "3"], ["--assoc-spa", "--assoc-spa-sd", "3"]])
def test_spa_needs_the_logistic_test(tmp_path, flags):
    base = write_cohort(tmp_path, case_control())
    refused(run(*base, "--assoc", "--assoc-no-loco", *flags), flags[0] + " needs --assoc-logistic")
    refused(run(*base, *flags), flags[0] + " needs --assoc")


def test_the_threshold_needs_the_flag(tmp_path):
    refused(run(*write_cohort(tmp_path, case_control()), *LOGISTIC, "--assoc-spa-sd", "3"), "--assoc-spa-sd needs --assoc-spa")


@pytest.mark.parametrize("t", ["0.05", "0", "-2", "nan", "inf", "2x", ""])
def test_threshold_must_be_a_finite_number_from_a_tenth(tmp_path, t):
    refused(run(*write_cohort(tmp_path, case_control()), *LOGISTIC, "--assoc-spa", "--assoc-spa-sd", t),
            "--assoc-spa-sd %s: the threshold must be a finite number of standard deviations >= 0.1" % t)


def test_valid_command_line_reaches_the_device(tmp_path):
    base = write_cohort(tmp_path, case_control())
    out = str(tmp_path / "t.logistic")
    for flags in (["--assoc-spa"], ["--assoc-spa", "--assoc-spa-sd", "0.1"]):
        r = run(*base, *LOGISTIC, *flags, "--assoc-out", out)
        assert "ASSOC  : 12 markers, 3 chromosomes in 4 runs, 0 covariates, %d individuals -> %s" % (N - 1, out) in r.stdout, r.stdout
        if has_gpu():
            assert r.returncode == 0 and "wrote 12 rows" in r.stdout, r.stderr
            assert "ASSOC  : SPA on " in r.stdout and "(|z| > %s): " % ("2" if len(flags) == 1 else "0.1") in r.stdout
            assert open(out).readline().split()[-6:] == ["N_CASE", "N_CTRL", "FREQ_CASE", "FREQ_CTRL", "P_NORM", "SPA"]
        else:
            assert r.returncode != 0 and "hgibbs_create" in r.stderr, r.stderr
