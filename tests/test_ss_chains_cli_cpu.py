"""hydra_mi355x --sumstats-chains, the part that runs before any device is touched: the option without
--sumstats, values that are no whole number from 1 to 64, and that it is accepted next to --sumstats-streams.  No GPU needed."""
import pytest

from test_ss_cli_cpu import M, command, has_gpu, refused, row, run, table


@pytest.fixture()
def base(tmp_path):
    return command(tmp_path)


@pytest.fixture()
def good(tmp_path):
    return table(tmp_path, [row(j) for j in range(M)])


def test_needs_the_mode(base):
    refused(run(*base, "--sumstats-chains", "3"), "--sumstats-chains needs --sumstats")


@pytest.mark.parametrize("r", ["0", "65", "2.5", "x"])
def test_chains_out_of_range(base, good, r):
    refused(run(*base, "--sumstats", good, "--sumstats-chains", r),
            "--sumstats-chains %s: the number of chains must be an integer from 1 to 64 (the most hgibbs_ss_replicas takes)" % r)


def test_accepted_next_to_streams(base, good):
    # past every refusal of the command line: the table is read and reported, then the device is asked for
    r = run(*base, "--sumstats", good, "--sumstats-chains", "3", "--sumstats-streams", "4")
    assert "--sumstats-chains" not in r.stderr and "--sumstats-streams" not in r.stderr, r.stderr
    assert "SUMSTAT: %d rows read from" % M in r.stdout, (r.stdout, r.stderr)
    if not has_gpu():
        assert r.returncode != 0
