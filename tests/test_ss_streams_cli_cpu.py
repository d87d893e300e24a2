"""hydra_mi355x --sumstats-streams, the part that runs before any device is touched: the option without
--sumstats, and values that are no whole number from 1 to 1024.  No GPU needed."""
import pytest

from test_ss_cli_cpu import M, command, refused, row, run, table


@pytest.fixture()
def base(tmp_path):
    return command(tmp_path)


@pytest.fixture()
def good(tmp_path):
    return table(tmp_path, [row(j) for j in range(M)])


def test_needs_the_mode(base):
    refused(run(*base, "--sumstats-streams", "8"), "--sumstats-streams needs --sumstats")


@pytest.mark.parametrize("s", ["0", "1025", "2.5", "x"])
def test_streams_out_of_range(base, good, s):
    refused(run(*base, "--sumstats", good, "--sumstats-streams", s),
            "--sumstats-streams %s: the number of streams must be an integer from 1 to 1024 (the most hgibbs_ss_sweep_streams takes)" % s)
