"""hydra_mi355x --sumstats-post, the part that runs before any device is touched: its sub-options without it,
the option without --sumstats, a plan of fewer than four records (with T and the three numbers it follows from), and that it is
accepted alone, with every sub-option, and next to --sumstats-chains and --sumstats-streams.  No GPU needed."""
import pytest

from test_ss_cli_cpu import M, command, has_gpu, refused, row, run, table


@pytest.fixture()
def base(tmp_path):
    return command(tmp_path)


@pytest.fixture()
def good(tmp_path):
    return table(tmp_path, [row(j) for j in range(M)])


def plan(length, burn, thin):
    return ["--chain-length", str(length), "--burn-in", str(burn), "--thin", str(thin)]


def test_needs_the_mode(base):
    refused(run(*base, "--sumstats-post"), "--sumstats-post needs --sumstats")


@pytest.mark.parametrize("sub", [["--sumstats-post-all"], ["--sumstats-post-only"], ["--sumstats-post-out", "f.post"]], ids=lambda s: s[0])
def test_sub_options_need_the_option(base, good, sub):
    refused(run(*base, "--sumstats", good, *plan(12, 2, 1), *sub), sub[0] + " needs --sumstats-post")
    refused(run(*base, *sub), sub[0] + " needs --sumstats-post")


@pytest.mark.parametrize("length,burn,thin,more,T,which", [
    (5, 2, 1, [], 3, "the thinned iterations at or after the burn-in"),
    (12, 2, 4, [], 2, "the thinned iterations at or after the burn-in"),       # iterations 4 and 8
    (12, 9, 4, ["--sumstats-post-all"], 3, "every iteration at or after the burn-in"),
    (4, 9, 1, [], 0, "the thinned iterations at or after the burn-in"),
])
def test_fewer_than_four_records(base, good, length, burn, thin, more, T, which):
    refused(run(*base, "--sumstats", good, "--sumstats-post", *more, *plan(length, burn, thin)),
            "--sumstats-post: T = %d record(s) per chain (--chain-length %d, --burn-in %d, --thin %d, %s): split-R^ of the halved chains needs at least 4"
            % (T, length, burn, thin, which))


@pytest.mark.parametrize("more", [
    [],
    ["--sumstats-post-all", "--sumstats-post-only", "--sumstats-post-out", "f.post"],
    ["--sumstats-chains", "3"],
    ["--sumstats-streams", "4"],
    ["--sumstats-chains", "3", "--sumstats-streams", "4", "--sumstats-post-only"],
], ids=["alone", "sub-options", "chains", "streams", "chains-streams-only"])
def test_accepted(base, good, more):
    # past every refusal of the command line: the table is read and reported, then the device is asked for.  12 iterations, burn-in 2,
    # thin 2: the records 2, 4, 6, 8, 10
    r = run(*base, "--sumstats", good, "--sumstats-post", *more, *plan(12, 2, 1 if "--sumstats-post-all" in more else 2))
    assert "--sumstats-post" not in r.stderr and "--sumstats-chains" not in r.stderr and "--sumstats-streams" not in r.stderr, r.stderr
    assert "SUMSTAT: %d rows read from" % M in r.stdout, (r.stdout, r.stderr)
    if not has_gpu():
        assert r.returncode != 0


def test_exactly_four_records_are_enough(base, good):
    r = run(*base, "--sumstats", good, "--sumstats-post", *plan(12, 5, 2))  # iterations 6, 8, 10 ... and none more: three
    refused(r, "--sumstats-post: T = 3 record(s) per chain")
    r = run(*base, "--sumstats", good, "--sumstats-post", *plan(13, 5, 2))  # 6, 8, 10, 12
    assert "--sumstats-post" not in r.stderr and "SUMSTAT: %d rows read from" % M in r.stdout, (r.stdout, r.stderr)
