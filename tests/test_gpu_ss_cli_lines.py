"""What hydra_mi355x --sumstats prints (DESIGN.md sections 31-33), line by line: a RESULT line per iteration and chain and the closing
SUMSTAT: line, each in the single chain's form or in the form of --sumstats-chains, which --sumstats-chains 1 selects too.  The
expressions restate the format strings; a number is [-0-9.eE+]+ or nan."""
import os
import re
import subprocess

import pytest

from hydra_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M, M1, ITERS = 400, 160, 90, 6
NA = [3, 17]
NUM = r"(?:[-0-9.eE+]+|nan)"
TAIL = r"sigmaG = +%s, sigmaE = +%s, mu = +%s, m0 = +\d+$" % (NUM, NUM, NUM)
RESULT_ONE = re.compile(r"^RESULT : it +(\d+): proc = +%s s, sweep = +%s ms on the device, " % (NUM, NUM) + TAIL)
RESULT_MANY = re.compile(r"^RESULT : chain +(\d+) it +(\d+): proc = +%s s \(all chains\), sweep = +%s ms on the device \(all chains\), " % (NUM, NUM) + TAIL)
HEAD = (r"^SUMSTAT: \d+ markers used, \d+ left out \(\d+ not in the table, \d+ with another allele pair, \d+ without usable BETA, SE and N, "
        r"\d+ without a finite sd in the panel\), n_eff %s, band %d x \d+ doubles = %s MiB of device memory \(built in %s ms\), " % (NUM, M, NUM, NUM))
STREAMS = r" in (\d+) streams \(largest interval (\d+) markers\)"
FILES = r"\{csv,bet,cpn,acu\}"


def closing_one(base, streams):
    return re.compile(HEAD + r"%s ms per sweep on the device over %d sweeps%s, wrote %s\.%s$" % (NUM, ITERS, STREAMS if streams else "", re.escape(base), FILES))


def closing_many(base, R, streams):
    b = re.escape(base)
    return re.compile(HEAD + r"%d chains, %s ms per sweep launch \(all chains\) on the device over %d sweeps%s, largest R\^ (?:%s|NA), "
                      r"wrote %s\.%s, %s\.c<r>\.%s for the chains r >= 1 and %s\.rhat$" % (R, NUM, ITERS, STREAMS if streams else "", NUM, b, FILES, b, FILES, b))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lines")
    geno = synth.make_genotypes(M, N, seed=21, missing_rate=0.01)
    y, _ = synth.make_phenotype(geno, seed=22, causal_frac=0.1)
    prefix = str(tmp / "train")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=NA)
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%d snp%d 0 %d A C\n" % (1 if j < M1 else 2, j, 1000 * j + 1))

    def run(out, *more):
        cmd = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp / out), "--mcmc-out-name", "r",
               "--number-individuals", str(N), "--number-markers", str(M), "--chain-length", str(ITERS), "--thin", "1", "--seed", "9"] + list(more)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()

    tab = str(tmp / "gwas.assoc")
    run("assoc", "--assoc", "--assoc-no-loco", "--assoc-out", tab)
    ss = ["--sumstats", tab, "--sumstats-n", str(N - len(NA))]
    return tmp, {"one": run("one", *ss), "streams": run("streams", "--sumstats-streams", "4", *ss), "two": run("two", "--sumstats-chains", "2", *ss),
                 "two-streams": run("two-streams", "--sumstats-chains", "2", "--sumstats-streams", "4", *ss), "chains-1": run("chains-1", "--sumstats-chains", "1", *ss)}


def closing(lines):
    last = [ln for ln in lines if ln.startswith("SUMSTAT: ") and " markers used, " in ln]
    assert len(last) == 1 and lines[-1] == last[0]  # the last line of the run
    return last[0]


@pytest.mark.parametrize("name,streams", [("one", False), ("streams", True)])
def test_single_chain_lines(runs, name, streams):
    tmp, out = runs
    lines = out[name]
    res = [ln for ln in lines if ln.startswith("RESULT :")]
    assert len(res) == ITERS
    for it, ln in enumerate(res):
        m = RESULT_ONE.match(ln)
        assert m and int(m.group(1)) == it, ln
    m = closing_one(str(tmp / name / "r"), streams).match(closing(lines))
    assert m, closing(lines)
    if streams:  # the two chromosomes of the .bim
        assert (int(m.group(1)), int(m.group(2))) == (2, M1)
    else:
        assert " streams" not in closing(lines)
    assert sorted(os.listdir(str(tmp / name))) == ["r.acu", "r.bet", "r.cpn", "r.csv"]


@pytest.mark.parametrize("name,R,streams", [("two", 2, False), ("two-streams", 2, True), ("chains-1", 1, False)])
def test_chains_lines(runs, name, R, streams):
    tmp, out = runs
    lines = out[name]
    res = [ln for ln in lines if ln.startswith("RESULT :")]
    assert len(res) == ITERS * R
    for i, ln in enumerate(res):  # iteration after iteration, the chains in order
        m = RESULT_MANY.match(ln)
        assert m and (int(m.group(2)), int(m.group(1))) == divmod(i, R), ln
    m = closing_many(str(tmp / name / "r"), R, streams).match(closing(lines))
    assert m, closing(lines)
    if streams:
        assert (int(m.group(1)), int(m.group(2))) == (2, M1)
    else:
        assert " streams" not in closing(lines)
    want = ["r." + e for e in ("acu", "bet", "cpn", "csv", "rhat")] + ["r.c%d.%s" % (r, e) for r in range(1, R) for e in ("acu", "bet", "cpn", "csv")]
    assert sorted(os.listdir(str(tmp / name))) == sorted(want)
