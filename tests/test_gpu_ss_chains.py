"""R chains on one band.  hydra_ss_multi: chain r of an SsMultiChain is, bit for bit, the device SsChain seeded
with seeds[r] -- every .csv line, effect, component, acum, c and generator over six iterations, single stream and with streams on a
window with cuts.  hydra_mi355x --sumstats --sumstats-chains: chain 0's files are those of the run without the option, chain 1's
those of the run with --seed raised by one, and <name>.rhat agrees with tests/mcmcdiag_restate.py applied to the chains' .csv files."""
import math
import os
import subprocess

import numpy as np
import pytest

import mcmcdiag_restate as md
import ss_common as sc
from hydra_amd import capi, synth
from test_ss_streams_cpu import blocks_ahead, same_rng

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
SEEDS = [31, 32, 33]
ITERS6 = 6


@pytest.fixture(scope="module")
def panel():
    # tests/test_gpu_ss_streams_chain.py's panel: windows that hold each block whole
    M, N, W = sc.CASE_M, sc.CASE_N, 149
    bed, y = sc.make_case(M, N, seed=12)
    dev = capi.Device(0)
    dev.load_bed(bed, N)
    mave, mstd = dev.marker_stats()[:2]
    X = sc.standardised(bed, N, mave, mstd)
    y = (y - y.mean()) / y.std(ddof=1)
    return dev, N, W, X.T @ y, blocks_ahead([90, 60, 150], W)


@pytest.mark.parametrize("streams", [None, 8], ids=["single-stream", "streams"])
def test_every_chain_is_the_single_chain_of_its_seed(panel, streams):
    dev, N, W, b, ahead = panel
    kw = dict(mS=sc.MS2, groups=(np.arange(dev.M) % 2).astype(np.int32))
    want = []
    for seed in SEEDS:  # one after the other: a handle holds one summary-statistics state
        ch = capi.SsChain(dev, N, W, b, ahead=ahead, seed=seed, streams=streams, **kw)
        rows = []
        for it in range(ITERS6):
            ch.iterate()
            rows.append((ch.csv_line(it), ch.effects(), ch.state(), ch.streams()[1], ch.last_nnz()))
        want.append(rows)
        del ch
    mc = capi.SsMultiChain(dev, N, W, b, SEEDS, ahead=ahead, streams=streams, **kw)
    if streams:
        assert np.array_equal(mc.streams()[0], [0, 90, 150, 300])
    moved = 0
    for it in range(ITERS6):
        mc.iterate()
        gens = mc.streams()[1]
        for r in range(len(SEEDS)):
            line, eff, st, sgen, nnz = want[r][it]
            assert mc.csv_line(r, it) == line, (r, it)
            for a, e in zip(mc.effects(r), eff):
                assert np.array_equal(a, e), (r, it)
            got = mc.state(r)
            assert got["rng_idx"] == st["rng_idx"] and np.array_equal(got["rng_x"], st["rng_x"]), (r, it)
            for k in ("sigmaG", "estPi", "m0", "cass"):
                assert np.array_equal(got[k], st[k]), (r, it, k)
            assert (got["sigmaE"], got["mu"]) == (st["sigmaE"], st["mu"]) and mc.last_nnz(r) == nnz, (r, it)
            if streams:
                assert all(same_rng(x, z) for x, z in zip(gens[r], sgen)), (r, it)
            moved += nnz
    assert moved > 0 and dev.last_ss_ms()[1] > 0.0
    assert want[0][-1][0] != want[1][-1][0]  # (other seeds, other chains)
    del mc


# ---- the command line ----
N, M, M1, ITERS = 400, 160, 90, 12
NA = [3, 17]
FILES = ("csv", "bet", "cpn", "acu")
ROWS = ["sigmaG[0]", "sigmaG", "sigmaE", "h2", "m0", "mu"]


def read(path):
    with open(path, "rb") as f:
        return f.read()


def unit(v):
    """the unit of the last of %.9g's digits at v"""
    return 10.0 ** (math.floor(math.log10(abs(v))) - 8) if v != 0.0 else 1e-15


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("chains")
    geno = synth.make_genotypes(M, N, seed=21, missing_rate=0.01)
    y, _ = synth.make_phenotype(geno, seed=22, causal_frac=0.1)
    prefix = str(tmp / "train")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=NA)
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%d snp%d 0 %d A C\n" % (1 if j < M1 else 2, j, 1000 * j + 1))

    def run(out, name, seed, *more):
        cmd = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp / out), "--mcmc-out-name", name,
               "--number-individuals", str(N), "--number-markers", str(M), "--chain-length", str(ITERS), "--thin", "1", "--seed", str(seed)] + list(more)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout

    tab = str(tmp / "gwas.assoc")
    run("multi", "r", 9, "--assoc", "--assoc-no-loco", "--assoc-out", tab)
    ss = ["--sumstats", tab, "--sumstats-n", str(N - len(NA))]
    out = {"multi": run("multi", "r", 9, "--burn-in", "2", "--sumstats-chains", "3", *ss),
           "one": run("one", "r", 9, "--burn-in", "2", *ss),
           "next": run("next", "other", 10, "--burn-in", "2", *ss),
           "short": run("short", "r", 9, "--burn-in", "9", "--sumstats-chains", "2", *ss)}
    return tmp, out


def test_chain_files_are_those_of_the_single_runs(runs):
    tmp, out = runs
    for ext in FILES:
        assert read(str(tmp / "multi" / ("r." + ext))) == read(str(tmp / "one" / ("r." + ext))), ext
        assert read(str(tmp / "multi" / ("r.c1." + ext))) == read(str(tmp / "next" / ("other." + ext))), ext
        assert os.path.getsize(str(tmp / "multi" / ("r.c2." + ext))) == os.path.getsize(str(tmp / "one" / ("r." + ext))), ext
    assert read(str(tmp / "multi" / "r.csv")) != read(str(tmp / "multi" / "r.c1.csv"))
    assert not os.path.exists(str(tmp / "one" / "r.rhat")) and " chains, " not in out["one"] and "largest R^" not in out["one"]
    assert ", 3 chains, " in out["multi"] and "ms per sweep launch (all chains) on the device over %d sweeps" % ITERS in out["multi"]
    for r in range(3):
        assert out["multi"].count("RESULT : chain %2d it " % r) == ITERS
    assert "RESULT : chain" not in out["one"]


def test_rhat_table_agrees_with_the_restatement_on_the_csv_files(runs):
    tmp, out = runs
    lines = read(str(tmp / "multi" / "r.rhat")).decode().splitlines()
    assert lines[0].split("\t") == ["PARAM", "NCHAINS", "NREC", "MEAN", "SD", "RHAT", "ESS"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [t[0] for t in rows] == ROWS and all(t[1:3] == ["3", "10"] for t in rows)
    # the .csv's columns (one group): iteration, G, sigmaG[0], sigmaE, h2, m0, G, K, pi...
    csv = [np.array([[float(v) for v in ln.split(",")] for ln in read(str(tmp / "multi" / name)).decode().splitlines()])
           for name in ("r.csv", "r.c1.csv", "r.c2.csv")]
    assert all(c.shape[0] == ITERS and np.array_equal(c[:, 0], np.arange(ITERS)) for c in csv)
    col = {"sigmaG[0]": 2, "sigmaG": 2, "sigmaE": 3, "h2": 4, "m0": 5}
    worst = 0.0
    for t in rows:
        if t[0] not in col:
            continue
        x = np.stack([c[2:, col[t[0]]] for c in csv])
        want = md.diag(x)
        for g, w, what in zip(t[3:], want, ("MEAN", "SD", "RHAT", "ESS")):
            dev = abs(float(g) - w) / unit(w)
            print("rhat table: %s %s = %s, restated %.12g, %.3f units of the last digit" % (t[0], what, g, w, dev))
            worst = max(worst, dev)
            assert dev <= 10.0, (t[0], what, g, w)
        if t[0] == "m0":
            assert t[3] == "%.9g" % x.mean()
    print("rhat table: largest deviation %.3f units of %%.9g's last digit" % worst)
    largest = max(float(t[5]) for t in rows if t[5] != "NA")
    assert "largest R^ %.9g," % largest in out["multi"]


def test_fewer_than_four_records_give_na(runs):
    tmp, out = runs
    lines = read(str(tmp / "short" / "r.rhat")).decode().splitlines()
    assert lines[0].split("\t") == ["PARAM", "NCHAINS", "NREC", "MEAN", "SD", "RHAT", "ESS"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [t[0] for t in rows] == ROWS and all(t[1:] == ["2", "3", "NA", "NA", "NA", "NA"] for t in rows)
    assert "3 thinned record(s) per chain at or after --burn-in 9, split-R^ needs at least 4: every statistic is NA" in out["short"]
    assert "largest R^ NA," in out["short"]
