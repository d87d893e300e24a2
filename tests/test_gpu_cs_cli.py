"""hydra_mi355x --sumstats-cs and --cs end to end, on genotypes with LD of their own (tests/cs_cases.py), two
chromosomes, one row without a phenotype; the sumstats table comes from a short --assoc --assoc-no-loco as in
tests/test_gpu_sspost_cli.py.

  --sumstats-cs   with three chains: <name>.cs is rebuilt as text from the three chains' .cpn records at or after the burn-in,
                  Device.ld_mask on the run's window and tests/cs_restate.py, and compared byte for byte; every other output is byte for
                  byte that of the command without the option; with --sumstats-post --sumstats-post-only the same bytes and no .bet
  --cs            on that run's three .bet files with the same (default) window: the same bytes (the files hold a component != 0 exactly where
                  the effect is != 0); and after a short individual-level chain, the table rebuilt from its .bet
The sumstats case must yield at least two sets, one of them with several members: asserted on the restatement."""
import os
import subprocess

import numpy as np
import pytest

import cs_cases as cc
import cs_restate as cr
from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M, M1, ITERS, BURN = 403, 300, 170, 40, 10
NA = [3]
W = M1 - 1  # the default window of both routes, 1000 kb, with bp 1000 apart: every marker ahead inside the chromosome
R2, LEAD = "0.5", "0.05"
CHAINS = ("r.", "r.c1.", "r.c2.")
CHAIN_FILES = [b + e for b in CHAINS for e in ("csv", "bet", "cpn", "acu")] + ["r.rhat"]
IDS = ["snp%d" % j for j in range(M)]
CHRS = [1 if j < M1 else 2 for j in range(M)]
BPS = [1000 * j + 1 for j in range(M)]


def read(path):
    with open(path, "rb") as f:
        return f.read()


def records(path, dtype):
    """(iterations, records (n, M)) of a .bet or .cpn"""
    raw = read(path)
    assert np.frombuffer(raw[:4], np.uint32)[0] == M
    rec = 4 + np.dtype(dtype).itemsize * M
    n = (len(raw) - 4) // rec
    its = [int(np.frombuffer(raw[4 + k * rec:8 + k * rec], np.uint32)[0]) for k in range(n)]
    return its, np.stack([np.frombuffer(raw[8 + k * rec:4 + (k + 1) * rec], dtype) for k in range(n)])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cs")
    geno, _ = cc.ld_genotypes(M, N, seed=23, missing_rate=0.02)
    y, _ = synth.make_phenotype(geno, seed=24, causal_frac=0.02)
    bed = synth.pack_bed_columns(geno)
    prefix = str(tmp / "train")
    synth.write_plink(prefix, bed, N, y=y, na_rows=NA)
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%d %s 0 %d A C\n" % (CHRS[j], IDS[j], BPS[j]))

    def run(out, *more):
        cmd = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp / out), "--mcmc-out-name", "r",
               "--number-individuals", str(N), "--number-markers", str(M), "--chain-length", str(ITERS), "--thin", "1", "--burn-in", str(BURN), "--seed", "9"] + list(more)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout

    tab = str(tmp / "gwas.assoc")
    run("plain", "--assoc", "--assoc-no-loco", "--assoc-out", tab)
    ss = ["--sumstats", tab, "--sumstats-n", str(N - len(NA)), "--sumstats-chains", "3"]
    cs = ["--sumstats-cs", "--sumstats-cs-lead", LEAD, "--sumstats-cs-r2", R2]
    out = {"plain": run("plain", *ss), "cs": run("cs", *ss, *cs),
           "only": run("only", *ss, *cs, "--sumstats-post", "--sumstats-post-only", "--sumstats-cs-out", str(tmp / "only" / "sets.txt")),
           "from_bet": run("cs", "--cs", "--cs-chains", "3", "--cs-lead", LEAD, "--cs-r2", R2, "--cs-out", str(tmp / "from_bet.cs")),
           "ind": run("ind")}
    out["ind_cs"] = run("ind", "--cs", "--cs-lead", LEAD, "--cs-r2", R2)
    # the masks of the run's window on the chain's rows
    keep = np.ones(N, np.uint8)
    keep[NA] = 0
    dev = capi.Device(0)
    dev.load_bed(bed, N, keep=keep)
    jj = np.arange(M)
    ahead = np.where(jj < M1, M1 - 1 - jj, M - 1 - jj).astype(np.uint32)
    fwd, bwd, _ = dev.ld_mask(W, float(R2), ahead=ahead)
    return tmp, out, fwd, bwd


def rebuilt(flags, C, T, fwd, bwd):
    """the table's text from flags (C T, M), record q = t C + r in row q"""
    h = cc.history_of(flags, C, T)
    return cr.sets_table(IDS, CHRS, BPS, C * T, h.counts(), h.words, M, W, fwd, bwd, lead=float(LEAD))


def test_sumstats_cs_is_the_restatement_on_the_chain_files(runs):
    tmp, out, fwd, bwd = runs
    comp = np.stack([records(str(tmp / "cs" / (b + "cpn")), np.int32)[1] for b in CHAINS])  # (3, ITERS, M)
    assert comp.shape == (3, ITERS, M)
    T = ITERS - BURN
    flags = np.concatenate([comp[:, t] != 0 for t in range(BURN, ITERS)])
    text, leads, (status, size, total, pep, members), taken = rebuilt(flags, 3, T, fwd, bwd)
    print("sumstats-cs: %d leads, %d reached alpha, %d sets, sizes %s" % (len(leads), int(np.count_nonzero(status == 0)), len(taken), [int(size[i]) for i in taken]))
    assert len(taken) >= 2 and max(int(size[i]) for i in taken) >= 2
    assert read(str(tmp / "cs" / "r.cs")).decode() == text
    line = [ln for ln in out["cs"].splitlines() if ln.startswith("SUMSTAT:")][-1]
    assert ", credible sets from %d records: %d leads, %d candidates reached alpha, " % (3 * T, len(leads), int(np.count_nonzero(status == 0))) in line, line
    assert "%d sets written to %s (history %d bytes on the device; " % (len(taken), str(tmp / "cs" / "r.cs"), (3 * T + 63) // 64 * 8 * M) in line, line


def test_every_other_output_is_that_of_the_run_without_the_option(runs):
    tmp, out, _, _ = runs
    for name in CHAIN_FILES:
        assert read(str(tmp / "cs" / name)) == read(str(tmp / "plain" / name)), name
    assert not os.path.exists(str(tmp / "plain" / "r.cs")) and "credible sets" not in out["plain"]
    plain = [ln for ln in out["plain"].splitlines() if ln.startswith("SUMSTAT:")][-1]
    line = [ln for ln in out["cs"].splitlines() if ln.startswith("SUMSTAT:")][-1]
    assert plain.split(" over %d sweeps" % ITERS)[1].replace(str(tmp / "plain"), "D") == line.split(" over %d sweeps" % ITERS)[1].split(", credible sets from")[0].replace(str(tmp / "cs"), "D")


def test_post_only_writes_the_same_sets_and_no_effect_files(runs):
    tmp, _, _, _ = runs
    assert read(str(tmp / "only" / "sets.txt")) == read(str(tmp / "cs" / "r.cs"))
    assert not os.path.exists(str(tmp / "only" / "r.cs")) and os.path.exists(str(tmp / "only" / "r.post"))
    for b in CHAINS:
        for e in ("bet", "cpn", "acu"):
            assert not os.path.exists(str(tmp / "only" / (b + e))), b + e


def test_cs_on_the_bet_files_writes_the_same_table(runs):
    tmp, out, _, _ = runs
    for b in CHAINS:  # the precondition: a component != 0 exactly where the effect is != 0
        its, beta = records(str(tmp / "cs" / (b + "bet")), np.float64)
        assert its == list(range(ITERS)) and np.array_equal(beta != 0.0, records(str(tmp / "cs" / (b + "cpn")), np.int32)[1] != 0)
    assert read(str(tmp / "from_bet.cs")) == read(str(tmp / "cs" / "r.cs"))
    line = [ln for ln in out["from_bet"].splitlines() if ln.startswith("CS     :")][-1]
    assert "credible sets from %d records" % (3 * (ITERS - BURN)) in line and "ms for the sets' kernel" in line, line


def test_cs_after_an_individual_level_chain(runs):
    tmp, _, fwd, bwd = runs
    its, beta = records(str(tmp / "ind" / "r.bet"), np.float64)
    assert its == list(range(ITERS))
    flags = beta[BURN:] != 0.0
    text, leads, (status, size, _, _, _), taken = rebuilt(flags, 1, ITERS - BURN, fwd, bwd)
    print("cs: %d leads, %d reached alpha, %d sets, sizes %s" % (len(leads), int(np.count_nonzero(status == 0)), len(taken), [int(size[i]) for i in taken]))
    assert len(leads) > 0
    assert read(str(tmp / "ind" / "r.cs")).decode() == text
