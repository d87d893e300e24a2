"""hydra_mi355x --sumstats --sumstats-post end to end, by tests/test_gpu_ss_chains.py's route: a short --assoc
--assoc-no-loco writes the table (two of its rows are then dropped, so two markers are not used), --sumstats samples from it.

  three chains   every chain's .csv, .bet, .cpn, .acu and the .rhat are byte for byte those of the command without --sumstats-post;
                 <name>.post agrees with tests/sspost_restate.py fed from the three chains' .bet and .cpn records at or after the
                 burn-in, within ten units of %.9g's last digit (section 33's rule for .rhat); the rows of unused markers are NA
  -post-only     the same .post, .csv and .rhat, and no .bet, .cpn or .acu
  one chain      with --sumstats-streams, --thin 2 and --sumstats-post-all every iteration from the burn-in on counts; the table
                 agrees with a hydra_ss_chain driven through the C ABI with hgibbs_ss_post_add after every counted iteration"""
import math
import os
import subprocess

import numpy as np
import pytest

import sspost_restate as pr
from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M, M1, ITERS, BURN = 400, 160, 90, 12, 2
NA = [3, 17]
DROPPED = [5, 100]
K = 4
HEAD = ["CHR", "SNP", "BP", "A1", "A2", "USED", "NCHAINS", "NREC", "MEAN", "SD", "BETA", "PIP", "PC1", "PC2", "PC3", "RHAT"]
CHAIN_FILES = ["r.csv", "r.c1.csv", "r.c2.csv", "r.rhat"]
EFFECT_FILES = [b + e for b in ("r.", "r.c1.", "r.c2.") for e in ("bet", "cpn", "acu")]


def read(path):
    with open(path, "rb") as f:
        return f.read()


def unit(v):
    """the unit of the last of %.9g's digits at v"""
    return 10.0 ** (math.floor(math.log10(abs(v))) - 8) if v != 0.0 else 1e-15


def records(path, dtype):
    raw = read(path)
    assert np.frombuffer(raw[:4], np.uint32)[0] == M
    rec = 4 + np.dtype(dtype).itemsize * M
    n = (len(raw) - 4) // rec
    return np.stack([np.frombuffer(raw[8 + k * rec:4 + (k + 1) * rec], dtype) for k in range(n)])


def post_table(path):
    lines = read(path).decode().splitlines()
    assert lines[0].split("\t") == HEAD
    rows = [ln.split("\t") for ln in lines[1:]]
    assert len(rows) == M and all(len(t) == len(HEAD) for t in rows)
    assert [t[1] for t in rows] == ["snp%d" % j for j in range(M)]
    assert [t[0] for t in rows] == ["1" if j < M1 else "2" for j in range(M)] and [t[2] for t in rows] == [str(1000 * j + 1) for j in range(M)]
    return rows


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("post")
    geno = synth.make_genotypes(M, N, seed=21, missing_rate=0.01)
    y, _ = synth.make_phenotype(geno, seed=22, causal_frac=0.1)
    bed = synth.pack_bed_columns(geno)
    prefix = str(tmp / "train")
    synth.write_plink(prefix, bed, N, y=y, na_rows=NA)
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%d snp%d 0 %d A C\n" % (1 if j < M1 else 2, j, 1000 * j + 1))

    def run(out, *more):
        cmd = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp / out), "--mcmc-out-name", "r",
               "--number-individuals", str(N), "--number-markers", str(M), "--chain-length", str(ITERS), "--thin", "1", "--seed", "9"] + list(more)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout

    full = str(tmp / "gwas.assoc")
    run("plain", "--assoc", "--assoc-no-loco", "--assoc-out", full)
    tab = str(tmp / "gwas.dropped.assoc")
    lines = read(full).decode().splitlines()
    snp = lines[0].split().index("SNP")
    with open(tab, "w") as f:
        f.write("\n".join(ln for ln in lines if ln.split()[snp] not in ["snp%d" % j for j in DROPPED]) + "\n")
    ss = ["--sumstats", tab, "--sumstats-n", str(N - len(NA)), "--burn-in", str(BURN)]
    out = {"plain": run("plain", "--sumstats-chains", "3", *ss),
           "post": run("post", "--sumstats-chains", "3", "--sumstats-post", *ss),
           "only": run("only", "--sumstats-chains", "3", "--sumstats-post", "--sumstats-post-only", "--sumstats-post-out", str(tmp / "only" / "table.txt"), *ss),
           "single": run("single", "--sumstats-streams", "4", "--sumstats-post", "--sumstats-post-all", "--thin", "2", *ss)}
    return tmp, out, tab, bed


def test_chain_files_are_those_of_the_run_without_the_option(runs):
    tmp, out, _, _ = runs
    for name in CHAIN_FILES + EFFECT_FILES:
        assert read(str(tmp / "post" / name)) == read(str(tmp / "plain" / name)), name
    assert not os.path.exists(str(tmp / "plain" / "r.post")) and "records per chain counted" not in out["plain"]
    line = [ln for ln in out["post"].splitlines() if ln.startswith("SUMSTAT:")][-1]
    assert ", %d records per chain counted on the device into %s (" % (ITERS - BURN, str(tmp / "post" / "r.post")) in line and "ms for all adds" in line, line
    # but for what the line gains, it is the line of the run without the option
    plain = [ln for ln in out["plain"].splitlines() if ln.startswith("SUMSTAT:")][-1]
    assert plain.split(" over %d sweeps" % ITERS)[1].replace(str(tmp / "plain"), "D") == line.split(" over %d sweeps" % ITERS)[1].split(", %d records per chain" % (ITERS - BURN))[0].replace(str(tmp / "post"), "D")


def test_post_table_agrees_with_the_restatement_on_the_chain_files(runs):
    tmp, _, _, bed = runs
    rows = post_table(str(tmp / "post" / "r.post"))
    beta = np.stack([records(str(tmp / "post" / (b + "bet")), np.float64) for b in ("r.", "r.c1.", "r.c2.")])  # (3, ITERS, M)
    comp = np.stack([records(str(tmp / "post" / (b + "cpn")), np.int32) for b in ("r.", "r.c1.", "r.c2.")])
    assert beta.shape == comp.shape == (3, ITERS, M)
    T = ITERS - BURN
    want = pr.run(((beta[:, t], comp[:, t]) for t in range(BURN, ITERS)), 3, M, K, T)
    mean, sd, pip, rhat = want.final()
    keep = np.ones(N, np.uint8)
    keep[NA] = 0
    dev = capi.Device(0)
    dev.load_bed(bed, N, keep=keep)
    mstd = dev.marker_stats()[1]
    used = [j for j in range(M) if rows[j][5] == "1"]
    assert [j for j in range(M) if j not in used] == DROPPED
    for j in DROPPED:
        assert rows[j][5] == "0" and rows[j][6:] == ["NA"] * (len(HEAD) - 6), rows[j]
        assert not beta[:, :, j].any()
    worst = 0.0
    for j in used:
        t = rows[j]
        assert t[6:8] == ["3", str(T)]
        cols = [("MEAN", t[8], mean[j]), ("SD", t[9], sd[j]), ("BETA", t[10], mean[j] * mstd[j]), ("PIP", t[11], pip[j]), ("RHAT", t[15], rhat[j])]
        cols += [("PC%d" % k, t[11 + k], float(want.cnt[k, j]) / float(3 * T)) for k in range(1, K)]
        for what, g, w in cols:
            if math.isnan(w):
                assert g == "NA", (j, what, g)
                continue
            assert g != "NA", (j, what)
            dev_units = abs(float(g) - w) / unit(w)
            worst = max(worst, dev_units)
            assert dev_units <= 10.0, (j, what, g, w)
    print("post table: largest deviation %.3f units of %%.9g's last digit over %d markers" % (worst, len(used)))
    assert np.any((pip[used] > 0.0) & (pip[used] < 1.0)) and np.any(np.isfinite(rhat[used]))


def test_post_only_writes_the_same_table_and_no_effect_files(runs):
    tmp, out, _, _ = runs
    assert read(str(tmp / "only" / "table.txt")) == read(str(tmp / "post" / "r.post"))
    assert not os.path.exists(str(tmp / "only" / "r.post"))
    for name in CHAIN_FILES:
        assert read(str(tmp / "only" / name)) == read(str(tmp / "post" / name)), name
    for name in EFFECT_FILES:
        assert not os.path.exists(str(tmp / "only" / name)), name
    line = [ln for ln in out["only"].splitlines() if ln.startswith("SUMSTAT:")][-1]
    assert "{csv,bet,cpn,acu}" not in line and "r.csv, " in line, line


def test_single_chain_with_streams_counting_every_iteration(runs):
    tmp, out, tab, bed = runs
    rows = post_table(str(tmp / "single" / "r.post"))
    T = ITERS - BURN
    assert len(read(str(tmp / "single" / "r.csv")).decode().splitlines()) == ITERS // 2  # (--thin 2: the files hold six records, the table ten)
    # the same chain through the C ABI from the same table (tests/test_gpu_ss_streams_chain.py's route)
    kept = N - len(NA)
    tr = [ln.split() for ln in open(tab).read().splitlines()]
    col = {h: i for i, h in enumerate(tr[0])}
    keep = np.ones(N, np.uint8)
    keep[NA] = 0
    dev = capi.Device(0)
    dev.load_bed(bed, N, keep=keep)
    mstd = dev.marker_stats()[1]
    xty, use = np.zeros(M), np.zeros(M, np.uint8)
    for t in tr[1:]:
        j = int(t[col["SNP"]][3:])
        try:
            b, se, n = float(t[col["BETA"]]), float(t[col["SE"]]), float(t[col["N"]])
        except ValueError:
            continue
        if not (np.isfinite(b) and np.isfinite(se) and se > 0 and n > 0 and np.isfinite(mstd[j])):
            continue
        z = b / se
        xty[j] = (kept - 1.0) * (z / np.sqrt(n - 2.0 + z * z))
        use[j] = 1
    jj = np.arange(M)
    ahead = np.where(jj < M1, M1 - 1 - jj, M - 1 - jj).astype(np.uint32)
    ch = capi.SsChain(dev, kept, M1 - 1, xty, ahead=ahead, use=use, mS=np.array([[0.0, 0.01, 0.001, 0.0001]]), seed=9, streams=4)
    dev.ss_post_begin(0, T)
    for it in range(ITERS):
        ch.iterate()
        if it >= BURN:
            dev.ss_post_add()
    mean, sd, pip, cnt, rhat = dev.ss_post_get()
    del ch
    # The two chains compute xty apart (tests/test_gpu_ss_cli.py's rule: components equal, effects at 1e-9 max(1, |b|)), and the table
    # rounds to nine digits.  So: the counts' columns equal as printed; MEAN, SD and BETA within 1e-9 max(1, |w|) plus a unit of the
    # printed last digit; R^ -- a ratio of sums of squares of effects whose scale s is at least 1e-3 (the smallest mixture sd is
    # sqrt(1e-4 sigmaG)), so a shift of 1e-9 in the effects moves it by some 1e-9 / s relative -- within 1e-6 relative.
    for j in range(M):
        t = rows[j]
        assert t[5] == str(int(use[j])), j
        if not use[j]:
            assert t[6:] == ["NA"] * (len(HEAD) - 6)
            continue
        assert t[6:8] == ["1", str(T)]
        assert t[11] == "%.9g" % pip[j] and [t[11 + k] for k in range(1, K)] == ["%.9g" % (float(cnt[k, j]) / float(T)) for k in range(1, K)], j
        for what, g, w in (("MEAN", t[8], mean[j]), ("SD", t[9], sd[j]), ("BETA", t[10], mean[j] * mstd[j])):
            assert abs(float(g) - w) <= 1e-9 * max(1.0, abs(w)) + unit(w), (j, what, g, w)
        if math.isnan(rhat[j]):
            assert t[15] == "NA", j
        else:
            assert abs(float(t[15]) - rhat[j]) <= 1e-6 * rhat[j] + unit(rhat[j]), (j, t[15], rhat[j])
    assert np.any((pip > 0.0) & (pip < 1.0)) and np.any(np.isfinite(rhat))
    line = [ln for ln in out["single"].splitlines() if ln.startswith("SUMSTAT:")][-1]
    assert "in 2 streams" in line and ", %d records per chain counted on the device into " % T in line, line
