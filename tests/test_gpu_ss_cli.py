"""hydra_mi355x --sumstats end to end: on a synthetic cohort a short --assoc --assoc-no-loco writes the table,
--sumstats samples from it with the same --bfile as the panel.  The output files parse with the chain's readers, --predict-bfile takes
the .bet, and with a window that holds each chromosome whole and --sumstats-n at the kept-row count the .bet records agree with a
hydra_ss_chain driven through the C ABI from the same table.  Nothing is claimed about prediction accuracy."""
import os
import subprocess

import numpy as np
import pytest

import ss_common as sc
from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M, M1, ITERS = 400, 160, 90, 6
NA = [3, 17]


def records(path, dtype):
    raw = open(path, "rb").read()
    assert np.frombuffer(raw[:4], np.uint32)[0] == M
    size = np.dtype(dtype).itemsize
    rec = 4 + size * M
    assert (len(raw) - 4) % rec == 0
    n = (len(raw) - 4) // rec
    its = [int(np.frombuffer(raw[4 + k * rec:8 + k * rec], np.uint32)[0]) for k in range(n)]
    return its, np.stack([np.frombuffer(raw[8 + k * rec:4 + (k + 1) * rec], dtype) for k in range(n)])


def test_assoc_table_to_sumstats_chain(tmp_path):
    geno = synth.make_genotypes(M, N, seed=21, missing_rate=0.01)
    y, _ = synth.make_phenotype(geno, seed=22, causal_frac=0.1)
    bed = synth.pack_bed_columns(geno)
    prefix, out = str(tmp_path / "train"), str(tmp_path / "out")
    synth.write_plink(prefix, bed, N, y=y, na_rows=NA)
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%d snp%d 0 %d A C\n" % (1 if j < M1 else 2, j, 1000 * j + 1))
    base = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", out, "--mcmc-out-name", "r",
            "--number-individuals", str(N), "--number-markers", str(M), "--chain-length", str(ITERS), "--thin", "1", "--seed", "9"]
    tab = str(tmp_path / "gwas.assoc")
    r = subprocess.run(base + ["--assoc", "--assoc-no-loco", "--assoc-out", tab], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    kept = N - len(NA)
    r = subprocess.run(base + ["--sumstats", tab, "--sumstats-n", str(kept)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "window 1000000 bp" in r.stdout and "widest window %d markers ahead" % (M1 - 1) in r.stdout
    assert "n_eff %d (--sumstats-n)" % kept in r.stdout and "ms per sweep on the device over %d sweeps" % ITERS in r.stdout

    # the chain's formats
    its, betas = records(out + "/r.bet", np.float64)
    its_c, comps = records(out + "/r.cpn", np.int32)
    its_a, acus = records(out + "/r.acu", np.float64)
    assert its == its_c == its_a == list(range(ITERS))
    assert np.array_equal(comps == 0, betas == 0.0) and comps.min() >= 0 and comps.max() <= 3
    csv = open(out + "/r.csv").read().splitlines()
    assert len(csv) == ITERS
    for it, line in enumerate(csv):
        f = [x.strip() for x in line.split(",")]
        assert int(f[0]) == it and int(f[1]) == 1 and len(f) == 2 + 1 + 2 + 3 + 4 and int(f[5]) >= int(np.count_nonzero(betas[it]))  # (m0 counts the markers left out too)

    # --predict-bfile takes the .bet
    r = subprocess.run(base + ["--burn-in", "2", "--predict-bfile", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "%d target markers: %d matched" % (M, M) in r.stdout

    # the same chain through the C ABI from the same table
    rows = [ln.split() for ln in open(tab).read().splitlines()]
    col = {h: i for i, h in enumerate(rows[0])}
    keep = np.ones(N, np.uint8)
    keep[NA] = 0
    dev = capi.Device(0)
    dev.load_bed(bed, N, keep=keep)
    mstd = dev.marker_stats()[1]
    xty, use = np.zeros(M), np.zeros(M, np.uint8)
    for t in rows[1:]:
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
    assert use.sum() > M // 2
    j = np.arange(M)
    ahead = np.where(j < M1, M1 - 1 - j, M - 1 - j).astype(np.uint32)
    ch = capi.SsChain(dev, kept, M1 - 1, xty, ahead=ahead, use=use, mS=np.array([[0.0, 0.01, 0.001, 0.0001]]), seed=9)
    for it in range(ITERS):
        ch.iterate()
        beta, comp, acum, _ = ch.effects()
        assert np.array_equal(comp, comps[it]), it
        assert sc.close(betas[it], beta) and sc.close(acus[it], acum), it
    assert np.count_nonzero(betas[-1]) > 0
