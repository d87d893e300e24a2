"""hydra_ss_chain with independent LD blocks in parallel streams on the device against the same chain on the
host engine, fed the device's own band; and hydra_mi355x --sumstats --sumstats-streams end to end against a chain driven through
the C ABI.  The streams draw another realisation than the single stream does, so nothing here is held to the oracle's chain: the
host engine with the same streams is the yardstick, and it is pinned to the oracle-pinned single-stream engine one block at a time
(tests/test_ss_streams_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest

import ss_common as sc
from hydra_amd import capi, synth
from test_ss_streams_cpu import blocks_ahead, same_rng

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")


def test_device_chain_with_streams_is_the_host_chain_with_streams():
    # windows that hold each block whole: a band truncated inside a block is not positive definite at N = 517 (e_sqn <= 0 by iteration 3)
    M, N, W = sc.CASE_M, sc.CASE_N, 149
    bed, y = sc.make_case(M, N, seed=12)
    dev = capi.Device(0)
    dev.load_bed(bed, N)
    mave, mstd = dev.marker_stats()[:2]
    X = sc.standardised(bed, N, mave, mstd)
    y = (y - y.mean()) / y.std(ddof=1)
    b = X.T @ y
    sizes = [90, 60, 150]
    ahead = blocks_ahead(sizes, W)
    kw = dict(mS=sc.MS2, groups=(np.arange(M) % 2).astype(np.int32), seed=31)
    ch = capi.SsChain(dev, N, W, b, ahead=ahead, streams=8, **kw)
    band = dev.ss_band()
    assert np.all(band[np.arange(W)[None, :] >= ahead[:, None]] == 0.0)
    ho = capi.SsChain(None, N, W, b, ahead=ahead, band=band, streams=8, **kw)
    assert np.array_equal(ch.streams()[0], np.concatenate([[0], np.cumsum(sizes)])) and np.array_equal(ho.streams()[0], ch.streams()[0])
    moved = 0
    for it in range(4):
        ch.iterate()
        ho.iterate()
        a, h = ch.state(), ho.state()
        (beta, comp, acum, c), (hbeta, hcomp, hacum, hc) = ch.effects(), ho.effects()
        assert np.array_equal(ch.order(), ho.order()) and np.array_equal(comp, hcomp) and np.array_equal(a["cass"], h["cass"]), it
        assert np.array_equal(a["m0"], h["m0"]) and ch.last_nnz() == ho.last_nnz(), it
        assert a["rng_idx"] == h["rng_idx"] and np.array_equal(a["rng_x"], h["rng_x"]), it
        assert all(same_rng(x, z) for x, z in zip(ch.streams()[1], ho.streams()[1])), it
        assert sc.close(beta, hbeta) and sc.close(acum, hacum) and sc.close(c, hc), it
        assert np.array_equal(beta == 0.0, hbeta == 0.0), it
        for k in ("sigmaG", "estPi", "sigmaE", "mu"):
            assert sc.close(a[k], h[k]), (it, k)
        moved += ch.last_nnz()
    assert moved > 0 and dev.last_ss_ms()[1] > 0.0


# ---- the command line ----
N, M, M1, ITERS = 400, 160, 90, 6
NA = [3, 17]


def records(path, dtype):
    raw = open(path, "rb").read()
    assert np.frombuffer(raw[:4], np.uint32)[0] == M
    rec = 4 + np.dtype(dtype).itemsize * M
    assert (len(raw) - 4) % rec == 0
    n = (len(raw) - 4) // rec
    its = [int(np.frombuffer(raw[4 + k * rec:8 + k * rec], np.uint32)[0]) for k in range(n)]
    return its, np.stack([np.frombuffer(raw[8 + k * rec:4 + (k + 1) * rec], dtype) for k in range(n)])


def test_sumstats_streams_end_to_end(tmp_path):
    geno = synth.make_genotypes(M, N, seed=21, missing_rate=0.01)
    y, _ = synth.make_phenotype(geno, seed=22, causal_frac=0.1)
    bed = synth.pack_bed_columns(geno)
    prefix = str(tmp_path / "train")
    synth.write_plink(prefix, bed, N, y=y, na_rows=NA)
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%d snp%d 0 %d A C\n" % (1 if j < M1 else 2, j, 1000 * j + 1))

    def base(out):
        return [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / out), "--mcmc-out-name", "r",
                "--number-individuals", str(N), "--number-markers", str(M), "--chain-length", str(ITERS), "--thin", "1", "--seed", "9"]

    tab = str(tmp_path / "gwas.assoc")
    r = subprocess.run(base("par") + ["--assoc", "--assoc-no-loco", "--assoc-out", tab], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    kept = N - len(NA)
    r = subprocess.run(base("par") + ["--sumstats", tab, "--sumstats-n", str(kept), "--sumstats-streams", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # quota ceil(160 / 8) = 20: the two chromosomes are an interval each
    assert "ms per sweep on the device over %d sweeps in 2 streams (largest interval %d markers), wrote" % (ITERS, M1) in r.stdout, r.stdout
    r0 = subprocess.run(base("one") + ["--sumstats", tab, "--sumstats-n", str(kept)], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr[-2000:]
    assert "ms per sweep on the device over %d sweeps, wrote" % ITERS in r0.stdout and " streams (" not in r0.stdout, r0.stdout

    # the chain's formats
    got = {}
    for out in ("par", "one"):
        d = str(tmp_path / out)
        its, betas = records(d + "/r.bet", np.float64)
        its_c, comps = records(d + "/r.cpn", np.int32)
        its_a, acus = records(d + "/r.acu", np.float64)
        assert its == its_c == its_a == list(range(ITERS))
        assert np.array_equal(comps == 0, betas == 0.0) and comps.min() >= 0 and comps.max() <= 3
        csv = open(d + "/r.csv").read()
        assert len(csv.splitlines()) == ITERS
        got[out] = (betas, comps, acus, csv)
    assert not np.array_equal(got["par"][0], got["one"][0])  # another realisation

    # --predict-bfile takes the .bet
    r = subprocess.run(base("par") + ["--burn-in", "2", "--predict-bfile", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "%d target markers: %d matched" % (M, M) in r.stdout

    # the same chains through the C ABI from the same table; without the option that is the existing single-stream SsChain
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
    j = np.arange(M)
    ahead = np.where(j < M1, M1 - 1 - j, M - 1 - j).astype(np.uint32)
    for out, streams in (("par", 8), ("one", None)):
        ch = capi.SsChain(dev, kept, M1 - 1, xty, ahead=ahead, use=use, mS=np.array([[0.0, 0.01, 0.001, 0.0001]]), seed=9, streams=streams)
        betas, comps, acus, _ = got[out]
        for it in range(ITERS):
            ch.iterate()
            beta, comp, acum, _ = ch.effects()
            assert np.array_equal(comp, comps[it]), (out, it)
            assert sc.close(betas[it], beta) and sc.close(acus[it], acum), (out, it)  # (xty is computed twice: tests/test_gpu_ss_cli.py's rule)
        del ch
    assert np.count_nonzero(got["par"][0][-1]) > 0
