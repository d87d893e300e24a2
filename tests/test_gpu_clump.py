"""hydra_mi355x --clump and --ld-prune end to end: every output file rebuilt from Device.ld's r on the chain's rows and the Python walk of
tests/ldwalk.py, and compared as text."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hydra_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldwalk  # noqa: E402

pytestmark = pytest.mark.gpu

N, M = 403, 300
NA = [7]
SPLIT = 170  # the first marker of chromosome 2
WMAX = 172  # a band wide enough for a window that holds a chromosome whole


def make(seed):
    """LD neighbours, missing calls in a fifth of the columns, an all-but-one-missing column, a monomorphic column"""
    geno = synth.make_genotypes(M, N, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for j in range(1, M):
        if j % 4:  # runs of four markers in LD, some of them across the chromosome break
            redraw = rng.random(N) < 0.15
            geno[j] = np.where(redraw, geno[j], geno[j - 1])
    for j in rng.choice(M, size=M // 5, replace=False):
        geno[j, rng.random(N) < rng.uniform(0.01, 0.05)] = 3
    geno[M // 3] = 3
    geno[M // 3, N // 2] = 1
    geno[M // 2] = 1
    return geno


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """the files, the chain's rows on a device, and Device.ld's band at the widest window of these tests, computed once"""
    tmp = tmp_path_factory.mktemp("clump")
    geno = make(31)
    y = np.random.default_rng(4).standard_normal(N)
    prefix = str(tmp / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=NA)
    chrom = ["1" if j < SPLIT else "2" for j in range(M)]
    bp = np.cumsum(np.random.default_rng(6).integers(1, 15, size=M)) + 1000
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%s snp%d 0 %d A C\n" % (chrom[j], j, bp[j]))
    g = geno[:, np.setdiff1d(np.arange(N), NA)]
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(g), g.shape[1])
    _, mstd, n1, n2, nmiss = dev.marker_stats()[:5]
    r, _ = dev.ld(WMAX, sums=False)
    r.setflags(write=False)
    called = g != 3
    p = np.where(called, g, 0).sum(axis=1) / (2.0 * np.maximum(1, called.sum(axis=1)))
    base = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp / "o"), "--mcmc-out-name", "n",
            "--number-individuals", str(N), "--number-markers", str(M)]
    return {"tmp": tmp, "base": base, "chrom": chrom, "bp": bp, "r": r, "finite": np.isfinite(mstd), "maf": np.minimum(p, 1.0 - p), "out": str(tmp / "o" / "n")}


def window(co, kb=None, snps=None):
    ahead = np.zeros(M, dtype=np.uint32)
    for j in range(M):
        q = j
        while q + 1 < M and co["chrom"][q + 1] == co["chrom"][j] and (q + 1 - j <= snps if snps else co["bp"][q + 1] - co["bp"][j] <= 1000 * kb):
            q += 1
        ahead[j] = q - j
    assert 1 <= ahead.max() <= WMAX
    return ahead


def adjacency(co, ahead, t):
    W = int(ahead.max())
    r = co["r"][:, :W]
    with np.errstate(invalid="ignore"):
        fband = (np.arange(1, W + 1)[None, :] <= ahead[:, None]) & ~np.isnan(r) & (r * r >= t)
    return ldwalk.adjacency(fband, ldwalk.backward_of(fband)), int(np.count_nonzero(fband))


def run(co, *args):
    r = subprocess.run(co["base"] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def clumped_text(co, pval, order, owner):
    lines = ["CHR F SNP BP P TOTAL NSIG S05 S01 S001 S0001 SP2"]
    for v in order:
        if owner[v] != v:
            continue
        mem = [q for q in range(M) if owner[q] == v and q != v]
        bins = [0] * 5
        for q in mem:
            bins[0 if pval[q] > 0.05 else 1 if pval[q] > 0.01 else 2 if pval[q] > 0.001 else 3 if pval[q] > 0.0001 else 4] += 1
        lines.append("%s 1 snp%d %d %.12g %d %d %d %d %d %d %s" % (co["chrom"][v], v, co["bp"][v], pval[v], len(mem), *bins,
                                                                   ",".join("snp%d(1)" % q for q in mem) or "NONE"))
    return "\n".join(lines) + "\n"


def test_clump(cohort):
    co = cohort
    rng = np.random.default_rng(9)
    # known P: a coarse grid, so that there are ties (kept in .bim order), P = 0 twice, and every bin
    grid = np.array([0.0, 1e-9, 5e-5, 1e-4, 2e-4, 1e-3, 5e-3, 1e-2, 3e-2, 5e-2, 0.2, 1.0])
    pval = grid[rng.integers(0, len(grid), size=M)]
    pval[[3, 200]] = 0.0
    text = {j: "%.12g" % pval[j] for j in range(M)}
    for j in (10, 11, 250):
        pval[j] = np.nan
    text[10], text[11], text[250] = "NA", "nan", "1.5"
    del text[20]  # a marker of the .bim that FILE does not list
    pval[20] = np.nan
    path = str(co["tmp"] / "known.txt")
    with open(path, "w") as f:
        f.write("CHR SNP BP P\n")
        for j in rng.permutation(M):  # (the order of FILE's rows does not matter)
            if j in text:
                f.write("%s snp%d %d %s\n" % (co["chrom"][j], j, co["bp"][j], text[j]))
            if j == 100:
                f.write("1 ghost 5 1e-8\n")  # an id the .bim does not have
    for args, kb, snps, p1, p2, r2, out in [
            ([], 250, None, 1e-4, 1e-2, 0.5, co["out"] + ".clumped"),  # the defaults: 250 kb hold each chromosome whole
            (["--clump-kb", "0.05", "--clump-p1", "0.001", "--clump-p2", "0.05", "--clump-r2", "0.2", "--clump-out", str(co["tmp"] / "c2.txt")],
             0.05, None, 1e-3, 5e-2, 0.2, str(co["tmp"] / "c2.txt")),
            (["--clump-snps", "64", "--clump-p1", "1", "--clump-p2", "1", "--clump-r2", "0.3", "--clump-out", str(co["tmp"] / "c3.txt")],
             None, 64, 1.0, 1.0, 0.3, str(co["tmp"] / "c3.txt"))]:
        ahead = window(co, kb=kb, snps=snps)
        A, npass = adjacency(co, ahead, r2)
        with np.errstate(invalid="ignore"):
            part = (pval <= p2) & co["finite"]
            lead = (pval <= p1).astype(np.uint8)
        order = np.array(sorted(np.flatnonzero(part), key=lambda j: (pval[j], j)), dtype=np.uint32)
        owner = ldwalk.walk(A, order, lead)
        stdout = run(co, "--clump", path, *args)
        assert "%d rows read from %s, %d matched to the .bim (1 ids not in it, 3 without a P in [0, 1])" % (M, path, M - 1) in stdout, stdout
        assert "%d pairs in the window" % int(ahead.sum()) in stdout and "%d passing pairs" % npass in stdout, stdout
        want = clumped_text(co, pval, order, owner)
        assert open(out).read() == want
        nclumps = want.count("\n") - 1
        assert nclumps > 5 and "(1)" in want
        assert "%d clumps with %d markers claimed" % (nclumps, np.count_nonzero((owner != -1) & (owner != np.arange(M)))) in stdout, stdout


@pytest.mark.parametrize("form", ["snps", "kb", "default"])
def test_ld_prune(cohort, form):
    co = cohort
    T = 0.3
    if form == "snps":
        args, ahead, prefix = ["--ld-prune-snps", "20", "--ld-prune-out", str(co["tmp"] / "p1")], window(co, snps=20), str(co["tmp"] / "p1")
    elif form == "kb":
        args, ahead, prefix = ["--ld-prune-kb", "0.1", "--ld-prune-out", str(co["tmp"] / "p2")], window(co, kb=0.1), str(co["tmp"] / "p2")
    else:
        args, ahead, prefix = [], window(co, snps=50), co["out"]
    A, npass = adjacency(co, ahead, np.nextafter(T, np.inf))  # removed iff r^2 > T
    order = np.array(sorted(np.flatnonzero(co["finite"]), key=lambda j: (-co["maf"][j], j)), dtype=np.uint32)
    owner = ldwalk.walk(A, order)
    stdout = run(co, "--ld-prune", str(T), *args)
    assert "%d pairs in the window" % int(ahead.sum()) in stdout and "%d passing pairs" % npass in stdout, stdout
    keep = owner == np.arange(M)
    got_in = open(prefix + ".prune.in").read()
    got_out = open(prefix + ".prune.out").read()
    assert got_in == "".join("snp%d\n" % j for j in range(M) if keep[j])
    assert got_out == "".join("snp%d\n" % j for j in range(M) if not keep[j])
    assert sorted(got_in.split() + got_out.split(), key=lambda s: int(s[3:])) == ["snp%d" % j for j in range(M)]  # the .bim exactly once
    assert "snp%d" % (M // 2) in got_out.split() and 20 < keep.sum() < M - 20
    # what was kept has no pair above T inside the window, and nothing that was removed could be put back
    assert not A[np.ix_(keep, keep)].any()
    assert all(A[j][keep].any() for j in np.flatnonzero(~keep & co["finite"]))


def test_assoc_then_clump(cohort):
    co = cohort
    run(co, "--assoc", "--assoc-no-loco")
    stdout = run(co, "--clump", co["out"] + ".assoc", "--clump-p1", "0.05", "--clump-p2", "0.5", "--clump-snps", "30", "--clump-out", str(co["tmp"] / "a.clumped"))
    assert "%d rows read from" % M in stdout and "%d matched to the .bim (0 ids not in it" % M in stdout, stdout
    lines = open(str(co["tmp"] / "a.clumped")).read().splitlines()
    assert lines[0] == "CHR F SNP BP P TOTAL NSIG S05 S01 S001 S0001 SP2" and len(lines) > 1
    assert "%d clumps" % (len(lines) - 1) in stdout
