"""Windowed LD (hgibbs_ld, hydra_mi355x --ld-window) against NumPy: the exact integer sums, r from the oracle's standardisation, the
chain's own dot, bit identity across chunkings and tuning, and the CLI's tables."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hydra_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402

pytestmark = pytest.mark.gpu


def oracle_stats(geno):
    """mave, mstd of every marker from the oracle's orc_marker_stats (the reference's formula), on the counts of geno"""
    L = orc.load()
    import ctypes as C
    M, N = geno.shape
    mave, mstd = np.zeros(M), np.zeros(M)
    for j in range(M):
        n1, n2, nm = (int(np.count_nonzero(geno[j] == v)) for v in (1, 2, 3))
        a, s = C.c_double(), C.c_double()
        L.orc_marker_stats(n1, n2, nm, N, C.byref(a), C.byref(s))
        mave[j], mstd[j] = a.value, s.value
    return mave, mstd


def reference(geno, W, block=64):
    """sums (M, W, 4) int64: G, Bjq, Bqj, D of (j, j + d + 1), 0 past M; r (M, W) f64 = x_j'x_q / (N - 1), NaN past M and where an mstd
    is not finite"""
    M, N = geno.shape
    g = np.where(geno == 3, 0, geno).astype(np.float64)
    c = (geno != 3).astype(np.float64)
    mave, mstd = oracle_stats(geno)
    with np.errstate(invalid="ignore"):
        x = np.where(geno == 3, 0.0, (g - mave[:, None]) * mstd[:, None])
    fin = np.isfinite(mstd)
    sums = np.zeros((M, W, 4), dtype=np.int64)
    r = np.full((M, W), np.nan)
    for j0 in range(0, M, block):
        j1 = min(M, j0 + block)
        q1 = min(M, j1 + W)
        # integer sums through f64 products: every entry is below 4 N < 2^53, so exact
        P = [g[j0:j1] @ g[j0:q1].T, g[j0:j1] @ c[j0:q1].T, c[j0:j1] @ g[j0:q1].T, c[j0:j1] @ c[j0:q1].T]
        with np.errstate(invalid="ignore"):
            X = x[j0:j1] @ x[j0:q1].T / (N - 1)
        # r is NaN where an mstd is not finite.  A monomorphic column brings that about by itself (x = 0 x inf), a column with no call
        # at all does not (mave and mstd are NaN, but x is 0 at every missing call), so the rule is applied
        X[~fin[j0:j1], :] = np.nan
        X[:, ~fin[j0:q1]] = np.nan
        for jj in range(j1 - j0):
            nd = min(W, M - 1 - (j0 + jj))  # pairs (j, j + d), d = 1 .. nd: columns jj + 1 .. jj + nd of the block's products
            for t in range(4):
                sums[j0 + jj, :nd, t] = P[t][jj, jj + 1:jj + 1 + nd].astype(np.int64)
            r[j0 + jj, :nd] = X[jj, jj + 1:jj + 1 + nd]
    return sums, r


def make(N, M, seed, missing_cols=True):
    geno = synth.make_genotypes(M, N, seed=seed)
    rng = np.random.default_rng(seed + 1)
    # neighbours in LD: a column copies its left neighbour with a fifth of the calls redrawn
    for j in range(1, M, 3):
        redraw = rng.random(N) < 0.2
        geno[j] = np.where(redraw, geno[j], geno[j - 1])
    if missing_cols:
        for j in rng.choice(M, size=M // 5, replace=False):  # 1-5 % missing calls next to clean columns
            geno[j, rng.random(N) < rng.uniform(0.01, 0.05)] = 3
        geno[M // 3] = 3
        geno[M // 3, N // 2] = 1  # missing everywhere but one individual
        geno[M // 2] = 1  # monomorphic (r NaN)
    return geno


def device(geno):
    M, N = geno.shape
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    assert np.array_equal(synth.unpack_bed_columns(dev.get_bed(), N), geno)
    dev.marker_stats()
    return dev


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("N,M", [(1001, 333), (4099, 97)])
def test_sums_and_r_match_numpy(N, M):
    geno = make(N, M, seed=N + M)
    dev = device(geno)
    for W in (1, 15, 16, 17, 64, 65, 300):
        ref_s, ref_r = reference(geno, W)
        r, s = dev.ld(W)
        assert np.array_equal(s, ref_s), "W=%d: integer sums differ" % W
        assert np.array_equal(np.isnan(r), np.isnan(ref_r)), "W=%d: NaN pattern differs" % W
        ok = ~np.isnan(ref_r)
        assert np.max(np.abs(r[ok] - ref_r[ok])) <= 1e-12, "W=%d: r beyond 1e-12" % W


def test_clean_data_and_padding():
    """no missing call anywhere (the one-product form), N one past a multiple of 4096"""
    geno = make(4097, 150, seed=5, missing_cols=False)
    dev = device(geno)
    for W in (3, 40):
        ref_s, ref_r = reference(geno, W)
        r, s = dev.ld(W)
        assert np.array_equal(s, ref_s)
        ok = ~np.isnan(ref_r)
        assert np.array_equal(np.isnan(r), ~ok) and np.max(np.abs(r[ok] - ref_r[ok])) <= 1e-12


GRID_N = [2, 15, 16, 17, 63, 65, 511, 512, 513, 1025]
GRID_M = [1, 2, 15, 16, 17, 63, 64, 65, 145]
GRID_W = [1, 16, 129, 4096]  # 129: the first window with a second pass of LD_QP tiles; 4096 = LD_WMAX: 29 passes, 256 tiles past M


def make_grid(N, M, seed, missing_cols=True):
    """make() where it can plant its columns (M >= 4); below that by hand: polymorphic columns, one missing call in the last"""
    if M >= 4:
        return make(N, M, seed, missing_cols)
    geno = synth.make_genotypes(M, N, seed=seed)
    if missing_cols:
        geno[M - 1, 0] = 3
    return geno


def check_band(dev, ref_s, ref_r, W, what):
    """hgibbs_ld at window W against the leading W columns of a reference taken at a window at least as wide"""
    r, s = dev.ld(W)
    rs, rr = ref_s[:, :W], ref_r[:, :W]
    assert np.array_equal(s, rs), "%s: integer sums differ" % (what,)
    ok = ~np.isnan(rr)
    assert np.array_equal(np.isnan(r), ~ok), "%s: NaN pattern differs" % (what,)
    if ok.any():
        assert np.max(np.abs(r[ok] - rr[ok])) <= 1e-12, "%s: r beyond 1e-12" % (what,)
    return r, s


def run_grid(N, missing_cols):
    for M in GRID_M:
        geno = make_grid(N, M, seed=N + M, missing_cols=missing_cols)
        assert bool((geno == 3).any()) == missing_cols
        dev = device(geno)
        ref_s, ref_r = reference(geno, max(GRID_W))
        for W in GRID_W:
            r, s = check_band(dev, ref_s, ref_r, W, "N=%d M=%d W=%d" % (N, M, W))
            if M == 1:  # a band without a pair
                assert np.all(np.isnan(r)) and not s.any()
        dev.close()


@pytest.mark.parametrize("N", GRID_N)
def test_edge_grid(N):
    """individuals below one slice of 512 and next to 16, 64, 512 and 1024; markers of one tile of sixteen or less and next to 16, 64
    and 144 (nine tiles: one pass); every window of GRID_W.  Data with missing calls: k_ld<true>"""
    run_grid(N, True)


@pytest.mark.parametrize("N", [16, 513])
def test_edge_grid_clean(N):
    """no missing call anywhere: k_ld<false>"""
    run_grid(N, False)


def test_the_piece_loop():
    """hgibbs_ld's own pieces: 4 200 band rows x 4 096 offsets are 17.2 M pairs, two pieces of at most 2^24.  r against NumPy, bit for bit
    against the same band fetched in chunks of 1 000 markers (one piece each), and those chunks' sums against NumPy exactly.  Then one
    call of two pieces whose first marker is no multiple of 16: rows [7, 4197) are 17.16 M pairs, cut into [7, 4103) and [4103, 4197)."""
    N, M, W = 130, 4200, 4096
    geno = make(N, M, seed=N + M)
    dev = device(geno)
    ref_s, ref_r = reference(geno, W, block=256)
    r, none = dev.ld(W, sums=False)
    assert none is None
    ok = ~np.isnan(ref_r)
    assert np.array_equal(np.isnan(r), ~ok) and np.max(np.abs(r[ok] - ref_r[ok])) <= 1e-12
    for a in range(0, M, 1000):
        n = min(1000, M - a)
        rc, sc = dev.ld(W, m0=a, count=n)
        assert same_bits(rc, r[a:a + n]), a
        assert np.array_equal(sc, ref_s[a:a + n]), a
    rc, sc = dev.ld(W, m0=7, count=4190)
    assert same_bits(rc, r[7:4197])
    assert np.array_equal(sc, ref_s[7:4197])


def test_the_chains_own_dot():
    """with the residual set to x_q, hgibbs_dot_marker(j) is x_j'x_q = r_jq (N - 1)"""
    N, M, W = 2003, 120, 20
    geno = make(N, M, seed=11)
    dev = device(geno)
    r, _ = dev.ld(W, sums=False)
    mave, mstd = oracle_stats(geno)
    for q in (5, 17, 60, 119):
        if not np.isfinite(mstd[q]):
            continue
        xq = np.where(geno[q] == 3, 0.0, (geno[q] - mave[q]) * mstd[q])
        dev.set_residual(xq)
        for j in range(max(0, q - W), q):
            if np.isnan(r[j, q - j - 1]):
                continue
            dot = dev.dot_marker(j)
            assert abs(dot - r[j, q - j - 1] * (N - 1)) <= 1e-9 * max(1.0, abs(dot)), (j, q)


def test_bit_identical_across_chunkings_options_and_launches():
    N, M, W = 3001, 260, 70
    geno = make(N, M, seed=3)
    dev = device(geno)
    r0, s0 = dev.ld(W)
    r1, s1 = dev.ld(W)
    assert same_bits(r0, r1) and np.array_equal(s0, s1)
    for cuts in ([0, 37, 200, M], [0, 1, 17, 18, 100, M - 1, M], [0, 64, 128, 192, M]):
        parts = [dev.ld(W, m0=a, count=b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        assert same_bits(np.concatenate([p[0] for p in parts]), r0), cuts
        assert np.array_equal(np.concatenate([p[1] for p in parts]), s0), cuts
    for split in (1, 2, 3, 5, 6, 1000, 0):
        dev.set_option("ld_split", split)
        r, s = dev.ld(W)
        assert same_bits(r, r0) and np.array_equal(s, s0), split
    with pytest.raises(capi.HgError, match="ld_split"):
        dev.set_option("ld_split", -1)
    assert dev.last_ld_ms() > 0.0


def test_refusals():
    geno = make(300, 40, seed=2)
    dev = device(geno)
    with pytest.raises(capi.HgError, match="W = 0"):
        dev.ld(0)
    with pytest.raises(capi.HgError, match="W = 4097"):
        dev.ld(4097, count=1)
    with pytest.raises(capi.HgError, match="out of range"):
        dev.ld(5, m0=30, count=11)


def test_large_case():
    """N = 100 003, M = 3 000, W = 300: many individual ranges and marker tiles per workgroup"""
    N, M, W = 100003, 3000, 300
    geno = make(N, M, seed=9)
    dev = device(geno)
    r, s = dev.ld(W)
    ref_s, ref_r = reference(geno, W, block=256)
    assert np.array_equal(s, ref_s)
    ok = ~np.isnan(ref_r)
    assert np.array_equal(np.isnan(r), ~ok) and np.max(np.abs(r[ok] - ref_r[ok])) <= 1e-12
    dev.set_option("ld_split", 1)  # every workgroup runs all 196 slices of individuals
    r1, s1 = dev.ld(W, m0=1000, count=700)
    assert same_bits(r1, r[1000:1700]) and np.array_equal(s1, s[1000:1700])


def test_cli_table_and_band(tmp_path):
    N, M, W, T, KB = 400, 60, 12, 0.05, 0.02  # (bp 20 apart at most 20: the kb limit cuts some pairs)
    geno = make(N, M, seed=21)
    y = np.random.default_rng(4).standard_normal(N)
    na = [3, 50, 51, 399]
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=na)
    chrom = ["1" if j < 25 else "2" for j in range(M)]
    bp = np.cumsum(np.random.default_rng(6).integers(1, 15, size=M)) + 1000
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%s snp%d 0 %d A C\n" % (chrom[j], j, bp[j]))
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", out,
                        "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(M), "--ld-window", str(W),
                        "--ld-window-kb", str(KB), "--ld-window-r2", str(T), "--ld-bin"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    kept_rows = np.setdiff1d(np.arange(N), na)
    _, ref_r = reference(geno[:, kept_rows], W)
    inwin = np.zeros((M, W), dtype=bool)
    for j in range(M):
        for d in range(1, W + 1):
            q = j + d
            inwin[j, d - 1] = q < M and chrom[q] == chrom[j] and abs(bp[q] - bp[j]) <= 1000 * KB
    keep = inwin & ~np.isnan(ref_r)
    assert "2 chromosomes, %d pairs in the window" % int(inwin.sum()) in r.stdout
    # both limits cut pairs here: the chromosome boundary and the kb limit
    assert any(chrom[j + d] != chrom[j] for j in range(M - W) for d in range(1, W + 1))
    assert any(chrom[j + d] == chrom[j] and abs(bp[j + d] - bp[j]) > 1000 * KB for j in range(M - W) for d in range(1, W + 1))
    # the .ld table: every kept pair with r^2 >= T, nothing else (pairs within 1e-9 of the threshold may go either way)
    with open(out + "/n.ld") as f:
        assert f.readline().split() == ["CHR_A", "BP_A", "SNP_A", "CHR_B", "BP_B", "SNP_B", "R"]
        got = {}
        for line in f:
            ca, ba, sa, cb, bb, sb, rv = line.split()
            j, q = int(sa[3:]), int(sb[3:])
            assert (ca, int(ba), cb, int(bb)) == (chrom[j], bp[j], chrom[q], bp[q])
            got[(j, q)] = float(rv)
    want = {(j, j + d + 1): ref_r[j, d] for j in range(M) for d in range(W) if keep[j, d] and ref_r[j, d] ** 2 >= T}
    near = {(j, j + d + 1) for j in range(M) for d in range(W) if keep[j, d] and abs(ref_r[j, d] ** 2 - T) < 1e-9}
    assert set(got) - near == set(want) - near
    assert len(want) > 10
    for k, v in want.items():
        if k in got:
            assert abs(got[k] - v) <= 1e-9 * max(1.0, abs(v)), k
    # the band
    raw = np.fromfile(out + "/n.ld.bin", dtype=np.uint8)
    assert tuple(raw[:8].view(np.uint32)) == (M, W)
    band = raw[8:].view(np.float32).reshape(M, W)
    assert np.array_equal(np.isnan(band), ~keep)
    assert np.all(np.abs(band[keep] - ref_r[keep]) <= 1e-7)  # f32 rounding of r (|r| <= 1: half an ulp is at most 2^-25)
