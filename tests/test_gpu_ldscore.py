"""LD scores (hgibbs_ld_scores, hydra_mi355x --ld-score) against NumPy: r as in tests/test_gpu_ld.py's reference, the term t, the sums
forwards and backwards in f64 with the same ahead / annot rules; bit identity across pieces, splits and launches; the CLI's files.

Tolerance.  tests/test_gpu_ld.py pins the device's r to within 1e-12 of this reference, so |dt| <= 2 |r| (1 + 1 / (N - 2)) 1e-12 <= 2.1e-12
for N >= 22; the fixed-point rounding adds 2^-45 a term.  Hence |l - l_ref| <= 3e-12 x (terms of the marker's window, self included)."""
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
from test_gpu_ld import GRID_M, GRID_W, make_grid  # noqa: E402

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


def reference_r(geno, W, block=64):
    """r (M, W) f64: r[j, d - 1] = x_j'x_{j + d} / (N - 1), NaN past M or where an mstd is not finite (tests/test_gpu_ld.py's reference)"""
    M, N = geno.shape
    g = np.where(geno == 3, 0, geno).astype(np.float64)
    mave, mstd = oracle_stats(geno)
    with np.errstate(invalid="ignore"):
        x = np.where(geno == 3, 0.0, (g - mave[:, None]) * mstd[:, None])
    fin = np.isfinite(mstd)
    r = np.full((M, W), np.nan)
    for j0 in range(0, M, block):
        j1 = min(M, j0 + block)
        q1 = min(M, j1 + W)
        with np.errstate(invalid="ignore"):
            X = x[j0:j1] @ x[j0:q1].T / (N - 1)
        X[~fin[j0:j1], :] = np.nan  # (a column with no call at all: x = 0 everywhere, tests/test_gpu_ld.py's reference)
        X[:, ~fin[j0:q1]] = np.nan
        for jj in range(j1 - j0):
            nd = min(W, M - 1 - (j0 + jj))
            r[j0 + jj, :nd] = X[jj, jj + 1:jj + 1 + nd]
    return r, np.isfinite(mstd)


def default_ahead(M, W):
    return np.minimum(W, M - 1 - np.arange(M)).astype(np.uint32)


def scores_from_r(r, finite, N, ahead, annot, C, adjust):
    """l2 (M, C) and the number of terms (M,) (self included) from a band r (M, W): t per pair, summed forwards and backwards in f64"""
    M = r.shape[0]
    A = ((annot[:, None] >> np.arange(C, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.float64)
    l2 = A.copy()
    terms = np.ones(M, dtype=np.int64)
    for j in range(M):
        n = int(ahead[j])
        if n == 0:
            continue
        terms[j] += n
        terms[j + 1:j + 1 + n] += 1
        rr = r[j, :n]
        ok = ~np.isnan(rr)
        r2 = np.where(ok, rr, 0.0) ** 2
        t = r2 - (1.0 - r2) / (N - 2) if adjust else r2
        t = np.where(ok, t, 0.0)
        l2[j] += t @ A[j + 1:j + 1 + n]
        l2[j + 1:j + 1 + n] += t[:, None] * A[j][None, :]
    l2[~finite] = np.nan
    return l2, terms


def reference(geno, W, ahead=None, annot=None, C=1, adjust=True, block=64):
    M, N = geno.shape
    r, finite = reference_r(geno, W, block)
    if ahead is None:
        ahead = default_ahead(M, W)
    if annot is None:
        annot = np.ones(M, dtype=np.uint64)
    return scores_from_r(r, finite, N, ahead, annot, C, adjust)


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
        geno[M // 2] = 1  # monomorphic (NaN row, contributes to nobody)
    return geno


def device(geno):
    M, N = geno.shape
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    dev.marker_stats()
    return dev


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def close(got, ref, terms, what=""):
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN pattern differs" % (what,)
    ok = ~np.isnan(ref)
    err = np.abs(np.where(ok, got - ref, 0.0))
    bound = 3e-12 * terms[:, None]
    worst = float(np.max(err / bound))
    print("%s: largest |l - l_ref| / (3e-12 x terms) = %.3g" % (what, worst))
    assert np.all(err <= bound), "%s: beyond 3e-12 x terms (%.3g of the bound)" % (what, worst)


@pytest.mark.parametrize("N,M", [(1001, 333), (4099, 97)])
def test_shapes(N, M):
    geno = make(N, M, seed=N + M)
    dev = device(geno)
    for W in (1, 15, 16, 17, 65, 300):
        r, finite = reference_r(geno, W)
        one = np.ones(M, dtype=np.uint64)
        for adjust in (True, False):
            ref, terms = scores_from_r(r, finite, N, default_ahead(M, W), one, 1, adjust)
            assert np.all(np.isnan(ref[M // 2]))  # the monomorphic marker
            close(dev.ld_scores(W, adjust=adjust), ref, terms, "N=%d M=%d W=%d adjust=%s" % (N, M, W, adjust))


def test_clean_data():
    """no missing call anywhere (k_ld<false>), N one past a multiple of 4096"""
    N, M = 4097, 150
    geno = make(N, M, seed=5, missing_cols=False)
    dev = device(geno)
    for W in (3, 40):
        ref, terms = reference(geno, W)
        close(dev.ld_scores(W), ref, terms, "W=%d" % W)


def irregular_ahead(M, W, seed):
    """ahead per "chromosome": runs that end inside tiles of 16 and 64, single-marker runs, widths that differ between neighbours"""
    rng = np.random.default_rng(seed)
    ends, j = [], 0
    for n in [1, 37, 1, 1, 90, 21]:
        j += n
        ends.append(j)
    ends.append(M)
    ahead = np.zeros(M, dtype=np.uint32)
    j0 = 0
    for e in ends:
        for j in range(j0, e):
            ahead[j] = min(int(rng.integers(0, W + 1)), e - 1 - j)
        j0 = e
    return ahead


def test_irregular_windows():
    N, M, W = 1501, 230, 45
    geno = make(N, M, seed=8)
    dev = device(geno)
    ahead = irregular_ahead(M, W, seed=1)
    assert ahead[0] == 0 and np.count_nonzero(ahead == 0) > 5 and ahead.max() == W
    assert np.any(np.abs(np.diff(ahead.astype(np.int64))) > 5)
    ref, terms = reference(geno, W, ahead=ahead)
    got = dev.ld_scores(W, ahead=ahead)
    close(got, ref, terms, "irregular")
    # symmetry: a pair counts for both markers or for neither.  One marker q in an annotation of its own: column 1 of marker j holds
    # t_jq exactly when (j, q) is a pair, and column 0 of q sums those same terms
    r, finite = reference_r(geno, W)
    for q in (40, 41, 128, 200):
        annot = np.ones(M, dtype=np.uint64)
        annot[q] |= np.uint64(2)
        l2 = dev.ld_scores(W, ahead=ahead, annot=annot, C=2, adjust=False)
        inwin = np.array([(j < q and q - j <= ahead[j]) or (q < j and j - q <= ahead[q]) for j in range(M)])
        fin = ~np.isnan(l2[:, 1])
        assert finite[q]
        touched = (l2[:, 1] != 0) & fin
        touched[q] = False
        assert not np.any(touched & ~inwin), q  # nobody outside q's pairs saw q
        back = np.where(fin & inwin, l2[:, 1], 0.0).sum()  # what q gave to its pairs' other markers
        assert abs((l2[q, 0] - 1.0) - back) <= 3e-12 * terms[q], q  # equals what they gave to q


@pytest.mark.parametrize("C", [3, 64])
def test_annotations(C):
    N, M, W = 1201, 200, 70
    geno = make(N, M, seed=12)
    dev = device(geno)
    rng = np.random.default_rng(C)
    annot = np.zeros(M, dtype=np.uint64)
    empty = 1  # annotation 1 holds nobody
    for c in range(C):
        if c == empty:
            continue
        annot |= (rng.random(M) < (0.5 if C == 3 else 0.12)).astype(np.uint64) << np.uint64(c)
    annot[7] = 0  # a marker in no annotation
    annot[M // 2] |= np.uint64(1) << np.uint64(C - 1)  # the monomorphic marker inside annotations (bit 63 for C = 64)
    annot[M // 2] |= np.uint64(1)
    annot[11] |= np.uint64(1) << np.uint64(C - 1)
    ref, terms = reference(geno, W, annot=annot, C=C)
    got = dev.ld_scores(W, annot=annot, C=C)
    close(got, ref, terms, "C=%d" % C)
    fin = ~np.isnan(ref[:, 0])
    assert np.all(got[fin, empty] == 0.0) and np.all(np.isnan(got[~fin, empty])) and not fin[M // 2]
    if C == 64:
        for c in (0, 1, 31, 32, 63):
            one = dev.ld_scores(W, annot=(annot >> np.uint64(c)) & np.uint64(1), C=1)
            assert same_bits(one[:, 0], got[:, c]), c


def test_bit_identity_and_options():
    N, M, W, C = 3001, 260, 70, 3
    geno = make(N, M, seed=3)
    dev = device(geno)
    rng = np.random.default_rng(2)
    annot = rng.integers(0, 8, size=M).astype(np.uint64)
    l0 = dev.ld_scores(W, annot=annot, C=C)
    assert same_bits(l0, dev.ld_scores(W, annot=annot, C=C))
    for piece in (16, 48, 64, 0):  # a window of 70 spans three or more pieces of 16; pieces of 48 end inside a tile of 64
        dev.set_option("ldscore_piece", piece)
        assert same_bits(l0, dev.ld_scores(W, annot=annot, C=C)), piece
    for split in (1, 3, 1000, 0):
        dev.set_option("ld_split", split)
        assert same_bits(l0, dev.ld_scores(W, annot=annot, C=C)), split
    dev.set_option("ldscore_piece", 16)
    dev.set_option("ld_split", 3)
    assert same_bits(l0, dev.ld_scores(W, annot=annot, C=C))
    for bad in (-1, (1 << 20) + 1):
        with pytest.raises(capi.HgError, match="ldscore_piece"):
            dev.set_option("ldscore_piece", bad)


def test_against_the_devices_own_band():
    """adjust off, no annotations: the sum of hgibbs_ld's r^2 over the same pairs differs by the fixed-point rounding only"""
    N, M, W = 2003, 190, 33
    geno = make(N, M, seed=17)
    dev = device(geno)
    r, _ = dev.ld(W, sums=False)
    ahead = default_ahead(M, W)
    _, finite = reference_r(geno, 1)
    ref, terms = scores_from_r(r, finite, N, ahead, np.ones(M, dtype=np.uint64), 1, False)
    got = dev.ld_scores(W, adjust=False)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    # (the host's own f64 summation of up to 67 terms below 1 each rounds too: at most terms x 2^-53 x l, far below 2^-44 a term)
    assert np.all(np.abs(got - ref)[ok] <= (terms[:, None] * 2.0 ** -44)[ok])


@pytest.mark.parametrize("N", [2, 16, 17, 513])
def test_edge_grid_against_the_devices_own_band(N):
    """tests/test_gpu_ld.py's grid of markers and windows (W = 4096: 64 reduce tiles a row): the scores of the device's own band, which
    that file holds to NumPy's at the same shapes.  The terms are the band's own, so only the fixed point (2^-45 a term) and the
    summation here differ: far inside close()'s 3e-12 x terms.  N = 2 without the adjustment, which needs N >= 3."""
    for M in GRID_M:
        geno = make_grid(N, M, seed=N + M)
        dev = device(geno)
        band, _ = dev.ld(max(GRID_W), sums=False)
        _, finite = reference_r(geno, 1)
        one = np.ones(M, dtype=np.uint64)
        three = np.random.default_rng(N + M).integers(0, 8, size=M).astype(np.uint64)
        for W in GRID_W:
            ahead = default_ahead(M, W)
            for adjust in ((True, False) if N >= 3 else (False,)):
                for annot, C in ((one, 1), (three, 3)):
                    ref, terms = scores_from_r(band[:, :W], finite, N, ahead, annot, C, adjust)
                    got = dev.ld_scores(W, annot=annot if C > 1 else None, C=C, adjust=adjust)
                    close(got, ref, terms, "N=%d M=%d W=%d C=%d adjust=%s" % (N, M, W, C, adjust))
        dev.close()


def test_refusals():
    geno = make(300, 40, seed=2)
    dev = device(geno)
    M = 40
    with pytest.raises(capi.HgError, match="W = 0"):
        dev.ld_scores(0)
    with pytest.raises(capi.HgError, match="W = 4097"):
        dev.ld_scores(4097)
    ahead = default_ahead(M, 5)
    bad = ahead.copy()
    bad[3] = 6
    with pytest.raises(capi.HgError, match=r"ahead\[3\] = 6 is above W = 5"):
        dev.ld_scores(5, ahead=bad)
    bad = ahead.copy()
    bad[M - 2] = 2
    with pytest.raises(capi.HgError, match="past the last marker"):
        dev.ld_scores(5, ahead=bad)
    annot = np.ones(M, dtype=np.uint64)
    with pytest.raises(capi.HgError, match="C = 0"):
        dev.ld_scores(5, annot=annot, C=0)
    with pytest.raises(capi.HgError, match="C = 65"):
        dev.ld_scores(5, annot=annot, C=65)
    annot[9] = 4
    with pytest.raises(capi.HgError, match=r"annot\[9\] has a bit at or above C = 2"):
        dev.ld_scores(5, annot=annot, C=2)
    assert dev.ld_scores(5, annot=annot, C=3).shape == (M, 3)
    # a three-row cohort whose phenotype-less row is gone: N = 2, the adjusted term divides by N - 2
    small = capi.Device(0)
    small.load_bed(synth.pack_bed_columns(geno[:, :2]), 2)
    with pytest.raises(capi.HgError, match="needs N >= 3"):
        small.ld_scores(5)


def test_large_case():
    """N = 100 003, M = 3 000, W = 300, C = 2: many individual ranges, and several pieces"""
    N, M, W, C = 100003, 3000, 300, 2
    geno = make(N, M, seed=9)
    dev = device(geno)
    annot = (np.arange(M) % 3 != 0).astype(np.uint64) | ((np.arange(M) % 5 < 2).astype(np.uint64) << np.uint64(1))
    dev.set_option("ldscore_piece", 1024)
    got = dev.ld_scores(W, annot=annot, C=C)
    ref, terms = reference(geno, W, annot=annot, C=C, block=256)
    close(got, ref, terms, "large")
    products, reduce = dev.last_ld_scores_ms()
    print("products %.3f ms, reduce %.3f ms" % (products, reduce))
    assert products > 0.0 and reduce > 0.0


def read_ldscore(path):
    with open(path) as f:
        header = f.readline().rstrip("\n").split("\t")
        rows = [line.rstrip("\n").split("\t") for line in f]
    return header, rows


def test_cli(tmp_path):
    N, M, KB = 400, 60, 0.02
    geno = make(N, M, seed=21)
    geno[5] = np.where(np.arange(N) % 40 == 0, 1, 0)  # a rare marker: MAF 0.0125 on either side of the NA rows
    y = np.random.default_rng(4).standard_normal(N)
    na = [3, 50, 51, 399]
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=na)
    chrom = ["1" if j < 25 else "2" for j in range(M)]
    bp = np.cumsum(np.random.default_rng(6).integers(1, 15, size=M)) + 1000
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%s snp%d 0 %d A C\n" % (chrom[j], j, bp[j]))
    sets = {"early": list(range(0, 30)), "odd": list(range(1, M, 2))}  # overlapping
    with open(prefix + ".sets", "w") as f:
        for name in ("early", "odd"):
            for j in sets[name]:
                f.write("%s snp%d\n" % (name, j))
    out = str(tmp_path / "o")
    base = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", out, "--mcmc-out-name", "n",
            "--number-individuals", str(N), "--number-markers", str(M), "--ld-score"]
    r = subprocess.run(base + ["--ld-score-kb", str(KB), "--ld-score-sets", prefix + ".sets"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    kept_rows = np.setdiff1d(np.arange(N), na)
    g = geno[:, kept_rows]
    Nk = len(kept_rows)
    ahead = np.zeros(M, dtype=np.uint32)
    for j in range(M):
        q = j
        while q + 1 < M and chrom[q + 1] == chrom[j] and bp[q + 1] - bp[j] <= 1000 * KB:
            q += 1
        ahead[j] = q - j
    W = int(ahead.max())
    # both limits cut pairs: the chromosome boundary and the kb limit
    assert any(chrom[j + 1] != chrom[j] and bp[j + 1] - bp[j] <= 1000 * KB for j in range(M - 1))
    assert any(chrom[j + int(ahead[j]) + 1] == chrom[j] for j in range(M) if j + int(ahead[j]) + 1 < M)
    annot = np.ones(M, dtype=np.uint64)
    for c, name in enumerate(("early", "odd")):
        for j in sets[name]:
            annot[j] |= np.uint64(1) << np.uint64(c + 1)
    ref, terms = reference(g, W, ahead=ahead, annot=annot, C=3)
    assert "%d pairs in the window" % int(ahead.sum()) in r.stdout, r.stdout
    keep = ~np.isnan(ref[:, 0])
    assert not keep[M // 2]
    header, rows = read_ldscore(out + "/n.l2.ldscore")
    assert header == ["CHR", "SNP", "BP", "baseL2", "earlyL2", "oddL2"]
    assert [row[1] for row in rows] == ["snp%d" % j for j in range(M) if keep[j]]
    for row in rows:
        j = int(row[1][3:])
        assert (row[0], int(row[2])) == (chrom[j], bp[j])
        for c in range(3):
            assert abs(float(row[3 + c]) - ref[j, c]) <= max(3e-12 * terms[j], 1e-11 * abs(ref[j, c])), (j, c)
    called = g != 3
    p = np.where(called, g, 0).sum(axis=1) / (2.0 * np.maximum(1, called.sum(axis=1)))
    common = np.minimum(p, 1 - p) > 0.05
    assert np.any(keep & common) and np.any(keep & ~common)
    A = ((annot[:, None] >> np.arange(3, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)
    assert open(out + "/n.l2.M").read().split() == [str(v) for v in A[keep].sum(axis=0)]
    assert open(out + "/n.l2.M_5_50").read().split() == [str(v) for v in A[keep & common].sum(axis=0)]

    # a marker window, raw r^2, no sets: one L2 column
    out2 = str(tmp_path / "p" / "q")
    os.makedirs(str(tmp_path / "p"))
    r = subprocess.run(base + ["--ld-score-snps", "12", "--ld-score-raw", "--ld-score-out", out2], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ahead = np.zeros(M, dtype=np.uint32)
    for j in range(M):
        q = j
        while q + 1 < M and chrom[q + 1] == chrom[j] and q + 1 - j <= 12:
            q += 1
        ahead[j] = q - j
    ref, terms = reference(g, 12, ahead=ahead, adjust=False)
    header, rows = read_ldscore(out2 + ".l2.ldscore")
    assert header == ["CHR", "SNP", "BP", "L2"]
    assert [row[1] for row in rows] == ["snp%d" % j for j in range(M) if keep[j]]
    for row in rows:
        j = int(row[1][3:])
        assert abs(float(row[3]) - ref[j, 0]) <= max(3e-12 * terms[j], 1e-11 * abs(ref[j, 0])), j
    assert open(out2 + ".l2.M").read().split() == [str(int(keep.sum()))]
