"""LD masks (hgibbs_ld_mask) and the selection on them (hgibbs_ld_clump): exact against the device's own band (hgibbs_ld's r), the edge of
the threshold, NumPy's r (tests/test_gpu_ld.py's reference), irregular windows, bit identity across pieces, splits and launches, and
hgibbs_ld_clump against the masks and the Python walk of tests/ldwalk.py."""
import os
import sys

import numpy as np
import pytest

from hydra_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldwalk  # noqa: E402
import orc  # noqa: E402
from test_gpu_ld import GRID_M, GRID_W, make_grid  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1001, 333), (257, 97)]
WINDOWS = [1, 15, 63, 64, 65, 130, 300]
THRESHOLDS = [0.0, 0.2, 0.5]
NUMPY_CASES = [(1001, 333, 130), (257, 97, 65)]  # (N, M, W) of test_against_numpy; the data's seed is N + M as everywhere here


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
    """r (M, W) f64: r[j, d - 1] = x_j'x_{j + d} / (N - 1), NaN past M or where an mstd is not finite (tests/test_gpu_ldscore.py's
    reference_r, restated)"""
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


def make(N, M, seed, missing_cols=True):
    """tests/test_gpu_ldscore.py's data: LD neighbours, 1-5 % missing calls in a fifth of the columns, an all-but-one-missing column, a
    monomorphic column"""
    geno = synth.make_genotypes(M, N, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for j in range(1, M, 3):
        redraw = rng.random(N) < 0.2
        geno[j] = np.where(redraw, geno[j], geno[j - 1])
    if missing_cols:
        for j in rng.choice(M, size=M // 5, replace=False):
            geno[j, rng.random(N) < rng.uniform(0.01, 0.05)] = 3
        geno[M // 3] = 3
        geno[M // 3, N // 2] = 1
        geno[M // 2] = 1
    return geno


def device(geno):
    M, N = geno.shape
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    dev.marker_stats()
    return dev


def default_ahead(M, W):
    return np.minimum(W, M - 1 - np.arange(M)).astype(np.uint32)


def band_from_r(r, ahead, t):
    """the forward band (M, W) bool of a band of r: in the window, not NaN, r * r >= t in f64"""
    M, W = r.shape
    inwin = np.arange(1, W + 1)[None, :] <= ahead[:, None]
    with np.errstate(invalid="ignore"):
        return inwin & ~np.isnan(r) & (r * r >= t)


def check_masks(fwd, bwd, npass, fband, W, what):
    got_f, pad_f = ldwalk.unpack(fwd, W)
    got_b, pad_b = ldwalk.unpack(bwd, W)
    assert not pad_f and not pad_b, "%s: a bit at an offset above W" % what
    assert np.array_equal(got_f, fband), "%s: fwd differs in %d bits" % (what, np.count_nonzero(got_f != fband))
    assert np.array_equal(got_b, ldwalk.backward_of(fband)), "%s: bwd is not the transpose of the band" % what
    assert npass == int(np.count_nonzero(fband)), what


@pytest.fixture(scope="module")
def cohorts():
    """per shape: the data, a device with it, and the device's own band at the widest window (a narrower one is its leading columns)"""
    out = {}
    for N, M in SHAPES:
        geno = make(N, M, seed=N + M)
        dev = device(geno)
        r, _ = dev.ld(max(WINDOWS), sums=False)
        r.setflags(write=False)
        out[(N, M)] = (geno, dev, r)
    return out


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("N,M", SHAPES)
def test_exact_against_the_devices_own_band(cohorts, N, M, W):
    geno, dev, rmax = cohorts[(N, M)]
    r = rmax[:, :W]
    if W in (15, 65):  # the band of a call with this W itself is those columns, bit for bit
        own, _ = dev.ld(W, sums=False)
        assert np.array_equal(own.view(np.int64), np.ascontiguousarray(r).view(np.int64))
    ahead = default_ahead(M, W)
    nan = np.isnan(r) & (np.arange(1, W + 1)[None, :] <= ahead[:, None])
    assert nan.any()  # the monomorphic column's pairs: NaN never passes, at t = 0 either
    for t in THRESHOLDS:
        fband = band_from_r(r, ahead, t)
        assert not (fband & nan).any()
        fwd, bwd, npass = dev.ld_mask(W, t)
        check_masks(fwd, bwd, npass, fband, W, "N=%d M=%d W=%d t=%g" % (N, M, W, t))
        only_f, none, n2 = dev.ld_mask(W, t, backward=False)
        assert none is None and n2 == npass and np.array_equal(only_f, fwd)


def test_the_thresholds_edge(cohorts):
    """with t = r * r the pair's bit is set, with the next f64 above it is clear"""
    N, M = SHAPES[0]
    geno, dev, rmax = cohorts[(N, M)]
    W = 65
    r = rmax[:, :W]
    ahead = default_ahead(M, W)
    for j, d in [(1, 1), (0, 64), (100, 65), (255, 3), (M - 2, 1)]:
        v = float(r[j, d - 1])
        assert v == v and d <= ahead[j]
        t = v * v
        for tt, want in [(t, True), (np.nextafter(t, 2.0), False)]:
            fwd, bwd, npass = dev.ld_mask(W, tt)
            assert bool((int(fwd[j, (d - 1) // 64]) >> ((d - 1) % 64)) & 1) == want, (j, d, tt)
            assert bool((int(bwd[j + d, (d - 1) // 64]) >> ((d - 1) % 64)) & 1) == want, (j, d, tt)
            check_masks(fwd, bwd, npass, band_from_r(r, ahead, tt), W, "edge")


@pytest.mark.parametrize("N,M,W", NUMPY_CASES)
def test_against_numpy(N, M, W):
    """The masks from NumPy's r.  tests/test_gpu_ld.py pins the device's r to 1e-12 of this reference, so r^2 is within about 2e-12 of the
    reference's; the test first asserts that no in-window finite pair of the REFERENCE lies within 1e-9 of a threshold, three orders of
    margin, and then compares every bit: no pair is excluded.
    Margins of the reference alone, found on the CPU for these seeds (min over all in-window finite pairs of |r_ref^2 - t|):
    N = 1001, M = 333, W = 130: 2.02e-3 at t = 0.2 and 5.44e-5 at t = 0.5 (34 275 pairs, 107 and 87 of them pass);
    N = 257, M = 97, W = 65: 5.69e-2 at t = 0.2 and 2.29e-2 at t = 0.5 (3 969 pairs, 31 and 29 pass)."""
    geno = make(N, M, seed=N + M)
    r, finite = reference_r(geno, W)
    ahead = default_ahead(M, W)
    inwin = (np.arange(1, W + 1)[None, :] <= ahead[:, None]) & ~np.isnan(r)
    assert np.array_equal(~np.isnan(r), finite[:, None] & ~np.isnan(r)) and not finite.all()
    dev = device(geno)
    for t in (0.2, 0.5):
        margin = float(np.min(np.abs(r[inwin] ** 2 - t)))
        print("N=%d M=%d W=%d t=%g: min |r_ref^2 - t| = %.3g over %d pairs" % (N, M, W, t, margin, np.count_nonzero(inwin)))
        assert margin > 1e-9, "the precondition on the reference fails: choose another seed"
        fwd, bwd, npass = dev.ld_mask(W, t)
        check_masks(fwd, bwd, npass, band_from_r(r, ahead, t), W, "numpy N=%d M=%d W=%d t=%g" % (N, M, W, t))
    fwd, bwd, npass = dev.ld_mask(W, 0.0)  # t = 0: every in-window pair with a finite r, whatever its value
    check_masks(fwd, bwd, npass, inwin, W, "numpy t=0")


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
    return ahead, ends


def test_irregular_windows():
    N, M, W = 1501, 230, 70
    geno = make(N, M, seed=8)
    dev = device(geno)
    ahead, ends = irregular_ahead(M, W, seed=1)
    assert ahead[0] == 0 and np.count_nonzero(ahead == 0) > 5 and 64 < ahead.max() <= W  # (two words a row)
    r, _ = dev.ld(W, sums=False)
    chrom = np.searchsorted(np.array(ends), np.arange(M), side="right")
    for t in (0.0, 0.2):
        fband = band_from_r(r, ahead, t)
        fwd, bwd, npass = dev.ld_mask(W, t, ahead=ahead)
        check_masks(fwd, bwd, npass, fband, W, "irregular t=%g" % t)  # (bwd = the transpose: fwd and bwd are twins)
        got_f, _ = ldwalk.unpack(fwd, W)
        got_b, _ = ldwalk.unpack(bwd, W)
        for j, d in zip(*np.nonzero(got_f)):
            assert chrom[j] == chrom[j + d + 1], "a forward bit crosses a break"
        for q, d in zip(*np.nonzero(got_b)):
            assert chrom[q] == chrom[q - d - 1], "a backward bit crosses a break"
    assert npass > 0


@pytest.mark.parametrize("clean", [False, True])
def test_bit_identity_and_options(clean):
    """M = 333 at piece 16 puts a window and its backward targets across several pieces and tiles; clean data takes k_ld<false>"""
    N, M, W = 1001, 333, 130
    geno = make(N, M, seed=3, missing_cols=not clean)
    dev = device(geno)
    f0, b0, n0 = dev.ld_mask(W, 0.2)
    r, _ = dev.ld(W, sums=False)
    check_masks(f0, b0, n0, band_from_r(r, default_ahead(M, W), 0.2), W, "clean=%s" % clean)
    assert n0 > 50

    def same():
        f, b, n = dev.ld_mask(W, 0.2)
        return np.array_equal(f, f0) and np.array_equal(b, b0) and n == n0

    assert same()
    for piece in (16, 48, 64, 0):
        dev.set_option("ldmask_piece", piece)
        assert same(), piece
    for split in (1, 3, 1000, 0):
        dev.set_option("ld_split", split)
        assert same(), split
    dev.set_option("ldmask_piece", 16)
    dev.set_option("ld_split", 3)
    assert same()
    products, reduce = dev.last_ld_mask_ms()
    assert products > 0.0 and reduce > 0.0
    for bad in (-1, (1 << 20) + 1):
        with pytest.raises(capi.HgError, match="ldmask_piece"):
            dev.set_option("ldmask_piece", bad)


def test_ld_clump_equals_the_mask_and_the_python_walk(cohorts):
    N, M = SHAPES[0]
    geno, dev, rmax = cohorts[(N, M)]
    W, t = 65, 0.2
    rng = np.random.default_rng(4)
    order = rng.permutation(M).astype(np.uint32)[:(3 * M) // 4]
    may = (rng.random(M) < 0.5).astype(np.uint8)
    fwd, bwd, npass = dev.ld_mask(W, t)
    fband, _ = ldwalk.unpack(fwd, W)
    bband, _ = ldwalk.unpack(bwd, W)
    A = ldwalk.adjacency(fband, bband)
    for ml in (may, None):
        owner, n = dev.ld_clump(W, t, order, may_lead=ml)
        assert n == npass
        assert np.array_equal(owner, ldwalk.walk(A, order, ml))
        assert np.array_equal(owner, capi.ld_greedy(M, W, fwd, bwd, order, ml))
        # the four properties against hgibbs_ld's r itself
        fr = band_from_r(rmax[:, :W], default_ahead(M, W), t)
        ldwalk.check_properties(ldwalk.adjacency(fr, ldwalk.backward_of(fr)), order, owner, ml)
        assert np.count_nonzero((owner != -1) & (owner != np.arange(M))) > 10
    assert dev.last_ld_mask_ms()[0] > 0.0
    with pytest.raises(capi.HgError, match="is in the order twice"):
        dev.ld_clump(W, t, np.array([1, 1], dtype=np.uint32))
    with pytest.raises(capi.HgError, match="hgibbs_ld_mask: t = -1"):
        dev.ld_clump(W, -1.0, order)


@pytest.mark.parametrize("N", [2, 16, 17, 513])
def test_edge_grid_against_the_devices_own_band(N):
    """tests/test_gpu_ld.py's grid of markers and windows (W = 4096: 64 words a marker), exactly, against the device's own band, which
    that file holds to NumPy's at the same shapes"""
    for M in GRID_M:
        geno = make_grid(N, M, seed=N + M)
        dev = device(geno)
        band, _ = dev.ld(max(GRID_W), sums=False)
        for W in GRID_W:
            ahead = default_ahead(M, W)
            for t in (0.0, 0.2):
                fwd, bwd, npass = dev.ld_mask(W, t)
                assert fwd.shape == (M, (W + 63) // 64)
                check_masks(fwd, bwd, npass, band_from_r(band[:, :W], ahead, t), W, "N=%d M=%d W=%d t=%g" % (N, M, W, t))
        dev.close()


def test_refusals():
    geno = make(300, 40, seed=2)
    dev = device(geno)
    M = 40
    for t in (-0.5, float("nan"), float("inf")):
        with pytest.raises(capi.HgError, match="the threshold on r\\^2 must be finite and >= 0"):
            dev.ld_mask(5, t)
    with pytest.raises(capi.HgError, match="W = 0"):
        dev.ld_mask(0, 0.2)
    with pytest.raises(capi.HgError, match="W = 4097"):
        dev.ld_mask(4097, 0.2)
    ahead = default_ahead(M, 5)
    bad = ahead.copy()
    bad[3] = 6
    with pytest.raises(capi.HgError, match=r"ahead\[3\] = 6 is above W = 5"):
        dev.ld_mask(5, 0.2, ahead=bad)
    bad = ahead.copy()
    bad[M - 2] = 2
    with pytest.raises(capi.HgError, match="past the last marker"):
        dev.ld_mask(5, 0.2, ahead=bad)
    assert dev.L.hgibbs_ld_mask(dev.h, 5, None, 0.2, None, None, None) != 0
    assert "null output (fwd)" in dev.L.hgibbs_last_error().decode()
    empty = capi.Device(0)
    z = np.zeros((1, 1), dtype=np.uint64)
    assert empty.L.hgibbs_ld_mask(empty.h, 5, None, 0.2, z.ctypes.data_as(capi.C_U64P), None, None) != 0
    assert "no genotypes loaded" in empty.L.hgibbs_last_error().decode()
