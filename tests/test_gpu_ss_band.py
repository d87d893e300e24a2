"""hgibbs_ss_begin's band equals (n_eff - 1) r of hgibbs_ld bit for bit inside the window, and is 0 outside it
and wherever r is NaN (a marker without a finite standard deviation has an all-zero row and column)."""
import numpy as np
import pytest

from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu

M, N = 150, 203


@pytest.fixture(scope="module")
def panel():
    geno = synth.make_genotypes(M, N, seed=31, missing_rate=0.02)
    geno[17, :] = np.where(geno[17, :] == 3, 3, 2)  # monomorphic: no finite standard deviation
    bed = synth.pack_bed_columns(geno)
    dev = capi.Device(0)
    dev.load_bed(bed, N)
    _, mstd, _, _, _ = dev.marker_stats()
    assert not np.isfinite(mstd[17]) and np.isfinite(np.delete(mstd, 17)).all()
    return dev


def expected(dev, n_eff, W, ahead):
    r, _ = dev.ld(W, sums=False)
    want = (n_eff - 1.0) * r
    d = np.arange(1, W + 1)[None, :]
    want[(d > ahead[:, None]) | np.isnan(r)] = 0.0
    return want


def chrom_ahead(W, ends):
    """windows of W markers that end at the chromosome ends `ends` (one past the last marker of each)"""
    ah = np.zeros(M, dtype=np.uint32)
    lo = 0
    for e in ends:
        j = np.arange(lo, e)
        ah[lo:e] = np.minimum(W, e - 1 - j)
        lo = e
    return ah


@pytest.mark.parametrize("W,ends,n_eff", [(1, (M,), N), (7, (40, 41, 100, M), 5000.0), (64, (90, M), 777.0), (300, (M,), N)])
def test_band_is_scaled_ld_bit_for_bit(panel, W, ends, n_eff):
    """W = 1; windows that end at chromosome ends (ahead = 0 at each last marker, a chromosome of one marker); W larger than the
    markers left; n_eff other than the panel's row count"""
    dev = panel
    ahead = chrom_ahead(W, ends)
    assert all(ahead[e - 1] == 0 for e in ends)
    dev.ss_begin(n_eff, W, np.zeros(M), ahead)
    got = dev.ss_band()
    want = expected(dev, float(n_eff), W, ahead)
    assert got.shape == (M, W) and np.array_equal(got, want)
    assert not got[17].any() and got[16, 0] == 0.0 and (W < 2 or got[15, 1] == 0.0)
    assert np.array_equal(dev.ss_band(33, 9), want[33:42])  # a range of rows
    if W == 300:  # ahead = NULL is min(W, M - 1 - j)
        dev.ss_begin(n_eff, W, np.zeros(M))
        assert np.array_equal(dev.ss_band(), want)
    assert dev.last_ss_ms()[0] > 0.0
    dev.ss_end()


def test_begin_sets_state_and_refuses_by_name(panel):
    dev = panel
    xty = np.linspace(-3, 3, M)
    dev.set_model(np.zeros(M, dtype=np.int32), np.array([[0.0, 0.01]]), np.array([[0.0, 100.0]]))
    dev.set_beta(np.ones(M))
    dev.ss_begin(500.0, 4, xty)
    c, sb, sc = dev.ss_state()
    assert np.array_equal(c, xty) and sb == 0.0 and sc == 0.0
    beta, comp, acum = dev.get_beta()
    assert not beta.any() and not comp.any()
    for kw, msg in ((dict(W=0), "W = 0"), (dict(W=4097), "W = 4097"), (dict(n_eff=1.5), "n_eff"), (dict(n_eff=float("inf")), "n_eff"),
                    (dict(xty=np.where(np.arange(M) == 3, np.nan, 0.0)), "xty[3] is not finite"),
                    (dict(ahead=np.full(M, 2, dtype=np.uint32)), "past the last marker"),
                    (dict(ahead=np.where(np.arange(M) == 0, 5, 0).astype(np.uint32)), "above W")):
        a = dict(dict(n_eff=500.0, W=4, xty=xty, ahead=None), **kw)
        with pytest.raises(capi.HgError) as e:
            dev.ss_begin(a["n_eff"], a["W"], a["xty"], a["ahead"])
        assert msg in str(e.value), str(e.value)
    assert np.array_equal(dev.ss_state()[0], xty)  # a refused call leaves the state of the last good one
    dev.ss_end()
    with pytest.raises(capi.HgError) as e:
        dev.ss_state()
    assert "hgibbs_ss_begin first" in str(e.value)
    empty = capi.Device(0)
    with pytest.raises(capi.HgError) as e:
        empty.M = M
        empty.ss_begin(500.0, 4, xty)
    assert "no genotypes loaded" in str(e.value)


def test_several_ranks_refused():
    geno = synth.make_genotypes(8, 64, seed=2)
    dev = capi.Device(0)
    dev.comm_init_external(2, 0, lambda arr: None)  # a stub world of two ranks
    dev.load_bed(synth.pack_bed_columns(geno), 64, row_begin=0, row_end=32, n_global=64)
    with pytest.raises(capi.HgError, match=r"hgibbs_ss_begin: one rank only \(this handle has 2\)"):
        dev.ss_begin(64.0, 2, np.zeros(8))
