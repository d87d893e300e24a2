"""hgibbs_set_gram against the restatement of tests/settest_restate.py: the raw sums against exact Python integers bit for bit, out
within ten times the restatement's float64 / longdouble difference, on a grid of set sizes (1, 15, 16, 17, 33 and 1024 markers) and
cohort sizes, clean and with missing calls; bit-identity across batching, set order, sgram_split and repeats; the diagonal against
hgibbs_marker_class_sums' x'Wx; every refusal."""
import numpy as np
import pytest

from hydra_amd import capi, synth

import settest_restate as S

pytestmark = pytest.mark.gpu

# Ten times the largest |float64 - longdouble| of out in the restatement over this grid, relative to the sum of the absolute terms of
# the combination (tests/test_settest_restatement_cpu.py measures 3.85e-16 and pins S.OUT_F64_LD).  The device evaluates the same
# expression in the same order in f64 on the same rounded sums and the device's own mave and mstd, which the restatement is given.
# Measured on an MI355X: 0 on every entry of the grid (the device's out equals the float64 restatement bit for bit).
TOL_OUT = 10 * S.OUT_F64_LD


def device(geno):
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), geno.shape[1])
    return dev


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.int64), np.asarray(y).view(np.int64)) for x, y in zip(a, b)) and len(a) == len(b)


def check(dev, case, w=None):
    """raw bit for bit, out within TOL_OUT; returns (outs, raws)"""
    w = case["w"] if w is None else w
    outs, raws = dev.set_gram(case["sets"], w, raw=True)
    mave, mstd = dev.marker_stats()[:2]
    for s, idx in enumerate(case["sets"]):
        want = S.raw_floats(case["geno"], idx, w)
        bad = np.argwhere(raws[s].view(np.int64) != want.view(np.int64))
        assert bad.size == 0, "set %d: raw sums differ from the exact integers rounded once, first at (a, b, sum) %s" % (s, bad[:1])
        ref, scale = S.gram_out(want, mave[idx], mstd[idx])
        assert np.array_equal(np.isnan(outs[s]), np.isnan(ref)), s
        ok = np.isfinite(ref)
        if ok.any():
            err = float(np.max(np.abs(outs[s][ok] - ref[ok]) / scale[ok]))
            print("set %d of %d: out differs by %.3g of the terms" % (s, len(idx), err))
            assert err <= TOL_OUT, (s, err)
    return outs, raws


@pytest.mark.parametrize("n", S.GRID_N)
@pytest.mark.parametrize("missing", [False, True])
def test_grid(n, missing):
    case = S.grid_case(n, missing)
    assert bool((case["geno"] == 3).any()) == missing
    dev = device(case["geno"])
    outs, raws = check(dev, case)
    assert dev.last_set_gram_ms() > 0.0
    # the monomorphic member of the set of 33 (and with missing calls the column missing in every row): NaN out, exact raw (checked above)
    assert np.all(np.isnan(outs[4][0])) and np.all(np.isnan(outs[4][:, 0])) and np.all(np.isfinite(raws[4]))
    assert np.all(np.isnan(outs[4][1])) == missing
    if n == 1000:  # a range boundary inside the data: two slices of 512 rows, one workgroup each
        dev.set_option("sgram_split", 2)
        assert same_bits(dev.set_gram(case["sets"], case["w"]), outs)
    dev.close()


@pytest.mark.parametrize("missing", [False, True])
def test_set_of_1024(missing):
    case = S.big_case(missing)
    dev = device(case["geno"])
    check(dev, case)
    dev.close()


@pytest.fixture(scope="module")
def cohort():
    case = S.grid_case(1000, True)
    dev = device(case["geno"])
    yield case, dev
    dev.close()


def test_integer_weights_are_exact(cohort):
    case, dev = cohort
    w = np.random.default_rng(1).integers(0, 1000, 1000).astype(np.float64)
    _, raws = check(dev, case, w)
    E, GG, GC, CC = S.raw_integers(case["geno"], case["sets"][3], w)
    for k, ints in enumerate((GG, GC, CC)):  # the sums themselves, not only their roundings: every one is below 2^53
        assert [[int(x) for x in row] for row in raws[3][:, :, k]] == [[int(x) >> E for x in row] for row in ints]


def test_weights_spanning_twelve_decades_stay_within_the_rounding_bound(cohort):
    case, dev = cohort
    w = 10.0 ** np.random.default_rng(3).uniform(-12, 0, 1000)
    _, raws = check(dev, case, w)
    E, _ = S.quantise(w)
    bound = S.rounding_bound(1000, E)
    wl = w.astype(np.longdouble)
    for s, idx in enumerate(case["sets"]):
        codes = case["geno"][idx]
        c = (codes != 3).astype(np.longdouble)
        g = np.where(codes == 3, 0, codes).astype(np.longdouble)
        for k, want in enumerate(((g * wl) @ g.T, (g * wl) @ c.T, (c * wl) @ c.T)):
            # the bound of the rounding of w, the one rounding of the sum to f64, and the longdouble reference's own summation
            slack = np.abs(want) * 2.0 ** -53 + 1000 * 4 * float(np.finfo(np.longdouble).eps)
            assert np.all(np.abs(raws[s][:, :, k] - want) <= bound[k] + slack), (s, k)


def test_bit_identical_across_batching_order_splits_and_repeats(cohort):
    case, dev = cohort
    dev.set_option("sgram_split", 0)
    outs, raws = dev.set_gram(case["sets"], case["w"], raw=True)
    again = dev.set_gram(case["sets"], case["w"], raw=True)
    assert same_bits(again[0], outs) and same_bits(again[1], raws)
    singles = [dev.set_gram([idx], case["w"], raw=True) for idx in case["sets"]]  # one call with five sets equals five calls
    assert same_bits([x[0][0] for x in singles], outs) and same_bits([x[1][0] for x in singles], raws)
    order = [3, 0, 4, 2, 1]
    shuffled = dev.set_gram([case["sets"][k] for k in order], case["w"], raw=True)
    assert same_bits(shuffled[0], [outs[k] for k in order]) and same_bits(shuffled[1], [raws[k] for k in order])
    twice = dev.set_gram([case["sets"][4], case["sets"][4]], case["w"])  # a marker may belong to several sets
    assert same_bits(twice, [outs[4], outs[4]])
    for split in (1, 2, 7):
        dev.set_option("sgram_split", split)
        got = dev.set_gram(case["sets"], case["w"], raw=True)
        assert same_bits(got[0], outs) and same_bits(got[1], raws), split
    dev.set_option("sgram_split", 0)
    # the order of the markers within a set permutes rows and columns and nothing else
    idx = case["sets"][3]
    rev = dev.set_gram([idx[::-1]], case["w"])[0]
    assert same_bits([rev[::-1, ::-1]], [outs[3]])


def test_diagonal_is_the_class_sums_xwx(cohort):
    """section 25's x'Wx = sd^2 (m^2 S0 + (1 - m)^2 S1 + (2 - m)^2 S2) from hgibbs_marker_class_sums, at out's tolerance"""
    case, dev = cohort
    mave, mstd = dev.marker_stats()[:2]
    Sc = dev.marker_class_sums(case["w"][None, :])[:, 0, :]
    with np.errstate(invalid="ignore"):  # (the monomorphic and the all-missing column)
        xwx = mstd * mstd * (mave * mave * Sc[:, 0] + (1.0 - mave) ** 2 * Sc[:, 1] + (2.0 - mave) ** 2 * Sc[:, 2])
    outs = dev.set_gram(case["sets"], case["w"])
    for s, idx in enumerate(case["sets"]):
        want = S.raw_floats(case["geno"], idx, case["w"])
        _, scale = S.gram_out(want, mave[idx], mstd[idx])
        d, ok = np.diag(outs[s]), np.isfinite(np.diag(outs[s]))
        assert np.array_equal(ok, np.isfinite(mstd[idx]))
        assert np.all(np.abs(d[ok] - xwx[idx][ok]) <= TOL_OUT * np.diag(scale)[ok]), s


def test_refusals(cohort):
    case, dev = cohort
    M = S.GRID_M
    w = case["w"]

    def refused(match, sets, ww=w):
        with pytest.raises(capi.HgError, match=match):
            dev.set_gram(sets, ww)
        assert dev.last_set_gram_ms() == 0.0
        dev.set_gram([[0, 1]], w)  # the handle still works
        assert dev.last_set_gram_ms() > 0.0

    refused(r"hgibbs_set_gram: nsets = 0", [])
    refused(r"hgibbs_set_gram: set 1 is empty", [[1, 2], []])
    refused(r"hgibbs_set_gram: idx\[2\] = %d of set 1 out of range \(M = %d\)" % (M, M), [[0, 1], [M]])
    refused(r"hgibbs_set_gram: set 0 lists marker 5 twice", [[5, 6, 5]])
    for bad, what in ((np.nan, "is not finite"), (np.inf, "is not finite"), (-0.25, "is negative")):
        ww = w.copy()
        ww[17] = bad
        refused(r"hgibbs_set_gram: w\[17\] = .* %s" % what, [[0, 1]], ww)
    with pytest.raises(capi.HgError, match="hgibbs_set_gram: no genotypes"):
        capi.Device(0).set_gram([[0]], np.zeros(0))


def test_more_than_1024_markers_refused():
    case = S.big_case(False)
    dev = device(case["geno"])
    with pytest.raises(capi.HgError, match=r"hgibbs_set_gram: set 0 has 1025 markers, at most 1024"):
        dev.set_gram([np.arange(1025)], case["w"])
    assert dev.last_set_gram_ms() == 0.0
    dev.close()


def test_too_many_rows_and_too_much_memory_refused():
    import ctypes as C
    # 2^29 rows of one marker (a 128 MiB BED made in HBM): refused before w is read, so the zeros are never touched
    big = capi.Device(0)
    big.synth_bed(1 << 29, 1, seed=3)
    with pytest.raises(capi.HgError, match="hgibbs_set_gram: 536870912 individuals, at most 536870911"):
        big.set_gram([[0]], np.zeros(1 << 29))
    assert big.last_set_gram_ms() == 0.0
    big.close()
    # 40 000 sets of 1024 markers: 4.2e10 entries of 24 bytes and more are 1 TB, above any device's memory; refused before out is written
    case = S.big_case(False)
    dev = device(case["geno"])
    nsets = 40000
    off = (np.arange(nsets + 1, dtype=np.uint64) * np.uint64(1024))
    idx = np.tile(np.arange(1024, dtype=np.uint32), nsets)
    out = np.zeros(1)
    with pytest.raises(capi.HgError, match=r"hgibbs_set_gram: 40000 sets of 40960000 markers in all \(41943040000 entries\) need [0-9.]+ MiB, "
                                           r"[0-9.]+ MiB of device memory are free"):
        capi.check(dev.L.hgibbs_set_gram(dev.h, nsets, off.ctypes.data_as(capi.C_U64P), idx.ctypes.data_as(capi.C_U32P),
                                         case["w"].ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)), None))
    assert dev.last_set_gram_ms() == 0.0
    dev.close()


def test_several_ranks_refused():
    N, M = 400, 30
    calls = []

    def allreduce(arr):  # a stub world of two identical ranks
        calls.append(arr.size)
        arr *= 2

    dev = capi.Device(0)
    dev.comm_init_external(2, 0, allreduce)
    dev.load_bed(synth.pack_bed_columns(S.genotypes(N, M, 6, True)), N, row_begin=0, row_end=N // 2, n_global=N)
    before = len(calls)
    with pytest.raises(capi.HgError, match="hgibbs_set_gram: one rank only"):
        dev.set_gram([[0, 1]], np.ones(dev.n_local))
    assert len(calls) == before and dev.last_set_gram_ms() == 0.0
