"""hgibbs_pair_tables against the exact integers of tests/epi_restate.py, cell for cell: cohort sizes around a k-step, a slice and the
image's padding; list lengths around a tile and a group of two; clean data and 2 % missing calls; unordered lists, the same marker on both
sides or twice; every form of cls; bit-identity across ptab_split, cuts of the lists and repeats; the clean build against the missing
build; every refusal; the timing."""
import ctypes as C

import numpy as np
import pytest

from hydra_amd import capi, synth

import epi_restate as E

pytestmark = pytest.mark.gpu

GRID_N = (1, 63, 64, 65, 511, 512, 513, 1000, 4097)
LENGTHS = (1, 15, 16, 17, 33)
M = 70
MONO, GONE, HET = 3, 20, 37  # a monomorphic column, one missing in every row (with missing calls), an all-het one


def cohort(n, missing, seed=0):
    rng = np.random.default_rng(100 + n + seed)
    geno = rng.binomial(2, rng.uniform(0.05, 0.5, size=M)[:, None], size=(M, n)).astype(np.uint8)
    if missing:
        geno = E.with_missing(geno, 0.02, 200 + n)
        geno[GONE] = 3
        geno[48:64] = np.where(geno[48:64] == 3, 0, geno[48:64])  # a clean granule beside the others
    geno[MONO] = 0
    geno[HET] = 1
    cls = (rng.random(n) < 0.45).astype(np.uint8)
    return geno, cls


def device(geno):
    """a handle on the cohort's rows; a single row is loaded as the first row of a file of two (hgibbs_load_bed takes no cohort of
    one: the handle then has n_local = 1 of n_global = 2)"""
    dev = capi.Device(0)
    n = geno.shape[1]
    if n == 1:
        dev.load_bed(synth.pack_bed_columns(np.concatenate([geno, geno], axis=1)), 2, row_begin=0, row_end=1, n_global=2)
    else:
        dev.load_bed(synth.pack_bed_columns(geno), n)
    assert dev.n_local == n
    return dev


def exact(dev, geno, A, B, cls):
    got = dev.pair_tables(A, B, cls)
    want = E.tables(geno, A, B, cls)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing cell (a, b, k, i, j) %s: %d, the exact count is %d" % (bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    return got


@pytest.mark.parametrize("n", GRID_N)
@pytest.mark.parametrize("missing", [False, True])
def test_grid(n, missing):
    geno, cls = cohort(n, missing)
    assert bool((geno == 3).any()) == missing
    dev = device(geno)
    rng = np.random.default_rng(n)
    special = np.array([MONO, GONE, HET])
    for na in LENGTHS:
        for nb in LENGTHS:
            A = rng.permutation(M)[:na]  # unordered, with holes
            B = rng.permutation(M)[:nb]
            if na == 33:
                A[:3] = special
            if nb == 33:
                B[5:8] = special
            got = exact(dev, geno, A, B, cls)
            assert np.all(got >= 0) and np.all(got.sum(axis=(2, 3, 4)) <= n)
    assert dev.last_pair_tables_ms() > 0.0
    A, B = np.arange(M)[::-1], np.arange(M)
    for c in (None, np.zeros(n, dtype=np.uint8), np.ones(n, dtype=np.uint8), cls):
        got = exact(dev, geno, A, B, c)
        if c is None:
            assert not got[:, :, 1].any()
    if n == 1000:  # a range boundary inside the data: two slices of 512 rows, one workgroup each
        dev.set_option("ptab_split", 2)
        assert np.array_equal(dev.pair_tables(A, B, cls), got)
        assert np.array_equal(dev.pair_tables(A, B, cls), got)
    dev.close()


@pytest.fixture(scope="module")
def loaded():
    geno, cls = cohort(1000, True)
    dev = device(geno)
    yield geno, cls, dev
    dev.close()


def test_same_marker_on_both_sides_is_diagonal(loaded):
    geno, cls, dev = loaded
    A = np.array([9, HET, GONE, MONO, 50, 9])
    got = exact(dev, geno, A, A, cls)
    for a in range(A.size):
        for b in range(A.size):
            if A[a] == A[b]:
                t = got[a, b]
                assert not (t * (1 - np.eye(3, dtype=np.int64))).any()
                for k in range(2):
                    assert [int(t[k, i, i]) for i in range(3)] == [int(((geno[A[a]] == i) & (cls == k)).sum()) for i in range(3)]
    assert not got[2].any() and not got[:, 2].any()  # the column missing in every row


def test_a_marker_twice_in_a_list(loaded):
    geno, cls, dev = loaded
    A = np.array([4, 4, 31, 4, 66] + list(range(20)))
    B = np.array([31, 12, 31] + list(range(40, 70)))
    got = exact(dev, geno, A, B, cls)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[3]) and np.array_equal(got[:, 0], got[:, 2])


def test_bit_identical_across_cuts_of_the_lists_and_repeats(loaded):
    geno, cls, dev = loaded
    rng = np.random.default_rng(5)
    A, B = rng.permutation(M)[:50], rng.permutation(M)[:45]
    whole = exact(dev, geno, A, B, cls)
    assert np.array_equal(dev.pair_tables(A, B, cls), whole)
    parts = np.zeros_like(whole)
    for a0, a1 in ((0, 7), (7, 24), (24, 50)):
        for b0, b1 in ((0, 33), (33, 34), (34, 45)):
            parts[a0:a1, b0:b1] = dev.pair_tables(A[a0:a1], B[b0:b1], cls)
    assert np.array_equal(parts, whole)
    for split in (2, 1, 0):
        dev.set_option("ptab_split", split)
        assert np.array_equal(dev.pair_tables(A, B, cls), whole)


def test_clean_build_against_missing_build():
    """One missing call in a marker that is not listed, but lies in a listed marker's 16-marker granule, takes the listed pairs through
    the missing build: the tables stay what the clean build gave."""
    geno, cls = cohort(1000, False)
    listed = np.array([j for j in range(M) if j not in (17, 40)])
    dev = device(geno)
    clean = exact(dev, geno, listed, listed[::-1], cls)
    dev.close()
    geno[17, 123] = 3  # granule 1: markers 16 .. 31
    geno[40, 999] = 3  # granule 2: markers 32 .. 47
    dev = device(geno)
    assert np.array_equal(exact(dev, geno, listed, listed[::-1], cls), clean)
    dev.close()


def raw_call(dev, na, A, nb, B, cls):
    out = np.zeros(18, dtype=np.int32)
    return dev.L.hgibbs_pair_tables(dev.h, na, None if A is None else A.ctypes.data_as(capi.C_U32P), nb, None if B is None else B.ctypes.data_as(capi.C_U32P),
                                    None if cls is None else cls.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_int32)))


def test_refusals_then_a_good_call(loaded):
    geno, cls, dev = loaded
    n = geno.shape[1]
    one = np.array([1], dtype=np.uint32)

    def refused(msg, *args):
        with pytest.raises(capi.HgError, match=msg):
            capi.check(raw_call(dev, *args))
        assert dev.last_pair_tables_ms() == 0.0

    exact(dev, geno, [1, 2], [3], cls)
    assert dev.last_pair_tables_ms() > 0.0
    refused("na = 0, nb = 1, a list needs at least one marker", 0, one, 1, one, cls)
    refused("na = 1, nb = 0, a list needs at least one marker", 1, one, 0, one, cls)
    refused("null argument", 1, None, 1, one, cls)
    refused("null argument", 1, one, 1, None, cls)
    refused("idxA\\[1\\] = 70 out of range \\(M = 70\\)", 2, np.array([0, M], dtype=np.uint32), 1, one, cls)
    refused("idxB\\[0\\] = 4000000000 out of range", 1, one, 1, np.array([4000000000], dtype=np.uint32), cls)
    bad = cls.copy()
    bad[n - 1] = 2
    refused("cls\\[999\\] = 2, a class is 0 or 1", 1, one, 1, one, bad)
    big = np.zeros(1 << 16, dtype=np.uint32)
    refused("lists of 65536 and 65536 markers need .* MiB, .* MiB of device memory are free", 1 << 16, big, 1 << 16, big, cls)
    empty = capi.Device(0)
    with pytest.raises(capi.HgError, match="hgibbs_pair_tables: no genotypes loaded on this handle"):
        capi.check(raw_call(empty, 1, one, 1, one, None))
    empty.close()
    with pytest.raises(capi.HgError, match="null handle"):
        capi.check(dev.L.hgibbs_pair_tables(None, 1, one.ctypes.data_as(capi.C_U32P), 1, one.ctypes.data_as(capi.C_U32P), None, None))
    with pytest.raises(capi.HgError, match="ptab_split must be in \\[0,65535\\]"):
        dev.set_option("ptab_split", 70000)
    with pytest.raises(ValueError):
        dev.pair_tables([1], [2], cls[:-1])
    # the handle then takes a good call
    exact(dev, geno, np.arange(M), np.arange(M)[::-1], cls)
    assert dev.last_pair_tables_ms() > 0.0


def test_too_many_rows_refused():
    # 2^29 rows of one marker (a 128 MiB BED made in HBM): refused before anything is allocated
    big = capi.Device(0)
    big.synth_bed(1 << 29, 1, seed=3)
    with pytest.raises(capi.HgError, match="hgibbs_pair_tables: 536870912 individuals, at most 536870911 \\(32-bit counts\\)"):
        big.pair_tables([0], [0])
    assert big.last_pair_tables_ms() == 0.0
    big.close()


def test_several_ranks_refused():
    geno, cls = cohort(1000, True)
    calls = []

    def allreduce(arr):  # a stub world of two identical ranks
        calls.append(arr.size)
        arr *= 2

    dev = capi.Device(0)
    dev.comm_init_external(2, 0, allreduce)
    dev.load_bed(synth.pack_bed_columns(geno), 1000, row_begin=0, row_end=500, n_global=1000)
    before = len(calls)
    with pytest.raises(capi.HgError, match="hgibbs_pair_tables: one rank only \\(this handle has 2\\): the counts are not summed over ranks"):
        dev.pair_tables([0, 1], [2], cls[:dev.n_local])
    assert len(calls) == before and dev.last_pair_tables_ms() == 0.0
    dev.close()
