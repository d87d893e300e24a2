"""hgibbs_marker_class_sums against exact Python integers: the four sums of the quantised vectors over the rows of each genotype code
bit for bit, on an edge grid of cohort sizes, for every vector count, across chunkings, splits and repeats; counts against
hgibbs_marker_stats, integer vectors against hgibbs_marker_dots' raw sums, rows dropped through keep, and every refusal."""
import numpy as np
import pytest

from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu


def quantise(U):
    """E_k = 52 - e_k with max_i |u_ik| < 2^e_k (0 for an all-zero row), q = rint(u 2^E_k) as int64 (|q| <= 2^52)"""
    E = np.zeros(U.shape[0], dtype=np.int64)
    for k in range(U.shape[0]):
        m = np.max(np.abs(U[k])) if U.shape[1] else 0.0
        E[k] = 52 - np.frexp(m)[1] if m > 0 else 0
    return E, np.rint(np.ldexp(U, E[:, None])).astype(np.int64)


def exact_sum(W, q):
    """W (M, n) of 0 and 1 (f64), q (K, n) int64 -> (M, K) Python ints sum_i W_ji q_ki, exact: q split into 26-bit halves so that
    every f64 product sum stays below 2^53"""
    ql = (q & ((1 << 26) - 1)).astype(np.float64)
    qh = (q >> 26).astype(np.float64)
    lo = (W @ ql.T).astype(np.int64).astype(object)
    hi = (W @ qh.T).astype(np.int64).astype(object)
    return hi * (1 << 26) + lo


def reference(geno, U):
    """(M, K, 4): the exact integer sum of q over the rows of each code, rounded ONCE to f64, times 2^-E_k"""
    E, q = quantise(U)
    to_f = np.vectorize(float, otypes=[np.float64])  # Python's int -> float rounds to nearest even once
    return np.stack([np.ldexp(to_f(exact_sum((geno == c).astype(np.float64), q)), -E[None, :]) for c in range(4)], axis=2)


def make(N, M, seed):
    geno = synth.make_genotypes(M, N, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for j in rng.choice(M, size=M // 4, replace=False):  # 1 % missing calls in some columns only: clean and missing tiles mix
        geno[j, rng.random(N) < 0.01] = 3
    geno[M // 2] = 1  # monomorphic
    return geno


def make_edge(N, M, seed, missing):
    """missing: make()'s data with one more missing call in every fourth column, so that small cohorts have some too; else data with
    no missing call anywhere, which takes the build without the third product"""
    if not missing:
        geno = synth.make_genotypes(M, N, seed=seed)
        geno[M // 2] = 1
        return geno
    geno = make(N, M, seed)
    for j in range(1, M, 4):
        geno[j, (3 * j) % N] = 3
    return geno


def vectors(K, n, seed):
    rng = np.random.default_rng(seed)
    scales = [1.0, 1e-3, 7e5, 3.0, 1e-9, 1.0, 2.0 ** 40, 0.5, 1.0, 11.0]
    U = np.stack([rng.standard_normal(n) * scales[k % len(scales)] for k in range(K)])
    if K >= 3:
        U[1] = 0.0  # an all-zero vector
        U[2, ::3] = np.round(U[2, ::3])  # exact integers mixed in
    return U


def device(geno, keep=None):
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), geno.shape[1], keep=keep)
    return dev


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def check(dev, geno, U):
    out = dev.marker_class_sums(U)
    assert out.shape == (geno.shape[0], U.shape[0], 4)
    assert np.all(np.isfinite(out))  # the monomorphic column included: the sums use no mstd
    ref = reference(geno, U)
    bad = np.argwhere(out.view(np.int64) != ref.view(np.int64))
    assert bad.size == 0, "sums differ from the exact integers rounded once, first at (marker, vector, code) %s" % bad[:1]
    return out


@pytest.mark.parametrize("N", [2, 15, 16, 17, 63, 65, 511, 512, 513])
@pytest.mark.parametrize("missing", [True, False])
def test_edge_grid(N, missing):
    """individuals below one slice of 512 and next to 16, 64 and 512; M = 257: one marker past a workgroup of 256 markers; K = 1, 5
    (a pass with three of its four tiles used) and 9 (a second pass)"""
    M = 257
    geno = make_edge(N, M, seed=N + M, missing=missing)
    assert bool((geno == 3).any()) == missing and np.all(geno[M // 2] == 1)
    dev = device(geno)
    for K in (1, 5, 9):
        check(dev, geno, vectors(K, N, seed=K + N))
    dev.close()


@pytest.fixture(scope="module")
def small_cohort():
    geno = make(1000, 97, seed=1097)
    dev = device(geno)
    yield geno, dev
    dev.close()


@pytest.mark.parametrize("K", range(1, 33))
def test_every_vector_count(small_cohort, K):
    geno, dev = small_cohort
    check(dev, geno, vectors(K, geno.shape[1], seed=K))
    assert dev.last_marker_class_sums_ms() > 0.0


def test_large_many_workgroups():
    """N = 130 001: 254 slices of individuals split over many workgroups, then all in one, with clean and missing tiles"""
    N, M, K = 130001, 203, 2
    geno = make(N, M, seed=17)
    dev = device(geno)
    U = vectors(K, N, seed=4)
    out = check(dev, geno, U)
    dev.set_option("mdots_split", 1)
    assert same_bits(dev.marker_class_sums(U), out)


def test_bit_identical_across_chunkings_splits_and_repeats():
    N, M, K = 3001, 530, 3
    geno = make(N, M, seed=3)
    dev = device(geno)
    U = vectors(K, N, seed=2)
    out0 = check(dev, geno, U)
    assert same_bits(dev.marker_class_sums(U), out0)
    for step in (1, 17, 256):
        parts = [dev.marker_class_sums(U, m0=a, count=min(step, M - a)) for a in range(0, M, step)]
        assert same_bits(np.concatenate(parts), out0), step
    for split in (0, 1, 7):
        dev.set_option("mdots_split", split)
        assert same_bits(dev.marker_class_sums(U), out0), split
    assert dev.marker_class_sums(U, m0=M, count=0).shape == (0, K, 4)


def test_counts_and_marker_dots_raw_sums():
    N, M = 2500, 150
    geno = make(N, M, seed=9)
    dev = device(geno)
    _, _, n1, n2, nm = dev.marker_stats()
    # all ones: the counts of the marker stats, class 0 the rest; a 0/1 indicator: that subset's counts
    ind = (np.random.default_rng(1).random(N) < 0.3).astype(np.float64)
    out = dev.marker_class_sums(np.stack([np.ones(N), ind]))
    for c, want in ((1, n1), (2, n2), (3, nm)):
        assert np.array_equal(out[:, 0, c], want.astype(np.float64))
    assert np.array_equal(out[:, 0, 0], N - (n1 + n2 + nm).astype(np.float64))
    sub = geno[:, ind == 1.0]
    for c in range(4):
        assert np.array_equal(out[:, 1, c], np.count_nonzero(sub == c, axis=1).astype(np.float64)), c
    # integer-valued vectors: every sum is exact in f64, so S1 + 2 S2 and S0 + S1 + S2 are marker_dots' raw P and Q bit for bit
    U = np.round(np.random.default_rng(2).standard_normal((3, N)) * np.array([[5.0], [1000.0], [2.0 ** 30]]))
    S = dev.marker_class_sums(U)
    _, raw = dev.marker_dots(U, raw=True)
    assert same_bits(S[:, :, 1] + 2.0 * S[:, :, 2], raw[:, :, 0])
    assert same_bits(S[:, :, 0] + S[:, :, 1] + S[:, :, 2], raw[:, :, 1])


def test_na_rows_dropped_through_keep():
    N, M, K = 2500, 150, 3
    geno = make(N, M, seed=5)
    keep = np.ones(N, dtype=np.uint8)
    keep[np.random.default_rng(3).choice(N, size=123, replace=False)] = 0
    kept = geno[:, keep.astype(bool)]
    dev = device(geno, keep=keep)
    assert dev.n_local == kept.shape[1]
    check(dev, kept, vectors(K, kept.shape[1], seed=8))


def test_refusals():
    N, M = 300, 40
    dev = device(make(N, M, seed=2))
    with pytest.raises(capi.HgError, match=r"hgibbs_marker_class_sums: K = 0, must be in \[1, 32\]"):
        dev.marker_class_sums(np.zeros((0, N)))
    with pytest.raises(capi.HgError, match=r"hgibbs_marker_class_sums: K = 33"):
        dev.marker_class_sums(np.ones((33, N)))
    U = np.ones((2, N))
    for bad in (np.nan, np.inf):
        U[1, 17] = bad
        with pytest.raises(capi.HgError, match=r"hgibbs_marker_class_sums: U\[1\]\[17\] = .* is not finite"):
            dev.marker_class_sums(U)
    with pytest.raises(capi.HgError, match=r"hgibbs_marker_class_sums: markers \[30, 41\) out of range \(M = 40\)"):
        dev.marker_class_sums(np.ones((1, N)), m0=30, count=11)
    with pytest.raises(capi.HgError, match="hgibbs_marker_class_sums: no genotypes"):
        capi.Device(0).marker_class_sums(np.ones((1, 0)))


def test_several_ranks_refused_before_any_product():
    N, M = 400, 30
    calls = []

    def allreduce(arr):  # a stub world of two identical ranks
        calls.append(arr.size)
        arr *= 2

    dev = capi.Device(0)
    dev.comm_init_external(2, 0, allreduce)
    dev.load_bed(synth.pack_bed_columns(make(N, M, seed=6)), N, row_begin=0, row_end=N // 2, n_global=N)
    before = len(calls)
    with pytest.raises(capi.HgError, match="hgibbs_marker_class_sums: one rank only"):
        dev.marker_class_sums(np.ones((1, dev.n_local)))
    assert len(calls) == before  # refused before the marker stats' collective, so before any product
