"""hgibbs_marker_dots against NumPy: the exact integer sums P, Q of the quantised vectors bit for bit, x_j'u_k as the f64 formula on
them and against X_std'U within the stated bound, bit identity across chunkings, splits and repeats, and every refusal."""
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
    q = np.rint(np.ldexp(U, E[:, None])).astype(np.int64)
    return E, q


def exact_sum(W, q):
    """W (M, n) small non-negative integers (f64), q (K, n) int64 -> (M, K) Python ints sum_i W_ji q_ki, exact: q split into 26-bit
    halves so that every f64 product sum stays below 2^53"""
    ql = (q & ((1 << 26) - 1)).astype(np.float64)
    qh = (q >> 26).astype(np.float64)
    lo = (W @ ql.T).astype(np.int64).astype(object)
    hi = (W @ qh.T).astype(np.int64).astype(object)
    return hi * (1 << 26) + lo


def reference(geno, U, mave, mstd):
    """raw (M, K, 2) = P, Q each rounded once to f64; out (M, K) = mstd (P - mave Q); the exact-real dots X_std'U and the bound"""
    E, q = quantise(U)
    called = (geno != 3).astype(np.float64)
    g = np.where(geno == 3, 0, geno).astype(np.float64)
    P = exact_sum(g, q)
    Q = exact_sum(called, q)
    to_f = np.vectorize(float, otypes=[np.float64])
    raw = np.stack([np.ldexp(to_f(P), -E[None, :]), np.ldexp(to_f(Q), -E[None, :])], axis=2)
    with np.errstate(invalid="ignore"):
        out = mstd[:, None] * (raw[:, :, 0] - mave[:, None] * raw[:, :, 1])
        out[~np.isfinite(mstd)] = np.nan
        x = np.where(geno == 3, 0.0, (g - mave[:, None]) * mstd[:, None])
    exact = x @ U.T
    n = geno.shape[1]
    with np.errstate(invalid="ignore"):
        tol = (np.abs(mstd)[:, None] * (n * np.ldexp(1.0, -E)[None, :] * (1.0 + np.abs(mave)[:, None])
                                        + 2.0 ** -51 * (np.abs(raw[:, :, 0]) + np.abs(mave[:, None] * raw[:, :, 1])))
               + 1e-12 * (np.abs(x) @ np.abs(U).T) + 1e-300)
    return raw, out, exact, tol


def make(N, M, seed):
    geno = synth.make_genotypes(M, N, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for j in rng.choice(M, size=M // 4, replace=False):  # 1 % missing calls in some columns only: clean and missing tiles mix
        geno[j, rng.random(N) < 0.01] = 3
    geno[M // 2] = 1  # monomorphic: NaN
    return geno


def vectors(K, n, seed):
    rng = np.random.default_rng(seed)
    scales = [1.0, 1e-3, 7e5, 3.0, 1e-9, 1.0, 2.0 ** 40, 0.5, 1.0, 11.0]
    U = np.stack([rng.standard_normal(n) * scales[k % len(scales)] for k in range(K)])
    if K >= 3:
        U[1] = 0.0  # an all-zero vector: 0 out
        U[2, ::3] = np.round(U[2, ::3])  # exact integers mixed in
    return U


def device(geno, keep=None):
    M, N = geno.shape
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N, keep=keep)
    mave, mstd, *_ = dev.marker_stats()
    return dev, mave, mstd


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def check(dev, geno, U, mave, mstd):
    out, raw = dev.marker_dots(U, raw=True)
    rraw, rout, exact, tol = reference(geno, U, mave, mstd)
    assert same_bits(raw, rraw), "P, Q differ from the exact sums rounded once"
    assert same_bits(out, rout), "out is not mstd (P - mave Q)"
    ok = np.isfinite(mstd)
    assert np.all(np.isnan(out[~ok]))
    assert np.all(np.abs(out[ok] - exact[ok]) <= tol[ok]), "beyond the bound against X_std'U"
    return out


@pytest.mark.parametrize("N,M", [(1000, 301), (4099, 97)])
@pytest.mark.parametrize("K", [1, 2, 3, 9])
def test_match_numpy(N, M, K):
    geno = make(N, M, seed=N + M + K)
    dev, mave, mstd = device(geno)
    U = vectors(K, N, seed=K)
    out = check(dev, geno, U, mave, mstd)
    if K >= 3:
        assert np.all(out[np.isfinite(mstd), 1] == 0.0)
    assert dev.last_marker_dots_ms() > 0.0


def test_na_rows_dropped_through_keep():
    N, M, K = 2500, 150, 3
    geno = make(N, M, seed=5)
    keep = np.ones(N, dtype=np.uint8)
    keep[np.random.default_rng(3).choice(N, size=123, replace=False)] = 0
    kept = geno[:, keep.astype(bool)]
    dev, mave, mstd = device(geno, keep=keep)
    assert dev.n_local == kept.shape[1]
    check(dev, kept, vectors(K, kept.shape[1], seed=8), mave, mstd)


def test_large_many_workgroups():
    """N = 130 001: many slices of individuals, split over many workgroups, with clean and missing tiles"""
    N, M, K = 130001, 203, 2
    geno = make(N, M, seed=17)
    dev, mave, mstd = device(geno)
    U = vectors(K, N, seed=4)
    out = check(dev, geno, U, mave, mstd)
    dev.set_option("mdots_split", 1)  # one workgroup takes all 254 slices
    assert same_bits(dev.marker_dots(U), out)


def test_bit_identical_across_chunkings_splits_and_repeats():
    N, M, K = 3001, 530, 3
    geno = make(N, M, seed=3)
    dev, mave, mstd = device(geno)
    U = vectors(K, N, seed=2)
    out0, raw0 = dev.marker_dots(U, raw=True)
    out1, raw1 = dev.marker_dots(U, raw=True)
    assert same_bits(out0, out1) and same_bits(raw0, raw1)
    for step in (1, 17, 256):
        parts = [dev.marker_dots(U, m0=a, count=min(step, M - a)) for a in range(0, M, step)]
        assert same_bits(np.concatenate(parts), out0), step
    for split in (0, 1, 7):
        dev.set_option("mdots_split", split)
        out, raw = dev.marker_dots(U, raw=True)
        assert same_bits(out, out0) and same_bits(raw, raw0), split
    with pytest.raises(capi.HgError, match="mdots_split"):
        dev.set_option("mdots_split", -1)
    assert dev.marker_dots(U, m0=M, count=0).shape == (0, K)


@pytest.fixture(scope="module")
def sweep_cohort():
    """N = 513: two slices of 512 individuals, the second with one; M = 257: one marker past a workgroup of 256.  make()'s mixed clean
    and missing tiles"""
    N, M = 513, 257
    geno = make(N, M, seed=N + M)
    dev, mave, mstd = device(geno)
    yield geno, dev, mave, mstd
    dev.close()


@pytest.mark.parametrize("K", range(1, 33))
def test_every_vector_count(sweep_cohort, K):
    """every K a call takes: passes of one, two, three (K = 5, 6) and four vector tiles, an odd last tile, and the second, third and
    fourth pass of K > 8, 16, 24"""
    geno, dev, mave, mstd = sweep_cohort
    check(dev, geno, vectors(K, geno.shape[1], seed=K), mave, mstd)


def test_chunks_at_the_largest_vector_count(sweep_cohort):
    geno, dev, mave, mstd = sweep_cohort
    M, K = geno.shape[0], 32
    U = vectors(K, geno.shape[1], seed=40)
    out0, raw0 = dev.marker_dots(U, raw=True)
    for step in (1, 17, 128):
        parts = [dev.marker_dots(U, m0=a, count=min(step, M - a), raw=True) for a in range(0, M, step)]
        assert same_bits(np.concatenate([p[0] for p in parts]), out0), step
        assert same_bits(np.concatenate([p[1] for p in parts]), raw0), step


def make_edge(N, M, seed, missing):
    """missing: make()'s data with one more missing call in every fourth column, so that small cohorts have some too; else data with no
    missing call anywhere, which takes the build without the second product"""
    if not missing:
        return synth.make_genotypes(M, N, seed=seed)
    geno = make(N, M, seed)
    for j in range(1, M, 4):
        geno[j, (3 * j) % N] = 3
    if M == 1:
        geno[0, N - 1] = 3
    return geno


@pytest.mark.parametrize("N", [2, 15, 16, 17, 63, 65, 511, 512, 513])
@pytest.mark.parametrize("missing", [True, False])
def test_edge_grid(N, missing):
    """individuals below one slice of 512 and next to 16, 64 and 512; markers of one tile of sixteen or less and next to 16, 128 and 256;
    K = 1, 5 (a pass with three of its four tiles used) and 9 (a second pass)"""
    for M in (1, 15, 16, 17, 127, 128, 129, 255, 257):
        geno = make_edge(N, M, seed=N + M, missing=missing)
        assert bool((geno == 3).any()) == missing
        dev, mave, mstd = device(geno)
        for K in (1, 5, 9):
            check(dev, geno, vectors(K, N, seed=K + M), mave, mstd)
        dev.close()


def test_refusals():
    N, M = 300, 40
    geno = make(N, M, seed=2)
    dev, _, _ = device(geno)
    with pytest.raises(capi.HgError, match="K = 0"):
        dev.marker_dots(np.zeros((0, N)))
    with pytest.raises(capi.HgError, match="K = 33"):
        dev.marker_dots(np.ones((33, N)))
    U = np.ones((2, N))
    U[1, 17] = np.nan
    with pytest.raises(capi.HgError, match="not finite"):
        dev.marker_dots(U)
    U[1, 17] = np.inf
    with pytest.raises(capi.HgError, match="not finite"):
        dev.marker_dots(U)
    with pytest.raises(capi.HgError, match="out of range"):
        dev.marker_dots(np.ones((1, N)), m0=30, count=11)
    empty = capi.Device(0)
    with pytest.raises(capi.HgError, match="no genotypes"):
        empty.marker_dots(np.ones((1, 0)))


def test_several_ranks_refused_before_any_product():
    N, M = 400, 30
    geno = make(N, M, seed=6)
    calls = []

    def allreduce(arr):  # a stub world of two identical ranks
        calls.append(arr.size)
        arr *= 2

    dev = capi.Device(0)
    dev.comm_init_external(2, 0, allreduce)
    dev.load_bed(synth.pack_bed_columns(geno), N, row_begin=0, row_end=N // 2, n_global=N)
    before = len(calls)
    with pytest.raises(capi.HgError, match="one rank only"):
        dev.marker_dots(np.ones((1, dev.n_local)))
    assert len(calls) == before  # refused before the marker stats' collective, so before any product
