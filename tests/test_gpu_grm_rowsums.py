"""The row sums of the relationship matrix (hgibbs_grm_rowsums) against a NumPy restatement of their definition built from
hgibbs_grm's own S and NSNP (pinned by tests/test_gpu_grm.py): bit for bit; bit identity across grm_split, grm_piece, repeats, the
number of vectors and the outputs asked for; the default piece size; planted cases; against longdouble within the derived bound; the
refusals."""
import functools

import numpy as np
import pytest

from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu


def make(N, M, seed):
    """tests/test_gpu_grm.py's recipe"""
    geno = synth.make_genotypes(M, N, seed=seed)
    rng = np.random.default_rng(seed + 7)
    for j in rng.choice(M, size=max(1, M // 5), replace=False):  # 1-5 % missing calls in a fifth of the columns
        geno[j, rng.random(N) < rng.uniform(0.01, 0.05)] = 3
    if M >= 3:
        geno[M // 3] = 3  # a marker missing everywhere
        geno[M // 2] = 1 if M % 2 else 0  # a monomorphic marker
    if M >= 5:
        geno[M - 2] = 2
    if N >= 3:
        geno[:, N // 2] = 3  # an individual missing everywhere
    if N >= 6:
        geno[:, 1] = geno[:, N - 1]  # a duplicate
    return geno


def device(geno, keep=None):
    M, N = geno.shape
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N, keep=keep)
    return dev


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def frac_bits(N):
    k = 0
    while (1 << k) < N:
        k += 1
    return 58 - k


def vectors(N, P, seed):
    return np.random.default_rng(seed).standard_normal((P, N))


# ---- the definition, restated on hgibbs_grm's S and NSNP ----
def restate(S, nsnp, N, Y):
    """ay (N, P), a1, a2, diag (N,), partners (N,) and the largest |term|, from the packed triangle: A = S / nsnp,
    fx = rint(ldexp(t, F)) as int64, summed in int64, ldexp(float(sum), -F).  With a term >= 16 the call is refused and the sums are not
    defined (M = 1 at the larger N: one marker's x_a x_b reaches 4, its square 16)."""
    P = Y.shape[0]
    F = frac_bits(N)
    AY = np.zeros((N, P), dtype=np.int64)
    A1 = np.zeros(N, dtype=np.int64)
    A2 = np.zeros(N, dtype=np.int64)
    partners = np.zeros(N, dtype=np.int64)
    diag = np.full(N, np.nan)
    tmax = 0.0

    def fx(t):
        return np.rint(np.ldexp(t, F)).astype(np.int64)

    off = 0
    for a in range(N):
        s, m = S[off:off + a + 1], nsnp[off:off + a + 1]
        off += a + 1
        if m[a] > 0:
            diag[a] = s[a] / m[a]
        on = m[:a] > 0
        if not on.any():
            continue
        A = s[:a][on] / m[:a][on].astype(np.float64)
        rowt = A[None, :] * Y[:, :a][:, on]  # (P, partners below a): row a takes A_ab Y_pb
        colt = A[None, :] * Y[:, a][:, None]  # row b takes A_ab Y_pa
        tmax = max(tmax, float(np.abs(A).max()), float((A * A).max()), float(np.abs(rowt).max()), float(np.abs(colt).max()))
        if tmax >= 16.0:
            continue  # (the call is refused: the integers are not defined)
        AY[a] += fx(rowt).sum(axis=1)
        A1[a] += fx(A).sum()
        A2[a] += fx(A * A).sum()
        partners[a] += int(on.sum())
        idx = np.flatnonzero(on)
        AY[idx] += fx(colt).T  # (idx holds no index twice)
        A1[idx] += fx(A)
        A2[idx] += fx(A * A)
        partners[idx] += 1
    conv = lambda v: np.ldexp(v.astype(np.float64), -F)  # noqa: E731  (|sum| < 2^62: int64 -> f64 rounds once, to nearest even)
    return conv(AY), conv(A1), conv(A2), diag, partners.astype(np.uint32), tmax


def same(got, want):
    """ay, a1, a2, diag, partners: bit for bit (diag: NaN where NaN)"""
    for k in (0, 1, 2):
        assert np.array_equal(bits(got[k]), bits(want[k])), "output %d" % k
    assert np.array_equal(np.isnan(got[3]), np.isnan(want[3]))
    ok = ~np.isnan(want[3])
    assert np.array_equal(bits(got[3][ok]), bits(want[3][ok]))
    assert got[4].dtype == np.uint32 and np.array_equal(got[4], want[4])


def check(dev, N, Y, S=None, nsnp=None):
    """the call against the restatement; a shape whose restated terms leave the range must be refused by that rule"""
    if S is None:
        S, nsnp = dev.grm()
    want = restate(S, nsnp, N, Y)
    if want[5] >= 16.0:
        with pytest.raises(capi.HgError, match="magnitude"):
            dev.grm_rowsums(Y)
        return None
    got = dev.grm_rowsums(Y)
    same(got, want)
    return got


@functools.lru_cache(maxsize=None)
def case(N, M, seed):
    """data, device, hgibbs_grm's triangle, eight vectors and their row sums of one shape, made once and left unchanged"""
    geno = make(N, M, seed)
    dev = device(geno)
    S, nsnp = dev.grm()
    Y = vectors(N, 8, seed + 1)
    got = check(dev, N, Y, S, nsnp)
    assert got is not None
    for v in (S, nsnp, Y) + tuple(got):
        v.setflags(write=False)
    return geno, dev, S, nsnp, Y, got


# ---- 1. bit for bit against the restatement ----
@pytest.mark.parametrize("M", [1, 65, 2049])
@pytest.mark.parametrize("N", [2, 3, 15, 16, 17, 63, 64, 65, 129, 513])
def test_bit_exact_against_the_restatement(N, M):
    geno = make(N, M, seed=N * 7 + M)
    dev = device(geno)
    S, nsnp = dev.grm()
    for P in (1, 8) + ((3,) if N in (65, 513) else ()):
        check(dev, N, vectors(N, P, N + M + P), S, nsnp)


@pytest.mark.parametrize("kind", ["monomorphic", "missing"])
def test_no_used_marker_is_refused_as_grm_refuses_it(kind):
    """M_used = 0: every marker monomorphic, or every marker monomorphic or missing everywhere; each call names itself"""
    N, M = 40, 70
    geno = np.ones((M, N), dtype=np.uint8)
    geno[::2] = 2
    if kind == "missing":
        geno[1::3] = 3
    dev = device(geno)
    assert not np.isfinite(dev.marker_stats()[1]).any()
    with pytest.raises(capi.HgError, match=r"hgibbs_grm: no marker of the 70 loaded has a finite mstd \(M_used = 0\)"):
        dev.grm()
    assert dev.grm_info() == (0, 0)
    with pytest.raises(capi.HgError, match=r"hgibbs_grm_rowsums: no marker of the 70 loaded has a finite mstd \(M_used = 0\)"):
        dev.grm_rowsums(vectors(N, 2, 0))
    assert dev.grm_info() == (0, 0) and dev.last_grm_rowsums_ms() == (0.0, 0.0)
    # the handle serves its other operators, and a handle with markers serves both calls after a refused one
    assert np.all(dev.king()[..., 0] == (M if kind == "monomorphic" else M - len(range(1, M, 3))))
    good = make(N, M, seed=1)
    dev2 = device(good)
    with pytest.raises(capi.HgError, match="P = 9"):
        dev2.grm_rowsums(vectors(N, 9, 1))
    assert dev2.grm_info() == (0, 0)
    assert check(dev2, N, vectors(N, 2, 9)) is not None
    assert dev2.grm_info()[0] > 0


# ---- 2. bit identity ----
def test_bit_identity():
    N, M = 700, 2049
    _, dev, _, _, Y, want = case(N, M, 5)
    for split in (1, 2, 7, 33, 0):
        dev.set_option("grm_split", split)
        same(dev.grm_rowsums(Y), want)
    for piece in (1, 1000, 5000, 1 << 22, 0):
        dev.set_option("grm_piece", piece)
        same(dev.grm_rowsums(Y), want)
    same(dev.grm_rowsums(Y), want)  # a repeat
    products_ms, reduce_ms = dev.last_grm_rowsums_ms()
    assert products_ms > 0.0 and reduce_ms > 0.0
    # each column of the call with eight vectors against the call with that vector alone
    for p in range(8):
        one = dev.grm_rowsums(Y[p])
        assert np.array_equal(bits(one[0][:, 0]), bits(want[0][:, p])), "vector %d" % p
        same((want[0],) + one[1:], want)
    # each output pointer alone
    u32p = capi.C.POINTER(capi.C.c_uint32)
    Yc = np.ascontiguousarray(Y)
    for k in range(5):
        out = [np.zeros((N, 8)), np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.uint32)]
        args = [capi._dp(v) if i < 4 else v.ctypes.data_as(u32p) for i, v in enumerate(out)]
        capi.check(dev.L.hgibbs_grm_rowsums(dev.h, 8, capi._dp(Yc), *[a if i == k else None for i, a in enumerate(args)]))
        same([out[i] if i == k else want[i] for i in range(5)], want)


def test_grm_does_not_depend_on_grm_piece():
    N, M = 700, 2049
    _, dev, S, nsnp, _, _ = case(N, M, 5)
    try:
        for piece in (1, 1000, 1 << 22):
            dev.set_option("grm_piece", piece)
            s2, n2 = dev.grm()
            assert np.array_equal(bits(s2), bits(S)) and np.array_equal(n2, nsnp), "grm_piece=%d" % piece
    finally:
        dev.set_option("grm_piece", 0)


# ---- 3. the default piece size ----
def test_default_piece_size_is_crossed():
    N, M = 8300, 65
    assert N * (N + 1) // 2 > (1 << 25)
    geno = make(N, M, seed=31)
    dev = device(geno)
    Y = vectors(N, 1, 3)
    S, nsnp = dev.grm()
    want = restate(S, nsnp, N, Y)
    assert want[5] < 16.0
    same(dev.grm_rowsums(Y), want)
    dev.set_option("grm_piece", 1 << 22)
    same(dev.grm_rowsums(Y), want)


# ---- 4. the planted cases ----
def test_planted_cases():
    N, M = 700, 2049
    geno, _, _, _, _, (ay, a1, a2, diag, partners) = case(N, M, 5)
    i = N // 2
    assert (geno[:, i] == 3).all()
    assert partners[i] == 0 and np.isnan(diag[i]) and not ay[i].any() and a1[i] == 0.0 and a2[i] == 0.0
    others = np.delete(np.arange(N), i)
    assert (partners[others] == N - 2).all() and not np.isnan(diag[others]).any()


# ---- 5. against longdouble ----
def test_against_longdouble():
    N, M = 700, 2049
    _, _, S, nsnp, Y, (ay, _, _, _, _) = case(N, M, 5)
    F = frac_bits(N)
    Sf = np.zeros((N, N))
    Sf[np.tril_indices(N)] = S
    nf = np.zeros((N, N), dtype=np.int64)
    nf[np.tril_indices(N)] = nsnp
    Sf, nf = np.tril(Sf, -1), np.tril(nf, -1)
    Sf, nf = Sf + Sf.T, nf + nf.T
    with np.errstate(all="ignore"):
        A = np.where(nf > 0, Sf / nf, 0.0).astype(np.longdouble)
    for p in range(Y.shape[0]):
        terms = A * Y[p].astype(np.longdouble)[None, :]
        ref = terms.sum(axis=1)
        err = float(np.max(np.abs(ay[:, p].astype(np.longdouble) - ref)))
        # one rounding per term to the grid, one product rounding per term, one conversion of the sum
        bound = (N - 1) * (2.0 ** -(F + 1) + 2.0 ** -53 * float(np.abs(terms).max())) + 2.0 ** -53 * float(np.abs(ref).max())
        print("MEASURED vector %d: |ay - (A o offdiag) y| max %.3g, bound %.3g (N %d, F %d)" % (p, err, bound, N, F))
        assert err <= bound


# ---- 6. refusals ----
def test_refusals():
    N, M = 40, 70
    geno = make(N, M, seed=1)
    dev = device(geno)
    Y = vectors(N, 2, 9)

    def still_serves():
        assert check(dev, N, Y) is not None

    still_serves()
    with pytest.raises(capi.HgError, match=r"P = 0, must be in \[1, 8\]"):
        dev.grm_rowsums(np.zeros((0, N)))
    still_serves()
    with pytest.raises(capi.HgError, match=r"P = 9, must be in \[1, 8\]"):
        dev.grm_rowsums(vectors(N, 9, 1))
    still_serves()
    bad = Y.copy()
    bad[1, 17] = np.nan
    with pytest.raises(capi.HgError, match=r"Y\[1\]\[17\] is not finite"):
        dev.grm_rowsums(bad)
    still_serves()
    with pytest.raises(capi.HgError, match="null Y"):
        capi.check(dev.L.hgibbs_grm_rowsums(dev.h, 1, None, None, None, None, None, None))
    still_serves()
    with pytest.raises(capi.HgError, match="no genotypes"):
        capi.Device(0).grm_rowsums(Y)
    one = capi.Device(0)  # one row of two on this handle (a cohort of one is refused at the load)
    one.load_bed(synth.pack_bed_columns(geno[:, :2]), 2, row_begin=0, row_end=1, n_global=2)
    assert one.n_local == 1
    with pytest.raises(capi.HgError, match="n_local >= 2"):
        one.grm_rowsums(np.ones((1, 1)))
    # the range rule: the message names the magnitude and no output is touched
    u32p = capi.C.POINTER(capi.C.c_uint32)
    big = np.ascontiguousarray(Y * 1e9)
    out = [np.full((N, 2), 7.0), np.full(N, 7.0), np.full(N, 7.0), np.full(N, 7.0), np.full(N, 7, dtype=np.uint32)]
    rc = dev.L.hgibbs_grm_rowsums(dev.h, 2, capi._dp(big), *[capi._dp(v) for v in out[:4]], out[4].ctypes.data_as(u32p))
    assert rc != 0
    msg = dev.L.hgibbs_last_error().decode()
    S, nsnp = dev.grm()
    tmax = restate(S, nsnp, N, big)[5]
    assert tmax >= 16.0 and "magnitude %g" % tmax in msg, (msg, tmax)
    assert all((v == 7).all() for v in out)
    still_serves()
    with pytest.raises(capi.HgError, match="grm_piece"):
        dev.set_option("grm_piece", -1)
    with pytest.raises(capi.HgError, match=r"grm_piece must be in \[0,33554432\]"):
        dev.set_option("grm_piece", (1 << 25) + 1)
    dev.set_option("grm_piece", 1 << 25)  # (the default, named)
    still_serves()
    # the other operators too
    assert np.all(dev.king()[..., 0] >= 0)
