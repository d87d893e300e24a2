"""hgibbs_pca restated step by step (hydra_amd/csrc/hg_pca.hip.h), for a comparison of BITS: tests/test_gpu_pca_exact.py feeds restate()
the two panel products from the device's public operators (Device.marker_dots, Device.score: the pipelines hgibbs_pca runs, pinned bit
for bit by their own tests) and does everything else here, in the order the source states; tests/test_pca_restatement_cpu.py checks
this module on its own with plain f64 products.  Also the helpers the PCA tests share (data, NumPy references, the twin of the start
panel, the grid of cases).

Every floating-point sum below is element-wise NumPy or plain Python floats, one rounding per operation, in the kernel's order:
no np.sum, no @, no np.dot (their order is NumPy's, not the kernel's).  A product and the add that takes it are two operations, as the
library is built (-ffp-contract=off).  Vectorising ACROSS independent sums (the entries of a Gram matrix, the workgroups of
k_pca_gram, the rows of k_pca_apply) leaves each sum's own order alone."""
import math

import numpy as np

from hydra_amd import capi, synth

VEC_BOUND = 8.8e-14
VAL_BOUND = 2.2e-14
assert VEC_BOUND <= 1e-9 and VAL_BOUND <= 1e-12  # a result that needs more has lost half its digits

PG_ROWS = 1024   # rows of the panel per workgroup of k_pca_gram
PG_LMAX = 32     # panel width at most


# ---- data: P populations, Balding-Nichols allele frequencies, binomial genotypes, missing calls ----
def structured(N, M, P=4, F=0.02, miss=0.02, seed=1, sizes=None):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.5, size=M)
    freq = rng.beta((p * (1 - F) / F)[:, None], ((1 - p) * (1 - F) / F)[:, None], size=(M, P))
    if sizes is None:
        pop = np.arange(N) % P
    else:  # unequal populations: their eigenvalues spread
        w = np.asarray(sizes, dtype=np.float64)
        pop = np.searchsorted(np.cumsum(w / w.sum()), (np.arange(N) + 0.5) / N)
    geno = rng.binomial(2, freq[:, pop]).astype(np.int8)
    if miss > 0:
        geno[rng.random((M, N)) < miss] = 3
    return geno, pop


def zmat(geno):
    """Z (N x M) from synth.standardize with the markers outside M_used (no finite mstd) as zero columns, and M_used"""
    with np.errstate(all="ignore"):
        Z = synth.standardize(geno)
    good = np.isfinite(Z).all(axis=0) & (geno != 3).any(axis=1)  # (a marker missing everywhere is a zero column there already)
    Z[:, ~good] = 0.0
    return Z, good


def fix_sign(V, *others):
    for k in range(V.shape[0]):
        at = int(np.argmax(np.abs(V[k])))  # (the lowest index on a tie)
        if V[k, at] < 0:
            V[k] = -V[k]
            for o in others:
                o[k] = -o[k]


def numpy_pca(Z, m_used, K, L, iters, tol, Q0):
    """The algorithm of hgibbs_pca restated: same start panel, Householder QR, numpy.linalg.eigh for the Ritz step"""
    Q = np.linalg.qr(Q0.T)[0]
    prev, it = None, 0
    while True:
        it += 1
        T = Z.T @ Q
        th, W = np.linalg.eigh(T.T @ T)
        th, W = th[::-1], W[:, ::-1]
        change = np.inf if prev is None else np.max(np.abs(th[:K] - prev[:K]) / th[:K])
        prev = th
        if it >= iters or (tol > 0 and it > 1 and change <= tol):
            break
        Q = np.linalg.qr(Z @ T)[0]
    val = th[:K] / m_used
    V = (Q @ W[:, :K]).T.copy()
    ld = (T @ W[:, :K] / np.sqrt(th[:K])).T.copy()
    fix_sign(V, ld)
    return val, V, ld, it


def dense(Z, m_used, K):
    lam, U = np.linalg.eigh(Z @ Z.T / m_used)
    return lam[::-1], U[:, ::-1][:, :K].T


def vec_err(V, R):
    """max_k |v_k - s_k r_k|_2, s_k the sign that aligns them"""
    return max(float(np.linalg.norm(V[k] - np.sign(V[k] @ R[k]) * R[k])) for k in range(V.shape[0]))


def val_err(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


_M64 = (1 << 64) - 1


def mix64(z):
    """synth._mix64 on uint64 arrays"""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def start_panel(seed, L, n, row_begin=0):
    """The NumPy twin of k_pca_init: entry (k, i) = (2 x + 1 - 2^52) 2^-52, x the top 52 bits of mix64((seed ^ mix64(k)) + r c), r the
    handle's row row_begin + i (with a keep list, i counts the rows that were kept)"""
    Q0 = np.zeros((L, n))
    i = np.uint64(row_begin) + np.arange(n, dtype=np.uint64)
    for k in range(L):
        assert int(mix64(np.array([k], dtype=np.uint64))[0]) == synth._mix64(k)
        base = np.uint64((seed & _M64) ^ synth._mix64(k))
        with np.errstate(over="ignore"):
            h = mix64(base + i * np.uint64(0xD1B54A32D192ED03))
        x = (h >> np.uint64(12)).astype(np.int64)
        Q0[k] = np.ldexp((2 * x + 1 - (1 << 52)).astype(np.float64), -52)
    return Q0


def device(geno, keep=None):
    M, N = geno.shape
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N, keep=keep)
    return dev


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- the pieces of hg_pca.hip.h ----
def rows_of(P, vecmajor):
    """the panel as (rows, L) whatever its layout in memory: (L, rows) vector-major, (rows, L) row-major.  The layouts differ in the
    addresses k_pca_gram and k_pca_apply read, not in what they add to what."""
    return P.T if vecmajor else P


def gram_partials(P, vecmajor):
    """k_pca_gram: workgroup w owns rows [1024 w, 1024 w + 1024); entry (a, b) of its partial is acc = 0.0, then acc += x_a * x_b row
    after row.  Row r of every workgroup is taken in one NumPy statement: the sums of different workgroups and entries never meet."""
    X = rows_of(P, vecmajor)
    n, L = X.shape
    nb = (n + PG_ROWS - 1) // PG_ROWS
    partial = np.zeros((nb, L, L))
    for r in range(min(n, PG_ROWS)):
        x = X[r::PG_ROWS]  # row r of the workgroups that have one (all, or all but the last)
        partial[:x.shape[0]] += x[:, :, None] * x[:, None, :]
    return partial


def gram_sum(partial):
    """k_pca_gram_sum: s = 0.0, then the partials in workgroup order (its eight-at-a-time loop adds in the same order)"""
    s = np.zeros(partial.shape[1:])
    for w in range(partial.shape[0]):
        s += partial[w]
    return s


def gram(P, vecmajor):
    return gram_sum(gram_partials(P, vecmajor))


def chol_inv(G):
    """pca_chol_inv: (index of the first pivot that is not safely positive or -1, that pivot, R^-1)"""
    L = G.shape[0]
    G = [[float(v) for v in row] for row in G]
    R = [[0.0] * L for _ in range(L)]
    for j in range(L):
        d = G[j][j]
        for k in range(j):
            d -= R[k][j] * R[k][j]
        if not (d > 1e-13 * G[j][j]) or not math.isfinite(d):
            return j, d, None
        rjj = math.sqrt(d)
        R[j][j] = rjj
        for c in range(j + 1, L):
            s = G[j][c]
            for k in range(j):
                s -= R[k][j] * R[k][c]
            R[j][c] = s / rjj
    Rinv = [[0.0] * L for _ in range(L)]
    for c in range(L):
        Rinv[c][c] = 1.0 / R[c][c]
        for r in range(c - 1, -1, -1):
            s = 0.0
            for k in range(r + 1, c + 1):
                s -= R[r][k] * Rinv[k][c]
            Rinv[r][c] = s / R[r][r]
    return -1, 0.0, np.array(Rinv, dtype=np.float64).reshape(L, L)


def jacobi(S):
    """pca_jacobi: (converged, theta descending, W with W[l, k] = component l of vector k).  The three k-loops of a rotation touch a
    different pair of entries for every k, so each is one element-wise statement."""
    L = S.shape[0]
    A = np.array(S, dtype=np.float64)
    V = np.zeros((L, L))
    for i in range(L):
        V[i, i] = 1.0
    for i in range(L):
        for j in range(i + 1, L):
            A[i, j] = A[j, i] = 0.5 * (A[i, j] + A[j, i])
    done = False
    for sweep in range(61):
        offd = diag = 0.0
        for i in range(L):
            diag += float(A[i, i]) * float(A[i, i])
            for j in range(i + 1, L):
                offd += float(A[i, j]) * float(A[i, j])
        if not (offd > 1e-34 * diag):
            done = True
            break
        if sweep == 60:
            break
        for p in range(L - 1):
            for q in range(p + 1, L):
                apq = float(A[p, q])
                if apq == 0.0:
                    continue
                tau = (float(A[q, q]) - float(A[p, p])) / (2.0 * apq)
                t = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + math.sqrt(1.0 + tau * tau))
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = t * c
                akp, akq = A[:, p].copy(), A[:, q].copy()  # columns p, q
                A[:, p] = c * akp - s * akq
                A[:, q] = s * akp + c * akq
                apk, aqk = A[p, :].copy(), A[q, :].copy()  # rows p, q
                A[p, :] = c * apk - s * aqk
                A[q, :] = s * apk + c * aqk
                A[p, q] = A[q, p] = 0.0
                vkp, vkq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = c * vkp - s * vkq
                V[:, q] = s * vkp + c * vkq
    # std::stable_sort with A[x][x] > A[y][y]: descending, equal values in index order
    order = sorted(range(L), key=lambda x: -float(A[x, x]))
    theta = np.array([A[o, o] for o in order], dtype=np.float64)
    W = np.ascontiguousarray(V[:, order]) if L else V
    return done, theta, W


def apply(P, vecmajor, B, mstd=None):
    """k_pca_apply: out[k, i] = s, s = 0.0, then s += P(i, l) * B[l, k] for l = 0 .. L - 1; vector-major (K, rows).  With mstd, rows
    without a finite mstd are NaN."""
    X = rows_of(P, vecmajor)
    n, L = X.shape
    K = B.shape[1]
    out = np.zeros((K, n))
    for l in range(L):
        out += X[:, l][None, :] * B[l][:, None]
    if mstd is not None:
        out[:, ~np.isfinite(mstd)] = np.nan
    return out


def fold(T, mave, mstd):
    """k_pca_fold: T (M, nv) with the rows of unused markers zeroed IN T as well, and the weights a = t mstd, o = -(a mave), both
    (nv, M) and 0.0 at an unused marker"""
    used = np.isfinite(mstd)
    T = np.where(used[:, None], T, 0.0)
    with np.errstate(all="ignore"):
        w = np.where(used[:, None], T * mstd[:, None], 0.0)
        o = np.where(used[:, None], -(w * mave[:, None]), 0.0)
    return T, np.ascontiguousarray(w.T), np.ascontiguousarray(o.T)


def refusal(check, iteration=None, pivot=None, value=None):
    return {"refused": check, "iteration": iteration, "pivot": pivot, "value": value}


def restate(products, mave, mstd, n, M, K, L, iters, tol, Q0, want_loadings=True):
    """hgibbs_pca line by line.  products = (xt, xy): xt(V), V (nv, n) -> X'V as (M, nv) with NaN rows at unused markers
    (Device.marker_dots); xy(a, o), both (nv, M) -> (n, nv) (Device.score).  Returns a dict with eigval, pcs, loadings, iters_run,
    ritz_change, resid, m_used, or the refusal the code would end with: {"refused": which check, "iteration", "pivot", "value"}."""
    xt, xy = products
    mave, mstd = np.asarray(mave, dtype=np.float64), np.asarray(mstd, dtype=np.float64)
    if K < 1 or K > L or L > PG_LMAX or iters < 1 or not (tol >= 0.0) or not math.isfinite(tol) or L >= n:
        return refusal("arguments")
    Q0 = np.ascontiguousarray(Q0, dtype=np.float64)
    assert Q0.shape == (L, n) and mave.shape == (M,) and mstd.shape == (M,)
    if not np.isfinite(Q0).all():
        return refusal("Q0")
    m_used = int(np.count_nonzero(np.isfinite(mstd)))
    if L > m_used:
        return refusal("m_used")

    def orth(src, vecmajor, it):  # CholeskyQR, twice; the result is vector-major
        P, vm = src, vecmajor
        for _ in range(2):
            bad, piv, Rinv = chol_inv(gram(P, vm))
            if bad >= 0:
                return refusal("lost rank", it, bad, piv)
            P, vm = apply(P, vm, Rinv), 1
        return P

    # 1. the start panel, orthonormalised
    Q = orth(Q0, 1, 0)
    if isinstance(Q, dict):
        return Q
    it, change, prev = 0, math.inf, [0.0] * L
    while True:
        it += 1
        T, a, o = fold(xt(Q), mave, mstd)                  # 2. T = X'Q
        ok, theta, W = jacobi(gram(T, 0))                  # 3. S = T'T
        if not ok:
            return refusal("jacobi", it)
        for k in range(K):
            if not (theta[k] > 0.0) or not math.isfinite(theta[k]):
                return refusal("ritz value", it, k, float(theta[k]))
        if it > 1:
            change = 0.0
            for k in range(K):
                change = max(change, abs(float(theta[k]) - prev[k]) / float(theta[k]))
        prev = [float(v) for v in theta]
        if it >= iters or (tol > 0.0 and it > 1 and change <= tol):
            break
        Q = orth(xy(a, o), 0, it)                          # Y = X T, 4. Q = orth(Y)
        if isinstance(Q, dict):
            return Q

    # 5. Rayleigh-Ritz
    m = float(m_used)
    lam = np.array([float(theta[k]) / m for k in range(K)], dtype=np.float64)
    V = apply(Q, 1, np.ascontiguousarray(W[:, :K]))        # (K, n): what stays on the device for the report
    pcs = V.copy()
    loadings = None
    if want_loadings:
        B = np.array([[float(W[l, k]) / math.sqrt(float(theta[k])) for k in range(K)] for l in range(L)], dtype=np.float64).reshape(L, K)
        loadings = apply(T, 0, B, mstd)
    for k in range(K):  # sign: the entry of largest magnitude positive, the lowest index on a tie
        at = 0
        for i in range(1, n):
            if abs(pcs[k, i]) > abs(pcs[k, at]):
                at = i
        if pcs[k, at] < 0.0:
            pcs[k] = -pcs[k]
            if want_loadings:
                loadings[k] = -loadings[k]
    # the report: one more pair of products on the PCs as the device holds them (before the sign rule)
    _, a, o = fold(xt(V), mave, mstd)
    Y = xy(a, o)                                            # (n, K)
    D = Y / m - lam[None, :] * V.T
    G = gram(D, 0)
    resid = np.array([math.sqrt(float(G[k, k])) / float(lam[k]) for k in range(K)], dtype=np.float64)
    return {"eigval": lam, "pcs": pcs, "loadings": loadings, "iters_run": it, "ritz_change": change, "resid": resid, "m_used": m_used}


# ---- plain f64 products for the CPU checks ----
def marker_stats(geno):
    """mave, mstd as the chain defines them (synth.standardize): the mean over the called rows, sqrt((N - 1) / sum_called (g - mave)^2);
    not finite for a monomorphic marker (inf) or one missing everywhere (NaN)"""
    M, N = geno.shape
    called = geno != 3
    g = np.where(called, geno, 0).astype(np.float64)
    with np.errstate(all="ignore"):
        mave = g.sum(axis=1) / called.sum(axis=1)
        ss = np.where(called, (g - mave[:, None]) ** 2, 0.0).sum(axis=1)
        mstd = np.sqrt((N - 1) / ss)
    return mave, mstd


def cpu_products(geno):
    """(xt, xy), mave, mstd with NumPy's own matrix products in place of the device's operators"""
    mave, mstd = marker_stats(geno)
    used = np.isfinite(mstd)
    called = (geno != 3).astype(np.float64)            # (M, N)
    g = np.where(geno != 3, geno, 0).astype(np.float64)
    with np.errstate(all="ignore"):
        Zt = np.where((geno != 3) & used[:, None], (g - mave[:, None]) * mstd[:, None], 0.0)  # (M, N)

    def xt(V):
        out = Zt @ np.asarray(V, dtype=np.float64).T
        out[~used] = np.nan
        return out

    def xy(a, o):
        return g.T @ np.asarray(a).T + called.T @ np.asarray(o).T

    return (xt, xy), mave, mstd


# ---- the grid of tests/test_gpu_pca_exact.py (its premise, no refusal, is checked on the CPU) ----
SIZES = [3, 4, 5, 6]


def planted(n, M, drop=0, seed=11):
    """(geno as loaded (M, n + drop), keep or None, geno of the kept rows): structured(), unequal populations, 2 % missing calls, the
    last marker (inside the last block of 64) missing everywhere, marker M // 3 monomorphic, the kept row n // 2 missing everywhere"""
    N = n + drop
    geno, _ = structured(N, M, P=4, F=0.02, miss=0.02, seed=seed, sizes=SIZES)
    keep = None
    rows = np.arange(N)
    if drop:
        keep = np.ones(N, dtype=np.uint8)
        keep[np.random.default_rng(seed + 1).choice(N, size=drop, replace=False)] = 0
        rows = np.flatnonzero(keep)
    geno[M - 1] = 3
    geno[M // 3] = np.where(geno[M // 3] == 3, 3, 1)
    geno[:, rows[n // 2]] = 3
    return geno, keep, np.ascontiguousarray(geno[:, rows])


def case(name, n, M, K, L, iters=2, tol=0.0, drop=0, seed=11):
    return dict(name=name, n=n, M=M, K=K, L=L, iters=iters, tol=tol, drop=drop, seed=seed)


def grid():
    g = []
    for L in range(1, 33):  # every panel width; K < L for even L: the K-wide report pass beside the L-wide one
        g.append(case("width_L%d" % L, 130, 200, L if L % 2 else max(1, L // 2), L, drop=5 if L % 3 == 0 else 0))
    for n in (17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049):
        g.append(case("n%d" % n, n, 200, 3, 5, drop=7 if n in (65, 257, 1025) else 0))
    g.append(case("n6", 6, 200, 1, 5, iters=1))  # n = L + 1
    for M in (7, 63, 64, 65, 129, 1023, 1024, 1025, 2049):
        g.append(case("m%d" % M, 130, M, 3, 5, drop=3 if M in (65, 1025) else 0))
    for n, M in ((8192, 300), (8193, 300), (300, 8192), (300, 8200)):  # k_pca_gram_sum: nb = 8 and 9 on Y and on T
        g.append(case("sum_n%d_m%d" % (n, M), n, M, 2, 4))
    g.append(case("sum_n15400_m300", 15400, 300, 2, 3))  # nb = 16: two rounds of eight, no tail
    for L in (32, 31):
        g.append(case("wide_L%d" % L, 1025, 1025, 10, L, iters=3))
    return g


GRID = {c["name"]: c for c in grid()}
STOP = case("stop", 300, 1200, 3, 8, iters=40, tol=1e-6)
OPTIONS = case("options", 257, 700, 3, 8, iters=3, drop=9)
SEEDED = case("seeded", 193, 300, 3, 7, iters=2, drop=11)


def start_for(c):
    return np.random.default_rng(1000 + c["seed"] + c["L"]).standard_normal((c["L"], c["n"]))
