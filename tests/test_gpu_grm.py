"""The genomic relationship matrix (hgibbs_grm, hydra_mi355x --grm) against an integer restatement of its definition in NumPy: bit
for bit; against plain f64 within the stated bound; bit identity across splits, row pieces and repeats; planted cases; agreement
with hgibbs_pca's eigenvalues; the refusals; the CLI's GCTA files."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")

pytestmark = pytest.mark.gpu

VAL_BOUND = 2.2e-14  # tests/test_gpu_pca.py: eigenvalues of hgibbs_pca against NumPy's dense decomposition


def make(N, M, seed):
    """tests/test_gpu_king.py's recipe"""
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


# ---- the definition, restated on integers ----
def table(mave, mstd):
    """used (M,), y and z (M, 3) f64 with every operation rounded on its own, W, E, qy and qz (M, 3) int64"""
    used = np.isfinite(mstd)
    g = np.arange(3.0)
    with np.errstate(all="ignore"):
        y = (mstd * mstd)[:, None] * (g[None, :] - mave[:, None])
        z = mave[:, None] * y
    y[~used] = 0.0
    z[~used] = 0.0
    W = float(max(np.abs(y).max(), np.abs(z).max())) if used.any() else 0.0
    E = 52 - math.frexp(W)[1] if W > 0.0 else 0  # W < 2^e
    qy = np.rint(np.ldexp(y, E)).astype(np.int64)  # (round half to even, as llrint)
    qz = np.rint(np.ldexp(z, E)).astype(np.int64)
    assert max(np.abs(qy).max(), np.abs(qz).max()) <= (1 << 52)  # (W 2^E < 2^52 before the rounding)
    return used, y, z, W, E, qy, qz


def restate(geno, mave, mstd, a0, acount):
    """Rows [a0, a0 + acount) against every column b: T as Python integers (acount, N), S (acount, N) rounded once, NSNP, M_used, E, W.
    Every f64 matrix product is one of 26-bit halves of q against codes 0, 1, 2: below 2^53, exact."""
    used, _, _, W, E, qy, qz = table(mave, mstd)
    g = np.ascontiguousarray(geno.T).astype(np.int64)  # (N, M)
    called = g != 3
    gz = np.where(called, g, 0)
    G = gz.astype(np.float64)                              # code side: g, 0 at a missing call
    C = called.astype(np.float64)                          # code side: [called]
    ga = gz[a0:a0 + acount]
    ca = called[a0:a0 + acount]
    cols = np.arange(geno.shape[0])[None, :]
    wy = np.where(ca, qy[cols, ga], 0)                     # weight side: qy[j][g_aj], 0 at a missing call
    wz = np.where(ca, qz[cols, ga], 0)
    mask = (1 << 26) - 1
    parts = []
    for q in (wy, wz):
        parts.append(((q >> 26).astype(np.float64), (q & mask).astype(np.float64)))
    assert geno.shape[0] * 2.0 * (1 << 26) < 2.0 ** 53
    hi = parts[0][0] @ G.T - parts[1][0] @ C.T
    lo = parts[0][1] @ G.T - parts[1][1] @ C.T
    T = hi.astype(np.int64).astype(object) * (1 << 26) + lo.astype(np.int64).astype(object)
    S = np.array([math.ldexp(float(t), -E) for t in T.ravel()]).reshape(T.shape)  # int -> float rounds once, to nearest even
    nsnp = ((ca & used[None, :]).astype(np.float64) @ C.T).astype(np.int64)
    return T, S, nsnp, int(used.sum()), E, W


def packed(full, a0, acount):
    """rows a0 .. of an (acount, N) array, each with its columns 0 .. a, in GCTA's order"""
    return np.concatenate([full[a - a0, :a + 1] for a in range(a0, a0 + acount)])


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def check_rows(dev, geno, a0, acount):
    mave, mstd = dev.marker_stats()[:2]
    _, S, nsnp, m_used, E, _ = restate(geno, mave, mstd, a0, acount)
    if m_used == 0:  # (the smallest shapes: every marker monomorphic or missing) the matrix is not defined
        with pytest.raises(capi.HgError, match="M_used = 0"):
            dev.grm(a0, acount)
        return None, None
    got_S, got_n = dev.grm(a0, acount)
    assert np.array_equal(got_n.astype(np.int64), packed(nsnp, a0, acount))
    assert np.array_equal(bits(got_S), bits(packed(S, a0, acount)))
    assert dev.grm_info() == (m_used, E)
    return got_S, got_n


@functools.lru_cache(maxsize=None)
def case(N, M, seed):
    """data, device and the whole triangle of one shape, made once and left unchanged"""
    geno = make(N, M, seed)
    dev = device(geno)
    S, nsnp = check_rows(dev, geno, 0, N)
    S.setflags(write=False)
    nsnp.setflags(write=False)
    return geno, dev, S, nsnp


def unpack(v, N):
    full = np.zeros((N, N), dtype=v.dtype)
    full[np.tril_indices(N)] = v
    return full


# ---- 1. bit-exact against the restatement ----
@pytest.mark.parametrize("M", [1, 63, 64, 65, 2049])
@pytest.mark.parametrize("N", [2, 15, 16, 17, 63, 65, 129, 513])
def test_bit_exact_against_the_restatement(N, M):
    if (N, M) == (513, 2049):
        case(N, M, 513 * 7 + 2049)
        return
    geno = make(N, M, seed=N * 7 + M)
    check_rows(device(geno), geno, 0, N)


def test_bit_exact_last_rows_of_several_blocks():
    N, M = 4097, 65
    geno = make(N, M, seed=N * 7 + M)
    check_rows(device(geno), geno, N - 100, 100)


def test_triangle_in_several_pieces():
    """more than 2^25 pairs in one call: pieces of rows inside it, the second one starting off a tile boundary"""
    N, M = 8300, 65
    geno = make(N, M, seed=31)
    dev = device(geno)
    first = next(a for a in range(N) if (a + 1) * (a + 2) // 2 > (1 << 25))  # the first row of the second piece
    assert 0 < first < N - 60 and first % 16 != 0
    S, nsnp = dev.grm()
    a0, acount = first - 40, 100
    mave, mstd = dev.marker_stats()[:2]
    _, rS, rn, _, _, _ = restate(geno, mave, mstd, a0, acount)
    off = a0 * (a0 + 1) // 2
    want_S, want_n = packed(rS, a0, acount), packed(rn, a0, acount)
    assert np.array_equal(nsnp[off:off + want_n.size].astype(np.int64), want_n)
    assert np.array_equal(bits(S[off:off + want_S.size]), bits(want_S))
    # the last rows, and the rows on their own
    tail_S, tail_n = dev.grm(N - 3, 3)
    assert np.array_equal(bits(S[-tail_S.size:]), bits(tail_S)) and np.array_equal(nsnp[-tail_n.size:], tail_n)
    part_S, part_n = dev.grm(a0, acount)
    assert np.array_equal(bits(part_S), bits(want_S)) and np.array_equal(part_n.astype(np.int64), want_n)


# ---- 2. against plain f64 ----
def test_against_plain_f64():
    N, M = 513, 2049
    geno, dev, S, _ = case(N, M, 513 * 7 + 2049)
    mave, mstd = dev.marker_stats()[:2]
    used, _, _, W, _, _, _ = table(mave, mstd)
    m_used = int(used.sum())
    g = geno.T.astype(np.float64)
    with np.errstate(all="ignore"):
        X = (g - mave[None, :]) * mstd[None, :]
    X[(geno.T == 3) | ~used[None, :]] = 0.0
    XL = X.astype(np.longdouble)
    ref = (XL @ XL.T)[np.tril_indices(N)]
    err = float(np.max(np.abs(S.astype(np.longdouble) - ref)))
    bound = 3.0 * m_used * W * 2.0 ** -52 + 2.0 ** -40 * m_used
    print("MEASURED |S - X X'| max %.3g, bound %.3g (M_used %d, W %.6g)" % (err, bound, m_used, W))
    assert err <= bound


# ---- 3. bit identity ----
def test_bit_identity():
    N, M = 700, 2049
    geno, dev, S, nsnp = case(N, M, 5)
    for split in (1, 2, 3, 7, 33, 0):
        dev.set_option("grm_split", split)
        s2, n2 = dev.grm()
        assert np.array_equal(bits(s2), bits(S)) and np.array_equal(n2, nsnp), "grm_split=%d" % split
    for step in (1, 37, 128, 129):
        got = [dev.grm(a0, min(step, N - a0)) for a0 in range(0, N, step)]
        assert np.array_equal(bits(np.concatenate([x[0] for x in got])), bits(S)), "row pieces of %d" % step
        assert np.array_equal(np.concatenate([x[1] for x in got]), nsnp), "row pieces of %d" % step
    s2, n2 = dev.grm()
    assert np.array_equal(bits(s2), bits(S)) and np.array_equal(n2, nsnp)
    assert dev.last_grm_ms() > 0.0
    # either output alone
    s3 = np.zeros(S.size)
    capi.check(dev.L.hgibbs_grm(dev.h, 0, N, capi._dp(s3), None))
    assert np.array_equal(bits(s3), bits(S))


# ---- 4. the planted cases ----
def test_planted_cases():
    N, M = 513, 2049
    geno, dev, S, nsnp = case(N, M, 513 * 7 + 2049)
    F, Fn = unpack(S, N), unpack(nsnp, N)
    # the duplicate pair
    assert np.array_equal(geno[:, 1], geno[:, N - 1])
    assert bits(F[N - 1, 1]) == bits(F[1, 1]) == bits(F[N - 1, N - 1])
    assert Fn[N - 1, 1] == Fn[1, 1] == Fn[N - 1, N - 1] > 0
    # the individual missing everywhere: row and column
    i = N // 2
    assert not Fn[i, :i + 1].any() and not Fn[i:, i].any()
    assert not F[i, :i + 1].any() and not F[i:, i].any()
    # an unused marker changes nothing
    _, E = dev.grm_info()
    mstd = dev.marker_stats()[1]
    drop = ~np.isfinite(mstd)
    assert drop[M // 3] and drop[M // 2] and drop[M - 2]
    dev2 = device(np.ascontiguousarray(geno[~drop]))
    S2, n2 = dev2.grm()
    assert dev2.grm_info() == (int((~drop).sum()), E)
    assert np.array_equal(bits(S2), bits(S)) and np.array_equal(n2, nsnp)


# ---- 5. agreement with --pca ----
def test_eigenvalues_agree_with_pca():
    """clean data (no missing call) with five populations: four eigenvalues stand clear of the rest, so the subspace iteration has
    converged to rounding after 40 iterations on a panel of 16"""
    N, M, K = 300, 2049, 4
    rng = np.random.default_rng(19)
    p = rng.uniform(0.05, 0.5, size=M)
    Fst = 0.1
    freq = rng.beta((p * (1 - Fst) / Fst)[:, None], ((1 - p) * (1 - Fst) / Fst)[:, None], size=(M, 5))
    geno = rng.binomial(2, freq[:, np.arange(N) % 5]).astype(np.int8)
    dev = device(geno)
    S, _ = dev.grm()
    m_used, _ = dev.grm_info()
    full = unpack(S, N)
    full = full + np.tril(full, -1).T
    lam = np.linalg.eigvalsh(full / m_used)[::-1][:K]
    val, _, _, rep = dev.pca(K, L=16, iters=40, tol=0.0, seed=3)
    err = float(np.max(np.abs(val - lam) / np.abs(lam)))
    print("MEASURED eigenvalues: grm %s, pca %s, relative difference %.3g" % (lam, val, err))
    assert rep["m_used"] == m_used
    assert err <= VAL_BOUND


# ---- 6. refusals through the C ABI ----
def test_refusals():
    N, M = 40, 70
    geno = make(N, M, seed=1)
    dev = device(geno)
    with pytest.raises(capi.HgError, match="out of range"):
        dev.grm(39, 2)
    with pytest.raises(capi.HgError, match="out of range"):
        dev.grm(0, 41)
    assert dev.grm_info() == (0, 0) and dev.last_grm_ms() == 0.0
    check_rows(dev, geno, 0, N)
    with pytest.raises(capi.HgError, match="acount = 0"):
        dev.grm(3, 0)
    check_rows(dev, geno, 3, 30)
    with pytest.raises(capi.HgError, match="grm_split"):
        dev.set_option("grm_split", -1)
    with pytest.raises(capi.HgError, match="no genotypes"):
        capi.Device(0).grm(0, 1)
    # every marker monomorphic: M_used = 0; the handle goes on serving its other operators
    mono = np.ones((M, N), dtype=geno.dtype)
    mono[::2] = 2
    dm = device(mono)
    with pytest.raises(capi.HgError, match="M_used = 0"):
        dm.grm()
    assert dm.grm_info() == (0, 0)
    assert np.all(dm.king()[..., 0] == M)
    check_rows(dev, geno, 0, N)


# ---- 7. the CLI ----
def test_cli_gcta_files(tmp_path):
    N, M = 200, 300
    geno = make(N, M, seed=23)
    y = np.random.default_rng(4).standard_normal(N)
    na = [3, 150]
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=na)
    kept = np.setdiff1d(np.arange(N), na)
    n = len(kept)
    assert n == 198
    out = str(tmp_path / "o" / "g")
    os.makedirs(str(tmp_path / "o"))
    cmd = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"),
           "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(M), "--grm", "--grm-out", out,
           "--grm-sparse", "0.05"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    keep = np.zeros(N, dtype=np.uint8)
    keep[kept] = 1
    dev = device(geno, keep=keep)
    S, nsnp = dev.grm()
    m_used, _ = dev.grm_info()
    with np.errstate(all="ignore"):
        A = np.where(nsnp != 0, S / nsnp, np.nan)
    with open(out + ".grm.id") as f:
        assert f.read() == "".join("fam%d\tind%d\n" % (i, i) for i in kept)
    gb = np.fromfile(out + ".grm.bin", dtype="<f4")
    gn = np.fromfile(out + ".grm.N.bin", dtype="<f4")
    assert gb.size == gn.size == n * (n + 1) // 2
    assert np.array_equal(gn, nsnp.astype(np.float32))
    assert np.isnan(A).any()  # (the individual missing everywhere)
    assert np.array_equal(gb.view(np.uint32), A.astype(np.float32).view(np.uint32))
    a, b = np.tril_indices(n)
    with np.errstate(invalid="ignore"):
        sel = (a == b) | (A >= 0.05)
    with open(out + ".grm.sp") as f:
        rows = [ln.split("\t") for ln in f.read().splitlines()]
    assert [(int(x[0]), int(x[1])) for x in rows] == list(zip(a[sel].tolist(), b[sel].tolist()))
    assert int(np.sum(sel & (a != b))) > 0
    for x, want in zip(rows, A[sel]):
        v = float(x[2])
        assert (math.isnan(v) and math.isnan(want)) or abs(v - want) <= 5e-9 * abs(want), (x, want)
    assert "GRM    : %d rows, %d of %d markers used, %d entries written to %s.grm.bin" % (n, m_used, M, n * (n + 1) // 2, out) in r.stdout
    assert "%d off-diagonal pairs with A >= 0.05 in %s.grm.sp" % (int(np.sum(sel & (a != b))), out) in r.stdout
    # the default prefix is <dir>/<name>
    r = subprocess.run(cmd[:cmd.index("--grm-out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(str(tmp_path / "o" / "n.grm.bin"), dtype="<f4").view(np.uint32), gb.view(np.uint32))
    assert not os.path.exists(str(tmp_path / "o" / "n.grm.sp"))
