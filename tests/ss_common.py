"""What the summary-statistics tests share (no test of its own): the cases, NumPy's restatement of the chain's standardised columns
with b = X'y and the band of X'X, and the rule by which a summary-statistics chain is held to the oracle's individual-level chain."""
import numpy as np

import orc
from hydra_amd import synth

BETA_TOL = 1e-9  # tests/test_gpu_parity.py's


def close(a, b, tol=BETA_TOL):
    """tests/test_gpu_parity.py's `close`"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))


def same_stream(xa, ia, xb, ib):
    """tests/test_gpu_parity.py's `_same_stream`: two MT19937 states are the same generator iff their next outputs agree."""
    L = orc.load()
    ga, gb = orc.OrcMt(), orc.OrcMt()
    for g, x, i in ((ga, xa, ia), (gb, xb, ib)):
        for k in range(624):
            g.x[k] = int(x[k])
        g.idx = int(i)
    return all(L.orc_rng_u32(ga) == L.orc_rng_u32(gb) for _ in range(1300))


def make_case(M, N, seed=7, missing_rate=0.02):
    geno = synth.make_genotypes(M, N, seed=seed, missing_rate=missing_rate)
    y, _ = synth.make_phenotype(geno, seed=seed + 1, h2=0.5, causal_frac=0.05)
    return synth.pack_bed_columns(geno), y


MS1 = np.array([[0.0, 0.0001, 0.001, 0.01]])
MS2 = np.array([[0.0, 0.0001, 0.001, 0.01], [0.0, 0.001, 0.01, 0.1]])
# (name, missing rate, mixtures G x K, groups of marker j, seed): M = 300, N = 517, K = 4; 2 % missing calls and none, one group and two
CASES = [
    ("missing-1group", 0.02, MS1, None, 1222),
    ("clean-1group", 0.0, MS1, None, 77),
    ("missing-2groups", 0.02, MS2, lambda M: (np.arange(M) % 2).astype(np.int32), 5),
    ("clean-2groups", 0.0, MS2, lambda M: (np.arange(M) >= M // 3).astype(np.int32), 901),
]
CASE_M, CASE_N = 300, 517


def standardised(bed, N, mave, mstd):
    """(N, M) float64: the chain's columns, x = (g - mave) mstd at a called genotype, 0 at a missing one (code 1; 0 -> 2, 2 -> 1, 3 -> 0)."""
    M = bed.shape[0]
    codes = ((bed[:, :, None] >> (2 * np.arange(4, dtype=np.uint8))) & 3).reshape(M, -1)[:, :N]
    g = np.array([2.0, 0.0, 1.0, 0.0])[codes]
    X = (g - mave[:, None]) * mstd[:, None]
    X[codes == 1] = 0.0
    return np.ascontiguousarray(X.T)


def full_band(X, W=None):
    """B = X'X as the engines take it: (M, W) with band[j, d - 1] = B[j, j + d], 0 past the last marker; W = M - 1 covers every pair."""
    M = X.shape[1]
    W = M - 1 if W is None else W
    B = X.T @ X
    band = np.zeros((M, W))
    for j in range(M):
        n = min(W, M - 1 - j)
        band[j, :n] = B[j, j + 1:j + 1 + n]
    return band


def oracle_case(L, name):
    """The oracle's chain of a case with what the summary-statistics chain of the same case takes: (ref, X, n, W, band, b, kwargs)."""
    _, miss, mS, grp, seed = next(c for c in CASES if c[0] == name)
    bed, y = make_case(CASE_M, CASE_N, seed=seed % 50 + 3, missing_rate=miss)
    groups = None if grp is None else grp(CASE_M)
    ref = orc.Chain(L, bed, CASE_N, y, groups=groups, mS=mS, seed=seed)
    X = standardised(bed, CASE_N, ref.arr("mave"), ref.arr("mstd"))
    b = X.T @ ref.arr("y")
    return ref, bed, X, full_band(X), b, dict(mS=mS, groups=groups, seed=seed)


def assert_chain_matches_oracle(ch, ref, X, iters=4):
    """ch: a capi.SsChain over the full band of ref's genotypes.  Order, components, cass, the generator and last_nnz are equal; beta, acum,
    sigmaG, pi, sigmaE and mu are `close`; c_j is x_j'eps of the oracle's residual at 1e-9."""
    for it in range(iters):
        ref.iterate()
        ch.iterate()
        st = ch.state()
        beta, comp, acum, c = ch.effects()
        assert np.array_equal(ch.order(), ref.arr("order")), it
        assert np.array_equal(comp, ref.arr("components")), it
        assert np.array_equal(st["cass"].ravel(), ref.arr("cass")), it
        assert ch.last_nnz() == ref.L.orc_chain_last_nnz(ref.h), it
        rx, ri = ref.rng_state()
        assert same_stream(st["rng_x"], st["rng_idx"], rx, ri), it
        assert close(beta, ref.arr("beta")), it
        assert close(acum, ref.arr("acum")), it
        assert close(st["sigmaG"], ref.arr("sigmaG")), it
        assert close(st["estPi"].ravel(), ref.arr("estPi")), it
        assert close(st["sigmaE"], ref.sigmaE), it
        assert close(st["mu"], ref.mu), it
        assert close(c, X.T @ ref.arr("eps"), 1e-9), it
