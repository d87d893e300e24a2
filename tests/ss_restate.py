"""The summary-statistics sweep restated on a dense matrix (no test of its own): plain NumPy and ctypes on the
oracle's exports.  Nothing here comes from hg_ss_step.h or hg_sumstat.cpp -- no `back` array, no window arithmetic, no tables of a
sweep, no grouping of the order: the band becomes a symmetric (M, M) matrix once, and a non-zero step is c += delta A[:, j].

The per-marker step is the oracle's own (orc_marker_draw, oracle/orc_gibbs.cpp:333-387) where n_eff is integral, and `step_py`, the
same lines written out in Python's float64 around the oracle's two draws (orc_rng_unif, orc_rng_norm), where it is not.  `step_py`
also says what the oracle's function does not return: which shares the 700 rule zeroed, and how far each decision lay from its
threshold.  The tests take their conditions on the inputs from that log alone."""
import ctypes as C
import math

import numpy as np

import orc

INF = float("inf")


def rng_from(words, idx):
    """An oracle generator from 624 words and an index (hgibbs_rng_state's layout: the two structs are the same bytes)"""
    g = orc.OrcMt()
    for k in range(624):
        g.x[k] = int(words[k])
    g.idx = int(idx)
    return g


def rng_words(g):
    return np.array(g.x, dtype=np.uint32), int(g.idx)


def _copy(g):
    c = orc.OrcMt()
    C.memmove(C.byref(c), C.byref(g), C.sizeof(orc.OrcMt))
    return c


def dense(band, ahead, n_eff):
    """(M, M) float64, symmetric: A[j, j + d] = A[j + d, j] = band[j, d - 1] for 1 <= d <= ahead[j], n_eff - 1 on the diagonal, 0 elsewhere"""
    M = band.shape[0]
    A = np.zeros((M, M))
    for j in range(M):
        for d in range(1, int(ahead[j]) + 1):
            A[j, j + d] = A[j + d, j] = band[j, d - 1]
        A[j, j] = n_eff - 1.0
    return A


# IEEE semantics for the three operations that Python's float refuses at the edges
def _div(a, b):
    if b == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def _log(x):
    if x == 0.0:
        return -INF
    return math.log(x) if x > 0.0 else math.nan


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def step_py(L, num, beta_old, dNm1, K, cVa_g, cVaI_g, estPi_g, sigmaE, sigmaG_g, rng):
    """oracle/orc_gibbs.cpp:333-387 in Python's float64, the operations in that order, the uniform before the walk; dNm1 = n - 1 as a
    double.  Returns (beta_new, component, acum, zeroed, margin, cut): zeroed[k] says that the 700 rule makes the share of component k
    zero (for every k, walked or not: a share k >= 1 entered acum iff component >= k); margin is the smallest |prob - acum| over the
    comparisons that decided something (those before the last component), inf where there was none; cut is the largest share that the
    rule replaced by 0 on the walk -- next to nothing where a later component lies 700 above (its exponential swamps the sum anyway),
    up to 1 where one lies 700 below: only there does the rule change what is drawn."""
    km1 = K - 1
    sigE_G = _div(sigmaE, sigmaG_g)
    sigG_E = _div(sigmaG_g, sigmaE)
    i_2sigE = _div(1.0, 2.0 * sigmaE)
    denom = [0.0] * K
    muk = [0.0] * K
    for i in range(1, K):
        denom[i] = dNm1 + sigE_G * cVaI_g[i]
    num = num + beta_old * dNm1
    for i in range(1, K):
        muk[i] = _div(num, denom[i])
    logL = [_log(estPi_g[i]) for i in range(K)]
    for i in range(1, K):
        logL[i] = logL[i] - 0.5 * _log(sigG_E * dNm1 * cVa_g[i] + 1.0) + muk[i] * num * i_2sigE

    prob = L.orc_rng_unif(rng)

    def share(k):
        s = 0.0
        for l in range(K):
            s += _exp(logL[l] - logL[k])
        return _div(1.0, s)

    # (the oracle tests the components from 1 on against component 0, and those from k on against k for k >= 1: the later ones)
    zeroed = tuple(any(abs(logL[l] - logL[k]) > 700.0 for l in range(k + 1, K)) for k in range(K))
    cut = share(0) if zeroed[0] else 0.0
    acum = 0.0 if zeroed[0] else share(0)
    acum0 = acum
    margin = INF
    for k in range(K):
        if k < km1:
            margin = min(margin, abs(prob - acum))
        if prob <= acum or k == km1:
            beta_new = 0.0 if k == 0 else L.orc_rng_norm(rng, muk[k], _div(sigmaE, denom[k]))
            return beta_new, k, acum0, zeroed, margin, cut
        if zeroed[k + 1]:
            cut = max(cut, share(k + 1))
        else:
            acum += share(k + 1)
    raise AssertionError("the walk ends at component K - 1")


def sweep(L, A, c, beta, comp, acum, groups, cVa, cVaI, order, sigmaE, sigmaG, estPi, mask, rng, n_eff, use_orc):
    """One sweep over `order` on the dense matrix A, in place on c, beta, comp and acum (float64 / int32 arrays of M entries); cVa,
    cVaI, estPi (G, K); sigmaG (G,); groups (M,) or None; rng: orc.OrcMt, advanced.  A masked marker takes the step -- the oracle's
    orc_marker_draw where use_orc is set (n_eff must be integral), step_py otherwise --, any other gets beta 0 and acum 1; a
    non-zero delta = old - new is c += delta A[:, j].  Returns (cass[G, K], nnz, log), log[i] = (j, zeroed, component, margin,
    beta_old, beta_new, cut) of the i-th step taken; zeroed, margin and cut are step_py's in both modes (run on a copy of the generator beside
    the oracle's function, whose results are the ones kept)."""
    cVa, cVaI, estPi = (np.ascontiguousarray(a, dtype=np.float64).reshape(cVa.shape) for a in (cVa, cVaI, estPi))
    G, K = cVa.shape
    dNm1 = float(n_eff) - 1.0
    if use_orc:
        assert float(n_eff) == int(n_eff), "orc_marker_draw takes an integral n"
    cass = np.zeros((G, K), dtype=np.int32)
    nnz = 0
    log = []
    bn, kk, ac = C.c_double(), C.c_int(), C.c_double()
    for j in (int(x) for x in order):
        g = 0 if groups is None else int(groups[j])
        old = float(beta[j])
        if mask[j]:
            args = (float(c[j]), old, dNm1, K, [float(x) for x in cVa[g]], [float(x) for x in cVaI[g]], [float(x) for x in estPi[g]], float(sigmaE),
                    float(sigmaG[g]))
            if use_orc:
                _, _, _, zeroed, margin, cut = step_py(L, *args, _copy(rng))
                rc = L.orc_marker_draw(float(c[j]), old, int(n_eff), K, orc.dptr(cVa[g]), orc.dptr(cVaI[g]), orc.dptr(estPi[g]), float(sigmaE),
                                       float(sigmaG[g]), C.byref(rng), C.byref(bn), C.byref(kk), C.byref(ac))
                assert rc == 0, "orc_marker_draw: the component walk found no component"
                new, k, a0 = bn.value, kk.value, ac.value
            else:
                new, k, a0, zeroed, margin, cut = step_py(L, *args, rng)
            cass[g, k] += 1
            comp[j] = k
            beta[j] = new
            acum[j] = a0
            log.append((j, zeroed, k, margin, old, new, cut))
        else:
            beta[j] = 0.0
            acum[j] = 1.0
        delta = old - float(beta[j])
        if delta != 0.0:
            c += delta * A[:, j]
            nnz += 1
    return cass, nnz, log


def invariant(xty, A, beta):
    """b - A beta in longdouble"""
    ld = np.longdouble
    return np.asarray(xty, dtype=ld) - np.asarray(A, dtype=ld) @ np.asarray(beta, dtype=ld)
