"""The summary-statistics chain on the host engine is the individual-level chain when the band covers every pair (DESIGN.md
section 31): hydra_ss_chain's iteration around hgibbs_ss_sweep_host, fed b = X'y and the whole of X'X (W = M - 1) from NumPy's
standardised columns, against the CPU oracle's chain (orc.Chain) for 4 iterations.  No device.

Equal: order, components, cass, the generator's position (tests/test_gpu_parity.py's _same_stream) and last_nnz.  Within that file's
`close`: beta, acum, sigmaG, pi, sigmaE, mu.  c_j against x_j'eps of the oracle's residual at 1e-9.

This test carries the claim "same chain".  The two chains round differently (a dot product over individuals against a running sum
over markers), so a decision prob <= acum could flip where the oracle's own margin |prob - acum| is below the tolerance; the seeds
of ss_common.CASES are ones where no decision of the 4 iterations is that close (none had to be replaced)."""
import numpy as np
import pytest

import ss_common as sc
from hydra_amd import capi


@pytest.mark.parametrize("name", [c[0] for c in sc.CASES])
def test_host_chain_is_the_oracles_chain(oracle, name):
    ref, _, X, band, b, kw = sc.oracle_case(oracle, name)
    M, N = sc.CASE_M, sc.CASE_N
    ch = capi.SsChain(None, N, M - 1, b, band=band, **kw)
    assert np.array_equal(ch.effects()[3], b)  # c = b while every effect is 0
    sc.assert_chain_matches_oracle(ch, ref, X)


def test_sweep_host_alone_one_sweep_against_the_oracles_sweep(oracle):
    """hgibbs_ss_sweep_host through its own binding: one sweep from the chain's start against orc_chain_sweep, identity order."""
    import ctypes as C
    ref, _, X, band, b, kw = sc.oracle_case(oracle, "missing-1group")
    M, N = sc.CASE_M, sc.CASE_N
    rx, ri = ref.rng_state()
    rng = capi.RngState()
    for k in range(624):
        rng.x[k] = int(rx[k])
    rng.idx = ri
    mS = kw["mS"]
    cVa = mS.copy()
    cVaI = np.zeros_like(mS)
    cVaI[:, 1:] = 1.0 / mS[:, 1:]
    c, beta, acum, comp = b.copy(), np.zeros(M), np.zeros(M), np.zeros(M, dtype=np.int32)
    order = np.arange(M, dtype=np.int32)
    cass, nnz = capi.ss_sweep_host(N, M - 1, None, band, c, beta, comp, acum, None, cVa, cVaI, order, ref.sigmaE, ref.arr("sigmaG"), ref.arr("estPi"),
                                   ref.arr("adaV"), rng)
    assert oracle.orc_chain_sweep(ref.h) == nnz
    assert np.array_equal(comp, ref.arr("components")) and np.array_equal(cass.ravel(), ref.arr("cass"))
    assert sc.same_stream(np.array(rng.x, dtype=np.uint32), int(rng.idx), *ref.rng_state())
    assert sc.close(beta, ref.arr("beta")) and sc.close(acum, ref.arr("acum"))
    assert sc.close(c, X.T @ ref.arr("eps"), 1e-9)


def test_refusals_name_the_argument():
    M, W = 5, 2
    z, zi = np.zeros(M), np.zeros(M, dtype=np.int32)
    cVa = np.array([[0.0, 0.01]])
    cVaI = np.array([[0.0, 100.0]])
    band = np.zeros((M, W))
    args = lambda **kw: dict(dict(n_eff=100.0, W=W, ahead=None, band=band, c=z.copy(), beta=z.copy(), components=zi.copy(), acum=z.copy(), groups=None,
                                  cVa=cVa, cVaI=cVaI, order=np.arange(M), sigmaE=0.5, sigmaG=np.array([0.1]), estPi=np.array([0.5, 0.5]),
                                  adaV=np.ones(M, dtype=np.uint8), rng=capi.RngState()), **kw)
    for kw, msg in ((dict(n_eff=1.0), "n_eff"), (dict(n_eff=float("nan")), "n_eff"), (dict(ahead=np.array([2, 2, 2, 2, 0])), "past the last marker"),
                    (dict(ahead=np.array([3, 0, 0, 0, 0])), "above W"), (dict(order=np.array([0, 1, 2, 3, 5])), "order[4]"),
                    (dict(groups=np.array([0, 0, 1, 0, 0])), "group")):
        with pytest.raises(capi.HgError) as e:
            capi.ss_sweep_host(**args(**kw))
        assert msg in str(e.value), (kw, str(e.value))
    with pytest.raises(capi.HgError) as e:
        capi.SsChain(None, 100, 4097, z, band=np.zeros((M, 4097)))
    assert "W must be in [1, 4096]" in str(e.value)


def test_non_positive_e_sqn_stops_the_iteration_by_name():
    """A band that is not positive definite (every neighbour at r = -1... beyond what a correlation matrix allows) with large effects:
    e_sqn <= 0 ends the iteration with the iteration's number and the value; nothing is clamped."""
    M, W, n = 6, 1, 50.0
    band = np.full((M, W), -3.0 * (n - 1))  # |r| = 3: no panel gives this
    band[M - 1] = 0.0
    b = np.full(M, 40.0)
    ch = capi.SsChain(None, n, W, b, band=band, mS=np.array([[0.0, 1.0]]), seed=3)
    with pytest.raises(capi.HgError) as e:
        for _ in range(50):
            ch.iterate()
    assert "iteration" in str(e.value) and "e_sqn = " in str(e.value) and "not positive" in str(e.value)
