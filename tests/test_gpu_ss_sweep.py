"""The device engine of the summary-statistics sweep (hgibbs_ss_sweep) held to the host engine
(hgibbs_ss_sweep_host) over three sweeps on the same band, fetched with hgibbs_ss_band_get.  Components, cass, nnz and the generator
(its 624 words and its index) are equal; beta, acum and c are within tests/test_gpu_parity.py's `close`.  Two device runs from the
same state give the same bits.

Shapes: the smallest at which the kernel can go wrong -- one marker; two with W = 1; 257 markers with windows of 1, 5, 64, 256 (as wide
as the workgroup) and 300 (wider than it, and than the markers left); windows of mixed lengths with zeros; 1500 markers, so that a
sweep crosses more than one 624-word generator block; K = 2 and K = 8 (the largest hgibbs_set_model takes); adaV = 0 at some markers;
a group with sigmaG = 0; shuffled and identity order; a start from non-zero effects, so that a step back to 0 is exercised."""
import numpy as np
import pytest

import ss_common as sc
from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu

N = 131
MS4 = sc.MS1
MS2K = np.array([[0.0, 0.01]])
MS8 = np.array([[0.0, 1e-5, 1e-4, 1e-3, 3e-3, 1e-2, 3e-2, 1e-1]])


def seeded(seed):
    r = capi.RngState()
    x = seed & 0xffffffff
    r.x[0] = x
    for i in range(1, 624):
        x = (1812433253 * (x ^ (x >> 30)) + i) & 0xffffffff
        r.x[i] = x
    r.idx = 624
    return r


def copy_rng(r):
    c = capi.RngState()
    for i in range(624):
        c.x[i] = r.x[i]
    c.idx = r.idx
    return c


def run_device(dev, n_eff, W, ahead, xty, beta0, plan):
    dev.ss_begin(n_eff, W, xty, ahead)
    if beta0 is not None:
        dev.set_beta(beta0)
    rng = seeded(plan["seed"])
    out = []
    for order, sigmaE, sigmaG, estPi, adaV in plan["sweeps"]:
        cass, nnz = dev.ss_sweep(order, sigmaE, sigmaG, estPi, adaV, rng)
        beta, comp, acum = dev.get_beta()
        c, sb, sc_ = dev.ss_state()
        out.append(dict(cass=cass, nnz=nnz, beta=beta, comp=comp, acum=acum, c=c, sb=sb, sc=sc_, x=np.array(rng.x, dtype=np.uint32), idx=int(rng.idx)))
    return out


def check_case(M, W, mS=MS4, ahead=None, groups=None, zero_group=False, shuffle=True, nonzero_start=False, some_fixed=True, seed=11):
    G, K = mS.shape
    rs = np.random.default_rng(seed)
    geno = synth.make_genotypes(M, N, seed=seed, missing_rate=0.02)
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    n_eff = 4000.0
    xty = rs.normal(0.0, np.sqrt(n_eff), M)
    xty[rs.random(M) < 0.15] *= 8.0  # signals: effects that leave 0, and come back
    cVa = mS.copy()
    cVaI = np.zeros_like(mS)
    cVaI[:, 1:] = 1.0 / mS[:, 1:]
    dev.set_model(groups, cVa, cVaI)
    beta0 = np.where(rs.random(M) < 0.3, rs.normal(0.0, 0.05, M), 0.0) if nonzero_start else None
    sweeps = []
    for s in range(3):
        order = rs.permutation(M).astype(np.int32) if shuffle else np.arange(M, dtype=np.int32)
        sigmaG = rs.uniform(0.2, 0.6, G)
        if zero_group:
            sigmaG[G - 1] = 0.0
        estPi = rs.dirichlet(np.ones(K) * 2.0, G)
        adaV = (rs.random(M) < 0.85).astype(np.uint8) if some_fixed else np.ones(M, dtype=np.uint8)
        sweeps.append((order, 0.4 + 0.1 * s, sigmaG, estPi, adaV))
    plan = dict(seed=seed + 100, sweeps=sweeps)

    got = run_device(dev, n_eff, W, ahead, xty, beta0, plan)
    band = dev.ss_band()
    # the host engine on the device's band
    c, beta = xty.copy(), (beta0.copy() if beta0 is not None else np.zeros(M))
    comp, acum = np.zeros(M, dtype=np.int32), np.zeros(M)
    rng = seeded(plan["seed"])
    updates = 0
    for s, (order, sigmaE, sigmaG, estPi, adaV) in enumerate(sweeps):
        cass, nnz = capi.ss_sweep_host(n_eff, W, ahead, band, c, beta, comp, acum, groups, cVa, cVaI, order, sigmaE, sigmaG, estPi, adaV, rng)
        g = got[s]
        assert np.array_equal(g["comp"], comp) and np.array_equal(g["cass"], cass) and g["nnz"] == nnz, s
        assert g["idx"] == int(rng.idx) and np.array_equal(g["x"], np.array(rng.x, dtype=np.uint32)), s
        assert sc.close(g["beta"], beta) and sc.close(g["acum"], acum) and sc.close(g["c"], c), s
        assert np.array_equal(g["beta"] == 0.0, beta == 0.0), s
        # hgibbs_ss_state's sums: marker order over the non-zero effects, on the device's own beta and c
        sb = sc_ = 0.0
        for j in np.flatnonzero(g["beta"]):
            sb += float(g["beta"][j]) * float(xty[j])
            sc_ += float(g["beta"][j]) * float(g["c"][j])
        assert g["sb"] == sb and g["sc"] == sc_, s
        updates += nnz
    if M > 2:
        assert updates > 0
    # the same bits from the same state
    again = run_device(dev, n_eff, W, ahead, xty, beta0, plan)
    for a, b in zip(got, again):
        for k in ("beta", "acum", "c", "comp", "cass", "x"):
            assert np.array_equal(a[k], b[k]), k
        assert (a["nnz"], a["idx"], a["sb"], a["sc"]) == (b["nnz"], b["idx"], b["sb"], b["sc"])
    return got


def test_one_marker():
    check_case(1, 1, some_fixed=False)


def test_two_markers_window_one():
    check_case(2, 1, some_fixed=False, nonzero_start=True)


@pytest.mark.parametrize("W", [1, 5, 64, 256, 300])
def test_257_markers(W):
    check_case(257, W, nonzero_start=(W in (5, 256)), shuffle=(W != 64), seed=20 + W)


def test_mixed_windows_with_zeros_two_groups_one_switched_off():
    M, W = 257, 64
    rs = np.random.default_rng(5)
    ahead = np.minimum(rs.integers(0, W + 1, M), M - 1 - np.arange(M)).astype(np.uint32)
    ahead[rs.random(M) < 0.2] = 0
    ahead[100:110] = 0
    groups = (np.arange(M) % 3 == 0).astype(np.int32)
    check_case(M, W, mS=sc.MS2, ahead=ahead, groups=groups, zero_group=True, nonzero_start=True, seed=9)


def test_1500_markers_cross_a_generator_block():
    got = check_case(1500, 5, seed=3)
    assert got[0]["idx"] <= 624  # 1500 uniforms and the draws: at least two refills in the first sweep alone


@pytest.mark.parametrize("mS", [MS2K, MS8], ids=["K2", "K8"])
def test_fewest_and_most_components(mS):
    check_case(257, 16, mS=mS, nonzero_start=True, seed=int(mS.shape[1]))
