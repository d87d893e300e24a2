"""The device engine with one workgroup per interval of independent LD blocks (hgibbs_ss_sweep_streams) held to
the host engine (hgibbs_ss_sweep_streams_host) over three sweeps on the same band, fetched with hgibbs_ss_band_get, by
tests/test_gpu_ss_sweep.py's rule: components, cass, nnz and every stream's generator (its 624 words and its index) are equal; beta,
acum and c are within `close`; the zero patterns are equal; two device runs from the same state give the same bits.

Shapes: borders inside one 128-byte line of c (intervals of 1, 2 and 254 markers); windows wider than the workgroup on both sides of
a border; one workgroup that refills its generator block beside one that does not; more workgroups than compute units (300 intervals
of two markers); K = 2 and K = 8.  With S = 1 the kernel gives hgibbs_ss_sweep's bits: one body, -ffp-contract=off."""
import numpy as np
import pytest

import ss_common as sc
from hydra_amd import capi, synth
from test_gpu_ss_sweep import MS2K, MS4, MS8, N, copy_rng, seeded
from test_ss_streams_cpu import blocks_ahead, words

pytestmark = pytest.mark.gpu


def make_plan(M, W, sizes, mS, groups, zero_group, seed, idx0=None):
    G, K = mS.shape
    rs = np.random.default_rng(seed)
    n_eff = 4000.0
    xty = rs.normal(0.0, np.sqrt(n_eff), M)
    xty[rs.random(M) < 0.15] *= 8.0  # signals: effects that leave 0, and come back
    beta0 = np.where(rs.random(M) < 0.3, rs.normal(0.0, 0.05, M), 0.0)
    sweeps = []
    for s in range(3):
        sigmaG = rs.uniform(0.2, 0.6, G)
        if zero_group:
            sigmaG[G - 1] = 0.0
        sweeps.append((rs.permutation(M).astype(np.int32), 0.4 + 0.1 * s, sigmaG, rs.dirichlet(np.ones(K) * 2.0, G), (rs.random(M) < 0.85).astype(np.uint8)))
    rngs = [seeded(seed + 100 + s) for s in range(len(sizes))]
    for s, i in (idx0 or {}).items():
        rngs[s].idx = i
    return dict(n_eff=n_eff, xty=xty, beta0=beta0, sweeps=sweeps, rngs=rngs, ahead=blocks_ahead(sizes, W),
                bounds=np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32))


def run_device(dev, W, plan, single=False):
    dev.ss_begin(plan["n_eff"], W, plan["xty"], plan["ahead"])
    dev.set_beta(plan["beta0"])
    rngs = [copy_rng(r) for r in plan["rngs"]]
    out = []
    for order, sigmaE, sigmaG, estPi, adaV in plan["sweeps"]:
        if single:
            cass, nnz = dev.ss_sweep(order, sigmaE, sigmaG, estPi, adaV, rngs[0])
        else:
            cass, nnz = dev.ss_sweep_streams(order, sigmaE, sigmaG, estPi, adaV, plan["bounds"], rngs)
        beta, comp, acum = dev.get_beta()
        c, sb, sc_ = dev.ss_state()
        out.append(dict(cass=cass, nnz=nnz, beta=beta, comp=comp, acum=acum, c=c, sb=sb, sc=sc_, x=np.stack([words(r)[0] for r in rngs]),
                        idx=[int(r.idx) for r in rngs]))
    return out


def same_bits(a, b):
    for x, y in zip(a, b):
        for k in ("beta", "acum", "c", "comp", "cass", "x"):
            assert np.array_equal(x[k], y[k]), k
        assert (x["nnz"], x["idx"], x["sb"], x["sc"]) == (y["nnz"], y["idx"], y["sb"], y["sc"])


def check_case(M, W, sizes, mS=MS4, groups=None, zero_group=False, seed=11, idx0=None):
    assert sum(sizes) == M
    geno = synth.make_genotypes(M, N, seed=seed, missing_rate=0.02)
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    cVa = mS.copy()
    cVaI = np.zeros_like(mS)
    cVaI[:, 1:] = 1.0 / mS[:, 1:]
    dev.set_model(groups, cVa, cVaI)
    plan = make_plan(M, W, sizes, mS, groups, zero_group, seed, idx0)
    got = run_device(dev, W, plan)
    band = dev.ss_band()
    # the host engine on the device's band
    c, beta, comp, acum = plan["xty"].copy(), plan["beta0"].copy(), np.zeros(M, dtype=np.int32), np.zeros(M)
    rngs = [copy_rng(r) for r in plan["rngs"]]
    updates = 0
    for s, (order, sigmaE, sigmaG, estPi, adaV) in enumerate(plan["sweeps"]):
        cass, nnz = capi.ss_sweep_streams_host(plan["n_eff"], W, plan["ahead"], band, c, beta, comp, acum, groups, cVa, cVaI, order, sigmaE, sigmaG, estPi, adaV,
                                               plan["bounds"], rngs)
        g = got[s]
        assert np.array_equal(g["comp"], comp) and np.array_equal(g["cass"], cass) and g["nnz"] == nnz, s
        assert g["idx"] == [int(r.idx) for r in rngs] and np.array_equal(g["x"], np.stack([words(r)[0] for r in rngs])), s
        assert sc.close(g["beta"], beta) and sc.close(g["acum"], acum) and sc.close(g["c"], c), s
        assert np.array_equal(g["beta"] == 0.0, beta == 0.0), s
        updates += nnz
    assert updates > 0
    same_bits(got, run_device(dev, W, plan))
    return plan, got


def test_borders_inside_one_line_of_c():
    check_case(257, 5, [1, 2, 254], mS=sc.MS2, groups=(np.arange(257) % 3 == 0).astype(np.int32), zero_group=True, seed=21)


def test_windows_wider_than_the_workgroup_on_both_sides_of_a_border():
    check_case(700, 300, [350, 350], seed=22)


def test_one_workgroup_refills_its_block_and_the_other_does_not():
    # stream 1 starts at the head of a block it holds: 20 markers a sweep never reach its end
    plan, got = check_case(1520, 5, [1500, 20], seed=23, idx0={1: 0})
    assert np.array_equal(got[-1]["x"][1], words(plan["rngs"][1])[0]) and 0 < got[-1]["idx"][1] < 624
    assert not np.array_equal(got[0]["x"][0], words(plan["rngs"][0])[0])


def test_more_workgroups_than_compute_units():
    plan, _ = check_case(600, 1, [2] * 300, seed=24)
    assert np.array_equal(plan["ahead"], np.tile([1, 0], 300))


@pytest.mark.parametrize("mS", [MS2K, MS8], ids=["K2", "K8"])
def test_fewest_and_most_components(mS):
    check_case(257, 16, [100, 57, 100], mS=mS, seed=30 + int(mS.shape[1]))


def test_one_stream_gives_the_single_sweeps_bits():
    M, W = 257, 16
    geno = synth.make_genotypes(M, N, seed=5, missing_rate=0.02)
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    cVa = MS4.copy()
    cVaI = np.zeros_like(MS4)
    cVaI[:, 1:] = 1.0 / MS4[:, 1:]
    dev.set_model(None, cVa, cVaI)
    plan = make_plan(M, W, [M], MS4, None, False, 5)
    a, b = run_device(dev, W, plan), run_device(dev, W, plan, single=True)
    same_bits(a, b)
    assert sum(x["nnz"] for x in a) > 0


def test_device_refusals():
    M, W = 12, 3
    geno = synth.make_genotypes(M, N, seed=1)
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    cVa = MS4.copy()
    cVaI = np.zeros_like(MS4)
    cVaI[:, 1:] = 1.0 / MS4[:, 1:]
    dev.set_model(None, cVa, cVaI)
    plan = make_plan(M, W, [4, 8], MS4, None, False, 1)
    dev.ss_begin(plan["n_eff"], W, plan["xty"], plan["ahead"])
    order, sigmaE, sigmaG, estPi, adaV = plan["sweeps"][0]
    bad = seeded(2)
    bad.idx = 625
    twice = order.copy()
    twice[3] = twice[7]
    for kw, msg in ((dict(bounds=[0, 6, 12], rngs=[seeded(1), seeded(2)]), "bounds[1] = 6 is not a cut: the window of marker 4 reaches marker 7"),
                    (dict(bounds=[0, 4, 4, 12], rngs=[seeded(1)] * 3), "strictly ascending"),
                    (dict(bounds=[1, 4, 12], rngs=[seeded(1)] * 2), "bounds must run from 0 to M = 12"),
                    (dict(bounds=[0], rngs=[seeded(1)], S=0), "S = 0, must be in [1, 1024]"),
                    (dict(bounds=np.zeros(1026), rngs=[seeded(1)], S=1025), "S = 1025, must be in [1, 1024]"),
                    (dict(bounds=[0, 4, 12], rngs=[seeded(1), bad]), "stream 1: rng idx 625 > 624"),
                    (dict(bounds=[0, 4, 12], rngs=[seeded(1), seeded(2)], order=twice), "the order must be a permutation")):
        with pytest.raises(capi.HgError) as e:
            dev.ss_sweep_streams(kw.pop("order", order), sigmaE, sigmaG, estPi, adaV, **kw)
        assert msg in str(e.value) and "hgibbs_ss_sweep_streams:" in str(e.value), (msg, str(e.value))
    # nothing was swept by a refused call
    assert np.array_equal(dev.ss_state()[0], plan["xty"])
    cass, _ = dev.ss_sweep_streams(order, sigmaE, sigmaG, estPi, adaV, [0, 4, 12], [seeded(1), seeded(2)])
    assert 0 < cass.sum() <= int(adaV.sum())  # (a marker without a finite sd is never adaptive)
