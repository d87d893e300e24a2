"""R chains on one band in one launch (hgibbs_ss_sweep_replicas) held to the single-chain kernels bit for bit:
every replica has its own orders, sigmaE, sigmaG, pi, mask, non-zero start and generator(s), and is compared over three sweeps with
hgibbs_ss_sweep (S = 1) or hgibbs_ss_sweep_streams run from the same inputs on the handle's own chain: beta, acum, c, components, cass,
nnz and every generator's words and index are equal, and so are hgibbs_ss_replica_sums' sums with hgibbs_ss_state's and
hgibbs_beta_sqnorm's.  The shapes are tests/test_gpu_ss_streams.py's, with the replicas' c arrays abutting.  One case is also held to
the host engine on the fetched band at `close`; the replicas and the handle's chain do not touch one another; the refusals."""
import numpy as np
import pytest

import ss_common as sc
from hydra_amd import capi, synth
from test_gpu_ss_streams import make_plan
from test_gpu_ss_sweep import MS2K, MS4, MS8, N, copy_rng, seeded
from test_ss_streams_cpu import words

pytestmark = pytest.mark.gpu

KEYS = ("beta", "acum", "c", "comp", "cass", "x", "bsq")


def open_device(M, mS, groups, seed):
    geno = synth.make_genotypes(M, N, seed=seed, missing_rate=0.02)
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    cVa = mS.copy()
    cVaI = np.zeros_like(mS)
    cVaI[:, 1:] = 1.0 / mS[:, 1:]
    dev.set_model(groups, cVa, cVaI)
    return dev, cVa, cVaI


def make_plans(R, M, W, sizes, mS, groups, zero_in, seed):
    """One plan of tests/test_gpu_ss_streams.py per replica (its own orders, sigmaE, sigmaG, pi, mask, start and generators) on the
    one xty, window and bounds; zero_in: the replica whose last group has sigmaG = 0, or None."""
    plans = [make_plan(M, W, sizes, mS, groups, zero_in == r, seed + 1000 * r) for r in range(R)]
    for p in plans[1:]:
        p["xty"] = plans[0]["xty"]
    return plans


def snapshot(cass, nnz, beta, comp, acum, c, sb, sc_, bsq, rngs):
    return dict(cass=cass, nnz=int(nnz), beta=beta, comp=comp, acum=acum, c=c, sb=sb, sc=sc_, bsq=bsq, x=np.stack([words(r)[0] for r in rngs]),
                idx=[int(r.idx) for r in rngs])


def run_single(dev, W, plan, single):
    """The handle's own chain: hgibbs_ss_sweep (single) or hgibbs_ss_sweep_streams over the plan's three sweeps"""
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
        out.append(snapshot(cass, nnz, beta, comp, acum, c, sb, sc_, dev.beta_sqnorm(), rngs))
    return out


def run_replicas(dev, W, plans, begin=True, shared_mask=False):
    """out[r][sweep]; bounds None (the single stream) when the plans hold one interval"""
    R, p0 = len(plans), plans[0]
    if begin:
        dev.ss_begin(p0["n_eff"], W, p0["xty"], p0["ahead"])
    dev.ss_replicas(R)
    for r, p in enumerate(plans):
        dev.ss_replica_set_beta(r, p["beta0"])
    rngs = [[copy_rng(g) for g in p["rngs"]] for p in plans]
    bounds = p0["bounds"] if len(p0["bounds"]) > 2 else None
    out = [[] for _ in plans]
    for s in range(3):
        sw = [p["sweeps"][s] for p in plans]
        mask = sw[0][4] if shared_mask else np.stack([x[4] for x in sw])
        cass, nnz = dev.ss_sweep_replicas(np.stack([x[0] for x in sw]), [x[1] for x in sw], np.stack([x[2] for x in sw]), np.stack([x[3] for x in sw]), mask,
                                          rngs, bounds=bounds)
        sb, sc_, bsq = dev.ss_replica_sums(R)
        for r in range(R):
            beta, comp, acum, c = dev.ss_replica_get(r)
            out[r].append(snapshot(cass[r], nnz[r], beta, comp, acum, c, sb[r], sc_[r], bsq[r], rngs[r]))
    return out


def same_bits(a, b):
    for x, y in zip(a, b):
        for k in KEYS:
            assert np.array_equal(x[k], y[k]), k
        assert (x["nnz"], x["idx"], x["sb"], x["sc"]) == (y["nnz"], y["idx"], y["sb"], y["sc"])


def check_case(R, M, W, sizes, mS=MS4, groups=None, zero_in=None, seed=41, single=False, shared_mask=False):
    assert sum(sizes) == M
    dev, cVa, cVaI = open_device(M, mS, groups, seed)
    plans = make_plans(R, M, W, sizes, mS, groups, zero_in, seed)
    if shared_mask:
        for p in plans[1:]:
            p["sweeps"] = [s[:4] + (q[4],) for s, q in zip(p["sweeps"], plans[0]["sweeps"])]
    want = [run_single(dev, W, p, single) for p in plans]
    got = run_replicas(dev, W, plans, shared_mask=shared_mask)
    for r in range(R):
        same_bits(got[r], want[r])
    assert sum(s["nnz"] for w in want for s in w) > 0
    return dev, plans, got, (cVa, cVaI)


def test_single_stream_against_the_single_sweep():
    check_case(3, 257, 16, [257], single=True, seed=41)


def test_borders_inside_one_line_of_c_two_groups_one_replica_switched_off():
    # the replicas' c arrays abut: 257 doubles each, so a replica's border and an interval's border fall inside one 128-byte line
    check_case(3, 257, 5, [1, 2, 254], mS=sc.MS2, groups=(np.arange(257) % 3 == 0).astype(np.int32), zero_in=1, seed=42)


def test_windows_wider_than_the_workgroup():
    check_case(2, 700, 300, [350, 350], seed=43)


def test_refilling_and_non_refilling_workgroups_in_both_replicas():
    _, plans, got, _ = check_case(2, 1520, 5, [1500, 20], seed=44)
    for r in range(2):
        assert not np.array_equal(got[r][0]["x"][0], words(plans[r]["rngs"][0])[0])


def test_more_workgroups_than_compute_units():
    check_case(5, 120, 1, [2] * 60, seed=45)


@pytest.mark.parametrize("mS", [MS2K, MS8], ids=["K2", "K8"])
def test_fewest_and_most_components(mS):
    check_case(2, 257, 16, [100, 57, 100], mS=mS, seed=50 + int(mS.shape[1]))


def test_the_most_replicas_with_one_mask_for_all():
    check_case(64, 12, 3, [4, 8], seed=46, shared_mask=True)


def test_replicas_and_the_handles_chain_do_not_touch_one_another():
    M, W, sizes = 257, 16, [100, 57, 100]
    dev, _, _ = open_device(M, MS4, None, 47)
    plans = make_plans(3, M, W, sizes, MS4, None, None, 47)
    own = np.where(np.arange(M) % 7 == 0, 0.01, 0.0)
    dev.ss_begin(plans[0]["n_eff"], W, plans[0]["xty"], plans[0]["ahead"])
    dev.set_beta(own)
    before = (dev.get_beta(), dev.ss_state(), dev.beta_sqnorm())
    got = run_replicas(dev, W, plans, begin=False)
    after = (dev.get_beta(), dev.ss_state(), dev.beta_sqnorm())
    for a, b in zip(before[0] + before[1] + (before[2],), after[0] + after[1] + (after[2],)):
        assert np.array_equal(a, b)
    assert np.array_equal(after[0][0], own) and np.array_equal(after[1][0], plans[0]["xty"])
    # a sweep of the handle's own chain leaves every replica as it was
    order, sigmaE, sigmaG, estPi, adaV = plans[0]["sweeps"][0]
    _, nnz = dev.ss_sweep_streams(order, sigmaE, sigmaG, estPi, adaV, plans[0]["bounds"], [copy_rng(g) for g in plans[0]["rngs"]])
    assert nnz > 0
    sb, sc_, bsq = dev.ss_replica_sums(3)
    for r in range(3):
        last = got[r][-1]
        for a, b in zip(dev.ss_replica_get(r), (last["beta"], last["comp"], last["acum"], last["c"])):
            assert np.array_equal(a, b)
        assert (sb[r], sc_[r]) == (last["sb"], last["sc"]) and np.array_equal(bsq[r], last["bsq"])
    # replica 1 swept alone is replica 1 swept among three; two runs from the same state give the same bits
    same_bits(run_replicas(dev, W, plans[1:2])[0], got[1])
    again = run_replicas(dev, W, plans)
    for r in range(3):
        same_bits(again[r], got[r])


def test_held_to_the_host_engine_on_the_fetched_band():
    M, W, sizes = 257, 16, [100, 57, 100]
    dev, plans, got, (cVa, cVaI) = check_case(2, M, W, sizes, seed=48)
    band = dev.ss_band()
    for r, plan in enumerate(plans):
        c, beta, comp, acum = plan["xty"].copy(), plan["beta0"].copy(), np.zeros(M, dtype=np.int32), np.zeros(M)
        rngs = [copy_rng(g) for g in plan["rngs"]]
        for s, (order, sigmaE, sigmaG, estPi, adaV) in enumerate(plan["sweeps"]):
            cass, nnz = capi.ss_sweep_streams_host(plan["n_eff"], W, plan["ahead"], band, c, beta, comp, acum, None, cVa, cVaI, order, sigmaE, sigmaG, estPi, adaV,
                                                   plan["bounds"], rngs)
            g = got[r][s]
            assert np.array_equal(g["comp"], comp) and np.array_equal(g["cass"], cass) and g["nnz"] == nnz, (r, s)
            assert g["idx"] == [int(x.idx) for x in rngs] and np.array_equal(g["x"], np.stack([words(x)[0] for x in rngs])), (r, s)
            assert sc.close(g["beta"], beta) and sc.close(g["acum"], acum) and sc.close(g["c"], c), (r, s)
            assert np.array_equal(g["beta"] == 0.0, beta == 0.0), (r, s)


def test_refusals():
    M, W = 12, 3
    dev, _, _ = open_device(M, MS4, None, 1)
    plans = make_plans(3, M, W, [4, 8], MS4, None, None, 1)
    p0 = plans[0]
    sw = [p["sweeps"][0] for p in plans]
    orders, sigmaE, sigmaG, estPi = np.stack([x[0] for x in sw]), [x[1] for x in sw], np.stack([x[2] for x in sw]), np.stack([x[3] for x in sw])
    adaV = sw[0][4]

    def fresh():
        return [[seeded(10 * r + s) for s in range(2)] for r in range(3)]

    def sweep(msg, orders=orders, rngs=None, **kw):
        with pytest.raises(capi.HgError) as e:
            dev.ss_sweep_replicas(orders, sigmaE, sigmaG, estPi, adaV, fresh() if rngs is None else rngs, bounds=kw.pop("bounds", p0["bounds"]), **kw)
        assert msg in str(e.value) and "hgibbs_ss_sweep_replicas:" in str(e.value), (msg, str(e.value))

    with pytest.raises(capi.HgError) as e:
        dev.ss_replicas(2)
    assert "hgibbs_ss_replicas: no summary-statistics state on this handle" in str(e.value)
    dev.ss_begin(p0["n_eff"], W, p0["xty"], p0["ahead"])
    sweep("no replicas on this handle (hgibbs_ss_replicas first)")
    for R in (0, 65):
        with pytest.raises(capi.HgError) as e:
            dev.ss_replicas(R)
        assert "hgibbs_ss_replicas: R = %d, must be in [1, 64]" % R in str(e.value)
    dev.ss_replicas(3)
    sweep("R = 2, but hgibbs_ss_replicas allocated 3 replicas", R=2)
    sweep("R = 0, must be in [1, 64]", R=0)
    sweep("R = 65, must be in [1, 64]", R=65)
    for call in (lambda: dev.ss_replica_get(3), lambda: dev.ss_replica_set_beta(3, np.zeros(M))):
        with pytest.raises(capi.HgError) as e:
            call()
        assert "replica 3 outside [0, 3)" in str(e.value)
    bad = fresh()
    bad[2][1].idx = 625
    sweep("replica 2: stream 1: rng idx 625 > 624", rngs=bad)
    twice = orders.copy()
    twice[1, np.flatnonzero(twice[1] < 4)[0]] = twice[1, np.flatnonzero(twice[1] >= 4)[0]]  # a marker of the second interval in place of one of the first
    sweep("replica 1: order[", orders=twice)
    sweep("the order must be a permutation", orders=twice)
    sweep("replica 0: bounds[1] = 6 is not a cut: the window of marker 4 reaches marker 7", bounds=[0, 6, 12])
    # nothing was swept by a refused call
    for r in range(3):
        beta, comp, acum, c = dev.ss_replica_get(r)
        assert np.array_equal(c, p0["xty"]) and not beta.any() and not comp.any() and not acum.any()
    cass, nnz = dev.ss_sweep_replicas(orders, sigmaE, sigmaG, estPi, adaV, fresh(), bounds=p0["bounds"])
    assert all(0 < cass[r].sum() <= int(adaV.sum()) for r in range(3))
