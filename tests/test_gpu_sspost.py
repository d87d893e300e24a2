"""The per-marker posterior accumulators on the device (hgibbs_ss_post_*) held to tests/sspost_restate.py on
real sweeps: after every hgibbs_ss_sweep_replicas (R >= 1) or hgibbs_ss_sweep (R = 0, the handle's own chain) the state is fetched,
fed to the restatement, and folded on the device by hgibbs_ss_post_add.

  cnt                               equal
  every half-chain's (mean, m2)     bit for bit (hgibbs_ss_post_raw), and the pooled pair: correctly rounded f64 + - x / in one order
  mean, sd, pip, rhat               ss_common.close, NaN in the same places
  two runs                          the same bits
  the chains' state                 the same bits before and after an add

Shapes, the edges of the kernel's indexing: one marker; 255, 256 and 257 markers (a workgroup is 256 threads) with R = 3 and the odd
T = 5, whose middle record is in no half; R = 1 with T = 4; R = 0 at 257 markers; R = 64 at 12 markers; K = 2 and K = 8; two groups.
Every case must hold a marker with 0 < PIP < 1 and one with a finite R^ (checked on the host's data), so no table is all zeros."""
import numpy as np
import pytest

import ss_common as sc
import sspost_restate as pr
from hydra_amd import capi, synth
from test_gpu_ss_sweep import MS2K, MS4, MS8, N, copy_rng, seeded

pytestmark = pytest.mark.gpu


def open_device(M, mS, groups, seed, model=True):
    geno = synth.make_genotypes(M, N, seed=seed, missing_rate=0.02)
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    if model:
        cVaI = np.zeros_like(mS)
        cVaI[:, 1:] = 1.0 / mS[:, 1:]
        dev.set_model(groups, mS.copy(), cVaI)
    return dev


def make_plan(C, M, mS, T, seed):
    """What C chains sweep T times: tests/test_gpu_ss_sweep.py's inputs (signals in xty, a start from non-zero effects, sigmaG and pi that
    keep a fair share of the markers in the model), each chain with its own."""
    G, K = mS.shape
    rs = np.random.default_rng(seed)
    n_eff = 4000.0
    xty = rs.normal(0.0, np.sqrt(n_eff), M)
    xty[rs.random(M) < 0.15] *= 8.0
    beta0 = np.where(rs.random((C, M)) < 0.3, rs.normal(0.0, 0.05, (C, M)), 0.0)
    records = []
    for t in range(T):
        records.append(dict(orders=np.stack([rs.permutation(M) for _ in range(C)]).astype(np.int32), sigmaE=0.4 + 0.05 * t + 0.01 * np.arange(C),
                            sigmaG=rs.uniform(0.2, 0.6, (C, G)), estPi=rs.dirichlet(np.ones(K) * 2.0, (C, G)),
                            adaV=(rs.random((C, M)) < 0.85).astype(np.uint8)))
    return dict(n_eff=n_eff, xty=xty, beta0=beta0, records=records, rngs=[seeded(seed + 100 + r) for r in range(C)])


def fetch(dev, R):
    """every chain's (beta, comp, acum, c), and the handle's own beside the replicas"""
    own = dev.get_beta() + (dev.ss_state()[0],)
    return [own] + [dev.ss_replica_get(r) for r in range(R)]


def run_case(dev, R, M, W, mS, T, seed):
    C, K = max(R, 1), mS.shape[1]
    plan = make_plan(C, M, mS, T, seed)
    dev.ss_begin(plan["n_eff"], W, plan["xty"])
    if R:
        dev.ss_replicas(R)
        for r in range(R):
            dev.ss_replica_set_beta(r, plan["beta0"][r])
    else:
        dev.set_beta(plan["beta0"][0])
    dev.ss_post_begin(R, T)
    rngs = [copy_rng(g) for g in plan["rngs"]]
    want = pr.Post(C, M, K, T)
    moved = 0
    for rec in plan["records"]:
        if R:
            _, nnz = dev.ss_sweep_replicas(rec["orders"], rec["sigmaE"], rec["sigmaG"], rec["estPi"], rec["adaV"], rngs)
            moved += int(nnz.sum())
        else:
            _, nnz = dev.ss_sweep(rec["orders"][0], rec["sigmaE"][0], rec["sigmaG"][0], rec["estPi"][0], rec["adaV"][0], rngs[0])
            moved += int(nnz)
        before = fetch(dev, R)
        dev.ss_post_add()
        after = fetch(dev, R)
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
        chains = before[1:] if R else before[:1]
        want.add(np.stack([c[0] for c in chains]), np.stack([c[1] for c in chains]))
    assert moved > 0
    raw = {(r, half): dev.ss_post_raw(r, half) for r in range(C) for half in range(2)}
    raw[(C, 0)] = dev.ss_post_raw(C, 0)
    got = dev.ss_post_get()
    add_ms, final_ms = dev.last_ss_post_ms()
    assert add_ms > 0.0 and final_ms > 0.0
    return want, raw, got


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_case(R, M, W, T, mS=MS4, groups=None, seed=61, twice=False):
    dev = open_device(M, mS, groups, seed)
    want, raw, got = run_case(dev, R, M, W, mS, T, seed)
    wmean, wsd, wpip, wrhat = want.final()
    # the condition on the host's data: the accumulators are not all zeros
    assert np.any((wpip > 0.0) & (wpip < 1.0)) and np.any(np.isfinite(wrhat)), (wpip, wrhat)
    mean, sd, pip, cnt, rhat = got
    assert np.array_equal(cnt, want.cnt)
    for key, (hm, h2) in raw.items():
        wm, w2 = want.raw(*key)
        assert np.array_equal(bits(hm), bits(wm)), key
        assert np.array_equal(bits(h2), bits(w2)), key
    assert np.array_equal(bits(mean), bits(wmean))  # (the pooled mean as it stands)
    assert sc.close(sd, wsd) and sc.close(pip, wpip)
    assert np.array_equal(np.isnan(rhat), np.isnan(wrhat))
    ok = ~np.isnan(wrhat)
    assert sc.close(rhat[ok], wrhat[ok])
    if twice:
        _, raw2, got2 = run_case(dev, R, M, W, mS, T, seed)
        for key in raw:
            for a, b in zip(raw[key], raw2[key]):
                assert np.array_equal(bits(a), bits(b)), key
        for a, b in zip(got, got2):
            assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)
    return dev


def test_one_marker():
    check_case(3, 1, 1, 5, seed=3)


@pytest.mark.parametrize("M", [255, 256, 257])
def test_around_one_workgroup_odd_T(M):
    check_case(3, M, 16, 5, seed=60 + M, twice=(M == 257))


def test_one_replica_four_records():
    check_case(1, 70, 5, 4, seed=62)


def test_the_handles_own_chain():
    check_case(0, 257, 16, 6, seed=63, twice=True)


def test_the_most_replicas():
    check_case(64, 12, 3, 4, seed=64)


@pytest.mark.parametrize("mS", [MS2K, MS8], ids=["K2", "K8"])
def test_fewest_and_most_components(mS):
    check_case(2, 130, 8, 4, mS=mS, seed=65 + int(mS.shape[1]))


def test_two_groups():
    check_case(2, 100, 8, 7, mS=sc.MS2, groups=(np.arange(100) % 2).astype(np.int32), seed=66)


def test_refusals():
    M, W = 12, 3
    xty = np.random.default_rng(1).normal(0.0, 60.0, M)

    def refused(call, msg):
        with pytest.raises(capi.HgError) as e:
            call()
        assert msg in str(e.value), (msg, str(e.value))

    bare = open_device(M, MS4, None, 2, model=False)
    bare.ss_begin(4000.0, W, xty)
    refused(lambda: bare.ss_post_begin(0, 4), "hgibbs_ss_post_begin: model not set")

    dev = open_device(M, MS4, None, 2)
    refused(lambda: dev.ss_post_begin(0, 4), "hgibbs_ss_post_begin: no summary-statistics state on this handle")
    dev.ss_begin(4000.0, W, xty)
    refused(dev.ss_post_add, "hgibbs_ss_post_add: no posterior accumulators on this handle (hgibbs_ss_post_begin first)")
    refused(dev.ss_post_get, "hgibbs_ss_post_get: no posterior accumulators on this handle (hgibbs_ss_post_begin first)")
    refused(lambda: dev.ss_post_begin(2, 4), "hgibbs_ss_post_begin: no replicas on this handle (hgibbs_ss_replicas first)")
    dev.ss_replicas(3)
    refused(lambda: dev.ss_post_begin(2, 4), "hgibbs_ss_post_begin: R = 2, but hgibbs_ss_replicas allocated 3 replicas")
    refused(lambda: dev.ss_post_begin(3, 3), "hgibbs_ss_post_begin: T = 3 records per chain, split-R^ needs at least 4")
    refused(lambda: dev.ss_post_begin(0, 0), "hgibbs_ss_post_begin: T = 0 records per chain, split-R^ needs at least 4")
    refused(lambda: dev.ss_post_begin(3, 2 ** 31), "hgibbs_ss_post_begin: R = 3 chains of T = 2147483648 records: the pooled count R T must stay below 2^32")

    dev.ss_post_begin(3, 4)
    refused(lambda: dev.ss_replicas(3), "hgibbs_ss_replicas: posterior accumulators are open on this handle (hgibbs_ss_post_end first)")
    cVaI = np.zeros_like(MS4)
    cVaI[:, 1:] = 1.0 / MS4[:, 1:]
    refused(lambda: dev.set_model(None, MS4.copy(), cVaI), "hgibbs_set_model: posterior accumulators are open on this handle (hgibbs_ss_post_end first)")
    dev.ss_post_add()
    dev.ss_post_add()
    refused(dev.ss_post_get, "hgibbs_ss_post_get: 2 of the 4 planned records were added")
    refused(lambda: dev.ss_post_raw(0, 0), "hgibbs_ss_post_raw: 2 of the 4 planned records were added")
    dev.ss_post_add()
    dev.ss_post_add()
    refused(dev.ss_post_add, "hgibbs_ss_post_add: the 4 planned records are all added")
    for r, half in ((4, 0), (0, 2), (3, 1)):
        refused(lambda: dev.ss_post_raw(r, half), "hgibbs_ss_post_raw: r = %d, half = %d: a half-chain is r in [0, 3) with half 0 or 1, the pooled pair r = 3 with half 0" % (r, half))
    mean, sd, pip, cnt, rhat = dev.ss_post_get()  # four records of all-zero effects
    assert not mean.any() and not sd.any() and not pip.any() and np.isnan(rhat).all() and np.array_equal(cnt[0], np.full(M, 12)) and not cnt[1:].any()

    # a second begin replaces the first; after the end both calls are taken again, and a begin after them
    dev.ss_post_begin(0, 5)
    refused(dev.ss_post_get, "hgibbs_ss_post_get: 0 of the 5 planned records were added")
    dev.ss_post_end()
    dev.ss_post_end()
    assert dev.last_ss_post_ms() == (0.0, 0.0)
    dev.ss_replicas(2)
    dev.set_model(None, MS4.copy(), cVaI)
    dev.ss_post_begin(2, 4)

    # a component outside [0, K): refused with the chain and the marker, and the accumulators are dropped
    dev.ss_post_begin(0, 4)
    comp = np.zeros(M, dtype=np.int32)
    comp[7], comp[9] = 4, -1
    capi.check(dev.L.hgibbs_set_components(dev.h, capi._ip(comp)))
    refused(dev.ss_post_add, "hgibbs_ss_post_add: record 0: chain 0, marker 7: its component is outside [0, 4)")
    refused(dev.ss_post_add, "hgibbs_ss_post_add: no posterior accumulators on this handle")
    dev.ss_end()
    refused(lambda: dev.ss_post_begin(0, 4), "hgibbs_ss_post_begin: no summary-statistics state on this handle")
