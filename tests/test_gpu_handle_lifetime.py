"""The handle owns its memory: a refused call leaves the handle as it was, a setter that replaces owned buffers
leaves it as a fresh handle with the second settings, and a handle can be given up at any point.  Every comparison is np.array_equal
against a fresh handle that saw only the good calls; N = 200 rows (one 1024-row block with padding), M = 64 markers (one PRED_CHUNK),
1 % missing calls."""
import ctypes as C

import numpy as np
import pytest

import sparse_restate as sr
from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu

N, M = 200, 64
_cache = {}


def data():
    if "data" not in _cache:
        geno = synth.make_genotypes(M, N, seed=77, missing_rate=0.01)
        bed = synth.pack_bed_columns(geno)
        y, _ = synth.make_phenotype(geno, seed=78, causal_frac=0.1)
        yw, fail, _ = synth.make_survival(geno, seed=79, causal_frac=0.1)
        eps = (y - y.mean()) * np.sqrt((N - 1) / np.sum((y - y.mean()) ** 2))
        X = np.random.default_rng(80).normal(size=(N, 3))
        for a in (bed, eps, yw, fail, X):
            a.setflags(write=False)
        _cache["data"] = (bed, eps, yw, fail, X)
    return _cache["data"]


def mixture(G, K):
    mS = np.tile(np.array([0.0, 1e-4, 1e-3, 1e-2])[:K], (G, 1))
    return mS, np.where(mS > 0.0, 1.0 / np.maximum(mS, 1e-300), 0.0)


def groups_of(G):
    return (np.arange(M) % G).astype(np.int32)


def set_models(dev, ops, G, K, quad):
    mS, inv = mixture(G, K)
    dev.set_model(groups_of(G), mS, inv)
    ops.set_model(mS, groups_of(G), quad=quad)


def mt_state(seed):
    rng = capi.RngState()
    for i, w in enumerate(np.random.default_rng(seed).integers(0, 1 << 32, size=624, dtype=np.uint64)):
        rng.x[i] = int(w)
    rng.idx = 624
    return rng


def results(dev, ops):
    """What the tests compare, array for array: marker_stats; BayesW's marker stats, vi after refresh_vi, the covariates' dots and one
    hgibbs_w_sweep as the BayesW chain starts it; three hgibbs_sweeps from a fixed generator state."""
    _, eps, yw, _, _ = data()
    G, K, L = dev.G, dev.K, dev.L
    out = list(dev.marker_stats())
    # BayesW: mu, alpha and sigmaG as the chain initialises them
    mu = yw.mean()
    alpha = np.pi / np.sqrt(6.0 * np.sum((yw - mu) ** 2) / (N - 1))
    dev.set_residual(yw - mu)
    out += list(ops.marker_stats())
    ops.refresh_vi(alpha)
    vi, vi_sum = ops.get_vi()
    out += [vi, np.array(vi_sum)]
    out += [np.array(dev.cov_dot(c, 0.25)) for c in range(dev_C(dev))]
    sigmaG = np.full(G, np.pi ** 2 / (6.0 * alpha ** 2) / G)
    pi = np.full((G, K), 1.0 / M)
    pi[:, 0], pi[:, 1] = 0.99, 0.01
    rng, grand = mt_state(5), capi.GrandState()
    L.hgibbs_grand_seed(C.byref(grand), 1222)
    cass, bsq, nnz = np.zeros((G, K), dtype=np.int32), np.zeros(G), C.c_uint64()
    capi.check(L.hgibbs_w_sweep(dev.h, capi._ip(np.arange(M, dtype=np.int32)), alpha, capi._dp(sigmaG), capi._dp(pi), float(sigmaG.sum()),
                                C.byref(rng), C.byref(grand), capi._ip(cass), capi._dp(bsq), C.byref(nnz)))
    out += [cass, bsq, np.array(nnz.value), *ops.get_beta(), dev.get_residual()]
    # BayesR
    dev.set_residual(eps)
    rng = mt_state(3)
    est = np.tile(np.array([0.5, 0.3, 0.15, 0.05])[:K] / np.sum(np.array([0.5, 0.3, 0.15, 0.05])[:K]), (G, 1))
    for it in range(3):
        cass, nnz = dev.sweep(np.random.default_rng(10 + it).permutation(M).astype(np.int32), 0.5, np.full(G, 0.1), est, np.ones(M, dtype=np.uint8), rng)
        out += [cass, np.array(nnz)]
    out += [*dev.get_beta(), dev.get_residual(), np.array(list(rng.x))]
    return out


def dev_C(dev):
    return getattr(dev, "_C", 0)


def set_cov(dev, X):
    dev.set_covariates(X)
    dev._C = 0 if X is None else X.shape[1]


def fresh(G, K, quad, ncov):
    """the results of a fresh handle given only the good calls with these settings, computed once"""
    key = (G, K, quad, ncov)
    if key not in _cache:
        bed, _, _, fail, X = data()
        dev = capi.Device(0)
        dev.load_bed(bed, N)
        ops = capi.BwOps(dev, fail)
        set_models(dev, ops, G, K, quad)
        if ncov:
            set_cov(dev, X[:, :ncov])
        _cache[key] = results(dev, ops)
        dev.close()
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


def same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "array %d differs" % i


def refused(pattern, fn, *a, **kw):
    with pytest.raises(capi.HgError, match=pattern):
        fn(*a, **kw)


def test_reuse_after_a_refusal(gpu_lib):
    bed, _, _, fail, _ = data()
    dev = capi.Device(0)
    refused(r"row_begin 2 must be a multiple of 4", dev.load_bed, bed, N, row_begin=2)
    refused(r"n_global must be at least 2", dev.load_bed, bed, N, n_global=1)
    refused(r"hgibbs_synth_bed: bad row range", dev.synth_bed, N, M, row_begin=5, row_end=5)
    dev.load_bed(bed, N)
    bad = np.array(fail)
    bad[N // 2] = 2
    refused(r"failure indicator of individual %d is 2" % (N // 2), capi.BwOps, dev, bad)
    ops = capi.BwOps(dev, fail)
    mS, inv = mixture(1, 4)
    outside = np.zeros(M, dtype=np.int32)
    outside[M - 1] = 1
    refused(r"hgibbs_set_model: groups\[%d\]=1 outside \[0,1\)" % (M - 1), dev.set_model, outside, mS, inv)
    refused(r"hgibbs_w_set_model: marker %d in group 1 outside \[0,1\)" % (M - 1), ops.set_model, mS, outside, 9)
    set_models(dev, ops, 1, 4, 9)
    # and once more with the good model in place: other G and K, a group outside them at the last marker
    mS3, inv3 = mixture(2, 3)
    outside = groups_of(2)
    outside[M - 1] = 2
    refused(r"hgibbs_set_model: groups\[%d\]=2 outside \[0,2\)" % (M - 1), dev.set_model, outside, mS3, inv3)
    refused(r"hgibbs_w_set_model: marker %d in group 2 outside \[0,2\)" % (M - 1), ops.set_model, mS3, outside, 25)
    same(results(dev, ops), fresh(1, 4, 9, 0))
    dev.close()


def test_replacement_of_owned_buffers(gpu_lib):
    bed, _, _, fail, X = data()
    dev = capi.Device(0)
    dev.load_bed(bed, N)
    ops = capi.BwOps(dev, fail)
    set_models(dev, ops, 1, 4, 9)
    set_cov(dev, X)
    dev.cov_dot(2, 0.0)  # the first settings' columns are in use before they are replaced
    set_models(dev, ops, 3, 3, 25)
    set_cov(dev, X[:, :1])
    same(results(dev, ops), fresh(3, 3, 25, 1))
    dev.close()


def test_abandon_and_destroy(gpu_lib):
    bed, _, _, fail, X = data()
    lists = sr.bed_to_lists(bed, N)
    dev = capi.Device(0)
    dev.sparse_begin(N, M)
    dev.close()  # a load in the making goes with its handle
    dev = capi.Device(0)
    dev.sparse_begin(N, M)
    dev.sparse_put(0, [(lists["ss" + c], lists["sl" + c], lists["si" + c], 0) for c in sr.CLASSES])
    dev.sparse_end()
    ref = capi.Device(0)
    ref.load_bed(bed, N)
    assert np.array_equal(dev.get_bed(), ref.get_bed())
    dev.close()
    ref.close()
    want = fresh(1, 4, 9, 3)
    for _ in range(5):
        dev = capi.Device(0)
        dev.load_bed(bed, N)
        ops = capi.BwOps(dev, fail)
        set_cov(dev, X)
        set_models(dev, ops, 1, 4, 9)
        same(results(dev, ops), want)
        dev.close()
