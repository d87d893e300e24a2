"""The inclusion history on the device and the candidate credible sets from it (hgibbs_cs_*) against
tests/cs_restate.py, everything compared for equality.

  history   cs_add_flags with random flags: the words and the counts after every add, at M = 1, 255, 256, 257 (a workgroup is 256
            threads) x (C, T) = (1, 4), (1, 65), (3, 22) (a record's bits across the word boundary: q = 63, 64, 65), (64, 2), (70, 2)
            (more than two words per add); no bit at or above NREC; two runs give the same bits
  ss        ss_cs_add after real sweeps of three replicas and of the handle's own chain at M = 257: the history of the fetched
            components, the chains' state untouched, cnt = NREC - the posterior table's cnt[0]
  sets      masks from Device.ld_mask on genotypes with LD of their own, M = 300 x W = 1, 63, 64, 65, 130 x max_size = 1, 3, 64 x
            NREC = 4, 64, 65, 130: status, size, sum, pep and members; the same for the leads in another order and split over two
            calls; the conditions of tests/test_cs_restatement_cpu.py again, from the device's own output
  refusals  of every entry point, and last_cs_ms"""
import numpy as np
import pytest

import cs_cases as cc
import cs_restate as cr
from hydra_amd import capi, synth
from test_gpu_ss_sweep import MS4, copy_rng
from test_gpu_sspost import fetch, make_plan, open_device

pytestmark = pytest.mark.gpu

HIST_M = [1, 255, 256, 257]
HIST_CT = [(1, 4), (1, 65), (3, 22), (64, 2), (70, 2)]


def plain_device(M, N=40, seed=5):
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(synth.make_genotypes(M, N, seed=seed)), N)
    return dev


@pytest.fixture(scope="module")
def hist_devices():
    return {M: plain_device(M) for M in HIST_M}


def run_history(dev, M, C, T, seed, want=None):
    """T adds of random flags; with `want`, the words and counts are held to the restatement after every add.  Returns the last words."""
    rng = np.random.default_rng(seed)
    dev.cs_begin(C, T)
    assert not dev.cs_history().any() and not dev.cs_counts().any()
    words = None
    for t in range(T):
        flags = (rng.random((C, M)) < rng.choice([0.1, 0.5, 0.9])).astype(np.uint8) * rng.integers(1, 256, (C, M)).astype(np.uint8)
        dev.cs_add_flags(flags)
        words = dev.cs_history()
        if want is not None:
            want.add(flags)
            assert np.array_equal(words, want.words), (t, C, M)
            assert np.array_equal(dev.cs_counts(), want.counts()), (t, C, M)
    return words


@pytest.mark.parametrize("C,T", HIST_CT)
@pytest.mark.parametrize("M", HIST_M)
def test_history_of_flags(hist_devices, M, C, T):
    dev = hist_devices[M]
    want = cr.History(C, T, M)
    words = run_history(dev, M, C, T, 31 * M + 7 * C + T, want)
    nrec = C * T
    assert words.shape == ((nrec + 63) // 64, M) and want.counts().any()
    if nrec % 64:
        assert not (words[-1] >> np.uint64(nrec % 64)).any()  # no bit at or above NREC
    assert int(cr.popcount(words).sum()) == int(dev.cs_counts().sum())
    again = run_history(dev, M, C, T, 31 * M + 7 * C + T)
    assert np.array_equal(again, words)
    add_ms, counts_ms, sets_ms = dev.last_cs_ms()
    assert add_ms > 0.0 and counts_ms > 0.0 and sets_ms == 0.0


@pytest.mark.parametrize("R", [3, 0])
def test_ss_cs_add_after_real_sweeps(R):
    M, W, T, seed = 257, 16, 6, 63 + R
    C = max(R, 1)
    dev = open_device(M, MS4, None, seed)
    plan = make_plan(C, M, MS4, T, seed)
    dev.ss_begin(plan["n_eff"], W, plan["xty"])
    if R:
        dev.ss_replicas(R)
        for r in range(R):
            dev.ss_replica_set_beta(r, plan["beta0"][r])
    else:
        dev.set_beta(plan["beta0"][0])
    dev.ss_post_begin(R, T)
    dev.cs_begin(C, T)
    rngs = [copy_rng(g) for g in plan["rngs"]]
    want = cr.History(C, T, M)
    for rec in plan["records"]:
        if R:
            dev.ss_sweep_replicas(rec["orders"], rec["sigmaE"], rec["sigmaG"], rec["estPi"], rec["adaV"], rngs)
        else:
            dev.ss_sweep(rec["orders"][0], rec["sigmaE"][0], rec["sigmaG"][0], rec["estPi"][0], rec["adaV"][0], rngs[0])
        before = fetch(dev, R)
        dev.ss_cs_add(R)
        after = fetch(dev, R)
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
        dev.ss_post_add()
        chains = before[1:] if R else before[:1]
        want.add(np.stack([c[1] for c in chains]) != 0)
        assert np.array_equal(dev.cs_history(), want.words)
    cnt = dev.cs_counts()
    assert np.array_equal(cnt, want.counts()) and np.any((cnt > 0) & (cnt < C * T))
    assert np.array_equal(cnt, np.uint32(C * T) - dev.ss_post_get()[3][0])
    # the history does not depend on the ss state
    dev.ss_post_end()
    dev.ss_end()
    assert np.array_equal(dev.cs_history(), want.words)
    dev.cs_end()


@pytest.fixture(scope="module")
def ld():
    geno, runs = cc.ld_genotypes()
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), cc.N)
    masks = {W: dev.ld_mask(W, cc.R2)[:2] for W in cc.WINDOWS}
    return dev, runs, masks


def same(got, want, what):
    for name, g, w in zip(("status", "size", "sum", "pep", "members"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, np.flatnonzero(np.asarray(g != w).reshape(len(w), -1).any(axis=1))[:5])


@pytest.mark.parametrize("nrec", sorted(cc.SHAPES))
@pytest.mark.parametrize("W", cc.WINDOWS)
def test_sets(ld, W, nrec):
    dev, runs, masks = ld
    fwd, bwd = masks[W]
    C, T = cc.SHAPES[nrec]
    flags = cc.crafted_flags(runs, cc.M, nrec, cc.SEEDS[(W, nrec)])
    h = cc.history_of(flags, C, T)
    dev.cs_begin(C, T)
    for t in range(T):
        dev.cs_add_flags(flags[t * C:(t + 1) * C])
    cnt = dev.cs_counts()
    assert np.array_equal(cnt, h.counts()) and np.array_equal(dev.cs_history(), h.words)
    leads = cc.leads_of(cnt)
    need = cr.ceil_count(cc.ALPHA, nrec)
    notes, results = {}, {}
    rng = np.random.default_rng(W + nrec)
    for k in cc.MAX_SIZES:
        want = cr.candidates(leads, cnt, h.words, cc.M, W, fwd, bwd, need, k, notes)
        got = dev.cs_sets(W, fwd, bwd, leads, need, k)
        same(got, want, (W, nrec, k))
        results[k] = got
        # another order, and split over two calls
        p = rng.permutation(len(leads))
        same(dev.cs_sets(W, fwd, bwd, leads[p], need, k), tuple(a[p] for a in got), (W, nrec, k, "permuted"))
        cut = len(leads) // 3
        two = [dev.cs_sets(W, fwd, bwd, part, need, k) for part in (leads[:cut], leads[cut:])]
        same(tuple(np.concatenate(pair) for pair in zip(*two)), got, (W, nrec, k, "two calls"))
    assert dev.last_cs_ms()[2] > 0.0
    assert cc.conditions(results, leads, cnt, nrec, notes) == []
    # after a part of the records only: the sets of the records added so far
    if T > 1:
        part = cc.history_of(flags[:C * (T // 2)], C, T // 2)
        dev.cs_begin(C, T)
        for t in range(T // 2):
            dev.cs_add_flags(flags[t * C:(t + 1) * C])
        pc = dev.cs_counts()
        assert np.array_equal(pc, part.counts())
        pl = cc.leads_of(pc)
        pw = np.zeros_like(h.words)
        pw[:part.words.shape[0]] = part.words
        same(dev.cs_sets(W, fwd, bwd, pl, max(1, need // 2), 64), cr.candidates(pl, pc, pw, cc.M, W, fwd, bwd, max(1, need // 2), 64), (W, nrec, "half"))


def test_refusals(ld):
    dev, _, masks = ld
    M = cc.M
    fwd, bwd = masks[64]

    def refused(call, msg):
        with pytest.raises(capi.HgError) as e:
            call()
        assert msg in str(e.value), (msg, str(e.value))

    L = dev.L
    dev.cs_end()
    assert dev.last_cs_ms() == (0.0, 0.0, 0.0)
    for name, call in (("hgibbs_cs_add_flags", lambda: capi.check(L.hgibbs_cs_add_flags(dev.h, None))), ("hgibbs_ss_cs_add", lambda: dev.ss_cs_add(0)),
                       ("hgibbs_cs_counts", dev.cs_counts), ("hgibbs_cs_history", lambda: capi.check(L.hgibbs_cs_history(dev.h, None))),
                       ("hgibbs_cs_sets", lambda: dev.cs_sets(64, fwd, bwd, [0], 1, 1))):
        refused(call, "%s: no inclusion history on this handle (hgibbs_cs_begin first)" % name)
    refused(lambda: capi.check(L.hgibbs_cs_begin(None, 1, 1)), "hgibbs_cs_begin: null handle")
    refused(lambda: capi.Device(0).cs_begin(1, 1), "hgibbs_cs_begin: no genotypes loaded on this handle")
    refused(lambda: dev.cs_begin(0, 4), "hgibbs_cs_begin: C = 0 chains, at least 1")
    refused(lambda: dev.cs_begin(2, 0), "hgibbs_cs_begin: T = 0 records per chain, at least 1")
    refused(lambda: dev.cs_begin(4, 2 ** 30), "hgibbs_cs_begin: C = 4 chains of T = 1073741824 records: the number of records C T must stay below 2^32")
    # 2^26 words per marker are 512 MiB: 600 GiB at M = 1200, more than any device holds
    refused(lambda: plain_device(1200).cs_begin(65535, 65537), "hgibbs_cs_begin: the history of M = 1200 markers over NREC = 4294967295 records (67108864 words per marker")

    dev.cs_begin(2, 2)
    refused(lambda: capi.check(L.hgibbs_cs_add_flags(dev.h, None)), "hgibbs_cs_add_flags: null flags")
    refused(lambda: dev.ss_cs_add(0), "hgibbs_ss_cs_add: no summary-statistics state on this handle (hgibbs_ss_begin first)")
    dev.ss_begin(4000.0, 8, np.random.default_rng(1).normal(0.0, 60.0, M))
    refused(lambda: dev.ss_cs_add(2), "hgibbs_ss_cs_add: no replicas on this handle (hgibbs_ss_replicas first)")
    refused(lambda: dev.ss_cs_add(0), "hgibbs_ss_cs_add: R = 0 is 1 chains, but hgibbs_cs_begin opened the history for C = 2")
    dev.ss_replicas(3)
    refused(lambda: dev.ss_cs_add(2), "hgibbs_ss_cs_add: R = 2, but hgibbs_ss_replicas allocated 3 replicas")
    refused(lambda: dev.ss_cs_add(3), "hgibbs_ss_cs_add: R = 3 is 3 chains, but hgibbs_cs_begin opened the history for C = 2")
    dev.ss_replicas(2)
    dev.ss_cs_add(2)
    dev.ss_end()  # the history stays
    dev.cs_add_flags(np.ones((2, M), np.uint8))
    refused(lambda: dev.cs_add_flags(np.ones((2, M), np.uint8)), "hgibbs_cs_add_flags: the 2 planned records are all added")
    assert np.array_equal(dev.cs_counts(), np.full(M, 2, np.uint32))  # (the replicas' components start at 0)

    u64, u32 = capi._u64, capi._u32
    out = [np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint64), np.zeros(4, np.uint32), np.zeros(4, np.uint32)]

    def sets(W=64, f=fwd, b=bwd, leads=(0,), need=1, max_size=1):
        ld_ = np.array(leads, dtype=np.uint32)
        capi.check(L.hgibbs_cs_sets(dev.h, W, u64(f) if f is not None else None, u64(b) if b is not None else None, ld_.size, u32(ld_), need, max_size, u32(out[0]),
                                    u32(out[1]), u64(out[2]), u32(out[3]), u32(out[4])))

    refused(lambda: sets(W=0), "hgibbs_cs_sets: W = 0, must be in [1, 4096]")
    refused(lambda: sets(W=4097), "hgibbs_cs_sets: W = 4097, must be in [1, 4096]")
    refused(lambda: sets(f=None), "hgibbs_cs_sets: null mask (fwd)")
    refused(lambda: sets(b=None), "hgibbs_cs_sets: null mask (bwd)")
    refused(lambda: sets(leads=(1, M)), "hgibbs_cs_sets: leads[1] = 300 is not below M = 300")
    refused(lambda: sets(leads=(5, 7, 5)), "hgibbs_cs_sets: leads[2] = 5 is among the leads twice")
    refused(lambda: sets(need=0), "hgibbs_cs_sets: need = 0, a set needs a count of at least 1")
    refused(lambda: sets(max_size=0), "hgibbs_cs_sets: max_size = 0, must be in [1, 256]")
    refused(lambda: sets(max_size=257), "hgibbs_cs_sets: max_size = 257, must be in [1, 256]")
    assert dev.last_cs_ms()[2] == 0.0
    sets(leads=(M - 1, 0), need=2)
    assert out[0][:2].tolist() == [0, 0] and out[1][:2].tolist() == [1, 1] and out[3][:2].tolist() == [2, 2] and out[4][:2].tolist() == [M - 1, 0]
    assert dev.last_cs_ms()[2] > 0.0
    # a second begin replaces the first; the end may be called twice
    dev.cs_begin(1, 3)
    assert not dev.cs_counts().any()
    dev.cs_end()
    dev.cs_end()
    refused(dev.cs_counts, "hgibbs_cs_counts: no inclusion history on this handle (hgibbs_cs_begin first)")
