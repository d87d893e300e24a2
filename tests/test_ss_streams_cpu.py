"""Independent LD blocks in parallel streams, the part that needs no device: the partition of the markers
into intervals of whole blocks (hgibbs_ss_partition) against a plain restatement; the host engine with one generator per interval
(hgibbs_ss_sweep_streams_host) against one call of hgibbs_ss_sweep_host per interval on the sliced sub-problem, bit for bit (same
code, same host); what both refuse; and the chain's iteration replayed by hand from snapshots of its state."""
import numpy as np
import pytest

import ss_common as sc
from hydra_amd import capi

# lengths of the human autosomes in Mb, rounded: chromosome 1 is 8.6 % of their sum
AUTOSOME_MB = [248, 242, 198, 190, 182, 171, 159, 145, 138, 134, 135, 133, 114, 107, 102, 90, 83, 80, 59, 64, 47, 51]


def partition(ahead, S_max):
    """The rule restated: a cut before j iff the running maximum of k + ahead[k] over k < j is below j; blocks in marker order go
    into the current interval, which closes as soon as it holds ceil(M / S_max) markers; the remainder is the last interval."""
    M = len(ahead)
    reach = np.maximum.accumulate(np.arange(M) + np.asarray(ahead, dtype=np.int64))
    cuts = [j for j in range(1, M) if reach[j - 1] < j]
    quota = -(-M // S_max)
    bounds = [0]
    for j in cuts:
        if j - bounds[-1] >= quota:
            bounds.append(j)
    return np.array(bounds + [M], dtype=np.uint32)


def blocks_ahead(sizes, W):
    """ahead of a band whose blocks have the given sizes: min(W, markers left in the block)"""
    return np.concatenate([np.minimum(W, n - 1 - np.arange(n)) for n in sizes]).astype(np.uint32)


def human_like(M, W):
    sizes = np.diff(np.round(np.cumsum([0] + AUTOSOME_MB) * (M / sum(AUTOSOME_MB))).astype(int))
    return sizes, blocks_ahead(sizes, W)


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


def words(r):
    return np.array(r.x, dtype=np.uint32), int(r.idx)


def same_rng(a, b):
    return np.array_equal(words(a)[0], words(b)[0]) and a.idx == b.idx


# ---- the partition ----
def test_partition_one_marker():
    assert np.array_equal(capi.ss_partition([0], 8), [0, 1])


def test_partition_without_a_cut():
    ahead = blocks_ahead([50], 3)
    for S_max in (1, 4, 1024):
        assert np.array_equal(capi.ss_partition(ahead, S_max), [0, 50])
        assert np.array_equal(partition(ahead, S_max), [0, 50])


@pytest.mark.parametrize("S_max", [4, 1024])
def test_partition_every_marker_its_own_block(S_max):
    M = 1030
    got = capi.ss_partition(np.zeros(M, dtype=np.uint32), S_max)
    assert np.array_equal(got, partition(np.zeros(M, dtype=int), S_max))
    assert len(got) - 1 <= S_max and got[0] == 0 and got[-1] == M and np.all(np.diff(got.astype(np.int64)) > 0)
    if S_max == 4:  # ceil(1030 / 4) = 258: three full intervals and the remainder
        assert np.array_equal(got, [0, 258, 516, 774, 1030])
    else:  # quota 2: 515 intervals of two
        assert len(got) - 1 == 515


def test_partition_a_marker_no_window_holds_can_be_jumped_over():
    # the engines take a window per pair: ahead[k] >= q - k.  Here marker 1's window holds 2, 3 and 4 while 2 and 3 hold nobody.
    # The place before 1 is a cut (0 reaches nothing), the places before 2, 3 and 4 are crossed by marker 1's window although the
    # marker just behind each has ahead == 0, and the places before 5 and 6 are cuts again.
    ahead = np.array([0, 3, 0, 0, 0, 0, 0], dtype=np.uint32)
    got = capi.ss_partition(ahead, 7)
    assert np.array_equal(got, [0, 1, 5, 6, 7])
    assert np.array_equal(got, partition(ahead, 7))
    # markers 1 and 2 reach nobody and nobody between 0 and 2 holds 2: only the running maximum (0 + 2 >= 2) says that the place
    # before 2 is no cut.  (With ss_back's definition back[2] = 2 here, so the two tests agree; the rule does not rely on it.)
    ahead = np.array([2, 0, 0, 0], dtype=np.uint32)
    assert np.array_equal(capi.ss_partition(ahead, 4), [0, 3, 4])
    assert np.array_equal(partition(ahead, 4), [0, 3, 4])


def test_partition_human_like_layout():
    M = 5744
    sizes, ahead = human_like(M, 8)
    assert sizes.sum() == M and 0.08 < sizes[0] / M < 0.09
    got = capi.ss_partition(ahead, 256)  # quota 23, the smallest chromosome has 94: nothing is merged
    assert np.array_equal(got, np.concatenate([[0], np.cumsum(sizes)]))
    assert np.array_equal(got, partition(ahead, 256))
    got = capi.ss_partition(ahead, 8)  # quota 718
    assert np.array_equal(got, partition(ahead, 8))
    assert len(got) - 1 <= 8 and set(got) <= set(np.concatenate([[0], np.cumsum(sizes)]))
    assert np.all(np.diff(got.astype(np.int64))[:-1] >= 718)


def test_partition_refusals():
    for ahead, S_max, msg in (([0, 0], 0, "S_max = 0"), ([0, 0], 1025, "S_max = 1025"), ([0, 1], 2, "marker 1 + ahead is past the last marker")):
        with pytest.raises(capi.HgError) as e:
            capi.ss_partition(ahead, S_max)
        assert msg in str(e.value)


# ---- the host engine ----
MS2 = sc.MS2


def problem(M, W, sizes, seed, two_groups=True):
    """A band with the given blocks (random, symmetric in meaning: only the `ahead` half is stored), a non-zero start, some adaV = 0."""
    rs = np.random.default_rng(seed)
    ahead = blocks_ahead(sizes, W)
    n_eff = 4000.0
    band = rs.uniform(-0.3, 0.3, (M, W)) * (n_eff - 1.0)
    band[np.arange(W)[None, :] >= ahead[:, None]] = 0.0
    xty = rs.normal(0.0, np.sqrt(n_eff), M)
    xty[rs.random(M) < 0.15] *= 8.0
    mS = MS2 if two_groups else sc.MS1
    G, K = mS.shape
    groups = (np.arange(M) % 3 == 0).astype(np.int32) if two_groups else None
    cVa = mS.copy()
    cVaI = np.zeros_like(mS)
    cVaI[:, 1:] = 1.0 / mS[:, 1:]
    beta0 = np.where(rs.random(M) < 0.3, rs.normal(0.0, 0.05, M), 0.0)
    sweeps = []
    for s in range(3):
        sigmaG = rs.uniform(0.2, 0.6, G)
        if two_groups:
            sigmaG[G - 1] = 0.0
        sweeps.append((rs.permutation(M).astype(np.int32), 0.4 + 0.1 * s, sigmaG, rs.dirichlet(np.ones(K) * 2.0, G), (rs.random(M) < 0.85).astype(np.uint8)))
    return dict(M=M, W=W, ahead=ahead, n_eff=n_eff, band=band, xty=xty, groups=groups, cVa=cVa, cVaI=cVaI, beta0=beta0, sweeps=sweeps)


@pytest.mark.parametrize("W,sizes", [(5, [1, 2, 254]), (64, [128, 129])], ids=["W5-1-2-254", "W64-128-129"])
def test_streams_host_is_sweep_host_per_interval(W, sizes):
    M = 257
    p = problem(M, W, sizes, seed=40 + W)
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    S = len(sizes)
    # all at once
    c, beta, comp, acum = p["xty"].copy(), p["beta0"].copy(), np.zeros(M, dtype=np.int32), np.zeros(M)
    rngs = [seeded(900 + s) for s in range(S)]
    # interval by interval on the slices
    c2, beta2, comp2, acum2 = c.copy(), beta.copy(), comp.copy(), acum.copy()
    rngs2 = [copy_rng(r) for r in rngs]
    updates = 0
    for order, sigmaE, sigmaG, estPi, adaV in p["sweeps"]:
        cass, nnz = capi.ss_sweep_streams_host(p["n_eff"], W, p["ahead"], p["band"], c, beta, comp, acum, p["groups"], p["cVa"], p["cVaI"], order, sigmaE,
                                               sigmaG, estPi, adaV, bounds, rngs)
        cass2, nnz2 = np.zeros_like(cass), 0
        for s in range(S):
            a, e = int(bounds[s]), int(bounds[s + 1])
            sub = [np.ascontiguousarray(v[a:e]) for v in (c2, beta2, comp2, acum2)]
            ca, nz = capi.ss_sweep_host(p["n_eff"], W, p["ahead"][a:e], p["band"][a:e], sub[0], sub[1], sub[2], sub[3],
                                        None if p["groups"] is None else p["groups"][a:e], p["cVa"], p["cVaI"], order[(order >= a) & (order < e)] - a, sigmaE,
                                        sigmaG, estPi, adaV[a:e], rngs2[s])
            for v, w in zip((c2, beta2, comp2, acum2), sub):
                v[a:e] = w
            cass2 += ca
            nnz2 += nz
        assert np.array_equal(beta, beta2) and np.array_equal(acum, acum2) and np.array_equal(c, c2) and np.array_equal(comp, comp2)
        assert np.array_equal(cass, cass2) and nnz == nnz2
        assert all(same_rng(x, y) for x, y in zip(rngs, rngs2))
        updates += nnz
    assert updates > 0 and np.any(beta != 0.0)


def test_one_stream_is_the_single_stream():
    M, W = 257, 5
    p = problem(M, W, [1, 2, 254], seed=3)
    st = [p["xty"].copy(), p["beta0"].copy(), np.zeros(M, dtype=np.int32), np.zeros(M)]
    st2 = [v.copy() for v in st]
    r1, r2 = [seeded(5)], seeded(5)
    for order, sigmaE, sigmaG, estPi, adaV in p["sweeps"]:
        a = capi.ss_sweep_streams_host(p["n_eff"], W, p["ahead"], p["band"], *st, p["groups"], p["cVa"], p["cVaI"], order, sigmaE, sigmaG, estPi, adaV, [0, M], r1)
        b = capi.ss_sweep_host(p["n_eff"], W, p["ahead"], p["band"], *st2, p["groups"], p["cVa"], p["cVaI"], order, sigmaE, sigmaG, estPi, adaV, r2)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and same_rng(r1[0], r2)
        assert all(np.array_equal(x, y) for x, y in zip(st, st2))


def test_streams_host_refusals():
    M, W = 12, 3
    p = problem(M, W, [4, 8], seed=1, two_groups=False)
    order, sigmaE, sigmaG, estPi, adaV = p["sweeps"][0]

    def call(bounds, rngs, S=None, order=order):
        st = [p["xty"].copy(), np.zeros(M), np.zeros(M, dtype=np.int32), np.zeros(M)]
        return capi.ss_sweep_streams_host(p["n_eff"], W, p["ahead"], p["band"], *st, None, p["cVa"], p["cVaI"], order, sigmaE, sigmaG, estPi, adaV, bounds, rngs, S=S)

    call([0, 4, 12], [seeded(1), seeded(2)])
    bad = seeded(2)
    bad.idx = 625
    twice = order.copy()
    twice[3] = twice[7]
    for kw, msg in ((dict(bounds=[0, 6, 12], rngs=[seeded(1), seeded(2)]), "bounds[1] = 6 is not a cut: the window of marker 4 reaches marker 7"),
                    (dict(bounds=[0, 4, 4, 12], rngs=[seeded(1)] * 3), "strictly ascending"),
                    (dict(bounds=[0, 12, 4, 12], rngs=[seeded(1)] * 3), "strictly ascending"),
                    (dict(bounds=[1, 4, 12], rngs=[seeded(1)] * 2), "bounds must run from 0 to M = 12"),
                    (dict(bounds=[0, 4, 11], rngs=[seeded(1)] * 2), "bounds must run from 0 to M = 12"),
                    (dict(bounds=[0], rngs=[seeded(1)], S=0), "S = 0, must be in [1, 1024]"),
                    (dict(bounds=np.zeros(1026), rngs=[seeded(1)], S=1025), "S = 1025, must be in [1, 1024]"),
                    (dict(bounds=[0, 4, 12], rngs=[seeded(1), bad]), "stream 1: rng idx 625 > 624"),
                    (dict(bounds=[0, 4, 12], rngs=[seeded(1), seeded(2)], order=twice), "the order must be a permutation")):
        with pytest.raises(capi.HgError) as e:
            call(**kw)
        assert msg in str(e.value), (msg, str(e.value))
        assert "hgibbs_ss_sweep_streams_host" in str(e.value)


# ---- the chain ----
def temper(z):
    z ^= z >> 11
    z ^= (z << 7) & 0x9d2c5680
    z ^= (z << 15) & 0xefc60000
    return (z ^ (z >> 18)) & 0xffffffff


def chain_case():
    M, N, W = sc.CASE_M, sc.CASE_N, 40
    rs = np.random.default_rng(17)
    X = rs.standard_normal((N, M))
    X = (X - X.mean(0)) / X.std(0, ddof=1)
    y = X[:, ::25] @ rs.normal(0.0, 0.15, len(range(0, M, 25))) + rs.standard_normal(N) * 0.8
    y = (y - y.mean()) / y.std(ddof=1)
    sizes = [90, 60, 150]
    ahead = blocks_ahead(sizes, W)
    band = sc.full_band(X, W)
    band[np.arange(W)[None, :] >= ahead[:, None]] = 0.0
    return M, N, W, ahead, band, X.T @ y, np.concatenate([[0], np.cumsum(sizes)])


def test_chain_iteration_is_the_streams_sweep_on_its_order():
    M, N, W, ahead, band, b, blocks = chain_case()
    plain = capi.SsChain(None, N, W, b, ahead=ahead, band=band, seed=31)
    before = plain.state()
    assert plain.streams()[1] == []
    ch = capi.SsChain(None, N, W, b, ahead=ahead, band=band, seed=31, streams=8)
    bounds, rngs = ch.streams()
    # quota ceil(300 / 8) = 38: every block is an interval of its own
    assert np.array_equal(bounds, blocks) and len(rngs) == 3
    # stream s is seeded from the next words of the chain's generator, which moves on by as many
    i0 = before["rng_idx"]
    assert i0 + 3 <= 624 and ch.state()["rng_idx"] == i0 + 3 and np.array_equal(ch.state()["rng_x"], before["rng_x"])
    for s in range(3):
        assert same_rng(rngs[s], seeded(temper(int(before["rng_x"][i0 + s]))))
    cVa = sc.MS1.copy()
    cVaI = np.zeros_like(cVa)
    cVaI[:, 1:] = 1.0 / cVa[:, 1:]
    adaV = np.ones(M, dtype=np.uint8)
    moved = 0
    for it in range(4):
        st = ch.state()
        beta, comp, acum, c = ch.effects()
        _, rngs = ch.streams()
        ch.iterate()
        cass, nnz = capi.ss_sweep_streams_host(N, W, ahead, band, c, beta, comp, acum, None, cVa, cVaI, ch.order(), st["sigmaE"], st["sigmaG"], st["estPi"], adaV,
                                               bounds, rngs)
        got = ch.effects()
        assert np.array_equal(got[0], beta) and np.array_equal(got[1], comp) and np.array_equal(got[2], acum) and np.array_equal(got[3], c), it
        assert np.array_equal(ch.state()["cass"], cass) and ch.last_nnz() == nnz, it
        assert all(same_rng(x, y) for x, y in zip(ch.streams()[1], rngs)), it
        moved += nnz
    assert moved > 0
    # another realisation than the single stream's, from the same seed
    for _ in range(4):
        plain.iterate()
    assert not np.array_equal(plain.effects()[0], ch.effects()[0])
    with pytest.raises(capi.HgError) as e:
        ch.set_streams(8)
    assert "hydra_ss_chain_set_streams" in str(e.value) and "4 iteration(s)" in str(e.value)


def test_chain_set_streams_refusals():
    M, N, W, ahead, band, b, _ = chain_case()
    ch = capi.SsChain(None, N, W, b, ahead=ahead, band=band, seed=31)
    for S_max in (0, 1025):
        with pytest.raises(capi.HgError) as e:
            ch.set_streams(S_max)
        assert "S_max = %d, must be in [1, 1024]" % S_max in str(e.value)
    ch.set_streams(2)  # quota 150: the first two blocks make one interval
    assert np.array_equal(ch.streams()[0], [0, 150, 300])
    with pytest.raises(capi.HgError) as e:
        ch.set_streams(2)
    assert "already set" in str(e.value)


def test_new_symbols_are_in_the_abi_list():
    for name in ("hgibbs_ss_partition", "hgibbs_ss_sweep_streams", "hgibbs_ss_sweep_streams_host", "hydra_ss_chain_set_streams", "hydra_ss_chain_streams"):
        assert name in capi.ABI_SYMBOLS and hasattr(capi.lib(), name)
