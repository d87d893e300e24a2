"""The three sweeps of the summary-statistics engine interleaved on ONE handle (DESIGN.md sections 31-33): hgibbs_ss_sweep,
hgibbs_ss_sweep_streams and hgibbs_ss_sweep_replicas share one set of staging buffers (generator states, results, bounds, grouped
orders, masks), sized at the largest chains x intervals seen so far.  The sequence below grows them twice, runs every entry point with
buffers larger than it needs, changes G K between two replica sweeps and replaces the replicas.

Every call has a twin on a handle that only ever makes calls of one OTHER kind, so that twin's buffers have another history and no
fault of the shared staging can show in both: the handle's own chain (single and streams sweeps) is mirrored by the one replica of a
handle that only makes replica sweeps, and replica r by the own chain of a handle that only makes streams sweeps.  (That the kinds give
one another's bits from the same inputs is what tests/test_gpu_ss_streams.py and tests/test_gpu_ss_replicas.py hold.)  After each call
the effects, components, acum, c, cass, nnz and every generator's words and index are equal bit for bit, the handle's own chain is as it
was after a replica sweep, and the replicas are as they were after a sweep of the handle's chain."""
import numpy as np
import pytest

import ss_common as sc
from hydra_amd import capi, synth
from test_gpu_ss_sweep import N, seeded
from test_ss_streams_cpu import blocks_ahead, words

pytestmark = pytest.mark.gpu

M, W, N_EFF = 301, 8, 4000.0
SIZES = [40, 45, 37, 50, 43, 41, 45]  # seven blocks: a zero-width place of `ahead` before each
B7 = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
B3 = B7[[0, 2, 4, 7]]
B1 = B7[[0, 7]]
GROUPS = (np.arange(M) % 2).astype(np.int32)
MS_K3 = np.array([[0.0, 0.001, 0.01], [0.0, 0.01, 0.1]])
MS_K4 = sc.MS2


def model(dev, mS):
    cVaI = np.zeros_like(mS)
    cVaI[:, 1:] = 1.0 / mS[:, 1:]
    dev.set_model(GROUPS, mS.copy(), cVaI)


def open_device(bed, xty, ahead, mS=MS_K3):
    dev = capi.Device(0)
    dev.load_bed(bed, N)
    model(dev, mS)
    dev.ss_begin(N_EFF, W, xty, ahead)
    return dev


def inputs(seed, K):
    """one chain's arguments of one sweep: order, sigmaE, sigmaG, estPi, adaV"""
    rs = np.random.default_rng(seed)
    return (rs.permutation(M).astype(np.int32), float(rs.uniform(0.4, 0.7)), rs.uniform(0.2, 0.6, 2), rs.dirichlet(np.ones(K) * 2.0, 2),
            (rs.random(M) < 0.85).astype(np.uint8))


def gens(S, seed):
    """S generators, the same for the same seed; some begin inside their block, one at its end"""
    out = [seeded(1000 * seed + s) for s in range(S)]
    for s, g in enumerate(out):
        g.idx = (211 * (seed + s)) % 625
    return out


def own_state(dev):
    beta, comp, acum = dev.get_beta()
    return dict(beta=beta, comp=comp, acum=acum, c=dev.ss_state()[0])


def replica_state(dev, r):
    beta, comp, acum, c = dev.ss_replica_get(r)
    return dict(beta=beta, comp=comp, acum=acum, c=c)


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def outcome(state, cass, nnz, rngs):
    return dict(state, cass=cass, nnz=np.uint64(nnz), x=np.stack([words(g)[0] for g in rngs]), idx=np.array([int(g.idx) for g in rngs]))


def test_interleaved_sweeps_on_one_handle():
    geno = synth.make_genotypes(M, N, seed=61, missing_rate=0.02)
    bed = synth.pack_bed_columns(geno)
    rs = np.random.default_rng(62)
    xty = rs.normal(0.0, np.sqrt(N_EFF), M)
    xty[rs.random(M) < 0.15] *= 8.0  # signals: effects that leave 0, and come back
    ahead = blocks_ahead(SIZES, W)
    assert np.count_nonzero(ahead == 0) == 7
    start = [np.where(rs.random(M) < 0.3, rs.normal(0.0, 0.05, M), 0.0) for _ in range(3)]  # own chain, replicas 0 and 1

    mixed = open_device(bed, xty, ahead)
    mixed.set_beta(start[0])
    own_twin = open_device(bed, xty, ahead)  # replica sweeps only: its one replica is the mixed handle's own chain
    own_twin.ss_replicas(1)
    own_twin.ss_replica_set_beta(0, start[0])
    rep_twins = []  # streams sweeps only: the own chain of rep_twins[r] is the mixed handle's replica r
    moved = [0]
    K = [3]

    def replicas_now():
        return [replica_state(mixed, r) for r in range(len(rep_twins))]

    def own_sweep(step, bounds):
        """hgibbs_ss_sweep (bounds None) or hgibbs_ss_sweep_streams on the mixed handle's own chain"""
        S = 1 if bounds is None else len(bounds) - 1
        order, sigmaE, sigmaG, estPi, adaV = inputs(100 + step, K[0])
        before = replicas_now()
        g, tg = gens(S, step), gens(S, step)
        if bounds is None:
            cass, nnz = mixed.ss_sweep(order, sigmaE, sigmaG, estPi, adaV, g[0])
        else:
            cass, nnz = mixed.ss_sweep_streams(order, sigmaE, sigmaG, estPi, adaV, bounds, g)
        tcass, tnnz = own_twin.ss_sweep_replicas(order[None], [sigmaE], sigmaG[None], estPi[None], adaV, tg if bounds is None else [tg], bounds=bounds)
        same(outcome(own_state(mixed), cass, nnz, g), outcome(replica_state(own_twin, 0), tcass[0], tnnz[0], tg), "step %d" % step)
        for r, (a, b) in enumerate(zip(before, replicas_now())):
            same(a, b, "step %d: replica %d after a sweep of the handle's chain" % (step, r))
        moved[0] += int(nnz)

    def replica_sweep(step, bounds):
        """hgibbs_ss_sweep_replicas on the mixed handle; bounds None: the single stream"""
        R = len(rep_twins)
        S = 1 if bounds is None else len(bounds) - 1
        ins = [inputs(100 * step + r, K[0]) for r in range(R)]
        before = own_state(mixed)
        g, tg = [gens(S, 10 * step + r) for r in range(R)], [gens(S, 10 * step + r) for r in range(R)]
        cass, nnz = mixed.ss_sweep_replicas(np.stack([x[0] for x in ins]), [x[1] for x in ins], np.stack([x[2] for x in ins]), np.stack([x[3] for x in ins]),
                                            np.stack([x[4] for x in ins]), [x[0] for x in g] if bounds is None else g, bounds=bounds)
        for r in range(R):
            tcass, tnnz = rep_twins[r].ss_sweep_streams(*ins[r], B1 if bounds is None else bounds, tg[r])
            same(outcome(replica_state(mixed, r), cass[r], nnz[r], g[r]), outcome(own_state(rep_twins[r]), tcass, tnnz, tg[r]), "step %d, replica %d" % (step, r))
            moved[0] += int(nnz[r])
        same(before, own_state(mixed), "step %d: the handle's chain after a replica sweep" % step)

    own_sweep(1, B3)
    own_sweep(2, None)
    own_sweep(3, B7)  # the buffers grow: 3 -> 7 states
    mixed.ss_replicas(2)
    for r in range(2):
        rep_twins.append(open_device(bed, xty, ahead))
        mixed.ss_replica_set_beta(r, start[1 + r])
        rep_twins[r].set_beta(start[1 + r])
    replica_sweep(4, None)
    replica_sweep(5, B7)  # and again: 7 -> 14
    own_sweep(6, None)
    own_sweep(7, B3)  # larger than needed
    K[0] = 4  # G K changes under the replicas' tables and counters
    for dev in [mixed] + rep_twins:
        model(dev, MS_K4)
    replica_sweep(8, B3)  # two chains at a stride of 3 in buffers of 14
    mixed.ss_replicas(3)  # new replicas: c = xty, every effect 0
    for dev in rep_twins:
        dev.ss_begin(N_EFF, W, xty, ahead)
    rep_twins.append(open_device(bed, xty, ahead, MS_K4))
    replica_sweep(9, B3)
    assert moved[0] > 0
