"""What the tests of the LD masks and of the greedy selection share (hgibbs_ld_mask, hgibbs_ld_greedy): the masks'
layout in NumPy, and a Python restatement of the walk on a dense adjacency."""
import numpy as np


def pack(band):
    """(M, W) bool, column d - 1 = offset d -> (M, wpr) uint64 in the masks' layout"""
    M, W = band.shape
    wpr = (W + 63) // 64
    full = np.zeros((M, wpr * 64), dtype=np.uint8)
    full[:, :W] = band
    return np.packbits(full, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(M, wpr)


def unpack(mask, W):
    """(M, wpr) uint64 -> (M, W) bool and whether a bit is set at an offset above W"""
    M = mask.shape[0]
    bits = np.unpackbits(np.ascontiguousarray(mask).astype("<u8").view(np.uint8).reshape(M, -1), axis=1, bitorder="little").astype(bool)
    return bits[:, :W], bool(bits[:, W:].any())


def backward_of(fband):
    """the backward band of a forward band: bband[q, d - 1] = fband[q - d, d - 1] where q >= d"""
    M, W = fband.shape
    bband = np.zeros_like(fband)
    for d in range(1, min(W, M - 1) + 1):
        bband[d:, d - 1] = fband[:M - d, d - 1]
    return bband


def adjacency(fband, bband):
    """A[v, q]: the pair's bit is set in v's forward or backward row"""
    M, W = fband.shape
    A = np.zeros((M, M), dtype=bool)
    for d in range(1, min(W, M - 1) + 1):
        v = np.arange(M - d)
        A[v, v + d] = fband[:M - d, d - 1]
        A[v + d, v] = bband[d:, d - 1]
    return A


def walk(A, order, may_lead=None):
    """the walk of hgibbs_ld_greedy, literally"""
    M = A.shape[0]
    owner = np.full(M, -1, dtype=np.int32)
    part = np.zeros(M, dtype=bool)
    part[np.asarray(order, dtype=np.int64)] = True
    for v in order:
        v = int(v)
        if owner[v] != -1:
            continue
        if may_lead is not None and not may_lead[v]:
            continue
        owner[v] = v
        owner[A[v] & part & (owner == -1)] = v
    return owner


def check_properties(A, order, owner, may_lead=None):
    """no two leaders share a set bit; every claimed marker has a set bit with its leader, which comes earlier in the order;
    non-participants are -1.  (Earlier in the order: a marker that may not lead is passed over when the walk reaches it and stays open to
    a leader that comes later, so for such a marker the leader's place is not bound; for every marker that may lead it is.)"""
    M = A.shape[0]
    order = np.asarray(order, dtype=np.int64)
    rank = np.full(M, -1, dtype=np.int64)
    rank[order] = np.arange(order.size)
    leaders = np.flatnonzero(owner == np.arange(M))
    assert not (A | A.T)[np.ix_(leaders, leaders)].any(), "two leaders share a set bit"
    for q in np.flatnonzero((owner != -1) & (owner != np.arange(M))):
        v = int(owner[q])
        assert owner[v] == v, "marker %d is owned by %d, which is no leader" % (q, v)
        assert A[v, q], "marker %d has no set bit with its leader %d" % (q, v)
        assert rank[v] >= 0 and rank[q] >= 0, "marker %d or its leader %d does not participate" % (q, v)
        if may_lead is None or may_lead[q]:
            assert rank[v] < rank[q], "leader %d does not come before marker %d in the order" % (v, q)
        assert may_lead is None or may_lead[v], "leader %d may not lead" % v
    assert np.all(owner[rank < 0] == -1), "a marker that does not participate is owned"
