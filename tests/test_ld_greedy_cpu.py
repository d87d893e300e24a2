"""The greedy selection on LD masks (hgibbs_ld_greedy, host only) against a Python restatement that builds a dense boolean adjacency
from the two masks and walks the order literally (tests/ldwalk.py).  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from hydra_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldwalk  # noqa: E402

SIZES = [1, 2, 63, 64, 65, 200]
WINDOWS = [1, 63, 64, 65, 130]


def random_masks(M, W, density, rng):
    """symmetric: each forward bit with its backward twin; nothing past the last marker"""
    fband = rng.random((M, W)) < density
    fband &= (np.arange(M)[:, None] + np.arange(1, W + 1)[None, :]) < M
    bband = ldwalk.backward_of(fband)
    return fband, bband


def orders(M, rng):
    full = rng.permutation(M).astype(np.uint32)
    return {"permutation": full, "subset": full[:max(0, (2 * M) // 3)].copy(), "bim": np.arange(M, dtype=np.uint32),
            "reverse": np.arange(M, dtype=np.uint32)[::-1].copy()}


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("M", SIZES)
def test_equals_the_python_walk(M, W):
    rng = np.random.default_rng(1000 * M + W)
    for density in (0.02, 0.15, 0.5):
        fband, bband = random_masks(M, W, density, rng)
        fwd, bwd = ldwalk.pack(fband), ldwalk.pack(bband)
        A = ldwalk.adjacency(fband, bband)
        assert np.array_equal(A, A.T)
        for name, order in orders(M, rng).items():
            for lead in ("all", "none", "random"):
                may = None if lead == "all" else (np.zeros(M, dtype=np.uint8) if lead == "none" else (rng.random(M) < 0.4).astype(np.uint8))
                what = "M=%d W=%d density=%g order=%s may_lead=%s" % (M, W, density, name, lead)
                got = capi.ld_greedy(M, W, fwd, bwd, order, may)
                ref = ldwalk.walk(A, order, may)
                assert np.array_equal(got, ref), what
                ldwalk.check_properties(A, order, got, may)
                if lead == "none":
                    assert np.all(got == -1), what
                if lead == "all":  # every participating marker ends up owned
                    assert np.all(got[order.astype(np.int64)] != -1), what


def test_only_the_leaders_own_rows_count():
    """asymmetric masks: a pair passes when its bit is set in the LEADER's forward or backward row"""
    M, W = 70, 65
    rng = np.random.default_rng(5)
    fband = rng.random((M, W)) < 0.2
    fband &= (np.arange(M)[:, None] + np.arange(1, W + 1)[None, :]) < M
    bband = rng.random((M, W)) < 0.2
    bband &= (np.arange(M)[:, None] - np.arange(1, W + 1)[None, :]) >= 0
    A = ldwalk.adjacency(fband, bband)
    order = rng.permutation(M).astype(np.uint32)
    assert np.array_equal(capi.ld_greedy(M, W, ldwalk.pack(fband), ldwalk.pack(bband), order), ldwalk.walk(A, order))


def test_bits_above_w_and_past_the_ends_are_ignored():
    M, W = 40, 70
    full = np.full((M, 2), ~np.uint64(0), dtype=np.uint64)
    order = np.arange(M, dtype=np.uint32)
    got = capi.ld_greedy(M, W, full, full, order)
    assert np.all(got == 0)  # marker 0 leads and reaches every other marker (M - 1 < W)
    got = capi.ld_greedy(M, W, full, full, order[::-1].copy())
    assert np.all(got == M - 1)


def test_refusals():
    M, W = 10, 5
    z = np.zeros((M, 1), dtype=np.uint64)
    with pytest.raises(capi.HgError, match=r"order\[2\] = 3 is in the order twice"):
        capi.ld_greedy(M, W, z, z, np.array([3, 1, 3], dtype=np.uint32))
    with pytest.raises(capi.HgError, match=r"order\[1\] = 10 is not below M = 10"):
        capi.ld_greedy(M, W, z, z, np.array([3, 10], dtype=np.uint32))
    with pytest.raises(capi.HgError, match="W = 0, must be in"):
        capi.ld_greedy(M, 0, z, z, np.arange(M, dtype=np.uint32))
    with pytest.raises(capi.HgError, match="W = 4097, must be in"):
        capi.ld_greedy(M, 4097, z, z, np.arange(M, dtype=np.uint32))
    L = capi.lib()
    order = np.arange(M, dtype=np.uint32)
    owner = np.zeros(M, dtype=np.int32)
    u64, u32, i32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    zp, op, wp = z.ctypes.data_as(u64), order.ctypes.data_as(u32), owner.ctypes.data_as(i32)
    for args, msg in [((None, zp, op, M, None, wp), "null mask (fwd)"), ((zp, None, op, M, None, wp), "null mask (bwd)"),
                      ((zp, zp, None, M, None, wp), "null order"), ((zp, zp, op, M, None, None), "null output")]:
        assert L.hgibbs_ld_greedy(M, W, *args) != 0
        assert msg in L.hgibbs_last_error().decode()
    # nothing participates: every owner is -1
    assert L.hgibbs_ld_greedy(M, W, zp, zp, None, 0, None, wp) == 0 and np.all(owner == -1)
