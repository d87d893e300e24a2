"""The host's fast marker shuffle (hydra_rng_shuffle -> hg::shuffle_libstdcxx6_fast) against the oracle's sequential
orc_rng_shuffle from the same generator state: the permutation element by element, and the generator afterwards (all
624 words and the position), because the sweep continues the same stream on the device.

Rejected words (a draw >= (i + 1) * scaling is thrown away and shifts every later word by one) are rare: about 60 per
million positions, next to none below 100 000.  Only the 1 M cases cover that path, and they assert that they do."""
import ctypes as C

import numpy as np
import pytest

import orc
from hydra_amd import capi

SIZES = [0, 1, 2, 3, 40, 623, 624, 625, 1000, 100000, 1000000]
SEEDS = [1222, 7, 99]
STARTS = [0, 1, 311, 623, 624]


def start_state(oracle, seed, idx):
    g = orc.OrcMt()
    oracle.orc_rng_seed(C.byref(g), seed)
    for _ in range(700):  # a state a running chain would hold: past the seeding block
        oracle.orc_rng_u32(C.byref(g))
    g.idx = idx
    return g


def to_product(g):
    st = capi.RngState()
    C.memmove(C.byref(st), C.byref(g), C.sizeof(orc.OrcMt))
    assert st.idx == g.idx
    return st


def words(st):
    return np.ctypeslib.as_array(st.x).copy(), int(st.idx)


def stream(g, count):
    """The next `count` raw outputs of the generator in state g (which is left alone)."""
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": np.ctypeslib.as_array(g.x).copy(), "pos": int(g.idx)}}
    return bg.random_raw(count).astype(np.uint32)


def words_consumed(oracle, before, after, n):
    """How many words the oracle's shuffle took: where its generator's next outputs continue the start state's stream."""
    if n < 2:
        return 0
    probe = orc.OrcMt()
    C.memmove(C.byref(probe), C.byref(after), C.sizeof(orc.OrcMt))
    nxt = np.array([oracle.orc_rng_u32(C.byref(probe)) for _ in range(8)], dtype=np.uint32)
    s = stream(before, n - 1 + 4096 + 8)
    for c in range(n - 1, n - 1 + 4096):
        if np.array_equal(s[c:c + 8], nxt):
            return c
    raise AssertionError("the oracle's generator does not continue the start state's stream")


def both(oracle, g, n, v0=None):
    v_ref = np.arange(n, dtype=np.int32) if v0 is None else v0.copy()
    v_new = v_ref.copy()
    st = to_product(g)
    oracle.orc_rng_shuffle(C.byref(g), v_ref.ctypes.data_as(C.POINTER(C.c_int)), n)
    capi.rng_shuffle(st, v_new)
    return v_ref, v_new, st


def test_numpy_lays_out_the_same_stream(oracle):
    g = start_state(oracle, 1222, 311)
    s = stream(g, 1000)
    assert [oracle.orc_rng_u32(C.byref(g)) for _ in range(1000)] == s.tolist()


@pytest.mark.parametrize("idx", STARTS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", SIZES)
def test_shuffle_equals_the_oracle(oracle, n, seed, idx):
    g = start_state(oracle, seed, idx)
    before = orc.OrcMt()
    C.memmove(C.byref(before), C.byref(g), C.sizeof(orc.OrcMt))
    v_ref, v_new, st = both(oracle, g, n)
    assert np.array_equal(v_new, v_ref)
    xr, ir = words(g)
    xn, i_n = words(st)
    assert i_n == ir
    assert np.array_equal(xn, xr)
    if n == 1000000:
        rejected = words_consumed(oracle, before, g, n) - (n - 1)
        print("n = %d seed %d idx %d: %d rejected words" % (n, seed, idx, rejected))
        assert rejected >= 1, "this case is here to cover rejected words and met none"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", [625, 1000, 100000, 1000000])
def test_two_shuffles_back_to_back(oracle, n, seed):
    """As the chain does across iterations: the second shuffle starts from the first one's array and generator."""
    g = start_state(oracle, seed, 311)
    st = to_product(g)
    v_ref = np.arange(n, dtype=np.int32)
    v_new = v_ref.copy()
    for _ in range(2):
        oracle.orc_rng_shuffle(C.byref(g), v_ref.ctypes.data_as(C.POINTER(C.c_int)), n)
        capi.rng_shuffle(st, v_new)
        assert np.array_equal(v_new, v_ref)
        xr, ir = words(g)
        xn, i_n = words(st)
        assert i_n == ir and np.array_equal(xn, xr)
    assert sorted(v_new.tolist()) == list(range(n))


def test_refuses_a_position_past_the_block():
    st = capi.RngState()
    st.idx = 625
    with pytest.raises(capi.HgError):
        capi.rng_shuffle(st, np.arange(4, dtype=np.int32))
