"""The second walker's candidate search (hg_walker2.hip.h: w2_first_candidate, w2_without_candidate) on the host, through
hgibbs_walker_search -- the functions the decider calls on the device -- against a naive loop over the window's slots.

The chain waves answer with one 64-bit mask each (wave i: the slots 64 i .. 64 i + 63); the decider wants the first candidate in
WINDOW ORDER from the cursor's slot: upwards, wrapping at the window's size -- for a cursor in the middle of a wave that wave is
visited twice, its upper lanes first and its lower lanes last.  A candidate the exact decision turns down is cleared and the
search goes on: repeated until the masks are empty, that lists every candidate once, in window order.  Windows below 64 slots use
one wave, and only bits below the window's size are ever set."""
import ctypes as C

import numpy as np
import pytest

# (window, chain waves): the windows the engine runs -- below 64 slots one partly used wave -- and, beside them, every wave count 1 .. 4 with
# all its slots in use: three waves (192 slots) is no window of the engine's, but the search takes it, and its wrap is the one at a wave
# count that is no power of two
SHAPES = [(8, 1), (32, 1), (64, 1), (128, 2), (192, 3), (256, 4)]


@pytest.fixture(scope="module")
def search(gpu_lib):
    def run(masks, nch, cursor):
        m = (C.c_uint64 * 4)(*([int(x) for x in masks] + [0] * (4 - len(masks))))
        out = (C.c_uint32 * 256)()
        n = gpu_lib.hgibbs_walker_search(m, nch, cursor, out, 256)
        assert n >= 0
        return list(out[:n])
    return run


def naive(bits, B, cursor):
    """every set slot of the window, in the order (cursor, cursor + 1, ... ) mod B"""
    return [(cursor + d) % B for d in range(B) if bits[(cursor + d) % B]]


def masks_of(bits, nch):
    return [sum(1 << l for l in range(64) if 64 * i + l < len(bits) and bits[64 * i + l]) for i in range(nch)]


def check(search, bits, B, nch):
    """every cursor slot of the window; the entry point lists the candidates by "first, clear it, next" until the masks are empty"""
    assert B <= 64 * nch and (nch == 1 or B == 64 * nch)
    masks = masks_of(bits, nch)
    for cursor in range(B):
        assert search(masks, nch, cursor) == naive(bits, B, cursor), (B, nch, cursor, [hex(m) for m in masks])


def test_every_wave_count_is_covered():
    assert sorted({nch for _, nch in SHAPES}) == [1, 2, 3, 4] and sorted({B for B, _ in SHAPES if B != 192}) == [8, 32, 64, 128, 256]


@pytest.mark.parametrize("B,nch", SHAPES)
def test_empty_and_full(search, B, nch):
    check(search, np.zeros(B, bool), B, nch)
    check(search, np.ones(B, bool), B, nch)


@pytest.mark.parametrize("B,nch", SHAPES)
def test_single_bits_at_the_waves_edges(search, B, nch):
    # lanes 0 and 63 of every wave (a window below 64 slots: its first and last slot), alone and all together
    edges = sorted({s for w in range(nch) for s in (64 * w, min(64 * w + 63, B - 1))})
    for s in edges:
        bits = np.zeros(B, bool)
        bits[s] = True
        check(search, bits, B, nch)
    bits = np.zeros(B, bool)
    bits[edges] = True
    check(search, bits, B, nch)


@pytest.mark.parametrize("B,nch", SHAPES)
def test_random_masks(search, B, nch):
    rng = np.random.default_rng(1000 + B)
    for density in (0.02, 0.3, 0.9):
        for _ in range(4):
            check(search, rng.random(B) < density, B, nch)


@pytest.mark.parametrize("nch", [1, 2, 3, 4])
def test_every_cursor_slot_with_every_single_candidate(search, nch):
    # each cursor slot against each candidate slot -- every wrap, inside a wave and at the window's end
    B = 64 * nch
    for s in range(B):
        masks = [(1 << (s & 63)) if i == s >> 6 else 0 for i in range(nch)]
        for cursor in range(B):
            assert search(masks, nch, cursor) == [s]


def test_arguments_are_checked(gpu_lib):
    m = (C.c_uint64 * 4)(1, 0, 0, 0)
    out = (C.c_uint32 * 4)()
    assert gpu_lib.hgibbs_walker_search(m, 0, 0, out, 4) == -1
    assert gpu_lib.hgibbs_walker_search(m, 5, 0, out, 4) == -1
    assert gpu_lib.hgibbs_walker_search(m, 2, 128, out, 4) == -1
    m = (C.c_uint64 * 4)(0xff, 0, 0, 0)
    assert gpu_lib.hgibbs_walker_search(m, 1, 0, out, 4) == -1  # more candidates than room
