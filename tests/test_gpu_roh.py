"""hgibbs_roh on the device against tests/roh_restate.py: the list is equal field for field, over row counts around the 64-row wave and the
4096-slot pad, runs that start off the 64-marker grid of a selection with holes, every window width at which the shifts change shape,
and each filter binding.  Integers only, so equal means equal."""
import numpy as np
import pytest

import roh_restate as rr
from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu

MTOT = 1500
NS = [1, 15, 64, 65, 257, 4097]
WS = [1, 2, 8, 50, 64]
GAP_AT = 300  # position of the 700-marker run whose bp lies 10^6 behind its neighbour's


def runs_of(W):
    """run lengths W - 1, W, W + 1, 63, 64, 65, 129 and 700: every run after the first few starts off the 64-marker grid"""
    lens = [W - 1, W, W + 1, 63, 64, 65, 129, 700]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)


def selection(W):
    """the markers of the runs: every eleventh marker of the 1500 is left out; bp with a jump inside the last run"""
    run_off = runs_of(W)
    idx = np.arange(MTOT)[np.arange(MTOT) % 11 != 5][:run_off[-1]]
    step = np.random.default_rng(1).integers(1, 3000, size=MTOT)
    step[idx[run_off[-2] + GAP_AT]] += 10**6
    return run_off, idx.astype(np.uint32), np.cumsum(step).astype(np.int64)[idx]


def genotypes(N, W):
    """random calls with 2 % missing; planted per row: a stretch of 500 markers of the last run without het or missing call (its start
    moves with the row), the 129-marker run of every third row likewise; from 65 rows on row 5 is all missing, row 6 all homozygous
    and row 7 alternates hets"""
    rng = np.random.default_rng(100 + N)
    g = rng.binomial(2, rng.uniform(0.05, 0.5, size=MTOT)[:, None], size=(MTOT, N)).astype(np.uint8)
    g[rng.random((MTOT, N)) < 0.02] = 3
    run_off, idx, _ = selection(W)
    rows = np.arange(N)
    pos = np.arange(700)[:, None]
    start = 60 + 7 * (rows % 5)[None, :]
    plant = (pos >= start) & (pos < start + 500)
    blk = g[idx[run_off[-2]:run_off[-1]]]
    blk[plant & ((blk == 1) | (blk == 3))] = 0
    g[idx[run_off[-2]:run_off[-1]]] = blk
    blk = g[idx[run_off[-3]:run_off[-2]]]
    blk[:, rows % 3 == 0] = np.where(np.isin(blk[:, rows % 3 == 0], (1, 3)), 2, blk[:, rows % 3 == 0])
    g[idx[run_off[-3]:run_off[-2]]] = blk
    if N >= 65:
        g[:, 5] = 3
        g[:, 6] = 0
        g[:, 7] = 1
        g[idx, 7] = np.arange(len(idx)) % 2  # (by position in the selection: a hole must not put two alike side by side)
    return g


_cache = {}


def cohort(N, W):
    """one device and one set of genotypes per (N, W), shared by the cases.  A cohort has two rows at least, so the handle of one row
    holds the first of two."""
    if (N, W) not in _cache:
        g = genotypes(max(N, 2), W)
        dev = capi.Device(0)
        dev.load_bed(synth.pack_bed_columns(g), g.shape[1], row_begin=0, row_end=N, n_global=g.shape[1])
        assert dev.n_local == N
        _cache[(N, W)] = (dev, g[:, :N])
    return _cache[(N, W)]


def as_list(segs):
    return [tuple(int(v) for v in s) for s in segs.tolist()]


def compare(N, W, must_cross=True, **kw):
    dev, g = cohort(N, W)
    run_off, idx, bp = selection(W)
    kw = dict(dict(window=W, min_snps=20, min_bp=20000, dens_bp=1650, gap_bp=40000), **kw)
    want = rr.segments(g, run_off, idx, bp, **kw)
    if must_cross:  # 65 markers and more lie across a boundary of any grid of 64
        assert any(s[3] >= 65 for s in want), "no segment crosses a 64-marker block boundary: the case checks nothing"
    got = dev.roh(run_off, idx, bp, **kw)
    assert got.dtype == capi.ROH_SEG
    assert all(s[0] < N for s in as_list(got)), "a segment for a row past N"
    assert as_list(got) == want
    return dev, got, want


GRID = [(W, h, m, th) for W in WS for h in (0, 1, 3) for m in (0, 5) for th in (0.05, 0.5, 1.0)]


@pytest.mark.parametrize("i", range(len(GRID)), ids=["N%d-W%d-h%d-m%d-t%g" % ((NS[i % 6],) + GRID[i]) for i in range(len(GRID))])
def test_grid(i):
    """every (W, h, m, threshold) once, the row counts in turn (each N meets each W three times); max_het given in every other case"""
    W, h, m, th = GRID[i]
    compare(NS[i % 6], W, window_het=h, window_missing=m, threshold=th, max_het=2 if i % 2 else None)


@pytest.mark.parametrize("N", NS)
def test_rows(N):
    """every row count at PLINK's window, with small thresholds (many short segments) and with filters only the planted stretches pass"""
    dev, got, want = compare(N, 50, window_het=1, window_missing=5, threshold=0.05, min_snps=2, min_bp=0, dens_bp=10**9)
    assert len(want) > N
    compare(N, 50, window_het=1, window_missing=5, threshold=0.05, min_snps=100, min_bp=100000, dens_bp=3000)


def test_each_filter_binds_and_the_gap_cuts():
    N, W = 257, 8
    _, g = cohort(N, W)
    run_off, idx, bp = selection(W)
    base = dict(window=W, window_het=1, window_missing=1, threshold=0.05, min_snps=1, min_bp=0, dens_bp=10**12, gap_bp=40000, max_het=None)
    loose = rr.segments(g, run_off, idx, bp, **base)
    for name, value in [("min_snps", 12), ("min_bp", 15000), ("dens_bp", 1600), ("max_het", 0)]:
        kw = dict(base, **{name: value})
        want = rr.segments(g, run_off, idx, bp, **kw)
        assert 0 < len(want) < len(loose), name + " does not bind"
        compare(N, W, **kw)
    # the planted stretch of every row is cut where the bp jumps; without the gap it is one segment
    cutpos = int(run_off[-2]) + GAP_AT
    assert sum(s[2] == cutpos - 1 for s in loose) >= N - 3 and sum(s[1] == cutpos for s in loose) >= N - 3
    _, _, uncut = compare(N, W, **dict(base, gap_bp=10**12))
    assert len(uncut) < len(loose) and not any(s[2] == cutpos - 1 or s[1] == cutpos for s in uncut if s[0] not in (5, 7))
    # a segment whose length equals the limits passes: len >= min_bp and len <= dens_bp n are not strict
    s = max(loose, key=lambda x: x[3])
    ln = int(bp[s[2]] - bp[s[1]])
    assert ln % s[3], "pick a segment whose length is no multiple of its markers"
    for kw in (dict(base, min_bp=ln, min_snps=s[3]), dict(base, min_bp=ln + 1, min_snps=s[3]), dict(base, dens_bp=ln // s[3] + 1, min_snps=s[3]),
               dict(base, dens_bp=ln // s[3], min_snps=s[3])):
        compare(N, W, must_cross=False, **kw)


def test_special_rows():
    """all missing, all homozygous and alternating hets, with filters that keep everything"""
    N = 65
    for W, h, m, missing_row, alternating_row in [(2, 0, 5, True, False), (8, 0, 5, False, False), (8, 3, 0, False, False), (2, 1, 0, False, True),
                                                  (64, 32, 64, True, True), (1, 0, 0, False, False)]:
        run_off, idx, bp = selection(W)
        _, got, want = compare(N, W, window_het=h, window_missing=m, threshold=1.0, min_snps=1, min_bp=0, dens_bp=10**12, gap_bp=10**12)
        whole = [(int(run_off[r]), int(run_off[r + 1]) - 1) for r in range(len(run_off) - 1) if run_off[r + 1] - run_off[r] >= W]
        assert len(whole) == (6 if W == 64 else 7), "the run of W - 1 markers has no window (nor have the two of 63 at W = 64)"
        by_row = {r: [(s[1], s[2]) for s in want if s[0] == r] for r in (5, 6, 7)}
        assert by_row[5] == (whole if missing_row else []), "all missing: covered everywhere with m >= W, nowhere with m < W"
        assert by_row[6] == whole, "all homozygous: every run from end to end"
        if W == 1 and h == 0:
            assert all(b - a == 0 for a, b in by_row[7]) and by_row[7], "W = 1: the homozygous markers one by one"
        else:
            assert by_row[7] == (whole if alternating_row else []), "alternating hets: every window holds W / 2 of them"
        for s in want:
            if s[0] == 5:
                assert s[5] == s[3] and s[4] == 0


def test_second_run_and_repeat():
    """a first capacity of 4 sends the call through its second run: the same list; a repeat gives the same bytes"""
    N, W = 65, 8
    kw = dict(window_het=0, window_missing=1, threshold=0.05, min_snps=10, min_bp=5000, dens_bp=3000)
    dev, got, want = compare(N, W, **kw)
    assert len(want) > 40
    dev.set_option("roh_list0", 4)
    try:
        _, small, _ = compare(N, W, **kw)
        assert small.tobytes() == got.tobytes()
        assert dev.last_roh_ms() > 0.0
    finally:
        dev.set_option("roh_list0", 0)
    _, again, _ = compare(N, W, **kw)
    assert again.tobytes() == got.tobytes()
    with pytest.raises(capi.HgError, match="roh_list0"):
        dev.set_option("roh_list0", -1)


def test_empty_cases():
    N, W = 15, 50
    dev, g = cohort(N, W)
    run_off, idx, bp = selection(W)
    assert len(dev.roh([0], [], [])) == 0
    assert len(dev.roh([0, 0, 0], [], [])) == 0
    short = dev.roh([0, W - 1], idx[:W - 1], bp[:W - 1], window=W, min_snps=1, min_bp=0, dens_bp=10**9, window_het=W)
    assert len(short) == 0 and rr.segments(g, [0, W - 1], idx, bp, window=W, min_snps=1, min_bp=0, dens_bp=10**9, window_het=W) == []
    exact = dev.roh([0, W], idx[:W], bp[:W], window=W, min_snps=1, min_bp=0, dens_bp=10**9, window_het=W)
    assert len(exact) == N and as_list(exact) == rr.segments(g, [0, W], idx, bp, window=W, min_snps=1, min_bp=0, dens_bp=10**9, window_het=W)


def test_refusals():
    N, W = 65, 8
    dev, g = cohort(N, W)
    run_off, idx, bp = selection(W)
    good = dict(window=W, window_het=0, window_missing=1, threshold=0.05, min_snps=10, min_bp=5000, dens_bp=3000, gap_bp=40000)
    before = dev.roh(run_off, idx, bp, **good)
    assert len(before)

    def refused(msg, run_off=run_off, idx=idx, bp=bp, **kw):
        with pytest.raises(capi.HgError, match=msg):
            dev.roh(run_off, idx, bp, **dict(good, **kw))
        assert dev.last_roh_ms() == 0.0
        kept = np.zeros(len(before), dtype=capi.ROH_SEG)  # the previous list is left alone
        capi.check(dev.L.hgibbs_roh_get(dev.h, kept.ctypes.data))
        assert kept.tobytes() == before.tobytes()

    refused(r"hgibbs_roh: window = 0, needs 1 to 64 markers", window=0, need=[1] * 65)
    refused(r"hgibbs_roh: window = 65, needs 1 to 64 markers", window=65, need=[1] * 65)
    need = rr.need_table(0.05, W)
    refused(r"hgibbs_roh: need\[3\] = 0, needs 1 to 3", need=need[:3] + [0] + need[4:])
    refused(r"hgibbs_roh: need\[3\] = 4, needs 1 to 3", need=need[:3] + [4] + need[4:])
    bad = idx.copy()
    bad[100] = MTOT
    refused(r"hgibbs_roh: entry 100 is marker 1500, the handle has 1500", idx=bad)
    bad = idx.copy()
    bad[101] = bad[100]
    refused(r"hgibbs_roh: idx is not ascending within run", idx=bad)
    down = bp.copy()
    down[200] = down[199] - 1
    refused(r"hgibbs_roh: bp decreases within run", bp=down)
    for name in ("min_bp", "dens_bp", "gap_bp"):
        refused(r"hgibbs_roh: negative limit", **{name: -1})
    # idx and bp may step down from one run to the next
    k = int(run_off[3])
    two = dev.roh([0, run_off[-1] - k, run_off[-1]], np.concatenate([idx[k:], idx[:k]]), np.concatenate([bp[k:], bp[:k]]), **good)
    assert as_list(two) == rr.segments(g, [0, int(run_off[-1]) - k, int(run_off[-1])], np.concatenate([idx[k:], idx[:k]]), np.concatenate([bp[k:], bp[:k]]), **good)

    p, n = capi.RohParams(), capi.C.c_uint64()
    with pytest.raises(capi.HgError, match="hgibbs_roh: null argument"):
        capi.check(dev.L.hgibbs_roh(dev.h, 1, None, None, None, capi.C.byref(p), capi.C.byref(n)))
    ro = (capi.C.c_uint32 * 2)(0, 5)
    with pytest.raises(capi.HgError, match="hgibbs_roh: null argument"):
        capi.check(dev.L.hgibbs_roh(dev.h, 1, ro, None, None, None, capi.C.byref(n)))
    p.window, p.need[1] = 1, 1
    with pytest.raises(capi.HgError, match="hgibbs_roh: null argument"):
        capi.check(dev.L.hgibbs_roh(dev.h, 1, ro, None, None, capi.C.byref(p), capi.C.byref(n)))
    with pytest.raises(capi.HgError, match="hgibbs_last_roh_ms: null argument"):
        capi.check(dev.L.hgibbs_last_roh_ms(dev.h, None))
    empty = capi.Device(0)
    with pytest.raises(capi.HgError, match="hgibbs_roh: no genotypes loaded on this handle"):
        empty.roh(run_off, idx, bp, **good)


def test_several_ranks_refused():
    N = 400

    def allreduce(arr):  # a stub world of two identical ranks
        arr *= 2

    g = genotypes(N, 8)
    dev = capi.Device(0)
    dev.comm_init_external(2, 0, allreduce)
    dev.load_bed(synth.pack_bed_columns(g), N, row_begin=0, row_end=N // 2, n_global=N)
    run_off, idx, bp = selection(8)
    with pytest.raises(capi.HgError, match=r"hgibbs_roh: one rank only \(this handle has 2\)"):
        dev.roh(run_off, idx, bp, window=8)
    assert dev.last_roh_ms() == 0.0
