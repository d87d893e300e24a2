"""tests/loader_restate.py against the CPU oracle and synth's packers, on the grids tests/test_gpu_loader.py holds the device to: a
restatement that were wrong in the kernel's way would pass there and fail here.  Every comparison is equality of bytes, integers or
float64 bit patterns."""
import ctypes as C

import numpy as np
import pytest

import loader_restate as R
import orc
from hydra_amd import synth


def oracle_compact(L, bed, N, keep):
    """orc_bed_compact of every column: (M, ceil(nk/4))"""
    nk = int(np.count_nonzero(keep))
    out = np.zeros((bed.shape[0], (nk + 3) // 4), dtype=np.uint8)
    for j in range(bed.shape[0]):
        col = np.ascontiguousarray(bed[j, :(N + 3) // 4])
        row = np.zeros((nk + 3) // 4, dtype=np.uint8)
        n_out = C.c_uint32()
        L.orc_bed_compact(orc.u8ptr(col), N, orc.u8ptr(np.ascontiguousarray(keep, dtype=np.uint8)), orc.u8ptr(row), C.byref(n_out))
        assert n_out.value == nk
        out[j] = row
    return out


def oracle_counts(L, img, n):
    out = np.zeros((3, img.shape[0]), dtype=np.int64)
    for j in range(img.shape[0]):
        c = [C.c_uint64() for _ in range(4)]
        L.orc_bed_counts(orc.u8ptr(np.ascontiguousarray(img[j])), n, *[C.byref(x) for x in c])
        assert sum(x.value for x in c) == n
        out[:, j] = [c[1].value, c[2].value, c[3].value]
    return out


def repacked(bed, N, keep, b, e):
    """the same rows through synth's unpack and pack"""
    g = synth.unpack_bed_columns(bed[:, :(N + 3) // 4], N)
    if keep is not None:
        g = g[:, keep != 0]
    return synth.pack_bed_columns(g[:, b:e])


@pytest.mark.parametrize("N", R.NS)
def test_image_is_the_oracles_compaction(oracle, N):
    """every keep mask of the grid over the whole kept range, from a file with random tail bits; an all-ones mask is no mask"""
    bed = R.case_bed(N, fill=None)
    for name in R.MASKS:
        keep = R.keep_mask(name, N)
        assert np.array_equal(R.image(bed, N, keep=keep), oracle_compact(oracle, bed, N, keep)), name
    assert np.array_equal(R.image(bed, N), R.image(bed, N, keep=R.keep_mask("all", N)))
    assert np.array_equal(R.image(bed, N), synth.pack_bed_columns(synth.unpack_bed_columns(bed, N)))


@pytest.mark.parametrize("N", R.NS)
def test_shards_are_slices(N):
    """every shard of the grid, with and without a keep list, equals slicing synth.unpack_bed_columns and repacking; the shards of a
    cover give the whole file"""
    bed = R.case_bed(N, fill=None)
    assert R.cover(N)[0][0] == 0 and R.cover(N)[-1][1] == N and all(b % 4 == 0 for b, _ in R.cover(N))
    assert all(x[1] == y[0] for x, y in zip(R.cover(N)[:-1], R.cover(N)[1:]))
    for b, e in R.cover(N) + R.inside_shards(N):
        file = R.called_after(bed, N, e)
        assert np.array_equal(R.image(file, N, row_begin=b, row_end=e), repacked(file, N, None, b, e)), (b, e)
        after = synth.unpack_bed_columns(file, N)[:, e:min(N, (e + 3) // 4 * 4)]
        assert not np.any(after == 3), (b, e)  # the neighbours in the shard's last byte are called genotypes
    parts = [synth.unpack_bed_columns(R.image(bed, N, row_begin=b, row_end=e), e - b) for b, e in R.cover(N)]
    assert np.array_equal(np.concatenate(parts, axis=1), synth.unpack_bed_columns(bed, N))
    for name in R.MASKS:
        keep = R.keep_mask(name, N)
        for b, e in R.keep_shards(int(keep.sum())):
            assert b % 4 and e < int(keep.sum())
            assert np.array_equal(R.image(bed, N, keep=keep, row_begin=b, row_end=e), repacked(bed, N, keep, b, e)), (name, b, e)


def test_the_grids_reach_what_they_are_for():
    """n_local % 4 takes each of 0 .. 3 without a keep list, row_begin each of 1, 2, 3 mod 4 with one, and [0, 1) of two rows is there"""
    assert (0, 1) in R.inside_shards(2)
    seen = {(e - b) % 4 for N in R.NS for b, e in R.cover(N) + R.inside_shards(N)}
    assert seen == {0, 1, 2, 3}
    for N in R.NS[3:]:
        assert {(e - b) % 4 for b, e in R.inside_shards(N)} == {1, 2, 3}, N
        assert N < 7 or {b % 4 for b, _ in R.keep_shards(N - 1)} == {1, 2, 3}, N


@pytest.mark.parametrize("N", R.NS)
def test_counts_and_stats_are_the_oracles(oracle, N):
    bed = R.case_bed(N, fill=None)
    todo = [(R.image(bed, N), N)]
    keep = R.keep_mask("run", N)
    todo.append((R.image(bed, N, keep=keep), int(keep.sum())))
    todo += [(R.image(bed, N, row_begin=b, row_end=e), e - b) for b, e in R.inside_shards(N)]
    for img, n in todo:
        n1, n2, nm = R.counts(img, n)
        want = oracle_counts(oracle, img, n)
        assert np.array_equal(np.stack([n1, n2, nm]), want), n
        for Ng in (max(n, 2), N + 5):  # as one rank's whole world, and as a share of a larger one
            mave, mstd = R.stats(n1, n2, nm, Ng)
            for j in range(img.shape[0]):
                a, s = C.c_double(), C.c_double()
                oracle.orc_marker_stats(int(n1[j]), int(n2[j]), int(nm[j]), Ng, C.byref(a), C.byref(s))
                assert R.same_bits([mave[j], mstd[j]], [a.value, s.value]), (n, Ng, j)
        ls = R.lists(img, n)
        for c, cnt in zip("12m", (n1, n2, nm)):
            assert np.array_equal(ls["sl" + c], cnt.astype(np.uint64)) and (ls["si" + c].size == 0 or int(ls["si" + c].max()) < n)


@pytest.mark.parametrize("N", R.NS)
def test_image_ignores_what_lies_beyond_the_rows(N):
    """the property the device is then held to: the five tail fills and the widened arrays give the same bytes"""
    base = R.case_bed(N, fill=0b01)
    assert np.array_equal(base, synth.pack_bed_columns(synth.unpack_bed_columns(base, N)))
    keep = R.keep_mask("run", N)
    want, want_k = R.image(base, N), R.image(base, N, keep=keep)
    assert np.array_equal(want, base)
    files = [R.with_tail(base, N, fill) for fill in R.FILLS]
    if N % 4:
        spare = [f[:, -1] >> (2 * (N % 4)) for f in files]
        assert np.all(spare[0] == 0) and not np.array_equal(spare[4], spare[0]) and len({s.tobytes() for s in spare}) == 5
    files += [R.widen(f, extra) for f in (files[0], files[4]) for extra in R.EXTRAS]
    for f in files:
        assert f.shape[1] >= (N + 3) // 4
        assert np.array_equal(R.image(f, N), want) and np.array_equal(R.image(f, N, keep=keep), want_k)
        for b, e in R.inside_shards(N):
            assert np.array_equal(R.image(f, N, row_begin=b, row_end=e), R.image(base, N, row_begin=b, row_end=e))
    assert R.widen(base, 3).shape[1] == base.shape[1] + 3 and np.array_equal(R.widen(base, 3)[:, :base.shape[1]], base)


def test_synth_reference_shards_are_rows_of_the_whole():
    N, M = 1003, 17
    whole = synth.synth_bed_reference(N, M, seed=42, missing_rate=0.01)
    for b, e in ((1, 1003), (2, 999), (3, 14), (501, 1003), (0, 1003)):
        part = synth.synth_bed_reference(N, M, seed=42, missing_rate=0.01, row_begin=b, row_end=e)
        assert np.array_equal(part, R.image(whole, N, keep=np.ones(N, dtype=np.uint8), row_begin=b, row_end=e)), (b, e)
    g = synth.unpack_bed_columns(whole, N)
    assert 0 < np.count_nonzero(g == 3) < 0.03 * g.size
    for rate, all_missing in ((-1.0, False), (0.0, False), (1.0, True), (2.0, True)):
        g = synth.unpack_bed_columns(synth.synth_bed_reference(37, 5, seed=42, missing_rate=rate), 37)
        assert np.all(g == 3) if all_missing else not np.any(g == 3), rate
