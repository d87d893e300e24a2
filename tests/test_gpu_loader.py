"""The front door: hgibbs_load_bed and hgibbs_synth_bed against tests/loader_restate.py, a numpy restatement of the image they promise
(itself held to the CPU oracle on these same grids by tests/test_loader_restatement_cpu.py).

Every kernel trusts two properties of the image: slots at local index >= n_local hold the missing code, and row i of the image is
kept row row_begin + i of the file.  Every handle loaded here is read back through three consumers that fail differently when one of
them is broken: hgibbs_get_bed (the bytes), hgibbs_marker_stats (column sums: padding counted as rows shifts them) and the sparse
readers (row indices: padding listed, or rows out of order).  No tolerance anywhere: bytes, integers and float64 bit patterns.

What the files hold where nobody should look is what a real PLINK file holds there: 00 in the unused slots of a column's last byte
(a called genotype), the next rank's rows behind a shard's end, and anything at all in the bytes of a padded row.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import loader_restate as R
from hydra_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")

pytestmark = pytest.mark.gpu

M_WIDE = 70000  # above 65535, the limit of a launch's second grid dimension


def check(dev, want, n_global, world_counts=None):
    """The handle's image is `want` (the restatement's bytes), to all three consumers.  world_counts: the (n1, n2, nm) that a stub
    world of ranks makes of this handle's own counts; the sparse readers refuse several ranks, so the lists are then left out."""
    n = dev.n_local
    assert want.shape == (dev.M, (n + 3) // 4) and dev.n_global == n_global
    assert np.array_equal(dev.get_bed(), want)
    own = R.counts(want, n)
    n1, n2, nm = own if world_counts is None else world_counts
    mave, mstd, g1, g2, gm = dev.marker_stats()
    for got, ref, what in ((g1, n1, "n1"), (g2, n2, "n2"), (gm, nm, "nmiss")):
        assert np.array_equal(got.astype(np.int64), ref), what
    wa, ws = R.stats(n1, n2, nm, n_global)
    assert R.same_bits(mave, wa) and R.same_bits(mstd, ws)
    if world_counts is not None:
        return
    ls = R.lists(want, n)
    for got, c in zip(dev.sparse_counts(), "12m"):
        assert np.array_equal(got, ls["sl" + c]), c
    for got, c in zip(dev.sparse_get(), "12m"):
        assert np.array_equal(got, ls["si" + c]), c


def load_and_check(file, n_total, keep=None, row_begin=0, row_end=None, want=None):
    """load on a fresh handle, hold it to the restatement of the same arguments (or to `want`, where the point is that another
    file gives the same image), and return the bytes"""
    nk = n_total if keep is None else int(np.count_nonzero(keep))
    n_global = max(nk, 2)
    if want is None:
        want = R.image(file, n_total, keep=keep, row_begin=row_begin, row_end=row_end)
    dev = capi.Device(0)
    try:
        dev.load_bed(file, n_total, keep=keep, row_begin=row_begin, row_end=row_end, n_global=n_global)
        assert (dev.n_local, dev.row_begin) == ((nk if row_end is None else row_end) - row_begin, row_begin)
        check(dev, want, n_global)
    finally:
        dev.close()
    return want


# ---------------------------------------------------------------------------------------------------------------------------------
# what lies beyond the rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [N for N in R.NS if N % 4])
def test_tail_bits_are_ignored(N):
    """the same genotypes with 00 (PLINK's), 01, 10, 11 and random bits in the unused slots of every column's last byte: one image"""
    want = R.image(R.case_bed(N, fill=0b01), N)
    for fill in R.FILLS:
        load_and_check(R.case_bed(N, fill=fill), N, want=want)


@pytest.mark.parametrize("N", R.NS)
def test_padded_rows(N):
    """stride_in wider than ceil(N/4), odd and no dword multiple, the spare bytes random: the same image without a keep list (the
    pitch of the 2-D copy) and with one (src_stride of k_compact_bed)"""
    bed = R.case_bed(N)
    keep = R.keep_mask("run", N)
    want, want_k = R.image(bed, N), R.image(bed, N, keep=keep)
    for extra in R.EXTRAS:
        wide = R.widen(bed, extra, seed=extra)
        assert wide.shape[1] == (N + 3) // 4 + extra
        load_and_check(wide, N, want=want)
        load_and_check(wide, N, keep=keep, want=want_k)


@pytest.mark.parametrize("N", R.NS)
def test_shards_without_a_keep_list(N):
    """row_begin at multiples of 4, n_local % 4 each of 0 .. 3; where the shard ends inside a byte the slots behind it hold the next
    rows' called genotypes, which are not this handle's.  The shards of a cover give the whole file."""
    bed = R.case_bed(N)
    for b, e in R.inside_shards(N):
        load_and_check(R.called_after(bed, N, e), N, row_begin=b, row_end=e)
    parts = [synth.unpack_bed_columns(load_and_check(bed, N, row_begin=b, row_end=e), e - b) for b, e in R.cover(N)]
    assert np.array_equal(np.concatenate(parts, axis=1), synth.unpack_bed_columns(bed, N))


@pytest.mark.parametrize("N", R.NS)
def test_keep_lists(N):
    """each mask over the whole kept range and over shards whose row_begin is 1, 2, 3 mod 4 and whose row_end is below the number
    kept, from a file with PLINK's tail and one with random bits there; an all-ones mask is no mask"""
    for fill in (0b00, None):
        bed = R.case_bed(N, fill=fill)
        for name in R.MASKS:
            keep = R.keep_mask(name, N)
            whole = load_and_check(bed, N, keep=keep)
            if name == "all":
                assert np.array_equal(whole, load_and_check(bed, N))
            for b, e in R.keep_shards(int(keep.sum())):
                load_and_check(bed, N, keep=keep, row_begin=b, row_end=e)


# ---------------------------------------------------------------------------------------------------------------------------------
# counts summed over ranks
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (7, 65, 4097))
def test_counts_over_a_stub_world(N):
    """two ranks, the other one a stub that adds its rows' counts (the restatement's) to the buffer it is handed: rank 0 holds
    [0, cut) without a keep list and ends inside a byte, rank 1 holds [cut, N) through an all-ones mask; both must report the
    whole file's counts, and mave / mstd of those at n_global = N."""
    cut = 4 * (N // 8) + 1
    bed = R.called_after(R.case_bed(N), N, cut)
    Mn = bed.shape[0]
    world = R.counts(R.image(bed, N), N)
    for rank, kw in ((0, dict(row_begin=0, row_end=cut)), (1, dict(keep=np.ones(N, dtype=np.uint8), row_begin=cut, row_end=N))):
        b, e = (cut, N) if rank == 0 else (0, cut)
        other = np.stack(R.counts(R.image(bed, N, row_begin=b, row_end=e, keep=np.ones(N, dtype=np.uint8)), e - b), axis=1).reshape(-1)
        calls = []

        def allreduce(arr):
            assert arr.dtype == np.uint64 and arr.size == 3 * Mn
            calls.append(arr.copy())
            arr += other.astype(np.uint64)

        dev = capi.Device(0)
        dev.comm_init_external(2, rank, allreduce)
        dev.load_bed(bed, N, n_global=N, **kw)
        want = R.image(bed, N, keep=kw.get("keep"), row_begin=kw["row_begin"], row_end=kw["row_end"])
        check(dev, want, N, world_counts=world)
        # what went into the exchange is this rank's own counts, marker-major (n1, n2, nmiss)
        assert len(calls) == 1 and np.array_equal(calls[0].astype(np.int64), np.stack(R.counts(want, dev.n_local), axis=1).reshape(-1))
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# hgibbs_get_bed itself
# ---------------------------------------------------------------------------------------------------------------------------------
def test_get_bed_ranges_stride_and_refusals():
    N, Mn = 17, 9
    bed = R.case_bed(N)
    want = R.image(bed, N)
    dev = capi.Device(0)
    dev.load_bed(bed, N)
    for m0, mc in ((0, 1), (Mn - 1, 1), (3, 4), (0, Mn)):
        assert np.array_equal(dev.get_bed(m0, mc), want[m0:m0 + mc]), (m0, mc)
    width = (N + 3) // 4
    for stride in (width + 1, width + 11):
        out = np.full((4, stride), 0xA5, dtype=np.uint8)
        capi.check(dev.L.hgibbs_get_bed(dev.h, 3, 4, out.ctypes.data_as(C.POINTER(C.c_uint8)), stride))
        assert np.array_equal(out[:, :width], want[3:7]) and np.all(out[:, width:] == 0xA5)
    out = np.zeros((Mn, width), dtype=np.uint8)
    ptr = out.ctypes.data_as(C.POINTER(C.c_uint8))
    for (m0, mc, stride), msg in (((0, Mn + 1, width), "marker range out of bounds"), ((Mn, 1, width), "marker range out of bounds"),
                                  ((0xFFFFFFFF, 2, width), "marker range out of bounds"), ((0, Mn, width - 1), "out_stride too small")):
        with pytest.raises(capi.HgError, match="hgibbs_get_bed: " + msg):
            capi.check(dev.L.hgibbs_get_bed(dev.h, m0, mc, ptr, stride))
    assert not out.any()
    dev.close()
    empty = capi.Device(0)
    with pytest.raises(capi.HgError, match="hgibbs_get_bed: no data"):
        capi.check(empty.L.hgibbs_get_bed(empty.h, 0, 1, ptr, width))
    empty.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# more markers than a launch's second grid dimension
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_file():
    return R.case_bed(5, M=M_WIDE, seed=3)


@pytest.mark.parametrize("drop", (True, False))
def test_wide_file(drop):
    """M = 70000 columns of 5 rows, through a keep list that drops one row (k_compact_bed, one launch row per marker) and without
    one: the bytes and the counts of every marker, the last one included.  (The lists at this width are test_gpu_sparse's test_wide.)"""
    N, bed = 5, wide_file()
    keep = None
    if drop:
        keep = np.ones(N, dtype=np.uint8)
        keep[2] = 0
    want = R.image(bed, N, keep=keep)
    n = N - int(drop)
    dev = capi.Device(0)
    dev.load_bed(bed, N, keep=keep)
    assert (dev.M, dev.n_local) == (M_WIDE, n)
    assert np.array_equal(dev.get_bed(), want)
    _, _, g1, g2, gm = dev.marker_stats()
    for got, ref in zip((g1, g2, gm), R.counts(want, n)):
        assert np.array_equal(got.astype(np.int64), ref)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# hgibbs_synth_bed
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synth_whole(N, M, rate):
    return synth.synth_bed_reference(N, M, seed=42, missing_rate=rate)


def synth_and_check(N, M, want, rate=0.01, **kw):
    dev = capi.Device(0)
    try:
        dev.synth_bed(N, M, seed=42, missing_rate=rate, **kw)
        check(dev, want, N)  # (the bytes equal the restatement's, whose unused slots are all missing)
    finally:
        dev.close()


def test_synth_second_slab_of_markers():
    """M = 32768 + 3: the markers of the second launch are markers 32768 .., not 0 .. again"""
    N, M = 5, 32768 + 3
    want = synth_whole(N, M, 0.01)
    assert not np.array_equal(want[32768:], want[:3])
    dev = capi.Device(0)
    dev.synth_bed(N, M, seed=42, missing_rate=0.01)
    assert np.array_equal(dev.get_bed(), want)
    _, _, g1, g2, gm = dev.marker_stats()
    for got, ref in zip((g1, g2, gm), R.counts(want, N)):
        assert np.array_equal(got.astype(np.int64), ref)
    dev.close()


@pytest.mark.parametrize("row_begin", (1, 2, 3, 501))
def test_synth_shards_are_rows_of_the_whole(row_begin):
    N, M = 1003, 17
    whole = synth_whole(N, M, 0.01)
    ones = np.ones(N, dtype=np.uint8)
    for row_end in (N, N - 2, row_begin + 1):
        synth_and_check(N, M, R.image(whole, N, keep=ones, row_begin=row_begin, row_end=row_end), row_begin=row_begin, row_end=row_end)


@pytest.mark.parametrize("rate,all_missing", ((-1.0, False), (0.0, False), (1.0, True), (2.0, True)))
def test_synth_missing_rate_is_clamped(rate, all_missing):
    N, M = 37, 5
    want = synth_whole(N, M, rate)
    g = synth.unpack_bed_columns(want, N)
    assert np.all(g == 3) if all_missing else not np.any(g == 3)
    synth_and_check(N, M, want, rate=rate)


def test_synth_refusals_then_a_good_load():
    N, M = 37, 5
    want = synth_whole(N, M, 0.01)
    for kw, msg in ((dict(row_begin=4, row_end=4), "hgibbs_synth_bed: bad row range"), (dict(row_begin=8, row_end=4), "hgibbs_synth_bed: bad row range"),
                    (dict(row_end=N + 1), "hgibbs_synth_bed: bad row range"), (dict(M=0), "empty problem")):
        dev = capi.Device(0)
        with pytest.raises(capi.HgError, match=msg):
            dev.synth_bed(N, kw.pop("M", M), seed=42, missing_rate=0.01, **kw)
        dev.synth_bed(N, M, seed=42, missing_rate=0.01)
        check(dev, want, N)
        for again in (lambda: dev.synth_bed(N, M, seed=1), lambda: dev.load_bed(want, N)):
            with pytest.raises(capi.HgError, match="data already loaded on this handle"):
                again()
        check(dev, want, N)
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals leave the handle as it was
# ---------------------------------------------------------------------------------------------------------------------------------
def raw_load(dev, bed, stride, n_total, M, keep, row_begin, row_end, n_global):
    u8 = C.POINTER(C.c_uint8)
    capi.check(dev.L.hgibbs_load_bed(dev.h, bed.ctypes.data_as(u8) if bed is not None else None, stride, n_total, M,
                                     keep.ctypes.data_as(u8) if keep is not None else None, row_begin, row_end, n_global))


def test_load_refusals_then_a_good_load():
    """hgibbs_load_bed validates before anything is allocated on the handle: after each refusal the same handle takes a good load"""
    N, Mn = 17, 9
    bed = R.case_bed(N, fill=None)
    width = (N + 3) // 4
    keep = R.keep_mask("run", N)
    nk = int(keep.sum())
    want, want_k = R.image(bed, N), R.image(bed, N, keep=keep)
    cases = (
        ((None, width, N, Mn, None, 0, N, N), "hgibbs_load_bed: null argument"),
        ((bed, width, N, Mn, None, 8, 8, N), "hgibbs_load_bed: empty row range"),
        ((bed, width, N, Mn, None, 12, 8, N), "hgibbs_load_bed: empty row range"),
        ((bed, width - 1, N, Mn, None, 0, N, N), r"hgibbs_load_bed: stride_in 4 < ceil\(17/4\)"),
        ((bed, width, N, Mn, None, 0, N + 1, N), "hgibbs_load_bed: row_end 18 > n_total 17"),
        ((bed, width, N, Mn, None, 2, N, N), "hgibbs_load_bed: row_begin 2 must be a multiple of 4"),
        ((bed, width, N, Mn, keep, 0, nk + 1, nk), "hgibbs_load_bed: row_end %d > kept individuals %d" % (nk + 1, nk)),
        ((bed, width, N, Mn, None, 0, N, 1), "hgibbs_load_bed: n_global must be at least 2"),
        ((bed, width, N, Mn, keep, 1, nk, 0), "hgibbs_load_bed: n_global must be at least 2"),
        ((bed, width, N, 0, None, 0, N, N), "empty problem: n_local=17 M=0"),
    )
    for k, (args, msg) in enumerate(cases):
        dev = capi.Device(0)
        with pytest.raises(capi.HgError, match=msg):
            raw_load(dev, *args)
        for call in (dev.get_bed, dev.marker_stats):  # nothing is on the handle
            with pytest.raises(capi.HgError, match="no data"):
                call()
        if k % 2:
            dev.load_bed(bed, N, keep=keep)
            check(dev, want_k, nk)
        else:
            dev.load_bed(bed, N)
            check(dev, want, N)
        # a second load on a loaded handle, by either path, is refused and changes nothing
        for kw in (dict(), dict(keep=keep)):
            with pytest.raises(capi.HgError, match="data already loaded on this handle"):
                dev.load_bed(R.case_bed(N, seed=1), N, **kw)
        check(dev, want_k if k % 2 else want, nk if k % 2 else N)
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# through the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_qc_does_not_read_the_tail(tmp_path):
    """--qc on two .bed files that differ only in the unused slots of each column's last byte, 01 as write_plink packs them and 00 as
    PLINK writes them, N % 4 == 1 and a few NA phenotypes: every output file is the same, byte for byte"""
    N, M = 101, 40
    y = np.random.default_rng(4).standard_normal(N)
    outs = []
    for fill in (0b01, 0b00):
        d = tmp_path / ("fill%d" % fill)
        d.mkdir()
        bed = R.case_bed(N, M=M, seed=9, fill=fill)
        synth.write_plink(str(d / "x"), bed, N, y=y, na_rows=[0, 50, 99, 100])
        r = subprocess.run([EXE, "--mpibayes", "bayesMPI", "--bfile", "x", "--pheno", "x.phen", "--mcmc-out-dir", "o", "--mcmc-out-name", "n",
                            "--number-individuals", str(N), "--number-markers", str(M), "--qc", "--qc-out", "q",
                            "--qc-maf", "0.05", "--qc-geno", "0.1", "--qc-mind", "0.1", "--qc-hwe", "1e-4", "--qc-het-sd", "2.0"],
                           capture_output=True, text=True, timeout=120, cwd=str(d))
        assert r.returncode == 0, r.stderr
        files = {}
        for base, _, names in os.walk(str(d)):
            for name in names:
                p = os.path.join(base, name)
                if os.path.relpath(p, str(d)) not in ("x.bed", "x.bim", "x.fam", "x.phen"):
                    files[os.path.relpath(p, str(d))] = open(p, "rb").read()
        outs.append((bed, files))
    (bed1, f1), (bed0, f0) = outs
    tail = bed1[:, -1] >> 2
    assert np.all(tail == 0b010101) and np.all(bed0[:, -1] >> 2 == 0) and np.array_equal(bed1[:, :-1], bed0[:, :-1])
    assert len(f1) >= 8 and sorted(f1) == sorted(f0) and all(len(v) > 0 for v in f1.values())
    for name in f1:
        assert f1[name] == f0[name], name
