"""hgibbs_row_sums (Device.row_sums) against its restatement in integers (tests/rowsums_restate.py): bit for bit over a grid of shapes
at the boundaries of the kernel's tiles, for the seven QC tables, random tables, an all-zero table, a table with entries only at
code 3 and a table of the integers at which signed base-256 digits carry; bit identity across ranges, repeats and T; the refusals."""
import functools

import numpy as np
import pytest

import rowsums_restate as rr
from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu

NS = [1, 5, 63, 64, 65, 255, 257]                 # the dword of sixteen individuals, the wave, the workgroup of 256 rows
MS = [1, 15, 16, 17, 63, 64, 65, 130, 1031]       # the group of sixteen markers, the block of 64
BIG = (4097, 1031)                                # the padding to 4096


def make(N, M, seed):
    """tests/test_gpu_grm.py's recipe (one individual alone: plain random genotypes, synth's recipe needs two)"""
    if N >= 2:
        geno = synth.make_genotypes(M, N, seed=seed)
    else:
        geno = np.random.default_rng(seed).integers(0, 3, size=(M, N)).astype(np.uint8)
    rng = np.random.default_rng(seed + 7)
    for j in rng.choice(M, size=max(1, M // 5), replace=False):  # 1-5 % missing calls in a fifth of the columns
        geno[j, rng.random(N) < rng.uniform(0.01, 0.05)] = 3
    if M >= 3:
        geno[M // 3] = 3  # a marker missing everywhere
        geno[M // 2] = 1 if M % 2 else 0  # a monomorphic marker
    if M >= 5:
        geno[M - 2] = 2
    if N >= 3:
        geno[:, N // 2] = 3  # an individual missing everywhere
    if N >= 6:
        geno[:, 1] = geno[:, N - 1]  # a duplicate
    return geno


def device(geno):
    M, N = geno.shape
    dev = capi.Device(0)
    if N == 1:  # (a file holds two individuals at least: the handle takes the first as its one row)
        dev.load_bed(synth.pack_bed_columns(np.concatenate([geno, geno], axis=1)), 2, row_end=1, n_global=2)
        assert dev.n_local == 1
    else:
        dev.load_bed(synth.pack_bed_columns(geno), N)
    return dev


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def boundary_table(M, rng):
    """Entries ldexp(q, -E) for chosen integers q, where signed base-256 digits carry; one entry just below 2^e fixes E = 52 - e."""
    e = 3
    E = 52 - e
    top = (1 << 52) - 1
    qs = [top, -top, 1 << 51, -(1 << 51), 0x0F7F7F7F7F7F7F, -0x0F7F7F7F7F7F7F, 0x0F808080808080, -0x0F808080808080]
    for d in range(7):  # +-127 / -+128 in single digits
        qs += [127 << (8 * d), -(127 << (8 * d)), 128 << (8 * d), -(128 << (8 * d))]
    qs = [q for q in qs if abs(q) <= top]
    pick = rng.integers(0, len(qs), size=(M, 4))
    tab = np.array([[np.ldexp(float(qs[k]), -E) for k in row] for row in pick])
    tab[0, 0] = np.ldexp(float(top), -E)  # just below 2^e
    assert rr.scale(tab) == E
    return tab


def tables(codes, seed):
    """sixteen tables: 0 .. 6 the QC tables, 7 .. 11 random normal at several scales, 12 all zero, 13 entries only at code 3,
    14 the digit boundaries, 15 random again"""
    N, M = codes.shape
    rng = np.random.default_rng(seed)
    tab = np.zeros((16, M, 4))
    tab[:7] = rr.qc_tables(codes, rr.polymorphic(codes))
    for k, s in enumerate([1.0, 1e-7, 3e11, 2.0 ** -40, 1000.0]):
        tab[7 + k] = rng.standard_normal((M, 4)) * s
    tab[13, :, 3] = rng.standard_normal(M)
    tab[14] = boundary_table(M, rng)
    tab[15] = rng.standard_normal((M, 4))
    return tab


@functools.lru_cache(maxsize=2)
def case(N, M):
    geno = make(N, M, seed=N * 7 + M)
    codes = rr.codes_of(geno)
    tab = tables(codes, seed=N + M)
    want = rr.row_sums_split(codes, tab)
    want.setflags(write=False)
    return geno, tab, want


def check_case(N, M, singles):
    geno, tab, want = case(N, M)
    dev = device(geno)
    got16 = dev.row_sums(tab)
    assert got16.shape == (N, 16)
    assert np.array_equal(bits(got16), bits(want))
    assert np.array_equal(bits(dev.row_sums(tab)), bits(want))                      # a repeat
    assert np.array_equal(bits(dev.row_sums(tab[:7])), bits(want[:, :7]))           # T = 7: the QC tables
    assert np.array_equal(bits(dev.row_sums(tab[[14, 9]])), bits(want[:, [14, 9]]))  # T = 2
    for t in singles:                                                               # T = 1: column t of the call with sixteen
        assert np.array_equal(bits(dev.row_sums(tab[t:t + 1])[:, 0]), bits(want[:, t])), t
    return dev, tab, want


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NS)
def test_bit_exact_against_the_restatement(N, M):
    check_case(N, M, singles=range(16) if M <= 130 else [3, 12, 13, 14])


def test_bit_exact_past_the_padding_and_across_ranges():
    N, M = BIG
    dev, tab, want = check_case(N, M, singles=[4, 14])
    for ranges in (0, 1, 3, 7):
        dev.set_option("rowsums_ranges", ranges)
        assert np.array_equal(bits(dev.row_sums(tab)), bits(want)), ranges
        assert dev.last_row_sums_ms() > 0.0


@pytest.mark.parametrize("N", [65, 257])
def test_ranges_give_identical_bits(N):
    geno, tab, want = case(N, 1031)
    dev = device(geno)
    for ranges in (0, 1, 3, 7):
        dev.set_option("rowsums_ranges", ranges)
        assert np.array_equal(bits(dev.row_sums(tab)), bits(want)), ranges
        assert np.array_equal(bits(dev.row_sums(tab[:7])), bits(want[:, :7])), ranges


def test_exact_counts():
    N, M = 257, 130
    geno = make(N, M, seed=5)
    codes = rr.codes_of(geno)
    tab = np.zeros((2, M, 4))
    tab[0, :, 3] = 1.0
    tab[1, :, 1] = 1.0
    got = device(geno).row_sums(tab)
    assert np.array_equal(got[:, 0], (codes == 3).sum(1)) and np.array_equal(got[:, 1], (codes == 1).sum(1))


def test_refusals():
    N, M = 65, 17
    geno, tab, want = case(N, M)
    dev = device(geno)

    def still_serves():
        mave, mstd, n1, n2, nm = dev.marker_stats()
        assert np.array_equal(nm, (geno == 3).sum(1).astype(np.uint64))
        assert np.array_equal(bits(dev.row_sums(tab[:2])), bits(want[:, :2]))
        assert dev.last_row_sums_ms() > 0.0

    for T, msg in ((0, "T = 0"), (17, "T = 17")):
        with pytest.raises(capi.HgError, match=msg):
            dev.row_sums(np.zeros((T, M, 4)))
        assert dev.last_row_sums_ms() == 0.0
        still_serves()
    bad = tab[:3].copy()
    bad[1, M // 2, 2] = np.nan
    with pytest.raises(capi.HgError, match="a table entry is not finite"):
        dev.row_sums(bad)
    assert dev.last_row_sums_ms() == 0.0
    still_serves()
    bad[1, M // 2, 2] = np.inf
    with pytest.raises(capi.HgError, match="a table entry is not finite"):
        dev.row_sums(bad)
    still_serves()
    empty = capi.Device(0)
    empty.M = M
    with pytest.raises(capi.HgError, match="no genotypes loaded"):
        empty.row_sums(tab[:1])
    still_serves()
