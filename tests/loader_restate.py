"""numpy restatement of the packed 2-bit image that hgibbs_load_bed and hgibbs_synth_bed leave on a handle, written from
include/hgibbs.h's words, not from the kernels: which 2-bit fields of the file are read, which rows stay, what the unused slots hold.
Also the grids that tests/test_loader_restatement_cpu.py (reference against the CPU oracle) and tests/test_gpu_loader.py (device
against the reference) share, so that the reference is checked at every shape the device is held to.

A row's field of a column: row i sits in byte i // 4, bits 2 * (i % 4); 0b00 -> genotype 2, 0b10 -> 1, 0b11 -> 0, 0b01 -> missing.
"""
import numpy as np

import sparse_restate

MISSING = 0b01


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _fields(bed, n):
    """the first n 2-bit fields of every row of a (M, >= ceil(n/4)) byte array: (M, n) uint8"""
    bed = np.asarray(bed, dtype=np.uint8)
    assert bed.ndim == 2 and bed.shape[1] >= (n + 3) // 4
    b = bed[:, :(n + 3) // 4]
    f = np.empty((b.shape[0], b.shape[1], 4), dtype=np.uint8)
    for s in range(4):
        f[:, :, s] = (b >> (2 * s)) & 3
    return f.reshape(b.shape[0], -1)[:, :n]


def _pack(f, unused):
    """(M, n) fields -> (M, ceil(n/4)) bytes, the slots beyond n filled with the field `unused` (an (M, 4*ceil(n/4) - n) array or a scalar)"""
    M, n = f.shape
    nb = (n + 3) // 4
    full = np.empty((M, nb * 4), dtype=np.uint8)
    full[:, :n] = f
    full[:, n:] = unused
    full = full.reshape(M, nb, 4)
    return np.ascontiguousarray(full[:, :, 0] | (full[:, :, 1] << 2) | (full[:, :, 2] << 4) | (full[:, :, 3] << 6), dtype=np.uint8)


def image(bed, n_total, keep=None, row_begin=0, row_end=None):
    """What hgibbs_get_bed promises after hgibbs_load_bed(bed, stride_in = bed.shape[1], n_total, keep, row_begin, row_end): the first
    n_total fields of each row, the kept ones of them, rows [row_begin, row_end) of those, every unused slot of the last byte missing.
    Bits beyond n_total and bytes beyond ceil(n_total/4) are never looked at."""
    f = _fields(bed, n_total)
    if keep is not None:
        keep = np.asarray(keep)
        assert keep.shape == (n_total,)
        f = f[:, keep != 0]
    if row_end is None:
        row_end = f.shape[1]
    assert 0 <= row_begin < row_end <= f.shape[1]
    return _pack(f[:, row_begin:row_end], MISSING)


def counts(img, n_local):
    """n1, n2, nmiss of every marker over the image's n_local rows, as Python-int-exact int64 arrays"""
    f = _fields(img, n_local)
    return tuple((f == code).sum(axis=1).astype(np.int64) for code in (0b10, 0b00, MISSING))


def lists(img, n_local):
    """the three ascending row-index lists per marker as sparse_restate.bed_to_lists gives them: sl?/ss?/si? for ? in 1, 2, m"""
    return sparse_restate.bed_to_lists(np.asarray(img, dtype=np.uint8)[:, :(n_local + 3) // 4], n_local)


def stats(n1, n2, nm, N):
    """mave, mstd in float64 with k_stats' operations in k_stats' order (src/BayesRRm.cpp:1502-1507); IEEE division, so a marker
    missing everywhere gives NaN and a monomorphic one an infinite or NaN mstd"""
    n1i, n2i, nmi = (np.asarray(a).astype(np.int64) for a in (n1, n2, nm))
    f = np.float64
    with np.errstate(all="ignore"):
        n0 = (int(N) - n1i - n2i - nmi).astype(f)
        n1, n2, nm, dN = n1i.astype(f), n2i.astype(f), nmi.astype(f), f(N)
        av = (n1 + f(2.0) * n2) / (dN - nm)
        tmp1 = n1 * (f(1.0) - av) * (f(1.0) - av)
        tmp2 = n2 * (f(2.0) - av) * (f(2.0) - av)
        tmp0 = n0 * (f(0.0) - av) * (f(0.0) - av)
        return av, np.sqrt(f(int(N) - 1) / (tmp0 + tmp1 + tmp2))


def same_bits(a, b):
    """equal as float64 bit patterns; a NaN equals any NaN (its sign and payload are the divider's choice, not IEEE's)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------------------------
# what a file may hold where nobody should look
# ---------------------------------------------------------------------------------------------------------------------------------
FILLS = (0b00, 0b01, 0b10, 0b11, None)  # PLINK writes 0b00 (a called genotype: 2); None = random bits


def with_tail(bed, n_total, fill, seed=5):
    """a copy of the (M, ceil(n_total/4)) array whose unused tail slots hold `fill`; None = random fields from a seeded generator"""
    bed = np.asarray(bed, dtype=np.uint8)
    assert bed.shape[1] == (n_total + 3) // 4
    f = _fields(bed, n_total)
    spare = bed.shape[1] * 4 - n_total
    if fill is None:
        fill = np.random.default_rng(seed).integers(0, 4, size=(bed.shape[0], spare), dtype=np.uint8)
    return _pack(f, fill)


def widen(bed, extra, seed=6):
    """a copy with `extra` more columns of random bytes: a file whose rows are padded, stride_in larger than needed"""
    bed = np.asarray(bed, dtype=np.uint8)
    pad = np.random.default_rng(seed).integers(0, 256, size=(bed.shape[0], extra), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([bed, pad], axis=1))


# ---------------------------------------------------------------------------------------------------------------------------------
# the grids
# ---------------------------------------------------------------------------------------------------------------------------------
# the edges of a byte (4 rows), a dword (16: k_counts, k_recode_bed), a wave's tile and BLOCK_IND
NS = (2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097)
M_SMALL = 9
EXTRAS = (1, 3, 61)
_CODE_OF_GENO = np.array([0b11, 0b10, 0b00, 0b01], dtype=np.uint8)


def case_fields(N, M=M_SMALL, seed=0, missing_rate=0.03):
    """(M, N) 2-bit fields: binomial genotypes with 3 % missing calls, the last column but one missing everywhere, the last monomorphic"""
    rng = np.random.default_rng(100003 * N + 17 * M + seed)
    p = rng.uniform(0.1, 0.5, size=M)
    g = rng.binomial(2, p[:, None], size=(M, N)).astype(np.uint8)
    g[rng.random((M, N)) < missing_rate] = 3
    g[M - 2] = 3
    g[M - 1] = 2
    return _CODE_OF_GENO[g]


def case_bed(N, M=M_SMALL, seed=0, fill=0b00):
    """the grid's file for N rows: tail slots as PLINK writes them unless told otherwise"""
    return with_tail(_pack(case_fields(N, M, seed), 0), N, fill)


def called_after(bed, N, row_end):
    """a copy of the file in which the rows that share row_end's byte behind it, [row_end, next multiple of 4) below N, hold called
    genotypes in every column (1, 2, 0 in turn): what a shard ending at row_end must not take for its own"""
    f = _fields(bed, N).copy()
    spare = _fields(bed, bed.shape[1] * 4)[:, N:]
    for c in range(row_end, min(N, (row_end + 3) // 4 * 4)):
        f[:, c] = _CODE_OF_GENO[(np.arange(f.shape[0]) + c) % 3]
    return _pack(f, spare)


def cover(N):
    """cuts of [0, N) at multiples of 4 into up to three shards: [(row_begin, row_end)]"""
    q = N // 4
    cuts = sorted(set([0, 4 * (q // 3), 4 * ((2 * q + 2) // 3), N]))  # (4 * ((2q + 2) // 3) <= 4q <= N for every q)
    return list(zip(cuts[:-1], cuts[1:]))


def inside_shards(N):
    """shards without a keep list that end inside a byte below N: row_begin 0 and a multiple of 4 near the middle, n_local % 4 each of
    1, 2, 3, one shard as short as that and one as long as fits.  [0, 1) of a two-row file is the smallest of them."""
    out = []
    for b in sorted(set([0, 4 * (N // 8)])):
        for r in (1, 2, 3):
            for e in (b + r, b + (N - 1 - b - r) // 4 * 4 + r):
                if b < e < N and e % 4 and (b, e) not in out:
                    out.append((b, e))
    return out


MASKS = ("first", "last", "run", "alternate", "two", "all")


def keep_mask(name, N):
    k = np.ones(N, dtype=np.uint8)
    if name == "first":
        k[0] = 0
    elif name == "last":
        k[N - 1] = 0
    elif name == "run":
        k[N // 3:N // 3 + max(1, N // 4)] = 0
    elif name == "alternate":
        k[1::2] = 0
    elif name == "two":
        k[:] = 0
        k[[N // 3, N - 1]] = 1
    else:
        assert name == "all"
    return k


def keep_shards(nk):
    """of nk kept rows: shards whose row_begin is 1, 2 and 3 mod 4 (near the middle where that fits, else at the start) and whose
    row_end is below nk"""
    out = []
    for r in (1, 2, 3):
        for b in (4 * (nk // 8) + r, r):
            e = nk - 1 - (r & 1)
            if b < e:
                out.append((b, e))
                break
    return out
