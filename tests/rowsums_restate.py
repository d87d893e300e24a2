"""hgibbs_row_sums restated in Python integers (include/hgibbs.h), for the tests that pin it bit for bit.

    scale     e_t from math.frexp of the table's largest magnitude (max < 2^e_t), E_t = 52 - e_t; E_t = 0 for an all-zero table
    quantise  q = int(np.rint(np.ldexp(v, E_t)))                      (round to nearest, ties to even, as llrint)
    sum       per row the big-integer sum of q[t][j][code_ij]
    result    float(total) * 2.0 ** -E_t                              (Python's int -> float is correctly rounded)
"""
import math

import numpy as np


def scale(table):
    mx = float(np.max(np.abs(table))) if table.size else 0.0
    if not mx > 0.0:
        return 0
    return 52 - math.frexp(mx)[1]


def quantise(table, E):
    """(M, 4) float64 -> (M, 4) object array of Python ints"""
    q = np.rint(np.ldexp(np.asarray(table, dtype=np.float64), E))
    return np.array([[int(v) for v in row] for row in q], dtype=object).reshape(q.shape)


def row_sums(codes, tab):
    """codes (N, M) in {0, 1, 2, 3}, tab (T, M, 4) float64 -> (N, T) float64"""
    codes = np.asarray(codes)
    tab = np.asarray(tab, dtype=np.float64)
    N, M = codes.shape
    T = tab.shape[0]
    out = np.zeros((N, T))
    cols = np.arange(M)
    for t in range(T):
        E = scale(tab[t])
        q = quantise(tab[t], E)
        for i in range(N):
            total = sum(q[cols, codes[i]].tolist(), 0) if M else 0
            out[i, t] = float(total) * 2.0 ** -E
    return out


def row_sums_split(codes, tab):
    """row_sums for the larger shapes: q = hi 2^26 + lo summed in two int64 NumPy sums (exact: |hi| <= 2^26 and 0 <= lo < 2^26 over
    fewer than 2^30 markers), the halves put together as Python integers.  tests/test_rowsums_restatement_cpu.py holds it to row_sums
    bit for bit."""
    codes = np.asarray(codes).astype(np.int64)
    tab = np.asarray(tab, dtype=np.float64)
    N, M = codes.shape
    T = tab.shape[0]
    out = np.zeros((N, T))
    cols = np.arange(M)[None, :]
    for t in range(T):
        E = scale(tab[t])
        q = np.rint(np.ldexp(tab[t], E)).astype(np.int64)
        hi = (q >> 26)[cols, codes].sum(axis=1)
        lo = (q & ((1 << 26) - 1))[cols, codes].sum(axis=1)
        for i in range(N):
            out[i, t] = float((int(hi[i]) << 26) + int(lo[i])) * 2.0 ** -E
    return out


def codes_of(geno):
    """synth's genotypes (M, N) int8, 3 (or negative) = missing call -> device codes (N, M), 3 = missing"""
    g = np.asarray(geno).T.astype(np.int64)
    return np.where((g < 0) | (g > 2), 3, g)


def qc_tables(codes, qc_marker):
    """the seven tables of --qc for codes (N, M) and the mask of QC markers (M,)"""
    N, M = codes.shape
    tab = np.zeros((7, M, 4))
    tab[0, :, 3] = 1.0
    for j in range(M):
        if not qc_marker[j]:
            continue
        c = codes[:, j]
        n = int(np.sum(c != 3))
        p = (int(np.sum(c == 1)) + 2.0 * int(np.sum(c == 2))) / (2.0 * n)
        h = 2.0 * p * (1.0 - p)
        e = 1.0 - h * (2.0 * n) / (2.0 * n - 1.0)
        for g in range(3):
            x = float(g)
            tab[1, j, g] = 1.0
            tab[2, j, g] = 0.0 if g == 1 else 1.0
            tab[3, j, g] = e
            tab[4, j, g] = (x - 2.0 * p) * (x - 2.0 * p) / h - 1.0
            tab[5, j, g] = 1.0 - x * (2.0 - x) / h
            tab[6, j, g] = (x * x - (1.0 + 2.0 * p) * x + 2.0 * p * p) / h
    return tab


def polymorphic(codes):
    """markers with a finite sd: some called genotype differs from another"""
    out = np.zeros(codes.shape[1], dtype=bool)
    for j in range(codes.shape[1]):
        c = codes[:, j]
        c = c[c != 3]
        out[j] = c.size > 0 and np.any(c != c[0])
    return out
