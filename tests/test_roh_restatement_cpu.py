"""tests/roh_restate.py, the rule of hgibbs_roh in numpy, checked without a device: against a second implementation that follows the
definition (every window of every position, one row at a time), against a case typed out by hand, and its need table."""
import numpy as np
import pytest

import roh_restate as rr


def by_definition(geno, run_off, idx, bp, window, window_het, window_missing, threshold, min_snps, min_bp, dens_bp, gap_bp, max_het=None):
    """the rule word for word: no prefix sums, no vectors"""
    W = window
    out = []
    for row in range(geno.shape[1]):
        for r in range(len(run_off) - 1):
            o, L = run_off[r], run_off[r + 1] - run_off[r]
            code = [int(geno[idx[o + k], row]) for k in range(L)]

            def homozygous(s):
                return sum(c == 1 for c in code[s:s + W]) <= window_het and sum(c == 3 for c in code[s:s + W]) <= window_missing

            cov = []
            for k in range(L):
                over = [s for s in range(0, L - W + 1) if s <= k < s + W]  # empty when L < W
                hom = sum(homozygous(s) for s in over)
                need = None
                if over:
                    need = next(c for c in range(0, len(over) + 2) if c >= 1 and float(c) / float(len(over)) >= threshold)
                cov.append(bool(over) and hom >= need)
            k = 0
            while k < L:
                if not cov[k]:
                    k += 1
                    continue
                e = k
                while e + 1 < L and cov[e + 1] and bp[o + e + 1] - bp[o + e] <= gap_bp:
                    e += 1
                n, ln = e - k + 1, int(bp[o + e]) - int(bp[o + k])
                nhet, nmis = sum(c == 1 for c in code[k:e + 1]), sum(c == 3 for c in code[k:e + 1])
                if n >= min_snps and ln >= min_bp and ln <= dens_bp * n and (max_het is None or nhet <= max_het):
                    out.append((row, o + k, o + e, n, nhet, nmis))
                k = e + 1
    return sorted(out, key=lambda x: (x[0], x[1]))


def test_need_table():
    n5 = rr.need_table(0.05, 64)
    assert n5[1:21] == [1] * 20 and n5[21] == 2 and n5[40] == 2 and n5[41] == 3 and n5[50] == 3 and n5[64] == 4
    assert n5[0] == 0
    nh = rr.need_table(0.5, 64)
    assert nh[1:9] == [1, 1, 2, 2, 3, 3, 4, 4] and nh[63] == 32 and nh[64] == 32
    n1 = rr.need_table(1.0, 64)
    assert n1[1:] == list(range(1, 65))
    assert rr.need_table(0.05, 8)[9:] == [0] * 56
    for th in (0.05, 0.5, 1.0, 1e-9, 0.3333333333333333):
        t = rr.need_table(th, 64)
        for n in range(1, 65):
            assert 1 <= t[n] <= n and float(t[n]) / n >= th and (t[n] == 1 or float(t[n] - 1) / n < th)


def test_hand_case():
    """12 markers, 3 rows, W = 3, h = 0, m = 1, threshold 1 (every window over a position must be homozygous).
         marker  0 1 2 3 4 5 6 7 8 9 10 11        bp = 10 x marker, but marker 8 .. 11 are 1000 further on
         row 0   0 0 0 1 0 0 0 0 0 0 0  0         windows 1, 2, 3 hold the het: covered 0 and 6 .. 11; 0 alone is too short
         row 1   3 0 0 0 3 3 2 2 2 1 2  2         two missing in windows 3, 4, the het in 7, 8, 9: covered 0 .. 2
         row 2   2 2 2 2 2 2 2 2 2 2 2  2         covered 0 .. 11, cut by the gap between 7 and 8
    """
    geno = np.array([[0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0],
                     [3, 0, 0, 0, 3, 3, 2, 2, 2, 1, 2, 2],
                     [2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2]], dtype=np.uint8).T.copy()
    bp = np.array([10 * j + (1000 if j >= 8 else 0) for j in range(12)], dtype=np.int64)
    kw = dict(window=3, window_het=0, window_missing=1, threshold=1.0, min_snps=2, min_bp=0, dens_bp=10**9, gap_bp=500)
    want = [(0, 6, 7, 2, 0, 0), (0, 8, 11, 4, 0, 0), (1, 0, 2, 3, 0, 1), (2, 0, 7, 8, 0, 0), (2, 8, 11, 4, 0, 0)]
    assert rr.segments(geno, [0, 12], np.arange(12), bp, **kw) == want
    assert by_definition(geno, [0, 12], np.arange(12), bp, **kw) == want
    # without the gap rows 0 and 2 are not cut; the length filter then drops what is shorter than 50 bp
    kw.update(gap_bp=5000, min_bp=50)
    want = [(0, 6, 11, 6, 0, 0), (2, 0, 11, 12, 0, 0)]
    assert rr.segments(geno, [0, 12], np.arange(12), bp, **kw) == want
    assert by_definition(geno, [0, 12], np.arange(12), bp, **kw) == want
    # threshold 0.05: one homozygous window covers its three positions (row 1: windows 0, 1, 2 and 5, 6 meet)
    kw.update(threshold=0.05, min_bp=0, min_snps=1)
    want = [(0, 0, 2, 3, 0, 0), (0, 4, 11, 8, 0, 0), (1, 0, 8, 9, 0, 3), (2, 0, 11, 12, 0, 0)]
    assert rr.segments(geno, [0, 12], np.arange(12), bp, **kw) == want
    assert by_definition(geno, [0, 12], np.arange(12), bp, **kw) == want


@pytest.fixture(scope="module")
def tried():
    return rr.tried_case()


def test_tried_case_counts(tried):
    geno, run_off, idx, bp = tried
    small = rr.segments(geno, run_off, idx, bp, window=8, window_het=0, window_missing=1, threshold=0.05, min_snps=10, min_bp=5000, dens_bp=3000,
                        gap_bp=40000)
    assert len(small) == 532 and len({s[0] for s in small}) == 65
    assert not [s for s in small if 40 <= s[1] < 47], "the 7-marker run is shorter than the window"
    big = rr.segments(geno, run_off, idx, bp, window=50, window_het=1, window_missing=5, threshold=0.05, min_snps=100, min_bp=5000, dens_bp=3000,
                      gap_bp=40000)
    assert [s[0] for s in big] == [3, 3, 3], big
    assert big[0][2] == 449 and big[1][1] == 450 and big[1][2] == 699 and big[2][1] == 700, "cut at the gap and at the run boundary"


@pytest.mark.parametrize("kw", [
    dict(window=8, window_het=0, window_missing=1, threshold=0.05, min_snps=10, min_bp=5000, dens_bp=3000, gap_bp=40000),
    dict(window=5, window_het=1, window_missing=0, threshold=0.5, min_snps=4, min_bp=0, dens_bp=1500, gap_bp=2500, max_het=1),
    dict(window=1, window_het=0, window_missing=0, threshold=1.0, min_snps=3, min_bp=2000, dens_bp=10**6, gap_bp=10**9),
    dict(window=40, window_het=3, window_missing=5, threshold=1.0, min_snps=1, min_bp=0, dens_bp=10**6, gap_bp=10**9),
    dict(window=64, window_het=12, window_missing=5, threshold=0.05, min_snps=70, min_bp=0, dens_bp=10**6, gap_bp=40000),
])
def test_against_the_definition(tried, kw):
    """a selection with holes, runs of 40, 7, 130 and 90 markers, 9 rows"""
    geno, _, _, bp = tried
    idx = np.concatenate([np.arange(0, 80, 2), np.arange(100, 107), np.arange(380, 520)[np.arange(140) % 14 != 3], np.arange(800, 890)])
    run_off = [0, 40, 47, 177, 267]
    g = geno[:, :9]
    got = rr.segments(g, run_off, idx, bp[idx], **kw)
    assert got and got == by_definition(g, run_off, idx, bp[idx], **kw)
