"""The rule of hgibbs_roh in numpy (include/hgibbs.h), for the tests: prefix sums of het and missing calls, the
need table, the segment walk.  Integers only, as the device; the list comes back sorted by (row, first)."""
import numpy as np

NONE = 0xFFFFFFFF  # max_het: no limit


def need_table(threshold, window):
    """need[0 .. 64]: need[n] = the smallest integer c with float(c) / float(n) >= threshold for n = 1 .. window (0 elsewhere)"""
    need = [0] * 65
    for n in range(1, window + 1):
        c = 1
        while float(c) / float(n) < threshold:
            c += 1
        need[n] = c
    return need


def params(window=50, window_het=1, window_missing=5, threshold=0.05, min_snps=100, min_bp=1000000, dens_bp=50000, gap_bp=1000000, max_het=None):
    """PLINK 1.9's defaults, in base pairs"""
    return dict(window=window, window_het=window_het, window_missing=window_missing, threshold=threshold, min_snps=min_snps, min_bp=min_bp,
                dens_bp=dens_bp, gap_bp=gap_bp, max_het=max_het)


def covered(het, mis, W, h, m, need):
    """het, mis: (L, R) 0/1 arrays of one run -> (L, R) bool: the covered positions"""
    L, R = het.shape
    cov = np.zeros((L, R), dtype=bool)
    if L < W:
        return cov
    ph = np.vstack([np.zeros((1, R), np.int64), np.cumsum(het, axis=0, dtype=np.int64)])
    pm = np.vstack([np.zeros((1, R), np.int64), np.cumsum(mis, axis=0, dtype=np.int64)])
    hom = ((ph[W:] - ph[:L - W + 1]) <= h) & ((pm[W:] - pm[:L - W + 1]) <= m)  # (L - W + 1, R): window s
    pw = np.vstack([np.zeros((1, R), np.int64), np.cumsum(hom, axis=0, dtype=np.int64)])
    k = np.arange(L)
    lo, hi = np.maximum(0, k - W + 1), np.minimum(k, L - W)
    nw = hi - lo + 1
    cnt = pw[hi + 1] - pw[lo]
    return cnt >= np.asarray(need, dtype=np.int64)[nw][:, None]


def segments(geno, run_off, idx, bp, window=50, window_het=1, window_missing=5, threshold=0.05, min_snps=100, min_bp=1000000, dens_bp=50000,
             gap_bp=1000000, max_het=None, need=None):
    """geno: (M, N) uint8, 1 = het, 3 = missing.  Returns the kept segments as a list of (row, first, last, nsnp, nhet, nmiss) sorted by
    (row, first); first and last are positions in idx."""
    if need is None:
        need = need_table(threshold, window)
    idx = np.asarray(idx, dtype=np.int64)
    bp = np.asarray(bp, dtype=np.int64)
    out = []
    for r in range(len(run_off) - 1):
        o, e = int(run_off[r]), int(run_off[r + 1])
        L = e - o
        if L < window:
            continue
        g = geno[idx[o:e]]
        het, mis = (g == 1).astype(np.int64), (g == 3).astype(np.int64)
        cov = covered(het, mis, window, window_het, window_missing, need)
        b = bp[o:e]
        cut = np.zeros(L, dtype=bool)  # cut[k]: position k starts a new segment whatever came before
        cut[1:] = (b[1:] - b[:-1]) > gap_bp
        first = cov.copy()
        first[1:] &= ~cov[:-1] | cut[1:, None]
        last = cov.copy()
        last[:-1] &= ~cov[1:] | cut[1:, None]
        rows, s = np.nonzero(first.T)  # ordered by row, then position: the starts and the ends pair up in order
        rows2, t = np.nonzero(last.T)
        assert np.array_equal(rows, rows2) and np.all(s <= t)
        ph = np.vstack([np.zeros((1, het.shape[1]), np.int64), np.cumsum(het, axis=0)])
        pm = np.vstack([np.zeros((1, mis.shape[1]), np.int64), np.cumsum(mis, axis=0)])
        n = t - s + 1
        nhet = ph[t + 1, rows] - ph[s, rows]
        nmis = pm[t + 1, rows] - pm[s, rows]
        ln = b[t] - b[s]
        keep = (n >= min_snps) & (ln >= min_bp) & (ln <= dens_bp * n)
        if max_het is not None and max_het != NONE:
            keep &= nhet <= max_het
        for i in np.flatnonzero(keep):
            out.append((int(rows[i]), o + int(s[i]), o + int(t[i]), int(n[i]), int(nhet[i]), int(nmis[i])))
    out.sort(key=lambda x: (x[0], x[1]))
    return out


def tried_case():
    """The case of the issue: 1500 markers x 65 rows in runs of 40, 7, 653 and 800 markers, a 50 kb jump at marker 450 and a stretch of
    row 3 without hets.  Returns geno, run_off, idx, bp."""
    from hydra_amd import synth

    geno = synth.make_genotypes(1500, 65, seed=7, missing_rate=0.02)
    run_off = [0, 40, 47, 700, 1500]
    bp = np.cumsum(np.random.default_rng(1).integers(1, 3000, size=1500)).astype(np.int64)
    bp[450:] += 50000
    stretch = geno[200:900, 3]
    stretch[stretch == 1] = 0
    return geno, run_off, np.arange(1500), bp
