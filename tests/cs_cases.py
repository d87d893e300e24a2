"""What the credible-set tests share (no test of its own): genotypes with LD of their own, masks from NumPy's r, crafted inclusion
flags, the cases of tests/test_gpu_cs.py, and the conditions those tests rely on, evaluated on any set of results."""
import os
import sys

import numpy as np

from hydra_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cs_restate as cr  # noqa: E402
import ldwalk  # noqa: E402

N, M = 300, 300
R2 = 0.5
WINDOWS = [1, 63, 64, 65, 130]
MAX_SIZES = [1, 3, 64]
# NREC -> (C, T): 65 = 5 x 13 puts a record's bits across the word boundary
SHAPES = {4: (1, 4), 64: (2, 32), 65: (5, 13), 130: (1, 130)}
ALPHA, PEP = 0.9, 0.7
# (W, NREC) -> seed of the flags.  A seed that fails a condition of tests/test_cs_restatement_cpu.py is changed HERE.
SEEDS = {(W, nrec): 100 + 7 * W + nrec for W in WINDOWS for nrec in SHAPES}
GENO_SEED = 11


def ld_genotypes(m=M, n=N, seed=GENO_SEED, missing_rate=0.02):
    """(m, n) uint8 and the runs [(first, length)]: runs of 2-6 neighbouring columns are copies of the run's first column with a share
    of the calls drawn afresh -- 3 %, 12 % or 30 %, so r^2 with the first is about 0.94, 0.77 or 0.49, and the copies' r^2 among
    themselves lies on both sides of 0.5 -- with now and then an independent column between two runs; 2 % missing calls"""
    rng = np.random.default_rng(seed)
    geno = synth.make_genotypes(m, n, seed=seed, maf_lo=0.2)
    runs, j = [], 0
    while j < m:
        length = min(int(rng.integers(2, 7)), m - j)
        for k in range(1, length):
            fresh = rng.random(n) < rng.choice([0.03, 0.12, 0.30])
            geno[j + k] = np.where(fresh, geno[j + k], geno[j])
        runs.append((j, length))
        j += length + int(rng.integers(0, 2))
    geno[rng.random((m, n)) < missing_rate] = 3
    return geno, runs


def numpy_masks(geno, W, t=R2):
    """fwd, bwd (M, wpr) uint64 from NumPy's r of the standardised columns, the default window min(W, M - 1 - j)"""
    m, n = geno.shape
    X = synth.standardize(geno)
    r = X.T @ X / (n - 1.0)
    band = np.zeros((m, W), dtype=bool)
    for d in range(1, min(W, m - 1) + 1):
        rr = np.diagonal(r, d)
        band[:m - d, d - 1] = rr * rr >= t
    return ldwalk.pack(band), ldwalk.pack(ldwalk.backward_of(band))


def crafted_flags(runs, m, nrec, seed):
    """(nrec, m) bool: per run of the genotypes one of six patterns, in turn, so that every kind of candidate occurs
      0 spread    the records are dealt round the run's markers, the first taking half: a set of several members, equal counts among
                  the rest (the index decides), PEP = all records
      1 single    the run's first marker is in every record
      2 short     the run's markers hold a quarter of the records between them
      3 stacked   every marker of the run is in the same 60 % of the records: the counts add up, the PEP does not
      4 hole      like 0, but the run's second marker is in no record (a friend with cnt 0)
      5 random    each marker in a random third of the records"""
    rng = np.random.default_rng(seed)
    flags = np.zeros((nrec, m), dtype=bool)
    rec = np.arange(nrec)
    for k, (j0, length) in enumerate(runs):
        cols = list(range(j0, j0 + length))
        kind = k % 6
        if kind in (0, 4):
            if kind == 4 and length >= 3:
                cols.pop(1)
            half = (nrec + 1) // 2
            flags[:half, cols[0]] = True
            for i, q in enumerate(rec[half:]):
                flags[q, cols[1 + i % (len(cols) - 1)]] = True
        elif kind == 1:
            flags[:, cols[0]] = True
        elif kind == 2:
            for i, q in enumerate(rec[:max(1, nrec // 4)]):
                flags[q, cols[i % len(cols)]] = True
        elif kind == 3:
            flags[:max(1, (6 * nrec) // 10), cols] = True
        else:
            for c in cols:
                flags[rng.random(nrec) < 1.0 / 3.0, c] = True
    return flags


def history_of(flags, C, T):
    """the restatement's history fed record by record: record q = t C + r is row q of flags"""
    h = cr.History(C, T, flags.shape[1])
    for t in range(T):
        h.add(flags[t * C:(t + 1) * C])
    return h


def leads_of(cnt, m=M):
    """marker 0, marker m - 1 and every marker with cnt >= 1, ascending"""
    return np.array(sorted(set([0, m - 1]) | set(np.flatnonzero(cnt >= 1).tolist())), dtype=np.uint32)


def conditions(results, leads, cnt, nrec, notes):
    """What a case must hold, from the results per max_size ({max_size: (status, size, sum, pep, members)}) and the notes of the
    restatement's picks: the kinds of candidates, and the three fates in the walk at the largest max_size.  Returns the missing ones."""
    missing = []
    status = np.concatenate([results[k][0] for k in MAX_SIZES])
    size = np.concatenate([results[k][1] for k in MAX_SIZES])
    if not np.any(size >= 3):
        missing.append("a candidate of size >= 3")
    if not np.any((status == 0) & (size == 1)):
        missing.append("a candidate of size 1")
    if not np.any(status == 1):
        missing.append("a short candidate")
    if not np.any(status == 2):
        missing.append("a candidate at the cap")
    if not notes.get("tie"):
        missing.append("a pick decided by the index")
    if not notes.get("zero"):
        missing.append("a friend with cnt 0 passed over")
    st, sz, _, pep, mem = results[MAX_SIZES[-1]]
    min_pep = cr.ceil_count(PEP, nrec)
    taken = cr.walk(leads, cnt[leads], st, sz, pep, mem, min_pep)
    if not taken:
        missing.append("an accepted candidate")
    if not np.any((st == 0) & (pep < min_pep)):
        missing.append("a PEP-rejected candidate")
    ok = [i for i in range(len(leads)) if st[i] == 0 and pep[i] >= min_pep]
    if len(ok) <= len(taken):
        missing.append("a candidate rejected for overlap")
    return missing
