"""Mean and variance of the scores of marker sets (hgibbs_region_var, hydra_mi355x --pve) against NumPy in f64, against hgibbs_score,
and against themselves: bit-identical however the work is cut."""
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import capi, synth
from test_gpu_score import EXE, _bet, digit_samples, load, weights

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def make_sets(M):
    """windows of 1, 63, 64, 65 and 130 markers off the multiples of 64, two overlapping windows, every 7th marker, the column that is
    all missing when the cohort has missing calls, an empty set, every marker"""
    return [np.arange(5, 6), np.arange(3, 66), np.arange(70, 134), np.arange(10, 75), np.arange(33, 163), np.arange(100, 160),
            np.arange(140, 200), np.arange(3, M, 7), np.array([M // 2]), np.zeros(0, dtype=np.int64), np.arange(M)]


def reference(geno, a, o, sets, rows=8192):
    """per set: mean and ddof = 1 variance over the rows of v = sum_{j in set} [g != 3] (a g + o), and mag = max_i sum_{j in set} |term|
    (the sum of test_gpu_score.reference).  Both as ONE product per slice of rows: the indicators of the genotypes 0, 1, 2 of the set's
    markers against the terms o, a + o, 2 a + o and their magnitudes.  v is kept sample-major, so NumPy sums it pairwise."""
    N, S = geno.shape[1], a.shape[0]
    mean, var, mag = (np.zeros((len(sets), S)) for _ in range(3))
    for r, idx in enumerate(sets):
        if idx.size == 0:
            continue
        terms = [o[:, idx], a[:, idx] + o[:, idx], 2.0 * a[:, idx] + o[:, idx]]
        W = np.concatenate([np.concatenate([t, np.abs(t)]) for t in terms], axis=1)  # (2 S, 3 |set|)
        v = np.zeros((S, N))
        ind = np.empty((3 * idx.size, min(rows, N)), dtype=np.float32)
        for i0 in range(0, N, rows):
            gs = geno[idx, i0:i0 + rows]
            for k in range(3):
                np.equal(gs, k, out=ind[k * idx.size:(k + 1) * idx.size, :gs.shape[1]], casting="unsafe")
            out = W @ ind[:, :gs.shape[1]]
            v[:, i0:i0 + rows] = out[:S]
            mag[r] = np.maximum(mag[r], out[S:].max(axis=1))
        mean[r] = v.mean(axis=1)
        var[r] = v.var(axis=1, ddof=1)
    return mean, var, mag


def check(got, ref, n, what):
    (mean, var), (rmean, rvar, mag) = got, ref
    assert mean.shape == rmean.shape and var.shape == rvar.shape
    em, ev = np.abs(mean - rmean), np.abs(var - rvar)
    print(what, "mean err / mag", float(np.max(em / np.maximum(mag, 1e-300))), "var err / mag^2", float(np.max(ev / np.maximum(mag * mag, 1e-300))))
    assert np.all(em <= (n * EPS + 1e-12) * mag), (what, float(np.max(em / np.maximum(mag, 1e-300))))
    assert np.all(ev <= (2 * n * EPS + 1e-11) * mag * mag), (what, float(np.max(ev / np.maximum(mag * mag, 1e-300))))


@pytest.mark.parametrize("N", [2, 63, 257, 4097, 130001])
@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_region_var_matches_numpy(N, missing):
    M = 200
    dev, geno = load(N, M, missing, seed=N + 7)
    sets = make_sets(M)
    counts = (1, 2, 7, 16, 33)
    # one reference for all the weight vectors of the case
    ws = [weights(S, M, seed=S) for S in counts]
    ref = reference(geno, np.concatenate([w[0] for w in ws]), np.concatenate([w[1] for w in ws]), sets)
    at = 0
    for S, (a, o) in zip(counts, ws):
        mean, var = dev.region_var(a, o, sets)
        assert mean.shape == (len(sets), S)
        check((mean, var), [x[:, at:at + S] for x in ref], N, (N, missing, S))
        at += S
        assert np.all(mean[9] == 0.0) and np.all(var[9] == 0.0)  # the empty set
        if missing:
            assert np.all(mean[8] == 0.0) and np.all(var[8] == 0.0)  # the all-missing column
        if S > 1:
            assert np.all(mean[:, 1] == 0.0) and np.all(var[:, 1] == 0.0)  # the all-zero sample
        assert np.any(var[10] > 0.0)


@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_region_var_agrees_with_the_score(missing):
    """v is never stored, but it is hgibbs_score's for the weights zeroed outside the set: only the order of the sums over i differs"""
    N, M, S = 4097, 700, 7
    dev, geno = load(N, M, missing, seed=5)
    sets = make_sets(M)
    a, o = weights(S, M, seed=13)
    mean, var = dev.region_var(a, o, sets)
    _, _, mag = reference(geno, a, o, sets)
    for r, idx in enumerate(sets):
        am, om = np.zeros_like(a), np.zeros_like(o)
        am[:, idx], om[:, idx] = a[:, idx], o[:, idx]
        v = dev.score(am, om)
        assert np.all(np.abs(mean[r] - v.mean(axis=0)) <= N * EPS * mag[r]), r
        assert np.all(np.abs(var[r] - v.var(axis=0, ddof=1)) <= 2 * N * EPS * mag[r] ** 2), r


@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_region_var_is_bit_identical_however_the_work_is_cut(missing):
    N, M, S = 4097, 700, 33
    dev, geno = load(N, M, missing, seed=3)
    sets = make_sets(M)
    a, o = weights(S, M, seed=11)
    first = dev.region_var(a, o, sets)

    def same(got, what):
        assert np.array_equal(first[0], got[0]) and np.array_equal(first[1], got[1]), what

    same(dev.region_var(a, o, sets), "repeat")
    parts = [dev.region_var(a[:5], o[:5], sets), dev.region_var(a[5:], o[5:], sets)]
    same([np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1)], "S in chunks of 5 and 28")
    rev = dev.region_var(a, o, sets[::-1])
    same([rev[0][::-1], rev[1][::-1]], "sets reversed")
    parts = [dev.region_var(a, o, sets[:4]), dev.region_var(a, o, sets[4:])]
    same([np.concatenate([p[k] for p in parts], axis=0) for k in (0, 1)], "sets in two calls")
    for sp in (2, 4, 8, 16):
        dev.set_option("score_sp", sp)
        same(dev.region_var(a, o, sets), ("score_sp", sp))
    dev.set_option("score_sp", 0)
    for kb in (1, 2):  # every set above 64 resp. 128 markers takes the large-set path
        dev.set_option("rvar_kb_max", kb)
        same(dev.region_var(a, o, sets), ("rvar_kb_max", kb))
        dev.set_option("score_sp", 16)
        same(dev.region_var(a, o, sets), ("rvar_kb_max", kb, "score_sp", 16))
        dev.set_option("score_sp", 0)
    dev.set_option("rvar_kb_max", 0)
    assert dev.last_region_var_ms() > 0.0


DIGIT_ANCHOR = 100
# 1, 2, 63 and 64 markers with the anchor among them, first, last and inside; and one of 65 (the anchor and 64 others), more than one
# block of 64, which rvar_kb_max = 1 sends through score_dev_run and k_rvar_dense
DIGIT_SETS = [np.array([DIGIT_ANCHOR]), np.array([DIGIT_ANCHOR, 150]), np.arange(38, 101), np.arange(100, 164), np.arange(64, 129)]


def digit_reference(geno, kappa, lam, sets):
    """mean and var of digit_samples' scores from exact integers.  v_i = K_i 256^d 2^-40 with K_i = sum_{j in set} [g != 3] (kappa g +
    lambda), |K_i| <= 64 (2 x 127 + 127) = 24 384 < 2^15 for the anchor and at most 64 other markers: every sum of v (< 2^15 x 4097) and
    of v^2 (< 2^30 x 4097 units) over at most 4 097 rows is exact in f64 in ANY order, so s1 and s2 are the exact ones, and k_rvar_final's
    formula m = s1 / n, var = max(0, (s2 - s1 m) / (n - 1)) in f64 (no fused multiply-add: the build has -ffp-contract=off) is all
    that rounds."""
    n = geno.shape[1]
    g = np.where(geno == 3, 0, geno).astype(np.int64)
    called = (geno != 3).astype(np.int64)
    mean, var = np.zeros((len(sets), 7)), np.zeros((len(sets), 7))
    for r, idx in enumerate(sets):
        K = kappa[:, idx] @ g[idx] + lam[:, idx] @ called[idx]  # (7, n) int64
        assert np.abs(K).max() < 1 << 15
        for d in range(7):
            unit = np.ldexp(1.0, 8 * d - 40)
            s1 = np.float64(int(K[d].sum())) * unit
            s2 = np.float64(int((K[d] * K[d]).sum())) * unit * unit
            m = s1 / np.float64(n)
            mean[r, d] = m
            var[r, d] = max(0.0, (s2 - s1 * m) / (np.float64(n) - 1.0))
    return mean, var


@pytest.mark.parametrize("N", [2, 63, 257, 4097])
@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_region_var_bits_of_every_digit_on_its_own(N, missing):
    """Weights for which every order of the sums over the rows gives the same bits (digit_samples, digit_reference), so mean and var are
    compared bit for bit without restating rv_tree: the weights of sample d live in base-256 digit d alone (E = 40,
    tests/test_score_restatement_cpu.py), and on clean data a kernel that drops that digit returns var = 0 there.  With missing calls
    the second product's operand -(3 q_a + q_o) carries into digit d + 1 for d < 6."""
    M = 200
    geno = synth.make_genotypes(M, N, seed=N + 11, missing_rate=missing)
    geno[DIGIT_ANCHOR] = 0
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    a, o, kappa, lam = digit_samples(M, DIGIT_ANCHOR, seed=N)
    rmean, rvar = digit_reference(geno, kappa, lam, DIGIT_SETS)
    assert np.all(rvar[0] == 0.0) and np.all(rmean[0] == 0.0)  # the anchor alone
    assert np.all(np.any(rvar > 0.0, axis=0))  # every digit's sample varies in some set

    def same(what):
        mean, var = dev.region_var(a, o, DIGIT_SETS)
        dm, dv = float(np.max(np.abs(mean - rmean))), float(np.max(np.abs(var - rvar)))
        print(N, missing, what, "largest |device - restatement|: mean", dm, "var", dv)
        assert np.array_equal(mean.view(np.int64), rmean.view(np.int64)), (what, dm)
        assert np.array_equal(var.view(np.int64), rvar.view(np.int64)), (what, dv)
        assert np.all(np.any(var > 0.0, axis=0)), what

    for kb in (0, 1):  # 1: the set of 65 markers takes the dense path
        dev.set_option("rvar_kb_max", kb)
        for sp in (0, 2, 4, 8, 16):
            dev.set_option("score_sp", sp)
            same(("rvar_kb_max", kb, "score_sp", sp))
    dev.set_option("score_sp", 0)
    dev.set_option("rvar_kb_max", 0)


@pytest.mark.parametrize("N,M", [(63, 20000), (130001, 3000)])
def test_region_var_many_blocks_in_one_workgroup(N, M):
    """One set of all markers: 313 resp. 47 blocks of 64 in every workgroup (the steady state of the loop: the list read two blocks
    ahead, codes and operands one, the LDS double buffer).  The data: at most 4 099 rows are drawn from synth with 2 % missing calls and
    repeated to N rows (a period that is no multiple of the 256 rows of a workgroup, so the row blocks differ; drawing 390 million
    genotypes would take longer than everything else in the test).  The blocks of 64 markers with index % 3 == 1 keep their missing
    calls in every column, the blocks between are made clean, and one column of a clean block is all missing: blocks with the second
    product sit between blocks without, as in test_score_many_marker_blocks_per_workgroup.  S = 7 and 16 at N = 63, S = 7 at
    N = 130 001 (one pass of eight samples; the passes themselves are test_region_var_matches_numpy's)."""
    base = synth.make_genotypes(M, min(N, 4099), seed=N + M, missing_rate=0.02)
    geno = np.ascontiguousarray(np.tile(base, (1, -(-N // base.shape[1])))[:, :N])
    clean = (np.arange(M) // 64) % 3 != 1
    geno[clean] = np.where(geno[clean] == 3, 0, geno[clean])
    geno[64 * 4 + 5, :] = 3
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N, n_global=max(N, 2))
    sets = [np.arange(M)]
    for S in ((7, 16) if N < 1000 else (7,)):
        a, o = weights(S, M, seed=S + 1)
        got = dev.region_var(a, o, sets)
        check(got, reference(geno, a, o, sets), N, (N, M, S))
        dev.set_option("rvar_kb_max", 8)
        large = dev.region_var(a, o, sets)
        dev.set_option("rvar_kb_max", 0)
        assert np.array_equal(got[0], large[0]) and np.array_equal(got[1], large[1])


def test_region_var_refusals():
    dev = capi.Device(0)
    a, o = weights(2, 70, seed=2)
    with pytest.raises(capi.HgError, match="no genotypes"):
        capi.check(dev.L.hgibbs_region_var(dev.h, 1, None, None, 1, None, None, None, None))
    dev.close()
    dev, _ = load(1, 70, 0.0, seed=1)
    with pytest.raises(capi.HgError, match="at least two rows"):
        dev.region_var(a, o, [np.arange(3)])
    dev.close()
    dev, geno = load(100, 70, 0.0, seed=1)
    sets = [np.arange(3, 40), np.array([1, 69])]
    with pytest.raises(capi.HgError, match="at least one weight vector"):
        dev.region_var(a[:0], o[:0], sets)
    with pytest.raises(capi.HgError, match="at least one marker set"):
        dev.region_var(a, o, [])
    with pytest.raises(capi.HgError, match="set 1 names marker 70, the handle has 70"):
        dev.region_var(a, o, [np.arange(3), np.array([1, 70])])
    with pytest.raises(capi.HgError, match="set 0: marker 5 after 5, the indices of a set must be strictly increasing"):
        dev.region_var(a, o, [np.array([2, 5, 5])])
    with pytest.raises(capi.HgError, match="set 1: marker 4 after 9"):
        dev.region_var(a, o, [np.arange(3), np.array([9, 4])])
    a[1, 5] = np.nan  # in a set
    with pytest.raises(capi.HgError, match="not finite"):
        dev.region_var(a, o, sets)
    a[1, 5] = 0.0
    o[0, 0] = np.inf  # in no set
    with pytest.raises(capi.HgError, match="not finite"):
        dev.region_var(a, o, sets)
    o[0, 0] = 0.0
    # the handle still answers
    check(dev.region_var(a, o, sets), reference(geno, a, o, sets), 100, "after the refusals")
    mean_only = np.zeros((2, 2))
    off = np.array([0, 37, 39], dtype=np.uint64)
    idx = np.concatenate(sets).astype(np.uint32)
    C = capi.C
    capi.check(dev.L.hgibbs_region_var(dev.h, 2, capi._dp(a), capi._dp(o), 2, off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       idx.ctypes.data_as(C.POINTER(C.c_uint32)), capi._dp(mean_only), None))  # var may be NULL
    assert np.array_equal(mean_only, dev.region_var(a, o, sets)[0])


def _raw_call(dev, a, o, off, idx):
    """hgibbs_region_var on offsets and indices as they stand (lists of millions of sets would take Device.region_var too long)"""
    C = capi.C
    nsets, S = len(off) - 1, a.shape[0]
    mean, var = np.zeros((nsets, S)), np.zeros((nsets, S))
    capi.check(dev.L.hgibbs_region_var(dev.h, S, capi._dp(a), capi._dp(o), nsets, off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       idx.ctypes.data_as(C.POINTER(C.c_uint32)), capi._dp(mean), capi._dp(var)))
    return mean, var


def _answers_like_the_score(dev, a, o, sets):
    """a valid call on the handle: mean and variance of hgibbs_score's values for each set's weights"""
    n = dev.n_local
    mean, var = dev.region_var(a, o, sets)
    for r, idx in enumerate(sets):
        am, om = np.zeros_like(a), np.zeros_like(o)
        am[:, idx], om[:, idx] = a[:, idx], o[:, idx]
        v = dev.score(am, om)
        mag = np.abs(v).max(axis=0)
        assert np.all(np.abs(mean[r] - v.mean(axis=0)) <= (n * EPS + 1e-12) * mag), r
        assert np.all(np.abs(var[r] - v.var(axis=0, ddof=1)) <= (2 * n * EPS + 1e-11) * mag ** 2) and np.any(var[r] > 0.0), r


def test_region_var_refuses_several_ranks():
    N, M = 400, 30
    geno = synth.make_genotypes(M, N, seed=6)
    calls = []

    def allreduce(arr):  # a stub world of two identical ranks
        calls.append(arr.size)
        arr *= 2

    dev = capi.Device(0)
    dev.comm_init_external(2, 0, allreduce)
    dev.load_bed(synth.pack_bed_columns(geno), N, row_begin=0, row_end=N // 2, n_global=N)
    a, o = weights(2, M, seed=3)
    before = len(calls)
    with pytest.raises(capi.HgError, match=r"hgibbs_region_var: one rank only \(this handle has 2\): the sums over the rows are taken in one fixed "
                                           r"order on one device"):
        dev.region_var(a, o, [np.arange(M)])
    assert len(calls) == before  # refused before the marker stats' collective
    # the handle still answers: the score takes any number of ranks
    ref = reference(geno[:, :N // 2], a, o, [np.arange(M)])[2]
    assert dev.score(a, o).shape == (N // 2, 2) and np.all(np.abs(dev.score(a, o)).max(axis=0) <= ref[0] * (1 + 1e-12))


def test_region_var_refuses_what_does_not_fit_in_device_memory():
    """The parts are nsets x row blocks x samples per pass x 16 bytes, for empty sets too: six million empty sets on 508 row blocks and
    eight samples need 390 GB, more than any device this library runs on holds (an MI355X has 288 GB); the host's share is 48 MB of
    offsets."""
    N, M, S = 130001, 8, 8
    dev = capi.Device(0)
    dev.synth_bed(N, M, seed=3, missing_rate=0.01)
    a, o = weights(S, M, seed=4)
    off = np.zeros(6_000_001, dtype=np.uint64)
    with pytest.raises(capi.HgError, match=r"hgibbs_region_var: 6000000 sets of 0 markers in all and 8 weight vectors need [0-9.]+ MiB of device memory, "
                                           r"[0-9.]+ MiB of device memory are free"):
        _raw_call(dev, a, o, off, np.zeros(1, dtype=np.uint32))
    _answers_like_the_score(dev, a, o, [np.arange(M), np.array([1, 6])])


def test_region_var_refuses_more_than_one_call_takes():
    """2^24 blocks of 64 list entries, and more workgroups than one launch: 2^24 - 1 one-marker sets on the 4 097 or more blocks of 256 rows
    that 2^20 + 1 rows are padded to"""
    N, M = 4096 * 256 + 1, 1
    dev = capi.Device(0)
    dev.synth_bed(N, M, seed=5)
    a, o = weights(1, M, seed=6)
    off = np.arange((1 << 24) + 1, dtype=np.uint64)
    idx = np.zeros(1 << 24, dtype=np.uint32)
    with pytest.raises(capi.HgError, match=r"the sets make 16777216 blocks of 64 markers, at most 2\^24 - 1 a call"):
        _raw_call(dev, a, o, off, idx)
    with pytest.raises(capi.HgError, match=r"16777215 sets on [0-9]+ blocks of 256 rows are more workgroups than one launch takes"):
        _raw_call(dev, a, o, off[:-1], idx)
    _answers_like_the_score(dev, a, o, [np.arange(M)])


# ---- the command line ----

def _table(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "SET CHR BP_FIRST BP_LAST NSNP PIP PVE_MEAN PVE_SD SHARE_MEAN SHARE_SD WPPA"
    return [ln.split() for ln in lines[1:]]


def _pve_bin(path):
    raw = open(path, "rb").read()
    R, S = np.frombuffer(raw[:8], np.uint32)
    return np.frombuffer(raw[8:], np.float64).reshape(R, S)


def test_cli_pve_end_to_end(tmp_path):
    N, M, iters, burn = 300, 240, 30, 10
    na = [3, 17]
    geno = synth.make_genotypes(M, N, seed=21, missing_rate=0.01)
    y, _ = synth.make_phenotype(geno, seed=22, causal_frac=0.1)
    prefix = str(tmp_path / "train")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=na)
    chrom = np.repeat([1, 2, 3], 80)
    bp = 1000 * (np.arange(M) % 80) + 17
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%d snp%d 0 %d A C\n" % (chrom[j], j, bp[j]))
    out = str(tmp_path / "out")
    base = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", out, "--mcmc-out-name", "r",
            "--number-individuals", str(N), "--number-markers", str(M), "--chain-length", str(iters), "--thin", "1", "--save", str(iters - 1),
            "--seed", "9"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    its, betas = _bet(out + "/r.bet", M)
    betas = betas[[k for k, it in enumerate(its) if it >= burn]]
    S = len(betas)
    assert S == iters - burn

    # the chain's standardisation over the kept rows, and every set's variance per record
    keep = np.ones(N, bool)
    keep[na] = False
    gk = geno[:, keep]
    nmk = gk != 3
    n = int(keep.sum())
    n1, n2 = (gk == 1).sum(1), (gk == 2).sum(1)
    mave = (n1 + 2.0 * n2) / nmk.sum(1)
    n0 = n - n1 - n2 - (~nmk).sum(1)
    mstd = np.sqrt((n - 1) / (n0 * mave ** 2 + n1 * (1 - mave) ** 2 + n2 * (2 - mave) ** 2))
    x = np.where(nmk, (gk - mave[:, None]) * mstd[:, None], 0.0)  # (M, n)

    def columns(sets):
        var = np.stack([(x[idx].T @ betas[:, idx].T).var(axis=0, ddof=1) if len(idx) else np.zeros(S) for idx in sets])
        share = np.where(var[-1] != 0.0, var / np.where(var[-1] != 0.0, var[-1], 1.0), 0.0)
        pip = [float(np.mean(np.any(betas[:, idx] != 0.0, axis=1))) for idx in sets]
        T = next(t for t in np.arange(0.15, 0.6, 0.01) if np.min(np.abs(share - t)) > 1e-6)  # no record's SHARE within 1e-6 of it
        return var, share, pip, float(T)

    def compare(rows, names, sets, var, share, pip, vbin, T):
        assert [row[0] for row in rows] == names + ["ALL"]
        assert vbin.shape == var.shape and np.allclose(vbin, var, rtol=1e-9, atol=0.0)
        wppa = np.mean(np.where(vbin[-1] != 0.0, vbin / np.where(vbin[-1] != 0.0, vbin[-1], 1.0), 0.0) > T, axis=1)
        for k, row in enumerate(rows):
            idx = sets[k]
            one = len(set(chrom[idx])) == 1
            assert row[1:4] == ([str(chrom[idx[0]]), str(bp[idx].min()), str(bp[idx].max())] if one else ["NA"] * 3), row
            assert int(row[4]) == len(idx)
            assert float(row[5]) == float("%.12g" % pip[k])
            want = [var[k].mean(), var[k].std(ddof=1), share[k].mean(), share[k].std(ddof=1)]
            assert np.allclose([float(v) for v in row[6:10]], want, rtol=1e-9, atol=0.0), (row, want)
            assert float(row[10]) == float("%.12g" % wppa[k])
        assert float(rows[-1][8]) == 1.0 and float(rows[-1][10]) == 1.0  # ALL: SHARE_MEAN and WPPA

    everything = np.arange(M)
    # windows of 50 markers within the runs of a chromosome: 50 + 30 in each
    wins = [np.arange(c * 80 + w0, c * 80 + min(w0 + 50, 80)) for c in range(3) for w0 in (0, 50)]
    names = ["%d:%d-%d" % (chrom[w[0]], w[0] + 1, w[-1] + 1) for w in wins]
    var, share, pip, T = columns(wins + [everything])
    r = subprocess.run(base + ["--burn-in", str(burn), "--pve", "--pve-window-snps", "50", "--pve-bin", "--pve-threshold", repr(T)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "PVE    : 6 sets (windows of 50 markers), 240 markers, 298 individuals, 20 records of" in r.stdout
    assert r.stdout.splitlines()[-1].startswith("PVE    : wrote 7 rows to %s/r.pve (" % out)
    compare(_table(out + "/r.pve"), names, wins + [everything], var, share, pip, _pve_bin(out + "/r.pve.bin"), T)

    # a sets file: a scattered set across the chromosomes, listed out of order, and a gene
    rng = np.random.default_rng(4)
    scattered = rng.permutation(np.arange(1, M, 9))
    gene = np.arange(90, 110)
    path = str(tmp_path / "sets.txt")
    with open(path, "w") as f:
        f.write("".join("far snp%d\n" % j for j in scattered[:10]) + "".join("gene snp%d\n" % j for j in gene)
                + "".join("far snp%d\n" % j for j in scattered[10:]))
    sets = [np.sort(scattered), gene, everything]
    var, share, pip, T = columns(sets)
    pout = str(tmp_path / "s.pve")
    r = subprocess.run(base + ["--burn-in", str(burn), "--pve", "--pve-sets", path, "--pve-bin", "--pve-out", pout, "--pve-threshold", repr(T)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    compare(_table(pout), ["far", "gene"], sets, var, share, pip, _pve_bin(pout + ".bin"), T)

    # no definer: one set per chromosome, and the default threshold 1 / 3
    r = subprocess.run(base + ["--burn-in", str(burn), "--pve", "--pve-out", pout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = _table(pout)
    assert [row[0] for row in rows] == ["chr1", "chr2", "chr3", "ALL"] and [row[4] for row in rows] == ["80", "80", "80", "240"]
    assert "threshold 0.333333" in r.stdout
