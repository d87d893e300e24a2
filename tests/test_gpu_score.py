"""Scoring a cohort (hgibbs_score, hydra_mi355x --predict-bfile) against NumPy in f64 and against the chain's own state."""
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import capi, synth
from test_gpu_marker_dots import exact_sum, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")

pytestmark = pytest.mark.gpu


def reference(geno, a, o, rows=8192):
    """out[i, s] = sum_j [g_ij != 3] (a_sj g_ij + o_sj), and sum_j |term| per entry (the tolerance's scale); in slices of individuals"""
    N = geno.shape[1]
    ref = np.zeros((N, a.shape[0]))
    mag = np.zeros_like(ref)
    for i0 in range(0, N, rows):
        gs = geno[:, i0:i0 + rows]
        nm = (gs != 3).astype(np.float64)  # (M, n)
        g = np.where(gs == 3, 0, gs).astype(np.float64)
        ref[i0:i0 + rows] = g.T @ a.T + nm.T @ o.T
        for s in range(a.shape[0]):
            mag[i0:i0 + rows, s] = (np.abs(g * a[s][:, None] + o[s][:, None]) * nm).sum(axis=0)
    return ref, mag


def quantise_weights(a, o):
    """hg_score.hip.h's fixed point: E_s = 52 - e with max_j max(|a_sj|, |o_sj|) < 2^e (frexp; 0 for an all-zero sample), q = rint(w 2^E_s)
    as int64 (|q| <= 2^52)"""
    E = np.zeros(a.shape[0], dtype=np.int64)
    for s in range(a.shape[0]):
        m = max(np.max(np.abs(a[s])), np.max(np.abs(o[s]))) if a.shape[1] else 0.0
        E[s] = 52 - np.frexp(m)[1] if m > 0 else 0
    qa = np.rint(np.ldexp(a, E[:, None])).astype(np.int64)
    qo = np.rint(np.ldexp(o, E[:, None])).astype(np.int64)
    return E, qa, qo


def signed_digits(q):
    """the seven signed base-256 digits of q (int64, |q| < 2^54) as sc_digit gives them: (..., 7) int64, digits 0..5 in [-128, 127],
    sum_d digit_d 256^d = q"""
    y = q.astype(np.int64) + 0x0000808080808080
    d = np.stack([(y >> (8 * k)) & 0xFF for k in range(7)], axis=-1)
    d[..., :6] ^= 0x80
    return np.where(d >= 128, d - 256, d)


def drop_lowest_digit(q):
    """q without its lowest signed base-256 digit"""
    return q - signed_digits(q)[..., 0]


def restate_from_q(geno, E, qa, qo):
    """out[i, s] = float(T_is) 2^-E_s with the exact integer T_is = sum_j [g_ij != 3] (qa_sj g_ij + qo_sj): Python's int -> float rounds
    once and correctly (to nearest, ties to even), as round_halves does on the device; the power of two is exact"""
    g = np.where(geno == 3, 0, geno).astype(np.float64).T  # (N, M)
    called = (geno != 3).astype(np.float64).T
    T = exact_sum(g, qa) + exact_sum(called, qo)
    to_f = np.vectorize(float, otypes=[np.float64])
    return np.ldexp(to_f(T), -E[None, :]) if T.size else np.zeros(T.shape)


def restate(geno, a, o):
    """hgibbs_score as hg_score.hip.h documents it, in integers: what the device must return bit for bit"""
    return restate_from_q(geno, *quantise_weights(a, o))


def bound(a, o, M, mag):
    """the operator's own bound, 3 M max_j |w_sj| 2^-52 per entry of sample s, plus the summation error of the plain f64 reference,
    M 2^-53 times the sum of the |terms|; never above the 1e-12 mag these tests held before (at M = 20 000 the second term alone is
    2.2e-12 mag).  Measured on the CPU with the integer restatement in the device's place, |restatement - f64 reference| is at most
    0.042 of this at (130001, 200), 8.2e-4 at (130001, 3000) and 1.1e-4 at (63, 20000): the plain f64 reference fits under it."""
    wmax = np.maximum(np.abs(a).max(axis=1), np.abs(o).max(axis=1))
    return np.minimum(3.0 * M * wmax[None, :] * 2.0 ** -52 + M * 2.0 ** -53 * mag, 1e-12 * mag)


def digit_samples(M, anchor, seed, used=None):
    """Seven samples, sample d with every quantised weight in digit d alone: a_j = kappa_j 256^d 2^-40, o_j = lambda_j 256^d 2^-40 with
    integers kappa, lambda in [-127, 127] for d < 6 and in [-15, 15] for d = 6 (zero outside `used` when that is given), and a = 2^11,
    o = 0 at the anchor marker, whose column is all code 0.  The anchor adds a 0 = 0 to every score and keeps the largest weight of
    every sample, and of every set that holds it, in [2^11, 2^12): 127 x 256^5 2^-40 < 2^7 and 15 x 256^6 2^-40 = 3840 < 2^12.  So
    E = 40 and q_a = kappa 256^d, |q| < 2^52, sits in digit d and nowhere else (tests/test_score_restatement_cpu.py checks this
    premise).  Returns a, o (7, M) and the integers kappa, lambda (7, M), zero at the anchor."""
    rng = np.random.default_rng(seed)
    kappa = rng.integers(-127, 128, size=(7, M))
    lam = rng.integers(-127, 128, size=(7, M))
    kappa[6] = rng.integers(-15, 16, size=M)
    lam[6] = rng.integers(-15, 16, size=M)
    if used is not None:
        off = np.ones(M, bool)
        off[used] = False
        kappa[:, off] = 0
        lam[:, off] = 0
    kappa[:, anchor] = 0
    lam[:, anchor] = 0
    unit = np.ldexp(1.0, 8 * np.arange(7) - 40)[:, None]
    a, o = kappa * unit, lam * unit
    a[:, anchor] = 2.0 ** 11
    return a, o, kappa, lam


def weights(S, M, seed):
    """magnitudes 1e-8 and 1e3 mixed within a sample, one all-zero sample (the second) when S > 1"""
    rng = np.random.default_rng(seed)
    big = rng.random((S, M)) < 0.3
    a = rng.standard_normal((S, M)) * np.where(big, 1e3, 1e-8)
    o = -a * rng.uniform(0.02, 1.98, size=(S, M))
    if S > 1:
        a[1] = 0.0
        o[1] = 0.0
    return a, o


def load(N, M, missing, seed):
    geno = synth.make_genotypes(M, N, seed=seed, missing_rate=missing) if N > 1 else np.random.default_rng(seed).integers(0, 3, (M, 1)).astype(np.uint8)
    if missing:
        geno[M // 2, :] = 3  # an all-missing column
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N, n_global=max(N, 2))
    return dev, geno


@pytest.mark.parametrize("N", [1, 63, 4097, 130001])
@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_score_matches_numpy(N, missing):
    M = 200
    dev, geno = load(N, M, missing, seed=N + 7)
    assert np.array_equal(synth.unpack_bed_columns(dev.get_bed(), N), geno)
    for S in (1, 2, 7, 16, 33):
        a, o = weights(S, M, seed=S)
        out = dev.score(a, o)
        ref, mag = reference(geno, a, o)
        assert out.shape == (N, S)
        err, tol = np.abs(out - ref), bound(a, o, M, mag)
        assert np.all(err <= tol), (S, float(np.max(err / np.maximum(tol, 1e-300))))
        if S > 1:
            assert np.all(out[:, 1] == 0.0)  # the all-zero sample


@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_score_is_bit_identical_across_launches_and_chunkings(missing):
    N, M, S = 4097, 700, 33
    dev, geno = load(N, M, missing, seed=3)
    a, o = weights(S, M, seed=11)
    first = dev.score(a, o)
    assert np.array_equal(first, dev.score(a, o))
    chunked = np.concatenate([dev.score(a[:5], o[:5]), dev.score(a[5:], o[5:])], axis=1)
    assert np.array_equal(first, chunked)
    one_by_one = np.concatenate([dev.score(a[s:s + 1], o[s:s + 1]) for s in range(0, S, 8)], axis=1)
    assert np.array_equal(first[:, ::8], one_by_one)
    for sp in (2, 4, 8, 16):
        dev.set_option("score_sp", sp)
        assert np.array_equal(first, dev.score(a, o)), sp
    dev.set_option("score_sp", 0)


GRID_N = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513]
GRID_M = [1, 63, 64, 65, 129]
GRID_S = [1, 2, 3, 8, 9, 17]


def assert_bits(out, ref, what):
    """the device's f64 bit patterns equal the restatement's; the largest |device - restatement| is printed first"""
    diff = float(np.max(np.abs(out - ref))) if out.size else 0.0
    print(what, "largest |device - restatement| =", diff)
    assert same_bits(out, ref), (what, diff, int(np.count_nonzero(out != ref)))


@pytest.mark.parametrize("N", GRID_N)
@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_score_bits_on_the_edge_grid(N, missing):
    """Bit for bit against the integer restatement where masks and tails live: rows below, at and next to the 16 of a product, the 64 of
    a wave and the 256 of a workgroup; markers of one block of 64 or less and next to one and two; sample counts at and next to every pass
    size.  One restatement per (N, M) for all the weight vectors: a sample's scale is its own."""
    for M in GRID_M:
        dev, geno = load(N, M, missing, seed=N + M)
        ws = [weights(S, M, seed=S + M) for S in GRID_S]
        ref = restate(geno, np.concatenate([w[0] for w in ws]), np.concatenate([w[1] for w in ws]))
        at = 0
        for S, (a, o) in zip(GRID_S, ws):
            assert_bits(dev.score(a, o), ref[:, at:at + S], (N, M, S, missing))
            at += S
        dev.close()


@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_score_bits_under_every_pass_size_and_range_count(missing):
    N, M, S = 4097, 700, 33
    dev, geno = load(N, M, missing, seed=3)
    a, o = weights(S, M, seed=11)
    ref = restate(geno, a, o)
    assert_bits(dev.score(a, o), ref, "automatic")
    for ranges in (1, 7):
        dev.set_option("score_ranges", ranges)
        for sp in (2, 4, 8, 16):
            dev.set_option("score_sp", sp)
            assert_bits(dev.score(a, o), ref, ("score_ranges", ranges, "score_sp", sp))
    dev.set_option("score_ranges", 0)
    dev.set_option("score_sp", 0)


@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_score_bits_of_every_digit_on_its_own(missing):
    """digit_samples: sample d has every quantised weight in base-256 digit d alone, so a kernel that drops, misplaces or mis-signs one
    digit position changes that sample and no other"""
    N, M, anchor = 257, 200, 100
    geno = synth.make_genotypes(M, N, seed=31, missing_rate=missing)
    geno[anchor] = 0
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    a, o, _, _ = digit_samples(M, anchor, seed=5)
    ref = restate(geno, a, o)
    assert np.all(np.any(ref != 0.0, axis=0))
    for sp in (0, 2, 4, 8, 16):
        dev.set_option("score_sp", sp)
        assert_bits(dev.score(a, o), ref, ("digits", missing, "score_sp", sp))
    dev.set_option("score_sp", 0)


@pytest.mark.parametrize("N,M", [(63, 20000), (130001, 3000)])
def test_score_many_marker_blocks_per_workgroup(N, M):
    """Workgroups that go through many 64-marker blocks (the steady state of the kernel's loop: the next block's codes and operands
    loaded while this one's products run, the LDS double buffer, the accumulators over blocks).  Automatic grid on 256 compute units:
    3 blocks per workgroup at (63, 20000), 12 at (130001, 3000); score_ranges = 1 gives every workgroup ALL the blocks (313, 47).
    Blocks with missing calls sit between clean ones: in every third block of 64 markers, one column all missing."""
    geno = synth.make_genotypes(M, N, seed=N + M, missing_rate=0.02)
    clean = (np.arange(M) // 64) % 3 != 1
    geno[clean] = np.where(geno[clean] == 3, 0, geno[clean])
    geno[64 * 4 + 5, :] = 3
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N, n_global=max(N, 2))
    for S in (7, 16):
        a, o = weights(S, M, seed=S + 1)
        ref, mag = reference(geno, a, o)
        auto = dev.score(a, o)
        err, tol = np.abs(auto - ref), bound(a, o, M, mag)
        assert np.all(err <= tol), (S, float(np.max(err / np.maximum(tol, 1e-300))))
        for ranges, sp in ((1, 0), (1, 2), (2, 16), (7, 4)):
            dev.set_option("score_ranges", ranges)
            dev.set_option("score_sp", sp)
            assert np.array_equal(auto, dev.score(a, o)), (S, ranges, sp)
        dev.set_option("score_ranges", 0)
        dev.set_option("score_sp", 0)


def test_score_refusals():
    dev = capi.Device(0)
    with pytest.raises(capi.HgError, match="no genotypes"):
        capi.check(dev.L.hgibbs_score(dev.h, 1, None, None, None))
    dev.close()
    dev, _ = load(100, 70, 0.0, seed=1)
    a, o = weights(2, 70, seed=2)
    with pytest.raises(capi.HgError, match="at least one"):
        dev.score(a[:0], o[:0])
    a[1, 5] = np.nan
    with pytest.raises(capi.HgError, match="not finite"):
        dev.score(a, o)
    a[1, 5] = 0.0
    o[0, 3] = np.inf
    with pytest.raises(capi.HgError, match="not finite"):
        dev.score(a, o)


# ---- the command line ----

def _chain(tmp_path, N, M, iters, na_rows, missing=0.01):
    geno = synth.make_genotypes(M, N, seed=21, missing_rate=missing)
    y, _ = synth.make_phenotype(geno, seed=22, causal_frac=0.1)
    prefix = str(tmp_path / "train")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=na_rows)
    out = str(tmp_path / "out")
    base = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", out, "--mcmc-out-name", "r",
            "--number-individuals", str(N), "--number-markers", str(M), "--chain-length", str(iters), "--thin", "1",
            "--save", str(iters - 1), "--seed", "9"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return geno, y, prefix, out, base


def _bet(path, M):
    raw = open(path, "rb").read()
    assert np.frombuffer(raw[:4], np.uint32)[0] == M
    rec = 4 + 8 * M
    n = (len(raw) - 4) // rec
    its = [int(np.frombuffer(raw[4 + k * rec:8 + k * rec], np.uint32)[0]) for k in range(n)]
    betas = np.stack([np.frombuffer(raw[8 + k * rec:4 + (k + 1) * rec], np.float64) for k in range(n)])
    return its, betas


def _prs_bin(path):
    raw = open(path, "rb").read()
    n, S = np.frombuffer(raw[:8], np.uint32)
    return np.frombuffer(raw[8:], np.float64).reshape(n, S)


def test_cli_residual_identity(tmp_path):
    """mu + score + eps = the chain's centred and scaled y on every kept row, at the saved iteration"""
    N, M, iters = 3000, 400, 6
    na = [3, 17, 400, 2999]
    geno, y, prefix, out, base = _chain(tmp_path, N, M, iters, na)
    last = iters - 1
    r = subprocess.run(base + ["--burn-in", str(last), "--predict-bfile", prefix], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "400 target markers: 400 matched (400 same alleles, 0 swapped)" in r.stdout
    score = _prs_bin(out + "/r.prs.bin")
    assert score.shape == (N, 1)
    keep = np.ones(N, bool)
    keep[na] = False
    raw = open(out + "/r.eps.0", "rb").read()
    it, nloc = np.frombuffer(raw[:8], np.uint32)
    assert it == last and nloc == keep.sum()
    eps = np.frombuffer(raw[8:], np.float64)
    mus = np.frombuffer(open(out + "/r.mus.0", "rb").read(), dtype=[("it", np.uint32), ("mu", np.float64)])
    mu = float(mus["mu"][list(mus["it"]).index(last)])
    yk = y[keep].astype(np.float64)
    yk = yk - yk.sum() / len(yk)
    yk = yk * np.sqrt((len(yk) - 1) / np.sum(yk * yk))
    assert np.max(np.abs(mu + score[keep, 0] + eps - yk)) <= 1e-9
    lines = open(out + "/r.prs").read().splitlines()
    assert lines[0] == "FID IID mean sd" and len(lines) == N + 1
    f, i, m, sd = lines[5].split()
    assert (f, i) == ("fam4", "ind4") and float(m) == score[4, 0] and float(sd) == 0.0


def test_cli_target_with_permuted_swapped_and_dropped_markers(tmp_path):
    N, M, iters = 2000, 300, 5
    na = [0, 50]
    geno, y, prefix, out, base = _chain(tmp_path, N, M, iters, na)
    its, betas = _bet(out + "/r.bet", M)
    burn = 2
    betas = betas[[k for k, it in enumerate(its) if it >= burn]]
    # the chain's standardisation, over the kept rows
    keep = np.ones(N, bool)
    keep[na] = False
    gk = geno[:, keep]
    nmk = gk != 3
    n1, n2 = (gk == 1).sum(1), (gk == 2).sum(1)
    mave = (n1 + 2.0 * n2) / nmk.sum(1)
    n0 = keep.sum() - n1 - n2 - (~nmk).sum(1)
    mstd = np.sqrt((keep.sum() - 1) / (n0 * mave ** 2 + n1 * (1 - mave) ** 2 + n2 * (2 - mave) ** 2))
    # target: 700 new individuals, markers permuted, every 5th swapped, every 7th dropped, two foreign ids, one allele mismatch
    rng = np.random.default_rng(5)
    NT = 700
    tgeno_train = synth.make_genotypes(M, NT, seed=33, missing_rate=0.02)
    order = [j for j in rng.permutation(M) if j % 7 != 3]
    rows, bim = [], []
    for t, j in enumerate(order):
        g = tgeno_train[j].copy()
        if t % 5 == 0:  # swapped alleles: the file counts the other allele
            g = np.where(g == 3, 3, 2 - g)
            bim.append("1 snp%d 0 %d C A" % (j, j + 1))
        elif t == 1:
            bim.append("1 snp%d 0 %d A G" % (j, j + 1))
        else:
            bim.append("1 snp%d 0 %d A C" % (j, j + 1))
        rows.append(g)
    for k in range(2):
        rows.append(rng.integers(0, 3, NT).astype(np.uint8))
        bim.append("1 foreign%d 0 1 A C" % k)
    tgeno = np.stack(rows)
    tprefix = str(tmp_path / "target")
    synth.write_plink(tprefix, synth.pack_bed_columns(tgeno), NT)
    with open(tprefix + ".bim", "w") as f:
        f.write("\n".join(bim) + "\n")
    r = subprocess.run(base + ["--burn-in", str(burn), "--predict-bfile", tprefix, "--predict-out", str(tmp_path / "t.prs")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    nsw = len(range(0, len(order), 5))
    assert "%d target markers: %d matched (%d same alleles, %d swapped), 1 allele mismatch, 2 not in training" % (
        len(order) + 2, len(order) - 1, len(order) - 1 - nsw, nsw) in r.stdout
    got = _prs_bin(str(tmp_path / "t.prs.bin"))
    # NumPy: the training-oriented genotype of each matched target column, standardised with the chain's mave / mstd
    ref = np.zeros((NT, len(betas)))
    mag = np.zeros((NT, len(betas)))
    for t, j in enumerate(order):
        if t == 1:
            continue
        g = tgeno[t].astype(np.float64)
        nm = tgeno[t] != 3
        if t % 5 == 0:
            g = 2.0 - g
        x = np.where(nm, (g - mave[j]) * mstd[j], 0.0)
        ref += np.outer(x, betas[:, j])
        mag += np.abs(np.outer(x, betas[:, j]))
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= 1e-12 * mag + 1e-15)
    lines = open(str(tmp_path / "t.prs")).read().splitlines()
    vals = np.array([[float(v) for v in ln.split()[2:]] for ln in lines[1:]])
    assert np.allclose(vals[:, 0], got.mean(1), rtol=1e-12, atol=1e-15)
    assert np.allclose(vals[:, 1], got.std(1, ddof=1), rtol=1e-9, atol=1e-15)
