"""KING-robust kinship (hgibbs_king, hgibbs_king_pairs, hydra_mi355x --king) against NumPy: the exact counts, their symmetry, bit
identity across chunkings and tuning, the filtered list (grown inside the call), a planted pedigree and the CLI's .kin0 table."""
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")

pytestmark = pytest.mark.gpu


def forms(geno):
    """(N, M) float64 indicator matrices of the individuals: called, het, hom 0, hom 2"""
    g = np.ascontiguousarray(geno.T)
    return [(g != 3).astype(np.float64), (g == 1).astype(np.float64), (g == 0).astype(np.float64), (g == 2).astype(np.float64)]


def reference(geno, a0, acount, b0, bcount):
    """(acount, bcount, 5) int64: NSNP, HET_a, HET_b, HETHET, IBS0 (f64 products of 0/1 indicators: exact below 2^53)"""
    c, h, p0, p2 = forms(geno)
    A, B = slice(a0, a0 + acount), slice(b0, b0 + bcount)
    out = np.stack([c[A] @ c[B].T, h[A] @ c[B].T, c[A] @ h[B].T, h[A] @ h[B].T, p0[A] @ p2[B].T + p2[A] @ p0[B].T], axis=-1)
    return out.astype(np.int64)


def kinship(k):
    """the f64 formula on counts (..., 5); NaN where min(HET_a, HET_b) = 0"""
    k = np.asarray(k, dtype=np.int64)
    mn = np.minimum(k[..., 1], k[..., 2])
    num = 4 * k[..., 4] + (k[..., 1] - k[..., 3]) + (k[..., 2] - k[..., 3])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(mn > 0, 0.5 - num / (4 * mn), np.nan)


def make(N, M, seed):
    geno = synth.make_genotypes(M, N, seed=seed)
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
    dev.load_bed(synth.pack_bed_columns(geno), N)
    return dev


def check_block(dev, geno, a0, acount, b0, bcount):
    got = dev.king(a0, acount, b0, bcount)
    want = reference(geno, a0, acount, b0, bcount)
    assert got.shape == want.shape
    assert np.array_equal(got.astype(np.int64), want), "block [%d, +%d) x [%d, +%d) differs" % (a0, acount, b0, bcount)
    return got


@pytest.mark.parametrize("M", [1, 63, 64, 65, 2049])
@pytest.mark.parametrize("N", [2, 15, 16, 17, 63, 65, 511, 513, 4097])
def test_counts_match_numpy(N, M):
    geno = make(N, M, seed=N * 7 + M)
    dev = device(geno)
    if N <= 513:
        full = check_block(dev, geno, 0, N, 0, N)
        # counts(a, b) = counts(b, a) with the HET pair swapped; on the diagonal HETHET = HET_a = HET_b
        sw = full.transpose(1, 0, 2)[..., [0, 2, 1, 3, 4]]
        assert np.array_equal(full, sw)
        d = full[np.arange(N), np.arange(N)]
        assert np.array_equal(d[:, 1], d[:, 3]) and np.array_equal(d[:, 2], d[:, 3])
    else:
        check_block(dev, geno, N - 100, 100, N - 100, 100)
    # blocks whose offsets are not multiples of 16, the diagonal inside them
    a0 = min(N - 1, 3)
    b0 = N // 3
    check_block(dev, geno, a0, min(N - a0, 37), b0, N - b0)
    check_block(dev, geno, b0, N - b0, a0, min(N - a0, 19))
    if N >= 40:
        check_block(dev, geno, 5, N - 5 - 11, 1, N - 1 - 3)


def test_bit_identical_across_chunkings_and_split():
    N, M = 700, 2049
    geno = make(N, M, seed=5)
    dev = device(geno)
    ref = dev.king()
    assert np.array_equal(ref.astype(np.int64), reference(geno, 0, N, 0, N))
    for split in (1, 2, 3, 7, 33, 0):
        dev.set_option("king_split", split)
        assert np.array_equal(dev.king(), ref), "king_split=%d" % split
    for step in (1, 37, 128, 129):
        parts = np.concatenate([dev.king(a0, min(step, N - a0), 0, N) for a0 in range(0, N, step)])
        assert np.array_equal(parts, ref), "row pieces of %d" % step
    assert np.array_equal(np.concatenate([dev.king(0, N, b0, min(200, N - b0)) for b0 in range(0, N, 200)], axis=1), ref)
    assert dev.last_king_ms() > 0.0
    # the filtered list does not depend on the option either, and matches the blocks
    dev.set_option("king_split", 5)
    ab, cnt, kin = dev.king_pairs(0.0)
    dev.set_option("king_split", 0)
    ab2, cnt2, kin2 = dev.king_pairs(0.0)
    assert np.array_equal(ab, ab2) and np.array_equal(cnt, cnt2) and np.array_equal(kin.view(np.int64), kin2.view(np.int64))
    assert np.array_equal(cnt, ref[ab[:, 0], ab[:, 1]])


def test_rectangle_in_several_pieces():
    """a rectangle of more than 2^25 pairs is computed in pieces of rows (the second one starting off a tile boundary)"""
    N, M = 6001, 65
    geno = make(N, M, seed=29)
    dev = device(geno)
    a0, b0 = 3, 1
    acount, bcount = N - a0, N - b0
    assert acount * bcount > (1 << 25) and (a0 + (1 << 25) // bcount) % 16 != 0
    got = dev.king(a0, acount, b0, bcount)
    for r0 in range(0, acount, 1000):
        r1 = min(acount, r0 + 1000)
        assert np.array_equal(got[r0:r1].astype(np.int64), reference(geno, a0 + r0, r1 - r0, b0, bcount)), "rows %d .. %d" % (r0, r1)


def test_triangle_beyond_a_one_dimensional_grid():
    """600 000 rows: 4 688 blocks of 128 rows, 11 M block pairs of 512 threads, more work-items than a u32 holds in one dimension"""
    N, M = 600000, 1024
    rng = np.random.default_rng(31)
    # codes 0, 1, 2 a third each and no missing call: KINSHIP is about -0.5 between distinct rows and exactly 0.5 for a duplicate
    geno = rng.integers(0, 3, size=(M, N), dtype=np.uint8)
    dups = [(0, N - 1), (524159, 524160), (300001, 599998), (17, 131072)]
    for a, b in dups:
        geno[:, b] = geno[:, a]
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    ab, cnt, kin = dev.king_pairs(0.25)
    want = sorted(dups)
    assert [tuple(int(x) for x in r) for r in ab] == want
    assert np.all(kin == 0.5)
    for (a, b), k in zip(want, cnt):
        assert np.array_equal(k.astype(np.int64), reference(geno[:, [a, b]], 0, 1, 1, 1)[0, 0])


def reference_list(geno, cutoff):
    N = geno.shape[1]
    full = reference(geno, 0, N, 0, N)
    kin = kinship(full)
    a, b = np.triu_indices(N, 1)
    sel = kin[a, b] >= cutoff
    return np.stack([a[sel], b[sel]], axis=1), full[a[sel], b[sel]], kin[a[sel], b[sel]]


@pytest.mark.parametrize("cutoff", [0.0442, 0.0, -0.05])
def test_filtered_list_matches_numpy(cutoff):
    N, M = 900, 3000
    geno = make(N, M, seed=11)
    rng = np.random.default_rng(3)
    for i in range(10, 40, 2):  # close relatives: half the markers shared
        share = rng.random(M) < 0.5
        geno[share, i + 1] = geno[share, i]
    dev = device(geno)
    ab, cnt, kin = dev.king_pairs(cutoff)
    wab, wcnt, wkin = reference_list(geno, cutoff)
    assert len(wab) > 10
    assert np.array_equal(ab.astype(np.int64), wab) and np.array_equal(cnt.astype(np.int64), wcnt)
    assert np.all(np.abs(kin - wkin) <= np.spacing(np.abs(wkin)))


def test_list_grows_inside_the_call():
    N, M = 3000, 300
    geno = make(N, M, seed=17)
    dev = device(geno)
    ab, cnt, kin = dev.king_pairs(-1.0)
    assert len(ab) > (1 << 20)  # beyond the list's first capacity
    full = dev.king()
    kf = kinship(full)
    a, b = np.triu_indices(N, 1)
    sel = kf[a, b] >= -1.0
    assert np.array_equal(ab.astype(np.int64), np.stack([a[sel], b[sel]], axis=1))
    assert np.array_equal(cnt, full[a[sel], b[sel]])
    assert np.all(np.abs(kin - kf[a[sel], b[sel]]) <= np.spacing(np.abs(kf[a[sel], b[sel]])))
    assert np.array_equal(full.astype(np.int64)[:64, :64], reference(geno, 0, 64, 0, 64))


def test_planted_pedigree():
    M = 20000
    rng = np.random.default_rng(2024)
    p = rng.uniform(0.05, 0.5, size=M)
    hap = []  # (2, M) allele pairs per individual

    def founder():
        hap.append((rng.random((2, M)) < p).astype(np.uint8))
        return len(hap) - 1

    def child(f, m):
        gam = [hap[x][rng.integers(0, 2, size=M), np.arange(M)] for x in (f, m)]  # one allele of each parent, unlinked markers
        hap.append(np.stack(gam))
        return len(hap) - 1

    unrel = [founder() for _ in range(40)]
    p1, p2, p3, u1, u2 = (founder() for _ in range(5))
    c1, c2 = child(p1, p2), child(p1, p2)  # full sibs, offspring of p1 and p2
    h = child(p1, p3)  # half sib of c1 and c2
    g1, g2 = child(c1, u1), child(c2, u2)  # first cousins
    hap.append(hap[unrel[0]].copy())  # a duplicate
    dup = len(hap) - 1
    geno = np.stack([x.sum(axis=0) for x in hap], axis=1).astype(np.uint8)  # (M, N)
    geno[rng.random(geno.shape) < 0.01] = 3
    dev = device(geno)
    ab, cnt, kin = dev.king_pairs(-1.0)
    K = {(int(a), int(b)): v for (a, b), v in zip(ab, kin)}

    def k(a, b):
        return K[(min(a, b), max(a, b))]

    for a, b, want in [(p1, c1, 0.25), (p2, c2, 0.25), (c1, c2, 0.25), (c1, h, 0.125), (c2, h, 0.125), (g1, g2, 0.0625),
                       (unrel[0], dup, 0.5)]:
        assert abs(k(a, b) - want) <= 0.02, (a, b, k(a, b), want)
    # unrelated: the founders of the pedigree, and the 741 pairs of the other founders (whose largest |KINSHIP| is about three
    # standard deviations, 0.006 each at this M, so one or two may pass 0.02)
    for a, b in [(p1, p2), (p1, p3), (p2, p3), (u1, u2), (c1, u1), (p3, c2), (g1, p3)]:
        assert abs(k(a, b)) <= 0.02, (a, b, k(a, b))
    vals = np.abs([k(a, b) for i, a in enumerate(unrel[1:]) for b in unrel[i + 2:]])
    assert vals.mean() <= 0.01 and np.percentile(vals, 99) <= 0.02
    wab, wcnt, wkin = reference_list(geno, -1.0)
    assert np.array_equal(ab.astype(np.int64), wab) and np.array_equal(cnt.astype(np.int64), wcnt)


def test_refusals():
    geno = make(40, 70, seed=1)
    dev = device(geno)
    for args in [(39, 2, 0, 1), (0, 1, 40, 1), (0, 41, 0, 1)]:
        with pytest.raises(capi.HgError, match="out of range"):
            dev.king(*args)
    for c in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(capi.HgError, match="finite"):
            dev.king_pairs(c)
    with pytest.raises(capi.HgError, match="king_split"):
        dev.set_option("king_split", -1)
    empty = capi.Device(0)
    with pytest.raises(capi.HgError, match="no genotypes"):
        empty.king_pairs(0.0)


def test_cli_kin0(tmp_path):
    N, M = 300, 800
    geno = make(N, M, seed=23)
    rng = np.random.default_rng(5)
    for i in range(20, 60, 2):
        share = rng.random(M) < rng.uniform(0.2, 0.9)
        geno[share, i + 1] = geno[share, i]
    y = np.random.default_rng(4).standard_normal(N)
    na = [3, 21, 50, 51, 299]
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=na)
    kept = np.setdiff1d(np.arange(N), na)
    base = [EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"),
            "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(M), "--king"]
    for extra, path, cutoff in [([], str(tmp_path / "o" / "n.kin0"), 0.0442),
                                (["--king-cutoff", "-0.02", "--king-out", str(tmp_path / "t.kin0")], str(tmp_path / "t.kin0"), -0.02)]:
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        wab, wcnt, wkin = reference_list(geno[:, kept], cutoff)
        want = ["#FID1\tIID1\tFID2\tIID2\tNSNP\tHETHET\tIBS0\tKINSHIP"]
        for (a, b), k, v in zip(wab, wcnt, wkin):
            ia, ib = kept[a], kept[b]
            want.append("fam%d\tind%d\tfam%d\tind%d\t%d\t%.12g\t%.12g\t%.12g" % (ia, ia, ib, ib, k[0], k[3] / k[0], k[4] / k[0], v))
        with open(path) as f:
            got = f.read().splitlines()
        assert len(want) > 5
        assert got == want
        assert "KING   : %d pairs tested, %d with KINSHIP >= %g written to %s" % (len(kept) * (len(kept) - 1) // 2, len(wab), cutoff, path) \
            in r.stdout
