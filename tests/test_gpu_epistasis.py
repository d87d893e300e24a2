"""hgibbs_epi_scan, hgibbs_epi_test and hydra_mi355x --epistasis against the restatement of tests/epi_restate.py on a cohort with a planted
interaction (N = 600, M = 40, 2 % missing calls) and a clean second one (N = 1000, M = 64).  The thresholds are chosen so that the
restatement alone puts no pair's KSA within 2 delta of one (tests/test_epi_restatement_cpu.py asserts it for these seeds): the device's
list then equals the restated set {KSA >= T} exactly, table for table."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import capi, synth

import epi_restate as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")


@functools.lru_cache(maxsize=None)
def case(name):
    geno, cls = E.planted_case() if name == "planted" else E.second_case()
    ab, t = E.triangle(geno, cls)
    r = E.epi_test(t)
    for a in (geno, cls, ab, t):
        a.setflags(write=False)
    return geno, cls, ab, t, r


def device(geno):
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), geno.shape[1])
    return dev


@pytest.fixture(scope="module")
def planted():
    dev = device(case("planted")[0])
    yield dev
    dev.close()


def check_list(got, name, T):
    """the device's list against the restated set {KSA >= T}: pairs, tables, values; then hgibbs_epi_test on every listed pair"""
    geno, cls, ab, t, r = case(name)
    assert float(np.min(np.abs(r["ksa"] - T))) > 2 * E.delta(geno.shape[1])  # the condition
    keep = r["ksa"] >= T
    gab, gt, gk = got
    assert np.array_equal(gab, ab[keep])
    assert np.array_equal(gt, t[keep])
    worst = float(np.max(np.abs(gk - r["ksa"][keep]) / r["ksa_scale"][keep])) if keep.any() else 0.0
    print("%s, T = %g: %d pairs listed; the device's KSA differs from the restatement by %.3g of the terms" % (name, T, int(keep.sum()), worst))
    assert worst <= 10 * E.KSA_F64_LD
    kept = []
    for p, i in enumerate(np.flatnonzero(keep)):
        c = capi.epi_test(gt[p])
        assert (c.df, c.iters, c.converged) == (r["df"][i], r["iters"][i], r["converged"][i])
        assert abs(c.lr - r["lr"][i]) <= 10 * E.LR_F64_LD * r["lr_scale"][i]
        assert abs(c.ksa - r["ksa"][i]) <= 10 * E.KSA_F64_LD * r["ksa_scale"][i]
        if c.lr >= T and c.df > 0:
            kept.append(tuple(gab[p]))
    assert kept == [tuple(x) for x in ab[(r["lr"] >= T) & (r["df"] > 0)]]
    return kept


@pytest.mark.parametrize("T", E.T_PLANTED)
def test_planted_case(planted, T):
    geno, cls, ab, t, r = case("planted")
    idx = np.arange(geno.shape[0])
    got = planted.epi_scan(idx, None, cls, T)
    kept = check_list(got, "planted", T)
    assert E.PLANTED in kept
    if T == 30.0:
        assert kept == [E.PLANTED]
    pm, sm = planted.last_epi_ms()
    assert pm > 0.0 and sm > 0.0


def same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y)) and np.array_equal(x[2].view(np.int64), y[2].view(np.int64))


def test_overflow_split_blocks_and_repeats_give_the_same_list(planted):
    geno, cls, ab, t, r = case("planted")
    idx = np.arange(geno.shape[0])
    T = E.T_PLANTED[1]
    first = planted.epi_scan(idx, None, cls, T)
    assert first[0].shape[0] > 1
    assert same(planted.epi_scan(idx, None, cls, T), first)
    for option, value in (("epi_list0", 1), ("ptab_split", 2), ("epi_block", 32)):
        planted.set_option(option, value)  # epi_list0 = 1: the list overflows and the scan runs a second time
        assert same(planted.epi_scan(idx, None, cls, T), first), option
        planted.set_option(option, 0)


def test_rectangular_scan_against_the_triangle(planted):
    geno, cls, ab, t, r = case("planted")
    idx = np.arange(geno.shape[0])
    T = E.T_PLANTED[1]
    tri = planted.epi_scan(idx, None, cls, T)
    A, B = idx[:20], idx[20:]
    gab, gt, gk = planted.epi_scan(A, B, cls, T)
    want = [p for p in range(tri[0].shape[0]) if tri[0][p, 0] < 20 <= tri[0][p, 1]]
    assert np.array_equal(gab + np.array([0, 20], dtype=np.uint32), tri[0][want])
    assert np.array_equal(gt, tri[1][want]) and np.array_equal(gk.view(np.int64), tri[2][want].view(np.int64))
    # the whole square holds every pair in both orders and the diagonal (a marker against itself: one category pairs, KSA far above T)
    sab, st, sk = planted.epi_scan(idx, idx, cls, T)
    upper = sab[:, 0] < sab[:, 1]
    assert np.array_equal(sab[upper], tri[0]) and np.array_equal(st[upper], tri[1])
    lower = sab[:, 0] > sab[:, 1]
    order = np.lexsort((sab[lower][:, 0], sab[lower][:, 1]))
    assert np.array_equal(sab[lower][order][:, ::-1], tri[0]) and np.array_equal(st[lower][order].transpose(0, 1, 3, 2), tri[1])


def test_second_case():
    geno, cls, ab, t, r = case("second")
    dev = device(geno)
    got = dev.epi_scan(np.arange(geno.shape[0]), None, cls, E.T_SECOND)
    check_list(got, "second", E.T_SECOND)
    dev.set_option("epi_block", 32)
    assert same(dev.epi_scan(np.arange(geno.shape[0]), None, cls, E.T_SECOND), got)
    dev.close()


def test_a_threshold_above_every_pair_gives_an_empty_list(planted):
    geno, cls, ab, t, r = case("planted")
    gab, gt, gk = planted.epi_scan(np.arange(geno.shape[0]), None, cls, 1e6)
    assert gab.shape == (0, 2) and gt.shape == (0, 2, 3, 3) and gk.shape == (0,)
    assert planted.L.hgibbs_epi_scan_get(planted.h, None, None, None) == 0


def test_refusals(planted):
    geno, cls, ab, t, r = case("planted")
    idx = np.arange(geno.shape[0])
    before = planted.epi_scan(idx, None, cls, E.T_PLANTED[0])
    for T in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.HgError, match="hgibbs_epi_scan: threshold = .*, needs a finite number > 0"):
            planted.epi_scan(idx, None, cls, T)
        assert planted.last_epi_ms() == (0.0, 0.0)
    with pytest.raises(capi.HgError, match="hgibbs_epi_scan: na = 0, nb = 0, a list needs at least one marker"):
        planted.epi_scan([], None, cls, 30.0)
    with pytest.raises(capi.HgError, match="hgibbs_epi_scan: na = 2, nb = 0"):
        planted.epi_scan([1, 2], [], cls, 30.0)
    with pytest.raises(capi.HgError, match="hgibbs_epi_scan: idxA\\[1\\] = 40 out of range \\(M = 40\\)"):
        planted.epi_scan([1, 40], None, cls, 30.0)
    with pytest.raises(capi.HgError, match="hgibbs_epi_scan: idxB\\[0\\] = 99 out of range"):
        planted.epi_scan([1, 2], [99], cls, 30.0)
    bad = np.array(cls)
    bad[17] = 3
    with pytest.raises(capi.HgError, match="hgibbs_epi_scan: cls\\[17\\] = 3, a class is 0 or 1"):
        planted.epi_scan(idx, None, bad, 30.0)
    n = C.c_uint64()
    one = np.array([1, 2], dtype=np.uint32)
    assert planted.L.hgibbs_epi_scan(planted.h, 2, one.ctypes.data_as(capi.C_U32P), 0, None, None, 30.0, None) != 0
    assert planted.L.hgibbs_epi_scan(planted.h, 2, None, 0, None, None, 30.0, C.byref(n)) != 0
    assert planted.L.hgibbs_epi_scan(None, 2, one.ctypes.data_as(capi.C_U32P), 0, None, None, 30.0, C.byref(n)) != 0
    empty = capi.Device(0)
    with pytest.raises(capi.HgError, match="hgibbs_epi_scan: no genotypes loaded on this handle"):
        empty.epi_scan([1, 2], None, None, 30.0)
    empty.close()
    for option, value, msg in (("epi_list0", -1, "epi_list0 must be in"), ("epi_block", 70000, "epi_block must be in \\[0,65536\\]")):
        with pytest.raises(capi.HgError, match=msg):
            planted.set_option(option, value)
    # a refused call leaves the previous list alone
    gab = np.zeros_like(before[0])
    assert planted.L.hgibbs_epi_scan_get(planted.h, gab.ctypes.data_as(C.POINTER(C.c_uint32)), None, None) == 0
    assert np.array_equal(gab, before[0])
    assert same(planted.epi_scan(idx, None, cls, E.T_PLANTED[0]), before)


def test_too_many_rows_and_too_much_memory_refused():
    # 2^29 rows of one marker (a 128 MiB BED made in HBM): refused before anything is allocated
    big = capi.Device(0)
    big.synth_bed(1 << 29, 1, seed=3)
    with pytest.raises(capi.HgError, match="hgibbs_epi_scan: 536870912 individuals, at most 536870911 \\(32-bit counts\\)"):
        big.epi_scan([0], [0], None, 30.0)
    assert big.last_epi_ms() == (0.0, 0.0)
    big.close()
    # one block of 65536 x 65536 pairs: 72 bytes each are 288 GiB of tables, above the device's memory
    geno, cls = case("planted")[:2]
    dev = device(geno)
    first = dev.epi_scan(np.arange(geno.shape[0]), None, cls, E.T_PLANTED[0])
    dev.set_option("epi_block", 65536)
    with pytest.raises(capi.HgError, match="hgibbs_epi_scan: lists of 65536 and 65536 markers need [0-9.]+ MiB, [0-9.]+ MiB of device memory are free"):
        dev.epi_scan(np.zeros(1 << 16, dtype=np.uint32), None, cls, 30.0)
    assert dev.last_epi_ms() == (0.0, 0.0)
    dev.set_option("epi_block", 0)
    assert same(dev.epi_scan(np.arange(geno.shape[0]), None, cls, E.T_PLANTED[0]), first)  # the handle then takes a good call
    dev.close()


def test_several_ranks_refused():
    geno, cls = case("planted")[:2]
    N = geno.shape[1]
    calls = []

    def allreduce(arr):  # a stub world of two identical ranks
        calls.append(arr.size)
        arr *= 2

    dev = capi.Device(0)
    dev.comm_init_external(2, 0, allreduce)
    dev.load_bed(synth.pack_bed_columns(geno), N, row_begin=0, row_end=N // 2, n_global=N)
    before = len(calls)
    with pytest.raises(capi.HgError, match="hgibbs_epi_scan: one rank only \\(this handle has 2\\): the counts are not summed over ranks"):
        dev.epi_scan(np.arange(geno.shape[0]), None, cls[:dev.n_local], 30.0)
    assert len(calls) == before and dev.last_epi_ms() == (0.0, 0.0)
    dev.close()


# ---- the CLI end to end, on the planted case ----
def run_cli(tmp_path, name, na_rows=(), extra=()):
    geno, cls = case("planted")[:2]
    N, M = geno.shape[1], geno.shape[0]
    prefix = str(tmp_path / "p")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=cls.astype(float), na_rows=na_rows)
    out = str(tmp_path / name)
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(tmp_path / "o"), "--mcmc-out-name", "n",
                        "--number-individuals", str(N), "--number-markers", str(M), "--epistasis", "--epistasis-out", out, *extra],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    return out, r.stdout


def compare(path, geno, cls, pairs, T):
    want, nums = E.epi_cc(geno, cls, pairs, T)
    got = [line.rstrip("\n").split("\t") for line in open(path)]
    assert len(got) == len(want), (len(got), len(want))
    assert got[0] == want[0]
    for g, w, (ksa, lr, p, ks, ls) in zip(got[1:], want[1:], nums):
        assert [g[c] for c in (0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 13)] == [w[c] for c in (0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 13)]
        assert abs(float(g[9]) - ksa) <= 10 * E.KSA_F64_LD * ks + 5e-9 * abs(ksa)    # (the second term: nine printed digits)
        assert abs(float(g[10]) - lr) <= 10 * E.LR_F64_LD * ls + 5e-9 * abs(lr)
        assert abs(float(g[12]) - p) <= E.tail_tol(lr, int(w[11]), 10 * E.LR_F64_LD * ls) + 5e-9 * p
    return len(got) - 1


def all_pairs(markers):
    m = sorted(markers)
    return [(a, b) for i, a in enumerate(m) for b in m[i + 1:]]


def test_cli_every_pair_twice_byte_equal(tmp_path):
    geno, cls = case("planted")[:2]
    out1, stdout = run_cli(tmp_path, "a.epi.cc", extra=["--epistasis-chisq", "12"])
    out2, _ = run_cli(tmp_path, "b.epi.cc", extra=["--epistasis-chisq", "12"])
    assert open(out1, "rb").read() == open(out2, "rb").read()
    rows = compare(out1, geno, cls, all_pairs(range(40)), 12.0)
    assert rows > 1
    assert "EPISTASIS: 780 pairs tested" in stdout and "%d written to %s" % (rows, out1) in stdout
    out3, _ = run_cli(tmp_path, "c.epi.cc")  # the default threshold: BOOST's 30
    assert compare(out3, geno, cls, all_pairs(range(40)), 30.0) == 1
    assert open(out3).readlines()[1].split("\t")[:6] == ["1", "snp5", "6", "1", "snp33", "34"]


def test_cli_sets_gap_and_na_row(tmp_path):
    geno, cls = case("planted")[:2]
    sets = str(tmp_path / "sets.txt")
    one = [33, 2, 5, 8, 11, 14, 17, 20, 39, 0]
    with open(sets, "w") as f:
        for j in one:
            f.write("g snp%d\n" % j)
        f.write("g nosuch\n")
    out, stdout = run_cli(tmp_path, "s1.epi.cc", extra=["--epistasis-chisq", "12", "--epistasis-sets", sets])
    assert compare(out, geno, cls, all_pairs(one), 12.0) >= 1
    assert "10 markers listed, 45 pairs" in stdout and "1 ids of the sets are not in the .bim" in stdout
    # two sets that share markers 5 and 33: (5, 33) is reachable in both orders and reported once, (5, 5) never
    first, second = [5, 33, 1, 2, 3, 4], [33, 5, 30, 31, 32, 6, 7]
    with open(sets, "w") as f:
        for j in first:
            f.write("left snp%d\n" % j)
        for j in second:
            f.write("right snp%d\n" % j)
    out, stdout = run_cli(tmp_path, "s2.epi.cc", extra=["--epistasis-chisq", "12", "--epistasis-sets", sets])
    pairs = sorted({(min(a, b), max(a, b)) for a in first for b in second if a != b})
    assert "13 markers in two sets listed, %d pairs" % len(pairs) in stdout
    compare(out, geno, cls, pairs, 12.0)
    assert sum(line.startswith("1\tsnp5\t6\t1\tsnp33\t34\t") for line in open(out)) == 1
    # the gap: every marker is on chromosome 1 at bp = index + 1; 0.02 kb leaves out the pairs at most 20 apart
    out, stdout = run_cli(tmp_path, "g.epi.cc", extra=["--epistasis-chisq", "12", "--epistasis-gap", "0.02"])
    compare(out, geno, cls, [(a, b) for a, b in all_pairs(range(40)) if b - a > 20], 12.0)
    # NA phenotype rows are dropped before anything is counted
    na = [0, 77, 599]
    keep = np.ones(geno.shape[1], dtype=bool)
    keep[na] = False
    out, stdout = run_cli(tmp_path, "n.epi.cc", na_rows=na, extra=["--epistasis-chisq", "12"])
    assert "EPISTASIS: 597 rows" in stdout
    compare(out, geno[:, keep], cls[keep], all_pairs(range(40)), 12.0)
