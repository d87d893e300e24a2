"""hydra's sparse genotype representation on the device: hgibbs_sparse_begin / _put / _end against
hgibbs_load_bed, hgibbs_sparse_counts / _get against the numpy restatement (tests/sparse_restate.py), the refusals, and the command
line's two routes.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import sparse_restate as sr
from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
M = 37
GRID = (2, 15, 16, 17, 4095, 4096, 4097, 8193)  # the dword (16 rows), the 4096-row chunk and the n_pad rounding on either side
_cache = {}


def data(N, miss):
    """(geno, bed, lists) of the grid's case, computed once: columns 0, 1, 2 are all 0 (three empty lists), all 2, all missing"""
    if (N, miss) not in _cache:
        geno = synth.make_genotypes(M, N, seed=1000 + N, missing_rate=miss)
        geno[0], geno[1], geno[2] = 0, 2, 3
        bed = synth.pack_bed_columns(geno)
        lists = sr.bed_to_lists(bed, N)
        for a in (geno, bed, *lists.values()):
            a.setflags(write=False)
        _cache[(N, miss)] = (geno, bed, lists)
    return _cache[(N, miss)]


def whole(lists):
    """the three lists of every marker as one slab: what Device.sparse_put takes"""
    return [(lists["ss" + c], lists["sl" + c], lists["si" + c], 0) for c in sr.CLASSES]


def slab(lists, a, b, rng=None):
    """markers [a, b) with only their piece of each index list (idx_base = the first marker's start); rng shuffles every list"""
    out = []
    for c in sr.CLASSES:
        ss, sl, si = lists["ss" + c], lists["sl" + c], lists["si" + c]
        lo, hi = int(ss[a]), int(ss[b - 1] + sl[b - 1])
        piece = si[lo:hi].copy()
        if rng is not None:
            for j in range(a, b):
                s = int(ss[j]) - lo
                rng.shuffle(piece[s:s + int(sl[j])])
        out.append((ss[a:b], sl[a:b], piece, lo))
    return out


def from_bed(bed, N, **kw):
    d = capi.Device(0)
    d.load_bed(bed, N, **kw)
    return d


def from_lists(lists, N, puts=None, **kw):
    d = capi.Device(0)
    d.sparse_begin(N, M, **kw)
    for m0, ls in (puts if puts is not None else [(0, whole(lists))]):
        d.sparse_put(m0, ls)
    d.sparse_end()
    return d


def mask_of(N):
    """drops the first row, the last row and a run in the middle (N = 2: the first row only, or nothing would be left)"""
    keep = np.ones(N, dtype=np.uint8)
    keep[0] = 0
    if N > 2:
        keep[N - 1] = 0
        keep[N // 3:N // 3 + max(1, N // 5)] = 0
    return keep


def shards_of(kept, masked):
    """two shards of the kept rows (without a mask a shard starts at a multiple of 4); a shard that would be empty is left out, which
    happens at N = 2 only"""
    cut = kept // 2 if masked else kept // 2 // 4 * 4
    return [(a, b) for a, b in ((0, cut), (cut, kept)) if b > a]


@pytest.mark.parametrize("miss", [0.0, 0.02])
@pytest.mark.parametrize("N", GRID)
def test_load_equals_load(gpu_lib, N, miss):
    _, bed, lists = data(N, miss)
    # whole, one put
    ref = from_bed(bed, N)
    want = ref.get_bed()
    dev = from_lists(lists, N)
    assert (dev.n_global, dev.n_local, dev.M, dev.row_begin) == (ref.n_global, ref.n_local, ref.M, ref.row_begin)
    assert np.array_equal(dev.get_bed(), want)
    assert dev.last_sparse_ms()[0] > 0.0
    # marker stats: the counts are the list lengths
    _, _, n1, n2, nm = dev.marker_stats()
    assert np.array_equal(n1, lists["sl1"]) and np.array_equal(n2, lists["sl2"]) and np.array_equal(nm, lists["slm"])
    # three uneven slabs, in reverse order, every list shuffled, each slab with only its piece of the index lists
    rng = np.random.default_rng(N)
    puts = [(a, slab(lists, a, b, rng)) for a, b in ((6, M), (5, 6), (0, 5))]
    assert np.array_equal(from_lists(lists, N, puts).get_bed(), want)
    # a keep mask; two shards, with and without the mask
    keep = mask_of(N)
    kept = int(keep.sum())
    ng = max(kept, 2)
    assert np.array_equal(from_lists(lists, N, keep=keep, n_global=ng).get_bed(), from_bed(bed, N, keep=keep, n_global=ng).get_bed())
    for kp, n_kept, n_glob in ((None, N, N), (keep, kept, ng)):
        for a, b in shards_of(n_kept, kp is not None):
            kw = dict(keep=kp, row_begin=a, row_end=b, n_global=n_glob)
            r, d = from_bed(bed, N, **kw), from_lists(lists, N, **kw)
            assert (d.n_local, d.row_begin) == (r.n_local, r.row_begin) == (b - a, a)
            assert np.array_equal(d.get_bed(), r.get_bed()), (a, b, kp is not None)


def split_get(dev, cuts, want=(True, True, True)):
    parts = [dev.sparse_get(a, b - a, want) for a, b in zip(cuts[:-1], cuts[1:])]
    return [np.concatenate([p[l] for p in parts]) if want[l] else None for l in range(3)]


@pytest.mark.parametrize("miss", [0.0, 0.02])
@pytest.mark.parametrize("N", GRID)
def test_write_equals_restatement(gpu_lib, N, miss):
    _, bed, lists = data(N, miss)
    dev = from_bed(bed, N)
    cnt = dev.sparse_counts()
    for c, got in zip(sr.CLASSES, cnt):
        assert np.array_equal(got, lists["sl" + c]), c
    for c, got in zip(sr.CLASSES, dev.sparse_counts(5, 7)):
        assert np.array_equal(got, lists["sl" + c][5:12]), c
    want = [lists["si" + c] for c in sr.CLASSES]

    def same(got):
        return all(g.dtype == np.uint32 and np.array_equal(g, w) for g, w in zip(got, want))

    assert same(dev.sparse_get())
    assert dev.last_sparse_ms()[1] > 0.0 or sum(w.size for w in want) == 0
    assert same(split_get(dev, (0, 5, 6, M)))           # m0 / count cut in three
    dev.set_option("sparse_piece", 1)                    # every marker a piece of its own
    assert same(dev.sparse_get())
    assert same(split_get(dev, (0, 11, 30, M)))
    dev.set_option("sparse_piece", 0)
    for skip in range(3):                                # each list in turn skipped by a NULL pointer
        wanted = tuple(l != skip for l in range(3))
        got = dev.sparse_get(0, M, wanted)
        assert got[skip] is None
        assert all(np.array_equal(got[l], want[l]) for l in range(3) if l != skip)
    # fed back with keep_host = NULL the lists reproduce the image
    back = {}
    for c, n, idx in zip(sr.CLASSES, cnt, dev.sparse_get()):
        ss = np.zeros(M, dtype=np.uint64)
        ss[1:] = np.cumsum(n)[:-1]
        back["sl" + c], back["ss" + c], back["si" + c] = n, ss, idx
    assert np.array_equal(from_lists(back, N).get_bed(), dev.get_bed())


def test_wide(gpu_lib):
    """M beyond one launch's grid.y, load and write once each"""
    Mw, N = 70000, 5
    rng = np.random.default_rng(7)
    geno = rng.integers(0, 4, size=(Mw, N), dtype=np.uint8)
    bed = synth.pack_bed_columns(geno)
    lists = sr.bed_to_lists(bed, N)
    dev = capi.Device(0)
    dev.sparse_begin(N, Mw)
    dev.sparse_put(0, whole(lists))
    dev.sparse_end()
    assert np.array_equal(dev.get_bed(), bed)
    for c, n, idx in zip(sr.CLASSES, dev.sparse_counts(), dev.sparse_get()):
        assert np.array_equal(n, lists["sl" + c]) and np.array_equal(idx, lists["si" + c]), c


def test_refusals(gpu_lib):
    """a refused put or end abandons the load: the message names marker and row, the handle has no genotypes afterwards, and the same
    handle then takes a good load"""
    N, Mr = 40, 5
    geno = synth.make_genotypes(Mr, N, seed=3, missing_rate=0.1)
    geno[3, 7], geno[3, 9], geno[3, 11] = 1, 2, 3
    geno[1, 5] = 2
    bed = synth.pack_bed_columns(geno)
    good = sr.bed_to_lists(bed, N)
    dev = capi.Device(0)

    def edit(cls, j, fn):
        """the lists with marker j's list of class cls rewritten by fn(rows) -> rows"""
        out = {}
        for c in sr.CLASSES:
            per = [good["si" + c][int(good["ss" + c][k]):int(good["ss" + c][k] + good["sl" + c][k])] for k in range(Mr)]
            if c == cls:
                per[j] = np.asarray(fn(per[j]), dtype=np.uint32)
            sl = np.array([p.size for p in per], dtype=np.uint64)
            ss = np.zeros(Mr, dtype=np.uint64)
            ss[1:] = np.cumsum(sl)[:-1]
            out["sl" + c], out["ss" + c], out["si" + c] = sl, ss, np.concatenate(per).astype(np.uint32)
        return out

    def refused(puts, words, at_end=False):
        dev.sparse_begin(N, Mr)
        with pytest.raises(capi.HgError) as e:
            for m0, ls in puts:
                dev.sparse_put(m0, ls)
            assert at_end
            dev.sparse_end()
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        with pytest.raises(capi.HgError) as e:
            dev.marker_stats()
        assert "no data loaded" in str(e.value)
        assert dev.last_sparse_ms()[0] == 0.0
        with pytest.raises(capi.HgError):  # the load is gone
            dev.sparse_end()

    def put_all(lists):
        return [(0, whole(lists))]

    # row 7 of marker 3 is a 1: listed among the twos as well
    refused(put_all(edit("2", 3, lambda r: np.append(r, 7))), ["marker 3", "row 7", "twice"])
    # row 11 of marker 3 twice among the missing calls
    refused(put_all(edit("m", 3, lambda r: np.append(r, 11))), ["marker 3", "row 11", "twice"])
    # an index = n_total
    refused(put_all(edit("1", 2, lambda r: np.append(r, N))), ["marker 2", "row %d" % N, "n_total"])
    # of two offences the smallest (marker, row) is named
    both = edit("1", 4, lambda r: np.append(r, N + 1))
    both["si2"], both["sl2"], both["ss2"] = (edit("2", 1, lambda r: np.append(r, 5))[k] for k in ("si2", "sl2", "ss2"))
    refused(put_all(both), ["marker 1", "row 5", "twice"])
    # a start outside the piece: below idx_base, and beyond its end
    ls = slab(good, 2, 4)
    ls[0] = (ls[0][0], ls[0][1], ls[0][2], ls[0][3] + 1)
    refused([(2, ls)], ["marker 2", "start", "idx_base"])
    ls = slab(good, 2, 4)
    ls[1] = (ls[1][0], ls[1][1], ls[1][2][:-1], ls[1][3])
    refused([(2, ls)], ["marker 3", "beyond the piece"])
    # len > n_total; markers beyond M
    ls = whole(good)
    ls[2] = (ls[2][0], np.full(Mr, N + 1, dtype=np.uint64), ls[2][2], 0)
    refused([(0, ls)], ["marker 0", "len", "n_total"])
    refused([(1, whole(good))], ["beyond M"])
    # a marker put twice
    refused([(0, slab(good, 0, 3)), (2, slab(good, 2, 5))], ["marker 2", "put already"])
    # end with a marker never put
    refused([(0, slab(good, 0, 2)), (3, slab(good, 3, 5))], ["marker 2", "never put"], at_end=True)
    # between begin and end the handle has no genotypes and takes no second load
    dev.sparse_begin(N, Mr)
    with pytest.raises(capi.HgError) as e:
        dev.marker_stats()
    assert "no data loaded" in str(e.value)
    for again in (lambda: dev.sparse_begin(N, Mr), lambda: dev.load_bed(bed, N)):
        with pytest.raises(capi.HgError) as e:
            again()
        assert "in progress" in str(e.value)
    # ... and the load goes on: the handle that refused all of the above ends up with the image
    dev.sparse_put(0, whole(good))
    dev.sparse_end()
    assert np.array_equal(dev.get_bed(), from_bed(bed, N).get_bed())
    # begin's refusals are hgibbs_load_bed's
    d2 = capi.Device(0)
    for kw, word in ((dict(row_begin=2, row_end=N), "multiple of 4"), (dict(row_end=N + 1), "n_total"), (dict(n_global=1), "n_global"),
                     (dict(row_begin=8, row_end=8), "empty row range")):
        with pytest.raises(capi.HgError) as e:
            d2.sparse_begin(N, Mr, **kw)
        assert word in str(e.value)
    # several ranks: counts and get refuse by name (the handle is cheap to make: no exchange happens before the refusal)
    d3 = capi.Device(0)
    d3.comm_init_external(2, 0, lambda a: None)
    d3.load_bed(bed, N, row_begin=0, row_end=20, n_global=N)
    for call in (d3.sparse_counts, d3.sparse_get):
        with pytest.raises(capi.HgError) as e:
            call()
        assert "2 ranks" in str(e.value)


# ---- the command line ------------------------------------------------------------------------------------------------------------
CN, CM, NA_ROWS = 300, 200, (17, 255)


def cli(*args):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def converted(tmp_path_factory):
    """a PLINK set of 300 rows x 200 markers with missing calls, two NA phenotypes, and its sparse files written by --bed-to-sparse"""
    d = tmp_path_factory.mktemp("sparse_cli")
    geno = synth.make_genotypes(CM, CN, seed=11, missing_rate=0.03)
    y, fail, _ = synth.make_survival(geno, seed=12, causal_frac=0.05)
    bed = synth.pack_bed_columns(geno)
    synth.write_plink(str(d / "x"), bed, CN, y=y, na_rows=NA_ROWS)
    np.savetxt(str(d / "x.fail"), fail, fmt="%d")
    os.mkdir(d / "sp")
    out = cli("--bed-to-sparse", "--bfile", str(d / "x"), "--pheno", str(d / "x.phen"), "--sparse-dir", str(d / "sp"), "--sparse-basename", "s",
              "--blocks-per-rank", "4")
    return d, bed, out


def test_cli_bed_to_sparse_writes_the_restatements_files(converted):
    d, bed, out = converted
    assert "--blocks-per-rank ignored" in out and "will always convert the whole file" in out
    want = sr.file_bytes(sr.bed_to_lists(bed, CN), CN, CM)  # every .fam row, the NA phenotypes included
    assert sorted(os.listdir(d / "sp")) == sorted("s." + k for k in want) and len(want) == 10
    for k, v in want.items():
        assert (d / "sp" / ("s." + k)).read_bytes() == v, k
    # without the pair, directory and name are --bfile's; existing files are overwritten
    (d / "x.si1").write_bytes(b"stale")
    cli("--bed-to-sparse", "--bfile", str(d / "x"))
    for k, v in want.items():
        assert (d / ("x." + k)).read_bytes() == v, k


def same_outputs(d, a, b, suffixes):
    for s in suffixes:
        fa, fb = open(str(d / a) + "." + s, "rb").read(), open(str(d / b) + "." + s, "rb").read()
        assert fa == fb, s
    assert os.path.getsize(str(d / a) + "." + suffixes[0]) > 0


CHAIN_FILES = ("csv", "bet", "cpn", "acu", "mus.0")         # (.mus carries the rank)
W_CHAIN_FILES = ("csv", "bet", "cpn", "xbet", "xcpn", "eps.0")  # what the bayesWMPI chain writes of them, and its last state


def test_cli_chain_from_sparse_files_without_bfile(converted):
    d, _, _ = converted
    common = ["--mpibayes", "bayesMPI", "--pheno", str(d / "x.phen"), "--mcmc-out-dir", str(d / "o"), "--number-individuals", str(CN),
              "--number-markers", str(CM), "--chain-length", "4", "--thin", "1", "--save", "2", "--seed", "5", "--S", "0.001,0.01"]
    cli(*common, "--mcmc-out-name", "bed", "--bfile", str(d / "x"))
    out = cli(*common, "--mcmc-out-name", "sparse", "--sparse-dir", str(d / "sp"), "--sparse-basename", "s")
    assert "genotypes are read from the sparse files" in out and "adjusted to %d - 2 = %d" % (CN, CN - 2) in out
    same_outputs(d / "o", "bed", "sparse", CHAIN_FILES)
    # --read-from-bed-file with the pair selects the BED
    out = cli(*common, "--mcmc-out-name", "both", "--bfile", str(d / "x"), "--sparse-dir", str(d / "sp"), "--sparse-basename", "s", "--read-from-bed-file")
    assert "genotypes are read from the sparse files" not in out
    same_outputs(d / "o", "bed", "both", CHAIN_FILES)


def test_cli_bayesw_chain_from_sparse_files_without_bfile(converted):
    d, _, _ = converted
    common = ["--mpibayes", "bayesWMPI", "--pheno", str(d / "x.phen"), "--failure", str(d / "x.fail"), "--quad_points", "7", "--mcmc-out-dir", str(d / "w"),
              "--number-individuals", str(CN), "--number-markers", str(CM), "--chain-length", "3", "--thin", "1", "--save", "2", "--seed", "5",
              "--S", "0.001,0.01"]
    cli(*common, "--mcmc-out-name", "bed", "--bfile", str(d / "x"))
    out = cli(*common, "--mcmc-out-name", "sparse", "--sparse-dir", str(d / "sp"), "--sparse-basename", "s")
    assert "genotypes are read from the sparse files" in out
    same_outputs(d / "w", "bed", "sparse", W_CHAIN_FILES)


def test_cli_qc_with_bfile_naming_rows_and_markers(converted):
    d, _, _ = converted
    common = ["--mpibayes", "bayesMPI", "--bfile", str(d / "x"), "--pheno", str(d / "x.phen"), "--mcmc-out-dir", str(d / "q"), "--mcmc-out-name", "n",
              "--number-individuals", str(CN), "--number-markers", str(CM), "--qc", "--qc-maf", "0.05", "--qc-geno", "0.04"]
    os.mkdir(d / "q")
    cli(*common, "--qc-out", str(d / "q" / "bed"))
    out = cli(*common, "--qc-out", str(d / "q" / "sparse"), "--sparse-dir", str(d / "sp"), "--sparse-basename", "s")
    assert "only .fam/.bim from --bfile" in out
    made = sorted(f[len("bed."):] for f in os.listdir(d / "q") if f.startswith("bed."))
    assert "frq" in made and "lmiss" in made and "imiss" in made
    same_outputs(d / "q", "bed", "sparse", made)
