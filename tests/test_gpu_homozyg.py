"""hydra_mi355x --homozyg end to end on one small cohort: the three files are rebuilt from tests/roh_restate.py and compared as text; the
genotypes read from hydra's sparse files give the same bytes."""
import os
import subprocess

import numpy as np
import pytest

import roh_restate as rr
from hydra_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 300, 1500
NA_ROWS = [3, 64, 65, 299]
CHROM = ["1"] * 500 + ["2"] * 420 + ["23"] * 80 + ["3"] * 500  # chromosome 23 is not selected (the .bim is counted with numeric chromosomes)
MONO = [17, 700, 1499]                                        # nor are these: one genotype among the kept rows
ARGS = ["--homozyg-window-snp", "8", "--homozyg-window-het", "0", "--homozyg-window-missing", "1", "--homozyg-window-threshold", "0.05",
        "--homozyg-snp", "10", "--homozyg-kb", "5", "--homozyg-density", "3", "--homozyg-gap", "40"]
KW = dict(window=8, window_het=0, window_missing=1, threshold=0.05, min_snps=10, min_bp=5000, dens_bp=3000, gap_bp=40000)


def g9(v):
    return "%.9g" % v


def cli(*args):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("homozyg")
    geno = synth.make_genotypes(M, N, seed=31, missing_rate=0.02)
    geno[200:460, 7][geno[200:460, 7] == 1] = 0  # a long stretch of row 7 without hets, over the gap below
    geno[MONO, :] = 2
    y = np.random.default_rng(4).standard_normal(N)
    prefix = str(d / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=NA_ROWS)
    bp = np.zeros(M, dtype=np.int64)
    step = np.random.default_rng(1).integers(1, 3000, size=M)
    step[300] += 50000
    for c in set(CHROM):
        on = np.flatnonzero(np.array(CHROM) == c)
        bp[on] = np.cumsum(step[on])
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%s snp%d 0 %d A C\n" % (CHROM[j], j, bp[j]))
    base = ["--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(d / "o"), "--mcmc-out-name", "n",
            "--number-individuals", str(N), "--number-markers", str(M)]
    return d, geno, bp, base


def expected(geno, bp, **kw):
    kept = np.setdiff1d(np.arange(N), NA_ROWS)
    g = geno[:, kept]
    sel = [j for j in range(M) if CHROM[j] != "23" and j not in MONO]
    run_off = [0]
    for c in ("1", "2", "3"):
        run_off.append(run_off[-1] + sum(CHROM[j] == c for j in sel))
    idx = np.array(sel)
    segs = rr.segments(g, run_off, idx, bp[idx], **kw)
    span = sum(int(bp[idx[run_off[r + 1] - 1]] - bp[idx[run_off[r]]]) for r in range(3))
    hom = ["FID\tIID\tCHR\tSNP1\tSNP2\tPOS1\tPOS2\tKB\tNSNP\tDENSITY\tPHOM\tPHET"]
    indiv = ["FID\tIID\tNSEG\tKB\tKBAVG\tFROH"]
    summary = ["CHR\tSNP\tBP\tN_ROH"]
    over = np.zeros(len(idx), dtype=np.int64)
    total, count = np.zeros(len(kept), dtype=np.int64), np.zeros(len(kept), dtype=np.int64)
    for row, first, last, n, nhet, nmis in segs:
        i, j1, j2 = kept[row], idx[first], idx[last]
        ln = int(bp[j2] - bp[j1])
        kb = ln / 1000.0
        hom.append("fam%d\tind%d\t%s\tsnp%d\tsnp%d\t%d\t%d\t%s\t%d\t%s\t%s\t%s" % (i, i, CHROM[j1], j1, j2, bp[j1], bp[j2], g9(kb), n, g9(kb / n),
                                                                                g9((n - nhet - nmis) / n), g9(nhet / n)))
        over[first:last + 1] += 1
        total[row] += ln
        count[row] += 1
    for r, i in enumerate(kept):
        kb = int(total[r]) / 1000.0
        indiv.append("fam%d\tind%d\t%d\t%s\t%s\t%s" % (i, i, count[r], g9(kb), g9(kb / count[r]) if count[r] else "NA", g9(int(total[r]) / span)))
    at = {int(j): k for k, j in enumerate(idx)}
    for j in range(M):
        summary.append("%s\tsnp%d\t%d\t%s" % (CHROM[j], j, bp[j], over[at[j]] if j in at else "NA"))
    return segs, {".hom": hom, ".hom.indiv": indiv, ".hom.summary": summary}


def test_files_equal_the_restatement(cohort):
    d, geno, bp, base = cohort
    out = cli(*base, "--homozyg", *ARGS)
    segs, want = expected(geno, bp, **KW)
    assert len(segs) > 200 and any(s[0] == 7 - 1 and s[3] > 64 for s in segs), "row 7 (the seventh kept row) has its planted stretch"
    for ext, lines in want.items():
        got = (d / "o" / ("n" + ext)).read_text().split("\n")
        assert got[-1] == "" and got[:-1] == lines, ext
    rows = len({s[0] for s in segs})
    assert "HOMOZYG: %d segments in %d rows" % (len(segs), rows) in out, out
    # other thresholds, another prefix: a limit on the hets of a segment, a wider window
    out2 = str(d / "second")
    cli(*base, "--homozyg", "--homozyg-out", out2, "--homozyg-window-snp", "20", "--homozyg-window-het", "2", "--homozyg-snp", "15", "--homozyg-kb", "10",
        "--homozyg-density", "2", "--homozyg-gap", "1000", "--homozyg-het", "1", "--homozyg-window-threshold", "0.5")
    segs2, want2 = expected(geno, bp, window=20, window_het=2, window_missing=5, threshold=0.5, min_snps=15, min_bp=10000, dens_bp=2000, gap_bp=1000000,
                            max_het=1)
    assert segs2 and segs2 != segs
    for ext, lines in want2.items():
        assert open(out2 + ext).read().split("\n")[:-1] == lines, ext


def test_plink_defaults_find_nothing_here(cohort):
    """PLINK's defaults ask for 1000 kb: the cohort's chromosomes are shorter, so every table has its rows and no segment"""
    d, geno, bp, base = cohort
    out = str(d / "defaults")
    cli(*base, "--homozyg", "--homozyg-out", out)
    segs, want = expected(geno, bp, **rr.params())
    assert segs == []
    for ext, lines in want.items():
        assert open(out + ext).read().split("\n")[:-1] == lines, ext


def test_sparse_route_gives_the_same_bytes(cohort):
    d, geno, bp, base = cohort
    os.makedirs(str(d / "sp"), exist_ok=True)
    cli("--bed-to-sparse", "--bfile", base[3], "--pheno", base[5], "--sparse-dir", str(d / "sp"), "--sparse-basename", "s")
    a, b = str(d / "from_bed"), str(d / "from_sparse")
    cli(*base, "--homozyg", *ARGS, "--homozyg-out", a)
    cli(*base, "--homozyg", *ARGS, "--homozyg-out", b, "--sparse-dir", str(d / "sp"), "--sparse-basename", "s")
    for ext in (".hom", ".hom.indiv", ".hom.summary"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert os.path.getsize(a + ".hom") > 1000
