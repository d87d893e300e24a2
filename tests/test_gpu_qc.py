"""hydra_mi355x --qc end to end: every column of every file against NumPy on the chain's rows (counts exactly, ratios to 1e-8
relative: %.9g prints nine digits and the operator's own error is orders below that), P against capi.hwe_exact, the two lists
against the same rules restated here, and one sanity check on the inbreeding statistics."""
import math
import os
import subprocess

import numpy as np
import pytest

import rowsums_restate as rr
from hydra_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")

pytestmark = pytest.mark.gpu

N, M = 300, 200
NA_ROWS = [7, 150, 299]
INBRED = list(range(20, 30))
CHR = [1] * 120 + [2] * 50 + [23] * 30
MAF, GENO, MIND, HWE, HETSD = 0.05, 0.1, 0.1, 1e-4, 2.0
RTOL = 1e-8


def make():
    rng = np.random.default_rng(11)
    p = rng.uniform(0.1, 0.5, size=M)
    geno = rng.binomial(2, p[:, None], size=(M, N)).astype(np.int8)
    for i in INBRED:  # homozygous at half the heterozygous sites
        het = np.flatnonzero(geno[:, i] == 1)
        for j in het[rng.random(het.size) < 0.5]:
            geno[j, i] = 0 if rng.random() < 0.5 else 2
    geno[rng.random((M, N)) < 0.01] = 3     # missing calls
    geno[5] = 2                             # a monomorphic marker
    geno[6] = 3                             # a marker missing everywhere
    geno[9] = rng.binomial(2, 0.01, size=N)  # a rare allele
    geno[12, rng.random(N) < 0.3] = 3       # a marker with many missing calls
    geno[15] = np.where(rng.random(N) < 0.5, 0, 2)  # no heterozygote at all
    geno[195] = np.where(rng.random(N) < 0.5, 0, 2)  # the same on chromosome 23
    geno[rng.random(M) < 0.4, 40] = 3       # an individual with many missing calls
    geno[:, 41] = 3                         # and one missing everywhere
    return geno


def fnum(t):
    return float("nan") if t == "NA" else float(t)


def close(got, want):
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= RTOL * abs(want)


def table(path, head):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert rows[0] == head, path
    return rows[1:]


@pytest.fixture(scope="module")
def qc(tmp_path_factory):
    d = tmp_path_factory.mktemp("qc")
    geno = make()
    prefix = str(d / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=np.random.default_rng(3).standard_normal(N), na_rows=NA_ROWS)
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%d snp%d 0 %d A C\n" % (CHR[j], j, j + 1))
    out = str(d / "q")
    r = subprocess.run([EXE, "--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", str(d / "o"),
                        "--mcmc-out-name", "n", "--number-individuals", str(N), "--number-markers", str(M), "--qc", "--qc-out", out,
                        "--qc-maf", str(MAF), "--qc-geno", str(GENO), "--qc-mind", str(MIND), "--qc-hwe", str(HWE), "--qc-het-sd", str(HETSD)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    keep = np.array([i for i in range(N) if i not in NA_ROWS])
    codes = rr.codes_of(geno)[keep]
    return out, keep, codes, r.stdout


def marker_counts(codes):
    n1, n2, nm = (codes == 1).sum(0), (codes == 2).sum(0), (codes == 3).sum(0)
    nc = codes.shape[0] - nm
    return n1, n2, nm, nc, nc - n1 - n2


def test_marker_tables(qc):
    out, keep, codes, _ = qc
    Nk = codes.shape[0]
    n1, n2, nm, nc, n0 = marker_counts(codes)
    frq = table(out + ".frq", ["CHR", "SNP", "A1", "A2", "MAF", "NCHROBS"])
    lmiss = table(out + ".lmiss", ["CHR", "SNP", "N_MISS", "N_GENO", "F_MISS"])
    hwe = table(out + ".hwe", ["CHR", "SNP", "TEST", "A1", "A2", "GENO", "O(HET)", "E(HET)", "P"])
    assert len(frq) == len(lmiss) == len(hwe) == M
    for j in range(M):
        p = (n1[j] + 2.0 * n2[j]) / (2.0 * nc[j]) if nc[j] else float("nan")
        assert frq[j][:4] == [str(CHR[j]), "snp%d" % j, "A", "C"] and int(frq[j][5]) == 2 * nc[j]
        assert close(fnum(frq[j][4]), p), (j, frq[j])
        assert lmiss[j][:2] == [str(CHR[j]), "snp%d" % j] and int(lmiss[j][2]) == nm[j] and int(lmiss[j][3]) == Nk
        assert close(fnum(lmiss[j][4]), nm[j] / Nk)
        assert hwe[j][:5] == [str(CHR[j]), "snp%d" % j, "ALL", "A", "C"]
        assert hwe[j][5] == "%d/%d/%d" % (n2[j], n1[j], n0[j])
        assert close(fnum(hwe[j][6]), n1[j] / nc[j] if nc[j] else float("nan"))
        assert close(fnum(hwe[j][7]), 2.0 * p * (1.0 - p))
        assert close(fnum(hwe[j][8]), capi.hwe_exact(int(n1[j]), int(n2[j]), int(n0[j]))), (j, hwe[j])
    assert frq[6][4] == "NA" and hwe[6][8] == "NA"  # the marker missing everywhere


def row_reference(codes):
    """O(HOM), E(HOM), N(NM), F and Fhat1 .. Fhat3 from their definitions over the QC markers, in exactly rounded sums"""
    Nk = codes.shape[0]
    n1, n2, nm, nc, n0 = marker_counts(codes)
    qcm = rr.polymorphic(codes) & np.array([1 <= c <= 22 for c in CHR])
    js = np.flatnonzero(qcm)
    p = (n1[js] + 2.0 * n2[js]) / (2.0 * nc[js])
    h = 2.0 * p * (1.0 - p)
    e = 1.0 - h * (2.0 * nc[js]) / (2.0 * nc[js] - 1.0)
    ref = []
    for i in range(Nk):
        g = codes[i, js]
        ok = g != 3
        x = g[ok].astype(np.float64)
        pp, hh = p[ok], h[ok]
        nn = int(ok.sum())
        O, E = int(np.sum(g[ok] != 1)), math.fsum(e[ok])
        nan = float("nan")
        F = (O - E) / (nn - E) if nn and nn - E != 0 else nan
        f1 = math.fsum((x - 2 * pp) ** 2 / hh - 1.0) / nn if nn else nan
        f2 = math.fsum(1.0 - x * (2.0 - x) / hh) / nn if nn else nan
        f3 = math.fsum((x * x - (1.0 + 2.0 * pp) * x + 2.0 * pp * pp) / hh) / nn if nn else nan
        ref.append((O, E, nn, F, f1, f2, f3))
    return qcm, ref


def test_row_tables(qc):
    out, keep, codes, _ = qc
    Nk = codes.shape[0]
    qcm, ref = row_reference(codes)
    assert not qcm[120 + 50:].any() and qcm[:170].sum() == 170 - 2  # chromosome 23 and the two markers without a finite sd stay out
    imiss = table(out + ".imiss", ["FID", "IID", "N_MISS", "N_GENO", "F_MISS"])
    het = table(out + ".het", ["FID", "IID", "O(HOM)", "E(HOM)", "N(NM)", "F"])
    ibc = table(out + ".ibc", ["FID", "IID", "NOMISS", "Fhat1", "Fhat2", "Fhat3"])
    assert len(imiss) == len(het) == len(ibc) == Nk
    for i in range(Nk):
        ids = ["fam%d" % keep[i], "ind%d" % keep[i]]
        O, E, nn, F, f1, f2, f3 = ref[i]
        nmiss = int((codes[i] == 3).sum())  # over every marker, chromosome 23 included
        assert imiss[i][:2] == ids and int(imiss[i][2]) == nmiss and int(imiss[i][3]) == M and close(fnum(imiss[i][4]), nmiss / M)
        assert het[i][:2] == ids and int(het[i][2]) == O and int(het[i][4]) == nn, (i, het[i], ref[i])
        assert close(fnum(het[i][3]), E) and close(fnum(het[i][5]), F), (i, het[i], ref[i])
        assert ibc[i][:2] == ids and int(ibc[i][2]) == nn
        for got, want in zip(ibc[i][3:], (f1, f2, f3)):
            assert close(fnum(got), want), (i, ibc[i], ref[i])
    # chromosome 23 is absent from the sums: N(NM) counts the called QC markers only, while N_MISS counts every marker
    i = 0
    assert int(het[i][4]) == int(((codes[i] != 3) & qcm).sum()) < int((codes[i] != 3).sum())
    k = list(keep).index(41)
    assert het[k][2:] == ["0", "0", "0", "NA"] and ibc[k][2:] == ["0", "NA", "NA", "NA"] and int(imiss[k][2]) == M


def test_lists(qc):
    out, keep, codes, stdout = qc
    Nk = codes.shape[0]
    n1, n2, nm, nc, n0 = marker_counts(codes)
    poly = rr.polymorphic(codes)
    want = []
    for j in range(M):
        why = []
        if not poly[j]:
            why = ["MONO"]
        else:
            p = (n1[j] + 2.0 * n2[j]) / (2.0 * nc[j])
            if min(p, 1.0 - p) < MAF:
                why.append("MAF")
            if nm[j] / Nk > GENO:
                why.append("GENO")
            if capi.hwe_exact(int(n1[j]), int(n2[j]), int(n0[j])) < HWE:
                why.append("HWE")
        if why:
            want.append(["snp%d" % j, ",".join(why)])
    got = table(out + ".qc.exclude", ["SNP", "REASON"])
    assert got == want
    reasons = dict(got)
    assert reasons["snp5"] == "MONO" and reasons["snp6"] == "MONO" and "MAF" in reasons["snp9"] and "GENO" in reasons["snp12"]
    assert "HWE" in reasons["snp15"] and "HWE" in reasons["snp195"]  # (marker thresholds apply on every chromosome)

    _, ref = row_reference(codes)
    F = np.array([r[3] for r in ref])
    fin = np.isfinite(F)
    mean, sd = F[fin].mean(), F[fin].std(ddof=1)
    want = []
    for i in range(Nk):
        why = []
        if (codes[i] == 3).sum() / M > MIND:
            why.append("MIND")
        if fin[i] and abs(F[i] - mean) > HETSD * sd:
            why.append("HET")
        if why:
            want.append(["fam%d" % keep[i], "ind%d" % keep[i], ",".join(why)])
    got = table(out + ".qc.remove", ["FID", "IID", "REASON"])
    assert got == want
    rows = {r[1]: r[2] for r in got}
    assert rows["ind40"] == "MIND" or rows["ind40"] == "MIND,HET"
    assert rows["ind41"] == "MIND"
    assert "QC     :" in stdout and "MONO 2" in stdout and "MIND" in stdout


def test_inbred_rows_stand_out(qc):
    out, keep, codes, _ = qc
    het = table(out + ".het", ["FID", "IID", "O(HOM)", "E(HOM)", "N(NM)", "F"])
    ibc = table(out + ".ibc", ["FID", "IID", "NOMISS", "Fhat1", "Fhat2", "Fhat3"])
    inb = np.isin(keep, INBRED)
    F = np.array([fnum(r[5]) for r in het])
    f3 = np.array([fnum(r[5]) for r in ibc])
    for v in (F, f3):
        assert np.nanmax(v[~inb]) < np.min(v[inb])
