"""hydra_mi355x --predict-bfile, the part that runs before any device is touched: refusals, the .bet records it keeps, and the
report of how the target's markers match the training markers.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 30, 12


def run(*args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=60, env=e)


def write_bet(path, its, M=M, seed=0):
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        f.write(np.uint32(M).tobytes())
        for it in its:
            f.write(np.uint32(it).tobytes())
            f.write(rng.standard_normal(M).tobytes())


def write_bim(path, rows):
    with open(path, "w") as f:
        for r in rows:
            f.write("1 %s 0 1 %s %s\n" % r)


@pytest.fixture()
def chain(tmp_path):
    geno = synth.make_genotypes(M, N, seed=1)
    y, _ = synth.make_phenotype(geno, seed=2)
    prefix = str(tmp_path / "x")
    synth.write_plink(prefix, synth.pack_bed_columns(geno), N, y=y, na_rows=[4])
    out = str(tmp_path / "o")
    os.makedirs(out)
    write_bet(out + "/n.bet", [0, 1, 2, 3])
    target = str(tmp_path / "t")
    synth.write_plink(target, synth.pack_bed_columns(geno[:, :9]), 9)
    base = ["--mpibayes", "bayesMPI", "--bfile", prefix, "--pheno", prefix + ".phen", "--mcmc-out-dir", out, "--mcmc-out-name", "n",
            "--number-individuals", str(N), "--number-markers", str(M), "--burn-in", "2"]
    return base, out, target


def test_refused_with_bayesw(chain):
    base, _, target = chain
    r = run(*[("bayesWMPI" if a == "bayesMPI" else a) for a in base], "--predict-bfile", target)
    assert r.returncode != 0 and "bayesMPI effects only" in r.stderr


def test_refused_with_restart(chain):
    base, _, target = chain
    r = run(*base, "--restart", "--predict-bfile", target)
    assert r.returncode != 0 and "cannot be combined with --restart" in r.stderr


def test_refused_with_several_ranks(chain):
    base, _, target = chain
    r = run(*base, "--predict-bfile", target, env={"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0 and "one process" in r.stderr


def test_predict_out_and_dry_run_need_predict_bfile(chain):
    base, _, _ = chain
    r = run(*base, "--predict-out", "x.prs")
    assert r.returncode != 0 and "--predict-out needs --predict-bfile" in r.stderr
    r = run(*base, "--predict-dry-run")
    assert r.returncode != 0 and "--predict-dry-run needs --predict-bfile" in r.stderr


def test_missing_bet(chain):
    base, out, target = chain
    os.remove(out + "/n.bet")
    r = run(*base, "--predict-bfile", target)
    assert r.returncode != 0 and "n.bet" in r.stderr and "run the chain first" in r.stderr


def test_no_record_at_or_after_burn_in(chain):
    base, _, target = chain
    r = run(*(base[:-1] + ["4"]), "--predict-bfile", target)
    assert r.returncode != 0 and "no record at or after --burn-in 4 (4 records)" in r.stderr
    r = run(*(base[:-1] + ["3"]), "--predict-bfile", target, "--predict-dry-run")
    assert r.returncode == 0 and "PREDICT: 1 records" in r.stdout and "iterations 3 .. 3" in r.stdout


def test_bet_of_another_chain_is_refused(chain):
    base, out, target = chain
    write_bet(out + "/n.bet", [0, 1, 2, 3], M=M + 1)
    r = run(*base, "--predict-bfile", target)
    assert r.returncode != 0 and "holds 13 markers" in r.stderr


def test_duplicate_target_ids_are_refused(chain):
    base, _, target = chain
    write_bim(target + ".bim", [("snp%d" % (j % 11), "A", "C") for j in range(M)])
    r = run(*base, "--predict-bfile", target)
    assert r.returncode != 0 and "lists SNP id snp0 twice" in r.stderr


def test_disjoint_target_is_refused(chain):
    base, _, target = chain
    write_bim(target + ".bim", [("other%d" % j, "A", "C") for j in range(M)])
    r = run(*base, "--predict-bfile", target)
    assert r.returncode != 0 and "no marker of" in r.stderr and "12 not in training" in r.stdout


def test_match_report_before_the_device(chain):
    """permuted, some alleles swapped, one allele pair that matches neither way, some markers dropped, one foreign id"""
    base, _, target = chain
    order = [7, 2, 9, 0, 11, 5, 3, 10]  # 1, 4, 6, 8 dropped
    rows = []
    for t, j in enumerate(order):
        if t in (1, 4, 6):
            rows.append(("snp%d" % j, "C", "A"))
        elif t == 2:
            rows.append(("snp%d" % j, "A", "T"))
        else:
            rows.append(("snp%d" % j, "A", "C"))
    rows.append(("rs_new", "A", "C"))
    write_bim(target + ".bim", rows)
    r = run(*base, "--predict-bfile", target, "--predict-dry-run")
    assert r.returncode == 0 and "dry run: inputs checked, nothing scored" in r.stdout
    assert ("PREDICT: 9 target markers: 7 matched (4 same alleles, 3 swapped), 1 allele mismatch, 1 not in training; "
            "5 of 12 training markers unused") in r.stdout
    assert "PREDICT: 2 records" in r.stdout and "iterations 2 .. 3" in r.stdout and "9 target individuals" in r.stdout
    assert not os.path.exists(os.path.join(os.path.dirname(target), "o", "n.prs"))


def test_dry_run_checks_the_target_bed(chain):
    base, _, target = chain
    with open(target + ".bed", "r+b") as f:
        f.truncate(10)
    r = run(*base, "--predict-bfile", target, "--predict-dry-run")
    assert r.returncode != 0 and "t.bed is shorter" in r.stderr
