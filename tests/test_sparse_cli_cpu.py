"""The command line's sparse routes, the part that runs before any device is touched: every refusal of --sparse-dir/--sparse-basename
and of --bed-to-sparse names the file and the fact.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import sparse_restate as sr
from hydra_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hydra_amd", "bin", "hydra_mi355x")
N, M = 30, 12


def run(*args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=60, env=e)


@pytest.fixture(scope="module")
def lists():
    geno = synth.make_genotypes(M, N, seed=1, missing_rate=0.05)
    return synth.pack_bed_columns(geno), sr.bed_to_lists(synth.pack_bed_columns(geno), N)


@pytest.fixture()
def files(tmp_path, lists):
    """a PLINK set x, its phenotype file and its ten sparse files s.*, fresh for every test (the tests damage them)"""
    bed, ls = lists
    y = np.arange(N, dtype=float)
    synth.write_plink(str(tmp_path / "x"), bed, N, y=y, na_rows=(3,))
    sr.write_files(str(tmp_path / "s"), ls, N, M)
    return tmp_path


def chain_args(d, bfile=False, n=N, m=M, base="s"):
    a = ["--mpibayes", "bayesMPI", "--pheno", str(d / "x.phen"), "--mcmc-out-dir", str(d / "out"), "--mcmc-out-name", "c", "--sparse-dir", str(d),
         "--sparse-basename", base, "--number-individuals", str(n), "--number-markers", str(m), "--chain-length", "1", "--seed", "1"]
    return a + (["--bfile", str(d / "x")] if bfile else [])


def reaches_the_device(r):
    """every check passed: the run went on to create a device (which this machine may lack)"""
    return "hgibbs_create" in r.stderr or r.returncode == 0


def test_good_files_pass_every_check(files):
    for bfile in (False, True):
        r = run(*chain_args(files, bfile))
        assert reaches_the_device(r), r.stderr
        assert "genotypes are read from the sparse files" in r.stdout
        assert ("only .fam/.bim from --bfile" in r.stdout) == bfile
    r = run(*chain_args(files, m=M - 2))  # fewer markers than the files hold
    assert reaches_the_device(r), r.stderr


def test_truncated_index_file(files):
    p = files / "s.si1"
    p.write_bytes(p.read_bytes()[:-4])
    r = run(*chain_args(files))
    assert r.returncode != 0 and "s.si1" in r.stderr and "fewer than 4 x (ss[last] + sl[last])" in r.stderr
    assert "hgibbs_create" not in r.stderr


def test_short_count_file(files):
    p = files / "s.slm"
    p.write_bytes(p.read_bytes()[:-1])
    r = run(*chain_args(files))
    assert r.returncode != 0 and "s.slm" in r.stderr and "fewer than 8 x --number-markers" in r.stderr


def test_missing_file(files):
    os.remove(files / "s.ss2")
    r = run(*chain_args(files))
    assert r.returncode != 0 and "can not open the file" in r.stderr and "s.ss2" in r.stderr


def test_dim(files):
    r = run(*chain_args(files, n=N + 1))  # (without --bfile N is the option's: the phenotype file is then one line short)
    assert r.returncode != 0 and "phenotype file covers" in r.stderr
    (files / "s.dim").write_text("%d %d\n" % (N + 1, M))
    r = run(*chain_args(files))
    assert r.returncode != 0 and "s.dim says N = %d" % (N + 1) in r.stderr and "--number-individuals says %d" % N in r.stderr
    (files / "s.dim").write_text("%d %d\n" % (N, M - 1))
    r = run(*chain_args(files))
    assert r.returncode != 0 and "s.dim says M = %d" % (M - 1) in r.stderr and "--number-markers %d exceeds it" % M in r.stderr
    (files / "s.dim").write_text("thirty twelve\n")
    r = run(*chain_args(files))
    assert r.returncode != 0 and "s.dim does not parse" in r.stderr
    for r in (r,):
        assert "hgibbs_create" not in r.stderr


def test_overlapping_starts(files, lists):
    ss = lists[1]["ss1"].copy()
    j = int(np.flatnonzero(lists[1]["sl1"][:-1] > 0)[0])
    ss[j + 1] -= 1
    (files / "s.ss1").write_bytes(ss.tobytes())
    r = run(*chain_args(files))
    assert r.returncode != 0 and "s.ss1: marker %d starts at %d, before marker %d ends" % (j + 1, ss[j + 1], j) in r.stderr


def test_count_beyond_n(files, lists):
    sl = lists[1]["sl2"].copy()
    sl[4] = N + 1
    (files / "s.sl2").write_bytes(sl.tobytes())
    r = run(*chain_args(files))
    assert r.returncode != 0 and "s.sl2: marker 4 lists %d rows, more than N = %d" % (N + 1, N) in r.stderr


def test_pairing(files):
    a = chain_args(files)
    i = a.index("--sparse-dir")
    r = run(*(a[:i] + a[i + 2:]))  # --sparse-basename alone
    assert r.returncode != 0 and "--sparse-dir and --sparse-basename must either be both set or unset" in r.stderr
    r = run("--mpibayes", "bayesMPI", "--sparse-basename", "s")  # ... before the mandatory output options are looked at
    assert r.returncode != 0 and "must either be both set or unset" in r.stderr
    for flag in ("--sparse-sync", "--bed-sync"):
        r = run(*a, flag)
        assert r.returncode != 0 and "does not reproduce" in r.stderr and flag in r.stderr


def test_neither_representation():
    r = run("--mpibayes", "bayesMPI", "--pheno", "p", "--mcmc-out-dir", "o", "--mcmc-out-name", "n")
    assert r.returncode != 0 and "either go for BED, SPARSE or BOTH" in r.stderr


def test_modes_need_bfile(files):
    for mode in (["--qc"], ["--king"], ["--grm"], ["--predict-bfile", str(files / "x")], ["--ld-window", "5"]):
        r = run(*chain_args(files), *mode)
        assert r.returncode != 0 and mode[0] + " needs --bfile" in r.stderr, (mode, r.stderr)
    r = run(*chain_args(files, bfile=True), "--qc")  # with it the mode passes every check
    assert reaches_the_device(r), r.stderr


def test_accepted_flags(files):
    r = run(*chain_args(files, bfile=True), "--read-from-bed-file", "--blocks-per-rank", "2")
    assert "invalid option" not in r.stderr and reaches_the_device(r), r.stderr
    assert "genotypes are read from the sparse files" not in r.stdout  # --read-from-bed-file selects the BED
    r = run(*chain_args(files), "--read-from-bed-file")  # ... which then has to be there
    assert r.returncode != 0 and "either go for BED, SPARSE or BOTH" in r.stderr


def test_bed_to_sparse_refusals(files):
    conv = ["--bed-to-sparse", "--bfile", str(files / "x"), "--pheno", str(files / "x.phen")]
    r = run(*conv, "--sparse-dir", str(files / "absent"), "--sparse-basename", "t")
    assert r.returncode != 0 and "requested directory for sparse output" in r.stderr and "absent" in r.stderr and "Must be an existing directory" in r.stderr
    r = run(*conv, "--sparse-dir", str(files))
    assert r.returncode != 0 and "must either be both set or unset" in r.stderr
    r = run(*conv, env={"WORLD_SIZE": "2"})
    assert r.returncode != 0 and "--bed-to-sparse runs on one process (WORLD_SIZE = 2)" in r.stderr
    r = run("--bed-to-sparse", "--pheno", str(files / "x.phen"))
    assert r.returncode != 0 and "--bed-to-sparse needs --bfile" in r.stderr
    r = run(*conv, "--blocks-per-rank", "3")  # valid: goes on to the device, needs no --mpibayes, --mcmc-out-* or --number-*
    assert reaches_the_device(r), r.stderr
    assert "--blocks-per-rank ignored" in r.stdout
