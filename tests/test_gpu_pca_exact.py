"""hgibbs_pca bit for bit against tests/pca_restate.py: the call replayed with the two panel products taken from the device's public
operators on the same handle (Device.marker_dots, Device.score: the pipelines hgibbs_pca runs on device pointers, pinned exactly by
test_gpu_marker_dots.py and test_gpu_score.py) and every other step (start panel, k_pca_fold, k_pca_gram with k_pca_gram_sum,
pca_chol_inv, k_pca_apply, pca_jacobi, the stop rule, the Ritz vectors, the sign rule, k_pca_resid and the report's K-wide pass) done
in NumPy in the order the source states.  Every output must have the same bits, NaN loadings included; there is no tolerance in this
file.  The restatement itself is checked without a device in test_pca_restatement_cpu.py, which also shows that no case of the grid
ends in a refusal and that a comparison of bits notices a reordered sum.

The grid (pca_restate.grid) goes where the kernels branch: every panel width 1 .. 32 (the eb + c < L guards and the zero columns of
k_pca_gram's LDS tile, the l < L predicate of k_pca_apply), n and M at 64 (PG_TILE, k_pca_fold's block), 256 (PG_TPB) and 1024
(PG_ROWS) and one to either side, n = L + 1, M_used = L, eight, nine and sixteen workgroups of k_pca_gram on either panel (the
eight-at-a-time loop of k_pca_gram_sum with and without a tail), K < L (the report's K-wide pass through fold, gram and resid, and
the row-major branch of k_pca_gram on a short panel).  Every cohort has 2 % missing calls, a marker missing everywhere inside the
last block of 64, a monomorphic marker and an individual missing everywhere; some are loaded through a keep list.

No case for a refusal from inside the iteration: test_pca_restatement_cpu.py found no clean input that loses rank in iteration 2 or
later (duplicated individuals lose it in iteration 1, at a pivot that depends on the rounding of the products)."""
import time

import numpy as np
import pytest

from pca_restate import GRID, OPTIONS, SEEDED, STOP, device, planted, restate, same_bits, start_for, start_panel

pytestmark = pytest.mark.gpu


def load(c):
    geno, keep, kept = planted(c["n"], c["M"], c["drop"], c["seed"])
    dev = device(geno, keep=keep)
    assert dev.n_local == c["n"] and dev.M == c["M"] and dev.row_begin == 0
    return dev


def replay(dev, K, L, iters, tol, start):
    mave, mstd, *_ = dev.marker_stats()
    want = restate((dev.marker_dots, dev.score), mave, mstd, dev.n_local, dev.M, K, L, iters, tol, start)
    assert "refused" not in want, want
    return want


def largest(a, b):
    both = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


def check(dev, K, L, iters, tol, Q0=None, seed=None, want=None, label=""):
    """hgibbs_pca against its restatement on the same handle: the same bits of every output, the same report"""
    t0 = time.perf_counter()
    if Q0 is not None:
        val, pcs, ld, rep = dev.pca(K, L=L, iters=iters, tol=tol, Q0=Q0, loadings=True)
    else:
        val, pcs, ld, rep = dev.pca(K, L=L, iters=iters, tol=tol, seed=seed, loadings=True)
    t1 = time.perf_counter()
    if want is None:
        want = replay(dev, K, L, iters, tol, Q0 if Q0 is not None else start_panel(seed, L, dev.n_local, dev.row_begin))
    t2 = time.perf_counter()
    got = {"eigval": val, "pcs": pcs, "loadings": ld, "resid": rep["resid"]}
    print("%s n = %d, M = %d, K = %d, L = %d: largest |device - restatement| %s; %d iterations, m_used %d; device call %.3f s, replay %.3f s"
          % (label, dev.n_local, dev.M, K, L, ", ".join("%s %.3g" % (k, largest(got[k], want[k])) for k in got), rep["iters_run"], rep["m_used"],
             t1 - t0, t2 - t1))
    for name in got:
        assert same_bits(got[name], want[name]), name
    assert np.array_equal(np.isnan(ld), np.broadcast_to(~np.isfinite(dev.marker_stats()[1]), ld.shape))
    assert rep["iters_run"] == want["iters_run"] and rep["m_used"] == want["m_used"]
    assert rep["ritz_change"] == want["ritz_change"]
    return want, rep


@pytest.mark.parametrize("name", list(GRID))
def test_grid(name):
    c = GRID[name]
    dev = load(c)
    want, rep = check(dev, c["K"], c["L"], c["iters"], c["tol"], Q0=start_for(c), label=name)
    assert rep["iters_run"] == c["iters"]
    if c["iters"] == 1:
        assert rep["ritz_change"] == np.inf
    if name == "m7":
        assert rep["m_used"] == c["L"]
    dev.close()


def test_stop_rule():
    c = STOP
    dev = load(c)
    want, rep = check(dev, c["K"], c["L"], c["iters"], c["tol"], Q0=start_for(c), label="stop")
    print("stopped after %d of %d iterations, last change %.17g" % (rep["iters_run"], c["iters"], rep["ritz_change"]))
    assert 1 < rep["iters_run"] < c["iters"]
    assert rep["ritz_change"] <= c["tol"]
    dev.close()


def test_seeded_start():
    """seed without Q0: k_pca_init hashes the handle's row, row_begin + i with i counting the KEPT rows (row_begin is 0 on one rank), not
    the row of the file the BED was loaded from"""
    c = SEEDED
    dev = load(c)
    assert c["drop"] and dev.n_local == c["n"]
    want, _ = check(dev, c["K"], c["L"], c["iters"], c["tol"], seed=77, label="seeded")
    twin, _ = check(dev, c["K"], c["L"], c["iters"], c["tol"], Q0=start_panel(77, c["L"], c["n"]), want=want, label="twin")
    other = dev.pca(c["K"], L=c["L"], iters=c["iters"], tol=c["tol"], seed=78, loadings=True)
    assert not same_bits(other[1], want["pcs"])
    dev.close()


def test_options():
    """the launch geometry of the two products is not an input: one restatement, the same bits under every option"""
    c = OPTIONS
    dev = load(c)
    Q0 = start_for(c)
    want, _ = check(dev, c["K"], c["L"], c["iters"], c["tol"], Q0=Q0, label="options: default")
    for name, values in [("mdots_split", [1, 3]), ("score_sp", [2, 16]), ("score_ranges", [1, 5])]:
        for v in values:
            dev.set_option(name, v)
            check(dev, c["K"], c["L"], c["iters"], c["tol"], Q0=Q0, want=want, label="options: %s = %d" % (name, v))
        dev.set_option(name, 0)
    dev.close()
