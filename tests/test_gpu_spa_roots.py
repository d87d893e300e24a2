"""hgibbs_spa_roots against the NumPy restatement of tests/spa_restate.py: flags, saddlepoints, K and K'' per tail and the numbers of
pass 0 on a grid of cohort sizes and null-model widths; bit-identity across chunkings, orders, duplicates and repeats; every refusal,
each followed by a call that works."""
import ctypes as C

import numpy as np
import pytest

from hydra_amd import capi, synth

import spa_restate as R

pytestmark = pytest.mark.gpu

# Ten times the largest relative difference between the float64 and the longdouble restatement over the markers of this grid, as
# tests/test_spa_restatement_cpu.py prints it.  Measured on the CPU: t 2.65e-13, K 3.98e-12, K'' 2.42e-13, p 1.11e-11.  The margin of
# ten covers the device's other summation order and the last places of its expm1, log1p and division.
TOL_T = 2.7e-12
TOL_K = 4.0e-11
TOL_K2 = 2.5e-12
TOL_P = 1.2e-10


def device(geno):
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), geno.shape[1])
    return dev


def call(dev, case, idx):
    idx = np.asarray(idx)
    return dev.spa_roots(idx, case["Z"], case["mu"], case["B"][idx], case["xv"][idx], case["s"][idx])


def raw(recs, k=None):
    b = bytes(recs)
    size = C.sizeof(capi.SpaRoot)
    return b if k is None else b[k * size:(k + 1) * size]


def close(got, want, tol):
    return abs(got - float(want)) <= tol * abs(float(want))


@pytest.mark.parametrize("n", R.GRID_N)
@pytest.mark.parametrize("q", R.GRID_Q)
def test_grid_against_the_restatement(n, q):
    case = R.roots_case(n, q)
    ref = R.case_roots(case)
    dev = device(case["geno"])
    everything = np.arange(R.GRID_M)
    recs = call(dev, case, everything)
    assert dev.last_spa_ms() > 0.0
    seen = set()
    for j, want in enumerate(ref):
        got = recs[j]
        assert got.flags == want["flags"] and got.reserved_ == 0, (j, got.flags, want["flags"])
        seen.add(got.flags)
        for name in ("k2_0", "s_lo", "s_hi"):
            assert close(getattr(got, name), want[name], 1e-12), (j, name)
        for z in range(2):
            assert 0 <= got.iters[z] <= R.PASSES
            if got.flags >> z & 1:
                assert close(got.t[z], want["t"][z], TOL_T), (j, z, got.t[z], want["t"][z])
                assert close(got.K[z], want["K"][z], TOL_K), (j, z, got.K[z], want["K"][z])
                assert close(got.K2[z], want["K2"][z], TOL_K2), (j, z)
                assert got.iters[z] >= 2
            elif got.flags >> (2 + z) & 1:  # unreachable: never iterated
                assert (got.t[z], got.K[z], got.K2[z], got.iters[z]) == (0.0, 0.0, 0.0, 0)
        gp, wp = capi.spa_pvalue(case["s"][j], got), R.pvalue(case["s"][j], want)
        assert gp[3] == wp[3], j
        if wp[3]:
            assert close(gp[2], wp[2], TOL_P), (j, gp, wp)
    assert 3 in seen and 12 in seen  # converged tails and the unreachable entry
    # bit-identity: reversed, in calls of 1 and of 7, repeated, and a duplicate index
    whole = raw(recs)
    rev = call(dev, case, everything[::-1])
    assert all(raw(rev, R.GRID_M - 1 - j) == raw(recs, j) for j in range(R.GRID_M))
    assert b"".join(raw(call(dev, case, [j])) for j in range(0, R.GRID_M, 9)) == b"".join(raw(recs, j) for j in range(0, R.GRID_M, 9))
    assert b"".join(raw(call(dev, case, everything[k:k + 7])) for k in range(0, R.GRID_M, 7)) == whole
    assert raw(call(dev, case, everything)) == whole
    dup = call(dev, case, [11, 40, 11])
    assert raw(dup, 0) == raw(dup, 2) == raw(recs, 11) and raw(dup, 1) == raw(recs, 40)
    dev.close()


# The same for the admitted entries of spa_restate.rule_cases(), as test_rule_cases_admitted_entries_are_well_conditioned prints it.
# Measured on the CPU: t 6.10e-13, K 1.02e-12, K'' 1.29e-11, p 3.09e-12 (the sums of pass 0: 1.9e-15 at the most).  The margin of ten
# and its reason are those above.
RULE_TOL_T = 6.1e-12
RULE_TOL_K = 1.1e-11
RULE_TOL_K2 = 1.3e-10
RULE_TOL_P = 3.1e-11


def against(case, recs, tol_t, tol_k, tol_k2, tol_p, passes):
    """every record of a call on the whole of `case` against the float64 restatement; with `passes` the numbers of passes too"""
    for e in range(R.case_size(case)):
        got, want = recs[e], R.roots(R.case_a(case, e), case["mu"], case["s"][e])
        where = (case["n"], case["Z"].shape[1], e)
        assert got.flags == want["flags"] and got.reserved_ == 0, (where, got.flags, want["flags"])
        if passes:
            assert list(got.iters) == want["iters"], (where, list(got.iters), want["iters"])
        for name in ("k2_0", "s_lo", "s_hi"):
            assert close(getattr(got, name), want[name], 1e-12), (where, name)
        for z in range(2):
            if got.flags >> z & 1:
                assert close(got.t[z], want["t"][z], tol_t), (where, z, got.t[z], want["t"][z])
                assert close(got.K[z], want["K"][z], tol_k), (where, z, got.K[z], want["K"][z])
                assert close(got.K2[z], want["K2"][z], tol_k2), (where, z, got.K2[z], want["K2"][z])
            else:
                assert got.flags >> (2 + z) & 1 and (got.t[z], got.K[z], got.K2[z], got.iters[z]) == (0.0, 0.0, 0.0, 0), where
        gp, wp = capi.spa_pvalue(case["s"][e], got), R.pvalue(case["s"][e], want)
        assert gp[3] == wp[3], where
        if wp[3]:
            assert close(gp[2], wp[2], tol_p), (where, gp, wp)


def same_bits_however_called(dev, case, recs):
    """reversed, entry by entry and repeated"""
    m = R.case_size(case)
    everything = np.arange(m)
    rev = call(dev, case, everything[::-1])
    assert all(raw(rev, m - 1 - e) == raw(recs, e) for e in range(m))
    assert b"".join(raw(call(dev, case, [e])) for e in range(m)) == raw(recs)
    assert raw(call(dev, case, everything)) == raw(recs)


def test_admitted_entries_against_the_restatement():
    """Tiny entries that take the rule's branches one by one (spa_restate.ADMITTED: midpoints, one-tailed entries, the score 0 whose
    first proposal is the bracket's end) and on which the float64 rule, the longdouble rule and twenty perturbed copies of either agree
    in every pass: flags and passes are the restatement's, the numbers lie within the tolerance measured for these entries."""
    for case in R.rule_cases()[0]:
        dev = device(case["geno"])
        recs = call(dev, case, np.arange(R.case_size(case)))
        against(case, recs, RULE_TOL_T, RULE_TOL_K, RULE_TOL_K2, RULE_TOL_P, passes=True)
        same_bits_however_called(dev, case, recs)
        dev.close()


def test_ill_conditioned_entries_end_in_one_of_three_ways():
    """spa_restate.ILL: scores a hair inside the reachable edge, first steps that saturate every row, entries that the float64 rule leaves
    open.  No value and no outcome is the restatement's here; each tail is unreachable, converged or open, and says so consistently."""
    tails = opened = 0
    for case in R.rule_cases()[1]:
        dev = device(case["geno"])
        recs = call(dev, case, np.arange(R.case_size(case)))  # (a refusal or a device error raises)
        for e in range(R.case_size(case)):
            got = recs[e]
            where = (case["n"], e)
            assert got.flags < 16 and got.reserved_ == 0, where
            for z in range(2):
                unreachable, converged = got.flags >> (2 + z) & 1, got.flags >> z & 1
                assert not (unreachable and converged), where
                if unreachable:
                    assert (got.t[z], got.K[z], got.K2[z], got.iters[z]) == (0.0, 0.0, 0.0, 0), where
                elif converged:
                    assert 1 <= got.iters[z] <= R.PASSES, where
                else:
                    assert got.iters[z] == R.PASSES and got.K[z] == got.K2[z] == 0.0, where
                    opened += 1
                tails += not unreachable
            if capi.spa_pvalue(case["s"][e], got)[3]:
                assert got.flags == 3, where
        same_bits_however_called(dev, case, recs)
        dev.close()
    print("ill-conditioned entries: %d of %d reachable tails are left open on the device" % (opened, tails))


@pytest.mark.parametrize("n,q", R.EDGE_SHAPES)
def test_edges_of_q_and_n(n, q):
    """q = 64 = SPA_QMAX and its neighbours, and cohorts of two rows, of one full BED dword and of one row more, against the restatement
    within the grid's tolerances (test_float64_against_longdouble_on_the_edges_of_q_and_n: the gap stays under a tenth of them)"""
    case = R.edge_case(n, q)
    dev = device(case["geno"])
    recs = call(dev, case, np.arange(R.EDGE_M))
    against(case, recs, TOL_T, TOL_K, TOL_K2, TOL_P, passes=False)
    dev.close()


def test_refusals_leave_the_handle_usable():
    case = R.roots_case(261, 5)
    dev = device(case["geno"])
    n, q = case["Z"].shape
    idx = np.arange(8)
    good = dict(markers=idx, Z=case["Z"], mu=case["mu"], B=case["B"][idx], xv=case["xv"][idx], s=case["s"][idx])
    want = raw(dev.spa_roots(**good))

    def spoiled(name, at, value):
        a = np.array(good[name], dtype=np.float64 if name != "markers" else np.uint32)
        a[at] = value
        return dict(good, **{name: a})

    def usable():
        sums = dev.marker_class_sums(np.ones((1, n)))
        assert sums.shape == (R.GRID_M, 1, 4) and np.all(sums.sum(axis=2) == n)
        assert raw(dev.spa_roots(**good)) == want
        assert dev.last_spa_ms() > 0.0

    bad = [
        (spoiled("markers", 3, R.GRID_M), "markers[3] = 64 out of range (M = 64)"),
        (spoiled("Z", (5, 2), np.nan), "Z[5][2] = nan is not finite"),
        (spoiled("B", (1, 4), np.inf), "B[1][4] = inf is not finite"),
        (spoiled("xv", (2, 3), np.nan), "xv[2][3] = nan is not finite"),
        (spoiled("s", 7, -np.inf), "s[7] = -inf is not finite"),
        (spoiled("mu", 9, 0.0), "mu[9] = 0 is not strictly inside (0, 1)"),
        (spoiled("mu", 9, 1.0), "mu[9] = 1 is not strictly inside (0, 1)"),
        (spoiled("mu", 9, np.nan), "mu[9] = nan is not strictly inside (0, 1)"),
        (dict(good, Z=np.ones((n, 65)), B=np.zeros((8, 65))), "q = 65, must be in [1, 64]"),
    ]
    for args, msg in bad:
        with pytest.raises(capi.HgError, match="hgibbs_spa_roots: "):
            try:
                dev.spa_roots(**args)
            except capi.HgError as e:
                assert msg in str(e), (msg, str(e))
                raise
        assert dev.last_spa_ms() == 0.0  # 0 after a refused call
        usable()
    # null arguments and q = 0 straight through the ABI
    L, dp = capi.lib(), C.POINTER(C.c_double)
    out = (capi.SpaRoot * 8)()
    ptr = dict(markers=idx.astype(np.uint32).ctypes.data_as(capi.C_U32P))
    keep = {k: np.ascontiguousarray(good[k].T if k == "Z" else good[k], dtype=np.float64) for k in ("Z", "mu", "B", "xv", "s")}
    ptr.update({k: v.ctypes.data_as(dp) for k, v in keep.items()})
    order = ("Z", "mu", "B", "xv", "s")
    for missing in ("markers",) + order + ("out",):
        a = dict(ptr, out=out)
        a[missing] = None
        assert L.hgibbs_spa_roots(dev.h, 8, a["markers"], q, *[a[k] for k in order], a["out"]) != 0
        assert "hgibbs_spa_roots: null argument" in L.hgibbs_last_error().decode()
        assert dev.last_spa_ms() == 0.0
        usable()
    assert L.hgibbs_spa_roots(dev.h, 8, ptr["markers"], 0, *[ptr[k] for k in order], out) != 0
    assert "hgibbs_spa_roots: q = 0, must be in [1, 64]" in L.hgibbs_last_error().decode()
    assert dev.last_spa_ms() == 0.0
    usable()
    assert L.hgibbs_spa_roots(None, 8, ptr["markers"], q, *[ptr[k] for k in order], out) != 0
    assert "hgibbs_spa_roots: null handle" in L.hgibbs_last_error().decode()
    assert L.hgibbs_last_spa_ms(dev.h, None) != 0 and L.hgibbs_last_spa_ms(None, C.byref(C.c_double())) != 0
    # an empty list touches nothing
    before = raw(out)
    assert L.hgibbs_spa_roots(dev.h, 0, ptr["markers"], q, *[ptr[k] for k in order], out) == 0 and raw(out) == before
    usable()
    dev.close()
    # a handle without genotypes
    empty = capi.Device(0)
    assert L.hgibbs_spa_roots(empty.h, 8, ptr["markers"], q, *[ptr[k] for k in order], out) != 0
    assert "hgibbs_spa_roots: no genotypes loaded on this handle" in L.hgibbs_last_error().decode()
    assert empty.last_spa_ms() == 0.0  # (as test_gpu_firth.py has it; the alternation with usable() above is what pins the zeroing)
    empty.close()


def test_several_ranks_refused():
    case = R.roots_case(261, 1)
    dev = capi.Device(0)
    dev.comm_init_external(2, 0, lambda arr: None)  # a stub world of two ranks
    dev.load_bed(synth.pack_bed_columns(case["geno"]), 261, row_begin=0, row_end=130, n_global=261)
    with pytest.raises(capi.HgError, match="hgibbs_spa_roots: one rank only"):
        dev.spa_roots([0], case["Z"][:dev.n_local], case["mu"][:dev.n_local], case["B"][:1], case["xv"][:1], case["s"][:1])
