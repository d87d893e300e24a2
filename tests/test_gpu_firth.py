"""hgibbs_firth_fit against the NumPy restatement of tests/firth_restate.py: flags, the fitted effect, K and K'' there, K''(0) and the
p-value of hgibbs_firth_stats on a grid of cohort sizes and null-model widths; bit-identity across chunkings, orders, duplicates, repeats
and the option firth_piece; every refusal, each followed by a call that works."""
import ctypes as C

import numpy as np
import pytest

from hydra_amd import capi, synth

import firth_restate as F
import spa_restate as R

pytestmark = pytest.mark.gpu

# Ten times the largest relative difference between the float64 and the longdouble restatement over the entries of this grid, as
# tests/test_firth_restatement_cpu.py prints it.  Measured on the CPU: beta 8.24e-13, K 9.86e-13, K'' 1.87e-12, p 8.58e-14.  The margin
# of ten covers the device's other summation order and the last places of its expm1, log1p and division.
TOL_BETA = 8.3e-12
TOL_K = 9.9e-12
TOL_K2 = 1.9e-11
TOL_P = 8.6e-13
NE = F.GRID_M + 1


def device(geno):
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), geno.shape[1])
    return dev


def call(dev, case, idx):
    idx = np.asarray(idx)
    return dev.firth_fit(case["markers"][idx], case["Z"], case["mu"], case["B"][idx], case["xv"][idx], case["s"][idx])


def raw(recs, k=None):
    b = bytes(recs)
    size = C.sizeof(capi.FirthRec)
    return b if k is None else b[k * size:(k + 1) * size]


def close(got, want, tol):
    return abs(got - float(want)) <= tol * abs(float(want))


def test_the_record_is_48_bytes():
    assert C.sizeof(capi.FirthRec) == 48


@pytest.mark.parametrize("n", F.GRID_N)
@pytest.mark.parametrize("q", F.GRID_Q)
def test_grid_against_the_restatement(n, q):
    case = F.fit_case(n, q)
    ref = F.case_fits(case)
    dev = device(case["geno"])
    everything = np.arange(NE)
    recs = call(dev, case, everything)
    ms = dev.last_firth_ms()
    print("n %d q %d: %d entries in %.3f ms on the device" % (n, q, NE, ms))
    assert ms > 0.0
    worst = dict(beta=0.0, K=0.0, K2=0.0, p=0.0)
    for e, want in enumerate(ref):
        got = recs[e]
        assert got.flags == want["flags"], (e, got.flags, want["flags"])
        if got.flags & F.DEGENERATE:
            assert e == F.FLAT and raw(recs, e) == bytes(40) + (0).to_bytes(4, "little") + (2).to_bytes(4, "little")
            assert capi.firth_stats(case["s"][e], got)[3] is False
            continue
        assert got.flags == F.CONVERGED and 1 <= got.iters <= F.PASSES, (e, got.iters)
        assert close(got.k2_0, want["k2_0"], 1e-12), e
        gp, wp = capi.firth_stats(case["s"][e], got), F.stats(case["s"][e], want)
        for name, a, b in (("beta", got.beta, want["beta"]), ("K", got.K, want["K"]), ("K2", got.K2, want["K2"]), ("p", gp[2], wp[2])):
            worst[name] = max(worst[name], F.rel(a, b))
        assert close(got.beta, want["beta"], TOL_BETA), (e, got.beta, want["beta"])
        assert close(got.K, want["K"], TOL_K), (e, got.K, want["K"])
        assert close(got.K2, want["K2"], TOL_K2), (e, got.K2, want["K2"])
        assert gp[3] and wp[3], e
        assert close(gp[2], wp[2], TOL_P), (e, gp, wp)
    print("largest relative difference device / restatement: beta %.3g, K %.3g, K2 %.3g, p %.3g" % (worst["beta"], worst["K"], worst["K2"], worst["p"]))
    # bit-identity: reversed, in calls of 1 and of 7, repeated, a duplicate index, and pieces of 1, of 3 and automatic
    whole = raw(recs)
    rev = call(dev, case, everything[::-1])
    assert all(raw(rev, NE - 1 - e) == raw(recs, e) for e in range(NE))
    assert b"".join(raw(call(dev, case, [e])) for e in range(0, NE, 9)) == b"".join(raw(recs, e) for e in range(0, NE, 9))
    assert b"".join(raw(call(dev, case, everything[k:k + 7])) for k in range(0, NE, 7)) == whole
    assert raw(call(dev, case, everything)) == whole
    dup = call(dev, case, [11, 40, 11])
    assert raw(dup, 0) == raw(dup, 2) == raw(recs, 11) and raw(dup, 1) == raw(recs, 40)
    for piece in (1, 3, 0):
        dev.set_option("firth_piece", piece)
        assert raw(call(dev, case, everything)) == whole, piece
    dev.close()


@pytest.mark.parametrize("q", (1, 5))
def test_k2_0_is_that_of_spa_roots_bit_for_bit(q):
    """Both kernels form a_i from one function (spa_adjusted, hg_spa.hip.h) and their terms from one logistic point: at t = 0 each sums
    a^2 mu (1 - mu) over the same rows per thread and through the same tree, so K''(0) of the two records has the same bits.  261 rows
    are one full stride of the 256 threads and a tail; the 64 markers of the grid, without the flat entry at the list's end."""
    case = F.fit_case(261, q)
    dev = device(case["geno"])
    idx = np.arange(F.GRID_M)
    args = (case["markers"][idx], case["Z"], case["mu"], case["B"][idx], case["xv"][idx], case["s"][idx])
    firth, spa = dev.firth_fit(*args), dev.spa_roots(*args)
    for e in idx:
        assert firth[e].k2_0 > 0.0 and firth[e].k2_0.hex() == spa[e].k2_0.hex(), (e, firth[e].k2_0.hex(), spa[e].k2_0.hex())
    dev.close()


# The same for the admitted entries of firth_restate.rule_cases(), as test_rule_cases_admitted_entries_are_well_conditioned prints it.
# Measured on the CPU: beta 5.53e-13, K 6.92e-13, K'' 4.65e-12, p 4.55e-13.  The margin of ten and its reason are those above.
RULE_TOL_BETA = 5.6e-12
RULE_TOL_K = 7.0e-12
RULE_TOL_K2 = 4.7e-11
RULE_TOL_P = 4.6e-12


def against(case, recs, tol_beta, tol_k, tol_k2, tol_p, passes):
    """every record of a call on the whole of `case` against the float64 restatement, all converged; with `passes` the numbers of
    passes too"""
    for e in range(R.case_size(case)):
        got, want = recs[e], F.fit(R.case_a(case, e), case["mu"], case["s"][e])
        where = (case["n"], case["Z"].shape[1], e)
        assert got.flags == want["flags"] == F.CONVERGED, (where, got.flags, want["flags"])
        if passes:
            assert got.iters == want["iters"], (where, got.iters, want["iters"])
        assert close(got.k2_0, want["k2_0"], 1e-12), where
        gp, wp = capi.firth_stats(case["s"][e], got), F.stats(case["s"][e], want)
        assert gp[3] and wp[3], where
        assert close(got.beta, want["beta"], tol_beta), (where, got.beta, want["beta"])
        assert close(got.K, want["K"], tol_k), (where, got.K, want["K"])
        assert close(got.K2, want["K2"], tol_k2), (where, got.K2, want["K2"])
        assert close(gp[2], wp[2], tol_p), (where, gp, wp)


def same_bits_however_called(dev, case, recs):
    """reversed, entry by entry, repeated, and in pieces of 1, of 3 and automatic"""
    m = R.case_size(case)
    everything = np.arange(m)
    rev = call(dev, case, everything[::-1])
    assert all(raw(rev, m - 1 - e) == raw(recs, e) for e in range(m))
    assert b"".join(raw(call(dev, case, [e])) for e in range(m)) == raw(recs)
    assert raw(call(dev, case, everything)) == raw(recs)
    for piece in (1, 3, 0):
        dev.set_option("firth_piece", piece)
        assert raw(call(dev, case, everything)) == raw(recs), piece


def test_admitted_entries_against_the_restatement():
    """Tiny entries that take the rule's branches one by one (firth_restate.ADMITTED and NEAR_MINIMUM: +-scale from 0, midpoints, 2 t, the
    saturated point with its bracket end, no stop next to a local minimum) and on which the float64 rule, the longdouble rule and
    twenty perturbed copies of either agree in every pass: flags and passes are the restatement's, the numbers lie within the tolerance
    measured for these entries."""
    for case in F.rule_cases()[0]:
        dev = device(case["geno"])
        recs = call(dev, case, np.arange(R.case_size(case)))
        against(case, recs, RULE_TOL_BETA, RULE_TOL_K, RULE_TOL_K2, RULE_TOL_P, passes=True)
        same_bits_however_called(dev, case, recs)
        dev.close()


def test_ill_conditioned_entries_end_consistently():
    """firth_restate.ILL: scores a hair inside the reachable edge and beyond it, first steps that saturate every row, entries that the
    float64 rule leaves open.  No value and no outcome is the restatement's here: an entry is converged, degenerate or open and says so
    consistently, and a fit that hgibbs_firth_stats lets stand is a stationary point and a local maximum in longdouble."""
    entries = opened = stand = 0
    for case in F.rule_cases()[1]:
        dev = device(case["geno"])
        recs = call(dev, case, np.arange(R.case_size(case)))  # (a refusal or a device error raises)
        for e in range(R.case_size(case)):
            got = recs[e]
            where = (case["n"], e)
            entries += 1
            assert got.flags in (0, F.CONVERGED, F.DEGENERATE), (where, got.flags)
            if got.flags == 0:
                assert got.iters == F.PASSES and got.K == got.K2 == 0.0, where
                opened += 1
            elif got.flags == F.DEGENERATE:
                assert raw(recs, e) == bytes(40) + (0).to_bytes(4, "little") + (2).to_bytes(4, "little"), where
            else:
                assert 1 <= got.iters <= F.PASSES, where
            if capi.firth_stats(case["s"][e], got)[3]:
                assert got.flags == F.CONVERGED, where
                assert F.stationary(R.case_a(case, e, np.longdouble), case["mu"], case["s"][e], dict(beta=got.beta, k2_0=got.k2_0)), (where, got.beta)
                stand += 1
        same_bits_however_called(dev, case, recs)
        dev.close()
    print("ill-conditioned entries: %d of %d are left open on the device, %d fits stand" % (opened, entries, stand))


@pytest.mark.parametrize("n,q", R.EDGE_SHAPES)
def test_edges_of_q_and_n(n, q):
    """q = 64 = SPA_QMAX and its neighbours, and cohorts of two rows, of one full BED dword and of one row more, against the restatement
    within the grid's tolerances (test_float64_against_longdouble_on_the_edges_of_q_and_n: the gap stays under a tenth of them); at
    q = 64 K''(0) has the bits of hgibbs_spa_roots', as in test_k2_0_is_that_of_spa_roots_bit_for_bit"""
    case = R.edge_case(n, q)
    dev = device(case["geno"])
    recs = call(dev, case, np.arange(R.EDGE_M))
    against(case, recs, TOL_BETA, TOL_K, TOL_K2, TOL_P, passes=False)
    if q == 64:
        spa = dev.spa_roots(case["markers"], case["Z"], case["mu"], case["B"], case["xv"], case["s"])
        for e in range(R.EDGE_M):
            assert recs[e].k2_0 > 0.0 and recs[e].k2_0.hex() == spa[e].k2_0.hex(), (e, recs[e].k2_0.hex(), spa[e].k2_0.hex())
    dev.close()


def test_refusals_leave_the_handle_usable():
    case = F.fit_case(261, 5)
    dev = device(case["geno"])
    n, q = case["Z"].shape
    idx = np.arange(8)
    good = dict(markers=idx, Z=case["Z"], mu=case["mu"], B=case["B"][idx], xv=case["xv"][idx], s=case["s"][idx])
    want = raw(dev.firth_fit(**good))

    def spoiled(name, at, value):
        a = np.array(good[name], dtype=np.float64 if name != "markers" else np.uint32)
        a[at] = value
        return dict(good, **{name: a})

    def usable():
        sums = dev.marker_class_sums(np.ones((1, n)))
        assert sums.shape == (F.GRID_M, 1, 4) and np.all(sums.sum(axis=2) == n)
        assert raw(dev.firth_fit(**good)) == want
        assert dev.last_firth_ms() > 0.0

    bad = [
        (spoiled("markers", 3, F.GRID_M), "markers[3] = 64 out of range (M = 64)"),
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
        with pytest.raises(capi.HgError, match="hgibbs_firth_fit: "):
            try:
                dev.firth_fit(**args)
            except capi.HgError as e:
                assert msg in str(e), (msg, str(e))
                raise
        assert dev.last_firth_ms() == 0.0  # 0 after a refused call
        usable()
    # the option takes a number of entries from 0
    with pytest.raises(capi.HgError, match="firth_piece must be >= 0"):
        dev.set_option("firth_piece", -1)
    usable()
    # null arguments and q = 0 straight through the ABI
    L, dp = capi.lib(), C.POINTER(C.c_double)
    out = (capi.FirthRec * 8)()
    ptr = dict(markers=idx.astype(np.uint32).ctypes.data_as(capi.C_U32P))
    keep = {k: np.ascontiguousarray(good[k].T if k == "Z" else good[k], dtype=np.float64) for k in ("Z", "mu", "B", "xv", "s")}
    ptr.update({k: v.ctypes.data_as(dp) for k, v in keep.items()})
    order = ("Z", "mu", "B", "xv", "s")
    for missing in ("markers",) + order + ("out",):
        a = dict(ptr, out=out)
        a[missing] = None
        assert L.hgibbs_firth_fit(dev.h, 8, a["markers"], q, *[a[k] for k in order], a["out"]) != 0
        assert "hgibbs_firth_fit: null argument" in L.hgibbs_last_error().decode()
        assert dev.last_firth_ms() == 0.0
        usable()
    assert L.hgibbs_firth_fit(dev.h, 8, ptr["markers"], 0, *[ptr[k] for k in order], out) != 0
    assert "hgibbs_firth_fit: q = 0, must be in [1, 64]" in L.hgibbs_last_error().decode()
    assert dev.last_firth_ms() == 0.0
    usable()
    assert L.hgibbs_firth_fit(None, 8, ptr["markers"], q, *[ptr[k] for k in order], out) != 0
    assert "hgibbs_firth_fit: null handle" in L.hgibbs_last_error().decode()
    assert L.hgibbs_last_firth_ms(dev.h, None) != 0 and L.hgibbs_last_firth_ms(None, C.byref(C.c_double())) != 0
    # an empty list touches nothing
    before = raw(out)
    assert L.hgibbs_firth_fit(dev.h, 0, ptr["markers"], q, *[ptr[k] for k in order], out) == 0 and raw(out) == before
    usable()
    dev.close()
    # a handle without genotypes
    empty = capi.Device(0)
    assert L.hgibbs_firth_fit(empty.h, 8, ptr["markers"], q, *[ptr[k] for k in order], out) != 0
    assert "hgibbs_firth_fit: no genotypes loaded on this handle" in L.hgibbs_last_error().decode()
    assert empty.last_firth_ms() == 0.0
    empty.close()


def test_refuses_what_does_not_fit_in_device_memory():
    """The scratch is one row of n_local doubles per entry of a piece.  With automatic pieces it never outgrows the device; an explicit
    firth_piece can: six million entries in one piece on 8197 rows need 393 GB of it, more than any device this library runs on holds
    (an MI355X has 288 GB).  The host's share is 0.6 GB of list and records."""
    case = F.fit_case(8197, 1)
    dev = device(case["geno"])
    good = dict(markers=np.arange(8), Z=case["Z"], mu=case["mu"], B=case["B"][:8], xv=case["xv"][:8], s=case["s"][:8])
    want = raw(dev.firth_fit(**good))
    assert dev.last_firth_ms() > 0.0
    nm = 6_000_000
    dev.set_option("firth_piece", nm)
    with pytest.raises(capi.HgError, match=r"hgibbs_firth_fit: 6000000 markers against a null model of 1 columns and pieces of 6000000 entries need "
                                           r"375801\.3 MiB, [0-9.]+ MiB of device memory are free"):
        dev.firth_fit(np.zeros(nm, dtype=np.uint32), case["Z"], case["mu"], np.zeros((nm, 1)), np.ones((nm, 4)), np.zeros(nm))
    assert dev.last_firth_ms() == 0.0
    assert raw(dev.firth_fit(**good)) == want and dev.last_firth_ms() > 0.0  # (eight entries fit in a piece of six million)
    dev.set_option("firth_piece", 0)
    assert raw(dev.firth_fit(**good)) == want
    dev.close()


def test_several_ranks_refused():
    case = F.fit_case(261, 1)
    dev = capi.Device(0)
    dev.comm_init_external(2, 0, lambda arr: None)  # a stub world of two ranks
    dev.load_bed(synth.pack_bed_columns(case["geno"]), 261, row_begin=0, row_end=130, n_global=261)
    with pytest.raises(capi.HgError, match="hgibbs_firth_fit: one rank only"):
        dev.firth_fit([0], case["Z"][:dev.n_local], case["mu"][:dev.n_local], case["B"][:1], case["xv"][:1], case["s"][:1])
    assert dev.last_firth_ms() == 0.0
