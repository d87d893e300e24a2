"""hgibbs_spa_pvalue (host only) against the restatement's formula, each validity rule in turn, an underflowing tail and the refusals.
No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

from hydra_amd import capi

import spa_restate as R


def record(r):
    out = capi.SpaRoot()
    for z in range(2):
        out.t[z], out.K[z], out.K2[z], out.iters[z] = float(r["t"][z]), float(r["K"][z]), float(r["K2"][z]), r["iters"][z]
    out.k2_0, out.s_lo, out.s_hi, out.flags = float(r["k2_0"]), float(r["s_lo"]), float(r["s_hi"]), r["flags"]
    return out


def manual(t, K, K2, flags=3):
    """tails at tau = +-1000 built by hand: index 0 from (t, K, K2), index 1 its mirror image"""
    return dict(t=[t, -t], K=[K, K], K2=[K2, K2], k2_0=1.0, s_lo=-1e9, s_hi=1e9, iters=[3, 3], flags=flags)


def test_matches_the_restatement():
    cases = [((1960, 39, 1), (98, 8, 1), 0.05), ((1960, 39, 1), (98, 6, 0), 0.05), ((1000, 800, 200), (300, 280, 75), 0.3),
             ((500, 90, 10), (40, 15, 3), 0.1)]
    for counts, cas, mu in cases:
        a, codes, U, _ = R.intercept_only(counts, cas, mu)
        for s in (U, -U, 0.5 * U):
            r = R.roots(a[codes], np.full(codes.size, mu), s)
            up, dn, p, ok = R.pvalue(s, r)
            assert ok
            gup, gdn, gp, gok = capi.spa_pvalue(s, record(r))
            assert gok
            for got, want in ((gup, up), (gdn, dn), (gp, p)):
                assert abs(got - want) <= 1e-12 * want, (counts, cas, s)


@pytest.mark.parametrize("name,r", [
    ("the converged flag is not set", manual(1.0, 200.0, 1600.0, flags=2)),
    ("neither flag is set", manual(1.0, 200.0, 1600.0, flags=0)),
    ("t tau - K is not positive", manual(1.0, 1000.0, 1600.0)),
    ("K'' is not positive", manual(1.0, 200.0, 0.0)),
    ("z has the wrong sign", manual(0.1, 99.5, 1e-10)),  # w = 1, v = 1e-6: z = 1 + log(1e-6) < 0
    ("K is not a number", manual(1.0, math.nan, 1600.0)),
])
def test_each_validity_rule(name, r):
    assert R.pvalue(1000.0, r)[3] is False, name
    up, dn, p, ok = capi.spa_pvalue(1000.0, record(r))
    assert not ok and math.isnan(p), name
    if r["flags"] == 2:  # the other tail is still reported
        assert math.isnan(up) and dn == 0.0


def test_an_underflowing_tail_is_valid():
    r = manual(1.0, 200.0, 1600.0)  # w = v = 40: z = 40, far below the smallest double
    assert R.pvalue(1000.0, r) == (0.0, 0.0, 0.0, True)
    assert capi.spa_pvalue(1000.0, record(r)) == (0.0, 0.0, 0.0, True)
    assert capi.spa_pvalue(-1000.0, record(r)) == (0.0, 0.0, 0.0, True)  # the tails are at +|s| and -|s| whatever the sign of s


def test_refusals():
    L = capi.lib()
    p, ok = C.c_double(), C.c_int()
    rec = record(manual(1.0, 200.0, 1600.0))
    assert L.hgibbs_spa_pvalue(1.0, None, None, None, C.byref(p), C.byref(ok)) != 0
    assert "hgibbs_spa_pvalue: null argument" in L.hgibbs_last_error().decode()
    assert L.hgibbs_spa_pvalue(1.0, C.byref(rec), None, None, None, C.byref(ok)) != 0
    assert "hgibbs_spa_pvalue: null argument" in L.hgibbs_last_error().decode()
    assert L.hgibbs_spa_pvalue(1000.0, C.byref(rec), None, None, C.byref(p), None) == 0 and p.value == 0.0  # the optional ones may be null
