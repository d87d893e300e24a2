"""The restatement of the epistasis path (tests/epi_restate.py) against hand-made tables and its own identities, the precision constants
it pins, the condition the GPU cases rest on, and hgibbs_epi_test (host only) against it.  No GPU needed."""
import functools
import math

import numpy as np
import pytest

from hydra_amd import capi

import epi_restate as E


@functools.lru_cache(maxsize=None)
def grid():
    t = E.grid_tables()
    r = E.epi_test(t)
    t.setflags(write=False)
    return t, r


def test_table_typed_out_by_hand():
    # marker a: 0 1 2 0 1 3 (3 = missing), marker b: 0 0 2 1 1 2, classes 0 0 0 1 1 1
    geno = np.array([[0, 1, 2, 0, 1, 3], [0, 0, 2, 1, 1, 2]], dtype=np.uint8)
    cls = np.array([0, 0, 0, 1, 1, 1])
    want = np.zeros((2, 3, 3), dtype=np.int64)
    want[0, 0, 0] = 1  # row 0
    want[0, 1, 0] = 1  # row 1
    want[0, 2, 2] = 1  # row 2
    want[1, 0, 1] = 1  # row 3
    want[1, 1, 1] = 1  # row 4; row 5 has a missing call at a: in no cell
    assert np.array_equal(E.tables(geno, [0], [1], cls)[0, 0], want)
    assert np.array_equal(E.tables(geno, [1], [0], cls)[0, 0], want.transpose(0, 2, 1))
    # the same marker on both sides: diagonal, and the missing row is gone
    d = E.tables(geno, [0], [0], cls)[0, 0]
    assert np.array_equal(d, np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0, 0], [0, 1, 0], [0, 0, 0]]]))
    # no classes: everything in class 0
    assert np.array_equal(E.tables(geno, [0], [1])[0, 0], want.sum(axis=0, keepdims=True).repeat(2, 0) * np.array([1, 0])[:, None, None])


def test_ksa_and_lr_of_a_table_typed_out_by_hand():
    """a 2 x 2 x 2 corner of the table with a known fit: the homogeneous-association fit of a table without three-way interaction is the
    table itself"""
    t = np.zeros((2, 3, 3), dtype=np.int64)
    # odds ratio 4 between the markers in both classes: no interaction
    t[0, :2, :2] = [[40, 10], [10, 10]]
    t[1, :2, :2] = [[20, 10], [5, 10]]
    r = E.epi_test(t[None])
    assert r["df"][0] == 1 and r["converged"][0] == 1
    assert r["lr"][0] <= 1e-9
    m, _, _ = E.ipf(t[None])
    assert np.allclose(m[0], t, atol=1e-6)
    # KSA by hand for the same table
    n = t.sum()
    nij, nik, njk = t.sum(0), t.sum(2), t.sum(1)
    ni, nj, nk = nij.sum(1), nij.sum(0), nik.sum(1)
    q = np.zeros((2, 3, 3))
    for k in range(2):
        for i in range(2):
            for j in range(2):
                q[k, i, j] = nij[i, j] * nik[k, i] * njk[k, j] / (ni[i] * nj[j] * nk[k])
    pk = q / q.sum()
    want = 2 * sum(t[c] * (math.log(t[c] / n) - math.log(pk[c])) for c in np.ndindex(2, 3, 3) if t[c] > 0)
    assert abs(r["ksa"][0] - want) <= 1e-12 * abs(want) + 1e-12
    assert r["ksa"][0] >= r["lr"][0]


def test_margins_of_every_table_against_the_markers_class_counts():
    geno, cls = E.planted_case()
    idx = np.arange(geno.shape[0])
    t = E.tables(geno, idx, idx, cls)
    for k in range(2):
        rows = cls == k
        for a in (0, 5, 17, 33, 39):
            for b in (1, 5, 33):
                both = rows & (geno[a] != 3) & (geno[b] != 3)
                assert [int(x) for x in t[a, b, k].sum(axis=1)] == [int(((geno[a] == i) & both).sum()) for i in range(3)]
                assert [int(x) for x in t[a, b, k].sum(axis=0)] == [int(((geno[b] == j) & both).sum()) for j in range(3)]
    assert np.array_equal(t, t.transpose(1, 0, 2, 4, 3))


def test_ksa_bounds_lr():
    t, r = grid()
    assert t.shape[0] > 3000
    gap = r["ksa"] - r["lr"]
    print("min KSA - LR over %d tables: %.3g (%d fits hit the cap)" % (t.shape[0], gap.min(), int((r["converged"] == 0).sum())))
    assert np.all(gap >= -1e-9)


def test_one_category_gives_lr_zero_and_the_df_as_stated():
    t, r = grid()
    nij = t.sum(axis=1)
    I, J = (nij.sum(axis=2) > 0).sum(axis=1), (nij.sum(axis=1) > 0).sum(axis=1)
    assert set(np.unique(r["df"])) == {0, 1, 2, 4}
    assert np.array_equal(r["df"], np.where((I > 0) & (J > 0), (I - 1) * (J - 1), 0))
    one = (I <= 1) | (J <= 1)
    assert one.sum() > 3
    assert np.all(r["lr"][one] == 0.0) and np.all(r["iters"][one] == 0) and np.all(r["converged"][one] == 1) and np.all(np.isnan(r["p"][one]))
    assert np.all(np.isfinite(r["p"][~one]))


def chi2_tail_series(x, d):
    """the upper tail of chi-square with even d by its finite series exp(-x / 2) sum_{k < d / 2} (x / 2)^k / k!"""
    return math.exp(-x / 2) * sum((x / 2) ** k / math.factorial(k) for k in range(d // 2))


def test_tails():
    for x in (0.0, 1e-3, 0.5, 3.84, 12.0, 30.0, 187.0, 900.0):
        assert E.tail(x, 1) == math.erfc(math.sqrt(x / 2))
        for d in (2, 4):
            assert abs(E.tail(x, d) - chi2_tail_series(x, d)) <= 4e-16 * chi2_tail_series(x, d)
    assert abs(E.tail(3.841458820694124, 1) - 0.05) < 1e-12
    assert abs(E.tail(5.991464547107979, 2) - 0.05) < 1e-12
    assert abs(E.tail(9.487729036781154, 4) - 0.05) < 1e-12
    assert math.isnan(E.tail(1.0, 0))


def test_precision_constants():
    """float64 against longdouble on the grid, relative to the sum of the absolute terms; delta covers ten times the pinned constant"""
    t, r = grid()
    kl, al = E.ksa(t, np.longdouble)
    ok = r["ksa_scale"] > 0
    dk = float(np.max(np.abs(r["ksa"][ok] - kl[ok]) / al[ok]))
    m, _, _ = E.ipf(t)
    ll, la = E.lr_of(t, m, np.longdouble)
    ok = r["lr_scale"] > 0
    dl = float(np.max(np.abs(r["lr"][ok] - ll[ok]) / la[ok]))
    print("largest float64 - longdouble difference relative to the terms: KSA %.3g, LR %.3g" % (dk, dl))
    assert 10 * dk <= E.KSA_F64_LD and 10 * dl <= E.LR_F64_LD
    n = t.sum(axis=(1, 2, 3))
    for i in range(t.shape[0]):
        assert E.delta(n[i]) >= 10 * E.KSA_F64_LD * r["ksa_scale"][i]
    # the scale never exceeds the bound delta is derived from
    assert np.all(r["ksa_scale"] <= 2.0 * np.maximum(n, 2) * (4.0 * np.log(np.maximum(n, 2)) + math.log(18.0)))
    assert 2.0 ** -44 >= 10 * E.KSA_F64_LD


@pytest.mark.parametrize("case,thresholds", [("planted", E.T_PLANTED), ("second", (E.T_SECOND,))])
def test_no_pair_of_the_gpu_cases_lies_within_two_delta_of_its_threshold(case, thresholds):
    geno, cls = E.planted_case() if case == "planted" else E.second_case()
    ab, t = E.triangle(geno, cls)
    r = E.epi_test(t)
    for T in thresholds:
        d = float(np.min(np.abs(r["ksa"] - T)))
        print("%s, T = %g: %d pairs with KSA >= T, %d with LR >= T; the nearest KSA is %.3g away, 2 delta = %.3g"
              % (case, T, int((r["ksa"] >= T).sum()), int(((r["lr"] >= T) & (r["df"] > 0)).sum()), d, 2 * E.delta(geno.shape[1])))
        assert d > 2 * E.delta(geno.shape[1])
        assert np.all(r["ksa"][(r["lr"] >= T) & (r["df"] > 0)] >= T)  # the screen loses no pair
    if case == "planted":
        top = int(np.argmax(r["lr"]))
        assert tuple(ab[top]) == E.PLANTED and r["lr"][top] > 100.0
        assert int((r["ksa"] >= 30.0).sum()) == 1


def test_epi_test_of_the_library_against_the_restatement():
    t, r = grid()
    worst_k = worst_l = 0.0
    for i in range(t.shape[0]):
        c = capi.epi_test(t[i])
        assert (c.df, c.iters, c.converged) == (r["df"][i], r["iters"][i], r["converged"][i]), i
        if r["ksa_scale"][i] > 0:
            worst_k = max(worst_k, abs(c.ksa - r["ksa"][i]) / r["ksa_scale"][i])
        else:
            assert c.ksa == 0.0
        if r["lr_scale"][i] > 0:
            worst_l = max(worst_l, abs(c.lr - r["lr"][i]) / r["lr_scale"][i])
        dx = 10 * E.LR_F64_LD * r["lr_scale"][i]
        if r["df"][i] == 0:
            assert c.lr == 0.0 and math.isnan(c.p)
        else:
            assert abs(c.p - r["p"][i]) <= E.tail_tol(float(r["lr"][i]), int(r["df"][i]), dx), i
    print("hgibbs_epi_test against the restatement, relative to the terms: KSA %.3g, LR %.3g" % (worst_k, worst_l))
    assert worst_k <= 10 * E.KSA_F64_LD and worst_l <= 10 * E.LR_F64_LD


def test_epi_test_refusals():
    with pytest.raises(capi.HgError, match="table\\[4\\] = -1 is negative"):
        capi.epi_test([0, 0, 0, 0, -1] + [0] * 13)
    with pytest.raises(ValueError):
        capi.epi_test([1, 2, 3])
    assert capi.lib().hgibbs_epi_test(None, None) != 0
