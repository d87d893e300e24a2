"""tests/cs_restate.py on two cases typed out by hand, and, for every (W, NREC, seed) tests/test_gpu_cs.py uses, the conditions those
tests rely on, evaluated on the restatement alone with masks from NumPy's r.  No GPU needed.  If a seed fails a condition, the seed
is changed in tests/cs_cases.py, not the condition."""
import numpy as np
import pytest

import cs_cases as cc
import cs_restate as cr
import ldwalk


def masks(M, W, pairs):
    """masks in which exactly the given pairs (j, q), j < q <= j + W, pass"""
    band = np.zeros((M, W), dtype=bool)
    for j, q in pairs:
        band[j, q - j - 1] = True
    return ldwalk.pack(band), ldwalk.pack(ldwalk.backward_of(band))


def history(columns, nrec):
    """columns: {marker: records in which it is in the model}; one chain"""
    M = 6
    h = cr.History(1, nrec, M)
    for q in range(nrec):
        h.add(np.array([[q in columns.get(j, ()) for j in range(M)]]))
    return h


def test_by_hand_two_friends_and_a_tie():
    # lead 2 (records 0-3) with friends 0, 3, 4 and 5: marker 0 and marker 4 both have 3 records, the index decides for 0; then marker 4
    # brings the sum to 10 = need.  Marker 3 has no record and is passed over, marker 1 is no friend though it has the most records.
    h = history({2: [0, 1, 2, 3], 0: [4, 5, 6], 4: [3, 4, 7], 5: [8], 1: range(10)}, 10)
    fwd, bwd = masks(6, 3, [(0, 2), (2, 3), (2, 4), (2, 5)])
    cnt = h.counts()
    assert cnt.tolist() == [3, 10, 4, 0, 3, 1] and h.words.shape == (1, 6) and int(h.words[0, 4]) == 0b10011000
    assert sorted(cr.friends(2, 6, 3, fwd, bwd)) == [0, 3, 4, 5]
    notes = {}
    got = cr.candidate(2, cnt, h.words, 6, 3, fwd, bwd, 10, 4, notes)
    assert got == (0, 3, 10, 8, [2, 0, 4, cr.NONE])  # records 0-7: record 3 and 4 are counted twice in the sum, once in the PEP
    assert notes == {"tie": True, "zero": True}
    # with room for two members only it stops at the cap, with the sum it reached
    assert cr.candidate(2, cnt, h.words, 6, 3, fwd, bwd, 10, 2) == (2, 0, 7, 0, [cr.NONE, cr.NONE])
    # the window's width cuts marker 5 off, and 0 (distance 2) stays
    assert sorted(cr.friends(2, 6, 2, *masks(6, 2, [(0, 2), (2, 3), (2, 4)]))) == [0, 3, 4]


def test_by_hand_a_lead_that_runs_short():
    h = history({2: [0, 1, 2, 3], 0: [4, 5, 6], 4: [3, 4, 7], 5: [8]}, 10)
    fwd, bwd = masks(6, 3, [(0, 2), (2, 3), (2, 4), (2, 5)])
    cnt = h.counts()
    assert cr.candidate(2, cnt, h.words, 6, 3, fwd, bwd, 12, 6) == (1, 0, 11, 0, [cr.NONE] * 6)
    # marker 5's one friend is marker 2
    assert cr.candidate(5, cnt, h.words, 6, 3, fwd, bwd, 5, 6) == (0, 2, 5, 5, [5, 2] + [cr.NONE] * 4)
    # marker 1 has no record and no friend: the cap is asked first, then the friends
    assert cr.candidate(1, cnt, h.words, 6, 3, fwd, bwd, 1, 1) == (2, 0, 0, 0, [cr.NONE])
    assert cr.candidate(1, cnt, h.words, 6, 3, fwd, bwd, 1, 2) == (1, 0, 0, 0, [cr.NONE, cr.NONE])
    # the walk: lead 2 first (4 records), then 0 and 4 (3 each, by index), then 5; 0 and 4 overlap with 2's set, 5 is below the PEP bound
    leads = np.array([5, 4, 2, 0], dtype=np.uint32)
    st, sz, tot, pep, mem = cr.candidates(leads, cnt, h.words, 6, 3, fwd, bwd, 5, 3)
    assert st.tolist() == [0, 0, 0, 0] and sz.tolist() == [2, 2, 2, 2] and mem[:, :2].tolist() == [[5, 2], [4, 2], [2, 0], [0, 2]]
    assert pep.tolist() == [5, 6, 7, 7] and tot.tolist() == [5, 7, 7, 7]
    assert cr.walk(leads, cnt[leads], st, sz, pep, mem, 6) == [2]
    assert cr.walk(leads, cnt[leads], st, sz, pep, mem, 8) == []
    text = cr.table_text(["s%d" % j for j in range(6)], [1] * 6, [10 * j for j in range(6)], 10, cnt, leads, sz, tot, pep, mem, [2])
    assert text == ("CS\tLEAD\tCHR\tBP_FIRST\tBP_LAST\tSIZE\tNREC\tPIP_LEAD\tPIP_SUM\tPEP\tSNPS\tPIPS\n"
                    "1\ts2\t1\t0\t20\t2\t10\t0.4\t0.7\t0.7\ts2,s0\t0.4,0.3\n")


def test_ceilings():
    assert cr.ceil_count(0.9, 4) == 4 and cr.ceil_count(0.7, 130) == 91 and cr.ceil_count(0.01, 4) == 1 and cr.ceil_count(0.5, 64) == 32 and cr.ceil_count(1.0, 65) == 65


@pytest.fixture(scope="module")
def data():
    geno, runs = cc.ld_genotypes()
    return geno, runs, {W: cc.numpy_masks(geno, W) for W in cc.WINDOWS}


def test_the_genotypes_straddle_the_threshold(data):
    geno, runs, m = data
    fwd, _ = m[130]
    inside = [(j0, j0 + k) for j0, n in runs for k in range(1, n)]
    passing = sum(1 for j, q in inside if (int(fwd[j, 0]) >> (q - j - 1)) & 1)
    assert 0 < passing < len(inside) and np.count_nonzero(geno == 3) > 0


@pytest.mark.parametrize("nrec", sorted(cc.SHAPES))
@pytest.mark.parametrize("W", cc.WINDOWS)
def test_conditions_of_the_gpu_cases(data, W, nrec):
    geno, runs, m = data
    fwd, bwd = m[W]
    C, T = cc.SHAPES[nrec]
    h = cc.history_of(cc.crafted_flags(runs, cc.M, nrec, cc.SEEDS[(W, nrec)]), C, T)
    cnt = h.counts()
    leads = cc.leads_of(cnt)
    assert leads[0] == 0 and leads[-1] == cc.M - 1
    notes = {}
    results = {k: cr.candidates(leads, cnt, h.words, cc.M, W, fwd, bwd, cr.ceil_count(cc.ALPHA, nrec), k, notes) for k in cc.MAX_SIZES}
    assert cc.conditions(results, leads, cnt, nrec, notes) == []
