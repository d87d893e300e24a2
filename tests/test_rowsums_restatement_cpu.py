"""The restatement of hgibbs_row_sums in Python integers (tests/rowsums_restate.py) against a plain f64 sum within the bound the
contract states, and the restatement's own claims: 0/1 tables give exact counts, columns do not depend on each other, and the
int64-halves form used at the larger shapes is the big-integer form bit for bit.  No GPU needed."""
import numpy as np
import pytest

import rowsums_restate as rr


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def make_codes(N, M, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 3, size=(N, M))
    codes[rng.random((N, M)) < 0.05] = 3
    if M >= 3:
        codes[:, M // 3] = 3
        codes[:, M // 2] = 0
    if N >= 3:
        codes[N // 2] = 3
    return codes


def tables(codes, seed):
    """the seven QC tables, random normal tables at three scales, an all-zero table and one with entries only at code 3"""
    N, M = codes.shape
    rng = np.random.default_rng(seed)
    qc = rr.polymorphic(codes)
    extra = np.zeros((5, M, 4))
    extra[0] = rng.standard_normal((M, 4))
    extra[1] = rng.standard_normal((M, 4)) * 1e-7
    extra[2] = rng.standard_normal((M, 4)) * 3e11
    extra[4, :, 3] = rng.standard_normal(M)
    return np.concatenate([rr.qc_tables(codes, qc), extra])


@pytest.mark.parametrize("N,M", [(1, 1), (5, 17), (33, 64), (70, 301)])
def test_against_plain_f64(N, M):
    codes = make_codes(N, M, seed=N + 3 * M)
    tab = tables(codes, seed=M)
    got = rr.row_sums(codes, tab)
    cols = np.arange(M)
    for t in range(tab.shape[0]):
        mx = np.max(np.abs(tab[t]))
        for i in range(N):
            plain = float(np.sum(tab[t][cols, codes[i]]))
            err = abs(got[i, t] - plain)
            print("N=%d M=%d t=%d i=%d err=%.3g bound=%.3g" % (N, M, t, i, err, M * mx * 2.0 ** -52 * 2))
            assert err <= M * mx * 2.0 ** -52 * 2


def test_zero_one_tables_give_exact_counts():
    codes = make_codes(40, 131, seed=9)
    M = codes.shape[1]
    tab = np.zeros((4, M, 4))
    tab[0, :, 3] = 1.0              # missing calls
    tab[1, :, :3] = 1.0             # called
    tab[2, :, 1] = 1.0              # heterozygous
    tab[3, ::2, 0] = tab[3, ::2, 2] = 1.0  # homozygous at the even markers
    got = rr.row_sums(codes, tab)
    want = np.stack([(codes == 3).sum(1), (codes != 3).sum(1), (codes == 1).sum(1), ((codes[:, ::2] == 0) | (codes[:, ::2] == 2)).sum(1)], axis=1)
    assert np.array_equal(got, want.astype(np.float64))


def test_scale_and_all_zero_table():
    assert rr.scale(np.zeros((3, 4))) == 0
    assert rr.scale(np.array([[1.0]])) == 51        # 1 < 2^1
    assert rr.scale(np.array([[0.999]])) == 52      # 0.999 < 2^0
    assert rr.scale(np.array([[-4.0, 3.0]])) == 49  # 4 < 2^3
    codes = make_codes(6, 9, seed=1)
    assert np.array_equal(bits(rr.row_sums(codes, np.zeros((1, 9, 4)))), bits(np.zeros((6, 1))))


def test_columns_do_not_depend_on_each_other():
    codes = make_codes(21, 77, seed=4)
    tab = tables(codes, seed=5)
    full = rr.row_sums(codes, tab)
    for t in range(tab.shape[0]):
        assert np.array_equal(bits(rr.row_sums(codes, tab[t:t + 1])[:, 0]), bits(full[:, t]))


@pytest.mark.parametrize("N,M", [(1, 1), (7, 65), (64, 130)])
def test_split_form_is_the_big_integer_form(N, M):
    codes = make_codes(N, M, seed=N * M)
    tab = tables(codes, seed=2)
    assert np.array_equal(bits(rr.row_sums_split(codes, tab)), bits(rr.row_sums(codes, tab)))
