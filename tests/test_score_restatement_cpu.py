"""The integer restatement of hgibbs_score that tests/test_gpu_score.py compares the device with bit for bit, checked on its own: it is
the operator (within the design bound of the plain f64 sum), and the comparison has the power it is there for (a kernel that loses the
lowest base-256 digit of every weight changes nearly every entry's bits)."""
import numpy as np
import pytest

from hydra_amd import synth
from test_gpu_score import (digit_samples, drop_lowest_digit, quantise_weights, reference, restate, restate_from_q, same_bits, signed_digits,
                            weights)


def cohort(N, M, missing, seed):
    """test_gpu_score.load's data without the device"""
    geno = synth.make_genotypes(M, N, seed=seed, missing_rate=missing)
    if missing:
        geno[M // 2, :] = 3
    return geno


@pytest.mark.parametrize("N,M", [(63, 200), (257, 65), (513, 129)])
@pytest.mark.parametrize("missing", [0.0, 0.02])
def test_restatement_is_the_operator_and_sees_a_lost_digit(N, M, missing):
    geno = cohort(N, M, missing, seed=N + 7)
    for S in (1, 7, 17):
        a, o = weights(S, M, seed=S)
        E, qa, qo = quantise_weights(a, o)
        out = restate_from_q(geno, E, qa, qo)
        assert same_bits(out, restate(geno, a, o))
        # (a) within hg_score.hip.h's bound of the plain f64 sum, whose own error M 2^-53 mag is far below it at these sizes
        ref, mag = reference(geno, a, o)
        wmax = np.maximum(np.abs(a).max(axis=1), np.abs(o).max(axis=1))
        design = 3.0 * M * wmax[None, :] * 2.0 ** -52
        live = wmax > 0
        ratio = float(np.max(np.abs(out - ref)[:, live] / design[:, live]))
        print("N=%d M=%d S=%d missing=%g: |restatement - f64| / (3 M max|w| 2^-52) = %.3g" % (N, M, S, missing, ratio))
        assert np.all(np.abs(out - ref) <= design)
        assert np.all(out[:, ~live] == 0.0)
        # (b) without the lowest signed digit of every quantised weight: at least 90 % of the entries of every non-zero sample change
        less = restate_from_q(geno, E, drop_lowest_digit(qa), drop_lowest_digit(qo))
        changed = (out.view(np.int64) != less.view(np.int64)).mean(axis=0)
        print("  share of entries whose bits change without digit 0: min %.4f" % float(changed[live].min()))
        assert np.all(changed[live] >= 0.9), changed


def test_quantisation_and_digits():
    """the scale puts the largest weight in [2^51, 2^52]; a dropped digit is a multiple of 256 within 128 of q; float() of a Python
    integer rounds ties to even, as the device's one rounding does"""
    a, o = weights(7, 200, seed=7)
    E, qa, qo = quantise_weights(a, o)
    top = np.maximum(np.abs(qa).max(axis=1), np.abs(qo).max(axis=1))
    assert E[1] == 0 and top[1] == 0
    live = np.arange(7) != 1
    assert np.all(top[live] >= 1 << 51) and np.all(top[live] <= 1 << 52)
    for q in (qa, qo):
        d = drop_lowest_digit(q)
        assert np.all(d % 256 == 0) and np.all(q - d >= -128) and np.all(q - d <= 127)
    assert float((1 << 53) + 1) == 2.0 ** 53 and float((1 << 53) + 3) == 2.0 ** 53 + 4.0
    assert float(-((1 << 53) + 1)) == -(2.0 ** 53) and float((1 << 54) + 2) == 2.0 ** 54


@pytest.mark.parametrize("seed", [2, 5, 63, 257, 4097])
def test_digit_samples_live_in_one_digit_each(seed):
    """the premise of the per-digit tests of hgibbs_score and hgibbs_region_var: every sample is scaled with E = 40, over all markers
    and over any set that holds the anchor, and each quantised weight off the anchor has digit d and no other.  The operand of the
    missing-call product, -(3 q_a + q_o) = -(3 kappa + lambda) 256^d with |3 kappa + lambda| <= 508, carries into digit d + 1 for d < 6
    and stays in digit 6 for d = 6 (<= 60).  The anchor's 2^51 is digit 6 and meets code 0 only."""
    M, anchor = 200, 100
    a, o, kappa, lam = digit_samples(M, anchor, seed=seed)
    for idx in (np.arange(M), np.array([anchor]), np.array([anchor, 150]), np.arange(38, 101), np.arange(64, 129)):
        E, qa, qo = quantise_weights(a[:, idx], o[:, idx])
        assert np.all(E == 40), E
        assert np.array_equal(qa, np.rint(np.ldexp(a[:, idx], 40)).astype(np.int64))
    E, qa, qo = quantise_weights(a, o)
    shift = (1 << (8 * np.arange(7)))[:, None]
    off = np.arange(M) != anchor
    assert np.array_equal(qa[:, off], (kappa * shift)[:, off]) and np.array_equal(qo, lam * shift)
    assert qa[0, anchor] == 1 << 51 and np.abs(qa).max() < 1 << 52 and np.abs(qo).max() < 1 << 52
    for q, spill in ((qa[:, off], 0), (qo[:, off], 0), (-(3 * qa + qo)[:, off], 1)):
        dig = signed_digits(q)  # (7, M - 1, 7)
        assert np.array_equal((dig * (1 << (8 * np.arange(7)))).sum(axis=-1), q)
        for d in range(7):
            others = (np.arange(7) < d) | (np.arange(7) > d + spill)
            assert not dig[d][:, others].any(), d
            assert dig[d][:, d].any(), d
    assert np.array_equal(np.flatnonzero(signed_digits(qa[:, anchor])[0]), [6])
