"""hgibbs_hwe_exact (capi.hwe_exact) against the exact test of Wigginton, Cutler & Abecasis (2005) restated in exact rationals, with the
same tie rule: every genotype triple up to 40 genotypes, and a few larger ones.  No GPU needed."""
import ctypes as C
import math
from fractions import Fraction

import pytest

from hydra_amd import capi

RTOL = 1e-9  # the recursion's rounding over n steps is of order n 2^-52: below 1e-10 at these sizes
TIE = Fraction(1) + Fraction(1, 10 ** 9)


def restate(n_het, n_hom_a, n_hom_b):
    """P(het = k) ~ 2^k n! / (n_rr! k! n_cc!) = 2^k C(n, k) C(n - k, n_rr) over the k of the rare allele count's parity, as exact
    integers: the first from math.comb, the next by w(k + 2) = w(k) 4 n_rr n_cc / ((k + 2)(k + 1)), which divides exactly.  The P
    value is the sum of the weights not above the observed one's times 1 + 1e-9, over the sum of all."""
    n = n_het + n_hom_a + n_hom_b
    rare = 2 * min(n_hom_a, n_hom_b) + n_het
    k = rare % 2
    rr = (rare - k) // 2
    cc = n - k - rr
    w = {k: (1 << k) * math.comb(n, k) * math.comb(n - k, rr)}
    while k + 2 <= rare:
        num = w[k] * 4 * rr * cc
        assert num % ((k + 2) * (k + 1)) == 0
        w[k + 2] = num // ((k + 2) * (k + 1))
        k, rr, cc = k + 2, rr - 1, cc - 1
    total = sum(w.values())
    thr = w[n_het] * TIE
    return Fraction(sum(v for v in w.values() if v <= thr), total)


def close(got, want):
    want = float(want)
    return abs(got - want) <= RTOL * want


def test_every_triple_up_to_forty():
    worst = 0.0
    for n in range(1, 41):
        for het in range(n + 1):
            for a in range(n - het + 1):
                b = n - het - a
                got, want = capi.hwe_exact(het, a, b), restate(het, a, b)
                worst = max(worst, abs(got - float(want)) / float(want))
                assert close(got, want), (het, a, b, got, float(want))
    print("largest relative difference %.3g" % worst)


@pytest.mark.parametrize("t", [(0, 0, 200000),          # monomorphic: p = 1
                               (0, 200000, 0),
                               (3960, 20, 196020),       # close to the proportions, and its mirror image
                               (3960, 196020, 20),
                               (3930, 35, 196035),       # too few heterozygotes
                               (3990, 5, 196005),        # too many
                               (3998, 1, 196001), (4000, 0, 196000), (21, 3, 99976), (1940, 30, 48030), (600, 700, 800),
                               (18960, 520, 180520)])    # 2 10^5 genotypes, 10 001 feasible counts
def test_larger_triples(t):
    got, want = capi.hwe_exact(*t), restate(*t)
    print(t, got, float(want))
    if want == 0 or float(want) < 1e-300:
        assert got < 1e-300
    else:
        assert close(got, want)
    if t[0] == 0 and 0 in t[1:]:
        assert got == 1.0


def test_mirror_images_agree():
    assert capi.hwe_exact(3930, 35, 196035) == capi.hwe_exact(3930, 196035, 35)
    assert capi.hwe_exact(7, 2, 11) == capi.hwe_exact(7, 11, 2)
    assert close(capi.hwe_exact(2, 1, 1), restate(2, 1, 1))


def test_empty_and_null():
    assert math.isnan(capi.hwe_exact(0, 0, 0))
    L = capi.lib()
    assert L.hgibbs_hwe_exact(1, 1, 1, None) != 0
    assert b"null" in L.hgibbs_last_error()
