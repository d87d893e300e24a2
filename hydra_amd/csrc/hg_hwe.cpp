// hg_hwe.cpp -- the exact test of Hardy-Weinberg proportions of Wigginton, Cutler & Abecasis (Am J Hum Genet 76:887, 2005), for --qc
// (DESIGN.md section 23): plain C++, no HIP.
//
// Given n genotypes with r copies of the rarer allele, the number of heterozygotes k has the parity of r and
//
//     P(k) ~ 2^k n! / (n_rr! k! n_cc!),   n_rr = (r - k)/2,  n_cc = n - k - n_rr,
//
// so P(k + 2) / P(k) = 4 n_rr n_cc / ((k + 2)(k + 1)).  The weights are walked outward from a k near the mode, where the weight is set
// to 1 (nothing overflows; far tails may underflow to 0, which is what they are worth), once for their sum and the observed count's
// weight and once for the sum of those not above it.  No array: a marker of 2^32 genotypes costs 2^32 steps and no memory.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../include/hgibbs.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {

// f(k, w) for every feasible k with its weight w relative to the start's, downward from the start and then upward
template <class F>
void walk(uint64_t n, uint64_t rare, uint64_t start, F f)
{
    double w = 1.0;
    uint64_t k = start, rr = (rare - start) / 2, cc = n - start - rr;
    f(k, w);
    while (k >= 2) { // P(k - 2) = P(k) k (k - 1) / (4 (n_rr + 1)(n_cc + 1))
        w = w * (double)k * (double)(k - 1) / (4.0 * (double)(rr + 1) * (double)(cc + 1));
        k -= 2;
        ++rr;
        ++cc;
        f(k, w);
    }
    w = 1.0;
    k = start;
    rr = (rare - start) / 2;
    cc = n - start - rr;
    while (k + 2 <= rare) { // P(k + 2) = P(k) 4 n_rr n_cc / ((k + 2)(k + 1))
        w = w * 4.0 * (double)rr * (double)cc / ((double)(k + 2) * (double)(k + 1));
        k += 2;
        --rr;
        --cc;
        f(k, w);
    }
}

} // namespace

extern "C" int hgibbs_hwe_exact(uint32_t n_het, uint32_t n_hom_a, uint32_t n_hom_b, double* p)
{
    if (!p) {
        hgibbs_set_error_("hgibbs_hwe_exact: null argument");
        return 1;
    }
    const uint64_t n = (uint64_t)n_het + n_hom_a + n_hom_b;
    if (n == 0) {
        *p = std::numeric_limits<double>::quiet_NaN();
        return 0;
    }
    const uint64_t rare = 2 * (uint64_t)(n_hom_a < n_hom_b ? n_hom_a : n_hom_b) + n_het;
    // a start near the mode E(k) = r (2 n - r) / (2 n), of r's parity (any feasible start gives the same distribution)
    uint64_t start = (uint64_t)std::floor((double)rare * (double)(2 * n - rare) / (double)(2 * n));
    if (start > rare) start = rare;
    if ((start ^ rare) & 1u) start = start < rare ? start + 1 : start - 1;

    double sum = 0.0, wobs = 0.0;
    walk(n, rare, start, [&](uint64_t k, double w) {
        sum += w;
        if (k == n_het) wobs = w;
    });
    // the tie rule: every k whose weight is within 1e-9 relative of the observed one counts as "as extreme"
    const double thr = wobs * (1.0 + 1e-9);
    double tail = 0.0;
    walk(n, rare, start, [&](uint64_t, double w) {
        if (w <= thr) tail += w;
    });
    const double v = tail / sum;
    *p = v > 1.0 ? 1.0 : v;
    return 0;
}
