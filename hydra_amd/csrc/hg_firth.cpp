// hg_firth.cpp -- the statistics of Firth's penalised fit of --assoc --assoc-logistic --assoc-firth: plain C++,
// no HIP, no handle.
//
//     int hgibbs_firth_stats(double s, const hgibbs_firth_rec* r, double* lrt, double* se, double* p, int* valid);
//
//   s      the marker's score U
//   r      what hgibbs_firth_fit wrote for the marker: beta, K(beta) and K''(beta), K''(0) and the flags
//   lrt    the penalised likelihood ratio statistic 2 (beta s - K + log(K2 / k2_0) / 2); a value in [-1e-9, 0) is rounding and becomes 0
//   se     1 / sqrt(K2), the standard error of beta from the information at beta
//   p      erfc(sqrt(lrt / 2)), the chi-square tail with one degree of freedom
//   valid  1 when the fit converged, is not degenerate, K2 > 0 and lrt is finite and >= 0 after the clamp; else 0, and lrt, se and p are
//          NaN: the caller keeps the score test
//
// lrt, se and valid may be NULL.  Refused: a null r or p.
#include <cmath>
#include <cstdint>
#include <limits>

#include "../../include/hgibbs.h"

extern "C" void hgibbs_set_error_(const char* msg);

extern "C" int hgibbs_firth_stats(double s, const hgibbs_firth_rec* r, double* lrt, double* se, double* p, int* valid)
{
    if (!r || !p) {
        hgibbs_set_error_("hgibbs_firth_stats: null argument");
        return 1;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double l = nan, e = nan, pv = nan;
    bool ok = (r->flags & 1u) != 0u && (r->flags & 2u) == 0u && r->K2 > 0.0;
    if (ok) {
        l = 2.0 * ((r->beta * s - r->K) + 0.5 * std::log(r->K2 / r->k2_0));
        if (l >= -1e-9 && l < 0.0) l = 0.0;
        ok = std::isfinite(l) && l >= 0.0;
    }
    if (ok) {
        e = 1.0 / std::sqrt(r->K2);
        pv = std::erfc(std::sqrt(l / 2.0));
    } else {
        l = nan;
    }
    if (lrt) *lrt = l;
    if (se) *se = e;
    *p = pv;
    if (valid) *valid = ok ? 1 : 0;
    return 0;
}
