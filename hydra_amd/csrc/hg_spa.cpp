// hg_spa.cpp -- the saddlepoint p-value of the logistic score test of --assoc --assoc-logistic --assoc-spa:
// plain C++, no HIP, no handle.
//
//     int hgibbs_spa_pvalue(double s, const hgibbs_spa_root* r, double* p_upper, double* p_lower, double* p, int* valid);
//
//   s        the marker's score U; the tails are at tau = +|s| (index 0 of r) and tau = -|s| (index 1)
//   r        what hgibbs_spa_roots wrote for the marker: the saddlepoint t of each tail, K(t) and K''(t) there, and the flags
//   p_upper  P(U >= |s|), p_lower P(U <= -|s|) by the Barndorff-Nielsen form (either may be NULL); NaN for a tail that is not valid
//   p        their sum, the two-sided p; NaN unless both tails are valid: the caller then keeps the normal approximation
//   valid    1 when both tails are valid, else 0 (may be NULL)
//
// Per tail:  w = sign(t) sqrt(2 (t tau - K)),  v = t sqrt(K''),  z = w + log(v / w) / w,  tail = erfc(|z| / sqrt 2) / 2.
// A tail is valid when its converged flag is set, t tau - K > 0, K'' > 0, v / w > 0, and z is finite with tau's sign.  A tail that
// underflows to 0 is valid.  Refused: a null r or p.
#include <cmath>
#include <cstdint>
#include <limits>

#include "../../include/hgibbs.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {

// the tail at tau from (t, K, K2); false when a validity rule fails
bool spa_tail(double tau, bool converged, double t, double K, double K2, double& tail)
{
    tail = std::numeric_limits<double>::quiet_NaN();
    if (!converged) return false;
    const double h = t * tau - K;
    if (!(h > 0.0) || !(K2 > 0.0)) return false;
    const double w = (t < 0.0 ? -1.0 : 1.0) * std::sqrt(2.0 * h);
    const double v = t * std::sqrt(K2);
    const double ratio = v / w;
    if (!(ratio > 0.0)) return false;
    const double z = w + std::log(ratio) / w;
    if (!std::isfinite(z) || !(tau > 0.0 ? z > 0.0 : z < 0.0)) return false;
    tail = 0.5 * std::erfc(std::fabs(z) / std::sqrt(2.0));
    return true;
}

} // namespace

extern "C" int hgibbs_spa_pvalue(double s, const hgibbs_spa_root* r, double* p_upper, double* p_lower, double* p, int* valid)
{
    if (!r || !p) {
        hgibbs_set_error_("hgibbs_spa_pvalue: null argument");
        return 1;
    }
    const double sabs = std::fabs(s);
    double up = 0.0, dn = 0.0;
    const bool oku = spa_tail(sabs, (r->flags & 1u) != 0u, r->t[0], r->K[0], r->K2[0], up);
    const bool okd = spa_tail(-sabs, (r->flags & 2u) != 0u, r->t[1], r->K[1], r->K2[1], dn);
    if (p_upper) *p_upper = up;
    if (p_lower) *p_lower = dn;
    *p = oku && okd ? up + dn : std::numeric_limits<double>::quiet_NaN();
    if (valid) *valid = oku && okd ? 1 : 0;
    return 0;
}
