// hg_settest.cpp -- burden and SKAT statistics of one marker set from its scores and their covariance, for --assoc-sets (DESIGN.md
// section 28): plain C++, no HIP, no handle.
//
//     int hgibbs_set_tests(uint32_t m, const double* U, const double* Phi, const double* a, hgibbs_set_result* r);
//
//   U        the m scores; Phi their m x m covariance under the null model (symmetric; the upper triangle is read); a the m weights
//   burden   T = (sum a_j U_j)^2 / (a'Phi a), P = erfc(sqrt(T / 2)); both NaN when a'Phi a <= 1e-9 sum a_j^2 Phi_jj (--assoc's guard)
//   SKAT     Q = sum a_j^2 U_j^2 against sum_k lam_k chi^2_1 with lam the eigenvalues of diag(a) Phi diag(a) above 1e-10 lam_max, by
//            cyclic Jacobi (written here: hgibbs_pca's solver is pinned where it lies), sorted descending; neig their number.  With
//            neig = 0 the SKAT fields are NaN and skat_ok = 0.
//   P_SKAT   the saddlepoint tail in the Barndorff-Nielsen form of hg_spa.cpp.  K(z) = -1/2 sum log(1 - 2 z lam_k); the root of
//            K'(z) = Q on (-inf, 1 / (2 lam_max)) by hgibbs_spa_roots' rule: start at z = (Q - sum lam) / K''(0) with the open bracket
//            (0, 1 / (2 lam_max)) resp. (-inf, 0), moved inside it by the safeguard when it is not; the sign of K' - Q tightens the
//            bracket; the proposal is z' = z - (K' - Q) / K''; first the stop rule |z' - z| <= 1e-9 max(|z|, 1 / sqrt(K''(0))) (z' is
//            taken, K and K'' are evaluated there), only then the safeguard (a z' not strictly inside the bracket becomes its
//            midpoint when both ends are finite, else 2 z).  At most 64 steps.  Every sum runs over the eigenvalues in their sorted
//            order: bit-reproducible.  Then w = sign(z) sqrt(2 (z Q - K)), v = z sqrt(K''), p = erfc((w + log(v / w) / w) / sqrt 2) / 2,
//            valid when the root converged, z Q - K > 0, K'' > 0, v / w > 0 and the argument is finite: spa_tail's rules without its
//            sign rule, which belongs to a symmetric pair of tails taken at |z|.  This tail keeps the argument's sign, and between
//            the median and the mean of the skewed sum the argument is rightly positive (p < 1/2) while z is negative.
//   limit    |Q - sum lam| < 1e-6 sqrt(2 sum lam^2): p = erfc(rho / (6 sqrt 2)) / 2 with rho = K'''(0) / K''(0)^(3/2), K''(0) = 2 sum lam^2,
//            K'''(0) = 8 sum lam^3: the limit of the form above as z -> 0, where log(v / w) / w -> rho / 6.  Its first-order expansion
//            1/2 - rho / (6 sqrt(2 pi)) is the limit of the Lugannani-Rice form and is off by up to 0.007 for a single eigenvalue, so the
//            erfc is kept whole and the two pieces meet.  Near the mean the formula's rounding error is about 2^-52 / w and the
//            limit's truncation error is O(w); at 1e-6 both are below 1e-6 absolute.
//   skat_ok  1 when the tail is valid (or the limit was taken); otherwise 0 and p_skat is the normal tail of
//            (Q - sum lam) / sqrt(2 sum lam^2), as --assoc-spa falls back.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/hgibbs.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN();

// Eigenvalues of the symmetric n x n matrix A (row-major, destroyed) by cyclic Jacobi: sweeps over (p, q), p < q, in row order until
// every off-diagonal entry is zero; at most 100 sweeps.  The rotation of Rutishauser (the smaller root t of t^2 + 2 t theta - 1 = 0).
void st_jacobi(std::vector<double>& A, uint32_t n, std::vector<double>& ev)
{
    for (int sweep = 0; sweep < 100; ++sweep) {
        double offn = 0.0;
        for (uint32_t p = 0; p < n; ++p)
            for (uint32_t q = p + 1; q < n; ++q) offn += std::fabs(A[(size_t)p * n + q]);
        if (offn == 0.0) break;
        for (uint32_t p = 0; p < n; ++p) {
            for (uint32_t q = p + 1; q < n; ++q) {
                const double apq = A[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
                const double g = 100.0 * std::fabs(apq);
                if (sweep > 3 && std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
                    A[(size_t)p * n + q] = A[(size_t)q * n + p] = 0.0;
                    continue;
                }
                const double hd = aqq - app;
                double t;
                if (std::fabs(hd) + g == std::fabs(hd)) t = apq / hd;
                else {
                    const double theta = 0.5 * hd / apq;
                    t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                }
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                A[(size_t)p * n + p] = app - t * apq;
                A[(size_t)q * n + q] = aqq + t * apq;
                A[(size_t)p * n + q] = A[(size_t)q * n + p] = 0.0;
                for (uint32_t k = 0; k < n; ++k) {
                    if (k == p || k == q) continue;
                    const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
                    const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
                    A[(size_t)k * n + p] = A[(size_t)p * n + k] = np_;
                    A[(size_t)k * n + q] = A[(size_t)q * n + k] = nq_;
                }
            }
        }
    }
    ev.resize(n);
    for (uint32_t i = 0; i < n; ++i) ev[i] = A[(size_t)i * n + i];
}

struct Cgf {
    double K, K1, K2;
};

Cgf st_cgf(const std::vector<double>& lam, double z)
{
    Cgf c{0.0, 0.0, 0.0};
    for (double l : lam) {
        const double d = 1.0 - 2.0 * z * l;
        c.K += -0.5 * std::log1p(-2.0 * z * l);
        c.K1 += l / d;
        c.K2 += 2.0 * (l / d) * (l / d);
    }
    return c;
}

// the saddlepoint tail P(sum lam chi^2_1 >= Q); false when a validity rule fails
bool st_tail(const std::vector<double>& lam, double Q, double mean, double k2_0, double& p)
{
    p = NaN;
    const double scale = 1.0 / std::sqrt(k2_0), pole = 1.0 / (2.0 * lam[0]);
    double lo, hi;
    if (Q > mean) {
        lo = 0.0;
        hi = pole;
    } else {
        lo = -std::numeric_limits<double>::infinity();
        hi = 0.0;
    }
    auto inside = [&](double t) { return t > lo && t < hi; };
    double z = (Q - mean) / k2_0;
    if (!inside(z)) z = std::isfinite(lo) && std::isfinite(hi) ? 0.5 * (lo + hi) : 2.0 * z;
    bool converged = false;
    Cgf c{};
    for (int it = 0; it < 64; ++it) {
        c = st_cgf(lam, z);
        const double f = c.K1 - Q;
        if (f > 0.0) hi = z;
        else if (f < 0.0) lo = z;
        double zn = z - f / c.K2;
        if (std::fabs(zn - z) <= 1e-9 * std::max(std::fabs(z), scale)) {
            // (a step this small from inside the bracket stays below the pole; a z' that does not is no root)
            if (!(zn < pole)) return false;
            z = zn;
            c = st_cgf(lam, z);
            converged = true;
            break;
        }
        if (!inside(zn)) zn = std::isfinite(lo) && std::isfinite(hi) ? 0.5 * (lo + hi) : 2.0 * z;
        z = zn;
    }
    if (!converged) return false;
    const double h = z * Q - c.K;
    if (!(h > 0.0) || !(c.K2 > 0.0)) return false;
    const double w = (z < 0.0 ? -1.0 : 1.0) * std::sqrt(2.0 * h);
    const double v = z * std::sqrt(c.K2);
    const double ratio = v / w;
    if (!(ratio > 0.0)) return false;
    const double x = w + std::log(ratio) / w;
    if (!std::isfinite(x)) return false;
    p = 0.5 * std::erfc(x / std::sqrt(2.0));
    return true;
}

} // namespace

extern "C" int hgibbs_set_tests(uint32_t m, const double* U, const double* Phi, const double* a, hgibbs_set_result* r)
{
    if (!U || !Phi || !a || !r) {
        hgibbs_set_error_("hgibbs_set_tests: null argument");
        return 1;
    }
    if (m == 0) {
        hgibbs_set_error_("hgibbs_set_tests: m = 0, at least one marker");
        return 1;
    }
    char msg[160];
    for (uint32_t j = 0; j < m; ++j) {
        if (!std::isfinite(U[j]) || !std::isfinite(a[j])) {
            snprintf(msg, sizeof msg, "hgibbs_set_tests: U[%u] = %g, a[%u] = %g: not finite", j, U[j], j, a[j]);
            hgibbs_set_error_(msg);
            return 1;
        }
        for (uint32_t k = j; k < m; ++k)
            if (!std::isfinite(Phi[(size_t)j * m + k])) {
                snprintf(msg, sizeof msg, "hgibbs_set_tests: Phi[%u][%u] = %g is not finite", j, k, Phi[(size_t)j * m + k]);
                hgibbs_set_error_(msg);
                return 1;
            }
    }
    r->q = r->p_skat = r->t_burden = r->p_burden = r->lam_sum = r->lam_max = NaN;
    r->neig = 0;
    r->skat_ok = 0;

    // burden: sums in row order over the full symmetric matrix (the upper triangle mirrored)
    auto phi = [&](uint32_t j, uint32_t k) { return j <= k ? Phi[(size_t)j * m + k] : Phi[(size_t)k * m + j]; };
    double su = 0.0, den = 0.0, dg = 0.0;
    for (uint32_t j = 0; j < m; ++j) {
        su += a[j] * U[j];
        dg += a[j] * a[j] * phi(j, j);
        double row = 0.0;
        for (uint32_t k = 0; k < m; ++k) row += phi(j, k) * a[k];
        den += a[j] * row;
    }
    if (den > 1e-9 * dg) {
        r->t_burden = su * su / den;
        r->p_burden = std::erfc(std::sqrt(r->t_burden / 2.0));
    }

    // SKAT
    std::vector<double> A((size_t)m * m), ev;
    for (uint32_t j = 0; j < m; ++j)
        for (uint32_t k = 0; k < m; ++k) A[(size_t)j * m + k] = a[j] * phi(j, k) * a[k];
    st_jacobi(A, m, ev);
    std::sort(ev.begin(), ev.end(), [](double x, double y) { return x > y; });
    std::vector<double> lam;
    if (ev[0] > 0.0)
        for (double l : ev)
            if (l > 1e-10 * ev[0]) lam.push_back(l);
    r->neig = (int32_t)lam.size();
    if (lam.empty()) return 0;
    double Q = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (uint32_t j = 0; j < m; ++j) Q += (a[j] * U[j]) * (a[j] * U[j]);
    for (double l : lam) {
        s1 += l;
        s2 += l * l;
        s3 += l * l * l;
    }
    r->q = Q;
    r->lam_sum = s1;
    r->lam_max = lam[0];
    const double k2_0 = 2.0 * s2, sd = std::sqrt(k2_0);
    if (std::fabs(Q - s1) < 1e-6 * sd) {
        r->p_skat = 0.5 * std::erfc(8.0 * s3 / (k2_0 * sd) / (6.0 * std::sqrt(2.0)));
        r->skat_ok = 1;
        return 0;
    }
    double p;
    if (st_tail(lam, Q, s1, k2_0, p)) {
        r->p_skat = p;
        r->skat_ok = 1;
    } else {
        r->p_skat = 0.5 * std::erfc((Q - s1) / sd / std::sqrt(2.0));
    }
    return 0;
}
