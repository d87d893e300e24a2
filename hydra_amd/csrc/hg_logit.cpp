// hg_logit.cpp -- the null model of the logistic score test of --assoc --assoc-logistic: plain C++, no HIP.
//
//     int hgibbs_logit_null(uint32_t n, int q, const double* Z, const double* y,
//                           double* coef, double* mu, double* w, double* chol, int* iters);
//
//   Z      n x q, column-major (Z[a n + i]), the first column all ones          y      n entries, each 0 or 1
//   coef   q maximum-likelihood coefficients of  logit P(y_i = 1) = sum_a Z_ia coef_a
//   mu     n fitted probabilities at coef,  w = mu (1 - mu)
//   chol   q x q column-major: the lower Cholesky factor L of Z'WZ at coef (L L' = Z'WZ, L[a + q b] for a >= b, zero above)
//   iters  Newton steps taken, the closing one included (may be NULL)
//
// Method: Newton / IRLS in f64 from coef = 0.  At an iterate: eta = Z coef, mu, w, the score s = Z'(y - mu), the information
// I = Z'WZ and its Cholesky factor; the step is I^-1 s.  The step is halved (at most 30 times) while the deviance
// 2 sum_i [log(1 + e^eta_i) - y_i eta_i] at the new iterate lies above the one it left by more than 1e-12 of it: near the maximum
// a step changes the deviance by less than the rounding of its sum, and a rise of that size is no reason to halve.  Every sum over
// the rows runs in row order and nothing is threaded, so equal inputs give equal bits.
//
// Stop rule: when max_a |s_a| / sqrt(I_aa) <= 1e-10 the fit takes ONE more full step (no halving) and ends there; mu, w and chol are
// evaluated at that last point.  At most 50 steps.
//
// Refused, each with a message that names the reason:
//   - a null argument, q < 1 or q > 64, a non-finite entry of Z, a first column that is not all ones;
//   - fewer rows than q + 2;
//   - a y outside {0, 1};
//   - dependent columns: Z'WZ has no Cholesky factor (a pivot at or below 1e-10 of its diagonal entry, at any iterate);
//   - separation: the stop rule is not met within 50 steps, or at some iterate every row is fitted to within 1e-6 of its y (the
//     likelihood has no maximum: the coefficients run off and w goes to zero everywhere, where the stop rule's ratio is 0/0).
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/hgibbs.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {

constexpr int LG_QMAX = 64;
constexpr int LG_ITERS = 50;
constexpr int LG_HALVINGS = 30;
constexpr double LG_STOP = 1e-10;
constexpr double LG_PIVOT = 1e-10;
constexpr double LG_FITTED = 1e-6;
constexpr double LG_RISE = 1e-12;

int lfail(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    hgibbs_set_error_(buf);
    return 1;
}

struct Fit {
    uint32_t n;
    int q;
    const double* Z;
    const double* y;
    std::vector<double> eta;

    // eta = Z b and the deviance there, in row order
    double deviance(const std::vector<double>& b)
    {
        for (uint32_t i = 0; i < n; ++i) eta[i] = 0.0;
        for (int a = 0; a < q; ++a) {
            const double* z = Z + (size_t)a * n;
            const double ba = b[a];
            for (uint32_t i = 0; i < n; ++i) eta[i] += z[i] * ba;
        }
        double d = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const double e = eta[i];
            const double l1p = e > 0.0 ? e + std::log1p(std::exp(-e)) : std::log1p(std::exp(e)); // log(1 + e^eta)
            d += l1p - y[i] * e;
        }
        return 2.0 * d;
    }

    // mu and w from the eta of the last deviance(); returns max_i |y_i - mu_i|
    double moments(double* mu, double* w) const
    {
        double worst = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const double e = eta[i];
            const double m = e >= 0.0 ? 1.0 / (1.0 + std::exp(-e)) : std::exp(e) / (1.0 + std::exp(e));
            mu[i] = m;
            w[i] = m * (1.0 - m);
            worst = std::fmax(worst, std::fabs(y[i] - m));
        }
        return worst;
    }

    // s = Z'(y - mu) and the lower triangle of I = Z'WZ (column-major q x q), in row order
    void score_info(const double* mu, const double* w, std::vector<double>& s, std::vector<double>& I) const
    {
        for (int a = 0; a < q; ++a) {
            const double* za = Z + (size_t)a * n;
            double sa = 0.0;
            for (uint32_t i = 0; i < n; ++i) sa += za[i] * (y[i] - mu[i]);
            s[a] = sa;
            for (int b = 0; b <= a; ++b) {
                const double* zb = Z + (size_t)b * n;
                double v = 0.0;
                for (uint32_t i = 0; i < n; ++i) v += w[i] * za[i] * zb[i];
                I[(size_t)a + (size_t)q * b] = v;
            }
        }
    }
};

// L L' = I on the lower triangle (column-major), zero above; the column whose pivot fails, or -1
int cholesky(int q, const std::vector<double>& I, double* L)
{
    for (int k = 0; k < q * q; ++k) L[k] = 0.0;
    for (int b = 0; b < q; ++b) {
        double d = I[(size_t)b + (size_t)q * b];
        for (int k = 0; k < b; ++k) d -= L[b + q * k] * L[b + q * k];
        if (!(d > LG_PIVOT * I[(size_t)b + (size_t)q * b]) || !std::isfinite(d)) return b;
        const double r = std::sqrt(d);
        L[b + q * b] = r;
        for (int a = b + 1; a < q; ++a) {
            double v = I[(size_t)a + (size_t)q * b];
            for (int k = 0; k < b; ++k) v -= L[a + q * k] * L[b + q * k];
            L[a + q * b] = v / r;
        }
    }
    return -1;
}

// x = (L L')^-1 s
void chol_solve(int q, const double* L, const std::vector<double>& s, std::vector<double>& x)
{
    for (int a = 0; a < q; ++a) {
        double v = s[a];
        for (int k = 0; k < a; ++k) v -= L[a + q * k] * x[k];
        x[a] = v / L[a + q * a];
    }
    for (int a = q - 1; a >= 0; --a) {
        double v = x[a];
        for (int k = a + 1; k < q; ++k) v -= L[k + q * a] * x[k];
        x[a] = v / L[a + q * a];
    }
}

} // namespace

extern "C" int hgibbs_logit_null(uint32_t n, int q, const double* Z, const double* y, double* coef, double* mu, double* w, double* chol,
                                 int* iters)
{
    if (!Z || !y || !coef || !mu || !w || !chol) return lfail("hgibbs_logit_null: null argument");
    if (q < 1 || q > LG_QMAX) return lfail("hgibbs_logit_null: q = %d, must be in [1, %d]", q, LG_QMAX);
    if ((uint64_t)n < (uint64_t)q + 2u) return lfail("hgibbs_logit_null: %u rows, %d columns need at least %d", n, q, q + 2);
    for (uint32_t i = 0; i < n; ++i)
        if (!(y[i] == 0.0 || y[i] == 1.0)) return lfail("hgibbs_logit_null: y[%u] = %g is outside {0, 1}", i, y[i]);
    for (size_t k = 0; k < (size_t)q * n; ++k)
        if (!std::isfinite(Z[k])) return lfail("hgibbs_logit_null: Z[%zu][%d] = %g is not finite", k % n, (int)(k / n), Z[k]);
    for (uint32_t i = 0; i < n; ++i)
        if (Z[i] != 1.0) return lfail("hgibbs_logit_null: Z[%u][0] = %g, the first column must be all ones", i, Z[i]);

    Fit f{n, q, Z, y, std::vector<double>(n)};
    std::vector<double> b(q, 0.0), nb(q), s(q), I((size_t)q * q, 0.0), step(q);
    double dev = f.deviance(b);
    int steps = 0;
    for (;;) {
        // (eta is that of b here)
        const double worst = f.moments(mu, w);
        if (worst < LG_FITTED)
            return lfail("hgibbs_logit_null: separation: after %d steps every row is fitted to within %g of its y, the likelihood has no maximum", steps,
                         LG_FITTED);
        f.score_info(mu, w, s, I);
        const int bad = cholesky(q, I, chol);
        if (bad >= 0) return lfail("hgibbs_logit_null: dependent columns: Z'WZ has no Cholesky factor (column %d, after %d steps)", bad, steps);
        double crit = 0.0;
        for (int a = 0; a < q; ++a) crit = std::fmax(crit, std::fabs(s[a]) / std::sqrt(I[(size_t)a + (size_t)q * a]));
        const bool last = crit <= LG_STOP;
        if (!last && steps >= LG_ITERS - 1) // (the closing step is one of the 50)
            return lfail("hgibbs_logit_null: separation: no convergence within %d steps (max |score| / sqrt(info) = %.3g)", LG_ITERS, crit);
        chol_solve(q, chol, s, step);
        double t = 1.0, nd = 0.0;
        for (int h = 0;; ++h) {
            for (int a = 0; a < q; ++a) nb[a] = b[a] + t * step[a];
            nd = f.deviance(nb);
            if (last || !(nd > dev * (1.0 + LG_RISE)) || h >= LG_HALVINGS) break;
            t *= 0.5;
        }
        b = nb;
        dev = nd;
        ++steps;
        if (last) break;
    }
    // the results at the last point
    (void)f.moments(mu, w);
    f.score_info(mu, w, s, I);
    const int bad = cholesky(q, I, chol);
    if (bad >= 0) return lfail("hgibbs_logit_null: dependent columns: Z'WZ has no Cholesky factor (column %d, after %d steps)", bad, steps);
    for (int a = 0; a < q; ++a) coef[a] = b[a];
    if (iters) *iters = steps;
    return 0;
}
