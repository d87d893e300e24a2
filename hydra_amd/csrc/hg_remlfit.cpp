// hg_remlfit.cpp -- the host half of --reml: plain C++, no HIP.
//
//   hgibbs_reml_next    the root rule on x = log delta: start point, first step by the sign of f_0, then secant steps clamped to
//                       |x| <= log 9999; done when two evaluated points lie closer than x_tol.
//   hgibbs_reml_finish  the estimate at the last evaluated point from the sums of hgibbs_reml_eval: variance components, their
//                       standard errors from the average-information matrix, and SE_MC, the leave-one-probe-out jackknife of the root.
//
// Both are sequential f64 in a fixed order under -ffp-contract=off; the transcendental calls are libm's log, exp and sqrt.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/hgibbs.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {

int rfail(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    hgibbs_set_error_(buf);
    return 1;
}

double clampx(double x)
{
    const double b = std::log(9999.0);
    return x > b ? b : x < -b ? -b : x;
}

// f from the sums of one evaluation ((T + 1) x 3: vAv, vv, vb), probe `skip` left out (-1: none), the sums ascending in t
double f_of(const double* s, int T, int skip)
{
    double a = 0.0, b = 0.0;
    for (int t = 0; t < T; ++t) {
        if (t == skip) continue;
        a += s[3 * t];
        b += s[3 * t + 1];
    }
    return std::log(a / b) - std::log(s[3 * T] / s[3 * T + 1]);
}

} // namespace

extern "C" int hgibbs_reml_next(int k, const double* x, const double* f, double h0, double x_tol, int max_steps, double* x_next, int* status)
{
    if (!x_next || !status || (k > 0 && (!x || !f))) return rfail("hgibbs_reml_next: null argument");
    if (k < 0) return rfail("hgibbs_reml_next: k = %d evaluated points", k);
    if (!(h0 > 0.0) || !(h0 < 1.0)) return rfail("hgibbs_reml_next: h2_start = %g, must lie inside (0, 1)", h0);
    if (!(x_tol > 0.0) || !std::isfinite(x_tol)) return rfail("hgibbs_reml_next: x_tol = %g, must be positive and finite", x_tol);
    if (max_steps < 2) return rfail("hgibbs_reml_next: max_steps = %d, the rule needs at least two evaluations", max_steps);
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(x[i]) || !std::isfinite(f[i])) return rfail("hgibbs_reml_next: point %d (x = %g, f = %g) is not finite", i, x[i], f[i]);
    *status = HGIBBS_REML_CONTINUE;
    if (k == 0) {
        *x_next = std::log((1.0 - h0) / h0);
        return 0;
    }
    if (k == 1) {
        const double h1 = f[0] < 0.0 ? std::fmin(2.0 * h0, (1.0 + h0) / 2.0) : h0 / 2.0; // f < 0: delta is too large, so h2 goes up
        *x_next = std::log((1.0 - h1) / h1);
        return 0;
    }
    const double x1 = x[k - 1], x0 = x[k - 2], f1 = f[k - 1], f0 = f[k - 2];
    *x_next = x1;
    if (x1 == x0 && std::fabs(x1) == std::log(9999.0)) {
        *status = HGIBBS_REML_AT_BOUND;
        return 0;
    }
    if (std::fabs(x1 - x0) < x_tol) {
        *status = HGIBBS_REML_CONVERGED;
        return 0;
    }
    if (f1 == f0) return rfail("hgibbs_reml_next: f is flat: f(%.9g) = f(%.9g) = %.9g after %d evaluations, no secant step", x0, x1, f1, k);
    if (k >= max_steps) return rfail("hgibbs_reml_next: no root after max_steps = %d evaluations (last step %.3g in log delta, f = %.3g)", max_steps, x1 - x0, f1);
    *x_next = clampx(x1 - f1 * (x1 - x0) / (f1 - f0));
    return 0;
}

extern "C" int hgibbs_reml_finish(int T, uint32_t n, int q, const double* x2, const double* sums_prev, const double* sums_last, const double* ai3,
                                  hgibbs_reml_estimate* out)
{
    if (!x2 || !sums_prev || !sums_last || !out) return rfail("hgibbs_reml_finish: null argument");
    if (T < 1 || T > 31) return rfail("hgibbs_reml_finish: trials = %d, must be in [1, 31]", T);
    if (q < 1 || (uint64_t)q + 1u >= n) return rfail("hgibbs_reml_finish: q = %d covariate columns against n = %u rows", q, n);
    for (int i = 0; i < 3 * (T + 1); ++i)
        if (!std::isfinite(sums_prev[i]) || !std::isfinite(sums_last[i])) return rfail("hgibbs_reml_finish: sum %d of probe %d is not finite", i % 3, i / 3);
    if (!std::isfinite(x2[0]) || !std::isfinite(x2[1])) return rfail("hgibbs_reml_finish: a point is not finite");
    hgibbs_reml_estimate e{};
    const double nan = std::nan("");
    e.logdelta = x2[1];
    e.delta = std::exp(x2[1]);
    e.vg = sums_last[3 * T + 2] / (double)(n - (uint32_t)q);
    e.ve = e.delta * e.vg;
    e.vp = e.vg + e.ve;
    e.h2 = 1.0 / (1.0 + e.delta);
    e.se_vg = e.se_ve = e.se_vp = e.se_h2 = e.se_mc = e.se_logdelta_mc = nan;
    if (ai3) {
        // AI = k [[a'z1, a'z2], [a'z2, v'z2]], k = 1 / (2 vg^3); the covariance of (vg, ve) is its inverse
        const double k = 1.0 / (2.0 * e.vg * e.vg * e.vg);
        const double a11 = k * ai3[0], a12 = k * ai3[1], a22 = k * ai3[2];
        const double det = a11 * a22 - a12 * a12;
        if (det > 0.0 && a11 > 0.0 && std::isfinite(det)) {
            const double c11 = a22 / det, c12 = -a12 / det, c22 = a11 / det;
            e.se_vg = std::sqrt(c11);
            e.se_ve = std::sqrt(c22);
            e.se_vp = std::sqrt(c11 + c22 + 2.0 * c12);
            const double g1 = e.ve / (e.vp * e.vp), g2 = -e.vg / (e.vp * e.vp); // d h2 / d vg, d h2 / d ve
            e.se_h2 = std::sqrt(g1 * g1 * c11 + 2.0 * g1 * g2 * c12 + g2 * g2 * c22);
        }
    }
    if (T >= 2) {
        // leave one probe out: f at both points without probe t, and the secant root through them
        std::vector<double> r(T);
        double mean = 0.0;
        bool ok = true;
        for (int t = 0; t < T; ++t) {
            const double f0 = f_of(sums_prev, T, t), f1 = f_of(sums_last, T, t);
            r[t] = x2[1] - f1 * (x2[1] - x2[0]) / (f1 - f0);
            if (!std::isfinite(r[t])) ok = false;
            mean += r[t];
        }
        if (ok) {
            mean /= (double)T;
            double ss = 0.0;
            for (int t = 0; t < T; ++t) ss += (r[t] - mean) * (r[t] - mean);
            e.se_logdelta_mc = std::sqrt((double)(T - 1) / (double)T * ss);
            e.se_mc = e.se_logdelta_mc * e.h2 * (1.0 - e.h2);
        }
    }
    *out = e;
    return 0;
}
