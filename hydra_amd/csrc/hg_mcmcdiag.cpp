// hg_mcmcdiag.cpp -- convergence diagnostics of R chains of one scalar parameter: host only, no HIP.
//
//   split chains   every chain of T draws is halved: draws [0, n) and [T - n, T) with n = T / 2, so an odd T drops the middle draw.
//                  m = 2 R half-chains of n draws each.
//   split-R^       Gelman et al., BDA3 section 11.4 (Vehtari et al. 2021 without the rank normalisation): with the half-chains'
//                  means and variances (n - 1 in the denominator), W = the mean of the variances, B / n = the variance of the means
//                  (m - 1 in the denominator), var+ = (n - 1) / n W + B / n, R^ = sqrt(var+ / W).
//   ESS            Stan reference manual, "Effective sample size": rho_t = 1 - (W - mean_k acov_k(t)) / var+ with the biased
//                  autocovariance acov_k(t) = 1/n sum_{i < n - t} (x_i - mean_k)(x_{i + t} - mean_k); the pairs P_k = rho_2k + rho_2k+1
//                  (rho_0 = 1) are taken while they are positive (Geyer's initial positive sequence) and each is lowered to the one
//                  before it (initial monotone sequence); tau = -1 + 2 sum P_k; ESS = m n / tau, at most m n log10(m n), which is
//                  also the value where tau is not positive (half-chains of two or three draws can give that).
//   W == 0         no half-chain moves: R^ and ESS are NaN.
//
// Every sum runs in index order, so the bits repeat.
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "../../include/hgibbs.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {
int dfail(const std::string& m)
{
    hgibbs_set_error_(m.c_str());
    return 1;
}
} // namespace

extern "C" int hgibbs_mcmc_diag(uint32_t R, uint32_t T, const double* x, double* mean, double* sd, double* rhat, double* ess)
{
    const char* who = "hgibbs_mcmc_diag";
    if (!x) return dfail(std::string(who) + ": null argument");
    if (R < 1u) return dfail(std::string(who) + ": R = 0, there must be at least one chain");
    if (T < 4u) return dfail(std::string(who) + ": T = " + std::to_string(T) + " draws per chain, split-R^ needs at least 4");
    const double nan = std::numeric_limits<double>::quiet_NaN();

    // mean and sd over all draws
    const size_t all = (size_t)R * T;
    double sum = 0.0;
    for (size_t i = 0; i < all; ++i) sum += x[i];
    const double mu = sum / (double)all;
    double ss = 0.0;
    for (size_t i = 0; i < all; ++i) ss += (x[i] - mu) * (x[i] - mu);
    if (mean) *mean = mu;
    if (sd) *sd = std::sqrt(ss / (double)(all - 1));

    const size_t n = T / 2u, m = 2 * (size_t)R;
    std::vector<const double*> half(m);
    for (uint32_t r = 0; r < R; ++r) {
        half[2 * (size_t)r] = x + (size_t)r * T;
        half[2 * (size_t)r + 1] = x + (size_t)r * T + (T - n);
    }
    std::vector<double> cm(m), cv(m);
    for (size_t k = 0; k < m; ++k) {
        double s = 0.0;
        for (size_t i = 0; i < n; ++i) s += half[k][i];
        cm[k] = s / (double)n;
        double q = 0.0;
        for (size_t i = 0; i < n; ++i) q += (half[k][i] - cm[k]) * (half[k][i] - cm[k]);
        cv[k] = q / (double)(n - 1);
    }
    double W = 0.0, gm = 0.0;
    for (size_t k = 0; k < m; ++k) {
        W += cv[k];
        gm += cm[k];
    }
    W /= (double)m;
    gm /= (double)m;
    double Bn = 0.0; // B / n
    for (size_t k = 0; k < m; ++k) Bn += (cm[k] - gm) * (cm[k] - gm);
    Bn /= (double)(m - 1);
    const double varp = (double)(n - 1) / (double)n * W + Bn;
    if (!(W > 0.0)) {
        if (rhat) *rhat = nan;
        if (ess) *ess = nan;
        return 0;
    }
    if (rhat) *rhat = std::sqrt(varp / W);
    if (!ess) return 0;

    auto rho = [&](size_t t) -> double {
        if (t == 0) return 1.0;
        double a = 0.0;
        for (size_t k = 0; k < m; ++k) {
            double s = 0.0;
            for (size_t i = 0; i + t < n; ++i) s += (half[k][i] - cm[k]) * (half[k][i + t] - cm[k]);
            a += s / (double)n;
        }
        return 1.0 - (W - a / (double)m) / varp;
    };
    double tau = -1.0, before = 0.0;
    for (size_t k = 0; 2 * k + 1 < n; ++k) {
        double P = rho(2 * k) + rho(2 * k + 1);
        if (!(P > 0.0)) break;
        if (k > 0 && P > before) P = before;
        tau += 2.0 * P;
        before = P;
    }
    const double mn = (double)(m * n), cap = mn * std::log10(mn);
    double e = tau > 0.0 ? mn / tau : cap;
    if (e > cap) e = cap;
    *ess = e;
    return 0;
}
