// hg_sumstat.cpp -- the summary-statistics sweep on host arrays: no device, no HIP.  The same step as the
// device engine (hg_sumstat.hip.h) from the same header (hg_ss_step.h), with a band the caller supplies.  It is what the device is
// held to, and what a CPU test holds to the oracle's chain: with a band that covers every pair, c_j is x_j'eps of the chain.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/hgibbs.h"
#include "hg_ss_step.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {
int sfail(const std::string& m)
{
    hgibbs_set_error_(m.c_str());
    return 1;
}

// What a sweep on host arrays is given (both entry points), and what both check about it
struct HostSweep {
    uint32_t M;
    double n_eff;
    uint32_t W;
    const uint32_t* ahead;
    const double* band;
    double *c, *beta;
    int32_t* components;
    double* acum;
    int G, K;
    const int32_t* groups;
    const double *cVa, *cVaI;
    const int32_t* order;
    double sigmaE;
    const double *sigmaG, *estPi;
    const uint8_t* adaV;
    int32_t* cass;
};

int host_check(const char* who, const HostSweep& a)
{
    if (!a.ahead || !a.band || !a.c || !a.beta || !a.components || !a.acum || !a.cVa || !a.cVaI || !a.order || !a.sigmaG || !a.estPi || !a.adaV || !a.cass)
        return sfail(std::string(who) + ": null argument");
    const uint32_t M = a.M, W = a.W;
    if (M == 0) return sfail(std::string(who) + ": no markers");
    if (W == 0 || W > hg::SS_WMAX) return sfail(std::string(who) + ": W = " + std::to_string(W) + ", must be in [1, " + std::to_string(hg::SS_WMAX) + "]");
    if (!(std::isfinite(a.n_eff) && a.n_eff >= 2.0)) return sfail(std::string(who) + ": n_eff must be a finite number >= 2");
    if (a.G < 1 || a.K < 2 || a.K > hg::SS_MAX_K) return sfail(std::string(who) + ": need G >= 1 and 2 <= K <= " + std::to_string(hg::SS_MAX_K));
    for (uint32_t j = 0; j < M; ++j) {
        if (a.ahead[j] > W) return sfail(std::string(who) + ": ahead[" + std::to_string(j) + "] = " + std::to_string(a.ahead[j]) + " is above W = " + std::to_string(W));
        if ((uint64_t)j + a.ahead[j] >= M) return sfail(std::string(who) + ": marker " + std::to_string(j) + " + ahead is past the last marker");
        if (a.groups && (a.groups[j] < 0 || a.groups[j] >= a.G)) return sfail(std::string(who) + ": group index out of range");
        if (a.order[j] < 0 || (uint32_t)a.order[j] >= M) return sfail(std::string(who) + ": order[" + std::to_string(j) + "] outside [0, M)");
    }
    return 0;
}

// The sweep of both entry points: the markers order[p0 .. p1) with one generator, interval after interval where there are several.
// cass and *nnz accumulate.
struct HostEngine {
    const HostSweep& a;
    std::vector<uint32_t> back;
    std::vector<double> tab;
    hg::ZigTables zt;
    HostEngine(const HostSweep& a_) : a(a_), back(a_.M), tab((size_t)4 * a_.G * a_.K), zt(hg::host_tables())
    {
        hg::ss_back(a.M, a.ahead, back.data());
        hg::ss_tables(a.G, a.K, a.n_eff - 1.0, a.sigmaE, a.sigmaG, a.estPi, a.cVa, a.cVaI, tab.data());
        for (int i = 0; i < a.G * a.K; ++i) a.cass[i] = 0;
    }
    int walk(const char* who, const int32_t* order, uint32_t p0, uint32_t p1, hgibbs_rng_state* rng, uint64_t& nnz)
    {
        const uint32_t W = a.W;
        const int G = a.G, K = a.K;
        const double dNm1 = a.n_eff - 1.0, i_2sigE = 1.0 / (2.0 * a.sigmaE);
        const double* denom = tab.data();
        const double* logpi = denom + (size_t)G * K;
        const double* hlog = logpi + (size_t)G * K;
        const double* sdk = hlog + (size_t)G * K;
        double *c = a.c, *beta = a.beta;
        hg::Mt gen{rng->x, rng->idx};
        for (uint32_t p = p0; p < p1; ++p) {
            const uint32_t j = (uint32_t)order[p];
            const int g = a.groups ? a.groups[j] : 0;
            const double bold = beta[j];
            if (a.adaV[j]) {
                int k = 0;
                if (hg::ss_marker_draw(c[j] + bold * dNm1, K, denom + (size_t)g * K, logpi + (size_t)g * K, hlog + (size_t)g * K, sdk + (size_t)g * K, i_2sigE,
                                       gen, zt, beta[j], k, a.acum[j]))
                    return sfail(std::string(who) + ": marker " + std::to_string(j) + ": the component walk found no component (logL overflow)");
                a.cass[g * K + k] += 1;
                a.components[j] = k;
            } else {
                beta[j] = 0.0;
                a.acum[j] = 1.0;
            }
            const double delta = bold - beta[j];
            if (delta != 0.0) {
                const double* row = a.band + (size_t)j * W;
                for (uint32_t d = 1; d <= a.ahead[j]; ++d) c[j + d] += delta * row[d - 1];
                for (uint32_t d = 1; d <= back[j]; ++d) {
                    const uint32_t k = j - d;
                    if (a.ahead[k] >= d) c[k] += delta * a.band[(size_t)k * W + d - 1];
                }
                c[j] += delta * dNm1;
                ++nnz;
            }
        }
        rng->idx = gen.idx;
        return 0;
    }
};
} // namespace

extern "C" int hgibbs_ss_sweep_host(uint32_t M, double n_eff, uint32_t W, const uint32_t* ahead, const double* band, double* c, double* beta,
                                    int32_t* components, double* acum, int G, int K, const int32_t* groups, const double* cVa, const double* cVaI,
                                    const int32_t* order, double sigmaE, const double* sigmaG, const double* estPi, const uint8_t* adaV,
                                    hgibbs_rng_state* rng, int32_t* cass, uint64_t* nnz_updates)
{
    const char* who = "hgibbs_ss_sweep_host";
    const HostSweep a{M, n_eff, W, ahead, band, c, beta, components, acum, G, K, groups, cVa, cVaI, order, sigmaE, sigmaG, estPi, adaV, cass};
    if (!rng) return sfail(std::string(who) + ": null argument");
    if (host_check(who, a)) return 1;
    if (rng->idx > (uint32_t)hg::MT_N) return sfail(std::string(who) + ": rng idx > 624");
    HostEngine e(a);
    uint64_t nnz = 0;
    if (e.walk(who, order, 0, M, rng, nnz)) return 1;
    if (nnz_updates) *nnz_updates = nnz;
    return 0;
}

extern "C" int hgibbs_ss_sweep_streams_host(uint32_t M, double n_eff, uint32_t W, const uint32_t* ahead, const double* band, double* c, double* beta,
                                            int32_t* components, double* acum, int G, int K, const int32_t* groups, const double* cVa,
                                            const double* cVaI, const int32_t* order, double sigmaE, const double* sigmaG, const double* estPi,
                                            const uint8_t* adaV, uint32_t S, const uint32_t* bounds, hgibbs_rng_state* rngs, int32_t* cass,
                                            uint64_t* nnz_updates)
{
    const char* who = "hgibbs_ss_sweep_streams_host";
    const HostSweep a{M, n_eff, W, ahead, band, c, beta, components, acum, G, K, groups, cVa, cVaI, order, sigmaE, sigmaG, estPi, adaV, cass};
    if (!bounds || !rngs) return sfail(std::string(who) + ": null argument");
    if (host_check(who, a)) return 1;
    std::vector<uint8_t> cut(M);
    hg::ss_cuts(M, ahead, cut.data());
    char why[256];
    if (hg::ss_streams_check(M, ahead, cut.data(), S, bounds, rngs, why, sizeof why)) return sfail(std::string(who) + ": " + why);
    std::vector<int32_t> grouped(M);
    if (const uint32_t bad = hg::ss_group_order(M, order, S, bounds, grouped.data()))
        return sfail(std::string(who) + ": order[" + std::to_string(bad - 1u) + "] = " + std::to_string(order[bad - 1u]) + " repeats a marker: the order must be a permutation");
    HostEngine e(a);
    uint64_t nnz = 0;
    for (uint32_t s = 0; s < S; ++s)
        if (e.walk(who, grouped.data(), bounds[s], bounds[s + 1], &rngs[s], nnz)) return 1;
    if (nnz_updates) *nnz_updates = nnz;
    return 0;
}

extern "C" int hgibbs_ss_partition(uint32_t M, const uint32_t* ahead, uint32_t S_max, uint32_t* bounds, uint32_t* S)
{
    const char* who = "hgibbs_ss_partition";
    if (!ahead || !bounds || !S) return sfail(std::string(who) + ": null argument");
    if (M == 0) return sfail(std::string(who) + ": no markers");
    if (S_max < 1u || S_max > hg::SS_SMAX) return sfail(std::string(who) + ": S_max = " + std::to_string(S_max) + ", must be in [1, " + std::to_string(hg::SS_SMAX) + "]");
    for (uint32_t j = 0; j < M; ++j)
        if ((uint64_t)j + ahead[j] >= M) return sfail(std::string(who) + ": marker " + std::to_string(j) + " + ahead is past the last marker");
    hg::ss_partition(M, ahead, S_max, bounds, S);
    return 0;
}
