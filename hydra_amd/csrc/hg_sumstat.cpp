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
} // namespace

extern "C" int hgibbs_ss_sweep_host(uint32_t M, double n_eff, uint32_t W, const uint32_t* ahead, const double* band, double* c, double* beta,
                                    int32_t* components, double* acum, int G, int K, const int32_t* groups, const double* cVa, const double* cVaI,
                                    const int32_t* order, double sigmaE, const double* sigmaG, const double* estPi, const uint8_t* adaV,
                                    hgibbs_rng_state* rng, int32_t* cass, uint64_t* nnz_updates)
{
    const char* who = "hgibbs_ss_sweep_host";
    if (!ahead || !band || !c || !beta || !components || !acum || !cVa || !cVaI || !order || !sigmaG || !estPi || !adaV || !rng || !cass)
        return sfail(std::string(who) + ": null argument");
    if (M == 0) return sfail(std::string(who) + ": no markers");
    if (W == 0 || W > hg::SS_WMAX) return sfail(std::string(who) + ": W = " + std::to_string(W) + ", must be in [1, " + std::to_string(hg::SS_WMAX) + "]");
    if (!(std::isfinite(n_eff) && n_eff >= 2.0)) return sfail(std::string(who) + ": n_eff must be a finite number >= 2");
    if (G < 1 || K < 2 || K > hg::SS_MAX_K) return sfail(std::string(who) + ": need G >= 1 and 2 <= K <= " + std::to_string(hg::SS_MAX_K));
    if (rng->idx > (uint32_t)hg::MT_N) return sfail(std::string(who) + ": rng idx > 624");
    for (uint32_t j = 0; j < M; ++j) {
        if (ahead[j] > W) return sfail(std::string(who) + ": ahead[" + std::to_string(j) + "] = " + std::to_string(ahead[j]) + " is above W = " + std::to_string(W));
        if ((uint64_t)j + ahead[j] >= M) return sfail(std::string(who) + ": marker " + std::to_string(j) + " + ahead is past the last marker");
        if (groups && (groups[j] < 0 || groups[j] >= G)) return sfail(std::string(who) + ": group index out of range");
        if (order[j] < 0 || (uint32_t)order[j] >= M) return sfail(std::string(who) + ": order[" + std::to_string(j) + "] outside [0, M)");
    }
    std::vector<uint32_t> back(M);
    hg::ss_back(M, ahead, back.data());
    const double dNm1 = n_eff - 1.0, i_2sigE = 1.0 / (2.0 * sigmaE);
    std::vector<double> tab((size_t)4 * G * K);
    hg::ss_tables(G, K, dNm1, sigmaE, sigmaG, estPi, cVa, cVaI, tab.data());
    const double* denom = tab.data();
    const double* logpi = denom + (size_t)G * K;
    const double* hlog = logpi + (size_t)G * K;
    const double* sdk = hlog + (size_t)G * K;
    const hg::ZigTables zt = hg::host_tables();
    hg::Mt gen{rng->x, rng->idx};
    for (int i = 0; i < G * K; ++i) cass[i] = 0;
    uint64_t nnz = 0;

    for (uint32_t p = 0; p < M; ++p) {
        const uint32_t j = (uint32_t)order[p];
        const int g = groups ? groups[j] : 0;
        const double bold = beta[j];
        if (adaV[j]) {
            int k = 0;
            if (hg::ss_marker_draw(c[j] + bold * dNm1, K, denom + (size_t)g * K, logpi + (size_t)g * K, hlog + (size_t)g * K, sdk + (size_t)g * K, i_2sigE, gen,
                                   zt, beta[j], k, acum[j]))
                return sfail(std::string(who) + ": marker " + std::to_string(j) + ": the component walk found no component (logL overflow)");
            cass[g * K + k] += 1;
            components[j] = k;
        } else {
            beta[j] = 0.0;
            acum[j] = 1.0;
        }
        const double delta = bold - beta[j];
        if (delta != 0.0) {
            const double* row = band + (size_t)j * W;
            for (uint32_t d = 1; d <= ahead[j]; ++d) c[j + d] += delta * row[d - 1];
            for (uint32_t d = 1; d <= back[j]; ++d) {
                const uint32_t k = j - d;
                if (ahead[k] >= d) c[k] += delta * band[(size_t)k * W + d - 1];
            }
            c[j] += delta * dNm1;
            ++nnz;
        }
    }
    rng->idx = gen.idx;
    if (nnz_updates) *nnz_updates = nnz;
    return 0;
}
