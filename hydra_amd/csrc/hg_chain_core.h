// hg_chain_core.h -- what hydra_chain.cpp (BayesR on genotypes) and hydra_ss_chain.cpp (BayesR from summary statistics) have in
// common: the K/G-sized state of BayesRRm::runMpiGibbs (src/BayesRRm.cpp), its initial values, the per-group hyper-parameter draws,
// the state copy and the .csv line.  Host code only.  Each chain keeps what differs: residual against c_j, how mu and e_sqn are
// obtained, covariates, restore, the host engine.  Both chains are held to the oracle bit for bit, so the order of the draws from
// the generator in here is part of the contract.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/hgibbs.h"
#include "hg_rng.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace hg {

inline int chain_fail(const std::string& m) // the library's error text; every entry point returns 1 with it
{
    hgibbs_set_error_(m.c_str());
    return 1;
}

const double V0E = 0.0001, S02E = 0.0001, V0G = 0.0001, S02G = 0.0001; // src/BayesRRm.h:30-33

struct ChainCore {
    int G = 1, K = 0;
    int shuffle = 1;
    std::vector<int32_t> groups, MtotGrp, order, cass, m0;
    std::vector<double> cVa, cVaI, priorPi, estPi, sigmaG;
    std::vector<uint8_t> adaV;
    double sigmaE = 0.0, mu = 0.0;
    hgibbs_rng_state rng{};
    uint64_t last_nnz = 0;
    uint32_t iteration = 0;
};

// The model tables (:1086-1110), the seed and sigmaG ~ beta(1, 1) (:1228-1240), the identity order (:1520-1521) and adaV
// (:1592-1597, and the markers a caller's `use` leaves out).  `who` is the entry point's name for the error text; the caller has
// checked K (and G, where it does).
inline int core_init(ChainCore& c, uint32_t M, const hydra_model_desc* model, const uint8_t* use, const char* who)
{
    c.G = model->G;
    c.K = model->K;
    c.shuffle = model->shuffle;
    const int G = c.G, K = c.K, km1 = K - 1;
    c.groups.assign(M, 0);
    if (model->groups) c.groups.assign(model->groups, model->groups + M);
    for (uint32_t i = 0; i < M; ++i)
        if (c.groups[i] < 0 || c.groups[i] >= G) return chain_fail(std::string(who) + ": group index out of range");

    // :1086-1110
    c.cVa.assign((size_t)G * K, 0.0);
    c.cVaI.assign((size_t)G * K, 0.0);
    c.priorPi.assign((size_t)G * K, 0.0);
    for (int g = 0; g < G; ++g) {
        c.priorPi[g * K] = 0.5;
        double s = 0.0;
        for (int k = 1; k <= km1; ++k) {
            const double v = model->mS[g * K + k];
            if (!(v > 0.0)) return chain_fail("FATAL  : mixture value can only be strictly positive"); // :992-993
            c.cVa[g * K + k] = v;
            c.cVaI[g * K + k] = 1.0 / v;
            s += v;
        }
        for (int k = 1; k <= km1; ++k) c.priorPi[g * K + k] = c.priorPi[g * K] * c.cVa[g * K + k] / s;
    }
    c.estPi = c.priorPi;
    c.sigmaG.assign(G, 0.0);
    c.cass.assign((size_t)G * K, 0);
    c.m0.assign(G, 0);
    c.MtotGrp.assign(G, 0);
    for (uint32_t i = 0; i < M; ++i) c.MtotGrp[c.groups[i]] += 1;

    // :1228-1240
    Mt gen{c.rng.x, 0};
    gen.seed(model->seed);
    for (int g = 0; g < G; ++g) c.sigmaG[g] = beta_rng(gen, 1.0, 1.0);
    for (int g = 0; g < G; ++g)
        if (c.MtotGrp[g] == 0) c.sigmaG[g] = 0.0;
    c.rng.idx = gen.idx;

    // :1520-1521
    c.order.resize(M);
    for (uint32_t i = 0; i < M; ++i) c.order[i] = (int32_t)i;

    // :1592-1597
    c.adaV.assign(M, 1);
    for (uint32_t i = 0; i < M; ++i)
        if (c.sigmaG[c.groups[i]] == 0.0 || (use && !use[i])) c.adaV[i] = 0;
    return 0;
}

// :2495-2578 -- per group: m0, a group with nothing in the model freezes out, else sigmaG and estPi.  bsq: G sums of beta^2.
inline void core_hyper(ChainCore& c, const double* bsq, Mt& gen)
{
    const int G = c.G, K = c.K;
    std::vector<double> dirin(K), pi(K);
    for (int g = 0; g < G; ++g) {
        if (c.MtotGrp[g] == 0) continue;
        c.m0[g] = c.MtotGrp[g] - c.cass[g * K];
        int rowsum = 0;
        for (int k = 0; k < K; ++k) rowsum += c.cass[g * K + k];
        if (c.m0[g] == 0 || rowsum == 0) {
            for (size_t i = 0; i < c.groups.size(); ++i)
                if (c.groups[i] == g) c.adaV[i] = 0;
            c.sigmaG[g] = 0.0;
            continue;
        }
        const double dm0 = (double)c.m0[g];
        c.sigmaG[g] = inv_scaled_chisq_rng(gen, V0G + dm0, (bsq[g] * dm0 + V0G * S02G) / (V0G + dm0));
        for (int k = 0; k < K; ++k) dirin[k] = (double)c.cass[g * K + k] + 1.0;
        dirichlet_rng(gen, dirin.data(), K, pi.data());
        for (int k = 0; k < K; ++k) c.estPi[g * K + k] = pi[k];
    }
}

inline void core_state(const ChainCore& c, double* sigmaE, double* mu, double* sigmaG, double* estPi, int32_t* m0, int32_t* cass,
                       hgibbs_rng_state* rng)
{
    if (sigmaE) *sigmaE = c.sigmaE;
    if (mu) *mu = c.mu;
    if (sigmaG) std::copy(c.sigmaG.begin(), c.sigmaG.end(), sigmaG);
    if (estPi) std::copy(c.estPi.begin(), c.estPi.end(), estPi);
    if (m0) std::copy(c.m0.begin(), c.m0.end(), m0);
    if (cass) std::copy(c.cass.begin(), c.cass.end(), cass);
    if (rng) *rng = c.rng;
}

/* the chain's .csv line, a11: src/BayesRRm.cpp:2742-2760 */
inline int core_csv_line(const ChainCore& c, uint32_t iteration, char* buf, size_t len)
{
    const int G = c.G, K = c.K;
    size_t o = 0;
    o += snprintf(buf + o, len - o, "%5d, %4d", (int)iteration, G);
    double sg = 0.0;
    for (int g = 0; g < G; ++g) {
        o += snprintf(buf + o, len - o, ", %20.15f", c.sigmaG[g]);
        sg += c.sigmaG[g];
    }
    int m0sum = 0;
    for (int g = 0; g < G; ++g) m0sum += c.m0[g];
    o += snprintf(buf + o, len - o, ", %20.15f, %20.15f, %7d, %4d, %2d", c.sigmaE, sg / (c.sigmaE + sg), m0sum, G, K);
    for (int g = 0; g < G; ++g)
        for (int k = 0; k < K; ++k) o += snprintf(buf + o, len - o, ", %20.15f", c.estPi[g * K + k]);
    o += snprintf(buf + o, len - o, "\n");
    return (int)o;
}

} // namespace hg
