// hg_ss_step.h -- what the two engines of the summary-statistics sweep share: the per-marker step of
// src/BayesRRm.cpp:1721-1723, 1744-1753, 1855-1921 as a plain f64 restatement, written once for host (hg_sumstat.cpp) and device
// (hg_sumstat.hip.h), the per-sweep tables of its marker-independent factors, the window's backward reach, and the cuts and
// intervals of the band's independent blocks with what both engines check about them (section 32).
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "hg_rng.h"

namespace hg {

constexpr int SS_MAX_K = 8;          // mixture components incl. zero (hgibbs_set_model's MAX_K)
constexpr uint32_t SS_WMAX = 4096u;  // widest window (hgibbs_ld's)

// The marker-independent factors of a group, one sweep: G*K each, column 0 unused but for logpi (hgibbs_sweep builds the same four)
//   denom = (n - 1) + sigmaE / sigmaG / cVa      logpi = log(pi)      hlog = 0.5 log(sigmaG / sigmaE (n - 1) cVa + 1)      sdk = sqrt(sigmaE / denom)
inline void ss_tables(int G, int K, double dNm1, double sigmaE, const double* sigmaG, const double* estPi, const double* cVa, const double* cVaI,
                      double* tab /* 4 G K */)
{
    double* denom = tab;
    double* logpi = denom + (size_t)G * K;
    double* hlog = logpi + (size_t)G * K;
    double* sdk = hlog + (size_t)G * K;
    for (int g = 0; g < G; ++g) {
        const double sigE_G = sigmaE / sigmaG[g];
        const double sigG_E = sigmaG[g] / sigmaE;
        for (int k = 0; k < K; ++k) {
            denom[g * K + k] = hlog[g * K + k] = sdk[g * K + k] = 0.0;
            logpi[g * K + k] = log(estPi[g * K + k]);
            if (k >= 1) {
                denom[g * K + k] = dNm1 + sigE_G * cVaI[g * K + k];
                hlog[g * K + k] = 0.5 * log(sigG_E * dNm1 * cVa[g * K + k] + 1.0);
                sdk[g * K + k] = sqrt(sigmaE / denom[g * K + k]);
            }
        }
    }
}

// One adaptive marker.  num = c_j + (n - 1) beta_old; the four tables at the marker's group; i_2sigE = 1 / (2 sigmaE).  Takes the
// uniform, walks the components and draws the normal in the reference's order.  Returns 0, or -1 on the reference's abort (:1910-1913).
template <class Gen, class Tab>
HG_HD int ss_marker_draw(double num, int K, const double* denom, const double* logpi, const double* hlog, const double* sdk, double i_2sigE,
                         Gen& gen, const Tab& zt, double& beta_new, int& component, double& acum_out)
{
    double muk[SS_MAX_K], logL[SS_MAX_K];
    muk[0] = 0.0;
    logL[0] = logpi[0];
#pragma unroll
    for (int i = 1; i < SS_MAX_K; ++i) {
        muk[i] = 0.0;
        logL[i] = 0.0;
        if (i < K) {
            muk[i] = num / denom[i];
            logL[i] = logpi[i] - hlog[i] + muk[i] * num * i_2sigE;
        }
    }
    const double prob = unif01(gen);

    // acum after component k of the walk: the share of component k (0 where a log-likelihood is more than 700 away from it)
    auto share = [&](int k) {
        bool big = false;
        double s = 0.0;
#pragma unroll
        for (int l = 0; l < SS_MAX_K; ++l)
            if (l < K) {
                // (the reference tests the components from 1 on against component 0, and those behind k against k + 1)
                if (l > k && fabs(logL[l] - logL[k]) > 700.0) big = true;
                s += exp(logL[l] - logL[k]);
            }
        return big ? 0.0 : 1.0 / s;
    };
    double acum = share(0);
    acum_out = acum;
#pragma unroll
    for (int k = 0; k < SS_MAX_K; ++k) {
        if (k >= K) break;
        if (prob <= acum || k == K - 1) {
            beta_new = (k == 0) ? 0.0 : norm_rng_sd(gen, zt, muk[k], sdk[k]);
            component = k;
            return 0;
        }
        if (k + 1 < SS_MAX_K) acum += share(k + 1);
    }
    return -1;
}

// back[q] = the farthest marker behind q whose window holds q, as a distance: q - min{k < q : k + ahead[k] >= q}, 0 where there is
// none.  A marker between the two need not reach q: the engines test ahead[k] >= q - k per neighbour.  O(M): k ascending, the first
// marker that covers q is the farthest.
inline void ss_back(uint32_t M, const uint32_t* ahead, uint32_t* back)
{
    uint64_t filled = 0;
    for (uint32_t q = 0; q < M; ++q) back[q] = 0u;
    for (uint32_t k = 0; k < M; ++k) {
        const uint64_t hi = (uint64_t)k + ahead[k];
        for (uint64_t q = (filled > k ? filled : k) + 1; q <= hi && q < M; ++q) back[q] = (uint32_t)(q - k);
        if (hi > filled) filled = hi;
    }
}

// ---- independent blocks of the band, swept at the same time ----
constexpr uint32_t SS_SMAX = 1024u; // intervals of one sweep: about what the device holds resident at once (a size limit only)

// cut[j] = 1 iff no window crosses the place before marker j: max over k < j of (k + ahead[k]) < j.  The running maximum, not
// back[j] == 0: a marker that no window holds can still be jumped over by a window from further back.  cut[0] = 1.
inline void ss_cuts(uint32_t M, const uint32_t* ahead, uint8_t* cut)
{
    uint64_t reach = 0;
    for (uint32_t j = 0; j < M; ++j) {
        cut[j] = (j == 0 || reach < j) ? 1 : 0;
        const uint64_t hi = (uint64_t)j + ahead[j];
        if (hi > reach) reach = hi;
    }
}

// The blocks between cuts in marker order, accumulated into intervals: an interval closes as soon as it holds at least
// ceil(M / S_max) markers, the remainder is the last one.  bounds[0] = 0 < ... < bounds[S] = M, S <= S_max (bounds has room for
// S_max + 1 entries); every interior bound is a cut.
inline void ss_partition(uint32_t M, const uint32_t* ahead, uint32_t S_max, uint32_t* bounds, uint32_t* S)
{
    const uint32_t quota = (uint32_t)(((uint64_t)M + S_max - 1u) / S_max);
    uint64_t reach = 0;
    uint32_t n = 0;
    bounds[0] = 0u;
    for (uint32_t j = 0; j < M; ++j) {
        if (j > 0 && reach < j && j - bounds[n] >= quota) bounds[++n] = j;
        const uint64_t hi = (uint64_t)j + ahead[j];
        if (hi > reach) reach = hi;
    }
    bounds[++n] = M;
    *S = n;
}

// The first marker whose window crosses the place before j (for a refusal's text); j is not a cut
inline uint32_t ss_crossing(uint32_t j, const uint32_t* ahead)
{
    for (uint32_t k = 0; k < j; ++k)
        if ((uint64_t)k + ahead[k] >= j) return k;
    return j;
}

// order grouped stably by interval: positions [bounds[s], bounds[s + 1]) of `grouped` hold the markers of interval s in the order
// the global shuffle gave them (interval s has exactly bounds[s + 1] - bounds[s] markers when order is a permutation).  O(M).
// Returns 0, or 1 + the first position of `order` that repeats a marker's interval beyond its size (order is no permutation).
inline uint32_t ss_group_order(uint32_t M, const int32_t* order, uint32_t S, const uint32_t* bounds, int32_t* grouped)
{
    std::vector<uint32_t> owner(M), fill(S);
    for (uint32_t s = 0; s < S; ++s) {
        fill[s] = bounds[s];
        for (uint32_t j = bounds[s]; j < bounds[s + 1]; ++j) owner[j] = s;
    }
    for (uint32_t p = 0; p < M; ++p) {
        const uint32_t s = owner[(uint32_t)order[p]];
        if (fill[s] >= bounds[s + 1]) return p + 1u;
        grouped[fill[s]++] = order[p];
    }
    return 0u;
}

// What both engines refuse about (S, bounds, rngs) beyond the single stream's checks: 0, or 1 with the text behind "<who>: " in buf
template <class Rng>
inline int ss_streams_check(uint32_t M, const uint32_t* ahead, const uint8_t* cut, uint32_t S, const uint32_t* bounds, const Rng* rngs, char* buf,
                            size_t len)
{
    buf[0] = 0;
    if (S < 1u || S > SS_SMAX) {
        snprintf(buf, len, "S = %u, must be in [1, %u]", S, SS_SMAX);
        return 1;
    }
    if (bounds[0] != 0u || bounds[S] != M) {
        snprintf(buf, len, "bounds must run from 0 to M = %u (bounds[0] = %u, bounds[%u] = %u)", M, bounds[0], S, bounds[S]);
        return 1;
    }
    for (uint32_t s = 0; s < S; ++s)
        if (bounds[s + 1] <= bounds[s] || bounds[s + 1] > M) {
            snprintf(buf, len, "bounds must be strictly ascending within [0, %u] (bounds[%u] = %u, bounds[%u] = %u)", M, s, bounds[s], s + 1u, bounds[s + 1]);
            return 1;
        }
    for (uint32_t s = 1; s < S; ++s)
        if (!cut[bounds[s]]) {
            const uint32_t k = ss_crossing(bounds[s], ahead);
            snprintf(buf, len, "bounds[%u] = %u is not a cut: the window of marker %u reaches marker %llu", s, bounds[s], k, (unsigned long long)k + ahead[k]);
            return 1;
        }
    for (uint32_t s = 0; s < S; ++s)
        if (rngs[s].idx > (uint32_t)MT_N) {
            snprintf(buf, len, "stream %u: rng idx %u > 624", s, rngs[s].idx);
            return 1;
        }
    return 0;
}

} // namespace hg
