// hydra_ss_chain.cpp -- hydra_chain.cpp's iteration for summary statistics: the same initial values and
// hyper-parameter draws, line for line, around hgibbs_ss_sweep instead of hgibbs_sweep.  What differs:
//
//   no residual  the state per marker is c_j = x_j'eps (on the device, or in this file's vectors for the host engine)
//   mu           norm_rng(0, sigmaE / n): the columns and y sum to zero, so the mean of the residual plus the old mu is 0
//   e_sqn        (y'y - sum_j beta_j (b_j + c_j)) + n mu^2, with y'y = n - 1, from hgibbs_ss_state's two sums; an e_sqn <= 0 (a
//                truncated band need not be positive definite) stops the iteration with an error and is never clamped
//   covariates   none
//
// One struct drives either engine: the device's (hydra_ss_chain_create) or the host's (hydra_ss_chain_create_host, no device at all),
// so the iteration that a CPU test holds to the oracle's chain is the one the device runs under.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hgibbs.h"
#include "hg_rng.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {
const double V0E = 0.0001, S02E = 0.0001, V0G = 0.0001, S02G = 0.0001; // src/BayesRRm.h:30-33

int cfail(const std::string& m)
{
    hgibbs_set_error_(m.c_str());
    return 1;
}
} // namespace

struct hydra_ss_chain {
    hgibbs_t dev = nullptr; // null: the host engine on the vectors below
    uint32_t M = 0, W = 0;
    double n = 0.0;
    int G = 1, K = 0;
    int shuffle = 1;
    std::vector<int32_t> groups, MtotGrp, order, cass, m0;
    std::vector<double> cVa, cVaI, priorPi, estPi, sigmaG;
    std::vector<uint8_t> adaV;
    double sigmaE = 0.0, mu = 0.0;
    hgibbs_rng_state rng{};
    uint64_t last_nnz = 0;
    uint32_t iteration = 0;
    // host engine
    std::vector<uint32_t> ahead;
    std::vector<double> band, xty, c, beta, acum;
    std::vector<int32_t> comp;
};

// the model tables, the seed and sigmaG ~ beta(1, 1), sigmaE, adaV: hydra_chain_create's, with y'y = n - 1
static int ss_init(hydra_ss_chain* c, const hydra_model_desc* model, const uint8_t* use)
{
    const uint32_t M = c->M;
    c->G = model->G;
    c->K = model->K;
    c->shuffle = model->shuffle;
    const int G = c->G, K = c->K, km1 = K - 1;
    if (G < 1) return cfail("hydra_ss_chain_create: G must be >= 1");
    if (K < 2) return cfail("hydra_ss_chain_create: K must be >= 2 (zero component + at least one mixture)");
    c->groups.assign(M, 0);
    if (model->groups) c->groups.assign(model->groups, model->groups + M);
    for (uint32_t i = 0; i < M; ++i)
        if (c->groups[i] < 0 || c->groups[i] >= G) return cfail("hydra_ss_chain_create: group index out of range");

    // :1086-1110
    c->cVa.assign((size_t)G * K, 0.0);
    c->cVaI.assign((size_t)G * K, 0.0);
    c->priorPi.assign((size_t)G * K, 0.0);
    for (int g = 0; g < G; ++g) {
        c->priorPi[g * K] = 0.5;
        double s = 0.0;
        for (int k = 1; k <= km1; ++k) {
            const double v = model->mS[g * K + k];
            if (!(v > 0.0)) return cfail("FATAL  : mixture value can only be strictly positive"); // :992-993
            c->cVa[g * K + k] = v;
            c->cVaI[g * K + k] = 1.0 / v;
            s += v;
        }
        for (int k = 1; k <= km1; ++k) c->priorPi[g * K + k] = c->priorPi[g * K] * c->cVa[g * K + k] / s;
    }
    c->estPi = c->priorPi;
    c->sigmaG.assign(G, 0.0);
    c->cass.assign((size_t)G * K, 0);
    c->m0.assign(G, 0);
    c->MtotGrp.assign(G, 0);
    for (uint32_t i = 0; i < M; ++i) c->MtotGrp[c->groups[i]] += 1;

    // :1228-1240
    hg::Mt gen{c->rng.x, 0};
    gen.seed(model->seed);
    for (int g = 0; g < G; ++g) c->sigmaG[g] = hg::beta_rng(gen, 1.0, 1.0);
    for (int g = 0; g < G; ++g)
        if (c->MtotGrp[g] == 0) c->sigmaG[g] = 0.0;
    c->rng.idx = gen.idx;

    c->order.resize(M);
    for (uint32_t i = 0; i < M; ++i) c->order[i] = (int32_t)i;
    c->sigmaE = (c->n - 1.0) / c->n * 0.5; // :1580 with y'y = n - 1

    // :1592-1597, and the markers the caller leaves out
    c->adaV.assign(M, 1);
    for (uint32_t i = 0; i < M; ++i)
        if (c->sigmaG[c->groups[i]] == 0.0 || (use && !use[i])) c->adaV[i] = 0;
    return 0;
}

extern "C" {

int hydra_ss_chain_create(hgibbs_t dev, const hydra_model_desc* model, double n_eff, uint32_t W, const uint32_t* ahead, const double* xty,
                          const uint8_t* use, hydra_ss_chain_t* out)
{
    if (!dev || !model || !xty || !out) return cfail("hydra_ss_chain_create: null argument");
    uint32_t n_global = 0, n_local = 0, M = 0, row_begin = 0;
    if (hgibbs_dims(dev, &n_global, &n_local, &M, &row_begin)) return 1;
    if (n_global < 2 || M == 0) return cfail("hydra_ss_chain_create: load the panel's genotypes first (hgibbs_load_bed / hgibbs_synth_bed)");
    hydra_ss_chain* c = new hydra_ss_chain();
    c->dev = dev;
    c->M = M;
    c->W = W;
    c->n = n_eff;
    // the band first: it refuses n_eff, W, ahead and xty by name
    if (hgibbs_ss_begin(dev, n_eff, W, ahead, xty) || ss_init(c, model, use) ||
        hgibbs_set_model(dev, c->G, c->K, c->groups.data(), c->cVa.data(), c->cVaI.data())) {
        (void)hgibbs_ss_end(dev);
        delete c;
        return 1;
    }
    *out = c;
    return 0;
}

int hydra_ss_chain_create_host(uint32_t M, const hydra_model_desc* model, double n_eff, uint32_t W, const uint32_t* ahead, const double* band,
                               const double* xty, const uint8_t* use, hydra_ss_chain_t* out)
{
    if (!model || !ahead || !band || !xty || !out) return cfail("hydra_ss_chain_create_host: null argument");
    if (M == 0) return cfail("hydra_ss_chain_create_host: no markers");
    if (W == 0 || W > 4096u) return cfail("hydra_ss_chain_create_host: W must be in [1, 4096]");
    if (!(std::isfinite(n_eff) && n_eff >= 2.0)) return cfail("hydra_ss_chain_create_host: n_eff must be a finite number >= 2");
    hydra_ss_chain* c = new hydra_ss_chain();
    c->M = M;
    c->W = W;
    c->n = n_eff;
    if (ss_init(c, model, use)) {
        delete c;
        return 1;
    }
    c->ahead.assign(ahead, ahead + M);
    c->band.assign(band, band + (size_t)M * W);
    c->xty.assign(xty, xty + M);
    c->c = c->xty;
    c->beta.assign(M, 0.0);
    c->acum.assign(M, 0.0);
    c->comp.assign(M, 0);
    *out = c;
    return 0;
}

int hydra_ss_chain_destroy(hydra_ss_chain_t c)
{
    if (c && c->dev) (void)hgibbs_ss_end(c->dev);
    delete c;
    return 0;
}

int hydra_ss_chain_iterate(hydra_ss_chain_t c)
{
    if (!c) return cfail("hydra_ss_chain_iterate: null chain");
    const int G = c->G, K = c->K;
    const uint32_t M = c->M;
    const double dN = c->n;
    hg::Mt gen{c->rng.x, c->rng.idx};

    // :1675-1686 with a residual whose mean plus the old mu is 0
    c->mu = hg::norm_rng(gen, 0.0, c->sigmaE / dN);

    // :1691-1694
    if (c->shuffle) hg::shuffle_libstdcxx6_fast(c->order.data(), c->order.size(), gen);
    std::fill(c->m0.begin(), c->m0.end(), 0);

    // :1709-2490; the generator travels with the call
    c->rng.idx = gen.idx;
    if (c->dev) {
        if (hgibbs_ss_sweep(c->dev, c->order.data(), c->sigmaE, c->sigmaG.data(), c->estPi.data(), c->adaV.data(), &c->rng, c->cass.data(), &c->last_nnz))
            return 1;
    } else if (hgibbs_ss_sweep_host(M, c->n, c->W, c->ahead.data(), c->band.data(), c->c.data(), c->beta.data(), c->comp.data(), c->acum.data(), G, K,
                                    c->groups.data(), c->cVa.data(), c->cVaI.data(), c->order.data(), c->sigmaE, c->sigmaG.data(), c->estPi.data(),
                                    c->adaV.data(), &c->rng, c->cass.data(), &c->last_nnz))
        return 1;
    gen.idx = c->rng.idx;

    // :2495-2578
    std::vector<double> bsq(G, 0.0);
    double sb = 0.0, sc = 0.0; // sum beta_j b_j, sum beta_j c_j in marker order over the non-zero effects (as hgibbs_ss_state)
    if (c->dev) {
        if (hgibbs_beta_sqnorm(c->dev, bsq.data())) return 1;
        if (hgibbs_ss_state(c->dev, nullptr, &sb, &sc)) return 1;
    } else
        for (uint32_t i = 0; i < M; ++i) {
            const double b = c->beta[i];
            if (b == 0.0) continue;
            bsq[c->groups[i]] += b * b;
            sb += b * c->xty[i];
            sc += b * c->c[i];
        }
    std::vector<double> dirin(K), pi(K);
    for (int g = 0; g < G; ++g) {
        if (c->MtotGrp[g] == 0) continue;
        c->m0[g] = c->MtotGrp[g] - c->cass[g * K];
        int rowsum = 0;
        for (int k = 0; k < K; ++k) rowsum += c->cass[g * K + k];
        if (c->m0[g] == 0 || rowsum == 0) {
            for (uint32_t i = 0; i < M; ++i)
                if (c->groups[i] == g) c->adaV[i] = 0;
            c->sigmaG[g] = 0.0;
            continue;
        }
        const double dm0 = (double)c->m0[g];
        c->sigmaG[g] = hg::inv_scaled_chisq_rng(gen, V0G + dm0, (bsq[g] * dm0 + V0G * S02G) / (V0G + dm0));
        for (int k = 0; k < K; ++k) dirin[k] = (double)c->cass[g * K + k] + 1.0;
        hg::dirichlet_rng(gen, dirin.data(), K, pi.data());
        for (int k = 0; k < K; ++k) c->estPi[g * K + k] = pi[k];
    }

    // :2685-2690
    const double e_sqn = ((dN - 1.0) - (sb + sc)) + dN * c->mu * c->mu;
    if (!(e_sqn > 0.0)) {
        char buf[256];
        std::snprintf(buf, sizeof buf,
                      "hydra_ss_chain_iterate: iteration %u: e_sqn = %.17g is not positive (the truncated band is not positive definite for these effects); not clamped",
                      c->iteration, e_sqn);
        c->rng.idx = gen.idx;
        return cfail(buf);
    }
    c->sigmaE = hg::inv_scaled_chisq_rng(gen, V0E + dN, (e_sqn + V0E * S02E) / (V0E + dN));
    c->rng.idx = gen.idx;
    c->iteration += 1;
    return 0;
}

int hydra_ss_chain_state(hydra_ss_chain_t c, double* sigmaE, double* mu, double* sigmaG, double* estPi, int32_t* m0, int32_t* cass, hgibbs_rng_state* rng)
{
    if (!c) return cfail("hydra_ss_chain_state: null chain");
    if (sigmaE) *sigmaE = c->sigmaE;
    if (mu) *mu = c->mu;
    if (sigmaG) std::copy(c->sigmaG.begin(), c->sigmaG.end(), sigmaG);
    if (estPi) std::copy(c->estPi.begin(), c->estPi.end(), estPi);
    if (m0) std::copy(c->m0.begin(), c->m0.end(), m0);
    if (cass) std::copy(c->cass.begin(), c->cass.end(), cass);
    if (rng) *rng = c->rng;
    return 0;
}

int hydra_ss_chain_effects(hydra_ss_chain_t c, double* beta, int32_t* components, double* acum, double* cvec)
{
    if (!c) return cfail("hydra_ss_chain_effects: null chain");
    if (c->dev) {
        if (hgibbs_get_beta(c->dev, beta, components, acum)) return 1;
        return cvec ? hgibbs_ss_state(c->dev, cvec, nullptr, nullptr) : 0;
    }
    if (beta) std::copy(c->beta.begin(), c->beta.end(), beta);
    if (components) std::copy(c->comp.begin(), c->comp.end(), components);
    if (acum) std::copy(c->acum.begin(), c->acum.end(), acum);
    if (cvec) std::copy(c->c.begin(), c->c.end(), cvec);
    return 0;
}

uint64_t hydra_ss_chain_last_nnz(hydra_ss_chain_t c) { return c ? c->last_nnz : 0; }

const int32_t* hydra_ss_chain_order(hydra_ss_chain_t c) { return c ? c->order.data() : nullptr; }

/* the chain's .csv line (src/BayesRRm.cpp:2742-2760) */
int hydra_ss_chain_csv_line(hydra_ss_chain_t c, uint32_t iteration, char* buf, size_t len)
{
    if (!c || !buf) return -1;
    const int G = c->G, K = c->K;
    size_t o = 0;
    o += snprintf(buf + o, len - o, "%5d, %4d", (int)iteration, G);
    double sg = 0.0;
    for (int g = 0; g < G; ++g) {
        o += snprintf(buf + o, len - o, ", %20.15f", c->sigmaG[g]);
        sg += c->sigmaG[g];
    }
    int m0sum = 0;
    for (int g = 0; g < G; ++g) m0sum += c->m0[g];
    o += snprintf(buf + o, len - o, ", %20.15f, %20.15f, %7d, %4d, %2d", c->sigmaE, sg / (c->sigmaE + sg), m0sum, G, K);
    for (int g = 0; g < G; ++g)
        for (int k = 0; k < K; ++k) o += snprintf(buf + o, len - o, ", %20.15f", c->estPi[g * K + k]);
    o += snprintf(buf + o, len - o, "\n");
    return (int)o;
}

} // extern "C"
