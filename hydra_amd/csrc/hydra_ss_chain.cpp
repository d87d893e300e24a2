// hydra_ss_chain.cpp -- hydra_chain.cpp's iteration for summary statistics: the same initial values and
// hyper-parameter draws (hg_chain_core.h) around hgibbs_ss_sweep instead of hgibbs_sweep.  What differs:
//
//   no residual  the state per marker is c_j = x_j'eps (on the device, or in this file's vectors for the host engine)
//   mu           norm_rng(0, sigmaE / n): the columns and y sum to zero, so the mean of the residual plus the old mu is 0
//   e_sqn        (y'y - sum_j beta_j (b_j + c_j)) + n mu^2, with y'y = n - 1, from hgibbs_ss_state's two sums; an e_sqn <= 0 (a
//                truncated band need not be positive definite) stops the iteration with an error and is never clamped
//   covariates   none
//   streams      hydra_ss_chain_set_streams: the sweep runs the band's independent blocks from generators of
//                their own, seeded from this chain's; mu, the shuffle and the hyper-parameters stay on the chain's generator
//
// One struct drives either engine: the device's (hydra_ss_chain_create) or the host's (hydra_ss_chain_create_host, no device at all),
// so the iteration that a CPU test holds to the oracle's chain is the one the device runs under.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hgibbs.h"
#include "hg_chain_core.h"

using hg::V0E, hg::S02E;

static int cfail(const std::string& m) { return hg::chain_fail(m); }

struct hydra_ss_chain : hg::ChainCore {
    hgibbs_t dev = nullptr; // null: the host engine on the vectors below
    uint32_t M = 0, W = 0;
    double n = 0.0;
    std::vector<uint32_t> ahead; // the window as the engine holds it
    // host engine
    std::vector<double> band, xty, c, beta, acum;
    std::vector<int32_t> comp;
    // independent blocks in parallel streams; none: the single stream
    std::vector<uint32_t> bounds;
    std::vector<hgibbs_rng_state> streams;
};

// the shared core's initial values, and sigmaE with y'y = n - 1
static int ss_init(hydra_ss_chain* c, const hydra_model_desc* model, const uint8_t* use)
{
    if (model->G < 1) return cfail("hydra_ss_chain_create: G must be >= 1");
    if (model->K < 2) return cfail("hydra_ss_chain_create: K must be >= 2 (zero component + at least one mixture)");
    if (hg::core_init(*c, c->M, model, use, "hydra_ss_chain_create")) return 1;
    c->sigmaE = (c->n - 1.0) / c->n * 0.5; // :1580 with y'y = n - 1
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
    std::unique_ptr<hydra_ss_chain> c(new hydra_ss_chain());
    c->dev = dev;
    c->M = M;
    c->W = W;
    c->n = n_eff;
    // the band first: it refuses n_eff, W, ahead and xty by name
    if (hgibbs_ss_begin(dev, n_eff, W, ahead, xty) || ss_init(c.get(), model, use) ||
        hgibbs_set_model(dev, c->G, c->K, c->groups.data(), c->cVa.data(), c->cVaI.data())) {
        (void)hgibbs_ss_end(dev);
        return 1;
    }
    c->ahead.resize(M);
    for (uint32_t j = 0; j < M; ++j) c->ahead[j] = ahead ? ahead[j] : std::min(W, M - 1u - j);
    *out = c.release();
    return 0;
}

int hydra_ss_chain_create_host(uint32_t M, const hydra_model_desc* model, double n_eff, uint32_t W, const uint32_t* ahead, const double* band,
                               const double* xty, const uint8_t* use, hydra_ss_chain_t* out)
{
    if (!model || !ahead || !band || !xty || !out) return cfail("hydra_ss_chain_create_host: null argument");
    if (M == 0) return cfail("hydra_ss_chain_create_host: no markers");
    if (W == 0 || W > 4096u) return cfail("hydra_ss_chain_create_host: W must be in [1, 4096]");
    if (!(std::isfinite(n_eff) && n_eff >= 2.0)) return cfail("hydra_ss_chain_create_host: n_eff must be a finite number >= 2");
    std::unique_ptr<hydra_ss_chain> c(new hydra_ss_chain());
    c->M = M;
    c->W = W;
    c->n = n_eff;
    if (ss_init(c.get(), model, use)) return 1;
    c->ahead.assign(ahead, ahead + M);
    c->band.assign(band, band + (size_t)M * W);
    c->xty.assign(xty, xty + M);
    c->c = c->xty;
    c->beta.assign(M, 0.0);
    c->acum.assign(M, 0.0);
    c->comp.assign(M, 0);
    *out = c.release();
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
    const uint32_t S = (uint32_t)c->streams.size();
    if (S) { // the main generator is not touched by the sweep
        if (c->dev ? hgibbs_ss_sweep_streams(c->dev, c->order.data(), c->sigmaE, c->sigmaG.data(), c->estPi.data(), c->adaV.data(), S, c->bounds.data(),
                                             c->streams.data(), c->cass.data(), &c->last_nnz)
                   : hgibbs_ss_sweep_streams_host(M, c->n, c->W, c->ahead.data(), c->band.data(), c->c.data(), c->beta.data(), c->comp.data(),
                                                  c->acum.data(), G, K, c->groups.data(), c->cVa.data(), c->cVaI.data(), c->order.data(), c->sigmaE,
                                                  c->sigmaG.data(), c->estPi.data(), c->adaV.data(), S, c->bounds.data(), c->streams.data(),
                                                  c->cass.data(), &c->last_nnz))
            return 1;
    } else if (c->dev) {
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
    hg::core_hyper(*c, bsq.data(), gen);

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
    hg::core_state(*c, sigmaE, mu, sigmaG, estPi, m0, cass, rng);
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

int hydra_ss_chain_set_streams(hydra_ss_chain_t c, uint32_t S_max)
{
    const char* who = "hydra_ss_chain_set_streams";
    if (!c) return cfail(std::string(who) + ": null chain");
    if (c->iteration > 0) return cfail(std::string(who) + ": the chain has run " + std::to_string(c->iteration) + " iteration(s): streams are set before the first");
    if (!c->streams.empty()) return cfail(std::string(who) + ": streams are already set");
    if (S_max < 1u || S_max > 1024u) return cfail(std::string(who) + ": S_max = " + std::to_string(S_max) + ", must be in [1, 1024]");
    std::vector<uint32_t> bounds((size_t)S_max + 1u);
    uint32_t S = 0;
    if (hgibbs_ss_partition(c->M, c->ahead.data(), S_max, bounds.data(), &S)) return 1;
    bounds.resize((size_t)S + 1u);
    hg::Mt gen{c->rng.x, c->rng.idx};
    std::vector<uint32_t> w(S);
    for (uint32_t s = 0; s < S; ++s) w[s] = gen.next();
    c->rng.idx = gen.idx;
    c->streams.resize(S);
    for (uint32_t s = 0; s < S; ++s) {
        hg::Mt st{c->streams[s].x, 0};
        st.seed(w[s]);
        c->streams[s].idx = st.idx;
    }
    c->bounds = bounds;
    return 0;
}

int hydra_ss_chain_streams(hydra_ss_chain_t c, uint32_t* S, uint32_t* bounds, hgibbs_rng_state* rngs)
{
    if (!c) return cfail("hydra_ss_chain_streams: null chain");
    if (S) *S = (uint32_t)c->streams.size();
    if (bounds) std::copy(c->bounds.begin(), c->bounds.end(), bounds);
    if (rngs) std::copy(c->streams.begin(), c->streams.end(), rngs);
    return 0;
}

uint64_t hydra_ss_chain_last_nnz(hydra_ss_chain_t c) { return c ? c->last_nnz : 0; }

const int32_t* hydra_ss_chain_order(hydra_ss_chain_t c) { return c ? c->order.data() : nullptr; }

int hydra_ss_chain_csv_line(hydra_ss_chain_t c, uint32_t iteration, char* buf, size_t len)
{
    return (c && buf) ? hg::core_csv_line(*c, iteration, buf, len) : -1;
}

} // extern "C"
