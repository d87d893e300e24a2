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
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hgibbs.h"
#include "hg_chain_core.h"

using hg::V0E, hg::S02E;

static int cfail(const std::string& m) { return hg::chain_fail(m); }

// HGIBBS_TIMING=1: where the host side of an iteration goes (stderr, milliseconds), as hydra_chain.cpp prints it
static bool ss_timing()
{
    static const bool timing = std::getenv("HGIBBS_TIMING") != nullptr;
    return timing;
}

static double ss_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static void ss_timing_line(const char* who, hgibbs_t dev, uint32_t chains, double t0, double t1, double t2, double t3, double t4)
{
    double band_ms = 0.0, sweep_ms = 0.0;
    if (dev) (void)hgibbs_last_ss_ms(dev, &band_ms, &sweep_ms);
    std::fprintf(stderr, "%s: %u chain(s): mu and shuffle %.3f, sweep call %.3f (kernel %.3f), sums %.3f, hyper-parameters %.3f, iteration %.3f ms\n", who, chains,
                 t1 - t0, t2 - t1, sweep_ms, t3 - t2, t4 - t3, t4 - t0);
}

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

// R chains on one band of the device: a core per chain, the replicas of the handle for their effects
struct hydra_ss_multi {
    hgibbs_t dev = nullptr;
    uint32_t M = 0, W = 0, S = 0; // S: the streams of every chain, 0 for the single stream
    double n = 0.0;
    std::vector<hg::ChainCore> chains;
    std::vector<uint32_t> ahead, bounds;
    std::vector<hgibbs_rng_state> streams; // R x S
    // what one iteration hands to the two launches and takes back, chain after chain
    std::vector<int32_t> orders, cass;
    std::vector<uint8_t> ada;
    std::vector<double> sigmaE, sigmaG, estPi, sb, sc, bsq;
    std::vector<uint64_t> nnz;
    std::vector<hgibbs_rng_state> rngs;
};

// the shared core's initial values, and sigmaE with y'y = n - 1
static int ss_init(hg::ChainCore& c, uint32_t M, double n, const hydra_model_desc* model, const uint8_t* use)
{
    if (model->G < 1) return cfail("hydra_ss_chain_create: G must be >= 1");
    if (model->K < 2) return cfail("hydra_ss_chain_create: K must be >= 2 (zero component + at least one mixture)");
    if (hg::core_init(c, M, model, use, "hydra_ss_chain_create")) return 1;
    c.sigmaE = (n - 1.0) / n * 0.5; // :1580 with y'y = n - 1
    return 0;
}

// hydra_ss_chain_set_streams' rule: stream s is seeded from w_s, the next S words of the chain's own generator
static void seed_streams(hgibbs_rng_state& rng, uint32_t S, hgibbs_rng_state* streams)
{
    hg::Mt gen{rng.x, rng.idx};
    std::vector<uint32_t> w(S);
    for (uint32_t s = 0; s < S; ++s) w[s] = gen.next();
    rng.idx = gen.idx;
    for (uint32_t s = 0; s < S; ++s) {
        hg::Mt st{streams[s].x, 0};
        st.seed(w[s]);
        streams[s].idx = st.idx;
    }
}

// the message of an e_sqn that is not positive; `chain`: its number among several, or -1
static std::string esqn_text(const char* who, uint32_t iteration, double e_sqn, int chain)
{
    char buf[320];
    int o = std::snprintf(buf, sizeof buf,
                          "%s: iteration %u: e_sqn = %.17g is not positive (the truncated band is not positive definite for these effects); not clamped", who,
                          iteration, e_sqn);
    if (chain >= 0) std::snprintf(buf + o, sizeof buf - o, " (chain %d)", chain);
    return buf;
}

// One chain's step around the sweep; the order in which it draws from its generator is the contract.  Before the sweep: mu, the shuffle, m0.
static void ss_before_sweep(hg::ChainCore& k, double dN)
{
    hg::Mt gen{k.rng.x, k.rng.idx};
    // :1675-1686 with a residual whose mean plus the old mu is 0
    k.mu = hg::norm_rng(gen, 0.0, k.sigmaE / dN);
    // :1691-1694
    if (k.shuffle) hg::shuffle_libstdcxx6_fast(k.order.data(), k.order.size(), gen);
    std::fill(k.m0.begin(), k.m0.end(), 0);
    k.rng.idx = gen.idx;
}

// After the sums (bsq per group; sb = sum beta_j b_j, sc = sum beta_j c_j): the hyper-parameters, e_sqn and sigmaE.  `chain`: esqn_text's.
static int ss_after_sums(hg::ChainCore& k, double dN, const double* bsq, double sb, double sc, const char* who, int chain)
{
    hg::Mt gen{k.rng.x, k.rng.idx};
    // :2495-2578
    hg::core_hyper(k, bsq, gen);
    // :2685-2690
    const double e_sqn = ((dN - 1.0) - (sb + sc)) + dN * k.mu * k.mu;
    k.rng.idx = gen.idx;
    if (!(e_sqn > 0.0)) return cfail(esqn_text(who, k.iteration, e_sqn, chain));
    k.sigmaE = hg::inv_scaled_chisq_rng(gen, V0E + dN, (e_sqn + V0E * S02E) / (V0E + dN));
    k.rng.idx = gen.idx;
    k.iteration += 1;
    return 0;
}

// What both device chains need before the band: the panel's M, and the window as hgibbs_ss_begin will hold it
static int ss_panel(hgibbs_t dev, const char* who, uint32_t W, const uint32_t* ahead, uint32_t& M, std::vector<uint32_t>& win)
{
    uint32_t n_global = 0, n_local = 0, row_begin = 0;
    if (hgibbs_dims(dev, &n_global, &n_local, &M, &row_begin)) return 1;
    if (n_global < 2 || M == 0) return cfail(std::string(who) + ": load the panel's genotypes first (hgibbs_load_bed / hgibbs_synth_bed)");
    win.resize(M);
    for (uint32_t j = 0; j < M; ++j) win[j] = ahead ? ahead[j] : std::min(W, M - 1u - j);
    return 0;
}

// Up to S_max intervals of independent blocks, then the S generators of each of the R chains from its own (streams: [R][S])
static int ss_make_streams(uint32_t M, const std::vector<uint32_t>& ahead, uint32_t S_max, hg::ChainCore* chains, uint32_t R, std::vector<uint32_t>& bounds,
                           std::vector<hgibbs_rng_state>& streams)
{
    std::vector<uint32_t> b((size_t)S_max + 1u);
    uint32_t S = 0;
    if (hgibbs_ss_partition(M, ahead.data(), S_max, b.data(), &S)) return 1;
    b.resize((size_t)S + 1u);
    bounds = b;
    streams.resize((size_t)R * S);
    for (uint32_t r = 0; r < R; ++r) seed_streams(chains[r].rng, S, streams.data() + (size_t)r * S);
    return 0;
}

extern "C" {

int hydra_ss_chain_create(hgibbs_t dev, const hydra_model_desc* model, double n_eff, uint32_t W, const uint32_t* ahead, const double* xty,
                          const uint8_t* use, hydra_ss_chain_t* out)
{
    if (!dev || !model || !xty || !out) return cfail("hydra_ss_chain_create: null argument");
    std::unique_ptr<hydra_ss_chain> c(new hydra_ss_chain());
    uint32_t M = 0;
    if (ss_panel(dev, "hydra_ss_chain_create", W, ahead, M, c->ahead)) return 1;
    c->dev = dev;
    c->M = M;
    c->W = W;
    c->n = n_eff;
    // the band first: it refuses n_eff, W, ahead and xty by name
    if (hgibbs_ss_begin(dev, n_eff, W, ahead, xty) || ss_init(*c, M, n_eff, model, use) ||
        hgibbs_set_model(dev, c->G, c->K, c->groups.data(), c->cVa.data(), c->cVaI.data())) {
        (void)hgibbs_ss_end(dev);
        return 1;
    }
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
    if (ss_init(*c, M, n_eff, model, use)) return 1;
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
    const bool timing = ss_timing();
    const double t0 = timing ? ss_now_ms() : 0.0;
    ss_before_sweep(*c, c->n);

    // :1709-2490; the generator travels with the call
    const double t1 = timing ? ss_now_ms() : 0.0;
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
    const double t2 = timing ? ss_now_ms() : 0.0;

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
    const double t3 = timing ? ss_now_ms() : 0.0;
    if (ss_after_sums(*c, c->n, bsq.data(), sb, sc, "hydra_ss_chain_iterate", -1)) return 1;
    if (timing) ss_timing_line("hydra_ss_chain_iterate", c->dev, 1u, t0, t1, t2, t3, ss_now_ms());
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
    return ss_make_streams(c->M, c->ahead, S_max, c, 1u, c->bounds, c->streams);
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

// ---- R chains on one band ----
// R cores around ONE hgibbs_ss_sweep_replicas and ONE hgibbs_ss_replica_sums per iteration.  Chain r draws what the hydra_ss_chain
// seeded with seeds[r] draws, in the same order from its own generator, so it is that chain bit for bit.

int hydra_ss_multi_create(hgibbs_t dev, const hydra_model_desc* model, uint32_t R, const uint32_t* seeds, double n_eff, uint32_t W, const uint32_t* ahead,
                          const double* xty, const uint8_t* use, uint32_t S_max, hydra_ss_multi_t* out)
{
    const char* who = "hydra_ss_multi_create";
    if (!dev || !model || !seeds || !xty || !out) return cfail(std::string(who) + ": null argument");
    if (R < 1u || R > 64u) return cfail(std::string(who) + ": R = " + std::to_string(R) + ", must be in [1, 64]");
    if (S_max > 1024u) return cfail(std::string(who) + ": S_max = " + std::to_string(S_max) + ", must be in [0, 1024] (0: the single stream)");
    std::unique_ptr<hydra_ss_multi> c(new hydra_ss_multi());
    uint32_t M = 0;
    if (ss_panel(dev, who, W, ahead, M, c->ahead)) return 1;
    c->dev = dev;
    c->M = M;
    c->W = W;
    c->n = n_eff;
    c->chains.resize(R);
    if (hgibbs_ss_begin(dev, n_eff, W, ahead, xty)) return 1;
    for (uint32_t r = 0; r < R; ++r) {
        hydra_model_desc md = *model;
        md.seed = seeds[r];
        if (ss_init(c->chains[r], M, n_eff, &md, use)) {
            (void)hgibbs_ss_end(dev);
            return 1;
        }
    }
    const hg::ChainCore& c0 = c->chains[0];
    if (hgibbs_set_model(dev, c0.G, c0.K, c0.groups.data(), c0.cVa.data(), c0.cVaI.data()) || hgibbs_ss_replicas(dev, R)) {
        (void)hgibbs_ss_end(dev);
        return 1;
    }
    if (S_max) {
        if (ss_make_streams(M, c->ahead, S_max, c->chains.data(), R, c->bounds, c->streams)) {
            (void)hgibbs_ss_end(dev);
            return 1;
        }
        c->S = (uint32_t)c->bounds.size() - 1u;
    }
    *out = c.release();
    return 0;
}

int hydra_ss_multi_destroy(hydra_ss_multi_t c)
{
    if (c && c->dev) (void)hgibbs_ss_end(c->dev);
    delete c;
    return 0;
}

int hydra_ss_multi_iterate(hydra_ss_multi_t c)
{
    if (!c) return cfail("hydra_ss_multi_iterate: null chains");
    const uint32_t M = c->M, R = (uint32_t)c->chains.size(), S = c->S;
    const int G = c->chains[0].G, K = c->chains[0].K;
    const size_t GK = (size_t)G * K;
    const double dN = c->n;
    c->orders.resize((size_t)R * M);
    c->ada.resize((size_t)R * M);
    c->sigmaE.resize(R);
    c->sigmaG.resize((size_t)R * G);
    c->estPi.resize(R * GK);
    c->cass.resize(R * GK);
    c->nnz.resize(R);
    c->rngs.resize(R);
    c->sb.resize(R);
    c->sc.resize(R);
    c->bsq.resize((size_t)R * G);

    // per chain: mu and the shuffle on its own generator
    const bool timing = ss_timing();
    const double t0 = timing ? ss_now_ms() : 0.0;
    for (uint32_t r = 0; r < R; ++r) {
        hg::ChainCore& k = c->chains[r];
        ss_before_sweep(k, dN);
        std::copy(k.order.begin(), k.order.end(), c->orders.begin() + (size_t)r * M);
        std::copy(k.adaV.begin(), k.adaV.end(), c->ada.begin() + (size_t)r * M);
        c->sigmaE[r] = k.sigmaE;
        std::copy(k.sigmaG.begin(), k.sigmaG.end(), c->sigmaG.begin() + (size_t)r * G);
        std::copy(k.estPi.begin(), k.estPi.end(), c->estPi.begin() + r * GK);
        c->rngs[r] = k.rng;
    }

    // one launch for every chain; with streams the chains' own generators are not touched by it
    const double t1 = timing ? ss_now_ms() : 0.0;
    if (hgibbs_ss_sweep_replicas(c->dev, R, c->orders.data(), c->sigmaE.data(), c->sigmaG.data(), c->estPi.data(), c->ada.data(), S ? S : 1u,
                                 S ? c->bounds.data() : nullptr, S ? c->streams.data() : c->rngs.data(), c->cass.data(), c->nnz.data()))
        return 1;
    const double t2 = timing ? ss_now_ms() : 0.0;
    if (hgibbs_ss_replica_sums(c->dev, c->sb.data(), c->sc.data(), c->bsq.data())) return 1;
    const double t3 = timing ? ss_now_ms() : 0.0;

    for (uint32_t r = 0; r < R; ++r) {
        hg::ChainCore& k = c->chains[r];
        if (!S) k.rng = c->rngs[r];
        std::copy(c->cass.begin() + r * GK, c->cass.begin() + (r + 1) * GK, k.cass.begin());
        k.last_nnz = c->nnz[r];
        if (ss_after_sums(k, dN, c->bsq.data() + (size_t)r * G, c->sb[r], c->sc[r], "hydra_ss_multi_iterate", (int)r)) return 1;
    }
    if (timing) ss_timing_line("hydra_ss_multi_iterate", c->dev, R, t0, t1, t2, t3, ss_now_ms());
    return 0;
}

static hg::ChainCore* multi_at(hydra_ss_multi_t c, uint32_t r, const char* who)
{
    if (!c) {
        cfail(std::string(who) + ": null chains");
        return nullptr;
    }
    if (r >= c->chains.size()) {
        cfail(std::string(who) + ": chain " + std::to_string(r) + " outside [0, " + std::to_string(c->chains.size()) + ")");
        return nullptr;
    }
    return &c->chains[r];
}

int hydra_ss_multi_state(hydra_ss_multi_t c, uint32_t r, double* sigmaE, double* mu, double* sigmaG, double* estPi, int32_t* m0, int32_t* cass,
                         hgibbs_rng_state* rng)
{
    const hg::ChainCore* k = multi_at(c, r, "hydra_ss_multi_state");
    if (!k) return 1;
    hg::core_state(*k, sigmaE, mu, sigmaG, estPi, m0, cass, rng);
    return 0;
}

int hydra_ss_multi_effects(hydra_ss_multi_t c, uint32_t r, double* beta, int32_t* components, double* acum, double* cvec)
{
    if (!multi_at(c, r, "hydra_ss_multi_effects")) return 1;
    return hgibbs_ss_replica_get(c->dev, r, beta, components, acum, cvec);
}

int hydra_ss_multi_streams(hydra_ss_multi_t c, uint32_t* S, uint32_t* bounds, hgibbs_rng_state* rngs)
{
    if (!c) return cfail("hydra_ss_multi_streams: null chains");
    if (S) *S = c->S;
    if (bounds) std::copy(c->bounds.begin(), c->bounds.end(), bounds);
    if (rngs) std::copy(c->streams.begin(), c->streams.end(), rngs);
    return 0;
}

uint64_t hydra_ss_multi_last_nnz(hydra_ss_multi_t c, uint32_t r) { return (c && r < c->chains.size()) ? c->chains[r].last_nnz : 0; }

int hydra_ss_multi_csv_line(hydra_ss_multi_t c, uint32_t r, uint32_t iteration, char* buf, size_t len)
{
    return (c && buf && r < c->chains.size()) ? hg::core_csv_line(c->chains[r], iteration, buf, len) : -1;
}

} // extern "C"
