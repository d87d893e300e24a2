// BayesR from summary statistics and the panel's LD band: the Gibbs step of the chain with c_j = x_j'eps kept
// per marker instead of the residual per individual.  Inputs: n_eff, b = X'y, and the band B_jk = (n_eff - 1) r_jk of the loaded panel.
//
//   band      the band frame of hg_ld.hip.h (ld_band_pieces): k_ld<MISS>, unchanged, fills the 64-bit sums of a piece of band rows;
//             k_ss_band replaces k_ld_final: r of ld_pair_r times (n_eff - 1), 0 outside ahead[j] and where r is NaN.  M x W doubles,
//             row j = the markers j + 1 .. j + W; only this `ahead` half is kept.  Nothing of it leaves the device.
//   sweep     k_ss_sweep: ONE launch per sweep, ONE workgroup, because the chain is sequential through c and through the generator.
//             decision  every lane runs the step of hg_ss_step.h on the same numbers (uniform): no broadcast, and a marker whose
//                       effect stays where it was costs no barrier at all.  The generator's block lies in LDS; a block that runs out
//                       is followed by the next one made by the whole workgroup (the three segments of the recurrence).
//             update    delta != 0: barrier (every wave has read its c_j), c_k += delta B_jk over the lanes -- j's own row forwards
//                       (coalesced), the rows of the markers behind at offset j - k (one load each) --, barrier.
//             ahead     the next marker's c, effect, group and window are loaded before the decision of this one; c is loaded again
//                       after an update, since the next marker may lie inside the window just updated.
//             memory    c is read and written with ordinary vector loads and stores; what orders them is the workgroup barrier.
//   streams   k_ss_sweep_streams: the same marker loop (ss_sweep_body), one workgroup per interval of independent
//             LD blocks, each with a generator of its own.  A workgroup touches c, beta, acum and comp at its own interval only (a cut
//             is where no window crosses), so the barriers above are all the ordering there is; cass is counted with integer atomics.
//   sums      k_ss_sums: sum beta_j b_j and sum beta_j c_j in marker order by one wave, the non-zero effects only (a zero effect adds
//             +-0 to a sum that is never -0): a fixed order, so the bits repeat.
#pragma once

#include <cstddef>

#include "hg_ss_step.h"

struct SsResult {
    unsigned long long nnz;
    uint32_t rng_idx, err; // err: 0, or 1 + the sweep position whose component walk found no component
    double sums[2];
};

// The summary-statistics side of the handle, between hgibbs_ss_begin and hgibbs_ss_end
struct SsState {
    double n_eff = 0.0;
    uint32_t W = 0, M = 0;
    DevBuf<double> band, c, xty;
    DevBuf<uint32_t> ahead, back;
    DevBuf<int32_t> order;
    DevBuf<uint8_t> ada;
    DevBuf<SsResult> res;
    // What a sweep of C chains in S intervals each stages (ss_sweep_run, the three entry points alike): C S generator states (625 words
    // each) and results, chain after chain, and S + 1 bounds; the grouped orders and masks of the C chains.  Sized at the largest C S so far.
    DevBuf<uint32_t> mts, bounds;
    DevBuf<SsResult> sres;
    uint32_t stage_cap = 0;
    std::vector<int32_t> grouped;
    std::vector<uint8_t> ada_host;
    std::vector<SsResult> sres_host;
    // hgibbs_ss_replicas: R chains on the one band.  Replica r's c, effects, components, acum, order and mask lie at
    // r M of the R x M arrays, its tables at r 4 G K, its counters at r G K.
    uint32_t R = 0, rep_gk = 0, rep_g = 0; // replicas; the G K the tables and counters are sized for; the G the group sums are
    DevBuf<double> rc, rbeta, racum, rtables, ri2s, rbsq;
    DevBuf<int32_t> rcomp, rorder, rcass;
    DevBuf<uint8_t> rada;
    DevBuf<SsResult> rsums;
    std::vector<uint32_t> ahead_host;
    std::vector<uint8_t> cut;    // per marker: no window crosses the place before it
    std::vector<uint8_t> ok;     // per marker: its standard deviation is finite
    double band_ms = 0.0, sweep_ms = 0.0;
    // hgibbs_ss_post_* (hg_sspost.hip.h): the per-marker accumulators over post_T records of post_R replicas (0: the
    // handle's own chain) -- the pooled pair, the pairs of the [chains][2] half-chains, cnt [K][M], the error word, the table's four columns
    bool post_open = false, post_final = false;
    uint32_t post_R = 0, post_T = 0, post_t = 0, post_K = 0;
    DevBuf<double> pmean, pm2, phmean, phm2, pout;
    DevBuf<uint32_t> pcnt;
    DevBuf<unsigned long long> pflag;
    double post_add_ms = 0.0, post_final_ms = 0.0;
};

namespace {

constexpr int SS_TPB = 256;
constexpr size_t SS_RNG_WORDS = sizeof(hgibbs_rng_state) / sizeof(uint32_t);
static_assert(SS_RNG_WORDS == (size_t)MT_N + 1 && offsetof(hgibbs_rng_state, idx) == MT_N * sizeof(uint32_t), "a state is its 624 words, then its index");
static_assert(SS_MAX_K == MAX_K, "the step's component arrays hold what hgibbs_set_model takes");

// Thread per pair of the piece's band rows: band[j W + o] = scale r(j, j + o + 1), 0 outside j's window and where r is NaN
__global__ __launch_bounds__(LD_TPB) void k_ss_band(const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ counts,
                                                    const double* __restrict__ mave, const double* __restrict__ mstd, const uint32_t* __restrict__ ahead,
                                                    uint32_t n_local, uint32_t N, uint32_t W, uint32_t p0, uint32_t pc, double scale,
                                                    double* __restrict__ band)
{
    const uint64_t k = (uint64_t)blockIdx.x * LD_TPB + threadIdx.x;
    if (k >= (uint64_t)pc * W) return;
    const uint32_t j = p0 + (uint32_t)(k / W), o = (uint32_t)(k % W);
    double v = 0.0;
    if (o < ahead[j]) { // q = j + o + 1 <= j + ahead[j] < M
        long long G, Bjq, Bqj, Dc;
        const double r = ld_pair_r(acc + 4 * k, counts, mave, mstd, j, j + o + 1u, n_local, N, G, Bjq, Bqj, Dc);
        if (r == r) v = scale * r;
    }
    band[(uint64_t)j * W + o] = v;
}

// The generator of the sweep's workgroup: two blocks of untempered words in LDS, the current one at `base`.  Every thread holds the
// same idx and calls next() at the same places, so the barriers of a refill are met by all.
struct SsGen {
    uint32_t* mt;
    uint32_t base, idx;
    __device__ __forceinline__ void refill()
    {
        const uint32_t* cur = mt + base;
        uint32_t* nxt = mt + (MT_N - base);
        const int tid = (int)threadIdx.x;
        for (int i = tid; i < 227; i += SS_TPB) nxt[i] = mt_mix(cur[i], cur[i + 1], cur[i + MT_M]);
        __syncthreads();
        for (int i = 227 + tid; i < 454; i += SS_TPB) nxt[i] = mt_mix(cur[i], cur[i + 1], nxt[i - 227]);
        __syncthreads();
        for (int i = 454 + tid; i < 623; i += SS_TPB) nxt[i] = mt_mix(cur[i], cur[i + 1], nxt[i - 227]);
        __syncthreads();
        if (tid == 0) nxt[623] = mt_mix(cur[623], nxt[0], nxt[396]);
        __syncthreads();
        base = MT_N - base;
        idx = 0;
    }
    __device__ __forceinline__ uint32_t next()
    {
        if (idx >= (uint32_t)MT_N) refill();
        return mt_temper(mt[base + idx++]);
    }
};

struct SsSweepParams {
    const int32_t* order;
    const int32_t* groups;
    const uint8_t* ada;
    const uint32_t* ahead;
    const uint32_t* back;
    const double* band;
    double* c;
    double* beta;
    int32_t* comp;
    double* acum;
    const double* tables; // denom, logpi, hlog, sdk: G K each
    uint32_t* mt;         // 624 words, in and out (per interval: S x 624)
    ZigTables zig;
    int32_t* cass;
    SsResult* res;
    uint32_t M, W, rng_idx;
    int K, GK;
    double dNm1, i_2sigE;
    const uint32_t* bounds; // k_ss_sweep_streams: S + 1 positions of the grouped order (last: k_ss_sweep's arguments lie where they lay)
};

// The marker loop of both sweep kernels: the positions [p0, p1) of p.order with the generator whose 624 words lie at `mt` (in and
// out) and whose index is rng_idx; the outcome goes to *res.  SHARED: other workgroups count into p.cass at the same time (an integer
// atomicAdd, exact in any order); everything else the loop loads or stores lies at the markers of its own positions and their windows.
template <bool SHARED>
__device__ __forceinline__ void ss_sweep_body(const SsSweepParams& p, uint32_t p0, uint32_t p1, uint32_t* __restrict__ mt, uint32_t rng_idx,
                                              SsResult* __restrict__ res)
{
    __shared__ uint32_t s_mt[2 * MT_N];
    __shared__ double s_nx[129], s_ny[129];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < (uint32_t)MT_N; i += SS_TPB) s_mt[i] = mt[i];
    for (uint32_t i = tid; i < 129u; i += SS_TPB) {
        s_nx[i] = p.zig.nx[i];
        s_ny[i] = p.zig.ny[i];
    }
    __syncthreads();
    SsGen gen{s_mt, 0u, rng_idx};
    const ZigTables zt{s_nx, s_ny, p.zig.ex, p.zig.ey};
    const uint32_t W = p.W;
    const int K = p.K;
    const double* denom = p.tables;
    const double* logpi = denom + p.GK;
    const double* hlog = logpi + p.GK;
    const double* sdk = hlog + p.GK;
    double* const c = p.c;

    unsigned long long nnz = 0;
    uint32_t err = 0;
    // the marker of this position (values loaded), the next one (index loaded)
    uint32_t j = (uint32_t)p.order[p0];
    double cj = c[j], bold = p.beta[j];
    int g = p.groups[j];
    uint32_t ada = p.ada[j], ah = p.ahead[j], bk = p.back[j];
    uint32_t jn = p0 + 1u < p1 ? (uint32_t)p.order[p0 + 1u] : 0u;

    for (uint32_t pos = p0; pos < p1; ++pos) {
        // ahead: the next marker's values, the index of the one after it
        const bool more = pos + 1u < p1;
        double cn = 0.0, bn = 0.0;
        int gn = 0;
        uint32_t adan = 0, ahn = 0, bkn = 0, jnn = 0;
        if (more) {
            cn = c[jn];
            bn = p.beta[jn];
            gn = p.groups[jn];
            adan = p.ada[jn];
            ahn = p.ahead[jn];
            bkn = p.back[jn];
            if (pos + 2u < p1) jnn = (uint32_t)p.order[pos + 2u];
        }

        double bnew = 0.0, ac = 1.0;
        if (ada) {
            int k = 0;
            const int o = g * K;
            if (ss_marker_draw(cj + bold * p.dNm1, K, denom + o, logpi + o, hlog + o, sdk + o, p.i_2sigE, gen, zt, bnew, k, ac)) {
                err = pos + 1u;
                break; // (uniform)
            }
            if (tid == 0) {
                if (SHARED)
                    atomicAdd(p.cass + (o + k), 1);
                else
                    p.cass[o + k] += 1;
                p.comp[j] = k;
            }
        }
        if (tid == 0) {
            p.beta[j] = bnew;
            p.acum[j] = ac;
        }
        const double delta = bold - bnew;
        if (delta != 0.0) { // (uniform)
            __syncthreads(); // every wave has read c_j and what it loaded ahead
            const double* row = p.band + (uint64_t)j * W;
            const uint32_t far = ah > bk ? ah : bk;
            for (uint32_t d = tid + 1u; d <= far; d += SS_TPB) {
                if (d <= ah) c[j + d] += delta * row[d - 1u];
                if (d <= bk) {
                    const uint32_t k = j - d;
                    if (p.ahead[k] >= d) c[k] += delta * p.band[(uint64_t)k * W + (d - 1u)];
                }
            }
            if (tid == 0) c[j] += delta * p.dNm1;
            ++nnz;
            __syncthreads(); // the window's c is written
            if (more) cn = c[jn]; // (it may lie in that window)
        }
        j = jn;
        cj = cn;
        bold = bn;
        g = gn;
        ada = adan;
        ah = ahn;
        bk = bkn;
        jn = jnn;
    }

    __syncthreads();
    for (uint32_t i = tid; i < (uint32_t)MT_N; i += SS_TPB) mt[i] = s_mt[gen.base + i];
    if (tid == 0) {
        res->nnz = nnz;
        res->rng_idx = gen.idx;
        res->err = err;
    }
}

__global__ __launch_bounds__(SS_TPB) void k_ss_sweep(const SsSweepParams p)
{
    ss_sweep_body<false>(p, 0u, p.M, p.mt, p.rng_idx, p.res);
}

// One workgroup per interval of independent blocks: positions [bounds[s], bounds[s + 1]) of the grouped order,
// the generator at p.mt + 625 s as the caller's hgibbs_rng_state holds it (624 words, then the index; the new index goes to res[s]).
// No workgroup waits for another.
__global__ __launch_bounds__(SS_TPB) void k_ss_sweep_streams(const SsSweepParams p)
{
    const uint32_t s = blockIdx.x;
    uint32_t* mt = p.mt + (size_t)s * SS_RNG_WORDS;
    ss_sweep_body<true>(p, p.bounds[s], p.bounds[s + 1u], mt, mt[MT_N], p.res + s);
}

// What k_ss_sweep_replicas is given beside SsSweepParams (a struct of its own: the two kernels above keep their arguments where they
// lay).  In its SsSweepParams every per-chain pointer is replica 0's; replica r's lie r M (order, ada, c, beta, comp, acum), r 4 GK
// (tables), r GK (cass) and r S (mt, res) further on.
struct SsReplicaParams {
    const double* i_2sigE; // R: 1 / (2 sigmaE) of each replica
};

// R chains on one band: the grid is S x R, workgroup (s, r) runs interval s of replica r.  The replica's
// pointers are derived once, in uniform arithmetic; the marker loop is the one of the two kernels above.  The workgroups of one
// replica count into that replica's cass; those of different replicas share nothing that is written.
__global__ __launch_bounds__(SS_TPB) void k_ss_sweep_replicas(const SsSweepParams p0, const SsReplicaParams q)
{
    const uint32_t s = blockIdx.x, r = blockIdx.y, S = gridDim.x;
    SsSweepParams p = p0;
    const size_t rM = (size_t)r * p.M, rGK = (size_t)r * (size_t)p.GK;
    p.order += rM;
    p.ada += rM;
    p.c += rM;
    p.beta += rM;
    p.comp += rM;
    p.acum += rM;
    p.tables += 4u * rGK;
    p.cass += rGK;
    p.i_2sigE = q.i_2sigE[r];
    const size_t rs = (size_t)r * S + s;
    uint32_t* mt = p.mt + rs * SS_RNG_WORDS;
    ss_sweep_body<true>(p, p.bounds[s], p.bounds[s + 1u], mt, mt[MT_N], p.res + rs);
}

// One wave per replica: k_ss_sums' two sums, and per group the sum of beta^2 in marker order (hgibbs_beta_sqnorm's order), over the
// non-zero effects.  The group sums are kept in LDS (G doubles, the launch's dynamic share) by lane 0, one add after the other.
__global__ __launch_bounds__(64) void k_ss_replica_sums(const double* __restrict__ beta, const double* __restrict__ xty, const double* __restrict__ c,
                                                        const int32_t* __restrict__ groups, uint32_t M, uint32_t G, SsResult* __restrict__ res,
                                                        double* __restrict__ bsq)
{
    extern __shared__ double s_bsq[];
    const uint32_t lane = threadIdx.x, r = blockIdx.x;
    beta += (size_t)r * M;
    c += (size_t)r * M;
    for (uint32_t g = lane; g < G; g += 64u) s_bsq[g] = 0.0;
    __syncthreads();
    double sb = 0.0, sc = 0.0;
    for (uint32_t base = 0; base < M; base += 64u) {
        const uint32_t i = base + lane;
        const double b = i < M ? beta[i] : 0.0;
        double pb = 0.0, pc = 0.0, sq = 0.0;
        int g = 0;
        if (b != 0.0) {
            pb = b * xty[i];
            pc = b * c[i];
            sq = b * b;
            g = groups[i];
        }
        for (unsigned long long m = __ballot(b != 0.0); m; m &= m - 1ull) { // (uniform)
            const int l = (int)__builtin_ctzll(m);
            sb += __shfl(pb, l);
            sc += __shfl(pc, l);
            const double v = __shfl(sq, l);
            const int gl = __shfl(g, l);
            if (lane == 0) s_bsq[gl] += v;
        }
    }
    __syncthreads();
    for (uint32_t g = lane; g < G; g += 64u) bsq[(size_t)r * G + g] = s_bsq[g];
    if (lane == 0) {
        res[r].sums[0] = sb;
        res[r].sums[1] = sc;
    }
}

// One wave: the two sums in marker order over the non-zero effects
__global__ __launch_bounds__(64) void k_ss_sums(const double* __restrict__ beta, const double* __restrict__ xty, const double* __restrict__ c, uint32_t M,
                                                SsResult* __restrict__ res)
{
    const uint32_t lane = threadIdx.x;
    double sb = 0.0, sc = 0.0;
    for (uint32_t base = 0; base < M; base += 64u) {
        const uint32_t i = base + lane;
        const double b = i < M ? beta[i] : 0.0;
        double pb = 0.0, pc = 0.0;
        if (b != 0.0) {
            pb = b * xty[i];
            pc = b * c[i];
        }
        for (unsigned long long m = __ballot(b != 0.0); m; m &= m - 1ull) { // (uniform)
            const int l = (int)__builtin_ctzll(m);
            sb += __shfl(pb, l);
            sc += __shfl(pc, l);
        }
    }
    if (lane == 0) {
        res->sums[0] = sb;
        res->sums[1] = sc;
    }
}

SsState* ss_of(hgibbs_ctx* h, const char* who)
{
    if (!h) {
        fail("%s: null handle", who);
        return nullptr;
    }
    if (!h->ss) {
        fail("%s: no summary-statistics state on this handle (hgibbs_ss_begin first)", who);
        return nullptr;
    }
    if (!h->bed || h->ss->M != h->M) {
        fail("%s: the genotypes were replaced after hgibbs_ss_begin", who);
        return nullptr;
    }
    return h->ss.get();
}

} // namespace

extern "C" int hgibbs_ss_begin(hgibbs_t h, double n_eff, uint32_t W, const uint32_t* ahead, const double* xty)
{
    const char* who = "hgibbs_ss_begin";
    if (ld_band_check(h, who, W, nullptr)) return 1;
    if (!(std::isfinite(n_eff) && n_eff >= 2.0)) return fail("%s: n_eff = %g, must be a finite number >= 2", who, n_eff);
    if (!xty) return fail("%s: null xty", who);
    const uint32_t M = h->M;
    for (uint32_t j = 0; j < M; ++j)
        if (!std::isfinite(xty[j])) return fail("%s: xty[%u] is not finite", who, j);
    std::vector<uint32_t> ah;
    if (ld_ahead(who, M, W, ahead, ah)) return 1;
    std::vector<uint32_t> back(M);
    ss_back(M, ah.data(), back.data());
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;

    const uint32_t piece = ld_piece_rows(W, 0, M);
    const size_t nb = (size_t)M * W, np = (size_t)piece * W;
    if (need_device_memory(nb * 8 + np * 32 + (size_t)M * 32 + ld_flag_count(M),
                           "%s: the band of %u x %u doubles (%.1f MiB) and the sums of a piece of %u band rows (%.1f MiB)", who, M, W, nb * 8 / 1048576.0,
                           piece, np * 32 / 1048576.0))
        return 1;
    std::unique_ptr<SsState> s(new SsState());
    s->n_eff = n_eff;
    s->W = W;
    s->M = M;
    if (s->band.alloc(nb) || s->c.alloc(M) || s->xty.alloc(M) || s->ahead.alloc(M) || s->back.alloc(M) || s->order.alloc(M) || s->ada.alloc(M) ||
        s->res.alloc(1))
        return 1;
    std::vector<double> mstd(M);
    HIP_TRY(hipMemcpy(mstd.data(), h->mstd, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
    s->ok.resize(M);
    for (uint32_t j = 0; j < M; ++j) s->ok[j] = std::isfinite(mstd[j]) ? 1 : 0;
    s->cut.resize(M);
    ss_cuts(M, ah.data(), s->cut.data());
    s->ahead_host = ah;
    HIP_TRY(hipMemcpy(s->ahead, ah.data(), (size_t)M * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->back, back.data(), (size_t)M * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->xty, xty, (size_t)M * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->c, xty, (size_t)M * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(s->res, 0, sizeof(SsResult)));

    LdBand band;
    if (ld_band_open(h, W, piece, band)) return 1;
    double ms = 0.0;
    const double scale = n_eff - 1.0;
    SsState* sp = s.get();
    // the step of a piece: its band rows inside the products' lap
    auto fill = [&](uint32_t p0, uint32_t pc, const unsigned long long* acc) -> int {
        const uint64_t npc = (uint64_t)pc * W;
        k_ss_band<<<(uint32_t)((npc + LD_TPB - 1) / LD_TPB), LD_TPB, 0, h->stream>>>(acc, h->counts, h->mave, h->mstd, sp->ahead, h->n_local, h->n_global, W, p0,
                                                                                      pc, scale, sp->band);
        HIP_TRY(hipGetLastError());
        return lap_end(h, ms);
    };
    if (ld_band_pieces(h, band, 0, M, fill)) return 1;
    HIP_TRY(hipMemsetAsync(h->beta, 0, (size_t)M * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(h->comp, 0, (size_t)M * sizeof(int32_t), h->stream));
    HIP_TRY(hipMemsetAsync(h->acum, 0, (size_t)M * sizeof(double), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    s->band_ms = ms;
    h->ss = std::move(s);
    return 0;
}

// ---- the sweep of a set of chains: what hgibbs_ss_sweep, _streams and _replicas do on the host ----
constexpr uint32_t SS_RMAX = 64u;        // replicas of one handle
constexpr uint32_t SS_SUMS_GMAX = 8192u; // groups whose sums fit the LDS of k_ss_replica_sums

namespace {

// The per-chain device arrays of C chains on the one band: chain r's order, mask, c, effects, components and acum lie r M behind
// chain 0's, its tables r 4 G K and its counters r G K (k_ss_sweep_replicas' strides; one chain has none).
struct SsChains {
    int32_t* order;
    uint8_t* ada;
    double *c, *beta;
    int32_t* comp;
    double *acum, *tables;
    int32_t* cass;
    uint32_t C;
};

// the handle's own chain
SsChains ss_own_chain(hgibbs_ctx* h, SsState* s) { return SsChains{s->order, s->ada, s->c, h->beta, h->comp, h->acum, h->tables, h->cass, 1u}; }

// the replicas of hgibbs_ss_replicas
SsChains ss_replica_chains(SsState* s) { return SsChains{s->rorder, s->rada, s->rc, s->rbeta, s->rcomp, s->racum, s->rtables, s->rcass, s->R}; }

// the ss state of a handle that has replicas: null (with the error set) unless it has, and, where the caller names their number, R of them
SsState* ss_replicas_of(hgibbs_ctx* h, const char* who, const uint32_t* R = nullptr)
{
    SsState* s = ss_of(h, who);
    if (!s) return nullptr;
    if (R && (*R < 1u || *R > SS_RMAX)) {
        fail("%s: R = %u, must be in [1, %u]", who, *R, SS_RMAX);
        return nullptr;
    }
    if (s->R == 0) {
        fail("%s: no replicas on this handle (hgibbs_ss_replicas first)", who);
        return nullptr;
    }
    if (R && *R != s->R) {
        fail("%s: R = %u, but hgibbs_ss_replicas allocated %u replicas", who, *R, s->R);
        return nullptr;
    }
    return s;
}

// What an entry point passes on, chain after chain where there are several: orders [C][M], sigmaE [C], sigmaG [C][G], estPi [C][G K],
// adaV [C][M], rngs [C][S] (in and out), cass [C][G K] and nnz [C] (out; nnz may be null).
struct SsSweepCall {
    const char* who;
    const char* tag;        // what a chain is called in a refusal ("replica"), null where there is only the one
    bool intervals;         // S intervals at `bounds`, each with a generator; false: hgibbs_ss_sweep's one generator and an order taken as it comes
    uint32_t S;
    const uint32_t* bounds; // S + 1
    const int32_t* orders;
    const double *sigmaE, *sigmaG, *estPi;
    const uint8_t* adaV;
    hgibbs_rng_state* rngs;
    int32_t* cass;
    uint64_t* nnz;
    uint32_t* mt; // where k_ss_sweep takes the one generator's 624 words (its index goes by value), or null: C S whole states in s->mts
    double* i2s;  // where k_ss_sweep_replicas takes 1 / (2 sigmaE) of every chain, or null: the kernel takes it by value
};

// The checks on orders, bounds and generators, the uploads, `launch` (the entry point's kernel on its grid) inside the lap, and the
// way back of the results, the generators and the counters.  A refused call has touched nothing on the device.
template <class Launch>
int ss_sweep_run(hgibbs_ctx* h, SsState* s, const SsChains& ch, const SsSweepCall& a, Launch launch)
{
    const char* who = a.who;
    const uint32_t M = h->M, C = ch.C, S = a.S;
    const int G = h->G, K = h->K;
    const size_t GK = (size_t)G * K, CS = (size_t)C * S;
    char why[256], pre[32] = "";
    auto chain = [&](uint32_t r, const char* sep) -> const char* { // "replica r: " in a refusal of several chains
        if (a.tag) snprintf(pre, sizeof pre, "%s %u%s", a.tag, r, sep);
        return pre;
    };
    if (a.intervals) s->grouped.resize((size_t)C * M);
    for (uint32_t r = 0; r < C; ++r) {
        const int32_t* order = a.orders + (size_t)r * M;
        hgibbs_rng_state* rngs = a.rngs + (size_t)r * S;
        for (uint32_t i = 0; i < M; ++i)
            if (order[i] < 0 || (uint32_t)order[i] >= M) return fail("%s: %sorder[%u]=%d outside [0,%u)", who, chain(r, ": "), i, order[i], M);
        if (!a.intervals) { // no permutation check: an order with repeated markers is swept as it stands
            if (rngs->idx > (uint32_t)MT_N) return fail("%s: rng idx %u > 624", who, rngs->idx);
            continue;
        }
        if (!a.bounds) return fail("%s: null argument", who);
        if (ss_streams_check(M, s->ahead_host.data(), s->cut.data(), S, a.bounds, rngs, why, sizeof why)) return fail("%s: %s%s", who, chain(r, ": "), why);
        if (const uint32_t bad = ss_group_order(M, order, S, a.bounds, s->grouped.data() + (size_t)r * M))
            return fail("%s: %sorder[%u] = %d repeats a marker: the order must be a permutation", who, chain(r, ": "), bad - 1u, order[bad - 1u]);
    }
    const int32_t* swept = a.intervals ? s->grouped.data() : a.orders; // the orders as the kernel walks them
    HIP_TRY(hipSetDevice(h->device));
    s->sweep_ms = 0.0;
    if (CS > s->stage_cap) {
        s->stage_cap = 0;
        if (s->mts.alloc(CS * SS_RNG_WORDS) || s->sres.alloc(CS) || s->bounds.alloc(CS + 1)) return 1;
        s->stage_cap = (uint32_t)CS;
    }
    uint32_t* const mt = a.mt ? a.mt : s->mts.p;
    const size_t mt_bytes = a.mt ? MT_N * sizeof(uint32_t) : CS * sizeof(hgibbs_rng_state); // the states of all intervals in one copy

    std::vector<double> tab((size_t)C * 4 * GK), i2s(C);
    s->ada_host.resize((size_t)C * M);
    for (uint32_t r = 0; r < C; ++r) {
        ss_tables(G, K, s->n_eff - 1.0, a.sigmaE[r], a.sigmaG + (size_t)r * G, a.estPi + r * GK, h->cVa.data(), h->cVaI.data(), tab.data() + (size_t)r * 4 * GK);
        i2s[r] = 1.0 / (2.0 * a.sigmaE[r]);
        const uint8_t* adaV = a.adaV + (size_t)r * M;
        uint8_t* ada = s->ada_host.data() + (size_t)r * M;
        for (uint32_t j = 0; j < M; ++j) ada[j] = (uint8_t)(adaV[j] && s->ok[j]); // a marker without a finite sd is never adaptive
    }
    HIP_TRY(hipMemcpyAsync(ch.tables, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (a.i2s) HIP_TRY(hipMemcpyAsync(a.i2s, i2s.data(), (size_t)C * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(ch.order, swept, (size_t)C * M * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(ch.ada, s->ada_host.data(), (size_t)C * M, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(ch.cass, 0, (size_t)C * GK * sizeof(int32_t), h->stream));
    HIP_TRY(hipMemcpyAsync(mt, a.rngs, mt_bytes, hipMemcpyHostToDevice, h->stream));
    if (a.intervals) HIP_TRY(hipMemcpyAsync(s->bounds, a.bounds, ((size_t)S + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));

    SsSweepParams p{};
    p.order = ch.order;
    p.groups = h->groups;
    p.ada = ch.ada;
    p.ahead = s->ahead;
    p.back = s->back;
    p.band = s->band;
    p.c = ch.c;
    p.beta = ch.beta;
    p.comp = ch.comp;
    p.acum = ch.acum;
    p.tables = ch.tables;
    p.mt = mt;
    p.zig = ZigTables{h->zig, h->zig + 129, h->zig + 258, h->zig + 515};
    p.cass = ch.cass;
    p.res = s->sres;
    p.M = M;
    p.W = s->W;
    p.rng_idx = a.rngs->idx;
    p.K = K;
    p.GK = G * K;
    p.dNm1 = s->n_eff - 1.0;
    p.i_2sigE = i2s[0];
    if (a.intervals) p.bounds = s->bounds;
    double ms = 0.0;
    if (lap_begin(h)) return 1;
    launch(p);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, ms)) return 1;
    s->sres_host.resize(CS);
    HIP_TRY(hipMemcpy(s->sres_host.data(), s->sres, CS * sizeof(SsResult), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < C; ++r) {
        uint64_t nnz = 0;
        for (uint32_t i = 0; i < S; ++i) {
            const SsResult& res = s->sres_host[(size_t)r * S + i];
            if (res.err) {
                const uint32_t pos = res.err - 1u;
                const int32_t marker = swept[(size_t)r * M + pos];
                if (!a.intervals) return fail("%s: sweep position %u (marker %d): the component walk found no component (logL overflow)", who, pos, marker);
                return fail("%s: %sstream %u, sweep position %u of its %u (marker %d): the component walk found no component (logL overflow)", who, chain(r, ", "), i,
                            pos - a.bounds[i], a.bounds[i + 1] - a.bounds[i], marker);
            }
            nnz += res.nnz;
        }
        if (a.nnz) a.nnz[r] = nnz;
    }
    HIP_TRY(hipMemcpy(a.rngs, mt, mt_bytes, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < CS; ++i) a.rngs[i].idx = s->sres_host[i].rng_idx;
    HIP_TRY(hipMemcpy(a.cass, ch.cass, (size_t)C * GK * sizeof(int32_t), hipMemcpyDeviceToHost));
    s->sweep_ms = ms;
    return 0;
}

} // namespace

extern "C" int hgibbs_ss_sweep(hgibbs_t h, const int32_t* order_host, double sigmaE, const double* sigmaG_host, const double* estPi_host,
                               const uint8_t* adaV_host, hgibbs_rng_state* rng, int32_t* cass_host, uint64_t* nnz_updates)
{
    const char* who = "hgibbs_ss_sweep";
    SsState* s = ss_of(h, who);
    if (!s) return 1;
    if (h->G < 1) return fail("%s: model not set", who);
    if (!order_host || !sigmaG_host || !estPi_host || !adaV_host || !rng || !cass_host) return fail("%s: null argument", who);
    const SsSweepCall a{who, nullptr, false, 1u, nullptr, order_host, &sigmaE, sigmaG_host, estPi_host, adaV_host, rng, cass_host, nnz_updates, h->mt, nullptr};
    return ss_sweep_run(h, s, ss_own_chain(h, s), a, [&](const SsSweepParams& p) { k_ss_sweep<<<1, SS_TPB, 0, h->stream>>>(p); });
}

extern "C" int hgibbs_ss_sweep_streams(hgibbs_t h, const int32_t* order_host, double sigmaE, const double* sigmaG_host, const double* estPi_host,
                                       const uint8_t* adaV_host, uint32_t S, const uint32_t* bounds, hgibbs_rng_state* rngs, int32_t* cass_host,
                                       uint64_t* nnz_updates)
{
    const char* who = "hgibbs_ss_sweep_streams";
    SsState* s = ss_of(h, who);
    if (!s) return 1;
    if (h->G < 1) return fail("%s: model not set", who);
    if (!order_host || !sigmaG_host || !estPi_host || !adaV_host || !rngs || !cass_host) return fail("%s: null argument", who);
    // (null bounds are refused behind the order's range, as they always were)
    const SsSweepCall a{who, nullptr, true, S, bounds, order_host, &sigmaE, sigmaG_host, estPi_host, adaV_host, rngs, cass_host, nnz_updates, nullptr, nullptr};
    return ss_sweep_run(h, s, ss_own_chain(h, s), a, [&](const SsSweepParams& p) { k_ss_sweep_streams<<<S, SS_TPB, 0, h->stream>>>(p); });
}

// ---- R chains on one band ----
extern "C" int hgibbs_ss_replicas(hgibbs_t h, uint32_t R)
{
    const char* who = "hgibbs_ss_replicas";
    SsState* s = ss_of(h, who);
    if (!s) return 1;
    if (R < 1u || R > SS_RMAX) return fail("%s: R = %u, must be in [1, %u]", who, R, SS_RMAX);
    if (s->post_open) return fail("%s: posterior accumulators are open on this handle (hgibbs_ss_post_end first): they count these replicas", who);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t M = h->M, n = (size_t)R * M;
    // the earlier replicas go first: their memory counts as free for the new ones
    s->R = 0;
    for (DevBuf<double>* b : {&s->rc, &s->rbeta, &s->racum}) b->release();
    for (DevBuf<int32_t>* b : {&s->rcomp, &s->rorder}) b->release();
    s->rada.release();
    const size_t bytes = n * (3 * sizeof(double) + 2 * sizeof(int32_t) + 1);
    if (need_device_memory(bytes, "%s: R = %u replicas of %u markers (c, effects, acum, components, order and mask: %zu bytes, %.1f MiB)", who, R, h->M, bytes,
                           bytes / 1048576.0))
        return 1;
    if (s->rc.alloc(n) || s->rbeta.alloc(n) || s->racum.alloc(n) || s->rcomp.alloc(n) || s->rorder.alloc(n) || s->rada.alloc(n) || s->ri2s.alloc(R) ||
        s->rsums.alloc(R))
        return 1;
    for (uint32_t r = 0; r < R; ++r) HIP_TRY(hipMemcpyAsync(s->rc + r * M, s->xty, M * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(s->rbeta, 0, n * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(s->racum, 0, n * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(s->rcomp, 0, n * sizeof(int32_t), h->stream));
    HIP_TRY(hipMemsetAsync(s->rsums, 0, R * sizeof(SsResult), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    s->rep_gk = s->rep_g = 0; // (sized at the first sweep and the first sums: the model may be set after this call)
    s->R = R;
    return 0;
}

extern "C" int hgibbs_ss_sweep_replicas(hgibbs_t h, uint32_t R, const int32_t* orders, const double* sigmaE, const double* sigmaG, const double* estPi,
                                        const uint8_t* adaV, uint32_t S, const uint32_t* bounds, hgibbs_rng_state* rngs, int32_t* cass_host,
                                        uint64_t* nnz_updates)
{
    const char* who = "hgibbs_ss_sweep_replicas";
    SsState* s = ss_replicas_of(h, who, &R);
    if (!s) return 1;
    if (h->G < 1) return fail("%s: model not set", who);
    if (!orders || !sigmaE || !sigmaG || !estPi || !adaV || !rngs || !cass_host) return fail("%s: null argument", who);
    if (!bounds && S != 1u) return fail("%s: null argument", who);
    const uint32_t whole[2] = {0u, h->M};
    const size_t GK = (size_t)h->G * h->K;
    if (GK != s->rep_gk) { // the replicas' tables and counters follow the model
        HIP_TRY(hipSetDevice(h->device));
        s->rep_gk = 0;
        if (s->rtables.alloc((size_t)R * 4 * GK) || s->rcass.alloc((size_t)R * GK)) return 1;
        s->rep_gk = (uint32_t)GK;
    }
    const SsSweepCall a{who, "replica", true, S, bounds ? bounds : whole, orders, sigmaE, sigmaG, estPi, adaV, rngs, cass_host, nnz_updates, nullptr, s->ri2s};
    const SsReplicaParams q{s->ri2s};
    return ss_sweep_run(h, s, ss_replica_chains(s), a, [&](const SsSweepParams& p) { k_ss_sweep_replicas<<<dim3(S, R), SS_TPB, 0, h->stream>>>(p, q); });
}

extern "C" int hgibbs_ss_replica_sums(hgibbs_t h, double* sb, double* sc, double* bsq)
{
    const char* who = "hgibbs_ss_replica_sums";
    SsState* s = ss_replicas_of(h, who);
    if (!s) return 1;
    if (h->G < 1) return fail("%s: model not set", who);
    const uint32_t R = s->R, G = (uint32_t)h->G;
    if (G > SS_SUMS_GMAX) return fail("%s: G = %u groups, the sums are built for at most %u", who, G, SS_SUMS_GMAX);
    HIP_TRY(hipSetDevice(h->device));
    if (G != s->rep_g) {
        s->rep_g = 0;
        if (s->rbsq.alloc((size_t)R * G)) return 1;
        s->rep_g = G;
    }
    k_ss_replica_sums<<<R, 64, (size_t)G * sizeof(double), h->stream>>>(s->rbeta, s->xty, s->rc, h->groups, h->M, G, s->rsums, s->rbsq);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::vector<SsResult> res(R);
    HIP_TRY(hipMemcpy(res.data(), s->rsums, (size_t)R * sizeof(SsResult), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < R; ++r) {
        if (sb) sb[r] = res[r].sums[0];
        if (sc) sc[r] = res[r].sums[1];
    }
    if (bsq) HIP_TRY(hipMemcpy(bsq, s->rbsq, (size_t)R * G * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hgibbs_ss_replica_get(hgibbs_t h, uint32_t r, double* beta, int32_t* comp, double* acum, double* c)
{
    const char* who = "hgibbs_ss_replica_get";
    SsState* s = ss_replicas_of(h, who);
    if (!s) return 1;
    if (r >= s->R) return fail("%s: replica %u outside [0, %u)", who, r, s->R);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const SsChains ch = ss_replica_chains(s);
    const size_t M = h->M, o = (size_t)r * M;
    if (beta) HIP_TRY(hipMemcpy(beta, ch.beta + o, M * sizeof(double), hipMemcpyDeviceToHost));
    if (comp) HIP_TRY(hipMemcpy(comp, ch.comp + o, M * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (acum) HIP_TRY(hipMemcpy(acum, ch.acum + o, M * sizeof(double), hipMemcpyDeviceToHost));
    if (c) HIP_TRY(hipMemcpy(c, ch.c + o, M * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hgibbs_ss_replica_set_beta(hgibbs_t h, uint32_t r, const double* beta)
{
    const char* who = "hgibbs_ss_replica_set_beta";
    SsState* s = ss_replicas_of(h, who);
    if (!s) return 1;
    if (r >= s->R) return fail("%s: replica %u outside [0, %u)", who, r, s->R);
    if (!beta) return fail("%s: null argument", who);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(s->rbeta + (size_t)r * h->M, beta, (size_t)h->M * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int hgibbs_ss_state(hgibbs_t h, double* c_out, double* beta_b, double* beta_c)
{
    const char* who = "hgibbs_ss_state";
    SsState* s = ss_of(h, who);
    if (!s) return 1;
    HIP_TRY(hipSetDevice(h->device));
    if (beta_b || beta_c) {
        k_ss_sums<<<1, 64, 0, h->stream>>>(h->beta, s->xty, s->c, h->M, s->res);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(h->stream));
        SsResult res{};
        HIP_TRY(hipMemcpy(&res, s->res, sizeof res, hipMemcpyDeviceToHost));
        if (beta_b) *beta_b = res.sums[0];
        if (beta_c) *beta_c = res.sums[1];
    }
    if (c_out) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(c_out, s->c, (size_t)h->M * sizeof(double), hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int hgibbs_ss_band_get(hgibbs_t h, uint32_t m0, uint32_t count, double* out)
{
    const char* who = "hgibbs_ss_band_get";
    SsState* s = ss_of(h, who);
    if (!s) return 1;
    if ((uint64_t)m0 + count > h->M) return fail("%s: markers [%u, %llu) out of range (M = %u)", who, m0, (unsigned long long)m0 + count, h->M);
    if (count == 0) return 0;
    if (!out) return fail("%s: null output", who);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, s->band + (size_t)m0 * s->W, (size_t)count * s->W * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hgibbs_ss_end(hgibbs_t h)
{
    if (!h) return fail("hgibbs_ss_end: null handle");
    if (h->ss) {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->ss.reset();
    return 0;
}

extern "C" int hgibbs_last_ss_ms(hgibbs_t h, double* band_ms, double* sweep_ms)
{
    if (!h || !band_ms || !sweep_ms) return fail("hgibbs_last_ss_ms: null argument");
    *band_ms = h->ss ? h->ss->band_ms : 0.0;
    *sweep_ms = h->ss ? h->ss->sweep_ms : 0.0;
    return 0;
}
