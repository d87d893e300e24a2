// The per-marker posterior table of the summary-statistics chains, accumulated where the chains' state lies.
// Between hgibbs_ss_post_begin and hgibbs_ss_post_end the handle's ss state holds, per marker, the pooled Welford pair of the effects
// over every chain and record, the pair of every half-chain (hg_mcmcdiag.cpp's split: records [0, n) and [T - n, T), n = T / 2), and
// the draws per component.  Nothing of a record crosses the bus.
//
//   add     k_ss_post_add: ONE launch per record, a thread per marker, the chains r = 0 .. C - 1 in order inside the thread.  The loads
//           of beta[r M + j] and comp[r M + j] depend on nothing the thread computes, so the unrolled loop issues them ahead of the
//           pooled pair's chain of divisions.  The component counts of the record are kept in MAX_K registers by compare-and-add (no
//           runtime-indexed array) and added to cnt[k M + j] once, so cnt costs K words per marker and not one per chain.
//   final   k_ss_post_final: mean, sd, PIP and split-R^ per marker from the accumulators, in hg_mcmcdiag.cpp's order of operations from
//           cv = hm2 / (n - 1) on.
//   step    d = x - mean; mean = mean + d / n; m2 = m2 + d (x - mean): correctly rounded f64 + - x /, and the file is built with
//           -ffp-contract=off, so a restatement in scalar f64 gives the same bits (tests/sspost_restate.py).
//
// Every accumulator is read and written by the one thread of its marker: no atomics, no LDS.  The one atomic is on the error word (a
// component outside [0, K)), which no valid record touches.
#pragma once

namespace {

constexpr int SP_TPB = 256;
constexpr unsigned long long SP_NO_FLAG = ~0ull;

// Thread per marker j.  C chains whose effects and components lie at r M; record t (0-based) of T; HALF: the record lies in half
// `half` of every chain and is draw number `nh` (1-based) of it.  hmean and hm2 are [C][2][M]; cnt is [K][M].
template <bool HALF>
__global__ __launch_bounds__(SP_TPB) void k_ss_post_add(const double* __restrict__ beta, const int32_t* __restrict__ comp, uint32_t M, uint32_t C, int K,
                                                        uint32_t t, uint32_t half, uint32_t nh, double* __restrict__ pmean, double* __restrict__ pm2,
                                                        double* __restrict__ hmean, double* __restrict__ hm2, uint32_t* __restrict__ cnt,
                                                        unsigned long long* __restrict__ flag)
{
    const uint32_t j = blockIdx.x * (uint32_t)SP_TPB + threadIdx.x;
    if (j >= M) return;
    double mean = pmean[j], m2 = pm2[j];
    const double dnh = (double)nh;
    const uint32_t q0 = t * C; // (C T < 2^32: hgibbs_ss_post_begin)
    uint32_t ck[MAX_K];
    unsigned long long bad = SP_NO_FLAG;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) ck[k] = 0u;
#pragma unroll 4
    for (uint32_t r = 0; r < C; ++r) {
        const size_t o = (size_t)r * M + j;
        const double x = beta[o];
        const int32_t k = comp[o];
        double d = x - mean;
        mean = mean + d / (double)(q0 + r + 1u);
        m2 = m2 + d * (x - mean);
        if (HALF) {
            const size_t oh = ((size_t)2u * r + half) * M + j;
            double hm = hmean[oh], h2 = hm2[oh];
            d = x - hm;
            hm = hm + d / dnh;
            h2 = h2 + d * (x - hm);
            hmean[oh] = hm;
            hm2[oh] = h2;
        }
#pragma unroll
        for (int kk = 0; kk < MAX_K; ++kk) ck[kk] += (k == kk) ? 1u : 0u;
        bad = ((uint32_t)k >= (uint32_t)K && bad == SP_NO_FLAG) ? (((unsigned long long)r << 32) | j) : bad; // this marker's first such chain
    }
    if (bad != SP_NO_FLAG) atomicMin(flag, bad); // over the markers: the first (chain, marker) in that order
    pmean[j] = mean;
    pm2[j] = m2;
#pragma unroll
    for (int kk = 0; kk < MAX_K; ++kk)
        if (kk < K) cnt[(size_t)kk * M + j] += ck[kk];
}

// Thread per marker: out = mean, sd, pip, rhat (M each).  C chains of T records, n = T / 2 records per half-chain, m = 2 C half-chains
// in the order h = 2 r + half.
__global__ __launch_bounds__(SP_TPB) void k_ss_post_final(const double* __restrict__ pmean, const double* __restrict__ pm2, const uint32_t* __restrict__ cnt0,
                                                          const double* __restrict__ hmean, const double* __restrict__ hm2, uint32_t M, uint32_t C, uint32_t T,
                                                          double* __restrict__ out)
{
    const uint32_t j = blockIdx.x * (uint32_t)SP_TPB + threadIdx.x;
    if (j >= M) return;
    const uint32_t all = C * T, n = T / 2u, m = 2u * C;
    out[j] = pmean[j];
    out[(size_t)M + j] = sqrt(pm2[j] / (double)(all - 1u));
    out[(size_t)2 * M + j] = (double)(all - cnt0[j]) / (double)all;
    double W = 0.0, gm = 0.0;
    for (uint32_t h = 0; h < m; ++h) {
        const size_t o = (size_t)h * M + j;
        W += hm2[o] / (double)(n - 1u);
        gm += hmean[o];
    }
    W /= (double)m;
    gm /= (double)m;
    double Bn = 0.0;
    for (uint32_t h = 0; h < m; ++h) {
        const double cm = hmean[(size_t)h * M + j];
        Bn += (cm - gm) * (cm - gm);
    }
    Bn /= (double)(m - 1u);
    const double varp = (double)(n - 1u) / (double)n * W + Bn;
    out[(size_t)3 * M + j] = W > 0.0 ? sqrt(varp / W) : __builtin_nan("");
}

// the open post state of a handle, with `adds` == T when `done` is asked for
SsState* ss_post_of(hgibbs_ctx* h, const char* who, bool done)
{
    SsState* s = ss_of(h, who);
    if (!s) return nullptr;
    if (!s->post_open) {
        fail("%s: no posterior accumulators on this handle (hgibbs_ss_post_begin first)", who);
        return nullptr;
    }
    if (done && s->post_t != s->post_T) {
        fail("%s: %u of the %u planned records were added: the table is read after the last", who, s->post_t, s->post_T);
        return nullptr;
    }
    return s;
}

// the chains the open accumulators count: post_R replicas, or (0) the handle's own chain
SsChains ss_post_chains(hgibbs_ctx* h, SsState* s) { return s->post_R ? ss_replica_chains(s) : ss_own_chain(h, s); }

void ss_post_close(SsState* s)
{
    s->post_open = false;
    for (DevBuf<double>* b : {&s->pmean, &s->pm2, &s->phmean, &s->phm2, &s->pout}) b->release();
    s->pcnt.release();
    s->pflag.release();
}

} // namespace

// hgibbs_set_model's question (the struct is incomplete where it is asked)
bool ss_post_is_open(const hgibbs_ctx* h) { return h && h->ss && h->ss->post_open; }

extern "C" int hgibbs_ss_post_begin(hgibbs_t h, uint32_t R, uint32_t T)
{
    const char* who = "hgibbs_ss_post_begin";
    SsState* s = R >= 1u ? ss_replicas_of(h, who, &R) : ss_of(h, who);
    if (!s) return 1;
    if (T < 4u) return fail("%s: T = %u records per chain, split-R^ needs at least 4", who, T);
    const uint32_t C = R ? R : 1u;
    if ((uint64_t)C * T >= (1ull << 32)) return fail("%s: R = %u chains of T = %u records: the pooled count R T must stay below 2^32", who, R, T);
    if (h->G < 1) return fail("%s: model not set (the number of components K is not known)", who);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    ss_post_close(s); // an earlier state goes first: its memory counts as free for the new one
    const size_t M = h->M, K = (size_t)h->K, nh = (size_t)C * 2u * M;
    const size_t bytes = M * (2 + 4) * sizeof(double) + K * M * sizeof(uint32_t) + 2 * nh * sizeof(double) + sizeof(unsigned long long);
    if (need_device_memory(bytes, "%s: R = %u, T = %u: the accumulators of %u markers (pooled pair, %zu component counts, %u half-chain pairs, the table: %zu bytes, %.1f MiB)",
                           who, R, T, h->M, K, 2u * C, bytes, bytes / 1048576.0))
        return 1;
    if (s->pmean.alloc(M) || s->pm2.alloc(M) || s->phmean.alloc(nh) || s->phm2.alloc(nh) || s->pout.alloc(4 * M) || s->pcnt.alloc(K * M) || s->pflag.alloc(1)) {
        ss_post_close(s);
        return 1;
    }
    HIP_TRY(hipMemsetAsync(s->pmean, 0, M * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(s->pm2, 0, M * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(s->phmean, 0, nh * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(s->phm2, 0, nh * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(s->pcnt, 0, K * M * sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(s->pflag, 0xff, sizeof(unsigned long long), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    s->post_R = R;
    s->post_T = T;
    s->post_t = 0;
    s->post_K = (uint32_t)K;
    s->post_add_ms = s->post_final_ms = 0.0;
    s->post_final = false;
    s->post_open = true;
    return 0;
}

extern "C" int hgibbs_ss_post_add(hgibbs_t h)
{
    const char* who = "hgibbs_ss_post_add";
    SsState* s = ss_post_of(h, who, false);
    if (!s) return 1;
    if (s->post_t >= s->post_T) return fail("%s: the %u planned records are all added", who, s->post_T);
    HIP_TRY(hipSetDevice(h->device));
    const SsChains ch = ss_post_chains(h, s);
    const uint32_t M = h->M, C = ch.C, T = s->post_T, t = s->post_t, n = T / 2u;
    const uint32_t grid = (M + (uint32_t)SP_TPB - 1u) / (uint32_t)SP_TPB;
    double ms = 0.0;
    if (lap_begin(h)) return 1;
    if (t < n)
        k_ss_post_add<true><<<grid, SP_TPB, 0, h->stream>>>(ch.beta, ch.comp, M, C, (int)s->post_K, t, 0u, t + 1u, s->pmean, s->pm2, s->phmean, s->phm2, s->pcnt, s->pflag);
    else if (t >= T - n)
        k_ss_post_add<true><<<grid, SP_TPB, 0, h->stream>>>(ch.beta, ch.comp, M, C, (int)s->post_K, t, 1u, t - (T - n) + 1u, s->pmean, s->pm2, s->phmean, s->phm2, s->pcnt,
                                                            s->pflag);
    else // the middle record of an odd T: in no half
        k_ss_post_add<false><<<grid, SP_TPB, 0, h->stream>>>(ch.beta, ch.comp, M, C, (int)s->post_K, t, 0u, 1u, s->pmean, s->pm2, s->phmean, s->phm2, s->pcnt, s->pflag);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, ms)) return 1;
    unsigned long long flag = SP_NO_FLAG;
    HIP_TRY(hipMemcpy(&flag, s->pflag, sizeof flag, hipMemcpyDeviceToHost));
    if (flag != SP_NO_FLAG) {
        const uint32_t K = s->post_K;
        ss_post_close(s); // the record is half counted: the accumulators are of no use any more
        return fail("%s: record %u: chain %u, marker %u: its component is outside [0, %u); the accumulators are dropped", who, t, (uint32_t)(flag >> 32),
                    (uint32_t)(flag & 0xffffffffull), K);
    }
    s->post_add_ms += ms;
    s->post_t = t + 1u;
    return 0;
}

namespace {

// the table, computed once after the last add
int ss_post_finish(hgibbs_ctx* h, SsState* s)
{
    if (s->post_final) return 0;
    const uint32_t M = h->M, C = ss_post_chains(h, s).C;
    double ms = 0.0;
    if (lap_begin(h)) return 1;
    k_ss_post_final<<<(M + (uint32_t)SP_TPB - 1u) / (uint32_t)SP_TPB, SP_TPB, 0, h->stream>>>(s->pmean, s->pm2, s->pcnt, s->phmean, s->phm2, M, C, s->post_T, s->pout);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, ms)) return 1;
    s->post_final_ms = ms;
    s->post_final = true;
    return 0;
}

} // namespace

extern "C" int hgibbs_ss_post_get(hgibbs_t h, double* mean, double* sd, double* pip, uint32_t* cnt, double* rhat)
{
    SsState* s = ss_post_of(h, "hgibbs_ss_post_get", true);
    if (!s) return 1;
    HIP_TRY(hipSetDevice(h->device));
    if (ss_post_finish(h, s)) return 1;
    const size_t M = h->M;
    double* const outs[4] = {mean, sd, pip, rhat};
    for (int i = 0; i < 4; ++i)
        if (outs[i]) HIP_TRY(hipMemcpy(outs[i], s->pout + (size_t)i * M, M * sizeof(double), hipMemcpyDeviceToHost));
    if (cnt) HIP_TRY(hipMemcpy(cnt, s->pcnt, (size_t)s->post_K * M * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hgibbs_ss_post_raw(hgibbs_t h, uint32_t r, uint32_t half, double* hmean, double* hm2)
{
    const char* who = "hgibbs_ss_post_raw";
    SsState* s = ss_post_of(h, who, true);
    if (!s) return 1;
    const uint32_t C = ss_post_chains(h, s).C;
    if (r > C || half > 1u || (r == C && half != 0u))
        return fail("%s: r = %u, half = %u: a half-chain is r in [0, %u) with half 0 or 1, the pooled pair r = %u with half 0", who, r, half, C, C);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t M = h->M, o = ((size_t)2u * r + half) * M;
    if (hmean) HIP_TRY(hipMemcpy(hmean, r == C ? s->pmean.p : s->phmean + o, M * sizeof(double), hipMemcpyDeviceToHost));
    if (hm2) HIP_TRY(hipMemcpy(hm2, r == C ? s->pm2.p : s->phm2 + o, M * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hgibbs_ss_post_end(hgibbs_t h)
{
    if (!h) return fail("hgibbs_ss_post_end: null handle");
    if (h->ss && h->ss->post_open) {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        ss_post_close(h->ss.get());
    }
    return 0;
}

extern "C" int hgibbs_last_ss_post_ms(hgibbs_t h, double* add_ms, double* final_ms)
{
    if (!h) return fail("hgibbs_last_ss_post_ms: null handle");
    const bool open = h->ss && h->ss->post_open;
    if (add_ms) *add_ms = open ? h->ss->post_add_ms : 0.0;
    if (final_ms) *final_ms = open ? h->ss->post_final_ms : 0.0;
    return 0;
}
