// Firth's penalised fit of the one-parameter logistic model of the score test, per listed marker: for entry e of
// the list, the inputs of hgibbs_spa_roots (hg_spa.hip.h: marker, Z, mu, the entry's b, xv and score s) and its a_i, u = a_i t, p_i and
// terms.  With the null fit as offset, logit P(d_i = 1) = logit(mu_i) + beta a_i, the log-likelihood ratio is l(t) - l(0) = t s - K(t),
// and Firth's penalised one adds log(K''(t) / K''(0)) / 2.  Over the rows
//
//     K' = sum a (p - mu),  K'' = sum a^2 v,  K''' = sum a^3 v (1 - 2 p),  K'''' = sum a^4 v (1 - 6 v),     v = p (1 - p)
//     g(t) = s - K' + K''' / (2 K''),     g'(t) = -K'' + (K'''' / K'' - (K''' / K'')^2) / 2
//
// and the record holds the stationary point of the penalised likelihood that the rule below finds from t = 0, with K and K'' there.
// The statistics are formed on the host from it (hg_firth.cpp).
//
//   shape    one workgroup of SPA_TPB threads per entry, the rows per thread and the tree of spa_reduce as in k_spa_roots: the order
//            of every sum depends on n_local only.  No atomics.  The entries share nothing.
//   a-cache  pass 0 forms a_i (spa_adjusted: q reads of the row-major Z per row) and writes it to the entry's row of `cache` (n doubles);
//            the later passes read that one double per row.  Thread tid writes and reads the elements tid, tid + SPA_TPB, ...: no element is
//            touched by two threads, so nothing is synchronised.  The host cuts the list into pieces whose rows of the cache fit.
//   pass 0   at t = 0: k2_0 = K''(0), scale = 1 / sqrt(k2_0); a k2_0 that is not finite or not positive ends the entry (flag bit 1, every
//            other field 0).  lo = -inf, hi = +inf, tg = 0 (the last point with a finite g and g').
//   rule     g and g' finite at t: tg = t; g > 0 sets lo = t, g < 0 sets hi = t; the proposal is t' = t - g / g'.  FIRST the stop rule
//            g' < 0 and |t' - t| <= 1e-9 max(|t|, scale): the entry takes t' and one closing pass for K(t') and K''(t'), then is
//            converged (flag bit 0).  (Without g' < 0 the rule would also stop next to a local MINIMUM of the penalised likelihood:
//            with few rows and a small mu g'(0) > 0, and a score that leaves g(0) within 1e-9 scale g' of 0 closed the entry at 0.)
//            ONLY THEN the safeguard: a t' not strictly inside (lo, hi) becomes the midpoint when both ends are finite, else
//            2 t, or +-scale with g's sign when t = 0.  g or g' not finite at t (the probabilities have saturated): the bracket end on
//            t's side of tg becomes t and the next point is (t + tg) / 2; no sign is taken.
//   bound    at most FIRTH_PASSES passes after pass 0, the closing one included; an entry still open then has no flag.  The rule runs
//            in every thread on the same reduced sums, so the workgroup branches as one; every loop is bounded.
#pragma once

namespace {

constexpr int FIRTH_PASSES = 64;
constexpr double FIRTH_STOP = 1e-9;
constexpr uint32_t FIRTH_PIECE_MAX = 1u << 24; // entries per launch

static_assert(sizeof(hgibbs_firth_rec) == 48, "hgibbs_firth_rec is part of the ABI");

// One row's terms at t, added to k1 .. k4 (K' .. K'''') and, in the closing pass, kk (K): spa_terms with two more sums
__device__ __forceinline__ void firth_terms(double a, double m, double t, bool closing, double& k1, double& k2, double& k3, double& k4, double& kk)
{
    double u, cE;
    const double p = logit_point(a, m, t, u, cE);
    const double v = p * (1.0 - p);
    const double a2 = a * a;
    k1 += a * (p - m);
    k2 += a2 * v;
    k3 += (a2 * a) * (v * (1.0 - 2.0 * p));
    k4 += (a2 * a2) * (v * (1.0 - 6.0 * v));
    if (closing) kk += logit_log_term(u, cE, m);
}

// the entries [e0, e0 + gridDim.x) of the list; cache: gridDim.x rows of n doubles
__global__ __launch_bounds__(SPA_TPB) void k_firth_fit(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t n, const uint32_t* __restrict__ markers,
                                                       int q, const double* __restrict__ Zr, const double* __restrict__ mu,
                                                       const double* __restrict__ B, const double* __restrict__ xv, const double* __restrict__ s,
                                                       uint32_t e0, double* __restrict__ cache, hgibbs_firth_rec* __restrict__ out)
{
    __shared__ double sb[SPA_QMAX];
    __shared__ double red[SPA_WAVES][6];
    const uint32_t tid = threadIdx.x, e = e0 + blockIdx.x;
    const uint32_t* col = reinterpret_cast<const uint32_t*>(bed + (uint64_t)markers[e] * stride);
    double* const ca = cache + (uint64_t)blockIdx.x * n;
    if (tid < (uint32_t)q) sb[tid] = B[(uint64_t)e * (uint32_t)q + tid];
    const double x0 = xv[4ull * e], x1 = xv[4ull * e + 1u], x2 = xv[4ull * e + 2u], x3 = xv[4ull * e + 3u];
    const double se = s[e];
    __syncthreads();

    double v[6];
    double t = 0.0, tg = 0.0, lo = -INFINITY, hi = INFINITY, scale = 0.0;
    hgibbs_firth_rec r;
    r.beta = r.K = r.K2 = r.g = r.k2_0 = 0.0;
    r.iters = 0;
    r.flags = 0u;
    bool closing = false;
    for (int pass = 0; pass <= FIRTH_PASSES; ++pass) {
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = 0.0;
        if (pass == 0) {
            for (uint32_t i = tid; i < n; i += SPA_TPB) {
                const double a = spa_adjusted(col, Zr, q, sb, x0, x1, x2, x3, i);
                ca[i] = a;
                firth_terms(a, mu[i], 0.0, false, v[0], v[1], v[2], v[3], v[4]);
            }
        } else {
            for (uint32_t i = tid; i < n; i += SPA_TPB) firth_terms(ca[i], mu[i], t, closing, v[0], v[1], v[2], v[3], v[4]);
        }
        spa_reduce<5>(v, red, tid);
        if (pass == 0) {
            if (!(isfinite(v[1]) && v[1] > 0.0)) {
                r.flags = 2u;
                break;
            }
            r.k2_0 = v[1];
            scale = 1.0 / sqrt(v[1]);
        } else {
            ++r.iters;
        }
        if (closing) {
            r.K = v[4];
            r.K2 = v[1];
            r.flags |= 1u;
            break;
        }
        const double ratio = v[2] / v[1];
        const double g = (se - v[0]) + 0.5 * ratio;
        const double gp = 0.5 * (v[3] / v[1] - ratio * ratio) - v[1];
        double tn;
        if (isfinite(g) && isfinite(gp)) {
            r.g = g;
            tg = t;
            if (g > 0.0) lo = t;
            else if (g < 0.0) hi = t;
            tn = t - g / gp;
            if (gp < 0.0 && fabs(tn - t) <= FIRTH_STOP * fmax(fabs(t), scale)) closing = true;
            else if (!(tn > lo && tn < hi))
                tn = (isfinite(lo) && isfinite(hi)) ? 0.5 * (lo + hi) : t == 0.0 ? (g > 0.0 ? scale : -scale) : 2.0 * t;
        } else {
            if (t > tg) hi = t;
            else if (t < tg) lo = t;
            tn = 0.5 * (t + tg);
        }
        t = tn;
    }
    if (tid == 0u) {
        if (!(r.flags & 2u)) r.beta = t;
        out[e] = r;
    }
}

} // namespace

extern "C" int hgibbs_firth_fit(hgibbs_t h, uint32_t nm, const uint32_t* markers, int q, const double* Z, const double* mu, const double* B,
                                const double* xv, const double* s, hgibbs_firth_rec* out)
{
    if (h) h->firth_ms = 0.0; // (before the guard: 0 after every refusal, those of the guard included)
    if (op_guard(h, "hgibbs_firth_fit", "the sums over the rows are not summed over ranks")) return 1;
    if (const int c = null_list_check(h, "hgibbs_firth_fit", nm, markers, q, Z, mu, B, xv, s, out)) return c > 0;
    HIP_TRY(hipSetDevice(h->device));

    // the list's own buffers, then the a-cache of one piece: `piece` entries of n doubles each
    const uint32_t n = h->n_local;
    const size_t row = (size_t)n * sizeof(double);
    const size_t bytes = NullList::bytes(n, nm, q) + (size_t)nm * sizeof(hgibbs_firth_rec);
    uint32_t piece = (uint32_t)std::min<uint64_t>({(uint64_t)nm, (uint64_t)FIRTH_PIECE_MAX, h->firth_piece ? (uint64_t)h->firth_piece : ~0ull});
    if (!h->firth_piece) { // automatic: a quarter of the free memory, one entry at the least
        size_t fre = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fre, &tot));
        piece = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(piece, fre / 4 / std::max<size_t>(row, sizeof(double))));
    }
    if (need_device_memory(bytes + (size_t)piece * row, "hgibbs_firth_fit: %u markers against a null model of %d columns and pieces of %u entries need %.1f MiB", nm,
                           q, piece, (bytes + (size_t)piece * row) / 1048576.0))
        return 1;
    NullList l;
    DevBuf<hgibbs_firth_rec> dout;
    DevBuf<double> dcache;
    // device time of every kernel, not the host copies around them; the pieces follow each other on the stream and share the cache
    double ms = 0.0;
    if (dout.alloc(nm) || dcache.alloc((size_t)piece * n) || null_list_begin(h, l, nm, markers, q, Z, mu, B, xv, s)) return 1;
    for (uint32_t e0 = 0; e0 < nm; e0 += piece) {
        k_firth_fit<<<std::min(piece, nm - e0), SPA_TPB, 0, h->stream>>>(h->bed, h->stride, n, l.dmk, q, l.dZr, l.dmu, l.dB, l.dxv, l.ds, e0, dcache, dout);
        HIP_TRY(hipGetLastError());
    }
    if (lap_end(h, ms)) return 1;
    HIP_TRY(hipMemcpy(out, dout, (size_t)nm * sizeof(hgibbs_firth_rec), hipMemcpyDeviceToHost));
    h->firth_ms = ms;
    return 0;
}

extern "C" int hgibbs_last_firth_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_firth_ms: null argument");
    *ms = h->firth_ms;
    return 0;
}
