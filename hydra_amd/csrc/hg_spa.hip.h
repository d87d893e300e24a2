// Saddlepoints of the logistic score test, per listed marker: for entry e of the list, marker j = markers[e],
// the null model's rows (Z n_local x q, mu) and the entry's own b (q), xv (4) and score s, with
//
//     a_i = xv[code_ij] - sum_k Z_ik b_k,     u = a_i t,     p_i = mu_i e^u / (1 - mu_i + mu_i e^u)
//     K(t) = sum_i [log(1 - mu_i + mu_i e^u) - u mu_i],   K'(t) = sum_i a_i (p_i - mu_i),   K''(t) = sum_i a_i^2 p_i (1 - p_i)
//
// the roots t of K'(t) = tau for the two tails tau = +|s| (index 0) and tau = -|s| (index 1), with K and K'' there.  The p-value is
// formed on the host from them (hg_spa.cpp).
//
//   shape    one workgroup of SPA_TPB threads per entry; the entries share nothing, so a record does not depend on the list around it.
//   rows     thread tid takes the rows tid, tid + SPA_TPB, ... < n_local in that order: neighbouring lanes read neighbouring rows of
//            the row-major copy of Z (k_spa_rowmajor), so a wave's reads of one column of Z fall into 4 q cache lines that its reads
//            of the other columns hit again, and the sixteen lanes of a stored BED dword read the same dword.  a_i is formed once per
//            row and pass and serves both tails.  Padding slots past n_local are never read.
//   sums     per thread in row order, then spa_reduce: a shuffle tree inside the wave, the waves' sums through LDS, added as
//            (w0 + w1) + (w2 + w3).  No atomics.  The order depends on n_local only: bit-identical for any chunking of the list, any
//            position in it and any repeat.
//   terms    the branch-free stable form (logit_point, also k_firth_fit's): E = expm1(-|u|); for u <= 0, D = 1 + mu E, p = mu (1 + E) / D,
//            log term log1p(mu E); for u > 0, D = 1 + (1 - mu) E, p = mu / D, log term u + log1p((1 - mu) E).  The log term is evaluated only
//            in a tail's closing pass (K is not needed before).  f64 expm1, log1p and division of the device library; no contraction.
//   pass 0   k2_0 = K''(0), c = sum a_i mu_i, s_hi = sum max(a_i, 0) - c, s_lo = sum min(a_i, 0) - c.  A tail whose tau is not
//            strictly inside (s_lo, s_hi) is unreachable (flag bit 2 + tail) and is not iterated.
//   root     from t = tau / k2_0 with the open bracket (0, inf) resp. (-inf, 0): the sign of K'(t) - tau tightens the bracket, the
//            proposal is t' = t - (K' - tau) / K''.  FIRST the stop rule |t' - t| <= 1e-9 max(|t|, 1 / sqrt(k2_0)): the tail takes t'
//            and one closing pass for K(t') and K''(t'), then is converged (flag bit tail).  ONLY THEN the safeguard: a t' not
//            strictly inside the bracket becomes its midpoint when both ends are finite, else 2 t.  (An exact hit K' = tau proposes
//            t' = t, which is not inside the bracket: the safeguard first would bisect on from a root already found.)
//   bound    at most SPA_PASSES passes per entry after pass 0, the closing ones included; a tail still open then stays unconverged.
//            The root rule runs in every thread on the same reduced sums, so the workgroup branches as one; every loop is bounded.
#pragma once

namespace {

constexpr int SPA_TPB = 256;
constexpr int SPA_WAVES = SPA_TPB / 64;
constexpr int SPA_QMAX = 64;
constexpr int SPA_PASSES = 64;
constexpr double SPA_STOP = 1e-9;

static_assert(sizeof(hgibbs_spa_root) == 88, "hgibbs_spa_root is part of the ABI");

// Z (n x q column-major) -> Zr (row-major): one thread per entry of Zr
__global__ __launch_bounds__(SPA_TPB) void k_spa_rowmajor(const double* __restrict__ Z, uint32_t n, int q, double* __restrict__ Zr)
{
    const uint64_t e = (uint64_t)blockIdx.x * SPA_TPB + threadIdx.x;
    if (e >= (uint64_t)n * (uint32_t)q) return;
    const uint32_t i = (uint32_t)(e / (uint32_t)q), k = (uint32_t)(e % (uint32_t)q);
    Zr[e] = Z[(uint64_t)k * n + i];
}

// The workgroup's sums of the first NV per-thread values, in every thread: the fixed tree of the header
template <int NV>
__device__ __forceinline__ void spa_reduce(double (&v)[6], double (*red)[6], uint32_t tid)
{
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    if ((tid & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    static_assert(SPA_WAVES == 4, "the tree adds four waves");
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    __syncthreads();
}

// The stable logistic point of one row at u = a t, in the form of the header: p, with u and cE = c E for the log term
__device__ __forceinline__ double logit_point(double a, double m, double t, double& u, double& cE)
{
    u = a * t;
    const bool neg = u <= 0.0;
    const double E = expm1(-fabs(u));
    const double c = neg ? m : 1.0 - m;
    cE = c * E;
    const double D = 1.0 + cE;
    return (neg ? m * (1.0 + E) : m) / D;
}
__device__ __forceinline__ double logit_log_term(double u, double cE, double m) { return ((u <= 0.0 ? 0.0 : u) + log1p(cE)) - u * m; } // the row's term of K

// One row's terms of one tail at t, added to k1 (K'), k2 (K'') and, in the closing pass, kk (K)
__device__ __forceinline__ void spa_terms(double a, double m, double t, bool closing, double& k1, double& k2, double& kk)
{
    double u, cE;
    const double p = logit_point(a, m, t, u, cE);
    k1 += a * (p - m);
    k2 += (a * a) * (p * (1.0 - p));
    if (closing) kk += logit_log_term(u, cE, m);
}

// The adjusted genotype a_i of row i: the value xv of the row's BED code in the marker's column `col`, less row i of the row-major Z
// times the entry's b (in LDS)
__device__ __forceinline__ double spa_adjusted(const uint32_t* col, const double* Zr, int q, const double* sb, double x0, double x1, double x2,
                                               double x3, uint32_t i)
{
    const uint32_t code = (col[i >> 4] >> (2u * (i & 15u))) & 3u;
    const double* z = Zr + (uint64_t)i * (uint32_t)q;
    double zb = 0.0;
#pragma unroll 4
    for (int k = 0; k < q; ++k) zb += z[k] * sb[k]; // (the loads of four columns in flight; the sum stays in column order)
    return (code == 0u ? x0 : code == 1u ? x1 : code == 2u ? x2 : x3) - zb;
}

__global__ __launch_bounds__(SPA_TPB) void k_spa_roots(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t n, const uint32_t* __restrict__ markers,
                                                       int q, const double* __restrict__ Zr, const double* __restrict__ mu,
                                                       const double* __restrict__ B, const double* __restrict__ xv, const double* __restrict__ s,
                                                       hgibbs_spa_root* __restrict__ out)
{
    __shared__ double sb[SPA_QMAX];
    __shared__ double red[SPA_WAVES][6];
    const uint32_t tid = threadIdx.x, e = blockIdx.x;
    const uint32_t* col = reinterpret_cast<const uint32_t*>(bed + (uint64_t)markers[e] * stride);
    if (tid < (uint32_t)q) sb[tid] = B[(uint64_t)e * (uint32_t)q + tid];
    const double x0 = xv[4u * e], x1 = xv[4u * e + 1u], x2 = xv[4u * e + 2u], x3 = xv[4u * e + 3u];
    const double sabs = fabs(s[e]);
    __syncthreads();

    double v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = 0.0;
    for (uint32_t i = tid; i < n; i += SPA_TPB) {
        const double a = spa_adjusted(col, Zr, q, sb, x0, x1, x2, x3, i), m = mu[i];
        v[0] += (a * a) * (m * (1.0 - m));
        v[1] += a * m;
        v[2] += fmax(a, 0.0);
        v[3] += fmin(a, 0.0);
    }
    spa_reduce<4>(v, red, tid);
    const double k2_0 = v[0], s_hi = v[2] - v[1], s_lo = v[3] - v[1];
    const double scale = 1.0 / sqrt(k2_0);

    double t[2], tau[2], lo[2], hi[2], K[2], K2[2];
    int st[2], iters[2]; // st: 0 idle, 1 iterating, 2 closing pass
    uint32_t flags = 0u;
#pragma unroll
    for (int z = 0; z < 2; ++z) {
        tau[z] = z == 0 ? sabs : -sabs;
        lo[z] = z == 0 ? 0.0 : -INFINITY;
        hi[z] = z == 0 ? INFINITY : 0.0;
        K[z] = K2[z] = 0.0;
        iters[z] = 0;
        const bool reach = tau[z] > s_lo && tau[z] < s_hi;
        st[z] = reach ? 1 : 0;
        t[z] = reach ? tau[z] / k2_0 : 0.0;
        if (!reach) flags |= 4u << z;
    }

    for (int pass = 0; pass < SPA_PASSES; ++pass) {
        const int st0 = __builtin_amdgcn_readfirstlane(st[0]), st1 = __builtin_amdgcn_readfirstlane(st[1]); // (the same in every thread)
        if (!(st0 | st1)) break;
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = 0.0;
        for (uint32_t i = tid; i < n; i += SPA_TPB) {
            const double a = spa_adjusted(col, Zr, q, sb, x0, x1, x2, x3, i), m = mu[i];
            if (st0) spa_terms(a, m, t[0], st0 == 2, v[0], v[1], v[2]);
            if (st1) spa_terms(a, m, t[1], st1 == 2, v[3], v[4], v[5]);
        }
        spa_reduce<6>(v, red, tid);
#pragma unroll
        for (int z = 0; z < 2; ++z) {
            const int sz = z == 0 ? st0 : st1;
            if (!sz) continue;
            ++iters[z];
            if (sz == 2) {
                K2[z] = v[3 * z + 1];
                K[z] = v[3 * z + 2];
                flags |= 1u << z;
                st[z] = 0;
                continue;
            }
            const double g = v[3 * z] - tau[z];
            if (g > 0.0) hi[z] = t[z];
            else if (g < 0.0) lo[z] = t[z];
            double tn = t[z] - g / v[3 * z + 1];
            if (fabs(tn - t[z]) <= SPA_STOP * fmax(fabs(t[z]), scale)) st[z] = 2;
            else if (!(tn > lo[z] && tn < hi[z])) tn = (isfinite(lo[z]) && isfinite(hi[z])) ? 0.5 * (lo[z] + hi[z]) : 2.0 * t[z];
            t[z] = tn;
        }
    }

    if (tid == 0u) {
        hgibbs_spa_root r;
#pragma unroll
        for (int z = 0; z < 2; ++z) {
            r.t[z] = t[z];
            r.K[z] = K[z];
            r.K2[z] = K2[z];
            r.iters[z] = iters[z];
        }
        r.k2_0 = k2_0;
        r.s_lo = s_lo;
        r.s_hi = s_hi;
        r.flags = flags;
        r.reserved_ = 0u;
        out[e] = r;
    }
}

// ---- a list of markers against a null model: the host code that hgibbs_spa_roots and hgibbs_firth_fit share ----
struct NullList {
    DevBuf<double> dZ, dZr, dmu, dB, dxv, ds;
    DevBuf<uint32_t> dmk;
    // the bytes of the buffers above for nm entries, without the caller's records
    static size_t bytes(uint32_t n, uint32_t nm, int q) { return (2 * ((size_t)n * q) + n + (size_t)nm * (q + 5)) * sizeof(double) + (size_t)nm * sizeof(uint32_t); }
};

// The arguments of `who`, after op_guard: null check, bound on q, every value.  0: go on; 1: refused; -1: an empty list, of which nothing is read
int null_list_check(const hgibbs_ctx* h, const char* who, uint32_t nm, const uint32_t* markers, int q, const double* Z, const double* mu, const double* B,
                    const double* xv, const double* s, const void* out)
{
    if (!markers || !Z || !mu || !B || !xv || !s || !out) return fail("%s: null argument", who);
    if (q < 1 || q > SPA_QMAX) return fail("%s: q = %d, must be in [1, %d]", who, q, SPA_QMAX);
    if (nm == 0) return -1;
    const uint32_t n = h->n_local;
    for (uint32_t e = 0; e < nm; ++e)
        if (markers[e] >= h->M) return fail("%s: markers[%u] = %u out of range (M = %u)", who, e, markers[e], h->M);
    for (size_t k = 0; k < (size_t)q * n; ++k)
        if (!std::isfinite(Z[k])) return fail("%s: Z[%zu][%d] = %g is not finite", who, k % n, (int)(k / n), Z[k]);
    for (uint32_t i = 0; i < n; ++i)
        if (!(mu[i] > 0.0 && mu[i] < 1.0)) return fail("%s: mu[%u] = %g is not strictly inside (0, 1)", who, i, mu[i]);
    for (size_t k = 0; k < (size_t)nm * q; ++k)
        if (!std::isfinite(B[k])) return fail("%s: B[%zu][%d] = %g is not finite", who, k / q, (int)(k % q), B[k]);
    for (size_t k = 0; k < (size_t)nm * 4; ++k)
        if (!std::isfinite(xv[k])) return fail("%s: xv[%zu][%d] = %g is not finite", who, k / 4, (int)(k % 4), xv[k]);
    for (uint32_t e = 0; e < nm; ++e)
        if (!std::isfinite(s[e])) return fail("%s: s[%u] = %g is not finite", who, e, s[e]);
    return 0;
}

// The list's buffers and their uploads on the handle's stream; then the caller's lap begins, with the row-major copy of Z as its first kernel
int null_list_begin(hgibbs_ctx* h, NullList& l, uint32_t nm, const uint32_t* markers, int q, const double* Z, const double* mu, const double* B,
                     const double* xv, const double* s)
{
    const uint32_t n = h->n_local;
    const size_t nq = (size_t)n * q;
    if (l.dZ.alloc(nq) || l.dZr.alloc(nq) || l.dmu.alloc(n) || l.dB.alloc((size_t)nm * q) || l.dxv.alloc((size_t)nm * 4) || l.ds.alloc(nm) || l.dmk.alloc(nm)) return 1;
    HIP_TRY(hipMemcpyAsync(l.dZ, Z, nq * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(l.dmu, mu, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(l.dB, B, (size_t)nm * q * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(l.dxv, xv, (size_t)nm * 4 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(l.ds, s, (size_t)nm * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(l.dmk, markers, (size_t)nm * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (lap_begin(h)) return 1;
    k_spa_rowmajor<<<(uint32_t)((nq + SPA_TPB - 1) / SPA_TPB), SPA_TPB, 0, h->stream>>>(l.dZ, n, q, l.dZr);
    HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace

extern "C" int hgibbs_spa_roots(hgibbs_t h, uint32_t nm, const uint32_t* markers, int q, const double* Z, const double* mu, const double* B,
                                const double* xv, const double* s, hgibbs_spa_root* out)
{
    if (h) h->spa_ms = 0.0; // (before the guard: 0 after every refusal, those of the guard included)
    if (op_guard(h, "hgibbs_spa_roots", "the sums over the rows are not summed over ranks")) return 1;
    if (const int c = null_list_check(h, "hgibbs_spa_roots", nm, markers, q, Z, mu, B, xv, s, out)) return c > 0;
    HIP_TRY(hipSetDevice(h->device));

    const size_t bytes = NullList::bytes(h->n_local, nm, q) + (size_t)nm * sizeof(hgibbs_spa_root);
    if (need_device_memory(bytes, "hgibbs_spa_roots: %u markers against a null model of %d columns need %.1f MiB", nm, q, bytes / 1048576.0)) return 1;
    NullList l;
    DevBuf<hgibbs_spa_root> dout;
    double ms = 0.0; // device time of both kernels, not the host copies around them
    if (dout.alloc(nm) || null_list_begin(h, l, nm, markers, q, Z, mu, B, xv, s)) return 1;
    k_spa_roots<<<nm, SPA_TPB, 0, h->stream>>>(h->bed, h->stride, h->n_local, l.dmk, q, l.dZr, l.dmu, l.dB, l.dxv, l.ds, dout);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, ms)) return 1;
    HIP_TRY(hipMemcpy(out, dout, (size_t)nm * sizeof(hgibbs_spa_root), hipMemcpyDeviceToHost));
    h->spa_ms = ms;
    return 0;
}

extern "C" int hgibbs_last_spa_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_spa_ms: null argument");
    *ms = h->spa_ms;
    return 0;
}
