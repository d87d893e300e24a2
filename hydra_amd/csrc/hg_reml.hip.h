// REML heritability without the relationship matrix (the contract is in include/hgibbs.h).  n = n_local rows,
// M_used the markers with a finite mstd, X the chain's standardisation, A = X X'/M_used, Q an orthonormal basis of the covariate
// columns Z (q x n), P_c = I - QQ', H(delta) = P_c A P_c + delta I.  A is never formed.  One iteration of the solver is
//
//     T  = X'P                    the marker-dots pipeline (hg_mdots.hip.h) on device pointers
//     a  = t mstd / M_used, o = -a mave, rows outside M_used zeroed      (k_reml_fold: k_pca_fold's job plus the scale)
//     Y  = X T                    the score pipeline (hg_score.hip.h) on device pointers
//     Hp = P_c Y + delta p        (k_reml_cross for Q'Y, k_reml_project)
//     the column dots p'Hp, the update of v and r, the column dots r'r, the update of p      (k_reml_dots, k_reml_update)
//
// for up to 32 columns at once, each with its own scalars; a column whose r'r has fallen to tol^2 b'b is frozen and its v, r and p
// stop changing.  The panels are vector-major (K x n) and stay in HBM; the host reads two K-vectors of dots per iteration.
//
// Every floating-point sum over rows or markers runs in k_pca_gram's order: workgroup w takes the RM_ROWS entries from w RM_ROWS,
// one thread sums an entry of the result over them IN ORDER, and k_pca_gram_sum adds the workgroups' partials in workgroup order.
// No floating-point atomic, no tree; a column's numbers do not depend on how many columns ride with it.
//
//   k_reml_cross    A'B of two tall panels (La x Lb entries, k_pca_gram's thread map): Q'Y of the projection, the 2 x 2 of the AI step
//   k_reml_dots     the L column dots of two tall panels
//   k_reml_project  out = in - Q C (+ delta p), C = Q'in from k_reml_cross; `in` in either layout, out vector-major
//   k_reml_fold     T -> a, o with the 1 / M_used scale
//   k_reml_update   phase 0: v += alpha p, r -= alpha Hp;  phase 1: p = r + beta p;  frozen columns skipped
//   k_reml_probe_w  the score weights of the marker probes s(2t, j) / sqrt(M_used);  k_reml_probe_e  the row probes s(2t + 1, i)
//   k_reml_rhs      b_t = G_t + sqrt(delta) E_t, b_T = P_c y
#pragma once

namespace {

constexpr int RM_TPB = 256;
constexpr int RM_ROWS = PG_ROWS;    // entries per workgroup of a sum (the fixed partition)
constexpr int RM_TILE = 64;         // entries staged in LDS at a time
constexpr int RM_KMAX = MD_KMAX;    // columns at most
constexpr int RM_LD = RM_KMAX + 2;  // doubles between the rows of an LDS tile (16-byte aligned rows)
static_assert(RM_TPB * 4 == RM_KMAX * RM_KMAX, "k_reml_cross: one thread per four entries of the result");

struct RmCoef {
    double c[RM_KMAX];
};

// +1 / -1 from the top bit of the counter's hash (k_pca_init's convention: vector c, index i)
__host__ __device__ inline double rm_sign(uint64_t seed, uint64_t c, uint64_t i)
{
    return (mix64((seed ^ mix64(c)) + i * 0xD1B54A32D192ED03ull) >> 63) ? -1.0 : 1.0;
}

// stages rows [t0, t0 + nr) of a panel (len x L; vm: P[l len + i], else P[i L + l]) into tile[r RM_LD + l], zero beyond nr
__device__ __forceinline__ void rm_stage(double* tile, const double* __restrict__ P, uint32_t len, uint32_t L, int vm, uint32_t t0, uint32_t nr)
{
    if (vm) {
        for (uint32_t idx = threadIdx.x; idx < (uint32_t)RM_TILE * L; idx += RM_TPB) {
            const uint32_t l = idx / RM_TILE, r = idx % RM_TILE;
            tile[r * RM_LD + l] = r < nr ? P[(size_t)l * len + t0 + r] : 0.0;
        }
    } else {
        for (uint32_t idx = threadIdx.x; idx < (uint32_t)RM_TILE * L; idx += RM_TPB) {
            const uint32_t r = idx / L, l = idx % L;
            tile[r * RM_LD + l] = r < nr ? P[(size_t)t0 * L + idx] : 0.0;
        }
    }
}

// partial[w][a Lb + b] = sum over the rows of workgroup w of A(i, a) B(i, b); thread t owns a = t / 8, b = 4 (t % 8) .. + 3
__global__ __launch_bounds__(RM_TPB) void k_reml_cross(const double* __restrict__ A, int La, int vmA, const double* __restrict__ B, int Lb, int vmB,
                                                       uint32_t len, double* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) double ta[RM_TILE * RM_LD];
    __shared__ __attribute__((aligned(16))) double tb[RM_TILE * RM_LD];
    const uint32_t tid = threadIdx.x, ua = (uint32_t)La, ub = (uint32_t)Lb;
    const uint32_t r0 = blockIdx.x * RM_ROWS, r1 = min(len, r0 + RM_ROWS);
    const uint32_t ea = tid >> 3, eb = 4u * (tid & 7u);
    const bool active = ea < ua && eb < ub;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t idx = tid; idx < (uint32_t)(RM_TILE * RM_LD); idx += RM_TPB) tb[idx] = 0.0; // (the columns from Lb on stay zero)
    __syncthreads();
    for (uint32_t t0 = r0; t0 < r1; t0 += RM_TILE) {
        const uint32_t nr = min((uint32_t)RM_TILE, r1 - t0);
        rm_stage(ta, A, len, ua, vmA, t0, nr);
        rm_stage(tb, B, len, ub, vmB, t0, nr);
        __syncthreads();
        if (active) {
            for (uint32_t r = 0; r < nr; ++r) { // (in order: the sum of an entry never leaves its thread)
                const double x = ta[r * RM_LD + ea];
                const double* row = tb + r * RM_LD;
                const double2 b01 = *reinterpret_cast<const double2*>(row + eb), b23 = *reinterpret_cast<const double2*>(row + eb + 2u);
                acc[0] += x * b01.x;
                acc[1] += x * b01.y;
                acc[2] += x * b23.x;
                acc[3] += x * b23.y;
            }
        }
        __syncthreads();
    }
    if (!active) return;
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c)
        if (eb + c < ub) partial[(size_t)blockIdx.x * ua * ub + ea * ub + eb + c] = acc[c];
}

// partial[w][l] = sum over the rows of workgroup w of A(i, l) B(i, l)
__global__ __launch_bounds__(RM_TPB) void k_reml_dots(const double* __restrict__ A, int vmA, const double* __restrict__ B, int vmB, int L, uint32_t len,
                                                      double* __restrict__ partial)
{
    __shared__ double ta[RM_TILE * RM_LD];
    __shared__ double tb[RM_TILE * RM_LD];
    const uint32_t tid = threadIdx.x, uL = (uint32_t)L;
    const uint32_t r0 = blockIdx.x * RM_ROWS, r1 = min(len, r0 + RM_ROWS);
    double acc = 0.0;
    for (uint32_t t0 = r0; t0 < r1; t0 += RM_TILE) {
        const uint32_t nr = min((uint32_t)RM_TILE, r1 - t0);
        rm_stage(ta, A, len, uL, vmA, t0, nr);
        rm_stage(tb, B, len, uL, vmB, t0, nr);
        __syncthreads();
        if (tid < uL)
            for (uint32_t r = 0; r < nr; ++r) acc += ta[r * RM_LD + tid] * tb[r * RM_LD + tid];
        __syncthreads();
    }
    if (tid < uL) partial[(size_t)blockIdx.x * uL + tid] = acc;
}

// out[l n + i] = (in(i, l) - sum_c Q[c n + i] C[c L + l]) + delta p[l n + i]   (c in order; the last term only with p)
// One thread per row; in place when `in` is vector-major and out == in.
__global__ __launch_bounds__(RM_TPB) void k_reml_project(const double* in, int vm, int L, const double* __restrict__ Q, int q, const double* __restrict__ C,
                                                         double delta, const double* __restrict__ p, uint32_t n, double* out)
{
    __shared__ double sC[RM_KMAX * RM_KMAX];
    for (uint32_t idx = threadIdx.x; idx < (uint32_t)(q * L); idx += RM_TPB) sC[idx] = C[idx];
    __syncthreads();
    const uint32_t i = blockIdx.x * RM_TPB + threadIdx.x;
    if (i >= n) return;
    double qv[RM_KMAX];
#pragma unroll
    for (int c = 0; c < RM_KMAX; ++c) qv[c] = c < q ? Q[(size_t)c * n + i] : 0.0;
    for (int l = 0; l < L; ++l) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < RM_KMAX; ++c)
            if (c < q) s += qv[c] * sC[c * L + l];
        double v = (vm ? in[(size_t)l * n + i] : in[(size_t)i * L + l]) - s;
        if (p) v += delta * p[(size_t)l * n + i];
        out[(size_t)l * n + i] = v;
    }
}

// k_pca_fold with the scale: block = 64 markers x L entries of T; a = t mstd / m_used, o = -a mave, zero (in T as well) outside M_used
__global__ __launch_bounds__(RM_TPB) void k_reml_fold(double* __restrict__ T, const double* __restrict__ mave, const double* __restrict__ mstd, uint32_t M,
                                                      int L, double m_used, double* __restrict__ a, double* __restrict__ o)
{
    __shared__ double tile[64 * (RM_KMAX + 1)];
    const uint32_t j0 = blockIdx.x * 64u, nj = min(64u, M - j0);
    for (uint32_t idx = threadIdx.x; idx < nj * (uint32_t)L; idx += RM_TPB) {
        const uint32_t jj = idx / (uint32_t)L, l = idx % (uint32_t)L;
        double t = T[(size_t)j0 * L + idx];
        if (!isfinite(mstd[j0 + jj])) {
            t = 0.0;
            T[(size_t)j0 * L + idx] = 0.0;
        }
        tile[jj * (RM_KMAX + 1) + l] = t;
    }
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < 64u * (uint32_t)L; idx += RM_TPB) {
        const uint32_t l = idx / 64u, jj = idx % 64u;
        if (jj >= nj) continue;
        const double sd = mstd[j0 + jj];
        const bool used = isfinite(sd);
        const double w = used ? tile[jj * (RM_KMAX + 1) + l] * sd / m_used : 0.0;
        a[(size_t)l * M + j0 + jj] = w;
        o[(size_t)l * M + j0 + jj] = used ? -(w * mave[j0 + jj]) : 0.0;
    }
}

// the columns whose bit of `live` is set: phase 0  v += c p, r -= c hp;  phase 1  p = r + c p
__global__ __launch_bounds__(RM_TPB) void k_reml_update(double* __restrict__ V, double* __restrict__ R, double* __restrict__ P, const double* __restrict__ HP,
                                                        RmCoef coef, uint32_t live, int phase, uint32_t n, int K)
{
    const uint64_t e = (uint64_t)blockIdx.x * RM_TPB + threadIdx.x;
    if (e >= (uint64_t)n * (uint32_t)K) return;
    const uint32_t k = (uint32_t)(e / n);
    if (!((live >> k) & 1u)) return;
    const double c = coef.c[k];
    if (phase == 0) {
        V[e] += c * P[e];
        R[e] -= c * HP[e];
    } else {
        P[e] = R[e] + c * P[e];
    }
}

__global__ __launch_bounds__(RM_TPB) void k_reml_probe_w(const double* __restrict__ mave, const double* __restrict__ mstd, uint32_t M, int T, uint64_t seed,
                                                         double root_m, double* __restrict__ a, double* __restrict__ o)
{
    const uint64_t e = (uint64_t)blockIdx.x * RM_TPB + threadIdx.x;
    if (e >= (uint64_t)M * (uint32_t)T) return;
    const uint64_t t = e / M, j = e % M;
    const double sd = mstd[j];
    const bool used = isfinite(sd);
    const double w = used ? rm_sign(seed, 2u * t, j) / root_m * sd : 0.0;
    a[e] = w;
    o[e] = used ? -(w * mave[j]) : 0.0;
}

__global__ __launch_bounds__(RM_TPB) void k_reml_probe_e(double* __restrict__ E, uint32_t n, int T, uint64_t seed, uint32_t row_begin)
{
    const uint64_t e = (uint64_t)blockIdx.x * RM_TPB + threadIdx.x;
    if (e >= (uint64_t)n * (uint32_t)T) return;
    E[e] = rm_sign(seed, 2u * (e / n) + 1u, row_begin + e % n);
}

__global__ __launch_bounds__(RM_TPB) void k_reml_rhs(const double* __restrict__ G, const double* __restrict__ E, const double* __restrict__ Py, double root_delta,
                                                     int T, uint32_t n, double* __restrict__ B)
{
    const uint64_t e = (uint64_t)blockIdx.x * RM_TPB + threadIdx.x;
    if (e >= (uint64_t)n * (uint32_t)(T + 1)) return;
    B[e] = e < (uint64_t)n * (uint32_t)T ? G[e] + root_delta * E[e] : Py[e - (uint64_t)n * (uint32_t)T];
}

// Q (q x n, vector-major) from Z: modified Gram-Schmidt applied twice, sequential f64 in a fixed order; -1, or the dependent column
int reml_basis(const double* Z, uint32_t n, int q, std::vector<double>& Q)
{
    Q.assign(Z, Z + (size_t)q * n);
    for (int c = 0; c < q; ++c) {
        double* v = Q.data() + (size_t)c * n;
        double before = 0.0;
        for (uint32_t i = 0; i < n; ++i) before += v[i] * v[i];
        for (int round = 0; round < 2; ++round)
            for (int b = 0; b < c; ++b) {
                const double* u = Q.data() + (size_t)b * n;
                double d = 0.0;
                for (uint32_t i = 0; i < n; ++i) d += u[i] * v[i];
                for (uint32_t i = 0; i < n; ++i) v[i] -= d * u[i];
            }
        double after = 0.0;
        for (uint32_t i = 0; i < n; ++i) after += v[i] * v[i];
        if (!(after > 1e-20 * before) || !std::isfinite(after)) return c;
        const double nrm = std::sqrt(after);
        for (uint32_t i = 0; i < n; ++i) v[i] /= nrm;
    }
    return -1;
}

// What the three entry points share: the panels, the two pipelines' work buffers, the clock (part 1 = products, 2 = the rest)
struct RemlWork {
    hgibbs_ctx* h = nullptr;
    const char* who = "";
    uint32_t n = 0, M = 0, m_used = 0;
    int q = 0, kmax = 0;
    DevBuf<double> Q, B, V, R, P, HP, Y, T, a, o, partial, small, G, E, Py;
    MdotsWs mw;
    ScoreWs sw;
    PcaClock clk;
    double host[3 * RM_KMAX];
    double* dC() const { return small; }                               // q x L of the projection, or the 2 x 2 of the AI step
    double* dS(int i) const { return small + RM_KMAX * RM_KMAX + i * RM_KMAX; } // three K-vectors of dots
};

// The refusals and the memory every entry point needs.  probes: room for G, E (T x n each, T = kmax - 1) and P_c y as well.
int reml_setup(RemlWork& w, hgibbs_ctx* h, const char* who, int kmax, int q, const double* Z, bool probes)
{
    w.h = h;
    w.who = who;
    if (!Z) return fail("%s: null argument", who);
    const uint32_t n = h->n_local, M = h->M;
    if (n >= MD_NMAX) return fail("%s: %u individuals, at most %u (64-bit sums of the marker dots)", who, n, MD_NMAX - 1u);
    if (q < 1 || q > RM_KMAX) return fail("%s: q = %d covariate columns, must be in [1, %d]", who, q, RM_KMAX);
    if ((uint64_t)q + 1u >= n) return fail("%s: q = %d covariate columns, must be below n - 1 = %u", who, q, n - 1u);
    for (size_t i = 0; i < (size_t)q * n; ++i)
        if (!std::isfinite(Z[i])) return fail("%s: Z[%d][%zu] = %g is not finite", who, (int)(i / n), i % n, Z[i]);
    std::vector<double> Q;
    const int dep = reml_basis(Z, n, q, Q);
    if (dep >= 0) return fail("%s: covariate column %d is linearly dependent on the columns before it (or zero)", who, dep);
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;
    uint32_t m_used = 0;
    {
        std::vector<double> sd(M);
        HIP_TRY(hipMemcpy(sd.data(), h->mstd, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
        for (uint32_t j = 0; j < M; ++j) m_used += std::isfinite(sd[j]) ? 1u : 0u;
    }
    if (m_used == 0) return fail("%s: M_used = 0: no marker has a finite standard deviation", who);
    w.n = n;
    w.M = M;
    w.m_used = m_used;
    w.q = q;
    w.kmax = kmax;
    const size_t nK = (size_t)n * kmax, MK = (size_t)M * kmax, nbmax = ((size_t)std::max(n, M) + RM_ROWS - 1) / RM_ROWS;
    const size_t npart = nbmax * RM_KMAX * RM_KMAX, nsmall = RM_KMAX * RM_KMAX + 3 * RM_KMAX;
    const size_t nprobe = probes ? 2 * (size_t)n * (kmax - 1) + n : 0;
    const size_t bytes = ((size_t)q * n + 6 * nK + 3 * MK + npart + nsmall + nprobe) * sizeof(double) + mdots_ws_bytes(h, kmax, M) + score_ws_bytes(h, kmax);
    if (need_device_memory(bytes, "%s: the panels and work buffers need %.1f MiB", who, bytes / 1048576.0)) return 1;
    if (w.Q.alloc((size_t)q * n) || w.B.alloc(nK) || w.V.alloc(nK) || w.R.alloc(nK) || w.P.alloc(nK) || w.HP.alloc(nK) || w.Y.alloc(nK)) return 1;
    if (w.T.alloc(MK) || w.a.alloc(MK) || w.o.alloc(MK) || w.partial.alloc(npart) || w.small.alloc(nsmall)) return 1;
    if (probes && (w.G.alloc((size_t)n * (kmax - 1)) || w.E.alloc((size_t)n * (kmax - 1)) || w.Py.alloc(n))) return 1;
    if (mdots_ws_create(h, w.mw, kmax, M)) return 1;
    if (score_ws_create(h, w.sw, kmax)) return 1;
    w.clk.stream = h->stream;
    if (w.clk.create()) return 1;
    HIP_TRY(hipMemcpy(w.Q, Q.data(), (size_t)q * n * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

// the partials of a sum in workgroup order: nb x LL -> dout
int reml_sum(RemlWork& w, uint32_t nb, uint32_t LL, double* dout)
{
    k_pca_gram_sum<<<(LL + PG_TPB - 1) / PG_TPB, PG_TPB, 0, w.h->stream>>>(w.partial, nb, LL, dout);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the L column dots of two panels of `len` rows into the device vector dout
int reml_dots(RemlWork& w, const double* A, int vmA, const double* B, int vmB, int L, uint32_t len, double* dout)
{
    const uint32_t nb = (len + RM_ROWS - 1) / RM_ROWS;
    k_reml_dots<<<nb, RM_TPB, 0, w.h->stream>>>(A, vmA, B, vmB, L, len, w.partial);
    HIP_TRY(hipGetLastError());
    return reml_sum(w, nb, (uint32_t)L, dout);
}

// out (vector-major) = P_c in (+ delta p): C = Q'in, then the rows
int reml_project(RemlWork& w, const double* in, int vm, int L, double delta, const double* p, double* out)
{
    const uint32_t nb = (w.n + RM_ROWS - 1) / RM_ROWS;
    k_reml_cross<<<nb, RM_TPB, 0, w.h->stream>>>(w.Q, w.q, 1, in, L, vm, w.n, w.partial);
    HIP_TRY(hipGetLastError());
    if (reml_sum(w, nb, (uint32_t)(w.q * L), w.dC())) return 1;
    k_reml_project<<<(w.n + RM_TPB - 1) / RM_TPB, RM_TPB, 0, w.h->stream>>>(in, vm, L, w.Q, w.q, w.dC(), delta, p, w.n, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// T = X'U for L vectors (vector-major), the rows outside M_used zeroed, folded to the score weights a, o
int reml_xt(RemlWork& w, const double* U, int L)
{
    hgibbs_ctx* h = w.h;
    if (mdots_dev_clear(h, w.mw, w.M, L)) return 1;
    if (w.clk.begin(1)) return 1;
    if (mdots_dev_run(h, w.mw, 0, w.M, L, U, w.T, nullptr)) return 1;
    if (w.clk.end()) return 1;
    if (w.clk.begin(2)) return 1;
    k_reml_fold<<<(w.M + 63u) / 64u, RM_TPB, 0, h->stream>>>(w.T, h->mave, h->mstd, w.M, L, (double)w.m_used, w.a, w.o);
    HIP_TRY(hipGetLastError());
    if (w.clk.end()) return 1;
    return 0;
}

// Y (n x L, row-major) = X T from the weights in a, o
int reml_xy(RemlWork& w, int L)
{
    if (score_dev_clear(w.h, w.sw, L, false)) return 1; // (the flag of non-finite weights gathers over every product)
    if (w.clk.begin(1)) return 1;
    if (score_dev_run(w.h, w.sw, L, w.a, w.o, w.Y)) return 1;
    if (w.clk.end()) return 1;
    return 0;
}

// reads `count` doubles from the device into w.host at the stream's next synchronisation, which it makes
int reml_read(RemlWork& w, const double* d, int count)
{
    HIP_TRY(hipMemcpyAsync(w.host, d, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, w.h->stream));
    return w.clk.sync();
}

// CG on the K columns of w.B (raw; left projected), the solution in w.V
int reml_solve_dev(RemlWork& w, int K, double delta, double tol, int max_iters, int* iters, double* relres)
{
    hgibbs_ctx* h = w.h;
    const uint32_t n = w.n;
    const size_t nK = (size_t)n * K;
    const uint32_t grid = (uint32_t)((nK + RM_TPB - 1) / RM_TPB);
    double rr[RM_KMAX], bb[RM_KMAX];
    RmCoef coef{};
    if (w.clk.begin(2)) return 1;
    if (reml_project(w, w.B, 1, K, 0.0, nullptr, w.B)) return 1;
    HIP_TRY(hipMemcpyAsync(w.R, w.B, nK * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(w.P, w.B, nK * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(w.V, 0, nK * sizeof(double), h->stream));
    if (reml_dots(w, w.R, 1, w.R, 1, K, n, w.dS(0))) return 1;
    if (w.clk.end()) return 1;
    if (reml_read(w, w.dS(0), K)) return 1;
    for (int k = 0; k < K; ++k) {
        rr[k] = bb[k] = w.host[k];
        iters[k] = 0;
        if (!std::isfinite(bb[k])) return fail("%s: right-hand side %d is not finite after the projection", w.who, k);
    }
    for (int it = 0;; ++it) {
        uint32_t live = 0;
        for (int k = 0; k < K; ++k)
            if (!(rr[k] <= tol * tol * bb[k])) live |= 1u << k;
        if (!live) break;
        if (it >= max_iters) {
            int k = 0;
            while (!((live >> k) & 1u)) ++k;
            return fail("%s: column %d has not converged after max_iters = %d iterations: |r| / |b| = %.3g against tol = %.3g", w.who, k, max_iters,
                        std::sqrt(rr[k] / bb[k]), tol);
        }
        if (reml_xt(w, w.P, K)) return 1;
        if (reml_xy(w, K)) return 1;
        if (w.clk.begin(2)) return 1;
        if (reml_project(w, w.Y, 0, K, delta, w.P, w.HP)) return 1;
        if (reml_dots(w, w.P, 1, w.HP, 1, K, n, w.dS(0))) return 1;
        if (w.clk.end()) return 1;
        if (reml_read(w, w.dS(0), K)) return 1;
        for (int k = 0; k < K; ++k) {
            coef.c[k] = 0.0;
            if (!((live >> k) & 1u)) continue;
            const double php = w.host[k];
            if (!(php > 0.0) || !std::isfinite(php)) return fail("%s: p'Hp = %g in column %d at iteration %d: not positive and finite", w.who, php, k, it + 1);
            coef.c[k] = rr[k] / php;
            ++iters[k];
        }
        if (w.clk.begin(2)) return 1;
        k_reml_update<<<grid, RM_TPB, 0, h->stream>>>(w.V, w.R, w.P, w.HP, coef, live, 0, n, K);
        HIP_TRY(hipGetLastError());
        if (reml_dots(w, w.R, 1, w.R, 1, K, n, w.dS(0))) return 1;
        if (w.clk.end()) return 1;
        if (reml_read(w, w.dS(0), K)) return 1;
        uint32_t next = 0;
        for (int k = 0; k < K; ++k) {
            coef.c[k] = 0.0;
            if (!((live >> k) & 1u)) continue;
            const double nrr = w.host[k];
            if (!std::isfinite(nrr)) return fail("%s: r'r = %g in column %d at iteration %d", w.who, nrr, k, it + 1);
            coef.c[k] = nrr / rr[k];
            rr[k] = nrr;
            if (!(rr[k] <= tol * tol * bb[k])) next |= 1u << k;
        }
        if (next) { // (a column that froze keeps its p)
            if (w.clk.begin(2)) return 1;
            k_reml_update<<<grid, RM_TPB, 0, h->stream>>>(w.V, w.R, w.P, w.HP, coef, next, 1, n, K);
            HIP_TRY(hipGetLastError());
            if (w.clk.end()) return 1;
        }
    }
    for (int k = 0; k < K; ++k) relres[k] = bb[k] > 0.0 ? std::sqrt(rr[k] / bb[k]) : 0.0;
    return 0;
}

// G, E and P_c y, once
int reml_probes(RemlWork& w, int T, uint64_t seed, const double* y)
{
    hgibbs_ctx* h = w.h;
    const uint32_t n = w.n, M = w.M;
    HIP_TRY(hipMemcpyAsync(w.Py, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (w.clk.begin(2)) return 1;
    k_reml_probe_w<<<(uint32_t)(((size_t)M * T + RM_TPB - 1) / RM_TPB), RM_TPB, 0, h->stream>>>(h->mave, h->mstd, M, T, seed, std::sqrt((double)w.m_used), w.a, w.o);
    HIP_TRY(hipGetLastError());
    k_reml_probe_e<<<(uint32_t)(((size_t)n * T + RM_TPB - 1) / RM_TPB), RM_TPB, 0, h->stream>>>(w.E, n, T, seed, h->row_begin);
    HIP_TRY(hipGetLastError());
    if (reml_project(w, w.E, 1, T, 0.0, nullptr, w.E)) return 1;
    if (reml_project(w, w.Py, 1, 1, 0.0, nullptr, w.Py)) return 1;
    if (w.clk.end()) return 1;
    if (reml_xy(w, T)) return 1;
    if (w.clk.begin(2)) return 1;
    if (reml_project(w, w.Y, 0, T, 0.0, nullptr, w.G)) return 1;
    if (w.clk.end()) return 1;
    return w.clk.sync();
}

// the (T + 1) x 3 sums at delta; the solution stays in w.V and u = X'v (zero outside M_used) in w.T
int reml_eval_dev(RemlWork& w, int T, double delta, double tol, int max_iters, double* sums, int* iters_max)
{
    hgibbs_ctx* h = w.h;
    const uint32_t n = w.n;
    const int K = T + 1;
    int iters[RM_KMAX];
    double relres[RM_KMAX];
    if (w.clk.begin(2)) return 1;
    k_reml_rhs<<<(uint32_t)(((size_t)n * K + RM_TPB - 1) / RM_TPB), RM_TPB, 0, h->stream>>>(w.G, w.E, w.Py, std::sqrt(delta), T, n, w.B);
    HIP_TRY(hipGetLastError());
    if (w.clk.end()) return 1;
    if (reml_solve_dev(w, K, delta, tol, max_iters, iters, relres)) return 1;
    if (reml_xt(w, w.V, K)) return 1;
    if (w.clk.begin(2)) return 1;
    if (reml_dots(w, w.T, 0, w.T, 0, K, w.M, w.dS(0))) return 1;
    if (reml_dots(w, w.V, 1, w.V, 1, K, n, w.dS(1))) return 1;
    if (reml_dots(w, w.V, 1, w.B, 1, K, n, w.dS(2))) return 1;
    if (w.clk.end()) return 1;
    if (reml_read(w, w.dS(0), 3 * RM_KMAX)) return 1;
    int mx = 0;
    for (int k = 0; k < K; ++k) {
        sums[3 * k] = w.host[k] / (double)w.m_used;
        sums[3 * k + 1] = w.host[RM_KMAX + k];
        sums[3 * k + 2] = w.host[2 * RM_KMAX + k];
        mx = std::max(mx, iters[k]);
    }
    if (iters_max) *iters_max = mx;
    return 0;
}

int reml_f(const double* sums, int T, double* f)
{
    double a = 0.0, b = 0.0;
    for (int t = 0; t < T; ++t) {
        a += sums[3 * t];
        b += sums[3 * t + 1];
    }
    *f = std::log(a / b) - std::log(sums[3 * T] / sums[3 * T + 1]);
    return std::isfinite(*f) ? 0 : 1;
}

// the closing checks and the publication of the device times
int reml_close(RemlWork& w)
{
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, w.sw.bad, sizeof(uint32_t), hipMemcpyDeviceToHost, w.h->stream));
    if (w.clk.sync()) return 1;
    if (bad) return fail("%s: a panel entry is not finite (a weight of one of the X T products)", w.who);
    w.h->reml_ms[0] = w.clk.ms[1];
    w.h->reml_ms[1] = w.clk.ms[2];
    return 0;
}

int reml_scalar_guard(const char* who, double delta, double tol, int max_iters)
{
    if (!(delta > 0.0) || !std::isfinite(delta)) return fail("%s: delta = %g, must be positive and finite", who, delta);
    if (!(tol > 0.0) || !std::isfinite(tol)) return fail("%s: tol = %g, must be positive and finite", who, tol);
    if (max_iters < 1) return fail("%s: max_iters = %d, needs at least one iteration", who, max_iters);
    return 0;
}

} // namespace

extern "C" int hgibbs_reml_solve(hgibbs_t h, int K, int q, const double* Z, double delta, double tol, int max_iters, const double* B, double* V,
                                 int* iters, double* relres)
{
    static const char* who = "hgibbs_reml_solve";
    if (op_guard(h, who, "the panel products are not summed over ranks")) return 1;
    if (K < 1 || K > RM_KMAX) return fail("%s: K = %d right-hand sides, must be in [1, %d]", who, K, RM_KMAX);
    if (!B || !V || !iters || !relres) return fail("%s: null argument", who);
    if (reml_scalar_guard(who, delta, tol, max_iters)) return 1;
    const uint32_t n = h->n_local;
    h->reml_ms[0] = h->reml_ms[1] = 0.0;
    RemlWork w;
    if (reml_setup(w, h, who, K, q, Z, false)) return 1;
    for (size_t i = 0; i < (size_t)K * n; ++i)
        if (!std::isfinite(B[i])) return fail("%s: B[%d][%zu] = %g is not finite", who, (int)(i / n), i % n, B[i]);
    HIP_TRY(hipMemcpyAsync(w.B, B, (size_t)K * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (reml_solve_dev(w, K, delta, tol, max_iters, iters, relres)) return 1;
    std::vector<double> out((size_t)K * n);
    HIP_TRY(hipMemcpyAsync(out.data(), w.V, (size_t)K * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (reml_close(w)) return 1;
    std::copy(out.begin(), out.end(), V);
    return 0;
}

extern "C" int hgibbs_reml_eval(hgibbs_t h, int T, int q, const double* Z, const double* y, uint64_t seed, double delta, double tol, int max_iters,
                                double* sums, int* iters)
{
    static const char* who = "hgibbs_reml_eval";
    if (op_guard(h, who, "the panel products are not summed over ranks")) return 1;
    if (T < 1 || T > RM_KMAX - 1) return fail("%s: trials = %d, must be in [1, %d]", who, T, RM_KMAX - 1);
    if (!y || !sums) return fail("%s: null argument", who);
    if (reml_scalar_guard(who, delta, tol, max_iters)) return 1;
    const uint32_t n = h->n_local;
    h->reml_ms[0] = h->reml_ms[1] = 0.0;
    RemlWork w;
    if (reml_setup(w, h, who, T + 1, q, Z, true)) return 1;
    for (uint32_t i = 0; i < n; ++i)
        if (!std::isfinite(y[i])) return fail("%s: y[%u] = %g is not finite", who, i, y[i]);
    if (reml_probes(w, T, seed, y)) return 1;
    double s[3 * RM_KMAX];
    int mx = 0;
    if (reml_eval_dev(w, T, delta, tol, max_iters, s, &mx)) return 1;
    if (reml_close(w)) return 1;
    std::copy(s, s + 3 * (T + 1), sums);
    if (iters) *iters = mx;
    return 0;
}

extern "C" int hgibbs_reml(hgibbs_t h, const hgibbs_reml_opts* opt, int q, const double* Z, const double* y, hgibbs_reml_result* res, double* blup)
{
    static const char* who = "hgibbs_reml";
    if (op_guard(h, who, "the panel products are not summed over ranks")) return 1;
    if (!opt || !y || !res) return fail("%s: null argument", who);
    const int T = opt->trials;
    if (T < 1 || T > RM_KMAX - 1) return fail("%s: trials = %d, must be in [1, %d]", who, T, RM_KMAX - 1);
    if (!(opt->h2_start > 0.0) || !(opt->h2_start < 1.0)) return fail("%s: h2_start = %g, must lie inside (0, 1)", who, opt->h2_start);
    if (reml_scalar_guard(who, 1.0, opt->cg_tol, opt->cg_iters)) return 1;
    if (!(opt->x_tol > 0.0) || !std::isfinite(opt->x_tol)) return fail("%s: x_tol = %g, must be positive and finite", who, opt->x_tol);
    if (opt->max_steps < 2 || opt->max_steps > HGIBBS_REML_MAX_STEPS)
        return fail("%s: max_steps = %d, must be in [2, %d]", who, opt->max_steps, HGIBBS_REML_MAX_STEPS);
    const uint32_t n = h->n_local, M = h->M;
    h->reml_ms[0] = h->reml_ms[1] = 0.0;
    RemlWork w;
    if (reml_setup(w, h, who, T + 1, q, Z, true)) return 1;
    for (uint32_t i = 0; i < n; ++i)
        if (!std::isfinite(y[i])) return fail("%s: y[%u] = %g is not finite", who, i, y[i]);
    if (reml_probes(w, T, opt->seed, y)) return 1;

    hgibbs_reml_result r{};
    r.n = n;
    r.m_used = w.m_used;
    r.q = q;
    r.trials = T;
    const int K = T + 1;
    for (;;) {
        double xn = 0.0;
        int st = 0;
        if (hgibbs_reml_next(r.steps, r.x, r.f, opt->h2_start, opt->x_tol, opt->max_steps, &xn, &st)) return 1;
        if (st != HGIBBS_REML_CONTINUE) {
            r.status = st;
            break;
        }
        const int k = r.steps;
        std::copy(r.sums_last, r.sums_last + 3 * K, r.sums_prev);
        if (reml_eval_dev(w, T, std::exp(xn), opt->cg_tol, opt->cg_iters, r.sums_last, &r.cg_iters[k])) return 1;
        r.x[k] = xn;
        if (reml_f(r.sums_last, T, &r.f[k])) return fail("%s: f is not finite at log delta = %.9g (evaluation %d)", who, xn, k);
        r.steps = k + 1;
    }
    const double delta = std::exp(r.x[r.steps - 1]);

    // the last evaluation was made at the estimate: v_T and u_T = X'v_T are on the device
    std::vector<double> bl;
    if (blup) {
        bl.resize(M);
        HIP_TRY(hipMemcpy2DAsync(bl.data(), sizeof(double), w.T + T, (size_t)K * sizeof(double), sizeof(double), M, hipMemcpyDeviceToHost, h->stream));
    }
    // the average-information step: a = P_c A P_c v, then H z1 = a, H z2 = v
    double *dv = w.G, *da = w.E; // (the probes have served)
    HIP_TRY(hipMemcpyAsync(dv, w.V + (size_t)T * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (reml_xt(w, dv, 1)) return 1;
    if (reml_xy(w, 1)) return 1;
    if (w.clk.begin(2)) return 1;
    if (reml_project(w, w.Y, 0, 1, 0.0, nullptr, da)) return 1;
    if (w.clk.end()) return 1;
    HIP_TRY(hipMemcpyAsync(w.B, da, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(w.B + n, dv, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    int it2[RM_KMAX];
    double rel2[RM_KMAX];
    if (reml_solve_dev(w, 2, delta, opt->cg_tol, opt->cg_iters, it2, rel2)) return 1;
    r.ai_cg_iters = std::max(it2[0], it2[1]);
    {
        const uint32_t nb = (n + RM_ROWS - 1) / RM_ROWS;
        if (w.clk.begin(2)) return 1;
        k_reml_cross<<<nb, RM_TPB, 0, h->stream>>>(w.B, 2, 1, w.V, 2, 1, n, w.partial);
        HIP_TRY(hipGetLastError());
        if (reml_sum(w, nb, 4u, w.dC())) return 1;
        if (w.clk.end()) return 1;
        if (reml_read(w, w.dC(), 4)) return 1;
        r.ai3[0] = w.host[0]; // a'z1
        r.ai3[1] = w.host[1]; // a'z2
        r.ai3[2] = w.host[3]; // v'z2
    }
    if (reml_close(w)) return 1;
    const double x2[2] = {r.x[r.steps - 2], r.x[r.steps - 1]};
    if (hgibbs_reml_finish(T, n, q, x2, r.sums_prev, r.sums_last, r.ai3, &r.est)) return 1;
    r.products_ms = h->reml_ms[0];
    r.algebra_ms = h->reml_ms[1];
    if (blup) {
        std::vector<double> sd(M);
        HIP_TRY(hipMemcpy(sd.data(), h->mstd, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
        for (uint32_t j = 0; j < M; ++j) blup[j] = std::isfinite(sd[j]) ? bl[j] / (double)w.m_used : std::nan("");
    }
    *res = r;
    return 0;
}

extern "C" int hgibbs_last_reml_ms(hgibbs_t h, double* products_ms, double* algebra_ms)
{
    if (!h || !products_ms || !algebra_ms) return fail("hgibbs_last_reml_ms: null argument");
    *products_ms = h->reml_ms[0];
    *algebra_ms = h->reml_ms[1];
    return 0;
}
