// Principal components of the loaded rows: the top K eigenpairs of A = X X' / M_used over the handle's n_local
// individuals, X the chain's standardised genotypes (x = 0 at a missing call; markers without a finite mstd are outside M_used), by
// block subspace iteration on a panel of L >= K vectors with a final Rayleigh-Ritz step.  A is never formed: the two panel products
//
//     T = X'Q  (M x L)   the marker-dots pipeline (hg_mdots.hip.h), on device pointers
//     Y = X T  (n x L)   the score pipeline (hg_score.hip.h), on device pointers, with a = t mstd, o = -t mstd mave (k_pca_fold)
//
// are the exact integer operators of sections 14 and 12, bit-identical for any tiling, and every panel stays in HBM from the first
// kernel to the last: what goes to the host is L x L.
//
//   k_pca_init   the start panel when the caller gives none: entry (k, i) from mix64 of (seed, k, row i), a double in (-1, 1).
//                Counter-based: no dependence on the launch, and restated in NumPy by the tests.
//   k_pca_fold   T -> a, o (M x L -> L x M through an LDS tile, both sides coalesced); a marker without a finite mstd gets t = 0,
//                in T as well (k_mdots_final leaves NaN there).
//   k_pca_gram   P'P of a tall panel, f64, deterministic.  Workgroup w takes the PG_ROWS rows from w PG_ROWS -- a partition that
//                depends on n alone --, stages them PG_TILE at a time in LDS, and thread t owns four neighbouring entries of a row of
//                the L x L result, which it sums over the rows IN ORDER.  No sum crosses threads, so there is no tree to fix and no
//                floating-point atomic; the workgroups' partials go to a buffer that k_pca_gram_sum adds in workgroup order.
//   k_pca_apply  panel (n x L, either layout) times a small L x K matrix into a vector-major K x n panel, each entry summed over
//                l = 0 .. L - 1 in order.  With mstd given, rows without a finite mstd become NaN (the loadings).
//   k_pca_resid  D = Y / M_used - lambda_k v_k for the residuals of the report (their norms come from k_pca_gram's diagonal).
//
// Orthonormalisation is CholeskyQR done twice (G = Y'Y on the device, L x L Cholesky and triangular inverse on the host, Q = Y R^-1
// on the device, and once more); the Ritz step is a cyclic Jacobi eigensolver on the host.  Both host pieces are plain sequential
// f64 under -ffp-contract=off, so the whole call is a deterministic function of (BED, Q0 or seed, K, L, iters, tol).
#pragma once

namespace {

constexpr int PG_TPB = 256;          // threads of the panel kernels
constexpr int PG_ROWS = 1024;        // rows of the panel per workgroup of k_pca_gram (the fixed partition)
constexpr int PG_TILE = 64;          // rows staged in LDS at a time
constexpr int PG_LMAX = MD_KMAX;     // panel width at most
constexpr int PG_LD = PG_LMAX + 2;   // doubles between the rows of the LDS tile of k_pca_gram: rows stay 16-byte aligned for the
                                     // double2 reads (the staging writes of a vector-major panel still share banks)
static_assert(PG_TPB * 4 == PG_LMAX * PG_LMAX, "k_pca_gram: one thread per four entries of the result");

__global__ __launch_bounds__(PG_TPB) void k_pca_init(double* __restrict__ Q, uint32_t n, int L, uint64_t seed, uint32_t row_begin)
{
    const uint64_t e = (uint64_t)blockIdx.x * PG_TPB + threadIdx.x;
    if (e >= (uint64_t)n * (uint32_t)L) return;
    const uint64_t k = e / n, i = row_begin + e % n;
    const uint64_t hsh = mix64((seed ^ mix64(k)) + i * 0xD1B54A32D192ED03ull);
    // the top 52 bits x: (2 x + 1 - 2^52) 2^-52, an odd multiple of 2^-52 inside (-1, 1), exact
    const long long v = (long long)(2ull * (hsh >> 12) + 1ull) - (1ll << 52);
    Q[e] = ldexp((double)v, -52);
}

// block = 64 markers x L entries of T
__global__ __launch_bounds__(PG_TPB) void k_pca_fold(double* __restrict__ T, const double* __restrict__ mave, const double* __restrict__ mstd,
                                                     uint32_t M, int L, double* __restrict__ a, double* __restrict__ o)
{
    __shared__ double tile[64 * (PG_LMAX + 1)];
    const uint32_t j0 = blockIdx.x * 64u, nj = min(64u, M - j0);
    for (uint32_t idx = threadIdx.x; idx < nj * (uint32_t)L; idx += PG_TPB) {
        const uint32_t jj = idx / (uint32_t)L, l = idx % (uint32_t)L;
        double t = T[(size_t)j0 * L + idx];
        if (!isfinite(mstd[j0 + jj])) {
            t = 0.0;
            T[(size_t)j0 * L + idx] = 0.0;
        }
        tile[jj * (PG_LMAX + 1) + l] = t;
    }
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < 64u * (uint32_t)L; idx += PG_TPB) {
        const uint32_t l = idx / 64u, jj = idx % 64u;
        if (jj >= nj) continue;
        const double sd = mstd[j0 + jj];
        const bool used = isfinite(sd); // (a marker missing everywhere has a NaN mave as well)
        const double w = used ? tile[jj * (PG_LMAX + 1) + l] * sd : 0.0;
        a[(size_t)l * M + j0 + jj] = w;
        o[(size_t)l * M + j0 + jj] = used ? -(w * mave[j0 + jj]) : 0.0;
    }
}

// entry (i, l) of the panel: P[i L + l] (vecmajor = 0) or P[l n + i] (vecmajor = 1).  Thread t owns the entries (a, b .. b + 3) of
// the result, a = t / 8, b = 4 (t % 8): per row one broadcast read of column a and two 16-byte reads of its four columns.
__global__ __launch_bounds__(PG_TPB) void k_pca_gram(const double* __restrict__ P, uint32_t n, int L, int vecmajor, double* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) double tile[PG_TILE * PG_LD];
    const uint32_t tid = threadIdx.x, uL = (uint32_t)L, LL = uL * uL;
    const uint32_t r0 = blockIdx.x * PG_ROWS, r1 = min(n, r0 + PG_ROWS);
    const uint32_t ea = tid >> 3, eb = 4u * (tid & 7u);
    const bool active = ea < uL && eb < uL;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t idx = tid; idx < (uint32_t)(PG_TILE * PG_LD); idx += PG_TPB) tile[idx] = 0.0; // (the columns from L on stay zero)
    __syncthreads();
    for (uint32_t t0 = r0; t0 < r1; t0 += PG_TILE) {
        const uint32_t nr = min((uint32_t)PG_TILE, r1 - t0);
        if (vecmajor) {
            for (uint32_t idx = tid; idx < (uint32_t)PG_TILE * uL; idx += PG_TPB) {
                const uint32_t l = idx / PG_TILE, r = idx % PG_TILE;
                tile[r * PG_LD + l] = r < nr ? P[(size_t)l * n + t0 + r] : 0.0;
            }
        } else {
            for (uint32_t idx = tid; idx < (uint32_t)PG_TILE * uL; idx += PG_TPB) {
                const uint32_t r = idx / uL, l = idx % uL;
                tile[r * PG_LD + l] = r < nr ? P[(size_t)t0 * uL + idx] : 0.0;
            }
        }
        __syncthreads();
        if (active) {
            for (uint32_t r = 0; r < nr; ++r) { // (in order: the sum of an entry never leaves its thread)
                const double* row = tile + r * PG_LD;
                const double x = row[ea];
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
        if (eb + c < uL) partial[(size_t)blockIdx.x * LL + ea * uL + eb + c] = acc[c];
}

// the workgroups' partials in workgroup order
__global__ __launch_bounds__(PG_TPB) void k_pca_gram_sum(const double* __restrict__ partial, uint32_t nb, uint32_t LL, double* __restrict__ out)
{
    const uint32_t e = blockIdx.x * PG_TPB + threadIdx.x;
    if (e >= LL) return;
    double s = 0.0;
    uint32_t w = 0;
    for (; w + 8u <= nb; w += 8u) { // eight loads in flight, added in workgroup order
        double v[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) v[u] = partial[(size_t)(w + u) * LL + e];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) s += v[u];
    }
    for (; w < nb; ++w) s += partial[(size_t)w * LL + e];
    out[e] = s;
}

// out[k n + i] = sum_l P(i, l) B[l K + k], l in order; one thread per row
__global__ __launch_bounds__(PG_TPB) void k_pca_apply(const double* __restrict__ P, uint32_t n, int L, int vecmajor, const double* __restrict__ B,
                                                      int K, const double* __restrict__ mstd, double* __restrict__ out)
{
    __shared__ double sB[PG_LMAX * PG_LMAX];
    for (uint32_t idx = threadIdx.x; idx < (uint32_t)(L * K); idx += PG_TPB) sB[idx] = B[idx];
    __syncthreads();
    const uint32_t i = blockIdx.x * PG_TPB + threadIdx.x;
    if (i >= n) return;
    double r[PG_LMAX];
#pragma unroll
    for (int l = 0; l < PG_LMAX; ++l) r[l] = l < L ? (vecmajor ? P[(size_t)l * n + i] : P[(size_t)i * L + l]) : 0.0;
    const bool off = mstd && !isfinite(mstd[i]);
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
#pragma unroll
        for (int l = 0; l < PG_LMAX; ++l)
            if (l < L) s += r[l] * sB[l * K + k];
        out[(size_t)k * n + i] = off ? __builtin_nan("") : s;
    }
}

// D[i K + k] = Y[i K + k] / m - lam[k] V[k n + i]
__global__ __launch_bounds__(PG_TPB) void k_pca_resid(const double* __restrict__ Y, const double* __restrict__ V, const double* __restrict__ lam,
                                                      uint32_t n, int K, double m, double* __restrict__ D)
{
    const uint64_t e = (uint64_t)blockIdx.x * PG_TPB + threadIdx.x;
    if (e >= (uint64_t)n * (uint32_t)K) return;
    const uint32_t i = (uint32_t)(e / (uint32_t)K), k = (uint32_t)(e % (uint32_t)K);
    D[e] = Y[e] / m - lam[k] * V[(size_t)k * n + i];
}

// G = R'R, R upper triangular; returns the index of the first pivot that is not safely positive, or -1.  Rinv = R^-1 (row-major).
int pca_chol_inv(const double* G, int L, double* Rinv, double* pivot)
{
    std::vector<double> R((size_t)L * L, 0.0);
    for (int j = 0; j < L; ++j) {
        double d = G[j * L + j];
        for (int k = 0; k < j; ++k) d -= R[k * L + j] * R[k * L + j];
        if (!(d > 1e-13 * G[j * L + j]) || !std::isfinite(d)) {
            *pivot = d;
            return j;
        }
        const double rjj = std::sqrt(d);
        R[j * L + j] = rjj;
        for (int c = j + 1; c < L; ++c) {
            double s = G[j * L + c];
            for (int k = 0; k < j; ++k) s -= R[k * L + j] * R[k * L + c];
            R[j * L + c] = s / rjj;
        }
    }
    for (int i = 0; i < L * L; ++i) Rinv[i] = 0.0;
    for (int c = 0; c < L; ++c) { // column c of the inverse by back substitution
        Rinv[c * L + c] = 1.0 / R[c * L + c];
        for (int r = c - 1; r >= 0; --r) {
            double s = 0.0;
            for (int k = r + 1; k <= c; ++k) s -= R[r * L + k] * Rinv[k * L + c];
            Rinv[r * L + c] = s / R[r * L + r];
        }
    }
    return -1;
}

// Cyclic Jacobi on a symmetric L x L matrix: S = W diag(theta) W', theta descending, W[l L + k] = component l of vector k; false
// when the off-diagonal part has not fallen below rounding after 60 sweeps (a matrix of this size takes fewer than ten)
bool pca_jacobi(const double* S, int L, double* theta, double* W)
{
    std::vector<double> A(S, S + (size_t)L * L), V((size_t)L * L, 0.0);
    for (int i = 0; i < L; ++i) V[i * L + i] = 1.0;
    for (int i = 0; i < L; ++i)
        for (int j = i + 1; j < L; ++j) A[i * L + j] = A[j * L + i] = 0.5 * (A[i * L + j] + A[j * L + i]);
    bool done = false;
    for (int sweep = 0; sweep <= 60 && !done; ++sweep) {
        double offd = 0.0, diag = 0.0;
        for (int i = 0; i < L; ++i) {
            diag += A[i * L + i] * A[i * L + i];
            for (int j = i + 1; j < L; ++j) offd += A[i * L + j] * A[i * L + j];
        }
        if (!(offd > 1e-34 * diag)) {
            done = true;
            break;
        }
        if (sweep == 60) break;
        for (int p = 0; p < L - 1; ++p)
            for (int q = p + 1; q < L; ++q) {
                const double apq = A[p * L + q];
                if (apq == 0.0) continue;
                const double tau = (A[q * L + q] - A[p * L + p]) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < L; ++k) { // columns p, q
                    const double akp = A[k * L + p], akq = A[k * L + q];
                    A[k * L + p] = c * akp - s * akq;
                    A[k * L + q] = s * akp + c * akq;
                }
                for (int k = 0; k < L; ++k) { // rows p, q
                    const double apk = A[p * L + k], aqk = A[q * L + k];
                    A[p * L + k] = c * apk - s * aqk;
                    A[q * L + k] = s * apk + c * aqk;
                }
                A[p * L + q] = A[q * L + p] = 0.0;
                for (int k = 0; k < L; ++k) {
                    const double vkp = V[k * L + p], vkq = V[k * L + q];
                    V[k * L + p] = c * vkp - s * vkq;
                    V[k * L + q] = s * vkp + c * vkq;
                }
            }
    }
    std::vector<int> ord(L);
    for (int i = 0; i < L; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return A[x * L + x] > A[y * L + y]; });
    for (int k = 0; k < L; ++k) {
        theta[k] = A[ord[k] * L + ord[k]];
        for (int l = 0; l < L; ++l) W[l * L + k] = V[l * L + ord[k]];
    }
    return done;
}

// device time by part: a fixed pool of event pairs recorded around the stream-ordered segments and read at the call's own
// synchronisation points (at most a handful of segments lie between two of them), so the timing adds no synchronisation
struct PcaClock {
    static constexpr int NSEG = 8;
    Event ev[2 * NSEG];
    int part[NSEG] = {};
    int used = 0; // events recorded since the last sync
    hipStream_t stream = nullptr;
    double ms[5] = {0, 0, 0, 0, 0};
    int create()
    {
        for (auto& e : ev)
            if (e.create()) return 1;
        return 0;
    }
    int begin(int p)
    {
        if (used + 2 > 2 * NSEG) return fail("hgibbs_pca: out of timing events");
        part[used / 2] = p;
        HIP_TRY(hipEventRecord(ev[used++], stream));
        return 0;
    }
    int end()
    {
        HIP_TRY(hipEventRecord(ev[used++], stream));
        return 0;
    }
    int sync() // the stream's synchronisation, then the segments that ended before it
    {
        HIP_TRY(hipStreamSynchronize(stream));
        for (int s = 0; 2 * s + 1 < used; ++s) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, ev[2 * s], ev[2 * s + 1]));
            ms[part[s]] += t;
            ms[0] += t;
        }
        used = 0;
        return 0;
    }
};

struct PcaBufs {
    DevBuf<double> Q, Q1, Y, T, a, o, partial, small, out;
};

// P'P (n x L panel) into dG (device, L x L): the partials, then their sum
int pca_gram(hgibbs_ctx* h, PcaBufs& b, const double* P, uint32_t n, int L, int vecmajor, double* dG)
{
    const uint32_t nb = (n + PG_ROWS - 1) / PG_ROWS, LL = (uint32_t)(L * L);
    k_pca_gram<<<nb, PG_TPB, 0, h->stream>>>(P, n, L, vecmajor, b.partial);
    HIP_TRY(hipGetLastError());
    k_pca_gram_sum<<<(LL + PG_TPB - 1) / PG_TPB, PG_TPB, 0, h->stream>>>(b.partial, nb, LL, dG);
    HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace

extern "C" int hgibbs_pca(hgibbs_t h, int K, int L, int iters, double tol, const double* Q0, uint64_t seed, double* eigval, double* pcs,
                          double* loadings, hgibbs_pca_report* rep)
{
    if (op_guard(h, "hgibbs_pca", "the panel products are not summed over ranks")) return 1;
    if (K < 1) return fail("hgibbs_pca: K = %d, needs at least one component", K);
    if (K > L) return fail("hgibbs_pca: K = %d above the panel width L = %d", K, L);
    if (L > PG_LMAX) return fail("hgibbs_pca: L = %d, at most %d vectors in the panel", L, PG_LMAX);
    if (iters < 1) return fail("hgibbs_pca: iters = %d, needs at least one iteration", iters);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail("hgibbs_pca: tol = %g, must be finite and not negative", tol);
    if (!eigval || !pcs) return fail("hgibbs_pca: null argument");
    const uint32_t n = h->n_local, M = h->M;
    if (n >= MD_NMAX) return fail("hgibbs_pca: %u individuals, at most %u (64-bit sums of the marker dots)", n, MD_NMAX - 1u);
    if ((uint32_t)L >= n) return fail("hgibbs_pca: L = %d, must be below the %u individuals", L, n);
    if (Q0)
        for (size_t i = 0; i < (size_t)L * n; ++i)
            if (!std::isfinite(Q0[i])) return fail("hgibbs_pca: Q0[%d][%zu] = %g is not finite", (int)(i / n), i % n, Q0[i]);
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;
    uint32_t m_used = 0;
    {
        std::vector<double> sd(M);
        HIP_TRY(hipMemcpy(sd.data(), h->mstd, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
        for (uint32_t j = 0; j < M; ++j) m_used += std::isfinite(sd[j]) ? 1u : 0u;
    }
    if ((uint32_t)L > m_used) return fail("hgibbs_pca: L = %d above the %u markers with a finite standard deviation", L, m_used);
    for (int i = 0; i < 5; ++i) h->pca_ms[i] = 0.0;

    // device memory: the panels Q, Q1, Y (n x L each), T (M x L), a, o (L x M each), the partials of k_pca_gram, the outputs, and the
    // two pipelines' work buffers
    const size_t nL = (size_t)n * L, ML = (size_t)M * L, big = std::max(n, M);
    const size_t nbmax = (big + PG_ROWS - 1) / PG_ROWS;
    const size_t outn = loadings ? (size_t)K * M : 0;
    const size_t bytes = (3 * nL + 3 * ML + nbmax * L * L + outn + 8 * PG_LMAX * PG_LMAX) * sizeof(double) + mdots_ws_bytes(h, L, M) + score_ws_bytes(h, L);
    if (need_device_memory(bytes, "hgibbs_pca: the panels and work buffers need %.1f MiB", bytes / 1048576.0)) return 1;
    PcaBufs b;
    MdotsWs mw;
    ScoreWs sw;
    PcaClock clk;
    clk.stream = h->stream;
    if (b.Q.alloc(nL) || b.Q1.alloc(nL) || b.Y.alloc(nL) || b.T.alloc(ML) || b.a.alloc(ML) || b.o.alloc(ML)) return 1;
    if (b.partial.alloc(nbmax * L * L) || b.small.alloc(8 * PG_LMAX * PG_LMAX)) return 1;
    if (loadings && b.out.alloc(outn)) return 1;
    if (mdots_ws_create(h, mw, L, M)) return 1;
    if (score_ws_create(h, sw, L)) return 1;
    if (clk.create()) return 1;
    double* dG = b.small;                              // an L x L matrix on its way to the host
    double* dB = b.small + PG_LMAX * PG_LMAX;          // an L x L matrix from the host
    double* dlam = b.small + 2 * PG_LMAX * PG_LMAX;    // K eigenvalues
    const int LL = L * L;
    std::vector<double> G(LL), B(LL), S(LL), W(LL), theta(L), prev(L, 0.0);

    // part: 1 = X'Q products, 2 = X T products, 3 = panel algebra of the iterations, 4 = start panel, final step and residuals
    // Orthonormalises src (n x L, either layout) into b.Q (vector-major): CholeskyQR, twice
    auto orth = [&](const double* src, int vecmajor, int part, int it) -> int {
        for (int round = 0; round < 2; ++round) {
            const double* in = round == 0 ? src : b.Q1;
            const int vm = round == 0 ? vecmajor : 1;
            if (round == 0) {
                if (clk.begin(part)) return 1;
            }
            if (pca_gram(h, b, in, n, L, vm, dG)) return 1;
            if (clk.end()) return 1;
            HIP_TRY(hipMemcpyAsync(G.data(), dG, LL * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            if (clk.sync()) return 1;
            double piv = 0.0;
            const int badp = pca_chol_inv(G.data(), L, B.data(), &piv);
            if (badp >= 0)
                return fail("hgibbs_pca: the panel lost rank in iteration %d: pivot %d of the Cholesky factor of its Gram matrix is %g against a diagonal of %g "
                            "(linearly dependent start vectors, or fewer independent rows than L)",
                            it, badp, piv, G[badp * L + badp]);
            HIP_TRY(hipMemcpyAsync(dB, B.data(), LL * sizeof(double), hipMemcpyHostToDevice, h->stream));
            if (clk.begin(part)) return 1;
            k_pca_apply<<<(n + PG_TPB - 1) / PG_TPB, PG_TPB, 0, h->stream>>>(in, n, L, vm, dB, L, nullptr, round == 0 ? b.Q1 : b.Q);
            HIP_TRY(hipGetLastError());
            if (round == 1) {
                if (clk.end()) return 1;
            }
        }
        return 0;
    };
    // T = X'Q for nv vectors of V (vector-major), NaN rows zeroed and folded into a, o; then optionally S = T'T to the host
    auto xt = [&](const double* V, int nv, int part, int part_alg, bool want_s) -> int {
        if (mdots_dev_clear(h, mw, M, nv)) return 1;
        if (clk.begin(part)) return 1;
        if (mdots_dev_run(h, mw, 0, M, nv, V, b.T, nullptr)) return 1;
        if (clk.end()) return 1;
        if (clk.begin(part_alg)) return 1;
        k_pca_fold<<<(M + 63u) / 64u, PG_TPB, 0, h->stream>>>(b.T, h->mave, h->mstd, M, nv, b.a, b.o);
        HIP_TRY(hipGetLastError());
        if (want_s && pca_gram(h, b, b.T, M, nv, 0, dG)) return 1;
        if (clk.end()) return 1;
        if (want_s) {
            HIP_TRY(hipMemcpyAsync(S.data(), dG, (size_t)nv * nv * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            if (clk.sync()) return 1;
        }
        return 0;
    };
    auto xy = [&](int nv, int part) -> int { // Y = X T from the folded weights
        if (score_dev_clear(h, sw, nv, false)) return 1; // (the flag of non-finite weights gathers over every product)
        if (clk.begin(part)) return 1;
        if (score_dev_run(h, sw, nv, b.a, b.o, b.Y)) return 1;
        if (clk.end()) return 1;
        return 0;
    };

    // 1. the start panel, in Y's memory (vector-major), orthonormalised into Q
    if (Q0) {
        HIP_TRY(hipMemcpyAsync(b.Y, Q0, nL * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else {
        if (clk.begin(4)) return 1;
        k_pca_init<<<(uint32_t)((nL + PG_TPB - 1) / PG_TPB), PG_TPB, 0, h->stream>>>(b.Y, n, L, seed, h->row_begin);
        HIP_TRY(hipGetLastError());
        if (clk.end()) return 1;
    }
    if (orth(b.Y, 1, 4, 0)) return 1;

    int it = 0;
    double change = HUGE_VAL;
    for (;;) {
        ++it;
        if (xt(b.Q, L, 1, 3, true)) return 1;          // 2. T = X'Q, 3. S = T'T
        if (!pca_jacobi(S.data(), L, theta.data(), W.data()))
            return fail("hgibbs_pca: the Jacobi eigensolver of the %d x %d Ritz matrix did not converge in iteration %d (a panel entry that is not finite?)", L, L, it);
        for (int k = 0; k < K; ++k)
            if (!(theta[k] > 0.0) || !std::isfinite(theta[k])) return fail("hgibbs_pca: Ritz value %d is %g in iteration %d", k + 1, theta[k], it);
        if (it > 1) {
            change = 0.0;
            for (int k = 0; k < K; ++k) change = std::max(change, std::fabs(theta[k] - prev[k]) / theta[k]);
        }
        prev = theta;
        if (it >= iters || (tol > 0.0 && it > 1 && change <= tol)) break;
        if (xy(L, 2)) return 1;                         //    Y = X T
        if (orth(b.Y, 0, 3, it)) return 1;              // 4. Q = orth(Y)
    }

    // 5. Rayleigh-Ritz: pcs = Q W, loadings = T W / sqrt(theta)
    std::vector<double> lam(K);
    for (int k = 0; k < K; ++k) lam[k] = theta[k] / (double)m_used;
    for (int l = 0; l < L; ++l)
        for (int k = 0; k < K; ++k) B[l * K + k] = W[l * L + k];
    HIP_TRY(hipMemcpyAsync(dB, B.data(), (size_t)L * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (clk.begin(4)) return 1;
    k_pca_apply<<<(n + PG_TPB - 1) / PG_TPB, PG_TPB, 0, h->stream>>>(b.Q, n, L, 1, dB, K, nullptr, b.Q1); // (Q1: K x n, the PCs)
    HIP_TRY(hipGetLastError());
    if (clk.end()) return 1;
    HIP_TRY(hipMemcpyAsync(pcs, b.Q1, (size_t)K * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (clk.sync()) return 1;
    if (loadings) {
        for (int l = 0; l < L; ++l)
            for (int k = 0; k < K; ++k) B[l * K + k] = W[l * L + k] / std::sqrt(theta[k]);
        HIP_TRY(hipMemcpyAsync(dB, B.data(), (size_t)L * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (clk.begin(4)) return 1;
        k_pca_apply<<<(M + PG_TPB - 1) / PG_TPB, PG_TPB, 0, h->stream>>>(b.T, M, L, 0, dB, K, h->mstd, b.out);
        HIP_TRY(hipGetLastError());
        if (clk.end()) return 1;
        HIP_TRY(hipMemcpyAsync(loadings, b.out, (size_t)K * M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (clk.sync()) return 1;
    }
    // sign: the entry of largest magnitude of each PC is positive (the lowest index on a tie)
    for (int k = 0; k < K; ++k) {
        double* v = pcs + (size_t)k * n;
        uint32_t at = 0;
        for (uint32_t i = 1; i < n; ++i)
            if (std::fabs(v[i]) > std::fabs(v[at])) at = i;
        if (v[at] < 0.0) {
            for (uint32_t i = 0; i < n; ++i) v[i] = -v[i];
            if (loadings)
                for (uint32_t j = 0; j < M; ++j) loadings[(size_t)k * M + j] = -loadings[(size_t)k * M + j];
        }
        eigval[k] = lam[k];
    }
    if (rep) {
        rep->iters_run = it;
        rep->m_used = m_used;
        rep->ritz_change = change;
        for (int k = 0; k < 32; ++k) rep->resid[k] = 0.0;
        // resid_k = |A v_k - lambda_k v_k| / lambda_k from one more pair of products on the PCs (Q1, K x n)
        if (xt(b.Q1, K, 4, 4, false)) return 1;
        if (xy(K, 4)) return 1;
        HIP_TRY(hipMemcpyAsync(dlam, lam.data(), (size_t)K * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (clk.begin(4)) return 1;
        k_pca_resid<<<(uint32_t)(((size_t)n * K + PG_TPB - 1) / PG_TPB), PG_TPB, 0, h->stream>>>(b.Y, b.Q1, dlam, n, K, (double)m_used, b.Q);
        HIP_TRY(hipGetLastError());
        if (pca_gram(h, b, b.Q, n, K, 0, dG)) return 1;
        if (clk.end()) return 1;
        HIP_TRY(hipMemcpyAsync(G.data(), dG, (size_t)K * K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (clk.sync()) return 1;
        for (int k = 0; k < K; ++k) rep->resid[k] = std::sqrt(G[k * K + k]) / lam[k];
    }
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, sw.bad, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (clk.sync()) return 1;
    if (bad) return fail("hgibbs_pca: a panel entry is not finite (a weight of one of the X T products)");
    for (int i = 0; i < 5; ++i) h->pca_ms[i] = clk.ms[i];
    return 0;
}

extern "C" int hgibbs_last_pca_ms(hgibbs_t h, double* ms4)
{
    if (!h || !ms4) return fail("hgibbs_last_pca_ms: null argument");
    for (int i = 0; i < 4; ++i) ms4[i] = h->pca_ms[i];
    return 0;
}
