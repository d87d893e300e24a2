// Dots of the loaded markers against dense vectors over the individuals: for markers j in [m0, m0 + count)
// and K vectors u_k over the handle's n_local individuals, the exact integer sums
//
//     P_jk = sum_{i called} g_ij q_ik,   Q_jk = sum_{i called} q_ik,      q_ik = round(u_ik 2^E_k)
//
// and from them, each rounded to f64 ONCE, x_j'u_k = mstd_j (P_jk - mave_j Q_jk) with the chain's own standardisation.  This is the
// refill's product x_j'eps (hg_streamer2.hip.h) as a standalone operator for K vectors: the digits of u against the BED codes on
// v_mfma_i32_16x16x64_i8.
//
//   scale    one per vector, as hgibbs_score takes it (k_score_max, k_score_ksum): E_k = 52 - e_k with max_i |u_ik| < 2^e_k (0 for an
//            all-zero vector), q = llrint(u 2^E_k), |q| <= 2^52, in seven signed base-256 digits (sc_quant, sc_digit).  The only error
//            is that rounding: |P 2^-E_k - sum g u| <= n 2^-E_k <= 2 n max|u_k| 2^-52 and |Q 2^-E_k - sum u| <= n max|u_k| 2^-52,
//            each before its one rounding to f64.  k_score_ksum also gives sum_{i < n_local} q_ik exactly (two 64-bit halves).
//   A        (16 rows x 64 individuals, bytes): the digits of two vectors.  Rows 0..6 hold vector 2 t, rows 8..14 vector 2 t + 1, rows
//            7 and 15 are zero; byte order of rl_expand16 (dword q, byte i = individual 4 i + q of the sixteen of a dword).  k_mdots_digits
//            writes this image once per call in HBM: [slice of 512 individuals][tile t][k-step s][lane] 16 bytes, zero past n_local.
//   B        (64 individuals x 16 markers): lane (c, g) of k-step s expands ONE stored BED dword of marker c, dword 8 g + s of the slice
//            (the lane loads its eight dwords of the slice as two 16-byte loads).  No transpose: this is hg_ld.hip.h's operand.
//   D        (i32): lane (c, g), register r = digit (4 g + r) mod 8 of vector 2 t + (g >> 1) against marker c.  The lane puts its four
//            digits together (d0 + 2^8 d1 + 2^16 d2 + 2^24 d3, |.| < 2^56) and adds them to the pair's low (g even) or high (g odd: units
//            of 2^32) 64-bit sum by an atomic add, as k_score does: |P| 2^E can exceed 2^64, the two halves do not.
//   missing  the first product counts a missing call (code 3) as 3; in 16-marker tiles that hold a column with missing calls (the
//            marker-stats nmiss) a second product of the same digits against the indicator bytes [code == 3] gives R = sum_missing q.
//            Then P = D - 3 R and Q = sum_all q - R (k_mdots_final).  The second product is compiled only into k_mdots<.., true>,
//            launched only when some column of the handle has missing calls.
//   padding  BED slots past n_local are code 3, but they meet zero digits: they add nothing to D or R.
//   exact    every i32 partial is a sum of |digit| x code <= 128 x 3 over the individuals of the workgroup's range; the host caps a
//            range at MD_SUB_MAX slices (2^22 individuals: 384 x 2^22 < 2^31), so no partial overflows before it leaves for the
//            64-bit sums.  n_local < 2^29 keeps the final halves (|lo| < 2 n 2^31.01) inside an int64; the adds themselves wrap
//            harmlessly (modular).  Integer sums do not depend on tiling, workgroups, the individual split (option mdots_split),
//            m0 / count chunking or launch order: the results are bit-identical across all of them.
//   reuse    workgroup = MD_WAVES waves x MT marker tiles (MT = 4 at TP <= 2: 256 markers), TP vector tiles a pass.  Per slice of 512
//            individuals the workgroup stages TP x 8 KB of digits in LDS (double-buffered, one barrier a slice) for all its markers:
//            32 bytes of digits per marker and tile against 128 bytes of codes, 1/4 at K <= 2.  K > 8 takes ceil(K / 8) passes.
//
// The frame.  Everything above but the product itself is shared by the operators on the digit image (k_mdots here, k_mclass in
// hg_mclass.hip.h), on either side of the launch:
//
//   md_frame      (device) the workgroup's range and tiles, the staging of the digits, the prefetch of the codes, the slice loop with
//                 its barrier, and the walk over (marker, vector) at the end.  A kernel owns its accumulators and gives two
//                 lambdas: the products of one slice, and what to add at one (marker tile m, vector tile t).
//   md_dword, md_join, md_add   the dword of a k-step, four digit registers as one 64-bit value, the atomic add of a non-zero
//                 value; k_sgram (hg_sgram.hip.h), which has no LDS stage and a loop of its own, takes only these.
//   digit_image   (host) k_score_max, k_score_ksum, k_mdots_digits: the scales, sum_i q and the image of K vectors.
//   md_passes     (host) the passes of at most MD_TPMAX vector tiles: per pass the build (from the operator's table, by tiles in
//                 the pass and h->any_missing), the grid and the ranges of individuals (mdots_split, MD_SUB_MAX).
//   kvec_guard    (host) the refusals of an entry point that takes K vectors against markers [m0, m0 + count).
#pragma once

namespace {

constexpr int MD_WAVES = 4;                  // waves per workgroup
constexpr int MD_SUBD = 32;                  // dwords of a column per slice: 512 individuals, 128 bytes, eight k-steps
constexpr int MD_SUBI = MD_SUBD * 16;        // individuals per slice
constexpr int MD_TPMAX = 4;                  // vector tiles per pass (the LDS staging: 2 x 4 x 8 KB = 64 KB)
constexpr int MD_KMAX = 32;                  // vectors per call at most (16 tiles: four passes)
constexpr uint32_t MD_SUB_MAX = 8192;        // slices per workgroup at most (i32 headroom, above)
constexpr uint32_t MD_NMAX = 1u << 29;       // n_local below this keeps the final 64-bit halves exact
constexpr int MD_TPB = 256;                  // threads of the helper kernels

constexpr int md_mt(int TP) { return TP <= 2 ? 4 : 2; } // marker tiles per wave

// The digit image: block (s8, t) = (k-step of the whole column, tile), lane (r, g): digit r & 7 of vector 2 t + (r >> 3) over the
// sixteen individuals of dword 8 g + (s8 % 8) of slice s8 / 8
__global__ __launch_bounds__(64) void k_mdots_digits(const double* __restrict__ U, uint32_t n_local, int K, int tiles,
                                                     const int* __restrict__ scale, rl_v4i* __restrict__ img)
{
    const uint32_t s8 = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const uint32_t r = lane & 15u, g = lane >> 4, d = r & 7u;
    const uint32_t k = 2u * t + (r >> 3);
    const uint32_t sub = s8 / 8u, s = s8 % 8u;
    rl_v4i w = {0, 0, 0, 0};
    if (k < (uint32_t)K && d < 7u) {
        const int E = scale[k];
        const uint64_t i0 = ((uint64_t)sub * MD_SUBD + 8u * g + s) * 16u; // first individual of the dword
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t wq = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint64_t ind = i0 + 4u * (uint32_t)i + (uint32_t)q;
                if (ind >= n_local) continue;
                wq |= (uint32_t)(uint8_t)sc_digit(sc_quant(U[(size_t)k * n_local + ind], E), (int)d) << (8 * i);
            }
            w[q] = (int)wq;
        }
    }
    img[(((size_t)sub * tiles + t) * 8u + s) * 64u + lane] = w;
}

// dword s of the eight a lane holds of a slice
__device__ __forceinline__ uint32_t md_dword(const uint4 (&w)[2], int s)
{
    const uint4 v = w[s >> 2];
    return (s & 3) == 0 ? v.x : (s & 3) == 1 ? v.y : (s & 3) == 2 ? v.z : v.w;
}

// four digit registers as one value: d0 + 2^8 d1 + 2^16 d2 + 2^24 d3
__device__ __forceinline__ long long md_join(const rl_v4i& a)
{
    return (long long)a[0] + ((long long)a[1] << 8) + ((long long)a[2] << 16) + ((long long)a[3] << 24);
}

__device__ __forceinline__ void md_add(unsigned long long* p, long long v)
{
    if (v) __hip_atomic_fetch_add(p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The frame of a product on the digit image, with the kernel's own arguments.  Workgroup (x, y): marker tiles tw + 0 .. MT - 1 for
// wave w, tw = t0 + MT (MD_WAVES x + w); slices [y sub_per, (y + 1) sub_per) of the n_sub; vector tiles tv0 .. tv0 + ntp - 1
// (ntp <= TP) of the image's `tiles`.  Per slice it calls
//     slice(st, cw, tm)    st: the staged digits at this lane, tile t of k-step s at st[(t * 8 + s) * 64]; cw[m]: the lane's eight
//                          dwords of marker 16 (tw + m) + c (zero past M); tm[m]: MISS and tile tw + m holds a column with missing
//                          calls (wave-uniform).  Only waves with a tile below t1 get the call.
// and at the end, for every (m, t) whose marker j lies in [m0, m0 + count) and whose vector k = 2 (tv0 + t) + (g >> 1) is below K,
//     out(m, t, tm[m], p)  p = acc + ((j - m0) K + k) W + (g & 1): the lane's half (low at g even, high at g odd) of the first of
//                          the entry's W 64-bit sums.  Lane (c, g), tile t, register r holds digit (4 g + r) mod 8 of that vector
//                          against that marker.
template <int TP, bool MISS, int W, class Slice, class Out>
__device__ __forceinline__ void md_frame(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t M, uint32_t t0, uint32_t t1,
                                         uint32_t sub_per, uint32_t n_sub, const rl_v4i* __restrict__ img, int tiles, int tv0, int ntp,
                                         int K, const uint8_t* __restrict__ tmiss, uint32_t m0, uint32_t count,
                                         unsigned long long* __restrict__ acc, Slice&& slice, Out&& out)
{
    constexpr int MT = md_mt(TP);
    constexpr int NU = TP * 8 * 64;                   // 16-byte units of digits per slice
    constexpr int UPT = NU / (MD_WAVES * 64);         // of them per thread when staging
    __shared__ rl_v4i stage[2][NU];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t s0 = blockIdx.y * sub_per, s1 = min(n_sub, s0 + sub_per);
    if (s0 >= s1) return; // (uniform)
    const uint32_t tw = t0 + (uint32_t)MT * (MD_WAVES * blockIdx.x + wave); // this wave's first marker tile
    const bool wave_on = tw < t1;                                            // (wave-uniform)
    const uint32_t c = lane & 15u, g = lane >> 4;
    const uint32_t nu = (uint32_t)ntp * 8u * 64u;     // units staged

    rl_v4i pre[UPT];
    auto load_digits = [&](uint32_t sub) {
        const rl_v4i* src = img + ((size_t)sub * tiles + (uint32_t)tv0) * 8u * 64u;
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            const uint32_t u = tid + (uint32_t)k * (MD_WAVES * 64);
            pre[k] = u < nu ? src[u] : rl_v4i{0, 0, 0, 0};
        }
    };
    auto store_digits = [&](int buf) {
#pragma unroll
        for (int k = 0; k < UPT; ++k) stage[buf][tid + (uint32_t)k * (MD_WAVES * 64)] = pre[k];
    };
    uint4 cw[MT][2];
    auto load_codes = [&](uint32_t sub, uint4 (&dst)[MT][2]) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const uint32_t j = 16u * (tw + (uint32_t)m) + c;
            uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a; // (markers past M: code 0, never written out)
            if (wave_on && j < M) {
                const uint4* p = reinterpret_cast<const uint4*>(bed + (uint64_t)j * stride + (uint64_t)sub * (MD_SUBD * 4) + g * 32u);
                a = p[0];
                b = p[1];
            }
            dst[m][0] = a;
            dst[m][1] = b;
        }
    };
    bool tm[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) tm[m] = MISS && wave_on && tw + (uint32_t)m < t1 && tmiss[tw + (uint32_t)m];

    load_digits(s0);
    store_digits(0);
    load_codes(s0, cw);
    __syncthreads();
    for (uint32_t sub = s0; sub < s1; ++sub) {
        const int buf = (int)((sub - s0) & 1u);
        const bool more = sub + 1u < s1;
        uint4 nw[MT][2];
        if (more) {
            load_digits(sub + 1u);
            load_codes(sub + 1u, nw);
        }
        if (wave_on) slice(stage[buf] + lane, cw, tm);
        if (more) {
            store_digits(buf ^ 1);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                cw[m][0] = nw[m][0];
                cw[m][1] = nw[m][1];
            }
        }
        __syncthreads();
    }
    if (!wave_on) return;

#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const uint32_t j = 16u * (tw + (uint32_t)m) + c;
        if (j < m0 || j - m0 >= count || j >= M) continue;
#pragma unroll
        for (int t = 0; t < TP; ++t) {
            const uint32_t k = 2u * (uint32_t)(tv0 + t) + (g >> 1);
            if (t >= ntp || k >= (uint32_t)K) continue;
            out(m, t, tm[m], acc + ((uint64_t)(j - m0) * (uint32_t)K + k) * (uint32_t)W + (g & 1u));
        }
    }
}

// The product: the codes of a k-step stay in registers (z) for all vector tiles; A is read from the stage per tile.
// acc: [marker - m0][vector][D, R][half] 64-bit sums.
template <int TP, bool MISS>
__global__ __launch_bounds__(MD_WAVES * 64) void k_mdots(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t M, uint32_t t0,
                                                         uint32_t t1, uint32_t sub_per, uint32_t n_sub, const rl_v4i* __restrict__ img,
                                                         int tiles, int tv0, int ntp, int K, const uint8_t* __restrict__ tmiss,
                                                         uint32_t m0, uint32_t count, unsigned long long* __restrict__ acc)
{
    constexpr int MT = md_mt(TP);
    rl_v4i D[MT][TP] = {}, R[MT][MISS ? TP : 1] = {};
    md_frame<TP, MISS, 4>(
        bed, stride, M, t0, t1, sub_per, n_sub, img, tiles, tv0, ntp, K, tmiss, m0, count, acc,
        [&](const rl_v4i* st, const uint4 (&cw)[MT][2], const bool (&tm)[MT]) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                rl_v4i z[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) z[m] = rl_expand16(md_dword(cw[m], s));
#pragma unroll
                for (int t = 0; t < TP; ++t) {
                    if (t < ntp) { // (uniform)
                        const rl_v4i A = st[(t * 8 + s) * 64];
#pragma unroll
                        for (int m = 0; m < MT; ++m) {
                            D[m][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, z[m], D[m][t], 0, 0, 0);
                            if constexpr (MISS) {
                                if (tm[m]) { // (wave-uniform) the tile holds a column with missing calls
                                    rl_v4i zm;
                                    zm.x = z[m].x & (z[m].x >> 1);
                                    zm.y = z[m].y & (z[m].y >> 1);
                                    zm.z = z[m].z & (z[m].z >> 1);
                                    zm.w = z[m].w & (z[m].w >> 1);
                                    R[m][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, zm, R[m][t], 0, 0, 0);
                                }
                            }
                        }
                    }
                }
            }
        },
        [&](int m, int t, bool missing, unsigned long long* p) {
            md_add(p, md_join(D[m][t]));
            if constexpr (MISS) {
                if (missing) md_add(p + 2, md_join(R[m][t]));
            }
        });
}

// One thread per (marker, vector): P = D - 3 R, Q = sum_all q - R, each rounded once; x_j'u_k = mstd (P - mave Q)
__global__ __launch_bounds__(MD_TPB) void k_mdots_final(const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ ksum,
                                                        const int* __restrict__ scale, const double* __restrict__ mave,
                                                        const double* __restrict__ mstd, uint32_t m0, uint32_t count, int K,
                                                        double* __restrict__ out, double* __restrict__ raw)
{
    const uint64_t e = (uint64_t)blockIdx.x * MD_TPB + threadIdx.x;
    if (e >= (uint64_t)count * (uint32_t)K) return;
    const uint32_t j = m0 + (uint32_t)(e / (uint32_t)K), k = (uint32_t)(e % (uint32_t)K);
    const unsigned long long* a = acc + 4u * e;
    const unsigned long long Rlo = a[2], Rhi = a[3];
    const long long Plo = (long long)(a[0] - 3ull * Rlo), Phi = (long long)(a[1] - 3ull * Rhi);
    const long long Qlo = (long long)(ksum[2u * k + 1u] - Rlo), Qhi = (long long)(ksum[2u * k] - Rhi);
    const int E = scale[k];
    const double P = round_halves(Phi, Plo, E), Q = round_halves(Qhi, Qlo, E);
    const double sd = mstd[j];
    out[e] = isfinite(sd) ? sd * (P - mave[j] * Q) : __builtin_nan("");
    if (raw) {
        raw[2u * e] = P;
        raw[2u * e + 1u] = Q;
    }
}

} // namespace

// The work buffers of the pipeline for up to `kmax` vectors against up to `cmax` markers of a chunk, allocated once by the caller
// (hgibbs_marker_dots per call, hgibbs_pca per call for all its iterations): everything but the vectors and the results.
struct MdotsWs {
    DevBuf<unsigned long long> maxbits, acc; // (ksum lies inside maxbits)
    DevBuf<uint32_t> bad;
    DevBuf<int> scale;
    DevBuf<rl_v4i> img;
    DevBuf<uint8_t> tmiss;
    int kmax = 0;
    uint32_t cmax = 0;
};

static size_t mdots_ws_bytes(const hgibbs_ctx* h, int kmax, uint32_t cmax)
{
    const uint32_t n_sub = (h->n_local + MD_SUBI - 1) / MD_SUBI;
    return (size_t)n_sub * ((kmax + 1) / 2) * 8 * 64 * sizeof(rl_v4i) + (size_t)cmax * kmax * 4 * sizeof(unsigned long long) + (h->M + 15u) / 16u + 4096;
}

// Allocates the buffers and reads the marker-stats counts once (tiles of sixteen markers with a missing call in a column); synchronises
static int mdots_ws_create(hgibbs_ctx* h, MdotsWs& b, int kmax, uint32_t cmax)
{
    const uint32_t n = h->n_local;
    std::vector<uint8_t> tmiss;
    if (missing_tiles(h, 16u, tmiss)) return 1;
    const int tiles = (kmax + 1) / 2;
    const uint32_t n_sub = (n + MD_SUBI - 1) / MD_SUBI; // slices that hold individuals (all inside n_pad, a multiple of 4096)
    b.kmax = kmax;
    b.cmax = cmax;
    if (b.maxbits.alloc((size_t)kmax * 3)) return 1; // max, then the two halves of sum_i q
    if (b.bad.alloc(1)) return 1;
    if (b.scale.alloc((size_t)kmax)) return 1;
    if (b.img.alloc((size_t)n_sub * tiles * 8 * 64)) return 1;
    if (b.tmiss.alloc(tmiss.size())) return 1;
    if (b.acc.alloc((size_t)cmax * kmax * 4)) return 1;
    HIP_TRY(hipMemcpy(b.tmiss, tmiss.data(), tmiss.size(), hipMemcpyHostToDevice));
    return 0;
}

// Zeroes the sums of one product (stream-ordered, no synchronisation)
static int mdots_dev_clear(hgibbs_ctx* h, MdotsWs& b, uint32_t count, int K)
{
    HIP_TRY(hipMemsetAsync(b.bad, 0, sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(b.maxbits, 0, (size_t)K * 3 * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(b.acc, 0, (size_t)count * K * 4 * sizeof(unsigned long long), h->stream));
    return 0;
}

// The scales and sum_i q of hgibbs_score with a = o = u_k, then the digit image: dU (K x n_local, vector-major) -> scale[K],
// maxbits[K] with ksum = maxbits + K (two halves a vector), img of (K + 1) / 2 tiles.  maxbits and bad were zeroed.  Stream-ordered.
static int digit_image(hgibbs_ctx* h, const double* dU, int K, unsigned long long* maxbits, uint32_t* bad, int* scale, rl_v4i* img)
{
    const uint32_t n = h->n_local, n_sub = (n + MD_SUBI - 1) / MD_SUBI;
    const int tiles = (K + 1) / 2;
    const uint32_t per = std::max<uint32_t>(1u, std::min<uint32_t>((n + 2047u) / 2048u, (2048u + (uint32_t)K - 1u) / (uint32_t)K));
    k_score_max<<<dim3(K, per), SC_TPB, 0, h->stream>>>(dU, dU, n, maxbits, bad);
    HIP_TRY(hipGetLastError());
    k_score_ksum<<<dim3(K, per), SC_TPB, 0, h->stream>>>(dU, n, maxbits, scale, maxbits + K);
    HIP_TRY(hipGetLastError());
    k_mdots_digits<<<dim3(n_sub * 8u, tiles), 64, 0, h->stream>>>(dU, n, K, tiles, scale, img);
    HIP_TRY(hipGetLastError());
    return 0;
}

// An operator's builds: [tiles in the pass: 1, 2, more][any_missing], each with the TP it was built for (md_mt gives the grid)
using MdKernel = decltype(&k_mdots<1, false>);
struct MdBuild {
    int tp;
    MdKernel clean, missing;
};

// The passes over the workspace's image of K vectors against markers [m0, m0 + count), into b.acc
static int md_passes(hgibbs_ctx* h, MdotsWs& b, uint32_t m0, uint32_t count, int K, const MdBuild (&builds)[3])
{
    const int tiles = (K + 1) / 2;
    const uint32_t n_sub = (h->n_local + MD_SUBI - 1) / MD_SUBI;
    const uint32_t t0 = m0 / 16u, t1 = (m0 + count - 1u) / 16u + 1u;
    for (int tv0 = 0; tv0 < tiles; tv0 += MD_TPMAX) {
        const int ntp = std::min(MD_TPMAX, tiles - tv0);
        const MdBuild& bd = builds[ntp <= 1 ? 0 : ntp <= 2 ? 1 : 2];
        const uint32_t per_wg = (uint32_t)(MD_WAVES * md_mt(bd.tp)); // marker tiles per workgroup
        const uint32_t gx = (t1 - t0 + per_wg - 1u) / per_wg;
        // individual ranges: enough workgroups for eight per compute unit (option mdots_split fixes the number), no range above MD_SUB_MAX slices
        uint32_t sub_per = 0;
        const uint32_t gy = split_ranges(n_sub, h->mdots_split ? (uint32_t)h->mdots_split : (8u * (uint32_t)h->num_cu + gx - 1u) / gx, MD_SUB_MAX, sub_per);
        (h->any_missing ? bd.missing : bd.clean)<<<dim3(gx, gy), MD_WAVES * 64, 0, h->stream>>>(h->bed, h->stride, h->M, t0, t1, sub_per, n_sub, b.img, tiles, tv0, ntp, K, b.tmiss, m0, count, b.acc);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// The kernels of one product on device pointers: dU (K x n_local, vector-major) -> dout (count x K), draw (count x K x 2) or null.
// Stream-ordered: no allocation, no synchronisation.  mdots_dev_clear comes first.
static int mdots_dev_run(hgibbs_ctx* h, MdotsWs& b, uint32_t m0, uint32_t count, int K, const double* dU, double* dout, double* draw)
{
    static const MdBuild builds[3] = {{1, k_mdots<1, false>, k_mdots<1, true>}, {2, k_mdots<2, false>, k_mdots<2, true>}, {4, k_mdots<4, false>, k_mdots<4, true>}};
    const size_t nk = (size_t)count * K;
    if (digit_image(h, dU, K, b.maxbits, b.bad, b.scale, b.img)) return 1;
    if (md_passes(h, b, m0, count, K, builds)) return 1;
    k_mdots_final<<<(uint32_t)((nk + MD_TPB - 1) / MD_TPB), MD_TPB, 0, h->stream>>>(b.acc, b.maxbits + K, b.scale, h->mave, h->mstd, m0, count, K, dout, draw);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The refusals of an entry point that takes K vectors U against markers [m0, m0 + count), after op_guard, under the name `who`
static int kvec_guard(hgibbs_ctx* h, const char* who, uint32_t m0, uint32_t count, int K, const double* U, const double* out)
{
    if (K <= 0 || K > MD_KMAX) return fail("%s: K = %d, must be in [1, %d]", who, K, MD_KMAX);
    if (!U || !out) return fail("%s: null argument", who);
    if ((uint64_t)m0 + count > h->M) return fail("%s: markers [%u, %llu) out of range (M = %u)", who, m0, (unsigned long long)m0 + count, h->M);
    if (h->n_local >= MD_NMAX) return fail("%s: %u individuals, at most %u (64-bit sums)", who, h->n_local, MD_NMAX - 1u);
    const uint32_t n = h->n_local;
    for (size_t i = 0; i < (size_t)K * n; ++i)
        if (!std::isfinite(U[i])) return fail("%s: U[%d][%zu] = %g is not finite", who, (int)(i / n), i % n, U[i]);
    return 0;
}

extern "C" int hgibbs_marker_dots(hgibbs_t h, uint32_t m0, uint32_t count, int K, const double* U, double* out, double* raw)
{
    if (op_guard(h, "hgibbs_marker_dots", "the dots are not summed over ranks")) return 1;
    if (kvec_guard(h, "hgibbs_marker_dots", m0, count, K, U, out)) return 1;
    if (count == 0) return 0;
    const uint32_t n = h->n_local;
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;

    // a thin wrapper around the device-pointer pipeline: its own workspace, the vectors in, the results out
    MdotsWs ws;
    DevBuf<double> dU, dout, draw;
    const size_t nk = (size_t)count * K;
    if (dU.alloc((size_t)K * n)) return 1;
    if (mdots_ws_create(h, ws, K, count)) return 1;
    if (dout.alloc(nk)) return 1;
    if (raw && draw.alloc(nk * 2)) return 1;
    HIP_TRY(hipMemcpyAsync(dU, U, (size_t)K * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (mdots_dev_clear(h, ws, count, K)) return 1;

    // device time from here to the rounded result: every kernel of the call, not the host copies around it
    double ms = 0.0;
    if (lap_begin(h)) return 1;
    if (mdots_dev_run(h, ws, m0, count, K, dU, dout, draw)) return 1;
    if (lap_end(h, ms)) return 1;
    HIP_TRY(hipMemcpy(out, dout, nk * sizeof(double), hipMemcpyDeviceToHost));
    if (raw) HIP_TRY(hipMemcpy(raw, draw, nk * 2 * sizeof(double), hipMemcpyDeviceToHost));
    h->mdots_ms = ms;
    return 0;
}

extern "C" int hgibbs_last_marker_dots_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_marker_dots_ms: null argument");
    *ms = h->mdots_ms;
    return 0;
}
