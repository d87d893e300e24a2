// Sums of dense vectors over the rows of each genotype code, per loaded marker: for markers j in
// [m0, m0 + count) and K vectors u_k over the handle's n_local individuals, the exact integer sums
//
//     S_jkc = sum_{i : code_ij = c} q_ik,   c = 0, 1, 2, 3,      q_ik = round(u_ik 2^E_k)
//
// each rounded to f64 ONCE (times 2^-E_k).  Codes 0, 1, 2 are the copies of A1 as hgibbs_load_bed reads them, code 3 is a missing
// call.  This is the per-marker counterpart of hgibbs_row_sums (hg_rowsums.hip.h): with the four sums any sum_i f(g_ij) u_ik is a
// four-term combination of exact integers.  The kernel is k_mdots (hg_mdots.hip.h) with indicator bytes where k_mdots has the code
// itself; the digit image (k_mdots_digits), the scales (k_score_max, k_score_ksum), the buffers (MdotsWs) and the error bound of the
// rounding of u are those of hg_mdots.hip.h, unchanged.
//
//   A        the digit image of k_mdots_digits: rows 0..6 vector 2 t, rows 8..14 vector 2 t + 1, zero past n_local.
//   B        lane (c, g) of k-step s takes ONE stored BED dword x of marker c, as k_mdots, and turns it into indicator bytes in
//            registers.  With z = rl_expand16(x) (one code a byte) they are  [code == 1] = z & ~(z >> 1) & 0x01010101,
//            [code == 2] = (z >> 1) & ~z & 0x01010101,  [code == 3] = z & (z >> 1) (the form k_mdots uses); the kernel forms the
//            same bytes with fewer instructions by taking x & ~(x >> 1), (x >> 1) & ~x and x & (x >> 1) on the packed dword first
//            and expanding each (shift by 2 q, mask 0x01010101: rl_expand16's placement).
//            One v_mfma_i32_16x16x64_i8 per class against the same A digits.
//   missing  the [code == 3] product runs only in 16-marker tiles that hold a column with missing calls (missing_tiles, granule 16)
//            and is compiled only into k_mclass<.., true>, launched only when some column of the handle has missing calls.  Elsewhere
//            S3 = 0 without a product.
//   class 0  S0 = sum_{i < n_local} q_ik - S1 - S2 - S3, formed in the two 64-bit halves before the rounding (k_mclass_final);
//            k_score_ksum gives the first term exactly.
//   padding  BED slots past n_local are code 3 but meet zero digits; markers past M read as code 0 (no indicator set) and are never
//            written.
//   exact    every i32 partial is a sum of |digit| x indicator <= 128 over the individuals of the workgroup's range, at most
//            MD_SUB_MAX slices (128 x 2^22 = 2^29 < 2^31).  The halves are added by 64-bit integer atomics and stay inside an int64
//            for n_local < 2^29 as k_mdots' do (the indicator is at most 1 where the code is at most 3).  The sums do not depend on
//            mave or mstd: a monomorphic marker has them like any other.  Integer sums do not depend on tiling, workgroups, the
//            individual split (option mdots_split), m0 / count chunking or launch order: bit-identical across all of them.
//   reuse    workgroup = MD_WAVES waves x MT marker tiles (mc_mt: 4 at TP = 2, 2 at TP = 4, as k_mdots), TP vector tiles a pass; the
//            accumulators are two, with MISS three, times those of k_mdots at the same TP and MT (DESIGN.md section 25 has the
//            resource table).  K > 8 takes ceil(K / 8) passes, each a read of the BED.
#pragma once

namespace {

constexpr int MC_NCLS = 3; // classes that come from products (codes 1, 2, 3); class 0 is the remainder

// Marker tiles per wave.  TP is 2 or 4: a build for ONE vector tile (k_mdots has one) takes 270 and more registers with three sets of
// accumulators on four marker tiles, one wave per SIMD, where the build for two takes 226, so K <= 2 runs the
// build for two with ntp = 1: the second tile is neither staged nor multiplied.
constexpr int mc_mt(int TP) { return TP <= 2 ? 4 : 2; }

// The product.  Geometry, staging and arguments as k_mdots.  acc: [marker - m0][vector][class - 1][half] 64-bit sums.
template <int TP, bool MISS>
__global__ __launch_bounds__(MD_WAVES * 64) void k_mclass(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t M, uint32_t t0,
                                                          uint32_t t1, uint32_t sub_per, uint32_t n_sub, const rl_v4i* __restrict__ img,
                                                          int tiles, int tv0, int ntp, int K, const uint8_t* __restrict__ tmiss,
                                                          uint32_t m0, uint32_t count, unsigned long long* __restrict__ acc)
{
    constexpr int MT = mc_mt(TP);
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

    rl_v4i D1[MT][TP], D2[MT][TP], D3[MT][MISS ? TP : 1];
    bool tm[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        tm[m] = MISS && wave_on && tw + (uint32_t)m < t1 && tmiss[tw + (uint32_t)m];
#pragma unroll
        for (int t = 0; t < TP; ++t) {
            D1[m][t] = rl_v4i{0, 0, 0, 0};
            D2[m][t] = rl_v4i{0, 0, 0, 0};
            if constexpr (MISS) D3[m][t] = rl_v4i{0, 0, 0, 0};
        }
    }

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
        if (wave_on) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                // the digits of the k-step stay in registers for all marker tiles; one tile's indicators are live at a time
                rl_v4i A[TP];
#pragma unroll
                for (int t = 0; t < TP; ++t) A[t] = t < ntp ? stage[buf][(t * 8 + s) * 64 + (int)lane] : rl_v4i{0, 0, 0, 0};
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const uint4 v = cw[m][s >> 2];
                    const uint32_t x = (s & 3) == 0 ? v.x : (s & 3) == 1 ? v.y : (s & 3) == 2 ? v.z : v.w;
                    // the indicators on the packed dword (bit 0 of each 2-bit slot; bit 1 is masked off below), then rl_expand16's
                    // placement: dword q, byte i = individual 4 i + q of the sixteen
                    const uint32_t h = x >> 1, p1 = x & ~h, p2 = h & ~x, p3 = x & h;
                    rl_v4i z1, z2, z3;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        z1[q] = (int)((p1 >> (2 * q)) & 0x01010101u);
                        z2[q] = (int)((p2 >> (2 * q)) & 0x01010101u);
                        z3[q] = (int)((p3 >> (2 * q)) & 0x01010101u);
                    }
#pragma unroll
                    for (int t = 0; t < TP; ++t) {
                        if (t < ntp) { // (uniform)
                            D1[m][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], z1, D1[m][t], 0, 0, 0);
                            D2[m][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], z2, D2[m][t], 0, 0, 0);
                            if constexpr (MISS) {
                                if (tm[m]) // (wave-uniform) the tile holds a column with missing calls
                                    D3[m][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], z3, D3[m][t], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }
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

    // lane (c, g), tile t, register r: digit (4 g + r) mod 8 of vector 2 (tv0 + t) + (g >> 1) against marker 16 (tw + m) + c
    auto put = [&](const rl_v4i& a) {
        return (long long)a[0] + ((long long)a[1] << 8) + ((long long)a[2] << 16) + ((long long)a[3] << 24);
    };
    auto add = [&](unsigned long long* p, long long v) {
        if (v) __hip_atomic_fetch_add(p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const uint32_t j = 16u * (tw + (uint32_t)m) + c;
        if (j < m0 || j - m0 >= count || j >= M) continue;
#pragma unroll
        for (int t = 0; t < TP; ++t) {
            const uint32_t k = 2u * (uint32_t)(tv0 + t) + (g >> 1);
            if (t >= ntp || k >= (uint32_t)K) continue;
            unsigned long long* p = acc + ((uint64_t)(j - m0) * (uint32_t)K + k) * (2u * MC_NCLS) + (g & 1u);
            add(p, put(D1[m][t]));
            add(p + 2, put(D2[m][t]));
            if constexpr (MISS) {
                if (tm[m]) add(p + 4, put(D3[m][t]));
            }
        }
    }
}

// One thread per (marker, vector): S0 = sum_all q - S1 - S2 - S3 in the integer halves, then the four sums rounded once each
__global__ __launch_bounds__(MD_TPB) void k_mclass_final(const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ ksum,
                                                         const int* __restrict__ scale, uint32_t count, int K, double* __restrict__ out)
{
    const uint64_t e = (uint64_t)blockIdx.x * MD_TPB + threadIdx.x;
    if (e >= (uint64_t)count * (uint32_t)K) return;
    const uint32_t k = (uint32_t)(e % (uint32_t)K);
    const unsigned long long* a = acc + (2u * MC_NCLS) * e;
    const unsigned long long lo0 = ksum[2u * k + 1u] - a[0] - a[2] - a[4], hi0 = ksum[2u * k] - a[1] - a[3] - a[5];
    const int E = scale[k];
    out[4u * e] = round_halves((long long)hi0, (long long)lo0, E);
#pragma unroll
    for (int cl = 0; cl < MC_NCLS; ++cl) out[4u * e + 1u + (uint32_t)cl] = round_halves((long long)a[2 * cl + 1], (long long)a[2 * cl], E);
}

template <int TP>
void mclass_launch(hgibbs_ctx* h, dim3 grid, uint32_t t0, uint32_t t1, uint32_t sub_per, uint32_t n_sub, const rl_v4i* img, int tiles,
                   int tv0, int ntp, int K, const uint8_t* tmiss, uint32_t m0, uint32_t count, unsigned long long* acc)
{
    if (h->any_missing)
        k_mclass<TP, true><<<grid, MD_WAVES * 64, 0, h->stream>>>(h->bed, h->stride, h->M, t0, t1, sub_per, n_sub, img, tiles, tv0, ntp, K, tmiss, m0, count, acc);
    else
        k_mclass<TP, false><<<grid, MD_WAVES * 64, 0, h->stream>>>(h->bed, h->stride, h->M, t0, t1, sub_per, n_sub, img, tiles, tv0, ntp, K, tmiss, m0, count, acc);
}

// MdotsWs holds four 64-bit sums per (marker, vector) and the class sums take six: a workspace made for this many markers has them
uint32_t mclass_ws_markers(uint32_t count) { return (uint32_t)(((uint64_t)count * (2u * MC_NCLS) + 3u) / 4u); }

// The kernels of one call on device pointers: dU (K x n_local, vector-major) -> dout (count x K x 4).  Stream-ordered: no
// allocation, no synchronisation.  The workspace was made for mclass_ws_markers(count) markers and cleared for as many.
int mclass_dev_run(hgibbs_ctx* h, MdotsWs& b, uint32_t m0, uint32_t count, int K, const double* dU, double* dout)
{
    const uint32_t n = h->n_local;
    const int tiles = (K + 1) / 2;
    const uint32_t n_sub = (n + MD_SUBI - 1) / MD_SUBI;
    const size_t nk = (size_t)count * K;
    unsigned long long* ksum = b.maxbits + K;
    {
        // the scales, sum_i q and the digit image, as mdots_dev_run makes them
        const uint32_t per = std::max<uint32_t>(1u, std::min<uint32_t>((n + 2047u) / 2048u, (2048u + (uint32_t)K - 1u) / (uint32_t)K));
        k_score_max<<<dim3(K, per), SC_TPB, 0, h->stream>>>(dU, dU, n, b.maxbits, b.bad);
        HIP_TRY(hipGetLastError());
        k_score_ksum<<<dim3(K, per), SC_TPB, 0, h->stream>>>(dU, n, b.maxbits, b.scale, ksum);
        HIP_TRY(hipGetLastError());
        k_mdots_digits<<<dim3(n_sub * 8u, tiles), 64, 0, h->stream>>>(dU, n, K, tiles, b.scale, b.img);
        HIP_TRY(hipGetLastError());
    }
    const uint32_t t0 = m0 / 16u, t1 = (m0 + count - 1u) / 16u + 1u;
    for (int tv0 = 0; tv0 < tiles; tv0 += MD_TPMAX) {
        const int ntp = std::min(MD_TPMAX, tiles - tv0);
        const int tp = ntp <= 2 ? 2 : 4; // (no build for one tile: K <= 2 runs the build for two with one used, see mc_mt)
        const uint32_t per_wg = (uint32_t)(MD_WAVES * mc_mt(tp)); // marker tiles per workgroup
        const uint32_t gx = (t1 - t0 + per_wg - 1u) / per_wg;
        // individual ranges as hgibbs_marker_dots splits them: eight workgroups per compute unit (option mdots_split fixes the number),
        // no range above MD_SUB_MAX slices
        uint32_t sub_per = 0;
        const uint32_t gy = split_ranges(n_sub, h->mdots_split ? (uint32_t)h->mdots_split : (8u * (uint32_t)h->num_cu + gx - 1u) / gx, MD_SUB_MAX, sub_per);
        const dim3 grid(gx, gy);
        switch (tp) {
        case 2: mclass_launch<2>(h, grid, t0, t1, sub_per, n_sub, b.img, tiles, tv0, ntp, K, b.tmiss, m0, count, b.acc); break;
        default: mclass_launch<4>(h, grid, t0, t1, sub_per, n_sub, b.img, tiles, tv0, ntp, K, b.tmiss, m0, count, b.acc); break;
        }
        HIP_TRY(hipGetLastError());
    }
    k_mclass_final<<<(uint32_t)((nk + MD_TPB - 1) / MD_TPB), MD_TPB, 0, h->stream>>>(b.acc, ksum, b.scale, count, K, dout);
    HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace

extern "C" int hgibbs_marker_class_sums(hgibbs_t h, uint32_t m0, uint32_t count, int K, const double* U, double* out)
{
    if (op_guard(h, "hgibbs_marker_class_sums", "the sums are not summed over ranks")) return 1;
    if (K <= 0 || K > MD_KMAX) return fail("hgibbs_marker_class_sums: K = %d, must be in [1, %d]", K, MD_KMAX);
    if (!U || !out) return fail("hgibbs_marker_class_sums: null argument");
    if ((uint64_t)m0 + count > h->M) return fail("hgibbs_marker_class_sums: markers [%u, %llu) out of range (M = %u)", m0, (unsigned long long)m0 + count, h->M);
    if (h->n_local >= MD_NMAX) return fail("hgibbs_marker_class_sums: %u individuals, at most %u (64-bit sums)", h->n_local, MD_NMAX - 1u);
    const uint32_t n = h->n_local;
    for (size_t i = 0; i < (size_t)K * n; ++i)
        if (!std::isfinite(U[i])) return fail("hgibbs_marker_class_sums: U[%d][%zu] = %g is not finite", (int)(i / n), i % n, U[i]);
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;

    const uint32_t cws = mclass_ws_markers(count);
    const size_t nk = (size_t)count * K, bytes = mdots_ws_bytes(h, K, cws) + ((size_t)K * n + nk * 4) * sizeof(double);
    if (need_device_memory(bytes, "hgibbs_marker_class_sums: %d vectors against %u markers need %.1f MiB", K, count, bytes / 1048576.0)) return 1;
    MdotsWs ws;
    DevBuf<double> dU, dout;
    if (dU.alloc((size_t)K * n)) return 1;
    if (mdots_ws_create(h, ws, K, cws)) return 1;
    if (dout.alloc(nk * 4)) return 1;
    HIP_TRY(hipMemcpyAsync(dU, U, (size_t)K * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (mdots_dev_clear(h, ws, cws, K)) return 1;

    // device time from here to the rounded result: every kernel of the call, not the host copies around it
    double ms = 0.0;
    if (lap_begin(h)) return 1;
    if (mclass_dev_run(h, ws, m0, count, K, dU, dout)) return 1;
    if (lap_end(h, ms)) return 1;
    HIP_TRY(hipMemcpy(out, dout, nk * 4 * sizeof(double), hipMemcpyDeviceToHost));
    h->mclass_ms = ms;
    return 0;
}

extern "C" int hgibbs_last_marker_class_sums_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_marker_class_sums_ms: null argument");
    *ms = h->mclass_ms;
    return 0;
}
