// Sums of dense vectors over the rows of each genotype code, per loaded marker: for markers j in
// [m0, m0 + count) and K vectors u_k over the handle's n_local individuals, the exact integer sums
//
//     S_jkc = sum_{i : code_ij = c} q_ik,   c = 0, 1, 2, 3,      q_ik = round(u_ik 2^E_k)
//
// each rounded to f64 ONCE (times 2^-E_k).  Codes 0, 1, 2 are the copies of A1 as hgibbs_load_bed reads them, code 3 is a missing
// call.  This is the per-marker counterpart of hgibbs_row_sums (hg_rowsums.hip.h): with the four sums any sum_i f(g_ij) u_ik is a
// four-term combination of exact integers.  The operator stands on the frame of hg_mdots.hip.h (md_frame, digit_image, md_passes,
// kvec_guard, MdotsWs; the scale and its error bound, the A operand, the geometry, the staging and the independence of tiling and
// chunking are described there).  Its own:
//
//   B        the lane's BED dword x of the k-step turned into indicator bytes in registers.  With z = rl_expand16(x) (one code a
//            byte) they are  [code == 1] = z & ~(z >> 1) & 0x01010101,  [code == 2] = (z >> 1) & ~z & 0x01010101,
//            [code == 3] = z & (z >> 1) (the form k_mdots uses); the kernel forms the same bytes with fewer instructions by taking
//            x & ~(x >> 1), (x >> 1) & ~x and x & (x >> 1) on the packed dword first and expanding each (shift by 2 q, mask
//            0x01010101: rl_expand16's placement).  One v_mfma_i32_16x16x64_i8 per class against the same A digits.
//   missing  the [code == 3] product runs only in 16-marker tiles that hold a column with missing calls and is compiled only into
//            k_mclass<.., true>.  Elsewhere S3 = 0 without a product.
//   class 0  S0 = sum_{i < n_local} q_ik - S1 - S2 - S3, formed in the two 64-bit halves before the rounding (k_mclass_final);
//            k_score_ksum gives the first term exactly.  Markers past M read as code 0 (no indicator set) and are never written.
//   exact    every i32 partial is a sum of |digit| x indicator <= 128 over the individuals of the workgroup's range, at most
//            MD_SUB_MAX slices (128 x 2^22 = 2^29 < 2^31).  The halves stay inside an int64 for n_local < 2^29 as k_mdots' do (the
//            indicator is at most 1 where the code is at most 3).  The sums do not depend on mave or mstd: a monomorphic marker has
//            them like any other.
//   no TP = 1  a build for ONE vector tile (k_mdots has one) takes 270 and more registers with three sets of accumulators on four
//            marker tiles, one wave per SIMD, where the build for two takes 226 (with the resource table), so
//            K <= 2 runs the build for two with ntp = 1: the second tile is neither staged nor multiplied.
#pragma once

namespace {

constexpr int MC_NCLS = 3; // classes that come from products (codes 1, 2, 3); class 0 is the remainder

// The product: the digits of a k-step stay in registers (A) for all marker tiles; one tile's indicators are live at a time (k_mdots
// holds the codes and reads A per tile: the register table of section 25 stands on this order).
// acc: [marker - m0][vector][class - 1][half] 64-bit sums.
template <int TP, bool MISS>
__global__ __launch_bounds__(MD_WAVES * 64) void k_mclass(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t M, uint32_t t0,
                                                          uint32_t t1, uint32_t sub_per, uint32_t n_sub, const rl_v4i* __restrict__ img,
                                                          int tiles, int tv0, int ntp, int K, const uint8_t* __restrict__ tmiss,
                                                          uint32_t m0, uint32_t count, unsigned long long* __restrict__ acc)
{
    constexpr int MT = md_mt(TP);
    rl_v4i D1[MT][TP] = {}, D2[MT][TP] = {}, D3[MT][MISS ? TP : 1] = {};
    md_frame<TP, MISS, 2 * MC_NCLS>(
        bed, stride, M, t0, t1, sub_per, n_sub, img, tiles, tv0, ntp, K, tmiss, m0, count, acc,
        [&](const rl_v4i* st, const uint4 (&cw)[MT][2], const bool (&tm)[MT]) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                rl_v4i A[TP];
#pragma unroll
                for (int t = 0; t < TP; ++t) A[t] = t < ntp ? st[(t * 8 + s) * 64] : rl_v4i{0, 0, 0, 0};
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const uint32_t x = md_dword(cw[m], s);
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
        },
        [&](int m, int t, bool missing, unsigned long long* p) {
            md_add(p, md_join(D1[m][t]));
            md_add(p + 2, md_join(D2[m][t]));
            if constexpr (MISS) {
                if (missing) md_add(p + 4, md_join(D3[m][t]));
            }
        });
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

// MdotsWs holds four 64-bit sums per (marker, vector) and the class sums take six: a workspace made for this many markers has them
uint32_t mclass_ws_markers(uint32_t count) { return (uint32_t)(((uint64_t)count * (2u * MC_NCLS) + 3u) / 4u); }

// The kernels of one call on device pointers: dU (K x n_local, vector-major) -> dout (count x K x 4).  Stream-ordered: no
// allocation, no synchronisation.  The workspace was made for mclass_ws_markers(count) markers and cleared for as many.
int mclass_dev_run(hgibbs_ctx* h, MdotsWs& b, uint32_t m0, uint32_t count, int K, const double* dU, double* dout)
{
    // (no build for one tile: a pass of one runs the build for two)
    static const MdBuild builds[3] = {{2, k_mclass<2, false>, k_mclass<2, true>}, {2, k_mclass<2, false>, k_mclass<2, true>}, {4, k_mclass<4, false>, k_mclass<4, true>}};
    const size_t nk = (size_t)count * K;
    if (digit_image(h, dU, K, b.maxbits, b.bad, b.scale, b.img)) return 1;
    if (md_passes(h, b, m0, count, K, builds)) return 1;
    k_mclass_final<<<(uint32_t)((nk + MD_TPB - 1) / MD_TPB), MD_TPB, 0, h->stream>>>(b.acc, b.maxbits + K, b.scale, count, K, dout);
    HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace

extern "C" int hgibbs_marker_class_sums(hgibbs_t h, uint32_t m0, uint32_t count, int K, const double* U, double* out)
{
    if (op_guard(h, "hgibbs_marker_class_sums", "the sums are not summed over ranks")) return 1;
    if (kvec_guard(h, "hgibbs_marker_class_sums", m0, count, K, U, out)) return 1;
    if (count == 0) return 0;
    const uint32_t n = h->n_local;
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
