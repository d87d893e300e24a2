// Row sums of a four-valued function of the genotype: for the BED loaded on a handle and T tables,
//
//     out[i][t] = sum_j tab[t][j][code_ij]
//
// as ONE pass over the codes per group of tables, the products on v_mfma_i32_16x16x64_i8 -- hgibbs_score's pass (hg_score.hip.h) with
// the one-hot expansion of the code where the score has the code itself, so that any function of {0, 1, 2, 3} is in its span.
//
//   tables   every entry becomes a fixed-point integer q = round(v 2^E_t), |q| <= 2^52, with one scale per table from its largest
//            magnitude; q is written in seven signed base-256 digits (sc_digit).  The only error is that rounding:
//            |out - exact| <= 0.5 M 2^-E_t <= M max|tab_t| 2^-52 per entry, before the one rounding to f64.
//   B        (64 x 16 individuals): the one-hot codes of SIXTEEN markers.  A marker's dword is 1u << (8 code): k = 4 marker + code.  The
//            codes are loaded and transposed as the score's are (one dword per lane, sc_transpose16, rl_expand16), so a lane holds
//            one individual's codes of sixteen markers of the block of 64; product u = 0 .. 3 of the block takes the four of them in
//            dword u of the expansion (markers 16 g + 4 i + u, i = 0 .. 3).
//   A        (16 rows x 64, bytes): the digits.  Row r of tile t is digit r & 7 of table 2 t + (r >> 3) (rows 7 and 15 zero); k as in B:
//            dword i, byte c = the digit of q[table][16 g + 4 i + u][c].
//   D        (i32): lane (c, g), register r = digit 4 g + r (mod 8) of individual c's sum -- exact.  Exactly one of a marker's four
//            one-hot bytes is 1, so a marker adds ONE digit, at most 128 in magnitude, to an accumulator: over a workgroup's range of
//            KB blocks of 64 markers |D| <= 128 x 64 KB = 2^13 KB, below 2^31 for KB < 2^18.  RW_KB_MAX = 2^17 keeps |D| <= 2^30; longer
//            marker lists are split into ranges (split_ranges), whatever rowsums_ranges says.
//   sums     as the score's: a lane puts four digits together (|.| < 2^55 per range) and adds them to the entry's low or high 64-bit
//            sum by an integer atomic.  Over all ranges |low sum| <= M 128 (1 + 2^8 + 2^16 + 2^24) < M 2^31.1, so M < 2^31 is asked for.
// No missing-call product and no constant: code 3 is a column of the table like the others.  Everything is an integer until
// k_rw_final rounds each entry once (round_halves), so a result does not depend on tiling, ranges, passes or repeats.
#pragma once

namespace {

constexpr uint32_t RW_KB_MAX = 131072; // blocks of 64 markers per workgroup at most (i32 headroom, above)
constexpr int RW_TMAX = 16;            // tables per call at most
constexpr int RW_SP = 8;               // tables per pass at most (the score's measured pass size)

// max |entry| of each table as an atomic max of the f64 bit patterns, and a flag for non-finite entries (k_score_max on 4 M entries)
__global__ __launch_bounds__(SC_TPB) void k_rw_max(const double* __restrict__ tab, uint64_t n4, unsigned long long* __restrict__ maxbits,
                                                    uint32_t* __restrict__ bad)
{
    __shared__ double smax[SC_TPB];
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const double* tt = tab + (size_t)t * n4;
    double mx = 0.0;
    bool nonfinite = false;
    for (uint64_t k = (uint64_t)blockIdx.y * SC_TPB + tid; k < n4; k += (uint64_t)gridDim.y * SC_TPB) {
        const double x = tt[k];
        if (!isfinite(x)) nonfinite = true;
        else mx = fmax(mx, fabs(x));
    }
    if (nonfinite) atomicOr(bad, 1u);
    smax[tid] = mx;
    __syncthreads();
    for (int w = SC_TPB / 2; w > 0; w >>= 1) {
        if (tid < (uint32_t)w) smax[tid] = fmax(smax[tid], smax[tid + w]);
        __syncthreads();
    }
    if (tid == 0 && smax[0] > 0.0) atomicMax(maxbits + t, (unsigned long long)__double_as_longlong(smax[0]));
}

// The A operands of one pass (tables t0 .. t0 + 2 tiles): [block of 64 markers][product u][tile][lane] 16 bytes, dword i, byte c =
// digit of q[table][64 kb + 16 g + 4 i + u][c]
__global__ __launch_bounds__(256) void k_rw_digits(const double* __restrict__ tab, uint32_t M, uint32_t T, uint32_t t0, int tiles,
                                                   const unsigned long long* __restrict__ maxbits, rl_v4i* __restrict__ dig)
{
    const uint32_t kb = blockIdx.x, tl = blockIdx.y, u = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t r = lane & 15u, g = lane >> 4, d = r & 7u;
    const uint32_t t = t0 + 2u * tl + (r >> 3);
    rl_v4i w = {0, 0, 0, 0};
    if (t < T && d < 7u) {
        const int E = sc_scale(maxbits[t]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t j = kb * 64u + 16u * g + 4u * (uint32_t)i + u;
            if (j >= M) continue;
            const double* e = tab + ((size_t)t * M + j) * 4u;
            uint32_t wq = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) wq |= (uint32_t)(uint8_t)sc_digit(sc_quant(e[c], E), (int)d) << (8 * c);
            w[i] = (int)wq;
        }
    }
    dig[(((size_t)kb * 4u + u) * (uint32_t)tiles + tl) * 64u + lane] = w;
}

// The product.  Workgroup (x, y): individuals [256 x, 256 x + 256) -- wave w the 64 from 256 x + 64 w --, blocks of 64 markers
// [y kb_per, (y + 1) kb_per); SP tables (SP / 2 tiles).  The A operands of a block (four products) are staged in LDS once for the
// four waves (double-buffered: one barrier per block); the codes of the next block and its operands are loaded while this block's
// MFMAs run.
template <int SP>
__global__ __launch_bounds__(SC_IND) void k_row_sums(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t M, uint32_t n_local,
                                                     uint32_t kb_per, const rl_v4i* __restrict__ dig, uint32_t T, uint32_t t0,
                                                     unsigned long long* __restrict__ acc)
{
    constexpr int TILES = SP / 2;
    constexpr int NOP = 4 * TILES * 64;              // A operands (16 bytes) per block: [product][tile][lane]
    constexpr int NPT = (NOP + SC_IND - 1) / SC_IND; // of them per thread when staging
    __shared__ rl_v4i sop[2][NOP];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nkb = (M + 63u) / 64u;
    const uint32_t kb0 = blockIdx.y * kb_per, kb1 = min(nkb, kb0 + kb_per);
    if (kb0 >= kb1) return; // (uniform)
    const uint64_t dw0 = (uint64_t)blockIdx.x * (SC_IND / 16) + wave * 4u; // first dword of this wave's individuals in a column

    auto load_codes = [&](uint32_t kb) {
        const uint32_t j = kb * 64u + lane;
        uint4 v = make_uint4(0u, 0u, 0u, 0u); // (markers past M: code 0 against zero digits)
        if (j < M) v = *reinterpret_cast<const uint4*>(bed + (uint64_t)j * stride + dw0 * 4u);
        return v;
    };
    rl_v4i rw[NPT];
    auto load_ops = [&](uint32_t kb) {
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const uint32_t idx = tid + (uint32_t)(k * SC_IND);
            if (idx < (uint32_t)NOP) rw[k] = dig[(size_t)kb * NOP + idx];
        }
    };
    auto store_ops = [&](int buf) {
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const uint32_t idx = tid + (uint32_t)(k * SC_IND);
            if (idx < (uint32_t)NOP) sop[buf][idx] = rw[k];
        }
    };

    rl_v4i D[4][TILES];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int t = 0; t < TILES; ++t) D[b][t] = rl_v4i{0, 0, 0, 0};

    uint4 cur = load_codes(kb0);
    load_ops(kb0);
    store_ops(0);
    __syncthreads();
    const uint32_t m16 = lane & 15u;
    for (uint32_t kb = kb0; kb < kb1; ++kb) {
        const int buf = (int)((kb - kb0) & 1u);
        const bool more = kb + 1u < kb1;
        uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
        if (more) {
            nxt = load_codes(kb + 1u);
            load_ops(kb + 1u);
        }
        const uint32_t wv[4] = {cur.x, cur.y, cur.z, cur.w};
        rl_v4i z[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) z[b] = rl_expand16(sc_transpose16(wv[b], m16));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            rl_v4i oh[4]; // one-hot: dword i = 1 << 8 code of marker 16 g + 4 i + u
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t x = (uint32_t)z[b][u] << 3; // byte i = 8 code
                oh[b].x = (int)(1u << (x & 0xFFu));
                oh[b].y = (int)(1u << ((x >> 8) & 0xFFu));
                oh[b].z = (int)(1u << ((x >> 16) & 0xFFu));
                oh[b].w = (int)(1u << (x >> 24));
            }
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                const rl_v4i A = sop[buf][(u * TILES + t) * 64 + lane];
#pragma unroll
                for (int b = 0; b < 4; ++b) D[b][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, oh[b], D[b][t], 0, 0, 0);
            }
        }
        if (more) store_ops(buf ^ 1);
        __syncthreads();
        cur = nxt;
    }

    // lane (c, g), tile t: table t0 + 2 t + (g >> 1), digits 4 (g & 1) .. +3 of individual c of each block of sixteen, put together
    // and added to the entry's low (g even) or high (g odd, units of 2^32) 64-bit sum, as k_score does
    const uint32_t c = lane & 15u, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const uint32_t tb = t0 + 2u * (uint32_t)t + (g >> 1);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t i = blockIdx.x * SC_IND + wave * 64u + 16u * (uint32_t)b + c;
            const long long v = (long long)D[b][t][0] + ((long long)D[b][t][1] << 8) + ((long long)D[b][t][2] << 16) + ((long long)D[b][t][3] << 24);
            if (i < n_local && tb < T && v != 0)
                __hip_atomic_fetch_add(acc + ((size_t)i * T + tb) * 2u + (g & 1u), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// out[i][t] = (hi 2^32 + lo) 2^-E_t, rounded once (round_halves)
__global__ __launch_bounds__(SC_TPB) void k_rw_final(const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ maxbits,
                                                     uint32_t n_local, uint32_t T, double* __restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * SC_TPB + threadIdx.x;
    if (k >= (uint64_t)n_local * T) return;
    out[k] = round_halves((long long)acc[2 * k + 1], (long long)acc[2 * k], sc_scale(maxbits[k % T]));
}

template <int SP>
void rw_launch(hgibbs_ctx* h, dim3 grid, uint32_t kb_per, const rl_v4i* dig, uint32_t T, uint32_t t0, unsigned long long* acc)
{
    k_row_sums<SP><<<grid, SC_IND, 0, h->stream>>>(h->bed, h->stride, h->M, h->n_local, kb_per, dig, T, t0, acc);
}

} // namespace

extern "C" int hgibbs_row_sums(hgibbs_t h, int T, const double* tab, double* out)
{
    if (h) h->row_sums_ms = 0.0;
    if (op_guard(h, "hgibbs_row_sums", "the sums run over this handle's rows of every marker")) return 1;
    if (T < 1 || T > RW_TMAX) return fail("hgibbs_row_sums: T = %d, needs 1 to %d tables", T, RW_TMAX);
    if (!tab || !out) return fail("hgibbs_row_sums: null argument");
    if (h->M >= 0x80000000u) return fail("hgibbs_row_sums: %u markers, the 64-bit sums of the digits take fewer than 2^31", h->M);
    HIP_TRY(hipSetDevice(h->device));
    const uint32_t M = h->M, n = h->n_local, nkb = (M + 63u) / 64u;
    int sp = 2;
    while (sp < T && sp < RW_SP) sp *= 2;
    const int tiles = sp / 2;
    const size_t TM4 = (size_t)T * M * 4, NT = (size_t)n * T, ndig = (size_t)nkb * 4 * tiles * 64;
    if (need_device_memory(TM4 * sizeof(double) + ndig * sizeof(rl_v4i) + NT * 3 * sizeof(double) + 4096,
                           "hgibbs_row_sums: %d tables of %u markers and their digits need %.1f MiB", T, M,
                           (TM4 * sizeof(double) + ndig * sizeof(rl_v4i) + NT * 3 * sizeof(double)) / 1048576.0))
        return 1;
    DevBuf<double> dtab, dout;
    DevBuf<rl_v4i> dig;
    DevBuf<unsigned long long> maxbits, acc;
    DevBuf<uint32_t> bad;
    if (dtab.alloc(TM4) || dout.alloc(NT) || dig.alloc(ndig) || maxbits.alloc((size_t)T) || acc.alloc(NT * 2) || bad.alloc(1)) return 1;
    HIP_TRY(hipMemcpyAsync(dtab, tab, TM4 * sizeof(double), hipMemcpyHostToDevice, h->stream));

    // device time from here to the rounded result: every kernel of the call, not the host copies around it
    if (lap_begin(h)) return 1;
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(maxbits, 0, (size_t)T * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(acc, 0, NT * 2 * sizeof(unsigned long long), h->stream));
    {
        // workgroups per table for the scale: about 2048 in all, at least 2048 entries each
        const uint64_t n4 = (uint64_t)M * 4u;
        const uint32_t per = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>((n4 + 2047u) / 2048u, (2048u + (uint32_t)T - 1u) / (uint32_t)T));
        k_rw_max<<<dim3(T, per), SC_TPB, 0, h->stream>>>(dtab, n4, maxbits, bad);
        HIP_TRY(hipGetLastError());
    }
    // grid: workgroups of 256 individuals x ranges of marker blocks, enough of them to fill the device (8 per compute unit); the
    // ranges never exceed RW_KB_MAX blocks (i32 headroom of the digit sums)
    const uint32_t gx = h->n_pad / SC_IND;
    uint32_t want = (8u * (uint32_t)h->num_cu + gx - 1u) / gx, kb_per = 0;
    if (h->rowsums_ranges) want = std::min(want, (uint32_t)h->rowsums_ranges);
    const uint32_t gy = split_ranges(nkb, want, RW_KB_MAX, kb_per);
    for (uint32_t t0 = 0; t0 < (uint32_t)T; t0 += (uint32_t)sp) {
        k_rw_digits<<<dim3(nkb, tiles), 256, 0, h->stream>>>(dtab, M, (uint32_t)T, t0, tiles, maxbits, dig);
        HIP_TRY(hipGetLastError());
        const dim3 grid(gx, gy);
        switch (sp) {
        case 2: rw_launch<2>(h, grid, kb_per, dig, (uint32_t)T, t0, acc); break;
        case 4: rw_launch<4>(h, grid, kb_per, dig, (uint32_t)T, t0, acc); break;
        default: rw_launch<8>(h, grid, kb_per, dig, (uint32_t)T, t0, acc); break;
        }
        HIP_TRY(hipGetLastError());
    }
    k_rw_final<<<(uint32_t)((NT + SC_TPB - 1) / SC_TPB), SC_TPB, 0, h->stream>>>(acc, maxbits, n, (uint32_t)T, dout);
    HIP_TRY(hipGetLastError());
    if (lap_mark(h)) return 1;
    uint32_t isbad = 0;
    HIP_TRY(hipMemcpyAsync(&isbad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (isbad) return fail("hgibbs_row_sums: a table entry is not finite"); // (out untouched; what the kernels made of it is dropped)
    HIP_TRY(hipMemcpy(out, dout, NT * sizeof(double), hipMemcpyDeviceToHost));
    double ms = 0.0;
    if (lap_read(h, ms)) return 1;
    h->row_sums_ms = ms;
    return 0;
}

extern "C" int hgibbs_last_row_sums_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_row_sums_ms: null argument");
    *ms = h->row_sums_ms;
    return 0;
}
