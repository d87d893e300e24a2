// Scoring a cohort with posterior effects: for the BED loaded on a handle and S weight vectors,
//
//     out[i][s] = sum_j [code_ij != 3] (a_sj code_ij + o_sj)
//
// as ONE pass over the codes per group of samples, the products on v_mfma_i32_16x16x64_i8 -- the refill's product of
// hg_streamer2.hip.h turned around: it sums over markers instead of individuals.
//
//   weights  every a_sj (and o_sj) becomes a fixed-point integer q = round(a 2^E_s), |q| < 2^52, with one scale per sample from
//            max_j max(|a_sj|, |o_sj|); q is written in seven signed base-256 digits (the refill's digits of eps, rl_digits).
//            The only error is that rounding: |out - exact| <= 1.5 M 2^-E_s <= 3 M max|weight| 2^-52 per entry.
//   A        (16 rows x 64 markers, bytes): the digits.  Row r of tile t is digit r & 7 of sample 2 t + (r >> 3) (row 7 and 15 zero),
//            so a lane of the result holds four digits of ONE sample: lanes g = 0, 2 digits 0..3, lanes g = 1, 3 digits 4..6.
//   B        (64 markers x 16 individuals): the codes, transposed on chip.  Stored, a dword holds sixteen individuals of one marker;
//            the product wants one individual's codes of sixteen markers per lane.  A wave loads one dword per lane (marker = lane)
//            and transposes the 16 x 16 matrix of 2-bit fields of each group of sixteen lanes in four butterfly stages
//            (ds_swizzle to the partner lane h = 8, 4, 2, 1 apart, one rotate, one bit-field insert), then expands the word to bytes.
//   D        (i32): lane (c, g), register r = digit 4 g + r (mod 8) of individual c's sum -- exact.  Per accumulator |D| <= 512 markers
//            x 128 per marker (code 3 x a digit + the missing-call digit), so a workgroup takes at most SC_KB_MAX blocks of 64
//            markers (2^21 markers: |D| < 2^30) before its digits leave for the 64-bit sums.
//   missing  code 3 enters the product as 3; a second product with the indicator operand [code == 3] against the digits of
//            -(3 q_a + q_o) removes it and the o term, only in blocks of 64 markers that hold a column with missing calls.  The o terms
//            of every column are ONE constant per sample, sum_j q_o (exact, 2 x 64-bit).
// Everything is an integer until the very end, so a result does not depend on tiling, workgroups or passes: the workgroups' parts
// meet in 64-bit atomic adds (order-free), and k_score_final rounds each entry once.
#pragma once

namespace {

constexpr int SC_WAVES = 4;                  // waves per workgroup; every wave 64 individuals (four dwords of a column)
constexpr int SC_IND = SC_WAVES * 64;        // individuals per workgroup
constexpr uint32_t SC_KB_MAX = 32768;        // blocks of 64 markers per workgroup at most (i32 headroom, above)
constexpr int SC_TPB = 256;                  // threads of the helper kernels

// signed base-256 digits of x, |x| < 2^54 (hg_streamer2.hip.h, rl_digits): digit j < 6 = byte j of y ^ 0x80, digit 6 = byte 6 of y
__device__ __forceinline__ int sc_digit(long long x, int d)
{
    const unsigned long long y = (unsigned long long)x + 0x0000808080808080ull;
    const uint32_t b = (uint32_t)(y >> (8 * d)) & 0xFFu;
    return (int)(int8_t)(uint8_t)(d < 6 ? (b ^ 0x80u) : b);
}

__device__ __forceinline__ long long sc_quant(double v, int E) { return llrint(ldexp(v, E)); }

// The scale of each sample, over SC_SPLIT(M, S) workgroups per sample in two launches (everything order-free):
// k_score_max   max |a|, |o| over the markers as an atomic max of the f64 bit patterns (non-negative doubles order as integers), and a
//               flag for non-finite weights;
// k_score_ksum  E_s = 52 - e with max_s < 2^e (frexp: e = floor(log2 max_s) + 1; E_s = 0 for an all-zero sample) and sum_j q_o as two
//               64-bit halves (q_o >> 32 and its low 32 bits: exact for M < 2^31) by atomic integer adds.
__global__ __launch_bounds__(SC_TPB) void k_score_max(const double* __restrict__ a, const double* __restrict__ o, uint32_t M,
                                                       unsigned long long* __restrict__ maxbits, uint32_t* __restrict__ bad)
{
    __shared__ double smax[SC_TPB];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const double* as = a + (size_t)s * M;
    const double* os = o + (size_t)s * M;
    double mx = 0.0;
    bool nonfinite = false;
    for (uint32_t j = blockIdx.y * SC_TPB + t; j < M; j += gridDim.y * SC_TPB) {
        const double x = as[j], y = os[j];
        if (!isfinite(x) || !isfinite(y)) nonfinite = true;
        else mx = fmax(mx, fmax(fabs(x), fabs(y)));
    }
    if (nonfinite) atomicOr(bad, 1u);
    smax[t] = mx;
    __syncthreads();
    for (int w = SC_TPB / 2; w > 0; w >>= 1) {
        if (t < (uint32_t)w) smax[t] = fmax(smax[t], smax[t + w]);
        __syncthreads();
    }
    if (t == 0 && smax[0] > 0.0) atomicMax(maxbits + s, (unsigned long long)__double_as_longlong(smax[0]));
}

__device__ __forceinline__ int sc_scale(unsigned long long maxbits)
{
    const double mx = __longlong_as_double((long long)maxbits);
    if (!(mx > 0.0)) return 0;
    int e;
    (void)frexp(mx, &e); // mx < 2^e
    return 52 - e;
}

__global__ __launch_bounds__(SC_TPB) void k_score_ksum(const double* __restrict__ o, uint32_t M, const unsigned long long* __restrict__ maxbits,
                                                        int* __restrict__ scale, unsigned long long* __restrict__ ksum)
{
    __shared__ long long shi[SC_TPB], slo[SC_TPB];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const int E = sc_scale(maxbits[s]);
    const double* os = o + (size_t)s * M;
    long long hi = 0, lo = 0;
    for (uint32_t j = blockIdx.y * SC_TPB + t; j < M; j += gridDim.y * SC_TPB) {
        const double y = os[j];
        if (!isfinite(y)) continue;
        const long long q = sc_quant(y, E);
        hi += q >> 32;
        lo += q & 0xFFFFFFFFll;
    }
    shi[t] = hi;
    slo[t] = lo;
    __syncthreads();
    for (int w = SC_TPB / 2; w > 0; w >>= 1) {
        if (t < (uint32_t)w) {
            shi[t] += shi[t + w];
            slo[t] += slo[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        if (blockIdx.y == 0) scale[s] = E;
        if (shi[0]) atomicAdd(ksum + 2 * s, (unsigned long long)shi[0]);
        if (slo[0]) atomicAdd(ksum + 2 * s + 1, (unsigned long long)slo[0]);
    }
}

// The A operands of one pass (samples s0 .. s0 + 2 tiles): [block of 64 markers][tile][lane] 16 bytes, in the byte order of rl_expand16
// (dword q, byte i = marker 16 g + 4 i + q of the block).  mslot[kb] >= 0: the block holds a column with missing calls, and its
// second operand, the digits of -(3 q_a + q_o), goes to mdig[mslot[kb]].
__global__ __launch_bounds__(64) void k_score_digits(const double* __restrict__ a, const double* __restrict__ o, uint32_t M, uint32_t S,
                                                     uint32_t s0, int tiles, const int* __restrict__ scale, const int32_t* __restrict__ mslot,
                                                     rl_v4i* __restrict__ wdig, rl_v4i* __restrict__ mdig)
{
    const uint32_t kb = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const uint32_t r = lane & 15u, g = lane >> 4, d = r & 7u;
    const uint32_t s = s0 + 2u * t + (r >> 3);
    const int ms = mslot[kb];
    rl_v4i w = {0, 0, 0, 0}, m = {0, 0, 0, 0};
    if (s < S && d < 7u) {
        const int E = scale[s];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t wq = 0, mq = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t j = kb * 64u + 16u * g + 4u * (uint32_t)i + (uint32_t)q;
                if (j >= M) continue;
                const long long qa = sc_quant(a[(size_t)s * M + j], E);
                wq |= (uint32_t)(uint8_t)sc_digit(qa, (int)d) << (8 * i);
                if (ms >= 0) {
                    const long long qw = -(3 * qa + sc_quant(o[(size_t)s * M + j], E));
                    mq |= (uint32_t)(uint8_t)sc_digit(qw, (int)d) << (8 * i);
                }
            }
            w[q] = (int)wq;
            m[q] = (int)mq;
        }
    }
    wdig[((size_t)kb * tiles + t) * 64u + lane] = w;
    if (ms >= 0) mdig[((size_t)ms * tiles + t) * 64u + lane] = m;
}

// 16 x 16 transpose of 2-bit fields over a group of sixteen lanes: lane m, field c  ->  lane c, field m.  Stage h swaps the fields
// (m, c) and (m ^ h, c ^ h) where bit h of m and of c differ; the four stages commute.
__device__ __forceinline__ uint32_t sc_transpose16(uint32_t x, uint32_t m)
{
#define SC_STAGE(h, LO)                                                                                           \
    {                                                                                                             \
        const uint32_t p = (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x1F | ((h) << 10)); /* lane m ^ h */     \
        const bool up = (m & (h)) != 0u;                                                                          \
        const uint32_t r = __builtin_rotateright32(p, up ? 2u * (h) : 32u - 2u * (h));                            \
        const uint32_t k = up ? (LO) : ~(LO); /* the fields this lane takes from its partner */                  \
        x = (r & k) | (x & ~k);                                                                                   \
    }
    SC_STAGE(8, 0x0000FFFFu)
    SC_STAGE(4, 0x00FF00FFu)
    SC_STAGE(2, 0x0F0F0F0Fu)
    SC_STAGE(1, 0x33333333u)
#undef SC_STAGE
    return x;
}

// The product.  Workgroup (x, y): individuals [256 x, 256 x + 256) -- wave w the 64 from 256 x + 64 w --, blocks of 64 markers
// [y kb_per, (y + 1) kb_per); SP samples (SP / 2 tiles).  The A operands of a block are staged in LDS once for the four waves
// (double-buffered: one barrier per block); the codes of the next block and its operands are loaded while this block's MFMAs run.
template <int SP>
__global__ __launch_bounds__(SC_IND) void k_score(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t M, uint32_t n_local,
                                                  uint32_t kb_per, const rl_v4i* __restrict__ wdig, const rl_v4i* __restrict__ mdig,
                                                  const int32_t* __restrict__ mslot, uint32_t S, uint32_t s0,
                                                  unsigned long long* __restrict__ acc)
{
    constexpr int TILES = SP / 2;
    constexpr int NOP = TILES * 64;                          // A operands (16 bytes) per block and kind
    constexpr int NPT = (NOP + SC_IND - 1) / SC_IND;         // of them per thread when staging
    __shared__ rl_v4i sop[2][2][NOP];                        // [buffer][product: codes, missing-call indicator][tile x lane]
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
    rl_v4i rw[NPT], rm[NPT];
    auto load_ops = [&](uint32_t kb) {
        const int ms = mslot[kb];
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const uint32_t idx = tid + (uint32_t)(k * SC_IND);
            if (idx < (uint32_t)NOP) {
                rw[k] = wdig[(size_t)kb * NOP + idx];
                if (ms >= 0) rm[k] = mdig[(size_t)ms * NOP + idx];
            }
        }
        return ms;
    };
    auto store_ops = [&](int buf, int ms) {
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const uint32_t idx = tid + (uint32_t)(k * SC_IND);
            if (idx < (uint32_t)NOP) {
                sop[buf][0][idx] = rw[k];
                if (ms >= 0) sop[buf][1][idx] = rm[k];
            }
        }
    };

    rl_v4i D[4][TILES];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int t = 0; t < TILES; ++t) D[b][t] = rl_v4i{0, 0, 0, 0};

    uint4 cur = load_codes(kb0);
    int ms_cur = load_ops(kb0);
    store_ops(0, ms_cur);
    __syncthreads();
    const uint32_t m16 = lane & 15u;
    for (uint32_t kb = kb0; kb < kb1; ++kb) {
        const int buf = (int)((kb - kb0) & 1u);
        const bool more = kb + 1u < kb1;
        uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
        int ms_nxt = -1;
        if (more) {
            nxt = load_codes(kb + 1u);
            ms_nxt = load_ops(kb + 1u);
        }
        const uint32_t wv[4] = {cur.x, cur.y, cur.z, cur.w};
        rl_v4i z[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) z[b] = rl_expand16(sc_transpose16(wv[b], m16));
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            const rl_v4i A = sop[buf][0][t * 64 + lane];
#pragma unroll
            for (int b = 0; b < 4; ++b) D[b][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, z[b], D[b][t], 0, 0, 0);
        }
        if (ms_cur >= 0) { // (uniform) the block holds a column with missing calls
            rl_v4i zm[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                zm[b].x = z[b].x & (z[b].x >> 1);
                zm[b].y = z[b].y & (z[b].y >> 1);
                zm[b].z = z[b].z & (z[b].z >> 1);
                zm[b].w = z[b].w & (z[b].w >> 1);
            }
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                const rl_v4i A = sop[buf][1][t * 64 + lane];
#pragma unroll
                for (int b = 0; b < 4; ++b) D[b][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, zm[b], D[b][t], 0, 0, 0);
            }
        }
        if (more) store_ops(buf ^ 1, ms_nxt);
        __syncthreads();
        cur = nxt;
        ms_cur = ms_nxt;
    }

    // lane (c, g), tile t: sample s0 + 2 t + (g >> 1), digits 4 (g & 1) .. +3 of individual c of each block of sixteen: the lane puts
    // them together (d0 + 2^8 d1 + 2^16 d2 + 2^24 d3, |.| < 2^55) and adds the part to the entry's low (g even) or high (g odd,
    // units of 2^32) 64-bit sum
    const uint32_t c = lane & 15u, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const uint32_t s = s0 + 2u * (uint32_t)t + (g >> 1);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t i = blockIdx.x * SC_IND + wave * 64u + 16u * (uint32_t)b + c;
            const long long v = (long long)D[b][t][0] + ((long long)D[b][t][1] << 8) + ((long long)D[b][t][2] << 16) + ((long long)D[b][t][3] << 24);
            if (i < n_local && s < S && v != 0)
                __hip_atomic_fetch_add(acc + ((size_t)i * S + s) * 2u + (g & 1u), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// out[i][s] = (hi 2^32 + lo) 2^-E_s, hi and lo with the constant sum_j q_o added, rounded once (round_halves)
__global__ __launch_bounds__(SC_TPB) void k_score_final(const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ ksum,
                                                        const int* __restrict__ scale, uint32_t n_local, uint32_t S, double* __restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * SC_TPB + threadIdx.x;
    if (k >= (uint64_t)n_local * S) return;
    const uint32_t s = (uint32_t)(k % S);
    const long long lo = (long long)(acc[2 * k] + ksum[2 * s + 1]);
    const long long hi = (long long)(acc[2 * k + 1] + ksum[2 * s]);
    out[k] = round_halves(hi, lo, scale[s]);
}

} // namespace

static int score_sp_for(const hgibbs_ctx* h, int S)
{
    if (h->score_sp) return h->score_sp;
    // measured at N = 100 000, M = 1 000 000: eight samples a pass beat sixteen (half the registers, two
    // workgroups per compute unit instead of one) and four at every S >= 8; below that the smallest pass that holds them all
    int sp = 2;
    while (sp < S && sp < 8) sp *= 2;
    return sp;
}

template <int SP>
static void score_launch(hgibbs_ctx* h, dim3 grid, uint32_t kb_per, const rl_v4i* wdig, const rl_v4i* mdig, const int32_t* mslot,
                         uint32_t S, uint32_t s0, unsigned long long* acc)
{
    k_score<SP><<<grid, SC_IND, 0, h->stream>>>(h->bed, h->stride, h->M, h->n_local, kb_per, wdig, mdig, mslot, S, s0, acc);
}

// The work buffers of the pipeline for up to `smax` weight vectors, allocated once by the caller (hgibbs_score per call, hgibbs_pca
// per call for all its iterations): everything but the weights and the results.
struct ScoreWs {
    DevBuf<int> scale;
    DevBuf<unsigned long long> maxbits, acc;
    unsigned long long* ksum = nullptr; // (lies inside maxbits)
    DevBuf<uint32_t> bad;
    DevBuf<int32_t> mslot;
    DevBuf<rl_v4i> wdig, mdig;
    int smax = 0, sp = 0;
};

static size_t score_ws_bytes(const hgibbs_ctx* h, int smax)
{
    const uint32_t nkb = (h->M + 63u) / 64u;
    const int tiles = score_sp_for(h, smax) / 2;
    return 2 * (size_t)nkb * tiles * 64 * sizeof(rl_v4i) + (size_t)h->n_local * smax * 2 * sizeof(unsigned long long) + (size_t)nkb * 4 + 4096;
}

// Allocates the buffers and reads the marker counts once (blocks of 64 markers with a column that has missing calls); synchronises
static int score_ws_create(hgibbs_ctx* h, ScoreWs& b, int smax)
{
    const uint32_t M = h->M, n = h->n_local, nkb = (M + 63u) / 64u;
    const int sp = score_sp_for(h, smax), tiles = sp / 2;
    // blocks of 64 markers with a column that has missing calls: from the counts of hgibbs_marker_stats when they exist (summed
    // over ranks: a superset of this shard's, which costs only a product over zeros), else from this shard's own counts (no collective)
    if (!h->have_stats && h->nranks <= 1 && !h->comm && compute_stats(h)) return 1;
    if (!h->have_stats) {
        k_counts<<<h->M, BLOCK, 0, h->stream>>>(h->bed, h->stride, h->n_pad, h->n_local, h->counts, h->M); // (local; compute_stats redoes them)
        HIP_TRY(hipGetLastError());
    }
    std::vector<uint8_t> miss;
    if (missing_tiles(h, 64u, miss)) return 1;
    std::vector<int32_t> mslot(nkb, -1); // the slots of the blocks with missing calls, in marker order
    uint32_t nm = 0;
    for (uint32_t kb = 0; kb < nkb; ++kb)
        if (miss[kb]) mslot[kb] = (int32_t)nm++;
    b.smax = smax;
    b.sp = sp;
    if (b.scale.alloc((size_t)smax)) return 1;
    if (b.maxbits.alloc((size_t)smax * 3)) return 1; // max, then the two halves of sum_j q_o
    if (b.bad.alloc(1)) return 1;
    if (b.mslot.alloc(nkb)) return 1;
    if (b.wdig.alloc((size_t)nkb * tiles * 64)) return 1;
    if (nm && b.mdig.alloc((size_t)nm * tiles * 64)) return 1;
    if (b.acc.alloc((size_t)n * smax * 2)) return 1;
    HIP_TRY(hipMemsetAsync(b.bad, 0, sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemcpyAsync(b.mslot, mslot.data(), (size_t)nkb * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream)); // (mslot is a local)
    return 0;
}

// Zeroes the sums of one product (stream-ordered, no synchronisation); with clear_bad = false the flag of non-finite weights, zero
// from score_ws_create, is left to gather over several products
static int score_dev_clear(hgibbs_ctx* h, ScoreWs& b, int S, bool clear_bad = true)
{
    b.ksum = b.maxbits + S;
    if (clear_bad) HIP_TRY(hipMemsetAsync(b.bad, 0, sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(b.maxbits, 0, (size_t)S * 3 * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(b.acc, 0, (size_t)h->n_local * S * 2 * sizeof(unsigned long long), h->stream));
    return 0;
}

// The kernels of one product on device pointers: da, dov (S x M, vector-major) -> dout (n_local x S).  Stream-ordered: no allocation,
// no synchronisation; b.bad is left for the caller to read.  score_dev_clear comes first.  S <= smax, with the pass size of smax.
static int score_dev_run(hgibbs_ctx* h, ScoreWs& b, int S, const double* da, const double* dov, double* dout)
{
    const uint32_t M = h->M, n = h->n_local, nkb = (M + 63u) / 64u;
    const int sp = b.sp, tiles = sp / 2;
    const size_t NS = (size_t)n * S;
    {
        // workgroups per sample for the scale: about 2048 in all, at least 2048 markers each (grid y: at most 65535)
        const uint32_t per = std::max<uint32_t>(1u, std::min<uint32_t>((M + 2047u) / 2048u, (2048u + (uint32_t)S - 1u) / (uint32_t)S));
        k_score_max<<<dim3(S, per), SC_TPB, 0, h->stream>>>(da, dov, M, b.maxbits, b.bad);
        HIP_TRY(hipGetLastError());
        k_score_ksum<<<dim3(S, per), SC_TPB, 0, h->stream>>>(dov, M, b.maxbits, b.scale, b.ksum);
        HIP_TRY(hipGetLastError());
    }

    // grid: workgroups of 256 individuals x ranges of marker blocks, enough of them to fill the device (8 per compute unit); the
    // ranges never exceed SC_KB_MAX blocks (i32 headroom of the digit sums)
    const uint32_t gx = h->n_pad / SC_IND;
    uint32_t want = (8u * (uint32_t)h->num_cu + gx - 1u) / gx, kb_per = 0;
    if (h->score_ranges) want = std::min(want, (uint32_t)h->score_ranges);
    const uint32_t gy = split_ranges(nkb, want, SC_KB_MAX, kb_per);
    for (uint32_t s0 = 0; s0 < (uint32_t)S; s0 += (uint32_t)sp) {
        k_score_digits<<<dim3(nkb, tiles), 64, 0, h->stream>>>(da, dov, M, (uint32_t)S, s0, tiles, b.scale, b.mslot, b.wdig, b.mdig);
        HIP_TRY(hipGetLastError());
        const dim3 grid(gx, gy);
        switch (sp) {
        case 2: score_launch<2>(h, grid, kb_per, b.wdig, b.mdig, b.mslot, (uint32_t)S, s0, b.acc); break;
        case 4: score_launch<4>(h, grid, kb_per, b.wdig, b.mdig, b.mslot, (uint32_t)S, s0, b.acc); break;
        case 8: score_launch<8>(h, grid, kb_per, b.wdig, b.mdig, b.mslot, (uint32_t)S, s0, b.acc); break;
        default: score_launch<16>(h, grid, kb_per, b.wdig, b.mdig, b.mslot, (uint32_t)S, s0, b.acc); break;
        }
        HIP_TRY(hipGetLastError());
    }
    k_score_final<<<(uint32_t)((NS + SC_TPB - 1) / SC_TPB), SC_TPB, 0, h->stream>>>(b.acc, b.ksum, b.scale, n, (uint32_t)S, dout);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int hgibbs_score(hgibbs_t h, int S, const double* a, const double* o, double* out)
{
    if (op_guard(h, "hgibbs_score", nullptr)) return 1;
    if (S <= 0) return fail("hgibbs_score: S = %d, needs at least one weight vector", S);
    if (!a || !o || !out) return fail("hgibbs_score: null argument");
    HIP_TRY(hipSetDevice(h->device));
    const uint32_t M = h->M, n = h->n_local;

    // a thin wrapper around the device-pointer pipeline: its own workspace, the weights in, the results out
    ScoreWs ws;
    DevBuf<double> da, dov, dout;
    const size_t SM = (size_t)S * M, NS = (size_t)n * S;
    if (score_ws_create(h, ws, S)) return 1;
    if (da.alloc(SM) || dov.alloc(SM) || dout.alloc(NS)) return 1;
    HIP_TRY(hipMemcpyAsync(da, a, SM * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dov, o, SM * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (score_dev_clear(h, ws, S)) return 1;

    // device time from here to the rounded result: every kernel of the call, not the host copies around it
    if (lap_begin(h)) return 1;
    if (score_dev_run(h, ws, S, da, dov, dout)) return 1;
    if (lap_mark(h)) return 1;
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, ws.bad, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (bad) return fail("hgibbs_score: a weight (a or o) is not finite"); // (out untouched; what the kernels made of it is dropped)
    HIP_TRY(hipMemcpy(out, dout, NS * sizeof(double), hipMemcpyDeviceToHost));
    double ms = 0.0;
    if (lap_read(h, ms)) return 1;
    h->score_ms = ms;
    return 0;
}

extern "C" int hgibbs_last_score_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_score_ms: null argument");
    *ms = h->score_ms;
    return 0;
}
