// Windowed LD of the loaded markers: for markers j and q = j + d, d = 1 .. W, the four exact integer sums
//
//     G = sum g_j g_q,   Bjq = sum g_j [q called],   Bqj = sum g_q [j called],   D = sum [j called][q called]      (g = 0 at a missing call)
//
// over the handle's individuals, and from them, in ONE f64 formula per pair, r = x_j'x_q / (N - 1) with the chain's own standardisation
// (x_j'x_q = mstd_j mstd_q (G - m_q Bjq - m_j Bqj + m_j m_q D)).
//
//   operands  A: 16 markers (rows), B: 16 other markers (columns), both BED dwords in their stored layout, each expanded by
//             rl_expand16 (hg_streamer2.hip.h).  Lane (c, k) of a k-step holds dword k of marker c's slice: A and B take the same
//             individuals in the same k slots, so the product is a sum over individuals with no transpose.
//   result    D[row][col] of v_mfma_i32_16x16x64_i8: lane (c, k), register r = marker 4 k + r of the A tile against marker c of the B tile.
//   clean     a pair of tiles whose 32 columns have no missing call takes ONE product of the codes (0, 1, 2): G.  Bjq, Bqj and D then
//             follow from the marker-stats counts (sum g_j, sum g_q, n_local), in k_ld_final.
//   missing   a pair of tiles with a missing call in one of its columns takes four products of g (= the code with 3 -> 0) and the
//             indicator [called] on either side: G, Bjq, Bqj, D.
//   padding   slots past n_local in the dword that holds n_local are masked (code 0 in a clean product, code 3 in the four-product
//             form), and the loop ends at that dword: padding counts nowhere, not in D either.
//   exact     every i32 partial is at most 4 x (individuals of the workgroup's range) (g <= 2, [called] <= 1), so n_local < 2^29 keeps it
//             exact; the workgroups' parts meet in 64-bit atomic adds (order-free).  The sums, and r, do not depend on tiling,
//             workgroups, the individual split (option ld_split), m0 / count chunking or launch order.
//   reuse     workgroup = LD_WAVES waves = LD_WAVES consecutive A tiles, and one pass of LD_QP B tiles per A tile (grid z: the passes
//             that cover the window).  Per slice of 512 individuals the workgroup stages its A tiles and the LD_QP + LD_WAVES - 1 B
//             tiles they share in LDS (double-buffered, one barrier a slice) and every wave runs its LD_QP x 8 products from there.
#pragma once

namespace {

constexpr int LD_WAVES = 4;                  // A tiles (waves) per workgroup
constexpr int LD_QP = 9;                     // B tiles per A tile and pass (W = 128 in one pass; the staging divides over the threads)
constexpr int LD_SUBD = 32;                  // dwords of a column per slice: 512 individuals, 128 bytes, eight k-steps
constexpr int LD_BT = LD_QP + LD_WAVES - 1;  // B tiles staged per slice
constexpr int LD_COLS = 16 * (LD_WAVES + LD_BT); // columns staged per slice (A region, then B region)
constexpr int LD_UNITS = LD_COLS * LD_SUBD / 4;  // 16-byte units of them
constexpr int LD_UPT = LD_UNITS / (LD_WAVES * 64); // units per thread
static_assert(LD_UNITS % (LD_WAVES * 64) == 0, "staging must divide over the threads");
constexpr uint32_t LD_WMAX = 4096;           // widest window (the host chunks markers so that a piece holds at most 2^24 pairs)
constexpr uint32_t LD_NMAX = 1u << 29;       // n_local below this keeps 4 x n in an i32
constexpr int LD_TPB = 256;

__device__ __forceinline__ uint32_t ld_valid_mask(uint32_t n_local, uint32_t dw)
{
    const int64_t v = (int64_t)n_local - 16 * (int64_t)dw; // individuals of this dword inside n_local
    if (v >= 16) return 0xFFFFFFFFu;
    if (v <= 0) return 0u;
    return (1u << (2 * (uint32_t)v)) - 1u;
}

// one product of the expanded forms of a and b into acc
__device__ __forceinline__ rl_v4i ld_mm(const rl_v4i& a, const rl_v4i& b, const rl_v4i& acc)
{
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
}

// g (code 3 -> 0) and [called] of sixteen expanded codes
__device__ __forceinline__ void ld_forms(const rl_v4i& z, rl_v4i& g, rl_v4i& c)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int m = z[e] & (z[e] >> 1) & 0x01010101; // [code == 3] per byte
        g[e] = z[e] ^ (m * 3);
        c[e] = m ^ 0x01010101;
    }
}

// Workgroup (x, y, z): slices [x sub_per, (x + 1) sub_per) of 512 individuals, A tiles tJ0 + 0 .. LD_WAVES - 1 with tJ0 = t0 + LD_WAVES y,
// B tiles (A tile) + LD_QP z + 0 .. LD_QP - 1 of the nq that cover the window.  MISS: some tile pair may take the four-product form.
template <bool MISS>
__global__ __launch_bounds__(LD_WAVES * 64) void k_ld(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t M, uint32_t n_local,
                                                      uint32_t t0, uint32_t t1, uint32_t nq, uint32_t sub_per, uint32_t n_sub,
                                                      const uint8_t* __restrict__ tmiss, uint32_t W, uint32_t m0, uint32_t count,
                                                      unsigned long long* __restrict__ acc)
{
    __shared__ uint4 stage[2][LD_UNITS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t s0 = blockIdx.x * sub_per, s1 = min(n_sub, s0 + sub_per);
    if (s0 >= s1) return; // (uniform)
    const uint32_t tJ0 = t0 + LD_WAVES * blockIdx.y;
    const uint32_t qoff = LD_QP * blockIdx.z;       // first B tile of this pass, relative to the A tile
    const uint32_t qlo = tJ0 + qoff;                // first staged B tile
    const uint32_t tj = tJ0 + wave;                 // this wave's A tile
    const bool wave_on = tj < t1;                   // (wave-uniform)
    const uint32_t nqp = min((uint32_t)LD_QP, nq - qoff); // B tiles of this pass per A tile
    // A tiles come from the B region when the pass starts at the A tiles themselves (tile tJ0 + w is B tile w there)
    const uint32_t ua = blockIdx.z ? 16u * LD_WAVES * (LD_SUBD / 4) : 0u; // units of the A region staged
    const uint32_t ub = 16u * min((uint32_t)LD_BT, nqp + LD_WAVES - 1u) * (LD_SUBD / 4);
    const uint32_t abase = blockIdx.z ? 0u : 16u * LD_WAVES * (LD_SUBD / 4); // A region's first unit in LDS

    uint4 pre[LD_UPT];
    auto load = [&](uint32_t sub) {
#pragma unroll
        for (int k = 0; k < LD_UPT; ++k) {
            const uint32_t u = tid + (uint32_t)k * (LD_WAVES * 64);
            uint32_t col = 0xFFFFFFFFu;
            if (u < ua) col = 16u * tJ0 + u / (LD_SUBD / 4);
            else if (u >= 16u * LD_WAVES * (LD_SUBD / 4) && u - 16u * LD_WAVES * (LD_SUBD / 4) < ub)
                col = 16u * qlo + (u - 16u * LD_WAVES * (LD_SUBD / 4)) / (LD_SUBD / 4);
            uint4 v = make_uint4(0u, 0u, 0u, 0u); // (markers past M: code 0, never written out)
            if (col < M) v = *reinterpret_cast<const uint4*>(bed + (uint64_t)col * stride + (uint64_t)sub * (LD_SUBD * 4) + (u % (LD_SUBD / 4)) * 16u);
            pre[k] = v;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int k = 0; k < LD_UPT; ++k) stage[buf][tid + (uint32_t)k * (LD_WAVES * 64)] = pre[k];
    };

    constexpr int NA = MISS ? 4 : 1;
    rl_v4i D[LD_QP][NA];
#pragma unroll
    for (int t = 0; t < LD_QP; ++t)
#pragma unroll
        for (int a = 0; a < NA; ++a) D[t][a] = rl_v4i{0, 0, 0, 0};

    const uint32_t c = lane & 15u, k4 = lane >> 4;
    const bool amiss = MISS && wave_on && tmiss[tj];
    bool bmiss[LD_QP];
#pragma unroll
    for (int t = 0; t < LD_QP; ++t) bmiss[t] = MISS && wave_on && (uint32_t)t < nqp && (amiss || tmiss[tj + qoff + (uint32_t)t]);

    load(s0);
    store(0);
    __syncthreads();
    for (uint32_t sub = s0; sub < s1; ++sub) {
        const int buf = (int)((sub - s0) & 1u);
        const bool more = sub + 1u < s1;
        if (more) load(sub + 1u);
        if (wave_on) {
            // lane (c, k): dwords 8 k .. 8 k + 7 of the slice of marker c; k-step i takes dword 8 k + i
            const uint4* sa = &stage[buf][abase + (wave * 16u + c) * (LD_SUBD / 4) + 2u * k4];
            const uint4 a0 = sa[0], a1 = sa[1];
            uint32_t aw[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            uint32_t vm[8];
            const bool edge = (uint64_t)(sub + 1u) * (LD_SUBD * 16) > n_local; // (uniform) the slice holds n_local
#pragma unroll
            for (int i = 0; i < 8; ++i) vm[i] = edge ? ld_valid_mask(n_local, sub * LD_SUBD + 8u * k4 + (uint32_t)i) : 0xFFFFFFFFu;
            rl_v4i za[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) za[i] = rl_expand16(aw[i] & vm[i]);
#pragma unroll
            for (int t = 0; t < LD_QP; ++t) {
                if ((uint32_t)t < nqp) { // (uniform)
                    const uint4* sb = &stage[buf][16u * LD_WAVES * (LD_SUBD / 4) + ((wave + (uint32_t)t) * 16u + c) * (LD_SUBD / 4) + 2u * k4];
                    const uint4 b0 = sb[0], b1 = sb[1];
                    const uint32_t bw[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
                    if (!bmiss[t]) { // (uniform) one product of the codes
#pragma unroll
                        for (int i = 0; i < 8; ++i) D[t][0] = ld_mm(za[i], rl_expand16(bw[i] & vm[i]), D[t][0]);
                    } else if constexpr (MISS) { // g and [called] on either side; padding as missing calls
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            rl_v4i ga, ca, gb, cb;
                            ld_forms(rl_expand16(aw[i] | ~vm[i]), ga, ca);
                            ld_forms(rl_expand16(bw[i] | ~vm[i]), gb, cb);
                            D[t][0] = ld_mm(ga, gb, D[t][0]);
                            D[t][1] = ld_mm(ga, cb, D[t][1]);
                            D[t][2] = ld_mm(ca, gb, D[t][2]);
                            D[t][3] = ld_mm(ca, cb, D[t][3]);
                        }
                    }
                }
            }
        }
        if (more) store(buf ^ 1);
        __syncthreads();
    }
    if (!wave_on) return;

    // lane (c, k), register r: A marker j = 16 tj + 4 k + r, B marker q = 16 (tj + qoff + t) + c
#pragma unroll
    for (int t = 0; t < LD_QP; ++t) {
        if ((uint32_t)t >= nqp) continue;
        const uint32_t q = 16u * (tj + qoff + (uint32_t)t) + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t j = 16u * tj + 4u * k4 + (uint32_t)r;
            if (q <= j || q - j > W || j < m0 || j - m0 >= count || q >= M) continue;
            unsigned long long* p = acc + (((uint64_t)(j - m0) * W + (q - j - 1u)) << 2);
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const int v = D[t][a][r];
                if ((a == 0 || bmiss[t]) && v) __hip_atomic_fetch_add(p + a, (unsigned long long)(long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// The four sums of pair (j, q), q < M, from its accumulators a4 (the clean pairs' Bjq, Bqj, D from the counts), and r in ONE f64 formula
// (NaN where an mstd is not finite).  hgibbs_ld and hgibbs_ld_scores (hg_ldscore.hip.h) both take r from here.
__device__ __forceinline__ double ld_pair_r(const unsigned long long* __restrict__ a4, const unsigned long long* __restrict__ counts,
                                            const double* __restrict__ mave, const double* __restrict__ mstd, uint32_t j, uint32_t q,
                                            uint32_t n_local, uint32_t N, long long& G, long long& Bjq, long long& Bqj, long long& Dc)
{
    const unsigned long long* cj = counts + 3ull * j;
    const unsigned long long* cq = counts + 3ull * q;
    G = (long long)a4[0];
    if (cj[2] == 0 && cq[2] == 0) {
        Bjq = (long long)(cj[0] + 2 * cj[1]);
        Bqj = (long long)(cq[0] + 2 * cq[1]);
        Dc = (long long)n_local;
    } else {
        Bjq = (long long)a4[1];
        Bqj = (long long)a4[2];
        Dc = (long long)a4[3];
    }
    const double sj = mstd[j], sq = mstd[q], mj = mave[j], mq = mave[q];
    if (isfinite(sj) && isfinite(sq))
        return sj * sq * ((double)G - mq * (double)Bjq - mj * (double)Bqj + mj * mq * (double)Dc) / (double)(N - 1u);
    return __builtin_nan("");
}

// One thread per pair: the sums and r of ld_pair_r (r NaN past M)
__global__ __launch_bounds__(LD_TPB) void k_ld_final(const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ counts,
                                                     const double* __restrict__ mave, const double* __restrict__ mstd, uint32_t M, uint32_t n_local,
                                                     uint32_t N, uint32_t W, uint32_t m0, uint32_t count, double* __restrict__ r,
                                                     long long* __restrict__ sums)
{
    const uint64_t k = (uint64_t)blockIdx.x * LD_TPB + threadIdx.x;
    if (k >= (uint64_t)count * W) return;
    const uint32_t j = m0 + (uint32_t)(k / W), q = j + 1u + (uint32_t)(k % W);
    long long G = 0, Bjq = 0, Bqj = 0, Dc = 0;
    double v = __builtin_nan("");
    if (q < M) v = ld_pair_r(acc + 4 * k, counts, mave, mstd, j, q, n_local, N, G, Bjq, Bqj, Dc);
    if (r) r[k] = v;
    if (sums) {
        sums[4 * k] = G;
        sums[4 * k + 1] = Bjq;
        sums[4 * k + 2] = Bqj;
        sums[4 * k + 3] = Dc;
    }
}

// ---- the band frame: the host code that hgibbs_ld, hgibbs_ld_scores (hg_ldscore.hip.h) and hgibbs_ld_mask
// (hg_ldmask.hip.h) share.  They run k_ld<MISS> on pieces of the same band and differ in what they do with a piece's sums.

// The checks every entry point makes first.  ms: the caller's two timers in the handle, zeroed once the handle is known to be usable, so
// that a call refused after that reads as 0 ms (null: hgibbs_ld, whose ld_ms keeps the last finished call's time)
int ld_band_check(hgibbs_ctx* h, const char* who, uint32_t W, double (hgibbs_ctx::*ms)[2])
{
    if (op_guard(h, who, "the band is not exchanged between ranks")) return 1;
    if (ms) (h->*ms)[0] = (h->*ms)[1] = 0.0;
    if (W == 0 || W > LD_WMAX) return fail("%s: W = %u, must be in [1, %u]", who, W, LD_WMAX);
    if (h->n_local >= LD_NMAX) return fail("%s: %u individuals, at most %u (i32 partial sums)", who, h->n_local, LD_NMAX - 1u);
    return 0;
}

// ah[j] = the pairs ahead of marker j: ahead[j], refused where it leaves the window or the markers (ahead = NULL: min(W, M - 1 - j))
int ld_ahead(const char* who, uint32_t M, uint32_t W, const uint32_t* ahead, std::vector<uint32_t>& ah)
{
    ah.resize(M);
    for (uint32_t j = 0; j < M; ++j) {
        if (!ahead) {
            ah[j] = std::min(W, M - 1u - j);
            continue;
        }
        if (ahead[j] > W) return fail("%s: ahead[%u] = %u is above W = %u", who, j, ahead[j], W);
        if ((uint64_t)j + ahead[j] >= M) return fail("%s: marker %u + ahead[%u] = %u is past the last marker (M = %u)", who, j, j, ahead[j], M);
        ah[j] = ahead[j];
    }
    return 0;
}

// Band rows of a piece: at most 2^24 pairs (the device's sums: 512 MiB; that bound on rows rounded up to 16) and 2^20 rows (grid y);
// rows_opt (options ldscore_piece, ldmask_piece; 0: none) fixes the rows, rounded up to 16; at most `count` rounded up to 16, at least 16.
// hgibbs_ld (rows_opt = 0) cut max(16, min(count, 2^20, cap)) before the frame: the same pieces for every input, since the two bounds are
// multiples of 16 (where one of them is at most count, both formulas give it; where count is below both, both give one piece of count rows).
uint32_t ld_piece_rows(uint32_t W, int rows_opt, uint32_t count)
{
    uint64_t piece = std::min<uint64_t>(((1ull << 24) / W + 15u) / 16u * 16u, 1ull << 20);
    if (rows_opt) piece = std::min<uint64_t>(piece, ((uint64_t)rows_opt + 15u) / 16u * 16u);
    return (uint32_t)std::max<uint64_t>(16u, std::min<uint64_t>(piece, ((uint64_t)count + 15u) / 16u * 16u));
}

// Flags of tiles of sixteen markers that k_ld may read: the markers' and the widest window's past them
size_t ld_flag_count(uint32_t M) { return (size_t)((M + 15u) / 16u) + LD_WMAX / 16 + LD_QP + LD_WAVES; }

// What the pieces of a call share on the device: the missing-tile flags (ld_flag_count(M) bytes) and the sums of one piece of `piece`
// rows (ld_piece_rows), 32 bytes a pair.  The caller has set the device and run compute_stats; its own buffers come after these.
struct LdBand {
    DevBuf<uint8_t> dmiss;
    DevBuf<unsigned long long> acc;
    uint32_t W = 0, piece = 0;
};

int ld_band_open(hgibbs_ctx* h, uint32_t W, uint32_t piece, LdBand& b)
{
    // tiles of sixteen markers with a missing call in a column (the counts of hgibbs_marker_stats)
    std::vector<uint8_t> tmiss;
    if (missing_tiles(h, 16u, tmiss)) return 1;
    tmiss.resize(ld_flag_count(h->M), 0); // (the window's tiles past M read as clean)
    b.W = W;
    b.piece = piece;
    if (b.dmiss.alloc(tmiss.size()) || b.acc.alloc((size_t)piece * W * 4)) return 1;
    HIP_TRY(hipMemcpy(b.dmiss, tmiss.data(), tmiss.size(), hipMemcpyHostToDevice));
    return 0;
}

// The band rows [m0, m0 + count) in pieces: per piece [p0, p0 + pc) the zeroing and the products, then step(p0, pc, acc), which does with
// the piece's sums what the caller is there for.  The step is entered with the products' lap open (lap_begin, the zeroing, k_ld) and
// closes it itself: after its own kernel into one timer (hgibbs_ld), or at once into the products' timer, then a second lap for its reduce.
template <class Step>
int ld_band_pieces(hgibbs_ctx* h, const LdBand& b, uint32_t m0, uint32_t count, Step&& step)
{
    const uint32_t M = h->M, W = b.W, piece = b.piece;
    const uint32_t n_sub = (h->n_local + LD_SUBD * 16 - 1) / (LD_SUBD * 16);
    const uint32_t nq = (W + 15u) / 16u + 1u; // B tiles per A tile: A tile t pairs with tiles t .. t + floor((W + 15) / 16)
    for (uint32_t p0 = m0; p0 < m0 + count; p0 += piece) {
        const uint32_t pc = std::min(piece, m0 + count - p0);
        const uint32_t t0 = p0 / 16u, t1 = (p0 + pc - 1u) / 16u + 1u;
        const uint32_t gy = (t1 - t0 + LD_WAVES - 1u) / LD_WAVES, gz = (nq + LD_QP - 1u) / LD_QP;
        // individual ranges: enough workgroups for eight per compute unit (option ld_split fixes the number)
        uint32_t sub_per = 0;
        const uint32_t gx = split_ranges(n_sub, h->ld_split ? (uint32_t)h->ld_split : (8u * (uint32_t)h->num_cu + gy * gz - 1u) / (gy * gz), NO_CAP, sub_per);
        if (lap_begin(h)) return 1;
        HIP_TRY(hipMemsetAsync(b.acc, 0, (size_t)pc * W * 4 * sizeof(unsigned long long), h->stream));
        const dim3 grid(gx, gy, gz);
        if (h->any_missing)
            k_ld<true><<<grid, LD_WAVES * 64, 0, h->stream>>>(h->bed, h->stride, M, h->n_local, t0, t1, nq, sub_per, n_sub, b.dmiss, W, p0, pc, b.acc);
        else
            k_ld<false><<<grid, LD_WAVES * 64, 0, h->stream>>>(h->bed, h->stride, M, h->n_local, t0, t1, nq, sub_per, n_sub, b.dmiss, W, p0, pc, b.acc);
        HIP_TRY(hipGetLastError());
        if (step(p0, pc, (unsigned long long*)b.acc)) return 1;
    }
    return 0;
}

} // namespace

extern "C" int hgibbs_ld(hgibbs_t h, uint32_t m0, uint32_t count, uint32_t W, double* r_host, int64_t* sums_host)
{
    if (ld_band_check(h, "hgibbs_ld", W, nullptr)) return 1;
    if ((uint64_t)m0 + count > h->M) return fail("hgibbs_ld: markers [%u, %llu) out of range (M = %u)", m0, (unsigned long long)m0 + count, h->M);
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;
    LdBand band;
    if (ld_band_open(h, W, ld_piece_rows(W, 0, count), band)) return 1;
    DevBuf<double> r;
    DevBuf<long long> sums;
    const size_t np = (size_t)band.piece * W;
    if (r_host && r.alloc(np)) return 1;
    if (sums_host && sums.alloc(np * 4)) return 1;

    double total_ms = 0.0;
    // the step of a piece: r and the sums of its pairs inside the products' lap, and the copies out
    auto finish = [&](uint32_t p0, uint32_t pc, const unsigned long long* acc) -> int {
        const uint64_t npc = (uint64_t)pc * W;
        k_ld_final<<<(uint32_t)((npc + LD_TPB - 1) / LD_TPB), LD_TPB, 0, h->stream>>>(acc, h->counts, h->mave, h->mstd, h->M, h->n_local, h->n_global,
                                                                                       W, p0, pc, r, sums);
        HIP_TRY(hipGetLastError());
        if (lap_end(h, total_ms)) return 1;
        const size_t off = (size_t)(p0 - m0) * W;
        if (r_host) HIP_TRY(hipMemcpy(r_host + off, r, npc * sizeof(double), hipMemcpyDeviceToHost));
        if (sums_host) HIP_TRY(hipMemcpy(sums_host + off * 4, sums, npc * 4 * sizeof(long long), hipMemcpyDeviceToHost));
        return 0;
    };
    if (ld_band_pieces(h, band, m0, count, finish)) return 1;
    h->ld_ms = total_ms;
    return 0;
}

extern "C" int hgibbs_last_ld_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_ld_ms: null argument");
    *ms = h->ld_ms;
    return 0;
}
