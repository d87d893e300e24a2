// LD scores of the loaded markers: l_jc = a_jc + sum_{q != j in j's window} a_qc t_jq, with t = r^2 or, adjusted,
// r^2 - (1 - r^2) / (N - 2), r the r of hgibbs_ld (ld_pair_r, hg_ld.hip.h) and a_qc bit c of annot[q].
//
//   pairs     (j, q), j < q, is in the window iff q - j <= ahead[j]; it counts for both of its markers.  A pair with a marker whose mstd
//             is not finite counts for neither.
//   products  the band frame of hg_ld.hip.h (ld_band_pieces): k_ld<MISS>, unchanged, fills the 64-bit sums of a piece of band rows.
//   reduce    k_lds_reduce replaces k_ld_final: a workgroup takes LS_ROWS band rows x LS_OFFS offsets of the piece.  A wave takes one row
//             at a time, lane = offset: 64 lanes read 2 KiB of sums in a row, form t and fx = llrint(t 2^44).
//             forward   L[j][c] += sum_q a_qc fx: C = 1 is one sum across the wave; otherwise lane c sums the 64 pairs, the pair's fx and
//                       annotation word broadcast by v_readlane (no LDS), and lanes c < C add 8 C contiguous bytes to row j.
//             backward  L[q][c] += a_jc fx: the tile's targets are the LS_SPAN = 127 markers behind its first row; they are summed in LDS
//                       (64-bit LDS adds, column-major [c][slot]: a wave's 64 lanes hit 64 consecutive slots, no bank conflict) and
//                       flushed once a tile, one global add per touched (q, c), consecutive threads on consecutive c of one q.
//   exact     every sum is a sum of the integers fx (|fx| <= 2^44, at most 8193 terms with the self term: below 2^58), added with integer
//             adds in LDS and in global memory: L does not depend on pieces, ld_split, tiles or launch order.  k_lds_final adds the
//             self term a_jc 2^44, converts once ((double)L 2^-44) and writes NaN rows.
//   memory    the band, r and the sums never leave the device: the host sends ahead and annot and receives M x C doubles.
#pragma once

namespace {

constexpr int LS_ROWS = 64;                        // band rows of a tile
constexpr int LS_OFFS = 64;                        // offsets of a tile: one per lane
constexpr int LS_SPAN = LS_ROWS + LS_OFFS - 1;     // backward targets of a tile
constexpr int LS_WAVES = 4;
constexpr int LS_FRAC = 44;                        // fixed point: t 2^44
constexpr uint32_t LS_CMAX = 64;                   // annotations at most (bits of a word; 64 x LS_SPAN x 8 bytes of LDS = 65 024)

__device__ __forceinline__ long long ls_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ unsigned long long ls_uniform(unsigned long long v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// Workgroup (x, y): offsets 64 x .. 64 x + 63 (distance = offset + 1) of band rows p0 + 64 y .. + 63 of the piece [p0, p0 + pc).
// ONE: C = 1 (bit 0 of annot is the only column)
template <bool ONE>
__global__ __launch_bounds__(LS_WAVES * 64) void k_lds_reduce(const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ counts,
                                                              const double* __restrict__ mave, const double* __restrict__ mstd,
                                                              const uint32_t* __restrict__ ahead, const unsigned long long* __restrict__ annot,
                                                              uint32_t M, uint32_t n_local, uint32_t N, uint32_t W, uint32_t p0, uint32_t pc, uint32_t C,
                                                              int adjust, unsigned long long* __restrict__ L)
{
    extern __shared__ unsigned long long ls_back[]; // [C][LS_SPAN]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t d0 = LS_OFFS * blockIdx.x, jt0 = p0 + LS_ROWS * blockIdx.y;
    for (uint32_t i = tid; i < C * LS_SPAN; i += LS_WAVES * 64) ls_back[i] = 0ull;
    __syncthreads();

    const uint32_t o = d0 + lane;
    for (uint32_t row = wave; row < (uint32_t)LS_ROWS; row += LS_WAVES) {
        const uint32_t j = jt0 + row;
        if (j - p0 >= pc) break; // (uniform)
        const uint32_t ah = ahead[j];
        if (ah <= d0) continue; // (uniform) the row's window ends before this tile
        long long fx = 0;
        unsigned long long aq = 0ull;
        if (o < ah) { // q = j + o + 1 <= j + ahead[j] < M
            const uint32_t q = j + o + 1u;
            long long G, Bjq, Bqj, Dc;
            const double r = ld_pair_r(acc + (((uint64_t)(j - p0) * W + o) << 2), counts, mave, mstd, j, q, n_local, N, G, Bjq, Bqj, Dc);
            if (r == r) {
                const double r2 = r * r;
                const double t = adjust ? r2 - (1.0 - r2) / (double)(N - 2u) : r2;
                fx = llrint(t * (double)(1ll << LS_FRAC));
                aq = annot[q];
            }
        }
        if (__ballot(fx != 0) == 0ull) continue; // (uniform)
        const unsigned long long aj = ls_uniform(annot[j]);

        // forward: row j takes a_qc fx
        if constexpr (ONE) {
            const long long s = ls_wave_sum((aq & 1ull) ? fx : 0ll);
            if (lane == 0u && s) __hip_atomic_fetch_add(L + j, (unsigned long long)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const int flo = (int)(uint32_t)fx, fhi = (int)(uint32_t)((unsigned long long)fx >> 32);
            const int alo = (int)(uint32_t)aq, ahi = (int)(uint32_t)(aq >> 32);
            long long s = 0;
#pragma unroll
            for (int d = 0; d < 64; ++d) {
                const unsigned long long a = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(ahi, d) << 32) | (uint32_t)__builtin_amdgcn_readlane(alo, d);
                const long long f = (long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(fhi, d) << 32) | (uint32_t)__builtin_amdgcn_readlane(flo, d));
                s += ((a >> lane) & 1ull) ? f : 0ll;
            }
            if (lane < C && s) __hip_atomic_fetch_add(L + (uint64_t)j * C + lane, (unsigned long long)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }

        // backward: marker q = j + o + 1 takes a_jc fx, in LDS slot q - (jt0 + d0 + 1) = row + lane
        if (fx != 0)
            for (unsigned long long b = ONE ? (aj & 1ull) : aj; b; b &= b - 1ull) { // (the bits are uniform)
                const uint32_t c = (uint32_t)__builtin_ctzll(b);
                atomicAdd(&ls_back[c * LS_SPAN + row + lane], (unsigned long long)fx);
            }
    }
    __syncthreads();

    const uint32_t qbase = jt0 + d0 + 1u;
    for (uint32_t i = tid; i < C * LS_SPAN; i += LS_WAVES * 64) {
        const uint32_t slot = i / C, c = i % C, q = qbase + slot;
        const unsigned long long v = ls_back[c * LS_SPAN + slot];
        if (v && q < M) __hip_atomic_fetch_add(L + (uint64_t)q * C + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Thread (j, c): the self term, one conversion, NaN rows; the double takes the accumulator's place
__global__ __launch_bounds__(256) void k_lds_final(unsigned long long* __restrict__ L, const unsigned long long* __restrict__ annot,
                                                   const double* __restrict__ mstd, uint32_t M, uint32_t C)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)M * C) return;
    const uint32_t j = (uint32_t)(i / C), c = (uint32_t)(i % C);
    double v = __builtin_nan("");
    if (isfinite(mstd[j])) {
        const long long s = (long long)L[i] + (long long)(((annot[j] >> c) & 1ull) << LS_FRAC);
        v = (double)s / (double)(1ll << LS_FRAC);
    }
    L[i] = (unsigned long long)__double_as_longlong(v);
}

} // namespace

extern "C" int hgibbs_ld_scores(hgibbs_t h, uint32_t W, const uint32_t* ahead, uint32_t C, const uint64_t* annot, int adjust, double* l2)
{
    if (ld_band_check(h, "hgibbs_ld_scores", W, &hgibbs_ctx::lds_ms)) return 1;
    if (C == 0 || C > LS_CMAX) return fail("hgibbs_ld_scores: C = %u, must be in [1, %u]", C, LS_CMAX);
    if (!annot && C != 1u) return fail("hgibbs_ld_scores: C = %u without annotations (annot = NULL means one column with every marker)", C);
    if (adjust && h->n_global < 3u) return fail("hgibbs_ld_scores: N = %u, the adjusted term r^2 - (1 - r^2) / (N - 2) needs N >= 3", h->n_global);
    if (!l2) return fail("hgibbs_ld_scores: null output");
    const uint32_t M = h->M;
    std::vector<uint32_t> ah;
    if (ld_ahead("hgibbs_ld_scores", M, W, ahead, ah)) return 1;
    std::vector<unsigned long long> an(M, 1ull);
    if (annot)
        for (uint32_t j = 0; j < M; ++j) {
            if (C < 64u && (annot[j] >> C)) return fail("hgibbs_ld_scores: annot[%u] has a bit at or above C = %u", j, C);
            an[j] = annot[j];
        }
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;

    const uint32_t piece = ld_piece_rows(W, h->ldscore_piece, M);
    const size_t np = (size_t)piece * W, nl = (size_t)M * C;
    if (need_device_memory(nl * 8 + np * 32 + (size_t)M * 12 + ld_flag_count(M),
                           "hgibbs_ld_scores: the %u x %u accumulator (%.1f MiB) and the sums of a piece of %u band rows (%.1f MiB)", M, C,
                           nl * 8 / 1048576.0, piece, np * 32 / 1048576.0))
        return 1;
    LdBand band;
    if (ld_band_open(h, W, piece, band)) return 1;
    DevBuf<unsigned long long> L, dan;
    DevBuf<uint32_t> dah;
    if (L.alloc(nl) || dan.alloc(M) || dah.alloc(M)) return 1;
    HIP_TRY(hipMemcpy(dan, an.data(), (size_t)M * sizeof(unsigned long long), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dah, ah.data(), (size_t)M * sizeof(uint32_t), hipMemcpyHostToDevice));

    const size_t lds = (size_t)C * LS_SPAN * sizeof(unsigned long long);
    double products_ms = 0.0, reduce_ms = 0.0;
    if (lap_begin(h)) return 1;
    HIP_TRY(hipMemsetAsync(L, 0, nl * sizeof(unsigned long long), h->stream));
    if (lap_end(h, reduce_ms)) return 1;
    // the step of a piece: the products' lap ends, the reduce has its own
    auto reduce = [&](uint32_t p0, uint32_t pc, const unsigned long long* acc) -> int {
        if (lap_end(h, products_ms)) return 1;
        if (lap_begin(h)) return 1;
        const dim3 rgrid((W + LS_OFFS - 1u) / LS_OFFS, (pc + LS_ROWS - 1u) / LS_ROWS);
        if (C == 1u)
            k_lds_reduce<true><<<rgrid, LS_WAVES * 64, lds, h->stream>>>(acc, h->counts, h->mave, h->mstd, dah, dan, M, h->n_local, h->n_global, W, p0, pc,
                                                                          C, adjust, L);
        else
            k_lds_reduce<false><<<rgrid, LS_WAVES * 64, lds, h->stream>>>(acc, h->counts, h->mave, h->mstd, dah, dan, M, h->n_local, h->n_global, W, p0, pc,
                                                                           C, adjust, L);
        HIP_TRY(hipGetLastError());
        return lap_end(h, reduce_ms);
    };
    if (ld_band_pieces(h, band, 0, M, reduce)) return 1;
    if (lap_begin(h)) return 1;
    k_lds_final<<<(uint32_t)((nl + 255u) / 256u), 256, 0, h->stream>>>(L, dan, h->mstd, M, C);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, reduce_ms)) return 1;
    HIP_TRY(hipMemcpy(l2, L, nl * sizeof(double), hipMemcpyDeviceToHost));
    h->lds_ms[0] = products_ms;
    h->lds_ms[1] = reduce_ms;
    return 0;
}

extern "C" int hgibbs_last_ld_scores_ms(hgibbs_t h, double* products_ms, double* reduce_ms)
{
    if (!h || !products_ms || !reduce_ms) return fail("hgibbs_last_ld_scores_ms: null argument");
    *products_ms = h->lds_ms[0];
    *reduce_ms = h->lds_ms[1];
    return 0;
}
