// LD masks of the loaded markers: one bit per pair of the band, forwards and backwards, for the greedy selection of
// hgibbs_ld_greedy (hg_ldgreedy.cpp) behind --clump and --ld-prune.
//
//   pairs     (j, q), j < q, is in the window iff q - j <= ahead[j] (ahead = NULL: min(W, M - 1 - j)), exactly as in hgibbs_ld_scores.
//   passes    a pair passes iff it is in the window, r is not NaN and r * r >= t: r is ld_pair_r (hg_ld.hip.h) unchanged, so both markers
//             have a finite mstd; the comparison is made on the f64 product (the build has -ffp-contract=off: r is bit for bit hgibbs_ld's).
//   masks     wpr = (W + 63) / 64 words per marker.  fwd[j wpr + (d - 1) / 64] bit (d - 1) % 64 is set iff pair (j, j + d) passes;
//             bwd[q wpr + (d - 1) / 64] bit (d - 1) % 64 is set iff q >= d and pair (q - d, q) passes.  Every other bit is 0, the bits of
//             offsets above W in a row's last word included.
//   products  the band frame of hg_ld.hip.h (ld_band_pieces), as in hgibbs_ld_scores: k_ld<MISS>, unchanged, fills a piece's 64-bit sums.
//   reduce    k_ldm_reduce replaces k_ld_final: a workgroup takes LM_ROWS band rows x LM_OFFS offsets of the piece.  A wave takes one row
//             at a time, lane = offset: 64 lanes read 2 KiB of sums in a row and decide `pass`.
//             forward   __ballot(pass) IS word blockIdx.x of row j: one lane stores it (plain store; each (row, word) belongs to exactly one
//                       tile; the masks are zeroed once up front, so a row whose window ends before the tile, or with no bit, stores nothing).
//             backward  the tile's targets are the LM_SPAN = 127 markers behind its first row: slot row + lane holds word blockIdx.x of
//                       marker q = j + o + 1, and the pair's bit there is `lane`.  The bits are ORed into 64-bit LDS words (a wave's 64 lanes
//                       hit 64 consecutive slots: no bank conflict) and flushed once a tile, one global 64-bit atomic OR per non-zero slot
//                       with q < M.  A target word gets its bits from two vertically adjacent tiles.
//             npass     the popcount of the forward words, one global 64-bit add per wave.
//   exact     a bit is a pure function of its pair's four exact integer sums, and OR is order-free: the masks do not depend on pieces
//             (option ldmask_piece), ld_split, tiles, launch order or repeats.
//   memory    the band, r and the sums never leave the device: the host sends ahead and receives 2 x M x wpr words: two bits per pair where
//             the band of hgibbs_ld is 8 to 40 bytes per pair.
#pragma once

namespace {

constexpr int LM_ROWS = 64;                        // band rows of a tile
constexpr int LM_OFFS = 64;                        // offsets of a tile: one per lane, one mask word
constexpr int LM_SPAN = LM_ROWS + LM_OFFS - 1;     // backward targets of a tile
constexpr int LM_WAVES = 4;

// Workgroup (x, y): offsets 64 x .. 64 x + 63 (distance = offset + 1), i.e. mask word x, of band rows p0 + 64 y .. + 63 of the piece
// [p0, p0 + pc).  bwd and npass may be null.
__global__ __launch_bounds__(LM_WAVES * 64) void k_ldm_reduce(const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ counts,
                                                              const double* __restrict__ mave, const double* __restrict__ mstd,
                                                              const uint32_t* __restrict__ ahead, uint32_t M, uint32_t n_local, uint32_t N, uint32_t W,
                                                              uint32_t wpr, uint32_t p0, uint32_t pc, double t, unsigned long long* __restrict__ fwd,
                                                              unsigned long long* __restrict__ bwd, unsigned long long* __restrict__ npass)
{
    __shared__ unsigned long long lm_back[LM_SPAN];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t d0 = LM_OFFS * blockIdx.x, jt0 = p0 + LM_ROWS * blockIdx.y;
    if (tid < (uint32_t)LM_SPAN) lm_back[tid] = 0ull;
    __syncthreads();

    const uint32_t o = d0 + lane;
    uint32_t found = 0; // (uniform) bits of this wave's forward words
    for (uint32_t row = wave; row < (uint32_t)LM_ROWS; row += LM_WAVES) {
        const uint32_t j = jt0 + row;
        if (j - p0 >= pc) break; // (uniform)
        const uint32_t ah = ahead[j];
        if (ah <= d0) continue; // (uniform) the row's window ends before this tile: its word stays 0
        bool pass = false;
        if (o < ah) { // q = j + o + 1 <= j + ahead[j] < M
            const uint32_t q = j + o + 1u;
            long long G, Bjq, Bqj, Dc;
            const double r = ld_pair_r(acc + (((uint64_t)(j - p0) * W + o) << 2), counts, mave, mstd, j, q, n_local, N, G, Bjq, Bqj, Dc);
            pass = r == r && r * r >= t;
        }
        const unsigned long long word = __ballot(pass);
        if (word == 0ull) continue; // (uniform)
        if (lane == 0u) fwd[(uint64_t)j * wpr + blockIdx.x] = word;
        found += (uint32_t)__popcll(word);
        // backward: marker q = j + o + 1 takes bit `lane` of its word blockIdx.x, in LDS slot q - (jt0 + d0 + 1) = row + lane
        if (bwd && pass) atomicOr(&lm_back[row + lane], 1ull << lane);
    }
    if (npass && lane == 0u && found) __hip_atomic_fetch_add(npass, (unsigned long long)found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!bwd) return; // (uniform over the grid)
    __syncthreads();

    if (tid < (uint32_t)LM_SPAN) {
        const uint64_t q = (uint64_t)jt0 + d0 + 1u + tid;
        const unsigned long long v = lm_back[tid];
        if (v && q < M) __hip_atomic_fetch_or(bwd + q * wpr + blockIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace

extern "C" int hgibbs_ld_mask(hgibbs_t h, uint32_t W, const uint32_t* ahead, double t, uint64_t* fwd, uint64_t* bwd, uint64_t* npass)
{
    if (ld_band_check(h, "hgibbs_ld_mask", W, &hgibbs_ctx::ldm_ms)) return 1;
    if (!(std::isfinite(t) && t >= 0.0)) return fail("hgibbs_ld_mask: t = %g, the threshold on r^2 must be finite and >= 0", t);
    if (!fwd) return fail("hgibbs_ld_mask: null output (fwd)");
    const uint32_t M = h->M;
    std::vector<uint32_t> ah;
    if (ld_ahead("hgibbs_ld_mask", M, W, ahead, ah)) return 1;
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;

    const uint32_t piece = ld_piece_rows(W, h->ldmask_piece, M);
    const uint32_t wpr = (W + 63u) / 64u;
    const size_t np = (size_t)piece * W, nm = (size_t)M * wpr;
    if (need_device_memory(2 * nm * 8 + np * 32 + (size_t)M * 4 + 8 + ld_flag_count(M),
                           "hgibbs_ld_mask: the two %u x %u-word masks (%.1f MiB) and the sums of a piece of %u band rows (%.1f MiB)", M, wpr,
                           2 * nm * 8 / 1048576.0, piece, np * 32 / 1048576.0))
        return 1;
    LdBand band;
    if (ld_band_open(h, W, piece, band)) return 1;
    DevBuf<unsigned long long> dfwd, dbwd, dn;
    DevBuf<uint32_t> dah;
    if (dfwd.alloc(nm) || (bwd && dbwd.alloc(nm)) || dn.alloc(1) || dah.alloc(M)) return 1;
    HIP_TRY(hipMemcpy(dah, ah.data(), (size_t)M * sizeof(uint32_t), hipMemcpyHostToDevice));

    double products_ms = 0.0, reduce_ms = 0.0;
    if (lap_begin(h)) return 1;
    HIP_TRY(hipMemsetAsync(dfwd, 0, nm * sizeof(unsigned long long), h->stream));
    if (bwd) HIP_TRY(hipMemsetAsync(dbwd, 0, nm * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(dn, 0, sizeof(unsigned long long), h->stream));
    if (lap_end(h, reduce_ms)) return 1;
    // the step of a piece: the products' lap ends, the reduce has its own
    auto reduce = [&](uint32_t p0, uint32_t pc, const unsigned long long* acc) -> int {
        if (lap_end(h, products_ms)) return 1;
        if (lap_begin(h)) return 1;
        const dim3 rgrid(wpr, (pc + LM_ROWS - 1u) / LM_ROWS);
        k_ldm_reduce<<<rgrid, LM_WAVES * 64, 0, h->stream>>>(acc, h->counts, h->mave, h->mstd, dah, M, h->n_local, h->n_global, W, wpr, p0, pc, t, dfwd,
                                                             bwd ? (unsigned long long*)dbwd : nullptr, dn);
        HIP_TRY(hipGetLastError());
        return lap_end(h, reduce_ms);
    };
    if (ld_band_pieces(h, band, 0, M, reduce)) return 1;
    HIP_TRY(hipMemcpy(fwd, dfwd, nm * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (bwd) HIP_TRY(hipMemcpy(bwd, dbwd, nm * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (npass) HIP_TRY(hipMemcpy(npass, dn, sizeof(uint64_t), hipMemcpyDeviceToHost));
    h->ldm_ms[0] = products_ms;
    h->ldm_ms[1] = reduce_ms;
    return 0;
}

extern "C" int hgibbs_last_ld_mask_ms(hgibbs_t h, double* products_ms, double* reduce_ms)
{
    if (!h || !products_ms || !reduce_ms) return fail("hgibbs_last_ld_mask_ms: null argument");
    *products_ms = h->ldm_ms[0];
    *reduce_ms = h->ldm_ms[1];
    return 0;
}

extern "C" int hgibbs_ld_clump(hgibbs_t h, uint32_t W, const uint32_t* ahead, double t, const uint32_t* order, uint32_t norder,
                               const uint8_t* may_lead, int32_t* owner, uint64_t* npass)
{
    if (op_guard(h, "hgibbs_ld_clump", "the band is not exchanged between ranks")) return 1;
    if (W == 0 || W > LD_WMAX) return fail("hgibbs_ld_clump: W = %u, must be in [1, %u]", W, LD_WMAX);
    if (!owner) return fail("hgibbs_ld_clump: null output (owner)");
    if (norder && !order) return fail("hgibbs_ld_clump: null order with norder = %u", norder);
    const size_t nm = (size_t)h->M * ((W + 63u) / 64u);
    std::vector<uint64_t> fwd(nm), bwd(nm);
    if (hgibbs_ld_mask(h, W, ahead, t, fwd.data(), bwd.data(), npass)) return 1;
    return hgibbs_ld_greedy(h->M, W, fwd.data(), bwd.data(), order, norder, may_lead, owner);
}
