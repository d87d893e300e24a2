// Joint genotype tables of pairs of markers, and the epistasis screen on them.  For two lists of markers and a
// class (0 or 1) per row, the 3 x 3 table of stored codes of every pair (a, b) per class, as exact integers:
//
//     tables[((a nb + b) 2 + k) 9 + 3 i + j] = #{rows of class k : code(idxA[a]) = i, code(idxB[b]) = j},      i, j in {0, 1, 2}
//
// a row with a missing call (code 3) at either marker in no cell.  The frame is k_sgram's (hg_sgram.hip.h: both operands come from the
// BED, gathered through a list, same individuals in the same k slots, no LDS stage), the operands are indicators.
//
//   bytes    per marker and k-step the lane's ONE stored dword x turned into indicator bytes (0 or 1, rl_expand16's placement) of
//            [code = 1], [code = 2] and, in the MISS build, [called]: the indicator is formed on the packed dword (bit 0 of each 2-bit
//            slot: lo & ~hi, hi & ~lo, ~(lo & hi)) and then spread, four shifts and four ANDs.  Padding slots are code 3: no indicator.
//   class    cls becomes ONE more column in the BED's own layout (k_ptab_class: slot 01 at a row of class 1, 00 elsewhere; the bit-plane
//            image), so a lane reads its dword of it as it reads a marker's, and the class rides on the row operand as an AND of packed
//            bits BEFORE the spread: [code_a = i][class 1].  Class 0 is all rows minus class 1, not a second mask: the number of
//            products is the same, but with cls = NULL the class products are not compiled into the launch at all (build CLS = false,
//            half the work), and the subtraction is exact in integers.
//   job      workgroup x = (16-marker tile ta of list A, group tg of PT_NB = 2 tiles of list B), y = a range of 512-row slices; its
//            four waves take the slices of the range in turn, each with accumulators of its own.  The row operands of tile ta are
//            spread once and meet both tiles of the group.
//   forms    MISS: nine sums per class and pair, S_uv = sum [u_a][v_b] over u, v in {1, 2, c}: the 2 x 2 of codes 1 and 2, the four margins
//            against [called], and [called][called].  Clean: a job whose 16 + 32 columns lie in 16-marker granules without a missing call
//            (missing_tiles, as k_ld and k_sgram choose their builds) takes the 2 x 2 alone; its margins are the per-marker class counts
//            of k_ptab_counts, made once per call: S_1c = #[code_a = 1], S_c1 = #[code_b = 1], S_cc = the rows of the class.  Both builds
//            are launched over the same grid and a workgroup of the wrong build returns at once, so clean data never issues the five
//            missing-call products.
//   D        (i32): lane (c, g), register r = the pair (a = 16 ta + 4 g + r, b = 16 tb + c).  Added to the pair's 18 sums by 32-bit
//            integer atomics (zeros skipped); positions past the end of a list load code 0 and are never written.
//   tables   k_ptab_final, one thread a pair, in place: n_11 .. n_22 = S; n_i0 = S_ic - S_i1 - S_i2; n_0j = S_cj - S_1j - S_2j;
//            n_00 = S_cc - the other eight; class 0 = all - class 1.
//   exact    every sum is a count of rows <= n_local < 2^29: i32 accumulators and i32 atomics are exact, integer sums depend on no tiling,
//            range split (option ptab_split), cut of the lists or order: bit-identical across all.
//   layout   no LDS: every operand byte is made in registers from the lane's own dword, so there is no staging and no bank conflict
//            to swizzle away (what DESIGN.md section 13 suspects of k_ld's staged layout does not arise).
//
// The screen (hgibbs_epi_scan): blocks of the pair space of EP_BLOCK x EP_BLOCK list positions; per block the tables as above, then
// k_epi_screen, one thread a pair, evaluates hg_epi_ksa (hg_epi_math.h, the host's own operations) and appends the pair, its table and
// the value to a list when KSA >= threshold - delta.  The list is counted in full and the scan runs again with the exact capacity when
// it overflows (hgibbs_roh's list); the host sorts it by (a, b).
#pragma once

#include "hg_epi_math.h"

namespace {

constexpr int PT_WAVES = 4;              // waves per workgroup
constexpr uint32_t PT_NB = 2;            // tiles of list B per workgroup
constexpr uint32_t PT_NONE = 0xFFFFFFFFu;
constexpr uint32_t EP_LIST0 = 1u << 20;  // first capacity of the pair list (option epi_list0)
constexpr uint32_t EP_BLOCK = 1024;      // list positions a side of a block (option epi_block)

struct EpiHit {
    uint32_t a, b;
    int32_t t[18];
    double ksa;
};

struct PtArgs {
    const uint8_t* bed;
    uint64_t stride;
    const uint32_t* idxA; // the block's part of the lists
    const uint32_t* idxB;
    uint32_t na, nb, ngb; // its lengths; groups of PT_NB tiles of list B
    const uint32_t* cimg; // the class column (null in the CLS = false build)
    const uint8_t* fA;    // per tile of A / group of B: a column in a granule with missing calls
    const uint8_t* fB;
    const int32_t* cntA;  // per list position: #[code 1], #[code 2], #[called] over all rows, then over class 1
    const int32_t* cntB;
    uint32_t sub_per, n_sub;
    int32_t* acc;         // 18 per pair: the sums, then (k_ptab_final) the tables
};

// packed indicator bits (bit 0 of each 2-bit slot) -> bytes 0 / 1 in rl_expand16's placement
__device__ __forceinline__ rl_v4i pt_spread(uint32_t p)
{
    rl_v4i r;
    r.x = (int)(p & 0x01010101u);
    r.y = (int)((p >> 2) & 0x01010101u);
    r.z = (int)((p >> 4) & 0x01010101u);
    r.w = (int)((p >> 6) & 0x01010101u);
    return r;
}

// the class column: dword d holds rows 16 d .. 16 d + 15, slot 01 at class 1
__global__ __launch_bounds__(256) void k_ptab_class(const uint8_t* __restrict__ cls, uint32_t n_local, uint32_t ndw, uint32_t* __restrict__ cimg)
{
    const uint32_t d = blockIdx.x * 256u + threadIdx.x;
    if (d >= ndw) return;
    uint32_t w = 0;
    for (uint32_t t = 0; t < 16u; ++t) {
        const uint64_t i = 16ull * d + t;
        if (i < n_local && cls[i]) w |= 1u << (2u * t);
    }
    cimg[d] = w;
}

// One block per list position: the six counts of its column
__global__ __launch_bounds__(256) void k_ptab_counts(const uint8_t* __restrict__ bed, uint64_t stride, const uint32_t* __restrict__ idx,
                                                     const uint32_t* __restrict__ cimg, uint32_t ndw, int32_t* __restrict__ cnt)
{
    __shared__ int s[6];
    if (threadIdx.x < 6u) s[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t* col = reinterpret_cast<const uint32_t*>(bed + (uint64_t)idx[blockIdx.x] * stride);
    int c[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t d = threadIdx.x; d < ndw; d += 256u) {
        const uint32_t x = col[d], lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u, k = cimg ? cimg[d] : 0u;
        const uint32_t p1 = lo & ~hi, p2 = hi & ~lo, pc = ~(lo & hi) & 0x55555555u;
        c[0] += __popc(p1);
        c[1] += __popc(p2);
        c[2] += __popc(pc);
        c[3] += __popc(p1 & k);
        c[4] += __popc(p2 & k);
        c[5] += __popc(pc & k);
    }
#pragma unroll
    for (int t = 0; t < 6; ++t)
        if (c[t]) atomicAdd(&s[t], c[t]);
    __syncthreads();
    if (threadIdx.x < 6u) cnt[6ull * blockIdx.x + threadIdx.x] = s[threadIdx.x];
}

template <bool MISS, bool CLS>
__global__ __launch_bounds__(PT_WAVES * 64) void k_ptab(PtArgs p)
{
    constexpr int NS = MISS ? 9 : 4; // sums per class and pair
    constexpr int NW = CLS ? 2 : 1;  // all rows, class 1
    const uint32_t ta = blockIdx.x / p.ngb, tg = blockIdx.x % p.ngb;
    if ((bool)(p.fA[ta] | p.fB[tg]) != MISS) return; // (uniform) the other build's job
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = lane & 15u, g = lane >> 4;
    const uint32_t s0 = blockIdx.y * p.sub_per, s1 = min(p.n_sub, s0 + p.sub_per);
    if (s0 + wave >= s1) return; // (wave-uniform; no barrier below)
    const uint32_t pa = 16u * ta + c;
    const uint32_t ja = pa < p.na ? p.idxA[pa] : PT_NONE;
    const uint8_t* ra = p.bed + (uint64_t)(ja == PT_NONE ? 0u : ja) * p.stride + g * 32u;
    uint32_t jb[PT_NB];
    const uint8_t* rb[PT_NB];
#pragma unroll
    for (uint32_t t = 0; t < PT_NB; ++t) {
        const uint32_t pb = 16u * (PT_NB * tg + t) + c;
        jb[t] = pb < p.nb ? p.idxB[pb] : PT_NONE;
        rb[t] = p.bed + (uint64_t)(jb[t] == PT_NONE ? 0u : jb[t]) * p.stride + g * 32u;
    }

    rl_v4i D[PT_NB][NW][NS];
#pragma unroll
    for (uint32_t t = 0; t < PT_NB; ++t)
#pragma unroll
        for (int w = 0; w < NW; ++w)
#pragma unroll
            for (int s = 0; s < NS; ++s) D[t][w][s] = rl_v4i{0, 0, 0, 0};

    for (uint32_t sub = s0 + wave; sub < s1; sub += PT_WAVES) {
        const uint64_t off = (uint64_t)sub * (MD_SUBD * 4);
        uint4 wa[2], wb[PT_NB][2], wc[2];
        wa[0] = wa[1] = wc[0] = wc[1] = make_uint4(0u, 0u, 0u, 0u); // (positions past a list: code 0, never written out)
        if (ja != PT_NONE) {
            const uint4* q = reinterpret_cast<const uint4*>(ra + off);
            wa[0] = q[0];
            wa[1] = q[1];
        }
#pragma unroll
        for (uint32_t t = 0; t < PT_NB; ++t) {
            wb[t][0] = wb[t][1] = make_uint4(0u, 0u, 0u, 0u);
            if (jb[t] != PT_NONE) {
                const uint4* q = reinterpret_cast<const uint4*>(rb[t] + off);
                wb[t][0] = q[0];
                wb[t][1] = q[1];
            }
        }
        if constexpr (CLS) {
            const uint4* q = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(p.cimg) + off + g * 32u);
            wc[0] = q[0];
            wc[1] = q[1];
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            // tile ta: the row operands, over all rows and over class 1
            const uint32_t xa = md_dword(wa, s), la = xa & 0x55555555u, ha = (xa >> 1) & 0x55555555u;
            const uint32_t a1 = la & ~ha, a2 = ha & ~la, ac = ~(la & ha) & 0x55555555u;
            rl_v4i R[NW][3];
            R[0][0] = pt_spread(a1);
            R[0][1] = pt_spread(a2);
            if constexpr (MISS) R[0][2] = pt_spread(ac);
            if constexpr (CLS) {
                const uint32_t k = md_dword(wc, s);
                R[NW - 1][0] = pt_spread(a1 & k);
                R[NW - 1][1] = pt_spread(a2 & k);
                if constexpr (MISS) R[NW - 1][2] = pt_spread(ac & k);
            }
#pragma unroll
            for (uint32_t t = 0; t < PT_NB; ++t) {
                const uint32_t xb = md_dword(wb[t], s), lb = xb & 0x55555555u, hb = (xb >> 1) & 0x55555555u;
                const rl_v4i C1 = pt_spread(lb & ~hb), C2 = pt_spread(hb & ~lb);
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    D[t][w][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(R[w][0], C1, D[t][w][0], 0, 0, 0);
                    D[t][w][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(R[w][0], C2, D[t][w][1], 0, 0, 0);
                    D[t][w][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(R[w][1], C1, D[t][w][2], 0, 0, 0);
                    D[t][w][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(R[w][1], C2, D[t][w][3], 0, 0, 0);
                }
                if constexpr (MISS) {
                    const rl_v4i Cc = pt_spread(~(lb & hb) & 0x55555555u);
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        D[t][w][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(R[w][0], Cc, D[t][w][4], 0, 0, 0);
                        D[t][w][5] = __builtin_amdgcn_mfma_i32_16x16x64_i8(R[w][1], Cc, D[t][w][5], 0, 0, 0);
                        D[t][w][6] = __builtin_amdgcn_mfma_i32_16x16x64_i8(R[w][2], C1, D[t][w][6], 0, 0, 0);
                        D[t][w][7] = __builtin_amdgcn_mfma_i32_16x16x64_i8(R[w][2], C2, D[t][w][7], 0, 0, 0);
                        D[t][w][8] = __builtin_amdgcn_mfma_i32_16x16x64_i8(R[w][2], Cc, D[t][w][8], 0, 0, 0);
                    }
                }
            }
        }
    }

#pragma unroll
    for (uint32_t t = 0; t < PT_NB; ++t) {
        const uint32_t b = 16u * (PT_NB * tg + t) + c;
        if (b >= p.nb) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t a = 16u * ta + 4u * g + (uint32_t)r;
            if (a >= p.na) continue;
            int32_t* o = p.acc + ((uint64_t)a * p.nb + b) * 18u;
#pragma unroll
            for (int w = 0; w < NW; ++w)
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int v = D[t][w][s][r];
                    if (v) __hip_atomic_fetch_add(o + 9 * w + s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
        }
    }
}

// The pair's 18 sums (all rows, class 1) -> its two tables (class 0, class 1), in place
__device__ __forceinline__ void pt_table(const int32_t* S, int32_t* T)
{
    T[4] = S[0];
    T[5] = S[1];
    T[7] = S[2];
    T[8] = S[3];
    T[3] = S[4] - S[0] - S[1];
    T[6] = S[5] - S[2] - S[3];
    T[1] = S[6] - S[0] - S[2];
    T[2] = S[7] - S[1] - S[3];
    T[0] = S[8] - (T[1] + T[2] + T[3] + T[4] + T[5] + T[6] + T[7] + T[8]);
}

__global__ __launch_bounds__(256) void k_ptab_final(PtArgs p)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint64_t)p.na * p.nb) return;
    const uint32_t a = (uint32_t)(e / p.nb), b = (uint32_t)(e % p.nb);
    int32_t* o = p.acc + e * 18u;
    int32_t S[18], all[9], one[9];
#pragma unroll
    for (int s = 0; s < 18; ++s) S[s] = o[s];
    if (!(p.fA[a / 16u] | p.fB[b / (16u * PT_NB)])) { // the clean form: the margins from the columns' own counts
        const int32_t* ca = p.cntA + 6ull * a;
        const int32_t* cb = p.cntB + 6ull * b;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            S[9 * w + 4] = ca[3 * w];
            S[9 * w + 5] = ca[3 * w + 1];
            S[9 * w + 6] = cb[3 * w];
            S[9 * w + 7] = cb[3 * w + 1];
            S[9 * w + 8] = ca[3 * w + 2];
        }
    }
    pt_table(S, all);
    pt_table(S + 9, one);
#pragma unroll
    for (int s = 0; s < 9; ++s) {
        o[s] = all[s] - one[s];
        o[9 + s] = one[s];
    }
}

struct EpiArgs {
    const int32_t* tables; // the block's
    uint32_t a0, b0, ca, cb;
    int tri;               // pairs a < b only
    double thr;            // threshold - delta
    unsigned long long* nlist;
    unsigned long long cap;
    EpiHit* hits;
};

__global__ __launch_bounds__(256) void k_epi_screen(EpiArgs e)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)e.ca * e.cb) return;
    const uint32_t a = e.a0 + (uint32_t)(i / e.cb), b = e.b0 + (uint32_t)(i % e.cb);
    if (e.tri && a >= b) return;
    int32_t t[18];
#pragma unroll
    for (int s = 0; s < 18; ++s) t[s] = e.tables[i * 18u + s];
    const double ksa = hg_epi_ksa(t, nullptr);
    if (!(ksa >= e.thr)) return;
    const unsigned long long slot = __hip_atomic_fetch_add(e.nlist, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot >= e.cap) return; // counted: the host runs again with the exact capacity
    EpiHit h;
    h.a = a;
    h.b = b;
#pragma unroll
    for (int s = 0; s < 18; ++s) h.t[s] = t[s];
    h.ksa = ksa;
    e.hits[slot] = h;
}

// What a call of either entry point holds on the device besides the tables: the lists, the class column, the flags and the counts
struct PtCall {
    uint32_t na = 0, nb = 0, n_sub = 0;
    bool cls = false;
    std::vector<uint8_t> hfA, hfB; // per tile of A, per group of B
    DevBuf<uint32_t> idxA, idxB, cimg;
    DevBuf<uint8_t> dcls, fA, fB;
    DevBuf<int32_t> cntA, cntB;
};

// The refusals of both entry points (every one before anything is allocated), then the uploads and the kernels a call runs once: the
// class column and the columns' counts.  pair_bytes: what the caller's own buffers need.  idxB null: list A on both sides.
int ptab_prepare(hgibbs_ctx* h, const char* who, uint32_t na, const uint32_t* idxA, uint32_t nb, const uint32_t* idxB, const uint8_t* cls, size_t pair_bytes,
                 PtCall& pc, double& ms)
{
    if (na == 0 || nb == 0) return fail("%s: na = %u, nb = %u, a list needs at least one marker", who, na, nb);
    if (h->n_local >= MD_NMAX) return fail("%s: %u individuals, at most %u (32-bit counts)", who, h->n_local, MD_NMAX - 1u);
    const uint32_t n = h->n_local, M = h->M;
    for (uint32_t a = 0; a < na; ++a)
        if (idxA[a] >= M) return fail("%s: idxA[%u] = %u out of range (M = %u)", who, a, idxA[a], M);
    for (uint32_t b = 0; idxB && b < nb; ++b)
        if (idxB[b] >= M) return fail("%s: idxB[%u] = %u out of range (M = %u)", who, b, idxB[b], M);
    for (size_t i = 0; cls && i < n; ++i)
        if (cls[i] > 1) return fail("%s: cls[%zu] = %u, a class is 0 or 1", who, i, (unsigned)cls[i]);
    const uint32_t nta = (na + 15u) / 16u, ngb = (nb + 16u * PT_NB - 1u) / (16u * PT_NB);
    HIP_TRY(hipSetDevice(h->device));
    const uint32_t ndw = h->n_pad / 16u;
    const size_t bytes = pair_bytes + ((size_t)na + nb) * (4 + 24) + nta + ngb + (cls ? (size_t)ndw * 4 + n : 0) + 4096;
    if (need_device_memory(bytes, "%s: lists of %u and %u markers need %.1f MiB", who, na, nb, bytes / 1048576.0)) return 1;
    if (compute_stats(h)) return 1;
    std::vector<uint8_t> gran;
    if (missing_tiles(h, 16u, gran)) return 1;
    const uint32_t* lb = idxB ? idxB : idxA;
    pc.na = na;
    pc.nb = nb;
    pc.n_sub = (n + MD_SUBI - 1) / MD_SUBI;
    pc.cls = cls != nullptr;
    pc.hfA.assign(nta, 0);
    pc.hfB.assign(ngb, 0);
    for (uint32_t a = 0; a < na; ++a) pc.hfA[a / 16u] |= gran[idxA[a] / 16u];
    for (uint32_t b = 0; b < nb; ++b) pc.hfB[b / (16u * PT_NB)] |= gran[lb[b] / 16u];
    if (pc.idxA.alloc(na) || pc.idxB.alloc(nb) || pc.fA.alloc(nta) || pc.fB.alloc(ngb) || pc.cntA.alloc((size_t)na * 6) || pc.cntB.alloc((size_t)nb * 6)) return 1;
    HIP_TRY(hipMemcpy(pc.idxA, idxA, (size_t)na * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pc.idxB, lb, (size_t)nb * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pc.fA, pc.hfA.data(), nta, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pc.fB, pc.hfB.data(), ngb, hipMemcpyHostToDevice));
    if (cls) {
        if (pc.dcls.alloc(n) || pc.cimg.alloc(ndw)) return 1;
        HIP_TRY(hipMemcpy(pc.dcls, cls, n, hipMemcpyHostToDevice));
    }
    if (lap_begin(h)) return 1;
    if (cls) {
        k_ptab_class<<<(ndw + 255u) / 256u, 256, 0, h->stream>>>(pc.dcls, n, ndw, pc.cimg);
        HIP_TRY(hipGetLastError());
    }
    k_ptab_counts<<<na, 256, 0, h->stream>>>(h->bed, h->stride, pc.idxA, pc.cimg, ndw, pc.cntA);
    HIP_TRY(hipGetLastError());
    k_ptab_counts<<<nb, 256, 0, h->stream>>>(h->bed, h->stride, pc.idxB, pc.cimg, ndw, pc.cntB);
    HIP_TRY(hipGetLastError());
    return lap_end(h, ms);
}

// The tables of the block of list positions [a0, a0 + ca) x [b0, b0 + cb) into `tables` (ca x cb x 18), on the handle's stream;
// a0 a multiple of 16, b0 of 16 PT_NB
int ptab_block(hgibbs_ctx* h, const PtCall& pc, uint32_t a0, uint32_t ca, uint32_t b0, uint32_t cb, int32_t* tables)
{
    PtArgs p{};
    p.bed = h->bed;
    p.stride = h->stride;
    p.idxA = pc.idxA + a0;
    p.idxB = pc.idxB + b0;
    p.na = ca;
    p.nb = cb;
    p.ngb = (cb + 16u * PT_NB - 1u) / (16u * PT_NB);
    p.cimg = pc.cimg;
    p.fA = pc.fA + a0 / 16u;
    p.fB = pc.fB + b0 / (16u * PT_NB);
    p.cntA = pc.cntA + 6ull * a0;
    p.cntB = pc.cntB + 6ull * b0;
    p.n_sub = pc.n_sub;
    p.acc = tables;
    const uint32_t nta = (ca + 15u) / 16u;
    const uint64_t njobs = (uint64_t)nta * p.ngb;
    if (njobs >= (1ull << 31)) return fail("hgibbs_pair_tables: %llu tile pairs in one launch, at most %llu", (unsigned long long)njobs, (1ull << 31) - 1ull);
    // row ranges: enough workgroups for eight per compute unit (option ptab_split fixes the number)
    const uint32_t want = h->ptab_split ? (uint32_t)h->ptab_split : (uint32_t)((8ull * (uint64_t)h->num_cu + njobs - 1u) / njobs);
    const uint32_t gy = split_ranges(pc.n_sub, want, NO_CAP, p.sub_per);
    uint32_t flaggedA = 0, flaggedB = 0; // tiles of A and groups of B of the block with a missing call
    for (uint32_t t = 0; t < nta; ++t) flaggedA += pc.hfA[a0 / 16u + t];
    for (uint32_t t = 0; t < p.ngb; ++t) flaggedB += pc.hfB[b0 / (16u * PT_NB) + t];
    const bool miss = flaggedA || flaggedB, clean = flaggedA < nta && flaggedB < p.ngb; // a job of the MISS build exists; a clean job exists
    HIP_TRY(hipMemsetAsync(tables, 0, (size_t)ca * cb * 18u * sizeof(int32_t), h->stream));
    const dim3 grid((uint32_t)njobs, gy);
    if (clean) {
        if (pc.cls) k_ptab<false, true><<<grid, PT_WAVES * 64, 0, h->stream>>>(p);
        else k_ptab<false, false><<<grid, PT_WAVES * 64, 0, h->stream>>>(p);
        HIP_TRY(hipGetLastError());
    }
    if (miss) {
        if (pc.cls) k_ptab<true, true><<<grid, PT_WAVES * 64, 0, h->stream>>>(p);
        else k_ptab<true, false><<<grid, PT_WAVES * 64, 0, h->stream>>>(p);
        HIP_TRY(hipGetLastError());
    }
    k_ptab_final<<<(uint32_t)(((uint64_t)ca * cb + 255u) / 256u), 256, 0, h->stream>>>(p);
    HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace

extern "C" int hgibbs_pair_tables(hgibbs_t h, uint32_t na, const uint32_t* idxA, uint32_t nb, const uint32_t* idxB, const uint8_t* cls, int32_t* tables)
{
    if (h) h->ptab_ms = 0.0;
    if (op_guard(h, "hgibbs_pair_tables", "the counts are not summed over ranks")) return 1;
    if (!idxA || !idxB || !tables) return fail("hgibbs_pair_tables: null argument");
    const size_t E = (size_t)na * nb * 18u;
    if ((uint64_t)na * nb >= (1ull << 36)) return fail("hgibbs_pair_tables: %u x %u pairs in one call, fewer than 2^36 are taken", na, nb);
    PtCall pc;
    double ms = 0.0;
    if (ptab_prepare(h, "hgibbs_pair_tables", na, idxA, nb, idxB, cls, E * sizeof(int32_t), pc, ms)) return 1;
    DevBuf<int32_t> dt;
    if (dt.alloc(E)) return 1;
    if (lap_begin(h)) return 1;
    if (ptab_block(h, pc, 0u, na, 0u, nb, dt)) return 1;
    if (lap_end(h, ms)) return 1;
    HIP_TRY(hipMemcpy(tables, dt, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    h->ptab_ms = ms;
    return 0;
}

extern "C" int hgibbs_last_pair_tables_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_pair_tables_ms: null argument");
    *ms = h->ptab_ms;
    return 0;
}

extern "C" int hgibbs_epi_scan(hgibbs_t h, uint32_t na, const uint32_t* idxA, uint32_t nb, const uint32_t* idxB, const uint8_t* cls, double threshold,
                               uint64_t* npairs)
{
    if (h) h->epi_ms[0] = h->epi_ms[1] = 0.0;
    if (op_guard(h, "hgibbs_epi_scan", "the counts are not summed over ranks")) return 1;
    if (!idxA || !npairs) return fail("hgibbs_epi_scan: null argument");
    if (!std::isfinite(threshold) || !(threshold > 0.0)) return fail("hgibbs_epi_scan: threshold = %g, needs a finite number > 0", threshold);
    const bool tri = idxB == nullptr;
    if (tri) nb = na;
    const uint32_t side = ((h->epi_block ? (uint32_t)h->epi_block : EP_BLOCK) + 31u) / 32u * 32u;
    const uint32_t sa = std::min(side, na ? na : 1u), sb = std::min(side, nb ? nb : 1u);
    unsigned long long cap = h->epi_list0 ? (unsigned long long)h->epi_list0 : EP_LIST0, found = 0;
    const size_t tab_bytes = (size_t)sa * sb * 18u * sizeof(int32_t);
    PtCall pc;
    double prod_ms = 0.0, screen_ms = 0.0;
    if (ptab_prepare(h, "hgibbs_epi_scan", na, idxA, nb, idxB, cls, tab_bytes + cap * sizeof(EpiHit), pc, prod_ms)) return 1;
    DevBuf<int32_t> dt;
    DevBuf<unsigned long long> nlist;
    DevBuf<EpiHit> dhits;
    if (dt.alloc((size_t)sa * sb * 18u) || nlist.alloc(1)) return 1;
    const double thr = threshold - hg_epi_delta((double)h->n_local);
    for (;;) {
        if (dhits.alloc(cap)) return 1;
        HIP_TRY(hipMemsetAsync(nlist, 0, sizeof(unsigned long long), h->stream));
        for (uint32_t a0 = 0; a0 < na; a0 += side)
            for (uint32_t b0 = 0; b0 < nb; b0 += side) {
                const uint32_t ca = std::min(side, na - a0), cb = std::min(side, nb - b0);
                if (tri && b0 + cb <= a0 + 1u) continue; // no pair a < b in the block
                if (lap_begin(h)) return 1;
                if (ptab_block(h, pc, a0, ca, b0, cb, dt)) return 1;
                if (lap_end(h, prod_ms)) return 1;
                EpiArgs e{};
                e.tables = dt;
                e.a0 = a0;
                e.b0 = b0;
                e.ca = ca;
                e.cb = cb;
                e.tri = tri ? 1 : 0;
                e.thr = thr;
                e.nlist = nlist;
                e.cap = cap;
                e.hits = dhits;
                if (lap_begin(h)) return 1;
                k_epi_screen<<<(uint32_t)(((uint64_t)ca * cb + 255u) / 256u), 256, 0, h->stream>>>(e);
                HIP_TRY(hipGetLastError());
                if (lap_end(h, screen_ms)) return 1;
            }
        HIP_TRY(hipMemcpy(&found, nlist, sizeof found, hipMemcpyDeviceToHost));
        if (found <= cap) break;
        // the list overflowed: every pair was counted, so the second run fits exactly (the first list goes before the check)
        dhits.release();
        cap = found;
        if (need_device_memory(cap * sizeof(EpiHit), "hgibbs_epi_scan: %llu pairs are kept: the list needs %.1f MiB", found, cap * sizeof(EpiHit) / 1048576.0))
            return 1;
    }
    std::vector<EpiHit> hits(found);
    if (found) HIP_TRY(hipMemcpy(hits.data(), dhits, found * sizeof(EpiHit), hipMemcpyDeviceToHost));
    // sorted by (a, b): the order of the atomics never shows
    std::sort(hits.begin(), hits.end(), [](const EpiHit& x, const EpiHit& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    h->epi_ab.resize(2 * found);
    h->epi_tables.resize(18 * found);
    h->epi_ksa.resize(found);
    for (size_t i = 0; i < found; ++i) {
        h->epi_ab[2 * i] = hits[i].a;
        h->epi_ab[2 * i + 1] = hits[i].b;
        std::memcpy(&h->epi_tables[18 * i], hits[i].t, sizeof hits[i].t);
        h->epi_ksa[i] = hits[i].ksa;
    }
    h->epi_ms[0] = prod_ms;
    h->epi_ms[1] = screen_ms;
    *npairs = found;
    return 0;
}

extern "C" int hgibbs_epi_scan_get(hgibbs_t h, uint32_t* ab, int32_t* tables, double* ksa)
{
    if (!h) return fail("hgibbs_epi_scan_get: null handle");
    if (ab && !h->epi_ab.empty()) std::memcpy(ab, h->epi_ab.data(), h->epi_ab.size() * sizeof(uint32_t));
    if (tables && !h->epi_tables.empty()) std::memcpy(tables, h->epi_tables.data(), h->epi_tables.size() * sizeof(int32_t));
    if (ksa && !h->epi_ksa.empty()) std::memcpy(ksa, h->epi_ksa.data(), h->epi_ksa.size() * sizeof(double));
    return 0;
}

extern "C" int hgibbs_last_epi_ms(hgibbs_t h, double* products_ms, double* screen_ms)
{
    if (!h) return fail("hgibbs_last_epi_ms: null handle");
    if (products_ms) *products_ms = h->epi_ms[0];
    if (screen_ms) *screen_ms = h->epi_ms[1];
    return 0;
}
