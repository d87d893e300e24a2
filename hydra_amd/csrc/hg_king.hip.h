// KING-robust kinship of the loaded rows: for individuals a and b, over the markers where both calls are
// present (code != 3), the five exact counts
//
//     NSNP = sum c_a c_b,   HET_a = sum h_a c_b,   HET_b = sum c_a h_b,   HETHET = sum h_a h_b,   IBS0 = (V - U) / 2
//
// with c = [called], h = [het], u = +1 at hom 2, -1 at hom 0, 0 otherwise, U = sum u_a u_b and V = cc - hc - ch + hh = sum [hom_a][hom_b]
// (so V - U = 2 sum ([0]_a [2]_b + [2]_a [0]_b)), and KINSHIP = 1/2 - (4 IBS0 + HET_a + HET_b - 2 HETHET) / (4 min(HET_a, HET_b)).
//
//   operands  A: 16 individuals (rows), B: 16 other individuals (columns), k = markers, 64 a k-step.  The stored BED is marker-major
//             (dword d of marker j holds individuals 16 d .. 16 d + 15), so the codes are transposed ONCE per call, by k_king_image, into
//             an individual-major image in HBM: word (g, i) holds the sixteen codes of individual i at markers 16 g .. 16 g + 15.  Lane
//             (c, k) of a k-step s reads word (4 s + k, 16 t + c) of its tile t and builds the three byte forms c, h, u (kg_forms, the
//             byte order of rl_expand16); A and B put the same markers in the same k slots, so every product sums over markers.
//   result    D[row][col] of v_mfma_i32_16x16x64_i8: lane (c, k), register r = individual 4 k + r of the A tile against individual c of the B
//             tile.  Five products a tile pair and k-step: c.c, h.c, c.h, h.h, u.u.
//   padding   k_king_image writes code 3 (all three forms 0) for individuals past n_local and markers past M: padding counts nowhere.
//   exact     every count is at most M < 2^31 in an i32 (|U| <= M too); with markers split over workgroups (hgibbs_king, option king_split)
//             the parts meet in i32 atomic adds (order-free); hgibbs_king_pairs runs every marker in one workgroup.  The counts, and the
//             one f64 formula per pair, do not depend on blocking, king_split, the block chunking or launch order: bit-identical.
//   reuse     workgroup = 8 waves over a block of 8 x 8 row tiles (128 x 128 individuals); wave w takes A tiles 2 (w & 3) + {0, 1} and
//             B tiles 4 (w >> 2) + {0 .. 3}: per k-step it builds the forms of 6 operands (one 4-byte load each, the image words of the
//             block sit in L1 / L2 for the 2 and 4 waves that share them) for 40 products.  hgibbs_king_pairs takes the upper triangle
//             of block pairs and, in a diagonal block, the tile pairs ta <= tb only.  The block pairs sit on a 2-D grid (king_grid).
//
// Registers (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no scratch, no spills):
//
//   build               VGPRs  AGPRs  LDS  waves / SIMD
//   k_king<false>         228      0     0     2          (hgibbs_king: the rectangle, i32 atomic adds)
//   k_king<true>          232      0     0     2          (hgibbs_king_pairs: the triangle, the formula and the list)
//   k_king_image           63      0     0     8
#pragma once

namespace {

constexpr int KG_WAVES = 8;              // waves per workgroup
constexpr int KG_RA = 2, KG_RB = 4;      // A and B tiles per wave
constexpr int KG_BT = 8;                 // row tiles per block side (4 x KG_RA = 2 x KG_RB)
constexpr uint32_t KG_LIST0 = 1u << 20;  // first capacity of the pair list (grown inside the call when the kernel finds more)
constexpr uint32_t KG_GX = 1u << 20;     // workgroups in grid x at most: an AQL packet holds each grid dimension in work-items as a u32
                                         // (2^20 x 512 = 2^29), so the block pairs go on a 2-D grid (x, y); y <= 2^31 / 2^20 = 2048

struct KingArgs {
    const uint32_t* img;    // [group][npi] words of sixteen 2-bit codes
    const uint32_t* bpairs; // block pairs, (bi << 16) | bj
    uint32_t nbp;           // block pairs (workgroup x + gridDim.x y of the 2-D grid; the last row of the grid runs short)
    uint32_t npi;           // individuals per image row (16 ntile)
    uint32_t ntile;         // row tiles in the image
    uint32_t nks;           // k-steps (64 markers each)
    uint32_t ks_per;        // k-steps per workgroup (grid z splits them)
    uint32_t ta0, tb0;      // first tile of block 0 on either side
    // rectangle (hgibbs_king): counts[(a - ra0) * rbcount + b - rb0][5]
    int32_t* counts;
    uint32_t ra0, racount, rb0, rbcount;
    // triangle (hgibbs_king_pairs): pairs a < b < n_local with KINSHIP >= cutoff appended to the list
    uint32_t n_local;
    double cutoff;
    unsigned long long* nlist;
    unsigned long long cap;
    uint32_t* ab;
    int32_t* lcounts;
    double* lkin;
};

// c = [called], h = [het], u = code - 1 on called codes (0 at a missing call), sixteen codes of one word, the byte order of rl_expand16
__device__ __forceinline__ void kg_forms(uint32_t x, rl_v4i& c, rl_v4i& h, rl_v4i& u)
{
    const uint32_t m = x & (x >> 1) & 0x55555555u; // [code == 3] in the low bit of each field
    const uint32_t cw = m ^ 0x55555555u;
    const uint32_t hw = (x & 0x55555555u) ^ m;     // code 1 (code 3 also has the low bit: taken out by m)
    const uint32_t zw = x ^ (m << 1);              // code 3 -> 1: u = 0
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        c[e] = (int)((cw >> (2 * e)) & 0x01010101u);
        h[e] = (int)((hw >> (2 * e)) & 0x01010101u);
        u[e] = (int)((((zw >> (2 * e)) & 0x03030303u) + 0x7F7F7F7Fu) ^ 0x80808080u); // per byte z - 1, no carry (z <= 2)
    }
}

// NSNP, HET_a, HET_b, HETHET, IBS0 from the five products
__device__ __forceinline__ void kg_counts(int cc, int hc, int ch, int hh, int uu, int32_t* k)
{
    k[0] = cc;
    k[1] = hc;
    k[2] = ch;
    k[3] = hh;
    k[4] = (int32_t)(((long long)cc - hc - ch + hh - uu) / 2); // (V - U) / 2: V - U is even, and up to 2 M: in 64 bits
}

__device__ __forceinline__ double kg_kinship(const int32_t* k)
{
    const int32_t mn = k[1] < k[2] ? k[1] : k[2];
    if (mn <= 0) return __builtin_nan("");
    const long long num = 4ll * k[4] + (long long)(k[1] - k[3]) + (long long)(k[2] - k[3]);
    return 0.5 - (double)num / (4.0 * (double)mn);
}

// Workgroup (x, y, z): block pair bpairs[x + gridDim.x y], k-steps [z ks_per, (z + 1) ks_per).  TRI: the triangle with the filter
// (else the rectangle).
template <bool TRI>
__global__ __launch_bounds__(KG_WAVES * 64) void k_king(KingArgs p)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = lane & 15u, k4 = lane >> 4;
    const uint64_t bpi = (uint64_t)blockIdx.x + (uint64_t)gridDim.x * blockIdx.y;
    if (bpi >= p.nbp) return; // (uniform: the last row of the grid)
    const uint32_t bp = p.bpairs[bpi];
    const uint32_t taw = p.ta0 + KG_BT * (bp >> 16) + KG_RA * (wave & 3u);
    const uint32_t tbw = p.tb0 + KG_BT * (bp & 0xFFFFu) + KG_RB * (wave >> 2);
    const uint32_t s0 = blockIdx.z * p.ks_per, s1 = min(p.nks, s0 + p.ks_per);

    // tiles of this wave that exist, and the tile pairs it runs (all wave-uniform)
    const uint32_t ta_end = TRI ? p.ntile : min(p.ntile, (p.ra0 + p.racount + 15u) / 16u);
    const uint32_t tb_end = TRI ? p.ntile : min(p.ntile, (p.rb0 + p.rbcount + 15u) / 16u);
    bool aon[KG_RA], bon[KG_RB], on[KG_RA][KG_RB];
    bool any = false;
#pragma unroll
    for (int i = 0; i < KG_RA; ++i) aon[i] = taw + (uint32_t)i < ta_end;
#pragma unroll
    for (int j = 0; j < KG_RB; ++j) bon[j] = tbw + (uint32_t)j < tb_end;
#pragma unroll
    for (int i = 0; i < KG_RA; ++i)
#pragma unroll
        for (int j = 0; j < KG_RB; ++j) {
            on[i][j] = aon[i] && bon[j] && (!TRI || taw + (uint32_t)i <= tbw + (uint32_t)j);
            any = any || on[i][j];
        }
    if (!any || s0 >= s1) return; // (uniform; no barrier in this kernel)

    rl_v4i acc[KG_RA][KG_RB][5];
#pragma unroll
    for (int i = 0; i < KG_RA; ++i)
#pragma unroll
        for (int j = 0; j < KG_RB; ++j)
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[i][j][q] = rl_v4i{0, 0, 0, 0};

    // lane (c, k) of k-step s: word (4 s + k, 16 t + c); an absent tile reads as code 3 everywhere (no load)
    auto load = [&](uint32_t s, uint32_t* wa, uint32_t* wb) {
        const uint32_t* row = p.img + (size_t)(4u * s + k4) * p.npi + c;
#pragma unroll
        for (int i = 0; i < KG_RA; ++i) wa[i] = aon[i] ? row[16u * (taw + (uint32_t)i)] : 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < KG_RB; ++j) wb[j] = bon[j] ? row[16u * (tbw + (uint32_t)j)] : 0xFFFFFFFFu;
    };
    uint32_t wa[KG_RA], wb[KG_RB];
    load(s0, wa, wb);
    for (uint32_t s = s0; s < s1; ++s) {
        uint32_t na[KG_RA], nb[KG_RB];
        if (s + 1u < s1) load(s + 1u, na, nb); // (uniform) the next k-step's words in flight
        rl_v4i ca[KG_RA], ha[KG_RA], ua[KG_RA];
#pragma unroll
        for (int i = 0; i < KG_RA; ++i) kg_forms(wa[i], ca[i], ha[i], ua[i]);
#pragma unroll
        for (int j = 0; j < KG_RB; ++j) {
            rl_v4i cb, hb, ub;
            kg_forms(wb[j], cb, hb, ub);
#pragma unroll
            for (int i = 0; i < KG_RA; ++i) {
                if (!on[i][j]) continue; // (uniform)
                acc[i][j][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ca[i], cb, acc[i][j][0], 0, 0, 0);
                acc[i][j][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ha[i], cb, acc[i][j][1], 0, 0, 0);
                acc[i][j][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ca[i], hb, acc[i][j][2], 0, 0, 0);
                acc[i][j][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ha[i], hb, acc[i][j][3], 0, 0, 0);
                acc[i][j][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ua[i], ub, acc[i][j][4], 0, 0, 0);
            }
        }
        if (s + 1u < s1) {
#pragma unroll
            for (int i = 0; i < KG_RA; ++i) wa[i] = na[i];
#pragma unroll
            for (int j = 0; j < KG_RB; ++j) wb[j] = nb[j];
        }
    }

    // lane (c, k), register r: a = 16 ta + 4 k + r, b = 16 tb + c
#pragma unroll
    for (int i = 0; i < KG_RA; ++i)
#pragma unroll
        for (int j = 0; j < KG_RB; ++j) {
            if (!on[i][j]) continue; // (uniform)
            const uint32_t b = 16u * (tbw + (uint32_t)j) + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t a = 16u * (taw + (uint32_t)i) + 4u * k4 + (uint32_t)r;
                int32_t k[5];
                kg_counts(acc[i][j][0][r], acc[i][j][1][r], acc[i][j][2][r], acc[i][j][3][r], acc[i][j][4][r], k);
                if constexpr (TRI) {
                    const double kin = kg_kinship(k);
                    const bool keep = a < b && b < p.n_local && kin >= p.cutoff; // (NaN: never)
                    // one atomic a wave: the lanes that keep a pair take consecutive slots
                    const unsigned long long mask = __ballot(keep);
                    if (!mask) continue; // (uniform)
                    const uint32_t lead = (uint32_t)__ffsll((long long)mask) - 1u;
                    unsigned long long base = 0;
                    if (lane == lead) base = __hip_atomic_fetch_add(p.nlist, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    base = __shfl(base, (int)lead);
                    if (!keep) continue;
                    const unsigned long long slot = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
                    if (slot >= p.cap) continue; // counted: the host grows the list and runs again
                    p.ab[2 * slot] = a;
                    p.ab[2 * slot + 1] = b;
#pragma unroll
                    for (int q = 0; q < 5; ++q) p.lcounts[5 * slot + q] = k[q];
                    p.lkin[slot] = kin;
                } else {
                    if (a < p.ra0 || a - p.ra0 >= p.racount || b < p.rb0 || b - p.rb0 >= p.rbcount) continue;
                    int32_t* o = p.counts + ((size_t)(a - p.ra0) * p.rbcount + (b - p.rb0)) * 5u;
#pragma unroll
                    for (int q = 0; q < 5; ++q)
                        if (k[q]) __hip_atomic_fetch_add(o + q, k[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
}

// Thread (d, g): dword d (individuals 16 d .. 16 d + 15) of markers 16 g .. 16 g + 15 -> the sixteen image words (g, 16 d + 0 .. 15):
// a 16 x 16 transpose of 2-bit codes.  Markers past M and individuals past n_local become code 3.
__global__ __launch_bounds__(256) void k_king_image(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t M, uint32_t n_local,
                                                    uint32_t ntile, uint32_t ngrp, uint32_t npi, uint32_t* __restrict__ img)
{
    const uint32_t d = blockIdx.x * 256u + threadIdx.x, g = blockIdx.y + 65535u * blockIdx.z;
    if (d >= ntile || g >= ngrp) return;
    const uint32_t vm = ld_valid_mask(n_local, d);
    uint32_t w[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const uint32_t j = 16u * g + (uint32_t)e;
        w[e] = j < M ? (reinterpret_cast<const uint32_t*>(bed + (uint64_t)j * stride)[d] | ~vm) : 0xFFFFFFFFu;
    }
    uint32_t o[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) v |= ((w[e] >> (2 * i)) & 3u) << (2 * e);
        o[i] = v;
    }
    uint4* dst = reinterpret_cast<uint4*>(img + (size_t)g * npi + 16u * d);
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
}

// the checks every entry point makes
int king_check(hgibbs_ctx* h, const char* who)
{
    if (op_guard(h, who, "pairs across shards are not formed")) return 1;
    if (h->M >= (1u << 31)) return fail("%s: %u markers, at most 2^31 - 1 (i32 counts)", who, h->M);
    if (h->n_local > 65535u * 16u * KG_BT) return fail("%s: %u rows, at most %u (blocks of %d rows)", who, h->n_local, 65535u * 16u * KG_BT, 16 * KG_BT);
    return 0;
}

// the individual-major image of the whole BED: allocated here, refused when it does not fit beside `extra` bytes; king_image_build
// writes it
int king_image(hgibbs_ctx* h, size_t extra, DevBuf<uint32_t>& img, uint32_t& npi, uint32_t& ntile, uint32_t& nks, const char* who)
{
    ntile = (h->n_local + 15u) / 16u;
    npi = 16u * ntile;
    nks = (h->M + 63u) / 64u;
    const uint32_t ngrp = 4u * nks;
    const size_t words = (size_t)ngrp * npi;
    if (need_device_memory(words * 4u + extra, "%s: the individual-major image needs %.1f MiB and the call %.1f MiB more", who, words * 4u / 1048576.0,
                           extra / 1048576.0))
        return 1;
    return img.alloc(words);
}

int king_image_build(hgibbs_ctx* h, uint32_t* img, uint32_t npi, uint32_t ntile, uint32_t nks)
{
    const uint32_t ngrp = 4u * nks;
    const uint32_t gy = std::min<uint32_t>(ngrp, 65535u), gz = (ngrp + 65534u) / 65535u;
    k_king_image<<<dim3((ntile + 255u) / 256u, gy, gz), 256, 0, h->stream>>>(h->bed, h->stride, h->M, h->n_local, ntile, ngrp, npi, img);
    HIP_TRY(hipGetLastError());
    return 0;
}

// nbp block pairs on a 2-D grid of at most KG_GX workgroups in x; z = ranges of markers
dim3 king_grid(size_t nbp, uint32_t split)
{
    const uint32_t gx = (uint32_t)std::min<size_t>(nbp, KG_GX);
    return dim3(gx, (uint32_t)((nbp + gx - 1) / gx), split);
}

} // namespace

extern "C" int hgibbs_king(hgibbs_t h, uint32_t a0, uint32_t acount, uint32_t b0, uint32_t bcount, int32_t* counts)
{
    if (king_check(h, "hgibbs_king")) return 1;
    if ((uint64_t)a0 + acount > h->n_local || (uint64_t)b0 + bcount > h->n_local)
        return fail("hgibbs_king: rows [%u, %llu) x [%u, %llu) out of range (n_local = %u)", a0, (unsigned long long)a0 + acount, b0,
                    (unsigned long long)b0 + bcount, h->n_local);
    if (acount && bcount && !counts) return fail("hgibbs_king: null counts");
    h->king_ms = 0.0;
    if (acount == 0 || bcount == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));

    // pieces of A rows: at most 2^25 pairs (640 MiB of counts) on the device at a time
    const uint32_t piece = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(acount, (1ull << 25) / bcount));
    const size_t pbytes = (size_t)piece * bcount * 5u * sizeof(int32_t);
    DevBuf<uint32_t> img, bpairs;
    DevBuf<int32_t> dcounts;
    uint32_t npi = 0, ntile = 0, nks = 0;
    double total_ms = 0.0;
    if (king_image(h, pbytes, img, npi, ntile, nks, "hgibbs_king")) return 1;
    if (dcounts.alloc((size_t)piece * bcount * 5u)) return 1;
    if (lap_begin(h)) return 1; // (after the allocations: the device time is the kernels')
    if (king_image_build(h, img, npi, ntile, nks)) return 1;
    if (lap_end(h, total_ms)) return 1;
    const uint32_t tb0 = b0 / 16u, nbb = ((b0 + bcount - 1u) / 16u - tb0) / KG_BT + 1u;
    for (uint32_t p0 = a0; p0 < a0 + acount; p0 += piece) {
        const uint32_t pc = std::min(piece, a0 + acount - p0);
        const uint32_t ta0 = p0 / 16u, nba = ((p0 + pc - 1u) / 16u - ta0) / KG_BT + 1u;
        std::vector<uint32_t> bp;
        bp.reserve((size_t)nba * nbb);
        for (uint32_t i = 0; i < nba; ++i)
            for (uint32_t j = 0; j < nbb; ++j) bp.push_back((i << 16) | j);
        if (bpairs.alloc(bp.size())) return 1;
        HIP_TRY(hipMemcpy(bpairs, bp.data(), bp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        // marker ranges: enough workgroups for two per compute unit (option king_split fixes the number)
        uint32_t ks_per = 0;
        const uint32_t split =
            split_ranges(nks, h->king_split ? (uint32_t)h->king_split : (uint32_t)((2ull * h->num_cu + bp.size() - 1) / bp.size()), NO_CAP, ks_per);
        KingArgs a{};
        a.img = img;
        a.bpairs = bpairs;
        a.nbp = (uint32_t)bp.size();
        a.npi = npi;
        a.ntile = ntile;
        a.nks = nks;
        a.ks_per = ks_per;
        a.ta0 = ta0;
        a.tb0 = tb0;
        a.counts = dcounts;
        a.ra0 = p0;
        a.racount = pc;
        a.rb0 = b0;
        a.rbcount = bcount;
        if (lap_begin(h)) return 1;
        HIP_TRY(hipMemsetAsync(dcounts, 0, (size_t)pc * bcount * 5u * sizeof(int32_t), h->stream));
        k_king<false><<<king_grid(bp.size(), split), KG_WAVES * 64, 0, h->stream>>>(a);
        HIP_TRY(hipGetLastError());
        if (lap_end(h, total_ms)) return 1;
        HIP_TRY(hipMemcpy(counts + (size_t)(p0 - a0) * bcount * 5u, dcounts, (size_t)pc * bcount * 5u * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    h->king_ms = total_ms;
    return 0;
}

extern "C" int hgibbs_king_pairs(hgibbs_t h, double cutoff, uint64_t* npairs)
{
    if (king_check(h, "hgibbs_king_pairs")) return 1;
    if (!npairs) return fail("hgibbs_king_pairs: null npairs");
    if (!std::isfinite(cutoff)) return fail("hgibbs_king_pairs: the cutoff must be a finite number");
    HIP_TRY(hipSetDevice(h->device));
    h->king_ab.clear();
    h->king_counts.clear();
    h->king_kin.clear();
    *npairs = 0;
    h->king_ms = 0.0;

    DevBuf<uint32_t> img, bpairs, dab;
    DevBuf<unsigned long long> nlist;
    DevBuf<int32_t> lcounts;
    DevBuf<double> lkin;
    uint32_t npi = 0, ntile = 0, nks = 0;
    const uint64_t all = (uint64_t)h->n_local * (h->n_local - 1u) / 2u;
    unsigned long long cap = std::max<uint64_t>(1, std::min<uint64_t>(all, KG_LIST0));
    const size_t per = 2 * sizeof(uint32_t) + 5 * sizeof(int32_t) + sizeof(double);
    double total_ms = 0.0;
    const uint32_t nb = ((h->n_local + 15u) / 16u + KG_BT - 1u) / KG_BT; // blocks of 128 rows
    std::vector<uint32_t> bp;
    bp.reserve((size_t)nb * (nb + 1u) / 2u);
    for (uint32_t i = 0; i < nb; ++i)
        for (uint32_t j = i; j < nb; ++j) bp.push_back((i << 16) | j);
    if (king_image(h, cap * per + bp.size() * sizeof(uint32_t), img, npi, ntile, nks, "hgibbs_king_pairs")) return 1;
    if (bpairs.alloc(bp.size())) return 1;
    HIP_TRY(hipMemcpy(bpairs, bp.data(), bp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (nlist.alloc(1)) return 1;
    unsigned long long found = 0;
    for (bool first = true;; first = false) {
        if (dab.alloc(cap * 2) || lcounts.alloc(cap * 5) || lkin.alloc(cap)) return 1;
        if (lap_begin(h)) return 1; // (after the allocations: the device time is the kernels')
        if (first && king_image_build(h, img, npi, ntile, nks)) return 1;
        HIP_TRY(hipMemsetAsync(nlist, 0, sizeof(unsigned long long), h->stream));
        KingArgs a{};
        a.img = img;
        a.bpairs = bpairs;
        a.nbp = (uint32_t)bp.size();
        a.npi = npi;
        a.ntile = ntile;
        a.nks = nks;
        a.ks_per = nks; // every marker in one workgroup: the formula needs the whole counts
        a.n_local = h->n_local;
        a.cutoff = cutoff;
        a.nlist = nlist;
        a.cap = cap;
        a.ab = dab;
        a.lcounts = lcounts;
        a.lkin = lkin;
        k_king<true><<<king_grid(bp.size(), 1), KG_WAVES * 64, 0, h->stream>>>(a);
        HIP_TRY(hipGetLastError());
        if (lap_end(h, total_ms)) return 1;
        HIP_TRY(hipMemcpy(&found, nlist, sizeof found, hipMemcpyDeviceToHost));
        if (found <= cap) break;
        // the list overflowed: every pair was counted, so the second run fits exactly (the first list goes before the check)
        dab.release();
        lcounts.release();
        lkin.release();
        cap = found;
        if (need_device_memory(cap * per, "hgibbs_king_pairs: %llu pairs pass the cutoff %g: the list needs %.1f MiB", found, cutoff, cap * per / 1048576.0))
            return 1;
    }

    // the list, sorted by (a, b): the order of the atomics never shows
    std::vector<uint32_t> ab(found * 2);
    std::vector<int32_t> cnt(found * 5);
    std::vector<double> kin(found);
    if (found) {
        HIP_TRY(hipMemcpy(ab.data(), dab, ab.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(cnt.data(), lcounts, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(kin.data(), lkin, kin.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    std::vector<uint64_t> key(found);
    for (size_t i = 0; i < found; ++i) key[i] = ((uint64_t)ab[2 * i] << 32) | ab[2 * i + 1];
    std::vector<size_t> ord(found);
    for (size_t i = 0; i < found; ++i) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return key[x] < key[y]; });
    h->king_ab.resize(found * 2);
    h->king_counts.resize(found * 5);
    h->king_kin.resize(found);
    for (size_t i = 0; i < found; ++i) {
        const size_t s = ord[i];
        h->king_ab[2 * i] = ab[2 * s];
        h->king_ab[2 * i + 1] = ab[2 * s + 1];
        for (int q = 0; q < 5; ++q) h->king_counts[5 * i + q] = cnt[5 * s + q];
        h->king_kin[i] = kin[s];
    }
    h->king_ms = total_ms;
    *npairs = found;
    return 0;
}

extern "C" int hgibbs_king_pairs_get(hgibbs_t h, uint32_t* ab, int32_t* counts, double* kin)
{
    if (!h) return fail("hgibbs_king_pairs_get: null handle");
    const size_t n = h->king_kin.size();
    if (ab && n) std::memcpy(ab, h->king_ab.data(), n * 2 * sizeof(uint32_t));
    if (counts && n) std::memcpy(counts, h->king_counts.data(), n * 5 * sizeof(int32_t));
    if (kin && n) std::memcpy(kin, h->king_kin.data(), n * sizeof(double));
    return 0;
}

extern "C" int hgibbs_last_king_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_king_ms: null argument");
    *ms = h->king_ms;
    return 0;
}
