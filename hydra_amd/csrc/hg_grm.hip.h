// GCTA-style genomic relationship matrix of the loaded rows: S = X X' with the chain's standardised genotypes
// (x = 0 at a missing call), the lower triangle with the diagonal, as exact integer sums on v_mfma_i32_16x16x64_i8.
//
// Definition.  Rows are the handle's n_local rows, markers its M columns, mave_j and mstd_j those of hgibbs_marker_stats, g in {0, 1, 2}
// the genotype as hgibbs_load_bed reads it.  A marker is USED when mstd_j is finite; M_used is their number.  Per used marker and
// genotype, two f64 values, every operation rounded on its own (no fused multiply-add):
//
//     y_jg = (mstd_j mstd_j) (g - mave_j)        z_jg = mave_j y_jg
//
// W = the largest |y| or |z| of the table, e the smallest integer with W < 2^e, E = 52 - e (E = 0 for an all-zero table);
// qy = llrint(y 2^E), qz = llrint(z 2^E).  For a >= b (row a is the weight side, b the code side):
//
//     T_ab    = sum_{j used, a and b called at j} ( g_bj qy[j][g_aj] - qz[j][g_aj] )      (an exact integer)
//     S_ab    = T_ab 2^-E, rounded to f64 once
//     NSNP_ab = #{ j used : a and b called at j }
//
// |S_ab - exact| <= 1.5 M_used 2^-E <= 3 M_used W 2^-52 (the form of hgibbs_score's bound); the GCTA entry is S_ab / NSNP_ab.
//
//   table     k_grm_max finds W and M_used, k_grm_table writes, per group of sixteen markers, 43 words of 16 bytes: word (2 d + kind) 3 + g
//             holds digit d (seven signed base-256 digits, sc_digit) of qy (kind 0) or of -qz (kind 1) at genotype g, word 42 the used
//             flags (1 or 0); in a word, dword e byte i = marker 16 grp + 4 i + e, the byte order of rl_expand16, which is where
//             kg_forms puts the codes of an image word.  A marker that is not used, or past M, has zeros everywhere.  The bytes depend
//             on the marker only.
//   operands  over k_king_image's individual-major image, lane (c, k) of k-step s reads word (4 s + k, 16 t + c) of its tiles as in
//             k_king.  The code side forms g and c = [called] as bytes.  The weight side forms three byte masks m0, m1, m2 (0xFF where
//             its genotype is 0, 1, 2; all zero at a missing call) and, per digit, the operand words
//             (Y0_d & m0) | (Y1_d & m1) | (Y2_d & m2), the same with the words of -qz: three bitwise operations a dword.  The table words
//             of a lane are those of group 4 s + k, the same for the sixteen lanes c and for every wave: the 172 words of a k-step
//             (2 752 bytes) are staged in LDS once for the eight waves, double-buffered with one barrier a k-step, and read as
//             ds_read_b128 at one address per sixteen lanes.  (Read as broadcast global loads instead, 42 loads of 16 bytes a wave and
//             k-step through the texture path, the same kernel took 918 ms where this one takes 731 ms: DESIGN.md section 19.)  A wave
//             of a diagonal block that holds no entry still stages and meets the barriers.
//   products  per tile pair and k-step 15: g x y-digit and c x (-z)-digit, both into the accumulator of digit d (seven accumulators),
//             and c x c' for NSNP, c' = the weight side's called bytes ANDed with the used flags.  A digit's sum is at most
//             (2 x 128 + 128) M = 384 M in absolute value: M <= GR_MMAX = 5 592 405 keeps it inside an i32 (below the 2^23 of KING's form
//             with one accumulator a product).
//   tiling    KING's blocks of 128 x 128 individuals, block pairs on king_grid's 2-D grid, 8 waves.  Eight accumulators a tile pair
//             (32 registers) do not fit at KING's 8 tile pairs a wave: a wave takes ONE weight tile against four code tiles (128
//             registers), in two passes over the markers for its two weight tiles 2 (w & 3) + {0, 1}; the code tiles are 4 (w >> 2) + {0..3}.
//             Only tile pairs that hold an entry with a >= b run.
//   exact     T = hi 2^32 + lo with lo = digits 0..3 and hi = digits 4..6 (64-bit), rounded once by round_halves.  With the markers
//             split over workgroups (option grm_split) the parts meet in i32 atomic adds of the eight accumulators and k_grm_final
//             rounds; one range (the automatic choice of a large call) rounds in the product kernel.  Both give the same bits, for
//             any chunking of the rows, any split and any repeat.
//
// Registers (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no scratch, no spills): DESIGN.md section 19.
#pragma once

namespace {

constexpr int GR_RB = 4;                      // code tiles per wave (one weight tile a pass, two passes)
constexpr int GR_ND = 7;                      // digits
constexpr int GR_NA = GR_ND + 1;              // accumulators a tile pair: the digits and NSNP
constexpr uint32_t GR_TW = 6 * GR_ND + 1;     // table words (16 bytes) per group of sixteen markers
constexpr uint32_t GR_STAGE = 4 * GR_TW;      // table words of a k-step (four groups)
constexpr uint32_t GR_MMAX = 0x7FFFFFFFu / 384u; // markers at most (the i32 digit sums, above)
constexpr uint64_t GR_PIECE = 1ull << 25;     // pairs on the device at a time

struct GrmArgs {
    const uint32_t* img;    // [group][npi] words of sixteen 2-bit codes (k_king_image)
    const rl_v4i* tab;      // [group][GR_TW]
    const uint32_t* bpairs; // block pairs, (bi << 16) | bj: weight block bi (from tile ta0), code block bj (from tile 0)
    uint32_t nbp, npi, ntile, nks, ks_per, ta0;
    uint32_t ra0, racount;  // rows of this piece
    unsigned long long off0; // packed offset of row ra0: ra0 (ra0 + 1) / 2
    int E;
    int32_t* acc;           // [pair][GR_NA] (several ranges of markers)
    double* S;              // [pair]
    int32_t* nsnp;          // [pair]
};

// y and z of marker (av, sd) at genotype g, every operation rounded on its own
__device__ __forceinline__ void gr_yz(double av, double sd, int g, double& y, double& z)
{
    y = __dmul_rn(__dmul_rn(sd, sd), __dsub_rn((double)g, av));
    z = __dmul_rn(av, y);
}

// meta[0] = the bit pattern of W (atomic max: non-negative doubles order as integers), meta[1] = M_used
__global__ __launch_bounds__(256) void k_grm_max(const double* __restrict__ mave, const double* __restrict__ mstd, uint32_t M,
                                                  unsigned long long* __restrict__ meta)
{
    __shared__ double smax[256];
    __shared__ uint32_t sused[256];
    const uint32_t t = threadIdx.x, j = blockIdx.x * 256u + t;
    double mx = 0.0;
    uint32_t used = 0;
    if (j < M && isfinite(mstd[j])) {
        used = 1;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            double y, z;
            gr_yz(mave[j], mstd[j], g, y, z);
            mx = fmax(mx, fmax(fabs(y), fabs(z)));
        }
    }
    smax[t] = mx;
    sused[t] = used;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < (uint32_t)w) {
            smax[t] = fmax(smax[t], smax[t + w]);
            sused[t] += sused[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        if (smax[0] > 0.0) atomicMax(meta, (unsigned long long)__double_as_longlong(smax[0]));
        if (sused[0]) atomicAdd(meta + 1, (unsigned long long)sused[0]);
    }
}

// Thread j: the 42 digit bytes and the used flag of marker j (the table is zero before: a marker that is not used writes nothing)
__global__ __launch_bounds__(256) void k_grm_table(const double* __restrict__ mave, const double* __restrict__ mstd, uint32_t M, int E,
                                                    uint8_t* __restrict__ tab)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= M || !isfinite(mstd[j])) return;
    const uint32_t w = j & 15u;
    uint8_t* t = tab + (size_t)(j >> 4) * GR_TW * 16u + (w & 3u) * 4u + (w >> 2);
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        double y, z;
        gr_yz(mave[j], mstd[j], g, y, z);
        const long long qy = sc_quant(y, E), nz = -sc_quant(z, E);
#pragma unroll
        for (int d = 0; d < GR_ND; ++d) {
            t[((2 * d) * 3 + g) * 16] = (uint8_t)sc_digit(qy, d);
            t[((2 * d + 1) * 3 + g) * 16] = (uint8_t)sc_digit(nz, d);
        }
    }
    t[(GR_TW - 1u) * 16u] = 1;
}

// the code side: g (0 at a missing call) and c = [called], sixteen codes of one word as bytes (the byte order of kg_forms)
__device__ __forceinline__ void gr_code_forms(uint32_t x, rl_v4i& g, rl_v4i& c)
{
    const uint32_t m = x & (x >> 1) & 0x55555555u; // [code == 3]
    const uint32_t cw = m ^ 0x55555555u;
    const uint32_t gw = x & ~(m | (m << 1));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        g[e] = (int)((gw >> (2 * e)) & 0x03030303u);
        c[e] = (int)((cw >> (2 * e)) & 0x01010101u);
    }
}

// the weight side: byte masks of genotype 0, 1, 2 (0xFF or 0) and c = [called]
__device__ __forceinline__ void gr_masks(uint32_t x, rl_v4i& m0, rl_v4i& m1, rl_v4i& m2, rl_v4i& c)
{
    const uint32_t lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
    const uint32_t e1 = lo & ~hi, e2 = hi & ~lo, e0 = (lo | hi) ^ 0x55555555u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t b0 = (e0 >> (2 * e)) & 0x01010101u, b1 = (e1 >> (2 * e)) & 0x01010101u, b2 = (e2 >> (2 * e)) & 0x01010101u;
        m0[e] = (int)((b0 << 8) - b0); // per byte 0xFF b: the bytes do not meet (mod 2^32)
        m1[e] = (int)((b1 << 8) - b1);
        m2[e] = (int)((b2 << 8) - b2);
        c[e] = (int)(b0 | b1 | b2);
    }
}

// hi (digits 4..6) and lo (digits 0..3) of T from the seven digit sums
__device__ __forceinline__ void gr_halves(const int32_t* a, long long& hi, long long& lo)
{
    lo = (long long)a[0] + ((long long)a[1] << 8) + ((long long)a[2] << 16) + ((long long)a[3] << 24);
    hi = (long long)a[4] + ((long long)a[5] << 8) + ((long long)a[6] << 16);
}

// Workgroup (x, y, z): block pair bpairs[x + gridDim.x y], k-steps [z ks_per, (z + 1) ks_per).  WHOLE: one range of markers, the entry is
// rounded here (else the accumulators meet in atomic adds and k_grm_final rounds).
template <bool WHOLE>
__global__ __launch_bounds__(KG_WAVES * 64) void k_grm(GrmArgs p)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = lane & 15u, k4 = lane >> 4;
    const uint64_t bpi = (uint64_t)blockIdx.x + (uint64_t)gridDim.x * blockIdx.y;
    if (bpi >= p.nbp) return; // (uniform: the last row of the grid)
    const uint32_t bp = p.bpairs[bpi];
    const uint32_t tbw = KG_BT * (bp & 0xFFFFu) + GR_RB * (wave >> 2);
    const uint32_t s0 = blockIdx.z * p.ks_per, s1 = min(p.nks, s0 + p.ks_per);
    const uint32_t ta_end = min(p.ntile, (p.ra0 + p.racount + 15u) / 16u);
    if (s0 >= s1) return; // (uniform over the workgroup: before any barrier)
    // the table words of a k-step (groups 4 s .. 4 s + 3: GR_STAGE words in a row), staged once for the eight waves, double-buffered
    __shared__ rl_v4i stab[2][GR_STAGE];
    const bool stager = threadIdx.x < GR_STAGE;

#pragma unroll 1
    for (uint32_t pass = 0; pass < 2u; ++pass) {
        const uint32_t ta = p.ta0 + KG_BT * (bp >> 16) + 2u * (wave & 3u) + pass;
        // the tile pairs that hold an entry with a >= b (tb <= ta < ntile: a code tile that is on exists); a wave without one
        // still stages and meets the barriers
        bool on[GR_RB];
        bool any = false;
#pragma unroll
        for (int j = 0; j < GR_RB; ++j) {
            on[j] = ta < ta_end && tbw + (uint32_t)j <= ta;
            any = any || on[j];
        }

        rl_v4i acc[GR_RB][GR_NA];
#pragma unroll
        for (int j = 0; j < GR_RB; ++j)
#pragma unroll
            for (int q = 0; q < GR_NA; ++q) acc[j][q] = rl_v4i{0, 0, 0, 0};

        // lane (c, k) of k-step s: word (4 s + k, 16 t + c); a tile that is off reads as code 3 everywhere (no load)
        auto load = [&](uint32_t s, uint32_t& wa, uint32_t* wb) {
            const uint32_t* row = p.img + (size_t)(4u * s + k4) * p.npi + c;
            wa = any ? row[16u * ta] : 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < GR_RB; ++j) wb[j] = on[j] ? row[16u * (tbw + (uint32_t)j)] : 0xFFFFFFFFu;
        };
        uint32_t wa, wb[GR_RB];
        load(s0, wa, wb);
        if (stager) stab[0][threadIdx.x] = p.tab[(size_t)4u * s0 * GR_TW + threadIdx.x];
        __syncthreads(); // (the last barrier of pass 0 is behind every read of stab[0])
        for (uint32_t s = s0; s < s1; ++s) {
            const uint32_t buf = (s - s0) & 1u;
            uint32_t na = 0, nb[GR_RB];
            rl_v4i pre = {0, 0, 0, 0};
            if (s + 1u < s1) { // (uniform) the next k-step's words in flight
                load(s + 1u, na, nb);
                if (stager) pre = p.tab[(size_t)4u * (s + 1u) * GR_TW + threadIdx.x];
            }
            if (any) { // (uniform over the wave)
                const rl_v4i* tw = &stab[buf][k4 * GR_TW];
                rl_v4i gb[GR_RB], cb[GR_RB];
#pragma unroll
                for (int j = 0; j < GR_RB; ++j) gr_code_forms(wb[j], gb[j], cb[j]);
                rl_v4i m0, m1, m2, ca;
                gr_masks(wa, m0, m1, m2, ca);
                ca &= tw[GR_TW - 1u];
#pragma unroll
                for (int j = 0; j < GR_RB; ++j)
                    if (on[j]) acc[j][GR_ND] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ca, cb[j], acc[j][GR_ND], 0, 0, 0);
#pragma unroll
                for (int d = 0; d < GR_ND; ++d) {
                    const rl_v4i Y = (tw[6 * d] & m0) | (tw[6 * d + 1] & m1) | (tw[6 * d + 2] & m2);
                    const rl_v4i Z = (tw[6 * d + 3] & m0) | (tw[6 * d + 4] & m1) | (tw[6 * d + 5] & m2);
#pragma unroll
                    for (int j = 0; j < GR_RB; ++j)
                        if (on[j]) acc[j][d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Y, gb[j], acc[j][d], 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < GR_RB; ++j)
                        if (on[j]) acc[j][d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Z, cb[j], acc[j][d], 0, 0, 0);
                }
            }
            if (s + 1u < s1) {
                wa = na;
#pragma unroll
                for (int j = 0; j < GR_RB; ++j) wb[j] = nb[j];
                if (stager) stab[buf ^ 1u][threadIdx.x] = pre; // (last read a k-step ago, a barrier in between)
            }
            __syncthreads();
        }
        if (!any) continue; // (uniform over the wave; no barrier below in this pass)

        // lane (c, k), register r: a = 16 ta + 4 k + r, b = 16 tb + c
#pragma unroll
        for (int j = 0; j < GR_RB; ++j) {
            if (!on[j]) continue; // (uniform)
            const uint32_t b = 16u * (tbw + (uint32_t)j) + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t a = 16u * ta + 4u * k4 + (uint32_t)r;
                if (a < p.ra0 || a - p.ra0 >= p.racount || b > a) continue;
                const unsigned long long at = (unsigned long long)a * (a + 1ull) / 2ull - p.off0 + b;
                int32_t v[GR_NA];
#pragma unroll
                for (int q = 0; q < GR_NA; ++q) v[q] = acc[j][q][r];
                if constexpr (WHOLE) {
                    long long hi, lo;
                    gr_halves(v, hi, lo);
                    p.S[at] = round_halves(hi, lo, p.E);
                    p.nsnp[at] = v[GR_ND];
                } else {
#pragma unroll
                    for (int q = 0; q < GR_NA; ++q)
                        if (v[q]) __hip_atomic_fetch_add(p.acc + at * GR_NA + q, v[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
}

// Thread t: entry t of the piece from its eight accumulators
__global__ __launch_bounds__(256) void k_grm_final(const int32_t* __restrict__ acc, unsigned long long n, int E, double* __restrict__ S,
                                                    int32_t* __restrict__ nsnp)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (t >= n) return;
    int32_t v[GR_NA];
#pragma unroll
    for (int q = 0; q < GR_NA; ++q) v[q] = acc[t * GR_NA + q];
    long long hi, lo;
    gr_halves(v, hi, lo);
    S[t] = round_halves(hi, lo, E);
    nsnp[t] = v[GR_ND];
}

// one piece of rows and its launch
struct GrmPiece {
    uint32_t p0, pc, ta0, split, ks_per;
    uint64_t pairs;
    std::vector<uint32_t> bp;
};

int grm_mmax_check(const hgibbs_ctx* h, const char* who)
{
    if (h->M > GR_MMAX) return fail("%s: %u markers, at most %u (a digit's sum, at most 384 a marker, stays inside an i32)", who, h->M, GR_MMAX);
    return 0;
}

// The frame of hgibbs_grm and hgibbs_grm_rowsums (`who`): rows [a0, a0 + acount) in pieces of at most grm_piece (GR_PIECE) pairs, the
// table and the image, then per piece the products, which leave the piece's S and NSNP on the device, and step(piece, pairs done
// before it, dS, dn), which does with them what the caller is there for.  The caller has set the device and run compute_stats (the
// marker stats are a precondition, not computed here); the device time of the kernels launched here goes to total_ms, M_used and E to
// used and E.
template <class Step>
int grm_pieces(hgibbs_ctx* h, const char* who, uint32_t a0, uint32_t acount, double& total_ms, uint32_t& used, int& E, Step&& step)
{
    // pieces of rows, at most GR_PIECE pairs each (a row alone has fewer), and their block pairs
    const uint64_t piece = h->grm_piece ? (uint64_t)h->grm_piece : GR_PIECE;
    const uint32_t nks = (h->M + 63u) / 64u, aend = a0 + acount;
    std::vector<GrmPiece> pieces;
    uint64_t maxpairs = 0, maxbp = 0;
    bool parts = false;
    for (uint32_t p0 = a0; p0 < aend;) {
        GrmPiece pc{};
        pc.p0 = p0;
        uint32_t a = p0;
        while (a < aend && (a == p0 || pc.pairs + a + 1ull <= piece)) pc.pairs += a++ + 1ull;
        pc.pc = a - p0;
        pc.ta0 = p0 / 16u;
        const uint32_t tlast = (a - 1u) / 16u, nba = (tlast - pc.ta0) / KG_BT + 1u;
        for (uint32_t i = 0; i < nba; ++i) {
            const uint32_t tmax = std::min(tlast, pc.ta0 + KG_BT * i + KG_BT - 1u); // the block's last weight tile: code blocks up to it
            for (uint32_t j = 0; j <= tmax / KG_BT; ++j) pc.bp.push_back((i << 16) | j);
        }
        pc.split = split_ranges(nks, h->grm_split ? (uint32_t)h->grm_split : (uint32_t)((2ull * h->num_cu + pc.bp.size() - 1) / pc.bp.size()), NO_CAP,
                                pc.ks_per);
        parts = parts || pc.split > 1u;
        maxpairs = std::max(maxpairs, pc.pairs);
        maxbp = std::max<uint64_t>(maxbp, pc.bp.size());
        p0 = a;
        pieces.push_back(std::move(pc));
    }

    DevBuf<uint32_t> img, bpairs;
    DevBuf<rl_v4i> tab;
    DevBuf<unsigned long long> meta;
    DevBuf<int32_t> dacc, dn;
    DevBuf<double> dS;
    uint32_t npi = 0, ntile = 0, nks2 = 0;
    const size_t tabw = (size_t)4u * nks * GR_TW;
    const size_t extra = tabw * sizeof(rl_v4i) + maxbp * sizeof(uint32_t) +
                         maxpairs * (sizeof(double) + sizeof(int32_t) + (parts ? GR_NA * sizeof(int32_t) : 0));
    if (king_image(h, extra, img, npi, ntile, nks2, who)) return 1;
    if (tab.alloc(tabw) || meta.alloc(2) || bpairs.alloc(maxbp) || dS.alloc(maxpairs) || dn.alloc(maxpairs)) return 1;
    if (parts && dacc.alloc(maxpairs * GR_NA)) return 1;

    // W and M_used, then the table and the image
    const uint32_t mblocks = (h->M + 255u) / 256u;
    if (lap_begin(h)) return 1;
    HIP_TRY(hipMemsetAsync(meta, 0, 2 * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(tab, 0, tabw * sizeof(rl_v4i), h->stream));
    k_grm_max<<<mblocks, 256, 0, h->stream>>>(h->mave, h->mstd, h->M, meta);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, total_ms)) return 1;
    unsigned long long mh[2] = {0, 0};
    HIP_TRY(hipMemcpy(mh, meta, sizeof mh, hipMemcpyDeviceToHost));
    if (mh[1] == 0) return fail("%s: no marker of the %u loaded has a finite mstd (M_used = 0): the matrix is not defined", who, h->M);
    E = 0;
    {
        double W;
        std::memcpy(&W, &mh[0], sizeof W);
        if (W > 0.0) {
            int e;
            (void)std::frexp(W, &e); // W < 2^e
            E = 52 - e;
        }
    }
    used = (uint32_t)mh[1];
    if (lap_begin(h)) return 1;
    k_grm_table<<<mblocks, 256, 0, h->stream>>>(h->mave, h->mstd, h->M, E, reinterpret_cast<uint8_t*>(tab.p));
    HIP_TRY(hipGetLastError());
    if (king_image_build(h, img, npi, ntile, nks)) return 1;
    if (lap_end(h, total_ms)) return 1;

    size_t done = 0;
    for (const GrmPiece& pc : pieces) {
        HIP_TRY(hipMemcpy(bpairs, pc.bp.data(), pc.bp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        GrmArgs a{};
        a.img = img;
        a.tab = tab;
        a.bpairs = bpairs;
        a.nbp = (uint32_t)pc.bp.size();
        a.npi = npi;
        a.ntile = ntile;
        a.nks = nks;
        a.ks_per = pc.ks_per;
        a.ta0 = pc.ta0;
        a.ra0 = pc.p0;
        a.racount = pc.pc;
        a.off0 = (unsigned long long)pc.p0 * (pc.p0 + 1ull) / 2ull;
        a.E = E;
        a.acc = dacc;
        a.S = dS;
        a.nsnp = dn;
        if (lap_begin(h)) return 1;
        if (pc.split > 1u) {
            HIP_TRY(hipMemsetAsync(dacc, 0, pc.pairs * GR_NA * sizeof(int32_t), h->stream));
            k_grm<false><<<king_grid(pc.bp.size(), pc.split), KG_WAVES * 64, 0, h->stream>>>(a);
            HIP_TRY(hipGetLastError());
            k_grm_final<<<(uint32_t)((pc.pairs + 255u) / 256u), 256, 0, h->stream>>>(dacc, pc.pairs, E, dS, dn);
        } else {
            k_grm<true><<<king_grid(pc.bp.size(), 1), KG_WAVES * 64, 0, h->stream>>>(a);
        }
        HIP_TRY(hipGetLastError());
        if (lap_end(h, total_ms)) return 1;
        if (step(pc, done, (const double*)dS, (const int32_t*)dn)) return 1;
        done += pc.pairs;
    }
    return 0;
}

} // namespace

extern "C" int hgibbs_grm(hgibbs_t h, uint32_t a0, uint32_t acount, double* S, int32_t* nsnp)
{
    if (king_check(h, "hgibbs_grm")) return 1;
    h->grm_ms = 0.0;
    h->grm_used = 0;
    h->grm_E = 0;
    if (grm_mmax_check(h, "hgibbs_grm")) return 1;
    if (acount == 0) return fail("hgibbs_grm: no rows asked for (acount = 0)");
    if ((uint64_t)a0 + acount > h->n_local)
        return fail("hgibbs_grm: rows [%u, %llu) out of range (n_local = %u)", a0, (unsigned long long)a0 + acount, h->n_local);
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;

    double total_ms = 0.0;
    uint32_t used = 0;
    int E = 0;
    // the step of a piece: the copy out
    auto copy_out = [&](const GrmPiece& pc, size_t done, const double* dS, const int32_t* dn) -> int {
        if (S) HIP_TRY(hipMemcpy(S + done, dS, pc.pairs * sizeof(double), hipMemcpyDeviceToHost));
        if (nsnp) HIP_TRY(hipMemcpy(nsnp + done, dn, pc.pairs * sizeof(int32_t), hipMemcpyDeviceToHost));
        return 0;
    };
    if (grm_pieces(h, "hgibbs_grm", a0, acount, total_ms, used, E, copy_out)) return 1;
    h->grm_ms = total_ms;
    h->grm_used = used;
    h->grm_E = E;
    return 0;
}

extern "C" int hgibbs_grm_info(hgibbs_t h, uint32_t* m_used, int32_t* E)
{
    if (!h) return fail("hgibbs_grm_info: null handle");
    if (m_used) *m_used = h->grm_used;
    if (E) *E = h->grm_E;
    return 0;
}

extern "C" int hgibbs_last_grm_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_grm_ms: null argument");
    *ms = h->grm_ms;
    return 0;
}
