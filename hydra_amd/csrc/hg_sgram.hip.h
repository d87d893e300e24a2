// Row-weighted Gram matrices of marker sets: for each set s of m_s listed markers and ONE weight vector w over
// the handle's n_local individuals, the exact integer sums
//
//     GG_ab = sum_i q_i g_ia g_ib,   GC_ab = sum_i q_i g_ia c_ib,   CC_ab = sum_i q_i c_ia c_ib,      q_i = llrint(w_i 2^E)
//
// (g in {0, 1, 2} the stored genotype, 0 at a missing call; c in {0, 1} "called"), each rounded to f64 ONCE (times 2^-E), and from them
// out_ab = sd_a sd_b (GG_ab - m_b GC_ab - m_a GC_ba + m_a m_b CC_ab) = sum_i w_i x_ia x_ib for the chain's standardised x.  This is the
// first term of the score covariance of a set test; hgibbs_marker_class_sums gives the second.  The frame is that of hg_mdots.hip.h
// (scale, digit image, 64-bit halves, one rounding); the product is turned: both operands come from the BED, and the digits of q ride
// on one of them.
//
//   scale    one E for the vector, hgibbs_marker_dots' rule (k_score_max, k_score_ksum): E = 52 - e with max_i w_i < 2^e, q in seven
//            signed base-256 digits.  The only error is that rounding, half a unit of 2^-E a row against g_a g_b <= 4:
//            |GG 2^-E - sum w g_a g_b| <= 2 n 2^-E <= 4 n max(w) 2^-52, |GC ..| <= n 2^-E <= 2 n max(w) 2^-52,
//            |CC ..| <= n 2^-E / 2 <= n max(w) 2^-52, each before its one rounding.
//   job      a workgroup owns one (set, 16-marker tile ta, 16-marker tile tb >= ta, range of 512-individual slices); its SG_WAVES
//            waves take the slices of the range in turn, each with accumulators of its own.  The upper triangle of tiles is
//            enough: GG and CC are symmetric, and the job forms both GC_ab and GC_ba.
//   B        (64 individuals x 16 markers of tile ta): lane (c, g) of k-step s expands ONE stored BED dword of ITS marker
//            idx[16 ta + c], gathered through the list (dword 8 g + s of the slice, k_mdots' operand): the bytes g_a, and in the MISS
//            build c_a.  A second form of each holds twice the value (0, 2, 4 resp. 0, 2).
//   A        (16 markers of tile tb x 64 individuals): lane (r, g) expands the dword of marker idx[16 tb + r] into the byte masks
//            [code == 1] and [code == 2] (0x00 or 0xFF, k_mclass' indicators times 255) and ANDs them onto digit k of q for the same
//            sixteen individuals, read from k_mdots_digits' image of w (row k of the image, the same 16 bytes for all sixteen lanes r).
//   form     the issue of a digit times a genotype of 2 not fitting in i8 is settled on the OTHER operand: digit & [code_b == 1]
//            meets g_a, digit & [code_b == 2] meets 2 g_a, and both land in the SAME accumulator, which then holds
//            sum digit_k g_b g_a.  Every i8 stays in range (|digit| <= 128, 2 g_a <= 4), and the seven accumulators of GG are half of
//            what separate d1 and d2 sums would take (registers and atomics), with the same number of products.
//   D        (i32): lane (c, g), register r = entry (b = 16 tb + 4 g + r, a = 16 ta + c) of digit k.  The lane puts digits 0..3
//            together into the entry's low 64-bit half and digits 4..6 into the high one (units of 2^32) and adds them by integer
//            atomics, as k_mdots does.
//   missing  the MISS build is launched when a listed marker lies in a 16-marker granule with missing calls (missing_tiles).  In a
//            job with such a marker in either tile three more families run against the same digits: digit & [code_b != 3] against
//            g_a (GC_ab) and against c_a (CC), and the GG operands against c_a and 2 c_a (GC_ba; not on a diagonal job, where GC_ba
//            is GC_ab transposed).  In every other job GC_ab = sum_i q_i g_ia and CC_ab = sum_i q_i: the first is one more product on
//            the diagonal job of tile ta (the image itself against g_a, k_mdots' product: psum), the second is k_score_ksum's.
//   padding  BED slots past n_local are code 3, but they meet zero digits; list positions past m_s read code 0 and are never written.
//   exact    every i32 partial is a sum of |digit| x 4 <= 512 over the individuals a wave sees, at most SG_SUB_MAX slices of the
//            range (2^21 individuals: 2^30 < 2^31).  n_local < 2^29 keeps the halves (|lo| < 4 n 2^31.01) inside an int64.  Integer
//            sums depend on no tiling, range split (option sgram_split), batching or order of the sets: bit-identical across all.
#pragma once

namespace {

constexpr int SG_WAVES = 4;              // waves per workgroup
constexpr uint32_t SG_SUB_MAX = 4096;    // slices per workgroup at most (i32 headroom, above)
constexpr uint32_t SG_MMAX = 1024;       // markers per set at most
constexpr uint32_t SG_NONE = 0xFFFFFFFFu;

struct SgJob {
    uint64_t ioff, base; // the set's first position in idx, its first entry of out
    uint32_t m, ta, tb, miss;
};

struct SgSet {
    uint64_t ioff, base, toff; // toff: the set's first tile flag
    uint32_t m, pad_;
};

__device__ __forceinline__ rl_v4i sg_and(const rl_v4i& a, const rl_v4i& b)
{
    rl_v4i r;
    r.x = a.x & b.x;
    r.y = a.y & b.y;
    r.z = a.z & b.z;
    r.w = a.w & b.w;
    return r;
}

// packed indicator bits (bit 0 of each 2-bit slot) -> byte masks 0x00 / 0xFF in rl_expand16's placement
__device__ __forceinline__ rl_v4i sg_mask(uint32_t p)
{
    rl_v4i r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t z = (p >> (2 * q)) & 0x01010101u;
        r[q] = (int)((z << 8) - z); // z * 255
    }
    return r;
}

template <bool MISS>
__global__ __launch_bounds__(SG_WAVES * 64) void k_sgram(const uint8_t* __restrict__ bed, uint64_t stride, const uint32_t* __restrict__ idx,
                                                         const SgJob* __restrict__ jobs, uint32_t sub_per, uint32_t n_sub,
                                                         const rl_v4i* __restrict__ img, unsigned long long* __restrict__ acc,
                                                         unsigned long long* __restrict__ psum)
{
    constexpr uint32_t NQ = MISS ? 4u : 1u; // 64-bit pairs per entry: GG, and with MISS GC_ab, GC_ba, CC
    const SgJob jb = jobs[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = lane & 15u, g = lane >> 4;
    const uint32_t s0 = blockIdx.y * sub_per, s1 = min(n_sub, s0 + sub_per);
    if (s0 + wave >= s1) return; // (wave-uniform; no barrier below)
    const bool diag = jb.ta == jb.tb;
    const bool pm = MISS && jb.miss; // (uniform) a tile of the job holds a column with missing calls
    const uint32_t pa = 16u * jb.ta + c, pb = 16u * jb.tb + c;
    const uint32_t ja = pa < jb.m ? idx[jb.ioff + pa] : SG_NONE, jbm = pb < jb.m ? idx[jb.ioff + pb] : SG_NONE;
    const uint8_t* ra = bed + (uint64_t)(ja == SG_NONE ? 0u : ja) * stride + g * 32u;
    const uint8_t* rb = bed + (uint64_t)(jbm == SG_NONE ? 0u : jbm) * stride + g * 32u;

    rl_v4i GG[7], G1[MISS ? 7 : 1], G2[MISS ? 7 : 1], CC[MISS ? 7 : 1], PS = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        GG[k] = rl_v4i{0, 0, 0, 0};
        if constexpr (MISS) {
            G1[k] = rl_v4i{0, 0, 0, 0};
            G2[k] = rl_v4i{0, 0, 0, 0};
            CC[k] = rl_v4i{0, 0, 0, 0};
        }
    }

    for (uint32_t sub = s0 + wave; sub < s1; sub += SG_WAVES) {
        uint4 wa[2], wb[2];
        wa[0] = wa[1] = wb[0] = wb[1] = make_uint4(0u, 0u, 0u, 0u); // (positions past m_s: code 0, never written out)
        if (ja != SG_NONE) {
            const uint4* p = reinterpret_cast<const uint4*>(ra + (uint64_t)sub * (MD_SUBD * 4));
            wa[0] = p[0];
            wa[1] = p[1];
        }
        if (jbm != SG_NONE) {
            const uint4* p = reinterpret_cast<const uint4*>(rb + (uint64_t)sub * (MD_SUBD * 4));
            wb[0] = p[0];
            wb[1] = p[1];
        }
        const rl_v4i* dg = img + (size_t)sub * 8u * 64u; // (one tile: the image of one vector)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const uint32_t xa = md_dword(wa, s), xb = md_dword(wb, s);
            // tile ta: the values.  Clean build: the code itself (a padding slot's 3 meets zero digits)
            rl_v4i ga = rl_expand16(xa), ga2, ca, ca2;
            if constexpr (MISS) {
                const uint32_t p3 = xa & (xa >> 1);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t z3 = (p3 >> (2 * q)) & 0x01010101u;
                    ga[q] = (int)((uint32_t)ga[q] & ~(z3 | (z3 << 1)));
                    ca[q] = (int)(z3 ^ 0x01010101u);
                    ca2[q] = ca[q] << 1;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) ga2[q] = ga[q] << 1;
            // tile tb: the masks
            const uint32_t hb = xb >> 1;
            const rl_v4i m1 = sg_mask(xb & ~hb), m2 = sg_mask(hb & ~xb);
            rl_v4i mc;
            if constexpr (MISS) {
                const rl_v4i m3 = sg_mask(xb & hb);
                mc.x = ~m3.x;
                mc.y = ~m3.y;
                mc.z = ~m3.z;
                mc.w = ~m3.w;
            }
            if (diag) PS = __builtin_amdgcn_mfma_i32_16x16x64_i8(dg[s * 64 + (int)lane], ga, PS, 0, 0, 0);
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const rl_v4i d = dg[s * 64 + k + 16 * (int)g];
                const rl_v4i a1 = sg_and(d, m1), a2 = sg_and(d, m2);
                GG[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, ga, GG[k], 0, 0, 0);
                GG[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2, ga2, GG[k], 0, 0, 0);
                if constexpr (MISS) {
                    if (pm) {
                        const rl_v4i ac = sg_and(d, mc);
                        G1[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ac, ga, G1[k], 0, 0, 0);
                        CC[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ac, ca, CC[k], 0, 0, 0);
                        if (!diag) {
                            G2[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, ca, G2[k], 0, 0, 0);
                            G2[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2, ca2, G2[k], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }

    auto put = [&](const rl_v4i (&D)[7], int r, unsigned long long* p) {
        md_add(p, md_join(rl_v4i{D[0][r], D[1][r], D[2][r], D[3][r]}));
        md_add(p + 1, md_join(rl_v4i{D[4][r], D[5][r], D[6][r], 0}));
    };
    if (pa < jb.m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t b = 16u * jb.tb + 4u * g + (uint32_t)r;
            if (b >= jb.m) continue;
            unsigned long long* p = acc + (jb.base + (uint64_t)pa * jb.m + b) * (2u * NQ);
            put(GG, r, p);
            if constexpr (MISS) {
                if (pm) {
                    put(G1, r, p + 2);
                    if (!diag) put(G2, r, p + 4);
                    put(CC, r, p + 6);
                }
            }
        }
        // the tile's own sums: lane (c, 0) registers 0..3 = digits 0..3, lane (c, 1) registers 0..2 = digits 4..6 (row 7 is zero)
        if (diag && g < 2u) md_add(psum + 2u * (jb.ioff + pa) + g, md_join(PS));
    }
}

// One block per (set, row a), threads over b: the halves rounded once each, then out in its fixed order
__global__ __launch_bounds__(MD_TPB) void k_sgram_final(const SgSet* __restrict__ sets, const uint32_t* __restrict__ rowset,
                                                        const uint32_t* __restrict__ rowpos, const uint32_t* __restrict__ idx,
                                                        const uint8_t* __restrict__ tflag, const unsigned long long* __restrict__ acc,
                                                        const unsigned long long* __restrict__ psum, const unsigned long long* __restrict__ ksum,
                                                        const int* __restrict__ scale, const double* __restrict__ mave,
                                                        const double* __restrict__ mstd, int miss, double* __restrict__ out,
                                                        double* __restrict__ raw)
{
    const SgSet st = sets[rowset[blockIdx.x]];
    const uint32_t a = rowpos[blockIdx.x], m = st.m, ta = a / 16u;
    const uint32_t nq = miss ? 4u : 1u;
    const int E = scale[0];
    const uint32_t ja = idx[st.ioff + a];
    const double ma = mave[ja], sa = mstd[ja];
    const bool fa = miss && tflag[st.toff + ta];
    for (uint32_t b = threadIdx.x; b < m; b += MD_TPB) {
        const uint32_t tb = b / 16u, jb = idx[st.ioff + b];
        const bool up = ta <= tb;
        const unsigned long long* p = acc + (st.base + (up ? (uint64_t)a * m + b : (uint64_t)b * m + a)) * (2u * nq);
        const double GG = round_halves((long long)p[1], (long long)p[0], E);
        double GCab, GCba, CC;
        if (fa || (miss && tflag[st.toff + tb])) {
            const unsigned long long* t = acc + (st.base + (uint64_t)b * m + a) * (2u * nq); // (a diagonal job's transposed entry)
            const unsigned long long* pab = ta == tb ? p + 2 : up ? p + 2 : p + 4;
            const unsigned long long* pba = ta == tb ? t + 2 : up ? p + 4 : p + 2;
            GCab = round_halves((long long)pab[1], (long long)pab[0], E);
            GCba = round_halves((long long)pba[1], (long long)pba[0], E);
            CC = round_halves((long long)p[7], (long long)p[6], E);
        } else {
            const unsigned long long* qa = psum + 2u * (st.ioff + a);
            const unsigned long long* qb = psum + 2u * (st.ioff + b);
            GCab = round_halves((long long)qa[1], (long long)qa[0], E);
            GCba = round_halves((long long)qb[1], (long long)qb[0], E);
            CC = round_halves((long long)ksum[0], (long long)ksum[1], E);
        }
        const double mb = mave[jb], sb = mstd[jb];
        const uint64_t e = st.base + (uint64_t)a * m + b;
        out[e] = isfinite(sa) && isfinite(sb) ? (sa * sb) * (((GG - mb * GCab) - ma * GCba) + (ma * mb) * CC) : __builtin_nan("");
        if (raw) {
            raw[3u * e] = GG;
            raw[3u * e + 1u] = GCab;
            raw[3u * e + 2u] = CC;
        }
    }
}

} // namespace

extern "C" int hgibbs_set_gram(hgibbs_t h, uint32_t nsets, const uint64_t* off, const uint32_t* idx, const double* w, double* out, double* raw)
{
    if (h) h->sgram_ms = 0.0;
    if (op_guard(h, "hgibbs_set_gram", "the sums are not summed over ranks")) return 1;
    if (!off || !idx || !w || !out) return fail("hgibbs_set_gram: null argument");
    if (nsets == 0) return fail("hgibbs_set_gram: nsets = 0, at least one set");
    if (h->n_local >= MD_NMAX) return fail("hgibbs_set_gram: %u individuals, at most %u (64-bit sums)", h->n_local, MD_NMAX - 1u);
    const uint32_t n = h->n_local, M = h->M;
    std::vector<uint32_t> seen(M, SG_NONE);
    for (uint32_t s = 0; s < nsets; ++s) {
        if (off[s + 1] < off[s]) return fail("hgibbs_set_gram: off[%u] = %llu is below off[%u] = %llu", s + 1, (unsigned long long)off[s + 1], s, (unsigned long long)off[s]);
        const uint64_t len = off[s + 1] - off[s];
        if (len == 0) return fail("hgibbs_set_gram: set %u is empty", s);
        if (len > SG_MMAX) return fail("hgibbs_set_gram: set %u has %llu markers, at most %u", s, (unsigned long long)len, SG_MMAX);
        for (uint64_t e = off[s]; e < off[s + 1]; ++e) {
            if (idx[e] >= M) return fail("hgibbs_set_gram: idx[%llu] = %u of set %u out of range (M = %u)", (unsigned long long)e, idx[e], s, M);
            if (seen[idx[e]] == s) return fail("hgibbs_set_gram: set %u lists marker %u twice", s, idx[e]);
            seen[idx[e]] = s;
        }
    }
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(w[i])) return fail("hgibbs_set_gram: w[%zu] = %g is not finite", i, w[i]);
        if (w[i] < 0.0) return fail("hgibbs_set_gram: w[%zu] = %g is negative", i, w[i]);
    }
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;
    std::vector<uint8_t> gran;
    if (missing_tiles(h, 16u, gran)) return 1;

    // what the call needs on the device, from the lists' lengths alone, before anything of their size is built on the host
    const uint64_t total = off[nsets] - off[0];
    uint64_t E = 0, njobs = 0, ntiles = 0;
    bool miss = false;
    for (uint32_t s = 0; s < nsets; ++s) {
        const uint64_t m = off[s + 1] - off[s], nt = (m + 15u) / 16u;
        E += m * m;
        njobs += nt * (nt + 1u) / 2u;
        ntiles += nt;
    }
    for (uint64_t e = off[0]; e < off[nsets] && !miss; ++e) miss = gran[idx[e] / 16u] != 0;
    const uint32_t nq = miss ? 4u : 1u;
    const uint32_t n_sub = (n + MD_SUBI - 1) / MD_SUBI;
    const size_t img_units = (size_t)n_sub * 8 * 64;
    const size_t bytes = E * (size_t)(2 * nq * 8 + 8 + (raw ? 24 : 0)) + total * (4 + 4 + 4 + 16) + njobs * sizeof(SgJob) + nsets * sizeof(SgSet) +
                         ntiles + img_units * sizeof(rl_v4i) + (size_t)n * 8 + 4096;
    if (need_device_memory(bytes, "hgibbs_set_gram: %u sets of %llu markers in all (%llu entries) need %.1f MiB", nsets, (unsigned long long)total,
                           (unsigned long long)E, bytes / 1048576.0))
        return 1;
    if (njobs >= (1ull << 31) || total >= (1ull << 31))
        return fail("hgibbs_set_gram: %llu markers in all and %llu tile pairs in one call, at most %llu of either", (unsigned long long)total,
                    (unsigned long long)njobs, (1ull << 31) - 1ull);

    // the sets, their tiles' flags and the jobs (all of one length: their order does not matter)
    std::vector<SgSet> sets(nsets);
    std::vector<SgJob> jobs;
    std::vector<uint8_t> tflag;
    std::vector<uint32_t> rowset(total), rowpos(total);
    jobs.reserve(njobs);
    tflag.reserve(ntiles);
    uint64_t base = 0;
    for (uint32_t s = 0; s < nsets; ++s) {
        const uint32_t m = (uint32_t)(off[s + 1] - off[s]), nt = (m + 15u) / 16u;
        sets[s] = SgSet{off[s] - off[0], base, (uint64_t)tflag.size(), m, 0u};
        for (uint32_t t = 0; t < nt; ++t) {
            uint8_t f = 0;
            for (uint32_t a = 16u * t; a < std::min(m, 16u * t + 16u); ++a) f |= gran[idx[off[s] + a] / 16u];
            tflag.push_back(f);
        }
        for (uint32_t a = 0; a < m; ++a) {
            rowset[off[s] - off[0] + a] = s;
            rowpos[off[s] - off[0] + a] = a;
        }
        for (uint32_t ta = 0; ta < nt; ++ta)
            for (uint32_t tb = ta; tb < nt; ++tb)
                jobs.push_back(SgJob{off[s] - off[0], base, m, ta, tb, (uint32_t)(tflag[sets[s].toff + ta] | tflag[sets[s].toff + tb])});
        base += (uint64_t)m * m;
    }

    DevBuf<double> dw, dout, draw;
    DevBuf<unsigned long long> maxbits, acc, psum;
    DevBuf<uint32_t> bad, didx, drowset, drowpos;
    DevBuf<int> scale;
    DevBuf<rl_v4i> img;
    DevBuf<uint8_t> dtflag;
    DevBuf<SgJob> djobs;
    DevBuf<SgSet> dsets;
    if (dw.alloc(n) || dout.alloc(E) || (raw && draw.alloc(E * 3))) return 1;
    if (maxbits.alloc(3) || acc.alloc(E * 2 * nq) || psum.alloc(total * 2) || bad.alloc(1) || scale.alloc(1)) return 1;
    if (didx.alloc(total) || drowset.alloc(total) || drowpos.alloc(total) || img.alloc(img_units)) return 1;
    if (dtflag.alloc(tflag.size()) || djobs.alloc(jobs.size()) || dsets.alloc(nsets)) return 1;
    HIP_TRY(hipMemcpyAsync(dw, w, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(didx, idx + off[0], total * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(drowset, rowset.data(), total * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(drowpos, rowpos.data(), total * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dtflag, tflag.data(), tflag.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(djobs, jobs.data(), jobs.size() * sizeof(SgJob), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dsets, sets.data(), (size_t)nsets * sizeof(SgSet), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(maxbits, 0, 3 * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(acc, 0, E * 2 * nq * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(psum, 0, total * 2 * sizeof(unsigned long long), h->stream));

    // device time from here to the rounded result: every kernel of the call, not the host copies around it
    double ms = 0.0;
    if (lap_begin(h)) return 1;
    if (digit_image(h, dw, 1, maxbits, bad, scale, img)) return 1; // (one vector, one tile)
    unsigned long long* ksum = maxbits + 1;
    // row ranges: enough workgroups for eight per compute unit (option sgram_split fixes the number), no range above SG_SUB_MAX slices
    const uint32_t nj = (uint32_t)jobs.size();
    uint32_t sub_per = 0;
    const uint32_t gy = split_ranges(n_sub, h->sgram_split ? (uint32_t)h->sgram_split : (8u * (uint32_t)h->num_cu + nj - 1u) / nj, SG_SUB_MAX, sub_per);
    if (miss)
        k_sgram<true><<<dim3(nj, gy), SG_WAVES * 64, 0, h->stream>>>(h->bed, h->stride, didx, djobs, sub_per, n_sub, img, acc, psum);
    else
        k_sgram<false><<<dim3(nj, gy), SG_WAVES * 64, 0, h->stream>>>(h->bed, h->stride, didx, djobs, sub_per, n_sub, img, acc, psum);
    HIP_TRY(hipGetLastError());
    k_sgram_final<<<(uint32_t)total, MD_TPB, 0, h->stream>>>(dsets, drowset, drowpos, didx, dtflag, acc, psum, ksum, scale, h->mave, h->mstd, miss ? 1 : 0, dout, draw);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, ms)) return 1;
    HIP_TRY(hipMemcpy(out, dout, E * sizeof(double), hipMemcpyDeviceToHost));
    if (raw) HIP_TRY(hipMemcpy(raw, draw, E * 3 * sizeof(double), hipMemcpyDeviceToHost));
    h->sgram_ms = ms;
    return 0;
}

extern "C" int hgibbs_last_set_gram_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_set_gram_ms: null argument");
    *ms = h->sgram_ms;
    return 0;
}
