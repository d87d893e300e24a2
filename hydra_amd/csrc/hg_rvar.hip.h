// Mean and variance over the rows of the scores of marker sets: for the BED loaded on a handle, S weight
// vectors and nsets lists of markers,
//
//     v_irs = sum_{j in set r} [code_ij != 3] (a_sj code_ij + o_sj),     mean_rs = (1/n) sum_i v_irs,   var_rs = sum_i (v - mean)^2 / (n - 1)
//
// without ever storing v: hg_score.hip.h's product with the blocks of 64 markers taken from the sets' index lists, and an epilogue
// that reduces the 256 rows of a workgroup to two numbers.
//
//   blocks   block k of a set is entries [64 k, 64 k + 64) of its list (the last one padded with nothing: zero digits against code 0).
//            Lane = entry: a lane loads the column idx[...] names, so a scattered set costs what a contiguous one does.
//   scale    one per (set, sample), from the weights of the set's markers: E = 52 - e, max < 2^e, exactly what hgibbs_score takes for
//            the same weights with everything outside the set zeroed -- so v is that call's value, bit for bit, and the error of an
//            entry is at most 3 |set| max_{j in set}|w_sj| 2^-52 however large the weights elsewhere are.
//   product  one workgroup owns (256 rows, one set, SP samples) and runs ALL the set's blocks: D[4][TILES] is complete in registers,
//            no atomics, no n x S accumulator.  LDS staging of the digit operands as in k_score (double buffer, one barrier a block).
//   epilogue the lane with digits 0..3 takes digits 4..6 from its partner sixteen lanes up, adds the set's constant sum_j q_o, rounds
//            once (round_halves), masks rows >= n_local; rv_tree sums v and v^2 over the rows in a fixed tree; the row blocks' parts
//            are added in ascending order by k_rvar_final.  Every floating-point sum has one order: results are bit-identical for
//            any chunking of S, any order or chunking of the sets, every score_sp and every rvar_kb_max.
//   large    a set of more than rvar_kb_max blocks (default SC_KB_MAX: the i32 headroom of D) goes through score_dev_run on weights
//            zeroed outside the set; k_rvar_dense reduces that n x SP buffer with the same rv_tree into the same parts.
#pragma once

namespace {

constexpr uint32_t RV_NOJ = 0xFFFFFFFFu; // no marker: a padded entry of a set's last block

// Sums of v and v^2 over a workgroup's 256 rows, in one fixed order.  Lane (c, g) of wave w holds the rows 64 w + 16 b + c, b = 0..3,
// of one sample per group g of sixteen lanes: first the lane's four, then the sixteen lanes of the group -- a DPP row -- as a butterfly
// on the VALU (dpp_f64: quad swaps, then the mirrors of eight and of sixteen lanes; both partners add the same two numbers, so every
// lane of the row ends with the same total), then rv_waves adds the four waves' sums from LDS as (w0 + w1) + (w2 + w3).
__device__ __forceinline__ void rv_tree(const double v[4], double& s1, double& s2)
{
    double a = (v[0] + v[1]) + (v[2] + v[3]);
    double q = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    a += dpp_f64<0xB1, 0xF>(a); // quad_perm [1,0,3,2]
    q += dpp_f64<0xB1, 0xF>(q);
    a += dpp_f64<0x4E, 0xF>(a); // quad_perm [2,3,0,1]
    q += dpp_f64<0x4E, 0xF>(q);
    a += dpp_f64<0x141, 0xF>(a); // row_half_mirror
    q += dpp_f64<0x141, 0xF>(q);
    a += dpp_f64<0x140, 0xF>(a); // row_mirror
    q += dpp_f64<0x140, 0xF>(q);
    s1 = a;
    s2 = q;
}

template <int NS>
__device__ __forceinline__ void rv_waves(const double (&red)[SC_WAVES][NS][2], uint32_t ls, double& s1, double& s2)
{
    s1 = (red[0][ls][0] + red[1][ls][0]) + (red[2][ls][0] + red[3][ls][0]);
    s2 = (red[0][ls][1] + red[1][ls][1]) + (red[2][ls][1] + red[3][ls][1]);
}

// Scale and constant of every (set, sample) pair, over chunks of at most RV_CHUNK entries of the sets' lists (chunk c: set cset[c],
// entries [cbeg[c], cend[c]) of idx; a long set has many) in two launches, everything order-free as in k_score_max / k_score_ksum:
// k_rvar_max   the largest |a|, |o| of the set's markers as an atomic max of the f64 bit patterns, and the flag for non-finite weights;
// k_rvar_ksum  E = sc_scale(max) -- hgibbs_score's for the masked weights -- and sum_{j in set} q_o in two halves by atomic integer
//              adds: ksum[2 p] the high halves, ksum[2 p + 1] the low ones.
constexpr uint32_t RV_CHUNK = 16384;

__global__ __launch_bounds__(SC_TPB) void k_rvar_max(const double* __restrict__ a, const double* __restrict__ o, uint32_t M, uint32_t S,
                                                      uint64_t nwork, const uint32_t* __restrict__ cset, const uint64_t* __restrict__ cbeg,
                                                      const uint64_t* __restrict__ cend, const uint32_t* __restrict__ idx,
                                                      unsigned long long* __restrict__ maxbits, uint32_t* __restrict__ bad)
{
    __shared__ double smax[SC_TPB];
    const uint32_t t = threadIdx.x;
    for (uint64_t w = blockIdx.x; w < nwork; w += gridDim.x) { // (uniform)
        const uint32_t c = (uint32_t)(w / S), s = (uint32_t)(w % S);
        const double* as = a + (size_t)s * M;
        const double* os = o + (size_t)s * M;
        double mx = 0.0;
        bool nonfinite = false;
        for (uint64_t e = cbeg[c] + t; e < cend[c]; e += SC_TPB) {
            const uint32_t j = idx[e];
            const double x = as[j], y = os[j];
            if (!isfinite(x) || !isfinite(y)) nonfinite = true;
            else mx = fmax(mx, fmax(fabs(x), fabs(y)));
        }
        if (nonfinite) atomicOr(bad, 1u);
        smax[t] = mx;
        __syncthreads();
        for (int h = SC_TPB / 2; h > 0; h >>= 1) {
            if (t < (uint32_t)h) smax[t] = fmax(smax[t], smax[t + h]);
            __syncthreads();
        }
        if (t == 0 && smax[0] > 0.0) atomicMax(maxbits + (size_t)cset[c] * S + s, (unsigned long long)__double_as_longlong(smax[0]));
        __syncthreads(); // (smax is written again by the next item)
    }
}

__global__ __launch_bounds__(SC_TPB) void k_rvar_ksum(const double* __restrict__ o, uint32_t M, uint32_t S, uint64_t nwork,
                                                       const uint32_t* __restrict__ cset, const uint64_t* __restrict__ cbeg,
                                                       const uint64_t* __restrict__ cend, const uint32_t* __restrict__ idx,
                                                       const unsigned long long* __restrict__ maxbits, int* __restrict__ scale,
                                                       unsigned long long* __restrict__ ksum)
{
    __shared__ long long shi[SC_TPB], slo[SC_TPB];
    const uint32_t t = threadIdx.x;
    for (uint64_t w = blockIdx.x; w < nwork; w += gridDim.x) { // (uniform)
        const uint32_t c = (uint32_t)(w / S), s = (uint32_t)(w % S);
        const size_t p = (size_t)cset[c] * S + s;
        const int E = sc_scale(maxbits[p]);
        const double* os = o + (size_t)s * M;
        long long hi = 0, lo = 0;
        for (uint64_t e = cbeg[c] + t; e < cend[c]; e += SC_TPB) {
            const double y = os[idx[e]];
            if (!isfinite(y)) continue;
            const long long q = sc_quant(y, E);
            hi += q >> 32;
            lo += q & 0xFFFFFFFFll;
        }
        shi[t] = hi;
        slo[t] = lo;
        __syncthreads();
        for (int h = SC_TPB / 2; h > 0; h >>= 1) {
            if (t < (uint32_t)h) {
                shi[t] += shi[t + h];
                slo[t] += slo[t + h];
            }
            __syncthreads();
        }
        if (t == 0) {
            scale[p] = E; // (every chunk of the set writes the same number)
            if (shi[0]) atomicAdd(ksum + 2 * p, (unsigned long long)shi[0]);
            if (slo[0]) atomicAdd(ksum + 2 * p + 1, (unsigned long long)slo[0]);
        }
        __syncthreads(); // (shi, slo are written again by the next item)
    }
}

// The A operands of one pass, k_score_digits with the block's markers taken from its set's list: block gb is block gb - blk0[set] of
// set bset[gb].  Same layout: [block][tile][lane] 16 bytes, dword q, byte i = entry 16 g + 4 i + q of the block.
__global__ __launch_bounds__(64) void k_rvar_digits(const double* __restrict__ a, const double* __restrict__ o, uint32_t M, uint32_t S,
                                                    uint32_t s0, int tiles, const uint32_t* __restrict__ bset, const uint32_t* __restrict__ blk0,
                                                    const uint64_t* __restrict__ off, const uint32_t* __restrict__ idx,
                                                    const int* __restrict__ scale, const int32_t* __restrict__ mslot,
                                                    rl_v4i* __restrict__ wdig, rl_v4i* __restrict__ mdig)
{
    const uint32_t gb = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const uint32_t r = lane & 15u, g = lane >> 4, d = r & 7u;
    const uint32_t s = s0 + 2u * t + (r >> 3);
    const uint32_t set = bset[gb];
    const uint64_t e0 = off[set] + (uint64_t)(gb - blk0[set]) * 64u, e1 = off[set + 1];
    const int ms = mslot[gb];
    rl_v4i w = {0, 0, 0, 0}, m = {0, 0, 0, 0};
    if (s < S && d < 7u) {
        const int E = scale[(size_t)set * S + s];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t wq = 0, mq = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint64_t e = e0 + 16u * g + 4u * (uint32_t)i + (uint32_t)q;
                if (e >= e1) continue;
                const uint32_t j = idx[e];
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
    wdig[((size_t)gb * tiles + t) * 64u + lane] = w;
    if (ms >= 0) mdig[((size_t)ms * tiles + t) * 64u + lane] = m;
}

// The product and its epilogue.  Workgroup wg of the flattened grid: set order[wg / gx], rows [256 rb, 256 rb + 256), rb = wg % gx (the
// workgroups of a set are neighbours: they share its operands); SP samples from s0.  part[((set gx + rb) SP + ls) 2 + 0 / 1] = sums
// of v and of v^2 over the workgroup's rows for sample s0 + ls.
template <int SP>
__global__ __launch_bounds__(SC_IND) void k_rvar(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t n_local, uint32_t gx, uint64_t nwg,
                                                 const uint32_t* __restrict__ order, const uint64_t* __restrict__ off,
                                                 const uint32_t* __restrict__ blk0, const uint32_t* __restrict__ idx,
                                                 const rl_v4i* __restrict__ wdig, const rl_v4i* __restrict__ mdig,
                                                 const int32_t* __restrict__ mslot, const int* __restrict__ scale,
                                                 const unsigned long long* __restrict__ ksum, uint32_t S, uint32_t s0, double* __restrict__ part)
{
    constexpr int TILES = SP / 2;
    constexpr int NOP = TILES * 64;                          // A operands (16 bytes) per block and kind
    constexpr int NPT = (NOP + SC_IND - 1) / SC_IND;         // of them per thread when staging
    __shared__ rl_v4i sop[2][2][NOP];                        // [buffer][product: codes, missing-call indicator][tile x lane]
    __shared__ double red[SC_WAVES][SP][2];
    const uint64_t wg = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (wg >= nwg) return; // (uniform)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t set = order[wg / gx], rb = (uint32_t)(wg % gx);
    const uint64_t e0 = off[set], len = off[set + 1] - e0;
    const uint32_t nblk = (uint32_t)((len + 63u) / 64u), gb0 = blk0[set];
    if (!nblk) return; // (uniform; the host launches no workgroup for an empty set: k_rvar_final writes its zeros)
    const uint64_t dw0 = (uint64_t)rb * (SC_IND / 16) + wave * 4u; // first dword of this wave's individuals in a column

    auto load_j = [&](uint32_t k) { // the column of this lane's entry of block k
        const uint64_t e = (uint64_t)k * 64u + lane;
        return k < nblk && e < len ? idx[e0 + e] : RV_NOJ;
    };
    auto load_codes = [&](uint32_t j) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u); // (no marker: code 0 against zero digits)
        if (j != RV_NOJ) v = *reinterpret_cast<const uint4*>(bed + (uint64_t)j * stride + dw0 * 4u);
        return v;
    };
    rl_v4i rw[NPT], rm[NPT];
    auto load_ops = [&](uint32_t k) {
        const int ms = mslot[gb0 + k];
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            const uint32_t at = tid + (uint32_t)(q * SC_IND);
            if (at < (uint32_t)NOP) {
                rw[q] = wdig[(size_t)(gb0 + k) * NOP + at];
                if (ms >= 0) rm[q] = mdig[(size_t)ms * NOP + at];
            }
        }
        return ms;
    };
    auto store_ops = [&](int buf, int ms) {
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            const uint32_t at = tid + (uint32_t)(q * SC_IND);
            if (at < (uint32_t)NOP) {
                sop[buf][0][at] = rw[q];
                if (ms >= 0) sop[buf][1][at] = rm[q];
            }
        }
    };

    // the constants of the pass's samples for the epilogue: the addresses are the same in every lane, so they come through the scalar
    // cache into scalar registers now and cost the loop nothing (a sample past S takes the last one's: it is masked below).  Sixteen
    // samples' constants are more scalar registers than there are: SP = 16 reads them in the epilogue, tile by tile
    constexpr bool PRE = SP <= 8;
    long long klo[PRE ? SP : 1], khi[PRE ? SP : 1];
    int Es[PRE ? SP : 1];
    if constexpr (PRE) {
#pragma unroll
        for (int ls = 0; ls < SP; ++ls) {
            const size_t p = (size_t)set * S + min(s0 + (uint32_t)ls, S - 1u);
            khi[ls] = (long long)ksum[2 * p];
            klo[ls] = (long long)ksum[2 * p + 1];
            Es[ls] = scale[p];
        }
    }

    rl_v4i D[4][TILES];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int t = 0; t < TILES; ++t) D[b][t] = rl_v4i{0, 0, 0, 0};

    // the list is read two blocks ahead of the product and the codes one block ahead: the load of a column waits for its index
    uint4 cur = load_codes(load_j(0u));
    uint32_t j_nxt = load_j(1u);
    int ms_cur = load_ops(0u);
    store_ops(0, ms_cur);
    __syncthreads();
    const uint32_t m16 = lane & 15u;
    for (uint32_t k = 0; k < nblk; ++k) {
        const int buf = (int)(k & 1u);
        const bool more = k + 1u < nblk;
        uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
        int ms_nxt = -1;
        if (more) {
            nxt = load_codes(j_nxt);
            ms_nxt = load_ops(k + 1u);
        }
        j_nxt = load_j(k + 2u);
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
        // the sums stay in accumulation registers over the back edge (without this the compiler carries them in vector registers and
        // copies all of them to the MFMAs' registers and back in every block)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int t = 0; t < TILES; ++t) asm volatile("" : "+a"(D[b][t]));
    }

    // lane (c, g), tile t: sample s0 + 2 t + (g >> 1), digits 4 (g & 1) .. +3 of row c of each block of sixteen.  The even g puts its
    // four digits together (the low 64-bit sum), takes the odd g's (units of 2^32) from sixteen lanes up, adds the set's constant and
    // rounds once: k_score's epilogue and k_score_final in one lane.
    const uint32_t c = lane & 15u, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const uint32_t ls = 2u * (uint32_t)t + (g >> 1), s = s0 + ls;
        const bool live = s < S && !(g & 1u), odd = (g >> 1) != 0u;
        long long kl, kh;
        int E;
        if constexpr (PRE) {
            kl = odd ? klo[2 * t + 1] : klo[2 * t];
            kh = odd ? khi[2 * t + 1] : khi[2 * t];
            E = odd ? Es[2 * t + 1] : Es[2 * t];
        } else {
            const size_t p = (size_t)set * S + min(s, S - 1u);
            kh = (long long)ksum[2 * p];
            kl = (long long)ksum[2 * p + 1];
            E = scale[p];
        }
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t i = rb * SC_IND + wave * 64u + 16u * (uint32_t)b + c;
            const long long x = (long long)D[b][t][0] + ((long long)D[b][t][1] << 8) + ((long long)D[b][t][2] << 16) + ((long long)D[b][t][3] << 24);
            const long long up = __shfl_down(x, 16);
            v[b] = live && i < n_local ? round_halves(up + kh, x + kl, E) : 0.0;
        }
        double s1, s2;
        rv_tree(v, s1, s2);
        if (c == 0u && !(g & 1u)) {
            red[wave][ls][0] = s1;
            red[wave][ls][1] = s2;
        }
        __builtin_amdgcn_sched_barrier(0); // one tile at a time: the tiles side by side would take the registers of a third workgroup
    }
    __syncthreads();
    if (tid < (uint32_t)SP && s0 + tid < S) {
        double s1, s2;
        rv_waves<SP>(red, tid, s1, s2);
        double* out = part + (((size_t)set * gx + rb) * SP + tid) * 2u;
        out[0] = s1;
        out[1] = s2;
    }
}

// The same parts from scores that exist: v (n_local x ns, hgibbs_score's layout) of ONE set, workgroup = row block.  Group g of sixteen
// lanes takes the samples g, g + 4, ...; the rows of a lane and the order of every sum are k_rvar's (rv_tree, rv_waves).
__global__ __launch_bounds__(SC_IND) void k_rvar_dense(const double* __restrict__ v_all, uint32_t ns, uint32_t n_local, uint32_t set, uint32_t gx,
                                                       uint32_t sp, double* __restrict__ part)
{
    __shared__ double red[SC_WAVES][16][2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, rb = blockIdx.x;
    const uint32_t c = lane & 15u, g = lane >> 4;
    for (uint32_t l0 = 0; l0 < ns; l0 += 4u) { // (uniform)
        const uint32_t ls = l0 + g;
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t i = rb * SC_IND + wave * 64u + 16u * (uint32_t)b + c;
            v[b] = ls < ns && i < n_local ? v_all[(size_t)i * ns + ls] : 0.0;
        }
        double s1, s2;
        rv_tree(v, s1, s2);
        if (c == 0u && ls < ns) {
            red[wave][ls][0] = s1;
            red[wave][ls][1] = s2;
        }
    }
    __syncthreads();
    if (tid < ns) {
        double s1, s2;
        rv_waves<16>(red, tid, s1, s2);
        double* out = part + (((size_t)set * gx + rb) * sp + tid) * 2u;
        out[0] = s1;
        out[1] = s2;
    }
}

// The weights of `ns` samples from s0 on the markers of one set, into buffers the caller has zeroed: what hgibbs_score is given for a
// set that takes its pipeline
__global__ __launch_bounds__(SC_TPB) void k_rvar_mask(const double* __restrict__ a, const double* __restrict__ o, uint32_t M, uint32_t s0,
                                                       const uint32_t* __restrict__ idx, uint64_t e0, uint64_t len, double* __restrict__ ma,
                                                       double* __restrict__ mo)
{
    const uint32_t ls = blockIdx.y;
    for (uint64_t e = (uint64_t)blockIdx.x * SC_TPB + threadIdx.x; e < len; e += (uint64_t)gridDim.x * SC_TPB) {
        const uint32_t j = idx[e0 + e];
        ma[(size_t)ls * M + j] = a[(size_t)(s0 + ls) * M + j];
        mo[(size_t)ls * M + j] = o[(size_t)(s0 + ls) * M + j];
    }
}

// mean and var of the pairs (set, s0 + ls), ls < ns: the row blocks' parts added in ascending order; an empty set has no parts and gets 0, 0
__global__ __launch_bounds__(SC_TPB) void k_rvar_final(const double* __restrict__ part, const uint64_t* __restrict__ off, uint32_t nsets, uint32_t gx, uint32_t sp, uint32_t ns,
                                                        uint32_t s0, uint32_t S, uint32_t n_local, double* __restrict__ mean, double* __restrict__ var)
{
    const uint64_t k = (uint64_t)blockIdx.x * SC_TPB + threadIdx.x;
    if (k >= (uint64_t)nsets * ns) return;
    const uint32_t set = (uint32_t)(k / ns), ls = (uint32_t)(k % ns);
    double s1 = 0.0, s2 = 0.0;
    for (uint32_t rb = 0; rb < (off[set + 1] > off[set] ? gx : 0u); ++rb) {
        const double* in = part + (((size_t)set * gx + rb) * sp + ls) * 2u;
        s1 += in[0];
        s2 += in[1];
    }
    const double n = (double)n_local, m = s1 / n;
    mean[(size_t)set * S + s0 + ls] = m;
    var[(size_t)set * S + s0 + ls] = fmax(0.0, (s2 - s1 * m) / (n - 1.0));
}

} // namespace

template <int SP>
static void rvar_launch(hgibbs_ctx* h, dim3 grid, uint32_t gx, uint64_t nwg, const uint32_t* order, const uint64_t* off, const uint32_t* blk0,
                        const uint32_t* idx, const rl_v4i* wdig, const rl_v4i* mdig, const int32_t* mslot, const int* scale,
                        const unsigned long long* ksum, uint32_t S, uint32_t s0, double* part)
{
    k_rvar<SP><<<grid, SC_IND, 0, h->stream>>>(h->bed, h->stride, h->n_local, gx, nwg, order, off, blk0, idx, wdig, mdig, mslot, scale, ksum, S, s0, part);
}

extern "C" int hgibbs_region_var(hgibbs_t h, int S, const double* a, const double* o, uint32_t nsets, const uint64_t* off, const uint32_t* idx,
                                 double* mean, double* var)
{
    if (op_guard(h, "hgibbs_region_var", "the sums over the rows are taken in one fixed order on one device")) return 1;
    if (S <= 0) return fail("hgibbs_region_var: S = %d, needs at least one weight vector", S);
    if (nsets == 0) return fail("hgibbs_region_var: nsets = 0, needs at least one marker set");
    if (!a || !o || !off || !mean) return fail("hgibbs_region_var: null argument");
    if (h->n_local < 2) return fail("hgibbs_region_var: n_local = %u, a variance needs at least two rows", h->n_local);
    const uint32_t M = h->M, n = h->n_local;
    const uint64_t total = off[nsets];
    if (off[0] != 0) return fail("hgibbs_region_var: off[0] = %llu, the first set starts at 0", (unsigned long long)off[0]);
    if (total && !idx) return fail("hgibbs_region_var: null argument");
    for (uint32_t r = 0; r < nsets; ++r) {
        if (off[r + 1] < off[r]) return fail("hgibbs_region_var: off[%u] > off[%u]: the offsets must not decrease", r, r + 1);
        for (uint64_t e = off[r]; e < off[r + 1]; ++e) {
            if (idx[e] >= M) return fail("hgibbs_region_var: set %u names marker %u, the handle has %u", r, idx[e], M);
            if (e > off[r] && idx[e] <= idx[e - 1])
                return fail("hgibbs_region_var: set %u: marker %u after %u, the indices of a set must be strictly increasing", r, idx[e], idx[e - 1]);
        }
    }
    HIP_TRY(hipSetDevice(h->device));

    // the sets' blocks: a set of at most `cap` blocks gets its range of the block table, a longer one takes the score's pipeline
    const uint32_t cap = h->rvar_kb_max ? (uint32_t)h->rvar_kb_max : SC_KB_MAX;
    const uint32_t gx = h->n_pad / SC_IND;
    const int sp = score_sp_for(h, S), tiles = sp / 2;
    {
        // what one call takes: the block table is indexed in 24 bits, and the product's workgroups go in one launch of at most
        // 65 535 x 2^20 of them
        uint64_t nb_all = 0, nsmall = 0;
        for (uint32_t r = 0; r < nsets; ++r) {
            const uint64_t nb = (off[r + 1] - off[r] + 63u) / 64u;
            if (nb && nb <= cap) {
                nb_all += nb;
                ++nsmall;
            }
        }
        if (nb_all >= (1ull << 24))
            return fail("hgibbs_region_var: the sets make %llu blocks of 64 markers, at most 2^24 - 1 a call: pass them in several calls", (unsigned long long)nb_all);
        if (nsmall * gx > 65535ull << 20)
            return fail("hgibbs_region_var: %llu sets on %u blocks of 256 rows are more workgroups than one launch takes (65535 x 2^20): pass the sets in several calls",
                        (unsigned long long)nsmall, gx);
    }
    if (compute_stats(h)) return 1;
    std::vector<uint8_t> miss;
    if (missing_tiles(h, 1u, miss)) return 1; // (per marker)
    std::vector<uint32_t> blk0(nsets, 0u), small, large, bset;
    std::vector<int32_t> mslot;
    uint32_t nm = 0;
    for (uint32_t r = 0; r < nsets; ++r) {
        const uint64_t len = off[r + 1] - off[r], nb = (len + 63u) / 64u;
        if (nb > cap) {
            large.push_back(r);
            continue;
        }
        if (nb) small.push_back(r); // (an empty set gets no workgroup)
        blk0[r] = (uint32_t)bset.size();
        for (uint64_t k = 0; k < nb; ++k) {
            bool any = false;
            for (uint64_t e = off[r] + 64u * k; e < std::min(off[r + 1], off[r] + 64u * k + 64u); ++e) any = any || miss[idx[e]];
            bset.push_back(r);
            mslot.push_back(any ? (int32_t)nm++ : -1);
        }
    }
    // the chunks of the lists the scales are taken over; an empty set has none (its scale and constant stay 0)
    std::vector<uint32_t> cset;
    std::vector<uint64_t> cbeg, cend;
    for (uint32_t r = 0; r < nsets; ++r)
        for (uint64_t e = off[r]; e < off[r + 1]; e += RV_CHUNK) {
            cset.push_back(r);
            cbeg.push_back(e);
            cend.push_back(std::min<uint64_t>(off[r + 1], e + RV_CHUNK));
        }
    const size_t nchunks = cset.size();
    // the longest sets first: their workgroups run longest
    std::stable_sort(small.begin(), small.end(), [&](uint32_t x, uint32_t y) { return off[x + 1] - off[x] > off[y + 1] - off[y]; });
    const size_t nblk = bset.size(), npairs = (size_t)nsets * S, SM = (size_t)S * M;
    const int ns_large = std::min(S, sp);
    const size_t bytes = 2 * SM * sizeof(double) + (size_t)total * 4 + (nblk + nm) * (size_t)tiles * 64 * sizeof(rl_v4i) +
                         (size_t)nsets * gx * sp * 2 * sizeof(double) + npairs * (4 + 24 + 16) + (size_t)nsets * 20 + nblk * 8 + nchunks * 20 +
                         (large.empty() ? 0 : score_ws_bytes(h, ns_large) + (size_t)ns_large * (2 * (size_t)M + n) * sizeof(double));
    if (need_device_memory(bytes, "hgibbs_region_var: %u sets of %llu markers in all and %d weight vectors need %.1f MiB of device memory", nsets,
                           (unsigned long long)total, S, bytes / 1048576.0))
        return 1;

    DevBuf<double> da, dov, dpart, dmean, dvar, ma, mo, dv;
    DevBuf<uint64_t> doff, dcbeg, dcend;
    DevBuf<uint32_t> didx, dblk0, dbset, dorder, bad, dcset;
    DevBuf<int32_t> dmslot;
    DevBuf<int> scale;
    DevBuf<unsigned long long> ksum, allmax;
    DevBuf<rl_v4i> wdig, mdig;
    ScoreWs ws;
    if (da.alloc(SM) || dov.alloc(SM) || dpart.alloc((size_t)nsets * gx * sp * 2) || dmean.alloc(npairs) || dvar.alloc(npairs)) return 1;
    if (doff.alloc((size_t)nsets + 1) || didx.alloc(std::max<uint64_t>(total, 1)) || dblk0.alloc(nsets) || bad.alloc(1)) return 1;
    if (dbset.alloc(std::max<size_t>(nblk, 1)) || dmslot.alloc(std::max<size_t>(nblk, 1)) || dorder.alloc(std::max<size_t>(small.size(), 1))) return 1;
    if (scale.alloc(npairs) || ksum.alloc(npairs * 3) || allmax.alloc((size_t)S)) return 1; // (ksum: the two halves, then the maxima)
    if (dcset.alloc(std::max<size_t>(nchunks, 1)) || dcbeg.alloc(std::max<size_t>(nchunks, 1)) || dcend.alloc(std::max<size_t>(nchunks, 1))) return 1;
    if (nblk && wdig.alloc(nblk * tiles * 64)) return 1;
    if (nm && mdig.alloc((size_t)nm * tiles * 64)) return 1;
    if (!large.empty()) {
        if (score_ws_create(h, ws, ns_large)) return 1;
        if (ma.alloc((size_t)ns_large * M) || mo.alloc((size_t)ns_large * M) || dv.alloc((size_t)n * ns_large)) return 1;
    }
    HIP_TRY(hipMemcpyAsync(da, a, SM * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dov, o, SM * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(doff, off, ((size_t)nsets + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    if (total) HIP_TRY(hipMemcpyAsync(didx, idx, (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dblk0, blk0.data(), (size_t)nsets * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (nblk) {
        HIP_TRY(hipMemcpyAsync(dbset, bset.data(), nblk * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dmslot, mslot.data(), nblk * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    }
    if (!small.empty()) HIP_TRY(hipMemcpyAsync(dorder, small.data(), small.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (nchunks) {
        HIP_TRY(hipMemcpyAsync(dcset, cset.data(), nchunks * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dcbeg, cbeg.data(), nchunks * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dcend, cend.data(), nchunks * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(scale, 0, npairs * sizeof(int), h->stream));
    HIP_TRY(hipMemsetAsync(ksum, 0, npairs * 3 * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(allmax, 0, (size_t)S * sizeof(unsigned long long), h->stream));

    // device time from here to mean and var: every kernel of the call, not the host copies
    double ms = 0.0;
    if (lap_begin(h)) return 1;
    {
        // a weight that is not finite is refused wherever it stands, in a set or not: k_score_max's flag over all the markers
        const uint32_t per = std::max<uint32_t>(1u, std::min<uint32_t>((M + 2047u) / 2048u, (2048u + (uint32_t)S - 1u) / (uint32_t)S));
        k_score_max<<<dim3(S, per), SC_TPB, 0, h->stream>>>(da, dov, M, allmax, bad);
        HIP_TRY(hipGetLastError());
        const uint64_t nwork = (uint64_t)nchunks * S;
        if (nwork) {
            unsigned long long* setmax = ksum + npairs * 2;
            const uint32_t gw = (uint32_t)std::min<uint64_t>(nwork, 1u << 20);
            k_rvar_max<<<gw, SC_TPB, 0, h->stream>>>(da, dov, M, (uint32_t)S, nwork, dcset, dcbeg, dcend, didx, setmax, bad);
            HIP_TRY(hipGetLastError());
            k_rvar_ksum<<<gw, SC_TPB, 0, h->stream>>>(dov, M, (uint32_t)S, nwork, dcset, dcbeg, dcend, didx, setmax, scale, ksum);
            HIP_TRY(hipGetLastError());
        }
    }
    const uint64_t nwg = (uint64_t)gx * small.size();
    const uint32_t gridx = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(nwg, 1), 1u << 20);
    const dim3 grid(gridx, (uint32_t)((nwg + gridx - 1) / gridx));
    for (uint32_t s0 = 0; s0 < (uint32_t)S; s0 += (uint32_t)sp) {
        const uint32_t ns = std::min<uint32_t>((uint32_t)sp, (uint32_t)S - s0);
        if (nblk) {
            k_rvar_digits<<<dim3((uint32_t)nblk, tiles), 64, 0, h->stream>>>(da, dov, M, (uint32_t)S, s0, tiles, dbset, dblk0, doff, didx, scale, dmslot, wdig, mdig);
            HIP_TRY(hipGetLastError());
        }
        if (nwg) {
            switch (sp) {
            case 2: rvar_launch<2>(h, grid, gx, nwg, dorder, doff, dblk0, didx, wdig, mdig, dmslot, scale, ksum, (uint32_t)S, s0, dpart); break;
            case 4: rvar_launch<4>(h, grid, gx, nwg, dorder, doff, dblk0, didx, wdig, mdig, dmslot, scale, ksum, (uint32_t)S, s0, dpart); break;
            case 8: rvar_launch<8>(h, grid, gx, nwg, dorder, doff, dblk0, didx, wdig, mdig, dmslot, scale, ksum, (uint32_t)S, s0, dpart); break;
            default: rvar_launch<16>(h, grid, gx, nwg, dorder, doff, dblk0, didx, wdig, mdig, dmslot, scale, ksum, (uint32_t)S, s0, dpart); break;
            }
            HIP_TRY(hipGetLastError());
        }
        for (const uint32_t r : large) {
            const uint64_t len = off[r + 1] - off[r];
            HIP_TRY(hipMemsetAsync(ma, 0, (size_t)ns * M * sizeof(double), h->stream));
            HIP_TRY(hipMemsetAsync(mo, 0, (size_t)ns * M * sizeof(double), h->stream));
            k_rvar_mask<<<dim3((uint32_t)std::min<uint64_t>((len + SC_TPB - 1) / SC_TPB, 4096), ns), SC_TPB, 0, h->stream>>>(da, dov, M, s0, didx, off[r], len, ma, mo);
            HIP_TRY(hipGetLastError());
            if (score_dev_clear(h, ws, (int)ns, false)) return 1;
            if (score_dev_run(h, ws, (int)ns, ma, mo, dv)) return 1;
            k_rvar_dense<<<gx, SC_IND, 0, h->stream>>>(dv, ns, n, r, gx, (uint32_t)sp, dpart);
            HIP_TRY(hipGetLastError());
        }
        k_rvar_final<<<(uint32_t)(((size_t)nsets * ns + SC_TPB - 1) / SC_TPB), SC_TPB, 0, h->stream>>>(dpart, doff, nsets, gx, (uint32_t)sp, ns, s0, (uint32_t)S, n, dmean, dvar);
        HIP_TRY(hipGetLastError());
    }
    if (lap_end(h, ms)) return 1;
    uint32_t isbad = 0;
    HIP_TRY(hipMemcpy(&isbad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (isbad) return fail("hgibbs_region_var: a weight (a or o) is not finite"); // (mean and var untouched)
    HIP_TRY(hipMemcpy(mean, dmean, npairs * sizeof(double), hipMemcpyDeviceToHost));
    if (var) HIP_TRY(hipMemcpy(var, dvar, npairs * sizeof(double), hipMemcpyDeviceToHost));
    h->rvar_ms = ms;
    return 0;
}

extern "C" int hgibbs_last_region_var_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_region_var_ms: null argument");
    *ms = h->rvar_ms;
    return 0;
}
