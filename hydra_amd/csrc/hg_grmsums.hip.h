// Row sums of the genomic relationship matrix: per row a of the n_local loaded rows, over its partners b != a with
// NSNP_ab > 0 and A_ab = S_ab / NSNP_ab (S and NSNP exactly hgibbs_grm's, one IEEE division),
//
//     AY[a][p] = sum_b fx(A_ab Y[p][b])    A1[a] = sum_b fx(A_ab)    A2[a] = sum_b fx(A_ab A_ab)    partners[a] = #b
//
// with fx(t) = llrint(t 2^F), F = 58 - k, n_local <= 2^k.  What Haseman-Elston regression (hg_hefit.cpp) needs of the matrix, without
// the matrix ever leaving the device.
//
//   products  grm_pieces (hg_grm.hip.h), unchanged: k_grm and k_grm_final leave a piece's packed S and NSNP on the device.
//   reduce    k_grs_reduce: a workgroup takes GS_T = 64 rows x 64 columns of the piece's packed triangle, the tiles on multiples of 64 of
//             the matrix (so a tile is on the diagonal or wholly below it) and cut to the piece's rows.  A wave takes a row at a time,
//             lane = column b: 64 lanes read 512 contiguous bytes of S and 256 of NSNP, form A and the P + 3 terms; b > a is masked,
//             b = a writes diag.
//             row direction     row a takes fx(A_ab Y_pb): one integer sum across the wave per term, kept in LDS (a row belongs to one
//                               wave: a plain store).
//             column direction  row b takes fx(A_ab Y_pa), Y_pa uniform over the wave: summed in the lane's registers over the wave's
//                               sixteen rows, then the four waves' sums meet in LDS.
//             flush             once a tile: thread i adds word i of the tile's 64 x (P + 3) row sums and word i of its column sums to
//                               the n_local x (P + 3) accumulator of 64-bit integers, where the tile's rows and the tile's columns are
//                               one contiguous block each (consecutive threads, consecutive words); zero words are skipped.  Everything
//                               that shares a destination inside a tile is summed on chip first: a word of the accumulator takes at most
//                               two atomic adds a tile, n_local / 64 tiles a row.
//             The columns of the accumulator: A1, A2, partners, then AY[0 .. P).
//   range     every term must satisfy |t| < 16; then |fx| <= 2^(62 - k) and a row's sum of fewer than 2^k terms stays below 2^62.  The
//             kernel keeps the largest |t| it met (an unsigned 64-bit max of the f64 bits: non-negative doubles order as integers); the
//             host refuses the call after the run when that is >= 16, before any output is written.
//   exact     every sum is a sum of the per-pair integers fx, added with integer adds in registers, LDS and global memory: the results
//             do not depend on grm_split, grm_piece, tiles, launch order or repeats.  k_grs_final converts once ((double)sum 2^-F).
//
// Registers (the metadata notes of the gfx950 code object; no scratch, no spills): DESIGN.md section 22.
#pragma once

namespace {

constexpr int GS_T = 64;                 // rows and columns of a tile: one column per lane
constexpr int GS_WAVES = 4;
constexpr int GS_PMAX = 8;               // vectors at most
constexpr int GS_QMAX = GS_PMAX + 3;     // columns of the accumulator at most: A1, A2, partners, AY[p]

struct GrsArgs {
    const double* S;        // the piece's packed triangle
    const int32_t* nsnp;
    const double* Y;        // [P][n]
    uint32_t n, P;
    uint32_t p0, pc;        // rows of the piece
    uint32_t rt0;           // the piece's first row tile: p0 / GS_T
    unsigned long long off0; // packed offset of row p0
    int F;
    unsigned long long* acc; // [n][P + 3]
    double* diag;           // [n]
    unsigned long long* tmax; // the bits of the largest |t|
};

__device__ __forceinline__ long long gs_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ unsigned long long gs_abs_bits(double t) { return (unsigned long long)__double_as_longlong(fabs(t)); }

// Workgroup (x, y): columns 64 x .. + 63 of rows 64 (rt0 + y) .. + 63, cut to the piece [p0, p0 + pc); nothing above the diagonal
__global__ __launch_bounds__(GS_WAVES * 64) void k_grs_reduce(GrsArgs g)
{
    __shared__ unsigned long long s_row[GS_T * GS_QMAX];            // [row][q]
    __shared__ unsigned long long s_col[GS_WAVES * GS_T * GS_QMAX]; // [wave][column][q]
    __shared__ unsigned long long s_max[GS_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t ct = blockIdx.x, rt = g.rt0 + blockIdx.y;
    if (ct > rt) return; // (uniform: before any barrier)
    const uint32_t P = g.P, Q = P + 3u, n = g.n;
    for (uint32_t i = tid; i < GS_T * Q; i += GS_WAVES * 64) s_row[i] = 0ull;
    __syncthreads();

    const uint32_t b = GS_T * ct + lane;
    const double scale = (double)(1ull << g.F);
    double yb[GS_PMAX];
#pragma unroll
    for (int p = 0; p < GS_PMAX; ++p) yb[p] = ((uint32_t)p < P && b < n) ? g.Y[(size_t)p * n + b] : 0.0;
    long long col[GS_QMAX];
#pragma unroll
    for (int q = 0; q < GS_QMAX; ++q) col[q] = 0;
    unsigned long long mx = 0ull;

    for (uint32_t r = wave; r < (uint32_t)GS_T; r += GS_WAVES) {
        const uint32_t a = GS_T * rt + r;
        if (a < g.p0 || a - g.p0 >= g.pc) continue; // (uniform) a row of the tile outside the piece; inside it, a < n
        double A = 0.0;
        bool on = false;
        if (b <= a) { // (b <= a < n)
            const unsigned long long at = (unsigned long long)a * (a + 1ull) / 2ull - g.off0 + b;
            const double s = g.S[at];
            const int32_t m = g.nsnp[at];
            if (b == a) {
                if (g.diag) g.diag[a] = m > 0 ? __ddiv_rn(s, (double)m) : __builtin_nan("");
            } else if (m > 0) {
                A = __ddiv_rn(s, (double)m);
                on = true;
            }
        }
        if (__ballot(on) == 0ull) continue; // (uniform)
        long long t[GS_QMAX];
        {
            const double A2 = __dmul_rn(A, A);
            const long long f1 = llrint(__dmul_rn(A, scale)), f2 = llrint(__dmul_rn(A2, scale));
            t[0] = f1; // (A = 0 where the pair is off: every term is 0 there)
            t[1] = f2;
            t[2] = on ? 1ll : 0ll;
            mx = max(mx, max(gs_abs_bits(A), gs_abs_bits(A2)));
        }
#pragma unroll
        for (int p = 0; p < GS_PMAX; ++p) {
            t[3 + p] = 0;
            if ((uint32_t)p < P) { // (uniform)
                const double ya = g.Y[(size_t)p * n + a];
                const double tb = __dmul_rn(A, yb[p]), ta = __dmul_rn(A, ya);
                t[3 + p] = llrint(__dmul_rn(tb, scale));
                col[3 + p] += llrint(__dmul_rn(ta, scale));
                mx = max(mx, max(gs_abs_bits(tb), gs_abs_bits(ta)));
            }
        }
        col[0] += t[0];
        col[1] += t[1];
        col[2] += t[2];
#pragma unroll
        for (int q = 0; q < GS_QMAX; ++q) {
            if ((uint32_t)q < Q) { // (uniform)
                const long long s = gs_wave_sum(t[q]);
                if (lane == 0u) s_row[r * Q + (uint32_t)q] = (unsigned long long)s;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < GS_QMAX; ++q)
        if ((uint32_t)q < Q) s_col[(wave * GS_T + lane) * Q + (uint32_t)q] = (unsigned long long)col[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned long long)__shfl_xor(mx, o));
    if (lane == 0u) s_max[wave] = mx;
    __syncthreads();

    // one flush a tile: the tile's rows and the tile's columns are one contiguous block of the accumulator each
    for (uint32_t i = tid; i < GS_T * Q; i += GS_WAVES * 64) {
        const uint32_t x = i / Q;
        const unsigned long long vr = s_row[i];
        if (vr && GS_T * rt + x < n)
            __hip_atomic_fetch_add(g.acc + (size_t)GS_T * rt * Q + i, vr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long vc = 0ull;
#pragma unroll
        for (int w = 0; w < GS_WAVES; ++w) vc += s_col[(size_t)w * GS_T * Q + i];
        if (vc && GS_T * ct + x < n)
            __hip_atomic_fetch_add(g.acc + (size_t)GS_T * ct * Q + i, vc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0u) {
        unsigned long long m = s_max[0];
#pragma unroll
        for (int w = 1; w < GS_WAVES; ++w) m = max(m, s_max[w]);
        if (m) atomicMax(g.tmax, m);
    }
}

// Thread (a, q): one conversion, (double)sum 2^-F; the partner count as it is
__global__ __launch_bounds__(256) void k_grs_final(const unsigned long long* __restrict__ acc, uint32_t n, uint32_t P, int F, double* __restrict__ ay,
                                                    double* __restrict__ a1, double* __restrict__ a2, uint32_t* __restrict__ partners)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t Q = P + 3u;
    if (i >= (uint64_t)n * Q) return;
    const uint32_t a = (uint32_t)(i / Q), q = (uint32_t)(i % Q);
    const long long s = (long long)acc[i];
    const double v = ldexp((double)s, -F);
    if (q == 0u) a1[a] = v;
    else if (q == 1u) a2[a] = v;
    else if (q == 2u) partners[a] = (uint32_t)s;
    else ay[(size_t)a * P + (q - 3u)] = v;
}

} // namespace

extern "C" int hgibbs_grm_rowsums(hgibbs_t h, int P, const double* Y, double* ay, double* a1, double* a2, double* diag, uint32_t* partners)
{
    const char* const who = "hgibbs_grm_rowsums";
    if (king_check(h, who)) return 1;
    h->grs_ms[0] = h->grs_ms[1] = 0.0;
    h->grm_used = 0;
    h->grm_E = 0;
    if (P < 1 || P > GS_PMAX) return fail("%s: P = %d, must be in [1, %d]", who, P, GS_PMAX);
    if (!Y) return fail("%s: null Y", who);
    const uint32_t n = h->n_local;
    if (n < 2u) return fail("%s: %u row, a pair needs two (n_local >= 2)", who, n);
    if (grm_mmax_check(h, who)) return 1;
    for (size_t i = 0; i < (size_t)P * n; ++i)
        if (!std::isfinite(Y[i])) return fail("%s: Y[%d][%zu] is not finite", who, (int)(i / n), i % n);
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;

    int k = 0;
    while (((uint64_t)1 << k) < n) ++k; // the smallest k with n <= 2^k
    const int F = 58 - k;
    const uint32_t Q = (uint32_t)P + 3u;
    const size_t nq = (size_t)n * Q, ny = (size_t)n * P;
    if (need_device_memory(nq * 8 + ny * 16 + (size_t)n * 28 + 8, "%s: the %u x %u accumulator, Y and the outputs (%.1f MiB)", who, n, Q,
                           (nq * 8 + ny * 16 + (size_t)n * 28) / 1048576.0))
        return 1;
    DevBuf<unsigned long long> acc, tmax;
    DevBuf<double> dY, day, da1, da2, ddiag;
    DevBuf<uint32_t> dpart;
    if (acc.alloc(nq) || tmax.alloc(1) || dY.alloc(ny) || day.alloc(ny) || da1.alloc(n) || da2.alloc(n) || ddiag.alloc(n) || dpart.alloc(n)) return 1;
    HIP_TRY(hipMemcpy(dY, Y, ny * sizeof(double), hipMemcpyHostToDevice));

    double products_ms = 0.0, reduce_ms = 0.0;
    if (lap_begin(h)) return 1;
    HIP_TRY(hipMemsetAsync(acc, 0, nq * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(tmax, 0, sizeof(unsigned long long), h->stream));
    if (lap_end(h, reduce_ms)) return 1;

    // the step of a piece: the reducer
    auto reduce = [&](const GrmPiece& pc, size_t, const double* dS, const int32_t* dn) -> int {
        GrsArgs g{};
        g.S = dS;
        g.nsnp = dn;
        g.Y = dY;
        g.n = n;
        g.P = (uint32_t)P;
        g.p0 = pc.p0;
        g.pc = pc.pc;
        g.rt0 = pc.p0 / GS_T;
        g.off0 = (unsigned long long)pc.p0 * (pc.p0 + 1ull) / 2ull;
        g.F = F;
        g.acc = acc;
        g.diag = ddiag;
        g.tmax = tmax;
        const uint32_t rt1 = (pc.p0 + pc.pc - 1u) / GS_T; // the piece's last row tile: column tiles 0 .. rt1
        if (lap_begin(h)) return 1;
        k_grs_reduce<<<dim3(rt1 + 1u, rt1 - g.rt0 + 1u), GS_WAVES * 64, 0, h->stream>>>(g);
        HIP_TRY(hipGetLastError());
        return lap_end(h, reduce_ms);
    };
    uint32_t used = 0;
    int E = 0;
    if (grm_pieces(h, who, 0, n, products_ms, used, E, reduce)) return 1;

    if (lap_begin(h)) return 1;
    k_grs_final<<<(uint32_t)((nq + 255u) / 256u), 256, 0, h->stream>>>(acc, n, (uint32_t)P, F, day, da1, da2, dpart);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, reduce_ms)) return 1;
    unsigned long long mb = 0;
    HIP_TRY(hipMemcpy(&mb, tmax, sizeof mb, hipMemcpyDeviceToHost));
    double tm;
    std::memcpy(&tm, &mb, sizeof tm);
    if (!(tm < 16.0))
        return fail("%s: a term of magnitude %g is outside the fixed-point range |t| < 16 (t = A_ab Y[p][b], A_ab or A_ab^2, F = %d): "
                    "scale Y down, nothing was written", who, tm, F);
    if (ay) HIP_TRY(hipMemcpy(ay, day, ny * sizeof(double), hipMemcpyDeviceToHost));
    if (a1) HIP_TRY(hipMemcpy(a1, da1, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (a2) HIP_TRY(hipMemcpy(a2, da2, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (diag) HIP_TRY(hipMemcpy(diag, ddiag, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (partners) HIP_TRY(hipMemcpy(partners, dpart, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    h->grs_ms[0] = products_ms;
    h->grs_ms[1] = reduce_ms;
    h->grm_used = used;
    h->grm_E = E;
    return 0;
}

extern "C" int hgibbs_last_grm_rowsums_ms(hgibbs_t h, double* products_ms, double* reduce_ms)
{
    if (!h || !products_ms || !reduce_ms) return fail("hgibbs_last_grm_rowsums_ms: null argument");
    *products_ms = h->grs_ms[0];
    *reduce_ms = h->grs_ms[1];
    return 0;
}
