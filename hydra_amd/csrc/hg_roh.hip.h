// Runs of homozygosity of the loaded rows: a walk along the markers of one row that carries state from marker to
// marker, where every other operator is a sum.  For a list of runs (the selected markers of one chromosome each, in order), per row:
//
//   window    s covers positions [s, s + W) of a run of L markers, 0 <= s <= L - W; it is homozygous when it holds at most h hets (code 1)
//             and at most m missing calls (code 3)
//   covered   position k lies in nw(k) = min(k, L - W) - max(0, k - W + 1) + 1 windows and is covered when at least need[nw(k)] of them are
//             homozygous (the host's table: the device compares integers only)
//   segment   a maximal stretch of covered positions, also cut between neighbours more than gap_bp apart; kept when it has at least
//             min_snps markers, len = bp[last] - bp[first] >= min_bp, len <= dens_bp n, and at most max_het hets
//
//   rows      a wave owns 64 rows (the 16 bytes of a marker's column that k_row_sums' wave loads), a workgroup four waves, grid y the runs:
//             runs and rows are independent, nothing waits for anything.
//   block     lane l loads those 16 bytes of entry 64 b + l of the run's idx (a gather: the selection has holes).  sc_transpose16 turns
//             each dword into one row's sixteen codes of the lane group's markers; four rotations among the lane groups (rh_gather) leave
//             lane l with row l's 64 codes of the block, packed into a het mask and a missing mask of 64 bits.
//   lag       a window that starts in block b ends in block b + 1 at the latest, so with block b + 1 in hand the windows that start in b
//             are decided (rh_windows: two sliding counts), then the positions of b (rh_covered: one sliding count over the window bits of
//             b - 1 and b), then the segments (rh_walk: bit scans for where covered stops and starts, popcounts for NHET and NMISS).
//             Positions, nw and need are the same for the 64 rows: only the masks differ between lanes.
//   state     per lane between blocks: the masks of the block, the window bits of the last two blocks, and of the open segment its first
//             position and its het and missing counts.
//   edges     entries past the end of a run load nothing; their windows (s > L - W) are never homozygous and their positions never
//             covered.  Padding rows (code 3 everywhere) would be homozygous with m >= W: rows >= n_local emit nothing.
//   list      a kept segment takes a slot by one atomic add; every segment is counted, so when the list overflows the host runs the
//             kernel once more with the exact capacity (as hgibbs_king_pairs does) and then sorts by (row, first): the order of the
//             atomics never shows.
// Integers only; the result does not depend on the grid, the capacity or repeats.
#pragma once

namespace {

constexpr uint32_t RH_LIST0 = 1u << 20; // first capacity of the segment list (option roh_list0)
constexpr int RH_TPB = 256;             // four waves of 64 rows

struct RohArgs {
    const uint8_t* bed;
    uint64_t stride;
    uint32_t n_local;
    const uint32_t* run_off; // nruns + 1
    const uint32_t* idx;     // per position: the marker
    const long long* bp;     // per position
    hgibbs_roh_params p;
    unsigned long long* nlist;
    unsigned long long cap;
    hgibbs_roh_seg* segs;
};

// the even bits of x (sixteen 2-bit fields' low bits) as sixteen bits
__device__ __forceinline__ uint32_t rh_even16(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}

// z[b]: lane (c, g) holds row 16 b + c's codes of markers 16 g .. 16 g + 15 of the block (sc_transpose16 of dword b).  Lane l = 16 b' + c'
// wants z[b'] of the lanes (c', 0 .. 3): in round t lane (c, g) sends z[(g - t) & 3] to lane 16 ((g - t) & 3) + c, which receives piece
// g = (b' + t) & 3.  Returns row l's het and missing masks of the block's 64 markers.
__device__ __forceinline__ void rh_gather(const uint32_t* z, uint32_t lane, unsigned long long& het, unsigned long long& mis)
{
    const uint32_t c = lane & 15u, g = lane >> 4;
    het = 0ull;
    mis = 0ull;
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) {
        const uint32_t sb = (g - t) & 3u; // the register this lane sends
        const uint32_t v = sb == 0u ? z[0] : sb == 1u ? z[1] : sb == 2u ? z[2] : z[3];
        const uint32_t piece = (g + t) & 3u; // as a receiver (b' = g): the piece that arrives, from lane (c, piece)
        const uint32_t x = (uint32_t)__shfl((int)v, (int)(16u * piece + c));
        const uint32_t m3 = x & (x >> 1) & 0x55555555u; // code 3
        const uint32_t h1 = (x & 0x55555555u) ^ m3;     // code 1
        het |= (unsigned long long)rh_even16(h1) << (16u * piece);
        mis |= (unsigned long long)rh_even16(m3) << (16u * piece);
    }
}

// bit i: the window that starts at position i of the block (lo: the block's mask, hi: the next block's) holds at most `lim` set bits.
// count(i + 1) = count(i) + [bit i + W] - [bit i]
__device__ __forceinline__ void rh_windows(unsigned long long hlo, unsigned long long hhi, unsigned long long mlo, unsigned long long mhi, uint32_t W,
                                           uint32_t h, uint32_t m, unsigned long long& out)
{
    const unsigned long long wm = W == 64u ? ~0ull : (1ull << W) - 1ull;
    const unsigned long long he = W == 64u ? hhi : (hlo >> W) | (hhi << (64u - W)); // bit i: bit i + W of (lo, hi)
    const unsigned long long me = W == 64u ? mhi : (mlo >> W) | (mhi << (64u - W));
    int ch = __popcll(hlo & wm), cm = __popcll(mlo & wm);
    uint32_t o0 = 0, o1 = 0;
    const uint32_t he0 = (uint32_t)he, he1 = (uint32_t)(he >> 32), hl0 = (uint32_t)hlo, hl1 = (uint32_t)(hlo >> 32);
    const uint32_t me0 = (uint32_t)me, me1 = (uint32_t)(me >> 32), ml0 = (uint32_t)mlo, ml1 = (uint32_t)(mlo >> 32);
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        o0 |= (uint32_t)(ch <= (int)h && cm <= (int)m) << i;
        ch += (int)((he0 >> i) & 1u) - (int)((hl0 >> i) & 1u);
        cm += (int)((me0 >> i) & 1u) - (int)((ml0 >> i) & 1u);
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        o1 |= (uint32_t)(ch <= (int)h && cm <= (int)m) << i;
        ch += (int)((he1 >> i) & 1u) - (int)((hl1 >> i) & 1u);
        cm += (int)((me1 >> i) & 1u) - (int)((ml1 >> i) & 1u);
    }
    out = ((unsigned long long)o1 << 32) | o0;
}

// bit i: position base + i (< L) is covered.  wprev, wcur: the window bits of the block before and of this block.  The windows over
// position i start at i - W + 1 .. i: count(i + 1) = count(i) + wcur[i + 1] - [window i - W + 1]
__device__ __forceinline__ unsigned long long rh_covered(unsigned long long wprev, unsigned long long wcur, uint32_t W, uint32_t base, uint32_t L,
                                                         const hgibbs_roh_params& p)
{
    const unsigned long long leave = W == 1u ? wcur : (wcur << (W - 1u)) | (wprev >> (65u - W)); // bit i: window i - W + 1
    int cnt = (W == 1u ? 0 : __popcll(wprev >> (65u - W))) + (int)(wcur & 1ull);
    const uint32_t lastw = L - W; // the last window
    unsigned long long out = 0ull;
    const uint32_t n = min(64u, L - base);
    for (uint32_t i = 0; i < n; ++i) { // (uniform)
        const uint32_t k = base + i;
        const uint32_t nw = min(k, lastw) - (k + 1u > W ? k + 1u - W : 0u) + 1u; // 1 .. W
        if (cnt >= (int)p.need[nw]) out |= 1ull << i;
        cnt += (i < 63u ? (int)((wcur >> (i + 1u)) & 1ull) : 0) - (int)((leave >> i) & 1ull);
    }
    return out;
}

struct RohOpen {
    bool open;
    uint32_t first, nhet, nmiss;
};

// closes the open segment at position `last` (of the run that starts at entry `off`): the filters, then the append
__device__ __forceinline__ void rh_close(const RohArgs& a, RohOpen& s, uint32_t off, uint32_t last, uint32_t row)
{
    s.open = false;
    const uint32_t n = last - s.first + 1u;
    if (row >= a.n_local || n < a.p.min_snps) return;
    if (a.p.max_het != 0xFFFFFFFFu && s.nhet > a.p.max_het) return;
    const long long len = a.bp[off + last] - a.bp[off + s.first]; // 0 <= len < 2^62 (checked by the host)
    if (len < a.p.min_bp || (len + (long long)n - 1) / (long long)n > a.p.dens_bp) return; // ceil(len / n) <= dens  <=>  len <= dens n
    const unsigned long long slot = __hip_atomic_fetch_add(a.nlist, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot >= a.cap) return; // counted: the host runs again with the exact capacity
    hgibbs_roh_seg g;
    g.row = row;
    g.first = off + s.first;
    g.last = off + last;
    g.nsnp = n;
    g.nhet = s.nhet;
    g.nmiss = s.nmiss;
    a.segs[slot] = g;
}

// the segments of one block: cov the covered positions, cut bit i = position base + i starts a new segment whatever came before it
__device__ __forceinline__ void rh_walk(const RohArgs& a, RohOpen& s, unsigned long long cov, unsigned long long cut, unsigned long long het,
                                        unsigned long long mis, uint32_t off, uint32_t base, uint32_t row)
{
    if (!s.open && !cov) return;
    const unsigned long long stop = ~cov | cut;
    uint32_t pos = 0; // the first position not yet looked at
    while (pos < 64u) {
        const unsigned long long from = ~0ull << pos;
        if (s.open) {
            const unsigned long long st = stop & from;
            const uint32_t e = st ? (uint32_t)__ffsll((long long)st) - 1u : 64u;
            const unsigned long long in = from & (e == 64u ? ~0ull : ~(~0ull << e)); // positions pos .. e - 1 join the segment
            s.nhet += (uint32_t)__popcll(het & in);
            s.nmiss += (uint32_t)__popcll(mis & in);
            if (e == 64u) return;
            rh_close(a, s, off, base + e - 1u, row); // (e = 0: the segment ended with the block before)
            pos = e;                                 // a covered position behind a cut opens the next one
        } else {
            const unsigned long long st = cov & from;
            if (!st) return;
            const uint32_t b = (uint32_t)__ffsll((long long)st) - 1u;
            s.open = true;
            s.first = base + b;
            s.nhet = (uint32_t)((het >> b) & 1ull);
            s.nmiss = (uint32_t)((mis >> b) & 1ull);
            pos = b + 1u;
        }
    }
}

// Workgroup (x, y): rows [256 x, 256 x + 256) -- wave w the 64 from 256 x + 64 w --, run y
__global__ __launch_bounds__(RH_TPB) void k_roh(RohArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t row0 = blockIdx.x * (uint32_t)RH_TPB + wave * 64u;
    if (row0 >= a.n_local) return; // (wave-uniform) padding rows only
    const uint32_t off = a.run_off[blockIdx.y], L = a.run_off[blockIdx.y + 1u] - off;
    const uint32_t W = a.p.window;
    if (L < W) return; // no window: nothing is covered
    const uint32_t nb = (L + 63u) / 64u, lastw = L - W;
    const uint8_t* col = a.bed + (uint64_t)row0 / 4u; // the wave's 16 bytes of a column
    const uint32_t m16 = lane & 15u, row = row0 + lane;

    auto load = [&](uint32_t b) {
        const uint32_t k = 64u * b + lane;
        uint4 v = make_uint4(0u, 0u, 0u, 0u); // (past the end of the run: in no window that counts)
        if (k < L) v = *reinterpret_cast<const uint4*>(col + (uint64_t)a.idx[off + k] * a.stride);
        return v;
    };
    auto masks = [&](const uint4& v, unsigned long long& het, unsigned long long& mis) {
        const uint32_t z[4] = {sc_transpose16(v.x, m16), sc_transpose16(v.y, m16), sc_transpose16(v.z, m16), sc_transpose16(v.w, m16)};
        rh_gather(z, lane, het, mis);
    };

    unsigned long long hcur, mcur, wprev = 0ull;
    RohOpen s{false, 0u, 0u, 0u};
    uint4 raw = load(0u);
    masks(raw, hcur, mcur);
    raw = load(1u);
    for (uint32_t b = 0; b < nb; ++b) {
        // block b + 1 (all zero past the run) decides the windows that start in block b
        unsigned long long hnxt, mnxt;
        masks(raw, hnxt, mnxt);
        raw = load(b + 2u); // in flight during this block's counts (nothing past the run)
        const uint32_t base = 64u * b;
        unsigned long long wcur;
        rh_windows(hcur, hnxt, mcur, mnxt, W, a.p.window_het, a.p.window_missing, wcur);
        if (lastw < base) wcur = 0ull;                                 // windows past L - W do not exist
        else if (lastw - base < 63u) wcur &= ~(~0ull << (lastw - base + 1u));
        const unsigned long long cov = rh_covered(wprev, wcur, W, base, L, a.p);
        // lane i: is position base + i more than gap_bp behind its neighbour?
        const uint32_t k = base + lane;
        const bool far = k > 0u && k < L && a.bp[off + k] - a.bp[off + k - 1u] > a.p.gap_bp;
        const unsigned long long cut = __ballot(far);
        rh_walk(a, s, cov, cut, hcur, mcur, off, base, row);
        wprev = wcur;
        hcur = hnxt;
        mcur = mnxt;
    }
    if (s.open) rh_close(a, s, off, L - 1u, row);
}

} // namespace

extern "C" int hgibbs_roh(hgibbs_t h, uint32_t nruns, const uint32_t* run_off, const uint32_t* idx, const int64_t* bp, const hgibbs_roh_params* p,
                          uint64_t* nseg)
{
    if (h) h->roh_ms = 0.0;
    if (op_guard(h, "hgibbs_roh", "a segment is a property of one row over every selected marker")) return 1;
    if (!run_off || !p || !nseg) return fail("hgibbs_roh: null argument");
    if (nruns > 65535u) return fail("hgibbs_roh: %u runs, at most 65535 (one row of the grid each)", nruns);
    if (run_off[0] != 0u) return fail("hgibbs_roh: run_off[0] = %u, the first run starts at entry 0", run_off[0]);
    for (uint32_t r = 0; r < nruns; ++r)
        if (run_off[r + 1] < run_off[r]) return fail("hgibbs_roh: run_off decreases at run %u (%u after %u)", r, run_off[r + 1], run_off[r]);
    const uint32_t total = run_off[nruns];
    if (total >= 0x80000000u) return fail("hgibbs_roh: %u entries, fewer than 2^31 are taken", total);
    if (total && (!idx || !bp)) return fail("hgibbs_roh: null argument");
    if (p->window < 1u || p->window > 64u) return fail("hgibbs_roh: window = %u, needs 1 to 64 markers (a window is one 64-bit word)", p->window);
    for (uint32_t n = 1; n <= p->window; ++n)
        if (p->need[n] < 1u || p->need[n] > n) return fail("hgibbs_roh: need[%u] = %u, needs 1 to %u (of the %u windows over a position)", n, p->need[n], n, n);
    if (p->min_bp < 0 || p->dens_bp < 0 || p->gap_bp < 0)
        return fail("hgibbs_roh: negative limit (min_bp = %lld, dens_bp = %lld, gap_bp = %lld)", (long long)p->min_bp, (long long)p->dens_bp, (long long)p->gap_bp);
    for (uint32_t r = 0; r < nruns; ++r)
        for (uint32_t k = run_off[r]; k < run_off[r + 1]; ++k) {
            if (idx[k] >= h->M) return fail("hgibbs_roh: entry %u is marker %u, the handle has %u", k, idx[k], h->M);
            if (bp[k] < 0 || bp[k] > (1ll << 62)) return fail("hgibbs_roh: entry %u has bp %lld, needs 0 to 2^62", k, (long long)bp[k]);
            if (k == run_off[r]) continue;
            if (idx[k] <= idx[k - 1]) return fail("hgibbs_roh: idx is not ascending within run %u (entry %u: marker %u after %u)", r, k, idx[k], idx[k - 1]);
            if (bp[k] < bp[k - 1]) return fail("hgibbs_roh: bp decreases within run %u (entry %u: %lld after %lld)", r, k, (long long)bp[k], (long long)bp[k - 1]);
        }
    HIP_TRY(hipSetDevice(h->device));

    unsigned long long cap = h->roh_list0 ? (unsigned long long)h->roh_list0 : RH_LIST0, found = 0;
    double total_ms = 0.0;
    std::vector<hgibbs_roh_seg> segs;
    if (nruns && total) {
        const size_t fixed = (size_t)(nruns + 1u) * sizeof(uint32_t) + (size_t)total * (sizeof(uint32_t) + sizeof(long long));
        if (need_device_memory(fixed + cap * sizeof(hgibbs_roh_seg), "hgibbs_roh: %u entries and a list of %llu segments need %.1f MiB", total, cap,
                               (fixed + cap * sizeof(hgibbs_roh_seg)) / 1048576.0))
            return 1;
        DevBuf<uint32_t> doff, didx;
        DevBuf<long long> dbp;
        DevBuf<unsigned long long> nlist;
        DevBuf<hgibbs_roh_seg> dsegs;
        if (doff.alloc(nruns + 1u) || didx.alloc(total) || dbp.alloc(total) || nlist.alloc(1)) return 1;
        HIP_TRY(hipMemcpy(doff, run_off, (size_t)(nruns + 1u) * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(didx, idx, (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dbp, bp, (size_t)total * sizeof(long long), hipMemcpyHostToDevice));
        for (;;) {
            if (dsegs.alloc(cap)) return 1;
            if (lap_begin(h)) return 1; // (after the allocations: the device time is the kernels')
            HIP_TRY(hipMemsetAsync(nlist, 0, sizeof(unsigned long long), h->stream));
            RohArgs a{};
            a.bed = h->bed;
            a.stride = h->stride;
            a.n_local = h->n_local;
            a.run_off = doff;
            a.idx = didx;
            a.bp = dbp;
            a.p = *p;
            a.nlist = nlist;
            a.cap = cap;
            a.segs = dsegs;
            k_roh<<<dim3(h->n_pad / (uint32_t)RH_TPB, nruns), RH_TPB, 0, h->stream>>>(a);
            HIP_TRY(hipGetLastError());
            if (lap_end(h, total_ms)) return 1;
            HIP_TRY(hipMemcpy(&found, nlist, sizeof found, hipMemcpyDeviceToHost));
            if (found <= cap) break;
            // the list overflowed: every segment was counted, so the second run fits exactly (the first list goes before the check)
            dsegs.release();
            cap = found;
            if (need_device_memory(cap * sizeof(hgibbs_roh_seg), "hgibbs_roh: %llu segments are kept: the list needs %.1f MiB", found,
                                   cap * sizeof(hgibbs_roh_seg) / 1048576.0))
                return 1;
        }
        segs.resize(found);
        if (found) HIP_TRY(hipMemcpy(segs.data(), dsegs, found * sizeof(hgibbs_roh_seg), hipMemcpyDeviceToHost));
        // sorted by (row, first): the order of the atomics never shows
        std::sort(segs.begin(), segs.end(), [](const hgibbs_roh_seg& x, const hgibbs_roh_seg& y) { return x.row != y.row ? x.row < y.row : x.first < y.first; });
    }
    h->roh_segs.swap(segs);
    h->roh_ms = total_ms;
    *nseg = found;
    return 0;
}

extern "C" int hgibbs_roh_get(hgibbs_t h, hgibbs_roh_seg* segs)
{
    if (!h) return fail("hgibbs_roh_get: null handle");
    if (segs && !h->roh_segs.empty()) std::memcpy(segs, h->roh_segs.data(), h->roh_segs.size() * sizeof(hgibbs_roh_seg));
    return 0;
}

extern "C" int hgibbs_last_roh_ms(hgibbs_t h, double* ms)
{
    if (!h || !ms) return fail("hgibbs_last_roh_ms: null argument");
    *ms = h->roh_ms;
    return 0;
}
