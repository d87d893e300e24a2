// hydra's sparse genotype representation (three lists of row indices per marker: genotype 1, genotype 2, missing call; layout
// restated from src/BayesRRm.cpp:437-770 and src/data.cpp:1072-1106, 1224-1290) to and from the 2-bit device image.
// Included at the end of hgibbs.hip.  DESIGN.md section 24.
//
//   hgibbs_sparse_begin / _put / _end   index lists -> image: k_sp_fill, then k_sp_scatter (one 32-bit atomic OR per entry; the value it
//                                       returns tells a row listed twice).  The image sits on the SparseLoad, not on the handle, until
//                                       _end publishes it.
//   hgibbs_sparse_counts / _get         image -> index lists: k_counts for the lengths, k_sp_compact (ordered stream compaction: one
//                                       workgroup walks one column, integer scans only, no atomics) for the entries.
#pragma once

namespace {

constexpr uint32_t SP_SKIP = 0xffffffffu;                   // rank table: the row is not on this handle
constexpr uint64_t SP_STAGE_ENTRIES = (256ull << 20) / 4;   // entries of one list staged at a time (256 MiB, as hgibbs_load_bed's slab)
constexpr uint32_t SP_SLAB = 32768;                         // markers per launch (grid.y <= 65535, as hgibbs_synth_bed)
constexpr unsigned long long SP_NO_ERR = ~0ull;
enum { SP_TWICE = 0, SP_RANGE = 1 };

// every dword of the image: device code 0 for the rows below n_local, GC_MISS for the padding slots
__global__ void k_sp_fill(uint32_t* __restrict__ bed, uint64_t ndwords, uint32_t nw, uint32_t n_local)
{
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ndwords; i += step) {
        const uint64_t row0 = (i % nw) * 16;
        uint32_t w = 0;
        if (row0 + 16 > n_local) w = row0 >= n_local ? 0xffffffffu : ~((1u << (2 * (uint32_t)(n_local - row0))) - 1u);
        bed[i] = w;
    }
}

struct SpLists {
    const uint32_t* idx[3];            // the staged piece of each list
    const unsigned long long* off[3];  // per marker of the part: its first entry in that piece
    const uint32_t* len[3];            // per marker of the part: its entries
};

__device__ __forceinline__ unsigned long long sp_key(uint32_t marker, uint32_t row, uint32_t kind)
{
    return ((unsigned long long)marker << 33) | ((unsigned long long)row << 1) | kind;
}

// grid (x: strides over a list's entries, y: marker of the part, z: list).  Entry i of marker j, list code c: skipped when the row is not
// on the handle, else c is ORed into the row's field; a field that was not 0 before had the row listed already.  The smallest
// (marker, row, kind) that offends goes to *err.
__global__ __launch_bounds__(256) void k_sp_scatter(SpLists L, const uint32_t* __restrict__ rank, uint32_t n_total, uint8_t* bed, uint64_t stride,
                                                    uint32_t marker0, unsigned long long* err)
{
    const uint32_t k = blockIdx.y, list = blockIdx.z, marker = marker0 + k;
    const uint64_t n = L.len[list][k];
    const uint32_t* __restrict__ src = L.idx[list] + L.off[list][k];
    uint32_t* col = reinterpret_cast<uint32_t*>(bed + (uint64_t)marker * stride);
    const uint32_t code = list + 1;
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += step) {
        const uint32_t i = src[e];
        if (i >= n_total) {
            atomicMin(err, sp_key(marker, i, SP_RANGE));
            continue;
        }
        const uint32_t r = rank[i];
        if (r == SP_SKIP) continue;
        const uint32_t sh = 2 * (r & 15u);
        const uint32_t old = atomicOr(col + (r >> 4), code << sh);
        if ((old >> sh) & 3u) atomicMin(err, sp_key(marker, i, SP_TWICE));
    }
}

// One workgroup per marker walks the column in chunks of 4096 rows (a lane takes a dword, 16 rows) and carries three running bases.
// Per chunk: class masks, popcounts, an exclusive scan in row order (wave scan by shuffles, the four waves through LDS; genotype 1 and 2
// share a word, 16 bits each: a chunk holds at most 4096 of a class), then every lane writes its up to 16 indices at base + prefix.
// Integers only and no atomics: the lists come out ascending by construction.  bases: 3 per marker, entries from the start of o1/o2/om.
__global__ __launch_bounds__(BLOCK) void k_sp_compact(const uint8_t* __restrict__ bed, uint64_t stride, uint32_t n_local,
                                                      const unsigned long long* __restrict__ bases, uint32_t* __restrict__ o1,
                                                      uint32_t* __restrict__ o2, uint32_t* __restrict__ om)
{
    __shared__ uint32_t sh[2][2][BLOCK_WAVES];
    const uint32_t marker = blockIdx.x;
    const uint32_t* __restrict__ col = reinterpret_cast<const uint32_t*>(bed + (uint64_t)marker * stride);
    const uint32_t nw = (uint32_t)(stride >> 2);
    unsigned long long b1 = bases[3ull * marker], b2 = bases[3ull * marker + 1], bm = bases[3ull * marker + 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int c = 0;
    for (uint32_t d0 = 0; d0 < nw; d0 += BLOCK, c ^= 1) {
        const uint32_t i = d0 + threadIdx.x;
        const uint32_t row0 = i * 16u;
        uint32_t m1 = 0, m2 = 0, mm = 0;
        if (i < nw && row0 < n_local) {
            code_masks(col[i], m1, m2, mm);
            if (n_local - row0 < 16u) { // padding slots are never listed
                const uint32_t valid = (1u << (2 * (n_local - row0))) - 1u;
                m1 &= valid;
                m2 &= valid;
                mm &= valid;
            }
        }
        const uint32_t p12 = (uint32_t)__popc(m1) | ((uint32_t)__popc(m2) << 16), pm = (uint32_t)__popc(mm);
        uint32_t s12 = p12, sm = pm; // inclusive over the wave
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t12 = __shfl_up(s12, off, 64), tm = __shfl_up(sm, off, 64);
            if (lane >= off) {
                s12 += t12;
                sm += tm;
            }
        }
        if (lane == 63) {
            sh[c][0][wave] = s12;
            sh[c][1][wave] = sm;
        }
        __syncthreads(); // (one barrier a chunk: the next chunk writes the other half of sh)
        uint32_t pre12 = 0, prem = 0, tot12 = 0, totm = 0;
        for (int w = 0; w < BLOCK_WAVES; ++w) {
            const uint32_t v12 = sh[c][0][w], vm = sh[c][1][w];
            if (w < wave) {
                pre12 += v12;
                prem += vm;
            }
            tot12 += v12;
            totm += vm;
        }
        const uint32_t ex12 = pre12 + s12 - p12, exm = prem + sm - pm;
        if (o1) {
            unsigned long long q = b1 + (ex12 & 0xffffu);
            for (; m1; m1 &= m1 - 1) o1[q++] = row0 + ((uint32_t)(__ffs(m1) - 1) >> 1);
        }
        if (o2) {
            unsigned long long q = b2 + (ex12 >> 16);
            for (; m2; m2 &= m2 - 1) o2[q++] = row0 + ((uint32_t)(__ffs(m2) - 1) >> 1);
        }
        if (om) {
            unsigned long long q = bm + exm;
            for (; mm; mm &= mm - 1) om[q++] = row0 + ((uint32_t)(__ffs(mm) - 1) >> 1);
        }
        b1 += tot12 & 0xffffu;
        b2 += tot12 >> 16;
        bm += totm;
    }
}

} // namespace

// a load between hgibbs_sparse_begin and hgibbs_sparse_end
struct SparseLoad {
    DevBuf<uint8_t> bed;             // the image, not yet on the handle
    uint32_t n_total = 0;
    DevBuf<uint32_t> rank;           // n_total: row of the file -> local row, or SP_SKIP
    DevBuf<unsigned long long> err;  // the smallest offence (sp_key), SP_NO_ERR when none
    DevBuf<uint32_t> stage[3];       // the piece of each list a part scatters from
    uint64_t stage_n[3] = {0, 0, 0};
    DevBuf<unsigned long long> off;  // 3 x SP_SLAB
    DevBuf<uint32_t> len;            // 3 x SP_SLAB
    std::vector<uint8_t> done;       // per marker: put
    double ms = 0.0;
};

// The load is given up: the handle is as it was before hgibbs_sparse_begin (what alloc_problem allocated is released).  Returns 1 and
// leaves the message as it stands, so a failed step ends with `return sp_abandon(h)`.
static int sp_abandon(hgibbs_ctx* h)
{
    drop_problem(h); // (synchronises the stream first)
    h->sp.reset();
    h->sparse_ms[0] = 0.0;
    return 1;
}

// ev0 .. ev1 around what the caller has just launched; waits for it
static int sp_elapsed(hgibbs_ctx* h, double* ms)
{
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipEventSynchronize(h->ev1));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, h->ev0, h->ev1));
    *ms += (double)t;
    return 0;
}

extern "C" int hgibbs_sparse_begin(hgibbs_t h, uint32_t n_total, uint32_t M, const uint8_t* keep_host, uint32_t row_begin, uint32_t row_end,
                                   uint32_t n_global)
{
    if (!h) return fail("hgibbs_sparse_begin: null handle");
    if (h->sp) return fail("hgibbs_sparse_begin: a sparse load is already in progress on this handle");
    if (h->bed) return fail("data already loaded on this handle");
    h->sparse_ms[0] = 0.0;
    if (row_end <= row_begin) return fail("hgibbs_sparse_begin: empty row range");
    if (M >= 0x80000000u) return fail("hgibbs_sparse_begin: M %u is beyond 2^31 - 1", M);
    HIP_TRY(hipSetDevice(h->device));
    // the rank of every row of the file among the kept rows of this shard
    std::vector<uint32_t> rk(n_total, SP_SKIP);
    if (!keep_host) {
        if (row_end > n_total) return fail("hgibbs_sparse_begin: row_end %u > n_total %u", row_end, n_total);
        if (row_begin & 3u) return fail("hgibbs_sparse_begin: row_begin %u must be a multiple of 4", row_begin);
        for (uint32_t i = row_begin; i < row_end; ++i) rk[i] = i - row_begin;
    } else {
        uint32_t r = 0;
        for (uint32_t i = 0; i < n_total; ++i)
            if (keep_host[i]) {
                if (r >= row_begin && r < row_end) rk[i] = r - row_begin;
                ++r;
            }
        if (row_end > r) return fail("hgibbs_sparse_begin: row_end %u > kept individuals %u", row_end, r);
    }
    if (n_global < 2) return fail("hgibbs_sparse_begin: n_global must be at least 2");
    if (alloc_problem(h, n_global, row_end - row_begin, M, row_begin)) return 1;
    h->sp.reset(new SparseLoad());
    SparseLoad* s = h->sp.get();
    s->bed = std::move(h->bed); // not published before hgibbs_sparse_end: every other operator sees a handle without genotypes
    s->n_total = n_total;
    s->done.assign(M, 0);
    const auto fill = [&]() -> int {
        if (s->rank.alloc(n_total) || s->err.alloc(1) || s->off.alloc((size_t)3 * SP_SLAB) || s->len.alloc((size_t)3 * SP_SLAB)) return 1;
        HIP_TRY(hipMemcpyAsync(s->rank, rk.data(), (size_t)n_total * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemsetAsync(s->err, 0xff, sizeof(unsigned long long), h->stream));
        HIP_TRY(hipEventRecord(h->ev0, h->stream));
        k_sp_fill<<<4096, 256, 0, h->stream>>>(reinterpret_cast<uint32_t*>(s->bed.p), (uint64_t)M * h->stride / 4, (uint32_t)(h->stride / 4), h->n_local);
        HIP_TRY(hipGetLastError());
        return sp_elapsed(h, &s->ms);
    };
    return fill() ? sp_abandon(h) : 0;
}

// The checks and the device work of hgibbs_sparse_put; whichever fails, the caller gives the load up
static int sp_put(hgibbs_ctx* h, uint32_t m0, uint32_t count, const hgibbs_sparse_list* const li[3])
{
    SparseLoad* s = h->sp.get();
    static const char* const nm[3] = {"ones", "twos", "miss"};
    // the host's refusals, before any device work
    for (int l = 0; l < 3; ++l)
        if (!li[l] || (count && (!li[l]->start || !li[l]->len)) || (li[l]->idx_count && !li[l]->idx)) return fail("hgibbs_sparse_put: null list (%s)", nm[l]);
    if ((uint64_t)m0 + count > h->M) return fail("hgibbs_sparse_put: markers [%u, %llu) beyond M = %u", m0, (unsigned long long)m0 + count, h->M);
    for (uint32_t k = 0; k < count; ++k)
        if (s->done[m0 + k]) return fail("hgibbs_sparse_put: marker %u was put already", m0 + k);
    for (int l = 0; l < 3; ++l)
        for (uint32_t k = 0; k < count; ++k) {
            const uint64_t st = li[l]->start[k], ln = li[l]->len[k];
            if (ln > s->n_total) return fail("hgibbs_sparse_put: marker %u, list %s: len %llu > n_total %u", m0 + k, nm[l], (unsigned long long)ln, s->n_total);
            if (st < li[l]->idx_base)
                return fail("hgibbs_sparse_put: marker %u, list %s: start %llu < idx_base %llu", m0 + k, nm[l], (unsigned long long)st,
                            (unsigned long long)li[l]->idx_base);
            if (st - li[l]->idx_base > li[l]->idx_count || ln > li[l]->idx_count - (st - li[l]->idx_base))
                return fail("hgibbs_sparse_put: marker %u, list %s: start %llu + len %llu is beyond the piece [%llu, %llu)", m0 + k, nm[l],
                            (unsigned long long)st, (unsigned long long)ln, (unsigned long long)li[l]->idx_base,
                            (unsigned long long)(li[l]->idx_base + li[l]->idx_count));
        }
    // parts of at most SP_SLAB markers whose entries, list by list, span at most SP_STAGE_ENTRIES (a marker alone may exceed it)
    std::vector<unsigned long long> off((size_t)3 * SP_SLAB);
    std::vector<uint32_t> len((size_t)3 * SP_SLAB);
    for (uint32_t k0 = 0; k0 < count;) {
        uint64_t lo[3], hi[3], maxlen = 0;
        uint32_t k1 = k0;
        for (; k1 < count && k1 - k0 < SP_SLAB; ++k1) {
            uint64_t nlo[3], nhi[3];
            bool fits = true;
            for (int l = 0; l < 3; ++l) {
                const uint64_t st = li[l]->start[k1], en = st + li[l]->len[k1];
                nlo[l] = k1 == k0 ? st : std::min(lo[l], st);
                nhi[l] = k1 == k0 ? en : std::max(hi[l], en);
                if (nhi[l] - nlo[l] > SP_STAGE_ENTRIES) fits = false;
            }
            if (!fits && k1 > k0) break;
            for (int l = 0; l < 3; ++l) {
                lo[l] = nlo[l];
                hi[l] = nhi[l];
                maxlen = std::max<uint64_t>(maxlen, li[l]->len[k1]);
            }
        }
        const uint32_t pc = k1 - k0;
        SpLists L;
        for (int l = 0; l < 3; ++l) {
            const uint64_t n = hi[l] - lo[l];
            if (n > s->stage_n[l]) {
                HIP_TRY(hipStreamSynchronize(h->stream));
                s->stage_n[l] = 0;
                if (s->stage[l].alloc(n)) return 1;
                s->stage_n[l] = n;
            }
            if (n) HIP_TRY(hipMemcpyAsync(s->stage[l], li[l]->idx + (lo[l] - li[l]->idx_base), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            for (uint32_t k = 0; k < pc; ++k) {
                off[(size_t)l * SP_SLAB + k] = li[l]->start[k0 + k] - lo[l];
                len[(size_t)l * SP_SLAB + k] = (uint32_t)li[l]->len[k0 + k];
            }
            HIP_TRY(hipMemcpyAsync(s->off + (size_t)l * SP_SLAB, off.data() + (size_t)l * SP_SLAB, (size_t)pc * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(s->len + (size_t)l * SP_SLAB, len.data() + (size_t)l * SP_SLAB, (size_t)pc * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            L.idx[l] = s->stage[l];
            L.off[l] = s->off + (size_t)l * SP_SLAB;
            L.len[l] = s->len + (size_t)l * SP_SLAB;
        }
        if (maxlen) {
            const uint32_t gx = (uint32_t)std::min<uint64_t>(64, (maxlen + 1023) / 1024);
            HIP_TRY(hipEventRecord(h->ev0, h->stream));
            k_sp_scatter<<<dim3(gx, pc, 3), 256, 0, h->stream>>>(L, s->rank, s->n_total, s->bed, h->stride, m0 + k0, s->err);
            HIP_TRY(hipGetLastError());
            if (sp_elapsed(h, &s->ms)) return 1;
        } else {
            HIP_TRY(hipStreamSynchronize(h->stream)); // (the host vectors are written again by the next part)
        }
        k0 = k1;
    }
    unsigned long long e = SP_NO_ERR;
    HIP_TRY(hipMemcpy(&e, s->err, sizeof e, hipMemcpyDeviceToHost));
    if (e != SP_NO_ERR) {
        const uint32_t marker = (uint32_t)(e >> 33), row = (uint32_t)(e >> 1);
        if ((e & 1u) == SP_RANGE) return fail("hgibbs_sparse_put: marker %u lists row %u, which is not below n_total = %u", marker, row, s->n_total);
        return fail("hgibbs_sparse_put: marker %u lists row %u twice (in one list or in two)", marker, row);
    }
    for (uint32_t k = 0; k < count; ++k) s->done[m0 + k] = 1;
    return 0;
}

extern "C" int hgibbs_sparse_put(hgibbs_t h, uint32_t m0, uint32_t count, const hgibbs_sparse_list* ones, const hgibbs_sparse_list* twos,
                                 const hgibbs_sparse_list* miss)
{
    if (!h) return fail("hgibbs_sparse_put: null handle");
    if (!h->sp) return fail("hgibbs_sparse_put: no sparse load in progress (hgibbs_sparse_begin)");
    HIP_TRY(hipSetDevice(h->device));
    const hgibbs_sparse_list* const li[3] = {ones, twos, miss};
    return sp_put(h, m0, count, li) ? sp_abandon(h) : 0;
}

extern "C" int hgibbs_sparse_end(hgibbs_t h)
{
    if (!h) return fail("hgibbs_sparse_end: null handle");
    if (!h->sp) return fail("hgibbs_sparse_end: no sparse load in progress (hgibbs_sparse_begin)");
    SparseLoad* s = h->sp.get();
    HIP_TRY(hipSetDevice(h->device));
    const auto complete = [&]() -> int {
        for (uint32_t j = 0; j < h->M; ++j)
            if (!s->done[j]) return fail("hgibbs_sparse_end: marker %u was never put", j);
        HIP_TRY(hipStreamSynchronize(h->stream));
        return 0;
    };
    if (complete()) return sp_abandon(h);
    h->bed = std::move(s->bed); // published
    h->sparse_ms[0] = s->ms;
    h->sp.reset();
    h->have_stats = false;
    return 0;
}

extern "C" int hgibbs_sparse_counts(hgibbs_t h, uint32_t m0, uint32_t count, uint64_t* n1, uint64_t* n2, uint64_t* nm)
{
    if (!h || !h->bed) return fail("hgibbs_sparse_counts: no data loaded");
    if (h->nranks > 1) return fail("hgibbs_sparse_counts: the handle is one of %d ranks: the lists are written from one rank that holds every row", h->nranks);
    if ((uint64_t)m0 + count > h->M) return fail("hgibbs_sparse_counts: marker range out of bounds");
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1; // k_counts: on one rank the handle's own rows' counts
    if (!count) return 0;
    std::vector<unsigned long long> c((size_t)count * 3);
    HIP_TRY(hipMemcpy(c.data(), h->counts + (size_t)m0 * 3, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < count; ++k) {
        if (n1) n1[k] = c[3ull * k];
        if (n2) n2[k] = c[3ull * k + 1];
        if (nm) nm[k] = c[3ull * k + 2];
    }
    return 0;
}

extern "C" int hgibbs_sparse_get(hgibbs_t h, uint32_t m0, uint32_t count, uint32_t* idx1, uint32_t* idx2, uint32_t* idxm)
{
    if (h) h->sparse_ms[1] = 0.0;
    if (!h || !h->bed) return fail("hgibbs_sparse_get: no data loaded");
    if (h->nranks > 1) return fail("hgibbs_sparse_get: the handle is one of %d ranks: the lists are written from one rank that holds every row", h->nranks);
    if ((uint64_t)m0 + count > h->M) return fail("hgibbs_sparse_get: marker range out of bounds");
    HIP_TRY(hipSetDevice(h->device));
    if (compute_stats(h)) return 1;
    if (!count) return 0;
    std::vector<unsigned long long> c((size_t)count * 3);
    HIP_TRY(hipMemcpy(c.data(), h->counts + (size_t)m0 * 3, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint32_t* const out_host[3] = {idx1, idx2, idxm};
    uint64_t cap = (uint64_t)h->sparse_piece;
    if (!cap) {
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        cap = std::min<uint64_t>(1ull << 30, fr / 4);
    }
    struct {
        DevBuf<unsigned long long> bases;
        DevBuf<uint32_t> out[3];
        uint64_t out_n[3] = {0, 0, 0};
    } b;
    std::vector<unsigned long long> bases;
    uint64_t done[3] = {0, 0, 0}; // entries handed to the caller so far
    size_t bases_n = 0;
    double ms = 0.0;
    for (uint32_t k0 = 0; k0 < count;) {
        // a piece: markers whose requested lists fit the bound together (a marker alone may exceed it)
        uint64_t tot[3] = {0, 0, 0};
        uint32_t k1 = k0;
        bases.clear();
        for (; k1 < count; ++k1) {
            uint64_t bytes = 0;
            for (int l = 0; l < 3; ++l)
                if (out_host[l]) bytes += 4 * (tot[l] + c[3ull * k1 + l]);
            if (bytes > cap && k1 > k0) break;
            for (int l = 0; l < 3; ++l) {
                bases.push_back(tot[l]);
                tot[l] += c[3ull * k1 + l];
            }
        }
        const uint32_t pc = k1 - k0;
        if (bases.size() > bases_n) {
            bases_n = std::max<size_t>(bases.size(), std::min<size_t>((size_t)3 * (count - k0), (size_t)3 * 65536));
            if (b.bases.alloc(bases_n)) return 1;
        }
        HIP_TRY(hipMemcpyAsync(b.bases, bases.data(), bases.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
        bool any = false;
        for (int l = 0; l < 3; ++l) {
            if (!out_host[l] || !tot[l]) continue;
            any = true;
            if (tot[l] > b.out_n[l]) {
                b.out_n[l] = 0;
                if (b.out[l].alloc(tot[l])) return 1;
                b.out_n[l] = tot[l];
            }
        }
        if (any) {
            HIP_TRY(hipEventRecord(h->ev0, h->stream));
            k_sp_compact<<<pc, BLOCK, 0, h->stream>>>(h->bed + (size_t)(m0 + k0) * h->stride, h->stride, h->n_local, b.bases,
                                                      (out_host[0] && tot[0]) ? b.out[0] : nullptr, (out_host[1] && tot[1]) ? b.out[1] : nullptr,
                                                      (out_host[2] && tot[2]) ? b.out[2] : nullptr);
            HIP_TRY(hipGetLastError());
            if (sp_elapsed(h, &ms)) return 1;
            for (int l = 0; l < 3; ++l)
                if (out_host[l] && tot[l]) {
                    HIP_TRY(hipMemcpy(out_host[l] + done[l], b.out[l], (size_t)tot[l] * sizeof(uint32_t), hipMemcpyDeviceToHost));
                    done[l] += tot[l];
                }
        } else {
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        k0 = k1;
    }
    h->sparse_ms[1] = ms;
    return 0;
}

extern "C" int hgibbs_last_sparse_ms(hgibbs_t h, double* put_ms, double* get_ms)
{
    if (!h) return fail("hgibbs_last_sparse_ms: null handle");
    if (put_ms) *put_ms = h->sparse_ms[0];
    if (get_ms) *get_ms = h->sparse_ms[1];
    return 0;
}
