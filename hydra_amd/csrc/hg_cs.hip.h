// Local credible sets from the chains' inclusion history, kept on the device.
// Between hgibbs_cs_begin and hgibbs_cs_end the handle holds one bit per marker and record: record q = t C + r (t adds so far, chain r),
// hist[(q / 64) M + j] bit q % 64 = "marker j is in the model in record q".  The layout is word-major: the M words of one group of 64
// records lie side by side, so an add is one coalesced pass; the price is a gather (stride M) per member when a set's PEP is formed.
//
//   add     k_cs_add: ONE launch per record of every chain, a thread per marker.  The thread gathers the C bits of its marker (a flag
//           byte, or a chain's component != 0) and ORs them into the words of its column that bits t C .. t C + C - 1 touch: a word is
//           flushed when its bit 63 is reached or the chains end.  Plain loads and stores: a word belongs to the one thread of its marker.
//   counts  k_cs_counts: a thread per marker, cnt[j] = the popcount of its words.
//   sets    k_cs_sets: one workgroup of CS_TPB threads per lead v.  The lead's two mask rows (2 wpr contiguous words) give its friends; the
//           cnt of friend slot s (s < 64 wpr: marker v + 1 + s; 64 wpr <= s: marker v - 1 - (s - 64 wpr)) goes to LDS, 0 where the bit is
//           not set, the offset is above W, the marker does not exist or its cnt is 0.  A pick is the maximum over the slots of
//           (cnt << 32) | ~index: the largest cnt, ties to the smallest index; the picked slot is cleared.  The picks end when the sum
//           reaches `need`, no friend is left (short) or max_size members are taken (cap).  Then the lanes stride the words of the
//           history: OR over the members, popcount, and a sum over the workgroup gives the PEP.
//
// Everything is integer: the results do not depend on the order of the leads, on how they are split over calls, or on repeats.
#pragma once

struct CsState {
    uint32_t M = 0, C = 0, T = 0, t = 0;
    size_t NW = 0;                    // words per marker: (C T + 63) / 64
    DevBuf<unsigned long long> hist;  // NW x M
    DevBuf<uint32_t> cnt;             // M: the counts as of `cnt_t` adds
    DevBuf<uint8_t> flags;            // C x M: hgibbs_cs_add_flags' staging
    uint32_t cnt_t = 0xFFFFFFFFu;
    double add_ms = 0.0, counts_ms = 0.0, sets_ms = 0.0;
};

namespace {

constexpr int CS_TPB = 256;
constexpr uint32_t CS_MAX_SIZE = 256u;
constexpr uint32_t CS_NONE = 0xFFFFFFFFu;

// Thread per marker j: bits q0 .. q0 + C - 1 of its column, bit r from src[r M + j] != 0
template <class T>
__global__ __launch_bounds__(CS_TPB) void k_cs_add(const T* __restrict__ src, uint32_t M, uint32_t C, uint32_t q0, unsigned long long* __restrict__ hist)
{
    const uint32_t j = blockIdx.x * (uint32_t)CS_TPB + threadIdx.x;
    if (j >= M) return;
    unsigned long long word = 0ull;
    for (uint32_t r = 0; r < C; ++r) {
        const uint32_t q = q0 + r, b = q & 63u; // (q0 + C <= C T < 2^32: hgibbs_cs_begin)
        word |= (unsigned long long)(src[(size_t)r * M + j] != 0) << b;
        if (b == 63u || r + 1u == C) {
            const size_t o = (size_t)(q >> 6) * M + j;
            hist[o] |= word;
            word = 0ull;
        }
    }
}

// Thread per marker: the popcount of its first nw words
__global__ __launch_bounds__(CS_TPB) void k_cs_counts(const unsigned long long* __restrict__ hist, uint32_t M, uint32_t nw, uint32_t* __restrict__ cnt)
{
    const uint32_t j = blockIdx.x * (uint32_t)CS_TPB + threadIdx.x;
    if (j >= M) return;
    uint32_t c = 0;
    for (uint32_t w = 0; w < nw; ++w) c += (uint32_t)__popcll(hist[(size_t)w * M + j]);
    cnt[j] = c;
}

// the maximum of a 64-bit key over the workgroup; red: CS_TPB / 64 words of LDS.  Every thread gets it; ends with the words free again
__device__ __forceinline__ unsigned long long cs_block_max(unsigned long long key, unsigned long long* red)
{
    for (int o = 32; o; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = key;
    __syncthreads();
    unsigned long long best = red[0];
#pragma unroll
    for (int w = 1; w < CS_TPB / 64; ++w) best = red[w] > best ? red[w] : best;
    __syncthreads();
    return best;
}

// Workgroup per lead.  Dynamic LDS: 128 wpr words of friend counts.  members: nlead x max_size.
__global__ __launch_bounds__(CS_TPB) void k_cs_sets(const unsigned long long* __restrict__ hist, const uint32_t* __restrict__ cnt, uint32_t M, uint32_t nw,
                                                    uint32_t W, uint32_t wpr, const unsigned long long* __restrict__ fwd,
                                                    const unsigned long long* __restrict__ bwd, const uint32_t* __restrict__ leads, uint32_t need,
                                                    uint32_t max_size, uint32_t* __restrict__ status, uint32_t* __restrict__ size,
                                                    unsigned long long* __restrict__ sum_out, uint32_t* __restrict__ pep, uint32_t* __restrict__ members)
{
    extern __shared__ uint32_t cs_fc[]; // [2][64 wpr]: forward slots, then backward slots
    __shared__ unsigned long long cs_red[CS_TPB / 64];
    __shared__ uint32_t cs_mem[CS_MAX_SIZE];
    __shared__ uint32_t cs_pop[CS_TPB / 64];
    const uint32_t tid = threadIdx.x, lead = blockIdx.x;
    const uint32_t v = leads[lead]; // (< M: hgibbs_cs_sets)
    const uint32_t half = 64u * wpr;
    const unsigned long long* fr = fwd + (size_t)v * wpr;
    const unsigned long long* br = bwd + (size_t)v * wpr;
    for (uint32_t s = tid; s < 2u * half; s += (uint32_t)CS_TPB) {
        const bool back = s >= half;
        const uint32_t o = back ? s - half : s; // distance o + 1
        const unsigned long long word = (back ? br : fr)[o >> 6];
        uint32_t c = 0u;
        if (((word >> (o & 63u)) & 1ull) && o < W) {
            // the marker exists: v + o + 1 < M forwards, o + 1 <= v backwards
            const bool in = back ? o < v : o < M - 1u - v;
            if (in) c = cnt[back ? v - 1u - o : v + 1u + o];
        }
        cs_fc[s] = c;
    }
    if (tid == 0u) cs_mem[0] = v;
    __syncthreads();

    unsigned long long sum = cnt[v];
    uint32_t n = 1u, st = 0u; // (uniform)
    while (sum < (unsigned long long)need) {
        if (n == max_size) {
            st = 2u;
            break;
        }
        unsigned long long key = 0ull;
        for (uint32_t s = tid; s < 2u * half; s += (uint32_t)CS_TPB) {
            const uint32_t c = cs_fc[s];
            if (c) {
                const uint32_t idx = s >= half ? v - 1u - (s - half) : v + 1u + s;
                const unsigned long long k = ((unsigned long long)c << 32) | (uint32_t)~idx;
                key = k > key ? k : key;
            }
        }
        key = cs_block_max(key, cs_red);
        if (key == 0ull) {
            st = 1u;
            break;
        }
        const uint32_t idx = ~(uint32_t)key;
        if (tid == 0u) {
            cs_mem[n] = idx;
            cs_fc[idx > v ? idx - v - 1u : half + (v - 1u - idx)] = 0u;
        }
        sum += key >> 32;
        ++n;
        __syncthreads();
    }

    uint32_t* mem_out = members + (size_t)lead * max_size;
    if (st != 0u) {
        for (uint32_t m = tid; m < max_size; m += (uint32_t)CS_TPB) mem_out[m] = CS_NONE;
        if (tid == 0u) {
            status[lead] = st;
            size[lead] = 0u;
            sum_out[lead] = sum;
            pep[lead] = 0u;
        }
        return; // (uniform)
    }
    __syncthreads(); // cs_mem[0 .. n) is whole (a lead that needs no friend comes here without a pick's barrier after it)
    uint32_t pc = 0u;
    for (uint32_t w = tid; w < nw; w += (uint32_t)CS_TPB) {
        const unsigned long long* row = hist + (size_t)w * M;
        unsigned long long u = 0ull;
        for (uint32_t m = 0; m < n; ++m) u |= row[cs_mem[m]];
        pc += (uint32_t)__popcll(u);
    }
    for (int o = 32; o; o >>= 1) pc += __shfl_xor(pc, o);
    if ((tid & 63u) == 0u) cs_pop[tid >> 6] = pc;
    __syncthreads();
    for (uint32_t m = tid; m < max_size; m += (uint32_t)CS_TPB) mem_out[m] = m < n ? cs_mem[m] : CS_NONE;
    if (tid == 0u) {
        uint32_t p = 0u;
#pragma unroll
        for (int w = 0; w < CS_TPB / 64; ++w) p += cs_pop[w];
        status[lead] = 0u;
        size[lead] = n;
        sum_out[lead] = sum;
        pep[lead] = p;
    }
}

// the open history of a handle
CsState* cs_of(hgibbs_ctx* h, const char* who)
{
    if (!h) {
        fail("%s: null handle", who);
        return nullptr;
    }
    if (!h->cs) {
        fail("%s: no inclusion history on this handle (hgibbs_cs_begin first)", who);
        return nullptr;
    }
    if (!h->bed || h->cs->M != h->M) {
        fail("%s: the genotypes were replaced after hgibbs_cs_begin", who);
        return nullptr;
    }
    return h->cs.get();
}

// one record of every chain from src[r M + j] != 0 (device memory), as add number s->t
template <class T>
int cs_add(hgibbs_ctx* h, CsState* s, const T* src)
{
    const uint32_t M = s->M;
    double ms = 0.0;
    if (lap_begin(h)) return 1;
    k_cs_add<T><<<(M + (uint32_t)CS_TPB - 1u) / (uint32_t)CS_TPB, CS_TPB, 0, h->stream>>>(src, M, s->C, s->t * s->C, s->hist);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, ms)) return 1;
    s->add_ms += ms;
    s->t += 1u;
    return 0;
}

// the words per marker that the records added so far touch
uint32_t cs_words(const CsState* s) { return (uint32_t)(((uint64_t)s->t * s->C + 63u) / 64u); }

// cnt as of the records added so far (computed once per number of adds)
int cs_count(hgibbs_ctx* h, CsState* s)
{
    if (s->cnt_t == s->t) return 0;
    const uint32_t M = s->M;
    double ms = 0.0;
    if (lap_begin(h)) return 1;
    k_cs_counts<<<(M + (uint32_t)CS_TPB - 1u) / (uint32_t)CS_TPB, CS_TPB, 0, h->stream>>>(s->hist, M, cs_words(s), s->cnt);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, ms)) return 1;
    s->counts_ms = ms;
    s->cnt_t = s->t;
    return 0;
}

} // namespace

extern "C" int hgibbs_cs_begin(hgibbs_t h, uint32_t C, uint32_t T)
{
    const char* who = "hgibbs_cs_begin";
    if (op_guard(h, who, "the history is kept on one device")) return 1;
    if (C == 0u) return fail("%s: C = 0 chains, at least 1", who);
    if (T == 0u) return fail("%s: T = 0 records per chain, at least 1", who);
    if ((uint64_t)C * T >= (1ull << 32)) return fail("%s: C = %u chains of T = %u records: the number of records C T must stay below 2^32", who, C, T);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->cs.reset(); // an earlier state goes first: its memory counts as free for the new one
    const uint64_t nrec = (uint64_t)C * T;
    const size_t M = h->M, NW = (size_t)((nrec + 63u) / 64u);
    const size_t bytes = NW * M * sizeof(unsigned long long) + M * sizeof(uint32_t) + (size_t)C * M;
    if (need_device_memory(bytes, "%s: the history of M = %u markers over NREC = %llu records (%zu words per marker, the counts, a record's flags: %zu bytes, %.1f MiB)",
                           who, h->M, (unsigned long long)nrec, NW, bytes, bytes / 1048576.0))
        return 1;
    std::unique_ptr<CsState> s(new CsState());
    if (s->hist.alloc(NW * M) || s->cnt.alloc(M) || s->flags.alloc((size_t)C * M)) return 1;
    HIP_TRY(hipMemsetAsync(s->hist, 0, NW * M * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(s->cnt, 0, M * sizeof(uint32_t), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    s->M = h->M;
    s->C = C;
    s->T = T;
    s->NW = NW;
    h->cs = std::move(s);
    return 0;
}

extern "C" int hgibbs_cs_add_flags(hgibbs_t h, const uint8_t* flags)
{
    const char* who = "hgibbs_cs_add_flags";
    CsState* s = cs_of(h, who);
    if (!s) return 1;
    if (!flags) return fail("%s: null flags", who);
    if (s->t >= s->T) return fail("%s: the %u planned records are all added", who, s->T);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(s->flags, flags, (size_t)s->C * s->M, hipMemcpyHostToDevice, h->stream));
    return cs_add<uint8_t>(h, s, s->flags);
}

extern "C" int hgibbs_ss_cs_add(hgibbs_t h, uint32_t R)
{
    const char* who = "hgibbs_ss_cs_add";
    CsState* s = cs_of(h, who);
    if (!s) return 1;
    SsState* ss = R >= 1u ? ss_replicas_of(h, who, &R) : ss_of(h, who);
    if (!ss) return 1;
    const SsChains ch = R ? ss_replica_chains(ss) : ss_own_chain(h, ss);
    if (ch.C != s->C) return fail("%s: R = %u is %u chains, but hgibbs_cs_begin opened the history for C = %u", who, R, ch.C, s->C);
    if (s->t >= s->T) return fail("%s: the %u planned records are all added", who, s->T);
    HIP_TRY(hipSetDevice(h->device));
    return cs_add<int32_t>(h, s, ch.comp);
}

extern "C" int hgibbs_cs_counts(hgibbs_t h, uint32_t* cnt)
{
    const char* who = "hgibbs_cs_counts";
    CsState* s = cs_of(h, who);
    if (!s) return 1;
    s->counts_ms = 0.0;
    if (!cnt) return fail("%s: null output (cnt)", who);
    HIP_TRY(hipSetDevice(h->device));
    s->cnt_t = 0xFFFFFFFFu; // the figure is this call's kernel
    if (cs_count(h, s)) return 1;
    HIP_TRY(hipMemcpy(cnt, s->cnt, (size_t)s->M * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hgibbs_cs_history(hgibbs_t h, uint64_t* out)
{
    const char* who = "hgibbs_cs_history";
    CsState* s = cs_of(h, who);
    if (!s) return 1;
    if (!out) return fail("%s: null output", who);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, s->hist, s->NW * s->M * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hgibbs_cs_sets(hgibbs_t h, uint32_t W, const uint64_t* fwd, const uint64_t* bwd, uint32_t nlead, const uint32_t* leads, uint32_t need,
                              uint32_t max_size, uint32_t* status, uint32_t* size, uint64_t* sum, uint32_t* pep, uint32_t* members)
{
    const char* who = "hgibbs_cs_sets";
    CsState* s = cs_of(h, who);
    if (!s) return 1;
    s->sets_ms = 0.0;
    if (W == 0u || W > LD_WMAX) return fail("%s: W = %u, must be in [1, %u]", who, W, LD_WMAX);
    if (!fwd || !bwd) return fail("%s: null mask (%s)", who, !fwd ? "fwd" : "bwd");
    if (need == 0u) return fail("%s: need = 0, a set needs a count of at least 1", who);
    if (max_size == 0u || max_size > CS_MAX_SIZE) return fail("%s: max_size = %u, must be in [1, %u]", who, max_size, CS_MAX_SIZE);
    if (nlead && !leads) return fail("%s: null leads with nlead = %u", who, nlead);
    if (nlead && (!status || !size || !sum || !pep || !members)) return fail("%s: null output", who);
    const uint32_t M = s->M;
    {
        std::vector<bool> seen(M, false);
        for (uint32_t i = 0; i < nlead; ++i) {
            if (leads[i] >= M) return fail("%s: leads[%u] = %u is not below M = %u", who, i, leads[i], M);
            if (seen[leads[i]]) return fail("%s: leads[%u] = %u is among the leads twice", who, i, leads[i]);
            seen[leads[i]] = true;
        }
    }
    if (nlead == 0u) return 0;
    HIP_TRY(hipSetDevice(h->device));
    const uint32_t wpr = (W + 63u) / 64u;
    const size_t nm = (size_t)M * wpr;
    const size_t bytes = 2 * nm * 8 + (size_t)nlead * (4 * 4 + 8 + (size_t)max_size * 4);
    if (need_device_memory(bytes, "%s: the two %u x %u-word masks and the results of %u leads of up to %u members (%zu bytes, %.1f MiB)", who, M, wpr, nlead,
                           max_size, bytes, bytes / 1048576.0))
        return 1;
    DevBuf<unsigned long long> dfwd, dbwd, dsum;
    DevBuf<uint32_t> dleads, dst, dsz, dpep, dmem;
    if (dfwd.alloc(nm) || dbwd.alloc(nm) || dsum.alloc(nlead) || dleads.alloc(nlead) || dst.alloc(nlead) || dsz.alloc(nlead) || dpep.alloc(nlead) ||
        dmem.alloc((size_t)nlead * max_size))
        return 1;
    HIP_TRY(hipMemcpyAsync(dfwd, fwd, nm * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dbwd, bwd, nm * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dleads, leads, (size_t)nlead * 4, hipMemcpyHostToDevice, h->stream));
    if (cs_count(h, s)) return 1;
    double ms = 0.0;
    if (lap_begin(h)) return 1;
    k_cs_sets<<<nlead, CS_TPB, (size_t)128u * wpr * sizeof(uint32_t), h->stream>>>(s->hist, s->cnt, M, cs_words(s), W, wpr, dfwd, dbwd, dleads, need, max_size, dst,
                                                                                    dsz, dsum, dpep, dmem);
    HIP_TRY(hipGetLastError());
    if (lap_end(h, ms)) return 1;
    HIP_TRY(hipMemcpy(status, dst, (size_t)nlead * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(size, dsz, (size_t)nlead * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sum, dsum, (size_t)nlead * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pep, dpep, (size_t)nlead * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(members, dmem, (size_t)nlead * max_size * 4, hipMemcpyDeviceToHost));
    s->sets_ms = ms;
    return 0;
}

extern "C" int hgibbs_cs_end(hgibbs_t h)
{
    if (!h) return fail("hgibbs_cs_end: null handle");
    if (h->cs) {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->cs.reset();
    }
    return 0;
}

extern "C" int hgibbs_last_cs_ms(hgibbs_t h, double* add_ms, double* counts_ms, double* sets_ms)
{
    if (!h) return fail("hgibbs_last_cs_ms: null handle");
    const CsState* s = h->cs.get();
    if (add_ms) *add_ms = s ? s->add_ms : 0.0;
    if (counts_ms) *counts_ms = s ? s->counts_ms : 0.0;
    if (sets_ms) *sets_ms = s ? s->sets_ms : 0.0;
    return 0;
}
