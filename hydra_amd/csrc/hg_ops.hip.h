// Host code shared by the operators that run on a handle's rows without sampling (hg_score, hg_ld, hg_mdots, hg_king, hg_roh, hg_pca, hg_grm.hip.h;
// DESIGN.md section 17): what every one of them needs around its kernels, once.
#pragma once

namespace {

// The checks every operator makes first.  one_rank: why the operator takes a handle of one rank only (null: any number of ranks)
int op_guard(const hgibbs_ctx* h, const char* who, const char* one_rank)
{
    if (!h) return fail("%s: null handle", who);
    if (!h->bed) return fail("%s: no genotypes loaded on this handle", who);
    if (one_rank && (h->nranks > 1 || h->comm)) return fail("%s: one rank only (this handle has %d): %s", who, h->nranks, one_rank);
    return 0;
}

// Refuses a call whose `bytes` of device memory do not fit beside 64 MiB of slack; the message is the caller's (printf-style: its
// name and what needs the memory), then the free memory
int need_device_memory(size_t bytes, const char* fmt, ...)
{
    size_t fre = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fre, &tot));
    if (bytes + (64ull << 20) <= fre) return 0;
    char why[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(why, sizeof why, fmt, ap);
    va_end(ap);
    return fail("%s, %.1f MiB of device memory are free", why, fre / 1048576.0);
}

// flags[t] = 1 when a column of the markers [t granule, (t + 1) granule) has a missing call, from h->counts as they stand (the
// caller has them computed); synchronises the stream
int missing_tiles(hgibbs_ctx* h, uint32_t granule, std::vector<uint8_t>& flags)
{
    std::vector<unsigned long long> c((size_t)h->M * 3);
    HIP_TRY(hipMemcpyAsync(c.data(), h->counts, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    flags.assign((h->M + granule - 1u) / granule, 0);
    for (uint32_t j = 0; j < h->M; ++j)
        if (c[3ull * j + 2]) flags[j / granule] = 1;
    return 0;
}

// n >= 1 units in about `want` ranges of one length, none above `cap` units (NO_CAP: any length): the length goes to `per`, and the
// number of ranges, counted again from it so that none is empty, comes back
constexpr uint32_t NO_CAP = 0xFFFFFFFFu;
uint32_t split_ranges(uint32_t n, uint32_t want, uint32_t cap, uint32_t& per)
{
    uint32_t g = std::max(want, (uint32_t)(((uint64_t)n + cap - 1u) / cap));
    g = std::max(1u, std::min(g, n));
    per = (n + g - 1u) / g;
    return (n + per - 1u) / per;
}

// Device time on the handle's pair of events: lap_begin, the stream-ordered work, then lap_end, which waits for the work and adds
// its milliseconds to `total`.  A caller with a synchronisation of its own after the work takes lap_mark, that synchronisation,
// lap_read instead.
int lap_begin(hgibbs_ctx* h)
{
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    return 0;
}

int lap_mark(hgibbs_ctx* h)
{
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    return 0;
}

int lap_read(hgibbs_ctx* h, double& total)
{
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    total += ms;
    return 0;
}

int lap_end(hgibbs_ctx* h, double& total)
{
    if (lap_mark(h)) return 1;
    HIP_TRY(hipEventSynchronize(h->ev1));
    return lap_read(h, total);
}

// (hi 2^32 + lo) 2^-E as ONE rounding: carry the low word's high bits into hi (exact), then hi 2^32 is exact in f64
__device__ __forceinline__ double round_halves(long long hi, long long lo, int E)
{
    hi += lo >> 32;
    lo &= 0xFFFFFFFFll;
    return ldexp(ldexp((double)hi, 32) + (double)lo, -E);
}

} // namespace
