// hg_csselect.cpp -- the walk over the candidate credible sets of hgibbs_cs_sets: plain C++, no HIP.
//
// The candidates are walked by descending count of their lead, ties by ascending lead index; one is accepted iff it reached its sum
// (status 0), its PEP count is at least min_pep, and none of its members belongs to a set accepted before it.  The accepted sets are
// therefore disjoint, and their order is the order taken.  Every step depends on the ones before it and is a handful of byte probes,
// so this stays on the host, like the greedy walk of hg_ldgreedy.cpp.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "../../include/hgibbs.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {

int sfail(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    hgibbs_set_error_(buf);
    return 1;
}

} // namespace

extern "C" int hgibbs_cs_select(uint32_t M, uint32_t nlead, const uint32_t* leads, const uint32_t* lead_cnt, const uint32_t* status, const uint32_t* size,
                                const uint32_t* pep, const uint32_t* members, uint32_t max_size, uint32_t min_pep, uint32_t* taken, uint32_t* ntaken)
{
    const char* who = "hgibbs_cs_select";
    if (!ntaken) return sfail("%s: null output (ntaken)", who);
    *ntaken = 0;
    if (max_size == 0u || max_size > 256u) return sfail("%s: max_size = %u, must be in [1, 256]", who, max_size);
    if (nlead && (!leads || !lead_cnt || !status || !size || !pep || !members)) return sfail("%s: null input with nlead = %u", who, nlead);
    if (nlead && !taken) return sfail("%s: null output (taken)", who);
    for (uint32_t i = 0; i < nlead; ++i) {
        if (size[i] > max_size) return sfail("%s: candidate %u has size %u, above max_size = %u", who, i, size[i], max_size);
        for (uint32_t m = 0; m < size[i]; ++m) {
            const uint32_t q = members[(size_t)i * max_size + m];
            if (q >= M) return sfail("%s: candidate %u: member %u is marker %u, not below M = %u", who, i, m, q, M);
        }
    }
    std::vector<uint32_t> walk(nlead);
    std::iota(walk.begin(), walk.end(), 0u);
    std::stable_sort(walk.begin(), walk.end(), [&](uint32_t a, uint32_t b) {
        if (lead_cnt[a] != lead_cnt[b]) return lead_cnt[a] > lead_cnt[b];
        return leads[a] < leads[b];
    });
    std::vector<uint8_t> owned(M, 0);
    uint32_t n = 0;
    for (const uint32_t i : walk) {
        if (status[i] != 0u || pep[i] < min_pep) continue;
        const uint32_t* mem = members + (size_t)i * max_size;
        bool free_ = true;
        for (uint32_t m = 0; m < size[i] && free_; ++m) free_ = !owned[mem[m]];
        if (!free_) continue;
        for (uint32_t m = 0; m < size[i]; ++m) owned[mem[m]] = 1;
        taken[n++] = i;
    }
    *ntaken = n;
    return 0;
}
